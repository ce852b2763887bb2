"""CPU tests of the determinant / condition-estimate surface (smlu_logabsdet, smlu_logabsdet_z,
smlu_rcond, include/smlu.h): the entry points exist and validate their arguments, the SMLU_NORM_*
constants of the Python mirror are the header's, and the mirror refuses an unknown `norm`."""
import ctypes
import os
import re

import pytest

import smlu
from smlu import _lib as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = ("smlu_logabsdet", "smlu_logabsdet_z", "smlu_rcond")


def test_null_handle_is_an_argument_error():
    L = smlu.lib()
    a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    ph = (ctypes.c_double * 2)()
    assert L.smlu_logabsdet(None, ctypes.byref(a), ctypes.byref(b)) == C.SMLU_ERR_ARG
    assert L.smlu_logabsdet(None, None, None) == C.SMLU_ERR_ARG
    assert L.smlu_logabsdet_z(None, ctypes.byref(a), ph) == C.SMLU_ERR_ARG
    for norm in (C.SMLU_NORM_ONE, C.SMLU_NORM_INF, 0, 7):
        assert L.smlu_rcond(None, norm, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == C.SMLU_ERR_ARG
        assert L.smlu_rcond(None, norm, None, None, None) == C.SMLU_ERR_ARG
    assert C.last_error(None)


def test_signatures_declared():
    for name in DIAG:
        assert name in C.SIGNATURES
        assert C.SIGNATURES[name][0] is C.i32
    assert len(C.SIGNATURES["smlu_logabsdet"][1]) == 3
    assert len(C.SIGNATURES["smlu_logabsdet_z"][1]) == 3
    assert len(C.SIGNATURES["smlu_rcond"][1]) == 5
    assert C.SIGNATURES["smlu_rcond"][1][1] is C.i32   # norm is the second argument


def test_norm_constants_match_header():
    src = open(os.path.join(ROOT, "include", "smlu.h")).read()
    norms = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(SMLU_NORM_[A-Z]+)\s+(-?\d+)", src)}
    assert sorted(norms) == ["SMLU_NORM_INF", "SMLU_NORM_ONE"]
    for name, val in norms.items():
        assert getattr(C, name) == val, name
    assert len(set(norms.values())) == 2


@pytest.mark.parametrize("norm", ["2", "fro", "I", None, 2, 1])
def test_unknown_norm_raises(norm):
    with pytest.raises(ValueError, match="norm"):
        smlu.ParallelSparseLU.rcond(None, norm=norm)   # refused before the factorization is looked at
    with pytest.raises(ValueError, match="norm"):
        smlu.ParallelSparseLU.condest(None, norm=norm)
