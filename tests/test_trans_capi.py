"""CPU tests of the transposed / adjoint solve surface (smlu_solve_trans*, include/smlu.h): the
entry points exist and validate their arguments, the SMLU_OP_* constants of the Python mirror are
the header's, and the mirror refuses an unknown `trans`."""
import os
import re

import numpy as np
import pytest

import smlu
from smlu import _lib as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANS = ("smlu_solve_trans", "smlu_solve_trans_device", "smlu_solve_trans_multi", "smlu_solve_trans_multi_device")


def test_null_handle_is_an_argument_error():
    L = smlu.lib()
    for op in (C.SMLU_OP_N, C.SMLU_OP_T, C.SMLU_OP_H, 7):
        assert L.smlu_solve_trans(None, op, None, None) == C.SMLU_ERR_ARG
        assert L.smlu_solve_trans_device(None, op, None, None) == C.SMLU_ERR_ARG
        assert L.smlu_solve_trans_multi(None, op, 1, None, 1, None, 1) == C.SMLU_ERR_ARG
        assert L.smlu_solve_trans_multi_device(None, op, 1, None, 1, None, 1) == C.SMLU_ERR_ARG
    assert C.last_error(None)


def test_signatures_declared():
    for name in TRANS:
        assert name in C.SIGNATURES
    # op is the second argument of all four
    assert all(C.SIGNATURES[name][1][1] is C.i32 for name in TRANS)


def test_op_constants_match_header():
    src = open(os.path.join(ROOT, "include", "smlu.h")).read()
    ops = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(SMLU_OP_[A-Z])\s+(-?\d+)", src)}
    assert sorted(ops) == ["SMLU_OP_H", "SMLU_OP_N", "SMLU_OP_T"]
    for name, val in ops.items():
        assert getattr(C, name) == val, name
    assert len(set(ops.values())) == 3


@pytest.mark.parametrize("trans", ["X", "n", "H", None, 1])
def test_unknown_trans_raises(trans):
    x = np.zeros(3)
    with pytest.raises(ValueError, match="trans"):
        smlu.ldiv_(x, None, x, trans=trans)   # refused before the factorization is looked at
