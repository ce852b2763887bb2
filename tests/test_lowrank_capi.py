"""CPU checks of the low-rank update boundary (smlu_lowrank_*, smlu_solve_lowrank*, include/smlu.h): the
symbols, their ctypes signatures, the struct layout, the rank limit, and the argument errors that need
no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import smlu
from smlu import _lib as C
from smlu import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("smlu_lowrank_set", "smlu_lowrank_set_device", "smlu_lowrank_clear", "smlu_solve_lowrank",
         "smlu_solve_lowrank_device")


def test_entry_points_are_exported_with_signatures():
    L = smlu.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in C.SIGNATURES
        assert C.SIGNATURES[name][0] is C.i32
    info = ctypes.POINTER(C.SmluLowrankInfo)
    for name in NAMES[:2]:
        assert C.SIGNATURES[name][1] == [C.vp, C.i32, C.vp, C.i64, C.vp, C.i64, info]
    assert C.SIGNATURES["smlu_lowrank_clear"][1] == [C.vp]
    for name in NAMES[3:]:
        assert C.SIGNATURES[name][1] == [C.vp, C.i32, C.i32, C.vp, C.vp, info]


def test_struct_layout_and_rank_limit_match_the_header():
    raw = open(os.path.join(ROOT, "include", "smlu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ctype = {"double": C.f64, "int32_t": C.i32}
    body = re.search(r"typedef struct smlu_lowrank_info \{(.*?)\} smlu_lowrank_info;", src, flags=re.S).group(1)
    fields = []
    for t, names in re.findall(r"(\w+)\s+([\w,\s]+?);", body):
        fields += [(nm.strip(), ctype[t]) for nm in names.split(",")]
    assert fields == list(C.SmluLowrankInfo._fields_), fields
    assert ctypes.sizeof(C.SmluLowrankInfo) == 4 * 4 + 5 * 8
    m = re.search(r"#define\s+SMLU_LOWRANK_MAX\s+(\d+)", raw)
    assert m and int(m.group(1)) == C.SMLU_LOWRANK_MAX == 32


def test_stat_keys_are_documented():
    raw = open(os.path.join(ROOT, "include", "smlu.h")).read()
    for key in ("lowrank_k", "lowrank_solves", "lowrank_set_ms_last", "lowrank_ms_last"):
        assert f'"{key}"' in raw, key


def test_null_handle_is_an_argument_error():
    L = smlu.lib()
    W = np.ones((3, 2), order="F")
    b, x = np.ones(3), np.empty(3)
    info = C.SmluLowrankInfo()
    for fn in (L.smlu_lowrank_set, L.smlu_lowrank_set_device):
        assert fn(None, 2, C.ptr(W), 3, C.ptr(W), 3, ctypes.byref(info)) == C.SMLU_ERR_ARG
        assert fn(None, 0, None, 0, None, 0, None) == C.SMLU_ERR_ARG
    assert L.smlu_lowrank_clear(None) == C.SMLU_ERR_ARG
    for fn in (L.smlu_solve_lowrank, L.smlu_solve_lowrank_device):
        assert fn(None, C.SMLU_OP_N, -1, C.ptr(b), C.ptr(x), ctypes.byref(info)) == C.SMLU_ERR_ARG
        assert fn(None, C.SMLU_OP_N, 0, None, None, None) == C.SMLU_ERR_ARG
    assert "NULL" in C.last_error(None)


class _Shell(smlu.ParallelSparseLU):
    """The Python checks run before any handle is looked at: a factorization that was never created."""

    def __init__(self, n, is_complex=False):
        self.n = self.m = n
        self.is_complex = is_complex
        self._h = None


def test_python_argument_checks():
    F = _Shell(5)
    b = np.ones(5)
    for steps in (-2, 1.5, True, None):
        with pytest.raises(ValueError):
            F.solve_lowrank(b, steps=steps)
    with pytest.raises(ValueError):
        F.solve_lowrank(b, trans="X")
    with pytest.raises(smlu.DimensionMismatch):
        F.solve_lowrank(np.ones(4))
    with pytest.raises(smlu.DimensionMismatch):
        F.solve_lowrank(b, x=np.empty(6))
    with pytest.raises(smlu.DimensionMismatch):
        F.lowrank_set(np.ones((5, 2)), np.ones((5, 3)))
    with pytest.raises(smlu.DimensionMismatch):
        F.lowrank_set(np.ones((4, 2)), np.ones((4, 2)))
    with pytest.raises(ValueError):
        F.lowrank_set(np.ones((5, 33)), np.ones((5, 33)))
    A = np.eye(5)
    with pytest.raises(ValueError):
        F.update_columns([1, 1], A, A)
    with pytest.raises(ValueError):
        F.update_columns([5], A, A)
    with pytest.raises(ValueError):
        F.update_columns([1], 2.0 * A, A)               # differs outside column 1
    with pytest.raises(smlu.DimensionMismatch):
        F.update_columns([1], np.eye(4), A)
    assert api._lowrank_steps(-1) == -1 and api._lowrank_steps(np.int64(4)) == 4


def test_complex_handle_is_a_state_error_in_python():
    F = _Shell(5, is_complex=True)
    for call in (lambda: F.lowrank_set(np.ones((5, 1)), np.ones((5, 1))), lambda: F.solve_lowrank(np.ones(5)),
                 lambda: F.lowrank_set_device(None, None), lambda: F.solve_lowrank_device(0, 0)):
        with pytest.raises(smlu.SmluError) as e:
            call()
        assert e.value.code == C.SMLU_ERR_STATE and "ComplexF64" in str(e.value)
