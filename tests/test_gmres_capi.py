"""CPU checks of the GMRES boundary (smlu_solve_gmres*, include/smlu.h): the symbols, their ctypes
signatures, the defaults, the status code, and the argument errors that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import smlu
from smlu import _lib as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("smlu_gmres_default_opts", "smlu_solve_gmres", "smlu_solve_gmres_device")


def test_entry_points_are_exported_with_signatures():
    L = smlu.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in C.SIGNATURES
    for name in NAMES[1:]:
        res, args = C.SIGNATURES[name]
        assert res is C.i32 and len(args) == 7
        assert args[5] == ctypes.POINTER(C.SmluGmresOpts) and args[6] == ctypes.POINTER(C.SmluGmresInfo)


def test_struct_layouts_match_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smlu.h")).read(), flags=re.S)
    ctype = {"double": C.f64, "int32_t": C.i32}
    for cname, S in (("smlu_gmres_opts", C.SmluGmresOpts), ("smlu_gmres_info", C.SmluGmresInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        fields = []
        for t, names in re.findall(r"(\w+)\s+([\w,\s]+?);", body):
            fields += [(nm.strip(), ctype[t]) for nm in names.split(",")]
        assert fields == list(S._fields_), (cname, fields)
    assert ctypes.sizeof(C.SmluGmresOpts) == 16 and ctypes.sizeof(C.SmluGmresInfo) == 48


def test_defaults():
    o = C.SmluGmresOpts()
    smlu.lib().smlu_gmres_default_opts(ctypes.byref(o))
    assert (o.rtol, o.restart, o.maxit) == (1e-10, 30, 200)
    smlu.lib().smlu_gmres_default_opts(None)   # NULL is ignored


def test_not_converged_code_matches_the_header():
    src = open(os.path.join(ROOT, "include", "smlu.h")).read()
    m = re.search(r"#define\s+SMLU_NOT_CONVERGED\s+(\d+)", src)
    assert m and int(m.group(1)) == C.SMLU_NOT_CONVERGED == 3
    assert C.SMLU_NOT_CONVERGED > 0      # a numerical status, not an error


def test_null_handle_is_an_argument_error():
    L = smlu.lib()
    b = np.ones(3)
    x = np.empty(3)
    info = C.SmluGmresInfo()
    for fn in (L.smlu_solve_gmres, L.smlu_solve_gmres_device):
        assert fn(None, C.SMLU_OP_N, None, C.ptr(b), C.ptr(x), None, ctypes.byref(info)) == C.SMLU_ERR_ARG
        assert fn(None, C.SMLU_OP_N, None, None, None, None, None) == C.SMLU_ERR_ARG
    assert C.last_error(None)


@pytest.mark.parametrize("kw", [dict(trans="X"), dict(trans=None), dict(restart=0), dict(restart=33),
                                dict(restart=2.5), dict(maxiter=0), dict(maxiter=-3), dict(rtol=-1e-3),
                                dict(rtol=float("nan")), dict(rtol=float("inf")), dict(rtol="tight")])
def test_bad_options_raise_before_the_handle_is_looked_at(kw):
    b = np.ones(3)
    with pytest.raises(ValueError):
        smlu.ParallelSparseLU.gmres(None, b, **kw)          # no handle at all: the options come first
    with pytest.raises(ValueError):
        smlu.ParallelSparseLU.gmres_device(None, 0, 0, **kw)
