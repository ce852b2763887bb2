"""CPU tests of the batched-refinement boundary (smlu_solve_refined_multi*): the header declares the
two functions and smlu_refine_info, the ctypes layer binds them with the header's layout, and a NULL
handle is refused before anything touches a device."""
import ctypes
import os
import re

import smlu
from smlu import _lib as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("smlu_solve_refined_multi", "smlu_solve_refined_multi_device")


def header():
    return open(os.path.join(ROOT, "include", "smlu.h")).read()


def test_header_declares_the_functions_and_the_struct():
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NAMES:
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 9, args
        assert args[0].startswith("smlu_handle*") and args[1] == "int op" and args[2] == "int max_steps"
        assert args[3] == "int64_t nrhs" and args[-1].startswith("smlu_refine_info*")
    m = re.search(r"typedef\s+struct\s+smlu_refine_info\s*\{([^}]*)\}\s*smlu_refine_info\s*;", src)
    assert m
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t steps", "int32_t stop", "double berr", "double resid"], fields


def test_ctypes_signatures_and_struct_layout():
    for name in NAMES:
        res, args = C.SIGNATURES[name]
        assert res is C.i32
        assert args == [C.vp, C.i32, C.i32, C.i64, C.vp, C.i64, C.vp, C.i64, ctypes.POINTER(C.SmluRefineInfo)]
    assert ctypes.sizeof(C.SmluRefineInfo) == 24
    assert [(f, t) for f, t in C.SmluRefineInfo._fields_] == [
        ("steps", C.i32), ("stop", C.i32), ("berr", C.f64), ("resid", C.f64)]
    assert C.SmluRefineInfo.berr.offset == 8 and C.SmluRefineInfo.resid.offset == 16


def test_library_exports_the_symbols():
    L = smlu.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_null_handle_is_an_argument_error():
    L = smlu.lib()
    info = (C.SmluRefineInfo * 1)()
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in NAMES:
        fn = getattr(L, name)
        assert fn(None, C.SMLU_OP_N, -1, 1, p, 4, p, 4, info) == C.SMLU_ERR_ARG
        assert fn(None, C.SMLU_OP_T, 0, 0, None, 0, None, 0, None) == C.SMLU_ERR_ARG
        assert C.last_error(None)


def test_python_surface():
    assert callable(smlu.ldiv_refined_) and "ldiv_refined_" in smlu.__all__
    assert callable(smlu.ParallelSparseLU.solve_refined_multi_device)
