"""One column through every solve entry point that can take one: the same bits, the same refine_*
stats and the same pass count whichever door it came in by.

The thirteen smlu_solve* functions share one driver (csrc/solve.cpp).  The suites of each family
compare a batch with its own single solves; this file compares the families with each other, at the
one width every door accepts.  Two handles: the golden poisson2d_16 (n = 256, diagonally dominant,
so the default rule never refines) and nondominant_fe_300 (refines under the default rule).  The C
functions are called directly, host forms on numpy arrays and device forms on torch tensors, so the
door under test is the one named.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import smlu
from smlu import _lib as C

from test_gpu_solve_trans import load_golden
from test_gpu_solve_trans_batched import nondominant_fe

pytestmark = pytest.mark.gpu

MATRICES = {"poisson2d_16": lambda: load_golden("poisson2d_16"), "nondominant_fe_300": nondominant_fe}
OPS = {"N": C.SMLU_OP_N, "T": C.SMLU_OP_T}
SENTINEL = -12345.5


# door name -> (C function, device form?, call(fn, h, op, nrhs, pb, px, n)); nrhs only reaches the
# forms that take one
def _single(fn, h, op, nrhs, pb, px, n):
    return fn(h, pb, px)


def _multi(fn, h, op, nrhs, pb, px, n):
    return fn(h, nrhs, pb, n, px, n)


def _trans(fn, h, op, nrhs, pb, px, n):
    return fn(h, op, pb, px)


def _trans_multi(fn, h, op, nrhs, pb, px, n):
    return fn(h, op, nrhs, pb, n, px, n)


def _refined(fn, h, op, nrhs, pb, px, n):
    return fn(h, op, -1, nrhs, pb, n, px, n, None)


FORWARD = {
    "solve": ("smlu_solve", False, _single),
    "solve_device": ("smlu_solve_device", True, _single),
    "solve_multi": ("smlu_solve_multi", False, _multi),
    "solve_multi_device": ("smlu_solve_multi_device", True, _multi),
}
ANY_OP = {
    "solve_trans": ("smlu_solve_trans", False, _trans),
    "solve_trans_device": ("smlu_solve_trans_device", True, _trans),
    "solve_trans_multi": ("smlu_solve_trans_multi", False, _trans_multi),
    "solve_trans_multi_device": ("smlu_solve_trans_multi_device", True, _trans_multi),
    "solve_refined_multi": ("smlu_solve_refined_multi", False, _refined),
    "solve_refined_multi_device": ("smlu_solve_refined_multi_device", True, _refined),
}
TAKES_NRHS = ["solve_multi", "solve_multi_device", "solve_trans_multi", "solve_trans_multi_device",
              "solve_refined_multi", "solve_refined_multi_device"]


def doors(trans):
    return {**FORWARD, **ANY_OP} if trans == "N" else dict(ANY_OP)


@pytest.fixture(scope="module")
def handles(gpu):
    out = {}
    for name, make in MATRICES.items():
        out[name] = smlu.ParallelSparseLU(sp.csc_matrix(make()))
    yield out
    for F in out.values():
        F.close()


def call(F, door, trans, b, nrhs=1, alias=False):
    """One call of the door on the host vector b (x = SENTINEL before, or b itself when alias).
    Returns (rc, x on the host)."""
    import torch
    name, device, shape = {**FORWARD, **ANY_OP}[door]
    fn = getattr(C.lib(), name)
    n = F.n
    if device:
        tb = torch.from_numpy(b.copy()).to("cuda:0")
        tx = tb if alias else torch.full_like(tb, SENTINEL)
        torch.cuda.synchronize()
        with C.caller_stream(F._h, tb):
            rc = shape(fn, F._h, OPS[trans], nrhs, ctypes.c_void_p(tb.data_ptr()), ctypes.c_void_p(tx.data_ptr()), n)
        torch.cuda.synchronize()
        return rc, tx.cpu().numpy()
    hb = b.copy()
    hx = hb if alias else np.full_like(hb, SENTINEL)
    rc = shape(fn, F._h, OPS[trans], nrhs, C.ptr(hb), C.ptr(hx), n)
    return rc, hx


def counters(F, trans):
    own, other = ("solve_passes", "solve_trans_passes") if trans == "N" else ("solve_trans_passes", "solve_passes")
    return F.stat(own), F.stat(other)


def refine_stats(F):
    return int(F.stat("refine_steps")), F.stat("refine_berr"), F.stat("refine_residual")


@pytest.mark.parametrize("trans", ["N", "T"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_one_column_through_every_door(handles, name, trans):
    F = handles[name]
    b = np.random.default_rng(410).random(F.n)
    seen = {}
    for door in doors(trans):
        for alias in (False, True):
            own0, other0 = counters(F, trans)
            rc, x = call(F, door, trans, b, alias=alias)
            own1, other1 = counters(F, trans)
            assert rc == C.SMLU_OK, (door, alias, C.last_error(F._h))
            assert np.isfinite(x).all() and not (x == SENTINEL).any(), (door, alias)
            seen[(door, alias)] = (x, refine_stats(F), own1 - own0)
            assert other1 == other0, (door, alias)
    first = next(iter(seen))
    x0, stats0, passes0 = seen[first]
    print(f"{name} {trans}: refine stats {stats0}, {passes0} passes per solve, {len(seen)} solves")
    if name == "poisson2d_16":
        assert F.stat("dominant") == 1 and stats0 == (0, -1.0, -1.0) and passes0 == 1
    else:
        assert F.stat("dominant") == 0 and stats0[0] >= 1 and passes0 == 1 + stats0[0]
    for key, (x, stats, passes) in seen.items():
        assert np.array_equal(x, x0), (key, first, np.abs(x - x0).max())
        assert stats == stats0, (key, stats, stats0)
        assert passes == passes0, (key, passes, passes0)


@pytest.mark.parametrize("name", list(MATRICES))
def test_no_columns_touches_nothing(handles, name):
    F = handles[name]
    b = np.random.default_rng(411).random(F.n)
    for trans in ("N", "T"):
        for door in TAKES_NRHS:
            if door not in doors(trans):
                continue
            before = counters(F, trans)
            rc, x = call(F, door, trans, b, nrhs=0)
            assert rc == C.SMLU_OK, (door, trans, C.last_error(F._h))
            assert (x == SENTINEL).all(), (door, trans)
            assert counters(F, trans) == before, (door, trans)
