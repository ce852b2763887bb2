"""The trailing updates in tree order (SMLU_TRAIL_SPAN / SMLU_TRAIL_NS) against the same library at
span 1, bit for bit.

With the knob on, a qualifying front's block (r, c) is loaded, updated and stored O(log) times with
k-ranges of 1, 2, 4, ... outer blocks instead of min(r, c) times with k = OB; each tile still runs
one FMA per k in ascending k from accumulators loaded from C, so factors, pivots, scaling and
solutions must be bitwise those of span 1 -- after the eager first factorization, after the
refactor that captures the graph, and after replays with new diagonal values.  A k-range applied
twice, skipped, or applied before its L columns and U rows are final shows as differing bits.
SMLU_TRAIL_NS is forced to its lower bound for tests so that oracle-sized fronts qualify:
poisson3d_24 at OB = 128 (root 576: four full blocks and a partial one, fronts below it with L21
and U12), poisson3d_32 at OB = 128 (eight blocks and more: boundaries of lowbit 1, 2 and 4) and at
the default OB (three blocks: the lowbit-2 boundary clamped at the last block)."""
import hashlib
import os

import numpy as np
import pytest

import smlu
from smlu import matrices as mats

from test_gpu_lside import _golden, diag_values, knobs, same, state

pytestmark = pytest.mark.gpu

SPAN, MINNS, LSIDE = "SMLU_TRAIL_SPAN", "SMLU_TRAIL_NS", "SMLU_LSIDE_MIN"
NS_TEST = "64"   # the lower bound SMLU_TRAIL_NS accepts for tests (include/smlu.h)


def run_pair(A, values, span, extra=None, expect=True, **kw):
    """One handle at span 1 and one at `span` with the threshold forced down: compared after create,
    after the first refactor (graph capture) and after the further ones (replay)."""
    env_one = dict(extra or {}, **{SPAN: "1"})
    env_on = dict(extra or {}, **{SPAN: span, MINNS: NS_TEST})
    b = np.random.default_rng(7).random(A.shape[0]).astype(A.dtype)
    with knobs(env_one):
        Fo = smlu.ParallelSparseLU(A, **kw)
    with knobs(env_on):
        Ft = smlu.ParallelSparseLU(A, **kw)
    try:
        assert Fo.stat("trail_fronts") == 0 and Fo.stat("trail_span") == 1
        ob = float((extra or {}).get("SMLU_OB", 384))
        assert Fo.stat("gemmo_kmax") in (0.0, ob)
        if expect:
            assert Ft.stat("trail_span") == float(span) and Ft.stat("trail_fronts") > 0
            # a longer k-range was scheduled.  (gemm_bytes falls once blocks save more C round trips
            # than the strips add operand reads -- test_trail_schedule.py; not with three blocks.)
            assert Ft.stat("gemmo_kmax") >= 2 * ob
            assert Ft.stat("gemm_bytes") != Fo.stat("gemm_bytes")
        else:
            assert Ft.stat("trail_fronts") == 0 and Ft.stat("gemmo_kmax") == Fo.stat("gemmo_kmax")
            assert Ft.stat("gemm_bytes") == Fo.stat("gemm_bytes")
        assert Ft.stat("launches") == Fo.stat("launches")
        for k in ("gemm_flops", "gemm22_flops"):
            assert abs(Ft.stat(k) - Fo.stat(k)) <= 1e-12 * Fo.stat(k), k
        same(state(Ft, b), state(Fo, b), "create")
        for i, v in enumerate(values):
            with knobs(env_one):
                Fo.refactor(v)
            with knobs(env_on):
                Ft.refactor(v)
            same(state(Ft, b), state(Fo, b), f"refactor {i}")
        if expect:   # no rebuild dropped the order on the way
            assert Ft.stat("trail_fronts") > 0
        return Ft, Fo
    except BaseException:
        Ft.close()
        Fo.close()
        raise


@pytest.mark.parametrize("N,span,extra", [
    (24, "0", {"SMLU_OB": "128"}), (24, "2", {"SMLU_OB": "128"}),
    (32, "0", {"SMLU_OB": "128"}), (32, "4", {"SMLU_OB": "128"}),
    (32, "0", None),
    (32, "4", {"SMLU_OB": "128", LSIDE: "64"}),
], ids=["24-OB128-span0", "24-OB128-span2", "32-OB128-span0", "32-OB128-span4", "32-span0", "32-OB128-span4-lside"])
def test_bitwise_against_span_one(gpu, N, span, extra):
    A = mats.poisson3d(N)
    Ft, Fo = run_pair(A, diag_values(A), span, extra)
    if extra and LSIDE in extra:   # the side stream and the tree order ran together
        assert Ft.stat("side_launches") > 0 and Fo.stat("side_launches") > 0
    Ft.close()
    Fo.close()


def test_profile_mode_same_bits_and_finite_times(gpu):
    A = mats.poisson3d(24)
    Ft, Fo = run_pair(A, diag_values(A), "0", {"SMLU_OB": "128"}, profile=True)
    for F in (Ft, Fo):
        t = F.stat("ms_gemmo")
        assert np.isfinite(t) and t > 0.0, t
    Ft.close()
    Fo.close()


def test_ten_refactors_one_factor_hash(gpu):
    A = mats.poisson3d(32)
    v = mats.perturb_diag(A, 3).data
    with knobs({SPAN: "0", MINNS: NS_TEST, "SMLU_OB": "128"}):
        F = smlu.ParallelSparseLU(A)
        try:
            assert F.stat("trail_fronts") > 0
            hashes = set()
            for _ in range(10):
                F.refactor(v)
                h = hashlib.sha1()
                for arr in (F.L.data, F.U.data, np.asarray(F.p)):
                    h.update(np.ascontiguousarray(arr).tobytes())
                hashes.add(h.hexdigest())
            assert len(hashes) == 1, hashes
        finally:
            F.close()


def test_complex_handle_is_untouched(gpu):
    A = mats.poisson3d(16).astype(np.complex128)
    A.data = A.data * (1.0 + 0.25j)
    vals = [mats.perturb_diag(mats.poisson3d(16), s).data * (1.0 + 0.25j) for s in (5, 6, 7)]
    Ft, Fo = run_pair(A, vals, "0", {"SMLU_OB": "128"}, expect=False)
    assert Ft.stat("complex") == 1.0
    Ft.close()
    Fo.close()


def test_nondominant_golden_is_untouched(gpu):
    A = _golden("fe_8.npz")
    rng = np.random.default_rng(3)
    vals = [A.data * (1.0 + 0.01 * rng.standard_normal(A.nnz)) for _ in range(3)]
    Ft, Fo = run_pair(A, vals, "0", {"SMLU_OB": "128"}, expect=False)
    assert Ft.stat("dominant") == 0.0
    Ft.close()
    Fo.close()


def test_nondominant_blocked_fronts_are_untouched(gpu):
    # the C1 fixture's pattern with values far from dominant: blocked fronts on the full-candidate
    # (mode 1) path, which the knob must leave alone
    A = _golden(os.path.join("c1", "c1_random_1000.npz"))
    rng = np.random.default_rng(9)
    A.data = rng.standard_normal(A.nnz)
    vals = [rng.standard_normal(A.nnz) for _ in range(3)]
    Ft, Fo = run_pair(A, vals, "0", {"SMLU_OB": "128"}, expect=False)
    assert Ft.stat("dominant") == 0.0 and Ft.stat("fronts_mode1") > 0
    Ft.close()
    Fo.close()
