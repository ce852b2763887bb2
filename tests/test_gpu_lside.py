"""The L rows below an outer block on the side stream (SMLU_LSIDE_MIN) against the same library
with the knob off, bit for bit.

With the knob on, a diagonal-tile front's step solves and updates the rows [oend, M) of the block's
columns in two launches of their own on the handle's side stream, joined before the block's
trailing update; every element still sees the same k = 64 updates in the same order, so factors,
pivots, scaling and solutions must be bitwise those of the knob at 0 -- after the eager first
factorization, after the refactor that captures the graph, and after replays with new values.  A
missing dependency between the two streams shows as differing bits or as a factor hash that changes
between refactors of the same values.  The threshold is forced to 64 so that oracle-sized fronts
qualify."""
import contextlib
import hashlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

import smlu
from smlu import matrices as mats

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOB = "SMLU_LSIDE_MIN"


@contextlib.contextmanager
def knobs(env):
    """The knobs are read at every schedule build (a refactor may rebuild): set around each call."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def state(F, b):
    x = np.empty_like(b)
    smlu.ldiv_(x, F, b)
    L, U = F.L, F.U
    return dict(Li=L.indices.copy(), Lx=L.data.copy(), Ui=U.indices.copy(), Ux=U.data.copy(), p=np.array(F.p),
                q=np.array(F.q), Rs=np.array(F.Rs), x=x,
                stats=[F.stat(k) for k in ("mode_refactors", "repivots", "weak", "growth_max", "dominant")])


def same(a, b, what):
    for k in ("Li", "Lx", "Ui", "Ux", "p", "q", "Rs", "x"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])


def run_pair(A, values, extra=None, expect_side=True, **kw):
    """One handle with the knob at 0 and one at 64: compared after create, after the first refactor
    (graph capture) and after two further refactors (replay).  values: three value arrays."""
    env_off, env_on = dict(extra or {}, **{KNOB: "0"}), dict(extra or {}, **{KNOB: "64"})
    b = np.random.default_rng(7).random(A.shape[0]).astype(A.dtype)
    with knobs(env_off):
        Fo = smlu.ParallelSparseLU(A, **kw)
    with knobs(env_on):
        Fs = smlu.ParallelSparseLU(A, **kw)
    try:
        assert Fo.stat("side_launches") == 0 and Fo.stat("side_rows") == 0
        if expect_side:
            assert Fs.stat("side_launches") > 0 and Fs.stat("side_rows") > 0
        else:
            assert Fs.stat("side_launches") == 0 and Fs.stat("launches") == Fo.stat("launches")
        same(state(Fs, b), state(Fo, b), "create")
        for i, v in enumerate(values):
            with knobs(env_off):
                Fo.refactor(v)
            with knobs(env_on):
                Fs.refactor(v)
            same(state(Fs, b), state(Fo, b), f"refactor {i}")
        if expect_side:   # no rebuild dropped the split on the way
            assert Fs.stat("side_launches") > 0
        return Fs, Fo
    except BaseException:
        Fs.close()
        Fo.close()
        raise


def diag_values(A, seeds=(5, 6, 7)):
    return [mats.perturb_diag(A, s).data for s in seeds]


@pytest.mark.parametrize("N,extra", [(24, None), (24, {"SMLU_OB": "128"}), (32, None)],
                         ids=["poisson3d_24", "poisson3d_24-OB128", "poisson3d_32"])
def test_bitwise_against_knob_off(gpu, N, extra):
    # 24: root 576 = 384 + 192 and fronts with update rows below their block; OB = 128: four full
    # blocks and a partial one; 32: root 1024, three blocks, fronts of one level that end their
    # blocks at different steps
    A = mats.poisson3d(N)
    Fs, Fo = run_pair(A, diag_values(A), extra)
    Fs.close()
    Fo.close()


def test_complex_handle_is_untouched(gpu):
    # pair-preserving pivots search every fully-summed row (mode 1): no front qualifies
    A = mats.poisson3d(16).astype(np.complex128)
    A.data = A.data * (1.0 + 0.25j)
    vals = [mats.perturb_diag(mats.poisson3d(16), s).data * (1.0 + 0.25j) for s in (5, 6, 7)]
    Fs, Fo = run_pair(A, vals, expect_side=False)
    assert Fs.stat("complex") == 1.0
    Fs.close()
    Fo.close()


def test_profile_mode_same_bits_and_finite_times(gpu):
    A = mats.poisson3d(24)
    Fs, Fo = run_pair(A, diag_values(A), profile=True)
    for k in ("trsm", "gemm", "gemmo", "gemm22", "panel", "urows", "small", "assemble"):
        for F in (Fs, Fo):
            t = F.stat("ms_" + k)
            assert np.isfinite(t) and t >= 0.0, (k, t)
    assert Fs.stat("ms_trsm") > 0.0 and Fs.stat("ms_gemm") > 0.0
    Fs.close()
    Fo.close()


def _golden(rel):
    z = np.load(os.path.join(HERE, "golden", rel), allow_pickle=False)
    n = int(z["n"])
    return sp.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=(n, n))


def test_nondominant_golden_is_untouched(gpu):
    A = _golden("fe_8.npz")
    rng = np.random.default_rng(3)
    vals = [A.data * (1.0 + 0.01 * rng.standard_normal(A.nnz)) for _ in range(3)]
    Fs, Fo = run_pair(A, vals, expect_side=False)
    assert Fs.stat("dominant") == 0.0
    Fs.close()
    Fo.close()


def test_nondominant_blocked_fronts_are_untouched(gpu):
    # the C1 fixture's pattern with values far from dominant: blocked fronts on the full-candidate
    # (mode 1) path, which the knob must leave alone
    A = _golden(os.path.join("c1", "c1_random_1000.npz"))
    rng = np.random.default_rng(9)
    A.data = rng.standard_normal(A.nnz)
    vals = [rng.standard_normal(A.nnz) for _ in range(3)]
    Fs, Fo = run_pair(A, vals, expect_side=False)
    assert Fs.stat("dominant") == 0.0 and Fs.stat("fronts_mode1") > 0
    Fs.close()
    Fo.close()


def test_ten_refactors_one_factor_hash(gpu):
    # the same values ten times through the captured graph: one hash of (L, U, p), as
    # tools/factor_hash.py forms it
    A = mats.poisson3d(32)
    v = mats.perturb_diag(A, 3).data
    with knobs({KNOB: "64"}):
        F = smlu.ParallelSparseLU(A)
        try:
            assert F.stat("side_launches") > 0
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
