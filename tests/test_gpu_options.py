"""Options of smlu_opts that switch kernels or numerics and that no other GPU test sets:
use_mfma = 0, scale = 0, pivot_tol other than 0.1 and leaf_size other than 64.  refine = 0
throughout: every number below is the factors' and the plain solves' own.  The inputs are proved on
the CPU by test_options_inputs.py.

use_mfma=False (schedule_build.cpp: trsm_gemm off, fuse_mode 0): the diagonal-tile fronts run the
panel, k_laswp and k_step_trsm as three launches, k > 64 updates take the VALU 64 tile, no tile inverse
is formed, and the solves of the large fronts work from factors without them.  Inputs and rtol are
those of test_gpu_kernel_parity.py.  The handle is compared with the oracle (factor_parity: p bit for
bit, values at rtol times the growth), its solves N and T with assert_batch_against_oracle, its
log|det| with the default handle's within rounding(n, cond_1), and one refactor replay goes from
dominant values to weak-tile values (re-pivoting from this schedule) and back, bitwise.

scale=False: Rs is all ones bitwise and the factors match the fixed-pivot oracle with Rs = 1; and
against its twin: with r = O.rowscale(A) and B = diag(r) A (each product rounded once), the
scale=False handle of B assembles exactly the products Rs[row] * a that the scale=True handle of A
assembles, so L, U, p and the whole front store are bitwise equal -- which carries the pivot-choice
check, the multifrontal oracle restating pivoting only under SUM scaling (front_parity runs it on A
and compares B's handle with it).  Solves: forward, x = Q U^-1 L^-1 P (Rs .* b), so
solve(B-handle, r * b) is bitwise solve(A-handle, b).  Transposed, the library ends with
x[p0] = Rs[p0] .* z where z = L^-T U^-T b[q] depends on L, U, q alone: the B-handle returns z
scattered (times 1.0), the A-handle r .* that, so solve_T(A-handle, b) is bitwise
r * solve_T(B-handle, b) -- the same b on both sides, the scaling moves to the output.

pivot_tol: 0 switches the weak-pivot flag and with it the re-pivoting refactor off
(_weak_tile_matrix(700, 21), which re-pivots at 0.1).  The stricter value: tile_pivoting_matrix(1100,
1111), whose largest multiplier in a row outside the diagonal tile is 3.4595 by the oracle: below
1 / 0.1 = 10, no re-pivoting at the default; above 1 / 0.6 = 1.67, one re-pivoting refactor at
pivot_tol = 0.6, a factor of 2 to spare on either side.

leaf_size 16 and 256 under graph nested dissection: other trees and front shapes of poisson2d(40) and
poisson3d(12).

Measured on the MI355X (worst scaled factor difference against the oracle as factor_parity scales
it, max |G - R| / (growth max(1, max|R|)); worst berr ratio GPU / oracle over N, T and the batches;
|log|det| difference| against its bound):

  handle                                   factors    berr ratio   log|det| diff / bound
  use_mfma=0  poisson3d(16)                1.4e-15    1.19         0        / 1.4e-09
  use_mfma=0  poisson3d(24)                1.6e-15    0.95         0        / 1.0e-08
  use_mfma=0  _dominant_dense(700, 5)      1.1e-16    0.92         0        / 4.5e-12
  use_mfma=0  tile_pivoting(1100, 1111)    2.6e-13    1.29         1.8e-12  / 1.3e-07
  use_mfma=0  replay, weak tiles re-pivoted 2.4e-14   0.52         -
  scale=0     random_dominant(300)         2.2e-16    1.15         1.1e-13  / 1.6e-10
  scale=0     tile_pivoting(700, 5)        3.3e-14    2.09         3.6e-12  / 9.5e-08
  scale=0     poisson2d(20)                6.1e-16    1.07         1.7e-13  / 3.4e-10
  scale=0     poisson3d(10)                7.8e-16    0.99         6.8e-13  / 7.4e-10
  scale=0     fe_8                         1.6e-14    1.56         5.2e-13  / 2.7e-09
  pivot_tol=0    _weak_tile_matrix(700, 21)  4.7e-14 (growth 8.8e+03, no re-pivoting)
  pivot_tol=0.1  tile_pivoting(1100, 1111)   2.9e-13 (growth 197, repivots 0)
  pivot_tol=0.6  the same                    2.6e-13 (growth 197, repivots 1)
  leaf_size=16   poisson2d(40) nsuper 256 (default 186)  1.3e-15   |x - xs| / |xs| 3.7e-15
  leaf_size=256  poisson2d(40) nsuper 150                1.4e-15   5.0e-15
  leaf_size=16   poisson3d(12) nsuper 450 (default 276)  6.7e-16   7.9e-16
  leaf_size=256  poisson3d(12) nsuper 192                1.0e-15   1.3e-15

The scale=0 handles are bitwise their scale=1 twins in L, U, p and every front's stored values, forward and
transposed solves included; front_parity of the scale=0 handle against the multifrontal oracle run on A:
worst 2.4e-13 (fe_8), 2.0e-15 (tile_pivoting), <= 2.8e-16 for the other three.  The three use_mfma=0
handles with a zero log|det| difference have factors bitwise equal to the default handle's (the VALU and
MFMA tiles round alike); all four schedules hold k > 64 updates (launches_valu64 = 2, 6, 1, 2, the default
handle's launches_mfma64).  The norm agreement of fe_8's solves, cond_2 = 1.6e4, is asked at ctol = 8 eps cond_2
= 2.8e-11: measured 1.9e-12 (N) and 9.4e-15 (T) with backward errors of 4.7e-15 and 8.9e-16.
Running launch_rowscale unconditionally (tried, then reverted) fails every test_no_scale case at
"Rs is all ones".
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle as O
import smlu

import _options_inputs as I
from _batch_ref import assert_batch_against_oracle
from _diag_ref import cond1, rounding
from _parity import DENSE_TOL, TOL, _real, factor_parity, front_parity, isapprox, tile_pivoting_matrix
from test_gpu_solve_trans import host_reference

pytestmark = pytest.mark.gpu


def parity(A, F, label, **kw):
    """factor_parity, and the quantity it bounds by rtol printed: max |G - R| / (growth max(1, max|R|))
    over L and U.  Returns the fixed-pivot oracle."""
    ref = factor_parity(A, F, **kw)
    fx = _real(F)
    S = (sp.diags(ref.Rs) @ sp.csc_matrix(A)).tocsr()[fx["p"]][:, fx["q"]]
    rho = max(1.0, abs(ref.U).max() / max(abs(S).max(), 1e-300))
    d = max(abs(G - R).max() / (rho * max(abs(R).max(), 1.0)) for G, R in ((fx["L"], ref.L), (fx["U"], ref.U)))
    print(f"{label}: worst scaled factor difference {d:.2e} (rtol {kw.get('rtol', 1e-12):.0e}, growth {rho:.3g})")
    return ref


def front_values(F):
    """Every front's stored factor values (L panel M x ns, then U12 ns x nu) as one array: the factor
    store without the padding between the fronts, which no kernel writes."""
    store, off = F.front_store()
    fr = F.fronts()
    ns, nu = np.diff(fr["first"]), np.diff(fr["rowptr"])
    return np.concatenate([np.concatenate([store[o[0]:o[0] + (a + b) * a], store[o[1]:o[1] + a * b]])
                           for o, a, b in zip(off, ns, nu)])


def norm_tol(A):
    """The agreement in norm asked next to the berr rule: assert_batch_against_oracle's own (TOL,
    DENSE_TOL for a full matrix), or 8 eps cond_2(A) when that is larger (ctol, as test_gpu_complex.py
    and test_gpu_reference_suite.py have it); not computed above n = 3000, where the inputs are
    Poisson matrices and TOL holds."""
    n = A.shape[0]
    tol = DENSE_TOL if A.nnz == n * n else TOL
    return tol if n > 3000 else max(tol, 8 * np.finfo(float).eps * np.linalg.cond(A.toarray()))


def solves(A, F, ref, label, seed=0):
    """N and T, single vectors and a batch of 5 on the device: every batch column bitwise its single
    solve, all of them within assert_batch_against_oracle's bound of the host solves on F's own
    factors (N: the fixed-pivot oracle `ref`; T: host_reference).  Returns the worst berr ratio."""
    import torch
    n = A.shape[0]
    B = np.random.default_rng(100 + seed).random((5, n))
    dB = torch.from_numpy(B).to("cuda:0")
    worst, tol = 0.0, norm_tol(A)
    for trans in ("N", "T"):
        dX = torch.full_like(dB, float("nan"))
        F.solve_multi_device(dX, dB, trans=trans)
        X = dX.cpu().numpy()
        for j in range(5):
            dx = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
            F.solve_device(dx, dB[j].contiguous(), trans=trans)
            assert np.array_equal(dx.cpu().numpy(), X[j]), (label, trans, j)
        if trans == "N":
            Xo = np.empty_like(B)
            for j in range(5):
                ref.ldiv(Xo[j], B[j])
        else:
            Xo = np.stack([host_reference(F, B[j], "T") for j in range(5)])
        worst = max(worst, assert_batch_against_oracle(A, F, B, X, trans=trans, Xo=Xo, tol=tol, label=label))
    assert F.stat("refine_steps") == 0
    return worst


def cond1_of(A):
    """cond_1(A): from the explicit inverse when A is small, else for the Poisson M-matrices
    (A^-1 >= 0, so ||A^-1||_1 = ||A^-T 1||_inf: one SuperLU solve, as _diag_ref.poisson does)."""
    if A.shape[0] <= 2000:
        return cond1(A.toarray())
    inv1 = np.abs(spla.splu(sp.csc_matrix(A)).solve(np.ones(A.shape[0]), trans="T")).max()
    return abs(A).sum(axis=0).max() * inv1


# ---- use_mfma = False --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(I.NO_MFMA))
def test_no_mfma(gpu, name):
    A = I.matrix("no_mfma", name)
    rtol = I.NO_MFMA[name][1]
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A, use_mfma=False, refine=0)
    Fd = smlu.ParallelSparseLU(A, refine=0)
    try:
        # the comparison path ran
        assert F.stat("fronts_mode2") > 0
        for k in ("tri_inv", "mfma128", "mfma64", "mfma128_trsm", "k64_trsm", "valu64_trsm"):
            assert F.stat("launches_" + k) == 0, k
        print(f"{name}: launches valu64 {F.stat('launches_valu64'):.0f} k64 {F.stat('launches_k64'):.0f}; default "
              f"handle: tri_inv {Fd.stat('launches_tri_inv'):.0f} k64_trsm {Fd.stat('launches_k64_trsm'):.0f} "
              f"mfma64 {Fd.stat('launches_mfma64'):.0f} mfma128 {Fd.stat('launches_mfma128'):.0f}")
        # every one of the four schedules holds updates with k > 64: on the VALU 64 tile here, on the
        # MFMA 64 tile in the default handle
        assert F.stat("launches_valu64") > 0 and F.stat("launches_valu64") == Fd.stat("launches_mfma64")
        assert Fd.stat("launches_k64_trsm") + Fd.stat("launches_mfma128_trsm") > 0   # what the default runs instead
        ref = parity(A, F, name + " use_mfma=0", rtol=rtol)
        assert np.array_equal(F.p, Fd.p)
        w = solves(A, F, ref, name + " use_mfma=0")
        (la, sg), (lad, sgd) = F.logabsdet(), Fd.logabsdet()
        bound = rounding(n, cond1_of(A))
        print(f"{name}: berr ratio {w:.3f}; |logabsdet - default's| {abs(la - lad):.3e}, bound {bound:.3e}")
        assert sg == sgd and abs(la - lad) <= bound
    finally:
        F.close()
        Fd.close()


def test_no_mfma_refactor_replay_repivots_and_returns(gpu):
    """Dominant values -> weak-tile values -> the dominant values again on a use_mfma=False handle (the
    value sets of test_refactor_device_redecides_pivoting_mode): the weak tile pivots are flagged by
    this schedule's own kernels (the panel and k_step_trsm, no GEMM-form epilogue), the re-pivoting
    refactor runs once and matches the oracle in pivmode 1, and the third factor store is bitwise the
    first."""
    n = 700
    Ad, Aw = I.csc(I.dominant_dense(n, 41)), I.csc(I.weak_tile_matrix(n, 42))
    F = smlu.ParallelSparseLU(Ad, use_mfma=False, refine=0, diag_pivot_tol=0.1)
    try:
        assert F.stat("dominant") == 1 and F.stat("pivmode") == 0 and F.stat("fronts_mode2") > 0
        store1 = front_values(F)
        p1 = F.p.copy()
        parity(Ad, F, "replay 1 (dominant)", rtol=1e-11)
        F.refactor(Aw.data)
        assert F.stat("dominant") == 0
        assert F.stat("repivots") == 1 and F.stat("pivmode") == 1 and F.stat("weak") == 0
        assert F.stat("launches_tri_inv") == 0
        ref = parity(Aw, F, "replay 2 (weak tiles, re-pivoted)", rtol=1e-10)
        solves(Aw, F, ref, "replay 2", seed=2)
        F.refactor(Ad.data)
        assert F.stat("dominant") == 1 and F.stat("pivmode") == 0 and F.stat("repivots") == 1
        assert np.array_equal(F.p, p1)
        assert np.array_equal(front_values(F), store1)
    finally:
        F.close()


# ---- scale = False -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(I.NO_SCALE))
def test_no_scale(gpu, name):
    A = I.matrix("no_scale", name)
    rtol = I.NO_SCALE[name][1]
    n = A.shape[0]
    B, r = I.row_scaled_twin(A)
    one = np.ones(n)
    FA = smlu.ParallelSparseLU(A, refine=0)
    FB = smlu.ParallelSparseLU(B, scale=False, refine=0)
    try:
        # against the fixed-pivot oracle with Rs = 1
        assert np.array_equal(FB.Rs, one)
        ref = parity(B, FB, name + " scale=0", rtol=rtol, Rs_ref=one)
        w = solves(B, FB, ref, name + " scale=0")
        Bd = B.toarray()
        sref, lref = np.linalg.slogdet(Bd)
        la, sg = FB.logabsdet()
        tol = max(rounding(n, cond1(Bd)), 1e-12 * abs(lref))
        print(f"{name}: berr ratio {w:.3f}; |logabsdet - slogdet| {abs(la - lref):.3e}, bound {tol:.3e}")
        assert sg == sref and abs(la - lref) <= tol
        # against its twin, and through it against the multifrontal oracle's own pivots
        assert np.array_equal(FA.Rs, r)
        for k in ("p", "q"):
            assert np.array_equal(getattr(FB, k), getattr(FA, k)), k
        for k in ("L", "U"):
            G, T = getattr(FB, k), getattr(FA, k)
            assert np.array_equal(G.indptr, T.indptr) and np.array_equal(G.indices, T.indices), k
            assert np.array_equal(G.data, T.data), k
        assert np.array_equal(FB.front_store()[1], FA.front_store()[1])
        assert np.array_equal(front_values(FB), front_values(FA))
        assert FB.stat("pivmode") == FA.stat("pivmode") and FB.stat("dominant") == FA.stat("dominant")
        nf, ne, worst = front_parity(A, FB, rtol=rtol, Rs_ref=one)
        print(f"{name}: front_parity of the scale=0 handle against the oracle on A: {nf} fronts, worst {worst:.2e}")
        b = np.random.default_rng(n).random(n)
        xA, xB = np.empty(n), np.empty(n)
        smlu.ldiv_(xA, FA, b)
        smlu.ldiv_(xB, FB, r * b)
        assert np.array_equal(xB, xA)
        smlu.ldiv_(xA, FA, b, trans="T")
        smlu.ldiv_(xB, FB, b, trans="T")
        assert np.array_equal(r * xB, xA)
    finally:
        FA.close()
        FB.close()


# ---- pivot_tol ---------------------------------------------------------------------------------------
def test_pivot_tol_zero_never_flags_or_repivots(gpu):
    A = I.csc(I.weak_tile_matrix(700, 21))
    F = smlu.ParallelSparseLU(A, pivot_tol=0.0, diag_pivot_tol=0.1, refine=0)
    try:
        assert F.stat("pivot_tol") == 0.0
        assert F.stat("weak") == 0 and F.stat("repivots") == 0 and F.stat("pivmode") == 0
        assert F.stat("fronts_mode2") > 0
        parity(A, F, "weak tiles, pivot_tol=0", rtol=1e-10)
    finally:
        F.close()


def test_stricter_pivot_tol_repivots_where_the_default_does_not(gpu):
    D = tile_pivoting_matrix(*I.FLIP_SEED)
    A = I.csc(D)
    loose, strict = I.FLIP_TOLS
    F1 = smlu.ParallelSparseLU(A, pivot_tol=loose, refine=0)
    F6 = smlu.ParallelSparseLU(A, pivot_tol=strict, refine=0)
    try:
        assert F1.stat("repivots") == 0 and F1.stat("pivmode") == 0 and F1.stat("weak") == 0
        assert F1.stat("fronts_mode2") > 0
        assert F6.stat("pivot_tol") == strict
        assert F6.stat("repivots") == 1 and F6.stat("pivmode") == 1 and F6.stat("fronts_mode2") == 0
        parity(A, F1, f"pivot_tol={loose}", rtol=1e-10)
        ref = parity(A, F6, f"pivot_tol={strict}", rtol=1e-10)
        # (with the diagonal kept down to 0.001 of the column, the full-candidate pivots of this
        # matrix come out as the tile pivots did: p is the same, the schedule and the kernels are not)
        assert F6.stat("launches_panel_tall") > 0 and F1.stat("launches_panel_tall") == 0
        b = np.random.default_rng(6).random(A.shape[0])
        x = np.empty_like(b)
        smlu.ldiv_(x, F6, b)
        ctol = max(DENSE_TOL, 8 * np.finfo(float).eps * np.linalg.cond(D))
        assert isapprox(x, np.linalg.solve(D, b), ctol, ctol)
    finally:
        F1.close()
        F6.close()


# ---- leaf_size ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", I.LEAF_SIZES)
@pytest.mark.parametrize("name", list(I.LEAF))
def test_leaf_size(gpu, name, leaf):
    A = I.csc(I.LEAF[name]())
    n = A.shape[0]
    F0 = smlu.ParallelSparseLU(A, ordering="nd", refine=0)
    F = smlu.ParallelSparseLU(A, ordering="nd", leaf_size=leaf, refine=0)
    try:
        assert F.stat("nsuper") != F0.stat("nsuper")
        parity(A, F, f"{name} leaf_size={leaf} (nsuper {F.stat('nsuper'):.0f}, default {F0.stat('nsuper'):.0f})")
        b = np.random.default_rng(leaf).random(n)
        x = np.empty(n)
        smlu.ldiv_(x, F, b)
        xs = spla.spsolve(A, b)
        print(f"{name} leaf_size={leaf}: |x - xs| / |xs| = {np.linalg.norm(x - xs) / np.linalg.norm(xs):.2e}")
        assert isapprox(x, xs, TOL, TOL)
    finally:
        F.close()
        F0.close()
