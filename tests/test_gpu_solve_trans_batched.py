"""Batched transposed and adjoint solves: up to 16 right-hand sides per pass of the transposed kernels
(smlu_solve_trans_multi[_device]; solve_multi_device(..., trans="T"|"C"), ldiv_ with 2D arrays).

The oracle throughout is the library's own single-vector transposed solve: column j of a batch must
be bitwise equal to solve_device of that column alone.  One residual check per matrix,
max|A^T x - b| <= 1e-12 max|b|, guards against both being wrong.  The shapes are those of
test_gpu_solve_trans.py, the smallest that reach each kernel: micro / tiny / small fronts and
n = 1, 2 (golden fixtures), large fronts with a partial last block, nu = 0 at the root and the
side-stream fork (poisson3d(28)), tall fronts (poisson2d(300)), row exchanges in every tile
(tile_pivoting_matrix), a complex handle and the refinement fallback.  Widths 2 .. 33 cross every
kernel instantiation (4, 8, 16 wide), partial batches and more than one batch.

Under the default options a non-dominant matrix is refined and the batch call goes column by column:
there the bitwise comparison is the single-vector solve against itself.  check_unrefined_batches
therefore repeats the non-dominant cases on a handle created with refine=0, counts the passes, and
holds a batch against unrefined host solves from the exported factors (tests/_batch_ref.py)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O
import smlu
from smlu import _lib as C
from smlu import matrices as mats

from _batch_ref import assert_batch_against_oracle, complex_tile_150, stale_slot_sequence
from _parity import DENSE_TOL, tile_pivoting_matrix
from test_gpu_solve_trans import load_golden

pytestmark = pytest.mark.gpu


def _rhs(n, nrhs, seed, complex_=False):
    import torch
    rng = np.random.default_rng(seed)
    B = rng.random((nrhs, n))
    if complex_:
        B = B + 1j * rng.random((nrhs, n))
    return torch.from_numpy(B).to("cuda:0")


def _single(F, bj, trans):
    import torch
    xj = torch.empty_like(bj)
    F.solve_device(xj, bj, trans=trans)
    return xj


def check_batch(F, nrhs, seed, trans="T"):
    """Solve nrhs columns in one call; every column bitwise its single solve.  Returns (B, X) on the
    device."""
    import torch
    B = _rhs(F.n, nrhs, seed, F.is_complex)
    X = torch.full_like(B, float("nan"))
    F.solve_multi_device(X, B, trans=trans)
    for j in range(nrhs):
        xj = _single(F, B[j].contiguous(), trans)
        assert torch.equal(X[j], xj), (nrhs, j, (X[j] - xj).abs().max().item())
    return B, X


def complex_p12():
    """The perturbed complex poisson3d(12) of test_gpu_solve_trans.py."""
    rng = np.random.default_rng(16)
    P = sp.lil_matrix(mats.poisson3d(12), dtype=np.complex128)
    n = P.shape[0]
    for i in rng.choice(n - 1, 40, replace=False):   # a few complex off-diagonals, unsymmetric
        P[i, i + 1] += 0.2j * rng.random()
        P[i + 1, i] -= 0.1 + 0.3j * rng.random()
    return sp.csc_matrix(P) + 0.3j * sp.identity(n, format="csc")


def nondominant_fe():
    return sp.csc_matrix(O.test_matrix(np.random.default_rng(15), 23, 14))   # 300 x 300 FE blocks


GOLDEN = ["dense_1", "dense_2", "dense_13", "fe_5", "poisson2d_16", "poisson3d_6", "random_dominant_200"]
MATRICES = {name: (lambda name=name: load_golden(name)) for name in GOLDEN}
MATRICES.update({
    "poisson3d_12": lambda: mats.poisson3d(12),
    "poisson3d_28": lambda: mats.poisson3d(28),
    "poisson2d_300": lambda: mats.poisson2d(300),
    "tile_pivoting_700_5": lambda: sp.csc_matrix(tile_pivoting_matrix(700, 5)),
    "complex_poisson3d_12": complex_p12,
    "nondominant_fe_300": nondominant_fe,
})


@pytest.mark.parametrize("name", list(MATRICES))
def test_residual_guard(gpu, name):
    """One residual check per matrix, max|A^T x - b| <= 1e-12 max|b| on a column of a batch (the
    bitwise tests compare the library with itself; this guards against both being wrong).

    The bound is absolute in b, so the right-hand sides are manufactured from solutions of order
    one, b = A^T x0 with x0 uniform in [0, 1) (A^H x0 for "C"): a residual in fp64 cannot be below
    about 2^-53 * (|A^T| |x|)_i, the effect of rounding x alone, and that is under the bound only
    while max|x| stays of order one.  With b uniform in [0, 1) poisson2d(300) has max|x| = 3.3e3:
    rounding the exact solution to fp64 already moves a row's residual by up to 8 * 2^-42 = 1.8e-12,
    and the solve measured 2.14e-11 there (normwise backward error 8e-16), the other twelve matrices
    3.5e-18 ... 2.9e-13.  A wrong solve leaves a residual of order max|b| with either kind of b."""
    import torch
    A = sp.csc_matrix(MATRICES[name]())
    F = smlu.ParallelSparseLU(A)
    X0 = _rhs(F.n, 2, 60, F.is_complex).cpu().numpy()
    for trans, At in (("T", A.T), ("C", A.conj().T)) if F.is_complex else (("T", A.T),):
        At = sp.csr_matrix(At)
        Bh = np.stack([At @ X0[0], At @ X0[1]])
        B = torch.from_numpy(Bh).to("cuda:0")
        X = torch.empty_like(B)
        F.solve_multi_device(X, B, trans=trans)
        b, x = Bh[1], X[1].cpu().numpy()
        res = np.abs(At @ x - b).max()
        print(f"{name} {trans}: max|A^T x - b| = {res:.3e}, max|b| = {np.abs(b).max():.3f}, max|x| = {np.abs(x).max():.3e}")
        assert res <= 1e-12 * np.abs(b).max(), res
    F.close()


# ---- one poisson3d(12) handle: pass count, width edges, layout, eager launches, neighbours -------
@pytest.fixture(scope="module")
def p12(gpu):
    A = mats.poisson3d(12)
    F = smlu.ParallelSparseLU(A)
    yield A, F
    F.close()


def test_pass_count(p12):
    import torch
    A, F = p12
    n = F.n
    p0 = F.stat("solve_trans_passes")
    assert np.isfinite(p0)
    B = _rhs(n, 17, 30)
    X = torch.empty_like(B)
    F.solve_multi_device(X[:8], B[:8], trans="T")
    p1 = F.stat("solve_trans_passes")
    assert p1 - p0 == 1, (p0, p1)
    F.solve_multi_device(X, B, trans="T")
    p2 = F.stat("solve_trans_passes")
    assert p2 - p1 == 2, (p1, p2)
    F.solve_device(X[0], B[0], trans="T")
    assert F.stat("solve_trans_passes") - p2 == 1


@pytest.mark.parametrize("nrhs", [2, 4, 5, 8, 9, 16, 17, 33])
def test_width_edges(p12, nrhs):
    import torch
    A, F = p12
    B, X = check_batch(F, nrhs, 31 + nrhs, "T")
    Xc = torch.empty_like(B)
    F.solve_multi_device(Xc, B, trans="C")   # a real handle: the adjoint is the transpose
    assert torch.equal(X, Xc)


def test_leading_dimensions(p12):
    import torch
    A, F = p12
    n, nr = F.n, 5
    ldb, ldx = n + 3, n + 7
    Bc = _rhs(n, nr, 40)
    Bbuf = torch.zeros(nr * ldb, dtype=torch.float64, device="cuda:0")
    Xbuf = torch.full((nr * ldx,), float("nan"), dtype=torch.float64, device="cuda:0")
    for j in range(nr):
        Bbuf[j * ldb:j * ldb + n] = Bc[j]
    torch.cuda.synchronize()
    with C.caller_stream(F._h, Bbuf):
        rc = C.lib().smlu_solve_trans_multi_device(F._h, C.SMLU_OP_T, nr, ctypes.c_void_p(Bbuf.data_ptr()), ldb,
                                                   ctypes.c_void_p(Xbuf.data_ptr()), ldx)
    assert rc == 0
    for j in range(nr):
        assert torch.equal(Xbuf[j * ldx:j * ldx + n], _single(F, Bc[j].contiguous(), "T")), j
        assert torch.isnan(Xbuf[j * ldx + n:(j + 1) * ldx]).all()   # the padding of X is never written


def test_x_aliases_b(p12):
    A, F = p12
    B, X = check_batch(F, 9, 41)
    V = B.clone()
    F.solve_multi_device(V, V, trans="T")
    import torch
    assert torch.equal(V, X)


def test_host_path_equals_device_path(p12):
    A, F = p12
    B, X = check_batch(F, 17, 42)
    Bh = np.asfortranarray(B.cpu().numpy().T)   # n x 17, column-major
    Xh = np.empty_like(Bh)
    smlu.ldiv_(Xh, F, Bh, trans="T")
    assert np.array_equal(Xh, X.cpu().numpy().T)
    V = Bh.copy(order="F")
    smlu.ldiv_(V, F, V, trans="T")             # in place on the host
    assert np.array_equal(V, Xh)


def test_eager_launches_equal_graph_replay(p12, monkeypatch):
    import torch
    A, F = p12
    B, X = check_batch(F, 8, 43)
    monkeypatch.setenv("SMLU_NO_GRAPH", "1")
    Xe = torch.empty_like(B)
    F.solve_multi_device(Xe, B, trans="T")
    monkeypatch.delenv("SMLU_NO_GRAPH")
    assert torch.equal(Xe, X)


def test_neighbouring_forward_batches(p12):
    import torch
    A, F = p12
    B = _rhs(F.n, 8, 44)
    X1 = torch.empty_like(B)
    F.solve_multi_device(X1, B)               # forward, in wrkm / vbufm
    Bt, Xt = check_batch(F, 8, 45)            # transposed, in the same buffers
    X2 = torch.empty_like(B)
    F.solve_multi_device(X2, B)
    assert torch.equal(X1, X2)
    Xt2 = torch.empty_like(Bt)
    F.solve_multi_device(Xt2, Bt, trans="T")
    assert torch.equal(Xt, Xt2)
    assert np.abs(A @ X1[0].cpu().numpy() - B[0].cpu().numpy()).max() <= 1e-12 * B[0].abs().max().item()


# ---- every kernel --------------------------------------------------------------------------------
def check_unrefined_batches(A, trans="T", label="", tol=None, **handle_kw):
    """A second handle with refine=0: under the default options a non-dominant matrix is refined and
    solve_cols goes column by column, so check_batch above compares the single-vector
    solve with itself there.  On this handle a batch of 8 is one pass of the batch kernels, widths 5,
    9 and 16 are bitwise their single solves, and the 5-wide batch is held against unrefined host
    solves from the exported factors (tests/_batch_ref.py)."""
    import torch
    F = smlu.ParallelSparseLU(A, refine=0, **handle_kw)
    B8 = _rhs(F.n, 8, 70, F.is_complex)
    X8 = torch.full_like(B8, float("nan"))
    p0 = F.stat("solve_trans_passes")
    F.solve_multi_device(X8, B8, trans=trans)
    assert F.stat("solve_trans_passes") - p0 == 1
    B, X = check_batch(F, 5, 71, trans)
    check_batch(F, 9, 72, trans)
    check_batch(F, 16, 73, trans)
    assert_batch_against_oracle(A, F, B.cpu().numpy(), X.cpu().numpy(), trans, tol=tol, label=label)
    return F


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_fixtures(gpu, name):
    A = load_golden(name)
    F = smlu.ParallelSparseLU(A)
    check_batch(F, 5, 50)
    check_batch(F, 16, 51)
    dominant = F.stat("dominant") == 1
    if name in ("dense_13", "fe_5"):
        assert not dominant
    F.close()
    if not dominant:
        check_unrefined_batches(A, "T", name).close()


def test_large_fronts_poisson3d_28(gpu):
    A = mats.poisson3d(28)
    F = smlu.ParallelSparseLU(A)
    assert F.stat("solve_sweeps") > 0   # the handle really has large fronts
    check_batch(F, 5, 52)
    check_batch(F, 16, 53)
    F.close()


def test_tall_fronts_poisson2d_300(gpu):
    A = mats.poisson2d(300)
    F = smlu.ParallelSparseLU(A)
    check_batch(F, 8, 54)
    F.close()


def test_row_exchanges_in_every_tile(gpu):
    A = sp.csc_matrix(tile_pivoting_matrix(700, 5))   # one front of 11 blocks, the last 60 wide
    F = smlu.ParallelSparseLU(A)
    assert not np.array_equal(F.p, F.fronts()["p0"])   # the rowperm scatter is not the identity
    check_batch(F, 8, 55)
    assert F.stat("dominant") == 0
    F.close()
    F0 = check_unrefined_batches(A, "T", "tile_pivoting_700_5")
    assert not np.array_equal(F0.p, F0.fronts()["p0"])
    F0.close()


def test_row_exchanges_in_small_fronts(gpu):
    """Rows moved inside micro, tiny and small fronts (the matrix of test_gpu_solve_batched.py)."""
    from test_gpu_solve_batched import HANDLE_KW, moved_rows_by_front_class, pivoting_small_fronts
    F = check_unrefined_batches(pivoting_small_fronts(), "T", "pivoting_small_fronts", tol=DENSE_TOL,
                                **HANDLE_KW["pivoting_small_fronts"])
    classes = moved_rows_by_front_class(F)
    assert classes["micro"] > 0 and classes["tiny"] > 0 and classes["small"] > 0, classes
    F.close()


def test_stale_slots_transposed(gpu):
    A = sp.csc_matrix(tile_pivoting_matrix(700, 5))
    F = smlu.ParallelSparseLU(A, refine=0)   # a fresh handle: nothing was solved on it before
    stale_slot_sequence(F, "T")
    F.close()


def test_complex_exchanged_pairs(gpu):
    """A complex handle whose real-equivalent pairs are moved and exchanged inside themselves:
    transposed and adjoint batches on unrefined factors."""
    A = complex_tile_150()
    Ft = check_unrefined_batches(A, "T", "complex_tile_150")
    assert Ft.is_complex and Ft.stat("cpair") == 1
    pk = Ft.real_equivalent_factors()["p"]
    assert int((pk[0::2] > pk[1::2]).sum()) > 0
    assert not np.array_equal(Ft.p, Ft.fronts()["p0"][0::2] // 2)
    Ft.close()
    check_unrefined_batches(A, "C", "complex_tile_150").close()


def test_complex_transpose_and_adjoint(gpu):
    A = complex_p12()
    F = smlu.ParallelSparseLU(A)
    assert F.is_complex
    B, Xt = check_batch(F, 5, 56, "T")
    Bc, Xc = check_batch(F, 5, 56, "C")   # the same right-hand sides
    assert (Xt - Xc).abs().max().item() > 1e-3 * Xc.abs().max().item()   # the two really differ
    F.close()


def test_refinement_falls_back_to_columns(gpu):
    A = nondominant_fe()
    assert A.shape == (300, 300)
    F = smlu.ParallelSparseLU(A)
    assert F.stat("dominant") == 0
    p0 = F.stat("solve_trans_passes")
    check_batch(F, 3, 57)   # 3 in the batch call + 3 single solves, corrections on top
    assert F.stat("solve_trans_passes") - p0 >= 6
    import torch
    B = _rhs(F.n, 3, 58)
    X = torch.empty_like(B)
    p1 = F.stat("solve_trans_passes")
    F.solve_multi_device(X, B, trans="T")
    assert F.stat("solve_trans_passes") - p1 >= 3   # one refined solve per column
    F.close()
