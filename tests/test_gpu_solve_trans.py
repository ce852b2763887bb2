"""Transposed and adjoint solves from the factors of A (smlu_solve_trans*; ldiv_(..., trans="T"|"C")).

Host reference from the handle's own exported factors, L U = (Rs .* A)[p, q]:
    c = b[q];  U^T y = c;  L^T z = y;  x[p] = Rs[p] * z
(conjugate transposes for "C" on a complex handle), solved with scipy's sparse triangular solver.
Cases are the smallest that reach each kernel of kernels_solve_t.hip: the micro / tiny / small
front kernels and the n = 1, 2 edges (golden fixtures), large fronts with a partial last block,
nu = 0 at the root and the side-stream fork (poisson3d(28)), tall fronts (poisson2d(300)), row
exchanges inside every tile of one large front (tile_pivoting_matrix), the refinement path
(non-dominant FE matrix) and a complex handle, where "T" and "C" differ."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle as O
import smlu
from smlu import matrices as mats

from _parity import TOL, DENSE_TOL, isapprox, tile_pivoting_matrix

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def host_reference(F, b, trans):
    """A^T \\ b ("T") or A^H \\ b ("C") from F.L, F.U, F.p, F.q, F.Rs."""
    L, U, p, q, Rs = F.L, F.U, F.p, F.q, F.Rs
    Lt, Ut = (L.conj().T, U.conj().T) if trans == "C" else (L.T, U.T)
    y = spla.spsolve_triangular(sp.csr_matrix(Ut), b[q], lower=True)
    z = spla.spsolve_triangular(sp.csr_matrix(Lt), y, lower=False)
    x = np.empty_like(z)
    x[p] = Rs[p] * z
    return x


def normwise_berr(At, x, b):
    """||A^T x - b||_inf / (||A||_1 ||x||_inf + ||b||_inf); ||A||_1 = ||A^T||_inf."""
    r = At @ x - b
    return np.abs(r).max() / (abs(At).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())


def load_golden(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)
    n = int(z["n"])
    return sp.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=(n, n))


@pytest.mark.parametrize("name", ["dense_1", "dense_2", "dense_13", "fe_5", "poisson2d_16", "poisson3d_6",
                                  "random_dominant_200"])
def test_golden_fixtures(gpu, name):
    A = load_golden(name)
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A)
    b = np.random.default_rng(11).random(n)
    x = np.empty(n)
    smlu.ldiv_(x, F, b, trans="T")
    xr = host_reference(F, b, "T")
    tol = DENSE_TOL if name.startswith("dense") else TOL
    assert isapprox(x, xr, tol, tol), (np.linalg.norm(x - xr), np.linalg.norm(xr))
    xc = np.empty(n)
    smlu.ldiv_(xc, F, b, trans="C")   # a real handle: the adjoint is the transpose
    assert np.array_equal(x, xc)
    F.close()


def test_large_fronts_poisson3d_28(gpu):
    A = mats.poisson3d(28)
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A)
    assert F.stat("solve_sweeps") > 0   # the handle really has large fronts
    b = np.random.default_rng(12).random(n)
    x = np.empty(n)
    smlu.ldiv_(x, F, b, trans="T")
    xr = host_reference(F, b, "T")
    assert isapprox(x, xr, TOL, TOL), (np.linalg.norm(x - xr), np.linalg.norm(xr))
    res = np.abs(A.T @ x - b).max()
    assert res <= 1e-12 * np.abs(b).max(), res
    F.close()


def test_tall_fronts_poisson2d_300(gpu):
    A = mats.poisson2d(300)
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A)
    b = np.random.default_rng(13).random(n)
    x = np.empty(n)
    smlu.ldiv_(x, F, b, trans="T")
    xr = host_reference(F, b, "T")
    assert isapprox(x, xr, TOL, TOL), (np.linalg.norm(x - xr), np.linalg.norm(xr))
    F.close()


def _berr_against_splu(A, F, b):
    """The library's transposed solve against SuperLU's on the normwise backward error: both are
    backward stable but pivot differently, one decade covers the growth difference; floor n 2^-52."""
    n = A.shape[0]
    x = np.empty(n)
    smlu.ldiv_(x, F, b, trans="T")
    At = sp.csr_matrix(A.T)
    mine = normwise_berr(At, x, b)
    theirs = normwise_berr(At, spla.splu(sp.csc_matrix(A)).solve(b, trans="T"), b)
    bound = max(10.0 * theirs, n * 2.0 ** -52)
    print(f"normwise backward error: smlu {mine:.3e}, splu {theirs:.3e}, bound {bound:.3e}")
    assert mine <= bound, f"normwise backward error {mine:.3e} (splu {theirs:.3e}, bound {bound:.3e})"
    return mine, theirs


def test_row_exchanges_in_every_tile(gpu):
    A = sp.csc_matrix(tile_pivoting_matrix(700, 5))   # one front of 11 blocks, the last 60 wide
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A)
    # identity front permutations could not pass for the wrong reason
    assert not np.array_equal(F.p, F.fronts()["p0"])
    _berr_against_splu(A, F, np.random.default_rng(14).random(n))
    F.close()


def test_nondominant_takes_the_refinement_path(gpu):
    rng = np.random.default_rng(15)
    A = sp.csc_matrix(O.test_matrix(rng, 23, 14))   # 300 x 300 FE blocks, not diagonally dominant
    assert A.shape == (300, 300)
    F = smlu.ParallelSparseLU(A)
    assert F.stat("dominant") == 0
    _berr_against_splu(A, F, rng.random(300))
    # the refinement rule ran: a residual was taken and its backward error is reported
    assert F.stat("refine_steps") >= 0 and F.stat("refine_berr") >= 0
    F.close()


def test_complex_transpose_and_adjoint(gpu):
    rng = np.random.default_rng(16)
    P = sp.lil_matrix(mats.poisson3d(12), dtype=np.complex128)
    n = P.shape[0]
    for i in rng.choice(n - 1, 40, replace=False):   # a few complex off-diagonals, unsymmetric
        P[i, i + 1] += 0.2j * rng.random()
        P[i + 1, i] -= 0.1 + 0.3j * rng.random()
    A = sp.csc_matrix(P) + 0.3j * sp.identity(n, format="csc")
    F = smlu.ParallelSparseLU(A)
    assert F.is_complex
    b = rng.random(n) + 1j * rng.random(n)
    xt = np.empty(n, np.complex128)
    xc = np.empty(n, np.complex128)
    smlu.ldiv_(xt, F, b, trans="T")
    smlu.ldiv_(xc, F, b, trans="C")
    rt = spla.spsolve(sp.csc_matrix(A.T), b)
    rc = spla.spsolve(sp.csc_matrix(A.conj().T), b)
    assert isapprox(xt, rt, 1e-10, 1e-10), np.linalg.norm(xt - rt)
    assert isapprox(xc, rc, 1e-10, 1e-10), np.linalg.norm(xc - rc)
    assert np.linalg.norm(xt - xc) > 1e-3 * np.linalg.norm(xc)   # the two really differ
    assert isapprox(xc, host_reference(F, b, "C"), 1e-10, 1e-10)
    assert isapprox(xt, host_reference(F, b, "T"), 1e-10, 1e-10)
    F.close()


# ---- surface checks, all on one poisson3d(12) handle ------------------------------------------
@pytest.fixture(scope="module")
def p12(gpu):
    A = mats.poisson3d(12)
    F = smlu.ParallelSparseLU(A)
    b = np.random.default_rng(17).random(A.shape[0])
    x = np.empty(A.shape[0])
    smlu.ldiv_(x, F, b, trans="T")
    yield A, F, b, x
    F.close()


def test_in_place_host_and_device(p12):
    import torch
    A, F, b, x = p12
    assert np.abs(A.T @ x - b).max() <= 1e-12 * np.abs(b).max()
    v = b.copy()
    smlu.ldiv_(v, F, v, trans="T")
    assert np.array_equal(v, x)
    d = torch.from_numpy(b).to("cuda:0")
    F.solve_device(d, d, trans="T")
    assert np.array_equal(d.cpu().numpy(), x)


def test_multi_columns_bitwise_single(p12):
    import torch
    A, F, b, x = p12
    n = A.shape[0]
    B = torch.from_numpy(np.random.default_rng(18).random((3, n))).to("cuda:0")
    X = torch.empty_like(B)
    F.solve_multi_device(X, B, trans="T")
    for j in range(3):
        xj = torch.empty(n, dtype=torch.float64, device="cuda:0")
        F.solve_device(xj, B[j].contiguous(), trans="T")
        assert torch.equal(xj, X[j]), j
    Bh = np.asfortranarray(B.cpu().numpy().T)
    Xh = np.empty_like(Bh)
    smlu.ldiv_(Xh, F, Bh, trans="T")
    assert np.array_equal(Xh, X.cpu().numpy().T)


def test_repeatable_and_eager_equals_graph(p12, monkeypatch):
    A, F, b, x = p12
    x2 = np.empty_like(x)
    smlu.ldiv_(x2, F, b, trans="T")
    assert np.array_equal(x, x2)
    monkeypatch.setenv("SMLU_NO_GRAPH", "1")
    x3 = np.empty_like(x)
    smlu.ldiv_(x3, F, b, trans="T")
    monkeypatch.delenv("SMLU_NO_GRAPH")
    assert np.array_equal(x, x3)


def test_trans_n_is_the_forward_solve(p12):
    A, F, b, x = p12
    xf = np.empty_like(b)
    smlu.ldiv_(xf, F, b)
    xn = np.empty_like(b)
    smlu.ldiv_(xn, F, b, trans="N")
    assert np.array_equal(xf, xn)
    xt = np.empty_like(b)
    smlu.ldiv_(xt, F, b, trans="T")   # a transposed solve in between leaves the forward one alone
    xf2 = np.empty_like(b)
    smlu.ldiv_(xf2, F, b)
    assert np.array_equal(xf, xf2) and np.array_equal(xt, x)
    assert np.abs(A @ xf - b).max() <= 1e-12 * np.abs(b).max()


def test_new_factors_after_refactor(gpu):
    A = mats.poisson3d(12)
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A)
    b = np.random.default_rng(19).random(n)
    x = np.empty(n)
    smlu.ldiv_(x, F, b, trans="T")
    rng = np.random.default_rng(20)
    A2 = A.copy()
    A2.data = A.data * (1.0 + 0.2 * rng.random(A.nnz))   # same pattern, unsymmetric values
    smlu.lu_(F, A2)
    x2 = np.empty(n)
    smlu.ldiv_(x2, F, b, trans="T")
    assert np.abs(A2.T @ x2 - b).max() <= 1e-12 * np.abs(b).max()
    assert np.abs(A.T @ x2 - b).max() > 1e-6 * np.abs(b).max()   # not the old factors
    F.close()
