"""A reference for the batched solves that is not the library: the componentwise backward error in
extended precision, and unrefined host solves on the GPU's own pivot order (the fixed-pivot oracle
for A x = b; the exported factors through scipy's sparse triangular solver for the transposed
directions, host_reference of test_gpu_solve_trans.py).  Shared by test_batch_ref.py, which proves
the checker on the CPU, test_gpu_solve_batched.py and test_gpu_solve_trans_batched.py.

Batches are host arrays of shape (nrhs, n), one right-hand side per row, as solve_multi_device
takes them.

The bound of assert_batch_against_oracle, per column j:
    berr(op(A), X[j], B[j]) <= max(4 * berr(op(A), Xo[j], B[j]), 2^-51)
4 is two bits for what legitimately differs between two stable substitutions on the same factors
(summation order -- dot64_split -- and FMA contraction); 2^-51, four unit roundoffs, is the
library's own rounding floor (solve_refined_by stops refining there).  Next to it X[j] must agree
with Xo[j] in norm at the parity tolerance (1e-10 for a full matrix, 1e-12 otherwise)."""
import numpy as np
import scipy.sparse as sp

import oracle as O

from _parity import TOL, DENSE_TOL, isapprox, tile_pivoting_matrix, _real

FLOOR = 2.0 ** -51
FACTOR = 4.0


def complex_tile_150():
    """The matrix of test_gpu_logabsdet.py::test_complex_pairs_exchanged_and_moved: tiny diagonals
    move the pairs of the real-equivalent matrix, random phases exchange many of them inside
    themselves."""
    rng = np.random.default_rng(7)
    return sp.csc_matrix(tile_pivoting_matrix(150, 7) * np.exp(2j * np.pi * rng.random((150, 150))))


def stale_slot_sequence(F, trans="N"):
    """On a real handle F that solves in batches (GPU): results of widths 1, 3, 5, 9, 15 before any
    NaN was seen; then a 16-wide all-NaN batch and an all-NaN single vector fill every slot of the
    work buffers; the same widths again must be finite and bitwise what they were.  Then a 9-wide
    batch with column 4 NaN and column 6 zero: the other seven columns unchanged, column 4 NaN,
    column 6 exactly zero.  No control flow of the solve kernels depends on values and the sweeps
    hand off by flags, so NaN provokes nothing; it only makes 0 * stale visible.  Every call is
    counted in "solve_passes" / "solve_trans_passes": one pass per batch."""
    import torch
    n = F.n
    B = torch.from_numpy(np.random.default_rng(160).random((15, n))).to("cuda:0")
    widths = (1, 3, 5, 9, 15)
    key = "solve_passes" if trans == "N" else "solve_trans_passes"

    def solve(Bw):
        X = torch.full_like(Bw, float("nan"))
        p0 = F.stat(key)
        F.solve_multi_device(X, Bw, trans=trans)
        assert F.stat(key) - p0 == 1, (Bw.shape[0], F.stat(key) - p0)
        return X

    before = {w: solve(B[15 - w:].contiguous()) for w in widths}   # a slot holds another column at every width
    for w in widths:
        assert torch.isfinite(before[w]).all(), w
    nan16 = torch.full((16, n), float("nan"), dtype=torch.float64, device="cuda:0")
    out16 = torch.zeros_like(nan16)
    F.solve_multi_device(out16, nan16, trans=trans)
    out1 = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    F.solve_device(out1, nan16[0].contiguous(), trans=trans)
    assert torch.isnan(out16).any() and torch.isnan(out1).any()   # the NaN really went through
    for w in widths:
        X = solve(B[15 - w:].contiguous())
        assert torch.isfinite(X).all(), w
        assert torch.equal(X, before[w]), w
    B9 = B[6:].clone()
    B9[4] = float("nan")
    B9[6] = 0.0
    X9 = solve(B9)
    keep = [0, 1, 2, 3, 5, 7, 8]
    assert torch.equal(X9[keep], before[9][keep])
    assert torch.isnan(X9[4]).any()
    assert (X9[6] == 0).all()


def _rowsum(indptr, vals, n):
    """Sum of vals over every CSR row, in vals' own precision (empty rows: 0)."""
    out = np.zeros(n, vals.dtype)
    rows = np.flatnonzero(np.diff(indptr) > 0)
    if rows.size:
        out[rows] = np.add.reduceat(vals, indptr[rows])
    return out


def berr(A, x, b):
    """Componentwise backward error max_i |b - A x|_i / (|A||x| + |b|)_i (Oettli-Prager); the
    products and the sums in np.longdouble, rows with a zero denominator skipped, complex input
    through moduli."""
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    n = A.shape[0]
    z = np.iscomplexobj(A.data) or np.iscomplexobj(x) or np.iscomplexobj(b)
    hp = np.clongdouble if z else np.longdouble
    a = A.data.astype(hp)
    xc = np.asarray(x).astype(hp)[A.indices]
    r = np.asarray(b).astype(hp) - _rowsum(A.indptr, a * xc, n)
    den = _rowsum(A.indptr, np.abs(a) * np.abs(xc), n) + np.abs(np.asarray(b).astype(hp))
    ok = den > 0
    if not ok.any():
        return 0.0
    return float((np.abs(r)[ok] / den[ok]).max())


def op_matrix(A, trans):
    A = sp.csc_matrix(A)
    return A if trans == "N" else sp.csc_matrix(A.T) if trans == "T" else sp.csc_matrix(A.conj().T)


def oracle_columns(A, F, B, trans="N"):
    """The columns of B solved without refinement on F's pivot order: "N" by the fixed-pivot oracle's
    ldiv (a complex F: the oracle's LU of the real-equivalent K on interleaved vectors), "T" / "C"
    from F's exported factors (the oracle has no transposed solve)."""
    B = np.asarray(B)
    Xo = np.empty_like(B)
    if trans == "N":
        if getattr(F, "is_complex", False):
            fx = _real(F)
            ref = O.OracleLU(O.real_equivalent(A), fx["p"], fx["q"], fx["Rs"])
            for j in range(B.shape[0]):
                xk = np.empty(2 * F.n)
                ref.ldiv(xk, np.ascontiguousarray(B[j], dtype=np.complex128).view(np.float64))
                Xo[j] = xk.view(np.complex128)
        else:
            ref = O.OracleLU(A, F.p, F.q, F.Rs)
            assert ref.status == 0
            for j in range(B.shape[0]):
                ref.ldiv(Xo[j], B[j])
    else:
        from test_gpu_solve_trans import host_reference
        for j in range(B.shape[0]):
            Xo[j] = host_reference(F, B[j], trans)
    return Xo


def assert_batch_against_oracle(A, F, B, X, trans="N", Xo=None, tol=None, label=""):
    """Every column of the batch X against the oracle's (or the given reference Xo): the backward
    error bound and the agreement in norm of the module docstring.  Returns the largest ratio
    berr(X[j]) / berr(Xo[j]) (printed with both errors)."""
    A = sp.csc_matrix(A)
    n = A.shape[0]
    B, X = np.asarray(B), np.asarray(X)
    assert B.shape == X.shape and B.shape[1] == n
    if Xo is None:
        Xo = oracle_columns(A, F, B, trans)
    if tol is None:
        tol = DENSE_TOL if A.nnz == n * n else TOL
    Op = sp.csr_matrix(op_matrix(A, trans))
    worst, wg, wo, dist = 0.0, 0.0, 0.0, 0.0
    fails = []
    for j in range(B.shape[0]):
        g, o = berr(Op, X[j], B[j]), berr(Op, Xo[j], B[j])
        ratio = g / max(o, 2.0 ** -70)
        if ratio >= worst:
            worst, wg, wo = ratio, g, o
        if not g <= max(FACTOR * o, FLOOR):
            fails.append(f"column {j}: backward error {g:.3e}, the oracle's {o:.3e}")
        dist = max(dist, np.linalg.norm(X[j] - Xo[j]) / max(np.linalg.norm(X[j]), np.linalg.norm(Xo[j]), 1e-300))
        if not isapprox(X[j], Xo[j], tol, tol):
            fails.append(f"column {j}: |x - xo| = {np.linalg.norm(X[j] - Xo[j]):.3e}, |xo| = {np.linalg.norm(Xo[j]):.3e}")
    print(f"{label or 'batch'} {trans}: {B.shape[0]} columns, largest berr ratio GPU/oracle {worst:.3f} "
          f"({wg:.3e} / {wo:.3e}), largest |x - xo| / |xo| {dist:.3e} (tolerance {tol:.0e})")
    assert not fails, "; ".join(fails[:4])
    return worst
