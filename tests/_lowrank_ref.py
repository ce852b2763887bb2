"""Shared by test_lowrank_derivation.py and test_gpu_lowrank.py: the seeded inputs of the low-rank
update tests and a NumPy restatement of smlu_lowrank_set* / smlu_solve_lowrank* (include/smlu.h,
csrc/lowrank.cpp).

The restatement is the algorithm step for step -- Y = op(A)^-1 W, the capacitance matrix, the
Sherman-Morrison-Woodbury solve, refinement on the updated system with the library's residual,
denominator and stopping rule -- with an exact preconditioner: a dense inverse of A for the goldens,
scipy's splu for the large inputs.

Update kinds:  "cols" replaces k random columns on A's pattern, U[:, t] = A[:, j_t] * u with u uniform
in [-1, 1] (default_rng(1000 + k)) and V = e_{j_t};  "dense" takes U and V uniform in [-1, 1]."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from smlu import matrices as mats

from _diag_ref import EPS, GOLDEN, load_golden

KS = [1, 2, 7, 16, 17, 32]          # 17 crosses the batch of 16 columns, 32 is the widest instantiation
LARGE = {"poisson3d_28+I": "3d_28", "poisson2d_300+I": "2d_300"}
LARGE_KS = {"poisson3d_28+I": KS, "poisson2d_300+I": [2, 16]}
TRANS_TOO = ["random_dominant_200", "fe_5", "dense_13", "poisson3d_28+I", "poisson2d_300+I"]
DENSE_KIND = [("dense_13", 7), ("random_dominant_200", 17), ("poisson3d_28+I", 32)]
BERR_STOP = 2.0 ** -51              # the refinement's target: 4 unit roundoffs


def _canon(A):
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    A.sum_duplicates()
    return A


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(A, n, b, prec, cond1): prec(op)(M) = op(A)^-1 M exactly, for a vector or a matrix."""
    if name in LARGE:
        P = mats.poisson3d(28) if LARGE[name] == "3d_28" else mats.poisson2d(300)
        A = _canon(P + sp.identity(P.shape[0], format="csc"))
        n = A.shape[0]
        lu = spla.splu(A)

        def prec(op):
            return lambda M: lu.solve(np.asarray(M, dtype=np.float64), trans="N" if op == "N" else "T")
        # an M-matrix: A^-1 >= 0, so ||A^-1||_1 = ||A^-T 1||_inf exactly
        c1 = float(abs(A).sum(axis=0).max() * np.abs(lu.solve(np.ones(n), trans="T")).max())
    else:
        A = _canon(load_golden(name))
        n = A.shape[0]
        Ainv = np.linalg.inv(A.toarray())

        def prec(op):
            M_ = Ainv if op == "N" else Ainv.T
            return lambda M: M_ @ M
        c1 = float(np.abs(A.toarray()).sum(axis=0).max() * np.abs(Ainv).sum(axis=0).max())
    b = np.random.default_rng(77).uniform(-1.0, 1.0, n)
    return dict(A=A, n=n, b=b, prec=prec, cond1=c1)


@functools.lru_cache(maxsize=None)
def update(name, k, kind):
    """(U, V, cols): n x k Fortran-ordered arrays; cols the replaced columns (kind "cols"), else None."""
    P = problem(name)
    A, n = P["A"], P["n"]
    rng = np.random.default_rng(1000 + k)
    if kind == "dense":
        U = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, k)))
        V = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, k)))
        return U, V, None
    cols = np.sort(rng.choice(n, size=k, replace=False))
    U = np.zeros((n, k), order="F")
    V = np.zeros((n, k), order="F")
    for t, j in enumerate(cols):
        lo, hi = A.indptr[j], A.indptr[j + 1]
        U[A.indices[lo:hi], t] = A.data[lo:hi] * rng.uniform(-1.0, 1.0, hi - lo)
        V[j, t] = 1.0
    return U, V, cols


def updated_matrix(name, k, kind):
    """A' = A + U V^T: sparse on A's pattern for kind "cols", dense otherwise (goldens only)."""
    A = problem(name)["A"]
    U, V, cols = update(name, k, kind)
    if cols is None:
        return A.toarray() + U @ V.T
    A2 = A.copy()
    for t, j in enumerate(cols):
        lo, hi = A.indptr[j], A.indptr[j + 1]
        A2.data[lo:hi] = A.data[lo:hi] + U[A.indices[lo:hi], t]
    return A2


def gpu_cases():
    """Every (input, k, kind, op) the GPU test runs."""
    out = []
    for name in GOLDEN + list(LARGE):
        n = problem(name)["n"]
        ks = [k for k in (LARGE_KS[name] if name in LARGE else KS) if k <= n]
        for k in ks:
            out.append((name, k, "cols", "N"))
        if name in TRANS_TOO:
            for op in ("T", "C"):
                for k in ks:
                    out.append((name, k, "cols", op))
    for name, k in DENSE_KIND:
        out.append((name, k, "dense", "N"))
        out.append((name, k, "dense", "T"))
    return out


def op_matrix(A, op):
    return sp.csr_matrix(A) if op == "N" else sp.csr_matrix(A.T)


def sides(U, V, op):
    """(W, Wd): op(A + U V^T) = op(A) + W Wd^T."""
    return (U, V) if op == "N" else (V, U)


def residual(A, U, V, x, b, op):
    """(r, berr): r = b - op(A) x - W (Wd^T x); berr = max_i |r_i| / (|op(A)||x| + |W| (|Wd|^T |x|) + |b|)_i."""
    M = op_matrix(A, op)
    W, Wd = sides(U, V, op)
    r = b - M @ x - W @ (Wd.T @ x)
    den = abs(M) @ np.abs(x) + np.abs(W) @ (np.abs(Wd).T @ np.abs(x)) + np.abs(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(r == 0.0, 0.0, np.where(den > 0.0, np.abs(r) / den, np.inf))
    return r, float(q.max())


def width(A, k, op):
    """Terms of one residual row: the most entries in a row of op(A), and 2 k for W (Wd^T x)."""
    return int(np.diff(op_matrix(A, op).indptr).max()) + 2 * k


def normwise(A, U, V, x, b, op, anorm=None):
    """eta = ||b - op(A') x||_inf / (||op(A')||_inf ||x||_inf + ||b||_inf), A' = A + U V^T.  anorm:
    ||op(A')||_inf where the caller has A' (the goldens); None: its upper bound by the row sums of
    |op(A)| + |W| |Wd|^T (the large inputs, where only ratios of eta on the same input are used)."""
    M = op_matrix(A, op)
    W, Wd = sides(U, V, op)
    r = b - M @ x - W @ (Wd.T @ x)
    if anorm is None:
        anorm = float((np.asarray(abs(M).sum(axis=1)).ravel() + np.abs(W) @ np.abs(Wd).sum(axis=0)).max())
    return float(np.abs(r).max() / (anorm * np.abs(x).max() + np.abs(b).max()))


def polished_solve(M, b):
    """np.linalg.solve(M, b) polished by three steps of refinement with the residual and the sum in
    extended precision, so that the forward-error check measures the code under test against the
    solution itself and not against the reference's own rounding (which is of the size of the bound:
    np.linalg.solve's backward error is no smaller than the library's)."""
    Ml, bl = M.astype(np.longdouble), b.astype(np.longdouble)
    x = np.linalg.solve(M, b).astype(np.longdouble)
    for _ in range(3):
        x = x + np.linalg.solve(M, (bl - Ml @ x).astype(np.float64))
    return x


def lowrank_ref(A, U, V, b, op, prec, steps=3):
    """The algorithm of smlu_lowrank_set + smlu_solve_lowrank.  Returns dict(x, x0, steps, stop, berr,
    berrs, C): x0 the unrefined solution, berrs every backward error measured."""
    k = U.shape[1]
    W, Wd = sides(U, V, op)
    Yw = prec(W)
    Cop = np.eye(k) + Wd.T @ Yw                      # N: C;  T: C^T

    def solve(v):
        y0 = prec(v)
        return y0 - Yw @ np.linalg.solve(Cop, Wd.T @ y0) if k else y0
    x = solve(b)
    out = dict(x0=x.copy(), steps=0, stop=0, berr=-1.0, berrs=[], C=Cop)
    prev = np.inf
    for _ in range(steps):
        r, berr = residual(A, U, V, x, b, op)
        out["berr"] = berr
        out["berrs"].append(berr)
        if berr <= BERR_STOP:
            out["stop"] = 1
            break
        if berr > 0.5 * prev:
            out["stop"] = 2
            break
        prev = berr
        x = x + solve(r)
        out["steps"] += 1
    if steps > 0 and out["stop"] == 0:
        out["stop"] = 3
    out["x"] = x
    return out


@functools.lru_cache(maxsize=None)
def reference(name, k, kind, op):
    P = problem(name)
    U, V, _ = update(name, k, kind)
    return lowrank_ref(P["A"], U, V, P["b"], op, P["prec"]("N" if op == "N" else "T"))


def berr_bound(A, k, op):
    """2^-51, the refinement's target, plus (w + 2) 2^-52: the rounding of evaluating one residual row of
    w terms in fp64 (the library's sum and NumPy's are ordered differently)."""
    return BERR_STOP + (width(A, k, op) + 2) * EPS
