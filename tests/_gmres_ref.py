"""Shared by test_gmres_derivation.py and test_gpu_gmres.py: a NumPy restatement of the algorithm of
smlu_solve_gmres* (include/smlu.h, csrc/krylov.cpp), the seeded inputs, and the per-input rtol.

The restatement is the algorithm step for step -- x0 = 0, right preconditioning, classical
Gram-Schmidt twice, Givens rotations, the same stopping and restart rules, convergence only on the
true residual -- with the operator and an exact preconditioner as callables: a dense inverse of the
unperturbed matrix for the small inputs, scipy's splu of it for the large ones.

Inputs: A' = A with every stored value scaled by 1 + delta u, u uniform in [-1, 1], seeded.  The
factorization the GPU preconditions with is that of A.

rtol per input: the library stops a cycle on `estimate <= rtol ||b||`, and the tests compare its
iteration count with the restatement's.  With rtol = 1e-10 itself a reference estimate that happens to
land near 1e-10 could fall on either side after the GPU's differently rounded arithmetic, so each input
takes the geometric mean of the two consecutive reference estimates that straddle 1e-10 (op N; the
restart cases from the history at their own restart length, because GMRES(1) and GMRES(30) do not pass
1e-10 at the same place: consecutive estimates here lie a factor of about 20 apart, so no single rtol
keeps a factor of 4 from both neighbours in five different histories, whatever the seed).  An estimate
below FLOOR = 2^-44 (4096 unit roundoffs: under what fp64 residuals of these sizes can resolve) counts
as FLOOR there, so that rtol never asks for a true residual that the arithmetic
cannot deliver (dense_1 and dense_2 end on an estimate of exactly or nearly 0).
tests/test_gmres_derivation.py checks that every (input, op, restart) the GPU test runs keeps a factor
of 4 between that rtol and the reference estimates on either side of the stop."""
import functools
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from smlu import matrices as mats

from _diag_ref import EPS, load_golden

FLOOR = 2.0 ** -44

# name -> (base matrix, delta, seed of u, seed of b)
SMALL = {
    "dense_1": ("dense_1", 1e-2, 101, 201),
    "dense_2": ("dense_2", 1e-2, 102, 202),
    "dense_13": ("dense_13", 1e-2, 103, 203),
    "fe_5": ("fe_5", 1e-2, 104, 204),
    "fe_8": ("fe_8", 1e-2, 105, 205),
    "poisson2d_16": ("poisson2d_16", 1e-2, 106, 206),
    "poisson3d_6": ("poisson3d_6", 1e-2, 107, 207),
    "random_dominant_200": ("random_dominant_200", 1e-2, 108, 208),
    "poisson3d_6@5e-2": ("poisson3d_6", 5e-2, 110, 228),   # seeds searched: test_gmres_derivation.py
    "random_dominant_200@5e-2": ("random_dominant_200", 5e-2, 110, 210),
}
LARGE = {
    "poisson3d_28+I": ("3d_28", 2e-2, 111, 211),
    "poisson2d_300+I": ("2d_300", 2e-2, 112, 212),
}
INPUTS = list(SMALL) + list(LARGE)
# the inputs whose A is not symmetric, and the large-front case, also run transposed and adjoint
TRANS_TOO = ["random_dominant_200", "fe_5", "dense_13", "poisson3d_28+I"]
RESTART_INPUTS = ["poisson3d_6@5e-2", "random_dominant_200@5e-2"]
RESTARTS = [1, 2, 5, 32]
MAXIT_INPUT = "poisson3d_6@5e-2"   # the maxit = 3, rtol = 1e-14 case


def gpu_cases():
    """Every (input, op, restart) the GPU test runs to convergence."""
    out = []
    for name in INPUTS:
        for op in ["N"] + (["T", "C"] if name in TRANS_TOO else []):
            out.append((name, op, 30))
    for name in RESTART_INPUTS:
        for m in RESTARTS:
            out.append((name, "N", m))
    return out


def _canon(A):
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    A.sum_duplicates()
    return A


def perturbed(A, delta, seed):
    """A' = A .* (1 + delta u) on A's stored entries, u uniform in [-1, 1]."""
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, A.nnz)
    A2 = A.copy()
    A2.data = A.data * (1.0 + delta * u)
    return A2


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(A, A2, b, delta, prec): A the factored matrix, A2 = A', prec(op)(v) = op(A)^-1 v exactly."""
    if name in SMALL:
        base, delta, su, sb = SMALL[name]
        A = _canon(load_golden(base))
        Ainv = np.linalg.inv(A.toarray())

        def prec(op):
            M = Ainv if op == "N" else Ainv.T
            return lambda v: M @ v
    else:
        base, delta, su, sb = LARGE[name]
        P = mats.poisson3d(28) if base == "3d_28" else mats.poisson2d(300)
        A = _canon(P + sp.identity(P.shape[0], format="csc"))
        lu = spla.splu(A)

        def prec(op):
            return lambda v: lu.solve(v, trans="N" if op == "N" else "T")
    A2 = perturbed(A, delta, su)
    b = np.random.default_rng(sb).uniform(-1.0, 1.0, A.shape[0])
    return dict(A=A, A2=A2, b=b, delta=delta, prec=prec, n=A.shape[0])


def operator(A2, op):
    """v -> op(A') v (real: the adjoint is the transpose)."""
    M = sp.csr_matrix(A2) if op == "N" else sp.csr_matrix(A2.T)
    return lambda v: M @ v


def gmres_ref(apply_op, prec, b, rtol, restart=30, maxit=200):
    """The algorithm of smlu_solve_gmres*.  Returns dict(x, converged, iters, cycles, solves, hist,
    true): hist[i] the relative estimate after Arnoldi step i (hist[0] = 1), true[c] the relative true
    residual at the start of cycle c and, last, of the returned x."""
    n = b.size
    x = np.zeros(n)
    bnorm = float(np.linalg.norm(b))
    out = dict(x=x, converged=False, iters=0, cycles=0, solves=0, hist=[1.0], true=[1.0], bnorm=bnorm)
    tol = rtol * bnorm
    if bnorm <= tol:     # b = 0 (or rtol >= 1): x = 0
        out["converged"] = True
        return out
    if not math.isfinite(bnorm):
        return out
    beta, prev, on_est = bnorm, math.inf, False
    iters = cycles = solves = 0
    r = b.copy()
    while True:
        if cycles > 0:
            r = b - apply_op(x)
            beta = float(np.linalg.norm(r))
            out["true"].append(beta / bnorm)
            if not math.isfinite(beta):
                break
            if beta <= tol:
                out["converged"] = True
                break
            if on_est and beta > 0.5 * prev:
                break
        if iters >= maxit:
            break
        prev, on_est = beta, False
        cycles += 1
        V = np.zeros((n, restart + 1))
        R = np.zeros((restart, restart))
        cs, sn, g = np.zeros(restart), np.zeros(restart), np.zeros(restart + 1)
        V[:, 0] = r / beta
        g[0] = beta
        k, finite = 0, True
        for j in range(restart):
            w = apply_op(prec(V[:, j]))
            solves += 1
            Vj = V[:, :j + 1]
            h1 = Vj.T @ w
            w = w - Vj @ h1
            h2 = Vj.T @ w
            w = w - Vj @ h2
            hc = h1 + h2
            hn = float(np.linalg.norm(w))
            for i in range(j):
                a, c = hc[i], hc[i + 1]
                hc[i] = cs[i] * a + sn[i] * c
                hc[i + 1] = -sn[i] * a + cs[i] * c
            a = hc[j]
            d = math.hypot(a, hn)
            c_, s_ = (a / d, hn / d) if (d > 0.0 and hn != 0.0) else (1.0, 0.0)
            hc[j] = d if hn != 0.0 else a
            cs[j], sn[j] = c_, s_
            g[j + 1] = -s_ * g[j]
            g[j] = c_ * g[j]
            R[:j + 1, j] = hc
            est = abs(g[j + 1])
            iters += 1
            out["hist"].append(est / bnorm)
            if not (math.isfinite(est) and math.isfinite(hn)):
                finite = False
                break
            k = j + 1
            if est <= tol or hn == 0.0:
                on_est = True
                break
            if iters >= maxit:
                break
            V[:, j + 1] = w / hn
        if not finite:
            out["true"].append(float(np.linalg.norm(b - apply_op(x))) / bnorm)
            break
        y = np.zeros(k)
        gg = g[:k].copy()
        for i in range(k - 1, -1, -1):
            y[i] = gg[i] / R[i, i]
            gg[:i] -= R[:i, i] * y[i]
        x = x + prec(V[:, :k] @ y)
        solves += 1
    out.update(x=x, iters=iters, cycles=cycles, solves=solves)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, op="N", restart=30, rtol=None, maxit=200):
    """gmres_ref on the named input (rtol None: the input's own, rtol_of(name))."""
    P = problem(name)
    return gmres_ref(operator(P["A2"], op), P["prec"](op), P["b"], rtol_of(name, restart) if rtol is None else rtol,
                     restart, maxit)


@functools.lru_cache(maxsize=None)
def rtol_of(name, restart=30):
    """Geometric mean of the two consecutive reference estimates (op N) that straddle 1e-10."""
    h = reference(name, "N", restart, 1e-10)["hist"]
    assert h[-1] <= 1e-10 < h[-2], (name, h)
    return math.sqrt(h[-2] * max(h[-1], FLOOR))


def gamma(A2, x, b, op="N"):
    """(max entries per row + 2) 2^-52 || |op(A')||x| + |b| ||_2 / ||b||_2: the rounding of evaluating
    the residual b - op(A') x in fp64, relative to ||b||."""
    M = sp.csr_matrix(abs(A2)) if op == "N" else sp.csr_matrix(abs(A2).T)
    width = int(np.diff(M.indptr).max())
    return (width + 2) * EPS * float(np.linalg.norm(M @ np.abs(x) + np.abs(b))) / float(np.linalg.norm(b))


def relres(A2, x, b, op="N"):
    return float(np.linalg.norm(b - operator(A2, op)(x)) / np.linalg.norm(b))
