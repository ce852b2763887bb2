"""CPU restatements of what csrc/diag.cpp and csrc/kernels_diag.hip compute, so that
the two claims the GPU tests lean on can be reproduced from the tree:

* the complex determinant's fold: an LU of the real-equivalent K with pair-preserving pivots gives
  det A = sign(pair permutation) i^sw prod (U[2k,2k] - i U[2k,2k+1]) and |det A|^2 = |det K|;
* the Hager / Higham estimate as diag.cpp runs it (dlacn2 / zlacn2 with est = max(est, sum|y|) and
  sign(0) = +1) reaches 0.9 of the exact ||A^-1|| on every input of tests/test_gpu_rcond.py, in at
  most 11 solves: the lower bound asserted there is a property of those inputs."""
import numpy as np
import pytest
import scipy.linalg as sla

from _diag_ref import GOLDEN, load_golden
from _parity import tile_pivoting_matrix
from test_gpu_complex import helmholtz3d
from test_oracle import complex_fe


def pair_lu(A):
    """Dense LU of K = phi(A), pivoting pair by pair: the pair with the largest complex modulus in
    the column, and inside the pair the larger entry first.  Returns U, the pair order and the
    number of pairs exchanged inside themselves."""
    n = A.shape[0]
    K = np.zeros((2 * n, 2 * n))
    K[0::2, 0::2] = A.real
    K[0::2, 1::2] = -A.imag
    K[1::2, 0::2] = A.imag
    K[1::2, 1::2] = A.real
    perm, nsw = list(range(n)), 0
    for k in range(n):
        i = k + int(np.argmax(np.hypot(K[2 * k::2, 2 * k], K[2 * k + 1::2, 2 * k])))
        if i != k:
            K[[2 * k, 2 * k + 1, 2 * i, 2 * i + 1]] = K[[2 * i, 2 * i + 1, 2 * k, 2 * k + 1]]
            perm[k], perm[i] = perm[i], perm[k]
        if abs(K[2 * k + 1, 2 * k]) > abs(K[2 * k, 2 * k]):
            K[[2 * k, 2 * k + 1]] = K[[2 * k + 1, 2 * k]]
            nsw += 1
        for c in (2 * k, 2 * k + 1):
            K[c + 1:, c:] -= np.outer(K[c + 1:, c] / K[c, c], K[c, c:])
    return K, perm, nsw


def parity(perm):
    seen, cycles = [False] * len(perm), 0
    for i in range(len(perm)):
        if not seen[i]:
            cycles += 1
            j = i
            while not seen[j]:
                seen[j] = True
                j = perm[j]
    return (len(perm) - cycles) & 1


@pytest.mark.parametrize("n", [1, 2, 5, 9, 40])
def test_complex_determinant_fold(n):
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    U, perm, nsw = pair_lu(A)
    if n >= 5:
        assert nsw > 0 and perm != list(range(n))   # both special terms take part
    ang = sum(np.arctan2(-U[2 * k, 2 * k + 1], U[2 * k, 2 * k]) for k in range(n))
    theta = ang + np.pi / 2 * (nsw & 3) + np.pi * parity(perm)
    logabs = 0.5 * np.log(np.abs(np.diag(U))).sum()
    sref, lref = np.linalg.slogdet(A)
    cond = np.linalg.cond(A, 1)
    tol = 8 * n * 2.0 ** -52 * cond
    assert abs(logabs - lref) <= max(tol, 1e-12 * abs(lref))
    assert abs(np.angle(np.exp(1j * theta) / sref)) <= tol


def estimate(solve, solve_h, n, complex_):
    """diag.cpp: eval_ainv with host solves; returns (est, solves)."""
    count = [0]

    def fwd(v):
        count[0] += 1
        return solve(v)

    def adj(v):
        count[0] += 1
        return solve_h(v)

    def sign(y):
        if complex_:
            a = np.abs(y)
            return np.where(a > np.finfo(float).tiny, y / np.where(a > 0, a, 1), 1.0)
        return np.where(y >= 0, 1.0, -1.0)

    dt = complex if complex_ else float
    y = fwd(np.full(n, 1.0 / n, dtype=dt))
    if n == 1:
        return abs(y[0]), count[0]
    est = np.abs(y).sum()
    xi = sign(y)
    z = adj(xi)
    j = int(np.argmax(np.abs(z)))
    for _ in range(2, 6):
        e = np.zeros(n, dtype=dt)
        e[j] = 1
        y = fwd(e)
        s = np.abs(y).sum()
        new = sign(y)
        same = not complex_ and np.array_equal(new, xi)
        grew = s > est
        est = max(est, s)
        xi = new
        if same or not grew:
            break
        z = adj(xi)
        jlast, j = j, int(np.argmax(np.abs(z)))
        if abs(z[jlast]) == np.abs(z).max():
            break
    alt = np.array([(-1.0) ** i * (1 + i / (n - 1)) for i in range(n)], dtype=dt)
    return max(est, 2 * np.abs(fwd(alt)).sum() / (3 * n)), count[0]


CASES = GOLDEN + ["tile_pivoting_700", "helmholtz3d", "complex_fe"]


def dense(name):
    if name == "tile_pivoting_700":
        return tile_pivoting_matrix(700, 5)
    if name == "helmholtz3d":
        return helmholtz3d(8, 0.5).toarray()
    if name == "complex_fe":
        return complex_fe(np.random.default_rng(5), 12).toarray()
    return load_golden(name).toarray()


@pytest.mark.parametrize("name", CASES)
def test_estimate_reaches_the_exact_norm_on_the_gpu_tests_inputs(name):
    Ad = dense(name)
    n = Ad.shape[0]
    z = np.iscomplexobj(Ad)
    lu = sla.lu_factor(Ad)
    inv = np.linalg.inv(Ad)
    for norm, ax in (("1", 0), ("inf", 1)):
        exact = np.abs(inv).sum(axis=ax).max()
        a, b = (lambda v: sla.lu_solve(lu, v)), (lambda v: sla.lu_solve(lu, v, trans=2))
        if norm == "inf":
            a, b = b, a
        est, solves = estimate(a, b, n, z)
        print(f"{name} norm={norm}: est/exact {est / exact:.6f} solves {solves}")
        assert solves <= 11
        assert 0.9 * exact <= est <= exact * (1 + 8 * n * 2.0 ** -52 * np.linalg.cond(Ad, 1))
