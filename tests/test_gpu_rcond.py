"""Reciprocal condition estimate from the device factors (smlu_rcond; F.rcond(), F.condest()).

Reference: the exact ||A^-1|| from numpy.linalg.inv of the dense matrix.  The Hager / Higham
estimate is a lower bound of it up to the rounding of the solves, est <= exact (1 + 8 n 2^-52
cond_1(A)); and est >= 0.9 exact on these inputs, a property of the inputs that
tests/test_diag_derivation.py establishes on the CPU with a NumPy restatement of the estimator
(est / exact = 1.000000 on all of them but random_dominant_200 in the 1-norm, 0.9661).  ||A|| must equal NumPy's to 4 x 2^-52
relative, and rcond == 1 / (anorm ainvnorm) exactly.  LAPACK's dgecon is printed beside each real
case, not asserted: a near-tie in the arg-max may take another path.

The partitioned-handle refusal (nranks > 1) needs two ranks in two processes:
tests/test_gpu_diag_dist.py."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import smlu
from smlu import _lib as C
from smlu import matrices as mats

from _diag_ref import EPS, GOLDEN, load_golden, poisson, rounding
from _parity import tile_pivoting_matrix
from test_gpu_complex import helmholtz3d
from test_oracle import complex_fe

pytestmark = pytest.mark.gpu

NORMS = ["1", "inf"]


def exact_norms(Ad, norm):
    ax = 0 if norm == "1" else 1
    return np.abs(Ad).sum(axis=ax).max(), np.abs(np.linalg.inv(Ad)).sum(axis=ax).max()


def check(F, Ad, norm, what=""):
    n = Ad.shape[0]
    anorm, exact = exact_norms(Ad, norm)
    a1, i1 = exact_norms(Ad, "1")
    r, an, ai = F.rcond(norm, parts=True)
    line = f"{what} n={n} norm={norm}: anorm {an!r} (numpy {anorm!r}) est {ai!r} exact {exact!r} " \
           f"est/exact {ai / exact:.6f} solves {F.stat('rcond_solves'):.0f} iters {F.stat('rcond_iters'):.0f}"
    if not np.iscomplexobj(Ad):
        lu, _, _ = sla.lapack.dgetrf(Ad)
        line += f" dgecon rcond {sla.lapack.dgecon(lu, anorm, norm='1' if norm == '1' else 'I')[0]!r} ours {r!r}"
    print(line)
    assert abs(an - anorm) <= 4 * EPS * anorm, (an, anorm)
    assert r == 1.0 / (an * ai)
    assert ai <= exact * (1.0 + rounding(n, a1 * i1)), (ai, exact)
    assert ai >= 0.9 * exact, (ai, exact)
    assert 1 <= F.stat("rcond_solves") <= 11 and 1 <= F.stat("rcond_iters") <= 5
    assert F.stat("rcond_solves") == F.stat("rcond_solves_fwd") + F.stat("rcond_solves_adj")
    assert F.condest(norm) == an * ai
    return r, an, ai


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("name", GOLDEN)
def test_golden_fixtures(gpu, name, norm):
    A = load_golden(name)
    F = smlu.ParallelSparseLU(A)
    check(F, A.toarray(), norm, name)
    F.close()


@pytest.mark.parametrize("norm", NORMS)
def test_row_exchanges_in_every_tile(gpu, norm):
    D = tile_pivoting_matrix(700, 5)
    F = smlu.ParallelSparseLU(sp.csc_matrix(D))
    check(F, D, norm, "tile_pivoting_matrix(700, 5)")
    F.close()


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("which", ["helmholtz3d", "complex_fe"])
def test_complex(gpu, which, norm):
    A = helmholtz3d(8, 0.5) if which == "helmholtz3d" else complex_fe(np.random.default_rng(5), 12)
    F = smlu.ParallelSparseLU(A)
    check(F, A.toarray(), norm, which)
    F.close()


@pytest.mark.parametrize("kind", ["3d_28", "2d_300"])
def test_large_fronts_and_grid_stride(gpu, kind):
    R = poisson(kind)
    n = R["n"]
    F = smlu.ParallelSparseLU(R["A"])
    if kind == "3d_28":
        assert F.stat("solve_sweeps") > 0   # the handle really has large fronts
    bound = rounding(n, R["anorm1"] * R["inv1"])
    for norm, anorm, exact in (("1", R["anorm1"], R["inv1"]), ("inf", R["anorminf"], R["invinf"])):
        r, an, ai = F.rcond(norm, parts=True)
        print(f"poisson{kind} norm={norm}: anorm {an!r} est {ai!r} exact {exact!r} est/exact {ai / exact:.6f} "
              f"solves {F.stat('rcond_solves'):.0f}")
        assert an == anorm            # sums of small integers are exact
        assert r == 1.0 / (an * ai)
        assert ai <= exact * (1.0 + bound) and ai >= 0.9 * exact, (ai, exact)
        assert F.stat("rcond_solves") <= 11
    F.close()


def test_determinism_and_caching(gpu):
    A = load_golden("random_dominant_200")
    F = smlu.ParallelSparseLU(A)
    got = []
    for _ in range(2):
        F.refactor(A.data)
        got.append((F.rcond("1", parts=True), F.rcond("inf", parts=True)))
        assert F.stat("rcond_solves") > 0
    assert got[0] == got[1]           # two estimates of the same values: bitwise equal
    assert F.rcond("inf", parts=True) == got[1][1]
    assert F.stat("rcond_solves") == 0   # the cached answer runs no solve
    assert F.rcond("1", parts=True) == got[1][0]
    assert F.stat("rcond_solves") == 0
    v = A.data.copy()
    v[mats.diag_positions(A)] *= 3.0
    F.refactor(v)
    r = F.rcond("1")
    assert F.stat("rcond_solves") > 0
    assert r != got[0][0][0]
    an = F.rcond("1", parts=True)[1]
    anorm = abs(sp.csc_matrix((v, A.indices, A.indptr), shape=A.shape)).sum(axis=0).max()
    assert abs(an - anorm) <= 4 * EPS * anorm   # the norm follows the new values too
    F.close()


def test_estimate_uses_the_plain_solves_and_leaves_them_alone(gpu):
    A = load_golden("fe_8")
    n = A.shape[0]
    b = np.random.default_rng(31).random(n)
    est = []
    for refine in (0, 2):
        F = smlu.ParallelSparseLU(A, refine=refine)
        x0, x1 = np.empty(n), np.empty(n)
        smlu.ldiv_(x0, F, b)
        est.append([F.rcond(norm, parts=True) for norm in NORMS])
        assert F.stat("rcond_solves") > 0
        smlu.ldiv_(x1, F, b)
        assert np.array_equal(x0, x1)   # no solve depends on what the estimate left in the work buffers
        F.close()
    assert est[0] == est[1]             # bitwise: the estimator never refines


def test_singular_factorization_is_a_state_error(gpu):
    A = load_golden("poisson2d_16")
    F = smlu.ParallelSparseLU(A)
    assert F.rcond("1") > 0
    A2 = A.tocsr()
    A2.data[A2.indptr[20]:A2.indptr[21]] = 0.0   # row 20 zero (stored zeros: same pattern)
    A2 = A2.tocsc()
    assert A2.nnz == A.nnz
    with pytest.raises(smlu.SingularException):
        F.refactor(A2.data)
    L = C.lib()
    r, a, b = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    for norm in (C.SMLU_NORM_ONE, C.SMLU_NORM_INF):
        assert L.smlu_rcond(F._h, norm, ctypes.byref(r), None, None) == C.SMLU_ERR_STATE
    assert L.smlu_logabsdet(F._h, ctypes.byref(a), ctypes.byref(b)) == C.SMLU_ERR_STATE
    assert L.smlu_rcond(F._h, 3, ctypes.byref(r), None, None) == C.SMLU_ERR_ARG
    F.refactor(A.data)                # a good factorization again
    assert L.smlu_rcond(F._h, C.SMLU_NORM_ONE, ctypes.byref(r), None, None) == C.SMLU_OK and r.value > 0
    F.close()
