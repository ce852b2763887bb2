"""log|det A| and its sign / phase from the device factors (smlu_logabsdet, smlu_logabsdet_z;
F.logabsdet(), F.det(), F.logdet()).

Reference: numpy.linalg.slogdet of the dense matrix.  Tolerance, derived: d log det = tr(A^-1 dA),
so a backward-stable factorization gives |logabs - ref| <= 8 n 2^-52 cond_1(A) (8 as in ctol), with
the floor 1e-12 |ref| for the rounding of the reference and of the sum itself.  The sign is exact;
a complex phase is within the same bound in absolute angle.  Cases: the n = 1, 2 edges and the small
front kernels (golden fixtures), front permutations that are not the identity (tile_pivoting_matrix),
the parities of p0 and q (row exchanges handled by the zero-free-diagonal transversal, three
orderings), several reduction workgroups and large fronts (poisson3d(28)) and the reduction's
grid-stride loop (poisson2d(300)), both against SuperLU's diagonal,
the cache across refactors, and complex handles, one of them with pairs exchanged and moved."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import smlu
from smlu import _lib as C
from smlu import matrices as mats

from _diag_ref import GOLDEN, cond1, load_golden, poisson, rounding
from _parity import tile_pivoting_matrix
from test_gpu_complex import helmholtz3d
from test_oracle import complex_fe

pytestmark = pytest.mark.gpu


def check(F, Ad, what=""):
    """F.logabsdet() against slogdet(Ad) under the derived bound; returns (logabs, sign)."""
    n = Ad.shape[0]
    sref, lref = np.linalg.slogdet(Ad)
    tol = max(rounding(n, cond1(Ad)), 1e-12 * abs(lref))
    la, sg = F.logabsdet()
    print(f"{what} n={n}: logabs {la!r} ref {lref!r} diff {abs(la - lref):.3e} tol {tol:.3e} sign {sg} ref {sref}")
    assert abs(la - lref) <= tol, (la, lref, tol)
    if np.iscomplexobj(Ad):
        assert abs(abs(sg) - 1.0) <= 4 * 2.0 ** -52
        assert abs(np.angle(sg / sref)) <= tol, (sg, sref, tol)
    else:
        assert sg == sref, (sg, sref)
    return la, sg


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_fixtures(gpu, name):
    A = load_golden(name)
    F = smlu.ParallelSparseLU(A)
    la, sg = check(F, A.toarray(), name)
    if name == "fe_5":
        assert sg == -1.0   # the fixture with a negative determinant
        with pytest.raises(ValueError):
            F.logdet()
    if sg > 0:
        assert F.logdet() == la
    d = F.det()
    assert d == sg * np.exp(la)
    F.close()


def test_front_permutations_not_the_identity(gpu):
    D = tile_pivoting_matrix(700, 5)
    sref, lref = np.linalg.slogdet(D)
    assert sref == -1.0 and abs(lref - 4836.845) < 1e-3   # the fixture itself
    F = smlu.ParallelSparseLU(sp.csc_matrix(D))
    # identity front permutations could not pass for the wrong reason
    assert not np.array_equal(F.p, F.fronts()["p0"])
    la, sg = check(F, D, "tile_pivoting_matrix(700, 5)")
    assert sg == -1.0
    F.close()


def test_row_permutations_flip_the_sign(gpu):
    A = load_golden("random_dominant_200").toarray()
    F = smlu.ParallelSparseLU(sp.csc_matrix(A))
    la0, sg0 = check(F, A, "random_dominant_200")
    F.close()
    assert sg0 == 1.0
    swap = np.arange(200)
    swap[[17, 130]] = swap[[130, 17]]
    cyc = np.arange(200)
    cyc[[5, 60, 171]] = cyc[[60, 171, 5]]
    out = []
    for perm, want in ((swap, -1.0), (cyc, 1.0)):
        B = A[perm]
        F = smlu.ParallelSparseLU(sp.csc_matrix(B))
        la, sg = check(F, B, "rows permuted")
        assert sg == want
        out.append(la)
        F.close()
    tol = 2 * max(rounding(200, cond1(A)), 1e-12 * abs(la0))
    assert abs(out[0] - la0) <= tol and abs(out[1] - la0) <= tol, (out, la0)


def test_orderings_agree(gpu):
    A = load_golden("fe_8")
    Ad = A.toarray()
    res = []
    for ordering in ("natural", "amd", "auto"):
        F = smlu.ParallelSparseLU(A, ordering=ordering)
        res.append(check(F, Ad, f"fe_8 ordering={ordering}"))
        F.close()
    assert len({sg for _, sg in res}) == 1


@pytest.mark.parametrize("kind", ["3d_28", "2d_300"])
def test_large_fronts_and_grid_stride(gpu, kind):
    R = poisson(kind)
    F = smlu.ParallelSparseLU(R["A"])
    if kind == "3d_28":
        assert F.stat("solve_sweeps") > 0   # the handle really has large fronts
    else:
        assert R["n"] > 256 * 256           # every reduction thread takes more than one index
    la, sg = F.logabsdet()
    tol = max(rounding(R["n"], R["anorm1"] * R["inv1"]), 1e-12 * abs(R["logabs"]))
    print(f"poisson{kind}: logabs {la!r} splu {R['logabs']!r} diff {abs(la - R['logabs']):.3e} tol {tol:.3e}")
    assert sg == 1.0   # SPD
    assert abs(la - R["logabs"]) <= tol
    F.close()


def test_refactor_invalidates_the_cache(gpu):
    A = load_golden("poisson2d_16")
    F = smlu.ParallelSparseLU(A)
    la0, _ = check(F, A.toarray(), "poisson2d_16")
    assert F.stat("logabsdet_evals") == 1
    assert F.logabsdet()[0] == la0
    assert F.stat("logabsdet_evals") == 1   # the cached answer
    rng = np.random.default_rng(21)
    A2 = A.copy()
    A2.data = A.data * (1.0 + 0.5 * rng.random(A.nnz))
    A2.data[mats.diag_positions(A)[3]] *= -1.0   # same pattern, other values
    F.refactor(A2.data)
    la1, sg1 = check(F, A2.toarray(), "poisson2d_16 refactored")
    assert la1 != la0
    assert F.stat("logabsdet_evals") == 2
    F.refactor(A2.data)                     # the same values again: a second evaluation, bitwise the first
    la2, sg2 = F.logabsdet()
    assert F.stat("logabsdet_evals") == 3
    assert la2 == la1 and sg2 == sg1
    F.close()


@pytest.mark.parametrize("which", ["helmholtz3d", "complex_fe"])
def test_complex(gpu, which):
    A = helmholtz3d(8, 0.5) if which == "helmholtz3d" else complex_fe(np.random.default_rng(5), 12)
    F = smlu.ParallelSparseLU(A)
    la, sg = check(F, A.toarray(), which)
    assert isinstance(sg, complex)
    assert F.logdet() == complex(la, np.angle(sg))
    # the real entry point refuses a complex handle
    a, b = ctypes.c_double(), ctypes.c_double()
    assert C.lib().smlu_logabsdet(F._h, ctypes.byref(a), ctypes.byref(b)) == C.SMLU_ERR_STATE
    F.close()


def test_complex_pairs_exchanged_and_moved(gpu):
    """The two special terms of the complex fold take part: tiny diagonals make the fronts pivot off
    the diagonal (a non-identity permutation of pairs), and random phases put many pivots' larger
    part in the imaginary slot (the pair exchanged inside itself, a factor i each)."""
    rng = np.random.default_rng(7)
    A = tile_pivoting_matrix(150, 7) * np.exp(2j * np.pi * rng.random((150, 150)))
    F = smlu.ParallelSparseLU(sp.csc_matrix(A))
    assert F.stat("cpair") == 1
    pk = F.real_equivalent_factors()["p"]
    p0 = F.fronts()["p0"]
    reversed_pairs = int((pk[0::2] > pk[1::2]).sum())
    assert reversed_pairs > 0
    assert not np.array_equal(F.p, p0[0::2] // 2)
    la, sg = check(F, A, f"complex tile pivoting, {reversed_pairs} pairs reversed")
    F.close()


def test_real_handle_refuses_the_complex_entry_point(gpu):
    F = smlu.ParallelSparseLU(load_golden("dense_13"))
    a = ctypes.c_double()
    ph = (ctypes.c_double * 2)()
    assert C.lib().smlu_logabsdet_z(F._h, ctypes.byref(a), ph) == C.SMLU_ERR_STATE
    F.close()
