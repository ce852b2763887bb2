"""The checker of the batched-solve tests proved on the CPU (tests/_batch_ref.py): scipy's SuperLU
stands in for the GPU on the golden fixtures.  SuperLU factors (Rs .* A) with its own threshold
pivoting; its row and column orders, its factors and the row scaling are handed to the checker as a
handle would hand them (F.p, F.q, F.Rs, F.L, F.U), so the oracle solves on the stand-in's pivot
order exactly as it does on the GPU's.  A correct batch passes; a batch with two columns swapped,
one with a single entry moved by 1e-9 relative, and a transposed batch whose column 3 was solved
with the untransposed matrix all fail."""
import functools
import glob
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle as O

from _batch_ref import FLOOR, assert_batch_against_oracle, berr, oracle_columns
from _diag_ref import HERE, load_golden

NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(HERE, "golden", "*.npz")))
NRHS = 5


class StandIn:
    """SuperLU of (Rs .* A) dressed as a handle: L U = (Rs .* A)[p, q], 0-based new -> old orders."""

    def __init__(self, A):
        A = sp.csc_matrix(A)
        self.n = A.shape[0]
        self.is_complex = False
        self.Rs = O.rowscale(A)
        self.lu = spla.splu(sp.csc_matrix(sp.diags(self.Rs) @ A))
        self.p = np.argsort(self.lu.perm_r)
        self.q = np.argsort(self.lu.perm_c)
        self.L, self.U = sp.csc_matrix(self.lu.L), sp.csc_matrix(self.lu.U)

    def solve(self, B, trans="N"):
        """The stand-in's batch: (nrhs, n) in, (nrhs, n) out."""
        if trans == "N":
            return np.stack([self.lu.solve(self.Rs * b) for b in B])
        return np.stack([self.Rs * self.lu.solve(b, trans="T") for b in B])


@functools.lru_cache(maxsize=None)
def _case(name):
    A = load_golden(name)
    F = StandIn(A)
    B = np.random.default_rng(90).random((NRHS, F.n))
    return types.SimpleNamespace(name=name, A=A, F=F, B=B, X=F.solve(B), Xt=F.solve(B, "T"))


def _unsymmetric(name):
    A = load_golden(name)
    return abs(A - A.T).max() > 0


UNSYMMETRIC = [name for name in NAMES if _unsymmetric(name)]   # where A^T x = b is another system


@pytest.fixture(params=NAMES)
def case(request):
    return _case(request.param)


def test_stand_in_relation(case):
    """The stand-in really is L U = (Rs .* A)[p, q]: what the oracle is told is true."""
    F = case.F
    S = (sp.diags(F.Rs) @ case.A).tocsr()[F.p][:, F.q]
    assert abs(F.L @ F.U - S).max() <= 1e-13 * max(abs(S).max(), 1e-300)


def test_berr_by_hand():
    """[[2, -1], [0, 4]] x = b with x = (1, 1): residual (0.5, 0) against b = (1.5, 4) over
    denominators (4.5, 8); the zero row is skipped; complex entries count by their moduli."""
    A = sp.csr_matrix(np.array([[2.0, -1.0], [0.0, 4.0]]))
    assert berr(A, np.ones(2), np.array([1.5, 4.0])) == pytest.approx(0.5 / 4.5, rel=1e-15)
    Z = sp.csr_matrix(np.array([[2.0, -1.0], [0.0, 0.0]]))
    assert berr(Z, np.ones(2), np.array([1.0, 0.0])) == 0.0
    Ac = sp.csr_matrix(np.array([[3.0 + 4.0j]]))
    assert berr(Ac, np.array([1.0j]), np.array([-4.0 + 2.0j])) == pytest.approx(1.0 / (5.0 + np.hypot(4, 2)), rel=1e-15)
    # extended precision: a residual below one ulp of the fp64 products is still seen
    assert 0.0 < berr(sp.csr_matrix(np.array([[1.0]])), np.array([1.0 + 2.0 ** -52]), np.array([1.0])) < 2.0 ** -52


def test_correct_batch_passes(case):
    assert_batch_against_oracle(case.A, case.F, case.B, case.X, "N", label=case.name)
    assert_batch_against_oracle(case.A, case.F, case.B, case.Xt, "T", label=case.name)


def test_oracle_columns_solve_the_system(case):
    """Substitution on SuperLU's threshold-pivoted factors is backward stable: a few n unit roundoffs
    at n <= 200 is under 64 * 2^-51 = 2.8e-14 (measured: at most 9.1e-15), and a solve of the wrong
    system is of order one."""
    for trans, Op in (("N", case.A), ("T", case.A.T)):
        Xo = oracle_columns(case.A, case.F, case.B, trans)
        for j in range(NRHS):
            assert berr(Op, Xo[j], case.B[j]) <= 64 * FLOOR


def test_swapped_columns_fail(case):
    for trans, X in (("N", case.X), ("T", case.Xt)):
        Xs = X.copy()
        Xs[[1, 3]] = X[[3, 1]]
        with pytest.raises(AssertionError):
            assert_batch_against_oracle(case.A, case.F, case.B, Xs, trans)


def test_one_entry_moved_fails(case):
    for trans, X in (("N", case.X), ("T", case.Xt)):
        Xm = X.copy()
        i = int(np.argmax(np.abs(X[2])))
        Xm[2, i] *= 1.0 + 1e-9
        with pytest.raises(AssertionError, match="column 2"):
            assert_batch_against_oracle(case.A, case.F, case.B, Xm, trans)


@pytest.mark.parametrize("name", UNSYMMETRIC)
def test_untransposed_column_fails_the_transposed_check(name):
    case = _case(name)
    Xm = case.Xt.copy()
    Xm[3] = case.X[3]
    with pytest.raises(AssertionError, match="column 3"):
        assert_batch_against_oracle(case.A, case.F, case.B, Xm, "T")
