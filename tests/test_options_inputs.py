"""The inputs of test_gpu_options.py, checked without a GPU (as test_front_shapes.py does for
test_gpu_front_shapes.py): conditions on the inputs, decided by the symbolic analysis (smlu.Plan)
and the CPU oracle alone, none of them by the library computing right numbers.

* scale=False twins: B = diag(rowscale(A)) A takes the same pivoting mode as A (O.dominant agrees for
  all five), and rowscale(B) is not exactly one, so only a scale=False handle of B is A's twin.
* pivot_tol: the oracle's own re-pivoting decision on tile_pivoting_matrix(1100, 1111) flips between
  0.1 and 0.6; by bisection it flips at pivot_tol = 0.28906, i.e. the largest multiplier in a row
  outside the diagonal tile is 3.4595.  And _weak_tile_matrix(700, 21) is re-pivoted at 0.1 but not
  at pivot_tol = 0.
* use_mfma=False: the host plans of its four inputs hold diagonal-tile fronts (mode 2).
* leaf_size 16 and 256 give other supernode partitions than the default 64."""
import numpy as np
import pytest

import oracle as O
import smlu

import _options_inputs as I
from _parity import tile_pivoting_matrix


@pytest.mark.parametrize("name", list(I.NO_SCALE))
def test_row_scaled_twin_keeps_the_pivoting_mode(name):
    A = I.matrix("no_scale", name)
    B, r = I.row_scaled_twin(A)
    want = I.NO_SCALE[name][2]
    assert O.dominant(A) == want and O.dominant(B) == want
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    # scaling the twin again would not be a no-op: rowscale(B) is one only to rounding
    rb = O.rowscale(B)
    assert not np.array_equal(rb, np.ones(A.shape[0])) and np.allclose(rb, 1.0, rtol=1e-14, atol=0)


def _decision(A, q, fr, **kw):
    p, pm, modes, flags = O.gpu_pivot_choice(A, q, fr, threads=4, **kw)
    return pm, modes


def test_pivot_tol_pair_flips_the_oracles_decision():
    A = I.csc(tile_pivoting_matrix(*I.FLIP_SEED))
    q, fr = I.plan_fronts(A)
    assert not O.dominant(A)
    loose, strict = I.FLIP_TOLS
    pm, modes = _decision(A, q, fr, pivot_tol=loose)
    assert pm == 0 and (modes == 2).any()
    pm, modes = _decision(A, q, fr, pivot_tol=strict)
    assert pm == 1 and not (modes == 2).any()
    # the growth that separates them, with a factor 1.5 to spare on either side: what the GPU's
    # growth epilogues compute in another order cannot land on the other side of either tolerance
    for tol, want in ((1 / (1.5 * 3.4595), 0), (1.5 / 3.4595, 1), (1 / 3.46, 0), (1 / 3.459, 1)):
        assert _decision(A, q, fr, pivot_tol=tol)[0] == want, tol
    assert 1 / loose > 1.5 * 3.4595 and 1 / strict < 3.4595 / 1.5


def test_weak_tile_matrix_is_repivoted_unless_pivot_tol_is_zero():
    A = I.csc(I.weak_tile_matrix(700, 21))
    q, fr = I.plan_fronts(A)
    assert _decision(A, q, fr, pivot_tol=0.1, diag_tol=0.1)[0] == 1
    pm, modes = _decision(A, q, fr, pivot_tol=0.0, diag_tol=0.1)
    assert pm == 0 and (modes == 2).any()


@pytest.mark.parametrize("name", list(I.NO_MFMA))
def test_no_mfma_inputs_hold_diagonal_tile_fronts(name):
    A = I.matrix("no_mfma", name)
    q, fr = I.plan_fronts(A)
    modes = O.front_modes(fr, 0, O.dominant(A))
    ns = np.diff(fr["first"])
    assert (modes == 2).any()
    assert ns[modes == 2].max() > 64          # more than one 64-wide panel in a tile front
    assert O.dominant(A) == (name != "tile_pivoting_1100")


def test_weak_and_dominant_700_share_a_pattern_and_a_tile_front():
    """The refactor replay puts the weak-tile values on the handle of the dominant ones and back."""
    D, W = I.csc(I.dominant_dense(700, 41)), I.csc(I.weak_tile_matrix(700, 42))
    assert np.array_equal(D.indptr, W.indptr) and np.array_equal(D.indices, W.indices)
    assert O.dominant(D) and not O.dominant(W)
    q, fr = I.plan_fronts(D)
    assert (O.front_modes(fr, 0, True) == 2).all() and (O.front_modes(fr, 0, False) == 2).all()
    assert _decision(W, q, fr, pivot_tol=0.1, diag_tol=0.1)[0] == 1
    assert _decision(D, q, fr, pivot_tol=0.1, diag_tol=0.1, pivmode=1)[0] == 0


@pytest.mark.parametrize("name", list(I.LEAF))
def test_leaf_sizes_give_other_trees(name):
    A = I.LEAF[name]()
    base = smlu.Plan(A, ordering="nd").stat("nsuper")
    got = [smlu.Plan(A, ordering="nd", leaf_size=ls).stat("nsuper") for ls in I.LEAF_SIZES]
    assert base not in got and got[0] != got[1], (base, got)
