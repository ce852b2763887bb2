"""The inputs of test_gpu_front_shapes.py, checked without a GPU: the matrices of _front_shapes.py
give exactly the fronts they are meant to give, the fronts stand on both sides of every kernel-class
threshold their set can reach, and the CPU oracle alone pivots in them as the GPU tests assume
(rows moved in every front of the pivot and tile sets, no re-pivoting, nothing moved under dominant
values).  These are conditions on the inputs: none depends on the library computing right numbers,
only on its symbolic analysis (smlu.Plan) and on the oracle."""
import functools

import numpy as np
import pytest

import oracle as O
import smlu

import _front_shapes as S

REAL = [name for name in S.SETS if not name.startswith("complex")]


@functools.lru_cache(maxsize=None)
def planned(name):
    """(A or its real-equivalent K, q, the plan's fronts as a dict) of a set."""
    A = S.set_matrix(name)
    K = O.real_equivalent(A) if name.startswith("complex") else A
    P = smlu.Plan(K, ordering="natural", relax=False)
    first, parent, rowptr, rows, p0 = P.fronts()
    return K, P.q(), dict(first=first, parent=parent, rowptr=rowptr, rows=rows, p0=p0)


@functools.lru_cache(maxsize=None)
def oracle_choice(name):
    """The oracle's own pivots on the plan's fronts: (p, pivmode, modes, front moved a row?)."""
    K, q, fr = planned(name)
    kw = S.HANDLE_KW.get(name, {})
    p, pm, modes, _ = O.gpu_pivot_choice(K, q, fr, diag_tol=kw.get("diag_pivot_tol", 0.001), threads=4)
    moved = p != fr["p0"]
    first = fr["first"]
    return p, pm, modes, [bool(moved[first[s]:first[s + 1]].any()) for s in range(first.size - 1)]


# ---- the class rules against cases worked by hand ------------------------------------------------
@pytest.mark.parametrize("ns, nu, mode, factor, solve", [
    (1, 7, 0, ("lds", 16), "micro"), (8, 1, 0, ("lds", 16), "tiny"), (16, 0, 0, ("lds", 16), "tiny"),
    (1, 16, 0, ("lds", 32), "tiny"), (33, 15, 0, ("lds", 48), "tiny"), (49, 0, 0, ("lds", 64), "tiny"),
    (64, 0, 0, ("lds", 64), "tiny"), (65, 0, 0, ("lds", 96), "small"), (1, 96, 0, ("lds", 128), "tiny"),
    (64, 64, 0, ("lds", 128), "tiny"), (65, 63, 0, ("lds", 128), "small"), (128, 0, 0, ("lds", 128), "small"),
    (64, 65, 1, ("blocked", 1), "small"), (1, 128, 2, ("blocked", 2), "small"), (128, 384, 1, ("blocked", 1), "small"),
    (128, 385, 2, ("blocked", 2), "big"), (256, 0, 1, ("blocked", 1), "small"), (256, 1, 1, ("blocked", 1), "big"),
    (257, 0, 2, ("blocked", 2), "big"), (513, 33, 2, ("blocked", 2), "big"),
])
def test_classify_by_hand(ns, nu, mode, factor, solve):
    c = S.classify(ns, nu, mode)
    assert (c["factor"], c["solve"]) == (factor, solve)


def test_panel_classes_by_hand():
    assert S.classify(64, 65, 1)["panels"] == (64, 64)
    assert S.classify(65, 64, 1)["panels"] == (128, 64, 64)
    assert S.classify(257, 1, 1)["panels"] == (512, 256, 256, 256, 256, 128, 128, 64, 64)
    assert S.classify(577, 130, 1)["panels"][:4] == ("more", "more", "more", 512)
    assert S.classify(577, 130, 2)["panels"] == ("tile",) * 10
    assert S.expected_mode(64, 64, "pivot") == 0 and S.expected_mode(64, 65, "pivot") == 1
    assert S.expected_mode(512, 0, "pivot") == 1 and S.expected_mode(513, 0, "pivot") == 2
    assert S.expected_mode(129, 0, "dominant") == 2 and S.expected_mode(600, 20, "complex") == 1


# ---- the plan gives the prescribed fronts ---------------------------------------------------------
@pytest.mark.parametrize("name", list(S.SETS))
def test_plan_gives_the_prescribed_fronts(name):
    K, q, fr = planned(name)
    got = list(zip(np.diff(fr["first"]).tolist(), np.diff(fr["rowptr"]).tolist()))
    want = [(ns, nu) for ns, nu, _ in S.set_fronts(name)]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    assert np.array_equal(q, np.arange(K.shape[0]))
    assert np.array_equal(fr["p0"], np.arange(K.shape[0]))   # no row matching ahead of the analysis
    n = S.set_matrix(name).shape[0]
    assert 1500 <= n <= 7500 or name == "repivot", n


def test_component_is_two_leaves_under_a_border():
    C = S.component(3, 2, np.random.default_rng(0), "pivot").toarray()
    assert C.shape == (8, 8)
    assert (C[:3, 3:6] == 0).all() and (C[3:6, :3] == 0).all()   # the leaves are not coupled
    C[:3, 3:6] = C[3:6, :3] = 1.0
    assert (C != 0).all()                                        # everything else is
    D = S.component(5, 0, np.random.default_rng(0), "dominant").toarray()
    assert D.shape == (5, 5) and (abs(D).sum(axis=1) < 2 * D.diagonal()).all()
    rows = S.component_rows([(3, 2), (5, 0), (1, 1)])
    assert rows == [((3, 2), 0, 8), ((5, 0), 8, 13), ((1, 1), 13, 16)]
    assert S.expected_fronts([(3, 2), (5, 0), (1, 1)]) == [(3, 2), (5, 0), (5, 0), (1, 1), (2, 0)]
    assert S.front_components([(3, 2), (5, 0), (1, 1)]) == [(3, 2), (3, 2), (5, 0), (1, 1), (1, 1)]


# ---- coverage: a front on each side of every threshold the set can reach ---------------------------
@pytest.mark.parametrize("name", list(S.SETS))
def test_every_threshold_has_a_front_on_each_side(name):
    names = S.set_thresholds(name)
    assert names
    assert S.uncovered(S.set_fronts(name), names) == []


@pytest.mark.parametrize("name, shape, lost", [
    ("small-pivot", (65, 63), "tiny|small by ns: upper side"),
    ("small-dominant", (1, 127), "extremes (1, M-1), (M-1, 1), (M, 0) at M = 128: lower side"),
    ("blocked-pivot", (256, 1), "small|big by work at ns 256: upper side"),
    ("blocked-dominant", (128, 385), "small|big by work at ns 128: upper side"),
    ("blocked-pivot", (384, 65), "outer block 383|384: upper side"),
    ("tile", (513, 33), "mode 2 at ns = 513 over a contribution block: lower side"),
    ("complex-pivot", (16, 17), "M 64|66: upper side"),
])
def test_coverage_check_notices_a_removed_shape(name, shape, lost):
    shapes, kind, _, values, _ = S.SETS[name]
    k = 2 if kind.startswith("complex") else 1
    left = [s for s in shapes if s != shape]
    assert len(left) == len(shapes) - 1
    fronts = [(k * ns, k * nu, S.expected_mode(k * ns, k * nu, values)) for ns, nu in S.expected_fronts(left)]
    assert lost in S.uncovered(fronts, S.set_thresholds(name))


def test_every_threshold_is_asked_of_some_set():
    asked = set()
    for name in S.SETS:
        asked.update(S.set_thresholds(name))
    assert asked == set(S.thresholds())


# ---- what the oracle alone does with these values -------------------------------------------------
@pytest.mark.parametrize("name", REAL)
def test_oracle_modes_are_the_restated_ones(name):
    K, q, fr = planned(name)
    p, pm, modes, moved = oracle_choice(name)
    assert modes.tolist() == [m for _, _, m in S.set_fronts(name)]
    assert pm == (1 if name == "repivot" else 0)


@pytest.mark.parametrize("name", ["small-pivot", "blocked-pivot"])
def test_pivot_sets_move_a_row_in_every_front(name):
    p, pm, modes, moved = oracle_choice(name)
    assert pm == 0 and not (modes == 2).any()
    still = [(ns, nu) for (ns, nu, _), mv in zip(S.set_fronts(name), moved) if ns >= 2 and not mv]
    assert still == []
    assert not any(mv for (ns, nu, _), mv in zip(S.set_fronts(name), moved) if ns == 1)   # nothing to move to


def test_tile_set_stays_on_the_diagonal_tiles_and_moves_rows():
    p, pm, modes, moved = oracle_choice("tile")
    assert pm == 0
    assert all(m == 2 for (ns, nu, _), m in zip(S.set_fronts("tile"), modes) if ns > 512)
    assert (modes == 2).all() and all(moved)


def test_repivot_set_is_repivoted():
    p, pm, modes, moved = oracle_choice("repivot")
    assert pm == 1 and (modes == 1).all() and all(moved)


@pytest.mark.parametrize("name", ["small-dominant", "blocked-dominant"])
def test_dominant_sets_move_nothing(name):
    K, q, fr = planned(name)
    assert O.dominant(K)
    p, pm, modes, moved = oracle_choice(name)
    assert pm == 0 and not any(moved) and np.array_equal(p, fr["p0"])


def test_pivot_and_dominant_blocked_values_share_a_pattern():
    """The refactor replay of the GPU tests puts dominant values on the blocked-pivot handle."""
    A = S.set_matrix("blocked-pivot")
    D = S.shape_matrix(S.BLOCKED_PIVOT, "dominant", 3)
    assert np.array_equal(A.indptr, D.indptr) and np.array_equal(A.indices, D.indices)
    assert O.dominant(D) and not O.dominant(A)
