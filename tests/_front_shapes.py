"""Matrices whose fronts have prescribed shapes, and a restatement of the rules that choose a front's
kernels.  Shared by test_front_shapes.py (CPU) and test_gpu_front_shapes.py.  No GPU needed.

A front has ns pivots and nu contribution rows, M = ns + nu.  With ordering="natural" and
relax=False a block-diagonal matrix of "two leaves under a border" components has exactly the fronts
one asks for: leaves [0, ns) and [ns, 2 ns) are dense, both are coupled densely (rows and columns) to
a dense border of nu columns, and the leaves are not coupled to each other.  The first leaf is the
front (ns, nu); the second leaf joins the border's supernode, the dense root (ns + nu, 0) with the
first leaf as the child it extend-adds.  nu = 0 gives one dense block, the front (ns, 0).  The
components are built as sparse matrices (no stored zeros between the leaves, which would make each
component one dense front) and every diagonal entry is nonzero (no row matching ahead of the
analysis).

The class rules (classify) are written from the table of thresholds, not imported from the library:

    LDS size class of a front factored whole      M <= 16 / 32 / 48 / 64 / 96 / 128
    LDS front against blocked front               M <= 128
    candidate mode of a blocked front             ns <= 512: 1 (panels of 32, every fully-summed row),
                                                  otherwise 2 (64 x 64 diagonal tile); dominant values: 2
                                                  for every blocked front; complex handles and a
                                                  re-pivoted handle: 1 for every blocked front
    mode-1 panel class of a step                  candidate rows R = ns - 32 t <= 64 / 128 / 256 / 512 / more
    panel width and outer block                   ns mod 32, ns mod 64, ns around 384
    solve class                                   micro M <= 8; tiny M <= 128 and ns <= 64;
                                                  big ns > 256 or ns M > 65 536; small the rest
    inside the small-front and tiny kernels       F22 on 16 x 16 x 4 tiles (nu mod 16, ns mod 4), U12 64
                                                  columns at a time, lane i owns rows i and i + 64

The sets, their components and the fronts they give, counted by class (classify):

    small    67 components, n = 5 726, values "dominant" and "pivot": M on both sides of 8|9, 16|17, 32|33,
             48|49, 64|65, 96|97 and at 127 and 128, each as (1, M-1), (M-1, 1), (M, 0) and as splits with nu in
             {1, 15, 16, 17, 63, 64, 65, 127} and ns in {1, 3, 4, 5, 63, 64, 65}; tiny|small solves at (64, 64) |
             (65, 63).  120 LDS fronts, 21 / 16 / 16 / 16 / 18 / 33 in the size classes 16 / 32 / 48 / 64 / 96 /
             128; solves 7 micro, 80 tiny, 33 small.
    blocked  values "pivot": 17 components, n = 7 500, every ns + nu <= 512 so that no front is in mode 2
             (the root (ns + nu, 0) of a larger one would be, and random values are re-pivoted there):
             (64, 64) | (64, 65), (65, 64), (1, 128), (128, 1), (129, 0), (127, 2), (97, 32), (128, 384), (256, 0) |
             (256, 1) | (257, 1), (383 | 384 | 385, 65), (479, 30), (512, 0); ns mod 64 in {1, 31, 33, 63}.  2 LDS
             and 29 blocked fronts, all in mode 1, with steps in the panel classes 64 / 128 / 256 / 512 in
             29 / 27 / 22 / 13 of them; solves 1 tiny, 16 small, 14 big.
             values "dominant": 17 components, n = 6 865: without (479, 30) and (512, 0), with (95, 34) and
             with (128, 385), the other side of ns M = 65 536 at ns = 128.  2 LDS and 30 blocked fronts, all
             in mode 2; solves 1 tiny, 18 small, 13 big.
    tile     (513, 33), (576, 64), (640, 0), n = 2 915, tile_pivoting_matrix values: 5 blocked fronts in mode
             2 with rows moved in every one, all big solves.
    repivot  (577, 130), n = 1 284, the same values: the oracle finds weak tile pivots in its root, so the
             handle is re-pivoted: 2 blocked fronts in mode 1 whose first steps have more than 512
             candidate rows (panel class "more").
    complex  23 components, n = 1 642 (3 284 real), values "complex" and "complex_pivot": real-equivalent
             fronts (2 ns, 2 nu) with M on both sides of 8|10, 16|18, 32|34, 48|50, 64|66, 96|98, 128|130;
             (100, 40) and (300, 10) give blocked fronts, in mode 1 as on every complex handle, the
             second with more than 512 candidate rows.  35 LDS fronts (11 / 5 / 4 / 6 / 4 / 5 by size
             class) and 7 blocked ones; solves 4 micro, 26 tiny, 9 small, 3 big.

Seeds: those for which the oracle alone does what the GPU tests assume (test_front_shapes.py): under
partial pivoting a front of three pivots keeps its diagonal with probability 1/6, so some seeds leave
a front of the small set unmoved (0 .. 4 do, 5 does not); seed 0 of the tile set has a weak tile pivot
in (513, 33) and would be re-pivoted, seed 1 has none.
"""
import numpy as np
import scipy.sparse as sp

from _parity import tile_pivoting_matrix

SMALL_M = 128
FULL_PIV_NS = 512
LDS_CLASSES = (16, 32, 48, 64, 96, 128)
PANEL_CLASSES = (64, 128, 256, 512)
NB = {1: 32, 2: 64}
MICRO_M, TINY_M, TINY_NS = 8, 128, 64
BIG_NS, BIG_WORK = 256, 65536


# ---- the matrices ---------------------------------------------------------------------------------
def _tile_block(k, rng, below):
    """tile_pivoting_matrix(k): tiny diagonal entries, so rows are exchanged inside every 64 x 64
    diagonal tile.  A last tile of a single row (k mod 64 = 1) has no row to exchange with; over a
    contribution block (`below`) its tiny diagonal would be a weak pivot and the whole handle would
    be re-pivoted, so there that one entry takes a value of the tiles' size."""
    D = tile_pivoting_matrix(k, int(rng.integers(1 << 30)))
    if below and k % 64 == 1:
        D[-1, -1] = k * (0.5 + 0.5 * rng.random())
    return D


def component(ns, nu, rng, kind):
    """One component as a sparse matrix of order 2 ns + nu (ns when nu = 0): fronts (ns, nu) and
    (ns + nu, 0).  kind: "dominant" (random values plus order x I), "pivot" (random values), "tile"
    (leaf pivot block and root block from tile_pivoting_matrix), "complex" / "complex_pivot" (the
    dominant / pivot values times random phases)."""
    base = {"complex": "dominant", "complex_pivot": "pivot"}.get(kind, kind)
    m = 2 * ns + nu if nu else ns
    if base == "tile":
        leaf = _tile_block(ns, rng, below=nu > 0)
        root = _tile_block(ns + nu, rng, below=False) if nu else None
    elif base in ("dominant", "pivot"):
        leaf = rng.random((ns, ns))
        root = rng.random((ns + nu, ns + nu)) if nu else None
    else:
        raise ValueError(kind)
    if nu == 0:
        D = leaf
        blocks = [[sp.csc_matrix(D)]]
    else:
        up = rng.random((ns, nu))      # first leaf's rows in the border's columns (its U12)
        left = rng.random((nu, ns))    # the border's rows in the first leaf's columns (its L21)
        blocks = [[sp.csc_matrix(leaf), None, sp.csc_matrix(up)],
                  [None, sp.csc_matrix(root[:ns, :ns]), sp.csc_matrix(root[:ns, ns:])],
                  [sp.csc_matrix(left), sp.csc_matrix(root[ns:, :ns]), sp.csc_matrix(root[ns:, ns:])]]
    C = sp.csc_matrix(sp.bmat(blocks, format="csc"))
    if base == "dominant":
        C = C + m * sp.identity(m, format="csc")
    C = sp.csc_matrix(C)
    if kind.startswith("complex"):
        C = C.astype(np.complex128)
        C.data = C.data * np.exp(2j * np.pi * rng.random(C.nnz))
    C.eliminate_zeros()
    C.sort_indices()
    return C


def shape_matrix(shapes, kind, seed):
    """Block-diagonal matrix of component(ns, nu) for every (ns, nu) of shapes, in that order."""
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix(sp.block_diag([component(ns, nu, rng, kind) for ns, nu in shapes], format="csc"))
    A.sort_indices()
    assert A.nnz == sum((2 * ns * ns + nu * nu + 4 * ns * nu) if nu else ns * ns for ns, nu in shapes)
    assert (A.diagonal() != 0).all()
    return A


def expected_fronts(shapes):
    """The (ns, nu) list the plan must produce, front for front."""
    out = []
    for ns, nu in shapes:
        out.append((ns, nu))
        if nu:
            out.append((ns + nu, 0))
    return out


def component_rows(shapes):
    """[(ns, nu), first row, one past the last row] per component of shape_matrix(shapes)."""
    out, r = [], 0
    for ns, nu in shapes:
        m = 2 * ns + nu if nu else ns
        out.append(((ns, nu), r, r + m))
        r += m
    return out


def front_components(shapes):
    """Per front of expected_fronts(shapes): the (ns, nu) of the component it belongs to."""
    out = []
    for ns, nu in shapes:
        out += [(ns, nu)] * (2 if nu else 1)
    return out


# ---- the class rules, restated --------------------------------------------------------------------
def expected_mode(ns, nu, values):
    """Candidate mode of a front under values "dominant", "pivot" (not dominant, never re-pivoted),
    "repivoted" or "complex"."""
    if ns + nu <= SMALL_M:
        return 0
    if values == "dominant":
        return 2
    if values in ("complex", "repivoted"):
        return 1
    assert values == "pivot", values
    return 1 if ns <= FULL_PIV_NS else 2


def classify(ns, nu, mode):
    """dict(factor=..., solve=..., panels=...) of a front.  factor: ("lds", size class) or
    ("blocked", mode); panels: the panel class of every step of a blocked front ("tile" in mode 2, the
    bound on the candidate rows -- 64, 128, 256, 512 or "more" -- in mode 1), () for an LDS front;
    solve: "micro", "tiny", "small" or "big"."""
    M = ns + nu
    if mode == 0:
        assert M <= SMALL_M, (ns, nu, mode)
        factor = ("lds", next(c for c in LDS_CLASSES if M <= c))
        panels = ()
    else:
        assert M > SMALL_M, (ns, nu, mode)
        factor = ("blocked", mode)
        nb = NB[mode]
        steps = -(-ns // nb)
        if mode == 2:
            panels = ("tile",) * steps
        else:
            panels = tuple(next((c for c in PANEL_CLASSES if ns - t * nb <= c), "more") for t in range(steps))
    if ns > BIG_NS or ns * M > BIG_WORK:
        solve = "big"
    elif M <= TINY_M and ns <= TINY_NS:
        solve = "micro" if M <= MICRO_M else "tiny"
    else:
        solve = "small"
    return dict(factor=factor, solve=solve, panels=panels)


def describe(ns, nu, mode):
    c = classify(ns, nu, mode)
    f = f"LDS class {c['factor'][1]}" if c["factor"][0] == "lds" else \
        f"blocked mode {mode}, panel classes {sorted(set(c['panels']), key=str)}"
    return f"front ({ns}, {nu}): {f}, {c['solve']} solve"


# ---- thresholds: every one is a pair of predicates on (ns, nu, mode), its two sides ----------------
def thresholds():
    """name -> (below, above): predicates on (ns, nu, mode, cls) with cls = classify(ns, nu, mode);
    a set covers a threshold when some front satisfies each.  Where a threshold is a single number
    the two sides are the two values next to it (M = 128 against 129), not merely "any front under"
    against "any front over"."""
    T = {}
    for c in (8, 16, 32, 48, 64, 96):
        T[f"M {c}|{c + 1}"] = (lambda ns, nu, mode, cls, c=c: ns + nu == c,
                               lambda ns, nu, mode, cls, c=c: ns + nu == c + 1)
    for c in (8, 16, 32, 48, 64, 96, 128):   # real-equivalent fronts of a complex handle: M is even
        T[f"M {c}|{c + 2}"] = (lambda ns, nu, mode, cls, c=c: ns + nu == c and classify(ns, nu + 2, 1 if c == 128 else 0) != cls,
                               lambda ns, nu, mode, cls, c=c: ns + nu == c + 2)
    T["M 127, 128"] = (lambda ns, nu, mode, cls: ns + nu == 127, lambda ns, nu, mode, cls: ns + nu == 128)
    for lo, hi in zip(LDS_CLASSES[:-1], LDS_CLASSES[1:]):
        T[f"LDS class {lo}|{hi}"] = (lambda ns, nu, mode, cls, lo=lo: cls["factor"] == ("lds", lo),
                                     lambda ns, nu, mode, cls, hi=hi: cls["factor"] == ("lds", hi))
    T["micro|tiny"] = (lambda ns, nu, mode, cls: cls["solve"] == "micro" and ns + nu == 8,
                       lambda ns, nu, mode, cls: cls["solve"] == "tiny" and ns + nu == 9)
    T["tiny|small by ns"] = (lambda ns, nu, mode, cls: cls["solve"] == "tiny" and ns == 64 and nu > 0,
                             lambda ns, nu, mode, cls: cls["solve"] == "small" and ns == 65 and nu > 0 and ns + nu <= 128)
    T["extremes (1, M-1), (M-1, 1), (M, 0) at M = 128"] = (
        lambda ns, nu, mode, cls: (ns, nu) == (1, 127),
        lambda ns, nu, mode, cls: (ns, nu) == (127, 1))
    T["dense (128, 0)"] = (lambda ns, nu, mode, cls: (ns, nu) == (128, 0), lambda ns, nu, mode, cls: (ns, nu) == (128, 0))
    T["nu mod 16 in {0, 1, 15}"] = (lambda ns, nu, mode, cls: mode == 0 and nu > 0 and nu % 16 == 15,
                                    lambda ns, nu, mode, cls: mode == 0 and nu > 0 and nu % 16 == 1)
    T["nu mod 16 = 0"] = (lambda ns, nu, mode, cls: mode == 0 and nu == 16, lambda ns, nu, mode, cls: mode == 0 and nu == 64)
    T["ns mod 4 in {1, 3}"] = (lambda ns, nu, mode, cls: mode == 0 and nu > 0 and ns % 4 == 3,
                               lambda ns, nu, mode, cls: mode == 0 and nu > 0 and ns % 4 == 1)
    T["U12 64 columns at a time: nu 63, 64 | 65, 127"] = (
        lambda ns, nu, mode, cls: mode == 0 and nu in (63, 64), lambda ns, nu, mode, cls: mode == 0 and nu in (65, 127))
    T["rows i and i + 64: M 64|65 with a contribution block"] = (
        lambda ns, nu, mode, cls: mode == 0 and ns + nu == 64 and nu > 0,
        lambda ns, nu, mode, cls: mode == 0 and ns + nu == 65 and nu > 0)
    # blocked fronts
    T["LDS|blocked, M 128|129"] = (lambda ns, nu, mode, cls: mode == 0 and ns + nu == 128,
                                   lambda ns, nu, mode, cls: mode != 0 and ns + nu == 129)
    T["M = 129 extremes"] = (lambda ns, nu, mode, cls: (ns, nu) == (1, 128), lambda ns, nu, mode, cls: (ns, nu) == (128, 1))
    T["M = 129 dense and split"] = (lambda ns, nu, mode, cls: (ns, nu) == (129, 0),
                                    lambda ns, nu, mode, cls: (ns, nu) in ((64, 65), (65, 64)))
    T["tiny|small by M (64, 64)|(64, 65)"] = (lambda ns, nu, mode, cls: (ns, nu) == (64, 64) and cls["solve"] == "tiny",
                                              lambda ns, nu, mode, cls: (ns, nu) == (64, 65) and cls["solve"] == "small")
    T["small|big by ns 256|257"] = (lambda ns, nu, mode, cls: (ns, nu) == (256, 0) and cls["solve"] == "small",
                                    lambda ns, nu, mode, cls: ns == 257 and cls["solve"] == "big")
    T["small|big by work at ns 256"] = (lambda ns, nu, mode, cls: (ns, nu) == (256, 0) and cls["solve"] == "small",
                                        lambda ns, nu, mode, cls: (ns, nu) == (256, 1) and cls["solve"] == "big")
    T["small|big by work at ns 128"] = (lambda ns, nu, mode, cls: (ns, nu) == (128, 384) and cls["solve"] == "small",
                                        lambda ns, nu, mode, cls: (ns, nu) == (128, 385) and cls["solve"] == "big")
    T["outer block 383|384"] = (lambda ns, nu, mode, cls: (ns, nu) == (383, 65), lambda ns, nu, mode, cls: (ns, nu) == (384, 65))
    T["outer block 384|385"] = (lambda ns, nu, mode, cls: (ns, nu) == (384, 65), lambda ns, nu, mode, cls: (ns, nu) == (385, 65))
    for r in (1, 31, 33, 63):
        T[f"blocked ns mod 64 = {r}"] = (lambda ns, nu, mode, cls, r=r: mode != 0 and ns % 64 == r and nu > 0,
                                         lambda ns, nu, mode, cls, r=r: mode != 0 and ns % 64 == r)
    for lo, hi in zip(PANEL_CLASSES, PANEL_CLASSES[1:] + ("more",)):
        T[f"panel class {lo}|{hi}"] = (lambda ns, nu, mode, cls, lo=lo: lo in cls["panels"],
                                       lambda ns, nu, mode, cls, hi=hi: hi in cls["panels"])
    T["mode 1 at ns = 512"] = (lambda ns, nu, mode, cls: mode == 1 and ns == 512, lambda ns, nu, mode, cls: mode == 1 and ns == 512)
    T["mode 2 at ns = 513 over a contribution block"] = (lambda ns, nu, mode, cls: mode == 2 and ns == 513 and nu > 0,
                                                        lambda ns, nu, mode, cls: mode == 2 and ns > 513 and nu > 0)
    T["mode 2 tile edge: ns mod 64 = 0 | 1"] = (lambda ns, nu, mode, cls: mode == 2 and ns % 64 == 0,
                                               lambda ns, nu, mode, cls: mode == 2 and ns % 64 == 1)
    return T


_SMALL_T = ["M 8|9", "M 16|17", "M 32|33", "M 48|49", "M 64|65", "M 96|97", "M 127, 128",
            "LDS class 16|32", "LDS class 32|48", "LDS class 48|64", "LDS class 64|96", "LDS class 96|128",
            "micro|tiny", "tiny|small by ns", "extremes (1, M-1), (M-1, 1), (M, 0) at M = 128", "dense (128, 0)",
            "nu mod 16 in {0, 1, 15}", "nu mod 16 = 0", "ns mod 4 in {1, 3}",
            "U12 64 columns at a time: nu 63, 64 | 65, 127", "rows i and i + 64: M 64|65 with a contribution block"]
_BLOCKED_T = ["LDS|blocked, M 128|129", "M = 129 extremes", "M = 129 dense and split",
              "tiny|small by M (64, 64)|(64, 65)", "small|big by ns 256|257", "small|big by work at ns 256",
              "outer block 383|384", "outer block 384|385",
              "blocked ns mod 64 = 1", "blocked ns mod 64 = 31", "blocked ns mod 64 = 33", "blocked ns mod 64 = 63"]

# ---- the shape sets -------------------------------------------------------------------------------
SMALL = [
    (1, 7), (7, 1), (4, 4), (8, 0), (1, 8), (8, 1), (5, 4), (9, 0),
    (1, 15), (15, 1), (3, 13), (16, 0), (1, 16), (16, 1), (4, 13), (17, 0),
    (1, 31), (31, 1), (15, 17), (17, 15), (32, 0), (1, 32), (32, 1), (16, 17), (33, 0),
    (1, 47), (47, 1), (32, 16), (33, 15), (48, 0), (1, 48), (48, 1), (34, 15), (49, 0),
    (1, 63), (63, 1), (3, 61), (48, 16), (64, 0), (1, 64), (64, 1), (5, 60), (65, 0),
    (1, 95), (95, 1), (32, 64), (33, 63), (31, 65), (96, 0), (1, 96), (96, 1), (32, 65), (97, 0),
    (1, 126), (126, 1), (63, 64), (64, 63), (127, 0),
    (1, 127), (127, 1), (64, 64), (65, 63), (63, 65), (4, 124), (5, 123), (3, 125), (128, 0),
]
_BLOCKED_BOTH = [
    (64, 64), (64, 65), (65, 64), (1, 128), (128, 1), (129, 0), (127, 2), (97, 32),
    (128, 384), (256, 0), (256, 1), (257, 1), (383, 65), (384, 65), (385, 65),
]
BLOCKED_PIVOT = _BLOCKED_BOTH + [(479, 30), (512, 0)]      # every ns + nu <= 512: no root in mode 2
BLOCKED_DOMINANT = _BLOCKED_BOTH + [(95, 34), (128, 385)]  # (128, 385): its root (513, 0) is in mode 2 either way
TILE = [(513, 33), (576, 64), (640, 0)]
REPIVOT = [(577, 130)]
COMPLEX = [(1, 3), (1, 4), (2, 2), (2, 3), (4, 4), (4, 5), (8, 0), (9, 0), (8, 8), (8, 9), (12, 12), (12, 13), (8, 24),
           (16, 16), (16, 17), (24, 24), (24, 25), (32, 32), (32, 33), (64, 0), (65, 0), (100, 40), (300, 10)]

# name -> (shapes, kind of the values, seed, values for expected_mode, thresholds the set must cover)
SETS = {
    "small-dominant": (SMALL, "dominant", 0, "dominant", _SMALL_T),
    "small-pivot": (SMALL, "pivot", 5, "pivot", _SMALL_T),
    "blocked-dominant": (BLOCKED_DOMINANT, "dominant", 0, "dominant",
                         _BLOCKED_T + ["small|big by work at ns 128", "mode 2 tile edge: ns mod 64 = 0 | 1"]),
    "blocked-pivot": (BLOCKED_PIVOT, "pivot", 0, "pivot",
                      _BLOCKED_T + ["panel class 64|128", "panel class 128|256", "panel class 256|512",
                                    "mode 1 at ns = 512"]),
    "tile": (TILE, "tile", 1, "pivot", ["mode 2 at ns = 513 over a contribution block",
                                        "mode 2 tile edge: ns mod 64 = 0 | 1"]),
    "repivot": (REPIVOT, "tile", 0, "repivoted", ["panel class 512|more"]),
    "complex-dominant": (COMPLEX, "complex", 0, "complex", None),
    "complex-pivot": (COMPLEX, "complex_pivot", 0, "complex", None),
}
# the complex sets are judged on their real-equivalent fronts (2 ns, 2 nu)
COMPLEX_T = ["M 8|10", "M 16|18", "M 32|34", "M 48|50", "M 64|66", "M 96|98", "M 128|130",
             "LDS class 16|32", "LDS class 32|48", "LDS class 48|64", "LDS class 64|96", "LDS class 96|128",
             "panel class 64|128", "panel class 128|256", "panel class 256|512", "panel class 512|more"]
# handles of the pivot values are created with partial pivoting (a diagonal entry is kept only where
# it is the largest of its column), as pivoting_small_fronts of test_gpu_solve_batched.py
HANDLE_KW = {"small-pivot": dict(diag_pivot_tol=1.0), "blocked-pivot": dict(diag_pivot_tol=1.0),
             "complex-pivot": dict(diag_pivot_tol=1.0)}


def set_matrix(name):
    shapes, kind, seed = SETS[name][:3]
    return shape_matrix(shapes, kind, seed)


def set_fronts(name):
    """[(ns, nu, mode)] the set's handle must have (a complex set: its real-equivalent fronts)."""
    shapes, kind, _, values, _ = SETS[name]
    k = 2 if kind.startswith("complex") else 1
    return [(k * ns, k * nu, expected_mode(k * ns, k * nu, values)) for ns, nu in expected_fronts(shapes)]


def set_thresholds(name):
    return COMPLEX_T if SETS[name][1].startswith("complex") else SETS[name][4]


def uncovered(fronts, names):
    """The sides of the thresholds `names` that no front of `fronts` ([(ns, nu, mode)]) stands on."""
    T = thresholds()
    cl = [(ns, nu, mode, classify(ns, nu, mode)) for ns, nu, mode in fronts]
    out = []
    for name in names:
        for side, pred in zip(("lower", "upper"), T[name]):
            if not any(pred(*f) for f in cl):
                out.append(f"{name}: {side} side")
    return out


def class_counts(fronts):
    from collections import Counter
    c = Counter()
    for ns, nu, mode in fronts:
        k = classify(ns, nu, mode)
        c[k["factor"]] += 1
        c[k["solve"]] += 1
        for p in set(k["panels"]):
            c[("panel", p)] += 1
    return dict(c)
