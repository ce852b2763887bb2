"""Fronts of prescribed shape on both sides of every kernel-class threshold, through the
factorization and every solve path.  The matrices, the class rules and the sets are those of
_front_shapes.py (their docstring lists the fronts by class); test_front_shapes.py proves on the CPU
that the inputs are what they are meant to be.  One handle per set, module-scoped, refine=0,
ordering="natural", relax=False; the handles of the pivot values with diag_pivot_tol=1 (partial
pivoting).

Per handle: the fronts and their candidate modes are the prescribed ones; the factors, front by
front, against the multifrontal oracle (_parity.front_parity: pivot order bitwise, then every front's
L panel and U12 at rtol 1e-12 times the growth; complex handles _parity.factor_parity); the solves
"N" and "T" ("C" as well on the complex sets) as single vectors and as batches of 5 and 17, every
batch column bitwise its single solve, pass counts asserted, outputs NaN before; the 5-wide batch
against the unrefined oracle solves (_batch_ref.assert_batch_against_oracle: backward error within 4 x
the oracle's or under 2^-51, agreement in norm at DENSE_TOL), and the same backward-error bound per
component of the block-diagonal matrix, so that a failure names the shape; log|det| against the
components' slogdet.  A failure names the component (ns, nu) and the classes of its fronts.

Measured on an MI355X (worst over the handle; the bounds are 1e-12, 4 -- or any ratio while the GPU's
backward error is under 2^-51 = 4.4e-16 --, and 1e-10):

    handle            front diff  berr ratio, whole batch (GPU / oracle)   worst component ratio  |x-xo|/|xo|
    small-dominant    1.110e-16   N 1.009 (1.038e-15 / 1.029e-15)          1.406 T (1, 64)        2.157e-16
    small-pivot       9.674e-14   T 3.754 (1.901e-14 / 5.064e-15)          3.754 T (32, 65)       2.005e-13
    blocked-dominant  1.110e-16   T 0.857 (1.570e-15 / 1.831e-15)          1.312 N (127, 2)       6.472e-16
    blocked-pivot     7.939e-15   T 1.202 (2.231e-15 / 1.856e-15)          2.333 N (383, 65)      2.352e-11
    tile              1.027e-13   T 1.001 (5.672e-12 / 5.666e-12)          2.824 N (640, 0)       3.796e-11
    repivot           9.536e-14   T 1.166 (1.233e-13 / 1.058e-13)          1.166 T (577, 130)     7.860e-12
    complex-dominant  (whole)     C 0.924 (1.534e-15 / 1.660e-15)          2.086 T (12, 13)       3.528e-16
    complex-pivot     (whole)     N 0.657 (1.725e-15 / 2.625e-15)          2.238 T (4, 5)         2.666e-13

"front diff" is the worst scaled difference of a front's stored values from the oracle's; the complex
handles are compared as whole factors (factor_parity) and pass at its 1e-12.  The component ratios count
only columns whose GPU backward error is above 2^-51.  The largest ratio, 3.754, is the front (32, 65) of
the small-pivot set in the transposed solve: 1.9e-14 against the host substitution's 5.1e-15, both a
few dozen unit roundoffs.  log|det|
differs from the components' slogdet by at most 1.8e-11 (tolerances 2.7e-8 .. 5.1e-4).  Every test of
this module passed as first written; it found no fault in the kernels or in the class rules.
"""
import math
import re

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O
import smlu

import _front_shapes as S
from _batch_ref import FACTOR, FLOOR, assert_batch_against_oracle, berr, op_matrix, oracle_columns
from _diag_ref import rounding
from _parity import DENSE_TOL, _real, factor_parity, front_parity
from test_gpu_solve_trans_batched import _rhs

pytestmark = pytest.mark.gpu

REAL = [name for name in S.SETS if not name.startswith("complex")]
OPTS = dict(refine=0, ordering="natural", relax=False)
HANDLE_KW = S.HANDLE_KW


def make_handle(name):
    A = S.set_matrix(name)
    return A, smlu.ParallelSparseLU(A, **OPTS, **HANDLE_KW.get(name, {}))


@pytest.fixture(scope="module")
def handles(gpu):
    """name -> (A, F), each set factored once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = make_handle(name)
        return cache[name]

    yield get
    for _, F in cache.values():
        F.close()


# ---- naming what failed ---------------------------------------------------------------------------
def front_owner(name):
    """Per front of the set: the index of the component it belongs to."""
    owner = []
    for c, (ns, nu) in enumerate(S.SETS[name][0]):
        owner += [c] * (2 if nu else 1)
    return owner


def component_text(name, c):
    """Component c of the set: its (ns, nu) and the classes of its fronts."""
    what = "; ".join(S.describe(*f) for f, o in zip(S.set_fronts(name), front_owner(name)) if o == c)
    real = " (real-equivalent fronts)" if name.startswith("complex") else ""
    return f"component {c} (ns, nu) = {S.SETS[name][0][c]}{real} [{what}]"


def locate(name, text):
    """The components a parity message speaks of: `front s` of front_parity, or the row positions
    after `first [...]` of a pivot-order mismatch."""
    k = 2 if name.startswith("complex") else 1
    out = []
    m = re.search(r"front (\d+) \(", text)
    if m:
        out.append(front_owner(name)[int(m.group(1))])
    m = re.search(r"first \[([\d\s]+)\]", text)
    if m:
        rows = S.component_rows(S.SETS[name][0])
        for pos in (int(v) for v in m.group(1).split()):
            out += [c for c, (_, r0, r1) in enumerate(rows) if k * r0 <= pos < k * r1]
    return [component_text(name, c) for c in dict.fromkeys(out)]


def worst_component_of_factors(name, K, F):
    """Where the exported factors of a handle differ most from the fixed-pivot oracle's (run only
    after factor_parity failed, to name the component)."""
    fx = _real(F)
    ref = O.OracleLU(K, fx["p"], fx["q"], fx["Rs"])
    k = 2 if name.startswith("complex") else 1
    worst = (-1.0, None)
    for c, (_, r0, r1) in enumerate(S.component_rows(S.SETS[name][0])):
        r0, r1 = k * r0, k * r1
        d = 0.0
        for G, R in ((fx["L"], ref.L), (fx["U"], ref.U)):
            Gc, Rc = G[r0:r1][:, r0:r1], R[r0:r1][:, r0:r1]
            d = max(d, abs(Gc - Rc).max() / max(abs(Rc).max(), 1.0))
        if d > worst[0]:
            worst = (d, c)
    return f"largest difference {worst[0]:.3e} in " + component_text(name, worst[1])


def parity(name, A, F, prev_pivmode=0):
    """front_parity (real) or factor_parity (complex) with the failing component named."""
    try:
        if F.is_complex:
            factor_parity(O.real_equivalent(A), F, prev_pivmode=prev_pivmode)
            return None
        return front_parity(A, F, prev_pivmode=prev_pivmode)
    except AssertionError as e:
        where = locate(name, str(e))
        if not where and F.is_complex:
            where = [worst_component_of_factors(name, O.real_equivalent(A), F)]
        raise AssertionError(f"{name}: {e}\n  " + "\n  ".join(where)) from e


# ---- shapes and modes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.SETS))
def test_shapes_and_modes_on_the_handle(handles, name):
    A, F = handles(name)
    fr = F.fronts()
    got = list(zip(np.diff(fr["first"]).tolist(), np.diff(fr["rowptr"]).tolist(), fr["mode"].tolist()))
    want = S.set_fronts(name)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, (len(got), len(want), bad[:5])
    nk = 2 * F.n if F.is_complex else F.n
    assert np.array_equal(F.perm_scale()[1], np.arange(nk))   # q is the identity
    assert np.array_equal(fr["p0"], np.arange(nk))
    assert F.stat("cpair") == (1 if F.is_complex else 0)
    if name == "repivot":
        assert F.stat("repivots") == 1 and F.stat("pivmode") == 1 and F.stat("weak") == 0
    else:
        assert F.stat("repivots") == 0 and F.stat("pivmode") == 0
    if not F.is_complex:
        assert F.stat("dominant") == (1 if name.endswith("dominant") else 0)
        moved = F.perm_scale()[0] != fr["p0"]
        per_front = [bool(moved[fr["first"][s]:fr["first"][s + 1]].any()) for s in range(len(got))]
        if name.endswith("dominant"):
            assert not any(per_front)
        else:   # a row moved in every front that has two pivots to choose from
            assert [g for g, mv in zip(got, per_front) if g[0] >= 2 and not mv] == []


# ---- factors, front by front -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.SETS))
def test_factors_front_by_front(handles, name):
    A, F = handles(name)
    res = parity(name, A, F)
    if res is not None:
        nf, entries, worst = res
        assert nf == len(S.set_fronts(name))
        print(f"{name}: {nf} fronts, {entries} entries, worst scaled front difference {worst:.3e} (rtol 1e-12)")


# ---- solves ------------------------------------------------------------------------------------------
def solve_cases():
    out = []
    for name in S.SETS:
        for trans in ("N", "T", "C") if name.startswith("complex") else ("N", "T"):
            out.append((name, trans))
    return out


def passes_key(trans):
    return "solve_passes" if trans == "N" else "solve_trans_passes"


def counted(F, trans, nrhs, call):
    key = passes_key(trans)
    p0 = F.stat(key)
    assert np.isfinite(p0)
    call()
    assert F.stat(key) - p0 == math.ceil(nrhs / 16), (trans, nrhs, F.stat(key) - p0)


@pytest.mark.parametrize("name, trans", solve_cases())
def test_solves(handles, name, trans):
    import torch
    A, F = handles(name)
    z = F.is_complex
    B = _rhs(F.n, 17, 700 + len(name), z)
    singles = []
    for j in range(17):
        bj = B[j].contiguous()
        xj = torch.full_like(bj, float("nan"))
        counted(F, trans, 1, lambda: F.solve_device(xj, bj, trans=trans))
        assert torch.isfinite(torch.view_as_real(xj) if z else xj).all(), j
        singles.append(xj)
    X5 = None
    for lo, hi in ((0, 5), (12, 17), (0, 17)):   # a slot holds another column in the second batch of 5
        Bw = B[lo:hi].contiguous()
        Xw = torch.full_like(Bw, float("nan"))
        counted(F, trans, hi - lo, lambda: F.solve_multi_device(Xw, Bw, trans=trans))
        for j in range(lo, hi):
            assert torch.equal(Xw[j - lo], singles[j]), (name, trans, (lo, hi), j)
        if X5 is None:
            X5 = Xw
    Bh, Xh = B[:5].cpu().numpy(), X5.cpu().numpy()
    Xo = oracle_columns(A, F, Bh, trans)
    # per component of the block-diagonal matrix: the same backward-error bound, naming the shape
    Op = sp.csr_matrix(op_matrix(A, trans))
    fails, worst = [], (0.0, None)
    for c, (shape, r0, r1) in enumerate(S.component_rows(S.SETS[name][0])):
        Oc = Op[r0:r1][:, r0:r1]
        for j in range(5):
            g, o = berr(Oc, Xh[j, r0:r1], Bh[j, r0:r1]), berr(Oc, Xo[j, r0:r1], Bh[j, r0:r1])
            if g > FLOOR and g / max(o, 2.0 ** -70) > worst[0]:
                worst = (g / max(o, 2.0 ** -70), shape)
            if not g <= max(FACTOR * o, FLOOR):
                fails.append(f"column {j}: backward error {g:.3e}, the oracle's {o:.3e}, in " + component_text(name, c))
    print(f"{name} {trans}: largest per-component berr ratio GPU/oracle over 2^-51: {worst[0]:.3f} at {worst[1]}")
    assert not fails, f"{name} {trans}: " + "\n  ".join(fails[:6])
    assert_batch_against_oracle(A, F, Bh, Xh, trans, Xo=Xo, tol=DENSE_TOL, label=name)


# ---- refactor replay across modes --------------------------------------------------------------------
def test_refactor_replay_across_modes(gpu):
    """Dominant values (every blocked front on the diagonal tile, mode 2), then the pivot values of
    the same pattern (mode 1, rows moved in every front), then the dominant values again: parity after
    each, a second factorization in the new mode each time the mode flips, and the third factor
    store bitwise the first."""
    A = S.set_matrix("blocked-pivot")
    D = S.shape_matrix(S.BLOCKED_PIVOT, "dominant", 3)
    assert np.array_equal(A.indptr, D.indptr) and np.array_equal(A.indices, D.indices)
    F = smlu.ParallelSparseLU(D, **OPTS, **HANDLE_KW["blocked-pivot"])
    want2 = [S.expected_mode(ns, nu, "dominant") for ns, nu in S.expected_fronts(S.BLOCKED_PIVOT)]
    want1 = [m for _, _, m in S.set_fronts("blocked-pivot")]
    assert F.fronts()["mode"].tolist() == want2 and F.stat("dominant") == 1
    parity("blocked-pivot", D, F)
    store1 = F.front_store()[0].copy()
    m0 = F.stat("mode_refactors")
    F.refactor(A.data)
    assert F.stat("dominant") == 0 and F.stat("mode_refactors") == m0 + 1
    assert F.fronts()["mode"].tolist() == want1
    assert F.stat("repivots") == 0 and F.stat("pivmode") == 0
    parity("blocked-pivot", A, F)
    assert not np.array_equal(F.perm_scale()[0], F.fronts()["p0"])
    F.refactor(D.data)
    assert F.stat("dominant") == 1 and F.stat("mode_refactors") == m0 + 2
    assert F.fronts()["mode"].tolist() == want2
    parity("blocked-pivot", D, F)
    store3 = F.front_store()[0]
    assert store3.shape == store1.shape and np.array_equal(store3, store1)
    F.refactor(D.data)                       # the same values again: no mode change
    assert F.stat("mode_refactors") == m0 + 2
    F.close()


# ---- log|det| ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REAL)
def test_logabsdet_is_the_sum_over_the_components(handles, name):
    """slogdet per component (sign product, log sum) at the bound of test_gpu_logabsdet.py:
    8 n 2^-52 cond_1(A), floor 1e-12 |ref|; cond_1 of a block-diagonal matrix from its blocks."""
    A, F = handles(name)
    A = sp.csr_matrix(A)
    sref, lref, a1, i1 = 1.0, 0.0, 0.0, 0.0
    for shape, r0, r1 in S.component_rows(S.SETS[name][0]):
        C = A[r0:r1][:, r0:r1].toarray()
        s, l = np.linalg.slogdet(C)
        sref *= s
        lref += l
        a1 = max(a1, np.abs(C).sum(axis=0).max())
        i1 = max(i1, np.abs(np.linalg.inv(C)).sum(axis=0).max())
    tol = max(rounding(F.n, a1 * i1), 1e-12 * abs(lref))
    la, sg = F.logabsdet()
    print(f"{name}: logabs {la!r} ref {lref!r} diff {abs(la - lref):.3e} tol {tol:.3e} sign {sg} ref {sref}")
    assert abs(la - lref) <= tol, (la, lref, tol)
    assert sg == sref, (sg, sref)
