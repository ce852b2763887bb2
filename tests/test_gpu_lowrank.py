"""Low-rank updates on the GPU (smlu_lowrank_set*, smlu_solve_lowrank*; F.lowrank_set, F.solve_lowrank,
F.update_columns).

Reference: tests/_lowrank_ref.py, a NumPy restatement of the same algorithm with an exact
preconditioner; tests/test_lowrank_derivation.py shows on the CPU that it stops on berr <= 2^-51 on every
case run here and that the goldens' forward check is never skipped.  Backward errors are NumPy's own.

The step count.  How many corrections a run makes hinges on whether the first backward error lies above
or below 2^-51 = 4 unit roundoffs, and that of an exact preconditioner (1e-16 .. 5e-16 on these inputs)
lies on either side of it, as does that of a real LU solve: on the first ten cases the exact
restatement needs 0 corrections where the library needs 1 eight times, both correctly.  So info.steps is
compared with the restatement run on the library's own plain factor solves (y0 and Y are then bitwise
the library's, and only the thin passes differ in rounding).  Even so a backward error near 4 unit
roundoffs is made of the last roundings of x, and the two runs' values there differ: on 5 of 76
cases they fell on opposite sides of 2^-51, the restatement's value at most 14 % from it (3.82e-16 on
fe_5, k = 2, T; 4.19e-16 on random_dominant_200, k = 17, T).  So the counts must be equal unless a
backward error the restatement measured lies within 25 % of 2^-51 (16 of those 76 cases), where they
may differ by one.  On every case the count is also checked against the library's own measurements:
the last berr is at most 2^-51, and a run limited to m <= info.steps corrections, which repeats the
full run bit for bit, reports a berr above 2^-51 before correction m.  The exact restatement keeps the
unrefined solution the eta check is measured against, and its counts are printed beside the others.

The forward check's reference is np.linalg.solve polished in extended precision
(_lowrank_ref.polished_solve): NumPy's own solution is no more accurate than the library's, and the
perturbation bound is a bound against the solution itself.

Bounds.  Refined: the returned x has componentwise backward error at most 2^-51 + (w + 2) 2^-52, the
refinement's target plus the rounding of evaluating one residual row of w = (max entries in a row of
op(A)) + 2 k terms.  Goldens: with eta the normwise backward error and kappa = cond_inf(A'), the forward
error against np.linalg.solve is at most 2 eta kappa / (1 - eta kappa).  Unrefined: eta is at most 8
times the restatement's unrefined eta on the same input plus rounding(n, cond_1(A)) = 8 n 2^-52
cond_1(A); 8 is _diag_ref.rounding's constant for a differently ordered factorization, and the second
term is what the factor solves' own backward error, which the exact-preconditioner restatement does
not have, can put into Y and y0.

The partitioned-handle refusal needs two processes: tests/test_gpu_lowrank_dist.py."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import smlu
from smlu import _lib as C

import _lowrank_ref as R
from _diag_ref import GOLDEN, load_golden, rounding
from test_gpu_complex import helmholtz3d

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(gpu):
    """One factorization per input, never refined by itself (refine=0), shared by this module."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = smlu.ParallelSparseLU(R.problem(name)["A"], refine=0)
        return cache[name]
    yield get
    for F in cache.values():
        F.close()


def dense_op(name, k, kind, op):
    P = R.problem(name)
    U, V, _ = R.update(name, k, kind)
    A2 = P["A"].toarray() + U @ V.T
    return A2 if op == "N" else A2.T


def forward_bound(M, eta):
    kappa = float(np.linalg.cond(M, np.inf))
    return (2 * eta * kappa / (1 - eta * kappa) if eta * kappa < 0.5 else None), kappa


def gpu_prec(F, op):
    """M -> op(A)^-1 M by the library's own plain factor solve (a refine=0 handle), columns in batches."""
    def prec(M):
        M = np.asfortranarray(M, dtype=np.float64)
        X = np.empty_like(M)
        if M.size:
            smlu.ldiv_(X, F, M, trans=op)
        return X
    return prec


def trans_batches(k):
    return (k + 15) // 16


@pytest.mark.parametrize("name,k,kind,op", R.gpu_cases())
def test_solves_the_updated_system(handles, name, k, kind, op):
    P = R.problem(name)
    A, b, n = P["A"], P["b"], P["n"]
    U, V, _ = R.update(name, k, kind)
    ref = R.reference(name, k, kind, op)
    F = handles(name)
    ref_f = R.lowrank_ref(A, U, V, b, op, gpu_prec(F, op))      # the restatement on the library's factor solves
    tp0, fp0 = F.stat("solve_trans_passes"), F.stat("solve_passes")
    si = F.lowrank_set(U, V)
    assert si.status == C.SMLU_OK and si.k == k and F.stat("lowrank_k") == k
    assert si.solves == trans_batches(k) == F.stat("lowrank_solves")
    assert F.stat("solve_trans_passes") == tp0 and F.stat("solve_passes") - fp0 == trans_batches(k)
    assert si.pivot_min > 0 and 0 < si.rcond_c <= 1 and np.isfinite(si.gram_max)
    assert F.stat("lowrank_set_ms_last") > 0
    # ---- refined (steps = -1) ----
    tp0, fp0 = F.stat("solve_trans_passes"), F.stat("solve_passes")
    x, info = F.solve_lowrank(b, trans=op)
    _, berr = R.residual(A, U, V, x, b, op)
    bound = R.berr_bound(A, k, op)
    print(f"{name} n={n} k={k} {kind} op={op}: steps {info.steps} (restatement: on the factor solves "
          f"{ref_f['steps']} berrs {' '.join('%.2e' % v for v in ref_f['berrs'])}; exact {ref['steps']} "
          f"berrs {' '.join('%.2e' % v for v in ref['berrs'])}) stop {info.stop} "
          f"berr {info.berr:.2e} numpy berr {berr:.2e} bound {bound:.2e} rcond_c {si.rcond_c:.2e} "
          f"set {F.stat('lowrank_set_ms_last'):.2f} ms solve {F.stat('lowrank_ms_last'):.2f} ms")
    assert info.status == C.SMLU_OK and info.stop == 1 and info.k == k
    # the count against the library's own measurements: the last backward error is at the target ...
    assert 0.0 <= info.berr <= R.BERR_STOP and 0 <= info.steps <= 3
    # ... and against the restatement's, unless one of its backward errors lies within 25 % of the target
    # (there the two runs differ by up to 14 %: berr is made of the last roundings of x)
    near = [v for v in ref_f["berrs"] if 0.75 * R.BERR_STOP < v < 1.25 * R.BERR_STOP]
    if not near:
        assert info.steps == ref_f["steps"]
    else:
        assert abs(info.steps - ref_f["steps"]) <= 1
    assert berr <= bound
    assert info.solves == 1 + info.steps == F.stat("lowrank_solves")
    if op == "N":
        assert F.stat("solve_trans_passes") == tp0 and F.stat("solve_passes") - fp0 == info.solves
    else:       # the first transposed solve after a set also computes Yt, 16 columns per pass
        assert F.stat("solve_passes") == fp0
        assert F.stat("solve_trans_passes") - tp0 == info.solves + trans_batches(k)
    if name == "poisson3d_28+I":
        assert F.stat("solve_sweeps") > 0      # the handle really has large fronts
    if name in GOLDEN:
        M = dense_op(name, k, kind, op)
        eta = R.normwise(A, U, V, x, b, op, anorm=float(np.abs(M).sum(axis=1).max()))
        fb, kappa = forward_bound(M, eta)
        xs = R.polished_solve(M, b)
        err = float(np.abs(x - xs).max() / np.abs(xs).max())
        print(f"  eta {eta:.2e} kappa {kappa:.2e} forward {err:.2e} bound {fb}")
        if fb is not None:                     # eta kappa >= 1/2: the bound says nothing
            assert err <= fb
    # ---- unrefined (steps = 0) ----
    tp0 = F.stat("solve_trans_passes")
    x0, i0 = F.solve_lowrank(b, trans=op, steps=0)
    assert (i0.steps, i0.stop, i0.berr, i0.solves, i0.k) == (0, 0, -1.0, 1, k)
    assert F.stat("solve_trans_passes") - tp0 == (1 if op != "N" else 0)      # Yt is kept
    eta0 = R.normwise(A, U, V, x0, b, op)
    eta_ref = R.normwise(A, U, V, ref["x0"], b, op)
    slack = rounding(n, P["cond1"])
    print(f"  unrefined eta {eta0:.2e} restatement {eta_ref:.2e} ratio {eta0 / eta_ref:.2f} slack {slack:.2e}")
    assert eta0 <= 8 * eta_ref + slack
    # ---- every counted correction followed a backward error above the target ----
    # A run limited to m <= info.steps corrections repeats the full run's first m rounds bit for bit and
    # ends at its limit, so the berr it reports is the one the full run measured before correction m.
    for m in range(1, info.steps + 1):
        xm, im = F.solve_lowrank(b, trans=op, steps=m)
        print(f"  limit {m}: steps {im.steps} stop {im.stop} berr before correction {m}: {im.berr:.2e}")
        assert (im.steps, im.stop, im.solves) == (m, 3, 1 + m)
        assert im.berr > R.BERR_STOP
    if info.steps > 0:
        assert np.array_equal(xm, x)              # the full run stopped without another correction


def test_zero_update_and_no_update_are_the_plain_solve(handles):
    name = "fe_8"
    P = R.problem(name)
    F = handles(name)
    b, n = P["b"], P["n"]
    V = np.random.default_rng(5).uniform(-1, 1, (n, 7))
    for op in ("N", "T"):
        xs = np.empty(n)
        smlu.ldiv_(xs, F, b, trans=op)
        si = F.lowrank_set(np.zeros((n, 7)), V)
        assert si.status == C.SMLU_OK and si.k == 7 and si.gram_max == 0.0 and si.rcond_c == 1.0
        x, info = F.solve_lowrank(b, trans=op, steps=0)
        assert np.array_equal(x, xs) and info.k == 7
        F.lowrank_clear()
        assert F.stat("lowrank_k") == 0
        x, info = F.solve_lowrank(b, trans=op, steps=0)
        assert np.array_equal(x, xs) and info.k == 0 and info.solves == 1
        x, info = F.solve_lowrank(b, trans=op)          # refined by the same rule, k = 0
        assert info.k == 0 and info.stop == 1
        assert R.residual(P["A"], np.zeros((n, 0)), np.zeros((n, 0)), x, b, op)[1] <= R.berr_bound(P["A"], 0, op)


def test_update_columns_and_refactor_agree(gpu):
    name, k = "fe_8", 7
    P = R.problem(name)
    A, b, n = P["A"], P["b"], P["n"]
    U, V, cols = R.update(name, k, "cols")
    A2 = R.updated_matrix(name, k, "cols")
    F = smlu.ParallelSparseLU(A, refine=0)
    Uh = A2[:, cols].toarray() - A[:, cols].toarray()    # the hand-built update: A2's columns minus A's
    assert np.abs(Uh - U).max() <= 2.0 ** -52 * np.abs(A2[:, cols].toarray()).max()
    F.lowrank_set(Uh, V)
    x1, i1 = F.solve_lowrank(b)
    si = F.update_columns(cols, A2, A)
    assert si.k == k
    x2, i2 = F.solve_lowrank(b)
    assert np.array_equal(x1, x2) and i1 == i2
    with pytest.raises(ValueError):
        F.update_columns(cols[:-1], A2, A)              # A2 differs from A outside these columns
    assert F.stat("lowrank_k") == k                     # a refused call installs and drops nothing
    # lifetime: a refactor drops the update; the plain solve of the new factors agrees to the forward bound
    F.refactor(A2.data)
    assert F.stat("lowrank_k") == 0
    xr = np.empty(n)
    smlu.ldiv_(xr, F, b)
    x3, i3 = F.solve_lowrank(b, steps=0)
    assert i3.k == 0 and np.array_equal(x3, xr)
    M = A2.toarray()
    Z = np.zeros((n, 0))
    anorm = float(np.abs(M).sum(axis=1).max())
    f1, _ = forward_bound(M, R.normwise(A2, Z, Z, x1, b, "N", anorm))
    f2, _ = forward_bound(M, R.normwise(A2, Z, Z, xr, b, "N", anorm))
    err = float(np.abs(x1 - xr).max() / np.abs(xr).max())
    print(f"lowrank vs refactor: {err:.2e} bounds {f1:.2e} + {f2:.2e}")
    assert err <= f1 + f2                               # each within its bound of the exact solution
    F.lowrank_clear()
    F.lowrank_clear()                                   # twice is fine
    F.close()


@pytest.mark.parametrize("name,k", [("fe_5", 17), ("poisson2d_300+I", 16)])
def test_determinism_and_forms(handles, name, k):
    """Two set + solve sequences, the host and device forms, x aliasing b and an odd caller ld: all
    bitwise equal."""
    P = R.problem(name)
    b, n = P["b"], P["n"]
    U, V, _ = R.update(name, k, "cols")
    F = handles(name)
    L = C.lib()
    for op in ("N", "T"):
        s0 = F.lowrank_set(U, V)
        x0, i0 = F.solve_lowrank(b, trans=op)
        s1 = F.lowrank_set(U, V)
        x1, i1 = F.solve_lowrank(b, trans=op)
        assert s0 == s1 and np.array_equal(x0, x1) and i0 == i1
        xb = b.copy()
        x2, i2 = F.solve_lowrank(xb, trans=op, x=xb)                    # host form, x is b
        assert x2 is xb and np.array_equal(x2, x0) and i2 == i0
        dU, dV = torch.from_numpy(U.T.copy()).cuda(), torch.from_numpy(V.T.copy()).cuda()
        s3 = F.lowrank_set_device(dU, dV)
        assert s3 == s0
        db = torch.from_numpy(b).cuda()
        dx = torch.empty_like(db)
        i3 = F.solve_lowrank_device(dx, db, trans=op)
        assert np.array_equal(dx.cpu().numpy(), x0) and i3 == i0
        assert np.array_equal(db.cpu().numpy(), b)                      # b is only read
        i4 = F.solve_lowrank_device(db, db, trans=op)                   # device form, x is b
        assert np.array_equal(db.cpu().numpy(), x0) and i4 == i0
        # the caller's leading dimension n + 3 (odd for even n, and never a multiple of 2 doubles for both)
        ld = n + 3
        Up, Vp = np.full((ld, k), 7.0, order="F"), np.full((ld, k), 7.0, order="F")
        Up[:n], Vp[:n] = U, V
        ci = C.SmluLowrankInfo()
        assert L.smlu_lowrank_set(F._h, k, C.ptr(Up), ld, C.ptr(Vp), ld, ctypes.byref(ci)) == C.SMLU_OK
        x5, i5 = F.solve_lowrank(b, trans=op)
        assert np.array_equal(x5, x0) and i5 == i0
        dUp, dVp = torch.from_numpy(Up.T.copy()).cuda(), torch.from_numpy(Vp.T.copy()).cuda()
        assert L.smlu_lowrank_set_device(F._h, k, ctypes.c_void_p(dUp.data_ptr()), ld, ctypes.c_void_p(dVp.data_ptr()),
                                         ld, ctypes.byref(ci)) == C.SMLU_OK
        torch.cuda.synchronize()
        x6, i6 = F.solve_lowrank(b, trans=op)
        assert np.array_equal(x6, x0) and i6 == i0
    F.lowrank_clear()


def test_smaller_and_larger_rank_behave_as_a_fresh_handle(gpu):
    name = "random_dominant_200"
    P = R.problem(name)
    b = P["b"]
    want = {}
    for k in (2, 17, 32):
        F = smlu.ParallelSparseLU(P["A"], refine=0)
        U, V, _ = R.update(name, k, "cols")
        F.lowrank_set(U, V)
        want[k] = [F.solve_lowrank(b, trans=op) for op in ("N", "T")]
        F.close()
    F = smlu.ParallelSparseLU(P["A"], refine=0)
    for k in (17, 2, 32, 2):                  # shrink, grow (the buffers are reallocated), shrink
        U, V, _ = R.update(name, k, "cols")
        F.lowrank_set(U, V)
        for (xw, iw), op in zip(want[k], ("N", "T")):
            x, info = F.solve_lowrank(b, trans=op)
            assert np.array_equal(x, xw) and info == iw, (k, op)
    F.close()


def test_handle_is_left_as_it_was(gpu):
    name = "fe_8"
    P = R.problem(name)
    F = smlu.ParallelSparseLU(P["A"])
    b = P["b"]
    U, V, _ = R.update(name, 7, "cols")
    x0, x1 = np.empty_like(b), np.empty_like(b)
    smlu.ldiv_(x0, F, b)
    r0 = F.rcond("1", parts=True)
    la0 = F.logabsdet()
    evals = F.stat("logabsdet_evals")
    F.lowrank_set(U, V)
    for op in ("N", "T"):
        _, info = F.solve_lowrank(b, trans=op)
        assert info.stop == 1
    smlu.ldiv_(x1, F, b)
    assert np.array_equal(x0, x1)                 # the plain solve ignores the installed update
    F.lowrank_clear()
    smlu.ldiv_(x1, F, b)
    assert np.array_equal(x0, x1)
    assert F.rcond("1", parts=True) == r0
    assert F.stat("rcond_solves") == 0            # still the cached answer
    assert F.logabsdet() == la0 and F.stat("logabsdet_evals") == evals
    F.close()


def test_singular_update_installs_nothing(gpu):
    A = sp.diags([2.0, 4.0, 8.0, 16.0]).tocsc()
    F = smlu.ParallelSparseLU(A, refine=0)
    b = np.array([1.0, 2.0, 3.0, 4.0])
    e2 = np.zeros(4)
    e2[2] = 1.0
    si = F.lowrank_set(e2 * 3.0, e2)              # an earlier, regular update: a_22 = 11
    assert si.status == C.SMLU_OK and F.stat("lowrank_k") == 1
    x, _ = F.solve_lowrank(b)
    assert np.allclose(x, b / np.array([2.0, 4.0, 11.0, 16.0]), rtol=2.0 ** -50, atol=0.0)
    si = F.lowrank_set(-A[:, [2]].toarray().ravel(), e2)   # every intermediate a power of two: C = 0 exactly
    assert si.status == C.SMLU_SINGULAR and si.k == 0 and si.pivot_min == 0.0 and si.rcond_c == 0.0
    assert si.gram_max == 1.0
    assert F.stat("lowrank_k") == 0               # the earlier update is dropped as well
    x, info = F.solve_lowrank(b, steps=0)
    assert info.k == 0 and np.array_equal(x, b / np.array([2.0, 4.0, 8.0, 16.0]))
    F.close()


def test_near_singular_and_nan(gpu):
    name = "fe_8"
    P = R.problem(name)
    A, n, b = P["A"], P["n"], P["b"]
    F = smlu.ParallelSparseLU(A, refine=0)
    j = n // 2
    ej = np.zeros(n)
    ej[j] = 1.0
    si = F.lowrank_set(-A[:, [j]].toarray().ravel(), ej)   # column j becomes zero: A' is singular
    print(f"zeroed column: status {si.status} pivot_min {si.pivot_min:.2e} rcond_c {si.rcond_c:.2e}")
    assert si.status == C.SMLU_SINGULAR or (si.status == C.SMLU_OK and si.pivot_min <= rounding(n, P["cond1"]))
    U, V, _ = R.update(name, 7, "cols")
    Un = U.copy()
    Un[3, 4] = np.nan
    si = F.lowrank_set(Un, V)
    assert si.status == C.SMLU_SINGULAR and F.stat("lowrank_k") == 0
    si = F.lowrank_set(U, V)                      # the handle is usable: no NaN stayed behind in a pad row
    assert si.status == C.SMLU_OK
    x, info = F.solve_lowrank(b)
    assert info.stop == 1 and R.residual(A, U, V, x, b, "N")[1] <= R.berr_bound(A, 7, "N")
    F.close()


def test_argument_and_state_errors(gpu):
    A = load_golden("poisson2d_16")
    F = smlu.ParallelSparseLU(A)
    L = C.lib()
    n = A.shape[0]
    b, x = np.sqrt(np.arange(1.0, n + 1.0)), np.empty(n)
    W = np.asfortranarray(np.random.default_rng(3).uniform(-1, 1, (n, 33)))
    ci = C.SmluLowrankInfo()

    def lset(k, pu=W, ldu=n, pv=W, ldv=n):
        return L.smlu_lowrank_set(F._h, k, C.ptr(pu), ldu, C.ptr(pv), ldv, ctypes.byref(ci))

    def solve(op=C.SMLU_OP_N, steps=-1, pb=b, px=x):
        return L.smlu_solve_lowrank(F._h, op, steps, C.ptr(pb), C.ptr(px), ctypes.byref(ci))
    assert lset(33) == C.SMLU_ERR_ARG and lset(-1) == C.SMLU_ERR_ARG
    assert lset(2, ldu=n - 1) == C.SMLU_ERR_ARG and lset(2, ldv=n - 1) == C.SMLU_ERR_ARG
    assert lset(2, pu=None) == C.SMLU_ERR_ARG and lset(2, pv=None) == C.SMLU_ERR_ARG
    assert lset(0, pu=None, pv=None) == C.SMLU_OK             # k = 0 is clear
    assert lset(2) == C.SMLU_OK and F.stat("lowrank_k") == 2
    assert solve() == C.SMLU_OK and ci.k == 2
    assert L.smlu_solve_lowrank(F._h, C.SMLU_OP_N, -1, C.ptr(b), C.ptr(x), None) == C.SMLU_OK   # NULL info
    assert solve(op=3) == C.SMLU_ERR_ARG and solve(op=-1) == C.SMLU_ERR_ARG
    assert solve(steps=-2) == C.SMLU_ERR_ARG
    assert solve(pb=None) == C.SMLU_ERR_ARG and solve(px=None) == C.SMLU_ERR_ARG
    A2 = A.tocsr()
    A2.data[A2.indptr[20]:A2.indptr[21]] = 0.0                # a zero row: singular, same pattern
    A2 = A2.tocsc()
    with pytest.raises(smlu.SingularException):
        F.refactor(A2.data)
    assert solve() == C.SMLU_ERR_STATE and lset(2) == C.SMLU_ERR_STATE
    F.refactor(A.data)
    assert F.stat("lowrank_k") == 0
    assert lset(2) == C.SMLU_OK and solve() == C.SMLU_OK
    F.close()


def test_refused_calls_leave_the_installed_update(gpu):
    """A set refused for its arguments (a negative code) changes nothing; one that fails on its values
    (SMLU_SINGULAR) drops what was installed."""
    name = "fe_5"
    P = R.problem(name)
    n, b = P["n"], P["b"]
    U, V, _ = R.update(name, 2, "cols")
    F = smlu.ParallelSparseLU(P["A"], refine=0)
    L = C.lib()
    F.lowrank_set(U, V)
    want = [F.solve_lowrank(b, trans=op) for op in ("N", "T")]
    tp = F.stat("solve_trans_passes")
    ci = C.SmluLowrankInfo()
    W = np.ones((n, 33), order="F")
    for k, pu, ldu, pv, ldv in ((33, W, n, W, n), (-1, W, n, W, n), (2, None, n, W, n), (2, W, n, None, n),
                                (2, W, n - 1, W, n), (2, W, n, W, n - 1)):
        assert L.smlu_lowrank_set(F._h, k, C.ptr(pu), ldu, C.ptr(pv), ldv, ctypes.byref(ci)) == C.SMLU_ERR_ARG
        assert F.stat("lowrank_k") == 2, (k, ldu, ldv)
    for (xw, iw), op in zip(want, ("N", "T")):
        x, info = F.solve_lowrank(b, trans=op)
        assert np.array_equal(x, xw) and info == iw
    assert F.stat("solve_trans_passes") - tp == want[1][1].solves      # Yt was kept too
    Un = U.copy()
    Un[0, 0] = np.inf
    assert F.lowrank_set(Un, V).status == C.SMLU_SINGULAR and F.stat("lowrank_k") == 0
    F.close()


def test_complex_handle_is_a_state_error(gpu):
    A = helmholtz3d(6, 0.5)
    F = smlu.ParallelSparseLU(A)
    n = A.shape[0]
    W = np.ones((n, 2))
    for call in (lambda: F.lowrank_set(W, W), lambda: F.solve_lowrank(np.ones(n))):
        with pytest.raises(smlu.SmluError) as e:
            call()
        assert e.value.code == C.SMLU_ERR_STATE and "ComplexF64" in str(e.value)
    # the library itself refuses too (2 n doubles per column: the leading dimensions pass)
    W2 = np.ones((2 * n, 2), order="F")
    ci = C.SmluLowrankInfo()
    L = C.lib()
    assert L.smlu_lowrank_set(F._h, 2, C.ptr(W2), 2 * n, C.ptr(W2), 2 * n, ctypes.byref(ci)) == C.SMLU_ERR_STATE
    v = np.ones(2 * n)
    assert L.smlu_solve_lowrank(F._h, C.SMLU_OP_N, -1, C.ptr(v), C.ptr(v), ctypes.byref(ci)) == C.SMLU_ERR_STATE
    assert "ComplexF64" in C.last_error(F._h)
    x = np.empty(n, dtype=complex)
    smlu.ldiv_(x, F, np.ones(n, dtype=complex))               # the handle still solves
    assert np.abs(A @ x - 1.0).max() < 1e-10
    F.close()
