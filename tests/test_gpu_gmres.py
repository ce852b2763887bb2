"""GMRES preconditioned by stale factors on the GPU (smlu_solve_gmres*; F.gmres, F.gmres_device).

Reference: tests/_gmres_ref.py, a NumPy restatement of the same algorithm with an exact
preconditioner.  Each case runs at its input's own rtol, which tests/test_gmres_derivation.py shows to
lie a factor of 4 from the reference estimates on either side of the stop, so the iteration and cycle
counts must equal the restatement's.  Residuals are NumPy's own; gamma = (max entries per row + 2)
2^-52 || |A'||x| + |b| ||_2 / ||b||_2 is the rounding of evaluating one.

The partitioned-handle refusal needs two processes: tests/test_gpu_gmres_dist.py."""
import ctypes

import numpy as np
import pytest
import torch

import smlu
from smlu import _lib as C

import _gmres_ref as G
from _diag_ref import cond1, load_golden, rounding
from test_gpu_complex import helmholtz3d

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(gpu):
    """One factorization of the unperturbed A per input, shared by the tests of this module."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = smlu.ParallelSparseLU(G.problem(name)["A"])
        return cache[name]
    yield get
    for F in cache.values():
        F.close()


def run(F, name, op="N", restart=30, **kw):
    P = G.problem(name)
    kw.setdefault("rtol", G.rtol_of(name, restart))
    return F.gmres(P["b"], values=P["A2"], trans=op, restart=restart, **kw)


def check_residual(P, x, info, op, bound):
    g = G.gamma(P["A2"], x, P["b"], op)
    rr = G.relres(P["A2"], x, P["b"], op)
    print(f"  numpy relres {rr:.3e} info.relres {info.relres:.3e} est {info.relres_est:.3e} berr {info.berr:.2e} "
          f"gamma {g:.2e} bound {bound:.3e}")
    assert rr <= bound + g
    assert abs(info.relres - rr) <= 2 * g
    return rr, g


@pytest.mark.parametrize("name,op,restart", G.gpu_cases())
def test_converges_in_the_restatements_count(handles, name, op, restart):
    P = G.problem(name)
    R = G.reference(name, op, restart)
    F = handles(name)
    passes = F.stat("solve_trans_passes")
    x, info = run(F, name, op, restart)
    print(f"{name} op={op} restart={restart} n={P['n']}: rtol {G.rtol_of(name, restart):.3e} iters {info.iters} "
          f"(ref {R['iters']}) cycles {info.cycles} (ref {R['cycles']}) solves {info.solves} "
          f"ms {F.stat('gmres_ms_last'):.2f}")
    assert info.status == C.SMLU_OK and info.converged
    assert info.iters == R["iters"]
    assert info.cycles == R["cycles"]
    assert info.solves == info.iters + info.cycles
    check_residual(P, x, info, op, G.rtol_of(name, restart))
    assert info.bnorm == pytest.approx(np.linalg.norm(P["b"]), rel=1e-13)
    assert info.berr <= 1e-6 and np.isfinite(x).all()
    assert (F.stat("gmres_iters"), F.stat("gmres_cycles"), F.stat("gmres_solves")) == \
        (info.iters, info.cycles, info.solves)
    assert F.stat("gmres_ms_last") > 0
    # every preconditioner solve of a transposed run is a transposed pass pair
    assert F.stat("solve_trans_passes") - passes == (info.solves if op != "N" else 0)
    if name == "poisson3d_28+I":
        assert F.stat("solve_sweeps") > 0      # the handle really has large fronts


@pytest.mark.parametrize("name", ["dense_13", "fe_8", "random_dominant_200"])
@pytest.mark.parametrize("op", ["N", "T"])
def test_own_values_is_refinement(handles, name, op):
    """values = None: the factored system itself.  The first step's w = A M^-1 v_0 is v_0 to rounding,
    so h_{1,0} is rounding noise (a near-breakdown) and at most one more step follows."""
    P = G.problem(name)
    F = handles(name)
    b = P["b"]
    x, info = F.gmres(b, trans=op)
    xs = np.empty_like(b)
    smlu.ldiv_(xs, F, b, trans=op)
    Ad = P["A"].toarray()
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f"{name} op={op}: iters {info.iters} relres {info.relres:.2e} berr {info.berr:.2e} |x - ldiv| {err:.2e}")
    assert info.converged and info.status == C.SMLU_OK
    assert 1 <= info.iters <= 2
    assert np.isfinite(x).all() and np.isfinite([info.relres, info.relres_est, info.berr]).all()
    assert err <= rounding(P["n"], cond1(Ad))
    check_residual(dict(A2=P["A"], b=b), x, info, op, 1e-10)


def test_maxit_returns_the_last_iterate(handles):
    name = G.MAXIT_INPUT
    P = G.problem(name)
    A, A2 = P["A"].toarray(), P["A2"].toarray()
    rho = float(np.linalg.norm((A2 - A) @ np.linalg.inv(A), 2))
    F = handles(name)
    x, info = run(F, name, rtol=1e-14, maxiter=3)
    print(f"{name}: rho {rho:.3e} status {info.status} iters {info.iters} relres {info.relres:.3e}")
    assert info.status == C.SMLU_NOT_CONVERGED and not info.converged
    assert info.iters == 3 and info.cycles == 1 and info.solves == 4
    assert np.isfinite(x).all()
    rr, g = check_residual(P, x, info, "N", rho ** 3)
    assert rr <= rho ** 3
    # the C entry point returns the same positive status
    ci = C.SmluGmresInfo()
    o = C.SmluGmresOpts(1e-14, 30, 3)
    v = np.ascontiguousarray(P["A2"].data)
    x2 = np.empty_like(x)
    rc = C.lib().smlu_solve_gmres(F._h, C.SMLU_OP_N, C.ptr(v), C.ptr(P["b"]), C.ptr(x2), ctypes.byref(o),
                                  ctypes.byref(ci))
    assert rc == C.SMLU_NOT_CONVERGED and np.array_equal(x2, x)


@pytest.mark.parametrize("name", ["dense_13", "fe_5"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_values_leave_the_handle_usable(gpu, name, bad):
    """Odd n: the basis' leading dimension has a pad row.  A call whose values hold a NaN or an Inf stops
    with SMLU_NOT_CONVERGED; the pad must still be zero afterwards, so the next call on the same
    handle converges in the restatement's count."""
    P = G.problem(name)
    assert P["n"] % 2 == 1
    R = G.reference(name, "N", 30)
    F = smlu.ParallelSparseLU(P["A"])
    v = P["A2"].data.copy()
    v[v.size // 2] = bad
    for op in ("N", "T"):
        x, info = F.gmres(P["b"], values=v, trans=op, rtol=G.rtol_of(name), restart=4)
        print(f"{name} {bad} op={op}: status {info.status} iters {info.iters} relres {info.relres}")
        assert info.status == C.SMLU_NOT_CONVERGED and not info.converged
        assert np.isfinite(x).all()          # the last iterate: x0 = 0 or a finite cycle's result
    x, info = run(F, name)
    assert info.status == C.SMLU_OK and info.converged
    assert info.iters == R["iters"] and info.cycles == R["cycles"]
    check_residual(P, x, info, "N", G.rtol_of(name))
    F.close()


def test_device_form_checks_its_tensors(gpu):
    P = G.problem("dense_13")
    F = smlu.ParallelSparseLU(P["A"])
    n, nnz = P["n"], P["A"].nnz
    d = torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(smlu.DimensionMismatch):
        F.gmres_device(d, d, torch.zeros(nnz - 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(smlu.DimensionMismatch):
        F.gmres_device(d[:-1], d)
    with pytest.raises(TypeError):
        F.gmres_device(d, d.float())
    with pytest.raises(TypeError):
        F.gmres_device(d, torch.zeros(n, dtype=torch.float64))
    F.close()


def test_zero_right_hand_side(handles):
    name = "random_dominant_200"
    F = handles(name)
    n = G.problem(name)["n"]
    x, info = F.gmres(np.zeros(n), values=G.problem(name)["A2"], x=np.full(n, 7.0))
    assert info.converged and info.status == C.SMLU_OK
    assert (info.iters, info.cycles, info.solves) == (0, 0, 0)
    assert not x.any() and info.relres == 0.0 and info.bnorm == 0.0


@pytest.mark.parametrize("name", ["random_dominant_200@5e-2", "poisson2d_300+I"])
def test_aliasing_determinism_and_the_two_forms(handles, name):
    """x aliasing b, two identical calls, and the host and device forms: all bitwise equal."""
    P = G.problem(name)
    F = handles(name)
    rtol = G.rtol_of(name)
    x0, i0 = run(F, name)
    x1, i1 = run(F, name)
    assert np.array_equal(x0, x1) and i0 == i1
    xb = P["b"].copy()
    x2, i2 = F.gmres(xb, values=P["A2"], rtol=rtol, x=xb)      # host form, x is b
    assert x2 is xb and np.array_equal(x2, x0) and i2 == i0
    dv = torch.from_numpy(np.ascontiguousarray(P["A2"].data)).cuda()
    db = torch.from_numpy(P["b"]).cuda()
    dx = torch.empty_like(db)
    i3 = F.gmres_device(dx, db, dv, rtol=rtol)
    assert np.array_equal(dx.cpu().numpy(), x0) and i3 == i0
    assert np.array_equal(db.cpu().numpy(), P["b"])           # b is only read
    i4 = F.gmres_device(db, db, dv, rtol=rtol)                  # device form, x is b
    assert np.array_equal(db.cpu().numpy(), x0) and i4 == i0


def test_handle_is_left_as_it_was(gpu):
    name = "fe_8"
    P = G.problem(name)
    F = smlu.ParallelSparseLU(P["A"])
    b = P["b"]
    x0, x1 = np.empty_like(b), np.empty_like(b)
    smlu.ldiv_(x0, F, b)
    r0 = F.rcond("1", parts=True)
    la0 = F.logabsdet()
    evals = F.stat("logabsdet_evals")
    for op in ("N", "T"):
        _, info = F.gmres(b, values=P["A2"], trans=op, rtol=G.rtol_of(name))
        assert info.converged
    smlu.ldiv_(x1, F, b)
    assert np.array_equal(x0, x1)                 # same factors, same values, same work buffers' use
    assert F.rcond("1", parts=True) == r0
    assert F.stat("rcond_solves") == 0            # still the cached answer: no refactor happened
    assert F.logabsdet() == la0 and F.stat("logabsdet_evals") == evals
    # the handle's own values are still A's: refinement of the factored system converges at once
    _, info = F.gmres(b)
    assert info.converged and info.iters <= 2
    F.close()


def test_argument_and_state_errors(gpu):
    A = load_golden("poisson2d_16")
    F = smlu.ParallelSparseLU(A)
    L = C.lib()
    n = A.shape[0]
    b, x = np.sqrt(np.arange(1.0, n + 1.0)), np.empty(n)
    ci = C.SmluGmresInfo()

    def call(op=C.SMLU_OP_N, opts=None, pb=b, px=x):
        o = None if opts is None else ctypes.byref(C.SmluGmresOpts(*opts))
        return L.smlu_solve_gmres(F._h, op, None, C.ptr(pb), C.ptr(px), o, ctypes.byref(ci))
    assert call() == C.SMLU_OK and ci.converged == 1          # NULL opts: the defaults; NULL values: A's
    assert L.smlu_solve_gmres(F._h, C.SMLU_OP_N, None, C.ptr(b), C.ptr(x), None, None) == C.SMLU_OK   # NULL info
    assert call(op=3) == C.SMLU_ERR_ARG and call(op=-1) == C.SMLU_ERR_ARG
    for bad in ((1e-10, 0, 200), (1e-10, 33, 200), (1e-10, 30, 0), (-1.0, 30, 200), (float("nan"), 30, 200),
                (float("inf"), 30, 200)):
        assert call(opts=bad) == C.SMLU_ERR_ARG, bad
    assert call(pb=None) == C.SMLU_ERR_ARG and call(px=None) == C.SMLU_ERR_ARG
    assert call(opts=(0.0, 1, 1)) == C.SMLU_NOT_CONVERGED     # rtol = 0 is allowed and never met
    A2 = A.tocsr()
    A2.data[A2.indptr[20]:A2.indptr[21]] = 0.0                # a zero row: singular, same pattern
    A2 = A2.tocsc()
    with pytest.raises(smlu.SingularException):
        F.refactor(A2.data)
    assert call() == C.SMLU_ERR_STATE
    F.refactor(A.data)
    assert call() == C.SMLU_OK
    F.close()


def test_complex_handle_is_a_state_error(gpu):
    A = helmholtz3d(6, 0.5)
    F = smlu.ParallelSparseLU(A)
    n = A.shape[0]
    with pytest.raises(smlu.SmluError) as e:
        F.gmres(np.ones(n, dtype=complex))
    assert e.value.code == C.SMLU_ERR_STATE and "ComplexF64" in str(e.value)
    d = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    with pytest.raises(smlu.SmluError) as e:
        F.gmres_device(d, d)
    assert e.value.code == C.SMLU_ERR_STATE
    x = np.empty(n, dtype=complex)
    smlu.ldiv_(x, F, np.ones(n, dtype=complex))               # the handle still solves
    assert np.abs(A @ x - 1.0).max() < 1e-10
    F.close()
