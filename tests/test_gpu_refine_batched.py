"""Batched iterative refinement (smlu_solve_refined_multi[_device]; solve_refined_multi_device,
ldiv_refined_): up to 16 right-hand sides share every solve pass and every residual pass, each column
stops by the rule of the single refined solve.

Two oracles, as in test_gpu_solve_batched.py.  Column j of a call must be bitwise solve_device of that
column alone on a handle with the same step limit, and its info entry the three refine_* stats read
after that single solve; and every returned column is held against a reference that is not the
library (scipy's spsolve, the componentwise backward error in extended precision of
tests/_batch_ref.py).  Every call asserts through the stats that the batch path ran:
"solve_passes" / "solve_trans_passes" grow by 1 + the largest step count of each batch of 16 and
"refine_batch_residuals" by the residual rounds of each batch, the largest over its columns of
steps + 1 (a column that met its step limit: steps).  Outputs start as NaN.

Matrices, under the default options unless a test says otherwise: nondominant_fe_300 (unrefined
backward error 6e-14: a random column needs a correction), tile_pivoting_700_5 (row exchanges,
n = 700: three workgroups of rows, the last ragged), dense_13 (one partial wave), complex_tile_150
(the conj path, 2n interleaved doubles) and poisson3d_12 (dominant: nothing is refined).

The reported backward error against numpy's (test_independent_check).  The library sums a row's
residual in fp64 in A's entry order, numpy in extended precision, so the two differ by the rounding
of that sum, a few unit roundoffs times the row's |A||x| + |b|: under FLOOR = 2^-51 both are rounding
and anything agrees; above it they must agree within FACTOR = 4 either way, the rule _batch_ref
applies to two backward errors of one system.  A complex handle measures its error on the
real-equivalent system, componentwise in (re, im), so numpy's is taken there too.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle as O
import smlu
from smlu import _lib as C
from smlu import matrices as mats

from _batch_ref import FACTOR, FLOOR, assert_batch_against_oracle, berr, complex_tile_150, op_matrix
from _parity import TOL, tile_pivoting_matrix
from test_gpu_solve_trans import load_golden
from test_gpu_solve_trans_batched import _rhs, nondominant_fe

pytestmark = pytest.mark.gpu

MATRICES = {
    "nondominant_fe_300": nondominant_fe,
    "tile_pivoting_700_5": lambda: tile_pivoting_matrix(700, 5),
    "dense_13": lambda: load_golden("dense_13"),
    "complex_tile_150": complex_tile_150,
    "poisson3d_12": lambda: mats.poisson3d(12),
}
REFINING = ["nondominant_fe_300", "tile_pivoting_700_5", "dense_13", "complex_tile_150"]
WIDTHS = (1, 2, 4, 5, 8, 9, 16, 17, 33)
EPS4 = 2.0 ** -51


@pytest.fixture(scope="module")
def handles(gpu):
    """(name, options) -> (A, F), each factored once per module."""
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            A = sp.csc_matrix(MATRICES[name]())
            cache[key] = (A, smlu.ParallelSparseLU(A, **kw))
        return cache[key]

    yield get
    for _, F in cache.values():
        F.close()


def single(F, bj, trans):
    """solve_device of one column and what the handle says about its refinement."""
    import torch
    xj = torch.full_like(bj, float("nan"))
    F.solve_device(xj, bj, trans=trans)
    return xj, (int(F.stat("refine_steps")), F.stat("refine_berr"), F.stat("refine_residual"))


def singles_of(F, B, trans):
    return [single(F, B[j].contiguous(), trans) for j in range(B.shape[0])]


def batches(v):
    return [v[j:j + 16] for j in range(0, len(v), 16)]


def expected_passes(info):
    return sum(1 + int(s.max()) for s in batches(info["steps"]))


def expected_rounds(info):
    """Residual launches: per batch the most any column took part in, steps + 1 for a column that
    stopped by its backward error, steps for one that met the step limit, none when not refined."""
    rounds = info["steps"] + np.isin(info["stop"], (1, 2))
    return sum(int(r.max()) for r in batches(rounds))


def refined(F, B, trans, steps=None, X=None):
    """One solve_refined_multi_device call into X (NaN before) with the counters of the batch path."""
    import torch
    if X is None:
        X = torch.full_like(B, float("nan"))
    key = "solve_passes" if trans == "N" else "solve_trans_passes"
    other = "solve_trans_passes" if trans == "N" else "solve_passes"
    p0, o0, r0 = F.stat(key), F.stat(other), F.stat("refine_batch_residuals")
    info = F.solve_refined_multi_device(X, B, trans=trans, steps=steps)
    assert F.stat(key) - p0 == expected_passes(info), (F.stat(key) - p0, info["steps"])
    assert F.stat(other) == o0
    assert F.stat("refine_batch_residuals") - r0 == expected_rounds(info), (info["steps"], info["stop"])
    assert F.stat("status_copy_retries") == 0
    check_info(F, info)
    return X, info


def check_info(F, info):
    """What a call's info says by itself, and the handle's stats after it: the maxima."""
    st, sp_, be, re_ = info["steps"], info["stop"], info["berr"], info["resid"]
    assert ((sp_ >= 0) & (sp_ <= 3)).all()
    assert ((sp_ == 0) == (be == -1)).all() and ((sp_ == 0) == (re_ == -1)).all()
    assert (st[sp_ == 0] == 0).all()
    assert (be[sp_ == 1] <= EPS4).all() and (be[np.isin(sp_, (2, 3))] > EPS4).all()
    if len(st):
        assert F.stat("refine_steps") == st.max()
        assert F.stat("refine_berr") == be.max() and F.stat("refine_residual") == re_.max()


def assert_columns(X, info, singles, label=""):
    import torch
    for j, (xj, (steps, be, resid)) in enumerate(singles):
        assert torch.equal(X[j], xj), (label, j, (X[j] - xj).abs().max().item())
        got = (int(info["steps"][j]), float(info["berr"][j]), float(info["resid"][j]))
        assert got == (steps, be, resid), (label, j, got, (steps, be, resid))


# ---- 1. bitwise against singles ------------------------------------------------------------------
@pytest.fixture(scope="module")
def columns33(handles):
    """(name, trans) -> 33 right-hand sides and their single refined solves, computed once."""
    cache = {}

    def get(name, trans):
        if (name, trans) not in cache:
            A, F = handles(name)
            B = _rhs(F.n, 33, 300, F.is_complex)
            cache[(name, trans)] = (B, singles_of(F, B, trans))
        return cache[(name, trans)]

    return get


@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_bitwise_against_singles(handles, columns33, name, trans):
    """Every width: the batch is the last nrhs of the 33 columns, so a slot holds another column at
    every width; 17 ends in a one-column batch, 33 is three batches."""
    A, F = handles(name)
    B, singles = columns33(name, trans)
    steps1 = [s[1][0] for s in singles]
    print(f"{name} {trans}: single refined solves took {sorted(set(steps1))} steps")
    if name in REFINING:
        assert F.stat("dominant") == 0 and max(steps1) >= 1
    for nrhs in WIDTHS:
        X, info = refined(F, B[33 - nrhs:].contiguous(), trans)
        assert_columns(X, info, singles[33 - nrhs:], (name, trans, nrhs))
        if name == "poisson3d_12":   # dominant: max_steps = -1 is a plain batch
            assert (info["steps"] == 0).all() and (info["stop"] == 0).all() and (info["berr"] == -1).all()


# ---- 2. masking ----------------------------------------------------------------------------------
def masking_batch(A, F, trans, k=5):
    """Seven columns: random, zero, b = op(A) e_k, four random."""
    import torch
    Bh = np.random.default_rng(310).random((7, F.n))
    Bh[1] = 0.0
    Bh[2] = np.asarray(op_matrix(A, trans)[:, k].todense()).ravel()
    return torch.from_numpy(Bh).to("cuda:0")


def check_masking(A, F, trans, distinct):
    import torch
    B = masking_batch(A, F, trans)
    singles = singles_of(F, B, trans)
    steps1 = [s[1][0] for s in singles]
    print(f"masking {trans}: single step counts {steps1}")
    assert len(set(steps1)) >= distinct and 0 in steps1 and max(steps1) >= 1, steps1
    X, info = refined(F, B, trans)
    assert_columns(X, info, singles, ("masking", trans))
    assert (X[1] == 0).all()
    assert info["steps"][1] == 0 and info["berr"][1] == 0 and info["stop"][1] == 1
    assert torch.isfinite(X).all()
    return info


@pytest.mark.parametrize("trans", ["N", "T"])
@pytest.mark.parametrize("name", ["nondominant_fe_300", "tile_pivoting_700_5"])
def test_masking(handles, name, trans):
    """Columns that stop at different rounds in one batch: the stopped ones keep their bits while the
    others go on, and the counters are those of the longest column."""
    A, F = handles(name)
    check_masking(A, F, trans, 2)


@pytest.mark.parametrize("trans", ["N", "T"])
def test_masking_three_step_counts(handles, trans):
    """tile_pivoting_700_5 under diag_pivot_tol = 1e-6 (growth 8.7e5 instead of 9.3e2): the zero column
    takes 0 corrections, the random ones 1 and b = op(A) e_k, whose solution is one nonzero among
    rounding-sized entries, 2 -- three rounds at which columns leave the batch.  (Measured on an
    MI355X; the default handles spread as far: 0, 1, 2 on this matrix and 0, 1, 3 on nondominant_fe_300,
    where that column meets the step limit.)"""
    A, F = handles("tile_pivoting_700_5", diag_pivot_tol=1e-6)
    check_masking(A, F, trans, 3)


# ---- 3. max_steps --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ["nondominant_fe_300", "tile_pivoting_700_5"])
def test_explicit_step_limit_equals_a_handle_with_that_limit(handles, name, k):
    """Factors are deterministic, so a refine=k handle's single solves are the reference of an explicit
    max_steps = k on a refine=0 handle."""
    A, F0 = handles(name, refine=0)
    _, Fk = handles(name, refine=k)
    B = _rhs(F0.n, 5, 320 + k)
    for trans in ("N", "T"):
        X, info = refined(F0, B, trans, steps=k)
        assert_columns(X, info, singles_of(Fk, B, trans), (name, trans, k))
        assert info["steps"].max() >= 1 and info["steps"].max() <= k


@pytest.mark.parametrize("name", ["nondominant_fe_300", "tile_pivoting_700_5"])
def test_zero_steps_is_the_plain_batch(handles, name):
    import torch
    A, F0 = handles(name, refine=0)
    _, F = handles(name)
    B = _rhs(F0.n, 17, 325)
    for trans in ("N", "T"):
        Xp = torch.full_like(B, float("nan"))
        F0.solve_multi_device(Xp, B, trans=trans)
        for Fh, steps in ((F0, 0), (F0, None), (F, 0)):   # explicit, the refine=0 handle's own rule, and over a default handle's
            X, info = refined(Fh, B, trans, steps=steps)
            assert torch.equal(X, Xp), (trans, steps)
            assert (info["steps"] == 0).all() and (info["stop"] == 0).all()
            assert (info["berr"] == -1).all() and (info["resid"] == -1).all()


# ---- 4. leading dimensions, aliasing, host form ---------------------------------------------------
def refined_raw(F, fn, op, steps, nrhs, pB, ldb, pX, ldx, info=None, stream_of=None):
    call = getattr(C.lib(), fn)
    args = (F._h, op, steps, nrhs, pB, ldb, pX, ldx, info)
    if stream_of is None:
        return call(*args)
    with C.caller_stream(F._h, stream_of):
        return call(*args)


def device_call(F, op, steps, nrhs, Bbuf, ldb, Xbuf, ldx, info=None):
    return refined_raw(F, "smlu_solve_refined_multi_device", op, steps, nrhs, ctypes.c_void_p(Bbuf.data_ptr()), ldb,
                       ctypes.c_void_p(Xbuf.data_ptr()), ldx, info, stream_of=Bbuf)


def padded(Bc, ld):
    """The rows of Bc at pitch ld in one flat buffer, NaN in the padding."""
    import torch
    nr, n = Bc.shape
    buf = torch.full((nr * ld,), float("nan"), dtype=torch.float64, device="cuda:0")
    buf.view(nr, ld)[:, :n] = Bc
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("trans", ["N", "T"])
@pytest.mark.parametrize("name", ["nondominant_fe_300", "tile_pivoting_700_5"])
def test_leading_dimensions_and_aliasing(handles, name, trans):
    import torch
    A, F = handles(name)
    n, nrhs = F.n, 17
    op = {"N": C.SMLU_OP_N, "T": C.SMLU_OP_T}[trans]
    Bc = _rhs(n, nrhs, 330)
    Xc, info_c = refined(F, Bc, trans)
    ldb, ldx = n + 3, n + 7
    Bbuf = padded(Bc, ldb)
    Xbuf = torch.full((nrhs * ldx,), float("nan"), dtype=torch.float64, device="cuda:0")
    info = (C.SmluRefineInfo * nrhs)()
    assert device_call(F, op, -1, nrhs, Bbuf, ldb, Xbuf, ldx, info) == C.SMLU_OK
    Xv = Xbuf.view(nrhs, ldx)
    assert torch.equal(Xv[:, :n], Xc)
    assert torch.isnan(Xv[:, n:]).all()                      # the padding of X is never written
    assert torch.equal(Bbuf.view(nrhs, ldb)[:, :n], Bc)      # B is only read
    assert [i.steps for i in info] == list(info_c["steps"]) and [i.berr for i in info] == list(info_c["berr"])
    assert [i.stop for i in info] == list(info_c["stop"]) and [i.resid for i in info] == list(info_c["resid"])
    V = Bc.clone()                                           # X is B, contiguous
    Xa, info_a = refined(F, V, trans, X=V)
    assert torch.equal(V, Xc) and np.array_equal(info_a["steps"], info_c["steps"])
    ld = n + 5                                               # X is B at a pitch, info NULL
    Vbuf = padded(Bc, ld)
    assert device_call(F, op, -1, nrhs, Vbuf, ld, Vbuf, ld, None) == C.SMLU_OK
    Vv = Vbuf.view(nrhs, ld)
    assert torch.equal(Vv[:, :n], Xc) and torch.isnan(Vv[:, n:]).all()


@pytest.mark.parametrize("name", ["nondominant_fe_300", "complex_tile_150"])
def test_host_form_equals_device_form(handles, name):
    A, F = handles(name)
    for trans in ("N", "T", "C"):
        B = _rhs(F.n, 17, 335, F.is_complex)
        X, info = refined(F, B, trans)
        Bh = np.asfortranarray(B.cpu().numpy().T)   # n x 17, column-major
        Xh = np.full_like(Bh, np.nan)
        key = "solve_passes" if trans == "N" else "solve_trans_passes"
        p0 = F.stat(key)
        info_h = smlu.ldiv_refined_(Xh, F, Bh, trans=trans)
        assert F.stat(key) - p0 == expected_passes(info_h)
        assert np.array_equal(Xh, X.cpu().numpy().T)
        for k in ("steps", "stop", "berr", "resid"):
            assert np.array_equal(info_h[k], info[k]), (trans, k)
        check_info(F, info_h)
        V = Bh.copy(order="F")
        smlu.ldiv_refined_(V, F, V, trans=trans)    # in place on the host
        assert np.array_equal(V, Xh)


# ---- 5. independent check --------------------------------------------------------------------------
def numpy_berr(A, F, x, b, trans):
    """The backward error the library measures, recomputed in extended precision: of op(A) x = b, on
    the real-equivalent system for a complex handle (op T there: K^T on the conjugated vectors)."""
    if not F.is_complex:
        return berr(op_matrix(A, trans), x, b)
    K = sp.csc_matrix(O.real_equivalent(A))
    if trans == "T":
        x, b = np.conj(x), np.conj(b)
    Kop = K if trans == "N" else sp.csc_matrix(K.T)
    return berr(Kop, np.ascontiguousarray(x).view(np.float64), np.ascontiguousarray(b).view(np.float64))


@pytest.mark.parametrize("trans", ["N", "T", "C"])
@pytest.mark.parametrize("name", REFINING)
def test_independent_check(handles, name, trans):
    A, F = handles(name)
    B = _rhs(F.n, 5, 340, F.is_complex)
    X, info = refined(F, B, trans)
    Bh, Xh = B.cpu().numpy(), X.cpu().numpy()
    Op = sp.csc_matrix(op_matrix(A, trans))
    Xr = np.asarray(spla.spsolve(Op, np.ascontiguousarray(Bh.T))).T   # one factorization for the five columns
    assert_batch_against_oracle(A, F, Bh, Xh, trans, Xo=Xr, tol=TOL, label=f"{name} refined as a batch")
    for j in range(5):
        ref = numpy_berr(A, F, Xh[j], Bh[j], trans)
        got = float(info["berr"][j])
        print(f"{name} {trans} column {j}: steps {info['steps'][j]} stop {info['stop'][j]} "
              f"berr reported {got:.3e} numpy {ref:.3e}")
        if info["stop"][j] in (1, 2):   # the last measured error is the returned x's
            assert got <= max(FACTOR * ref, FLOOR) and ref <= max(FACTOR * got, FLOOR), (j, got, ref)


# ---- 6. the handle is left intact ------------------------------------------------------------------
def test_handle_left_intact(gpu, monkeypatch):
    import torch
    A = sp.csc_matrix(nondominant_fe())
    F = smlu.ParallelSparseLU(A)   # a fresh handle: the work buffers are allocated by the first call
    b = _rhs(F.n, 1, 350)[0].contiguous()
    B = _rhs(F.n, 9, 351)
    before = {t: single(F, b, t) for t in ("N", "T")}
    det, rc = F.logabsdet(), F.rcond("1")
    evals = F.stat("logabsdet_evals")
    out = {}
    for trans in ("N", "T"):
        out[trans] = refined(F, B, trans)
        x, st = single(F, b, trans)
        assert torch.equal(x, before[trans][0]) and st == before[trans][1]
    assert F.logabsdet() == det and F.stat("logabsdet_evals") == evals    # still the cached value
    assert F.rcond("1") == rc and F.stat("rcond_solves") == 0
    monkeypatch.setenv("SMLU_NO_GRAPH", "1")
    for trans in ("N", "T"):
        Xe, info_e = refined(F, B, trans)
        assert torch.equal(Xe, out[trans][0])
        assert np.array_equal(info_e["steps"], out[trans][1]["steps"])
        assert np.array_equal(info_e["berr"], out[trans][1]["berr"])
    monkeypatch.delenv("SMLU_NO_GRAPH")
    F.close()


# ---- 7. errors -------------------------------------------------------------------------------------
def test_argument_and_state_errors(handles):
    import torch
    A, F = handles("nondominant_fe_300")
    n = F.n
    B = _rhs(n, 3, 360)
    X = torch.full_like(B, float("nan"))
    stats = ("solve_passes", "solve_trans_passes", "refine_batch_residuals")
    s0 = [F.stat(k) for k in stats]
    N = C.SMLU_OP_N
    assert device_call(F, 3, -1, 3, B, n, X, n) == C.SMLU_ERR_ARG         # op
    assert device_call(F, -1, -1, 3, B, n, X, n) == C.SMLU_ERR_ARG
    assert device_call(F, N, -2, 3, B, n, X, n) == C.SMLU_ERR_ARG         # max_steps
    assert device_call(F, N, -1, 3, B, n - 1, X, n) == C.SMLU_ERR_ARG     # leading dimensions
    assert device_call(F, C.SMLU_OP_T, -1, 3, B, n, X, n - 1) == C.SMLU_ERR_ARG
    assert device_call(F, N, -1, -1, B, n, X, n) == C.SMLU_ERR_ARG        # nrhs
    null = ctypes.c_void_p(0)
    for fn in ("smlu_solve_refined_multi", "smlu_solve_refined_multi_device"):
        assert refined_raw(F, fn, N, -1, 3, null, n, ctypes.c_void_p(X.data_ptr()), n) == C.SMLU_ERR_ARG
        assert refined_raw(F, fn, N, -1, 3, ctypes.c_void_p(B.data_ptr()), n, null, n) == C.SMLU_ERR_ARG
        assert refined_raw(F, fn, N, -1, 0, null, n, null, n) == C.SMLU_OK   # nrhs = 0 needs no pointers
    assert C.last_error(F._h)
    for op in (N, C.SMLU_OP_T, C.SMLU_OP_H):
        assert device_call(F, op, -1, 0, B, n, X, n) == C.SMLU_OK          # nrhs = 0 touches nothing
    torch.cuda.synchronize()
    assert torch.isnan(X).all()
    assert [F.stat(k) for k in stats] == s0
    with pytest.raises(ValueError):
        F.solve_refined_multi_device(X, B, steps=-1)
    with pytest.raises(ValueError):
        F.solve_refined_multi_device(X, B, trans="X")
    with pytest.raises(smlu.DimensionMismatch):
        F.solve_refined_multi_device(X[:2], B)


def test_singular_create_is_a_state_error(gpu):
    """smlu_create of a singular matrix returns SMLU_SINGULAR with a handle that holds no usable
    factorization: the refined solve refuses it, as smlu_logabsdet does."""
    A = load_golden("poisson2d_16").tocsr()
    A.data[A.indptr[20]:A.indptr[21]] = 0.0   # row 20 zero (stored zeros)
    A = sp.csc_matrix(A.tocsc())
    A.sort_indices()
    n = A.shape[0]
    colptr, rowval = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    vals = np.ascontiguousarray(A.data, dtype=np.float64)
    L = C.lib()
    opts = C.default_opts(index_base=0)
    h = ctypes.c_void_p()
    assert L.smlu_create(n, C.ptr(colptr), C.ptr(rowval), C.ptr(vals), ctypes.byref(opts),
                         ctypes.byref(h)) == C.SMLU_SINGULAR
    assert h.value
    try:
        Bh = np.ones((n, 2), order="F")
        Xh = np.full_like(Bh, np.nan)
        for op in (C.SMLU_OP_N, C.SMLU_OP_T):
            assert L.smlu_solve_refined_multi(h, op, -1, 2, C.ptr(Bh), n, C.ptr(Xh), n, None) == C.SMLU_ERR_STATE
        assert np.isnan(Xh).all()
    finally:
        L.smlu_destroy(h)
