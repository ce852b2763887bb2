"""The C ABI as the Julia drop-in calls it: index_base left at the library's default of 1, 1-based
colptr / rowval, and UMFPACK's 1-based p, q and L/U patterns for smlu_create_with_pivots.  Every
other GPU test reaches the library through the Python mirror, which always sets index_base = 0.

Each 1-based handle is made by raw ctypes calls (_capi_raw.py) and compared with a twin: the
mirror's 0-based handle of the same matrix and options.  Index arrays that cross the ABI must be
exactly the twin's plus 1, values bitwise the twin's (np.array_equal), and the exports the header
declares 0-based (smlu_get_fronts, smlu_plan_*, smlu_last_error_col) must not move.  The twin is tied
to the oracle by factor_parity, the given-pivot handles to the committed fixtures at the tolerances of
test_gpu_reference_suite.py (factors 1e-11 max(1, max|R|), solution rtol 1e-10 / atol 1e-12), the
complex solves to scipy's at the ctol of test_gpu_complex.py.

Measured on the MI355X (worst differences per handle; "0" is bitwise):

  handle (1-based)                  index arrays   values vs twin   vs fixture / scipy
  smlu_create       fe_8            twin + 1       0                -
  smlu_create       dense_13        twin + 1       0                -
  smlu_create       random_dom_200  twin + 1       0                -
  smlu_create       poisson2d_16    twin + 1       0                -
  smlu_create_i32   (the same four) twin + 1       0                -
  with_pivots       fe_8            given + 1      -                L 2.1e-14  U 1.5e-15  x 4.3e-14
  with_pivots       dense_13        given + 1      -                L 8.6e-16  U 1.7e-16  x 1.0e-15
  with_pivots       random_dom_200  given + 1      -                L 5.6e-17  U 1.1e-16  x 2.5e-16
  with_pivots       poisson2d_16    given + 1      -                L 8.9e-16  U 5.6e-16  x 8.5e-16
  smlu_create_z     helmholtz3d(6)  twin + 1       0                x 6.4e-16 (ctol 1e-12)
  refactor_csc[_z]  same / changed  twin + 1       0                -

(L, U: max |G - R| / max(1, max|R|); x: |x - x_ref| / |x_ref|.)

Found while writing these tests, by reading the code, and fixed with them: smlu_last_error_col returned the
pivot POSITION of the zero pivot (first column of its front + offset), not the caller's column -- the two
agree only under the natural order; it now maps the position through q.  A 0-based colptr under base 1
was refused only after the zero-free-diagonal scan had indexed rowval with colptr[0] - 1 = -1; the check
now comes first, in smlu_create* and in the re-analysing branch of smlu_refactor_csc.

Breaking the library on purpose makes these tests fail (tried on the MI355X, then reverted): without
"- base" in refactor_csc_impl's comparison test_refactor_csc_one_based fails ("a same-pattern lu!
re-analysed"); with p emitted without "+ b" every test_create_one_based_against_the_zero_based_twin fails."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle as O
import smlu
from smlu import _lib as C

import _capi_raw as R
from _parity import factor_parity, isapprox
from test_gpu_complex import crand, ctol, helmholtz3d

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["fe_8", "dense_13", "random_dominant_200", "poisson2d_16"]
# factor_parity's rtol as test_gpu_parity.py has it for the same kinds of matrix (FE and dense 1e-10,
# random dominant 1e-11, Poisson 1e-12)
PARITY_RTOL = {"fe_8": 1e-10, "dense_13": 1e-10, "random_dominant_200": 1e-11, "poisson2d_16": 1e-12}


def fixture(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)
    n = int(z["n"])
    A = R.csc(sp.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=(n, n)))
    return z, n, A


def fixture_LU(z, n):
    L = sp.csc_matrix((z["L_data"], z["L_indices"], z["L_indptr"]), shape=(n, n))
    U = sp.csc_matrix((z["U_data"], z["U_indices"], z["U_indptr"]), shape=(n, n))
    return R.csc(L), R.csc(U)


def with_two_entries(A, v1, v2):
    """The changed pattern of test_complex_refactor_same_and_new_pattern: (0, n-1) and (n-1, 0) added."""
    n = A.shape[0]
    A3 = A.tolil()
    assert A3[0, n - 1] == 0 and A3[n - 1, 0] == 0
    A3[0, n - 1] = v1
    A3[n - 1, 0] = v2
    A3 = R.csc(A3)
    assert A3.nnz == A.nnz + 2
    return A3


# ---- 1. smlu_create / smlu_create_i32 ----------------------------------------------------------------
@pytest.mark.parametrize("entry", ["smlu_create", "smlu_create_i32"])
@pytest.mark.parametrize("name", FIXTURES)
def test_create_one_based_against_the_zero_based_twin(gpu, name, entry):
    z, n, A = fixture(name)
    rc, h = R.create(A, base=1, entry=entry)
    assert rc == C.SMLU_OK and h.value, C.last_error(None)
    F = smlu.ParallelSparseLU(A, int32_indices=entry == "smlu_create_i32")
    try:
        R.assert_factors_shifted(R.factors(h), R.mirror_factors(F), 1)
        # the exports the header declares 0-based
        f1, f0 = R.fronts(h), F.fronts()
        for k in f0:
            assert np.array_equal(f1[k], f0[k]), k
        rng = np.random.default_rng(n)
        b = rng.random(n)
        for trans in ("N", "T"):
            x0 = np.empty(n)
            smlu.ldiv_(x0, F, b, trans=trans)
            assert np.array_equal(R.solve(h, b, trans), x0), trans
        B = np.asfortranarray(rng.random((n, 5)))
        X0 = np.empty_like(B)
        smlu.ldiv_(X0, F, B)
        assert np.array_equal(R.solve_multi(h, B), X0)
        factor_parity(A, F, rtol=PARITY_RTOL[name])   # ties both to the oracle
    finally:
        R.destroy(h)
        F.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_plan_exports_stay_zero_based(gpu, name):
    z, n, A = fixture(name)
    o = R.raw_opts(1)
    cp, ri = A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1
    ph = ctypes.c_void_p()
    L = C.lib()
    assert L.smlu_plan_create(n, C.ptr(cp), C.ptr(ri), ctypes.byref(o), ctypes.byref(ph)) == C.SMLU_OK
    try:
        P0 = smlu.Plan(A)
        ns = int(L.smlu_plan_stat(ph, b"nsuper"))
        assert ns == int(P0.stat("nsuper"))
        q, Lp = np.empty(n, np.int64), np.empty(n + 1, np.int64)
        assert L.smlu_plan_pattern(ph, C.ptr(q), C.ptr(Lp), None) == C.SMLU_OK
        Li = np.empty(Lp[-1], np.int64)
        assert L.smlu_plan_pattern(ph, None, None, C.ptr(Li)) == C.SMLU_OK
        L0 = P0.L_pattern()
        assert np.array_equal(q, P0.q()) and np.array_equal(Lp, L0.indptr) and np.array_equal(Li, L0.indices)
        first, parent, level = np.empty(ns + 1, np.int64), np.empty(ns, np.int64), np.empty(ns, np.int64)
        assert L.smlu_plan_supernodes(ph, C.ptr(first), C.ptr(parent), C.ptr(level)) == C.SMLU_OK
        for a, b in zip((first, parent, level), P0.supernodes()):
            assert np.array_equal(a, b)
        rowptr = np.empty(ns + 1, np.int64)
        assert L.smlu_plan_fronts(ph, C.ptr(rowptr), None, None) == C.SMLU_OK
        rows, p0 = np.empty(rowptr[-1], np.int64), np.empty(n, np.int64)
        assert L.smlu_plan_fronts(ph, None, C.ptr(rows), C.ptr(p0)) == C.SMLU_OK
        for a, b in zip((rowptr, rows, p0), P0.fronts()[2:]):
            assert np.array_equal(a, b)
    finally:
        L.smlu_plan_destroy(ph)


# ---- 2. smlu_create_with_pivots ----------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_with_pivots_one_based(gpu, name):
    z, n, A = fixture(name)
    Lf, Uf = fixture_LU(z, n)
    pat = R.pattern_args(Lf, Uf, 1)
    rc, h = R.create(A, base=1, entry="smlu_create_with_pivots", p=z["p"], q=z["q"], Rs=z["Rs"], pattern=pat)
    assert rc == C.SMLU_OK and h.value, C.last_error(None)
    try:
        assert R.stat(h, "given_pattern") == 1 and R.stat(h, "pattern_dropped") == 0
        f = R.factors(h)
        assert np.array_equal(f["p"], z["p"] + 1) and np.array_equal(f["q"], z["q"] + 1)
        assert np.array_equal(f["Rs"], z["Rs"])
        worst = {}
        for nm, Rm in (("L", Lf), ("U", Uf)):
            assert np.array_equal(f[nm + "p"], Rm.indptr.astype(np.int64) + 1), "colptr is not the given one + 1"
            assert np.array_equal(f[nm + "i"], Rm.indices.astype(np.int64) + 1), "rowval is not the given one + 1"
            worst[nm] = abs(f[nm + "x"] - Rm.data).max() / max(1.0, abs(Rm.data).max())
        x = R.solve(h, np.ascontiguousarray(z["b"], dtype=np.float64))
        dx = np.linalg.norm(x - z["x"]) / np.linalg.norm(z["x"])
        print(f"with_pivots 1-based {name}: L {worst['L']:.2e} U {worst['U']:.2e} x {dx:.2e}")
        assert worst["L"] <= 1e-11 and worst["U"] <= 1e-11
        np.testing.assert_allclose(x, z["x"], rtol=1e-10, atol=1e-12)
    finally:
        R.destroy(h)
    # Rs = NULL: the library's own SUM scaling
    rc, h = R.create(A, base=1, entry="smlu_create_with_pivots", p=z["p"], q=z["q"], pattern=pat)
    assert rc == C.SMLU_OK and h.value, C.last_error(None)
    try:
        assert np.array_equal(R.factors(h)["Rs"], O.rowscale(A))
    finally:
        R.destroy(h)


def test_with_pivots_error_paths(gpu):
    z, n, A = fixture("poisson2d_16")
    Lf, Uf = fixture_LU(z, n)
    kw = dict(entry="smlu_create_with_pivots", p=z["p"], q=z["q"], Rs=z["Rs"])
    # one L entry outside the structural fill of (Rs.*A)[p, q]
    Ld = Lf.toarray() != 0
    i, j = np.argwhere(~Ld & np.tri(n, k=-1, dtype=bool))[0]
    L2 = Lf.tolil()
    L2[i, j] = 1.0
    rc, h = R.create(A, base=1, pattern=R.pattern_args(L2, Uf, 1), **kw)
    assert rc == C.SMLU_ERR_PATTERN and not h.value
    # a 0-based colptr under base 1
    rc, h = R.create(A, base=1, shift=0, pattern=R.pattern_args(Lf, Uf, 1), **kw)
    assert rc == C.SMLU_ERR_ARG and not h.value
    rc, h = R.create(A, base=1, shift=0)
    assert rc == C.SMLU_ERR_ARG and not h.value
    # a 0-based L pattern under base 1: refused, no handle
    rc, h = R.create(A, base=1, pattern=R.pattern_args(Lf, Uf, 0), **kw)
    assert rc < 0 and not h.value
    assert C.last_error(None)
    # and the right call still works afterwards
    rc, h = R.create(A, base=1, pattern=R.pattern_args(Lf, Uf, 1), **kw)
    assert rc == C.SMLU_OK and h.value
    R.destroy(h)


# ---- 3. smlu_refactor_csc ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random_dominant_200", "poisson2d_16"])
def test_refactor_csc_one_based(gpu, name):
    z, n, A = fixture(name)
    rng = np.random.default_rng(3)
    rc, h = R.create(A, base=1)
    assert rc == C.SMLU_OK and h.value
    F = smlu.ParallelSparseLU(A)
    F3 = None
    try:
        # same pattern, new values: the `same` branch, i.e. smlu_refactor
        A2 = A.copy()
        A2.data = A.data * (1 + 0.3 * rng.random(A.nnz))
        t0 = R.stat(h, "analysis_ms")
        assert R.refactor_csc(h, A2, base=1) == C.SMLU_OK, C.last_error(h)
        assert R.stat(h, "analysis_ms") == t0, "a same-pattern lu! re-analysed"
        F.refactor(A2.data)
        assert R.stat(h, "mode_refactors") == F.stat("mode_refactors")
        R.assert_factors_shifted(R.factors(h), R.mirror_factors(F), 1)
        factor_parity(A2, F, rtol=PARITY_RTOL[name])
        # two entries added: re-analysis; equal to a fresh 0-based handle of the new matrix
        A3 = with_two_entries(A2, -0.25, -0.125)
        assert R.refactor_csc(h, A3, base=1) == C.SMLU_OK, C.last_error(h)
        assert R.stat(h, "nnzA") == A3.nnz
        F3 = smlu.ParallelSparseLU(A3)
        R.assert_factors_shifted(R.factors(h), R.mirror_factors(F3), 1)
        factor_parity(A3, F3, rtol=PARITY_RTOL[name])
        b = rng.random(n)
        x0 = np.empty(n)
        smlu.ldiv_(x0, F3, b)
        assert np.array_equal(R.solve(h, b), x0)
        # a 0-based pattern is not this handle's pattern and is not a 1-based matrix: refused, handle intact
        assert R.refactor_csc(h, A3, base=0) == C.SMLU_ERR_ARG
        assert np.array_equal(R.solve(h, b), x0)
    finally:
        R.destroy(h)
        F.close()
        if F3 is not None:
            F3.close()


# ---- 4. ComplexF64 -----------------------------------------------------------------------------------
def test_complex_one_based(gpu):
    rng = np.random.default_rng(6)
    A = helmholtz3d(6, 0.5)
    n = A.shape[0]
    rc, h = R.create(A, base=1, entry="smlu_create_z")
    assert rc == C.SMLU_OK and h.value, C.last_error(None)
    F = smlu.ParallelSparseLU(A)
    F3 = None

    def check(Fz, Az, what):
        R.assert_factors_shifted(R.factors(h, z=True), R.mirror_factors(Fz, z=True), 1)
        R.assert_factors_shifted(R.factors(h), R.mirror_factors(Fz), 1)   # K's factors, 2n rows
        b = crand(rng, n)
        x = R.solve(h, b.view(np.float64)).view(np.complex128)
        x0 = np.empty(n, np.complex128)
        smlu.ldiv_(x0, Fz, b)
        assert np.array_equal(x, x0)
        xs = spla.spsolve(Az.tocsc(), b)
        print(f"complex 1-based {what}: |x - xs| / |xs| = {np.linalg.norm(x - xs) / np.linalg.norm(xs):.2e}, "
              f"ctol {ctol(Az):.1e}")
        assert isapprox(x, xs, ctol(Az), ctol(Az))

    try:
        assert R.stat(h, "complex") == 1
        check(F, A, "create_z")
        factor_parity(O.real_equivalent(A), F, rtol=1e-10)
        A2 = A.copy()
        A2.data = A.data * (1 + 0.3 * crand(rng, A.nnz))
        t0 = R.stat(h, "analysis_ms")
        assert R.refactor_csc(h, A2, base=1, z=True) == C.SMLU_OK, C.last_error(h)
        assert R.stat(h, "analysis_ms") == t0, "a same-pattern lu! re-analysed"
        F.refactor(A2.data)
        check(F, A2, "refactor_csc_z same pattern")
        A3 = with_two_entries(A2, 0.01 + 0.02j, -0.01j)
        assert R.refactor_csc(h, A3, base=1, z=True) == C.SMLU_OK, C.last_error(h)
        F3 = smlu.ParallelSparseLU(A3)
        check(F3, A3, "refactor_csc_z changed pattern")
        factor_parity(O.real_equivalent(A3), F3, rtol=1e-10)
    finally:
        R.destroy(h)
        F.close()
        if F3 is not None:
            F3.close()


# ---- 5. smlu_last_error_col --------------------------------------------------------------------------
@pytest.mark.parametrize("j", [0, 37, 255])
def test_last_error_col_real(gpu, j):
    z, n, A = fixture("poisson2d_16")
    A = A.tolil()
    A[:, j] = 0.0
    A = R.csc(A)
    A.eliminate_zeros()
    assert A.indptr[j] == A.indptr[j + 1]
    rc, h = R.create(A, base=1)
    try:
        assert rc == C.SMLU_SINGULAR and h.value
        assert C.lib().smlu_last_error_col(h) == j      # 0-based, as the header states
    finally:
        R.destroy(h)
    with pytest.raises(smlu.SingularException) as ei:   # the mirror reports the same column
        smlu.ParallelSparseLU(A)
    assert ei.value.info == j


@pytest.mark.parametrize("j", [4, 130])
def test_last_error_col_complex(gpu, j):
    A = helmholtz3d(6, 0.5).tolil()
    A[:, j] = 0.0
    A = R.csc(A)
    A.eliminate_zeros()
    rc, h = R.create(A, base=1, entry="smlu_create_z")
    try:
        assert rc == C.SMLU_SINGULAR and h.value
        assert C.lib().smlu_last_error_col(h) == j      # the complex column, not K's
    finally:
        R.destroy(h)


# ---- the mirror's own index_base keyword -------------------------------------------------------------
def test_mirror_index_base_keyword(gpu):
    """smlu.ParallelSparseLU(A, index_base=1) passes 1-based arrays and stays 0-based on its Python side:
    everything it returns equals the 0-based handle's, through a pattern change as well."""
    z, n, A = fixture("poisson2d_16")
    with pytest.raises(ValueError):
        smlu.ParallelSparseLU(A, index_base=2)
    F1, F0 = smlu.ParallelSparseLU(A, index_base=1), smlu.ParallelSparseLU(A)
    try:
        assert F1._opts.index_base == 1 and F0._opts.index_base == 0
        R.assert_factors_shifted(R.factors(F1._h), R.mirror_factors(F0), 1)   # what crossed the ABI
        R.assert_factors_shifted(R.mirror_factors(F1), R.mirror_factors(F0), 0)
        for a, b in zip(F1.perm_scale(), F0.perm_scale()):
            assert np.array_equal(a, b)
        A3 = with_two_entries(A, -0.25, -0.125)
        smlu.lu_(F1, A3)
        smlu.lu_(F0, A3)
        assert F1.stat("nnzA") == A3.nnz
        R.assert_factors_shifted(R.mirror_factors(F1), R.mirror_factors(F0), 0)
        Lf, Uf = fixture_LU(z, n)
        G = smlu.ParallelSparseLU(A, p=z["p"], q=z["q"], L_pattern=Lf, U_pattern=Uf, index_base=1)
        assert G.stat("given_pattern") == 1 and np.array_equal(G.p, z["p"]) and np.array_equal(G.q, z["q"])
        assert np.array_equal(G.L.indices, Lf.indices) and np.array_equal(G.U.indptr, Uf.indptr)
        G.close()
    finally:
        F1.close()
        F0.close()
