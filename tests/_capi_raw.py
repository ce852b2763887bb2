"""Raw ctypes calls into libsmlu.so with the index base the caller chooses: what the Julia drop-in
does (it never sets index_base, so 1-based colptr / rowval / p / q / patterns go in and 1-based
factors come out), next to the Python mirror, which always passes index_base = 0.  Shared by
test_gpu_capi_one_based.py; nothing here computes anything, it only shifts index arrays by `base`
on the way in and returns the library's arrays untouched on the way out."""
import ctypes

import numpy as np
import scipy.sparse as sp

from smlu import _lib as C


def csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    A.sum_duplicates()
    return A


def raw_opts(base=1, **kw):
    """smlu_default_opts with index_base left as the library sets it (1, asserted); base=0 sets it."""
    o = C.default_opts(**kw)
    assert o.index_base == 1, "the library's default index base is Julia's"
    if base != 1:
        o.index_base = base
    return o


def _i64(a, base=0):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64) + base


def pattern_args(Lm, Um, base):
    """(Lcolptr, Lrowval, Ucolptr, Urowval) of two scipy matrices in the given base."""
    out = []
    for M in (Lm, Um):
        M = csc(M)
        out += [_i64(M.indptr, base), _i64(M.indices, base)]
    return out


def create(A, base=1, entry="smlu_create", opts=None, p=None, q=None, Rs=None, pattern=None, shift=None):
    """(rc, handle) of smlu_create / smlu_create_i32 / smlu_create_z / smlu_create_with_pivots on A
    with every index array shifted by `base` (shift: another shift for colptr and rowval, to hand a
    0-based matrix to a 1-based handle).  pattern: the four arrays of pattern_args, passed as
    they are.  p, q: 0-based, shifted here.  The caller destroys the handle (destroy(h))."""
    A = csc(A)
    n = A.shape[0]
    o = opts if opts is not None else raw_opts(base)
    sh = base if shift is None else shift
    it = np.int32 if entry == "smlu_create_i32" else np.int64
    cp = np.ascontiguousarray(A.indptr, dtype=it) + it(sh)
    ri = np.ascontiguousarray(A.indices, dtype=it) + it(sh)
    vals = np.ascontiguousarray(A.data, dtype=np.complex128 if entry == "smlu_create_z" else np.float64)
    h = ctypes.c_void_p()
    L = C.lib()
    if entry == "smlu_create_with_pivots":
        pat = pattern if pattern is not None else [None] * 4
        rs = None if Rs is None else np.ascontiguousarray(Rs, dtype=np.float64)
        pp, qq = _i64(p, base), _i64(q, base)   # named: C.ptr keeps no reference to its array
        rc = L.smlu_create_with_pivots(n, C.ptr(cp), C.ptr(ri), C.ptr(vals), C.ptr(pp), C.ptr(qq),
                                       C.ptr(rs), *[C.ptr(a) for a in pat], ctypes.byref(o), ctypes.byref(h))
    else:
        rc = getattr(L, entry)(n, C.ptr(cp), C.ptr(ri), C.ptr(vals), ctypes.byref(o), ctypes.byref(h))
    return rc, h


def destroy(h):
    if h is not None and h.value:
        C.lib().smlu_destroy(h)
        h.value = None


def stat(h, key):
    return C.lib().smlu_stat(h, key.encode())


def factors(h, z=False):
    """smlu_get_factors (z: smlu_get_factors_z) as the library writes them: dict of Lp, Li, Lx, Up,
    Ui, Ux, p, q, Rs (complex values as complex128)."""
    L = C.lib()
    n, nl, nu = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    sizes, get = (L.smlu_get_sizes_z, L.smlu_get_factors_z) if z else (L.smlu_get_sizes, L.smlu_get_factors)
    assert sizes(h, ctypes.byref(n), ctypes.byref(nl), ctypes.byref(nu)) == C.SMLU_OK, C.last_error(h)
    n, dt = n.value, np.complex128 if z else np.float64
    f = dict(Lp=np.empty(n + 1, np.int64), Li=np.empty(nl.value, np.int64), Lx=np.empty(nl.value, dt),
             Up=np.empty(n + 1, np.int64), Ui=np.empty(nu.value, np.int64), Ux=np.empty(nu.value, dt),
             p=np.empty(n, np.int64), q=np.empty(n, np.int64), Rs=np.empty(n))
    assert get(h, *[C.ptr(f[k]) for k in ("Lp", "Li", "Lx", "Up", "Ui", "Ux", "p", "q", "Rs")]) == C.SMLU_OK, \
        C.last_error(h)
    return f


def mirror_factors(F, z=False):
    """The same dict from a handle of the Python mirror (0-based)."""
    fx = F._download() if z else F.real_equivalent_factors()
    Lm, Um = fx["L"], fx["U"]
    return dict(Lp=Lm.indptr, Li=Lm.indices, Lx=Lm.data, Up=Um.indptr, Ui=Um.indices, Ux=Um.data,
                p=fx["p"], q=fx["q"], Rs=fx["Rs"])


def assert_factors_shifted(f1, f0, base=1):
    """Every index array of f1 is exactly f0's plus `base`; every value array is bitwise f0's."""
    for k in ("Lp", "Li", "Up", "Ui", "p", "q"):
        assert np.array_equal(f1[k], np.asarray(f0[k], dtype=np.int64) + base), k
    for k in ("Lx", "Ux", "Rs"):
        assert np.array_equal(f1[k], f0[k]), k


def fronts(h):
    """smlu_get_fronts: dict(first, parent, rowptr, rows, p0, mode), 0-based whatever the handle's base."""
    L = C.lib()
    ns, n = int(stat(h, "nsuper")), int(stat(h, "n"))
    first, parent = np.empty(ns + 1, np.int64), np.empty(ns, np.int64)
    rowptr, mode = np.empty(ns + 1, np.int64), np.empty(ns, np.int32)
    assert L.smlu_get_fronts(h, C.ptr(first), C.ptr(parent), C.ptr(rowptr), None, None, C.ptr(mode)) == C.SMLU_OK
    rows, p0 = np.empty(rowptr[-1], np.int64), np.empty(n, np.int64)
    assert L.smlu_get_fronts(h, None, None, None, C.ptr(rows), C.ptr(p0), None) == C.SMLU_OK
    return dict(first=first, parent=parent, rowptr=rowptr, rows=rows, p0=p0, mode=mode)


def solve(h, b, trans="N"):
    """smlu_solve ("N") / smlu_solve_trans ("T", "C") on a host vector (complex: interleaved)."""
    b = np.ascontiguousarray(b)
    x = np.full_like(b, np.nan)
    L = C.lib()
    if trans == "N":
        rc = L.smlu_solve(h, C.ptr(b), C.ptr(x))
    else:
        rc = L.smlu_solve_trans(h, C.SMLU_OP_T if trans == "T" else C.SMLU_OP_H, C.ptr(b), C.ptr(x))
    assert rc == C.SMLU_OK, C.last_error(h)
    return x


def solve_multi(h, B):
    """smlu_solve_multi on the columns of a Fortran-ordered real host array."""
    B = np.asfortranarray(B, dtype=np.float64)
    X = np.full_like(B, np.nan)
    n, nrhs = B.shape
    assert C.lib().smlu_solve_multi(h, nrhs, C.ptr(B), n, C.ptr(X), n) == C.SMLU_OK, C.last_error(h)
    return X


def refactor_csc(h, A, base=1, z=False):
    """smlu_refactor_csc[_z] with A's pattern shifted by `base`; returns the status."""
    A = csc(A)
    cp, ri = _i64(A.indptr, base), _i64(A.indices, base)
    vals = np.ascontiguousarray(A.data, dtype=np.complex128 if z else np.float64)
    fn = C.lib().smlu_refactor_csc_z if z else C.lib().smlu_refactor_csc
    return fn(h, A.shape[0], C.ptr(cp), C.ptr(ri), C.ptr(vals))
