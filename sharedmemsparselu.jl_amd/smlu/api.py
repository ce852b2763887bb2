"""Python mirror of the reference's Julia surface (SharedMemSparseLU.jl, src/SharedMemSparseLU.jl).

Julia name                          here                          reference
----------------------------------  ----------------------------  -----------------------
ParallelSparseLU(A, chunk_size)     ParallelSparseLU(A, cs)       :64-98
lu!(F, A)                           lu_(F, A)                     :245-279
ldiv!(x, F, b)                      ldiv_(x, F, b)                :286-342
ldiv!(x, transpose(F), b)           ldiv_(x, F, b, trans="T")     (not in the reference)
ldiv!(x, F', b)                     ldiv_(x, F, b, trans="C")     (not in the reference)
ldiv_refined!(X, F, B)              ldiv_refined_(X, F, B)        (not in the reference)
lsolve!(F, x), rsolve!(F, x)        lsolve_(F, x), rsolve_(F, x)  :349-392
logabsdet(F), det(F), logdet(F)     F.logabsdet() F.det() F.logdet()  (not in the reference)
cond(F, 1), cond(F, Inf)            F.condest("1"|"inf"), F.rcond()   (not in the reference)
gmres!(x, F, A, b)                  F.gmres(b, values=A)          (not in the reference)
lowrank!(F, U, V)                   F.lowrank_set(U, V)           (not in the reference)
ldiv_lowrank!(x, F, b)              F.solve_lowrank(b)            (not in the reference)
F.L F.U F.p F.q F.Rs                F.L F.U F.p F.q F.Rs          :45-52 (0-based here)
cleanup_ParallelSparseLU!(F)        cleanup_ParallelSparseLU_(F)  :31 (exported, undefined there)
DimensionMismatch                   DimensionMismatch             :288-290
SingularException (UMFPACK)         SingularException             :74 / :247

Tf = ComplexF64 (the reference is generic in Tf, :43, :64, :286): pass a complex matrix and
complex vectors to the same functions; the library factors the real-equivalent 2n x 2n matrix
(``smlu_create_z``, include/smlu.h), so F.L / F.U / F.p / F.q / F.Rs of a complex F are those
of that real-equivalent matrix (2n rows).

All numerics run on the MI355X through libsmlu.so; nothing here computes factors or solves.
"""
from __future__ import annotations

import collections
import ctypes
import math

import numpy as np
import scipy.sparse as sp

from . import _lib as C


class DimensionMismatch(ValueError):
    """Julia's DimensionMismatch (src/SharedMemSparseLU.jl:288-290)."""


class SingularException(np.linalg.LinAlgError):
    """UMFPACK's SingularException raised by lu(A)/lu!(F, A) with check=true."""

    def __init__(self, col):
        super().__init__(f"matrix is singular: zero pivot at column {col}")
        self.info = col


class SmluError(RuntimeError):
    code = None   # the library's status code, when the error came from a C call


def _csc(A):
    dt = np.complex128 if (np.iscomplexobj(A.data) if sp.issparse(A) else np.iscomplexobj(A)) \
        else np.float64
    if not sp.issparse(A):
        A = sp.csc_matrix(np.asarray(A, dtype=dt))
    A = sp.csc_matrix(A, dtype=dt)
    if not A.has_sorted_indices:
        A = A.sorted_indices()
    A.sum_duplicates()
    return A


def _op(trans):
    """trans = "N" | "T" | "C" -> SMLU_OP_N / SMLU_OP_T / SMLU_OP_H (include/smlu.h)."""
    try:
        return {"N": C.SMLU_OP_N, "T": C.SMLU_OP_T, "C": C.SMLU_OP_H}[trans]
    except (KeyError, TypeError):
        raise ValueError(f'trans must be "N", "T" or "C", got {trans!r}') from None


def _norm(norm):
    """norm = "1" | "inf" -> SMLU_NORM_ONE / SMLU_NORM_INF (include/smlu.h)."""
    try:
        return {"1": C.SMLU_NORM_ONE, "inf": C.SMLU_NORM_INF}[norm]
    except (KeyError, TypeError):
        raise ValueError(f'norm must be "1" or "inf", got {norm!r}') from None


GmresInfo = collections.namedtuple(
    "GmresInfo", "converged iters cycles solves relres relres_est berr bnorm status")
GmresInfo.__doc__ = """What smlu_solve_gmres* reports: converged (bool), iters (Arnoldi steps), cycles,
solves (factor solves = iters + cycles), relres (true ||b - op(A')x|| / ||b|| of the returned x),
relres_est (the last estimate), berr (componentwise backward error), bnorm, status (the C return code:
0 or SMLU_NOT_CONVERGED)."""


def _gmres_opts(trans, rtol, restart, maxiter):
    """(op, SmluGmresOpts) after the argument checks of smlu_solve_gmres*, raised as ValueError
    before any handle is looked at."""
    op = _op(trans)
    for name, v in (("restart", restart), ("maxiter", maxiter)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not 1 <= restart <= 32:
        raise ValueError(f"restart must be in 1..32, got {restart!r}")
    if maxiter < 1:
        raise ValueError(f"maxiter must be at least 1, got {maxiter!r}")
    try:
        rt = float(rtol)
    except (TypeError, ValueError):
        raise ValueError(f"rtol must be a finite number >= 0, got {rtol!r}") from None
    if not (math.isfinite(rt) and rt >= 0.0):
        raise ValueError(f"rtol must be a finite number >= 0, got {rtol!r}")
    return op, C.SmluGmresOpts(rt, int(restart), int(maxiter))


def _device_f64(name, t, size):
    """A torch tensor handed to a *_device entry point as `size` doubles must be that: float64, on a
    GPU, contiguous, `size` elements (a raw pointer int, or None, is taken as it is)."""
    if t is None or not hasattr(t, "data_ptr"):
        return
    import torch
    if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"`{name}` must be a contiguous float64 tensor on the GPU")
    if t.numel() != size:
        raise DimensionMismatch(f"`{name}` has {t.numel()} elements, expected {size}")


def _gmres_info(rc, ci):
    return GmresInfo(bool(ci.converged), ci.iters, ci.cycles, ci.solves, ci.relres, ci.relres_est, ci.berr,
                     ci.bnorm, rc)


LowrankInfo = collections.namedtuple(
    "LowrankInfo", "k steps stop solves berr resid rcond_c pivot_min gram_max status")
LowrankInfo.__doc__ = """What smlu_lowrank_set* and smlu_solve_lowrank* report: k (rank in force), steps
(corrections made), stop (0 not refined, 1 berr <= 2^-51, 2 berr did not halve, 3 step limit), solves
(factor solves run), berr and resid (last measured, -1 if never), rcond_c, pivot_min and gram_max (of the
capacitance matrix, from a set; -1 from a solve), status (the C return code: 0 or SMLU_SINGULAR)."""


def _lowrank_info(rc, ci):
    return LowrankInfo(ci.k, ci.steps, ci.stop, ci.solves, ci.berr, ci.resid, ci.rcond_c, ci.pivot_min,
                       ci.gram_max, rc)


def _lowrank_steps(steps):
    """max_steps of smlu_solve_lowrank*: an integer >= -1, raised as ValueError before any handle is
    looked at."""
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < -1:
        raise ValueError(f"steps must be an integer >= -1, got {steps!r}")
    return int(steps)


def _refine_steps(steps):
    """steps=None -> -1 (the handle's rule); otherwise an integer >= 0 (max_steps of
    smlu_solve_refined_multi*)."""
    if steps is None:
        return -1
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
        raise ValueError(f"steps must be None or an integer >= 0, got {steps!r}")
    return int(steps)


def _refine_info(info, nrhs):
    """The smlu_refine_info array of a call as a dict of per-column numpy arrays."""
    return dict(steps=np.array([info[j].steps for j in range(nrhs)], np.int32),
                stop=np.array([info[j].stop for j in range(nrhs)], np.int32),
                berr=np.array([info[j].berr for j in range(nrhs)], np.float64),
                resid=np.array([info[j].resid for j in range(nrhs)], np.float64))


def _check(rc, h=None):
    if rc < 0:
        e = SmluError(f"libsmlu error {rc}: {C.last_error(h)}")
        e.code = rc
        raise e
    return rc


class ParallelSparseLU:
    """LU factorisation of a square sparse matrix on the MI355X.

    ``F.L * F.U == (F.Rs[:, None] * A)[F.p][:, F.q]`` (UMFPACK's relation quoted at
    src/SharedMemSparseLU.jl:305-316), with 0-based ``p``/``q``.

    ``scale=False``: no row scaling (``smlu_opts.scale = 0``, ``F.Rs`` all ones).  ``index_base=1``:
    the index arrays cross the C ABI 1-based, as the Julia shim passes them; everything on the
    Python side stays 0-based.
    """

    def __init__(self, A, chunk_size=None, *, ordering="auto", grid=None, device=0,
                 profile=False, p=None, q=None, Rs=None, pivot_tol=None, diag_pivot_tol=None,
                 leaf_size=None, relax=True, use_mfma=None, refine=None,
                 int32_indices=False, L_pattern=None, U_pattern=None, scale=True, index_base=0):
        A = _csc(A)
        m, n = A.shape
        if m != n:
            raise DimensionMismatch(f"matrix is not square: {m} x {n}")
        if chunk_size is None:
            chunk_size = 8                       # :67-70
        chunk_size = min(int(chunk_size), n)     # :72
        order = {"auto": C.ORDER_AUTO, "natural": C.ORDER_NATURAL, "nd": C.ORDER_GRAPH_ND,
                 "geometric": C.ORDER_GEOMETRIC_ND, "amd": C.ORDER_AMD, "given": C.ORDER_GIVEN}[ordering]
        if index_base not in (0, 1):
            raise ValueError(f"index_base must be 0 or 1, got {index_base!r}")
        # index_base=1: the index arrays cross the C-ABI 1-based, as Julia passes them; this class
        # stays 0-based on its Python side (arguments and F.L / F.U / F.p / F.q)
        base = self._base = int(index_base)
        kw = dict(chunk_size=chunk_size, index_base=base, ordering=order, device=device,
                  profile=1 if profile else 0, relax=1 if relax else 0, scale=1 if scale else 0)
        if grid is not None:
            kw["grid"] = grid
            if ordering == "auto":
                kw["ordering"] = C.ORDER_GEOMETRIC_ND
        if pivot_tol is not None:
            kw["pivot_tol"] = float(pivot_tol)
        if diag_pivot_tol is not None:
            kw["diag_pivot_tol"] = float(diag_pivot_tol)
        if leaf_size is not None:
            kw["leaf_size"] = int(leaf_size)
        if use_mfma is not None:
            kw["use_mfma"] = 1 if use_mfma else 0
        if refine is not None:
            kw["refine"] = int(refine)
        self._opts = C.default_opts(**kw)
        self.m, self.n = m, n
        self.chunk_size = chunk_size
        self.is_complex = A.dtype == np.complex128
        self._dt = A.dtype
        self._colptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        self._rowval = np.ascontiguousarray(A.indices, dtype=np.int64)
        vals = np.ascontiguousarray(A.data, dtype=self._dt)
        h = ctypes.c_void_p()
        L = C.lib()
        colptr, rowval = self._colptr + base, self._rowval + base
        if self.is_complex:
            if p is not None or q is not None or int32_indices:
                raise ValueError("complex matrices take neither a given (p, q) nor Int32 indices")
            rc = L.smlu_create_z(n, C.ptr(colptr), C.ptr(rowval), C.ptr(vals),
                                 ctypes.byref(self._opts), ctypes.byref(h))
        elif p is not None or q is not None:
            pp = np.ascontiguousarray(p, dtype=np.int64) + base
            qq = np.ascontiguousarray(q, dtype=np.int64) + base
            rs = None if Rs is None else np.ascontiguousarray(Rs, dtype=np.float64)
            # UMFPACK's F.L / F.U patterns: any sparse matrix, only the pattern is used
            pat = []
            for M in (L_pattern, U_pattern):
                if M is None:
                    pat += [None, None]
                else:
                    M = sp.csc_matrix(M)
                    M.sort_indices()
                    pat += [np.ascontiguousarray(M.indptr, dtype=np.int64) + base,
                            np.ascontiguousarray(M.indices, dtype=np.int64) + base]
            rc = L.smlu_create_with_pivots(n, C.ptr(colptr), C.ptr(rowval), C.ptr(vals),
                                           C.ptr(pp), C.ptr(qq), C.ptr(rs), *[C.ptr(a) for a in pat],
                                           ctypes.byref(self._opts), ctypes.byref(h))
        elif int32_indices:
            # SparseMatrixCSC{Float64,Int32}: the Int32 entry point
            cp32 = np.ascontiguousarray(A.indptr, dtype=np.int32) + np.int32(base)
            ri32 = np.ascontiguousarray(A.indices, dtype=np.int32) + np.int32(base)
            rc = L.smlu_create_i32(n, C.ptr(cp32), C.ptr(ri32), C.ptr(vals),
                                   ctypes.byref(self._opts), ctypes.byref(h))
        else:
            rc = L.smlu_create(n, C.ptr(colptr), C.ptr(rowval), C.ptr(vals),
                               ctypes.byref(self._opts), ctypes.byref(h))
        if rc < 0:
            raise SmluError(f"smlu_create failed ({rc}): {C.last_error(None)}")
        self._h = h
        self._factors = None
        if rc == C.SMLU_SINGULAR:
            col = L.smlu_last_error_col(h)
            self.close()
            raise SingularException(col)

    # ---- factor access (F.L, F.U, F.p, F.q, F.Rs) ----
    def _download(self):
        """F.L, F.U, F.p, F.q, F.Rs as the reference has them: complex n x n factors on a complex
        handle (smlu_get_factors_z), real ones otherwise."""
        if not self.is_complex:
            return self.real_equivalent_factors()
        if getattr(self, "_zfactors", None) is None:
            L = C.lib()
            n = self.n
            nl, nu = ctypes.c_int64(), ctypes.c_int64()
            _check(L.smlu_get_sizes_z(self._h, None, ctypes.byref(nl), ctypes.byref(nu)), self._h)
            Lp = np.empty(n + 1, np.int64); Li = np.empty(nl.value, np.int64); Lx = np.empty(nl.value, np.complex128)
            Up = np.empty(n + 1, np.int64); Ui = np.empty(nu.value, np.int64); Ux = np.empty(nu.value, np.complex128)
            p = np.empty(n, np.int64); q = np.empty(n, np.int64); Rs = np.empty(n)
            _check(L.smlu_get_factors_z(self._h, C.ptr(Lp), C.ptr(Li), C.ptr(Lx), C.ptr(Up), C.ptr(Ui),
                                        C.ptr(Ux), C.ptr(p), C.ptr(q), C.ptr(Rs)), self._h)
            b = self._base
            self._zfactors = dict(L=sp.csc_matrix((Lx, Li - b, Lp - b), shape=(n, n)),
                                  U=sp.csc_matrix((Ux, Ui - b, Up - b), shape=(n, n)), p=p - b, q=q - b, Rs=Rs)
        return self._zfactors

    def real_equivalent_factors(self):
        """The factors the GPU holds: on a complex handle those of the 2n x 2n real-equivalent K."""
        if self._factors is None:
            L = C.lib()
            n = 2 * self.n if self.is_complex else self.n   # complex: the real-equivalent matrix
            nl, nu = ctypes.c_int64(), ctypes.c_int64()
            _check(L.smlu_get_sizes(self._h, None, ctypes.byref(nl), ctypes.byref(nu)), self._h)
            Lp = np.empty(n + 1, np.int64); Li = np.empty(nl.value, np.int64); Lx = np.empty(nl.value)
            Up = np.empty(n + 1, np.int64); Ui = np.empty(nu.value, np.int64); Ux = np.empty(nu.value)
            p = np.empty(n, np.int64); q = np.empty(n, np.int64); Rs = np.empty(n)
            _check(L.smlu_get_factors(self._h, C.ptr(Lp), C.ptr(Li), C.ptr(Lx), C.ptr(Up), C.ptr(Ui),
                                      C.ptr(Ux), C.ptr(p), C.ptr(q), C.ptr(Rs)), self._h)
            b = self._base
            self._factors = dict(L=sp.csc_matrix((Lx, Li - b, Lp - b), shape=(n, n)),
                                 U=sp.csc_matrix((Ux, Ui - b, Up - b), shape=(n, n)), p=p - b, q=q - b, Rs=Rs)
        return self._factors

    @property
    def L(self):
        return self._download()["L"]

    @property
    def U(self):
        return self._download()["U"]

    @property
    def p(self):
        return self._download()["p"]

    @property
    def q(self):
        return self._download()["q"]

    @property
    def Rs(self):
        return self._download()["Rs"]

    def stat(self, key):
        return C.lib().smlu_stat(self._h, key.encode())

    def perm_scale(self):
        """(F.p, F.q, F.Rs) without downloading L and U (smlu_get_factors with NULL factor
        pointers); real-equivalent order on a complex handle."""
        n = 2 * self.n if self.is_complex else self.n
        p = np.empty(n, np.int64); q = np.empty(n, np.int64); Rs = np.empty(n)
        _check(C.lib().smlu_get_factors(self._h, None, None, None, None, None, None, C.ptr(p), C.ptr(q),
                                        C.ptr(Rs)), self._h)
        return p - self._base, q - self._base, Rs

    def front_store(self):
        """Diagnostics (smlu_dev_front_offsets / smlu_dev_copy): the factor store as one host array
        and per front (Loff, Uoff, Foff, M); front s is store[Loff:Loff+M*ns] (L panel, ld M) and
        store[Uoff:Uoff+ns*nu] (U12, ld ns)."""
        L = C.lib()
        ns = int(self.stat("nsuper"))
        off = np.empty(4 * ns, np.int64)
        _check(L.smlu_dev_front_offsets(self._h, C.ptr(off)), self._h)
        ln = ctypes.c_int64()
        _check(L.smlu_dev_copy(self._h, 0, 0, -1, None, ctypes.byref(ln)), self._h)
        store = np.empty(ln.value)
        _check(L.smlu_dev_copy(self._h, 0, 0, ln.value, C.ptr(store), None), self._h)
        return store, off.reshape(ns, 4)

    def fronts(self):
        """The analysis' assembly tree and the current schedule's pivot-candidate mode per front
        (smlu_get_fronts): dict(first, parent, rowptr, rows, p0, mode), 0-based."""
        ns = int(self.stat("nsuper"))
        n = int(self.stat("n"))
        first = np.empty(ns + 1, np.int64)
        parent = np.empty(ns, np.int64)
        rowptr = np.empty(ns + 1, np.int64)
        mode = np.empty(ns, np.int32)
        L = C.lib()
        _check(L.smlu_get_fronts(self._h, C.ptr(first), C.ptr(parent), C.ptr(rowptr), None, None,
                                 C.ptr(mode)), self._h)
        rows = np.empty(rowptr[-1], np.int64)
        p0 = np.empty(n, np.int64)
        _check(L.smlu_get_fronts(self._h, None, None, None, C.ptr(rows), C.ptr(p0), None), self._h)
        return dict(first=first, parent=parent, rowptr=rowptr, rows=rows, p0=p0, mode=mode)

    def refactor(self, values):
        """lu!(F, A) with host values in A's CSC order (same pattern): smlu_refactor, the call the
        Julia shim makes (src/SharedMemSparseLU.jl:245-279)."""
        v = np.ascontiguousarray(values, dtype=self._dt)
        L = C.lib()
        rc = _check((L.smlu_refactor_z if self.is_complex else L.smlu_refactor)(self._h, C.ptr(v)), self._h)
        self._factors = None
        self._zfactors = None
        if rc == C.SMLU_SINGULAR:
            raise SingularException(L.smlu_last_error_col(self._h))
        return rc

    # ---- device-resident entry points (values / vectors already in HBM) ----
    def refactor_device(self, d_values):
        """lu! with values already on the device (torch tensor or raw pointer int; complex
        handles take interleaved complex values, e.g. a complex128 tensor)."""
        ptr = d_values.data_ptr() if hasattr(d_values, "data_ptr") else int(d_values)
        fn = C.lib().smlu_refactor_z_device if self.is_complex else C.lib().smlu_refactor_device
        with C.caller_stream(self._h, d_values):
            rc = _check(fn(self._h, ctypes.c_void_p(ptr)), self._h)
        self._factors = None
        self._zfactors = None
        if rc == C.SMLU_SINGULAR:
            raise SingularException(C.lib().smlu_last_error_col(self._h))
        return rc

    def solve_device(self, d_x, d_b, trans="N"):
        """ldiv! on device vectors; trans="T" / "C": the transposed / adjoint solve from the same
        factors (smlu_solve_trans_device)."""
        op = _op(trans)
        px = d_x.data_ptr() if hasattr(d_x, "data_ptr") else int(d_x)
        pb = d_b.data_ptr() if hasattr(d_b, "data_ptr") else int(d_b)
        with C.caller_stream(self._h, d_b):
            if op != C.SMLU_OP_N:
                return _check(C.lib().smlu_solve_trans_device(self._h, op, ctypes.c_void_p(pb),
                                                              ctypes.c_void_p(px)), self._h)
            return _check(C.lib().smlu_solve_device(self._h, ctypes.c_void_p(pb), ctypes.c_void_p(px)),
                          self._h)

    def solve_multi_device(self, d_X, d_B, trans="N"):
        """ldiv! for several right-hand sides on the device: d_B, d_X are (nrhs, n) contiguous
        torch tensors (column r = row r, i.e. column-major n x nrhs).  One GPU: batches of up to
        16 columns go through the solve kernels together.  trans="T" / "C": the transposed /
        adjoint solve, also in batches of up to 16 columns, every column bitwise equal to
        solve_device(..., trans=...) of that column alone; one refined solve per column when
        iterative refinement applies (smlu_solve_trans_multi_device)."""
        op = _op(trans)
        nrhs, n = d_B.shape
        if n != self.n or tuple(d_X.shape) != (nrhs, n):
            raise DimensionMismatch(f"B has shape {tuple(d_B.shape)}, X has shape {tuple(d_X.shape)}, n={self.n}")
        ld = 2 * n if self.is_complex else n     # leading dimension in doubles
        with C.caller_stream(self._h, d_B):
            if op != C.SMLU_OP_N:
                return _check(C.lib().smlu_solve_trans_multi_device(
                    self._h, op, nrhs, ctypes.c_void_p(d_B.data_ptr()), ld, ctypes.c_void_p(d_X.data_ptr()), ld),
                    self._h)
            return _check(C.lib().smlu_solve_multi_device(self._h, nrhs, ctypes.c_void_p(d_B.data_ptr()), ld,
                                                          ctypes.c_void_p(d_X.data_ptr()), ld), self._h)

    def solve_refined_multi_device(self, d_X, d_B, trans="N", steps=None):
        """ldiv! for several right-hand sides with iterative refinement run as a batch
        (smlu_solve_refined_multi_device): d_B, d_X are (nrhs, n) contiguous torch tensors as in
        solve_multi_device.  Up to 16 columns share each solve pass and each residual pass; every
        column is refined by the rule of the single solve and is bitwise solve_device(...,
        trans=...) of that column alone.  steps=None: the handle's own rule; 0: a plain batch;
        k > 0: up to k corrections per column.  Returns a dict of per-column arrays: steps and stop
        (int32; stop 0 not refined, 1 berr <= 2^-51, 2 berr did not halve, 3 step limit), berr and
        resid (float64, the last ones measured; -1 when nothing was refined)."""
        op = _op(trans)
        nrhs, n = d_B.shape
        if n != self.n or tuple(d_X.shape) != (nrhs, n):
            raise DimensionMismatch(f"B has shape {tuple(d_B.shape)}, X has shape {tuple(d_X.shape)}, n={self.n}")
        ld = 2 * n if self.is_complex else n     # leading dimension in doubles
        info = (C.SmluRefineInfo * max(nrhs, 1))()
        with C.caller_stream(self._h, d_B):
            _check(C.lib().smlu_solve_refined_multi_device(
                self._h, op, _refine_steps(steps), nrhs, ctypes.c_void_p(d_B.data_ptr()), ld,
                ctypes.c_void_p(d_X.data_ptr()), ld, info), self._h)
        return _refine_info(info, nrhs)

    # ---- determinant and condition estimate (smlu_logabsdet*, smlu_rcond) ----
    def logabsdet(self):
        """(log|det A|, sign) of the current factorization, as Julia's logabsdet(F): sign is +1.0 or
        -1.0, and a complex number of modulus 1 on a complex factorization.  Computed on the device
        from the factors' diagonal and permutations; cached until the next refactor."""
        la = ctypes.c_double()
        if self.is_complex:
            ph = (ctypes.c_double * 2)()
            _check(C.lib().smlu_logabsdet_z(self._h, ctypes.byref(la), ph), self._h)
            return la.value, complex(ph[0], ph[1])
        sg = ctypes.c_double()
        _check(C.lib().smlu_logabsdet(self._h, ctypes.byref(la), ctypes.byref(sg)), self._h)
        return la.value, sg.value

    def det(self):
        """det(F) = sign * exp(log|det A|); overflows to inf where the determinant does."""
        la, sg = self.logabsdet()
        return sg * np.exp(la)

    def logdet(self):
        """logdet(F): log(det A).  A negative real determinant raises, as Julia's DomainError does;
        a complex factorization returns log|det A| + i arg(det A)."""
        la, sg = self.logabsdet()
        if self.is_complex:
            return complex(la, np.angle(sg))
        if sg < 0:
            raise ValueError("logdet: the determinant is negative (use logabsdet)")
        return la

    def rcond(self, norm="1", parts=False):
        """Reciprocal condition estimate 1 / (||A|| est||A^-1||) in the 1-norm (norm="1") or the
        infinity norm (norm="inf") from the current factors (smlu_rcond: LAPACK's dgecon / zgecon
        estimator on the GPU solves).  parts=True returns (rcond, ||A||, est||A^-1||)."""
        nm = _norm(norm)
        r, an, ai = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check(C.lib().smlu_rcond(self._h, nm, ctypes.byref(r), ctypes.byref(an), ctypes.byref(ai)), self._h)
        return (r.value, an.value, ai.value) if parts else r.value

    def condest(self, norm="1"):
        """Estimate of cond(A) in the given norm: ||A|| est||A^-1|| (inf when rcond is 0)."""
        _norm(norm)
        _, an, ai = ParallelSparseLU.rcond(self, norm, parts=True)
        return an * ai if an * ai > 0 else float("inf")

    # ---- solve with stale factors (smlu_solve_gmres*) ----
    def gmres(self, b, values=None, trans="N", rtol=1e-10, restart=30, maxiter=200, x=None):
        """Solve op(A') x = b by restarted GMRES(restart) preconditioned by the current factors, all
        on the GPU (smlu_solve_gmres): A' has F's pattern and `values` (an nnz array in A's CSC order,
        or a scipy matrix of the same pattern; None: the values F holds, i.e. GMRES-based refinement).
        trans as ldiv_.  Returns (x, info); x is written into the given array when one is passed
        (it may be b).  Non-convergence does not raise: info.converged is False and x the last
        iterate.  F itself -- values, factors, caches -- is left as it was."""
        op, o = _gmres_opts(trans, rtol, restart, maxiter)
        if self.is_complex:   # out of scope, as in the library (smlu_solve_gmres: SMLU_ERR_STATE)
            e = SmluError(f"libsmlu error {C.SMLU_ERR_STATE}: gmres: ComplexF64 handles are not supported")
            e.code = C.SMLU_ERR_STATE
            raise e
        if len(b) != self.n:
            raise DimensionMismatch(f"`b` does not have same size as F: length(b)={len(b)}, F.n={self.n}")
        vals = None
        if values is not None:
            if sp.issparse(values):
                A = _csc(values)
                if A.shape != (self.m, self.n) or A.nnz != self._rowval.size or \
                        not np.array_equal(A.indptr, self._colptr) or not np.array_equal(A.indices, self._rowval):
                    raise ValueError("gmres: `values` must have the sparsity pattern F was created with")
                values = A.data
            vals = np.ascontiguousarray(values, dtype=np.float64)
            if vals.shape != (self._rowval.size,):
                raise DimensionMismatch(f"`values` has shape {vals.shape}, nnz(A)={self._rowval.size}")
        bb = np.ascontiguousarray(b, dtype=np.float64)
        if x is None:
            x = np.empty(self.n)
        elif len(x) != self.n:
            raise DimensionMismatch(f"`x` does not have same size as F: length(x)={len(x)}, F.n={self.n}")
        xx = x if (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous) \
            else np.empty(self.n)
        ci = C.SmluGmresInfo()
        rc = _check(C.lib().smlu_solve_gmres(self._h, op, C.ptr(vals), C.ptr(bb), C.ptr(xx), ctypes.byref(o),
                                             ctypes.byref(ci)), self._h)
        if xx is not x:
            x[:] = xx
        return x, _gmres_info(rc, ci)

    def gmres_device(self, d_x, d_b, d_values=None, trans="N", rtol=1e-10, restart=30, maxiter=200):
        """gmres on device vectors (torch tensors or raw pointer ints; d_x may be d_b): d_values holds
        nnz doubles in A's CSC order on the device, None: the values F holds.  Returns info
        (smlu_solve_gmres_device, ordered after the stream that produced d_b)."""
        op, o = _gmres_opts(trans, rtol, restart, maxiter)
        if self.is_complex:
            e = SmluError(f"libsmlu error {C.SMLU_ERR_STATE}: gmres: ComplexF64 handles are not supported")
            e.code = C.SMLU_ERR_STATE
            raise e
        for name, t, size in (("d_x", d_x, self.n), ("d_b", d_b, self.n), ("d_values", d_values, self._rowval.size)):
            _device_f64(name, t, size)
        px = d_x.data_ptr() if hasattr(d_x, "data_ptr") else int(d_x)
        pb = d_b.data_ptr() if hasattr(d_b, "data_ptr") else int(d_b)
        pv = None if d_values is None else \
            ctypes.c_void_p(d_values.data_ptr() if hasattr(d_values, "data_ptr") else int(d_values))
        ci = C.SmluGmresInfo()
        with C.caller_stream(self._h, d_b):
            rc = _check(C.lib().smlu_solve_gmres_device(self._h, op, pv, ctypes.c_void_p(pb), ctypes.c_void_p(px),
                                                        ctypes.byref(o), ctypes.byref(ci)), self._h)
        return _gmres_info(rc, ci)

    # ---- low-rank updates of the solve (smlu_lowrank_*, smlu_solve_lowrank*) ----
    def _lowrank_real(self, who):
        if self.is_complex:   # out of scope, as in the library (SMLU_ERR_STATE)
            e = SmluError(f"libsmlu error {C.SMLU_ERR_STATE}: {who}: ComplexF64 handles are not supported")
            e.code = C.SMLU_ERR_STATE
            raise e

    def lowrank_set(self, U, V):
        """Install the update A + U V^T on the current factors (smlu_lowrank_set): U and V are n x k
        arrays (or n-vectors, k = 1), k <= 32.  Y = A^-1 U, C = I + V^T Y and C^-1 are computed on the
        GPU.  Returns LowrankInfo (k, solves, rcond_c, pivot_min, gram_max; status SMLU_OK, or
        SMLU_SINGULAR when C is singular or not finite: then nothing is installed).  Every refactor
        drops the update.  k = 0 (n x 0 arrays) clears it."""
        self._lowrank_real("lowrank_set")
        U = np.asarray(U, dtype=np.float64)
        V = np.asarray(V, dtype=np.float64)
        if U.ndim == 1:
            U = U[:, None]
        if V.ndim == 1:
            V = V[:, None]
        if U.ndim != 2 or V.ndim != 2 or U.shape != V.shape or U.shape[0] != self.n:
            raise DimensionMismatch(f"U has shape {U.shape}, V has shape {V.shape}, expected two ({self.n}, k) arrays")
        k = U.shape[1]
        if k > C.SMLU_LOWRANK_MAX:
            raise ValueError(f"the rank of an update is at most {C.SMLU_LOWRANK_MAX}, got {k}")
        Uf, Vf = np.asfortranarray(U), np.asfortranarray(V)     # column j at j * n
        ci = C.SmluLowrankInfo()
        rc = _check(C.lib().smlu_lowrank_set(self._h, k, C.ptr(Uf) if k else None, self.n, C.ptr(Vf) if k else None,
                                             self.n, ctypes.byref(ci)), self._h)
        return _lowrank_info(rc, ci)

    def lowrank_set_device(self, d_U, d_V):
        """lowrank_set with U and V on the device: (k, n) contiguous float64 torch tensors (row j is
        column j, as in solve_multi_device).  Ordered after the stream that produced d_U."""
        self._lowrank_real("lowrank_set_device")
        if tuple(d_U.shape) != tuple(d_V.shape) or d_U.dim() != 2 or d_U.shape[1] != self.n:
            raise DimensionMismatch(f"U has shape {tuple(d_U.shape)}, V has shape {tuple(d_V.shape)}, n={self.n}")
        k = int(d_U.shape[0])
        if k > C.SMLU_LOWRANK_MAX:
            raise ValueError(f"the rank of an update is at most {C.SMLU_LOWRANK_MAX}, got {k}")
        for name, t in (("d_U", d_U), ("d_V", d_V)):
            _device_f64(name, t, k * self.n)
        ci = C.SmluLowrankInfo()
        with C.caller_stream(self._h, d_U):
            rc = _check(C.lib().smlu_lowrank_set_device(self._h, k, ctypes.c_void_p(d_U.data_ptr()), self.n,
                                                        ctypes.c_void_p(d_V.data_ptr()), self.n, ctypes.byref(ci)),
                        self._h)
        return _lowrank_info(rc, ci)

    def lowrank_clear(self):
        """Drop the installed update (smlu_lowrank_clear); the buffers are kept."""
        _check(C.lib().smlu_lowrank_clear(self._h), self._h)

    def update_columns(self, cols, A_new, A):
        """The update that replaces the columns `cols` of A, the matrix F holds the factors of, by those
        of A_new: U[:, t] = A_new[:, cols[t]] - A[:, cols[t]], V[:, t] = e_cols[t], then lowrank_set.
        Outside `cols` the two matrices must be equal, pattern and values; the changed columns may have
        any pattern (a dense column costs no fill).  Returns lowrank_set's info."""
        A, A_new = _csc(A), _csc(A_new)
        cols = np.asarray(cols, dtype=np.int64).ravel()
        if A.shape != (self.m, self.n) or A_new.shape != A.shape:
            raise DimensionMismatch(f"A has shape {A.shape}, A_new has shape {A_new.shape}, F.n={self.n}")
        if cols.size and (cols.min() < 0 or cols.max() >= self.n or np.unique(cols).size != cols.size):
            raise ValueError("update_columns: `cols` must be distinct column indices of A")
        keep = np.ones(self.n, bool)
        keep[cols] = False
        rest, rest_new = A[:, keep], A_new[:, keep]
        if not (np.array_equal(rest.indptr, rest_new.indptr) and np.array_equal(rest.indices, rest_new.indices)
                and np.array_equal(rest.data, rest_new.data)):
            raise ValueError("update_columns: A_new must equal A, pattern and values, outside `cols`")
        U = np.asfortranarray((A_new[:, cols] - A[:, cols]).toarray())
        V = np.zeros((self.n, cols.size), order="F")
        V[cols, np.arange(cols.size)] = 1.0
        return self.lowrank_set(U, V)

    def solve_lowrank(self, b, trans="N", steps=-1, x=None):
        """Solve op(A + U V^T) x = b with the installed update (smlu_solve_lowrank); trans as ldiv_.
        steps: refinement on the updated system, -1 up to 3 corrections (the default), 0 none, m > 0
        up to m.  Returns (x, info); x is written into the given array when one is passed (it may be
        b).  With no update installed it is the plain solve of that direction (info.k == 0)."""
        op = _op(trans)
        steps = _lowrank_steps(steps)
        self._lowrank_real("solve_lowrank")
        if len(b) != self.n:
            raise DimensionMismatch(f"`b` does not have same size as F: length(b)={len(b)}, F.n={self.n}")
        bb = np.ascontiguousarray(b, dtype=np.float64)
        if x is None:
            x = np.empty(self.n)
        elif len(x) != self.n:
            raise DimensionMismatch(f"`x` does not have same size as F: length(x)={len(x)}, F.n={self.n}")
        xx = x if (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous) \
            else np.empty(self.n)
        ci = C.SmluLowrankInfo()
        rc = _check(C.lib().smlu_solve_lowrank(self._h, op, steps, C.ptr(bb), C.ptr(xx), ctypes.byref(ci)), self._h)
        if xx is not x:
            x[:] = xx
        return x, _lowrank_info(rc, ci)

    def solve_lowrank_device(self, d_x, d_b, trans="N", steps=-1):
        """solve_lowrank on device vectors (torch tensors or raw pointer ints; d_x may be d_b).  Returns
        info (smlu_solve_lowrank_device, ordered after the stream that produced d_b)."""
        op = _op(trans)
        steps = _lowrank_steps(steps)
        self._lowrank_real("solve_lowrank_device")
        for name, t in (("d_x", d_x), ("d_b", d_b)):
            _device_f64(name, t, self.n)
        px = d_x.data_ptr() if hasattr(d_x, "data_ptr") else int(d_x)
        pb = d_b.data_ptr() if hasattr(d_b, "data_ptr") else int(d_b)
        ci = C.SmluLowrankInfo()
        with C.caller_stream(self._h, d_b):
            rc = _check(C.lib().smlu_solve_lowrank_device(self._h, op, steps, ctypes.c_void_p(pb), ctypes.c_void_p(px),
                                                          ctypes.byref(ci)), self._h)
        return _lowrank_info(rc, ci)

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            C.lib().smlu_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self):
        return f"ParallelSparseLU(n={self.n}, nnz(L+U)={self.stat('nnzLU'):.0f})"


def lu_(F: ParallelSparseLU, A):
    """lu!(F, A) — src/SharedMemSparseLU.jl:245-279.  Same pattern: numeric refactor on the
    GPU; different pattern: re-analysis (the reference's reallocate branch, :252-273)."""
    A = _csc(A)
    if A.shape != (F.m, F.n):
        raise DimensionMismatch(f"A has size {A.shape}, F has size {(F.m, F.n)}")
    if A.dtype == np.complex128 and not F.is_complex:
        raise TypeError("complex values for a real factorization (create it from a complex matrix)")
    vals = np.ascontiguousarray(A.data, dtype=F._dt)   # real values into a complex F are promoted
    L = C.lib()
    same = (A.nnz == F._rowval.size and np.array_equal(A.indptr, F._colptr)
            and np.array_equal(A.indices, F._rowval))
    if same:
        rc = (L.smlu_refactor_z if F.is_complex else L.smlu_refactor)(F._h, C.ptr(vals))
    else:
        F._colptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        F._rowval = np.ascontiguousarray(A.indices, dtype=np.int64)
        fn = L.smlu_refactor_csc_z if F.is_complex else L.smlu_refactor_csc
        colptr, rowval = F._colptr + F._base, F._rowval + F._base
        rc = fn(F._h, F.n, C.ptr(colptr), C.ptr(rowval), C.ptr(vals))
    F._factors = None
    F._zfactors = None
    _check(rc, F._h)
    if rc == C.SMLU_SINGULAR:
        raise SingularException(L.smlu_last_error_col(F._h))
    return None


def ldiv_(x, F: ParallelSparseLU, b, trans="N"):
    """ldiv!(x, F, b) — src/SharedMemSparseLU.jl:286-342.  ``x is b`` is allowed.
    trans="T" solves ``A.T x = b`` and trans="C" ``A.conj().T x = b`` from the same factors
    (Julia's ``ldiv!(x, transpose(F), b)`` / ``ldiv!(x, F', b)``; smlu_solve_trans*).  2D ``x`` / ``b``
    (columns) are solved in batches of up to 16 in either direction; a transposed batch gives every
    column bitwise its single-vector result."""
    op = _op(trans)
    if F.m != F.n:
        raise DimensionMismatch(f"`F` is not square: F.m={F.m}, F.n={F.n}")
    if len(x) != F.n:
        raise DimensionMismatch(f"`x` does not have same size as F: length(x)={len(x)}, F.n={F.n}")
    if len(b) != F.n:
        raise DimensionMismatch(f"`b` does not have same size as F: length(b)={len(b)}, F.n={F.n}")
    if not F.is_complex and (np.iscomplexobj(b) or np.iscomplexobj(x)):
        raise TypeError("complex vectors need a factorization of a complex matrix")
    _need_complex_x(F, x)
    if np.ndim(b) == 2 or np.ndim(x) == 2:
        # several right-hand sides (columns), SURVEY §8f-4: one C-ABI call, column-major buffers
        if np.shape(x) != np.shape(b):
            raise DimensionMismatch(f"`x` has size {np.shape(x)}, `b` has size {np.shape(b)}")
        nrhs = np.shape(b)[1]
        dt = F._dt
        bb = np.asfortranarray(b, dtype=dt)
        xx = x if (isinstance(x, np.ndarray) and x.dtype == dt and x.flags.f_contiguous) \
            else np.empty((F.n, nrhs), dtype=dt, order="F")
        ld = 2 * F.n if F.is_complex else F.n   # leading dimension in doubles
        if op != C.SMLU_OP_N:
            _check(C.lib().smlu_solve_trans_multi(F._h, op, nrhs, C.ptr(bb), ld, C.ptr(xx), ld), F._h)
        else:
            _check(C.lib().smlu_solve_multi(F._h, nrhs, C.ptr(bb), ld, C.ptr(xx), ld), F._h)
        if xx is not x:
            x[:, :] = xx
        return x
    bb = np.ascontiguousarray(b, dtype=F._dt)
    xx = x if (isinstance(x, np.ndarray) and x.dtype == F._dt and x.flags.c_contiguous) \
        else np.empty(F.n, dtype=F._dt)
    if op != C.SMLU_OP_N:
        _check(C.lib().smlu_solve_trans(F._h, op, C.ptr(bb), C.ptr(xx)), F._h)
    else:
        _check(C.lib().smlu_solve(F._h, C.ptr(bb), C.ptr(xx)), F._h)
    if xx is not x:
        x[:] = xx
    return x


def ldiv_refined_(X, F: ParallelSparseLU, B, trans="N", steps=None):
    """ldiv!(X, F, B) for 2D ``X`` / ``B`` (columns) with iterative refinement run as a batch
    (smlu_solve_refined_multi): up to 16 columns share every pass, each column is refined by the rule
    of the single solve and is bitwise ``ldiv_(x, F, b, trans)`` of that column.  ``X is B`` is
    allowed.  steps as in ParallelSparseLU.solve_refined_multi_device, whose dict it returns."""
    op = _op(trans)
    if np.ndim(B) != 2 or np.shape(X) != np.shape(B):
        raise DimensionMismatch(f"`X` has size {np.shape(X)}, `B` has size {np.shape(B)}: two equal 2D arrays")
    if np.shape(B)[0] != F.n:
        raise DimensionMismatch(f"`B` does not have same size as F: size(B, 1)={np.shape(B)[0]}, F.n={F.n}")
    if not F.is_complex and (np.iscomplexobj(B) or np.iscomplexobj(X)):
        raise TypeError("complex vectors need a factorization of a complex matrix")
    _need_complex_x(F, X)
    nrhs = np.shape(B)[1]
    dt = F._dt
    bb = np.asfortranarray(B, dtype=dt)
    xx = X if (isinstance(X, np.ndarray) and X.dtype == dt and X.flags.f_contiguous) \
        else np.empty((F.n, nrhs), dtype=dt, order="F")
    ld = 2 * F.n if F.is_complex else F.n   # leading dimension in doubles
    info = (C.SmluRefineInfo * max(nrhs, 1))()
    _check(C.lib().smlu_solve_refined_multi(F._h, op, _refine_steps(steps), nrhs, C.ptr(bb), ld, C.ptr(xx), ld, info),
           F._h)
    if xx is not X:
        X[:, :] = xx
    return _refine_info(info, nrhs)


def _need_complex_x(F, x):
    """A complex factorization writes a complex solution: a real x would silently drop the
    imaginary part (Julia raises InexactError there), so it is refused."""
    if F.is_complex and not np.iscomplexobj(x):
        raise TypeError("the solution of a complex factorization needs a complex x")


def _tri(F, x, which):
    _need_complex_x(F, x)
    if len(x) != F.n:
        raise DimensionMismatch(f"`x` does not have same size as F: length(x)={len(x)}, F.n={F.n}")
    xx = x if (isinstance(x, np.ndarray) and x.dtype == F._dt and x.flags.c_contiguous) \
        else np.ascontiguousarray(x, dtype=F._dt)
    fn = C.lib().smlu_lsolve if which == "L" else C.lib().smlu_rsolve
    _check(fn(F._h, C.ptr(xx)), F._h)
    if xx is not x:
        x[:] = xx
    return None


def lsolve_(F: ParallelSparseLU, x):
    """lsolve!(F, x) — src/SharedMemSparseLU.jl:349-367: in place ``L \\ x``."""
    return _tri(F, x, "L")


def rsolve_(F: ParallelSparseLU, x):
    """rsolve!(F, x) — src/SharedMemSparseLU.jl:374-392: in place ``U \\ x``."""
    return _tri(F, x, "U")


def chunked_setup(F: ParallelSparseLU, chunk_size=None):
    """Build the reference's dense-chunk solve layout on the GPU from F's current factors
    (get_chunking_parameters / allocate_chunks / fill_chunks!, src/SharedMemSparseLU.jl:101-243;
    chunk_size defaults to 8 as :67-70).  SURVEY §8f-3 parity mode for small banded systems."""
    _check(C.lib().smlu_chunked_setup(F._h, 0 if chunk_size is None else int(chunk_size)), F._h)


def chunked_ldiv_(x, F: ParallelSparseLU, b):
    """ldiv!(x, F, b) (:286-342) through the chunked layout: lsolve!/rsolve! (:349-392) chunk by
    chunk on the GPU.  Same DimensionMismatch checks as ldiv_; x may be b."""
    if len(x) != F.n or len(b) != F.n:
        raise DimensionMismatch(f"x and b must have length F.n={F.n}: {len(x)}, {len(b)}")
    _need_complex_x(F, x)
    bb = np.ascontiguousarray(b, dtype=F._dt)
    xx = np.empty(F.n, dtype=F._dt)
    _check(C.lib().smlu_chunked_ldiv(F._h, C.ptr(bb), C.ptr(xx)), F._h)
    x[:] = xx
    return x


def cleanup_ParallelSparseLU_(F: ParallelSparseLU):
    """cleanup_ParallelSparseLU!(F) — exported but undefined in the reference (:31); here it
    releases the device memory, stream and host plan of F."""
    F.close()


def allocate_shared(T, *dims):
    """allocate_shared — exported but undefined in the reference (:31).  There are no MPI
    shared-memory windows on the GPU path; this returns a zeroed host array of the shape."""
    return np.zeros(dims, dtype=T)
