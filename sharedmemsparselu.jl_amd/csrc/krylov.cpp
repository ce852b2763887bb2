// krylov.cpp — solve with stale factors: restarted, right-preconditioned GMRES(m) for op(A') x = b,
// A' on the handle's pattern with the caller's values (NULL: the handle's own), preconditioned by the
// handle's current factorization M = LU ~ op(A) (PARDISO's "iterate with the previous LU"; not in
// the reference).  All n-vectors stay on the device (kernels_krylov.hip); the host reads one 64-byte
// record per Arnoldi step and one per true residual.
//
//   x = 0
//   cycle:  r = b - op(A') x, beta = ||r||           (true residual; the only convergence test)
//           v_0 = r / beta, g = beta e_0
//           step j:  z = M^-1 v_j;  w = op(A') z;  h = V^T w, w -= V h;  h2 = V^T w, w -= V h2  (CGS2)
//                    h_{j+1,j} = ||w||;  column h + h2 through the rotations;  estimate |g_{j+1}|
//                    end on estimate <= rtol ||b||, j + 1 == restart, maxit, or h_{j+1,j} == 0
//           R y = g;  x += M^-1 (V y)
// so a call runs iters + cycles factor solves.  The solves are the plain factor solves
// run_solve_dev / run_solve_t_dev, never refined (as smlu_rcond).
#include "handle.hpp"

namespace {

double as_double(long long w) {
  double v;
  std::memcpy(&v, &w, sizeof v);
  return v;
}

// an allocation that does not fit is SMLU_ERR_ALLOC, not a HIP error
template <class T>
int kry_alloc(smlu_handle* h, DBuf<T>& b, size_t cnt, const char* what) {
  b.free();
  if (b.alloc(cnt) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    b.n = 0;
    return fail(h, SMLU_ERR_ALLOC, std::string("smlu_solve_gmres: no device memory for ") + what);
  }
  return SMLU_OK;
}

// Work buffers for `restart`: restart + 1 basis columns of leading dimension ldv (n rounded up to
// even), the vectors z, w, b of the same length, the partials, the state and the record.  The pad
// row of every vector is zero and stays zero: the kernels that store pairs store 0 there whatever
// they computed (a NaN coefficient times the zero pad is NaN).  Each group is all or nothing:
// kry_cols / kry_ready are set last, and a failure part-way frees the group, so a call after
// SMLU_ERR_ALLOC allocates again and never launches on a missing buffer.
int kry_buffers(smlu_handle* h, int restart, bool host_x, bool host_vals) {
  const int64_t n = h->plan.n, ldv = n + (n & 1);
  hipStream_t st = h->stream;
  int rc;
  if (h->kry_cols < restart + 1) {
    h->kry_cols = 0;
    if ((rc = kry_alloc(h, h->kry_V, (size_t)ldv * (restart + 1), "the basis")) != SMLU_OK) return rc;
    if (hipMemsetAsync(h->kry_V.p, 0, sizeof(double) * ldv * (restart + 1), st) != hipSuccess) {
      (void)hipGetLastError();
      h->kry_V.free();
      return fail(h, SMLU_ERR_HIP, "smlu_solve_gmres: clearing the basis failed");
    }
    h->kry_cols = restart + 1;
  }
  if (!h->kry_ready) {
    auto group = [&]() -> int {
      int r;
      DBuf<double>* v[] = {&h->kry_z, &h->kry_w, &h->kry_b};
      for (auto* b : v) {
        if ((r = kry_alloc(h, *b, (size_t)ldv, "the work vectors")) != SMLU_OK) return r;
        HIPCHK(hipMemsetAsync(b->p, 0, sizeof(double) * ldv, st));
      }
      if ((r = kry_alloc(h, h->kry_part, (size_t)kDgMaxBlocks * kKryPartStride, "the partials")) != SMLU_OK) return r;
      if ((r = kry_alloc(h, h->kry_state, (size_t)kKryStateWords, "the state")) != SMLU_OK) return r;
      if ((r = kry_alloc(h, h->kry_rec, 8, "the record")) != SMLU_OK) return r;
      HIPCHK(hipMemsetAsync(h->kry_state.p, 0, sizeof(double) * kKryStateWords, st));
      HIPCHK(hipMemsetAsync(h->kry_rec.p, 0, 8 * sizeof(long long), st));
      return SMLU_OK;
    };
    if ((rc = group()) != SMLU_OK) {
      DBuf<double>* v[] = {&h->kry_z, &h->kry_w, &h->kry_b, &h->kry_part, &h->kry_state};
      for (auto* b : v) b->free();
      h->kry_rec.free();
      return rc;
    }
    h->kry_ready = true;
  }
  if (host_x && !h->kry_x.p && (rc = kry_alloc(h, h->kry_x, (size_t)ldv, "x")) != SMLU_OK) return rc;
  if (host_vals && !h->kry_vals.p &&
      (rc = kry_alloc(h, h->kry_vals, (size_t)std::max<int64_t>(h->plan.nnzA, 1), "the values")) != SMLU_OK)
    return rc;
  if (!h->Acolp.p && h->Acolp.upload(h->plan.Acolptr.data(), h->plan.Acolptr.size(), st) != hipSuccess) {
    (void)hipGetLastError();
    h->Acolp.free();
    return fail(h, SMLU_ERR_HIP, "smlu_solve_gmres: uploading A's column pointers failed");
  }
  return ensure_acol(h);
}

// the record stamped `seq`, after the work on the handle's stream (dg_read's rule)
int kry_read(smlu_handle* h, long long seq, long long out[8]) {
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int attempt = 0; attempt < 4; ++attempt) {
    HIPCHK(hipMemcpy(out, h->kry_rec.p, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    if (out[0] == seq && out[7] == seq) return SMLU_OK;
    ++h->status_copy_retries;
  }
  return fail(h, SMLU_ERR_HIP, "GMRES record read back with a wrong sequence stamp (device-to-host copy)");
}

int check_args(smlu_handle* h, int op, const double* b, double* x, const smlu_gmres_opts* o) {
  if (!h || !b || !x) return fail(h, SMLU_ERR_ARG, "NULL argument");
  if (op != SMLU_OP_N && op != SMLU_OP_T && op != SMLU_OP_H)
    return fail(h, SMLU_ERR_ARG, "op must be SMLU_OP_N, SMLU_OP_T or SMLU_OP_H");
  if (o->restart < 1 || o->restart > kKryMaxRestart) return fail(h, SMLU_ERR_ARG, "restart must be in 1..32");
  if (o->maxit < 1) return fail(h, SMLU_ERR_ARG, "maxit must be at least 1");
  if (!(std::isfinite(o->rtol) && o->rtol >= 0.0)) return fail(h, SMLU_ERR_ARG, "rtol must be finite and >= 0");
  if (!h->have_numeric || h->errcol >= 0)
    return fail(h, SMLU_ERR_STATE, "smlu_solve_gmres: no numeric factorization (none yet, or a singular one)");
  if (h->nranks > 1) return fail(h, SMLU_ERR_STATE, "smlu_solve_gmres is single-GPU only (partitioned handle)");
  if (h->zc) return fail(h, SMLU_ERR_STATE, "smlu_solve_gmres: ComplexF64 handles are not supported");
  return SMLU_OK;
}

// GMRES on device vectors: a = A''s values, db the handle's copy of b, dx the iterate (both of n
// doubles; dx is written from the start).  Buffers are in place and the stream is ordered.
int run_gmres(smlu_handle* h, bool trans, const double* a, const double* db, double* dx, const smlu_gmres_opts& o,
              smlu_gmres_info* info) {
  const Plan& P = h->plan;
  const int64_t n = P.n, ldv = n + (n & 1);
  hipStream_t st = h->stream;
  double* V = h->kry_V.p;
  double *z = h->kry_z.p, *w = h->kry_w.p, *part = h->kry_part.p;
  void* state = h->kry_state.p;
  long long* drec = h->kry_rec.p;
  long long rec[8];
  int rc;
  auto t0 = std::chrono::steady_clock::now();
  h->gmres_iters = h->gmres_cycles = h->gmres_solves = 0;
  auto msolve = [&](const double* in, double* out) {   // out = M^-1 in, the plain factor solve
    ++h->gmres_solves;
    return trans ? run_solve_t_dev(h, 0, in, out) : run_solve_dev(h, in, out, 0);
  };
  // r = b - op(A') x into v_0 (x = nullptr: x = 0) with ||r|| and the backward error of x
  auto residual = [&](const double* x, double* nrm, double* berr) {
    const long long seq = ++h->kry_seq;
    HIPCHK(launch_kry_resid(st, trans, n, h->Arowptr.p, h->Arow_ent.p, h->Acol.p, h->Acolp.p, h->Arow.p, a, x, db, V,
                            part, state, drec, seq));
    int r = kry_read(h, seq, rec);
    if (r != SMLU_OK) return r;
    *nrm = as_double(rec[1]);
    *berr = as_double(rec[2]);
    return (int)SMLU_OK;
  };
  double bnorm = 0, beta = 0, berr = 0, est = 0, prev = HUGE_VAL;
  bool converged = false, on_estimate = false;
  int iters = 0, cycles = 0;
  HIPCHK(hipMemsetAsync(dx, 0, sizeof(double) * n, st));
  if ((rc = residual(nullptr, &bnorm, &berr)) != SMLU_OK) return rc;
  beta = bnorm;
  est = bnorm;
  const double tol = o.rtol * bnorm;
  if (bnorm == 0.0) converged = true;   // b = 0: x = 0
  while (!converged && std::isfinite(beta)) {
    if (cycles > 0) {
      if ((rc = residual(dx, &beta, &berr)) != SMLU_OK) return rc;
      if (!std::isfinite(beta)) break;
      if (beta <= tol) {
        converged = true;
        break;
      }
      if (on_estimate && beta > 0.5 * prev) break;   // stagnation
    }
    if (iters >= o.maxit) break;
    prev = beta;
    on_estimate = false;
    ++cycles;
    int k = 0;   // steps of this cycle
    bool finite = true;
    for (int j = 0; j < o.restart; ++j) {
      double* vj = V + (int64_t)j * ldv;
      if ((rc = msolve(vj, z)) != SMLU_OK) return rc;
      HIPCHK(launch_kry_spmv(st, trans, n, h->Arowptr.p, h->Arow_ent.p, h->Acol.p, h->Acolp.p, h->Arow.p, a, z, state,
                             vj, w));
      const long long seq = ++h->kry_seq;
      HIPCHK(launch_kry_arnoldi(st, n, ldv, j, V, w, part, state, drec, seq));
      if ((rc = kry_read(h, seq, rec)) != SMLU_OK) return rc;
      est = as_double(rec[1]);
      const double hn = as_double(rec[2]);
      ++iters;
      if (!std::isfinite(est) || !std::isfinite(hn)) {
        finite = false;
        break;
      }
      k = j + 1;
      if (est <= tol || hn == 0.0) {
        on_estimate = true;
        break;
      }
      if (iters >= o.maxit) break;
    }
    if (!finite) {   // x stays the last iterate; its residual for the report
      if ((rc = residual(dx, &beta, &berr)) != SMLU_OK) return rc;
      break;
    }
    HIPCHK(launch_kry_update(st, n, ldv, k, V, state, w));
    if ((rc = msolve(w, z)) != SMLU_OK) return rc;
    HIPCHK(launch_axpy1(st, n, z, dx));
  }
  HIPCHK(hipStreamSynchronize(st));
  h->gmres_iters = iters;
  h->gmres_cycles = cycles;
  h->gmres_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (info) {
    info->converged = converged ? 1 : 0;
    info->iters = iters;
    info->cycles = cycles;
    info->solves = (int32_t)h->gmres_solves;
    info->relres = bnorm > 0.0 ? beta / bnorm : 0.0;
    info->relres_est = bnorm > 0.0 ? est / bnorm : 0.0;
    info->berr = berr;
    info->bnorm = bnorm;
  }
  return converged ? SMLU_OK : SMLU_NOT_CONVERGED;
}

}  // namespace

void smlu_gmres_default_opts(smlu_gmres_opts* o) {
  if (!o) return;
  o->rtol = 1e-10;
  o->restart = 30;
  o->maxit = 200;
}

int smlu_solve_gmres_device(smlu_handle* h, int op, const double* d_nzval, const double* d_b, double* d_x,
                            const smlu_gmres_opts* opts, smlu_gmres_info* info) {
  smlu_gmres_opts o;
  smlu_gmres_default_opts(&o);
  if (opts) o = *opts;
  int rc = check_args(h, op, d_b, d_x, &o);
  if (rc != SMLU_OK) return rc;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(after_caller(h));
  if ((rc = kry_buffers(h, o.restart, false, false)) != SMLU_OK) return rc;
  // x may be b: the handle keeps its own copy of b
  HIPCHK(hipMemcpyAsync(h->kry_b.p, d_b, sizeof(double) * h->plan.n, hipMemcpyDeviceToDevice, h->stream));
  return run_gmres(h, op != SMLU_OP_N, d_nzval ? d_nzval : h->A.p, h->kry_b.p, d_x, o, info);
}

int smlu_solve_gmres(smlu_handle* h, int op, const double* nzval, const double* b, double* x,
                     const smlu_gmres_opts* opts, smlu_gmres_info* info) {
  smlu_gmres_opts o;
  smlu_gmres_default_opts(&o);
  if (opts) o = *opts;
  int rc = check_args(h, op, b, x, &o);
  if (rc != SMLU_OK) return rc;
  HIPCHK(hipSetDevice(h->device));
  if ((rc = kry_buffers(h, o.restart, true, nzval != nullptr)) != SMLU_OK) return rc;
  const int64_t n = h->plan.n;
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(h->kry_b.p, b, sizeof(double) * n, hipMemcpyHostToDevice, st));
  if (nzval) HIPCHK(hipMemcpyAsync(h->kry_vals.p, nzval, sizeof(double) * h->plan.nnzA, hipMemcpyHostToDevice, st));
  rc = run_gmres(h, op != SMLU_OP_N, nzval ? h->kry_vals.p : h->A.p, h->kry_b.p, h->kry_x.p, o, info);
  if (rc < 0) return rc;
  HIPCHK(hipMemcpyAsync(x, h->kry_x.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return rc;
}
