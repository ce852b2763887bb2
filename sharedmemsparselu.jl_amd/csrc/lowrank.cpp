// lowrank.cpp — low-rank updates of the solve: op(A + U V^T) x = b from the handle's current factors
// of A by the Sherman-Morrison-Woodbury identity (what MUMPS and PARDISO users do by hand on the host
// for a few changed columns, dense constraint rows or a bordered system; not in the reference).
// All n-vectors stay on the device (kernels_lowrank.hip); the host reads one 64-byte record per set and
// one per residual.
//
//   set:    Y = A^-1 U (k columns, 16 per solve pass);  C = I + V^T Y;  LU of C, C^-1 kept
//   solve:  N:  y0 = A^-1 b;   t = V^T y0;  x = y0 - Y  C^-1 t
//           T:  y0 = A^-T b;   t = U^T y0;  x = y0 - Yt C^-T t,   Yt = A^-T V on the first such solve
//   refinement on the updated system, solve_refined_by's rule (solve.cpp):
//           r = b - op(A) x - W (Wd^T x)  (N: W = U, Wd = V; T: W = V, Wd = U);  x += correction of r
// The solves are the plain factor solves run_solve_dev / run_solve_t_dev, never refined (as
// smlu_rcond and smlu_solve_gmres).  The update belongs to the factorization it was installed on:
// it is in force while lr_version == nfactor, so every refactor drops it.
#include "handle.hpp"

namespace {

double as_double(long long w) {
  double v;
  std::memcpy(&v, &w, sizeof v);
  return v;
}

// an allocation that does not fit is SMLU_ERR_ALLOC, not a HIP error; the buffer is cleared
int lr_alloc(smlu_handle* h, DBuf<double>& b, size_t cnt, const char* what) {
  b.free();
  if (b.alloc(cnt) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    b.n = 0;
    return fail(h, SMLU_ERR_ALLOC, std::string("smlu_lowrank: no device memory for ") + what);
  }
  HIPCHK(hipMemsetAsync(b.p, 0, sizeof(double) * cnt, h->stream));
  return SMLU_OK;
}

// The small buffers: three n-vectors of leading dimension ld (b, x, r; the pad row zero and kept
// zero), the partials, the state and the record.  All or nothing, as kry_buffers.
int lr_vectors(smlu_handle* h, bool trans) {
  const int64_t n = h->plan.n, ld = n + (n & 1);
  int rc;
  if (!h->lr_ready) {
    auto group = [&]() -> int {
      int r;
      DBuf<double>* v[] = {&h->lr_b, &h->lr_x, &h->lr_r};
      for (auto* b : v)
        if ((r = lr_alloc(h, *b, (size_t)ld, "the work vectors")) != SMLU_OK) return r;
      if ((r = lr_alloc(h, h->lr_part, (size_t)kDgMaxBlocks * kLrPartStride, "the partials")) != SMLU_OK) return r;
      if ((r = lr_alloc(h, h->lr_gpart, (size_t)kDgMaxBlocks * kLrMax * kLrMax, "the Gram partials")) != SMLU_OK) return r;
      if ((r = lr_alloc(h, h->lr_state, (size_t)kLrStateWords, "the state")) != SMLU_OK) return r;
      h->lr_rec.free();
      if (h->lr_rec.alloc(8) != hipSuccess) {
        (void)hipGetLastError();
        h->lr_rec.p = nullptr;
        return fail(h, SMLU_ERR_ALLOC, "smlu_lowrank: no device memory for the record");
      }
      HIPCHK(hipMemsetAsync(h->lr_rec.p, 0, 8 * sizeof(long long), h->stream));
      return SMLU_OK;
    };
    if ((rc = group()) != SMLU_OK) {
      DBuf<double>* v[] = {&h->lr_b, &h->lr_x, &h->lr_r, &h->lr_part, &h->lr_gpart, &h->lr_state};
      for (auto* b : v) b->free();
      h->lr_rec.free();
      return rc;
    }
    h->lr_ready = true;
  }
  if (trans && !h->Acolp.p && h->Acolp.upload(h->plan.Acolptr.data(), h->plan.Acolptr.size(), h->stream) != hipSuccess) {
    (void)hipGetLastError();
    h->Acolp.free();
    return fail(h, SMLU_ERR_HIP, "smlu_lowrank: uploading A's column pointers failed");
  }
  return ensure_acol(h);
}

// U, V and Y for k columns: grown together, all or nothing (lr_cols is set last).  Growing drops Yt.
int lr_columns(smlu_handle* h, int k) {
  const int64_t n = h->plan.n, ld = n + (n & 1);
  if (h->lr_cols >= k) return SMLU_OK;
  h->lr_cols = 0;
  h->lr_cols_t = 0;
  h->lr_Yt.free();
  DBuf<double>* v[] = {&h->lr_U, &h->lr_V, &h->lr_Y};
  for (auto* b : v) {
    int rc = lr_alloc(h, *b, (size_t)ld * k, "U, V and Y");
    if (rc != SMLU_OK) {
      for (auto* c : v) c->free();
      return rc;
    }
  }
  h->lr_cols = k;
  return SMLU_OK;
}

// the record stamped `seq`, after the work on the handle's stream (dg_read's rule)
int lr_read(smlu_handle* h, long long seq, long long out[8]) {
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int attempt = 0; attempt < 4; ++attempt) {
    HIPCHK(hipMemcpy(out, h->lr_rec.p, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    if (out[0] == seq && out[7] == seq) return SMLU_OK;
    ++h->status_copy_retries;
  }
  return fail(h, SMLU_ERR_HIP, "low-rank record read back with a wrong sequence stamp (device-to-host copy)");
}

// krylov.cpp's check_args: the state a low-rank call needs
int check_state(smlu_handle* h, const char* who) {
  if (!h->have_numeric || h->errcol >= 0)
    return fail(h, SMLU_ERR_STATE, std::string(who) + ": no numeric factorization (none yet, or a singular one)");
  if (h->nranks > 1) return fail(h, SMLU_ERR_STATE, std::string(who) + " is single-GPU only (partitioned handle)");
  if (h->zc) return fail(h, SMLU_ERR_STATE, std::string(who) + ": ComplexF64 handles are not supported");
  return SMLU_OK;
}

void fill_info(smlu_lowrank_info* info, int k, int steps, int stop, int64_t solves, double berr, double resid,
               double rcond, double pmin, double gmax) {
  if (!info) return;
  info->k = k;
  info->steps = steps;
  info->stop = stop;
  info->solves = (int32_t)solves;
  info->berr = berr;
  info->resid = resid;
  info->rcond_c = rcond;
  info->pivot_min = pmin;
  info->gram_max = gmax;
}

// out = op(A)^-1 in for nb <= kMultiRhs columns of leading dimension ld (in may be out)
int factor_solve(smlu_handle* h, bool trans, const double* in, double* out, int nb, int64_t ld) {
  ++h->lowrank_solves;
  return trans ? run_solve_t_dev(h, 0, in, out, nb, ld, ld) : run_solve_dev(h, in, out, 0, nb, ld, ld);
}

// Y (trans: Yt) = op(A)^-1 W, k columns in batches of kMultiRhs
int solve_columns(smlu_handle* h, bool trans, int k, const double* W, double* Y) {
  const int64_t n = h->plan.n, ld = n + (n & 1);
  for (int j = 0; j < k; j += kMultiRhs) {
    const int nb = std::min(kMultiRhs, k - j);
    int rc = factor_solve(h, trans, W + (size_t)j * ld, Y + (size_t)j * ld, nb, ld);
    if (rc != SMLU_OK) return rc;
  }
  return SMLU_OK;
}

// U and V are staged in lr_U / lr_V and the stream is ordered: Y, C, its inverse, the record.
int run_set(smlu_handle* h, int k, smlu_lowrank_info* info, std::chrono::steady_clock::time_point t0) {
  const int64_t n = h->plan.n, ld = n + (n & 1);
  hipStream_t st = h->stream;
  int rc = solve_columns(h, false, k, h->lr_U.p, h->lr_Y.p);
  if (rc != SMLU_OK) return rc;
  const long long seq = ++h->lr_seq;
  HIPCHK(launch_lr_capacitance(st, n, ld, k, h->lr_V.p, h->lr_Y.p, h->lr_gpart.p, h->lr_state.p, h->lr_rec.p, seq));
  long long rec[8];
  if ((rc = lr_read(h, seq, rec)) != SMLU_OK) return rc;
  const bool singular = rec[1] != 0;
  h->lowrank_set_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_info(info, singular ? 0 : k, 0, 0, h->lowrank_solves, -1.0, -1.0, as_double(rec[2]), as_double(rec[3]),
            as_double(rec[4]));
  if (singular)
    return fail(h, SMLU_SINGULAR,
                rec[1] == 2 ? "smlu_lowrank_set: the capacitance matrix I + V^T A^-1 U has a non-finite entry"
                            : "smlu_lowrank_set: the capacitance matrix I + V^T A^-1 U is singular (A + U V^T is)");
  h->lr_k = k;
  h->lr_version = h->nfactor;
  return SMLU_OK;
}

int check_set(smlu_handle* h, int32_t k, const double* U, int64_t ldu, const double* V, int64_t ldv) {
  if (!h) return fail(h, SMLU_ERR_ARG, "NULL handle");
  if (k < 0 || k > SMLU_LOWRANK_MAX) return fail(h, SMLU_ERR_ARG, "k must be in 0..32");
  if (k > 0 && (!U || !V)) return fail(h, SMLU_ERR_ARG, "NULL argument");
  if (k > 0 && (ldu < h->plan.n || ldv < h->plan.n)) return fail(h, SMLU_ERR_ARG, "leading dimension smaller than n");
  return SMLU_OK;
}

// What every set of k > 0 starts with.  A call refused for its arguments or the handle's state
// (a negative code) leaves an installed update as it was; past these checks nothing is installed
// until the call succeeds.
int begin_set(smlu_handle* h) {
  int rc = check_state(h, "smlu_lowrank_set");
  if (rc != SMLU_OK) return rc;
  h->lr_k = 0;
  h->lr_have_t = false;
  h->lowrank_solves = 0;
  HIPCHK(hipSetDevice(h->device));
  return SMLU_OK;
}

int check_solve(smlu_handle* h, int op, int max_steps, const double* b, double* x) {
  if (!h || !b || !x) return fail(h, SMLU_ERR_ARG, "NULL argument");
  if (op != SMLU_OP_N && op != SMLU_OP_T && op != SMLU_OP_H)
    return fail(h, SMLU_ERR_ARG, "op must be SMLU_OP_N, SMLU_OP_T or SMLU_OP_H");
  if (max_steps < -1) return fail(h, SMLU_ERR_ARG, "max_steps must be -1 (up to 3), 0 or a step limit");
  return check_state(h, "smlu_solve_lowrank");
}

// The solve on the handle's vectors: b in lr_b, x into lr_x.  Buffers are in place, the stream ordered.
int run_solve(smlu_handle* h, bool trans, int max_steps, smlu_lowrank_info* info) {
  const Plan& P = h->plan;
  const int64_t n = P.n, ld = n + (n & 1);
  hipStream_t st = h->stream;
  const int k = h->lowrank_k();
  const int steps = max_steps < 0 ? 3 : max_steps;
  auto t0 = std::chrono::steady_clock::now();
  h->lowrank_solves = 0;
  int rc;
  if (trans && k > 0 && !h->lr_have_t) {   // Yt = A^-T V, once per installed update
    if (h->lr_cols_t < h->lr_cols) {
      h->lr_cols_t = 0;
      if ((rc = lr_alloc(h, h->lr_Yt, (size_t)ld * h->lr_cols, "Yt")) != SMLU_OK) return rc;
      h->lr_cols_t = h->lr_cols;
    }
    if ((rc = solve_columns(h, true, k, h->lr_V.p, h->lr_Yt.p)) != SMLU_OK) return rc;
    h->lr_have_t = true;
    h->lowrank_solves = 0;   // the call reports the passes of its own solve and corrections
  }
  // N: W = U, Wd = V, Yw = Y;  T: W = V, Wd = U, Yw = Yt
  const double* W = trans ? h->lr_V.p : h->lr_U.p;
  const double* Wd = trans ? h->lr_U.p : h->lr_V.p;
  const double* Yw = trans ? h->lr_Yt.p : h->lr_Y.p;
  double *b = h->lr_b.p, *x = h->lr_x.p, *r = h->lr_r.p, *part = h->lr_part.p;
  // v = (op(A) + W Wd^T)^-1 v in place
  auto solve = [&](double* in, double* out) {
    int r2 = factor_solve(h, trans, in, out, 1, ld);
    if (r2 != SMLU_OK) return r2;
    if (k > 0) HIPCHK(launch_lr_correct(st, trans, n, ld, k, Wd, Yw, h->lr_state.p, part, out));
    return (int)SMLU_OK;
  };
  if ((rc = solve(b, x)) != SMLU_OK) return rc;
  const double eps = std::ldexp(1.0, -51);   // 4 unit roundoffs (solve_refined_by)
  double prev = HUGE_VAL, berr = -1.0, resid = -1.0;
  int done = 0, stop = 0;
  for (int it = 0; it < steps; ++it) {
    const long long seq = ++h->lr_seq;
    HIPCHK(launch_lr_resid(st, trans, n, ld, k, h->Arowptr.p, h->Arow_ent.p, h->Acol.p, h->Acolp.p, h->Arow.p, h->A.p, x,
                           b, W, Wd, r, part, h->lr_rec.p, seq));
    long long rec[8];
    if ((rc = lr_read(h, seq, rec)) != SMLU_OK) return rc;
    resid = as_double(rec[1]);
    berr = as_double(rec[2]);
    if (berr <= eps) {
      stop = 1;
      break;
    }
    if (berr > 0.5 * prev) {
      stop = 2;
      break;
    }
    prev = berr;
    if ((rc = solve(r, r)) != SMLU_OK) return rc;
    HIPCHK(launch_axpy1(st, n, r, x));
    ++done;
  }
  if (steps > 0 && stop == 0) stop = 3;   // the step limit
  HIPCHK(hipStreamSynchronize(st));
  h->lowrank_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fill_info(info, k, done, stop, h->lowrank_solves, berr, resid, -1.0, -1.0, -1.0);
  return SMLU_OK;
}

}  // namespace

int smlu_lowrank_clear(smlu_handle* h) {
  if (!h) return fail(h, SMLU_ERR_ARG, "NULL handle");
  h->lr_k = 0;
  h->lr_have_t = false;
  return SMLU_OK;
}

int smlu_lowrank_set_device(smlu_handle* h, int32_t k, const double* d_U, int64_t ldu, const double* d_V, int64_t ldv,
                            smlu_lowrank_info* info) {
  fill_info(info, 0, 0, 0, 0, -1.0, -1.0, -1.0, -1.0, -1.0);
  int rc = check_set(h, k, d_U, ldu, d_V, ldv);
  if (rc != SMLU_OK) return rc;
  if (k == 0) return smlu_lowrank_clear(h);
  auto t0 = std::chrono::steady_clock::now();
  if ((rc = begin_set(h)) != SMLU_OK) return rc;
  HIPCHK(after_caller(h));
  if ((rc = lr_vectors(h, false)) != SMLU_OK || (rc = lr_columns(h, k)) != SMLU_OK) return rc;
  const int64_t n = h->plan.n, ld = n + (n & 1);
  HIPCHK(launch_lr_stage(h->stream, n, ld, k, d_U, ldu, h->lr_U.p));
  HIPCHK(launch_lr_stage(h->stream, n, ld, k, d_V, ldv, h->lr_V.p));
  return run_set(h, k, info, t0);
}

int smlu_lowrank_set(smlu_handle* h, int32_t k, const double* U, int64_t ldu, const double* V, int64_t ldv,
                     smlu_lowrank_info* info) {
  fill_info(info, 0, 0, 0, 0, -1.0, -1.0, -1.0, -1.0, -1.0);
  int rc = check_set(h, k, U, ldu, V, ldv);
  if (rc != SMLU_OK) return rc;
  if (k == 0) return smlu_lowrank_clear(h);
  auto t0 = std::chrono::steady_clock::now();
  if ((rc = begin_set(h)) != SMLU_OK) return rc;
  if ((rc = lr_vectors(h, false)) != SMLU_OK || (rc = lr_columns(h, k)) != SMLU_OK) return rc;
  const int64_t n = h->plan.n, ld = n + (n & 1);
  // the host columns straight into the even-ld buffers: the pad row is not part of the copy
  HIPCHK(hipMemcpy2DAsync(h->lr_U.p, sizeof(double) * ld, U, sizeof(double) * ldu, sizeof(double) * n, (size_t)k,
                          hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpy2DAsync(h->lr_V.p, sizeof(double) * ld, V, sizeof(double) * ldv, sizeof(double) * n, (size_t)k,
                          hipMemcpyHostToDevice, h->stream));
  return run_set(h, k, info, t0);
}

int smlu_solve_lowrank_device(smlu_handle* h, int op, int max_steps, const double* d_b, double* d_x,
                              smlu_lowrank_info* info) {
  fill_info(info, 0, 0, 0, 0, -1.0, -1.0, -1.0, -1.0, -1.0);
  int rc = check_solve(h, op, max_steps, d_b, d_x);
  if (rc != SMLU_OK) return rc;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(after_caller(h));
  if ((rc = lr_vectors(h, op != SMLU_OP_N)) != SMLU_OK) return rc;
  const int64_t n = h->plan.n;
  // x may be b: the handle keeps its own copy of b
  HIPCHK(hipMemcpyAsync(h->lr_b.p, d_b, sizeof(double) * n, hipMemcpyDeviceToDevice, h->stream));
  if ((rc = run_solve(h, op != SMLU_OP_N, max_steps, info)) != SMLU_OK) return rc;
  HIPCHK(hipMemcpyAsync(d_x, h->lr_x.p, sizeof(double) * n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SMLU_OK;
}

int smlu_solve_lowrank(smlu_handle* h, int op, int max_steps, const double* b, double* x, smlu_lowrank_info* info) {
  fill_info(info, 0, 0, 0, 0, -1.0, -1.0, -1.0, -1.0, -1.0);
  int rc = check_solve(h, op, max_steps, b, x);
  if (rc != SMLU_OK) return rc;
  HIPCHK(hipSetDevice(h->device));
  if ((rc = lr_vectors(h, op != SMLU_OP_N)) != SMLU_OK) return rc;
  const int64_t n = h->plan.n;
  HIPCHK(hipMemcpyAsync(h->lr_b.p, b, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  if ((rc = run_solve(h, op != SMLU_OP_N, max_steps, info)) != SMLU_OK) return rc;
  HIPCHK(hipMemcpyAsync(x, h->lr_x.p, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SMLU_OK;
}
