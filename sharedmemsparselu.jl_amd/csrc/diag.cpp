// diag.cpp — what a factorization says about A besides its solves: log|det A| with its sign or
// phase (umfpack_get_determinant, Julia's logabsdet(F)) and the reciprocal condition estimate
// 1 / (||A|| est||A^-1||) (UMFPACK_RCOND, dgecon / dgscon), both from what the handle already holds
// on the device: no factor export, no n-length copy to the host (kernels_diag.hip).
#include "handle.hpp"

namespace {

int dg_buffers(smlu_handle* h) {
  if (!h->dg_part.p) HIPCHK(h->dg_part.alloc((size_t)kDgMaxBlocks * kDgPartWords));
  if (!h->dg_rec.p) {
    HIPCHK(h->dg_rec.alloc(8));
    HIPCHK(hipMemsetAsync(h->dg_rec.p, 0, 8 * sizeof(long long), h->stream));
  }
  return SMLU_OK;
}

// The 64-byte record of the reduction stamped `seq`, after the work on the handle's stream; like
// read_status, a copy counts only when both stamps match.
int dg_read(smlu_handle* h, long long seq, long long out[8]) {
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int attempt = 0; attempt < 4; ++attempt) {
    HIPCHK(hipMemcpy(out, h->dg_rec.p, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    if (out[0] == seq && out[7] == seq) return SMLU_OK;
    ++h->status_copy_retries;
  }
  return fail(h, SMLU_ERR_HIP, "reduction record read back with a wrong sequence stamp (device-to-host copy)");
}

double as_double(long long w) {
  double v;
  std::memcpy(&v, &w, sizeof v);
  return v;
}

// a one-GPU handle holding a nonsingular factorization
int dg_state(smlu_handle* h, const char* what) {
  if (!h->have_numeric || h->errcol >= 0)
    return fail(h, SMLU_ERR_STATE, std::string(what) + ": no numeric factorization (none yet, or a singular one)");
  if (h->nranks > 1) return fail(h, SMLU_ERR_STATE, std::string(what) + " is single-GPU only (partitioned handle)");
  return SMLU_OK;
}

// log|det| and the sign / phase of the current factorization into the handle's cache.
//   L U = (Rs .* A)[p, q],  p[k] = p0[first[s] + rowperm_s[k - first[s]]]
//   log|det A| = sum log|u_kk| - sum log|Rs_i|
//   sign       = sign(p0) sign(q) prod_s sign(rowperm_s) prod sign(u_kk) prod sign(Rs_i)
// with sign(rowperm_s) = (-1)^(ns - cycles).  ComplexF64 handle (K, pair-preserving pivots): K's
// factors fold into the complex LU of (D Rs .* A)[p, q], D = -i on the rows whose pair was exchanged
// (complex.cpp: export_complex), with the pivots u_k = U[2k, 2k] - i U[2k, 2k+1], so
//   det A = sign(p) sign(q) i^(exchanged pairs) prod u_k / prod Rs_i,   |det A|^2 = |det K|
// where p, q and the front permutations are read as permutations of pairs.
int eval_det(smlu_handle* h) {
  if (h->det_version == h->nfactor) return SMLU_OK;
  const Plan& P = h->plan;
  HIPCHK(hipSetDevice(h->device));
  int rc = dg_buffers(h);
  if (rc != SMLU_OK) return rc;
  hipStream_t st = h->stream;
  if (!h->dg_col2s.p) {
    HIPCHK(h->dg_col2s.upload(P.col2s.data(), P.col2s.size(), st));
    HIPCHK(hipStreamSynchronize(st));
  }
  const long long seq = ++h->dg_seq;
  HIPCHK(launch_dg_logdet(st, h->zc, P.n, h->dg_col2s.p, h->sn.p, h->store.p, h->Rs.p, h->rowperm.p, h->dg_part.p,
                          h->dg_rec.p, seq));
  long long rec[8];
  rc = dg_read(h, seq, rec);
  if (rc != SMLU_OK) return rc;
  ++h->logabsdet_evals;
  const double lu = as_double(rec[1]), lr = as_double(rec[2]), ang = as_double(rec[3]);
  const long long cycles = rec[4], neg_u = rec[5] & 0xffffffffll, swapped = rec[5] >> 32, neg_rs = rec[6];
  if (!h->zc) {
    const long long odd = (P.n - cycles + neg_u + neg_rs + P.perm_parity) & 1;
    h->det_logabs = lu - lr;
    h->det_phase[0] = odd ? -1.0 : 1.0;
    h->det_phase[1] = 0.0;
  } else {
    const long long odd = (P.n / 2 - cycles + neg_rs / 2 + P.pair_parity) & 1;
    const double theta = ang + 1.5707963267948966 * (double)(swapped & 3) + (odd ? 3.141592653589793 : 0.0);
    h->det_logabs = 0.5 * (lu - lr);
    h->det_phase[0] = std::cos(theta);
    h->det_phase[1] = std::sin(theta);
  }
  h->det_version = h->nfactor;
  return SMLU_OK;
}

// ||A||_1 (largest column sum) or ||A||_inf (largest row sum) of the values the handle factored
int eval_anorm(smlu_handle* h, bool inf, double* out) {
  const Plan& P = h->plan;
  hipStream_t st = h->stream;
  if (!inf && !h->Acolp.p) {
    HIPCHK(h->Acolp.upload(P.Acolptr.data(), P.Acolptr.size(), st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (inf && h->zc) {   // a row of K lists both columns of a pair: the entries' columns tell them apart
    int rc = ensure_acol(h);
    if (rc != SMLU_OK) return rc;
  }
  const long long seq = ++h->dg_seq;
  HIPCHK(launch_dg_norm(st, h->zc, inf, h->zc ? h->zn : P.n, inf ? h->Arowptr.p : h->Acolp.p, h->Arow_ent.p,
                        h->Acol.p, h->A.p, h->dg_part.p, h->dg_rec.p, seq));
  long long rec[8];
  int rc = dg_read(h, seq, rec);
  if (rc != SMLU_OK) return rc;
  *out = as_double(rec[1]);
  return SMLU_OK;
}

// Hager / Higham estimate of ||A^-1||_1 (inf: of ||A^-1||_inf = ||A^-H||_1, the two solves change
// roles) as LAPACK's dlacn2 / zlacn2 drive it, the vectors on the device:
//   x = 1/n, y = A^-1 x, est = sum|y|, xi = sign(y), z = A^-H xi, j = argmax|z|;  then up to four times
//   x = e_j, y = A^-1 x, est = max(est, sum|y|); stop on a repeated sign vector (real) or no growth of
//   sum|y|; xi = sign(y), z = A^-H xi, j = argmax|z|; stop when the old j still holds the maximum;
// last the alternating vector x_i = (-1)^i (1 + i/(n-1)): est = max(est, 2 sum|A^-1 x| / (3n)).
// The host reads one 64-byte record after each reduction (sum|y| and the changed-sign count, or j,
// max|z| and |z_jold|).  The solves are the plain factor solves run_solve_dev / run_solve_t_dev, never
// refined: the estimate is a property of the factors.  On a ComplexF64 handle K's transposed pass is A^H.
int eval_ainv(smlu_handle* h, bool inf, double* out) {
  const Plan& P = h->plan;
  const bool z = h->zc;
  const int64_t n = z ? h->zn : P.n;
  hipStream_t st = h->stream;
  if (!h->dg_x.p) {
    HIPCHK(h->dg_x.alloc((size_t)P.n));
    HIPCHK(h->dg_y.alloc((size_t)P.n));
    HIPCHK(h->dg_xi.alloc((size_t)P.n));
  }
  double *x = h->dg_x.p, *y = h->dg_y.p, *xi = h->dg_xi.p;
  long long rec[8];
  h->rcond_solves = h->rcond_solves_fwd = h->rcond_solves_adj = h->rcond_iters = 0;
  auto solve = [&](bool hermitian, const double* b, double* r) {   // hermitian: the A^-H role
    const bool adj = hermitian != inf;
    ++h->rcond_solves;
    ++(adj ? h->rcond_solves_adj : h->rcond_solves_fwd);
    return adj ? run_solve_t_dev(h, 0, b, r) : run_solve_dev(h, b, r, 0);
  };
  auto abs_sum = [&](double* sign, int cmp, double* sum, long long* changed) {
    const long long seq = ++h->dg_seq;
    HIPCHK(launch_dg_sign(st, z, n, y, sign, cmp, h->dg_part.p, h->dg_rec.p, seq));
    int rc = dg_read(h, seq, rec);
    if (rc != SMLU_OK) return rc;
    *sum = as_double(rec[1]);
    *changed = rec[2];
    return (int)SMLU_OK;
  };
  auto arg_max = [&](int64_t jlast, int64_t* j, double* zmax, double* zlast) {   // of z, which lies in x
    const long long seq = ++h->dg_seq;
    HIPCHK(launch_dg_argmax(st, z, n, x, jlast, h->dg_part.p, h->dg_rec.p, seq));
    int rc = dg_read(h, seq, rec);
    if (rc != SMLU_OK) return rc;
    *j = rec[1];
    *zmax = as_double(rec[2]);
    *zlast = as_double(rec[3]);
    return (int)SMLU_OK;
  };
  double est = 0, s = 0, zmax = 0, zlast = 0;
  long long changed = 0;
  int64_t j = 0;
  int rc;
  HIPCHK(launch_dg_vec(st, z, n, 0, 0, x));
  if ((rc = solve(false, x, y)) != SMLU_OK) return rc;
  h->rcond_iters = 1;
  if (n == 1) {
    if ((rc = abs_sum(nullptr, 0, &est, &changed)) != SMLU_OK) return rc;
    *out = est;
    return SMLU_OK;
  }
  if ((rc = abs_sum(xi, 0, &est, &changed)) != SMLU_OK) return rc;
  if ((rc = solve(true, xi, x)) != SMLU_OK) return rc;
  if ((rc = arg_max(-1, &j, &zmax, &zlast)) != SMLU_OK) return rc;
  constexpr int itmax = 5;   // dlacn2's ITMAX, the first pass counted
  for (int iter = 2; iter <= itmax; ++iter) {
    h->rcond_iters = iter;
    HIPCHK(launch_dg_vec(st, z, n, 1, j, x));
    if ((rc = solve(false, x, y)) != SMLU_OK) return rc;
    if ((rc = abs_sum(xi, 1, &s, &changed)) != SMLU_OK) return rc;
    const bool grew = s > est;
    est = std::max(est, s);
    if ((!z && changed == 0) || !grew) break;
    if ((rc = solve(true, xi, x)) != SMLU_OK) return rc;
    const int64_t jlast = j;
    if ((rc = arg_max(jlast, &j, &zmax, &zlast)) != SMLU_OK) return rc;
    if (zlast == zmax) break;
  }
  HIPCHK(launch_dg_vec(st, z, n, 2, 0, x));
  if ((rc = solve(false, x, y)) != SMLU_OK) return rc;
  if ((rc = abs_sum(nullptr, 0, &s, &changed)) != SMLU_OK) return rc;
  *out = std::max(est, 2.0 * s / (3.0 * (double)n));
  return SMLU_OK;
}

}  // namespace

int smlu_logabsdet(smlu_handle* h, double* logabs, double* sign) {
  if (!h || !logabs || !sign) return fail(h, SMLU_ERR_ARG, "NULL argument");
  int rc = dg_state(h, "smlu_logabsdet");
  if (rc != SMLU_OK) return rc;
  if (h->zc) return fail(h, SMLU_ERR_STATE, "complex handle: use smlu_logabsdet_z");
  rc = eval_det(h);
  if (rc != SMLU_OK) return rc;
  *logabs = h->det_logabs;
  *sign = h->det_phase[0];
  return SMLU_OK;
}

int smlu_logabsdet_z(smlu_handle* h, double* logabs, double phase[2]) {
  if (!h || !logabs || !phase) return fail(h, SMLU_ERR_ARG, "NULL argument");
  int rc = dg_state(h, "smlu_logabsdet_z");
  if (rc != SMLU_OK) return rc;
  if (!h->zc) return fail(h, SMLU_ERR_STATE, "real handle: use smlu_logabsdet");
  if (!h->cpair || h->plan.pair_parity < 0)
    return fail(h, SMLU_ERR_STATE, "complex determinant: the row pivots do not keep the complex row pairs "
                                   "(a zero-free-diagonal row transversal was needed)");
  rc = eval_det(h);
  if (rc != SMLU_OK) return rc;
  *logabs = h->det_logabs;
  phase[0] = h->det_phase[0];
  phase[1] = h->det_phase[1];
  return SMLU_OK;
}

int smlu_rcond(smlu_handle* h, int norm, double* rcond, double* anorm, double* ainvnorm) {
  if (!h || !rcond) return fail(h, SMLU_ERR_ARG, "NULL argument");
  if (norm != SMLU_NORM_ONE && norm != SMLU_NORM_INF)
    return fail(h, SMLU_ERR_ARG, "norm must be SMLU_NORM_ONE or SMLU_NORM_INF");
  int rc = dg_state(h, "smlu_rcond");
  if (rc != SMLU_OK) return rc;
  const int k = norm == SMLU_NORM_INF ? 1 : 0;
  if (h->rc_version[k] == h->nfactor) {
    h->rcond_solves = h->rcond_solves_fwd = h->rcond_solves_adj = 0;   // a cached answer: no GPU work
  } else {
    HIPCHK(hipSetDevice(h->device));
    rc = dg_buffers(h);
    if (rc != SMLU_OK) return rc;
    double an = 0, ai = 0;
    rc = eval_anorm(h, k == 1, &an);
    if (rc != SMLU_OK) return rc;
    rc = eval_ainv(h, k == 1, &ai);
    if (rc != SMLU_OK) return rc;
    h->rc_anorm[k] = an;
    h->rc_ainv[k] = ai;
    h->rc_version[k] = h->nfactor;
  }
  const double an = h->rc_anorm[k], ai = h->rc_ainv[k];
  *rcond = (an == 0.0 || ai == 0.0) ? 0.0 : 1.0 / (an * ai);
  if (anorm) *anorm = an;
  if (ainvnorm) *ainvnorm = ai;
  return SMLU_OK;
}
