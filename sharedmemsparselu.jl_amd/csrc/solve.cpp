// solve.cpp — ldiv! / lsolve! / rsolve! (src/SharedMemSparseLU.jl:286-392) on the GPU: the level
// schedule of solve launches, iterative refinement, batched right-hand sides and the chunked layout.
#include "handle.hpp"

// One solve launch for rh.n right-hand sides (x columns at w + r*rh.ldx, front vectors at
// v + r*rh.ldv); the multi-GPU kinds (K_BWDU12C, K_VCOPY) are single-vector only.
static hipError_t run_solve_launch(smlu_handle* h, const Launch& L, double* w, double* v, Rhs rh, hipStream_t st) {
  switch (L.kind) {
    case K_FWD:
      return launch_fwd(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->chlist.p, h->relmap.p,
                        h->rowperm.p, h->store.p, w, v, rh);
    case K_BWD:
      return launch_bwd(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->rows.p, h->store.p, w, v, rh);
    case K_FWDT:
      return launch_fwd_tiny(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->chlist.p, h->relmap.p, h->rowperm.p,
                             h->store.p, w, v, rh, (int)L.aux);
    case K_BWDT:
      return launch_bwd_tiny(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->rows.p, h->store.p, w, v, rh, (int)L.aux);
    case K_FWDP:
      return launch_fwd_pull(st, L.nwg, h->ftiles.p + L.off, (int)L.cnt, h->sn.p, h->rowperm.p, h->gptr.p, h->gent.p,
                             w, v, rh);
    case K_FWDG:
      return launch_fwd_gather(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->chlist.p, h->relmap.p,
                               h->rowperm.p, w, v, rh);
    case K_TRIF:
      return launch_tri_block(st, false, L.nwg, h->ftiles.p + L.off, (int)L.cnt, L.step, h->sn.p,
                              h->store.p, w, v, rh);
    case K_TRIB:
      return launch_tri_block(st, true, L.nwg, h->ftiles.p + L.off, (int)L.cnt, L.step, h->sn.p,
                              h->store.p, w, v, rh);
    case K_BWDU:
      return launch_bwd_u12(st, L.nwg, h->ftiles.p + L.off, (int)L.cnt, h->sn.p, h->rows.p, h->store.p, w, v,
                            rh);
    case K_SWEEPF:
    case K_SWEEPB:
      return launch_tri_sweep(st, L.kind == K_SWEEPB, L.nwg, h->ftiles.p + L.off, (int)L.cnt, h->stick.p + L.aux2,
                              h->ssync.p + L.aux, h->sxh.p + L.aux * 64 * kMultiRhs, h->sstatus.p, h->sn.p, h->store.p,
                              w, v, rh, h->sweep_spin);
    case K_BWDU12C:
      return launch_bwd_u12_cols(st, h->sn.p, L.node, h->sch.hsn[L.node].ns, L.aux, L.aux2, (int)L.cnt, h->rows.p,
                                 h->store.p, w, h->vbuf.p);
    case K_VCOPY:
      return launch_vcopy(st, h->sn.p, L.node, h->sch.hsn[L.node].ns, w, h->vbuf.p);
  }
  return hipErrorInvalidValue;
}

// The launches [lo, hi) of a sequence in order, launch(L, stream) for each.  overlap: a level's side
// launches (grp > 0, side) go on the side stream, forked after everything before the level and
// joined before the next level -- and on the error path, so a failed launch never leaves the side
// stream unjoined (inside a capture that would invalidate it).
template <class F>
static hipError_t walk_launches(smlu_handle* h, const std::vector<Launch>& seq, size_t lo, size_t hi, bool overlap,
                                F&& launch) {
  hipStream_t st = h->stream;
  bool forked = false;
  hipError_t e = hipSuccess;
  for (size_t i = lo; i < hi && e == hipSuccess; ++i) {
    const Launch& L = seq[i];
    const bool first = overlap && L.grp > 0 && (i == lo || seq[i - 1].grp != L.grp);
    const bool last = overlap && L.grp > 0 && (i + 1 == hi || seq[i + 1].grp != L.grp);
    if (first) {
      e = hipEventRecord(h->fork_ev, st);
      if (e == hipSuccess) e = hipStreamWaitEvent(h->side, h->fork_ev, 0);
      forked = e == hipSuccess;
    }
    if (e == hipSuccess) e = launch(L, L.side && forked ? h->side : st);
    if (e == hipSuccess && last && forked) {
      e = hipEventRecord(h->join_ev, h->side);
      if (e == hipSuccess) e = hipStreamWaitEvent(st, h->join_ev, 0);
      if (e == hipSuccess) forked = false;
    }
  }
  if (forked) {
    (void)hipEventRecord(h->join_ev, h->side);
    (void)hipStreamWaitEvent(st, h->join_ev, 0);
  }
  return e;
}

// body()'s launches on the handle's stream (fixed pointers: the handle's work buffers), captured once
// per key into a hipGraph (h->sol_execs) and replayed.  A capture or instantiation that fails sets
// graph_failed, and body() then runs eagerly, as it does when use_graph is false.
template <class F>
static int run_graphed(smlu_handle* h, bool use_graph, int key, F&& body) {
  hipStream_t st = h->stream;
  hipGraphExec_t ex = nullptr;
  if (use_graph && !h->graph_failed) {
    for (auto& g : h->sol_execs)
      if (g.first == key) ex = g.second;
    if (!ex) {
      hipGraph_t g = nullptr;
      HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
      int rc = body();
      hipError_t ec = hipStreamEndCapture(st, &g);
      if (rc == SMLU_OK && ec == hipSuccess && g) ec = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
      if (g) (void)hipGraphDestroy(g);
      if (rc != SMLU_OK || ec != hipSuccess || !ex) {
        (void)hipGetLastError();
        h->graph_failed = true;
        ex = nullptr;
      } else {
        h->sol_execs.push_back({key, ex});
      }
    }
  }
  if (!ex) return body();
  HIPCHK(hipGraphLaunch(ex, st));
  return SMLU_OK;
}

// What the two plain passes open and close alike: the host clock behind solve_ms, the profile
// timer, and the work buffers of the width -- wrk / vbuf for one column, wrkm / vbufm (allocated on
// first use) for a batch.
struct Pass {
  smlu_handle* h;
  Timer tm;
  hipEvent_t stop = nullptr;
  std::chrono::steady_clock::time_point t0;
  double* w = nullptr;
  double* v = nullptr;
  Rhs rh{};
  explicit Pass(smlu_handle* hh) : h(hh), tm(hh) {}
  int open(int nrhs) {
    t0 = std::chrono::steady_clock::now();
    HIPCHK(tm.begin(K_FWD, &stop, h->stream));
    w = h->wrk.p;
    v = h->vbuf.p;
    rh = Rhs{1, (int64_t)h->plan.n, (int64_t)h->vbuf.n};
    if (nrhs > 1) {
      if (!h->vbufm.p) HIPCHK(h->vbufm.alloc(h->vbuf.n * kMultiRhs));
      if (!h->wrkm.p) HIPCHK(h->wrkm.alloc((size_t)h->plan.n * kMultiRhs));
      w = h->wrkm.p;
      v = h->vbufm.p;
      rh.n = nrhs;
    }
    return SMLU_OK;
  }
  int close() {   // the pass is complete on return
    HIPCHK(tm.end(stop));
    HIPCHK(hipStreamSynchronize(h->stream));
    tm.collect();
    return SMLU_OK;
  }
  void stamp() { h->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

int run_solve_dev(smlu_handle* h, const double* db, double* dx, int mode, int nrhs, int64_t ldb, int64_t ldx) {
  // mode 0: ldiv (b -> x); 1: lsolve in place on dx (final order); 2: rsolve in place.
  // nrhs > 1 (mode 0, one GPU): columns of db / dx with leading dimensions ldb / ldx.
  Plan& P = h->plan;
  if (h->nranks > 1 && mode != 0) return fail(h, SMLU_ERR_STATE, "lsolve!/rsolve! are single-GPU only");
  if (nrhs > 1 && (mode != 0 || h->nranks > 1 || nrhs > kMultiRhs))
    return fail(h, SMLU_ERR_STATE, "batched right-hand sides: ldiv on one GPU only");
  hipStream_t st = h->stream;
  Pass ps(h);
  if (int rc = ps.open(nrhs); rc != SMLU_OK) return rc;
  double* const w = ps.w;
  double* const v = ps.v;
  const Rhs rh = ps.rh;
  // batches of up to 8 run the sweeps too (round 6: the NR substitution chains interleaved,
  // tri64_rows, NR-wide hand-off slots); wider ones the per-block schedule (fwdm / bwdm)
  const bool wide = rh.n > 8 && h->nranks == 1;
  // The sync-free sweeps' waits are bounded: a wait that gives up raises sstatus, which is read back
  // after every solve that ran them; the solve is then re-run on the per-block schedule (fwdm / bwdm,
  // bitwise the same arithmetic), so a timed-out sweep never returns a wrong x.  Partitioned handles
  // agree on the re-run (allreduce of the flag: the per-block sequences hold the same comm steps).
  const bool check = !wide && (h->sch.ssync_n > 0 || h->nranks > 1);
  const double* src = mode == 0 ? db : dx;
  const int64_t lds = mode == 0 && ldb > 0 ? ldb : P.n;
  auto load_input = [&](const double* in, int64_t ld) -> hipError_t {
    if (mode == 0) return launch_perm_in(st, P.n, h->p0.p, h->Rs.p, in, w, nrhs, ld, rh.ldx);
    if (mode == 1) return launch_unswap(st, P.n, h->posfirst.p, h->rowperm.p, in, w);
    return hipMemcpyAsync(w, in, sizeof(double) * P.n, hipMemcpyDeviceToDevice, st);
  };
  const double* rerun_src = src;
  int64_t rerun_ld = lds;
  if (check && (mode != 0 || db == dx)) {   // the final step overwrites the input: keep a copy for a re-run
    if (!h->bstash.p) HIPCHK(h->bstash.alloc((size_t)P.n * kMultiRhs));
    HIPCHK(hipMemcpy2DAsync(h->bstash.p, sizeof(double) * P.n, src, sizeof(double) * lds, sizeof(double) * P.n,
                            (size_t)nrhs, hipMemcpyDeviceToDevice, st));
    rerun_src = h->bstash.p;
    rerun_ld = P.n;
  }
  HIPCHK(load_input(src, lds));
  // launches between communication steps (one GPU: a single segment each)
  // overlap: a level's small fronts on the side stream next to its large fronts' per-block chain
  // (batched right-hand sides: 8 per 128^3 solve 59.5 -> 57.4 ms).  Not next to the sync-free
  // sweeps, whose waiting workgroups lose CUs to them (1 rhs: 13.8 -> 15.2 ms, round 6).
  auto launch = [&](const Launch& L, hipStream_t s) { return run_solve_launch(h, L, w, v, rh, s); };
  auto run_seq = [&](const std::vector<Launch>& seq, const std::vector<size_t>& seg, const std::vector<int>& cm,
                     bool overlap) {
    for (size_t k = 0; k < seg.size(); ++k) {
      if (k > 0) {
        int rc = exec_comm(h, cm[k - 1]);
        if (rc != SMLU_OK) return rc;
      }
      const size_t hi = k + 1 < seg.size() ? seg[k + 1] : seq.size();
      HIPCHK(walk_launches(h, seq, seg[k], hi, overlap, launch));
    }
    return (int)SMLU_OK;
  };
  auto sweeps = [&](bool per_block) {   // per_block: the per-block sequences instead of the sweeps
    if (mode != 2) {
      int rc = per_block ? run_seq(h->sch.fwdm, h->sch.fwdm_seg, h->sch.fwd_comm, true) : run_seq(h->sch.fwd, h->sch.fwd_seg, h->sch.fwd_comm, false);
      if (rc != SMLU_OK) return rc;
    }
    if (mode != 1) {
      int rc = per_block ? run_seq(h->sch.bwdm, h->sch.bwdm_seg, h->sch.bwd_comm, true) : run_seq(h->sch.bwd, h->sch.bwd_seg, h->sch.bwd_comm, false);
      if (rc != SMLU_OK) return rc;
    }
    return (int)SMLU_OK;
  };
  auto finish = [&]() -> hipError_t {
    if (mode == 0) return launch_perm_out(st, P.n, h->q.p, w, dx, nrhs, rh.ldx, ldx > 0 ? ldx : P.n);
    return hipMemcpyAsync(dx, w, sizeof(double) * P.n, hipMemcpyDeviceToDevice, st);
  };
  // One GPU: the forward and backward sweeps (~1,400 launches at 128^3, fixed pointers: the
  // handle's wrk / vbuf) are captured once per (mode, rhs count) into a hipGraph and replayed;
  // only the permutation kernels see the caller's b and x.
  int rc = run_graphed(h, h->nranks == 1 && !tune().no_graph, mode * 256 + rh.n, [&] { return sweeps(wide); });
  if (rc != SMLU_OK) return rc;
  if (mode == 0) ++h->solve_passes;   // a sweep-timeout re-run below is the same pass
  HIPCHK(finish());
  rc = ps.close();
  if (rc != SMLU_OK) return rc;
  if (check) {
    long long rec[16];
    int rs = read_status(h, nullptr, 0, h->sstatus.p, 1, rec);
    if (rs != SMLU_OK) return rs;
    double bad = (rec[6] & 0xffffffffll) != 0 ? 1.0 : 0.0;
    if (h->nranks > 1 && h->tr.allreduce_max(h->tr.ctx, &bad, 1) != 0)
      return fail(h, SMLU_ERR_HIP, "transport allreduce failed (sweep status)");
    if (bad != 0) {
      ++h->sweep_timeouts;
      HIPCHK(hipMemsetAsync(h->sstatus.p, 0, sizeof(int32_t), st));
      HIPCHK(load_input(rerun_src, rerun_ld));
      rc = sweeps(true);
      if (rc != SMLU_OK) return rc;
      HIPCHK(finish());
      HIPCHK(hipStreamSynchronize(st));
    }
  }
  ps.stamp();
  return SMLU_OK;
}

// ldiv! plus iterative refinement on the original (unscaled) A: x <- x + A \ (b - A x).  The
// diagonal-tile pivoting of large fronts cannot always keep growth below 1/pivot_tol; when a
// refactor flags such weak pivots (h->weak), refine = -1 applies up to 3 steps (the pivot-
// failure fallback).  So it does for non-dominant values factored under a diagonal
// tolerance below the pivot tolerance (UMFPACK's symmetric default 0.001 < 0.1): a diagonal kept
// at 0.001 of its column lets the factors grow up to 1000x per step, and UMFPACK's own solve
// refines by default (IRSTEP 2) for the same reason.  Stopping rule of LAPACK's dgerfs with a
// rounding floor: a correction is solved only while the componentwise backward error
// max |r|/(|A||x|+|b|) exceeds 4 unit roundoffs (2^-51; dgerfs uses 1, which a residual summed in
// fp64 rarely reaches, so it spends two extra solves to gain nothing) and at most halves the
// previous one -- an accurate solve costs one residual and no extra solve.
// Residual buffers and the column of every A entry (allocated on first use).
int ensure_residual(smlu_handle* h) {
  Plan& P = h->plan;
  const int64_t n = P.n;
  if (!h->ref_b.p) {
    HIPCHK(h->ref_b.alloc((size_t)n));
    HIPCHK(h->ref_r.alloc((size_t)n));
    HIPCHK(h->ref_d.alloc((size_t)n));
    HIPCHK(h->ref_nrm.alloc(2));
  }
  return ensure_acol(h);
}

// The column of every A entry (residuals, dominance check, row sums of a complex handle).
int ensure_acol(smlu_handle* h) {
  Plan& P = h->plan;
  if (!h->Acol.p) {
    std::vector<int32_t> ac((size_t)std::max<int64_t>(P.nnzA, 1));
    for (int64_t c = 0; c < P.n; ++c)
      for (int64_t e = P.Acolptr[c]; e < P.Acolptr[c + 1]; ++e) ac[e] = (int32_t)c;
    HIPCHK(h->Acol.upload(ac.data(), ac.size(), h->stream));
  }
  return SMLU_OK;
}

static int auto_refine_steps(const smlu_handle* h) {
  if (h->opts.refine >= 0) return h->opts.refine;
  const bool diag_pref = !h->plan.given_order && !h->dominant && h->opts.diag_pivot_tol < h->opts.pivot_tol;
  return (h->weak > 0 || diag_pref) ? 3 : 0;
}

// The refined solve of either direction: solve(b, x) is one plain solve on device vectors,
// residual(x, b, r, nrm) launches r = b - op(A) x with its two norms (k_residual's rule).
template <class SOLVE, class RESID>
static int solve_refined_by(smlu_handle* h, const double* db, double* dx, SOLVE&& solve, RESID&& residual) {
  const int steps = auto_refine_steps(h);
  h->refine_steps = 0;
  h->refine_resid = -1;
  h->refine_berr = -1;
  if (steps == 0) return solve(db, dx);
  const int64_t n = h->plan.n;
  hipStream_t st = h->stream;
  int rc = ensure_residual(h);
  if (rc != SMLU_OK) return rc;
  HIPCHK(hipMemcpyAsync(h->ref_b.p, db, sizeof(double) * n, hipMemcpyDeviceToDevice, st));   // db may alias dx
  rc = solve(h->ref_b.p, dx);
  if (rc != SMLU_OK) return rc;
  const double ms = h->solve_ms;
  const double eps = std::ldexp(1.0, -51);   // 4 unit roundoffs
  double prev = HUGE_VAL;
  for (int it = 0; it < steps; ++it) {
    HIPCHK(hipMemsetAsync(h->ref_nrm.p, 0, 2 * sizeof(double), st));
    HIPCHK(residual(dx, h->ref_b.p, h->ref_r.p, h->ref_nrm.p));
    long long rec[16];
    rc = read_status(h, nullptr, 0, reinterpret_cast<const int32_t*>(h->ref_nrm.p), 4, rec);
    if (rc != SMLU_OK) return rc;
    double nrm, berr;
    std::memcpy(&nrm, &rec[6], sizeof nrm);
    std::memcpy(&berr, &rec[7], sizeof berr);
    h->refine_resid = nrm;
    h->refine_berr = berr;
    if (berr <= eps || berr > 0.5 * prev) break;
    prev = berr;
    rc = solve(h->ref_r.p, h->ref_d.p);
    if (rc != SMLU_OK) return rc;
    HIPCHK(launch_axpy1(st, n, h->ref_d.p, dx));
    ++h->refine_steps;
  }
  HIPCHK(hipStreamSynchronize(st));
  h->solve_ms = ms;   // the plain solve's time (refinement steps reported separately)
  return SMLU_OK;
}

int smlu_residual_device(smlu_handle* h, const double* d_x, const double* d_b, double* d_r, double* nrm) {
  if (!h || !d_x || !d_b || !d_r) return fail(h, SMLU_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(after_caller(h));
  int rc = ensure_residual(h);
  if (rc != SMLU_OK) return rc;
  hipStream_t st = h->stream;
  HIPCHK(hipMemsetAsync(h->ref_nrm.p, 0, 2 * sizeof(double), st));
  HIPCHK(launch_residual(st, h->plan.n, h->Arowptr.p, h->Arow_ent.p, h->Acol.p, h->A.p, d_x, d_b, d_r,
                         h->ref_nrm.p));
  long long rec[16];
  rc = read_status(h, nullptr, 0, reinterpret_cast<const int32_t*>(h->ref_nrm.p), 2, rec);
  if (rc != SMLU_OK) return rc;
  double v;
  std::memcpy(&v, &rec[6], sizeof v);
  if (nrm) *nrm = v;
  return SMLU_OK;
}

// ---- transposed / adjoint solves: A^T x = b, A^H x = b from the factors of A -------------------
// (Rs .* A)[p0, q] = P_fronts^T L U, so A^T x = b is w = b[q]; U^T y = w, leaves -> root; the L^T and
// front-permutation pass root -> leaves; x[p0] = Rs[p0] .* z (kernels_solve_t.hip).  The two passes
// walk the per-block sequences fwdm / bwdm, which every one-GPU handle has, and reinterpret each
// launch by kind on the same work lists and workgroup counts; the schedule itself is untouched.
// A ComplexF64 handle's K^T is the real equivalent of A^H: the same passes give the adjoint solve,
// and the plain transpose is conj(A^H \ conj(b)), the conjugations folded into the permutations.
static hipError_t run_solve_launch_t(smlu_handle* h, const Launch& L, double* w, double* v, Rhs rh, hipStream_t st) {
  switch (L.kind) {
    case K_FWDT:
      return launch_ut_tiny(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->chlist.p, h->relmap.p, h->store.p, w, v,
                            rh, (int)L.aux);
    case K_FWD:
      return launch_ut_front(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->chlist.p, h->relmap.p, h->store.p, w, v,
                             rh);
    case K_FWDP:
      return launch_pull_t(st, L.nwg, h->ftiles.p + L.off, (int)L.cnt, h->sn.p, h->gptr.p, h->gent.p, w, v, rh);
    case K_TRIF:
      return launch_tri_t(st, false, L.nwg, h->ftiles.p + L.off, (int)L.cnt, L.step, h->sn.p, h->rowperm.p,
                          h->store.p, w, v, rh);
    case K_BWDT:
      return launch_lt_tiny(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->rows.p, h->rowperm.p, h->store.p, w,
                            rh, (int)L.aux);
    case K_BWD:
      return launch_lt_front(st, (int)L.cnt, h->ilist.p + L.off, h->sn.p, h->rows.p, h->rowperm.p, h->store.p, w, v,
                             rh);
    case K_BWDU:
      return launch_bwdu_t(st, L.nwg, h->ftiles.p + L.off, (int)L.cnt, h->sn.p, h->rows.p, h->store.p, w, v, rh);
    case K_TRIB:
      return launch_tri_t(st, true, L.nwg, h->ftiles.p + L.off, (int)L.cnt, L.step, h->sn.p, h->rowperm.p,
                          h->store.p, w, v, rh);
  }
  return hipErrorInvalidValue;   // no transposed meaning (the sequences of a one-GPU handle hold none)
}

// sol_execs keys of the transposed passes: kTransGraphKey + columns in the batch (forward: mode * 256 + rhs)
constexpr int kTransGraphKey = 1 << 12;

// One pass pair for nrhs <= kMultiRhs columns of db / dx (leading dimensions ldb / ldx; one column:
// unused).  A batch runs in wrkm / vbufm, the forward batch's buffers (calls on one handle are
// serialised); db may alias dx when ldb == ldx: the whole batch is permuted into the work buffer
// before any x is written.
int run_solve_t_dev(smlu_handle* h, int conj, const double* db, double* dx, int nrhs, int64_t ldb, int64_t ldx) {
  Plan& P = h->plan;
  if (nrhs < 1 || nrhs > kMultiRhs) return fail(h, SMLU_ERR_STATE, "transposed batch: 1 to 16 right-hand sides");
  hipStream_t st = h->stream;
  Pass ps(h);
  int rc = ps.open(nrhs);
  if (rc != SMLU_OK) return rc;
  double* const w = ps.w;
  double* const v = ps.v;
  const Rhs rh = ps.rh;
  HIPCHK(launch_perm_in_t(st, P.n, h->q.p, db, ldb, w, conj, rh));
  auto launch = [&](const Launch& L, hipStream_t s) { return run_solve_launch_t(h, L, w, v, rh, s); };
  auto passes = [&]() {   // the whole of fwdm, then of bwdm, with the side-stream overlap
    hipError_t e = walk_launches(h, h->sch.fwdm, 0, h->sch.fwdm.size(), true, launch);
    if (e == hipSuccess) e = walk_launches(h, h->sch.bwdm, 0, h->sch.bwdm.size(), true, launch);
    if (e != hipSuccess) return fail(h, SMLU_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(e) + " in the transposed solve");
    return (int)SMLU_OK;
  };
  // the two passes (fixed pointers: the handle's wrk / vbuf, or wrkm / vbufm), one graph per batch width
  rc = run_graphed(h, !tune().no_graph, kTransGraphKey + rh.n, passes);
  if (rc != SMLU_OK) return rc;
  ++h->trans_passes;
  HIPCHK(launch_perm_out_t(st, P.n, h->p0.p, h->Rs.p, w, dx, ldx, conj, rh));
  rc = ps.close();
  if (rc != SMLU_OK) return rc;
  ps.stamp();
  return SMLU_OK;
}

// ---- the front end of the smlu_solve* entry points ---------------------------------------------
// The operation of a call, filled by check_solve.
struct SolveOp {
  bool trans = false;   // A^T x = b or A^H x = b: the transposed passes and residual
  int conj = 0;         // ... conjugated in and out (the plain transpose of a ComplexF64 handle)
};

// Argument and state checks of the ten smlu_solve* entry points.  refined: the batched-refinement
// pair, which takes max_steps and, as smlu_logabsdet, refuses the handle of a singular factorization.
static int check_solve(smlu_handle* h, int op, bool refined, int max_steps, int64_t nrhs, const double* B, int64_t ldb,
                       const double* X, int64_t ldx, SolveOp* o) {
  if (!h || nrhs < 0 || (nrhs > 0 && (!B || !X))) return fail(h, SMLU_ERR_ARG, "NULL argument or nrhs < 0");
  if (op != SMLU_OP_N && op != SMLU_OP_T && op != SMLU_OP_H)
    return fail(h, SMLU_ERR_ARG, "op must be SMLU_OP_N, SMLU_OP_T or SMLU_OP_H");
  if (max_steps < -1) return fail(h, SMLU_ERR_ARG, "max_steps must be -1 (the handle's rule), 0 or a step limit");
  if (!h->have_numeric || (refined && h->errcol >= 0))
    return fail(h, SMLU_ERR_STATE, "no numeric factorization (none yet, or a singular one)");
  if (h->nranks > 1 && (op != SMLU_OP_N || refined))
    return fail(h, SMLU_ERR_STATE, "transposed solves and batched refinement are single-GPU only");
  if (ldb < h->plan.n || ldx < h->plan.n) return fail(h, SMLU_ERR_ARG, "leading dimension smaller than n");
  o->trans = op != SMLU_OP_N;
  o->conj = h->zc && op == SMLU_OP_T;
  return SMLU_OK;
}

// One plain pass over w <= kMultiRhs columns (one column: the leading dimensions are unused).
static int plain_pass(smlu_handle* h, const SolveOp& o, const double* b, double* x, int w, int64_t ldb, int64_t ldx) {
  return o.trans ? run_solve_t_dev(h, o.conj, b, x, w, ldb, ldx) : run_solve_dev(h, b, x, 0, w, ldb, ldx);
}

// One refined column.  Transposed: solve_refined_by's rule with r = b - A^T x by columns of A's CSC,
// componentwise denominator |A^T||x| + |b|, same stop test and the same refine_* stats.
static int refined_column(smlu_handle* h, const SolveOp& o, const double* db, double* dx) {
  Plan& P = h->plan;
  if (o.trans && auto_refine_steps(h) != 0 && !h->Acolp.p)
    HIPCHK(h->Acolp.upload(P.Acolptr.data(), P.Acolptr.size(), h->stream));
  return solve_refined_by(
      h, db, dx, [&](const double* b, double* x) { return plain_pass(h, o, b, x, 1, 0, 0); },
      [&](const double* x, const double* b, double* r, double* nrm) {
        return o.trans ? launch_residual_t(h->stream, P.n, h->Acolp.p, h->Arow.p, h->A.p, x, b, r, nrm, o.conj)
                       : launch_residual(h->stream, P.n, h->Arowptr.p, h->Arow_ent.p, h->Acol.p, h->A.p, x, b, r, nrm);
      });
}

// The columns of a call: device pointers, or host memory staged through the handle.
struct Cols {
  const double* B;
  int64_t ldb;
  double* X;
  int64_t ldx;
  bool host;
};

// body(b, ldb, x, ldx, j, nb) on device pointers for every chunk [j, j + nb) of up to width columns.
// Host columns are copied into the handle's staging buffer (wrk2 at width 1, else wrk2m, allocated on
// first use), solved there in place and copied back, with one synchronisation after the last chunk;
// a single column moves by a plain copy.
template <class F>
static int over_chunks(smlu_handle* h, const Cols& c, int64_t nrhs, int width, F&& body) {
  const int64_t n = h->plan.n;
  hipStream_t st = h->stream;
  if (c.host && width > 1 && !h->wrk2m.p) HIPCHK(h->wrk2m.alloc((size_t)n * kMultiRhs));
  double* d = width > 1 ? h->wrk2m.p : h->wrk2.p;
  auto copy = [&](double* dst, int64_t ldd, const double* src, int64_t lds, int nb, hipMemcpyKind kind) {
    if (nb == 1) return hipMemcpyAsync(dst, src, sizeof(double) * n, kind, st);
    return hipMemcpy2DAsync(dst, sizeof(double) * ldd, src, sizeof(double) * lds, sizeof(double) * n, (size_t)nb, kind, st);
  };
  for (int64_t j = 0; j < nrhs; j += width) {
    const int nb = (int)std::min<int64_t>(width, nrhs - j);
    const double* Bj = c.B + j * c.ldb;
    double* Xj = c.X + j * c.ldx;
    if (c.host) HIPCHK(copy(d, n, Bj, c.ldb, nb, hipMemcpyHostToDevice));
    int rc = c.host ? body(d, n, d, n, j, nb) : body(Bj, c.ldb, Xj, c.ldx, j, nb);
    if (rc != SMLU_OK) return rc;
    if (c.host) HIPCHK(copy(Xj, c.ldx, d, n, nb, hipMemcpyDeviceToHost));
  }
  if (c.host) HIPCHK(hipStreamSynchronize(st));
  return SMLU_OK;
}

// The driver of the plain entry points.  One GPU without refinement: batches of up to kMultiRhs
// columns go through the solve kernels together (each factor value read once per batch, not per
// column; every column bitwise its single-vector solve); otherwise (refinement, several GPUs, one
// column) one refined solve per column.  B may alias X when ldb == ldx (a batch is permuted into the
// work buffer before any x is written).  solve_ms: the sum over what the call ran.
static int solve_cols(smlu_handle* h, const SolveOp& o, const Cols& c, int64_t nrhs) {
  const bool batched = auto_refine_steps(h) == 0 && h->nranks == 1 && nrhs > 1;
  if (batched) {
    h->refine_steps = 0;
    h->refine_resid = -1;
    h->refine_berr = -1;
  }
  double ms = 0;
  int rc = over_chunks(h, c, nrhs, batched ? kMultiRhs : 1,
                       [&](const double* b, int64_t ldb, double* x, int64_t ldx, int64_t, int nb) {
                         int r = batched ? plain_pass(h, o, b, x, nb, ldb, ldx) : refined_column(h, o, b, x);
                         ms += h->solve_ms;
                         return r;
                       });
  if (rc == SMLU_OK) h->solve_ms = ms;
  return rc;
}

// ---- batched iterative refinement: smlu_solve_refined_multi*  ----------------------
// solve_refined_by for up to kMultiRhs columns at once: one batched solve, then per round one
// batched residual over the columns still active, one host read of their norms, the stopping rule
// per column on the host, and one batched solve of the survivors' residuals at their own width.
// Every column sees the operations of its single refined solve: the batch kernels give each column
// its single-vector bits at any width, k_residual_batch the single residual's, and a column that
// has stopped is not touched again.
static int ensure_refine_batch(smlu_handle* h, bool trans) {
  Plan& P = h->plan;
  if (!h->refm_rec.p) {
    const size_t nm = (size_t)P.n * kMultiRhs;
    hipError_t e = h->refm_b.alloc(nm);
    if (e == hipSuccess) e = h->refm_r.alloc(nm);
    if (e == hipSuccess) e = h->refm_d.alloc(nm);
    if (e == hipSuccess) e = h->refm_nrm.alloc(2 * kMultiRhs);
    if (e == hipSuccess) e = h->refm_rec.alloc(2 * kMultiRhs + 2);
    if (e == hipSuccess) e = hipMemsetAsync(h->refm_rec.p, 0, (2 * kMultiRhs + 2) * sizeof(long long), h->stream);
    if (e != hipSuccess) {
      h->refm_b.free();
      h->refm_r.free();
      h->refm_d.free();
      h->refm_nrm.free();
      h->refm_rec.free();
      (void)hipGetLastError();
      if (e == hipErrorOutOfMemory)
        return fail(h, SMLU_ERR_ALLOC, "batched refinement: no device memory for its three n x 16 work buffers (" +
                                           std::to_string(3.0 * 8.0 * nm / 1e9) + " GB)");
      HIPCHK(e);
    }
  }
  if (trans && !h->Acolp.p) HIPCHK(h->Acolp.upload(P.Acolptr.data(), P.Acolptr.size(), h->stream));
  return ensure_acol(h);
}

// The norm words of the round stamped seq (dg_read's rule: both stamps must match).
static int read_refine_record(smlu_handle* h, long long seq, long long out[2 * kMultiRhs + 2]) {
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int attempt = 0; attempt < 4; ++attempt) {
    HIPCHK(hipMemcpy(out, h->refm_rec.p, (2 * kMultiRhs + 2) * sizeof(long long), hipMemcpyDeviceToHost));
    if (out[0] == seq && out[2 * kMultiRhs + 1] == seq) return SMLU_OK;
    ++h->status_copy_retries;
  }
  return fail(h, SMLU_ERR_HIP, "refinement record read back with a wrong sequence stamp (device-to-host copy)");
}

// One batch of nb <= kMultiRhs columns.  solve(b, ldb, x, ldx, width) is one plain batched solve,
// residual(x, ldx, b, r, nrm, nact, list) one batched residual launch (b: the stash, leading
// dimension n).  info: nb entries.  *ms: the plain solve's time.
template <class SOLVE, class RESID>
static int refine_batch(smlu_handle* h, int steps, int nb, const double* dB, int64_t ldb, double* dX, int64_t ldx,
                        smlu_refine_info* info, double* ms, SOLVE&& solve, RESID&& residual) {
  const int64_t n = h->plan.n;
  hipStream_t st = h->stream;
  for (int j = 0; j < nb; ++j) info[j] = smlu_refine_info{0, 0, -1.0, -1.0};
  if (steps == 0) {
    int rc = solve(dB, ldb, dX, ldx, nb);
    *ms = h->solve_ms;
    return rc;
  }
  HIPCHK(hipMemcpy2DAsync(h->refm_b.p, sizeof(double) * n, dB, sizeof(double) * ldb, sizeof(double) * n, (size_t)nb,
                          hipMemcpyDeviceToDevice, st));   // dB may alias dX
  int rc = solve(h->refm_b.p, n, dX, ldx, nb);
  if (rc != SMLU_OK) return rc;
  *ms = h->solve_ms;
  const double eps = std::ldexp(1.0, -51);   // 4 unit roundoffs (solve_refined_by)
  int32_t act[kMultiRhs];
  double prev[kMultiRhs];
  int nact = nb;
  for (int j = 0; j < nb; ++j) {
    act[j] = j;
    prev[j] = HUGE_VAL;
  }
  for (int it = 0; it < steps && nact > 0; ++it) {
    HIPCHK(hipMemsetAsync(h->refm_nrm.p, 0, 2 * kMultiRhs * sizeof(double), st));
    HIPCHK(residual(dX, ldx, h->refm_b.p, h->refm_r.p, h->refm_nrm.p, nact, act));
    ++h->refine_batch_residuals;
    const long long seq = ++h->refm_seq;
    HIPCHK(launch_refine_record(st, h->refm_nrm.p, h->refm_rec.p, seq));
    long long rec[2 * kMultiRhs + 2];
    rc = read_refine_record(h, seq, rec);
    if (rc != SMLU_OK) return rc;
    int nsurv = 0;
    for (int s = 0; s < nact; ++s) {
      const int j = act[s];
      double nrm, berr;
      std::memcpy(&nrm, &rec[1 + 2 * j], sizeof nrm);
      std::memcpy(&berr, &rec[2 + 2 * j], sizeof berr);
      info[j].resid = nrm;
      info[j].berr = berr;
      if (berr <= eps) {
        info[j].stop = 1;
      } else if (berr > 0.5 * prev[j]) {
        info[j].stop = 2;
      } else {
        prev[j] = berr;
        if (nsurv != s)   // the survivor's residual moves down to its new slot
          HIPCHK(hipMemcpyAsync(h->refm_r.p + (size_t)nsurv * n, h->refm_r.p + (size_t)s * n, sizeof(double) * n,
                                hipMemcpyDeviceToDevice, st));
        act[nsurv++] = j;
      }
    }
    nact = nsurv;
    if (nact == 0) break;
    rc = solve(h->refm_r.p, n, h->refm_d.p, n, nact);
    if (rc != SMLU_OK) return rc;
    HIPCHK(launch_axpy_cols(st, n, h->refm_d.p, dX, ldx, nact, act));
    for (int s = 0; s < nact; ++s) ++info[act[s]].steps;
  }
  for (int s = 0; s < nact; ++s) info[act[s]].stop = 3;   // the step limit
  HIPCHK(hipStreamSynchronize(st));
  return SMLU_OK;
}

// The driver of the refined pair: every batch of a call refined as a batch; info may be NULL.  The
// refine_* stats hold the largest over the call's columns, solve_ms the sum of the batches' first solves.
static int refined_cols(smlu_handle* h, const SolveOp& o, int steps, const Cols& c, int64_t nrhs,
                        smlu_refine_info* info) {
  Plan& P = h->plan;
  if (steps > 0) {
    int rc = ensure_refine_batch(h, o.trans);
    if (rc != SMLU_OK) return rc;
  }
  auto solve = [&](const double* b, int64_t lb, double* x, int64_t lx, int w) { return plain_pass(h, o, b, x, w, lb, lx); };
  auto residual = [&](const double* x, int64_t lx, const double* b, double* r, double* nrm, int nact,
                      const int32_t* list) {
    return o.trans ? launch_residual_t_batch(h->stream, P.n, h->Acolp.p, h->Arow.p, h->A.p, x, lx, b, r, nrm, o.conj,
                                             nact, list)
                   : launch_residual_batch(h->stream, P.n, h->Arowptr.p, h->Arow_ent.p, h->Acol.p, h->A.p, x, lx, b, r,
                                           nrm, nact, list);
  };
  int max_steps = 0;
  double max_berr = -1, max_resid = -1, ms = 0;
  int rc = over_chunks(h, c, nrhs, kMultiRhs, [&](const double* b, int64_t ldb, double* x, int64_t ldx, int64_t j, int nb) {
    smlu_refine_info bi[kMultiRhs];
    double bms = 0;
    int r = refine_batch(h, steps, nb, b, ldb, x, ldx, bi, &bms, solve, residual);
    if (r != SMLU_OK) return r;
    ms += bms;
    for (int k = 0; k < nb; ++k) {
      max_steps = std::max(max_steps, (int)bi[k].steps);
      max_berr = std::max(max_berr, bi[k].berr);
      max_resid = std::max(max_resid, bi[k].resid);
      if (info) info[j + k] = bi[k];
    }
    return (int)SMLU_OK;
  });
  if (rc != SMLU_OK) return rc;
  h->refine_steps = max_steps;
  h->refine_berr = max_berr;
  h->refine_resid = max_resid;
  h->solve_ms = ms;
  return SMLU_OK;
}

// Behind every smlu_solve* entry point: the checks, then the columns through their driver.  The
// _device forms (host false) are ordered after the caller's stream.  refined: the batched-refinement
// pair with its max_steps and info; nrhs = 0 touches nothing.
static int solve_call(smlu_handle* h, int op, int64_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx,
                      bool host, bool refined = false, int max_steps = -1, smlu_refine_info* info = nullptr) {
  SolveOp o;
  int rc = check_solve(h, op, refined, max_steps, nrhs, B, ldb, X, ldx, &o);
  if (rc != SMLU_OK || nrhs == 0) return rc;
  HIPCHK(hipSetDevice(h->device));
  if (!host) HIPCHK(after_caller(h));
  const Cols c{B, ldb, X, ldx, host};
  if (!refined) return solve_cols(h, o, c, nrhs);
  return refined_cols(h, o, max_steps < 0 ? auto_refine_steps(h) : max_steps, c, nrhs, info);
}

// a single vector is one column of leading dimension n
static int64_t dim(const smlu_handle* h) { return h ? h->plan.n : 0; }

int smlu_solve(smlu_handle* h, const double* b, double* x) {
  return solve_call(h, SMLU_OP_N, 1, b, dim(h), x, dim(h), true);
}
int smlu_solve_device(smlu_handle* h, const double* d_b, double* d_x) {
  return solve_call(h, SMLU_OP_N, 1, d_b, dim(h), d_x, dim(h), false);
}
int smlu_solve_multi(smlu_handle* h, int64_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx) {
  return solve_call(h, SMLU_OP_N, nrhs, B, ldb, X, ldx, true);
}
int smlu_solve_multi_device(smlu_handle* h, int64_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                            int64_t ldx) {
  return solve_call(h, SMLU_OP_N, nrhs, d_B, ldb, d_X, ldx, false);
}
int smlu_solve_trans(smlu_handle* h, int op, const double* b, double* x) {
  return solve_call(h, op, 1, b, dim(h), x, dim(h), true);
}
int smlu_solve_trans_device(smlu_handle* h, int op, const double* d_b, double* d_x) {
  return solve_call(h, op, 1, d_b, dim(h), d_x, dim(h), false);
}
int smlu_solve_trans_multi(smlu_handle* h, int op, int64_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx) {
  return solve_call(h, op, nrhs, B, ldb, X, ldx, true);
}
int smlu_solve_trans_multi_device(smlu_handle* h, int op, int64_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                                  int64_t ldx) {
  return solve_call(h, op, nrhs, d_B, ldb, d_X, ldx, false);
}
int smlu_solve_refined_multi(smlu_handle* h, int op, int max_steps, int64_t nrhs, const double* B, int64_t ldb,
                             double* X, int64_t ldx, smlu_refine_info* info) {
  return solve_call(h, op, nrhs, B, ldb, X, ldx, true, true, max_steps, info);
}
int smlu_solve_refined_multi_device(smlu_handle* h, int op, int max_steps, int64_t nrhs, const double* d_B,
                                    int64_t ldb, double* d_X, int64_t ldx, smlu_refine_info* info) {
  return solve_call(h, op, nrhs, d_B, ldb, d_X, ldx, false, true, max_steps, info);
}

static int tri_solve_host(smlu_handle* h, double* x, int mode) {
  if (!h || !x) return fail(h, SMLU_ERR_ARG, "NULL argument");
  if (!h->have_numeric) return fail(h, SMLU_ERR_STATE, "no numeric factorization");
  HIPCHK(hipSetDevice(h->device));
  return over_chunks(h, Cols{x, h->plan.n, x, h->plan.n, true}, 1, 1,
                     [&](const double*, int64_t, double* d, int64_t, int64_t, int) { return run_solve_dev(h, nullptr, d, mode); });
}

int smlu_lsolve(smlu_handle* h, double* x) { return tri_solve_host(h, x, 1); }
int smlu_rsolve(smlu_handle* h, double* x) { return tri_solve_host(h, x, 2); }

// ---- the reference's dense-chunk solve layout on the GPU -------------------
// Chunk geometry, negated rectangles and back-to-front U chunks exactly as
// get_chunking_parameters / allocate_chunks / fill_chunks! (src/SharedMemSparseLU.jl:101-243)
// lay them out (quirks Q1-Q4 of SURVEY appendix B), built from the current factors.
int smlu_chunked_setup(smlu_handle* h, int64_t chunk_size) {
  if (!h) return fail(h, SMLU_ERR_ARG, "NULL handle");
  if (!h->have_numeric) return fail(h, SMLU_ERR_STATE, "no numeric factorization");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  Exported X;
  int rc = export_factors(h, X, true);
  if (rc != SMLU_OK) return rc;
  const int64_t n = h->plan.n, m = n;
  int64_t cs = chunk_size > 0 ? chunk_size : 8;   // :67-70
  cs = std::min(cs, n);                           // :72 (clamped with A.n)
  const int64_t T = (m + cs - 1) / cs;            // :108 (with m, quirk Q1)
  {   // the layout is dense per chunk (the reference's): refuse what cannot fit
    double total = 0;
    for (int64_t c = 0; c < T; ++c) {
      const int64_t cmin = c * cs, cmax = std::min(m, (c + 1) * cs), s = cmax - cmin;
      int64_t rmax = cmax, rmin = cmin;
      for (int64_t j = cmin; j < cmax; ++j) {
        if (X.Lp[j + 1] > X.Lp[j]) rmax = std::max(rmax, X.Li[X.Lp[j + 1] - 1] + 1);
        if (X.Up[j + 1] > X.Up[j]) rmin = std::min(rmin, X.Ui[X.Up[j]]);
      }
      total += 2.0 * s * s + (double)(rmax - cmax) * s + (double)(cmin - rmin) * s;
    }
    if (total > 4.0e9)
      return fail(h, SMLU_ERR_ALLOC, "chunked layout needs " + std::to_string(8.0 * total / 1e9) +
                                         " GB (dense chunks, as in the reference); use smlu_solve");
  }
  std::vector<ChunkDesc> desc;
  std::vector<double> data;
  // one chunk: columns [c0, c1), rectangle rows [r0, r1) (0-based)
  auto add = [&](int64_t c0, int64_t c1, int64_t r0, int64_t r1, bool upper) {
    ChunkDesc d;
    d.c0 = c0;
    d.s = c1 - c0;
    d.r0 = r0;
    d.nr = std::max<int64_t>(r1 - r0, 0);
    d.tri = (int64_t)data.size();
    data.resize(data.size() + d.s * d.s, 0.0);
    d.rect = (int64_t)data.size();
    data.resize(data.size() + d.nr * d.s, 0.0);
    const auto& Cp = upper ? X.Up : X.Lp;
    const auto& Ci = upper ? X.Ui : X.Li;
    const auto& Cx = upper ? X.Ux : X.Lx;
    for (int64_t j = c0; j < c1; ++j)
      for (int64_t e = Cp[j]; e < Cp[j + 1]; ++e) {
        const int64_t i = Ci[e];
        const bool in_tri = upper ? i >= c0 : i < c1;
        if (in_tri) data[d.tri + (j - c0) * d.s + (i - c0)] = Cx[e];
        else if (i >= r0 && i < r1) data[d.rect + (j - c0) * d.nr + (i - r0)] = -Cx[e];   // :207, :238
      }
    desc.push_back(d);
  };
  for (int64_t c = 1; c <= T; ++c) {              // L chunks, :111-123
    const int64_t cmin = (c - 1) * cs, cmax = std::min(m, c * cs);
    int64_t rmax = cmax;                          // one past the max row of the chunk's columns
    for (int64_t j = cmin; j < cmax; ++j)
      if (X.Lp[j + 1] > X.Lp[j]) rmax = std::max(rmax, X.Li[X.Lp[j + 1] - 1] + 1);
    add(cmin, cmax, cmax, rmax, false);
  }
  for (int64_t c = 1; c <= T; ++c) {              // U chunks from the back, :132-144 (Q2)
    const int64_t cmin = (T - c) * cs, cmax = std::min(m, (T - c + 1) * cs);
    int64_t rmin = cmin;                          // min row of the chunk's columns
    for (int64_t j = cmin; j < cmax; ++j)
      if (X.Up[j + 1] > X.Up[j]) rmin = std::min(rmin, X.Ui[X.Up[j]]);
    add(cmin, cmax, rmin, cmin, true);
  }
  hipStream_t st = h->stream;
  h->ch_data.free();
  h->ch_desc.free();
  h->ch_p.free();
  h->ch_q.free();
  HIPCHK(h->ch_data.upload(data.data(), data.size(), st));
  HIPCHK(h->ch_desc.upload(desc.data(), desc.size(), st));
  HIPCHK(h->ch_p.upload(X.p.data(), X.p.size(), st));
  HIPCHK(h->ch_q.upload(X.q.data(), X.q.size(), st));
  HIPCHK(hipStreamSynchronize(st));
  h->ch_T = T;
  h->ch_size = cs;
  h->ch_version = h->nfactor;
  return SMLU_OK;
}

// ldiv! (:286-342) through the chunked layout: wrk = (Rs.*b)[p]; lsolve!; rsolve!; x[q] = wrk.
// Device pointers; x may alias b.  Refills the chunks when the factors changed since the setup
// (the reference refills them in lu!, :265-276).
int smlu_chunked_ldiv_device(smlu_handle* h, const double* d_b, double* d_x) {
  if (!h || !d_b || !d_x) return fail(h, SMLU_ERR_ARG, "NULL argument");
  if (!h->have_numeric) return fail(h, SMLU_ERR_STATE, "no numeric factorization");
  if (h->ch_version != h->nfactor) {
    int rc = smlu_chunked_setup(h, h->ch_size);
    if (rc != SMLU_OK) return rc;
  }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(after_caller(h));
  hipStream_t st = h->stream;
  const int64_t n = h->plan.n;
  double* w = h->wrk.p;
  HIPCHK(launch_perm_in(st, n, h->ch_p.p, h->Rs.p, d_b, w, 1, n, n));
  HIPCHK(launch_chunked_solve(st, false, h->ch_T, h->ch_desc.p, h->ch_data.p, w));
  HIPCHK(launch_chunked_solve(st, true, h->ch_T, h->ch_desc.p + h->ch_T, h->ch_data.p, w));
  HIPCHK(launch_perm_out(st, n, h->ch_q.p, w, d_x, 1, n, n));
  HIPCHK(hipStreamSynchronize(st));
  return SMLU_OK;
}

int smlu_chunked_ldiv(smlu_handle* h, const double* b, double* x) {
  if (!h || !b || !x) return fail(h, SMLU_ERR_ARG, "NULL argument");
  if (!h->have_numeric) return fail(h, SMLU_ERR_STATE, "no numeric factorization");
  HIPCHK(hipSetDevice(h->device));
  return over_chunks(h, Cols{b, h->plan.n, x, h->plan.n, true}, 1, 1,
                     [&](const double* db, int64_t, double* dx, int64_t, int64_t, int) {
                       return smlu_chunked_ldiv_device(h, db, dx);
                     });
}

