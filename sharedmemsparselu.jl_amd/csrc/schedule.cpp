// schedule.cpp — the device side of the static schedule (schedule_build.cpp builds it on the
// host): the handle's device buffers, the upload of the schedule's work lists and tasks, and the
// byte report of a schedule that is never uploaded.
#include <cstddef>

#include "handle.hpp"

// Staging of the communication steps: device send / receive staging (largest step) and the
// pinned host staging of a host-memory transport (every peer's message side by side).
static void stage_sizes(const Schedule& S, int64_t& ss, int64_t& rs, int64_t& hs, int64_t& hr) {
  ss = rs = hs = hr = 0;
  for (const CommOp& op : S.comm) {
    int64_t a = 0, b = 0, sa = 0, sb = 0;
    for (size_t i = 0; i < op.peer.size(); ++i) {
      if (op.sbase[i] == 4) a = std::max(a, op.soff[i] + op.sbytes[i]);
      if (op.rbase[i] == 5) b = std::max(b, op.roff[i] + op.rbytes[i]);
      sa += op.sbytes[i];
      sb += op.rbytes[i];
    }
    if (op.type == 1 && op.bbase == 4) a = std::max(a, op.bytes);
    ss = std::max(ss, a);
    rs = std::max(rs, b);
    hs = std::max(hs, std::max(sa, op.type == 1 ? op.bytes : 0));
    hr = std::max(hr, std::max(sb, op.type == 1 ? op.bytes : 0));
  }
}

// Element counts of the large per-handle buffers (doubles).
struct Sizes {
  int64_t store, scratch, bcbuf;
};
static Sizes sizes_of(const Plan& P, const RankLayout& lay, int rank, int nranks) {
  Sizes z{};
  // k_urows reads up to 64 columns and 16 rows past a block (values discarded): pad the store
  int64_t maxM = 1;
  for (int64_t s = 0; s < P.nsup; ++s) maxM = std::max<int64_t>(maxM, P.M(s));
  z.store = std::max<int64_t>(lay.store_size, 1) + 64 * maxM + 4096;
  z.scratch = std::max<int64_t>(lay.scratch_size, 1);
  z.bcbuf = 0;
  if (nranks > 1) {   // received pivot block + tile inverses + swap lists + rowperm
    z.bcbuf = 1;
    for (int64_t s = 0; s < P.nsup; ++s)
      if (P.dist(s) && std::binary_search(P.group[s].begin(), P.group[s].end(), rank))
        z.bcbuf = std::max<int64_t>(z.bcbuf, P.M(s) * P.dob + (P.dob / 64) * 8192 + (P.dob / 64) * kSwapStride / 2 + P.dob / 2 + 64);
  }
  return z;
}

// All schedule-dependent allocations and uploads.  schedule_bytes below lists the same buffers in
// the same order: a buffer added here is added there.
static int upload_schedule(smlu_handle* h) {
  Schedule& S = h->sch;
  hipStream_t st = h->stream;
  static_assert(sizeof(AEnt) == sizeof(int2) && alignof(AEnt) == alignof(int2) && offsetof(AEnt, y) == offsetof(int2, y),
                "the kernels read the A-entry lists as int2");
  HIPCHK(h->sn.upload(S.hsn.data(), S.hsn.size(), st));
  HIPCHK(h->ilist.upload(S.ilist.data(), S.ilist.size(), st));
  HIPCHK(h->xtasks.upload(S.xt.data(), S.xt.size(), st));
  HIPCHK(h->aents.upload(reinterpret_cast<const int2*>(S.ae.data()), S.ae.size(), st));
  HIPCHK(h->ftiles.upload(S.ft.data(), S.ft.size(), st));
  if (!S.gptr.empty()) {
    HIPCHK(h->gptr.upload(S.gptr.data(), S.gptr.size(), st));
    HIPCHK(h->gent.upload(S.gent.data(), S.gent.size(), st));
  }
  if (S.ssync_n > 0) {   // zeroed once per schedule: the sweeps never reset them (epochs, kernels_solve.hip)
    HIPCHK(h->ssync.alloc((size_t)S.ssync_n));
    HIPCHK(h->stick.alloc((size_t)S.ntick));
    HIPCHK(h->sxh.alloc((size_t)S.ssync_n * 64 * kMultiRhs));
    {   // hand-off slots start as the sweep's sentinel (kernels_solve.hip: k_tri_sweep)
      const long long sent = 0x7ff4dead5eed0001ll;
      double sv;
      std::memcpy(&sv, &sent, sizeof sv);
      HIPCHK(launch_fill(st, S.ssync_n * 64 * kMultiRhs, h->sxh.p, sv));
    }
    HIPCHK(hipMemsetAsync(h->ssync.p, 0, sizeof(int32_t) * S.ssync_n, st));
    HIPCHK(hipMemsetAsync(h->stick.p, 0, sizeof(unsigned long long) * S.ntick, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (!h->sstatus.p) {
    HIPCHK(h->sstatus.alloc(1));
    HIPCHK(hipMemsetAsync(h->sstatus.p, 0, sizeof(int32_t), st));
  }
  h->sweep_spin = tune().sweep_spin;
  if (S.uses_tinv || h->nranks > 1) HIPCHK(h->tinv.alloc((size_t)S.max_list * 8192));
  std::vector<GemmTask> gt(S.gt.size());
  {   // GEMM operands: (buffer, offset) -> address
    double* base[8] = {h->store.p, h->scratch.p, nullptr, nullptr, nullptr, nullptr, h->bcbuf.p, h->tinv.p};
    auto addr = [&](const Operand& o) { return o.buf < 0 ? nullptr : base[o.buf] + o.off; };
    for (size_t i = 0; i < gt.size(); ++i) {
      const GemmRec& r = S.gt[i];
      gt[i] = GemmTask{addr(r.A), addr(r.B), addr(r.C), r.m, r.n, r.k, r.lda, r.ldb, r.ldc, r.tiles_m, r.gsid, r.tile0};
    }
  }
  HIPCHK(h->gtasks.upload(gt.data(), gt.size(), st));
  if (!S.g22.empty()) {
    HIPCHK(h->f22tasks.upload(S.g22.data(), S.g22.size(), st));
    HIPCHK(h->f22ch.upload(S.g22ch.data(), S.g22ch.size(), st));
    HIPCHK(h->f22inv.upload(S.g22inv.data(), S.g22inv.size(), st));
  }
  HIPCHK(h->stasks.upload(S.st_tasks.data(), S.st_tasks.size(), st));
  HIPCHK(h->urtasks.upload(S.ur_tasks.data(), S.ur_tasks.size(), st));
  HIPCHK(h->xcols.upload(S.xc.data(), S.xc.size(), st));
  HIPCHK(h->swaps.alloc((size_t)S.max_list * kSwapStride));
  HIPCHK(h->vbuf.alloc((size_t)std::max<int64_t>(S.voff, 1)));
  // communication steps: staging sizes, then every pack / unpack copy as a device descriptor
  if (!S.comm.empty()) {
    int64_t ss, rs, hs, hr;
    stage_sizes(S, ss, rs, hs, hr);
    h->stage_bytes_s = ss;
    h->stage_bytes_r = rs;
    HIPCHK(h->stage_s.alloc((size_t)(ss + 7) / 8 + 1));
    HIPCHK(h->stage_r.alloc((size_t)(rs + 7) / 8 + 1));
    if (!h->tr.device_memory) {
      HIPCHK(hipHostMalloc((void**)&h->hstage_s, (size_t)std::max<int64_t>(hs, 8), 0));
      HIPCHK(hipHostMalloc((void**)&h->hstage_r, (size_t)std::max<int64_t>(hr, 8), 0));
    }
    char* base[10] = {(char*)h->store.p, (char*)h->scratch.p, (char*)h->vbuf.p, (char*)h->wrk.p,
                      (char*)h->stage_s.p, (char*)h->stage_r.p, (char*)h->bcbuf.p, (char*)h->tinv.p,
                      (char*)h->swaps.p, (char*)h->rowperm.p};
    std::vector<SegDesc> d;
    for (CommOp& op : S.comm) {
      auto emit = [&](const std::vector<HSeg>& v, int64_t& at) {
        at = (int64_t)d.size();
        for (const HSeg& g : v)
          d.push_back(SegDesc{(uint64_t)(base[g.sb] + g.so), (uint64_t)(base[g.db] + g.dof), g.bytes / 4});
      };
      emit(op.pack, op.pack0);
      emit(op.unpack, op.unpack0);
    }
    HIPCHK(h->segdesc.upload(d.data(), d.size(), st));
  }
  HIPCHK(hipStreamSynchronize(st));
  // the device holds the work lists and tasks now: only the launch records stay on the host
  S.ilist = {}; S.xt = {}; S.ae = {}; S.xc = {}; S.ft = {}; S.gptr = {}; S.gent = {};
  S.gt = {}; S.st_tasks = {}; S.ur_tasks = {}; S.g22 = {}; S.g22ch = {}; S.g22inv = {};
  return SMLU_OK;
}

// The bytes a rank would allocate for schedule S, without a device (smlu_plan_rank_schedule):
// [0] device bytes in all, [1] factor store, [2] front scratch, [3] staging + received-block
// buffer, [4] pinned host staging (host-memory transports).  The schedule's buffers are those of
// upload_schedule, in its order.
void schedule_bytes(const Plan& P, const RankLayout& lay, const Schedule& S, int rank, int nranks, double out[5]) {
  const Sizes z = sizes_of(P, lay, rank, nranks);
  const double n = (double)P.n, nnzA = (double)P.nnzA;
  const int64_t nnodes = P.nsup + (int64_t)lay.blocks.size();
  int64_t ss, rs, hs, hr;
  stage_sizes(S, ss, rs, hs, hr);
  int64_t nseg = 0;
  for (const CommOp& op : S.comm) nseg += (int64_t)(op.pack.size() + op.unpack.size());
  out[1] = 8.0 * z.store;
  out[2] = 8.0 * z.scratch;
  out[3] = 8.0 * z.bcbuf + (nranks > 1 ? 64.0 : 0.0) + 8.0 * ((ss + 7) / 8 + 1) + 8.0 * ((rs + 7) / 8 + 1);
  out[4] = (double)hs + (double)hr;
  // setup_device: A, Rs, wrk, wrk2, growth, Arowptr, Arow_ent, Arow, p0, q, rows, relmap, chlist,
  // posfirst, rowperm, rowperm0, info, status record
  out[0] = out[1] + out[2] + 8.0 * nnzA + 8.0 * n * 3 + 8.0 + 8.0 * (n + 1) + 4.0 * nnzA * 2 + 8.0 * n * 3 +
           4.0 * (double)(P.s_rows.size() + P.relmap.size() + P.ch_list.size()) + 4.0 * n * 2 + 4.0 * (double)nnodes +
           8.0 * (16 + 5 * 512) + out[3];
  // upload_schedule: sn, ilist, xtasks, aents, ftiles, gptr, gent, ssync, stick, sxh, sstatus,
  // tinv, gtasks (+ the F22 gather records, if any), stasks, urtasks, xcols, swaps, vbuf, segdesc
  out[0] += sizeof(F22Gather) * (double)S.g22.size() + sizeof(F22Child) * (double)S.g22ch.size() +
            4.0 * S.g22inv.size();
  out[0] += sizeof(SNode) * (double)S.hsn.size() + 4.0 * S.ilist.size() + sizeof(XContrib) * (double)S.xt.size() +
            sizeof(AEnt) * (double)S.ae.size() + sizeof(FrontTile) * (double)S.ft.size() +
            4.0 * (S.gptr.size() + S.gent.size()) + 4.0 * S.ssync_n + 8.0 * S.ntick +
            8.0 * 64 * kMultiRhs * S.ssync_n + 4.0 + ((S.uses_tinv || nranks > 1) ? 8.0 * 8192 * S.max_list : 0.0) +
            sizeof(GemmTask) * (double)S.gt.size() + sizeof(SwapTask) * (double)S.st_tasks.size() +
            sizeof(URowTask) * (double)S.ur_tasks.size() + sizeof(XCol) * (double)S.xc.size() +
            4.0 * kSwapStride * S.max_list + 8.0 * std::max<int64_t>(S.voff, 1) + sizeof(SegDesc) * (double)nseg;
}

static int build_and_upload(smlu_handle* h) {
  ScheduleInput in;
  in.plan = &h->plan;
  in.lay = &h->lay;
  in.tn = tune();
  in.rank = h->rank;
  in.nranks = h->nranks;
  in.dominant = h->dominant;
  in.pivmode = h->pivmode;
  in.cpair = h->cpair;
  in.use_mfma = h->opts.use_mfma != 0;
  in.ob = h->sch.ob;
  const std::string e = build_schedule(in, h->sch);
  static_assert(kSchedErrArg == SMLU_ERR_ARG && kSchedErrAlloc == SMLU_ERR_ALLOC && kSchedErrState == SMLU_ERR_STATE,
                "the builder's error codes are smlu.h's");
  if (!e.empty()) return fail(h, h->sch.err_code, e);
  return upload_schedule(h);
}

int setup_device(smlu_handle* h) {
  Plan& P = h->plan;
  HIPCHK(hipSetDevice(h->device));
  // one high-priority stream per handle (the schedule is one stream-ordered sequence)
  int prio_lo = 0, prio_hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  if (!h->stream) HIPCHK(hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prio_hi));
  if (!h->side) HIPCHK(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, prio_hi));
  if (!h->fork_ev) HIPCHK(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
  if (!h->join_ev) HIPCHK(hipEventCreateWithFlags(&h->join_ev, hipEventDisableTiming));
  if (!h->lside_ev) HIPCHK(hipEventCreateWithFlags(&h->lside_ev, hipEventDisableTiming));
  if (!h->ljoin_ev) HIPCHK(hipEventCreateWithFlags(&h->ljoin_ev, hipEventDisableTiming));
  hipStream_t st = h->stream;
  rank_layout_of(P, h->rank, h->nranks, h->lay);
  const Sizes z = sizes_of(P, h->lay, h->rank, h->nranks);
  HIPCHK(h->A.alloc((size_t)std::max<int64_t>(P.nnzA, 1)));
  HIPCHK(h->Rs.alloc((size_t)P.n));
  HIPCHK(h->store.alloc((size_t)z.store));
  HIPCHK(h->scratch.alloc((size_t)z.scratch));
  if (h->nranks > 1) {
    HIPCHK(h->bcbuf.alloc((size_t)z.bcbuf));
    HIPCHK(h->d_red.alloc(8));
  }
  HIPCHK(h->wrk.alloc((size_t)P.n));
  HIPCHK(h->wrk2.alloc((size_t)P.n));
  HIPCHK(h->growth.alloc(2));   // [0] growth maximum, [1] dominance flags (factor.cpp)
  HIPCHK(h->Arowptr.upload(P.Arowptr.data(), P.Arowptr.size(), st));
  HIPCHK(h->Arow_ent.upload(P.Arow_ent.data(), P.Arow_ent.size(), st));
  HIPCHK(h->Arow.upload(P.Arow.data(), P.Arow.size(), st));
  HIPCHK(h->p0.upload(P.p0.data(), P.p0.size(), st));
  HIPCHK(h->q.upload(P.q.data(), P.q.size(), st));
  HIPCHK(h->rows.upload(P.s_rows.data(), P.s_rows.size(), st));
  HIPCHK(h->relmap.upload(P.relmap.data(), P.relmap.size(), st));
  HIPCHK(h->chlist.upload(P.ch_list.data(), P.ch_list.size(), st));
  std::vector<int64_t> pf(P.n);
  for (int64_t s = 0; s < P.nsup; ++s)
    for (int64_t j = P.s_first[s]; j < P.s_first[s + 1]; ++j) pf[j] = P.s_first[s];
  HIPCHK(h->posfirst.upload(pf.data(), pf.size(), st));
  HIPCHK(h->rowperm.alloc((size_t)P.n));
  {
    std::vector<int32_t> id(P.n);
    for (int64_t j = 0; j < P.n; ++j) id[j] = (int32_t)(j - pf[j]);
    HIPCHK(h->rowperm0.upload(id.data(), id.size(), st));
  }
  const int64_t nnodes = P.nsup + (int64_t)h->lay.blocks.size();
  HIPCHK(h->info.alloc((size_t)std::max<int64_t>(nnodes, 1)));
  HIPCHK(init_kernel_attributes());
  if (!h->rb.p) HIPCHK(h->rb.alloc(16 + 5 * 512));   // record + k_status_part's partials
  return build_and_upload(h);
}

// Schedule-dependent device buffers and graphs (rebuilt when the pivoting mode changes).
static void release_schedule(smlu_handle* h) {
  h->release_graphs();
  h->sn.free();
  h->ilist.free();
  h->xtasks.free();
  h->aents.free();
  h->ftiles.free();
  h->gptr.free();
  h->gent.free();
  h->ssync.free();
  h->stick.free();
  h->sxh.free();
  h->gtasks.free();
  h->f22tasks.free();
  h->f22ch.free();
  h->f22inv.free();
  h->stasks.free();
  h->urtasks.free();
  h->xcols.free();
  h->swaps.free();
  h->vbuf.free();
  h->vbufm.free();
  h->tinv.free();
  h->stage_s.free();
  h->stage_r.free();
  h->segdesc.free();
  if (h->hstage_s) (void)hipHostFree(h->hstage_s);
  if (h->hstage_r) (void)hipHostFree(h->hstage_r);
  h->hstage_s = h->hstage_r = nullptr;
}

int rebuild_schedule(smlu_handle* h) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  release_schedule(h);
  return build_and_upload(h);
}

bool has_tile_fronts(const smlu_handle* h) {
  for (const SNode& r : h->sch.hsn)
    if (r.mode == 2) return true;
  return false;
}
