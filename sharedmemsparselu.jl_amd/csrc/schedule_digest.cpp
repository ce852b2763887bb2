// schedule_digest.cpp — section hashes of a built schedule (smlu_plan_schedule_digest): a host-only
// diagnostic that lets a CPU test see that a change to the schedule builder moved nothing.
//
// Output words: 19 FNV-1a hashes (nodes | fac fwd bwd fwdm bwdm | segments | comm |
// ilist xt ae xc ft gptr gent | gt st_tasks ur_tasks | scalars), then the per-kind launch counts of
// fac, fwd and bwd (3 x K_NKIND) and the number of exchange and broadcast steps (2), then the bit
// patterns of gemm_flops, gemm22_flops, gemm_bytes and bytes[0..4] (8 doubles; compared by value,
// not hashed: summation order may change).  Structs are hashed field by field (padding), GEMM
// operands as element offsets from the base of their buffer (which buffer is not hashed: the GPU
// parity tests see a wrong buffer).
#include <cstring>

#include "schedule.hpp"

namespace smlu {
namespace {

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void u64(uint64_t v) {
    for (int i = 0; i < 8; ++i) {
      h ^= (v >> (8 * i)) & 0xff;
      h *= 1099511628211ull;
    }
  }
  void i(int64_t v) { u64((uint64_t)v); }
  template <class T>
  void ints(const std::vector<T>& v) {
    i((int64_t)v.size());
    for (const T& x : v) i((int64_t)x);
  }
};

}  // namespace

void schedule_digest(const Schedule& S, const double bytes[5], std::vector<uint64_t>& out) {
  out.clear();
  const std::vector<Launch>* seqs[5] = {&S.fac, &S.fwd, &S.bwd, &S.fwdm, &S.bwdm};
  const std::vector<size_t>* segs5[5] = {&S.fac_seg, &S.fwd_seg, &S.bwd_seg, &S.fwdm_seg, &S.bwdm_seg};
  const std::vector<int>* cms[3] = {&S.fac_comm, &S.fwd_comm, &S.bwd_comm};
  {
    Fnv f;
    f.i((int64_t)S.hsn.size());
    for (const SNode& r : S.hsn) {
      f.i(r.first); f.i(r.Loff); f.i(r.Uoff); f.i(r.Foff); f.i(r.rowptr); f.i(r.voff);
      f.i(r.ns); f.i(r.nu); f.i(r.parent); f.i(r.nb); f.i(r.mode); f.i(r.chbeg); f.i(r.chend);
      f.i(r.level); f.i(r.cpair);
    }
    f.ints(S.node_front);
    out.push_back(f.h);
  }
  for (int q = 0; q < 5; ++q) {
    Fnv f;
    f.i((int64_t)seqs[q]->size());
    for (const Launch& L : *seqs[q]) {
      f.i(L.kind); f.i(L.node); f.i(L.step); f.i(L.off); f.i(L.cnt); f.i(L.nwg); f.i(L.aux); f.i(L.aux2);
      f.i(L.off2); f.i(L.cnt2); f.i(L.nwg2); f.i(L.grp); f.i(L.side ? 1 : 0);
    }
    out.push_back(f.h);
  }
  {
    Fnv f;
    for (int q = 0; q < 5; ++q) f.ints(*segs5[q]);
    for (int q = 0; q < 3; ++q) f.ints(*cms[q]);
    out.push_back(f.h);
  }
  {
    Fnv f;
    f.i((int64_t)S.comm.size());
    auto segs = [&](const std::vector<HSeg>& v) {
      f.i((int64_t)v.size());
      for (const HSeg& g : v) { f.i(g.sb); f.i(g.so); f.i(g.db); f.i(g.dof); f.i(g.bytes); }
    };
    for (const CommOp& op : S.comm) {
      f.i(op.type);
      f.ints(op.peer); f.ints(op.sbase); f.ints(op.rbase);
      f.ints(op.soff); f.ints(op.roff); f.ints(op.sbytes); f.ints(op.rbytes);
      f.i(op.root); f.ints(op.grp); f.i(op.bbase); f.i(op.bytes);
      segs(op.pack); segs(op.unpack);
      f.i(op.pack0); f.i(op.unpack0);
    }
    out.push_back(f.h);
  }
  { Fnv f; f.ints(S.ilist); out.push_back(f.h); }
  {
    Fnv f;
    f.i((int64_t)S.xt.size());
    for (const XContrib& x : S.xt) { f.i(x.child); f.i(x.pad); f.i(x.src); }
    out.push_back(f.h);
  }
  {
    Fnv f;
    f.i((int64_t)S.ae.size());
    for (const AEnt& a : S.ae) { f.i(a.x); f.i(a.y); }
    out.push_back(f.h);
  }
  {
    Fnv f;
    f.i((int64_t)S.xc.size());
    for (const XCol& c : S.xc) { f.i(c.p); f.i(c.tj); f.i(c.off); f.i(c.cnt); f.i(c.acnt); f.i(c.aoff); }
    out.push_back(f.h);
  }
  {
    Fnv f;
    f.i((int64_t)S.ft.size());
    for (const FrontTile& t : S.ft) { f.i(t.s); f.i(t.pad); f.i(t.wg0); }
    out.push_back(f.h);
  }
  { Fnv f; f.ints(S.gptr); out.push_back(f.h); }
  { Fnv f; f.ints(S.gent); out.push_back(f.h); }
  {
    Fnv f;
    f.i((int64_t)S.gt.size());
    for (const GemmRec& g : S.gt) {
      f.i(g.A.off); f.i(g.B.off); f.i(g.C.off); f.i(g.m); f.i(g.n); f.i(g.k); f.i(g.lda); f.i(g.ldb); f.i(g.ldc);
      f.i(g.tiles_m); f.i(g.gsid); f.i(g.tile0);
    }
    out.push_back(f.h);
  }
  {
    Fnv f;
    f.i((int64_t)S.st_tasks.size());
    for (const SwapTask& s : S.st_tasks) {
      f.i(s.s); f.i(s.kb0); f.i(s.nsub); f.i(s.slot0); f.i(s.a); f.i(s.b); f.i(s.c_lo); f.i(s.c_hi); f.i(s.wg0);
    }
    out.push_back(f.h);
  }
  {
    Fnv f;
    f.i((int64_t)S.ur_tasks.size());
    for (const URowTask& u : S.ur_tasks) {
      f.i(u.s); f.i(u.ob0); f.i(u.ob1); f.i(u.slot0); f.i(u.ld); f.i(u.ncols); f.i(u.coff);
    }
    out.push_back(f.h);
  }
  {
    Fnv f;
    const int64_t scalars[11] = {S.max_list, S.ssync_n, S.ntick, S.voff, S.nnodes, S.gemm_launches,
                                 S.gemm128_launches, S.ob, S.t128_min, S.small_k, S.trsm_gemm};
    for (int64_t v : scalars) f.i(v);
    out.push_back(f.h);
  }
  for (int q = 0; q < 3; ++q) {
    std::vector<uint64_t> cnt(K_NKIND, 0);
    for (const Launch& L : *seqs[q]) ++cnt[L.kind];
    out.insert(out.end(), cnt.begin(), cnt.end());
  }
  uint64_t ntype[2] = {0, 0};
  for (const CommOp& op : S.comm) ++ntype[op.type == 1];
  out.push_back(ntype[0]);
  out.push_back(ntype[1]);
  auto bits = [&](double d) {
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    out.push_back(u);
  };
  bits(S.gemm_flops);
  bits(S.gemm22_flops);
  bits(S.gemm_bytes);
  for (int i = 0; i < 5; ++i) bits(bytes[i]);
}

}  // namespace smlu
