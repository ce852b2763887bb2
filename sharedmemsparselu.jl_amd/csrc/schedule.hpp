// schedule.hpp — the static schedule of the multifrontal refactorization and the solves as plain
// host data: launch records, work lists, tasks and communication steps (schedule_build.cpp builds
// it from the plan; schedule.cpp uploads it).  No device header: the builder compiles with a plain
// host compiler and runs under the host sanitizers (tools/sanitize).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "device.hpp"
#include "plan.hpp"

namespace smlu {

constexpr int kSmallM = 128;     // fronts up to this order are factored whole in LDS
constexpr int kFullPivNs = 512;  // blocked fronts up to this many pivots search all fully-summed rows
constexpr int kNbFull = 32;
constexpr int kNbTile = 64;
constexpr int kSwapStride = 1 + 2 * 64;
constexpr int kOBDefault = 384;   // outer block of the two-level blocked front factorization (256/384/512 within 1 %; 384 best)

enum Kind : int {
  K_EXTADD, K_FRONT_LDS, K_PANEL, K_TRSMU, K_TRSML,
  K_GEMM, K_FWD, K_BWD, K_FWDG, K_TRIF, K_BWDU, K_TRIB, K_GEMM22, K_LASWP, K_STEPTRSM, K_GEMMU,
  K_GEMMO, K_TRIINV, K_BWDU12C, K_VCOPY, K_FWDT, K_BWDT, K_SWEEPF, K_SWEEPB, K_UROWS, K_FWDP, K_NKIND
};
inline const char* const kKindName[] = {"assemble", "small", "panel",
                                  "trsm", "trsm", "gemm", "solve", "solve", "solve", "solve",
                                  "solve", "solve", "gemm22", "trsm", "trsm", "gemmu", "gemmo", "trsm", "solve", "solve",
                                  "solve", "solve", "solve", "solve", "urows", "solve"};
static_assert(sizeof(kKindName) / sizeof(kKindName[0]) == K_NKIND, "one kKindName entry per launch kind");
constexpr int kSolveBigNs = 256;  // fronts with more pivots use the multi-workgroup solve
// ... and so do fronts whose L panel (M x ns entries) exceeds this: one workgroup streams a
// tall panel at single-CU bandwidth (a 10^4-row front with 200 pivots took ~350 us per sweep)
constexpr int64_t kSolveBigWork = 1 << 16;
constexpr int kSolveMicroM = 8;    // tiny fronts with M <= 8: eight per wave (k_fwd_micro / k_bwd_micro)
constexpr int kSolveTinyM = 128;   // fronts with M <= 128 rows and ns <= 64: one wave each (k_fwd_tiny / k_bwd_tiny)

struct Launch {
  int kind = 0;
  int node = 0;                           // K_BWDU12C / K_VCOPY: front or block node
  int step = 0;
  int64_t off = 0, cnt = 0, nwg = 0, aux = 0, aux2 = 0;
  int64_t off2 = 0, cnt2 = 0, nwg2 = 0;   // second work list (merged launches)
  double flops = 0;
  // solves (one GPU): consecutive launches with the same grp > 0 are one level's fronts; in batched
  // solves (the per-block schedule) the side ones (small and tiny fronts) run on the handle's side
  // stream next to the large fronts' chain.
  // factorization (one GPU): side marks the K_TRSML / K_GEMM launches of a step that hold the L rows
  // below the outer block (grp = level + 1); they run on the side stream, off the panel chain
  int grp = 0;
  bool side = false;
};
// Factor launches ahead of which the main stream waits for pending side launches: the readers of
// the rows below an outer block (trailing and F22 updates) and whatever opens the next level.  The
// end of the sequence joins too.  (The builder's checks and enqueue_factor share this rule.)
inline bool fac_joins_side(int kind) {
  return kind == K_GEMMO || kind == K_GEMM22 || kind == K_EXTADD || kind == K_FRONT_LDS;
}

// Host description of one copy of a pack / unpack step, resolved to device addresses once the
// buffers exist: base 0 store, 1 scratch, 2 vbuf, 3 wrk (x), 4 send staging, 5 receive staging,
// 6 broadcast block buffer, 7 tile inverses, 8 swap lists, 9 rowperm; offsets in bytes.
struct HSeg {
  int sb;
  int64_t so;
  int db;
  int64_t dof;
  int64_t bytes;
};

// One communication step between segments of the schedule.
struct CommOp {
  int type = 0;                          // 0: exchange with peers, 1: broadcast within a group
  std::vector<int32_t> peer;             // exchange: peers (ascending)
  std::vector<int> sbase, rbase;         // per peer: buffer (HSeg base ids) and byte offsets
  std::vector<int64_t> soff, roff, sbytes, rbytes;
  int32_t root = -1;                     // broadcast: root and group (ascending, includes root)
  std::vector<int32_t> grp;
  int bbase = 4;                         // broadcast buffer: send staging on the root, the
  int64_t bytes = 0;                     //   block buffer elsewhere
  std::vector<HSeg> pack, unpack;        // copies before / after the transfer
  int64_t pack0 = 0, unpack0 = 0;        // ranges in the device descriptor array (set at upload)
  // per-peer helpers used while the schedule is built
  int at(int32_t p) {
    for (size_t i = 0; i < peer.size(); ++i)
      if (peer[i] == p) return (int)i;
    peer.push_back(p);
    sbase.push_back(4);
    rbase.push_back(5);
    soff.push_back(0);
    roff.push_back(0);
    sbytes.push_back(0);
    rbytes.push_back(0);
    return (int)peer.size() - 1;
  }
};

// A GEMM operand before the buffers exist: buffer (HSeg base ids: 0 store, 1 scratch, 6 block
// buffer, 7 tile inverses) and element offset.
struct Operand {
  int buf = -1;
  int64_t off = 0;
  Operand operator+(int64_t d) const { return Operand{buf, off + d}; }
};
// GemmTask (device.hpp) with unresolved operands; the upload turns it into one.
struct GemmRec {
  Operand A, B, C;
  int32_t m, n, k;
  int32_t lda, ldb, ldc;
  int32_t tiles_m = 0;
  int32_t gsid = -1;
  int64_t tile0 = 0;
  int32_t front = -1;   // F22 update of this front (builder only: neither hashed nor uploaded)
};

struct ScheduleInput {
  const Plan* plan = nullptr;
  const RankLayout* lay = nullptr;   // this rank's offsets and owned column blocks
  Tune tn;
  int rank = 0, nranks = 1;
  bool dominant = false;   // values diagonally dominant: every blocked front on the diagonal-tile path
  int pivmode = 0;         // 1: full-candidate pivoting in every blocked front (re-pivoting refactor)
  bool cpair = false;      // pair-preserving pivots (complex handle)
  bool use_mfma = true;
  int ob = kOBDefault;     // outer block width unless tn.ob overrides
};

struct Schedule {
  // nodes: fronts [0, nsup), then one block node per owned column block of a shared front
  std::vector<SNode> hsn;
  std::vector<int32_t> node_front;                 // node -> front
  int64_t nnodes = 0;
  std::vector<Launch> fac, fwd, bwd;
  std::vector<Launch> fwdm, bwdm;   // per-block launches instead of sweeps: batched right-hand sides (one
                                    // GPU) and the re-run of a solve whose sweep wait timed out
  // the sequences cut into segments at the communication steps
  std::vector<size_t> fac_seg, fwd_seg, bwd_seg;   // launch index where each segment starts
  std::vector<size_t> fwdm_seg, bwdm_seg;
  std::vector<int> fac_comm, fwd_comm, bwd_comm;   // comm op run before segment k >= 1
  std::vector<CommOp> comm;
  // work lists and tasks the launches index (uploaded, then dropped on the host)
  std::vector<int32_t> ilist;
  std::vector<XContrib> xt;
  std::vector<AEnt> ae;
  std::vector<XCol> xc;
  std::vector<FrontTile> ft;
  std::vector<int32_t> gptr, gent;   // k_fwd_pull lists
  std::vector<GemmRec> gt;
  std::vector<SwapTask> st_tasks;
  std::vector<URowTask> ur_tasks;
  // F22 gathered by the Schur GEMM (tile code 143): per task of such a launch (Launch.off2), the
  // contributing children and their inverse row maps; all empty when no front qualifies
  std::vector<F22Gather> g22;
  std::vector<F22Child> g22ch;
  std::vector<int32_t> g22inv;
  int64_t f22_gather_fronts = 0;
  double f22_gather_entries = 0;   // sum of nu^2 over those fronts
  // L rows below the outer block on the side stream (Launch.side in fac): launches, and the rows
  // their TRSM tasks take off the panel chain, summed over the steps
  int64_t side_launches = 0, side_rows = 0;
  // trailing updates in tree order (SMLU_TRAIL_SPAN): the span as built, the fronts that take it,
  // and the longest k of a K_GEMMO task
  int64_t trail_span = 1, trail_fronts = 0, gemmo_kmax = 0;
  // statistics
  double gemm_flops = 0, gemm22_flops = 0;
  double gemm_bytes = 0;      // algorithmic bytes of the GEMM launches: A, B read, C read + written
  int64_t gemm_launches = 0, gemm128_launches = 0;
  int64_t nlaunch = 0;
  // sizes of the buffers the schedule addresses
  int64_t max_list = 1;       // swap-list / tile-inverse slots
  int64_t ssync_n = 0, ntick = 0;   // flags and ticket counters of the sweep launches
  int64_t voff = 0;           // front vectors (doubles)
  bool uses_tinv = false;     // some GEMM operand is a tile inverse
  // knobs as built
  int ob = kOBDefault;        // outer block width (SMLU_OB overrides; multiple of 64)
  int64_t t128_min = 512;     // 128x128 GEMM tiles when a launch has at least this many
  bool small_k = true;        // k <= 64 launches use k_gemm_k64 (SMLU_SMALLK=0: off)
  bool trsm_gemm = true;      // GEMM-form triangular solves of the blocked fronts
  int err_code = 0;           // a failed build: its SMLU_ERR_* code (smlu.h), next to the text returned
};
// the codes a build can fail with (smlu.h is not included here; schedule.cpp checks the values)
constexpr int kSchedErrArg = -1, kSchedErrAlloc = -3, kSchedErrState = -6;

// Builds `out` from scratch; returns an error text ("" = ok) and leaves its code in out.err_code.
std::string build_schedule(const ScheduleInput& in, Schedule& out);
// This rank's layout: the plan's own on one GPU; ordinary fronts + owned column blocks of the
// shared fronts on a partitioned handle.
void rank_layout_of(const Plan& P, int rank, int nranks, RankLayout& Y);
// Section hashes of a built schedule and the bytes it would allocate (schedule_digest.cpp).
void schedule_digest(const Schedule& S, const double bytes[5], std::vector<uint64_t>& out);

}  // namespace smlu
