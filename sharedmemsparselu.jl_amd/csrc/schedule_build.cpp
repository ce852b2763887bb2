// schedule_build.cpp — builds the static launch schedule of the multifrontal refactorization and
// the solves from the plan (once per plan and pivoting mode).  Host only: no device header, no
// device address; GEMM operands are (buffer, offset) pairs that the upload resolves (schedule.cpp).
#include "schedule.hpp"

#include <limits>
#include <unordered_map>
#include <utility>

namespace smlu {
namespace {

const Operand kStore{0, 0}, kScratch{1, 0}, kBlockBuf{6, 0}, kTinv{7, 0};

// C(m x n, ldc) -= A(m x k, lda) * B(k x n, ldb)
GemmRec gemm_task(Operand A, Operand B, Operand C, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb,
                  int64_t ldc, int32_t gsid = -1) {
  GemmRec g;
  g.A = A; g.B = B; g.C = C;
  g.m = (int32_t)m; g.n = (int32_t)n; g.k = (int32_t)k;
  g.lda = (int32_t)lda; g.ldb = (int32_t)ldb; g.ldc = (int32_t)ldc;
  g.gsid = gsid;
  return g;
}
// ... as a rank update: skipped when empty, its flops added to fl
void update(std::vector<GemmRec>& cand, double& fl, Operand A, Operand B, Operand C, int64_t m, int64_t n, int64_t k,
            int64_t lda, int64_t ldb, int64_t ldc) {
  if (m <= 0 || n <= 0 || k <= 0) return;
  cand.push_back(gemm_task(A, B, C, m, n, k, lda, ldb, ldc));
  fl += 2.0 * (double)m * (double)n * (double)k;
}
// I - L_kk^-1 (lower) and I - U_kk^-1 (upper) of a tile-inverse slot, 64 x 64, ld 64
Operand tinv_at(int64_t slot, bool upper) { return kTinv + (slot * 8192 + (upper ? 4096 : 0)); }

// Workgroups of one 64-column block step (block at column jb) of a front's triangular solve:
// 256-row chunks of the rows below the block (forward) or above it (backward).
int64_t tri_wg(bool upper, int64_t M, int64_t ns, int64_t jb) {
  if (upper) return std::max<int64_t>(1, (jb + 255) / 256);
  const int64_t bw = std::min<int64_t>(64, ns - jb);
  return std::max<int64_t>(1, (M - jb - bw + 255) / 256);
}

// MFMA 128 tile: code 131 (v3: LDS-DMA staging, kernels_gemm.hip); the F22 launches (k = ns, the
// long-k shapes) take 135, the same tile with the next slice's barrier between its last two
// k-quads (+3 % at k >= 2048, neutral at the k = 384 trailing shapes: tools/gemm_bench)
constexpr int kMfmaTile = 131;
// ... and 143 when some task of the F22 launch gathers its C from the children's F22 blocks
// instead of loading what the assembly wrote (choose_f22_gather)
constexpr int kMfmaGatherTile = 143;
// look-ahead (depth 1) of the shared fronts: the owner of pivot block b+1 applies block b to block
// b+1 first, factors and broadcasts b+1, and only then applies b to its other blocks (`pending`).
// Off: the broadcast is a rendezvous (receivers post it after their own trailing updates), so the
// deferred work only loads the next owner -- the schedule model projects 3.0x instead of 4.3x at
// 256^3 / 8 ranks with it on
constexpr bool kDistLookahead = false;

struct Builder {
  const ScheduleInput& in;
  const Plan& P;
  const RankLayout& Y;
  Schedule& S;
  const int rank, nranks;
  std::string err;
  std::vector<int32_t> blknode;                    // index in Y.blocks -> node
  std::unordered_map<int64_t, int32_t> blkmap;     // (front, block) -> index in Y.blocks
  std::vector<int64_t> fr_ptr;                     // A entries grouped by front, sorted by (local column, local row)
  std::vector<int32_t> fr_ent;
  std::vector<int64_t> LP;                         // this rank's fronts by level (every front when nranks == 1)
  std::vector<int32_t> LS;
  std::vector<std::vector<int32_t>> dfront;        // shared fronts this rank works on, per level
  std::vector<char> dlevel;                        // a level holding any shared front (any rank)
  int64_t dist_slots = 0;                          // swap / tile-inverse slots of the shared front
  int64_t spf = 0;                                 // ... and per blocked front
  int fuse_mode = 0;
  bool fuse_panel = false, fuse_inv = false, fuse_urows = false;
  // front -> index in big (swap-list slots).  Dense over the fronts and set per level without a
  // reset: entries of earlier levels stay, and only the current level's fronts are ever looked up
  std::vector<int64_t> bidx;
  std::vector<int32_t> col_cnt, col_pos;           // front_columns' counters
  std::vector<std::vector<Launch>> bwd_levels;     // backward launches per level, emitted root first
  std::vector<char> f22g;                          // front -> its F22 is gathered by the Schur GEMM
  int cur_level = 0;                               // the level whose launches are being emitted
  std::vector<size_t> lvl_end;                     // S.fac.size() after each level (lside_check)

  Builder(const ScheduleInput& i, Schedule& s)
      : in(i), P(*i.plan), Y(*i.lay), S(s), rank(i.rank), nranks(i.nranks) {}

  // ---- shared helpers ---------------------------------------------------------------------
  // a launch of `kind` at `step` whose work list starts at `off`
  static Launch launch(int kind, int step, size_t off) {
    Launch L;
    L.kind = kind;
    L.step = step;
    L.off = (int64_t)off;
    return L;
  }
  void fail(int code, const char* msg) {
    S.err_code = code;
    err = msg;
  }
  // a communication step ends the current segment of `seq`
  void add_comm(std::vector<Launch>& seq, std::vector<size_t>& seg, std::vector<int>& cm, CommOp&& op) {
    seg.push_back(seq.size());
    cm.push_back((int)S.comm.size());
    S.comm.push_back(std::move(op));
  }
  // where child column jc of c lives: (rank, scratch offset on that rank if it is this rank)
  int32_t child_col(int64_t c, int64_t jc, int64_t* src) const {
    const int64_t nuc = P.nu(c);
    if (!P.dist(c)) {
      if (src && P.owner[c] == rank) *src = Y.Foff[c] + jc * nuc;
      return P.owner[c];
    }
    const int64_t b = P.npblk(c) + jc / P.dob;
    const int32_t o = P.blk_owner(c, b);
    if (src && o == rank) {
      const RankLayout::Blk& B = Y.blocks[blkmap.at((int64_t)c * 1048576 + b)];
      *src = B.foff + (P.ns(c) + jc - B.c0) * nuc;
    }
    return o;
  }
  int32_t node_of(int64_t s, int64_t b) const { return blknode[blkmap.at(s * 1048576 + b)]; }
  int32_t holder(int64_t c) const { return P.dist(c) ? P.blk_owner(c, P.npblk(c) - 1) : P.owner[c]; }
  // fronts whose triangular solves run in GEMM form (tile inverses); they also take the
  // super-block level of the three-level blocking (SB columns; OB for the others)
  bool gform(int64_t s) const { return S.trsm_gemm && S.hsn[s].nb == kNbTile; }
  // swap-list slot of sub-panel u of a front's current outer block
  int64_t slot_of(int64_t s, int64_t u) const { return dist_slots + bidx[s] * spf + u; }
  // Step t of blocked front s: panel columns [kb, kb+w) inside the outer block [ostart, oend); R rows
  // the panel finishes (w for diagonal-tile panels, every fully-summed row for full-candidate ones)
  struct Step {
    int64_t kb, w, ostart, oend, R, M, slot;
  };
  Step geom(int64_t s, int64_t t) const {
    const SNode& r = S.hsn[s];
    Step g;
    g.M = (int64_t)r.ns + r.nu;
    g.kb = t * r.nb;
    g.w = std::min<int64_t>(r.nb, r.ns - g.kb);
    g.ostart = (g.kb / S.ob) * S.ob;
    g.oend = std::min<int64_t>(r.ns, g.ostart + S.ob);
    g.R = r.mode == 1 ? r.ns - g.kb : g.w;
    g.slot = slot_of(s, t % (S.ob / r.nb));
    return g;
  }
  // GEMM launches: 128x128 tiles when the launch has enough of them to fill the GPU,
  // otherwise 64x64 tiles (same per-element arithmetic, bitwise-identical results).
  void add_gemm_launch(std::vector<GemmRec>& cand, double fl, int step, int kind = K_GEMM, bool side = false) {
    if (cand.empty()) return;
    const bool count = kind != K_TRSML;   // GEMM-form TRSM is accounted as "trsm", not GEMM
    int64_t t128 = 0;
    for (auto& g : cand) t128 += (int64_t)((g.m + 127) / 128) * ((g.n + 127) / 128);
    // GEMM-form TRSM (k = n = w <= 64: tall L-row and wide U-row strips) always on the one-shot
    // 64 x 64 tile: the 128 tile would take its generic edge body for the 64-wide strips
    // (round 5: TRSM 23.0 -> 21.3 ms per 128^3 refactor)
    int tile = t128 >= S.t128_min && !(kind == K_TRSML && S.small_k) ? 128 : 64;
    if (tile == 128) tile = in.use_mfma ? kMfmaTile : 64;   // use_mfma = 0: the VALU 64 tile
    if (tile == 131 && step < 0) tile = 135;
    if (tile == 64 && S.small_k) {                    // every k <= 64: one-shot K staging
      int kmax = 0;
      for (auto& g : cand) kmax = std::max(kmax, g.k);
      tile = kmax <= 64 ? 65 : in.use_mfma ? 66 : 64;   // 66: the 64 tile on the matrix cores
    }
    // F22, and the outer trailing updates (tree order: k from one outer block to `span` of them):
    // longest k first, so the launch's last tiles are short ones
    if (step < 0 || kind == K_GEMMO)
      std::stable_sort(cand.begin(), cand.end(), [](const GemmRec& a, const GemmRec& b) { return a.k > b.k; });
    Launch L = launch(step < 0 ? K_GEMM22 : kind, step, S.gt.size());
    if (step < 0 && !f22_gather(cand, tile, L)) return;
    L.aux = tile;
    int64_t tiles = 0;
    const int ts = tile >= 128 ? 128 : 64;
    for (GemmRec& g : cand) {
      if (count) S.gemm_bytes += 8.0 * ((double)g.m * g.k + (double)g.k * g.n + 2.0 * g.m * g.n);
      if (g.A.buf == kTinv.buf || g.B.buf == kTinv.buf) S.uses_tinv = true;
      if (kind == K_GEMMO) S.gemmo_kmax = std::max<int64_t>(S.gemmo_kmax, g.k);
      g.tiles_m = (g.m + ts - 1) / ts;
      g.tile0 = tiles;
      tiles += (int64_t)g.tiles_m * ((g.n + ts - 1) / ts);
      S.gt.push_back(g);
    }
    L.cnt = (int64_t)cand.size();
    L.nwg = tiles;
    L.flops = fl;
    if (side) {   // the L rows below the outer block: the side stream (factor.cpp)
      L.side = true;
      L.grp = cur_level + 1;
      ++S.side_launches;
      if (kind == K_TRSML)
        for (const GemmRec& g : cand) S.side_rows += g.m;
    }
    S.fac.push_back(L);
    if (!count) return;
    S.gemm_flops += fl;
    ++S.gemm_launches;
    if (tile >= 128) ++S.gemm128_launches;
    if (step < 0) S.gemm22_flops += fl;
  }

  // ---- F22 assembled in the Schur GEMM's C prologue ---------------------------------------
  // A blocked front's F22 holds no A entry (an entry belongs to the front of its pivot row or
  // column), so what the assembly writes there is the sum of the children's F22 entries in child
  // order -- written to HBM only for the level's F22 launch to read it back as C.  For the large
  // fronts with few children the tile forms that sum itself (same order, same bits) and the
  // assembly stops at row ns of their non-pivot columns.  One GPU, real values, and only where the
  // level's F22 launch takes the 128 MFMA tile (the test below is add_gemm_launch's).
  void choose_f22_gather(int l) {
    if (nranks > 1 || in.cpair || !in.use_mfma || in.tn.f22_gather_nu <= 0) return;
    int64_t t128 = 0;
    for (int64_t k = LP[l]; k < LP[l + 1]; ++k) {
      const SNode& r = S.hsn[LS[k]];
      if (r.mode != 0 && r.nu > 0 && r.ns > 0) t128 += (int64_t)((r.nu + 127) / 128) * ((r.nu + 127) / 128);
    }
    if (t128 < S.t128_min) return;
    for (int64_t k = LP[l]; k < LP[l + 1]; ++k) {
      const int64_t s = LS[k];
      const SNode& r = S.hsn[s];
      if (r.mode == 0 || r.ns <= 0 || r.nu < in.tn.f22_gather_nu) continue;
      int64_t nch = 0, numax = 0;
      for (int64_t e = P.ch_ptr[s]; e < P.ch_ptr[s + 1]; ++e) {
        nch += P.nu(P.ch_list[e]) > 0;
        numax = std::max(numax, P.nu(P.ch_list[e]));
      }
      // (the tile addresses a child's F22 by 32-bit byte offsets: 8 nu^2 < 2^32)
      if (nch <= in.tn.f22_gather_ch && numax <= 23170) f22g[s] = 1;
    }
  }
  // The gather records of an F22 launch holding such fronts: per task the contributing children
  // with their inverse row maps (parent F22 index -> child F22 index; one map serves rows and
  // columns as the child's relmap does).  Checks that every map inverts its relmap and that the
  // launch writes no F22 range a tile of it reads.  false: failed (err set).
  bool f22_gather(const std::vector<GemmRec>& cand, int& tile, Launch& L) {
    bool any = false;
    for (const GemmRec& g : cand) any = any || (g.front >= 0 && f22g[g.front]);
    if (!any) return true;
    if (tile != 135) {
      fail(kSchedErrState, "internal: F22 gather chosen for a launch off the 128 MFMA tile");
      return false;
    }
    tile = kMfmaGatherTile;
    L.off2 = (int64_t)S.g22.size();
    std::vector<std::pair<int64_t, int64_t>> wr, rd;
    for (const GemmRec& g : cand) {
      wr.push_back({g.C.off, g.C.off + (int64_t)g.ldc * (g.n - 1) + g.m});
      if (g.front < 0 || !f22g[g.front]) {
        S.g22.push_back(F22Gather{0, -1});
        continue;
      }
      const int64_t s = g.front, ns = P.ns(s), nu = P.nu(s);
      F22Gather G{(int32_t)S.g22ch.size(), 0};
      for (int64_t e = P.ch_ptr[s]; e < P.ch_ptr[s + 1]; ++e) {
        const int64_t c = P.ch_list[e], nuc = P.nu(c);
        if (nuc <= 0) continue;
        const int32_t* rm = P.relmap.data() + S.hsn[c].rowptr;
        const int64_t inv0 = (int64_t)S.g22inv.size();
        S.g22inv.resize(inv0 + nu, -1);
        int32_t* inv = S.g22inv.data() + inv0;
        int64_t lo = nu, hi = -1, want = 0, have = 0;
        for (int64_t jc = 0; jc < nuc; ++jc) {
          const int64_t i = (int64_t)rm[jc] - ns;
          if (i < 0) continue;
          if (i >= nu) {
            fail(kSchedErrState, "internal: a child's row map leaves its parent front");
            return false;
          }
          inv[i] = (int32_t)jc;
          lo = std::min(lo, i);
          hi = std::max(hi, i);
          ++want;
        }
        for (int64_t i = 0; i < nu; ++i) have += inv[i] >= 0;
        bool ok = have == want;
        for (int64_t jc = 0; jc < nuc && ok; ++jc)
          if (rm[jc] >= ns) ok = inv[rm[jc] - ns] == jc;
        if (!ok) {
          fail(kSchedErrState, "internal: an F22 gather map does not invert its row map");
          return false;
        }
        if (want == 0) {   // the child lands in the pivot rows and columns only
          S.g22inv.resize(inv0);
          continue;
        }
        S.g22ch.push_back(F22Child{S.hsn[c].Foff, inv0, (int32_t)nuc, (int32_t)lo, (int32_t)hi, 0});
        rd.push_back({S.hsn[c].Foff, S.hsn[c].Foff + nuc * nuc});
        ++G.cnt;
      }
      S.g22.push_back(G);
      ++S.f22_gather_fronts;
      S.f22_gather_entries += (double)nu * (double)nu;
    }
    std::sort(wr.begin(), wr.end());
    for (size_t i = 1; i < wr.size(); ++i) wr[i].second = std::max(wr[i].second, wr[i - 1].second);   // running end
    for (const auto& r : rd) {   // the written ranges that start below r's end must all end at or below its start
      auto it = std::upper_bound(wr.begin(), wr.end(), std::make_pair(r.second, (int64_t)-1));
      if (it != wr.begin() && std::prev(it)->second > r.first) {
        fail(kSchedErrState, "internal: an F22 launch writes a child's F22 block it gathers from");
        return false;
      }
    }
    return true;
  }

  // ---- node records and block nodes -------------------------------------------------------
  // fronts [0, nsup) with this rank's offsets (RankLayout); a shared front (multi-GPU) keeps a
  // front node for its solves and the row maps, plus one block node per owned column block whose
  // offsets are shifted so that the front's column c of the block sits at the usual place
  // (pivot block: L + c*M; update block: U + (c-ns)*ns, F + (c-ns)*nu)
  void nodes() {
    const int64_t nsup = P.nsup;
    // Largest ns factored with full-candidate pivoting.  A diagonally dominant matrix needs no
    // row exchanges (partial pivoting keeps the diagonal and the Schur complements stay
    // dominant), so there every blocked front takes the faster diagonal-tile path (round 6: the
    // mid-size fronts too -- C2 refactor 5.42 -> 3.51 ms, 128^3 465 -> 461 ms); its growth check
    // still flags weak pivots if a refactor's new values lose dominance (the re-pivoting refactor
    // then runs).  SMLU_FULLPIV_NS overrides (dev).
    // a complex handle's pair-preserving pivots search every fully-summed row (mode 1): the
    // diagonal-tile panels have no pair rule
    const int64_t full_piv_ns = (in.pivmode == 1 || in.cpair) ? std::numeric_limits<int64_t>::max()
                                : in.tn.fullpiv_ns >= 0 ? in.tn.fullpiv_ns
                                : in.dominant ? (int64_t)0 : (int64_t)kFullPivNs;
    S.hsn.resize(nsup);
    for (int64_t s = 0; s < nsup; ++s) {
      SNode r{};
      r.first = P.s_first[s];
      r.Loff = Y.Loff[s] >= 0 ? Y.Loff[s] : 0;
      r.Uoff = Y.Uoff[s] >= 0 ? Y.Uoff[s] : 0;
      r.Foff = Y.Foff[s];
      r.rowptr = P.s_rowptr[s];
      r.voff = S.voff;
      r.ns = (int32_t)P.ns(s);
      r.nu = (int32_t)P.nu(s);
      S.voff += P.M(s);
      r.parent = (int32_t)P.s_parent[s];
      if (P.M(s) <= kSmallM) { r.mode = 0; r.nb = 0; }
      else if (r.ns <= full_piv_ns) { r.mode = 1; r.nb = kNbFull; }
      else { r.mode = 2; r.nb = kNbTile; }
      r.chbeg = (int32_t)P.ch_ptr[s];
      r.chend = (int32_t)P.ch_ptr[s + 1];
      r.level = P.s_level[s];
      r.cpair = in.cpair ? 1 : 0;
      if (nranks > 1 && P.dist(s)) { r.mode = 2; r.nb = kNbTile; }   // shared fronts: diagonal-tile pivoting
      S.hsn[s] = r;
    }
    S.node_front.resize(nsup);
    for (int64_t s = 0; s < nsup; ++s) S.node_front[s] = (int32_t)s;
    blknode.resize(Y.blocks.size());
    for (size_t i = 0; i < Y.blocks.size(); ++i) {
      const RankLayout::Blk& B = Y.blocks[i];
      SNode r = S.hsn[B.s];
      const int64_t ns = r.ns, nu = r.nu, M = ns + nu;
      if (B.c0 < ns) {
        r.Loff = B.loff - B.c0 * M;
      } else {
        r.Uoff = B.loff - (B.c0 - ns) * ns;
        r.Foff = B.foff - (B.c0 - ns) * nu;
      }
      blknode[i] = (int32_t)S.hsn.size();
      blkmap[(int64_t)B.s * 1048576 + B.b] = (int32_t)i;
      S.hsn.push_back(r);
      S.node_front.push_back(B.s);
    }
    S.nnodes = (int64_t)S.hsn.size();
  }

  // ---- A entries grouped by front, sorted by (local column, local row) --------------------
  void group_entries() {
    const int64_t nsup = P.nsup;
    fr_ptr.assign(nsup + 1, 0);
    fr_ent.resize((size_t)P.nnzA);
    for (int64_t e = 0; e < P.nnzA; ++e) ++fr_ptr[P.A_s[e] + 1];
    for (int64_t s = 0; s < nsup; ++s) fr_ptr[s + 1] += fr_ptr[s];
    std::vector<int64_t> fp(fr_ptr.begin(), fr_ptr.end() - 1);
    for (int64_t e = 0; e < P.nnzA; ++e) fr_ent[fp[P.A_s[e]]++] = (int32_t)e;
    // (only the fronts this rank assembles: its own and the shared ones of its groups)
    for (int64_t s = 0; s < nsup; ++s) {
      if (nranks > 1 && !(P.dist(s) ? std::binary_search(P.group[s].begin(), P.group[s].end(), rank)
                                    : P.owner[s] == rank))
        continue;
      std::sort(fr_ent.begin() + fr_ptr[s], fr_ent.begin() + fr_ptr[s + 1], [&](int32_t a, int32_t b) {
        return P.A_lj[a] != P.A_lj[b] ? P.A_lj[a] < P.A_lj[b] : P.A_li[a] < P.A_li[b];
      });
    }
  }

  // ---- this rank's fronts by level, the segment bookkeeping and the fusion choices --------
  void levels() {
    LP.assign(P.nlevels + 1, 0);
    dfront.assign(P.nlevels, {});
    dlevel.assign(P.nlevels, 0);
    for (int l = 0; l < P.nlevels; ++l) {
      for (int64_t k = P.lev_ptr[l]; k < P.lev_ptr[l + 1]; ++k) {
        const int64_t s = P.lev_sup[k];
        if (nranks == 1) { LS.push_back((int32_t)s); continue; }
        if (!P.dist(s)) {
          if (P.owner[s] == rank) LS.push_back((int32_t)s);
          continue;
        }
        dlevel[l] = 1;
        if (std::binary_search(P.group[s].begin(), P.group[s].end(), rank)) dfront[l].push_back((int32_t)s);
      }
      LP[l + 1] = (int64_t)LS.size();
    }
    S.fac_seg.assign(1, 0);
    S.fwd_seg.assign(1, 0);
    S.bwd_seg.assign(1, 0);
    bidx.assign(P.nsup, 0);
    dist_slots = nranks > 1 ? S.ob / 32 : 0;
    spf = S.ob / 32;
    // fused panels (k_panel_blk<16, true>: panel + tile inverses + in-block row interchanges) for
    // the GEMM-form fronts (every 64-wide panel then belongs to one): 2, panel + the in-block row
    // interchanges (no k_laswp inside the block) + the tile inverses by 16 x 16 blocks on the
    // matrix cores (no k_tri_inv); 0: three launches
    fuse_mode = !(S.trsm_gemm && S.ob <= 64 + 16 * 20) ? 0 : 2;
    fuse_panel = fuse_mode > 0;
    fuse_inv = fuse_mode == 2;
    // fused U rows at the end of an outer block (k_urows) for the GEMM-form fronts; otherwise
    // one TRSM + one update launch per sub-panel
    fuse_urows = S.ob <= 384;
  }

  // ---- per level: the shared fronts' F22 exchange -----------------------------------------
  // the children's F22 columns move to the owners of the target columns; a rank receives them
  // into its receive area ordered by (source rank, child, column)
  using RecvAt = std::unordered_map<int64_t, int64_t>;   // (child, column) -> scratch offset of a received F22 column
  RecvAt f22_exchange(int l) {
    RecvAt recv_at;
    for (const int32_t t : dfront[l]) {
      CommOp op;
      std::vector<std::vector<std::pair<int64_t, int64_t>>> from(nranks);   // per source: (c, jc)
      for (int64_t e = P.ch_ptr[t]; e < P.ch_ptr[t + 1]; ++e) {
        const int64_t c = P.ch_list[e];
        const int32_t* rm = P.relmap.data() + P.s_rowptr[c];
        const int64_t nuc = P.nu(c);
        for (int64_t jc = 0; jc < nuc; ++jc) {
          const int32_t dst = P.col_owner(t, rm[jc]);
          int64_t src = -1;
          const int32_t o = child_col(c, jc, &src);
          if (o == dst) continue;
          if (o == rank) {            // send: pack into the staging buffer
            const int pi = op.at(dst);
            op.pack.push_back(HSeg{1, 8 * src, 4, 0, 8 * nuc});   // staging offset fixed below
            op.pack.back().db = 1000 + pi;                           // peer marker
            op.sbytes[pi] += 8 * nuc;
          } else if (dst == rank) {
            from[o].push_back({c, jc});
          }
        }
      }
      int64_t ro = Y.recv_off[t];
      for (int32_t o = 0; o < nranks; ++o) {
        if (from[o].empty()) continue;
        const int pi = op.at(o);
        op.rbase[pi] = 1;
        op.roff[pi] = 8 * ro;
        for (auto& cj : from[o]) {
          recv_at[cj.first * 1048576 + cj.second] = ro;
          ro += P.nu(cj.first);
          op.rbytes[pi] += 8 * P.nu(cj.first);
        }
      }
      // send staging offsets: per peer contiguous, in (child, column) order
      std::vector<int64_t> base(op.peer.size(), 0);
      int64_t acc = 0;
      for (size_t i = 0; i < op.peer.size(); ++i) {
        op.soff[i] = acc;
        base[i] = acc;
        acc += op.sbytes[i];
      }
      for (auto& g : op.pack) {
        const int pi = g.db - 1000;
        g.db = 4;
        g.dof = base[pi];
        base[pi] += g.bytes;
      }
      add_comm(S.fac, S.fac_seg, S.fac_comm, std::move(op));
    }
    return recv_at;
  }

  // ---- per level: assembly columns --------------------------------------------------------
  // every column of this level's fronts built once (zeros, scaled A entries, the children's F22
  // columns in child order) -- k_assemble, one wave per column
  void front_columns(int64_t s, const std::vector<std::pair<int64_t, int64_t>>& ranges,
                     const std::vector<int32_t>& nodes, const RecvAt& recv_at) {
    std::vector<int32_t>&cnt = col_cnt, &pos = col_pos;
    const int64_t M = P.M(s);
    cnt.assign(M + 1, 0);
    for (int64_t ci = P.ch_ptr[s]; ci < P.ch_ptr[s + 1]; ++ci) {
      const int64_t c = P.ch_list[ci];
      const int32_t* rm = P.relmap.data() + S.hsn[c].rowptr;
      for (int64_t jc = 0; jc < P.nu(c); ++jc) ++cnt[rm[jc] + 1];
    }
    for (int64_t tj = 0; tj < M; ++tj) cnt[tj + 1] += cnt[tj];
    const int64_t base = (int64_t)S.xt.size();
    S.xt.resize(base + cnt[M]);
    pos.assign(cnt.begin(), cnt.end() - 1);
    for (int64_t ci = P.ch_ptr[s]; ci < P.ch_ptr[s + 1]; ++ci) {
      const int64_t c = P.ch_list[ci];
      const int32_t* rm = P.relmap.data() + S.hsn[c].rowptr;
      for (int64_t jc = 0; jc < P.nu(c); ++jc) {
        int64_t src = -1;
        if (nranks == 1) src = S.hsn[c].Foff + jc * P.nu(c);
        else if (P.col_owner(s, rm[jc]) == rank) {
          if (child_col(c, jc, &src) != rank) src = recv_at.at(c * 1048576 + jc);
        }
        S.xt[base + pos[rm[jc]]++] = XContrib{(int32_t)c, 0, src};
      }
    }
    // A entries of this front by (column, row); one task per column of the given ranges
    int64_t ea = fr_ptr[s];
    const int64_t eb = fr_ptr[s + 1];
    for (size_t ri = 0; ri < ranges.size(); ++ri)
      for (int64_t tj = ranges[ri].first; tj < ranges[ri].second; ++tj) {
        while (ea < eb && P.A_lj[fr_ent[ea]] < tj) ++ea;
        const int64_t a0 = (int64_t)S.ae.size();
        while (ea < eb && P.A_lj[fr_ent[ea]] == tj) {
          S.ae.push_back(AEnt{fr_ent[ea], P.A_li[fr_ent[ea]]});
          ++ea;
        }
        // a gathered front's non-pivot column stops at row ns (the lists stay whole)
        const int32_t tjf = (int32_t)tj | (f22g[s] && tj >= P.ns(s) ? kXColNoF22 : 0);
        S.xc.push_back(XCol{nodes[ri], tjf, base + cnt[tj], cnt[tj + 1] - cnt[tj],
                            (int32_t)((int64_t)S.ae.size() - a0), a0});
      }
  }
  void assembly(int l, const RecvAt& recv_at) {
    Launch L = launch(K_EXTADD, 0, S.xc.size());
    for (int64_t k = LP[l]; k < LP[l + 1]; ++k) {   // small fronts assemble inside k_front_small
      const int64_t s = LS[k];
      if (S.hsn[s].mode != 0) front_columns(s, {{0, P.M(s)}}, {(int32_t)s}, recv_at);
    }
    for (const int32_t t : dfront[l]) {   // the shared front: this rank's column blocks
      std::vector<std::pair<int64_t, int64_t>> ranges;
      std::vector<int32_t> nodes;
      for (size_t i = 0; i < Y.blocks.size(); ++i)
        if (Y.blocks[i].s == t) {
          ranges.push_back({Y.blocks[i].c0, Y.blocks[i].c1});
          nodes.push_back(blknode[i]);
        }
      front_columns(t, ranges, nodes, recv_at);
    }
    L.cnt = (int64_t)S.xc.size() - L.off;
    if (L.cnt > 0) S.fac.push_back(L);
  }

  // ---- per level: small-front size classes and the F22-overlap check ----------------------
  // small fronts (assembly fused into the factorization), launched per size class so that
  // small fronts get small LDS (occupancy); ilist: (front, first A entry, A entry count), the
  // front's A entries as (entry, local column << 16 | local row)
  void small_fronts(int l) {
    const int64_t cls[6] = {16, 32, 48, 64, 96, kSmallM};
    for (int c = 0; c < 6; ++c) {
      Launch L = launch(K_FRONT_LDS, 0, S.ilist.size());
      int64_t Mmax = 0;
      for (int64_t k = LP[l]; k < LP[l + 1]; ++k) {
        int64_t s = LS[k];
        if (S.hsn[s].mode != 0) continue;
        int64_t M = P.M(s);
        if (M > cls[c] || (c > 0 && M <= cls[c - 1])) continue;
        S.ilist.push_back((int32_t)s);
        S.ilist.push_back((int32_t)S.ae.size());
        S.ilist.push_back((int32_t)(fr_ptr[s + 1] - fr_ptr[s]));
        for (int64_t e = fr_ptr[s]; e < fr_ptr[s + 1]; ++e) {
          const int32_t id = fr_ent[e];
          S.ae.push_back(AEnt{id, (int32_t)((P.A_lj[id] << 16) | P.A_li[id])});
        }
        Mmax = std::max(Mmax, M);
      }
      L.cnt = ((int64_t)S.ilist.size() - L.off) / 3;
      L.aux = Mmax;
      // overlap group: the size classes of one level run on two streams (factor.cpp).  That is
      // race-free only because the scratch plan (plan.cpp: one F22 block per level, live until
      // the parents' level) keeps every F22 a front of this level writes disjoint from every
      // other one and from the children's F22 the level reads -- checked below.  (Round 6: the
      // level's blocked fronts on a third stream next to them, C2 3.51 -> 4.25 ms: not kept.)
      L.aux2 = l + 1;
      if (L.cnt > 0) S.fac.push_back(L);
    }
    std::vector<std::pair<int64_t, int64_t>> wr, rd;   // F22 ranges written / read by the level
    for (int64_t k = LP[l]; k < LP[l + 1]; ++k) {
      const int64_t s = LS[k];
      if (S.hsn[s].mode != 0) continue;
      const int64_t nu = P.nu(s);
      if (nu > 0 && S.hsn[s].Foff >= 0) wr.push_back({S.hsn[s].Foff, S.hsn[s].Foff + nu * nu});
      for (int64_t e = P.ch_ptr[s]; e < P.ch_ptr[s + 1]; ++e) {
        const int64_t c = P.ch_list[e], nuc = P.nu(c);
        if (nuc > 0 && S.hsn[c].Foff >= 0) rd.push_back({S.hsn[c].Foff, S.hsn[c].Foff + nuc * nuc});
      }
    }
    std::sort(wr.begin(), wr.end());
    for (size_t i = 1; i < wr.size(); ++i)
      if (wr[i].first < wr[i - 1].second) {
        fail(kSchedErrState, "internal: overlapping F22 blocks in one level");
        return;
      }
    for (const auto& r : rd) {   // a read range must not meet any written range
      auto it = std::upper_bound(wr.begin(), wr.end(), std::make_pair(r.second, (int64_t)-1));
      if (it != wr.begin() && std::prev(it)->second > r.first) {
        fail(kSchedErrState, "internal: a level's F22 block overlaps a child's F22 it reads");
        return;
      }
    }
  }

  // ---- per level: blocked-front steps and the F22 update ----------------------------------
  void blocked_fronts(int l) {
    std::vector<int64_t> big;   // this level's blocked fronts
    int64_t maxsteps = 0;
    for (int64_t k = LP[l]; k < LP[l + 1]; ++k) {
      int64_t s = LS[k];
      const SNode& r = S.hsn[s];
      if (r.mode == 0) continue;
      bidx[s] = (int64_t)big.size();
      big.push_back(s);
      S.trail_fronts += trail(s);
      maxsteps = std::max<int64_t>(maxsteps, (r.ns + r.nb - 1) / r.nb);
    }
    S.max_list = std::max<int64_t>(S.max_list, dist_slots + (int64_t)big.size() * spf);
    for (int64_t t = 0; t < maxsteps; ++t) {
      std::vector<int64_t> act;
      for (auto s : big) {
        const SNode& r = S.hsn[s];
        if (t * r.nb < r.ns) act.push_back(s);
      }
      if (act.empty()) continue;
      step_panels(t, act);
      if (!err.empty()) return;
      step_solves(t, act);
      // end of an outer block [ostart, oend): deferred row swaps on the columns outside it, the
      // U rows of the block right of it, and the trailing update with k = oend - ostart
      std::vector<int64_t> fin_all;
      for (auto s : act) {
        const Step g = geom(s, t);
        if (g.kb + g.w == g.oend) fin_all.push_back(s);
      }
      if (!fin_all.empty()) outer_block_end(t, fin_all);
    }
    // F22 -= L21 * U12 for the blocked fronts of this level
    std::vector<GemmRec> cand;
    double fl = 0;
    for (auto s : big) {
      const SNode& r = S.hsn[s];
      const size_t had = cand.size();
      update(cand, fl, kStore + r.Loff + r.ns, kStore + r.Uoff, kScratch + r.Foff, r.nu, r.nu, r.ns,
             (int64_t)r.ns + r.nu, r.ns, r.nu);
      if (cand.size() > had) cand.back().front = (int32_t)s;
    }
    add_gemm_launch(cand, fl, -1);
  }
  // panel launch classes by register-kernel shape: (W=64, 1 wave), (W=32, 1/2/4/8 waves)
  int pclass(int64_t s, int64_t t) const {
    const SNode& r = S.hsn[s];   // (a sort key: R without the rest of geom)
    if (r.nb > 32) return 0;
    const int64_t R = r.mode == 1 ? r.ns - t * r.nb : std::min<int64_t>(r.nb, r.ns - t * r.nb);
    return R <= 64 ? 1 : R <= 128 ? 2 : R <= 256 ? 3 : R <= 512 ? 4 : 5;
  }
  void step_panels(int64_t t, std::vector<int64_t>& act) {
    std::stable_sort(act.begin(), act.end(), [&](int64_t a, int64_t b) { return pclass(a, t) < pclass(b, t); });
    size_t pos = 0;
    for (int c = 0; c < 6 && pos < act.size(); ++c) {
      Launch L = launch(K_PANEL, (int)t, S.ilist.size());
      int64_t rmax = 1, wmax = 1, cnt = 0;
      while (pos < act.size() && pclass(act[pos], t) == c) {
        const Step g = geom(act[pos], t);
        rmax = std::max(rmax, g.R);
        wmax = std::max<int64_t>(wmax, S.hsn[act[pos]].nb);
        S.ilist.push_back((int32_t)act[pos]);
        S.ilist.push_back((int32_t)g.slot);
        ++pos;
        ++cnt;
      }
      L.cnt = cnt;
      L.aux = 0;
      L.nwg = rmax;
      L.aux2 = wmax;
      L.cnt2 = c == 0 ? fuse_mode : 0;   // 64-wide panels of GEMM-form fronts: fused tail
      if (L.cnt > 0) S.fac.push_back(L);
    }
    if (pos != act.size()) fail(kSchedErrArg, "internal: panel classes");
  }
  // after the panels of step t: tile inverses, in-block row swaps, the triangular solves of the
  // step and the trailing update inside the outer block
  void step_solves(int64_t t, const std::vector<int64_t>& act) {
    Launch L;
    // inverses of the diagonal tiles of the GEMM-form fronts (I - L_kk^-1, I - U_kk^-1)
    L.kind = K_TRIINV;
    L.step = (int)t;
    L.off = (int64_t)S.ilist.size();
    for (auto s : act) {
      if (!gform(s) || fuse_inv) continue;   // fused into the panel launch
      S.ilist.push_back((int32_t)s);
      S.ilist.push_back((int32_t)geom(s, t).slot);
    }
    L.cnt = ((int64_t)S.ilist.size() - L.off) / 2;
    if (L.cnt > 0) S.fac.push_back(L);
    // row swaps inside the outer block (the other columns get them at the end of the block)
    L = launch(K_LASWP, (int)t, S.st_tasks.size());
    int64_t wg = 0;
    for (auto s : act) {
      const Step g = geom(s, t);
      const int64_t ncol = g.oend - g.ostart - g.w;
      if (ncol <= 0 || (fuse_panel && gform(s))) continue;   // fused panels swap these rows themselves
      S.st_tasks.push_back(SwapTask{(int32_t)s, (int32_t)g.kb, 1, (int32_t)g.slot, (int32_t)g.ostart,
                                    (int32_t)g.oend, (int32_t)g.kb, (int32_t)(g.kb + g.w), wg});
      wg += (ncol + 63) / 64;
    }
    L.cnt = (int64_t)S.st_tasks.size() - L.off;
    L.nwg = wg;
    if (wg > 0) S.fac.push_back(L);
    // k_step_trsm of the other fronts: U rows right of the panel, then L rows below it
    Launch T = launch(K_STEPTRSM, (int)t, S.ft.size());
    int64_t wgU = 0, W = 32, ntri = 0;
    for (auto s : act) {
      if (gform(s)) continue;
      ++ntri;
      const Step g = geom(s, t);
      S.ft.push_back(FrontTile{(int32_t)s, (int32_t)g.kb, wgU});
      wgU += (g.oend - g.kb - g.w + 255) / 256;
      W = std::max<int64_t>(W, g.w);
    }
    T.cnt = ntri;
    T.nwg = wgU;
    T.off2 = (int64_t)S.ft.size();
    int64_t wgL = 0;
    for (auto s : act) {
      if (gform(s)) continue;
      const Step g = geom(s, t);
      S.ft.push_back(FrontTile{(int32_t)s, (int32_t)g.kb, wgL});
      wgL += (g.M - g.kb - g.R + 255) / 256;
    }
    T.cnt2 = ntri;
    T.nwg2 = wgL;
    T.aux = W;
    if (wgU + wgL > 0) S.fac.push_back(T);
    // GEMM-form step TRSM of the blocked fronts, in place:
    //   U rows [kb, kb+w) x columns [kb+w, oend):  C - (I - L_kk^-1) C = L_kk^-1 C
    //   L rows [kb+R, M) x columns [kb, kb+w):     C - C (I - U_kk^-1) = C U_kk^-1 (+ growth)
    //
    // L rows below the outer block on the side stream (lside): in a diagonal-tile step nothing
    // before the block's trailing update (k = OB width) or the level's F22 update reads the rows
    // [oend, M) of the block's columns -- the panels (k_panel_blk: R = w candidate rows, the tile's
    // interchanges on rows [kb, kb+w)), k_laswp and k_urows stay inside rows [ostart, oend) -- so
    // of a front with at least lside_min such rows both tasks are cut at row oend, and the lower
    // parts form a second K_TRSML and a second K_GEMM launch marked `side`.  They need this step's
    // panel (NU_t) and U rows, follow the previous step's side launches, and are joined ahead of
    // the launches of fac_joins_side.  Same tiles, same k = 64 updates per element in the same order.
    std::vector<GemmRec> tri, cand, stri, scand;
    double fl = 0, sfl = 0;
    for (auto s : act) {
      const Step g = geom(s, t);
      const Operand F = kStore + S.hsn[s].Loff;
      // rows of the L-row solve / the in-block update that stay in the chain
      const int64_t cut = lside(s, g) ? g.oend : g.M;
      if (gform(s)) {
        if (g.oend - g.kb - g.w > 0) {
          const Operand X = F + (g.kb + g.w) * g.M + g.kb;
          tri.push_back(gemm_task(tinv_at(g.slot, false), X, X, g.w, g.oend - g.kb - g.w, g.w, 64, g.M, g.M));
          tri.back().front = (int32_t)s;
        }
        if (cut - g.kb - g.R > 0) {
          const Operand X = F + g.kb * g.M + g.kb + g.R;
          tri.push_back(gemm_task(X, tinv_at(g.slot, true), X, cut - g.kb - g.R, g.w, g.w, g.M, 64, g.M, (int32_t)s));
          tri.back().front = (int32_t)s;
        }
        if (cut < g.M) {
          const Operand X = F + g.kb * g.M + cut;
          stri.push_back(gemm_task(X, tinv_at(g.slot, true), X, g.M - cut, g.w, g.w, g.M, 64, g.M, (int32_t)s));
          stri.back().front = (int32_t)s;
        }
      }
      // inner trailing update: rows [kb+w, M) x columns [kb+w, oend) of the outer block
      const size_t had = cand.size(), shad = scand.size();
      update(cand, fl, F + g.kb * g.M + g.kb + g.w, F + (g.kb + g.w) * g.M + g.kb,
             F + (g.kb + g.w) * g.M + g.kb + g.w, cut - g.kb - g.w, g.oend - g.kb - g.w, g.w, g.M, g.M, g.M);
      if (cut < g.M)
        update(scand, sfl, F + g.kb * g.M + cut, F + (g.kb + g.w) * g.M + g.kb, F + (g.kb + g.w) * g.M + cut,
               g.M - cut, g.oend - g.kb - g.w, g.w, g.M, g.M, g.M);
      if (cand.size() > had) cand.back().front = (int32_t)s;
      if (scand.size() > shad) scand.back().front = (int32_t)s;
    }
    // (the side launches stand right behind the step's TRSM: factor.cpp records their start
    // event after the last main-stream launch ahead of them, and issues them behind the next one)
    add_gemm_launch(tri, 0.0, (int)t, K_TRSML);
    add_gemm_launch(stri, 0.0, (int)t, K_TRSML, true);
    add_gemm_launch(scand, sfl, (int)t, K_GEMM, true);
    add_gemm_launch(cand, fl, (int)t);
  }
  // Whether step g of front s sends its L rows below the outer block to the side stream: one GPU,
  // a schedule whose blocked fronts all pivot inside the diagonal tile (dominant values), and
  // enough rows there to be worth two more launches per step (SMLU_LSIDE_MIN; 0: off)
  bool lside(int64_t s, const Step& g) const {
    return nranks == 1 && in.tn.lside_min > 0 && in.dominant && in.pivmode == 0 && !in.cpair && gform(s) &&
           S.hsn[s].mode == 2 && g.M - g.oend >= in.tn.lside_min;
  }
  // The side launches checked over the finished factor sequence.  Every side task belongs to a
  // diagonal-tile front, lies in the columns of one outer block, and its rows (C, and the L rows an
  // update reads) start at or below that block's end and stay inside the front.  While a front has
  // side launches pending, its step tasks on the main stream end at or above that row.  And a join
  // (fac_joins_side, or the end of the sequence) comes before the first launch of another level.
  // The join ahead of K_GEMMO is also what keeps the tile inverses alive: their slots are reused
  // per outer block (slot = t mod OB/64, and per level by the next level's fronts), so the next
  // block's panels must not start before the side stream has read NU of this block's steps.
  void lside_check() {
    if (S.side_launches == 0) return;
    struct Pos {
      int64_t row, col, oend, M;
    };
    auto where = [&](const GemmRec& g, const Operand& X, Pos& p) {
      if (g.front < 0 || X.buf != kStore.buf) return false;
      const SNode& r = S.hsn[g.front];
      p.M = (int64_t)r.ns + r.nu;
      const int64_t rel = X.off - r.Loff;
      if (rel < 0 || rel >= p.M * r.ns) return false;
      p.col = rel / p.M;
      p.row = rel % p.M;
      p.oend = std::min<int64_t>(r.ns, (p.col / S.ob + 1) * S.ob);
      return true;
    };
    std::vector<char> pend(P.nsup, 0);   // fronts with side launches not yet joined
    std::vector<int32_t> plist;
    size_t lv = 0, plevel = 0;
    for (size_t i = 0; i < S.fac.size(); ++i) {
      while (lv < lvl_end.size() && lvl_end[lv] <= i) ++lv;   // the level of launch i
      const Launch& L = S.fac[i];
      const bool step_gemm = L.kind == K_TRSML || L.kind == K_GEMM;
      if (L.side) {
        if (!step_gemm || L.grp != (int)lv + 1) return fail(kSchedErrState, "internal: a side launch of another kind or level");
        for (int64_t j = L.off; j < L.off + L.cnt; ++j) {
          const GemmRec& g = S.gt[j];
          Pos c{}, a{};
          bool ok = where(g, g.C, c) && S.hsn[g.front].mode == 2 && c.row >= c.oend && c.row + g.m <= c.M &&
                    c.col + g.n <= c.oend;
          if (ok && L.kind == K_GEMM) ok = where(g, g.A, a) && a.row == c.row && a.oend == c.oend;
          if (!ok) return fail(kSchedErrState, "internal: a side task reaches above its outer block's end");
          if (!pend[g.front]) {
            pend[g.front] = 1;
            plist.push_back(g.front);
          }
        }
        plevel = lv;
        continue;
      }
      if (plist.empty()) continue;
      if (fac_joins_side(L.kind)) {
        for (const int32_t f : plist) pend[f] = 0;
        plist.clear();
        continue;
      }
      if (lv != plevel) return fail(kSchedErrState, "internal: side launches not joined before the next level");
      if (!step_gemm) continue;
      for (int64_t j = L.off; j < L.off + L.cnt; ++j) {
        const GemmRec& g = S.gt[j];
        Pos c{};
        if (g.front < 0 || !pend[g.front]) continue;
        if (!where(g, g.C, c) || c.row + g.m > c.oend)
          return fail(kSchedErrState, "internal: a main-stream task writes rows a pending side launch owns");
      }
    }
  }
  // End of an outer block: the deferred row swaps on the columns outside it, its U rows on every
  // column right of it (sub-panel by sub-panel, k_urows or GEMM-form TRSM), then the trailing
  // update with k = OB width
  void outer_block_end(int64_t t, const std::vector<int64_t>& fin_all) {
    Launch L = launch(K_LASWP, (int)t, S.st_tasks.size());
    int64_t wg = 0;
    for (auto s : fin_all) {
      const SNode& r = S.hsn[s];
      const Step g = geom(s, t);
      const int64_t ncol = g.M - (g.oend - g.ostart);
      if (ncol <= 0) continue;
      S.st_tasks.push_back(SwapTask{(int32_t)s, (int32_t)g.ostart, (int32_t)((g.oend - g.ostart + r.nb - 1) / r.nb),
                                    (int32_t)slot_of(s, (g.ostart % S.ob) / r.nb), 0, (int32_t)g.M,
                                    (int32_t)g.ostart, (int32_t)g.oend, wg});
      wg += (ncol + 63) / 64;
    }
    L.cnt = (int64_t)S.st_tasks.size() - L.off;
    L.nwg = wg;
    if (wg > 0) S.fac.push_back(L);
    std::vector<URows> items;
    std::vector<GemmRec> c1;
    double fl1 = 0;
    for (auto s : fin_all) {
      const SNode& r = S.hsn[s];
      const Step g = geom(s, t);
      if (g.oend == g.M) continue;   // nothing right of the block
      items.push_back(URows{s, g.ostart, g.oend, g.oend, r.ns, true});
      // L columns and U rows [k0, oend) applied to the block rows and columns [oend, e): the whole
      // trailing part (e = ns) with the block just finished, or, in tree order, the next lowbit(j)
      // outer blocks with the last lowbit(j) finished ones
      int64_t k0 = g.ostart, e = r.ns;
      if (trail(s) && g.oend < r.ns) {
        const int64_t j = g.oend / S.ob, span = in.tn.trail_span, b = j & -j;
        if (span > 0 && j % span == 0) {
          k0 = (j - span) * S.ob;
        } else {
          k0 = (j - b) * S.ob;
          e = std::min<int64_t>(r.ns, (j + b) * S.ob);
        }
      }
      rank_update(s, g.oend, g.M, g.oend, e, false, k0, g.oend, c1, fl1);   // column strip, with the L21 rows
      rank_update(s, g.oend, e, e, r.ns, true, k0, g.oend, c1, fl1);        // row strip and its U12 rows
    }
    urows(t, items);
    add_gemm_launch(c1, fl1, (int)t, K_GEMMO);
  }
  struct URows {
    int64_t s, ob0, ob1, c0, c1;   // OB rows [ob0, ob1); L-panel columns [c0, c1); + U12 if u12
    bool u12;
  };
  // TRSM of the U rows of a set of OBs (one per front), sub-panel by sub-panel: L_uu^-1 C in
  // place on the given columns, then the rows below the sub-panel inside the OB
  void urows(int64_t t, const std::vector<URows>& all_items) {
    // GEMM-form fronts: one fused k_urows launch (every column block runs the whole
    // sub-panel sequence); the others keep one launch pair per sub-panel
    std::vector<URows> items;
    Launch L = launch(K_UROWS, (int)t, S.ur_tasks.size());
    for (auto& it : all_items) {
      const SNode& r = S.hsn[it.s];
      if (!(fuse_urows && gform(it.s))) {
        items.push_back(it);
        continue;
      }
      const int64_t M = (int64_t)r.ns + r.nu;
      const int32_t slot0 = (int32_t)slot_of(it.s, (it.ob0 % S.ob) / r.nb);
      for (int64_t c = it.c0; c < it.c1; c += kUrowsCols)
        S.ur_tasks.push_back(URowTask{(int32_t)it.s, (int32_t)it.ob0, (int32_t)it.ob1, slot0, (int32_t)M,
                                      (int32_t)std::min<int64_t>(kUrowsCols, it.c1 - c), r.Loff + c * M});
      if (it.u12)
        for (int64_t c = 0; c < r.nu; c += kUrowsCols)
          S.ur_tasks.push_back(URowTask{(int32_t)it.s, (int32_t)it.ob0, (int32_t)it.ob1, slot0, r.ns,
                                        (int32_t)std::min<int64_t>(kUrowsCols, r.nu - c), r.Uoff + c * r.ns});
    }
    L.cnt = (int64_t)S.ur_tasks.size() - L.off;
    if (L.cnt > 0) S.fac.push_back(L);
    int64_t nsub = 0;
    for (auto& it : items) nsub = std::max<int64_t>(nsub, (it.ob1 - it.ob0 + S.hsn[it.s].nb - 1) / S.hsn[it.s].nb);
    for (int64_t u = 0; u < nsub; ++u) {
      L = Launch();
      L.kind = K_TRSMU;
      L.step = (int)t;
      L.aux = 1;   // outer mode
      L.off = (int64_t)S.ft.size();
      int64_t wg = 0, cnt = 0;
      std::vector<GemmRec> cand, ctri;
      double fl = 0;
      for (auto& it : items) {
        const int64_t s = it.s;
        const SNode& r = S.hsn[s];
        const int64_t M = (int64_t)r.ns + r.nu;
        const int64_t kbu = it.ob0 + u * r.nb;
        if (kbu >= it.ob1) continue;
        const int64_t wu = std::min<int64_t>(r.nb, it.ob1 - kbu);
        const int64_t n1 = it.c1 - it.c0;
        const Operand F = kStore + r.Loff, U = kStore + r.Uoff;
        const bool u12 = it.u12 && r.nu > 0;
        if (gform(s)) {   // U rows [kbu, kbu+wu) on the columns: L_uu^-1 C, in place
          const Operand Ti = tinv_at(slot_of(s, (kbu % S.ob) / r.nb), false);
          if (n1 > 0) ctri.push_back(gemm_task(Ti, F + it.c0 * M + kbu, F + it.c0 * M + kbu, wu, n1, wu, 64, M, M));
          if (u12) ctri.push_back(gemm_task(Ti, U + kbu, U + kbu, wu, r.nu, wu, 64, r.ns, r.ns));
        } else {          // k_trsm_u: columns [oend, M) of the plain two-level scheme
          S.ft.push_back(FrontTile{(int32_t)s, (int32_t)kbu, wg});
          wg += (M - it.c0 + 255) / 256;
          ++cnt;
        }
        // rows below the sub-panel inside the OB: [kbu+wu, ob1) x the columns
        const int64_t m = it.ob1 - kbu - wu;
        update(cand, fl, F + kbu * M + kbu + wu, F + it.c0 * M + kbu, F + it.c0 * M + kbu + wu, m, n1, wu, M, M, M);
        if (u12) update(cand, fl, F + kbu * M + kbu + wu, U + kbu, U + kbu + wu, m, r.nu, wu, M, r.ns, r.ns);
      }
      L.cnt = cnt;
      L.nwg = wg;
      if (wg > 0) S.fac.push_back(L);
      add_gemm_launch(ctri, 0.0, (int)t, K_TRSML);
      add_gemm_launch(cand, fl, (int)t, K_GEMMU);
    }
  }
  // C(rows [r0, r1) x L-panel columns [c0, c1) (+ U12 when u12)) -= L(rows, [k0, k1)) U([k0, k1), cols)
  void rank_update(int64_t s, int64_t r0, int64_t r1, int64_t c0, int64_t c1, bool u12, int64_t k0, int64_t k1,
                   std::vector<GemmRec>& cand, double& fl) {
    const SNode& r = S.hsn[s];
    const int64_t M = (int64_t)r.ns + r.nu;
    const Operand F = kStore + r.Loff, U = kStore + r.Uoff;
    const size_t had = cand.size();
    update(cand, fl, F + k0 * M + r0, F + c0 * M + k0, F + c0 * M + r0, r1 - r0, c1 - c0, k1 - k0, M, M, M);
    const int64_t ru1 = std::min<int64_t>(r1, r.ns);   // U12 rows live above ns
    if (u12) update(cand, fl, F + k0 * M + r0, U + k0, U + r0, ru1 - r0, r.nu, k1 - k0, M, r.ns, r.ns);
    for (size_t i = had; i < cand.size(); ++i) cand[i].front = (int32_t)s;
  }

  // ---- trailing updates in tree order -----------------------------------------------------
  // Today's order loads, updates (k = OB) and stores block (r, c) of a front once per finished
  // outer block, min(r, c) times.  Only the next outer block's rows and columns have to be complete
  // when its chain starts, so after j finished blocks a qualifying front updates just the blocks
  // with min(r, c) in [j, j + lowbit(j)), with the last lowbit(j) blocks as one k-range (the order
  // of recursive LU; outer_block_end).  With a finite span every span-th boundary updates all that
  // is right of it with k = span * OB instead, and the pattern restarts there.  The k-ranges a
  // block receives tile [0, min(r, c) * OB) once, ascending, each tile one FMA per k from
  // accumulators loaded from C: the FMA sequence of every element is today's.
  // Same conditions as lside: one GPU, every blocked front on the diagonal-tile path.
  bool trail(int64_t s) const {
    const SNode& r = S.hsn[s];
    return nranks == 1 && in.tn.trail_span != 1 && in.dominant && in.pivmode == 0 && !in.cpair && gform(s) &&
           r.mode == 2 && r.ns >= in.tn.trail_ns;
  }
  // The K_GEMMO tasks of the qualifying fronts checked over the finished factor sequence.  Per
  // front, blocks are OB x OB with one more block row (the L21 rows below ns) and one more block
  // column (U12); done[r][c] counts the leading k-blocks applied to block (r, c).  Every task starts
  // at that count on all blocks it covers and ends at the boundary of its launch; the first panel
  // of outer block j finds every block with min(r, c) == j at j; the level's F22 update finds
  // every block complete.
  void trail_check() {
    if (S.trail_fronts == 0) return;
    struct Fr {
      int64_t nB = 0;              // outer blocks; row / column nB: L21 / U12
      std::vector<int32_t> done;   // (nB + 1) x (nB + 1)
    };
    std::unordered_map<int32_t, Fr> fr;
    auto front = [&](int32_t s) -> Fr& {
      Fr& f = fr[s];
      if (f.done.empty()) {
        f.nB = (S.hsn[s].ns + S.ob - 1) / S.ob;
        f.done.assign((size_t)((f.nB + 1) * (f.nB + 1)), 0);
      }
      return f;
    };
    const char* const bad = "internal: a trailing update out of tree order";
    for (const Launch& L : S.fac) {
      if (L.kind == K_GEMMO) {
        for (int64_t i = L.off; i < L.off + L.cnt; ++i) {
          const GemmRec& g = S.gt[i];
          if (g.front < 0 || !trail(g.front)) continue;
          const SNode& r = S.hsn[g.front];
          Fr& f = front(g.front);
          const int64_t ns = r.ns, M = ns + r.nu, ob = S.ob;
          const int64_t a = g.A.off - r.Loff, c = g.C.off - r.Loff, cu = g.C.off - r.Uoff;
          const bool u12 = !(c >= 0 && c < M * ns);
          if (g.A.buf != kStore.buf || g.B.buf != kStore.buf || g.C.buf != kStore.buf || a < 0 || a >= M * ns ||
              g.lda != M || (u12 && (r.nu == 0 || cu < 0 || cu >= ns * r.nu)))
            return fail(kSchedErrState, bad);
          const int64_t k0 = a / M, k1 = k0 + g.k, r0 = a % M, r1 = r0 + g.m;
          // L-panel columns [c0, c1), or all of U12 (block column nB)
          const int64_t c0 = u12 ? ns : c / M, c1 = u12 ? M : c0 + g.n;
          const int64_t ld = u12 ? ns : M, crow = u12 ? cu % ns : c % M, ccol = u12 ? cu / ns : 0;
          // operands: C and B in the same columns, C in A's rows, B in A's k-range; rows and
          // columns from a block's start to a block's end (ns and M end the last ones)
          const bool ok = g.ldc == ld && g.ldb == ld && crow == r0 && ccol == 0 && (!u12 || g.n == r.nu) &&
                          g.B.off == (u12 ? r.Uoff : r.Loff + c0 * M) + k0 && k0 % ob == 0 && k1 % ob == 0 &&
                          k1 == geom(g.front, L.step).oend && k1 < ns && r0 % ob == 0 && r0 >= k1 && r0 < ns &&
                          (r1 == M || (r1 <= ns && (r1 % ob == 0 || r1 == ns))) && (!u12 || r1 <= ns) &&
                          (u12 || (c0 % ob == 0 && c0 >= k1 && c1 <= ns && (c1 % ob == 0 || c1 == ns)));
          if (!ok) return fail(kSchedErrState, bad);
          const int64_t br1 = r1 > ns ? f.nB + 1 : (r1 + ob - 1) / ob;   // block rows [r0 / ob, br1)
          const int64_t bc0 = u12 ? f.nB : c0 / ob, bc1 = u12 ? f.nB + 1 : (c1 + ob - 1) / ob;
          for (int64_t br = r0 / ob; br < br1; ++br)
            for (int64_t bc = bc0; bc < bc1; ++bc) {
              int32_t& d = f.done[(size_t)(br * (f.nB + 1) + bc)];
              if (d != k0 / ob || k1 / ob > std::min(br, bc)) return fail(kSchedErrState, bad);
              d = (int32_t)(k1 / ob);
            }
        }
      } else if (L.kind == K_PANEL) {
        for (int64_t i = L.off; i < L.off + 2 * L.cnt; i += 2) {
          const int32_t s = S.ilist[i];
          if (!trail(s)) continue;
          const Step g = geom(s, L.step);
          if (g.kb != g.ostart) continue;
          const Fr& f = front(s);
          const int64_t j = g.ostart / S.ob;
          for (int64_t q = j; q < f.nB + (S.hsn[s].nu > 0); ++q)   // with the L21 rows and U12
            if (f.done[(size_t)(q * (f.nB + 1) + j)] != j || f.done[(size_t)(j * (f.nB + 1) + q)] != j)
              return fail(kSchedErrState, "internal: an outer block starts before its trailing updates are complete");
        }
      } else if (L.kind == K_GEMM22) {
        for (int64_t i = L.off; i < L.off + L.cnt; ++i) {
          const int32_t s = S.gt[i].front;
          if (s < 0 || !trail(s)) continue;
          const Fr& f = front(s);
          for (int64_t br = 0; br <= f.nB; ++br)
            for (int64_t bc = 0; bc <= f.nB; ++bc)
              if (br + bc < 2 * f.nB && f.done[(size_t)(br * (f.nB + 1) + bc)] != std::min(br, bc))
                return fail(kSchedErrState, "internal: an F22 update before the front's trailing updates are complete");
          fr.erase(s);
        }
      }
    }
  }

  // ---- the shared front's pivot-block chain (multi-GPU) -----------------------------------
  // for each pivot block, its owner runs the inner steps (64-column panels with diagonal-tile
  // pivoting, tile inverses, in-block swaps, GEMM-form triangular solves, in-block updates) on its
  // copy, broadcasts the factored block (L rows [ob, M), tile inverses, swap lists, rowperm) to
  // the group, and every member applies it to the column blocks it owns: deferred swaps, U rows
  // (GEMM-form TRSM per sub-panel), the rows below each sub-panel, and the trailing update
  // (k = block width) down to the F22 rows
  void shared_front(int32_t t) {
    const int64_t np = P.npblk(t);
    std::vector<size_t> mine;
    for (size_t i = 0; i < Y.blocks.size(); ++i)
      if (Y.blocks[i].s == t) mine.push_back(i);
    std::vector<Launch> pending;
    for (int64_t b = 0; b < np; ++b) {
      const bool own = P.blk_owner(t, b) == rank;
      const int32_t bn = own ? node_of(t, b) : -1;
      if (own) shared_block_factor(t, b, bn);
      shared_block_bcast(t, b, bn);
      for (auto& q : pending) S.fac.push_back(q);   // the previous block's deferred updates
      pending.clear();
      shared_block_apply(t, b, bn, mine, pending);
    }
    for (auto& q : pending) S.fac.push_back(q);
  }
  // the owner's inner steps on pivot block b (node bn)
  void shared_block_factor(int32_t t, int64_t b, int32_t bn) {
    const int64_t M = P.M(t), ob = P.blk_c0(t, b), oe = P.blk_c1(t, b);
    const Operand Lb = kStore + S.hsn[bn].Loff;
    for (int64_t kb = ob; kb < oe; kb += 64) {
      const int64_t wk = std::min<int64_t>(64, oe - kb);
      const int step = (int)(kb / 64);
      const int32_t u = (int32_t)((kb - ob) / 64);
      Launch Q = launch(K_PANEL, step, S.ilist.size());
      S.ilist.push_back(bn);
      S.ilist.push_back(u);
      Q.cnt = 1;
      Q.nwg = wk;
      Q.aux2 = 64;
      S.fac.push_back(Q);
      Q = launch(K_TRIINV, step, S.ilist.size());
      S.ilist.push_back(bn);
      S.ilist.push_back(u);
      Q.cnt = 1;
      S.fac.push_back(Q);
      if (oe - ob - wk > 0) {
        Q = launch(K_LASWP, step, S.st_tasks.size());
        S.st_tasks.push_back(SwapTask{bn, (int32_t)kb, 1, u, (int32_t)ob, (int32_t)oe, (int32_t)kb,
                                      (int32_t)(kb + wk), 0});
        Q.cnt = 1;
        Q.nwg = (oe - ob - wk + 63) / 64;
        S.fac.push_back(Q);
      }
      std::vector<GemmRec> tri, cand;
      double fl = 0;
      if (oe - kb - wk > 0) {
        const Operand X = Lb + (kb + wk) * M + kb;
        tri.push_back(gemm_task(tinv_at(u, false), X, X, wk, oe - kb - wk, wk, 64, M, M));
      }
      if (M - kb - wk > 0) {
        const Operand X = Lb + kb * M + kb + wk;
        tri.push_back(gemm_task(X, tinv_at(u, true), X, M - kb - wk, wk, wk, M, 64, M, bn));
      }
      add_gemm_launch(tri, 0.0, step, K_TRSML);
      update(cand, fl, Lb + kb * M + kb + wk, Lb + (kb + wk) * M + kb, Lb + (kb + wk) * M + kb + wk, M - kb - wk,
             oe - kb - wk, wk, M, M, M);
      add_gemm_launch(cand, fl, step);
    }
  }
  // broadcast of pivot block b: [L rows [ob, M) x w, ld M-ob | tile inverses | swap lists | rowperm]
  void shared_block_bcast(int32_t t, int64_t b, int32_t bn) {
    const SNode& fr = S.hsn[t];
    const int64_t M = P.M(t), ob = P.blk_c0(t, b), oe = P.blk_c1(t, b), w = oe - ob, nsub = (w + 63) / 64;
    const int64_t lbytes = 8 * (M - ob) * w, tbytes = 8 * nsub * 8192;
    const int64_t swbytes = 4 * nsub * kSwapStride, rpbytes = 4 * w;
    CommOp op;
    op.type = 1;
    op.root = P.blk_owner(t, b);
    op.grp = P.group[t];
    op.bytes = lbytes + tbytes + swbytes + rpbytes;
    if (op.root == rank) {
      op.bbase = 4;
      for (int64_t c = ob; c < oe; ++c)
        op.pack.push_back(HSeg{0, 8 * (S.hsn[bn].Loff + c * M + ob), 4, 8 * (c - ob) * (M - ob), 8 * (M - ob)});
      op.pack.push_back(HSeg{7, 0, 4, lbytes, tbytes});
      op.pack.push_back(HSeg{8, 0, 4, lbytes + tbytes, swbytes});
      op.pack.push_back(HSeg{9, 4 * (fr.first + ob), 4, lbytes + tbytes + swbytes, rpbytes});
    } else {
      op.bbase = 6;
      op.unpack.push_back(HSeg{6, lbytes + tbytes, 8, 0, swbytes});
      op.unpack.push_back(HSeg{6, lbytes + tbytes + swbytes, 9, 4 * (fr.first + ob), rpbytes});
    }
    add_comm(S.fac, S.fac_seg, S.fac_comm, std::move(op));
  }
  // every member applies pivot block b to the column blocks it owns (`mine`)
  void shared_block_apply(int32_t t, int64_t b, int32_t bn, const std::vector<size_t>& mine,
                          std::vector<Launch>& pending) {
    const SNode& fr = S.hsn[t];
    const int64_t ns = fr.ns, nu = fr.nu, M = ns + nu, np = P.npblk(t);
    const int64_t ob = P.blk_c0(t, b), oe = P.blk_c1(t, b), w = oe - ob, nsub = (w + 63) / 64;
    const bool own = bn >= 0;
    const Operand Lb = own ? kStore + S.hsn[bn].Loff : Operand{};
    const int64_t ldL = own ? M : M - ob;
    auto Lsrc = [&](int64_t row, int64_t col) {
      return own ? Lb + col * M + row : kBlockBuf + ((col - ob) * (M - ob) + (row - ob));
    };
    // deferred row swaps on this rank's other blocks (left and right)
    {
      Launch Q = launch(K_LASWP, 0, S.st_tasks.size());
      int64_t wg = 0;
      for (size_t i : mine) {
        const RankLayout::Blk& T = Y.blocks[i];
        if (T.b == b) continue;
        S.st_tasks.push_back(SwapTask{blknode[i], (int32_t)ob, (int32_t)nsub, 0, (int32_t)T.c0, (int32_t)T.c1,
                                      (int32_t)T.c1, (int32_t)T.c1, wg});
        wg += (T.c1 - T.c0 + 63) / 64;
      }
      Q.cnt = (int64_t)S.st_tasks.size() - Q.off;
      Q.nwg = wg;
      if (wg > 0) S.fac.push_back(Q);
    }
    // target blocks right of this one: (node, columns, pivot block?) and their row pointers
    struct Tgt { int32_t node; int64_t c0, c1; bool piv; };
    std::vector<Tgt> right_all, right;
    for (size_t i : mine) {
      const RankLayout::Blk& T = Y.blocks[i];
      if (T.c0 >= oe) right_all.push_back({blknode[i], T.c0, T.c1, T.c0 < ns});
    }
    // this rank owns pivot block b+1 (look-ahead): block b+1 first, the rest deferred
    const bool ahead = kDistLookahead && b + 1 < np && P.blk_owner(t, b + 1) == rank;
    for (int pass = 0; pass < 2; ++pass) {
      if (!ahead && pass == 1) break;
      right.clear();
      for (const Tgt& T : right_all)
        if (!ahead || (pass == 0) == (T.c0 == P.blk_c0(t, b + 1))) right.push_back(T);
      if (right.empty()) continue;
      std::vector<Launch> saved;
      if (ahead && pass == 1) saved.swap(S.fac);   // emit the deferred part into `pending`
      auto trow = [&](const Tgt& T, int64_t row) {   // rows < ns of the target's first column
        const SNode& q = S.hsn[T.node];
        return T.piv ? kStore + q.Loff + T.c0 * M + row : kStore + q.Uoff + (T.c0 - ns) * ns + row;
      };
      for (int64_t u = 0; u < nsub; ++u) {
        const int64_t kbu = ob + 64 * u, wu = std::min<int64_t>(64, oe - kbu);
        std::vector<GemmRec> ctri, cand;
        double fl = 0;
        for (const Tgt& T : right) {
          const int64_t ldt = T.piv ? M : ns;
          const Operand Ti = own ? tinv_at(u, false) : kBlockBuf + ((M - ob) * w + u * 8192);
          ctri.push_back(gemm_task(Ti, trow(T, kbu), trow(T, kbu), wu, T.c1 - T.c0, wu, 64, ldt, ldt));
          update(cand, fl, Lsrc(kbu + wu, kbu), trow(T, kbu), trow(T, kbu + wu), oe - kbu - wu, T.c1 - T.c0, wu, ldL,
                 ldt, ldt);
        }
        add_gemm_launch(ctri, 0.0, (int)(kbu / 64), K_TRSML);
        add_gemm_launch(cand, fl, (int)(kbu / 64), K_GEMMU);
      }
      std::vector<GemmRec> cand;
      double fl = 0;
      for (const Tgt& T : right) {
        const int64_t nc = T.c1 - T.c0;
        if (T.piv) {
          update(cand, fl, Lsrc(oe, ob), trow(T, ob), trow(T, oe), M - oe, nc, w, ldL, M, M);
        } else {
          update(cand, fl, Lsrc(oe, ob), trow(T, ob), trow(T, oe), ns - oe, nc, w, ldL, ns, ns);
          update(cand, fl, Lsrc(ns, ob), trow(T, ob), kScratch + S.hsn[T.node].Foff + (T.c0 - ns) * nu, nu, nc, w, ldL,
                 ns, nu);
        }
      }
      add_gemm_launch(cand, fl, (int)(ob / 64), K_GEMMO);
      if (ahead && pass == 1) {
        pending.swap(S.fac);
        S.fac.swap(saved);
      }
    }
  }

  // ---- the per-level solve launches -------------------------------------------------------
  // small fronts by one workgroup each; large fronts (ns > kSolveBigNs) gather + one sync-free
  // sweep launch per direction (default) or one launch per 64-column block (SMLU_SOLVE_STEPS=1)
  void solve_level(int l) {
    std::vector<int64_t> tiny, small, bigs;
    for (int64_t k = LP[l]; k < LP[l + 1]; ++k) {
      int64_t s = LS[k];
      const SNode& r = S.hsn[s];
      const bool is_big = r.ns > kSolveBigNs || (int64_t)r.ns * ((int64_t)r.ns + r.nu) > kSolveBigWork;
      const bool tiny_front = (int64_t)r.ns + r.nu <= kSolveTinyM && r.ns <= 64;
      (is_big ? bigs : tiny_front ? tiny : small).push_back(s);
    }
    std::vector<Launch> bl;
    const size_t fwd0 = S.fwd.size();
    // tiny fronts: one wave per front; micro fronts (M <= 8) eight per wave for a single rhs
    for (int micro = 1; micro >= 0; --micro) {
      Launch L;
      L.kind = K_FWDT;
      L.aux = micro;
      L.off = (int64_t)S.ilist.size();
      for (auto s : tiny)
        if ((P.M(s) <= kSolveMicroM) == (micro == 1)) S.ilist.push_back((int32_t)s);
      L.cnt = (int64_t)S.ilist.size() - L.off;
      if (L.cnt == 0) continue;
      S.fwd.push_back(L);
      L.kind = K_BWDT;
      bl.push_back(L);
    }
    if (!small.empty()) {
      Launch L = launch(K_FWD, 0, S.ilist.size());
      for (auto s : small) S.ilist.push_back((int32_t)s);
      L.cnt = (int64_t)small.size();
      S.fwd.push_back(L);
      L.kind = K_BWD;
      bl.push_back(L);
    }
    if (!bigs.empty()) solve_big(bigs, bl);
    // one GPU: a level's small and tiny fronts are independent of its large fronts (disjoint x rows
    // and front vectors, children in lower levels): they run on the side stream next to the large
    // fronts' gather / sweep chain (solve.cpp)
    if (nranks == 1 && !bigs.empty() && !(tiny.empty() && small.empty())) {
      auto mark = [&](std::vector<Launch>& seq, size_t from) {
        for (size_t i = from; i < seq.size(); ++i) {
          Launch& X = seq[i];
          X.grp = l + 1;
          X.side = X.kind == K_FWDT || X.kind == K_FWD || X.kind == K_BWDT || X.kind == K_BWD;
        }
      };
      mark(S.fwd, fwd0);
      mark(bl, 0);
    }
    bwd_levels.push_back(bl);
  }
  // gather: one thread per front row pulls its own value and the children's contributions (in
  // child order) -- k_fwd_pull; pull lists per front row: gptr (CSR, relative to the front's
  // block) -> gent (vbuf index of each contribution)
  void solve_gather(const std::vector<int64_t>& bigs) {
    Launch L = launch(K_FWDP, 0, S.ft.size());
    int64_t wgp = 0;
    for (auto s : bigs) {
      const SNode& r = S.hsn[s];
      const int64_t M = (int64_t)r.ns + r.nu;
      S.ft.push_back(FrontTile{(int32_t)s, (int32_t)S.gptr.size(), wgp});
      wgp += (M + 255) / 256;
      std::vector<int32_t> cnt(M + 1, 0);
      for (int c = r.chbeg; c < r.chend; ++c) {
        const SNode& ch = S.hsn[P.ch_list[c]];
        const int32_t* rm = P.relmap.data() + ch.rowptr;
        for (int32_t k = 0; k < ch.nu; ++k) ++cnt[rm[k] + 1];
      }
      for (int64_t t = 0; t < M; ++t) cnt[t + 1] += cnt[t];
      const int64_t base = (int64_t)S.gent.size();
      for (int64_t t = 0; t <= M; ++t) S.gptr.push_back((int32_t)(base + cnt[t]));
      S.gent.resize(base + cnt[M]);
      for (int c = r.chbeg; c < r.chend; ++c) {
        const SNode& ch = S.hsn[P.ch_list[c]];
        const int32_t* rm = P.relmap.data() + ch.rowptr;
        for (int32_t k = 0; k < ch.nu; ++k) S.gent[base + cnt[rm[k]]++] = (int32_t)(ch.voff + ch.ns + k);
      }
      if ((int64_t)S.gptr.size() >= INT32_MAX || (int64_t)S.gent.size() >= INT32_MAX || r.voff + M >= INT32_MAX) {
        fail(kSchedErrAlloc, "solve gather lists exceed 32-bit indices");
        return;
      }
    }
    L.cnt = (int64_t)bigs.size();
    L.nwg = wgp;
    S.fwd.push_back(L);
  }
  void solve_big(const std::vector<int64_t>& bigs, std::vector<Launch>& bl) {
    solve_gather(bigs);
    if (!err.empty()) return;
    // backward: U12 product first
    Launch U = launch(K_BWDU, 0, S.ft.size());
    int64_t wg = 0;
    for (auto s : bigs) {
      S.ft.push_back(FrontTile{(int32_t)s, 0, wg});
      wg += (S.hsn[s].ns + 63) / 64;   // k_bwd_u12: 64 rows per workgroup
    }
    U.cnt = (int64_t)bigs.size();
    U.nwg = wg;
    bl.push_back(U);
    if (!in.tn.solve_steps) {   // one sync-free sweep launch per direction (k_tri_sweep)
      for (int upper = 0; upper < 2; ++upper) {
        Launch F = launch(upper ? K_SWEEPB : K_SWEEPF, 0, S.ft.size());
        F.aux = S.ssync_n;
        F.aux2 = S.ntick++;
        int64_t w = 0;
        int32_t fb = 0;
        for (auto s : bigs) {
          const SNode& r = S.hsn[s];
          const int64_t nbs = (r.ns + 63) / 64;
          S.ft.push_back(FrontTile{(int32_t)s, fb, w});
          w += upper ? (nbs + kSweepWK - 1) / kSweepWK
                     : ((int64_t)r.ns + r.nu + 64 * kSweepWK - 1) / (64 * kSweepWK);
          fb += (int32_t)nbs;
        }
        F.cnt = (int64_t)bigs.size();
        F.nwg = w;
        S.ssync_n += fb;
        (upper ? bl : S.fwd).push_back(F);
      }
      return;
    }
    int64_t nb = 0;
    for (auto s : bigs) nb = std::max<int64_t>(nb, (S.hsn[s].ns + 63) / 64);
    for (int64_t t = 0; t < nb; ++t)
      for (int upper = 0; upper < 2; ++upper) {
        Launch F = launch(upper ? K_TRIB : K_TRIF, (int)t, S.ft.size());
        int64_t w = 0, cnt = 0;
        for (auto s : bigs) {
          const SNode& r = S.hsn[s];
          const int64_t nbs = (r.ns + 63) / 64;
          if (t >= nbs) continue;
          S.ft.push_back(FrontTile{(int32_t)s, 0, w});
          w += tri_wg(upper, (int64_t)r.ns + r.nu, r.ns, (upper ? nbs - 1 - t : t) * 64);
          ++cnt;
        }
        F.cnt = cnt;
        F.nwg = w;
        (upper ? bl : S.fwd).push_back(F);
      }
  }
  // the 64-column block steps of one pivot block [ob, oe) of a shared front's node
  void tri_steps(bool upper, int32_t node, int64_t ob, int64_t oe, std::vector<Launch>& out) {
    const SNode& r = S.hsn[node];
    const int64_t M = (int64_t)r.ns + r.nu, nbs = (r.ns + 63) / 64;
    std::vector<int64_t> jbs;
    for (int64_t jb = ob; jb < oe; jb += 64) jbs.push_back(jb);
    if (upper) std::reverse(jbs.begin(), jbs.end());
    for (int64_t jb : jbs) {
      Launch F = launch(upper ? K_TRIB : K_TRIF, (int)(upper ? nbs - 1 - jb / 64 : jb / 64), S.ft.size());
      S.ft.push_back(FrontTile{node, 0, 0});
      F.cnt = 1;
      F.nwg = tri_wg(upper, M, r.ns, jb);
      out.push_back(F);
    }
  }
  // one vector segment of vbuf (doubles [off, off+cnt)) from rank a to rank b, in place
  void vhop(std::vector<Launch>& seq, std::vector<size_t>& seg, std::vector<int>& cm, int32_t a, int32_t b,
            int64_t off, int64_t cnt) {
    if (a == b || cnt <= 0 || (rank != a && rank != b)) return;
    CommOp op;
    const int pi = op.at(rank == a ? b : a);
    if (rank == a) { op.sbase[pi] = 2; op.soff[pi] = 8 * off; op.sbytes[pi] = 8 * cnt; }
    else { op.rbase[pi] = 2; op.roff[pi] = 8 * off; op.rbytes[pi] = 8 * cnt; }
    add_comm(seq, seg, cm, std::move(op));
  }

  // ---- the shared front's forward chain ---------------------------------------------------
  // the children's update vectors go to the first block's owner, which gathers the front vector;
  // the vector then follows the pivot blocks' owners
  void shared_forward(int32_t t) {
    const int64_t np = P.npblk(t), M = P.M(t);
    const int64_t tv = S.hsn[t].voff;
    const int32_t o0 = P.blk_owner(t, 0);
    {
      CommOp op;
      std::vector<std::vector<int64_t>> kids(nranks);
      for (int64_t e = P.ch_ptr[t]; e < P.ch_ptr[t + 1]; ++e) kids[holder(P.ch_list[e])].push_back(P.ch_list[e]);
      for (int32_t q = 0; q < nranks; ++q) {
        if (q == o0 || kids[q].empty()) continue;
        if (rank != q && rank != o0) continue;
        const int pi = op.at(rank == q ? o0 : q);
        int64_t acc = 0;
        for (int64_t c : kids[q]) {
          const int64_t off = 8 * (S.hsn[c].voff + P.ns(c)), nb8 = 8 * P.nu(c);
          if (rank == q) op.pack.push_back(HSeg{2, off, 4, acc, nb8});
          else op.unpack.push_back(HSeg{5, acc, 2, off, nb8});
          acc += nb8;
        }
        if (rank == q) op.sbytes[pi] = acc;
        else op.rbytes[pi] = acc;
      }
      // receive offsets: per peer contiguous in the receive staging
      int64_t racc = 0;
      for (size_t i = 0; i < op.peer.size(); ++i) {
        op.roff[i] = racc;
        racc += op.rbytes[i];
      }
      if (rank == o0) {   // unpack offsets were per peer from 0: shift by the peer's roff
        size_t k = 0;
        for (int32_t q = 0; q < nranks; ++q) {
          if (q == o0 || kids[q].empty()) continue;
          int64_t shift = 0;
          for (size_t i = 0; i < op.peer.size(); ++i)
            if (op.peer[i] == q) shift = op.roff[i];
          for (size_t j = 0; j < kids[q].size(); ++j) op.unpack[k++].so += shift;
        }
      }
      if (!op.peer.empty()) add_comm(S.fwd, S.fwd_seg, S.fwd_comm, std::move(op));
    }
    if (rank == o0) {
      Launch L = launch(K_FWDG, 0, S.ilist.size());
      S.ilist.push_back(t);
      L.cnt = 1;
      S.fwd.push_back(L);
    }
    for (int64_t b = 0; b < np; ++b) {
      const int32_t o = P.blk_owner(t, b);
      const int64_t ob = P.blk_c0(t, b), oe = P.blk_c1(t, b);
      if (rank == o) tri_steps(false, node_of(t, b), ob, oe, S.fwd);
      if (b + 1 < np) vhop(S.fwd, S.fwd_seg, S.fwd_comm, o, P.blk_owner(t, b + 1), tv + oe, M - oe);
    }
  }

  // ---- the backward chain -----------------------------------------------------------------
  // from the root level down; after each level holding a shared front (and at the end) every
  // rank shares the solution rows it computed since the previous exchange
  using Rows = std::vector<std::pair<int64_t, int64_t>>;   // x rows (first, count)
  void backward() {
    std::vector<Rows> pending_rows(nranks);   // per rank, since the last exchange
    Rows myrows;
    for (int l = P.nlevels - 1; l >= 0; --l) {
      for (auto& L : bwd_levels[l]) S.bwd.push_back(L);
      if (nranks == 1) continue;
      // rows every rank computes at this level (global enumeration)
      for (int64_t k = P.lev_ptr[l]; k < P.lev_ptr[l + 1]; ++k) {
        const int64_t s = P.lev_sup[k];
        if (!P.dist(s)) {
          pending_rows[P.owner[s]].push_back({P.s_first[s], P.ns(s)});
          continue;
        }
        for (int64_t b = 0; b < P.npblk(s); ++b)
          pending_rows[P.blk_owner(s, b)].push_back({P.s_first[s] + P.blk_c0(s, b), P.blk_c1(s, b) - P.blk_c0(s, b)});
      }
      for (const int32_t t : dfront[l]) shared_backward(t);
      for (auto& rg : pending_rows[rank]) myrows.push_back(rg);
      pending_rows[rank].clear();
      if (dlevel[l] || l == 0) xbwd(pending_rows, myrows);
    }
  }
  void xbwd(std::vector<Rows>& pending_rows, Rows& myrows) {
    CommOp op;
    int64_t mine = 0;
    for (auto& rg : myrows) {
      op.pack.push_back(HSeg{3, 8 * rg.first, 4, 8 * mine, 8 * rg.second});
      mine += rg.second;
    }
    // every peer's rows, in its own order (the same enumeration on every rank)
    std::vector<Rows> theirs(nranks);
    theirs.swap(pending_rows);
    int64_t racc = 0;
    for (int32_t q = 0; q < nranks; ++q) {
      if (q == rank) continue;
      const int pi = op.at(q);
      op.soff[pi] = 0;
      op.sbytes[pi] = 8 * mine;
      op.roff[pi] = racc;
      int64_t cnt = 0;
      for (auto& rg : theirs[q]) {
        op.unpack.push_back(HSeg{5, racc + 8 * cnt, 3, 8 * rg.first, 8 * rg.second});
        cnt += rg.second;
      }
      op.rbytes[pi] = 8 * cnt;
      racc += 8 * cnt;
    }
    myrows.clear();
    add_comm(S.bwd, S.bwd_seg, S.bwd_comm, std::move(op));
  }
  void shared_backward(int32_t t) {
    const int64_t np = P.npblk(t), nbk = np + P.nublk(t), ns = P.ns(t);
    const int64_t tv = S.hsn[t].voff;
    // the forward solve left y of each pivot block in x on the block's owner: the rank that
    // starts the backward chain collects all of them first
    const int32_t cs = nbk > np ? P.blk_owner(t, np) : P.blk_owner(t, np - 1);
    {
      CommOp op;
      const int64_t f0 = P.s_first[t];
      for (int32_t q = 0; q < nranks; ++q) {
        if (q == cs || (rank != q && rank != cs)) continue;
        int64_t acc = 0;
        std::vector<HSeg> segs;
        for (int64_t b = 0; b < np; ++b) {
          if (P.blk_owner(t, b) != q) continue;
          const int64_t o8 = 8 * (f0 + P.blk_c0(t, b)), nb8 = 8 * (P.blk_c1(t, b) - P.blk_c0(t, b));
          segs.push_back(rank == q ? HSeg{3, o8, 4, acc, nb8} : HSeg{5, acc, 3, o8, nb8});
          acc += nb8;
        }
        if (acc == 0) continue;
        const int pi = op.at(rank == q ? cs : q);
        if (rank == q) {
          op.sbytes[pi] = acc;
          for (auto& g : segs) op.pack.push_back(g);
        } else {
          op.rbytes[pi] = acc;
          for (auto& g : segs) op.unpack.push_back(g);
        }
      }
      if (rank == cs) {   // receive offsets per peer, shift the unpack copies
        int64_t racc = 0;
        size_t k = 0;
        for (size_t i = 0; i < op.peer.size(); ++i) {
          op.roff[i] = racc;
          int64_t left = op.rbytes[i];
          while (left > 0 && k < op.unpack.size()) {
            op.unpack[k].so += racc;
            left -= op.unpack[k].bytes;
            ++k;
          }
          racc += op.rbytes[i];
        }
      }
      if (!op.peer.empty()) add_comm(S.bwd, S.bwd_seg, S.bwd_comm, std::move(op));
    }
    int32_t prev = -1;
    bool first = true;
    for (int64_t ub = np; ub < nbk; ++ub) {   // U12 contributions, block by block
      const int32_t o = P.blk_owner(t, ub);
      if (prev >= 0) vhop(S.bwd, S.bwd_seg, S.bwd_comm, prev, o, tv, ns);
      if (rank == o) {
        Launch L;
        L.kind = K_BWDU12C;
        L.node = node_of(t, ub);
        L.aux = P.blk_c0(t, ub);
        L.aux2 = P.blk_c1(t, ub);
        L.cnt = first ? 1 : 0;
        S.bwd.push_back(L);
      }
      prev = o;
      first = false;
    }
    if (first) {   // no update columns: the chain starts from the solution rows of the front
      prev = P.blk_owner(t, np - 1);
      if (rank == prev) {
        Launch L;
        L.kind = K_VCOPY;
        L.node = t;
        S.bwd.push_back(L);
      }
    }
    for (int64_t b = np - 1; b >= 0; --b) {
      const int32_t o = P.blk_owner(t, b);
      const int64_t ob = P.blk_c0(t, b), oe = P.blk_c1(t, b);
      vhop(S.bwd, S.bwd_seg, S.bwd_comm, prev, o, tv, oe);
      if (rank == o) tri_steps(true, node_of(t, b), ob, oe, S.bwd);
      prev = o;
    }
  }

  // ---- the per-block expansion fwdm / bwdm ------------------------------------------------
  // batched right-hand sides (one GPU): the sweep's single chain wave per block would run the NR
  // chains one after another, so batches keep the per-64-column-block launches (k_tri_block: the
  // diagonal block solved by four chain waves for four right-hand sides at a time).  The same
  // per-block sequences (with the comm segments of fwd / bwd) re-run a solve whose sweep timed out.
  void expand(const Launch& Sw, bool upper, std::vector<Launch>& out) {
    std::vector<int32_t> fr;
    for (int64_t i = Sw.off; i < Sw.off + Sw.cnt; ++i) fr.push_back(S.ft[i].s);
    int64_t nb = 0;
    for (auto s : fr) nb = std::max<int64_t>(nb, (S.hsn[s].ns + 63) / 64);
    for (int64_t t = 0; t < nb; ++t) {
      Launch F;
      F.kind = upper ? K_TRIB : K_TRIF;
      F.grp = Sw.grp;
      F.step = (int)t;
      F.off = (int64_t)S.ft.size();
      int64_t w = 0, cnt = 0;
      for (auto s : fr) {
        const SNode& r = S.hsn[s];
        const int64_t nbs = (r.ns + 63) / 64;
        if (t >= nbs) continue;
        S.ft.push_back(FrontTile{s, 0, w});
        w += tri_wg(upper, (int64_t)r.ns + r.nu, r.ns, (upper ? nbs - 1 - t : t) * 64);
        ++cnt;
      }
      F.cnt = cnt;
      F.nwg = w;
      out.push_back(F);
    }
  }
  void expand_all(const std::vector<Launch>& seq, const std::vector<size_t>& seg, bool upper,
                  std::vector<Launch>& out, std::vector<size_t>& oseg) {
    std::vector<size_t> at(seq.size() + 1);
    for (size_t i = 0; i < seq.size(); ++i) {
      at[i] = out.size();
      if (seq[i].kind == (upper ? K_SWEEPB : K_SWEEPF)) expand(seq[i], upper, out);
      else out.push_back(seq[i]);
    }
    at[seq.size()] = out.size();
    oseg.clear();
    for (size_t k : seg) oseg.push_back(at[std::min(k, seq.size())]);
  }

  std::string run() {
    S = Schedule();
    S.ob = in.tn.ob > 0 ? in.tn.ob : in.ob;
    S.t128_min = in.tn.t128_min;
    S.small_k = in.tn.small_k;
    // GEMM-form TRSM (k_tri_inv + GEMM tasks) needs the growth epilogue of the MFMA/64 tiles
    // (the 32-wide panels keep k_step_trsm: measured best)
    S.trsm_gemm = in.use_mfma;
    S.trail_span = in.tn.trail_span;
    nodes();
    group_entries();
    levels();
    f22g.assign(P.nsup, 0);
    for (int l = 0; l < P.nlevels && err.empty(); ++l) {
      cur_level = l;
      choose_f22_gather(l);
      assembly(l, f22_exchange(l));
      small_fronts(l);
      if (err.empty()) blocked_fronts(l);
      if (!err.empty()) break;
      for (const int32_t t : dfront[l]) shared_front(t);   // in front order on every rank
      lvl_end.push_back(S.fac.size());
    }
    if (err.empty()) lside_check();
    if (err.empty()) trail_check();
    for (int l = 0; l < P.nlevels && err.empty(); ++l) {
      solve_level(l);
      for (const int32_t t : dfront[l]) shared_forward(t);
    }
    if (!err.empty()) return err;
    backward();
    S.nlaunch = (int64_t)S.fac.size();
    expand_all(S.fwd, S.fwd_seg, false, S.fwdm, S.fwdm_seg);
    expand_all(S.bwd, S.bwd_seg, true, S.bwdm, S.bwdm_seg);
    if (nranks > 1) S.max_list = std::max<int64_t>(S.max_list, dist_slots);
    return err;
  }
};

}  // namespace

std::string build_schedule(const ScheduleInput& in, Schedule& out) { return Builder(in, out).run(); }

void rank_layout_of(const Plan& P, int rank, int nranks, RankLayout& Y) {
  if (nranks > 1) {
    rank_layout(P, rank, Y);
    return;
  }
  Y = RankLayout();
  Y.Loff = P.Loff;
  Y.Uoff = P.Uoff;
  Y.Foff = P.Foff;
  Y.recv_off.assign(P.nsup, -1);
  Y.recv_size.assign(P.nsup, 0);
  Y.store_size = P.factor_size;
  Y.scratch_size = P.scratch_size;
}

}  // namespace smlu
