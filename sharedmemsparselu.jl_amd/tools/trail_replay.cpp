// Host replay of the outer trailing updates (K_GEMMO) of a 3D Poisson plan under SMLU_TRAIL_SPAN /
// SMLU_TRAIL_NS (csrc/schedule_build.cpp, outer_block_end): builds the one-GPU schedule for each
// setting and prints, per setting and k class, the launches, tasks, 128x128 tiles, rounds of 512
// resident workgroups and a modelled time.  No device code; built with the host compiler
// (make tools/trail_replay).
//
// Model: a launch on the 128 tile is list-scheduled in task order onto 512 slots (two workgroups
// on each of 256 CUs), a tile of depth k holding its slot for a + b k.  a and b come from two
// tools/gemm_bench lines, both whole rounds of equal tiles: 16000^2 x 384 at 62.4 TF (31 rounds in
// 3.150 ms) and 12000^2 x 6000 at 70.89 TF (18 rounds in 24.38 ms): a = 16.0 us, b = 0.2230 us per
// k.  Launches under the 128-tile threshold run the 64 tile, taken flat at 22 TF (its rate on
// k = 384 strips and squares).  The model knows nothing of clocks, L2 or the side stream; it ranks
// settings and bounds the gain, the A/B decides.
//
// Usage: trail_replay [N=128] [trail_ns=1024]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <queue>
#include <string>
#include <vector>

#include "../csrc/plan.hpp"
#include "../csrc/schedule.hpp"

using namespace smlu;

namespace {
constexpr double kA = 16.0e-6, kB = 0.2230e-6, kSlots = 512, kTf64 = 22e12;

struct Row {
  int64_t launches = 0, tasks = 0, tiles = 0;
  double rounds = 0, flops = 0, sec = 0;
};

double launch_time(const Schedule& S, const Launch& L, int64_t* tiles_out) {
  std::priority_queue<double, std::vector<double>, std::greater<double>> slot;
  int64_t tiles = 0;
  double end = 0;
  for (int64_t i = L.off; i < L.off + L.cnt; ++i) {
    const GemmRec& g = S.gt[i];
    const int64_t nt = (int64_t)((g.m + 127) / 128) * ((g.n + 127) / 128);
    const double c = kA + kB * g.k;
    for (int64_t t = 0; t < nt; ++t) {
      double at = 0;
      if ((int64_t)slot.size() >= (int64_t)kSlots) {
        at = slot.top();
        slot.pop();
      }
      slot.push(at + c);
      end = std::max(end, at + c);
    }
    tiles += nt;
  }
  *tiles_out = tiles;
  return end;
}
}  // namespace

int main(int argc, char** argv) {
  const int64_t m = argc > 1 ? std::atoll(argv[1]) : 128, n = m * m * m;
  const int64_t trail_ns = argc > 2 ? std::atoll(argv[2]) : 1024;
  std::vector<int64_t> cp{0}, ri;
  for (int64_t k = 0; k < m; ++k)
    for (int64_t j = 0; j < m; ++j)
      for (int64_t i = 0; i < m; ++i) {
        if (k > 0) ri.push_back(i + m * (j + m * (k - 1)));
        if (j > 0) ri.push_back(i + m * (j - 1 + m * k));
        if (i > 0) ri.push_back(i - 1 + m * (j + m * k));
        ri.push_back(i + m * (j + m * k));
        if (i + 1 < m) ri.push_back(i + 1 + m * (j + m * k));
        if (j + 1 < m) ri.push_back(i + m * (j + 1 + m * k));
        if (k + 1 < m) ri.push_back(i + m * (j + m * (k + 1)));
        cp.push_back((int64_t)ri.size());
      }
  Plan P;
  PlanOptions o;
  const std::string e = P.build(n, cp.data(), ri.data(), 0, o, nullptr, nullptr, nullptr);
  if (!e.empty()) {
    std::fprintf(stderr, "plan failed: %s\n", e.c_str());
    return 1;
  }
  RankLayout Y;
  rank_layout_of(P, 0, 1, Y);
  std::printf("poisson3d_%lld, SMLU_TRAIL_NS=%lld: K_GEMMO launches by longest k; model a=%.1f us b=%.4f us/k\n",
              (long long)m, (long long)trail_ns, kA * 1e6, kB * 1e6);
  double base = 0;
  for (int span : {1, 2, 4, 8, 0}) {
    ScheduleInput in;
    in.plan = &P;
    in.lay = &Y;
    in.dominant = true;
    in.tn = tune();
    in.tn.trail_span = span;
    in.tn.trail_ns = trail_ns;
    if (in.tn.ob > 0) in.ob = in.tn.ob;
    Schedule S;
    const std::string se = build_schedule(in, S);
    if (!se.empty()) {
      std::fprintf(stderr, "span %d: schedule failed: %s\n", span, se.c_str());
      return 1;
    }
    std::map<int64_t, Row> by_k;   // 0: launches on the 64 tile
    Row all;
    for (const Launch& L : S.fac) {
      if (L.kind != K_GEMMO) continue;
      int64_t kmax = 0, tiles = 0;
      for (int64_t i = L.off; i < L.off + L.cnt; ++i) kmax = std::max<int64_t>(kmax, S.gt[i].k);
      double sec = launch_time(S, L, &tiles);
      const bool t128 = L.aux >= 128;
      if (!t128) sec = L.flops / kTf64;
      for (Row* r : {&by_k[t128 ? kmax : 0], &all}) {
        ++r->launches;
        r->tasks += L.cnt;
        r->tiles += tiles;
        r->rounds += t128 ? (double)tiles / kSlots : 0;
        r->flops += L.flops;
        r->sec += sec;
      }
    }
    if (span == 1) base = all.sec;
    std::printf("span %d: trail_fronts %lld gemmo_kmax %lld gemm_bytes %.1f GB\n", span, (long long)S.trail_fronts,
                (long long)S.gemmo_kmax, S.gemm_bytes * 1e-9);
    std::printf("  %8s %8s %6s %9s %8s %9s %9s %7s\n", "kmax", "launches", "tasks", "tiles128", "rounds", "TFLOP",
                "model ms", "TF/s");
    for (const auto& kv : by_k) {
      const Row& r = kv.second;
      std::printf("  %8s %8lld %6lld %9lld %8.1f %9.3f %9.2f %7.1f\n",
                  kv.first ? std::to_string(kv.first).c_str() : "64-tile", (long long)r.launches, (long long)r.tasks,
                  (long long)r.tiles, r.rounds, r.flops * 1e-12, r.sec * 1e3, r.flops / r.sec * 1e-12);
    }
    std::printf("  %8s %8lld %6lld %9lld %8.1f %9.3f %9.2f %7.1f   vs span 1: %+.2f ms\n", "all", (long long)all.launches,
                (long long)all.tasks, (long long)all.tiles, all.rounds, all.flops * 1e-12, all.sec * 1e3,
                all.flops / all.sec * 1e-12, (all.sec - base) * 1e3);
  }
  return 0;
}
