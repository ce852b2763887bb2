// Host AddressSanitizer / UBSan driver of the schedule builder with the L rows below an outer
// block on the side stream (SMLU_LSIDE_MIN; csrc/schedule_build.cpp step_solves, lside_check):
// 3D Poisson 24^3 (root 576 = 384 + 192) on one GPU with the threshold forced to 64, at the
// default outer block and at OB = 128, against the same builds with the knob off.  Built and run
// next to host_asan.cpp (tools/sanitize/Makefile); no device code.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sharedmemsparselu.jl_amd/csrc/plan.hpp"
#include "../../sharedmemsparselu.jl_amd/csrc/schedule.hpp"

using namespace smlu;

static int check(bool ok, const char* what) {
  if (!ok) std::fprintf(stderr, "FAIL: %s\n", what);
  return ok ? 0 : 1;
}

int main() {
  const int64_t m = 24, n = m * m * m;
  std::vector<int64_t> cp{0}, ri;
  for (int64_t k = 0; k < m; ++k)
    for (int64_t j = 0; j < m; ++j)
      for (int64_t i = 0; i < m; ++i) {   // column i + m (j + m k): rows ascending
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
  int bad = 0;
  RankLayout L;
  rank_layout_of(P, 0, 1, L);
  for (int ob : {0, 128}) {
    Schedule S[2];
    for (int on = 0; on < 2; ++on) {
      ScheduleInput in;
      in.plan = &P;
      in.lay = &L;
      in.dominant = true;
      in.tn.ob = ob;
      in.tn.lside_min = on ? 64 : 0;
      const std::string se = build_schedule(in, S[on]);
      if (!se.empty()) std::fprintf(stderr, "schedule: %s\n", se.c_str());
      bad += check(se.empty(), "schedule builds (the builder's side-launch checks pass)");
    }
    int64_t side = 0, tasks = 0;
    for (const Launch& q : S[1].fac) {
      if (!q.side) continue;
      ++side;
      tasks += q.cnt;
      bad += check((q.kind == K_TRSML || q.kind == K_GEMM) && q.off >= 0 && q.cnt > 0 &&
                       q.off + q.cnt <= (int64_t)S[1].gt.size(),
                   "side launch kind and task range");
    }
    bad += check(side > 0 && side == S[1].side_launches && S[1].side_rows > 0, "side launches scheduled and counted");
    bad += check(S[0].side_launches == 0 && S[0].side_rows == 0, "knob off: no side launch");
    bad += check(S[1].fac.size() > S[0].fac.size() && S[1].fac.size() <= S[0].fac.size() + (size_t)side &&
                     S[1].gt.size() <= S[0].gt.size() + (size_t)tasks,
                 "no launch or task beyond the side ones is added");
    std::printf("lside poisson3d_24 ob=%d side_launches=%lld side_rows=%lld ok=%d\n", ob, (long long)side,
                (long long)S[1].side_rows, bad == 0);
  }
  std::printf(bad == 0 ? "LSIDE SANITIZER RUN OK\n" : "LSIDE SANITIZER RUN FAILED\n");
  return bad == 0 ? 0 : 1;
}
