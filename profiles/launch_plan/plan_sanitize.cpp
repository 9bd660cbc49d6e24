// plan_solve (csrc/mpmpc_launch_plan.hpp) over its argument space in a stand-alone host program, for a sanitizer build:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Wno-unknown-pragmas -Iinclude \
//       -Imulti-purpose-mpc_amd/csrc profiles/launch_plan/plan_sanitize.cpp -o /tmp/plan_sanitize && /tmp/plan_sanitize
// Horizons 3 .. 255, every packing mpmpc_set_packing accepts there, both launch kinds, the closed loop, tail kernel 0 / 1 / 2,
// warm start 0 / 1 / 2, seven batch sizes, the reference's weights and a terminal cost on t.  Prints the number of plans.
#include <cstdio>
#include <initializer_list>
#include <cstring>
#include <limits>
#include "mpmpc_launch_plan.hpp"
using namespace mpmpc;
int main() {
  mpmpc_config c{}; mpmpc_settings st{};
  st.reduce = 1; st.polish = 2; st.native = 1; st.early_polish = 1; st.max_iter = 4000; st.ipm_start_mu = 0.01; st.early_scaling = 1; st.scaling = 10; st.phase1 = 1;
  const double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < 3; ++i) { c.xmin[i] = -inf; c.xmax[i] = inf; }
  c.Q[0] = 1; c.R[0] = 0.5; c.QN[0] = 1;
  long n = 0, stages = 0;
  for (int tt = 0; tt < 2; ++tt) {
    c.QN[2] = tt;
    for (int N = 3; N <= 255; ++N) for (int g : {0, 16, 32, 64, 128, 256}) {
      if (!packing_valid(N, g)) continue;
      c.N = N;
      for (int B : {1, 16, 17, 129, 1025, 2049, 65536}) for (int cl = 0; cl < 2; ++cl) for (int kind = 0; kind < 2; ++kind) for (int lean = 0; lean < 3; ++lean)
        for (int warm = 0; warm < 3; ++warm) {
          SolvePlan p = plan_solve(c, st, LaunchKnobs{g, lean != 0, lean == 2, 3, warm}, B, cl, (LaunchKind)kind);
          if (p.n < 1 || p.n > 3) { std::printf("bad n\n"); return 1; }
          for (int i = 0; i < p.n; ++i) if (p.stage[i].grid < 1 || p.stage[i].reads > 3 || p.stage[i].fills > 3) { std::printf("bad stage\n"); return 1; }
          ++n; stages += p.n;
        }
    }
  }
  std::printf("%ld plans, %ld stages\n", n, stages);
}
