// Which solve kernels a launch runs: the decision, as a pure function of (configuration, settings, knobs of the handle, batch
// size, how the launch was asked for).  Host code only - no HIP, no handle, no globals, no heap: the launcher (mpmpc_hip.hip)
// calls plan_solve and enqueues what it says, mpmpc_launch_plan (include/mpmpc.h) writes the same plan out for the tests.
// Every packing returns the same bits, so a wrong choice here is silent on the device - merely slower; tests/test_launch_plan.py
// pins the policy on the CPU.
//
// A plan is at most three stages in stream order.  A stage names its kernel family and instantiation, its grid and block, and
// the tail lists it works on by ROLE (MPMPC_LIST_*): which pointers those are is the executor's business, and so is whether a
// stage that MAY be deferred is (that depends on what the host has seen of earlier launches, not on the arguments).
#pragma once
#include "mpmpc_core.hpp"
#include "mpmpc_reduced.hpp"
#include "mpmpc_reduced_t.hpp"
#include "mpmpc_reduced_tail.hpp"

namespace mpmpc {

// how a solve launch was asked for: waited for on its own, or one of several in flight (resident launches, begun staged calls)
enum LaunchKind { LAUNCH_SINGLE = 0, LAUNCH_PIPELINED = 1 };

// what the policy reads of the handle
struct LaunchKnobs {
  int force_lanes;                       // mpmpc_set_packing
  bool lean_tail, lean_tail_single;      // mpmpc_set_tail_kernel 1 / 2
  int pipeline;                          // launch slots in use (mpmpc_set_pipeline)
  int ro_warm;                           // mpmpc_rollout_warm_start
};

// one row of mpmpc_launch_plan: MPMPC_PLAN_ROW int32 fields, in this order
struct PlanStage {
  int32_t family;          // MPMPC_K_*
  int32_t G, C;            // template arguments of the instantiation: lanes per instance, chain split (0: the family has none)
  int32_t var, warm;       // ... VAR of the general kernels, WARM
  int32_t mode;            // general kernels: 0 the whole solve, 2 the full run on the instances of a list
  int32_t grid, block;
  int32_t reads, fills;    // MPMPC_LIST_*: the list whose instances it takes / the list it appends what it leaves to
  int32_t clear;           // the list it fills is emptied on the stream in front of it (no kernel of the sequence does it)
  int32_t deferrable;      // need not be enqueued while the list it reads is expected to stay empty
  int32_t turn;            // first stage of a reduced-native launch at N + 1 <= 64: the launch takes the slot's next flip list
                           // and a new sequence number (the kernel stamps it into tail_flag if it leaves a tail)
};
static_assert(sizeof(PlanStage) == MPMPC_PLAN_ROW * sizeof(int32_t), "PlanStage is the row of mpmpc_launch_plan");

struct SolvePlan {
  int n;
  PlanStage stage[MPMPC_PLAN_MAX_STAGES];
};

// mpmpc_set_packing's rule: may a handle of horizon N hold `g` lanes per instance?  16 / 32 / 64 must hold the N + 1 stages -
// or half of them where the two-stages-per-lane kernels exist (16 at 17 .. 32 stages, 64 at 65 .. 128); 128 / 256 name the
// workgroup kernels of the long horizons.
inline bool packing_valid(int N, int g) {
  const int stages = N + 1;
  if (g == 0) return true;
  if (g != 16 && g != 32 && g != 64 && !(g == 128 && stages > 64) && !(g == 256 && stages > 128)) return false;
  const bool two = (g == 16 && stages > 16 && stages <= 32) || ((g == 64 || g == 128) && stages > 64 && stages <= 128) ||
                   ((g == 128 || g == 256) && stages > 128);
  return stages <= g || two;
}

inline PlanStage plan_stage(int family, int G, int C, int grid, int block, int reads, int fills) {
  PlanStage s{};
  s.family = family; s.G = G; s.C = C; s.grid = grid; s.block = block; s.reads = reads; s.fills = fills;
  return s;
}

inline SolvePlan plan_solve(const mpmpc_config& cfg, const mpmpc_settings& st, const LaunchKnobs& knobs, int B, bool closed_loop,
                            LaunchKind kind) {
  SolvePlan p{};
  auto add = [&p](const PlanStage& s) -> PlanStage& { return p.stage[p.n++] = s; };
  const int N = cfg.N;
  // Full weights (Q, R or QN with off-diagonal entries), bounds on e_psi / t or a cost on t rule the reduction out:
  // such configurations run the general kernels, one instance per wave (or workgroup).
  const bool fullqn = full_weights(cfg);
  const bool red = reducible(cfg, st);      // the polish may work on the (e_y, e_psi, kappa) problem
  // The reduced-native kernels (mpmpc_reduced.hpp) take the batch path of every configuration they apply to - cold and
  // warm-started - and only they pack several instances into a wave; the general kernel then sees their tail.
  const bool rnt = reduced_native_tt(cfg, st);      // ... or their twin for a terminal cost on the time state
  // The tail of a batch launch goes to the reduced-native tail solver first (two waves per SIMD instead of one).
  const bool lean = knobs.lean_tail && reduced_native_tail(cfg, st);

  if (N + 1 > 64) {
    // Horizons above 63.  65 .. 128 stages of the reference's own weights (or of a terminal cost on the time state): TWO stages
    // per lane, the whole instance in ONE wavefront (K2r2<64> / K2t2<64>), its tail to K2p2<64>; 129 .. 256 stages: the same on
    // a workgroup of two wavefronts (K2rb2); what they leave goes to the general solver on a workgroup.  mpmpc_set_packing(h,
    // 128 / 256) keeps the one-stage workgroup kernel K2rb in front instead.  Everything else - full weights, bounded
    // e_psi / t - the general workgroup kernel alone, over every instance.  No packing, no deferred tail, cold starts in the
    // closed loop too; the lists are not the flip lists of the short horizons: the first is emptied on the stream.
    const int W = N + 1 <= 128 ? 128 : 256;          // lanes of the workgroup kernels
    const bool pairs = knobs.force_lanes != W;
    int list = MPMPC_LIST_NONE;                      // what the general workgroup kernel works on (none: the whole solve)
    if (!fullqn && reduced_native(cfg, st)) {
      list = MPMPC_LIST_THIS;
      if (!pairs) add(plan_stage(MPMPC_K_RBLOCK, W, 0, B, W, MPMPC_LIST_NONE, MPMPC_LIST_THIS));
      else if (W == 128) add(plan_stage(MPMPC_K_PAIR, 64, 0, B, 64, MPMPC_LIST_NONE, MPMPC_LIST_THIS));
      else add(plan_stage(MPMPC_K_PAIR_BLOCK, 128, 0, B, 128, MPMPC_LIST_NONE, MPMPC_LIST_THIS));
      if (pairs && lean) {
        // (K2r2<64> empties the lists behind the one it fills, as for "the next launch"; the workgroup form does not)
        add(plan_stage(W == 128 ? MPMPC_K_PAIR_TAIL : MPMPC_K_PAIR_BLOCK_TAIL, W == 128 ? 64 : 128, 0, B, W == 128 ? 64 : 128,
                       MPMPC_LIST_THIS, MPMPC_LIST_NEXT)).clear = W != 128;
        list = MPMPC_LIST_NEXT;
      }
    } else if (!fullqn && rnt && pairs) {
      add(plan_stage(W == 128 ? MPMPC_K_PAIR_T : MPMPC_K_PAIR_BLOCK_T, W == 128 ? 64 : 128, 0, B, W == 128 ? 64 : 128,
                     MPMPC_LIST_NONE, MPMPC_LIST_THIS));
      list = MPMPC_LIST_THIS;
    }
    if (p.n) p.stage[0].clear = 1;
    PlanStage& g = add(plan_stage(MPMPC_K_BLOCK, W, 0, B, W, list, MPMPC_LIST_NONE));
    g.var = fullqn ? 1 : (red ? 2 : 0);
    g.mode = list != MPMPC_LIST_NONE ? 2 : 0;
    return p;
  }

  const bool rn = rnt || reduced_native(cfg, st);
  const int var = fullqn ? 1 : (red ? 2 : (free_states(cfg) ? 3 : 0));
  // lanes per instance: one instance per wave while there are no more instances than SIMDs (1024); beyond that the
  // smallest power of two holding N + 1 stages, so that a wave carries 2 or 4 instances and a SIMD two such waves
  int G = 64;
  bool two = false;
  if (rn && !rnt) {      // (the terminal-time kernels run one instance per wave)
    // A launch that is one of several in flight - a pipelined resident launch (mpmpc_solve_resident with mpmpc_set_pipeline > 1:
    // the default) or the begun half of a split host-buffer call (mpmpc_staged_begin: the caller keeps several handles busy) -
    // is after throughput, and a packed wave does two or four instances for about the instructions of one: such launches pack
    // from 128 instances on - the launches in flight fill the chip, not the waves of one launch (B = 1 024, four launches in
    // flight: 36.5 M solves/s with one instance per wave, measured 41.4 M with two launches of the packed kernel, DESIGN.md
    // section 4).  A launch that is waited for on its own - mpmpc_solve, mpmpc_solve_staged, the timed launch, a handle held at
    // one launch in flight - and the closed loop (one launch per step, each waiting for the one before) keep one instance per
    // wave up to the chip's 1 024 SIMDs: the latency of a single launch is 43 us against 52 (the decision used to
    // follow the handle's pipeline depth alone, so single calls paid the packed kernel's latency).  The choice depends on the
    // entry point, the handle's settings and the batch size only: a given call gives the same bits every time - and every
    // packing returns the same bits anyway (tests).
    const bool throughput = kind == LAUNCH_PIPELINED && knobs.pipeline > 1 && !closed_loop;
    if (N + 1 <= 32 && B > (throughput ? 128 : 1024)) G = 32;
    if (N + 1 <= 16 && B > (throughput ? 256 : 2048)) G = 16;
    if (knobs.force_lanes && N + 1 <= knobs.force_lanes) G = knobs.force_lanes;      // mpmpc_set_packing
    // TWO stages per lane (K2r2<16>): 17 .. 32 stages in 16 lanes, four instances per wavefront; cold starts only.  Measured
    // slower than <32,16> at two waves per SIMD: never the automatic choice.
    if (knobs.force_lanes == 16 && N + 1 > 16 && N + 1 <= 32 && !closed_loop) { G = 16; two = true; }
  }
  // closed loop: the previous step's active sets as a first guess.  A launch with one instance per wave ends with
  // its slowest car, and with more than a handful of cars one of them always misses its guess (hit rate 91-93 %
  // per car and step: the miss pays for the attempt AND the normal path, 1024 cars -7 %), so "auto" warm-starts the
  // packed launches (x1.5 at 8192 cars) and the very small fleets (x1.7 at 8 cars) only.
  const bool warm = closed_loop && !rnt && (knobs.ro_warm == 1 || (knobs.ro_warm == 2 && (G < 64 || B <= 16)));
  const int per = two ? 4 : 64 / G;
  const int grid = (B + per - 1) / per;
  const int C = lane_split(G, N);        // where the two elimination chains of the factorisation meet
  const int C64 = lane_split(64, N);     // ... of the one-instance-per-wave kernels that take a tail
  if (!rn) {
    // the general kernel, one instance per wave, the whole solve
    PlanStage& g = add(plan_stage(MPMPC_K_GENERAL, 64, C, grid, 64, MPMPC_LIST_NONE, MPMPC_LIST_NONE));
    g.var = var; g.warm = warm;
    return p;
  }
  PlanStage& first = add(rnt   ? plan_stage(MPMPC_K_REDUCED_T, 64, C, grid, 64, MPMPC_LIST_NONE, MPMPC_LIST_THIS)
                         : two ? plan_stage(MPMPC_K_PAIR, 16, 0, grid, 64, MPMPC_LIST_NONE, MPMPC_LIST_THIS)
                               : plan_stage(MPMPC_K_REDUCED, G, C, grid, 64, MPMPC_LIST_NONE, MPMPC_LIST_THIS));
  first.warm = warm;
  first.turn = 1;
  // The tail is short (infeasible / very hard instances).  One block per instance of the batch: blocks beyond the
  // list's length return at once (an all-empty launch takes 4.8 us at 1 024 blocks, 15 us at 65 536: rocprofv3 kernel
  // trace - which is why it may be deferred; a grid-stride loop over the list around the solver costs the general kernels
  // 70 registers and puts 148-544 B of scratch into kernels that have none: measured on the code object, not kept).  Its
  // instances carry no guess for the next closed-loop step (act stays 0 from the first launch).  The closed loop consumes
  // the results on the device and always launches the tail - the general kernel on all of it: its step would pay for a
  // third launch every time.
  int list = MPMPC_LIST_THIS;
  if (lean && !rnt && !closed_loop) {
    // (the list's order differs from run to run - atomic appends - and with it the two instances that share a wave of the
    //  packed form: the solver's arithmetic does not depend on the partner, Solver::active_set)
    add(C64 == 32                ? plan_stage(MPMPC_K_REDUCED_TAIL, 64, 32, B, 64, MPMPC_LIST_THIS, MPMPC_LIST_LEFT)      // horizons 32 .. 63
        : knobs.lean_tail_single ? plan_stage(MPMPC_K_REDUCED_TAIL, 64, 16, B, 64, MPMPC_LIST_THIS, MPMPC_LIST_LEFT)
                                 : plan_stage(MPMPC_K_REDUCED_TAIL, 32, 16, (B + 1) / 2, 64, MPMPC_LIST_THIS, MPMPC_LIST_LEFT))
        .deferrable = 1;
    list = MPMPC_LIST_LEFT;
  }
  PlanStage& g = add(plan_stage(MPMPC_K_GENERAL, 64, C64, B, 64, list, MPMPC_LIST_NONE));
  g.var = var; g.mode = 2;
  g.deferrable = !closed_loop;
  return p;
}

}  // namespace mpmpc
