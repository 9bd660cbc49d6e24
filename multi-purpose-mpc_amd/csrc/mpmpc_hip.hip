// libmpmpc.so: HIP kernels for gfx950 (MI355X) + the C ABI of include/mpmpc.h.
//
//   K1  mpmpc_assemble_kernel   one thread per (instance, stage): gathers waypoint data from
//                               LDS-staged path tables, builds the stage's dynamics blocks,
//                               offsets, bounds and cost terms, stores them stage-blocked
//                               ([field][instance][stage], unit-stride across lanes).  HBM bound.
//   K2  mpmpc_solve_kernel      the general solve kernel, one 64-lane wavefront per instance, lane = horizon stage;
//                               Ruiz scaling, OSQP ADMM, certified polish, phase 1, all state in VGPRs,
//                               stage coupling by DPP shifts, norms by wavefront reductions.
//                               FP64-VALU issue bound; builds its QP per lane with
//                               K1's code and keeps it in registers: HBM sees the batch inputs and the solution.
//   K2r mpmpc_reduced_kernel    the batch path of the reference's own weights: the (e_y, e_psi, kappa) problem only, 1 / 2 / 4
//                               instances per wavefront, <= 256 registers and 20 KB of LDS: two wavefronts per SIMD
//   K2t mpmpc_reduced_t_kernel  its twin for a terminal cost on the time state (rank-one term, Sherman-Morrison)
//   K2p mpmpc_reduced_tail_kernel  the tail of a K2r launch (infeasible / marginal / capped instances) on the same footing:
//                               phase 1 and one more attempt; K2 takes what it leaves
//   K2r2 / K2t2 / K2p2          mpmpc_reduced_pair_kernel, mpmpc_reduced_t_pair_kernel, mpmpc_reduced_tail_pair_kernel: the same
//                               three solvers with TWO STAGES PER LANE (lane_pair.hpp) - 17 .. 32 stages in 16 lanes (K2r2<16>,
//                               on request) and horizons 64 .. 127 in ONE wavefront (<64>)
//   K2b / K2rb                  mpmpc_solve_block_kernel, mpmpc_reduced_block_kernel - horizons 64 .. 255: the general and the
//                               reduced-native solver on a WORKGROUP of 2 / 4 wavefronts per instance (lane_gpu.hpp: LaneBlock)
//   K2rb2                       mpmpc_reduced_pair_block_kernel, with mpmpc_reduced_tail_pair_block_kernel and
//                               mpmpc_reduced_t_pair_block_kernel - horizons 128 .. 255: two stages per lane on a workgroup of two
//   The twelve solve kernels (K2 ...) are the same steps around their solvers: "the steps of a solve kernel" below.
//   K0 / K3 / K4                corridor tables from the map and the closed-loop rollout (mpmpc_closed_loop.hpp: the kernels, the
//                               setters and getters; mpmpc_rollout_step.hpp, behind the features it drives: the step itself - its
//                               plan, one enqueue function per kernel, the loop), the plant K3n / K3p (mpmpc_plant.hpp), the
//                               actuation delay K3d / K3q (mpmpc_delay.hpp), the dynamic plant K3y (mpmpc_dynamics.hpp), the pose estimator K3e (mpmpc_estimator.hpp), the lidar localisation K0d / K3l (mpmpc_localiser.hpp), the corridor commitment K0k (mpmpc_commitment.hpp), the lookaheads' entry points (mpmpc_lookahead.hpp), perception K0s (mpmpc_perception.hpp),
//                               the speed profile (mpmpc_speed_profile.hpp), the lidar K0l (mpmpc_lidar.hpp), the
//                               footprint audit K0f (mpmpc_footprint.hpp), the walls K0w and K-world (mpmpc_walls.hpp), the
//                               reference paths' static width K0p (mpmpc_path.hpp), the pose projection and the re-route of a
//                               running rollout (mpmpc_project.hpp).
// Host side: the handle and its sub-states are mpmpc_handle.hpp, their buffers device_buf.hpp; this file keeps create / destroy /
// settings, the path and corridor tables, upload / download / the staged calls, the launch dispatch, the resident and timed launches.
//
// No CPU path exists in this library: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#define MPMPC_HD __device__ __forceinline__
#define MPMPC_HOST_DEVICE __host__ __device__
#ifdef MPMPC_PHASE_CLOCK
// profiling builds only (profiles/phases.sh): per-wave time of the phases of K2 in 10 ns ticks
__device__ long long g_phase[4096 * 32];
#define MPMPC_TICK_BEGIN(i) do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096) g_phase[blockIdx.x * 32 + (i)] -= wall_clock64(); } while (0)
#define MPMPC_TICK_END(i) do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096) g_phase[blockIdx.x * 32 + (i)] += wall_clock64(); } while (0)
#define MPMPC_TICK_COUNT(i) do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096) g_phase[blockIdx.x * 32 + (i)] += 1; } while (0)
#endif
#include "lane_gpu.hpp"
#include "lane_pair.hpp"
#include "mpmpc_core.hpp"
#include "mpmpc_reduced.hpp"
#include "mpmpc_reduced_t.hpp"
#include "mpmpc_reduced_tail.hpp"
#include "mpmpc_launch_plan.hpp"
#include "corridor_core.hpp"
#include "rollout_core.hpp"
#include "obstacle_motion_core.hpp"
#include "lookahead_core.hpp"
#include "traffic_core.hpp"
#include "traffic_lookahead_core.hpp"
#include "lidar_core.hpp"
#include "footprint_core.hpp"
#include "wall_core.hpp"
#include "perception_core.hpp"
#include "speed_core.hpp"
#include "path_core.hpp"
#include "project_core.hpp"
#include "plant_core.hpp"
#include "delay_core.hpp"
#include "dynamics_core.hpp"
#include "estimator_core.hpp"
#include "localiser_core.hpp"
#include "commitment_core.hpp"

using namespace mpmpc;

// ------------------------------------------------------------------------------------ kernels
constexpr int K1_THREADS = 256;
constexpr int K1_LDS_WP = 1024;   // path tables of up to this many waypoints are staged in LDS

// NT: non-temporal stores - the default (MPMPC_K1_NT=0: plain stores).  Where the kernel stands (profiles/r4/k1_occupancy.txt,
// same-box medians): 71 - 76 % of the HBM peak at B = 65 536 (550 MB per launch), 59 - 62 % at B = 8 192.  Two things it took:
// rows written to the end of their last 128-byte line (N = 30 fills 31 of a row's 32 doubles; with partial lines the kernel
// reached 39 %, and non-temporal stores were SLOWER than plain ones), and then non-temporal stores (plain ones: 56 - 58 %).
// That is the rate of the store pattern alone (profiles/micro/k1_pattern.hip: 77 %).  Off the solve path: the solve launches
// build their QP in registers with the same code.
// (-DMPMPC_K1_WAVES=w: occupancy experiments, profiles/k1_occupancy.py)
#ifdef MPMPC_K1_WAVES
#define MPMPC_K1_OCC __attribute__((amdgpu_waves_per_eu(MPMPC_K1_WAVES, MPMPC_K1_WAVES)))
#else
#define MPMPC_K1_OCC
#endif
template <bool NT>
__global__ __launch_bounds__(K1_THREADS) MPMPC_K1_OCC void mpmpc_assemble_kernel(
    mpmpc_config cfg, PathTables tab, int B, int ld, const int* __restrict__ wp_id, const double* __restrict__ x0,
    const double* __restrict__ cc, const double* __restrict__ lb, const double* __restrict__ ub,
    double* __restrict__ qp) {
  // (dynamic LDS: 3 x n_wp doubles when the tables are staged - a 200-waypoint lap takes 4.8 KB of a block, not 24)
  extern __shared__ double s_tab[];
  double *s_kappa = s_tab, *s_vref = s_tab + tab.n_wp, *s_ds = s_tab + 2 * tab.n_wp;
  PathTables t = tab;
  if (tab.n_wp <= K1_LDS_WP) {   // block-uniform
    for (int i = threadIdx.x; i < tab.n_wp; i += K1_THREADS) {
      s_kappa[i] = tab.kappa[i];
      s_vref[i] = tab.v_ref[i];
      s_ds[i] = tab.ds_next[i];
    }
    __syncthreads();
    t.kappa = s_kappa;
    t.v_ref = s_vref;
    t.ds_next = s_ds;
  }
  // one thread per (instance, stage) pair, stage fastest: a wavefront writes 64 consecutive doubles of one field.
  // NO grid-stride loop: around a loop the compiler keeps every constant of the stage (the tangent's polynomial, the
  // configuration's doubles) in registers - 109 of them, four waves per SIMD; without it 48 and eight waves per SIMD,
  // and what bounds this kernel is how many waves have their stores in flight (profiles/micro/k1_pattern.hip: the store
  // pattern alone reaches 77 % of the HBM peak)
  using L = LaneGpu<64>;
  const int total = B * ld;
  const int g = blockIdx.x * K1_THREADS + threadIdx.x;
  if (g < total) {
    const int inst = g / ld, k = g - inst * ld;
    if constexpr (!NT) {
      assemble_lane<L>(cfg, t, B, ld, inst, k, wp_id, x0, cc, lb, ub, qp);
    } else {
      double f0[MPMPC_NUM_FIELDS];
      assemble_fields<L>(cfg, t, B, inst, k, wp_id, x0, cc, lb, ub, f0);
      // (rows written to the end of their last 128-byte line, like assemble_lane)
      const int kfill = ((cfg.N + 1 + 15) / 16) * 16 < ld ? ((cfg.N + 1 + 15) / 16) * 16 : ld;
      if (inst < B && k < kfill) {
        double* base = qp + (size_t)inst * ld + k;
        MPMPC_UNROLL
        for (int f = 0; f < MPMPC_NUM_FIELDS; ++f) __builtin_nontemporal_store(k <= cfg.N ? f0[f] : 0.0, base + f * ((size_t)B * ld));
      }
    }
  }
}

// mode 0: the whole solve (early polish attempt, then the full OSQP run of what it could not certify).
// mode 1: the early attempt only; the ids of uncertified instances are appended to tail[1..], tail[0] counts.
// mode 2: the full run only, on the instances listed in tail (one per wave).
// A packed launch (2 or 4 instances per wave) uses modes 1 + 2: the few instances that need hundreds or
// thousands of ADMM iterations then run one per wave, on the faster G = 64 code, instead of holding a
// packed wave (and its finished partner lanes) for the whole tail.
// The launch assembles its own QP: every lane builds the 27 fields of its (instance, stage) with K1's code
// (assemble_fields) and goes on with them in registers - the stage-blocked QP is never written to or read from
// memory on this path (mpmpc_assemble, the parity / debug export, is what runs K1 proper).
struct AssembleIn {
  PathTables tab;
  const int* wp_id;
  const double *x0, *cc, *lb, *ub;
};

// ---------------------------------------------------------------------------------- the steps of a solve kernel
// Every solve kernel below is the same eight steps around its solver; each step is written once here:
//   1 empty_lists          the tail list(s) the NEXT launch appends to start empty
//   2 inst_in_*            which instance this lane has - in batch order (a workgroup kernel is batch order with one
//                          instance per group), or in the order of a tail list, one entry per group or packed - and
//                          its stage, minus the lane offset of the layout
//   3 the warm-start guess (K2 and K2r, written out there: as a function it changes the branches of both)
//   4 assemble_in          the lane's 27 fields, in registers
//   5 the solver's run     (the kernel's own: the solvers' signatures differ)
//   6 *_again              instance and stage formed anew, so that they do not live in registers through the solve
//   7 the solver's store   (the kernel's own)
//   8 MPMPC_LEFT_UNSOLVED / leave_to_tail   stage 0 of an instance left MPMPC_UNSOLVED appends it to the list of the next kernel
// (tests/emul/wave_loop.hpp is the same skeleton for the CPU emulation, with the same names)
template <class... P>
MPMPC_HD void empty_lists(P*... list) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ((*list = 0), ...);
}

// batch order: group g carries the instances g * per_wave .. (the last group of a packed launch may carry ids >= B: "none")
template <class L>
MPMPC_HD typename L::ival inst_in_batch() { return L::slot() + (int)(blockIdx.x * L::per_wave); }
template <class L>
MPMPC_HD typename L::ival inst_in_batch_again() { return L::slot_again() + (int)(blockIdx.x * L::per_wave); }
// list order: the groups take consecutive entries of list[1..], list[0] counts; groups beyond its end return at once
#define MPMPC_PAST_LIST(list) ((int)blockIdx.x * L::per_wave >= (list)[0])          // (L: the kernel's lanes; a macro for the reason given at step 8)
MPMPC_HD int inst_in_list(const int* list) { return list[1 + blockIdx.x]; }      // one instance per group
// ... packed: the last wave may carry B = "none"
template <class L>
MPMPC_HD int inst_in_packed_list(const int* list, int B) {
  const int e = blockIdx.x * L::per_wave + L::slot();
  return e < list[0] ? list[1 + e] : B;
}
template <class L>
MPMPC_HD int inst_in_packed_list_again(const int* list, int B) {
  const int e = blockIdx.x * L::per_wave + L::slot_again();
  return e < list[0] ? list[1 + e] : B;
}
// (the workgroup kernels keep the values of step 2 through the solve: LaneBlock's *_again are the same threadIdx.x)

// (ROUTES = false: without the route view of gather_stage - the warm-started kernels of the closed loop, which refuses routes)
template <class L, bool ROUTES = true>
MPMPC_HD void assemble_in(const mpmpc_config& cfg, const AssembleIn& ain, int B, const typename L::ival& inst,
                          const typename L::ival& k, typename L::real* fields) {
  assemble_fields<L, ROUTES>(cfg, ain.tab, B, inst, k, ain.wp_id, ain.x0, ain.cc, ain.lb, ain.ub, fields);
}

// Has this lane stage 0 of an instance of the batch that the solver left MPMPC_UNSOLVED?  For an `if`, on the scalars of the
// lane's first stage (two stages per lane: component 0).
// (Why the tests of steps 2 and 8 are macros and the stage line and step 3 are written out in the kernels: a function is
//  optimised on its own before it is inlined - an && chain it returns becomes selects, `stage - lane_offset` is reassociated -
//  and the branches and the register allocation of every kernel that calls it change; the pieces that are functions are
//  those that leave every kernel's instructions as they were: profiles/kernel_resources.py --compare, docs/HISTORY.md.)
#define MPMPC_LEFT_UNSOLVED(inst, k, status) ((k) == 0 && (inst) < B && (status) == MPMPC_UNSOLVED)
// ... of a kernel that takes one instance per group from a list: its entries are always < B and no lane carries "none"
#define MPMPC_LEFT_UNSOLVED_LISTED(k, status) ((k) == 0 && (status) == MPMPC_UNSOLVED)
MPMPC_HD void leave_to_tail(int* list, int inst) { list[1 + atomicAdd(list, 1)] = inst; }
// ... and "this launch left a tail": the launch's sequence number, in host memory the device writes through (read by the host
// after the stream has drained: observe_tail)
MPMPC_HD void leave_to_tail(int* list, int inst, unsigned* flag, unsigned seq) {
  leave_to_tail(list, inst);
  __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// VAR: 0 = the full problem with diagonal weights, 1 = full weights (FQ: Q, R, QN with off-diagonal entries), 2 = reduced polish (RED),
//      3 = the full problem whose states e_psi and t have no bounds (FREEX; one-instance-per-wave kernels only)
template <int G, int C, bool WARM, int VAR = 0>
__global__ __launch_bounds__(64) void mpmpc_solve_kernel(mpmpc_config cfg, SolverParams st, int B, int ld,
                                                         AssembleIn ain, double* __restrict__ z,
                                                         double* __restrict__ u0, int* __restrict__ status,
                                                         int* __restrict__ iters, double* __restrict__ resid,
                                                         double* __restrict__ y, int mode, int* __restrict__ tail,
                                                         int* __restrict__ act, const int* __restrict__ shift,
                                                         int* __restrict__ tail_reset) {
  using L = LaneGpu<G, C>;
  int inst = inst_in_batch<L>();
  if (mode == 2) {
    // the list the NEXT launch on this handle will fill starts empty (two lists, used in turn: no memset between launches)
    empty_lists(tail_reset);
    if (MPMPC_PAST_LIST(tail)) return;       // wave-uniform: G = 64 here
    inst = inst_in_list(tail);
  }
  const int k = L::stage() - lane_offset(G, C, cfg.N);      // stage of this lane (negative / > N: none)
  // closed loop: the active set the previous step certified for this car, moved on by the waypoints it advanced
  int guess = 0;
  if (WARM && act && shift && inst < B && k >= 0 && k <= cfg.N) {
    int kk = k + shift[inst];
    guess = act[inst * ld + (kk > cfg.N ? cfg.N : kk)];
  }
  MPMPC_TICK_BEGIN(8);
  double fields[MPMPC_NUM_FIELDS];
  assemble_in<L, !WARM>(cfg, ain, B, inst, k, fields);
  Solver<L, VAR == 1, VAR == 2, VAR == 3, VAR == 2> s;   // (the reduced variant factors its 16-lane chains by cyclic reduction, like the reduced-native kernels)
  // (second launch of a packed batch: the interior-point iterations the first launch spent on this instance)
  const int base_ipm = (mode == 2 && iters) ? iters[inst * 2 + 1] : 0;
  static_assert(G == 64, "the general kernels run one instance per wave (only the reduced-native kernels pack)");
  double woff[7];
  weight_offdiag(cfg, woff);
  s.template run<WARM, true>(fields, B, inst, k, cfg.N, st, mode, guess, base_ipm, VAR == 1 ? woff : nullptr);
  MPMPC_TICK_BEGIN(7);
  s.store(inst, k, cfg.wheelbase, z, u0, status, iters, resid, y, WARM ? act : nullptr, ld);
  MPMPC_TICK_END(7);
  MPMPC_TICK_END(8);
  if (mode == 1 && MPMPC_LEFT_UNSOLVED(inst, k, s.status)) leave_to_tail(tail, inst);
}

// K2b: the general solve kernel for horizons above 63 - one instance per WORKGROUP of G = 128 / 256 threads (2 / 4
// wavefronts), one lane per stage as before; the lanes of different wavefronts talk through LDS (lane_gpu.hpp: LaneBlock).
// Same Solver code, the whole solve in one launch (mode 0), cold starts.  VAR as for mpmpc_solve_kernel: 0 = the full problem,
// 1 = full weight matrices, 2 = the polish on the (e_y, e_psi, kappa) problem where the time state separates (the reference's
// own weights: 2 x 2 blocks in the sweeps instead of 3 x 3, three entries per lane instead of five, fewer iterations).
template <int G, int VAR>
__global__ __launch_bounds__(G) void mpmpc_solve_block_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                              double* __restrict__ z, double* __restrict__ u0,
                                                              int* __restrict__ status, int* __restrict__ iters,
                                                              double* __restrict__ resid, double* __restrict__ y,
                                                              const int* __restrict__ tail) {
  using L = LaneBlock<G>;
  // tail: the instances the reduced-native workgroup kernel (below) could not certify - one workgroup each, straight to
  // phase 1 and the full iteration (mode 2, as for the wavefront kernels); null: every instance, the whole solve
  if (tail && MPMPC_PAST_LIST(tail)) return;
  const int inst = tail ? inst_in_list(tail) : inst_in_batch<L>();
  const int k = L::stage() - lane_offset(G, G / 2, cfg.N);
  double fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  // (the reduced variant factors its chains of four / eight rows by cyclic reduction: Solver::kCR64)
  Solver<L, VAR == 1, VAR == 2, false, VAR == 2> s;
  double woff[7];
  weight_offdiag(cfg, woff);
  const int base_ipm = (tail && iters) ? iters[inst * 2 + 1] : 0;       // (the interior-point iterations the first kernel spent on it)
  s.template run<false, true>(fields, B, inst, k, cfg.N, st, tail ? 2 : 0, 0, base_ipm, VAR == 1 ? woff : nullptr);
  s.store(inst, k, cfg.wheelbase, z, u0, status, iters, resid, y, nullptr, 0);
}

// K2rb: the reduced-native solver (mpmpc_reduced.hpp: the (e_y, e_psi, kappa) problem from the start - own scaling, interior
// point from x = 0, active-set rounds, certificate) on a workgroup, for the reference's own weights at horizons above 63.
// What it cannot certify is listed in `tail` for mpmpc_solve_block_kernel<G, 2>.
// (40 cold slots like K2r instead of the general solver's 66: 50 KB of LDS per workgroup at G = 128 - three workgroups per CU)
// (the workgroup kernels empty no list: the launch plan has them emptied on the stream in front of them)
constexpr int RNB_SLOTS = 40;
template <int G>
__global__ __launch_bounds__(G) void mpmpc_reduced_block_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                                double* __restrict__ z, double* __restrict__ u0,
                                                                int* __restrict__ status, int* __restrict__ iters,
                                                                double* __restrict__ resid, double* __restrict__ y,
                                                                int* __restrict__ tail) {
  using L = LaneBlock<G, RNB_SLOTS>;
  const int inst = inst_in_batch<L>();
  const int k = L::stage() - lane_offset(G, G / 2, cfg.N);
  double fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedSolver<L> s;
  s.template run<false>(fields, B, inst, k, cfg.N, st, 0);
  s.store(inst, k, cfg.wheelbase, z, u0, status, iters, resid, y, nullptr, 0);
  if (MPMPC_LEFT_UNSOLVED(inst, k, s.status)) leave_to_tail(tail, inst);
}

// K2r: the reduced-native solve kernel (mpmpc_reduced.hpp) - the batch path of every configuration whose time state
// separates (the reference's own weights).  One launch assembles (K1's code, in registers), solves and stores; the ids of
// the instances it cannot certify are appended to tail[1..] (tail[0] counts) for the general kernel in mode 2.
// 40 LDS slots (20 KB) and at most 256 registers: two wavefronts per SIMD.
constexpr int RN_SLOTS = 40;
// WARM (closed loop): act [B x ld] holds the active sets the previous step certified, shift [B] the waypoints each car has
// advanced since; the kernel starts from them and leaves this step's sets in act.
template <int G, int C, bool WARM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void mpmpc_reduced_kernel(mpmpc_config cfg, SolverParams st, int B, int ld, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           int* __restrict__ tail, int* __restrict__ act,
                                                           const int* __restrict__ shift, int* __restrict__ tail_reset,
                                                           unsigned* __restrict__ tail_flag, unsigned seq, int* __restrict__ tail2_reset) {
  using L = LaneGpu<G, C, RN_SLOTS>;
  // (the list of the NEXT launch is emptied here as well: the tail launch, which does it too, may be deferred - see
  //  run_stages; and so is the list the reduced-native tail kernel of THIS launch appends to)
  empty_lists(tail_reset, tail2_reset);
  // (the instance stays written out in K2r and K2t, which carry every headline number: a helper around these lines has
  //  moved their instructions in every form tried - docs/HISTORY.md)
  const int inst = blockIdx.x * L::per_wave + L::slot();
  const int k = L::stage() - lane_offset(G, C, cfg.N);
  int guess = 0;          // (step 3 as in mpmpc_solve_kernel, whose launch may come without the two arrays)
  if (WARM && inst < B && k >= 0 && k <= cfg.N) {
    const int kk = k + shift[inst];
    guess = act[inst * ld + (kk > cfg.N ? cfg.N : kk)];
  }
  MPMPC_TICK_BEGIN(8);
  double fields[MPMPC_NUM_FIELDS];
  assemble_in<L, !WARM>(cfg, ain, B, inst, k, fields);
  ReducedSolver<L> s;
  s.template run<WARM>(fields, B, inst, k, cfg.N, st, guess);
  MPMPC_TICK_BEGIN(7);
  // (instance and stage are formed again rather than kept in registers through the solve)
  const int inst_o = blockIdx.x * L::per_wave + L::slot_again();
  const int k_o = L::stage_again() - lane_offset(G, C, cfg.N);
  s.store(inst_o, k_o, cfg.wheelbase, z, u0, status, iters, resid, y, WARM ? act : nullptr, ld);
  MPMPC_TICK_END(7);
  MPMPC_TICK_END(8);
  if (MPMPC_LEFT_UNSOLVED(inst_o, k_o, s.status)) leave_to_tail(tail, inst_o, tail_flag, seq);
}

// K2r2: K2r with TWO STAGES PER LANE (lane_pair.hpp): an instance of 17 .. 32 stages takes 16 lanes, a
// wavefront carries FOUR.  The same ReducedSolver on the pair backend: every elementwise operation is issued for both stages of
// the lane (the work per stage is what it was), a stage-order shift moves one of the two components across lanes, a wave
// reduction serves four instances, and the cyclic reduction eliminates the even stages inside the lanes before its four
// cross-lane levels run on the survivors (mpmpc_solver_s2.hpp).  Twice the state per lane: up to 512 registers and 80 LDS slots
// (40 KB), ONE wavefront per SIMD - the two independent stages of a lane stand in for the second wave.  Cold starts only (the
// closed loop keeps K2r); same launch contract as K2r, same tail lists.
// GB = 64: an instance of 65 .. 128 stages (horizons 64 .. 127) in ONE wavefront - a chain of four rows, no LDS exchange and
// no workgroup barrier, where the one-stage layout takes a workgroup of two wavefronts (K2rb); what it cannot certify goes to
// mpmpc_solve_block_kernel<128, 2> through the same list.
constexpr int RN2_SLOTS = 80;
template <int GB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void mpmpc_reduced_pair_kernel(mpmpc_config cfg, SolverParams st, int B, int ld, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           int* __restrict__ tail, int* __restrict__ tail_reset,
                                                           unsigned* __restrict__ tail_flag, unsigned seq, int* __restrict__ tail2_reset) {
  using L = LanePair<LaneGpu<GB, GB, RN2_SLOTS>>;
  empty_lists(tail_reset, tail2_reset);
  const I2 inst = inst_in_batch<L>();
  const I2 k = L::stage();          // (one chain, stage 0 on lane 0: no lane offset)
  MPMPC_TICK_BEGIN(8);
  D2 fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedSolver<L> s;
  s.template run<false>(fields, B, inst, k, cfg.N, st);
  MPMPC_TICK_BEGIN(7);
  const I2 inst_o = inst_in_batch_again<L>();
  const I2 k_o = L::stage_again();
  s.store(inst_o, k_o, cfg.wheelbase, z, u0, status, iters, resid, y, nullptr, ld);
  MPMPC_TICK_END(7);
  MPMPC_TICK_END(8);
  if (MPMPC_LEFT_UNSOLVED(inst_o.v[0], k_o.v[0], s.status.v[0])) leave_to_tail(tail, inst_o.v[0], tail_flag, seq);
}

// K2rb2: horizons 128 .. 255 with two stages per lane - the instance on a workgroup of TWO wavefronts (128 lanes, one chain of
// eight rows; the lanes of the two wavefronts talk through LDS: LaneBlock<128, ., 128>) instead of four with one stage per lane.
// Lean LDS - 37 pair slots (ReducedSolver::kLean) + 4 exchange rows = 80 000 B - so that TWO workgroups share a CU: four
// wavefronts per CU, one per SIMD, and two instances per CU in flight where K2rb<256> (100 KB, 298 registers) holds one.
constexpr int RNB2_SLOTS = 74, RNB2_XR = 4;
using LanePairBlock = LanePair<LaneBlock<128, RNB2_SLOTS, 128, RNB2_XR>>;
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1))) void mpmpc_reduced_pair_block_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           int* __restrict__ tail) {
  using L = LanePairBlock;
  const I2 inst = inst_in_batch<L>();
  const I2 k = L::stage();
  D2 fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedSolver<L> s;
  static_assert(ReducedSolver<L>::kLean, "37 pair slots: the lean cold storage");
  s.template run<false>(fields, B, inst, k, cfg.N, st);
  s.store(inst, k, cfg.wheelbase, z, u0, status, iters, resid, y, nullptr, 0);
  if (MPMPC_LEFT_UNSOLVED(inst.v[0], k.v[0], s.status.v[0])) leave_to_tail(tail, inst.v[0]);
}

// ... its tail (K2p's solver) and its twin for a terminal cost on the time state (K2t's solver) on the same workgroup layout, with
// the FULL cold storage (80 slots + 4 exchange rows = 86 KB: one workgroup per CU - the tail is a tenth of a batch, and the
// terminal-time weights ran the general 3-state solver on FOUR wavefronts before: 0.19 M solves/s at N = 150)
using LanePairBlockFull = LanePair<LaneBlock<128, RN2_SLOTS, 128, RNB2_XR>>;
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1))) void mpmpc_reduced_tail_pair_block_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           const int* __restrict__ tail, int* __restrict__ tail2) {
  using L = LanePairBlockFull;
  if (MPMPC_PAST_LIST(tail)) return;
  const int in0 = inst_in_list(tail);
  const I2 inst(in0);
  const I2 k = L::stage();
  D2 fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedTailSolver<L> s;
  const int base = iters ? iters[in0 * 2 + 1] : 0;
  s.run(fields, B, inst, k, cfg.N, st, I2(base));
  s.store(inst, k, cfg.wheelbase, z, u0, status, iters, resid, y);
  if (MPMPC_LEFT_UNSOLVED_LISTED(k.v[0], s.status.v[0])) leave_to_tail(tail2, in0);
}
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1))) void mpmpc_reduced_t_pair_block_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           int* __restrict__ tail) {
  using L = LanePairBlockFull;
  const I2 inst = inst_in_batch<L>();
  const I2 k = L::stage();
  D2 fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedTSolver<L> s;
  s.run(fields, B, inst, k, cfg.N, st, cfg.QN[2]);
  s.store(inst, k, cfg.wheelbase, z, u0, status, iters, resid, y);
  if (MPMPC_LEFT_UNSOLVED(inst.v[0], k.v[0], s.status.v[0])) leave_to_tail(tail, inst.v[0]);
}

// K2p2: the reduced-native TAIL solver (mpmpc_reduced_tail.hpp: phase 1 / Farkas ray / relaxed plan, one more attempt) with two
// stages per lane - the tail of K2r2<64> at horizons 64 .. 127, one instance per wavefront, where the general solver on a workgroup
// used to take all of it (40 % of an obstacle-course step at N = 100); what it leaves is listed in tail2 for that kernel.
template <int GB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void mpmpc_reduced_tail_pair_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           const int* __restrict__ tail, int* __restrict__ tail2) {
  using L = LanePair<LaneGpu<GB, GB, RN2_SLOTS>>;
  static_assert(L::per_wave == 1, "one instance per wavefront");
  if (MPMPC_PAST_LIST(tail)) return;
  const int in0 = inst_in_list(tail);
  const I2 inst(in0, in0);
  const I2 k = L::stage();
  D2 fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedTailSolver<L> s;
  const int base = iters ? iters[in0 * 2 + 1] : 0;
  s.run(fields, B, inst, k, cfg.N, st, I2(base));
  const I2 k_o = L::stage_again();
  s.store(inst, k_o, cfg.wheelbase, z, u0, status, iters, resid, y);
  if (MPMPC_LEFT_UNSOLVED_LISTED(k_o.v[0], s.status.v[0])) leave_to_tail(tail2, in0);
}

// K2t2: K2t with two stages per lane, for horizons 64 .. 127 - ONE wavefront per instance where such weights used to run the
// general 3-state solver on a workgroup of two (mpmpc_solve_block_kernel<128, 0>); 502 registers, no scratch.
template <int GB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void mpmpc_reduced_t_pair_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           int* __restrict__ tail) {
  using L = LanePair<LaneGpu<GB, GB, RN2_SLOTS>>;
  const I2 inst = inst_in_batch<L>();
  const I2 k = L::stage();
  D2 fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedTSolver<L> s;
  s.run(fields, B, inst, k, cfg.N, st, cfg.QN[2]);
  const I2 inst_o = inst_in_batch_again<L>();
  const I2 k_o = L::stage_again();
  s.store(inst_o, k_o, cfg.wheelbase, z, u0, status, iters, resid, y);
  if (MPMPC_LEFT_UNSOLVED(inst_o.v[0], k_o.v[0], s.status.v[0])) leave_to_tail(tail, inst_o.v[0]);
}

// K2t: the reduced-native kernel of the weightings with a TERMINAL cost on the time state (mpmpc_reduced_t.hpp; BASELINE
// config 3): the (e_y, e_psi, kappa) problem plus the speeds plus one rank-one term, Sherman-Morrison on the 2 x 2-block
// solves.  Same launch contract as K2r (cold starts only: a warm-started closed loop of such weights starts cold here).
template <int G, int C>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void mpmpc_reduced_t_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           int* __restrict__ tail, int* __restrict__ tail_reset,
                                                           unsigned* __restrict__ tail_flag, unsigned seq) {
  using L = LaneGpu<G, C, RN_SLOTS>;
  empty_lists(tail_reset);           // (no reduced-native tail kernel follows this one: one list)
  // (the instance stays written out in K2r and K2t, which carry every headline number: a helper around these lines has
  //  moved their instructions in every form tried - docs/HISTORY.md)
  const int inst = blockIdx.x * L::per_wave + L::slot();
  const int k = L::stage() - lane_offset(G, C, cfg.N);
  MPMPC_TICK_BEGIN(8);
  double fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedTSolver<L> s;
  s.run(fields, B, inst, k, cfg.N, st, cfg.QN[2]);
  MPMPC_TICK_BEGIN(7);
  // (instance and stage are formed again rather than kept in registers through the solve)
  const int inst_o = blockIdx.x * L::per_wave + L::slot_again();
  const int k_o = L::stage_again() - lane_offset(G, C, cfg.N);
  s.store(inst_o, k_o, cfg.wheelbase, z, u0, status, iters, resid, y);
  MPMPC_TICK_END(7);
  MPMPC_TICK_END(8);
  if (MPMPC_LEFT_UNSOLVED(inst_o, k_o, s.status)) leave_to_tail(tail, inst_o, tail_flag, seq);
}

// K2p: the reduced-native TAIL kernel (mpmpc_reduced_tail.hpp): phase 1 and one more attempt of the certified polish on
// the instances the reduced-native launch listed in `tail` - two per wave (<32,16>, the default: 243 registers, no scratch),
// one per wave in the split layout (<64,16>) or, for horizons 32 .. 63, one per wave with a lane per stage (<64,32>: 235
// registers, no scratch) - within the same 256 registers and 40 LDS slots: a tail wave shares its SIMD.  What it leaves UNSOLVED is appended to tail2 for the general kernel (mode 2).
template <int G, int C>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void mpmpc_reduced_tail_kernel(mpmpc_config cfg, SolverParams st, int B, AssembleIn ain,
                                                           double* __restrict__ z, double* __restrict__ u0,
                                                           int* __restrict__ status, int* __restrict__ iters,
                                                           double* __restrict__ resid, double* __restrict__ y,
                                                           const int* __restrict__ tail, int* __restrict__ tail_reset,
                                                           int* __restrict__ tail2, unsigned* __restrict__ tail2_flag, unsigned seq) {
  using L = LaneGpu<G, C, RN_SLOTS>;
  empty_lists(tail_reset);
  if (MPMPC_PAST_LIST(tail)) return;
  const int inst = inst_in_packed_list<L>(tail, B);
  const int k = L::stage() - lane_offset(G, C, cfg.N);
  MPMPC_TICK_BEGIN(8);
  double fields[MPMPC_NUM_FIELDS];
  assemble_in<L>(cfg, ain, B, inst, k, fields);
  ReducedTailSolver<L> s;
  s.run(fields, B, inst, k, cfg.N, st, (iters && inst < B) ? iters[inst * 2 + 1] : 0);
  MPMPC_TICK_BEGIN(7);
  const int inst_o = inst_in_packed_list_again<L>(tail, B);
  const int k_o = L::stage_again() - lane_offset(G, C, cfg.N);
  s.store(inst_o, k_o, cfg.wheelbase, z, u0, status, iters, resid, y);
  MPMPC_TICK_END(7);
  MPMPC_TICK_END(8);
  if (MPMPC_LEFT_UNSOLVED(inst_o, k_o, s.status)) leave_to_tail(tail2, inst_o, tail2_flag, seq);
}

// ------------------------------------------------------------------------------------ host side
#include "mpmpc_handle.hpp"

// the memory of device_buf.hpp: the only four places of the library that take or return device or page-locked memory
int mpmpc::device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
int mpmpc::device_free(void* p) { return hipFree(p); }
int mpmpc::pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
int mpmpc::pinned_free(void* p) { return hipHostFree(p); }

static int host_stage_ld(int N) { return N + 1 <= 16 ? 16 : (N + 1 <= 32 ? 32 : (N + 1 <= 64 ? 64 : (N + 1 <= 128 ? 128 : 256))); }

static int check_settings(const mpmpc_settings* s) {
  if (!s) return fail(MPMPC_E_ARG, "settings is NULL");
  if (!(s->rho > 0) || !(s->sigma > 0) || !(s->alpha > 0 && s->alpha < 2))
    return fail(MPMPC_E_ARG, "need rho > 0, sigma > 0, 0 < alpha < 2");
  if (s->early_polish < 0) return fail(MPMPC_E_ARG, "early_polish must be >= 0");
  if (s->early_scaling < 0) return fail(MPMPC_E_ARG, "early_scaling must be >= 0");
  if (s->max_iter < 0 || s->check_termination < 0 || s->scaling < 0 || s->ipm_max_iter < 0 || s->as_rounds < 0 ||
      s->as_refine < 0)
    return fail(MPMPC_E_ARG, "iteration counts must be non-negative");
  if (s->polish != 0 && s->polish != 2) return fail(MPMPC_E_ARG, "polish must be 0 or 2");
  if (s->polish == 2 && (!(s->ipm_reg > 0) || !(s->as_delta > 0) || !(s->ipm_tol > 0)))
    return fail(MPMPC_E_ARG, "polish needs ipm_reg, ipm_tol, as_delta > 0");
  if (s->phase1 != 0 && s->phase1 != 1) return fail(MPMPC_E_ARG, "phase1 must be 0 or 1");
  if (s->reduce != 0 && s->reduce != 1) return fail(MPMPC_E_ARG, "reduce must be 0 or 1");
  if (s->native != 0 && s->native != 1) return fail(MPMPC_E_ARG, "native must be 0 or 1");
  if (!(s->native_ipm_tol > 0)) return fail(MPMPC_E_ARG, "need native_ipm_tol > 0");
  if (s->early_start != 0 && s->early_start != 1) return fail(MPMPC_E_ARG, "early_start must be 0 or 1");
  if (s->phase1_accept != 0 && s->phase1_accept != 1) return fail(MPMPC_E_ARG, "phase1_accept must be 0 or 1");
  if (!(s->phase1_band >= 0)) return fail(MPMPC_E_ARG, "phase1_band must be >= 0");
  if (!(s->ipm_start_dual >= 0)) return fail(MPMPC_E_ARG, "need ipm_start_dual >= 0");
  if (!(s->ipm_start_mu >= 0) || !(s->ipm_start_slack > 0)) return fail(MPMPC_E_ARG, "need ipm_start_mu >= 0, ipm_start_slack > 0");
  if (!(s->as_add_fraction >= 0) || !(s->as_add_fraction <= 1)) return fail(MPMPC_E_ARG, "need 0 <= as_add_fraction <= 1");
  if (!(s->ipm_diverged > 1) || !(s->phase1_theta > 0) || !(s->phase1_eps > 0))
    return fail(MPMPC_E_ARG, "need ipm_diverged > 1, phase1_theta > 0, phase1_eps > 0");
  return MPMPC_OK;
}

static int grow_slots(mpmpc_handle h, int want);
static int upload_through_bounce(mpmpc_handle h, void* dst, const void* src, size_t bytes);
static int launch_assemble(mpmpc_handle h, int B);
static int launch_solve(mpmpc_handle h, Slot& sl, int B, bool closed_loop = false, bool want_y = true, LaunchKind kind = LAUNCH_SINGLE);

extern "C" {

#ifndef MPMPC_SRC_HASH
#define MPMPC_SRC_HASH "unhashed"
#endif
const char* mpmpc_version(void) { return "mpmpc 0.2.0 (gfx950, float64, src " MPMPC_SRC_HASH ")"; }
const char* mpmpc_last_error(void) { return g_err.c_str(); }

int mpmpc_device_count(int32_t* count) {
  if (!count) return fail(MPMPC_E_ARG, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(MPMPC_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = n;
  return MPMPC_OK;
}

void mpmpc_default_settings(mpmpc_settings* s) {
  if (!s) return;
  s->rho = 0.1; s->sigma = 1e-6; s->alpha = 1.6;
  s->eps_abs = 1e-3; s->eps_rel = 1e-3; s->eps_prim_inf = 1e-4; s->eps_dual_inf = 1e-4;
  s->max_iter = 4000; s->check_termination = 25; s->scaling = 10;
  s->adaptive_rho = 1; s->adaptive_rho_interval = 50; s->adaptive_rho_tolerance = 5.0;
  s->polish = 2; s->ipm_max_iter = 30; s->ipm_tol = 1e-8; s->ipm_reg = 1e-8;
  s->as_delta = 1e-10; s->as_refine = 5; s->as_rounds = 4; s->cert_tol = 1e-8;
  s->early_polish = 1;
  s->early_scaling = 1;
  s->phase1 = 1;
  s->ipm_diverged = 1e2;
  s->phase1_theta = 1.0;
  s->phase1_eps = 1e-6;
  s->reduce = 1;
  s->ipm_start_slack = 0.1;
  s->ipm_start_mu = 0.01;
  s->ipm_start_dual = 0.2;
  s->as_add_fraction = 0.25;
  s->phase1_accept = 1;
  s->native = 1;
  s->native_ipm_tol = 1e-7;
  s->early_start = 0;
  s->phase1_band = 3.0;
}

int32_t mpmpc_stage_ld(int32_t N) { return host_stage_ld(N); }

static size_t pad8(size_t b) { return (b + 7) & ~size_t(7); }
struct BlockLayout {
  size_t wp_id, x0, cc, lb, ub, in_end_cc, in_end;          // byte offsets in in_block
  size_t u0, resid, status, iters, z, y, out_end_z, out_end;  // byte offsets in out_block
};
static BlockLayout block_layout(int N, int B) {
  BlockLayout L;
  const size_t d = sizeof(double), n = 5 * (size_t)N + 3, m = 8 * (size_t)N + 6, b = (size_t)B;
  L.wp_id = 0;
  L.x0 = pad8(sizeof(int) * b);
  L.cc = L.x0 + d * 3 * b;
  L.lb = L.in_end_cc = L.cc + d * 2 * N * b;
  L.ub = L.lb + d * N * b;
  L.in_end = L.ub + d * N * b;
  L.u0 = 0;
  L.resid = L.u0 + d * 2 * b;
  L.status = L.resid + d * 2 * b;
  L.iters = L.status + pad8(sizeof(int) * b);
  L.z = L.iters + pad8(sizeof(int) * 2 * b);
  L.y = L.out_end_z = L.z + d * n * b;
  L.out_end = L.y + d * m * b;
  return L;
}
static void lay_out(mpmpc_handle h, int B) {
  const BlockLayout L = block_layout(h->cfg.N, B);
  h->io.wp_id = (int*)(h->io.in_block + L.wp_id);
  h->io.x0 = (double*)(h->io.in_block + L.x0);
  h->io.cc = (double*)(h->io.in_block + L.cc);
  h->io.lb = (double*)(h->io.in_block + L.lb);
  h->io.ub = (double*)(h->io.in_block + L.ub);
  for (int i = 0; i < h->n_slots; ++i) {
    Slot& a = h->slot[i];
    a.u0 = (double*)(a.out_block + L.u0);
    a.resid = (double*)(a.out_block + L.resid);
    a.status = (int*)(a.out_block + L.status);
    a.iters = (int*)(a.out_block + L.iters);
    a.z = (double*)(a.out_block + L.z);
    a.y = (double*)(a.out_block + L.y);
  }
  h->io.laid_out = B;
}

// ---- Launch streams and hardware queues.  The HIP runtime maps the streams of a process onto GPU_MAX_HW_QUEUES hardware queues
// (4 when the variable is absent); two streams that land on one queue take turns, and a resident launch on such a stream
// waits for a launch it was meant to run beside.  So a handle never drives more launch streams than the process has queues:
// mpmpc_set_pipeline asks, mpmpc_pipeline_streams answers.  The variable is read once per process and never written.
int32_t mpmpc_hw_queue_budget(const char* text) {
  const int32_t runtime_default = 4;
  if (!text) return runtime_default;
  char* end = nullptr;
  errno = 0;
  const long v = std::strtol(text, &end, 10);
  if (end == text || errno != 0) return runtime_default;      // no number at all, or out of range
  while (*end == ' ' || *end == '\t') ++end;
  if (*end != '\0' || v < 1) return runtime_default;           // trailing text, zero, negative: not a queue count
  return v > 1024 ? 1024 : (int32_t)v;
}
int32_t mpmpc_pipeline_streams(int32_t depth, int32_t hw_queues) {
  if (depth < 1) depth = 1;
  if (depth > mpmpc_handle_s::MAX_PIPELINE) depth = mpmpc_handle_s::MAX_PIPELINE;
  if (hw_queues < 1) hw_queues = 1;
  return depth < hw_queues ? depth : hw_queues;
}
// The plan of a solve launch (mpmpc_launch_plan.hpp: the launcher runs what plan_solve says), written out row by row.
int32_t mpmpc_launch_plan(const mpmpc_config* cfg, const mpmpc_settings* settings, const int32_t* knobs, int32_t B, int32_t closed_loop,
                          int32_t kind, int32_t* rows) {
  if (!cfg || !settings || !knobs || !rows) return fail(MPMPC_E_ARG, "cfg, settings, knobs and rows must not be NULL");
  if (cfg->N < 3 || cfg->N > MPMPC_MAX_HORIZON) return fail(MPMPC_E_ARG, "horizon N must satisfy 3 <= N <= 255");
  if (B < 1 || kind < 0 || kind > 1) return fail(MPMPC_E_ARG, "need B >= 1 and kind 0 or 1");
  if (!packing_valid(cfg->N, knobs[0]) || knobs[1] < 0 || knobs[1] > 2 || knobs[2] < 1 || knobs[2] > mpmpc_handle_s::MAX_PIPELINE ||
      knobs[3] < 0 || knobs[3] > 2)
    return fail(MPMPC_E_ARG, "knobs: a packing of this horizon, tail kernel 0 .. 2, 1 .. 8 launch slots, warm start 0 .. 2");
  const SolvePlan p = plan_solve(*cfg, *settings, LaunchKnobs{knobs[0], knobs[1] != 0, knobs[1] == 2, knobs[2], knobs[3]}, B,
                                 closed_loop != 0, kind ? LAUNCH_PIPELINED : LAUNCH_SINGLE);
  std::memcpy(rows, p.stage, (size_t)p.n * sizeof(PlanStage));
  return p.n;
}
static int launch_streams(int depth) {
  static const int32_t budget = mpmpc_hw_queue_budget(std::getenv("GPU_MAX_HW_QUEUES"));
  return mpmpc_pipeline_streams(depth, budget);
}
static hipError_t create_launch_stream(hipStream_t* s) { return hipStreamCreate(s); }

static void free_slot(Slot& s) {
  s.out_block.reset();
  s.tail.reset();
  s.tail_flag.reset();
  if (s.stream) (void)hipStreamDestroy(s.stream);
  s = Slot{};
}
// One launch slot: its stream FIRST (nothing in this library may run on the null stream - its first use makes the runtime give it
// a hardware queue for the life of the process, one fewer for the launch streams, see launch_streams), the output block for
// max_batch instances, the tail lists, the tail flag.  The lists are cleared on the slot's own stream: they are only ever used
// by launches on it, which are ordered behind that; the wait reports a failure here.
static int alloc_slot(mpmpc_handle h, Slot& s) {
  const size_t out_bytes = block_layout(h->cfg.N, h->cfg.max_batch).out_end, tail_bytes = 3 * ((size_t)h->cfg.max_batch + 1) * sizeof(int);
  if (create_launch_stream(&s.stream) != hipSuccess || alloc_all(Want{s.out_block, out_bytes}, Want{s.tail, tail_bytes / sizeof(int)}, Want{s.tail_flag, 2}) != 0 ||
      hipMemsetAsync(s.tail, 0, tail_bytes, s.stream) != hipSuccess || hipStreamSynchronize(s.stream) != hipSuccess) {
    const std::string why = hipGetErrorString(hipGetLastError());
    free_slot(s);
    return fail(MPMPC_E_HIP, "allocation of a launch slot failed (stream / output block / tail lists / tail flag): " + why);
  }
  s.tail_flag[0] = s.tail_flag[1] = 0u;
  return MPMPC_OK;
}
// launch slots up to `want`, in slot order (and so are their streams), laid out like the ones there are
static int grow_slots(mpmpc_handle h, int want) {
  for (; h->n_slots < want; ++h->n_slots)
    if (int rc = alloc_slot(h, h->slot[h->n_slots])) return rc;
  lay_out(h, h->io.laid_out ? h->io.laid_out : h->cfg.max_batch);
  return MPMPC_OK;
}

int mpmpc_destroy(mpmpc_handle h) {
  if (!h) return MPMPC_OK;
  (void)hipSetDevice(h->cfg.device);
  // events and streams by hand (the slots' buffers go before their streams: free_slot); every buffer has its owner
  for (auto& s : h->slot) free_slot(s);
  for (hipEvent_t e : {h->ev_order, h->io.ev_bounce[0], h->io.ev_bounce[1], h->ev[0], h->ev[1], h->ev[2], h->io.ev_in})
    if (e) (void)hipEventDestroy(e);
  delete h;
  return MPMPC_OK;
}

int mpmpc_create(const mpmpc_config* cfg, const mpmpc_settings* settings, mpmpc_handle* out) {
  if (!cfg || !out) return fail(MPMPC_E_ARG, "cfg/out is NULL");
  *out = nullptr;
  if (cfg->N < 3 || cfg->N > MPMPC_MAX_HORIZON)
    return fail(MPMPC_E_ARG, "horizon N must satisfy 3 <= N <= " + std::to_string(MPMPC_MAX_HORIZON));
  if (cfg->max_batch < 1) return fail(MPMPC_E_ARG, "max_batch must be >= 1");
  if (!(cfg->wheelbase > 0)) return fail(MPMPC_E_ARG, "wheelbase must be > 0");
  for (int i = 0; i < 3; ++i)
    if (!(cfg->Q[i] >= 0) || !(cfg->QN[i] >= 0)) return fail(MPMPC_E_ARG, "Q, QN diagonals must be >= 0");
  {
    // Q, QN positive semidefinite: principal minors of the symmetric 3 x 3 (with a rounding allowance)
    auto psd3 = [](const double* dg, const double* od) {
      const double a = dg[0], b = dg[1], c = dg[2], d = od[0], e = od[1], f = od[2];
      if (!std::isfinite(d) || !std::isfinite(e) || !std::isfinite(f)) return false;
      const double tol = 1e-12 * (1.0 + a * a + b * b + c * c);
      const double m2a = a * b - d * d, m2b = a * c - e * e, m2c = b * c - f * f;
      const double det = a * (b * c - f * f) - d * (d * c - f * e) + e * (d * f - b * e);
      return !(m2a < -tol || m2b < -tol || m2c < -tol || det < -tol * (1.0 + a + b + c));
    };
    if (!psd3(cfg->QN, cfg->QN_offdiag)) return fail(MPMPC_E_ARG, "QN must be finite and positive semidefinite");
    if (!psd3(cfg->Q, cfg->Q_offdiag)) return fail(MPMPC_E_ARG, "Q must be finite and positive semidefinite");
    const double r = cfg->R_offdiag[0];
    if (!std::isfinite(r) || cfg->R[0] * cfg->R[1] - r * r < -1e-12 * (1.0 + cfg->R[0] * cfg->R[0] + cfg->R[1] * cfg->R[1]))
      return fail(MPMPC_E_ARG, "R must be finite and positive semidefinite");
  }
  for (int i = 0; i < 2; ++i) {
    if (!(cfg->R[i] >= 0)) return fail(MPMPC_E_ARG, "R diagonal must be >= 0");
    if (!std::isfinite(cfg->umin[i]) || !std::isfinite(cfg->umax[i]) || cfg->umin[i] > cfg->umax[i])
      return fail(MPMPC_E_ARG, "input bounds must be finite with umin <= umax");
  }
  mpmpc_settings st;
  if (settings) st = *settings; else mpmpc_default_settings(&st);
  if (int rc = check_settings(&st)) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev)
    return fail(MPMPC_E_HIP, "no such HIP device (this library has no CPU fallback)");
  HIP_TRY(hipSetDevice(cfg->device));
  mpmpc_handle h = new (std::nothrow) mpmpc_handle_s();
  if (!h) return fail(MPMPC_E_STATE, "out of host memory");
  h->cfg = *cfg;
  h->st = st;
  h->ld = host_stage_ld(cfg->N);
  h->n = 5 * cfg->N + 3;
  h->m = 8 * cfg->N + 6;
  h->pipeline = launch_streams(h->pipeline);
  const size_t B = (size_t)cfg->max_batch;
  // Slot 0 comes first, and its stream first of it: everything below that touches the device goes to that stream (alloc_slot).
  // (the further launch slots of pipelined resident launches are allocated by the first such launch: next_slot)
  if (int rc = alloc_slot(h, h->slot[0])) {
    mpmpc_destroy(h);
    return rc;
  }
  h->n_slots = 1;
  hipError_t e = hipSuccess;
  for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&h->ev[i]);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->io.ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming);
  if (e != hipSuccess) {
    mpmpc_destroy(h);
    return fail(MPMPC_E_HIP, std::string("event creation: ") + hipGetErrorString(e));
  }
  const BlockLayout lay = block_layout(cfg->N, cfg->max_batch);
  int ea = h->io.in_block.alloc(lay.in_end);
  if (!ea) ea = h->io.qp.alloc((size_t)MPMPC_NUM_FIELDS * B * h->ld);
  if (ea) {
    const std::string what = h->io.in_block ? "hipMalloc h->qp: " : "hipMalloc h->in_block: ";
    mpmpc_destroy(h);
    return fail(MPMPC_E_HIP, what + hipGetErrorString(static_cast<hipError_t>(ea)));
  }
  lay_out(h, cfg->max_batch);
  // (staging blocks up to STAGE_LIMIT bytes; a handle whose blocks could not be had works without them)
  const size_t STAGE_LIMIT = 64u << 20;
  if (lay.in_end <= STAGE_LIMIT) (void)h->io.stage_in.alloc(lay.in_end);
  if (lay.out_end <= STAGE_LIMIT) (void)h->io.stage_out.alloc(lay.out_end);
  *out = h;
  return MPMPC_OK;
}

int mpmpc_set_packing(mpmpc_handle h, int32_t lanes_per_instance) {
  if (int rc = enter(h)) return rc;
  if (!packing_valid(h->cfg.N, lanes_per_instance))
    return fail(MPMPC_E_ARG, "lanes_per_instance must be 0 (auto) or 16, 32, 64 and hold the N + 1 stages of an instance - half of them at 16 / 64, two stages "
                             "per lane - or 128 / 256: the workgroup kernels of horizons 64 .. 255");
  h->force_lanes = lanes_per_instance;
  return MPMPC_OK;
}

int mpmpc_set_tail_kernel(mpmpc_handle h, int32_t reduced_native) {
  if (int rc = enter(h)) return rc;
  if (reduced_native < 0 || reduced_native > 2) return fail(MPMPC_E_ARG, "reduced_native must be 0, 1 or 2");
  h->lean_tail = reduced_native != 0;
  h->lean_tail_single = reduced_native == 2;
  return MPMPC_OK;
}

int mpmpc_set_settings(mpmpc_handle h, const mpmpc_settings* settings) {
  if (int rc = enter(h)) return rc;
  if (int rc = check_settings(settings)) return rc;
  h->st = *settings;
  return MPMPC_OK;
}

// (frees and allocates on every call: a table is as long as its path)
static int upload_table(mpmpc_handle h, Buf<double>& dst, const double* src, size_t count) {
  HIP_TRY(dst.alloc(count));
  HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyHostToDevice, h->last().stream));
  return MPMPC_OK;
}

int mpmpc_set_path(mpmpc_handle h, int32_t n_wp, const double* kappa, const double* v_ref, const double* ds_next) {
  if (int rc = enter(h, kappa && v_ref && ds_next)) return rc;
  if (n_wp < 2) return fail(MPMPC_E_ARG, "need at least 2 waypoints");
  for (int i = 0; i < n_wp; ++i)
    if (!(v_ref[i] > 0) || !std::isfinite(kappa[i]) || !(ds_next[i] >= 0))
      return fail(MPMPC_E_ARG, "path table: need v_ref > 0, finite kappa, ds_next >= 0");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int cols = h->tab.n_wp == n_wp ? h->tab.n_cols : 0;   // a corridor table of another path is void
  h->tab.n_wp = h->tab.n_cols = 0;      // a failure below leaves "no path set", not tables of mixed lengths
  h->tab.routes.clear();                // routes belong to the path they were set on
  if (int rc = upload_table(h, h->tab.kappa, kappa, n_wp)) return rc;
  if (int rc = upload_table(h, h->tab.v_ref, v_ref, n_wp)) return rc;
  if (int rc = upload_table(h, h->tab.ds_next, ds_next, n_wp)) return rc;
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  h->tab.n_wp = n_wp;
  h->tab.n_cols = cols;
  ++h->cor.base_gen;
  return MPMPC_OK;
}

int mpmpc_set_corridor(mpmpc_handle h, int32_t n_wp, int32_t n_cols, const double* ub, const double* lb) {
  if (int rc = enter(h, ub && lb)) return rc;
  if (h->tab.n_wp == 0 || n_wp != h->tab.n_wp) return fail(MPMPC_E_STATE, "set the path first; n_wp must match it");
  if (n_cols < h->cfg.N) return fail(MPMPC_E_ARG, "corridor table needs n_cols >= N");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (int rc = upload_table(h, h->tab.ub_tab, ub, (size_t)n_wp * n_cols)) return rc;
  if (int rc = upload_table(h, h->tab.lb_tab, lb, (size_t)n_wp * n_cols)) return rc;
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  h->tab.n_cols = n_cols;
  return MPMPC_OK;
}

// The routes change.  A corridor table that mpmpc_build_corridor made walked its horizons under the old ones (or the one path):
// it is void - the solves then ask for a table instead of reading rows that cross a route's end.  (built_gen != 0: a build has
// succeeded on this handle, whatever mpmpc_set_map / _set_path_geometry did to the generation since; a table that
// mpmpc_set_corridor gave AFTER a build goes too - the safe side: the caller gives it again.)  And the batch on the device was
// checked against the old routes: its local wp_id may lie outside the new ones, so it has to be uploaded again.
static void routes_change(mpmpc_handle h) {
  if (h->cor.built_gen != 0) h->tab.n_cols = 0;
  ++h->cor.base_gen;
  h->io.uploaded = 0;
  h->ro.valid = false;
}

// ---- Route fleets: the path table as the concatenation of P routes, every instance on one of them (the law: include/mpmpc.h;
// the state and every check on it: route_state.hpp - host only, tests/emul_routes drives it without a device).
int mpmpc_check_routes(int32_t n_wp, int32_t P, const int32_t* first, const int32_t* circular) {
  const char* why = "";
  if (int rc = RouteState::check(n_wp, P, first, circular, &why)) return fail(rc, why);
  return MPMPC_OK;
}

int mpmpc_set_routes(mpmpc_handle h, int32_t P, const int32_t* first, const int32_t* circular) {
  if (int rc = enter(h)) return rc;
  const char* why = "";
  bool changed = false;
  const int rc = h->tab.routes.set_routes(h->tab.n_wp, P, first, circular, &changed, &why);
  if (changed) routes_change(h);
  return rc ? fail(rc, why) : MPMPC_OK;
}

int mpmpc_set_car_routes(mpmpc_handle h, int32_t B, const int32_t* route) {
  if (int rc = enter(h, route)) return rc;
  TabState& t = h->tab;
  const char* why = "";
  std::vector<int32_t> hdr;
  if (int rc = t.routes.car_headers(h->cfg.max_batch, B, route, &hdr, &why)) return fail(rc, why);
  HIP_TRY(hipSetDevice(h->cfg.device));
  t.routes.car_B = 0;      // a failure below leaves "not given"
  // The batch on the device was checked against the routes its cars had (check_wp_ids): re-dealt, a local wp_id may lie past
  // its new route's end - the corridor row first + wp would be read out of bounds - so it is to be uploaded again.
  h->io.uploaded = 0;
  h->ro.valid = false;
  // (the one header array is safe to overwrite here: `enter` has drained every other slot with launches in flight, and what the
  //  last slot's stream still has queued is ordered in front of this copy)
  if (!t.car_hdr) HIP_TRY(t.car_hdr.alloc(2 * (size_t)h->cfg.max_batch));
  HIP_TRY(hipMemcpyAsync(t.car_hdr, hdr.data(), hdr.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));      // `hdr` leaves scope
  t.routes.keep_car_routes(B, route);
  return MPMPC_OK;
}

}  // extern "C"

static int check_car_routes(mpmpc_handle h, int B) {
  const char* why = "";
  if (int rc = h->tab.routes.check_batch(B, &why)) return fail(rc, why);
  return MPMPC_OK;
}
static int check_wp_ids(mpmpc_handle h, int B, const int32_t* wp_id) {
  const char* why = "";
  if (int rc = h->tab.routes.check_wp_ids(B, wp_id, h->cfg.N, h->tab.n_wp, h->cfg.circular != 0, &why)) return fail(rc, why);
  return MPMPC_OK;
}
// (the kernels of the two keep their order in the code object: K4, then K0 / K3 and the recorder)
#include "mpmpc_speed_profile.hpp"
#include "mpmpc_walls.hpp"
#include "mpmpc_plant.hpp"
#include "mpmpc_delay.hpp"
#include "mpmpc_dynamics.hpp"
#include "mpmpc_estimator.hpp"
#include "mpmpc_localiser.hpp"
#include "mpmpc_commitment.hpp"
#include "mpmpc_closed_loop.hpp"
#include "mpmpc_lookahead.hpp"
#include "mpmpc_lidar.hpp"
#include "mpmpc_path.hpp"
#include "mpmpc_perception.hpp"
#include "mpmpc_footprint.hpp"
#include "mpmpc_rollout_step.hpp"      // (behind every feature a step drives)
#include "mpmpc_project.hpp"

extern "C" {

int mpmpc_upload(mpmpc_handle h, int32_t B, const int32_t* wp_id, const double* x0, const double* cc_prev,
                 const double* lb, const double* ub) {
  if (int rc = enter(h, wp_id && x0 && cc_prev)) return rc;
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (h->tab.n_wp == 0) return fail(MPMPC_E_STATE, "no path set (mpmpc_set_path)");
  if ((lb == nullptr) != (ub == nullptr)) return fail(MPMPC_E_ARG, "lb and ub must both be given or both NULL");
  if (!lb && h->tab.n_cols == 0) return fail(MPMPC_E_STATE, "no corridor rows given and no corridor table set");
  const int N = h->cfg.N;
  if (int rc = check_wp_ids(h, B, wp_id)) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  h->ro.valid = false;        // the batch blocks are about to be re-laid out and overwritten
  if (B != h->io.laid_out) lay_out(h, B);
  const BlockLayout L = block_layout(N, B);
  if (h->io.stage_in) {
    // through pinned staging: the batch is gathered in the device block's own layout and goes over in one copy.
    // The caller's buffers are free as soon as they are gathered, so nothing waits for the copy here - only the
    // NEXT upload does, before it overwrites the staging buffer.
    if (h->io.in_flight) HIP_TRY(hipEventSynchronize(h->io.ev_in));
    char* st = h->io.stage_in;
    std::memcpy(st + L.wp_id, wp_id, sizeof(int) * B);
    std::memcpy(st + L.x0, x0, sizeof(double) * 3 * B);
    std::memcpy(st + L.cc, cc_prev, sizeof(double) * 2 * N * B);
    if (lb) {
      std::memcpy(st + L.lb, lb, sizeof(double) * N * B);
      std::memcpy(st + L.ub, ub, sizeof(double) * N * B);
    }
    HIP_TRY(hipMemcpyAsync(h->io.in_block, st, lb ? L.in_end : L.in_end_cc, hipMemcpyHostToDevice, h->last().stream));
    HIP_TRY(hipEventRecord(h->io.ev_in, h->last().stream));
    h->io.in_flight = true;
  } else {
    // (no staging block of this size: through the bounce buffer - asynchronous on the device's side, the caller's buffers are
    //  free when the call returns)
    if (int rc = upload_through_bounce(h, h->io.wp_id, wp_id, sizeof(int) * B)) return rc;
    if (int rc = upload_through_bounce(h, h->io.x0, x0, sizeof(double) * 3 * B)) return rc;
    if (int rc = upload_through_bounce(h, h->io.cc, cc_prev, sizeof(double) * 2 * N * B)) return rc;
    if (lb) {
      if (int rc = upload_through_bounce(h, h->io.lb, lb, sizeof(double) * N * B)) return rc;
      if (int rc = upload_through_bounce(h, h->io.ub, ub, sizeof(double) * N * B)) return rc;
    }
  }
  h->io.have_rows = lb != nullptr;
  h->io.uploaded = B;
  return MPMPC_OK;
}

constexpr size_t BOUNCE_HALF = 8u << 20;
static int upload_through_bounce(mpmpc_handle h, void* dst, const void* src, size_t bytes) {
  if (!h->io.bounce) {
    HIP_TRY(h->io.bounce.alloc(2 * BOUNCE_HALF));
    for (auto& e : h->io.ev_bounce) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  for (size_t off = 0; off < bytes; off += BOUNCE_HALF) {
    const int k = h->io.bounce_turn;
    if (h->io.bounce_busy[k]) HIP_TRY(hipEventSynchronize(h->io.ev_bounce[k]));      // its last copy has left this half
    const size_t n = bytes - off < BOUNCE_HALF ? bytes - off : BOUNCE_HALF;
    char* half = h->io.bounce + (size_t)k * BOUNCE_HALF;
    std::memcpy(half, static_cast<const char*>(src) + off, n);
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + off, half, n, hipMemcpyHostToDevice, h->last().stream));
    HIP_TRY(hipEventRecord(h->io.ev_bounce[k], h->last().stream));
    h->io.bounce_busy[k] = true;
    h->io.bounce_turn = 1 - k;
  }
  return MPMPC_OK;
}

static int launch_assemble(mpmpc_handle h, int B) {
  if (int rc = check_car_routes(h, B)) return rc;
  const AssembleIn in = h->io.inputs(h->tab);
  const int total = B * h->ld;
  const int blocks = (total + K1_THREADS - 1) / K1_THREADS;
  // (tuning knob of profiles/k1_timing.py: MPMPC_K1_NT = 0 forces plain stores)
  static const int force_nt = std::getenv("MPMPC_K1_NT") ? std::atoi(std::getenv("MPMPC_K1_NT")) : -1;
  const bool nt = force_nt != 0;
  const size_t k1_lds = h->tab.n_wp <= K1_LDS_WP ? 3 * sizeof(double) * (size_t)h->tab.n_wp : 0;
#define K1_LAUNCH(V)                                                                                                       \
  hipLaunchKernelGGL(mpmpc_assemble_kernel<V>, dim3(blocks), dim3(K1_THREADS), k1_lds, h->last().stream, h->cfg, in.tab, B, h->ld, in.wp_id, \
                     in.x0, in.cc, in.lb, in.ub, h->io.qp.get())
  if (nt) K1_LAUNCH(true);
  else K1_LAUNCH(false);
#undef K1_LAUNCH
  HIP_TRY(hipGetLastError());
  return MPMPC_OK;
}

}  // extern "C"  (the dispatch functions below are templates)

// ---------------------------------------------------------------------------------------------------- launch dispatch
// What a solve launch hands to its kernels.  plan_solve (mpmpc_launch_plan.hpp) decides WHICH kernels run - policy: packing,
// warm start, tail solver, what may be deferred; `enqueue` below maps a stage of that plan to the launch of an instantiation,
// and run_stages enqueues the stages of the slot's plan in order, holding back what may be and need not run.
struct SolveLaunch {
  mpmpc_handle h;
  Slot* slot;      // the launch slot it goes to: stream, outputs, tail flag, tail lists by role
  SolverParams prm;
  AssembleIn ain;
  int B;
  double* y_out;
};
// THE launcher: every solve kernel starts with the same arguments - cfg, prm, B, [ld,] ain, z, u0, status, iters, resid, y - which
// come from the launch; `own` are the kernel's trailing ones.  (Whether the kernel takes ld is read off its parameter list.)
template <class... K>
constexpr bool takes_ld(void (*)(mpmpc_config, SolverParams, int, int, AssembleIn, K...)) { return true; }
template <class... K>
constexpr bool takes_ld(void (*)(mpmpc_config, SolverParams, int, AssembleIn, K...)) { return false; }
template <auto KERNEL, class... T>
static void go(const SolveLaunch& a, int grid, int block, size_t lds, T... own) {
  mpmpc_handle h = a.h;
  const Slot& s = *a.slot;
  if constexpr (takes_ld(KERNEL))
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), lds, s.stream, h->cfg, a.prm, a.B, h->ld, a.ain, s.z, s.u0, s.status, s.iters, s.resid,
                       a.y_out, own...);
  else
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), lds, s.stream, h->cfg, a.prm, a.B, a.ain, s.z, s.u0, s.status, s.iters, s.resid, a.y_out,
                       own...);
}
// The workgroup kernels need more dynamic LDS than the default limit: the attribute is set once per function AND DEVICE (one
// process may drive several - sharded.py, bench.py --single-process - and the attribute belongs to the function on the device
// that is current; two threads may both set it once: the call is idempotent).  A device ordinal beyond the table sets it
// every time.
constexpr int MAX_DEVICES = 64;
template <auto KERNEL>
static int raise_lds_limit(mpmpc_handle h, size_t bytes) {
  static std::atomic<bool> attr_set[MAX_DEVICES];
  const int d = h->cfg.device;
  const bool known = d >= 0 && d < MAX_DEVICES;
  if (!known || !attr_set[d]) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (known) attr_set[d] = true;
  }
  return MPMPC_OK;
}
// ... one instance per WORKGROUP
template <auto KERNEL, class... T>
static int go_workgroups(const SolveLaunch& a, const PlanStage& s, size_t lds, T... own) {
  if (int rc = raise_lds_limit<KERNEL>(a.h, lds)) return rc;
  go<KERNEL>(a, s.grid, s.block, lds, own...);
  return MPMPC_OK;
}
// (knob of the occupancy experiment, profiles/r3/occupancy.txt: MPMPC_RN_OCC=1 pads every block of the one-stage reduced-native
//  kernels with 20 KB of unused dynamic LDS - 40 KB per wave, four waves per CU, ONE per SIMD - so that the same code object can
//  be timed at one and at two waves per SIMD)
static int rn_pad() {
  static const int pad = (std::getenv("MPMPC_RN_OCC") && std::atoi(std::getenv("MPMPC_RN_OCC")) == 1) ? 20 * 1024 : 0;
  return pad;
}
// A run-time value as a template argument: f(std::integral_constant<int, v>) for the one of V... that equals v (false: none does)
template <int... V, class F>
static bool pick(int v, F&& f) {
  return ((v == V && f(std::integral_constant<int, V>{})) || ...);
}
// One stage of a plan -> the launch of its instantiation.  The instantiations named here are the solve kernels of the code
// object; a stage that names none of them is an error, never another kernel.
static int enqueue(const SolveLaunch& a, const PlanStage& s) {
  mpmpc_handle h = a.h;
  const Slot& sl = *a.slot;
  int *const reads = sl.list[s.reads], *const fills = sl.list[s.fills];      // (none: null)
  int *const next = sl.list[MPMPC_LIST_NEXT], *const left = sl.list[MPMPC_LIST_LEFT];
  int* const act = s.warm ? h->ro.act.get() : nullptr;
  const int* const shift = s.warm ? h->ro.shift.get() : nullptr;
  int rc = MPMPC_OK;
  bool found = false;
  switch (s.family) {
    case MPMPC_K_GENERAL:      // one instance per wave: the whole solve (mode 0) or the tail of a reduced-native launch (mode 2); empties `next`
      found = pick<16, 32>(s.C, [&](auto C) { return pick<0, 1>(s.warm, [&](auto W) { return pick<0, 1, 2, 3>(s.var, [&](auto V) {
        go<mpmpc_solve_kernel<64, C(), W() != 0, V()>>(a, s.grid, s.block, 0, s.mode, reads, act, shift, next);
        return true; }); }); });
      break;
    case MPMPC_K_REDUCED:      // K2r: the reduced-native batch kernel, 1 / 2 / 4 instances per wave
      found = pick<64, 32, 16>(s.G, [&](auto G) { return pick<16, 32>(s.C, [&](auto C) { return pick<0, 1>(s.warm, [&](auto W) {
        if constexpr (G() == 64 || C() == 16) {      // (chains split at 32 need the 64 lanes)
          go<mpmpc_reduced_kernel<G(), C(), W() != 0>>(a, s.grid, s.block, rn_pad(), fills, act, shift, next, sl.tail_flag.get(), sl.seq, left);
          return true;
        } else return false; }); }); });
      break;
    case MPMPC_K_REDUCED_T:      // K2t: its twin for a terminal cost on the time state (one instance per wave)
      found = s.G == 64 && pick<16, 32>(s.C, [&](auto C) {
        go<mpmpc_reduced_t_kernel<64, C()>>(a, s.grid, s.block, rn_pad(), fills, next, sl.tail_flag.get(), sl.seq);
        return true; });
      break;
    case MPMPC_K_REDUCED_TAIL:      // K2p: the reduced-native tail solver on the list it reads; what it leaves goes to the list it fills
      found = pick<64, 32>(s.G, [&](auto G) { return pick<16, 32>(s.C, [&](auto C) {
        if constexpr (G() == 64 || C() == 16) {
          go<mpmpc_reduced_tail_kernel<G(), C()>>(a, s.grid, s.block, rn_pad(), reads, next, fills, sl.tail_flag + 1, sl.seq);
          return true;
        } else return false; }); });
      break;
    case MPMPC_K_PAIR:      // K2r2 / K2t2 / K2p2: two stages per lane (lane_pair.hpp)
      found = pick<16, 64>(s.G, [&](auto G) {
        go<mpmpc_reduced_pair_kernel<G()>>(a, s.grid, s.block, 0, fills, next, sl.tail_flag.get(), sl.seq, left);
        return true; });
      break;
    case MPMPC_K_PAIR_T:
      if ((found = s.G == 64)) go<mpmpc_reduced_t_pair_kernel<64>>(a, s.grid, s.block, 0, fills);
      break;
    case MPMPC_K_PAIR_TAIL:
      if ((found = s.G == 64)) go<mpmpc_reduced_tail_pair_kernel<64>>(a, s.grid, s.block, 0, reads, fills);
      break;
    case MPMPC_K_BLOCK:      // K2b / K2rb and the pair kernels on a workgroup: one instance per WORKGROUP of 128 / 256 lanes
      found = pick<128, 256>(s.G, [&](auto G) { return pick<0, 1, 2>(s.var, [&](auto V) {
        rc = go_workgroups<mpmpc_solve_block_kernel<G(), V()>>(a, s, LaneBlock<G()>::lds_bytes, (const int*)reads);
        return true; }); });
      break;
    case MPMPC_K_RBLOCK:
      found = pick<128, 256>(s.G, [&](auto G) {
        rc = go_workgroups<mpmpc_reduced_block_kernel<G()>>(a, s, LaneBlock<G(), RNB_SLOTS>::lds_bytes, fills);
        return true; });
      break;
    case MPMPC_K_PAIR_BLOCK:
      if ((found = s.G == 128)) rc = go_workgroups<mpmpc_reduced_pair_block_kernel>(a, s, LanePairBlock::L1::lds_bytes, fills);
      break;
    case MPMPC_K_PAIR_BLOCK_TAIL:
      if ((found = s.G == 128)) rc = go_workgroups<mpmpc_reduced_tail_pair_block_kernel>(a, s, LanePairBlockFull::L1::lds_bytes, reads, fills);
      break;
    case MPMPC_K_PAIR_BLOCK_T:
      if ((found = s.G == 128)) rc = go_workgroups<mpmpc_reduced_t_pair_block_kernel>(a, s, LanePairBlockFull::L1::lds_bytes, fills);
      break;
  }
  if (!found) return fail(MPMPC_E_STATE, "no solve kernel for a stage of the launch plan");
  return rc;
}

// Enqueue the stages of the slot's plan from next_stage on.  A deferrable stage stops the run while the launches the host has
// SEEN left the list it reads empty (Slot: deferred tail) - `late`: not the stage the run starts at, which observe_tail has just
// found to be needed.  What is held back stays in the slot: next_stage.
static int run_stages(mpmpc_handle h, Slot& sl, bool late) {
  SolveLaunch a{};
  a.h = h;
  a.slot = &sl;
  a.B = sl.launch_B;
  a.prm = sl.prm;
  a.y_out = sl.want_y ? sl.y : nullptr;        // nobody wants the multipliers: the kernel skips their stores
  a.ain = h->io.inputs(h->tab);
  const int first = sl.next_stage, end = sl.plan.n;
  for (int i = first; i < end; ++i) {
    const PlanStage& s = sl.plan.stage[i];
    const bool forced = late && i == first;
    if (s.deferrable && !forced && (s.reads == MPMPC_LIST_THIS ? sl.tail_expect_empty : sl.tail2_expect_empty)) break;
    sl.next_stage = end;      // (an error below leaves nothing held back)
    if (s.clear) HIP_TRY(hipMemsetAsync(sl.list[s.fills], 0, sizeof(int), sl.stream));
    if (int rc = enqueue(a, s)) return rc;
    sl.next_stage = i + 1;
  }
  HIP_TRY(hipGetLastError());
  return MPMPC_OK;
}

// A solve launch on slot `sl`: plan it, bind the slot's lists to their roles, run the stages.
static int launch_solve(mpmpc_handle h, Slot& sl, int B, bool closed_loop, bool want_y, LaunchKind kind) {
  if (int rc = check_car_routes(h, B)) return rc;
  // (route fleets start every closed-loop solve cold: the warm-started instantiations are compiled without the route view -
  //  gather_stage<L, ROUTES = false> - so that they keep the registers they had)
  sl.y_valid = sl.want_y = want_y;
  sl.launch_B = B;
  sl.prm = make_params(h->st);
  sl.plan = plan_solve(h->cfg, h->st, LaunchKnobs{h->force_lanes, h->lean_tail, h->lean_tail_single, h->pipeline, h->tab.routes.n_routes ? 0 : h->ro.warm}, B, closed_loop, kind);
  sl.next_stage = 0;
  // tail lists ([0] = count, [1..] = instance ids), two of them used in turn: the tail launch of this step empties the
  // list of the next one, so that no memset has to sit between the launches of consecutive steps; the third is what the
  // reduced-native tail kernel leaves to the general one.  (Horizons above 63 never turn: the same three lists every launch.)
  const size_t stride = (size_t)h->cfg.max_batch + 1;
  sl.list[MPMPC_LIST_NONE] = nullptr;
  sl.list[MPMPC_LIST_THIS] = sl.tail + (size_t)sl.tail_flip * stride;
  sl.list[MPMPC_LIST_NEXT] = sl.tail + (size_t)(1 - sl.tail_flip) * stride;
  sl.list[MPMPC_LIST_LEFT] = sl.tail + 2 * stride;
  if (sl.plan.stage[0].turn) { sl.tail_flip = 1 - sl.tail_flip; sl.seq += 1; }
  return run_stages(h, sl, false);
}

extern "C" {

// Drain the slot's stream, see whether its last reduced-native launch left a tail, run the stages that were held back if it did.
// Two levels: a late tail solver is followed by the general kernel unless tail2_expect_empty says to hold that back too, and a
// general kernel held back on the tail solver's leftovers runs after the second stamp has been read.
static int observe_tail(mpmpc_handle h, Slot& sl) {
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  sl.busy = false;
  h->order_pending = false;
  if (sl.seq == 0) return MPMPC_OK;
  sl.tail_ran_late = false;
  // stages held back in front of a stage that reads `list`: dropped if the launch left that list empty, else run now
  auto resume = [&](int list, bool left) -> int {
    if (!sl.deferred() || sl.plan.stage[sl.next_stage].reads != list) return MPMPC_OK;
    if (!left) { sl.next_stage = sl.plan.n; return MPMPC_OK; }
    sl.tail_ran_late = true;
    if (int rc = run_stages(h, sl, true)) return rc;
    HIP_TRY(hipStreamSynchronize(sl.stream));
    return MPMPC_OK;
  };
  const bool left = *static_cast<volatile unsigned*>(sl.tail_flag.get()) == sl.seq;
  if (int rc = resume(MPMPC_LIST_THIS, left)) return rc;
  sl.tail_expect_empty = !left;
  // (second level: read after a tail that ran late has run)
  const bool left2 = static_cast<volatile unsigned*>(sl.tail_flag.get())[1] == sl.seq;
  if (int rc = resume(MPMPC_LIST_LEFT, left2)) return rc;
  sl.tail2_expect_empty = !left2;
  return MPMPC_OK;
}

// Resident launches are PIPELINED over the `pipeline` launch slots in use: launch k + 1 goes to the next slot (stream, output
// block, tail lists) and runs beside launch k - a batch launch fills one of the two wave slots of a SIMD (B <= 1 024) or leaves
// SIMDs idle while its last waves and its tail launch run, and the next batches take what is idle.  The results of launch k stay
// where they are until launch k + pipeline; mpmpc_download / mpmpc_sync and every other call on the handle refer to the LAST
// launch and wait for all of them.
// next_slot makes the next slot of the ring "the slot of the last launch": cur -> (cur + 1) % pipeline, which from slot 0 takes
// the launches through slots 1, 2, .., pipeline - 1, 0, ..  That is also the whole rule after mpmpc_set_pipeline (which has
// settled every slot): the ring goes on from wherever `cur` is.  If that is a slot the new ring no longer holds, the next launch
// goes to (cur + 1) % pipeline all the same, and the slot left behind is not launched on again until a deeper ring reaches it.
// At depth 1 `cur` stays: every launch on the one stream.  What the stream of the last launch still has queued that solves read (an upload, closed-loop steps) must be
// done before ANY slot's next launch starts: an event goes to the streams of all slots in use.  Shared by mpmpc_solve_resident
// and mpmpc_solve_resident_profile (the profile loop used to change slots without it, so an upload followed by it
// could be overtaken).  The further slots are allocated on first use: a handle that never launches resident batches (single
// calls, host-buffer streams, the closed loop) holds one output block, not three.
static int next_slot(mpmpc_handle h) {
  if (h->pipeline > 1) {
    if (h->n_slots < h->pipeline) {
      if (int rc = grow_slots(h, h->pipeline)) return rc;
    }
    const bool order = h->order_pending;
    if (order) HIP_TRY(hipEventRecord(h->ev_order, h->last().stream));
    h->cur = (h->cur + 1) % h->pipeline;
    if (order)
      for (int i = 0; i < h->pipeline; ++i) HIP_TRY(hipStreamWaitEvent(h->slot[i].stream, h->ev_order, 0));
    h->order_pending = false;
  }
  h->last().busy = true;
  return MPMPC_OK;
}

int mpmpc_solve_resident(mpmpc_handle h, int32_t B) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (h->io.staged_bytes) {
    if (int rc = mpmpc_staged_end(h)) return rc;
  }
  if (B < 1 || B > h->io.uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (int rc = next_slot(h)) return rc;
  return launch_solve(h, h->last(), B, false, h->resident_y, LAUNCH_PIPELINED);      // one launch: the assembly runs inside K2
}

int mpmpc_set_pipeline(mpmpc_handle h, int32_t depth) {
  if (int rc = enter(h)) return rc;
  if (depth < 1 || depth > mpmpc_handle_s::MAX_PIPELINE) return fail(MPMPC_E_ARG, "pipeline depth must be in [1, 8]");
  h->pipeline = launch_streams(depth);      // as many launch slots as the process has hardware queues for, at most (the ring: next_slot)
  return MPMPC_OK;
}

int mpmpc_set_outputs(mpmpc_handle h, int32_t want_y) {
  if (int rc = enter(h)) return rc;
  h->resident_y = want_y != 0;
  return MPMPC_OK;
}

int mpmpc_solve_resident_timed(mpmpc_handle h, int32_t B, float* ms_assemble, float* ms_solve) {
  if (int rc = enter(h)) return rc;          // (a timed launch runs alone: nothing of an earlier launch is left on the chip)
  Slot& sl = h->last();
  if (B < 1 || B > h->io.uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(hipEventRecord(h->ev[0], sl.stream));
  if (int rc = launch_assemble(h, B)) return rc;
  HIP_TRY(hipEventRecord(h->ev[1], sl.stream));
  if (int rc = launch_solve(h, sl, B, false, h->resident_y)) return rc;
  HIP_TRY(hipEventRecord(h->ev[2], sl.stream));
  HIP_TRY(hipEventSynchronize(h->ev[2]));
  float a = 0.f, s = 0.f;
  HIP_TRY(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIP_TRY(hipEventElapsedTime(&s, h->ev[1], h->ev[2]));
  // a deferred tail this launch turns out to need runs now, and its time counts
  HIP_TRY(hipEventRecord(h->ev[1], sl.stream));
  if (int rc = observe_tail(h, sl)) return rc;
  if (sl.tail_ran_late) {
    HIP_TRY(hipEventRecord(h->ev[2], sl.stream));
    HIP_TRY(hipEventSynchronize(h->ev[2]));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, h->ev[1], h->ev[2]));
    s += t;
  }
  if (ms_assemble) *ms_assemble = a;
  if (ms_solve) *ms_solve = s;
  return MPMPC_OK;
}

// n resident launches exactly as mpmpc_solve_resident issues them (pipelined unless mpmpc_set_pipeline(h, 1)), each
// bracketed by HIP events on the stream it goes to: ms_each[i] = duration of launch i (its kernels, with whatever else is on
// the chip beside it - the other slots' launches), *ms_span = first start to last end.  For bench.py's roofline line: rocprofv3's
// per-kernel durations of the same loop must agree with ms_each.
int mpmpc_solve_resident_profile(mpmpc_handle h, int32_t B, int32_t n, float* ms_each, float* ms_span) {
  if (!h || !ms_each) return fail(MPMPC_E_ARG, "NULL argument");
  if (n < 1 || n > 4096) return fail(MPMPC_E_ARG, "n must be in [1, 4096]");
  if (int rc = settle(h)) return rc;
  if (B < 1 || B > h->io.uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
  HIP_TRY(hipSetDevice(h->cfg.device));
  std::vector<hipEvent_t> ev(2 * (size_t)n, nullptr);
  int rc = MPMPC_OK;
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) { rc = fail(MPMPC_E_HIP, "hipEventCreate"); break; }
  for (int i = 0; i < n && rc == MPMPC_OK; ++i) {
    if ((rc = next_slot(h)) != MPMPC_OK) break;
    Slot& sl = h->last();
    if (hipEventRecord(ev[2 * i], sl.stream) != hipSuccess) { rc = fail(MPMPC_E_HIP, "hipEventRecord"); break; }
    rc = launch_solve(h, sl, B, false, h->resident_y, LAUNCH_PIPELINED);
    if (rc == MPMPC_OK && hipEventRecord(ev[2 * i + 1], sl.stream) != hipSuccess) rc = fail(MPMPC_E_HIP, "hipEventRecord");
  }
  if (rc == MPMPC_OK) rc = drain(h);
  if (rc == MPMPC_OK) {
    for (int i = 0; i < n; ++i)
      if (hipEventElapsedTime(&ms_each[i], ev[2 * i], ev[2 * i + 1]) != hipSuccess) { rc = fail(MPMPC_E_HIP, "hipEventElapsedTime"); break; }
    if (rc == MPMPC_OK && ms_span) {
      // (the last END is the later of the last two launches' - they run side by side)
      float last = 0.f;
      for (int i = n - 1; i >= 0 && i >= n - h->pipeline; --i) {
        float a = 0.f;
        (void)hipEventElapsedTime(&a, ev[0], ev[2 * i + 1]);
        if (a > last) last = a;
      }
      *ms_span = last;
    }
  }
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

int mpmpc_assemble_resident_timed(mpmpc_handle h, int32_t B, int32_t n, float* ms_each) {
  if (!h || !ms_each) return fail(MPMPC_E_ARG, "NULL argument");
  if (n < 1 || n > 4096) return fail(MPMPC_E_ARG, "n must be in [1, 4096]");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->io.uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
  HIP_TRY(hipSetDevice(h->cfg.device));
  std::vector<hipEvent_t> ev((size_t)n + 1, nullptr);
  int rc = MPMPC_OK;
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) { rc = fail(MPMPC_E_HIP, "hipEventCreate"); break; }
  if (rc == MPMPC_OK && hipEventRecord(ev[0], sl.stream) != hipSuccess) rc = fail(MPMPC_E_HIP, "hipEventRecord");
  for (int i = 0; i < n && rc == MPMPC_OK; ++i) {
    rc = launch_assemble(h, B);
    if (rc == MPMPC_OK && hipEventRecord(ev[i + 1], sl.stream) != hipSuccess) rc = fail(MPMPC_E_HIP, "hipEventRecord");
  }
  if (rc == MPMPC_OK && hipStreamSynchronize(sl.stream) != hipSuccess) rc = fail(MPMPC_E_HIP, "hipStreamSynchronize");
  for (int i = 0; i < n && rc == MPMPC_OK; ++i)
    if (hipEventElapsedTime(&ms_each[i], ev[i], ev[i + 1]) != hipSuccess) rc = fail(MPMPC_E_HIP, "hipEventElapsedTime");
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

int mpmpc_sync(mpmpc_handle h) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (h->io.staged_bytes) return mpmpc_staged_end(h);
  return drain(h);
}

int mpmpc_download(mpmpc_handle h, int32_t B, double* z, double* u0, int32_t* status, int32_t* iters,
                   double* resid, double* y) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = mpmpc_staged_end(h)) return rc;    // (of a staged call that was begun, if any)
  if (int rc = drain(h)) return rc;               // (also how the single-call path learns that its launches leave no tail)
  Slot& sl = h->last();
  if (B < 1 || B > h->io.uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
  if (y && !sl.y_valid)
    return fail(MPMPC_E_STATE, "the last solve launch did not store the multipliers (mpmpc_set_outputs(h, 0) / closed loop)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (h->io.stage_out && B == h->io.laid_out) {
    // the whole batch was laid out for this B: one copy of the output block (without y, z when they are not wanted)
    const BlockLayout L = block_layout(h->cfg.N, B);
    char* st = h->io.stage_out;
    HIP_TRY(hipMemcpyAsync(st, sl.out_block, y ? L.out_end : (z ? L.out_end_z : L.z), hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
    if (z) std::memcpy(z, st + L.z, sizeof(double) * h->n * B);
    if (u0) std::memcpy(u0, st + L.u0, sizeof(double) * 2 * B);
    if (status) std::memcpy(status, st + L.status, sizeof(int) * B);
    if (iters) std::memcpy(iters, st + L.iters, sizeof(int) * 2 * B);
    if (resid) std::memcpy(resid, st + L.resid, sizeof(double) * 2 * B);
    if (y) std::memcpy(y, st + L.y, sizeof(double) * h->m * B);
    return MPMPC_OK;
  }
  struct Pull { void* user; const char* staged; size_t bytes; } pulls[6];
  int np = 0;
  char* stage = h->io.stage_out;
  auto pull = [&](void* user, const void* dev, size_t bytes) -> hipError_t {
    if (!user) return hipSuccess;
    void* to = user;
    if (stage) { to = stage; pulls[np++] = Pull{user, stage, bytes}; stage += (bytes + 7) & ~size_t(7); }
    return hipMemcpyAsync(to, dev, bytes, hipMemcpyDeviceToHost, sl.stream);
  };
  HIP_TRY(pull(z, sl.z, sizeof(double) * h->n * B));
  HIP_TRY(pull(u0, sl.u0, sizeof(double) * 2 * B));
  HIP_TRY(pull(status, sl.status, sizeof(int) * B));
  HIP_TRY(pull(iters, sl.iters, sizeof(int) * 2 * B));
  HIP_TRY(pull(resid, sl.resid, sizeof(double) * 2 * B));
  HIP_TRY(pull(y, sl.y, sizeof(double) * h->m * B));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  for (int i = 0; i < np; ++i) std::memcpy(pulls[i].user, pulls[i].staged, pulls[i].bytes);
  return MPMPC_OK;
}

// ---- zero-copy host path: the caller works in the handle's own page-locked staging blocks
int mpmpc_staging(mpmpc_handle h, int32_t B, int32_t** wp_id, double** x0, double** cc_prev, double** lb, double** ub,
                  double** z, double** u0, int32_t** status, int32_t** iters, double** resid, double** y) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (!h->io.stage_in || !h->io.stage_out) return fail(MPMPC_E_STATE, "this handle has no staging blocks (max_batch above the staging limit)");
  // The blocks are the ones mpmpc_upload / mpmpc_download stage through: an upload still on its way out of the input block
  // must have left it before the caller may write there, and a begun staged call owns both blocks
  if (int rc = settle(h)) return rc;
  if (h->io.in_flight) { HIP_TRY(hipEventSynchronize(h->io.ev_in)); h->io.in_flight = false; }
  const BlockLayout L = block_layout(h->cfg.N, B);
  char *si = h->io.stage_in, *so = h->io.stage_out;
  if (wp_id) *wp_id = reinterpret_cast<int32_t*>(si + L.wp_id);
  if (x0) *x0 = reinterpret_cast<double*>(si + L.x0);
  if (cc_prev) *cc_prev = reinterpret_cast<double*>(si + L.cc);
  if (lb) *lb = reinterpret_cast<double*>(si + L.lb);
  if (ub) *ub = reinterpret_cast<double*>(si + L.ub);
  if (u0) *u0 = reinterpret_cast<double*>(so + L.u0);
  if (resid) *resid = reinterpret_cast<double*>(so + L.resid);
  if (status) *status = reinterpret_cast<int32_t*>(so + L.status);
  if (iters) *iters = reinterpret_cast<int32_t*>(so + L.iters);
  if (z) *z = reinterpret_cast<double*>(so + L.z);
  if (y) *y = reinterpret_cast<double*>(so + L.y);
  return MPMPC_OK;
}

int mpmpc_staged_end(mpmpc_handle h) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (!h->io.staged_bytes) return MPMPC_OK;
  const size_t out_bytes = h->io.staged_bytes;
  Slot& sl = h->last();
  if (int rc = drain(h)) return rc;                 // drains the streams; a launch that left a deferred tail has it run now
  h->io.staged_bytes = 0;                              // (only now: an error above leaves the call begun)
  if (sl.tail_ran_late) {
    HIP_TRY(hipMemcpyAsync(h->io.stage_out, sl.out_block, out_bytes, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
  }
  return MPMPC_OK;
}

int mpmpc_solve_staged(mpmpc_handle h, int32_t B, int32_t with_rows, int32_t want_z, int32_t want_y) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  h->io.staged_async = false;          // one call, waited for at once: the packing of a single launch
  const int rc = mpmpc_staged_begin(h, B, with_rows, want_z, want_y);
  h->io.staged_async = true;
  if (rc) return rc;
  return mpmpc_staged_end(h);
}

int mpmpc_staged_begin(mpmpc_handle h, int32_t B, int32_t with_rows, int32_t want_z, int32_t want_y) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (h->io.staged_bytes) return fail(MPMPC_E_STATE, "mpmpc_staged_begin: the previous one has not been ended");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (!h->io.stage_in || !h->io.stage_out) return fail(MPMPC_E_STATE, "this handle has no staging blocks (max_batch above the staging limit)");
  if (h->tab.n_wp == 0) return fail(MPMPC_E_STATE, "no path set (mpmpc_set_path)");
  if (!with_rows && h->tab.n_cols == 0) return fail(MPMPC_E_STATE, "no corridor rows given and no corridor table set");
  const int N = h->cfg.N;
  const BlockLayout L = block_layout(N, B);
  const int32_t* wp = reinterpret_cast<const int32_t*>(h->io.stage_in + L.wp_id);
  if (int rc = check_wp_ids(h, B, wp)) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (h->io.in_flight) { HIP_TRY(hipEventSynchronize(h->io.ev_in)); h->io.in_flight = false; }
  h->ro.valid = false;
  if (B != h->io.laid_out) lay_out(h, B);
  HIP_TRY(hipMemcpyAsync(h->io.in_block, h->io.stage_in, with_rows ? L.in_end : L.in_end_cc, hipMemcpyHostToDevice, sl.stream));
  h->io.have_rows = with_rows != 0;
  h->io.uploaded = B;
  if (int rc = launch_solve(h, sl, B, false, want_y != 0, h->io.staged_async ? LAUNCH_PIPELINED : LAUNCH_SINGLE)) return rc;
  const size_t out_bytes = want_y ? L.out_end : (want_z ? L.out_end_z : L.z);
  HIP_TRY(hipMemcpyAsync(h->io.stage_out, sl.out_block, out_bytes, hipMemcpyDeviceToHost, sl.stream));
  h->io.staged_bytes = out_bytes;
  return MPMPC_OK;
}

int mpmpc_assemble(mpmpc_handle h, int32_t B, const int32_t* wp_id, const double* x0, const double* cc_prev,
                   const double* lb, const double* ub, double* qp_out) {
  if (int rc = mpmpc_upload(h, B, wp_id, x0, cc_prev, lb, ub)) return rc;
  if (int rc = launch_assemble(h, B)) return rc;
  if (qp_out) {
    // device layout is [field][B][ld]; rows of B*ld doubles per field are contiguous
    HIP_TRY(hipMemcpyAsync(qp_out, h->io.qp, sizeof(double) * MPMPC_NUM_FIELDS * (size_t)B * h->ld,
                           hipMemcpyDeviceToHost, h->last().stream));
  }
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  return MPMPC_OK;
}

int mpmpc_solve(mpmpc_handle h, int32_t B, const int32_t* wp_id, const double* x0, const double* cc_prev,
                const double* lb, const double* ub, double* z, double* u0, int32_t* status, int32_t* iters,
                double* resid, double* y) {
  if (int rc = mpmpc_upload(h, B, wp_id, x0, cc_prev, lb, ub)) return rc;
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (int rc = launch_solve(h, h->last(), B, false, y != nullptr)) return rc;      // no y asked for: none stored
  return mpmpc_download(h, B, z, u0, status, iters, resid, y);
}

}  // extern "C"

#ifdef MPMPC_PHASE_CLOCK
extern "C" int mpmpc_debug_phase(long long* out, int reset) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(long long) * 4096 * 32) != hipSuccess) return -1;
  if (reset) {
    static long long zeros[4096 * 32];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), zeros, sizeof(zeros)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
