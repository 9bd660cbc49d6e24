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
//   K0 / K3 / K4                corridor tables from the map, closed-loop rollout, speed profile (see below).
//
// No CPU path exists in this library: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
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
#include "speed_core.hpp"

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

template <class L>
MPMPC_HD void assemble_in(const mpmpc_config& cfg, const AssembleIn& ain, int B, const typename L::ival& inst,
                          const typename L::ival& k, typename L::real* fields) {
  assemble_fields<L>(cfg, ain.tab, B, inst, k, ain.wp_id, ain.x0, ain.cc, ain.lb, ain.ub, fields);
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
  assemble_in<L>(cfg, ain, B, inst, k, fields);
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
  assemble_in<L>(cfg, ain, B, inst, k, fields);
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

// K4: speed profile.  The kernel of choice is mpmpc_speed_profile_wave_kernel below (one wavefront per path); these
// two run the same code one thread per path (a serial interior-point / active-set run over a scalar tridiagonal
// system, speed_core.hpp) for paths too long for the LDS: workspace path-minor in HBM, so that the threads of a
// wave touch consecutive addresses, or in LDS for a few paths.
__global__ __launch_bounds__(64) void mpmpc_speed_profile_kernel(int B, int n, const double* __restrict__ li,
                                                                 const double* __restrict__ kappa,
                                                                 const double* __restrict__ limits, double eps,
                                                                 double* __restrict__ work, double* __restrict__ v,
                                                                 int* __restrict__ status, int* __restrict__ iters) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= B) return;
  SpWork W{work + p, n, B};
  SpLimits lim{limits[5 * p], limits[5 * p + 1], limits[5 * p + 2], limits[5 * p + 3], limits[5 * p + 4]};
  int it = 0;
  status[p] = sp_solve(n, li + (long)p * n, kappa + (long)p * n, 1, lim, eps, W, v + (long)p * n, 1, &it);
  iters[p] = it;
}

// Few paths (the usual case is one): one path per block with the workspace in LDS, so that the serial
// run is bound by LDS latency instead of HBM latency.
__global__ __launch_bounds__(64) void mpmpc_speed_profile_lds_kernel(int B, int n, const double* __restrict__ li,
                                                                     const double* __restrict__ kappa,
                                                                     const double* __restrict__ limits, double eps,
                                                                     double* __restrict__ v, int* __restrict__ status,
                                                                     int* __restrict__ iters) {
  extern __shared__ double sp_lds[];
  const int p = blockIdx.x;
  if (threadIdx.x != 0 || p >= B) return;
  SpWork W{sp_lds, n, 1};
  SpLimits lim{limits[5 * p], limits[5 * p + 1], limits[5 * p + 2], limits[5 * p + 3], limits[5 * p + 4]};
  int it = 0;
  status[p] = sp_solve(n, li + (long)p * n, kappa + (long)p * n, 1, lim, eps, W, v + (long)p * n, 1, &it);
  iters[p] = it;
}

// One WAVEFRONT per path: the elementwise loops of sp_solve_t run strided over the 64 lanes, reductions are
// shuffles, and the tridiagonal systems are solved by parallel cyclic reduction in LDS - "factor" keeps the two
// multipliers of every row and level (ceil(log2 n) levels) and the final reciprocal diagonal, "solve" applies them to
// a right-hand side.  Everything (25 work arrays + 25 n doubles of cyclic-reduction state) lives in LDS.
struct SpWave {
  double* x;          // cyclic-reduction state behind the SP_ARRAYS work arrays
  int cap;            // row capacity (n of the launch)
  int levels = 0;
  __device__ int first() const { return threadIdx.x; }
  __device__ int step() const { return 64; }
  __device__ void sync() const { __syncthreads(); }
  __device__ double rmax(double v) const {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
  }
  __device__ double rsum(double v) const {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  }
  __device__ bool any(bool b) const { __syncthreads(); return __ballot(b) != 0ull; }
  // layout of x: A0 B0 C0 A1 B1 C1 (double-buffered rows), D0 D1, BINV, then K1[l], K2[l] per level
  __device__ double* arr(int a) const { return x + (long)a * cap; }
  __device__ void tri_factor(const SpWork& W, int n) const {
    const int lane = threadIdx.x;
    double *a0 = arr(0), *b0 = arr(1), *c0 = arr(2), *a1 = arr(3), *b1 = arr(4), *c1 = arr(5);
    for (int i = lane; i < n; i += 64) {
      a0[i] = i > 0 ? W(SP_ME, i - 1) : 0.0;
      b0[i] = W(SP_MD, i);
      c0[i] = i + 1 < n ? W(SP_ME, i) : 0.0;
    }
    __syncthreads();
    int l = 0;
    for (int s = 1; s < n; s <<= 1, ++l) {
      double *k1 = arr(9 + 2 * l), *k2 = arr(10 + 2 * l);
      for (int i = lane; i < n; i += 64) {
        const bool lo = i - s >= 0, hi = i + s < n;
        const double m1 = lo ? a0[i] / b0[i - s] : 0.0, m2 = hi ? c0[i] / b0[i + s] : 0.0;
        k1[i] = m1; k2[i] = m2;
        a1[i] = lo ? -a0[i - s] * m1 : 0.0;
        c1[i] = hi ? -c0[i + s] * m2 : 0.0;
        b1[i] = b0[i] - (lo ? c0[i - s] * m1 : 0.0) - (hi ? a0[i + s] * m2 : 0.0);
      }
      __syncthreads();
      double* t;
      t = a0; a0 = a1; a1 = t; t = b0; b0 = b1; b1 = t; t = c0; c0 = c1; c1 = t;
    }
    double* binv = arr(8);
    for (int i = lane; i < n; i += 64) binv[i] = 1.0 / b0[i];
    __syncthreads();
  }
  __device__ void tri_solve(const SpWork& W, int n) const {
    const int lane = threadIdx.x;
    double *d0 = arr(6), *d1 = arr(7);
    for (int i = lane; i < n; i += 64) d0[i] = W(SP_RHS, i);
    __syncthreads();
    int l = 0;
    for (int s = 1; s < n; s <<= 1, ++l) {
      const double *k1 = arr(9 + 2 * l), *k2 = arr(10 + 2 * l);
      for (int i = lane; i < n; i += 64)
        d1[i] = d0[i] - (i - s >= 0 ? d0[i - s] * k1[i] : 0.0) - (i + s < n ? d0[i + s] * k2[i] : 0.0);
      __syncthreads();
      double* t = d0; d0 = d1; d1 = t;
    }
    const double* binv = arr(8);
    for (int i = lane; i < n; i += 64) W(SP_DX, i) = d0[i] * binv[i];
    __syncthreads();
  }
};
__host__ __device__ inline int sp_wave_arrays(int n) {      // doubles of SpWave state per row
  int levels = 0;
  for (int s = 1; s < n; s <<= 1) ++levels;
  return 9 + 2 * levels;
}
__global__ __launch_bounds__(64) void mpmpc_speed_profile_wave_kernel(int B, int n, const double* __restrict__ li,
                                                                      const double* __restrict__ kappa,
                                                                      const double* __restrict__ limits, double eps,
                                                                      double* __restrict__ v, int* __restrict__ status,
                                                                      int* __restrict__ iters) {
  extern __shared__ double sp_lds[];
  const int p = blockIdx.x;
  if (p >= B) return;
  SpWork W{sp_lds, n, 1};
  SpWave pol{sp_lds + (long)SP_ARRAYS * n, n};
  SpLimits lim{limits[5 * p], limits[5 * p + 1], limits[5 * p + 2], limits[5 * p + 3], limits[5 * p + 4]};
  int it = 0;
  const int st = sp_solve_t(pol, n, li + (long)p * n, kappa + (long)p * n, 1, lim, eps, W, v + (long)p * n, 1, &it);
  if (threadIdx.x == 0) { status[p] = st; iters[p] = it; }
}

// K0a: free segments of every waypoint's border line, one WAVEFRONT per waypoint.  Lane 0 walks Zingl's anti-aliased
// line (a float32 recurrence in skimage's exact cell order: inherently serial, ~95 cells on Sim_Track) and leaves the
// cells in LDS; all 64 lanes then fetch the occupancies (one memory round trip for the whole line instead of one per
// cell; cells outside the grid count as occupied); lane 0 runs the run-length state machine over the LDS copy and, for
// a waypoint with at most one free segment, computes its bounds once (cor_forced) instead of once per start waypoint
// and column in K0b.  A line longer than COR_CELL_CAP cells or with more than COR_MAXSEG free segments raises *err
// (1 / 2) - mpmpc_build_corridor then fails instead of working with a truncated list.
__global__ __launch_bounds__(64) void mpmpc_free_segments_kernel(MapView map, PathGeom g, const double* __restrict__ bub,
                                                                 const double* __restrict__ blb, double min_width,
                                                                 double safety_margin, double* __restrict__ segs,
                                                                 int* __restrict__ nseg, double* __restrict__ wpc,
                                                                 int* __restrict__ err, int* __restrict__ line_cells,
                                                                 int* __restrict__ line_box) {
  __shared__ int cells[COR_CELL_CAP];
  __shared__ unsigned char occ[COR_CELL_CAP];
  __shared__ int s_n;
  __shared__ double seg[4 * COR_MAXSEG];      // lane 0's segment list (in LDS: a per-lane array would live in scratch)
  const int i = blockIdx.x, lane = threadIdx.x;
  int ux, uy, lx, ly;
  cor_w2m(map, bub[2 * i], bub[2 * i + 1], ux, uy);
  cor_w2m(map, blb[2 * i], blb[2 * i + 1], lx, ly);
  if (lane == 0) s_n = cor_line_cells(ux, uy, lx, ly, cells, COR_CELL_CAP);
  __syncthreads();
  const int n = s_n;
  int cnt;
  if (n > COR_CELL_CAP) {
    cnt = COR_E_CELLS;
  } else {
    for (int k = lane; k < n; k += 64) {
      int x, y;
      cor_unpack_cell(cells[k], x, y);
      occ[k] = cor_cell_free(map, x, y) ? 1 : 0;
      line_cells[(long)i * COR_CELL_CAP + k] = cells[k];      // K0c's cache of the line
    }
    __syncthreads();
    if (lane != 0) return;
    cor_line_box(cells, n, (ux + 1) | ((uy + 1) << 16), (lx + 1) | ((ly + 1) << 16), line_box + (long)i * COR_LINE_BOX);
    cnt = cor_scan_cells(map, ux, uy, lx, ly, min_width, n, [&](int c, int& x, int& y) { cor_unpack_cell(cells[c], x, y); },
                         [&](int c) { return occ[c] != 0; }, seg);
    for (int k = 0; k < 4 * COR_MAXSEG; ++k) segs[(long)i * 4 * COR_MAXSEG + k] = (cnt > 0 && k < 4 * cnt) ? seg[k] : 0.0;
  }
  if (lane != 0) return;
  if (cnt < 0) { atomicMax(err, cnt == COR_E_CELLS ? 1 : 2); cnt = 0; }
  nseg[i] = cnt;
  if (cnt <= 1) cor_forced(g, segs, nseg, i, safety_margin, wpc + (long)i * COR_WPC);
}

// K0b: horizon walk for every start waypoint w (table row w = update_path_constraints(w + 1, ...)).
// K0b: one thread per (start waypoint, column): cor_select_one replays only the short run of multi-segment waypoints
// right before its column, everything else is a row of K0a's per-waypoint table.
__global__ __launch_bounds__(256) void mpmpc_corridor_select_kernel(PathGeom g, const double* __restrict__ segs,
                                                                    const int* __restrict__ nseg, int n_cols,
                                                                    double safety_margin, double* __restrict__ ub_tab,
                                                                    double* __restrict__ lb_tab, int* __restrict__ bad,
                                                                    const double* __restrict__ wpc) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int w = t / n_cols, n = t - w * n_cols;
  if (w >= g.n_wp) return;
  double ub, lb;
  if (!cor_select_one(g, segs, nseg, w + 1, n, safety_margin, wpc, &ub, &lb)) {
    ub = lb = __builtin_nan("");
    if (n == 0) atomicAdd(bad, 1);
  }
  ub_tab[(long)w * n_cols + n] = ub;
  lb_tab[(long)w * n_cols + n] = lb;
}

// K0c: the corridor rows of one rollout step when every car carries its own obstacle discs (mpmpc_rollout_set_obstacles).
// One wavefront per car; lanes loop over the car's N columns (N up to 255).  Column n reads waypoint
// cor_wp(wp_id + 1 + n): if none of the car's discs meets the box of that waypoint's cached border line, it keeps the
// base segments of the last build (nseg / wpc / segs).  The others ("touched") are rescanned in the car's world: the
// wave stages the cached cells of as many touched lines as fit COR_CELL_CAP cells in LDS together with their occupancy
// (base map and discs, every lane fetching cells of its own - one memory round trip per batch of lines instead of one
// per cell), then the lane of each staged column runs the state machine over its cells in LDS (cor_scan_runs) and keeps
// the segment end cells as packed pairs plus the cor_forced row.  After a barrier every lane selects its columns as
// K0b does (cor_select_car_one) and writes lb / ub into the per-instance rows the solve reads.  flag[b] = COR_ROW_*: a
// car still running whose row is blocked / overflowing ends with alive = -3 / -4 (and gets a zero row, so that the
// solve of a stopped car stays an ordinary QP).  Every car gets its row - the solve runs on stopped cars too, and their
// status then matches the shared-table rollout's.
// LDS: 5 KB of staged cells + 0.8 KB of discs + N * (COR_WPC doubles + (2 COR_MAXSEG + 3) ints) = 5.9 KB + 124 B per column.
__global__ __launch_bounds__(64) void mpmpc_car_corridor_kernel(MapView map, PathGeom g, int N, double min_width,
                                                                double safety_margin, const double* __restrict__ segs,
                                                                const int* __restrict__ nseg, const double* __restrict__ wpc,
                                                                const int* __restrict__ line_cells,
                                                                const int* __restrict__ line_box,
                                                                const int* __restrict__ off, const int* __restrict__ discs,
                                                                const int* __restrict__ wp_id, int* __restrict__ alive,
                                                                int* __restrict__ flag, double* __restrict__ lb,
                                                                double* __restrict__ ub) {
  constexpr int PENDING = -1000000;
  extern __shared__ double lds[];
  double* col_o = lds;                                             // [N][COR_WPC]
  int* col_seg = (int*)(col_o + (long)N * COR_WPC);                // [N][2 * COR_MAXSEG] packed end cells
  int* col_cnt = col_seg + (long)N * 2 * COR_MAXSEG;               // [N]; < 0: COR_E_SEGMENTS; +1000: touched
  int* col_aux = col_cnt + N;                                      // [N] touched: cells of the line
  int* col_off = col_aux + N;                                      // [N] touched and staged: offset in stg_*, else -1
  int* dsc = col_off + N;                                          // [COR_MAX_DISCS][3]
  int* stg_cell = dsc + 3 * COR_MAX_DISCS;                         // [COR_CELL_CAP]
  unsigned char* stg_free = (unsigned char*)(stg_cell + COR_CELL_CAP);   // [COR_CELL_CAP]
  __shared__ int s_over;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int d0 = off[b], nd = off[b + 1] - d0;
  for (int k = lane; k < 3 * nd; k += 64) dsc[k] = discs[3L * d0 + k];
  if (lane == 0) s_over = 0;
  __syncthreads();
  const int wp = wp_id[b] + 1;
  auto disc = [&](int j) { return (const int*)(dsc + 3 * j); };
  for (int n = lane; n < N; n += 64) {
    const int i = cor_wp(g, wp + n);
    const int* box = line_box + (long)i * COR_LINE_BOX;
    col_off[n] = -1;
    if (nd > 0 && cor_car_touches(box, nd, disc)) {
      col_cnt[n] = PENDING;
      col_aux[n] = box[0];
    } else {
      const int cnt = nseg[i];
      if (cnt <= 1)
        for (int k = 0; k < COR_WPC; ++k) col_o[(long)n * COR_WPC + k] = wpc[(long)i * COR_WPC + k];
      col_cnt[n] = cnt;
    }
  }
  __syncthreads();
  for (int n = 0; n < N;) {            // (uniform: every lane reads the same LDS words)
    int used = 0, e = n;
    for (; e < N; ++e) {
      if (col_cnt[e] != PENDING) continue;
      const int nc = col_aux[e];
      if (used > 0 && used + nc > COR_CELL_CAP) break;
      used += nc;
    }
    used = 0;
    for (int c = n; c < e; ++c) {
      if (col_cnt[c] != PENDING) continue;
      const int nc = col_aux[c];
      if (lane == 0) col_off[c] = used;
      const int* cells = line_cells + (long)cor_wp(g, wp + c) * COR_CELL_CAP;
      for (int k = lane; k < nc; k += 64) {
        const int cell = cells[k];
        stg_cell[used + k] = cell;
        stg_free[used + k] = cor_car_cell_free(map, cell, nd, disc) ? 1 : 0;
      }
      used += nc;
    }
    __syncthreads();
    for (int c = n + lane; c < e; c += 64) {      // the lane of column c scans it
      const int o0 = col_off[c];
      if (o0 < 0) continue;
      const int nc = col_aux[c];
      const int i = cor_wp(g, wp + c);
      const int* box = line_box + (long)i * COR_LINE_BOX;
      int ux, uy, lx, ly;
      cor_unpack_cell(box[5], ux, uy);
      cor_unpack_cell(box[6], lx, ly);
      int* cs = col_seg + (long)c * 2 * COR_MAXSEG;
      double s0[4] = {0, 0, 0, 0};
      const int cnt = cor_scan_runs(map, ux, uy, lx, ly, min_width, nc,
                                    [&](int k, int& x, int& y) { cor_unpack_cell(stg_cell[o0 + k], x, y); },
                                    [&](int k) { return stg_free[o0 + k] != 0; },
                                    [&](int q, int sx, int sy, int x, int y, double ax, double ay, double bx, double by) {
                                      cs[2 * q] = (sx + 1) | ((sy + 1) << 16);
                                      cs[2 * q + 1] = (x + 1) | ((y + 1) << 16);
                                      if (q == 0) { s0[0] = ax; s0[1] = ay; s0[2] = bx; s0[3] = by; }
                                    });
      if (cnt < 0) s_over = 1;
      else if (cnt <= 1) cor_forced_seg(g, i, cnt, s0, safety_margin, col_o + (long)c * COR_WPC);
      col_cnt[c] = cnt < 0 ? cnt : cnt + 1000;
    }
    __syncthreads();
    n = e;
  }
  auto cnt = [&](int c) { const int v = col_cnt[c]; return v >= 1000 ? v - 1000 : v; };
  auto forced = [&](int c, double* o) { for (int k = 0; k < COR_WPC; ++k) o[k] = col_o[(long)c * COR_WPC + k]; };
  auto seg = [&](int c, int k, double* s) {
    if (col_cnt[c] >= 1000) {
      const int* cs = col_seg + (long)c * 2 * COR_MAXSEG;
      int x, y;
      cor_unpack_cell(cs[2 * k], x, y);
      cor_m2w(map, x, y, s[0], s[1]);
      cor_unpack_cell(cs[2 * k + 1], x, y);
      cor_m2w(map, x, y, s[2], s[3]);
    } else {
      const double* sg = segs + (long)cor_wp(g, wp + c) * 4 * COR_MAXSEG + 4 * k;
      for (int j = 0; j < 4; ++j) s[j] = sg[j];
    }
  };
  const int verdict = cnt(0) == 0 ? COR_ROW_BLOCKED : (s_over ? COR_ROW_OVERFLOW : COR_ROW_OK);   // the reference raises at column 0 first
  for (int n = lane; n < N; n += 64) {
    double u = 0.0, l = 0.0;
    if (verdict == COR_ROW_OK) cor_select_car_one(g, wp, n, safety_margin, cnt, forced, seg, &u, &l);
    ub[(long)b * N + n] = u;
    lb[(long)b * N + n] = l;
  }
  if (lane == 0) {
    flag[b] = verdict;
    if (verdict != COR_ROW_OK && alive[b] == 1) alive[b] = verdict == COR_ROW_BLOCKED ? -3 : -4;
  }
}

// K0m: the movers of one rollout step (mpmpc_rollout_set_movers), launched between K3a and K0c when there are any.  One
// thread per mover of the whole fleet; its parameters are structure-of-arrays ([n] each: a wavefront loads consecutive
// words), its disc of step k (mov_disc: closed form in k; kind 1 searches ro_cum, ~9 probes that stay in L2) goes into
// its slot of its car's disc list - dst[j], laid out on the host when either setting changes - where K0c reads it
// behind the car's static discs.
__global__ __launch_bounds__(256) void mpmpc_obstacle_move_kernel(int n, long long k, long long step0, MapView map,
                                                                  MoverPath path, const int* __restrict__ kind,
                                                                  const int* __restrict__ radius,
                                                                  const double* __restrict__ prm,
                                                                  const int* __restrict__ dst, int* __restrict__ discs) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  int d[3];
  mov_disc(map, path, kind[j], radius[j], prm[j], prm[(long)n + j], prm[2L * n + j], prm[3L * n + j], k, step0, d);
  int* o = discs + 3L * dst[j];
  o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
}

// K3a: where is each car on the path, and what is its path-relative state (one thread per car)
// (alive: 0 = lap finished, s past the path's length; -2 = an open path's end reached, the reference's exit(1) in
//  get_waypoint - wp_id and x0 are still written, they are the state the reference computed before it exited)
__global__ __launch_bounds__(256) void mpmpc_localise_kernel(int B, int n_wp, int N, int circular, const double* __restrict__ cum,
                                                             const double* __restrict__ gx, const double* __restrict__ gy,
                                                             const double* __restrict__ gpsi, const double* __restrict__ s,
                                                             const double* __restrict__ pose, int* __restrict__ alive,
                                                             int* __restrict__ wp_id, double* __restrict__ x0,
                                                             int* __restrict__ shift) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B || alive[i] != 1) return;
  const int wp = ro_current_waypoint(cum, n_wp, s[i]);
  if (wp < 0) { alive[i] = 0; return; }              // lap finished
  if (shift) {                                        // waypoints advanced since the last step (warm start)
    int d = wp - wp_id[i];
    if (d < 0) d += n_wp;
    shift[i] = d;
  }
  wp_id[i] = wp;
  ro_t2s(pose[3 * i], pose[3 * i + 1], pose[3 * i + 2], gx[wp], gy[wp], gpsi[wp], x0 + 3 * i);
  if (ro_past_open_end(n_wp, N, circular != 0, wp)) alive[i] = -2;     // end of an open path
}

// K3b: use the solution (or the fallback plan), drive the plant one step (one thread per car)
__global__ __launch_bounds__(256) void mpmpc_advance_kernel(int B, int N, double L, double Ts, const double* __restrict__ kappa,
                                                            const int* __restrict__ wp_id, const double* __restrict__ x0,
                                                            const int* __restrict__ status, const double* __restrict__ z,
                                                            double* __restrict__ cc, int* __restrict__ counter,
                                                            int* __restrict__ alive, double* __restrict__ pose,
                                                            double* __restrict__ s, double* __restrict__ u_last) {
  // one thread per (car, plan entry): the N arctangents of a car's new plan are independent; the thread of entry 0
  // then drives the car (it reads only plan entries it wrote itself, or - fallback - entries nobody writes)
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int i = g / N, k = g - i * N;
  if (i >= B || alive[i] != 1) return;
  const int n = 5 * N + 3;
  const int st = status[i];
  if (ro_usable(st)) ro_plan_entry(N, L, z + (long)i * n, cc + (long)i * 2 * N, k);
  if (k == 0 && !ro_drive(N, L, Ts, st, cc + (long)i * 2 * N, counter + i, x0 + 3 * i, kappa[wp_id[i]], pose + 3 * i,
                          s + i, u_last + 2 * i))
    alive[i] = -1;
}

// K3r: the recorder of a rollout (mpmpc_rollout_record), two launches around a recorded step.  Both give every ENTRY of
// a car's record its own thread, and the record's fields lie car-major ([B][len], the host's layout): consecutive threads
// store consecutive words.  `rec` is the record's base address (64-bit arithmetic on the host).
//   snapshot  before localise: s, pose, alive as the step finds them (4 entries per car)
//   write     after advance: x0, u, wp_id, status, counter, alive, plan, predicted path, corridor row (ro_record_finish)
__global__ __launch_bounds__(256) void mpmpc_record_snapshot_kernel(int B, const double* __restrict__ s,
                                                                    const double* __restrict__ pose,
                                                                    const int* __restrict__ alive, int* __restrict__ a_in,
                                                                    char* __restrict__ rec, RoTraceLayout lay) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(g / RO_REC_BEGIN_ENTRIES), c = (int)(g - (long)i * RO_REC_BEGIN_ENTRIES);
  if (i >= B) return;
  ro_record_begin(s, pose, alive, a_in, rec, lay, i, c);
}
__global__ __launch_bounds__(256) void mpmpc_record_write_kernel(int B, RoRecSrc src, char* __restrict__ rec, RoTraceLayout lay) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(g / lay.entries), e = (int)(g - (long)i * lay.entries);
  if (i >= B) return;
  ro_record_finish(src, rec, lay, i, e);
}

// ------------------------------------------------------------------------------------ host side
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(MPMPC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
  } while (0)

struct mpmpc_handle_s {
  mpmpc_config cfg;
  mpmpc_settings st;
  int ld = 0, n = 0, m = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_in = nullptr;      // the last staged upload has left the pinned buffer
  bool in_flight = false;
  // tables
  double *kappa = nullptr, *v_ref = nullptr, *ds_next = nullptr, *ub_tab = nullptr, *lb_tab = nullptr;
  int n_wp = 0, n_cols = 0;
  // corridor generation on the device: grid, per-waypoint geometry, per-waypoint free segments
  int8_t* map = nullptr;
  int map_h = 0, map_w = 0;
  double map_ox = 0, map_oy = 0, map_res = 0;
  double *gx = nullptr, *gy = nullptr, *gpsi = nullptr, *bub = nullptr, *blb = nullptr, *segs = nullptr, *gtrig = nullptr;
  int *nseg = nullptr, *bad = nullptr;      // bad[0]: start waypoints without a free segment, bad[1]: K0a overflow code
  int geom_n = 0;
  std::vector<double> host_bub, host_blb;   // border points, kept to validate them against the map of the moment
  // per-car obstacles (K0c): cached border lines of the last build, and what that build was made from
  int *line_cells = nullptr, *line_box = nullptr;      // [n_wp x COR_CELL_CAP], [n_wp x COR_LINE_BOX]
  unsigned base_gen = 1;        // bumped by mpmpc_set_path / _set_map / _set_path_geometry
  unsigned built_gen = 0;       // base_gen of the last successful mpmpc_build_corridor (0: none)
  double built_min_width = 0, built_sm = 0;
  int *obst_off = nullptr, *obst_discs = nullptr, *ro_flag = nullptr;   // CSR lists on the device, per-car row verdicts
  int obst_B = 0;               // > 0: the rollout's cars carry their own discs (mpmpc_rollout_set_obstacles)
  unsigned obst_gen = 0;        // base_gen the discs were validated against
  bool car_rows = false;        // the last rollout step built per-car rows
  // The two per-car settings, kept on the host: static discs (mpmpc_rollout_set_obstacles; st_B > 0: set; obst_gen) and
  // movers (mpmpc_rollout_set_movers; mv_B > 0: set; mv_gen).  Whichever setter is called lays out ONE CSR list per car
  // on the device (obst_off / obst_discs, what K0c reads: the static discs, then a slot per mover that K0m fills every
  // step) - sync_disc_lists; obst_B is the B of whichever is set.
  std::vector<int32_t> st_off, st_discs, mv_off, comb_off;
  int st_B = 0, mv_B = 0;
  int mv_n = 0, mv_cap = 0;     // movers of the fleet; movers the device block holds
  unsigned mv_gen = 0;          // base_gen the movers were set against
  long long mv_step0 = 0;
  char* mv_block = nullptr;     // [4][mv_n] doubles (parameters), then [mv_n] ints each: kind, radius, slot
  bool discs_live = false;      // obst_discs hold the lists the last rollout step used (mpmpc_rollout_obstacles)
  // closed-loop rollout state
  double *ro_cum = nullptr, *ro_s = nullptr, *ro_pose = nullptr, *ro_u = nullptr;
  int *ro_counter = nullptr, *ro_alive = nullptr;
  int *ro_act = nullptr, *ro_shift = nullptr;      // warm start: certified active sets [B x ld], waypoints advanced [B]
  int ro_warm = 2;      // 0 off, 1 on, 2 where it pays (see plan_solve)
  double ro_Ts = 0;
  int ro_B = 0;
  bool ro_valid = false;      // the batch blocks still hold the rollout's plans / waypoint ids / states
  // recorder (mpmpc_rollout_record): the trace has its own memory, [rec_cap] records of rec_lay.bytes each
  char* rec_buf = nullptr;
  int* rec_ain = nullptr;       // [rec_B] alive before the step being recorded
  RoTraceLayout rec_lay{};
  int rec_cap = 0, rec_B = 0, rec_fields = 0, rec_stride = 1;
  int rec_count = 0;            // records held
  long long ro_steps = 0;       // rollout steps since mpmpc_rollout_init
  // per-batch inputs
  int* wp_id = nullptr;
  double *x0 = nullptr, *cc = nullptr, *lb = nullptr, *ub = nullptr;
  bool have_rows = false;     // per-instance corridor rows uploaded (else: table)
  int uploaded = 0;
  // the inputs of a batch lie back to back in ONE device block (wp_id, x0, cc, lb, ub, laid out for the batch size
  // of the last upload), and so do the outputs of every launch slot (Slot::out_block: u0, resid, status, iters, z, y): an upload
  // or a download through the pinned staging buffers is then a single copy instead of five or six - what a single-car call is made of
  char* in_block = nullptr;
  int laid_out = 0;
  double* qp = nullptr;      // stage-blocked QP
  // pinned host staging for mpmpc_upload / mpmpc_download (small copies from pageable memory are
  // synchronous and slow; nullptr above STAGE_LIMIT bytes: large batches amortise the direct path)
  char *stage_in = nullptr, *stage_out = nullptr;
  size_t stage_in_bytes = 0, stage_out_bytes = 0;
  // ... above that limit an upload goes through a small page-locked bounce buffer in two halves (allocated by the first such
  // upload): the device copy of one half runs while the host fills the other, and the call returns when the caller's buffers
  // have been read - not when the device has them.  (A copy from pageable memory is synchronous: one process feeding several
  // devices - sharded.py - would otherwise serve them one after the other)
  char* bounce = nullptr;
  hipEvent_t ev_bounce[2] = {nullptr, nullptr};
  bool bounce_busy[2] = {false, false};
  int bounce_turn = 0;
  size_t staged_bytes = 0;  // mpmpc_staged_begin without its mpmpc_staged_end: bytes of the output block on their way back
  // ---- Launch slots: what ONE solve launch in flight owns - its stream, its output block, its tail lists and its deferred-tail
  // state.  slot[0] is made by mpmpc_create (its stream before anything else touches the device) and is all a handle needs that
  // never pipelines; slot[1 .. n_slots - 1] are made by the first pipelined resident launch (next_slot).  `cur` is the slot of the
  // LAST launch, and everything in this file that is not a resident launch - uploads, downloads, the staged calls, corridor build,
  // rollout, recorder, timed launches - works on last(): its stream, its outputs.  A resident launch first moves `cur` one slot on
  // (round robin over the `pipeline` slots in use), so that launches k + 1 .. k + pipeline - 1 run beside launch k, each on its
  // own stream, writing its own outputs.  A function that acts on a slot is handed it; nothing is copied between slots.
  struct Slot {
    hipStream_t stream = nullptr;
    char* out_block = nullptr;      // pointers into it (lay_out):
    double *z = nullptr, *u0 = nullptr, *resid = nullptr, *y = nullptr;
    int *status = nullptr, *iters = nullptr;
    bool y_valid = false;     // the slot's last solve launch stored y
    bool busy = false;        // resident launches in flight on the slot's stream that nothing has waited for yet
    // instances the early pass of a packed (2 or 4 per wave) launch could not certify: [0] = count, [1..] = ids
    int* tail = nullptr;
    int tail_flip = 0;          // which of the two lists the next reduced-native launch fills
    // Deferred tail (batch launches of the reduced-native kernels, not the closed loop).  Launching the tail kernel costs
    // 4.8 us even when its list is empty - 10 % of a 1 024-instance step - so when the last launch whose outcome the host
    // has SEEN left no tail, the next launches do not enqueue one: the reduced-native kernel stamps its sequence number into
    // tail_flag (host memory) if it appends anything, and every entry point through which results or state can be observed
    // or changed (sync, download, upload, set_*, rollout, timed launches) first drains the stream, looks at the stamp and
    // runs the tail of the slot's LAST launch if it left one (observe_tail).  A launch that is followed by another launch on
    // the slot without such a call in between has unobservable results either way (same output buffers).
    unsigned* tail_flag = nullptr;      // hipHostMalloc'ed, device-visible
    unsigned seq = 0;                   // sequence number of the last reduced-native launch
    bool tail_expect_empty = false;     // the last observed launch left no tail
    bool tail_ran_late = false;         // the last observe_tail had to run a deferred tail
    // Second level (reduced_native_tail configurations): the tail goes to the reduced-native tail kernel first, which appends
    // what IT leaves to a third list (tail + 2 (max_batch + 1)) and stamps tail_flag[1]; the general kernel on that list is
    // deferred by the same rule.
    bool tail2_expect_empty = false;
    // The slot's last solve launch: its plan (mpmpc_launch_plan.hpp), the first stage not yet enqueued, and what the stages
    // still to come need of the launch they belong to - the batch size, whether y is stored, the solver parameters, the lists
    // by role (MPMPC_LIST_*).  (The handle's input buffers and path tables are read when a stage is enqueued: every call that
    // changes them settles first.)
    SolvePlan plan{};
    int next_stage = 0;
    int launch_B = 0;
    bool want_y = false;
    SolverParams prm{};
    int* list[4] = {nullptr, nullptr, nullptr, nullptr};
    bool deferred() const { return next_stage < plan.n; }      // stages of the last launch were held back
  };
  static constexpr int MAX_PIPELINE = 8;
  Slot slot[MAX_PIPELINE];
  int n_slots = 0;          // slots allocated: slot[0 .. n_slots - 1]
  int cur = 0;              // the slot of the last launch
  Slot& last() { return slot[cur]; }
  int pipeline = 3;         // launch slots in use = resident launches in flight (1 = one slot only): what mpmpc_set_pipeline asked
                            // for, three by default, but never more than the process has hardware queues (launch_streams below:
                            // GPU_MAX_HW_QUEUES, 4 if unset) - two streams on one queue take turns.  Measured, config 2, four
                            // queues: depth 4 = 68.7 M solves/s with the four launch streams on four queues, 39.5 M while a
                            // synchronous hipMemset of this file had made the null stream hold one of them (two launch streams
                            // shared a queue: 2.0 instead of 3.85 solve kernels on the chip; profiles/hw_queues/)
  hipEvent_t ev_order = nullptr;
  bool order_pending = false;      // asynchronous work other than resident solves is queued on last().stream: the next resident launch
                                   // goes to ANOTHER stream and has to wait for it (uploads, closed-loop steps: they write what solves read)
  int force_lanes = 0;      // mpmpc_set_packing: 0 = chosen from the batch size
  // mpmpc_set_tail_kernel (MPMPC_LEAN_TAIL=0 in the environment: off from the start, for A/B timings of whole programs)
  bool lean_tail = !(std::getenv("MPMPC_LEAN_TAIL") && std::atoi(std::getenv("MPMPC_LEAN_TAIL")) == 0);
  bool lean_tail_single = std::getenv("MPMPC_LEAN_TAIL") && std::atoi(std::getenv("MPMPC_LEAN_TAIL")) == 2;      // ONE tail instance per wave
  bool staged_async = true; // mpmpc_staged_begin was called as such (not as the first half of mpmpc_solve_staged)
  bool resident_y = true;   // mpmpc_set_outputs: do resident launches store the multipliers y (46 % of the output bytes)?
};
using Slot = mpmpc_handle_s::Slot;

static int host_stage_ld(int N) { return N + 1 <= 16 ? 16 : (N + 1 <= 32 ? 32 : (N + 1 <= 64 ? 64 : (N + 1 <= 128 ? 128 : 256))); }

static int observe_tail(mpmpc_handle h, Slot& s);
// The other slots' launches are drained and their deferred tails, if any, are run (the slot of the last launch is left as it
// is: what follows on its stream is ordered behind it anyway).
static int settle_other_slots(mpmpc_handle h) {
  for (int i = 0; i < h->n_slots; ++i) {
    Slot& s = h->slot[i];
    if (i == h->cur || (!s.busy && !s.deferred())) continue;
    if (int rc = observe_tail(h, s)) return rc;
  }
  return MPMPC_OK;
}
// ... and then the slot of the last launch: every launch of the handle is done, deferred tails included
static int drain(mpmpc_handle h) {
  if (int rc = settle_other_slots(h)) return rc;
  return observe_tail(h, h->last());
}
// first statement of every entry point that reads results or changes what a launch in flight - or a deferred tail launch -
// works on: `if (int rc = settle(h)) return rc;`
static int settle(mpmpc_handle h) {
  if (h->staged_bytes) {
    if (int rc = mpmpc_staged_end(h)) return rc;
  }
  if (int rc = settle_other_slots(h)) return rc;
  if (h->last().deferred()) {
    if (int rc = observe_tail(h, h->last())) return rc;
  }
  h->order_pending = true;
  return MPMPC_OK;
}

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
  h->wp_id = (int*)(h->in_block + L.wp_id);
  h->x0 = (double*)(h->in_block + L.x0);
  h->cc = (double*)(h->in_block + L.cc);
  h->lb = (double*)(h->in_block + L.lb);
  h->ub = (double*)(h->in_block + L.ub);
  for (int i = 0; i < h->n_slots; ++i) {
    Slot& a = h->slot[i];
    a.u0 = (double*)(a.out_block + L.u0);
    a.resid = (double*)(a.out_block + L.resid);
    a.status = (int*)(a.out_block + L.status);
    a.iters = (int*)(a.out_block + L.iters);
    a.z = (double*)(a.out_block + L.z);
    a.y = (double*)(a.out_block + L.y);
  }
  h->laid_out = B;
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
  if (s.out_block) (void)hipFree(s.out_block);
  if (s.tail) (void)hipFree(s.tail);
  if (s.tail_flag) (void)hipHostFree(s.tail_flag);
  if (s.stream) (void)hipStreamDestroy(s.stream);
  s = Slot{};
}
// One launch slot: its stream FIRST (nothing in this library may run on the null stream - its first use makes the runtime give it
// a hardware queue for the life of the process, one fewer for the launch streams, see launch_streams), the output block for
// max_batch instances, the tail lists, the tail flag.  The lists are cleared on the slot's own stream: they are only ever used
// by launches on it, which are ordered behind that; the wait reports a failure here.
static int alloc_slot(mpmpc_handle h, Slot& s) {
  const size_t out_bytes = block_layout(h->cfg.N, h->cfg.max_batch).out_end, tail_bytes = 3 * ((size_t)h->cfg.max_batch + 1) * sizeof(int);
  if (create_launch_stream(&s.stream) != hipSuccess || hipMalloc((void**)&s.out_block, out_bytes) != hipSuccess ||
      hipMalloc((void**)&s.tail, tail_bytes) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&s.tail_flag), 2 * sizeof(unsigned), hipHostMallocDefault) != hipSuccess ||
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
  lay_out(h, h->laid_out ? h->laid_out : h->cfg.max_batch);
  return MPMPC_OK;
}

int mpmpc_destroy(mpmpc_handle h) {
  if (!h) return MPMPC_OK;
  (void)hipSetDevice(h->cfg.device);
  void* ptrs[] = {h->kappa, h->v_ref, h->ds_next, h->ub_tab, h->lb_tab, h->in_block,
                  h->qp,    h->map, h->gx,  h->gy,
                  h->gpsi,  h->bub,   h->blb,     h->segs,   h->nseg,   h->bad,    h->ro_cum, h->ro_s, h->ro_pose, h->gtrig,
                  h->ro_u,  h->ro_counter, h->ro_alive, h->ro_act, h->ro_shift, h->line_cells, h->line_box,
                  h->obst_off, h->obst_discs, h->ro_flag, h->rec_buf, h->rec_ain, h->mv_block};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (auto& s : h->slot) free_slot(s);
  if (h->ev_order) (void)hipEventDestroy(h->ev_order);
  if (h->bounce) (void)hipHostFree(h->bounce);
  for (auto& e : h->ev_bounce)
    if (e) (void)hipEventDestroy(e);
  if (h->stage_in) (void)hipHostFree(h->stage_in);
  if (h->stage_out) (void)hipHostFree(h->stage_out);
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->ev_in) (void)hipEventDestroy(h->ev_in);
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
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming);
  if (e != hipSuccess) {
    mpmpc_destroy(h);
    return fail(MPMPC_E_HIP, std::string("event creation: ") + hipGetErrorString(e));
  }
#define ALLOC(ptr, count)                                                                \
  do {                                                                                   \
    hipError_t e_ = hipMalloc((void**)&(ptr), (count) * sizeof(*(ptr)));                 \
    if (e_ != hipSuccess) {                                                              \
      mpmpc_destroy(h);                                                                  \
      return fail(MPMPC_E_HIP, std::string("hipMalloc " #ptr ": ") + hipGetErrorString(e_)); \
    }                                                                                    \
  } while (0)
  const BlockLayout lay = block_layout(cfg->N, cfg->max_batch);
  ALLOC(h->in_block, lay.in_end);
  lay_out(h, cfg->max_batch);
  ALLOC(h->qp, (size_t)MPMPC_NUM_FIELDS * B * h->ld);
#undef ALLOC
  {
    const size_t STAGE_LIMIT = 64u << 20;
    const size_t in_b = lay.in_end, out_b = lay.out_end;
    if (in_b <= STAGE_LIMIT && hipHostMalloc((void**)&h->stage_in, in_b, hipHostMallocDefault) == hipSuccess) h->stage_in_bytes = in_b;
    else h->stage_in = nullptr;
    if (out_b <= STAGE_LIMIT && hipHostMalloc((void**)&h->stage_out, out_b, hipHostMallocDefault) == hipSuccess) h->stage_out_bytes = out_b;
    else h->stage_out = nullptr;
  }
  *out = h;
  return MPMPC_OK;
}

int mpmpc_set_packing(mpmpc_handle h, int32_t lanes_per_instance) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  if (!packing_valid(h->cfg.N, lanes_per_instance))
    return fail(MPMPC_E_ARG, "lanes_per_instance must be 0 (auto) or 16, 32, 64 and hold the N + 1 stages of an instance - half of them at 16 / 64, two stages "
                             "per lane - or 128 / 256: the workgroup kernels of horizons 64 .. 255");
  h->force_lanes = lanes_per_instance;
  return MPMPC_OK;
}

int mpmpc_set_tail_kernel(mpmpc_handle h, int32_t reduced_native) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  if (reduced_native < 0 || reduced_native > 2) return fail(MPMPC_E_ARG, "reduced_native must be 0, 1 or 2");
  h->lean_tail = reduced_native != 0;
  h->lean_tail_single = reduced_native == 2;
  return MPMPC_OK;
}

int mpmpc_set_settings(mpmpc_handle h, const mpmpc_settings* settings) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  if (int rc = check_settings(settings)) return rc;
  h->st = *settings;
  return MPMPC_OK;
}

static int upload_table(mpmpc_handle h, double** dst, const double* src, size_t count) {
  if (*dst) { HIP_TRY(hipFree(*dst)); *dst = nullptr; }
  HIP_TRY(hipMalloc((void**)dst, count * sizeof(double)));
  HIP_TRY(hipMemcpyAsync(*dst, src, count * sizeof(double), hipMemcpyHostToDevice, h->last().stream));
  return MPMPC_OK;
}

int mpmpc_set_path(mpmpc_handle h, int32_t n_wp, const double* kappa, const double* v_ref, const double* ds_next) {
  if (!h || !kappa || !v_ref || !ds_next) return fail(MPMPC_E_ARG, "NULL argument");
  if (int rc = settle(h)) return rc;
  if (n_wp < 2) return fail(MPMPC_E_ARG, "need at least 2 waypoints");
  for (int i = 0; i < n_wp; ++i)
    if (!(v_ref[i] > 0) || !std::isfinite(kappa[i]) || !(ds_next[i] >= 0))
      return fail(MPMPC_E_ARG, "path table: need v_ref > 0, finite kappa, ds_next >= 0");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (int rc = upload_table(h, &h->kappa, kappa, n_wp)) return rc;
  if (int rc = upload_table(h, &h->v_ref, v_ref, n_wp)) return rc;
  if (int rc = upload_table(h, &h->ds_next, ds_next, n_wp)) return rc;
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  if (h->n_wp != n_wp) { h->n_cols = 0; }   // a corridor table of another path is void
  h->n_wp = n_wp;
  ++h->base_gen;
  return MPMPC_OK;
}

int mpmpc_set_corridor(mpmpc_handle h, int32_t n_wp, int32_t n_cols, const double* ub, const double* lb) {
  if (!h || !ub || !lb) return fail(MPMPC_E_ARG, "NULL argument");
  if (int rc = settle(h)) return rc;
  if (h->n_wp == 0 || n_wp != h->n_wp) return fail(MPMPC_E_STATE, "set the path first; n_wp must match it");
  if (n_cols < h->cfg.N) return fail(MPMPC_E_ARG, "corridor table needs n_cols >= N");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (int rc = upload_table(h, &h->ub_tab, ub, (size_t)n_wp * n_cols)) return rc;
  if (int rc = upload_table(h, &h->lb_tab, lb, (size_t)n_wp * n_cols)) return rc;
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  h->n_cols = n_cols;
  return MPMPC_OK;
}

int mpmpc_set_map(mpmpc_handle h, int32_t height, int32_t width, const int8_t* data, double origin_x,
                  double origin_y, double resolution) {
  if (!h || !data) return fail(MPMPC_E_ARG, "NULL argument");
  if (int rc = settle(h)) return rc;
  if (height < 1 || width < 1 || !(resolution > 0)) return fail(MPMPC_E_ARG, "map needs positive size and resolution");
  if (height > COR_MAX_SIDE || width > COR_MAX_SIDE) return fail(MPMPC_E_ARG, "map sides are limited to 65534 cells");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (h->map) { HIP_TRY(hipFree(h->map)); h->map = nullptr; }
  HIP_TRY(hipMalloc((void**)&h->map, (size_t)height * width));
  HIP_TRY(hipMemcpyAsync(h->map, data, (size_t)height * width, hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  h->map_h = height; h->map_w = width; h->map_ox = origin_x; h->map_oy = origin_y; h->map_res = resolution;
  ++h->base_gen;
  return MPMPC_OK;
}

int mpmpc_set_path_geometry(mpmpc_handle h, int32_t n_wp, const double* x, const double* y, const double* psi,
                            const double* border_ub, const double* border_lb) {
  if (!h || !x || !y || !psi || !border_ub || !border_lb) return fail(MPMPC_E_ARG, "NULL argument");
  if (int rc = settle(h)) return rc;
  if (h->n_wp == 0 || n_wp != h->n_wp) return fail(MPMPC_E_STATE, "set the path first; n_wp must match it");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (int rc = upload_table(h, &h->gx, x, n_wp)) return rc;
  if (int rc = upload_table(h, &h->gy, y, n_wp)) return rc;
  if (int rc = upload_table(h, &h->gpsi, psi, n_wp)) return rc;
  if (int rc = upload_table(h, &h->bub, border_ub, 2 * (size_t)n_wp)) return rc;
  if (int rc = upload_table(h, &h->blb, border_lb, 2 * (size_t)n_wp)) return rc;
  {
    // everything of a waypoint that needs libm, from the HOST's libm: the device tables then hold no device-libm
    // result (bit-exact against the reference's tables, golden G3)
    std::vector<double> trig((size_t)n_wp * COR_TRIG);
    for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
    if (int rc = upload_table(h, &h->gtrig, trig.data(), trig.size())) return rc;
    HIP_TRY(hipStreamSynchronize(h->last().stream));      // `trig` leaves scope
  }
  h->host_bub.assign(border_ub, border_ub + 2 * (size_t)n_wp);
  h->host_blb.assign(border_lb, border_lb + 2 * (size_t)n_wp);
  if (h->segs) { HIP_TRY(hipFree(h->segs)); h->segs = nullptr; }
  if (h->nseg) { HIP_TRY(hipFree(h->nseg)); h->nseg = nullptr; }
  if (!h->bad) HIP_TRY(hipMalloc((void**)&h->bad, 2 * sizeof(int)));
  HIP_TRY(hipMalloc((void**)&h->segs, sizeof(double) * (4 * COR_MAXSEG + COR_WPC) * (size_t)n_wp));   // + cor_forced rows
  HIP_TRY(hipMalloc((void**)&h->nseg, sizeof(int) * (size_t)n_wp));
  if (h->line_cells) { HIP_TRY(hipFree(h->line_cells)); h->line_cells = nullptr; }
  if (h->line_box) { HIP_TRY(hipFree(h->line_box)); h->line_box = nullptr; }
  HIP_TRY(hipMalloc((void**)&h->line_cells, sizeof(int) * COR_CELL_CAP * (size_t)n_wp));
  HIP_TRY(hipMalloc((void**)&h->line_box, sizeof(int) * COR_LINE_BOX * (size_t)n_wp));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  h->geom_n = n_wp;
  ++h->base_gen;
  return MPMPC_OK;
}

int mpmpc_build_corridor(mpmpc_handle h, int32_t n_cols, double min_width, double safety_margin, double* ub_out,
                         double* lb_out, int32_t* bad_rows) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (!h->map || h->geom_n == 0 || h->geom_n != h->n_wp)
    return fail(MPMPC_E_STATE, "needs mpmpc_set_path, mpmpc_set_map and mpmpc_set_path_geometry first");
  if (n_cols < h->cfg.N) return fail(MPMPC_E_ARG, "corridor table needs n_cols >= N");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int n = h->n_wp;
  if (h->n_cols != n_cols || !h->ub_tab) {
    if (h->ub_tab) { HIP_TRY(hipFree(h->ub_tab)); h->ub_tab = nullptr; }
    if (h->lb_tab) { HIP_TRY(hipFree(h->lb_tab)); h->lb_tab = nullptr; }
    HIP_TRY(hipMalloc((void**)&h->ub_tab, sizeof(double) * (size_t)n * n_cols));
    HIP_TRY(hipMalloc((void**)&h->lb_tab, sizeof(double) * (size_t)n * n_cols));
  }
  MapView mv{h->map, h->map_h, h->map_w, h->map_ox, h->map_oy, h->map_res};
  PathGeom pg{h->gx, h->gy, h->gpsi, h->ds_next, n, h->cfg.circular, h->gtrig};
  // the border cells of every waypoint must lie on the map of the moment (numpy indexing in the reference raises
  // IndexError past the upper edges and silently wraps around below zero: here both are an error)
  for (int i = 0; i < n; ++i) {
    int cx[2], cy[2];
    cor_w2m(mv, h->host_bub[2 * i], h->host_bub[2 * i + 1], cx[0], cy[0]);
    cor_w2m(mv, h->host_blb[2 * i], h->host_blb[2 * i + 1], cx[1], cy[1]);
    for (int e = 0; e < 2; ++e)
      if (cx[e] < 0 || cx[e] >= h->map_w || cy[e] < 0 || cy[e] >= h->map_h)
        return fail(MPMPC_E_ARG, "border cell of waypoint " + std::to_string(i) + " lies outside the map");
  }
  HIP_TRY(hipMemsetAsync(h->bad, 0, 2 * sizeof(int), sl.stream));
  double* wpc = h->segs + (size_t)4 * COR_MAXSEG * n;
  hipLaunchKernelGGL(mpmpc_free_segments_kernel, dim3(n), dim3(64), 0, sl.stream, mv, pg, h->bub, h->blb, min_width,
                     safety_margin, h->segs, h->nseg, wpc, h->bad + 1, h->line_cells, h->line_box);
  hipLaunchKernelGGL(mpmpc_corridor_select_kernel, dim3((n * n_cols + 255) / 256), dim3(256), 0, sl.stream, pg, h->segs,
                     h->nseg, n_cols, safety_margin, h->ub_tab, h->lb_tab, h->bad, wpc);
  HIP_TRY(hipGetLastError());
  int bad2[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(bad2, h->bad, 2 * sizeof(int), hipMemcpyDeviceToHost, sl.stream));
  if (ub_out) HIP_TRY(hipMemcpyAsync(ub_out, h->ub_tab, sizeof(double) * (size_t)n * n_cols, hipMemcpyDeviceToHost, sl.stream));
  if (lb_out) HIP_TRY(hipMemcpyAsync(lb_out, h->lb_tab, sizeof(double) * (size_t)n * n_cols, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  h->built_gen = 0;
  if (bad2[1] != 0) {
    h->n_cols = 0;        // the table is not usable
    return fail(MPMPC_E_ARG, bad2[1] == 1 ? "a waypoint's border line has more than 1024 cells (COR_CELL_CAP)"
                                           : "a waypoint's border line has more than 8 free segments (COR_MAXSEG)");
  }
  const int bad = bad2[0];
  if (bad_rows) *bad_rows = bad;
  h->n_cols = n_cols;
  h->built_gen = h->base_gen;
  h->built_min_width = min_width;
  h->built_sm = safety_margin;
  return MPMPC_OK;
}

int mpmpc_rollout_init(mpmpc_handle h, int32_t B, double Ts, const double* cum_lengths, const double* s,
                       const double* pose, const double* cc0) {
  if (!h || !cum_lengths || !s || !pose) return fail(MPMPC_E_ARG, "NULL argument");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (!(Ts > 0)) return fail(MPMPC_E_ARG, "Ts must be > 0");
  if (h->n_wp == 0 || h->geom_n != h->n_wp) return fail(MPMPC_E_STATE, "needs mpmpc_set_path and mpmpc_set_path_geometry");
  if (h->n_cols == 0) return fail(MPMPC_E_STATE, "needs a corridor table (mpmpc_set_corridor / mpmpc_build_corridor)");
  if (h->rec_cap > 0 && h->rec_B != B) return fail(MPMPC_E_STATE, "mpmpc_rollout_record was set up for another number of cars");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->ro_s) {
    HIP_TRY(hipMalloc((void**)&h->ro_s, sizeof(double) * mb));
    HIP_TRY(hipMalloc((void**)&h->ro_pose, sizeof(double) * 3 * mb));
    HIP_TRY(hipMalloc((void**)&h->ro_u, sizeof(double) * 2 * mb));
    HIP_TRY(hipMalloc((void**)&h->ro_counter, sizeof(int) * mb));
    HIP_TRY(hipMalloc((void**)&h->ro_alive, sizeof(int) * mb));
    HIP_TRY(hipMalloc((void**)&h->ro_act, sizeof(int) * mb * h->ld));
    HIP_TRY(hipMalloc((void**)&h->ro_shift, sizeof(int) * mb));
  }
  if (!h->ro_flag) HIP_TRY(hipMalloc((void**)&h->ro_flag, sizeof(int) * mb));
  if (int rc = upload_table(h, &h->ro_cum, cum_lengths, h->n_wp)) return rc;
  const int N = h->cfg.N;
  if (B != h->laid_out) lay_out(h, B);
  HIP_TRY(hipMemcpyAsync(h->ro_s, s, sizeof(double) * B, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipMemcpyAsync(h->ro_pose, pose, sizeof(double) * 3 * B, hipMemcpyHostToDevice, sl.stream));
  if (cc0) HIP_TRY(hipMemcpyAsync(h->cc, cc0, sizeof(double) * 2 * N * B, hipMemcpyHostToDevice, sl.stream));
  else HIP_TRY(hipMemsetAsync(h->cc, 0, sizeof(double) * 2 * N * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->ro_counter, 0, sizeof(int) * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->ro_act, 0, sizeof(int) * (size_t)B * h->ld, sl.stream));     // no guess yet
  HIP_TRY(hipMemsetAsync(h->ro_shift, 0, sizeof(int) * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->ro_u, 0, sizeof(double) * 2 * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->wp_id, 0, sizeof(int) * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->x0, 0, sizeof(double) * 3 * B, sl.stream));
  HIP_TRY(hipMemsetAsync(sl.status, 0, sizeof(int) * B, sl.stream));
  std::string ones(sizeof(int) * (size_t)B, '\0');
  for (int i = 0; i < B; ++i) ((int*)ones.data())[i] = 1;
  HIP_TRY(hipMemcpyAsync(h->ro_alive, ones.data(), sizeof(int) * B, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  h->ro_Ts = Ts;
  h->ro_B = B;
  h->ro_valid = true;
  h->have_rows = false;       // the corridor comes from the table
  h->car_rows = false;
  h->discs_live = false;
  h->uploaded = B;
  h->ro_steps = 0;            // the recorder keeps its configuration and starts over
  h->rec_count = 0;
  return MPMPC_OK;
}

// records that steps ro_steps .. ro_steps + n_steps - 1 add (every rec_stride-th step counted from mpmpc_rollout_init)
static long long records_of(const mpmpc_handle_s* h, long long n_steps) {
  const long long st = h->rec_stride, a = h->ro_steps, b = h->ro_steps + n_steps;
  return (b + st - 1) / st - (a + st - 1) / st;
}

int mpmpc_rollout_record(mpmpc_handle h, int32_t B, int32_t capacity, int32_t fields, int32_t stride) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  if (capacity < 0) return fail(MPMPC_E_ARG, "capacity must be >= 0");
  if (stride < 1) return fail(MPMPC_E_ARG, "stride must be >= 1");
  if (fields & ~RO_REC_ALL) return fail(MPMPC_E_ARG, "unknown bits in fields");
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  if (h->rec_buf) { (void)hipFree(h->rec_buf); h->rec_buf = nullptr; }
  h->rec_cap = 0;
  h->rec_count = 0;
  if (capacity == 0) return MPMPC_OK;
  const RoTraceLayout lay = ro_trace_layout(h->cfg.N, B, fields);
  if (!h->rec_ain) HIP_TRY(hipMalloc((void**)&h->rec_ain, sizeof(int) * (size_t)h->cfg.max_batch));
  if (hipMalloc((void**)&h->rec_buf, (size_t)lay.bytes * (size_t)capacity) != hipSuccess) {
    (void)hipGetLastError();
    h->rec_buf = nullptr;
    return fail(MPMPC_E_HIP, "no device memory for " + std::to_string(capacity) + " records of " + std::to_string(lay.bytes) + " bytes");
  }
  h->rec_lay = lay;
  h->rec_cap = capacity;
  h->rec_B = B;
  h->rec_fields = fields;
  h->rec_stride = stride;
  return MPMPC_OK;
}

int mpmpc_rollout_recorded(mpmpc_handle h, int32_t* n_records, int32_t* n_steps) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (n_records) *n_records = h->rec_count;
  if (n_steps) *n_steps = (int32_t)h->ro_steps;
  return MPMPC_OK;
}

// field `off` of records first .. first + count - 1 -> host [count][bytes]: one strided copy
static int pull_field(mpmpc_handle h, void* dst, long long off, size_t bytes, int first, int count) {
  const char* src = h->rec_buf + (size_t)h->rec_lay.bytes * (size_t)first + off;
  if (count == 1) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->last().stream));
  else HIP_TRY(hipMemcpy2DAsync(dst, bytes, src, (size_t)h->rec_lay.bytes, bytes, (size_t)count, hipMemcpyDeviceToHost, h->last().stream));
  return MPMPC_OK;
}

int mpmpc_rollout_trace(mpmpc_handle h, int32_t B, int32_t first, int32_t count, double* s, double* pose, int32_t* wp_id,
                        double* x0, double* u, int32_t* status, int32_t* counter, int32_t* alive, double* plan,
                        double* pred_x, double* pred_y, double* ub, double* lb) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  if (first < 0 || count < 0) return fail(MPMPC_E_ARG, "first and count must be >= 0");
  if (h->rec_cap == 0) return fail(MPMPC_E_STATE, "recording is off (mpmpc_rollout_record)");
  if (B != h->rec_B) return fail(MPMPC_E_STATE, "mpmpc_rollout_record was set up for another number of cars");
  if ((long long)first + count > h->rec_count)
    return fail(MPMPC_E_STATE, "records " + std::to_string(first) + " .. " + std::to_string((long long)first + count - 1) +
                                   " asked for, " + std::to_string(h->rec_count) + " held");
  const RoTraceLayout& l = h->rec_lay;
  if ((plan && l.plan < 0) || ((pred_x || pred_y) && l.pred_x < 0) || ((ub || lb) && l.ub < 0))
    return fail(MPMPC_E_STATE, "a field was asked for that mpmpc_rollout_record did not select");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (count > 0) {
    const size_t N = (size_t)h->cfg.N, nb = (size_t)B;
#define PULL(dst, off, per_car) if (dst) { if (int rc = pull_field(h, dst, off, (per_car) * nb, first, count)) return rc; }
    PULL(s, l.s, 8); PULL(pose, l.pose, 24); PULL(wp_id, l.wp_id, 4); PULL(x0, l.x0, 24); PULL(u, l.u, 16);
    PULL(status, l.status, 4); PULL(counter, l.counter, 4); PULL(alive, l.alive, 4);
    PULL(plan, l.plan, 16 * N); PULL(pred_x, l.pred_x, 8 * (N - 2)); PULL(pred_y, l.pred_y, 8 * (N - 2));
    PULL(ub, l.ub, 8 * N); PULL(lb, l.lb, 8 * N);
#undef PULL
  }
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  return MPMPC_OK;
}

int mpmpc_rollout_set_counters(mpmpc_handle h, int32_t B, const int32_t* counter) {
  if (!h || !counter) return fail(MPMPC_E_ARG, "NULL argument");
  if (int rc = settle(h)) return rc;
  if (B < 1 || B > h->ro_B || !h->ro_valid) return fail(MPMPC_E_STATE, "call mpmpc_rollout_init for at least B cars first");
  for (int i = 0; i < B; ++i)
    if (counter[i] < 0 || counter[i] >= h->cfg.N - 1) return fail(MPMPC_E_ARG, "infeasibility counters must be in [0, N - 2]");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(hipMemcpyAsync(h->ro_counter, counter, sizeof(int) * B, hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  return MPMPC_OK;
}

int mpmpc_rollout_step(mpmpc_handle h, int32_t B, int32_t n_steps) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->ro_B) return fail(MPMPC_E_STATE, "call mpmpc_rollout_init for at least B cars first");
  if (!h->ro_valid)
    return fail(MPMPC_E_STATE, "the rollout's state was overwritten by an upload / solve / assemble on this handle: "
                               "call mpmpc_rollout_init again (or use a second handle for single solves)");
  if (n_steps < 0) return fail(MPMPC_E_ARG, "n_steps must be >= 0");
  const bool per_car = h->obst_B > 0;
  if (per_car) {
    if (h->obst_B != B) return fail(MPMPC_E_STATE, "the per-car obstacles were set for another number of cars");
    if ((h->st_B > 0 && h->obst_gen != h->base_gen) || (h->mv_B > 0 && h->mv_gen != h->base_gen) || h->built_gen != h->base_gen)
      return fail(MPMPC_E_STATE, "map, path or geometry changed since mpmpc_rollout_set_obstacles / mpmpc_build_corridor");
  }
  const bool recording = h->rec_cap > 0;
  if (recording) {
    if (h->rec_B != B) return fail(MPMPC_E_STATE, "mpmpc_rollout_record was set up for another number of cars");
    if (h->rec_count + records_of(h, n_steps) > h->rec_cap)
      return fail(MPMPC_E_STATE, "the trace is full: " + std::to_string(h->rec_count) + " of " + std::to_string(h->rec_cap) +
                                     " records held, this call would add " + std::to_string(records_of(h, n_steps)));
  }
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int blocks = (B + 255) / 256;
  const int N = h->cfg.N;
  const size_t car_lds = sizeof(double) * COR_WPC * N + sizeof(int) * (2 * COR_MAXSEG + 3) * N + sizeof(int) * 3 * COR_MAX_DISCS +
                         (sizeof(int) + 1) * COR_CELL_CAP;
  MapView mv{h->map, h->map_h, h->map_w, h->map_ox, h->map_oy, h->map_res};
  PathGeom pg{h->gx, h->gy, h->gpsi, h->ds_next, h->n_wp, h->cfg.circular, h->gtrig};
  h->have_rows = per_car;     // K1 / K2 read the per-instance rows K0c writes (else: the table)
  const int movers = per_car && h->mv_B > 0 ? h->mv_n : 0;
  const MoverPath mp{h->ro_cum, h->gx, h->gy, h->gtrig, h->n_wp, COR_TRIG, h->cfg.circular ? 1 : 0};
  const double* mv_p = (const double*)h->mv_block;
  const int* mv_i = (const int*)(mv_p + (size_t)MOV_PARAMS * movers);
  for (int t = 0; t < n_steps; ++t) {
    char* rec = recording && h->ro_steps % h->rec_stride == 0 ? h->rec_buf + (size_t)h->rec_lay.bytes * (size_t)h->rec_count : nullptr;
    if (rec)
      hipLaunchKernelGGL(mpmpc_record_snapshot_kernel, dim3((unsigned)(((long)B * RO_REC_BEGIN_ENTRIES + 255) / 256)), dim3(256), 0,
                         sl.stream, B, h->ro_s, h->ro_pose, h->ro_alive, h->rec_ain, rec, h->rec_lay);
    hipLaunchKernelGGL(mpmpc_localise_kernel, dim3(blocks), dim3(256), 0, sl.stream, B, h->n_wp, h->cfg.N,
                       h->cfg.circular ? 1 : 0, h->ro_cum, h->gx, h->gy,
                       h->gpsi, h->ro_s, h->ro_pose, h->ro_alive, h->wp_id, h->x0, h->ro_shift);
    if (movers > 0)
      hipLaunchKernelGGL(mpmpc_obstacle_move_kernel, dim3((movers + 255) / 256), dim3(256), 0, sl.stream, movers, h->ro_steps,
                         h->mv_step0, mv, mp, mv_i, mv_i + movers, mv_p, mv_i + 2 * (size_t)movers, h->obst_discs);
    if (per_car)
      hipLaunchKernelGGL(mpmpc_car_corridor_kernel, dim3(B), dim3(64), car_lds, sl.stream, mv, pg, N, h->built_min_width,
                         h->built_sm, h->segs, h->nseg, h->segs + (size_t)4 * COR_MAXSEG * h->n_wp, h->line_cells,
                         h->line_box, h->obst_off, h->obst_discs, h->wp_id, h->ro_alive, h->ro_flag, h->lb, h->ub);
    if (int rc = launch_solve(h, sl, B, true, false)) return rc;  // (the plant step reads z and the status only)
    hipLaunchKernelGGL(mpmpc_advance_kernel, dim3((B * h->cfg.N + 255) / 256), dim3(256), 0, sl.stream, B, h->cfg.N, h->cfg.wheelbase, h->ro_Ts,
                       h->kappa, h->wp_id, h->x0, sl.status, sl.z, h->cc, h->ro_counter, h->ro_alive, h->ro_pose, h->ro_s,
                       h->ro_u);
    if (rec) {
      const RoRecSrc src{h->ro_alive, h->rec_ain, h->wp_id, sl.status, h->ro_counter, h->x0, h->ro_u, h->cc, sl.z,
                         h->gx, h->gy, h->gtrig, per_car ? h->ub : h->ub_tab, per_car ? h->lb : h->lb_tab,
                         per_car ? (long long)N : (long long)h->n_cols, per_car ? 1 : 0, COR_TRIG, N, h->n_wp, h->cfg.circular ? 1 : 0};
      hipLaunchKernelGGL(mpmpc_record_write_kernel, dim3((unsigned)(((long)B * h->rec_lay.entries + 255) / 256)), dim3(256), 0,
                         sl.stream, B, src, rec, h->rec_lay);
      ++h->rec_count;
    }
    ++h->ro_steps;
  }
  HIP_TRY(hipGetLastError());
  if (n_steps > 0) h->car_rows = h->discs_live = per_car;
  return MPMPC_OK;
}

// Lays out the device's per-car disc lists from the two host-side settings (st_* / mv_*): combined offsets, the static
// discs in place, every mover slot as the absent disc (K0m fills the slots in front of every K0c), and the movers' slot
// indices.  new_mv: the movers' block as mpmpc_rollout_set_movers assembled it ([4][n] doubles, [2][n] ints kind / radius,
// the slots follow on the device), or NULL when the movers did not change (only their slot indices are written anew).
static int sync_disc_lists(mpmpc_handle h, std::vector<char>* new_mv) {
  const int B = h->st_B > 0 ? h->st_B : h->mv_B;
  h->obst_B = B;
  h->discs_live = false;
  if (B == 0) return MPMPC_OK;
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->obst_off) {
    HIP_TRY(hipMalloc((void**)&h->obst_off, sizeof(int) * (mb + 1)));
    HIP_TRY(hipMalloc((void**)&h->obst_discs, sizeof(int) * 3 * COR_MAX_DISCS * mb));
  }
  if (!h->ro_flag) HIP_TRY(hipMalloc((void**)&h->ro_flag, sizeof(int) * mb));
  const int n = h->mv_B > 0 ? h->mv_n : 0;
  h->comb_off.assign((size_t)B + 1, 0);
  std::vector<int32_t> dst((size_t)n);
  mov_combine(B, h->st_B > 0 ? h->st_off.data() : nullptr, h->mv_B > 0 ? h->mv_off.data() : nullptr, h->comb_off.data(),
              dst.data());
  const size_t total = (size_t)h->comb_off[B];
  std::vector<int32_t> discs(3 * total, 0);
  if (h->st_B > 0)
    for (int b = 0; b < B; ++b)
      std::memcpy(discs.data() + 3 * (size_t)h->comb_off[b], h->st_discs.data() + 3 * (size_t)h->st_off[b],
                  sizeof(int32_t) * 3 * (size_t)(h->st_off[b + 1] - h->st_off[b]));
  HIP_TRY(hipMemcpyAsync(h->obst_off, h->comb_off.data(), sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice, sl.stream));
  if (total > 0) HIP_TRY(hipMemcpyAsync(h->obst_discs, discs.data(), sizeof(int) * 3 * total, hipMemcpyHostToDevice, sl.stream));
  if (n > 0) {
    const size_t head = (sizeof(double) * MOV_PARAMS + 2 * sizeof(int)) * (size_t)n;      // parameters, kind, radius
    if (new_mv) {
      if (n > h->mv_cap) {
        if (h->mv_block) { HIP_TRY(hipFree(h->mv_block)); h->mv_block = nullptr; h->mv_cap = 0; }
        HIP_TRY(hipMalloc((void**)&h->mv_block, (sizeof(double) * MOV_PARAMS + 3 * sizeof(int)) * (size_t)n));
        h->mv_cap = n;
      }
      HIP_TRY(hipMemcpyAsync(h->mv_block, new_mv->data(), head, hipMemcpyHostToDevice, sl.stream));
    }
    HIP_TRY(hipMemcpyAsync(h->mv_block + head, dst.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, sl.stream));
  }
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the host vectors leave scope
  return MPMPC_OK;
}

int mpmpc_rollout_set_obstacles(mpmpc_handle h, int32_t B, const int32_t* offsets, const int32_t* discs) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  if (!offsets) {      // no static discs: back to the shared table, unless movers are set
    h->st_B = 0;
    return sync_disc_lists(h, nullptr);
  }
  const char* why = "";
  const bool built = h->built_gen == h->base_gen && h->built_gen != 0 && h->n_cols > 0 && h->line_cells;
  if (int rc = cor_check_obstacles(B, h->cfg.max_batch, offsets, discs, built, h->map_w, h->map_h, &why))
    return fail(rc == -3 ? MPMPC_E_STATE : MPMPC_E_ARG, why);
  if (int rc = mov_check_combined(B, offsets, h->mv_B, h->mv_off.data(), &why))
    return fail(rc == -3 ? MPMPC_E_STATE : MPMPC_E_ARG, why);
  h->st_off.assign(offsets, offsets + (size_t)B + 1);
  h->st_discs.assign(discs, discs + 3 * (size_t)offsets[B]);
  h->st_B = B;
  h->obst_gen = h->base_gen;
  return sync_disc_lists(h, nullptr);
}

int mpmpc_rollout_set_movers(mpmpc_handle h, int32_t B, const int32_t* offsets, const int32_t* kind,
                             const int32_t* radius_cells, const double* params, int64_t step0) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  if (!offsets) {      // no movers
    h->mv_B = 0;
    h->mv_n = 0;
    return sync_disc_lists(h, nullptr);
  }
  const char* why = "";
  const bool built = h->built_gen == h->base_gen && h->built_gen != 0 && h->n_cols > 0 && h->line_cells;
  if (int rc = mov_check_movers(B, h->cfg.max_batch, offsets, kind, radius_cells, params, built, h->st_B, h->st_off.data(), &why))
    return fail(rc == -3 ? MPMPC_E_STATE : MPMPC_E_ARG, why);
  const size_t n = (size_t)offsets[B];
  std::vector<char> blk((sizeof(double) * MOV_PARAMS + 2 * sizeof(int)) * n);
  double* p = (double*)blk.data();
  int32_t* ki = (int32_t*)(p + MOV_PARAMS * n);
  for (size_t j = 0; j < n; ++j) {
    for (int t = 0; t < MOV_PARAMS; ++t) p[(size_t)t * n + j] = params[MOV_PARAMS * j + t];
    ki[j] = kind[j];
    ki[n + j] = radius_cells[j];
  }
  h->mv_off.assign(offsets, offsets + (size_t)B + 1);
  h->mv_B = B;
  h->mv_n = (int)n;
  h->mv_step0 = step0;
  h->mv_gen = h->base_gen;
  return sync_disc_lists(h, &blk);
}

int mpmpc_rollout_obstacles(mpmpc_handle h, int32_t B, int32_t* discs_out, int32_t* offsets_out) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->ro_B || !h->ro_valid) return fail(MPMPC_E_STATE, "call mpmpc_rollout_init for at least B cars first");
  if (!h->car_rows || !h->discs_live || B != h->obst_B)
    return fail(MPMPC_E_STATE, "the last rollout step did not build per-car rows for B cars, or the obstacles / movers were set anew "
                               "since (mpmpc_rollout_set_obstacles / mpmpc_rollout_set_movers)");
  if (offsets_out) std::memcpy(offsets_out, h->comb_off.data(), sizeof(int32_t) * ((size_t)B + 1));
  if (discs_out && h->comb_off[B] > 0) {
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipMemcpyAsync(discs_out, h->obst_discs, sizeof(int) * 3 * (size_t)h->comb_off[B], hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
  }
  return MPMPC_OK;
}

int mpmpc_rollout_corridor(mpmpc_handle h, int32_t B, double* ub, double* lb) {
  if (!h || !ub || !lb) return fail(MPMPC_E_ARG, "NULL argument");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->ro_B || !h->ro_valid) return fail(MPMPC_E_STATE, "call mpmpc_rollout_init for at least B cars first");
  if (!h->car_rows) return fail(MPMPC_E_STATE, "the last rollout step did not build per-car rows (mpmpc_rollout_set_obstacles)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t nb = (size_t)B * h->cfg.N;
  std::vector<int> flag(B);
  HIP_TRY(hipMemcpyAsync(ub, h->ub, sizeof(double) * nb, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipMemcpyAsync(lb, h->lb, sizeof(double) * nb, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipMemcpyAsync(flag.data(), h->ro_flag, sizeof(int) * B, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  for (int b = 0; b < B; ++b)
    if (flag[b] != COR_ROW_OK)
      for (int n = 0; n < h->cfg.N; ++n) ub[(size_t)b * h->cfg.N + n] = lb[(size_t)b * h->cfg.N + n] = std::nan("");
  return MPMPC_OK;
}

int mpmpc_rollout_warm_start(mpmpc_handle h, int32_t enable) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  h->ro_warm = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
  return MPMPC_OK;
}

int mpmpc_rollout_state(mpmpc_handle h, int32_t B, double* s, double* pose, double* cc, int32_t* wp_id, double* x0,
                        double* u_last, int32_t* status, int32_t* counter, int32_t* alive) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->ro_B) return fail(MPMPC_E_STATE, "call mpmpc_rollout_init for at least B cars first");
  if (!h->ro_valid)
    return fail(MPMPC_E_STATE, "the rollout's state was overwritten by an upload / solve / assemble on this handle: "
                               "call mpmpc_rollout_init again");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int N = h->cfg.N;
#define PULL(dst, src, bytes) if (dst) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, sl.stream))
  PULL(s, h->ro_s, sizeof(double) * B);
  PULL(pose, h->ro_pose, sizeof(double) * 3 * B);
  PULL(cc, h->cc, sizeof(double) * 2 * N * B);
  PULL(wp_id, h->wp_id, sizeof(int) * B);
  PULL(x0, h->x0, sizeof(double) * 3 * B);
  PULL(u_last, h->ro_u, sizeof(double) * 2 * B);
  PULL(status, sl.status, sizeof(int) * B);
  PULL(counter, h->ro_counter, sizeof(int) * B);
  PULL(alive, h->ro_alive, sizeof(int) * B);
#undef PULL
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

int mpmpc_upload(mpmpc_handle h, int32_t B, const int32_t* wp_id, const double* x0, const double* cc_prev,
                 const double* lb, const double* ub) {
  if (!h || !wp_id || !x0 || !cc_prev) return fail(MPMPC_E_ARG, "NULL argument");
  if (int rc = settle(h)) return rc;
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (h->n_wp == 0) return fail(MPMPC_E_STATE, "no path set (mpmpc_set_path)");
  if ((lb == nullptr) != (ub == nullptr)) return fail(MPMPC_E_ARG, "lb and ub must both be given or both NULL");
  if (!lb && h->n_cols == 0) return fail(MPMPC_E_STATE, "no corridor rows given and no corridor table set");
  const int N = h->cfg.N;
  for (int i = 0; i < B; ++i) {
    if (wp_id[i] < 0 || wp_id[i] >= h->n_wp) return fail(MPMPC_E_ARG, "wp_id out of range");
    // an open path ends the run when the horizon passes its last waypoint (src/reference_path.py:367-369)
    if (!h->cfg.circular && wp_id[i] + N >= h->n_wp) return fail(MPMPC_E_ARG, "Reached end of path!");
  }
  HIP_TRY(hipSetDevice(h->cfg.device));
  h->ro_valid = false;        // the batch blocks are about to be re-laid out and overwritten
  if (B != h->laid_out) lay_out(h, B);
  const BlockLayout L = block_layout(N, B);
  if (h->stage_in) {
    // through pinned staging: the batch is gathered in the device block's own layout and goes over in one copy.
    // The caller's buffers are free as soon as they are gathered, so nothing waits for the copy here - only the
    // NEXT upload does, before it overwrites the staging buffer.
    if (h->in_flight) HIP_TRY(hipEventSynchronize(h->ev_in));
    char* st = h->stage_in;
    std::memcpy(st + L.wp_id, wp_id, sizeof(int) * B);
    std::memcpy(st + L.x0, x0, sizeof(double) * 3 * B);
    std::memcpy(st + L.cc, cc_prev, sizeof(double) * 2 * N * B);
    if (lb) {
      std::memcpy(st + L.lb, lb, sizeof(double) * N * B);
      std::memcpy(st + L.ub, ub, sizeof(double) * N * B);
    }
    HIP_TRY(hipMemcpyAsync(h->in_block, st, lb ? L.in_end : L.in_end_cc, hipMemcpyHostToDevice, h->last().stream));
    HIP_TRY(hipEventRecord(h->ev_in, h->last().stream));
    h->in_flight = true;
  } else {
    // (no staging block of this size: through the bounce buffer - asynchronous on the device's side, the caller's buffers are
    //  free when the call returns)
    if (int rc = upload_through_bounce(h, h->wp_id, wp_id, sizeof(int) * B)) return rc;
    if (int rc = upload_through_bounce(h, h->x0, x0, sizeof(double) * 3 * B)) return rc;
    if (int rc = upload_through_bounce(h, h->cc, cc_prev, sizeof(double) * 2 * N * B)) return rc;
    if (lb) {
      if (int rc = upload_through_bounce(h, h->lb, lb, sizeof(double) * N * B)) return rc;
      if (int rc = upload_through_bounce(h, h->ub, ub, sizeof(double) * N * B)) return rc;
    }
  }
  h->have_rows = lb != nullptr;
  h->uploaded = B;
  return MPMPC_OK;
}

constexpr size_t BOUNCE_HALF = 8u << 20;
static int upload_through_bounce(mpmpc_handle h, void* dst, const void* src, size_t bytes) {
  if (!h->bounce) {
    HIP_TRY(hipHostMalloc((void**)&h->bounce, 2 * BOUNCE_HALF, hipHostMallocDefault));
    for (auto& e : h->ev_bounce) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  for (size_t off = 0; off < bytes; off += BOUNCE_HALF) {
    const int k = h->bounce_turn;
    if (h->bounce_busy[k]) HIP_TRY(hipEventSynchronize(h->ev_bounce[k]));      // its last copy has left this half
    const size_t n = bytes - off < BOUNCE_HALF ? bytes - off : BOUNCE_HALF;
    char* half = h->bounce + (size_t)k * BOUNCE_HALF;
    std::memcpy(half, static_cast<const char*>(src) + off, n);
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + off, half, n, hipMemcpyHostToDevice, h->last().stream));
    HIP_TRY(hipEventRecord(h->ev_bounce[k], h->last().stream));
    h->bounce_busy[k] = true;
    h->bounce_turn = 1 - k;
  }
  return MPMPC_OK;
}

static int launch_assemble(mpmpc_handle h, int B) {
  PathTables t{h->kappa, h->v_ref, h->ds_next, h->n_wp, h->ub_tab, h->lb_tab, h->n_cols};
  const int total = B * h->ld;
  const int blocks = (total + K1_THREADS - 1) / K1_THREADS;
  // (tuning knob of profiles/k1_timing.py: MPMPC_K1_NT = 0 forces plain stores)
  static const int force_nt = std::getenv("MPMPC_K1_NT") ? std::atoi(std::getenv("MPMPC_K1_NT")) : -1;
  const bool nt = force_nt != 0;
  const size_t k1_lds = h->n_wp <= K1_LDS_WP ? 3 * sizeof(double) * (size_t)h->n_wp : 0;
#define K1_LAUNCH(V)                                                                                                       \
  hipLaunchKernelGGL(mpmpc_assemble_kernel<V>, dim3(blocks), dim3(K1_THREADS), k1_lds, h->last().stream, h->cfg, t, B, h->ld, h->wp_id, \
                     h->x0, h->cc, h->have_rows ? h->lb : nullptr, h->have_rows ? h->ub : nullptr, h->qp)
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
  int* const act = s.warm ? h->ro_act : nullptr;
  const int* const shift = s.warm ? h->ro_shift : nullptr;
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
          go<mpmpc_reduced_kernel<G(), C(), W() != 0>>(a, s.grid, s.block, rn_pad(), fills, act, shift, next, sl.tail_flag, sl.seq, left);
          return true;
        } else return false; }); }); });
      break;
    case MPMPC_K_REDUCED_T:      // K2t: its twin for a terminal cost on the time state (one instance per wave)
      found = s.G == 64 && pick<16, 32>(s.C, [&](auto C) {
        go<mpmpc_reduced_t_kernel<64, C()>>(a, s.grid, s.block, rn_pad(), fills, next, sl.tail_flag, sl.seq);
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
        go<mpmpc_reduced_pair_kernel<G()>>(a, s.grid, s.block, 0, fills, next, sl.tail_flag, sl.seq, left);
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
  a.ain.tab = PathTables{h->kappa, h->v_ref, h->ds_next, h->n_wp, h->ub_tab, h->lb_tab, h->n_cols};
  a.ain.wp_id = h->wp_id; a.ain.x0 = h->x0; a.ain.cc = h->cc;
  a.ain.lb = h->have_rows ? h->lb : nullptr; a.ain.ub = h->have_rows ? h->ub : nullptr;
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
  sl.y_valid = sl.want_y = want_y;
  sl.launch_B = B;
  sl.prm = make_params(h->st);
  sl.plan = plan_solve(h->cfg, h->st, LaunchKnobs{h->force_lanes, h->lean_tail, h->lean_tail_single, h->pipeline, h->ro_warm}, B, closed_loop, kind);
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
  const bool left = *static_cast<volatile unsigned*>(sl.tail_flag) == sl.seq;
  if (int rc = resume(MPMPC_LIST_THIS, left)) return rc;
  sl.tail_expect_empty = !left;
  // (second level: read after a tail that ran late has run)
  const bool left2 = static_cast<volatile unsigned*>(sl.tail_flag)[1] == sl.seq;
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
  if (h->staged_bytes) {
    if (int rc = mpmpc_staged_end(h)) return rc;
  }
  if (B < 1 || B > h->uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (int rc = next_slot(h)) return rc;
  return launch_solve(h, h->last(), B, false, h->resident_y, LAUNCH_PIPELINED);      // one launch: the assembly runs inside K2
}

int mpmpc_set_pipeline(mpmpc_handle h, int32_t depth) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  if (depth < 1 || depth > mpmpc_handle_s::MAX_PIPELINE) return fail(MPMPC_E_ARG, "pipeline depth must be in [1, 8]");
  h->pipeline = launch_streams(depth);      // as many launch slots as the process has hardware queues for, at most (the ring: next_slot)
  return MPMPC_OK;
}

int mpmpc_set_outputs(mpmpc_handle h, int32_t want_y) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;
  h->resident_y = want_y != 0;
  return MPMPC_OK;
}

int mpmpc_solve_resident_timed(mpmpc_handle h, int32_t B, float* ms_assemble, float* ms_solve) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (int rc = settle(h)) return rc;          // (a timed launch runs alone: nothing of an earlier launch is left on the chip)
  Slot& sl = h->last();
  if (B < 1 || B > h->uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
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
  if (B < 1 || B > h->uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
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
  if (B < 1 || B > h->uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
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

// device scratch of mpmpc_speed_profile, kept between calls (a call is a set-up step, and without this its cost was
// allocation: 3.5 of 4 ms for a single path).  One scratch per device, each behind its own mutex: callers on
// different devices neither serialise nor free each other's block.
struct SpScratch {
  std::mutex mu;
  size_t bytes = 0;
  char* block = nullptr;
  hipStream_t stream = nullptr;
};
constexpr int SP_MAX_DEVICES = 64;
static SpScratch g_sp_dev[SP_MAX_DEVICES];

int mpmpc_speed_profile(int32_t device, int32_t B, int32_t n, const double* li, const double* kappa,
                        const double* limits, double eps, double* v, int32_t* status, int32_t* iters) {
  if (B < 1 || n < 2) return fail(MPMPC_E_ARG, "speed profile needs B >= 1 paths of n >= 2 segments");
  if (!li || !kappa || !limits || !v || !status) return fail(MPMPC_E_ARG, "li, kappa, limits, v, status must not be NULL");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MPMPC_E_HIP, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  const size_t vec = sizeof(double) * (size_t)B * n;
  const size_t lds = sizeof(double) * SP_ARRAYS * (size_t)n;
  const size_t lds_wave = sizeof(double) * (SP_ARRAYS + sp_wave_arrays(n)) * (size_t)n;
  const bool wave = lds_wave <= 156 * 1024, small = !wave && B <= 256 && lds <= 64 * 1024;
  // one block: li, kappa, v, limits, status, iters (+ the HBM workspace of the thread-per-path kernel)
  const size_t o_li = 0, o_kappa = vec, o_v = 2 * vec, o_lim = 3 * vec, o_status = o_lim + pad8(sizeof(double) * 5 * B),
               o_iters = o_status + pad8(sizeof(int) * (size_t)B), o_work = o_iters + pad8(sizeof(int) * (size_t)B),
               need = o_work + ((wave || small) ? 0 : vec * SP_ARRAYS);
  if (device >= SP_MAX_DEVICES) return fail(MPMPC_E_ARG, "device ordinal beyond the speed-profile scratch table");
  SpScratch& g_sp = g_sp_dev[device];
  std::lock_guard<std::mutex> lock(g_sp.mu);
  if (g_sp.bytes < need) {
    if (g_sp.block) (void)hipFree(g_sp.block);
    g_sp.block = nullptr; g_sp.bytes = 0;
    HIP_TRY(hipMalloc((void**)&g_sp.block, need));
    g_sp.bytes = need;
  }
  if (!g_sp.stream) HIP_TRY(hipStreamCreate(&g_sp.stream));
  hipStream_t stream = g_sp.stream;
  char* blk = g_sp.block;
  double *d_li = (double*)(blk + o_li), *d_kappa = (double*)(blk + o_kappa), *d_v = (double*)(blk + o_v),
         *d_lim = (double*)(blk + o_lim), *d_work = (double*)(blk + o_work);
  int *d_status = (int*)(blk + o_status), *d_iters = (int*)(blk + o_iters);
  HIP_TRY(hipMemcpyAsync(d_li, li, vec, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_kappa, kappa, vec, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_lim, limits, sizeof(double) * 5 * B, hipMemcpyHostToDevice, stream));
  if (wave) {
    // one wavefront per path (any batch size): lane-parallel arithmetic, cyclic reduction for the tridiagonal solves
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&mpmpc_speed_profile_wave_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_wave));
    hipLaunchKernelGGL(mpmpc_speed_profile_wave_kernel, dim3(B), dim3(64), lds_wave, stream, B, n, d_li, d_kappa, d_lim,
                       eps, d_v, d_status, d_iters);
  } else if (small) {
    hipLaunchKernelGGL(mpmpc_speed_profile_lds_kernel, dim3(B), dim3(64), lds, stream, B, n, d_li, d_kappa, d_lim, eps,
                       d_v, d_status, d_iters);
  } else {
    hipLaunchKernelGGL(mpmpc_speed_profile_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, B, n, d_li, d_kappa, d_lim,
                       eps, d_work, d_v, d_status, d_iters);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(v, d_v, vec, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(status, d_status, sizeof(int) * B, hipMemcpyDeviceToHost, stream));
  if (iters) HIP_TRY(hipMemcpyAsync(iters, d_iters, sizeof(int) * B, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return MPMPC_OK;
}

int mpmpc_sync(mpmpc_handle h) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (h->staged_bytes) return mpmpc_staged_end(h);
  return drain(h);
}

int mpmpc_download(mpmpc_handle h, int32_t B, double* z, double* u0, int32_t* status, int32_t* iters,
                   double* resid, double* y) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (h->staged_bytes) {
    if (int rc = mpmpc_staged_end(h)) return rc;
  }
  if (int rc = drain(h)) return rc;               // (also how the single-call path learns that its launches leave no tail)
  Slot& sl = h->last();
  if (B < 1 || B > h->uploaded) return fail(MPMPC_E_STATE, "B exceeds the uploaded batch");
  if (y && !sl.y_valid)
    return fail(MPMPC_E_STATE, "the last solve launch did not store the multipliers (mpmpc_set_outputs(h, 0) / closed loop)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (h->stage_out && B == h->laid_out) {
    // the whole batch was laid out for this B: one copy of the output block (without y, z when they are not wanted)
    const BlockLayout L = block_layout(h->cfg.N, B);
    char* st = h->stage_out;
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
  char* stage = h->stage_out;
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
  if (!h->stage_in || !h->stage_out) return fail(MPMPC_E_STATE, "this handle has no staging blocks (max_batch above the staging limit)");
  // The blocks are the ones mpmpc_upload / mpmpc_download stage through: an upload still on its way out of the input block
  // must have left it before the caller may write there, and a begun staged call owns both blocks
  if (int rc = settle(h)) return rc;
  if (h->in_flight) { HIP_TRY(hipEventSynchronize(h->ev_in)); h->in_flight = false; }
  const BlockLayout L = block_layout(h->cfg.N, B);
  char *si = h->stage_in, *so = h->stage_out;
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
  if (!h->staged_bytes) return MPMPC_OK;
  const size_t out_bytes = h->staged_bytes;
  Slot& sl = h->last();
  if (int rc = drain(h)) return rc;                 // drains the streams; a launch that left a deferred tail has it run now
  h->staged_bytes = 0;                              // (only now: an error above leaves the call begun)
  if (sl.tail_ran_late) {
    HIP_TRY(hipMemcpyAsync(h->stage_out, sl.out_block, out_bytes, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
  }
  return MPMPC_OK;
}

int mpmpc_solve_staged(mpmpc_handle h, int32_t B, int32_t with_rows, int32_t want_z, int32_t want_y) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  h->staged_async = false;          // one call, waited for at once: the packing of a single launch
  const int rc = mpmpc_staged_begin(h, B, with_rows, want_z, want_y);
  h->staged_async = true;
  if (rc) return rc;
  return mpmpc_staged_end(h);
}

int mpmpc_staged_begin(mpmpc_handle h, int32_t B, int32_t with_rows, int32_t want_z, int32_t want_y) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (h->staged_bytes) return fail(MPMPC_E_STATE, "mpmpc_staged_begin: the previous one has not been ended");
  if (int rc = settle(h)) return rc;
  Slot& sl = h->last();
  if (B < 1 || B > h->cfg.max_batch) return fail(MPMPC_E_ARG, "B must be in [1, max_batch]");
  if (!h->stage_in || !h->stage_out) return fail(MPMPC_E_STATE, "this handle has no staging blocks (max_batch above the staging limit)");
  if (h->n_wp == 0) return fail(MPMPC_E_STATE, "no path set (mpmpc_set_path)");
  if (!with_rows && h->n_cols == 0) return fail(MPMPC_E_STATE, "no corridor rows given and no corridor table set");
  const int N = h->cfg.N;
  const BlockLayout L = block_layout(N, B);
  const int32_t* wp = reinterpret_cast<const int32_t*>(h->stage_in + L.wp_id);
  for (int i = 0; i < B; ++i) {
    if (wp[i] < 0 || wp[i] >= h->n_wp) return fail(MPMPC_E_ARG, "wp_id out of range");
    if (!h->cfg.circular && wp[i] + N >= h->n_wp) return fail(MPMPC_E_ARG, "Reached end of path!");
  }
  HIP_TRY(hipSetDevice(h->cfg.device));
  if (h->in_flight) { HIP_TRY(hipEventSynchronize(h->ev_in)); h->in_flight = false; }
  h->ro_valid = false;
  if (B != h->laid_out) lay_out(h, B);
  HIP_TRY(hipMemcpyAsync(h->in_block, h->stage_in, with_rows ? L.in_end : L.in_end_cc, hipMemcpyHostToDevice, sl.stream));
  h->have_rows = with_rows != 0;
  h->uploaded = B;
  if (int rc = launch_solve(h, sl, B, false, want_y != 0, h->staged_async ? LAUNCH_PIPELINED : LAUNCH_SINGLE)) return rc;
  const size_t out_bytes = want_y ? L.out_end : (want_z ? L.out_end_z : L.z);
  HIP_TRY(hipMemcpyAsync(h->stage_out, sl.out_block, out_bytes, hipMemcpyDeviceToHost, sl.stream));
  h->staged_bytes = out_bytes;
  return MPMPC_OK;
}

int mpmpc_assemble(mpmpc_handle h, int32_t B, const int32_t* wp_id, const double* x0, const double* cc_prev,
                   const double* lb, const double* ub, double* qp_out) {
  if (int rc = mpmpc_upload(h, B, wp_id, x0, cc_prev, lb, ub)) return rc;
  if (int rc = launch_assemble(h, B)) return rc;
  if (qp_out) {
    // device layout is [field][B][ld]; rows of B*ld doubles per field are contiguous
    HIP_TRY(hipMemcpyAsync(qp_out, h->qp, sizeof(double) * MPMPC_NUM_FIELDS * (size_t)B * h->ld,
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
