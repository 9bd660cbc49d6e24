// CPU lock-step emulation of the general solve kernel for horizons above 63 (TEST INFRASTRUCTURE ONLY).
// On the device such an instance takes a WORKGROUP of 2 / 4 wavefronts - one lane per stage, neighbours across the wavefront
// boundaries through LDS (lane_gpu.hpp: LaneBlock<128> / LaneBlock<256>, mpmpc_solve_block_kernel); here the same lane code
// (mpmpc_core.hpp: Solver) runs on an emulated execution group of MPMPC_EMU_W = 128 / 256 lanes.  Built twice
// (tests/emul/Makefile: libmpmpc_emul_w128.so, libmpmpc_emul_w256.so).  Never loaded by the product.
#include <cstring>
#define MPMPC_TICK_BEGIN(i) ((void)0)
#define MPMPC_TICK_END(i) ((void)0)
#define MPMPC_TICK_COUNT(i) ((void)0)
#include "lane_emu.hpp"
#include "lane_pair.hpp"
#include "mpmpc_core.hpp"
#include "mpmpc_reduced.hpp"
#include "mpmpc_reduced_t.hpp"
#include "mpmpc_reduced_tail.hpp"

using namespace mpmpc;
#include "wave_loop.hpp"
static_assert(EMU_W == 128 || EMU_W == 256, "build with -DMPMPC_EMU_W=128 or 256");

// (a chain of the 128-lane workgroup is a wavefront: the reduced variant factors it by cyclic reduction, as on the device)
static_assert(EMU_W != 128 || Solver<LaneEmu<EMU_W, EMU_W / 2>, false, true, false, true>::kCR64, "cyclic reduction of 64-lane chains");
static_assert(EMU_W != 256 || Solver<LaneEmu<EMU_W, EMU_W / 2>, false, true, false, true>::kCRrows == 8, "256 lanes: chains of eight rows");

using LW = LaneEmu<EMU_W, EMU_W / 2>;          // one lane per stage, two chains that meet in the middle (LaneBlock<EMU_W>)

// mpmpc_solve_block_kernel<EMU_W, VAR>: every instance, the whole solve (list = null) - or, on the instances of a list, straight
// to phase 1 and the full iteration (mode 2): what follows the reduced-native kernels
template <int VAR>
static void solve_wide(const Problem& p, const Outputs& o, const ListOrder* list = nullptr) {
  using S = Solver<LW, VAR == 1, VAR == 2, false, VAR == 2>;      // (cyclic reduction where a chain is a wavefront)
  const int N = p.cfg->N, ld = stage_ld(N);
  double woff7[7];
  weight_offdiag(*p.cfg, woff7);
  auto solve = [&](S& s, const VD* fields, const VI& inst, const VI& k) {
    const VI base = list ? spent_ipm(o.iters, inst, p.B) : VI(0);
    s.template run<false, true>(fields, p.B, inst, k, N, make_params(*p.st), list ? 2 : 0, VI(0), base, VAR == 1 ? woff7 : nullptr);
    s.store(inst, k, p.cfg->wheelbase, o.z, o.u0, o.status, o.iters, o.resid, o.y, nullptr, ld);
  };
  if (list) wave_loop<S, LW>(p, *list, nullptr, solve);
  else wave_loop<S, LW>(p, BatchOrder{}, nullptr, solve);
}

// the tail alone: mpmpc_solve_block_kernel<G, VAR> on the listed instances - what follows the reduced-native kernels with two
// stages per lane (horizons 64 .. 127 in one wavefront: emul.cpp)
extern "C" int emuw_solve_tail(const mpmpc_config* cfg, const mpmpc_settings* st, const double* qp, int B, double* z, double* u0,
                               int* status, int* iters, double* resid, double* y, const int* ids, int n_ids) {
  if (stage_ld(cfg->N) != EMU_W || full_weights(*cfg)) return -1;
  const Problem p{cfg, st, qp, B};
  const Outputs o{z, u0, status, iters, resid, y};
  const ListOrder list(ids, n_ids);
  if (reducible(*cfg, *st)) solve_wide<2>(p, o, &list);
  else solve_wide<0>(p, o, &list);      // (the terminal-time kernel's tail: the full problem)
  return 0;
}

// Horizons 128 .. 255 with TWO stages per lane: the instance on an emulated workgroup of 128 lanes - one chain of eight rows over
// two wavefronts (the 128-lane build only; -1 from the other).  ids <- the instances a kernel leaves UNSOLVED (*n of them): they
// go to the general solver on 256 lanes (the 256-lane build's emuw_solve_tail).
#if MPMPC_EMU_W == 128
using LWPair = LanePair<LaneEmu<128, 128>>;                 // the full cold storage: one workgroup per CU
using LWPairLean = LanePair<LaneEmu<128, 128, 74>>;         // 37 pair slots: the lean cold storage of the device kernel
static_assert(ReducedSolver<LWPairLean>::kLean, "lean cold storage");
#endif
// mpmpc_reduced_pair_block_kernel
extern "C" int emuw_solve_rn_pair(const mpmpc_config* cfg, const mpmpc_settings* st, const double* qp, int B, double* z, double* u0,
                                  int* status, int* iters, double* resid, double* y, int* ids, int* n) {
#if MPMPC_EMU_W == 128
  if (stage_ld(cfg->N) != 256 || full_weights(*cfg) || !reduced_native(*cfg, *st)) return -1;
  std::vector<int> tail;
  solve_rn<LWPairLean>({cfg, st, qp, B}, {z, u0, status, iters, resid, y}, tail);
  list_out(tail, ids, n);
  return 0;
#else
  return -1;
#endif
}
// ... its twin for a terminal cost on the time state (mpmpc_reduced_t_pair_block_kernel)
extern "C" int emuw_solve_rnt_pair(const mpmpc_config* cfg, const mpmpc_settings* st, const double* qp, int B, double* z, double* u0,
                                   int* status, int* iters, double* resid, double* y, int* ids, int* n) {
#if MPMPC_EMU_W == 128
  if (stage_ld(cfg->N) != 256 || full_weights(*cfg) || !reduced_native_tt(*cfg, *st)) return -1;
  std::vector<int> tail;
  solve_rnt<LWPair>({cfg, st, qp, B}, {z, u0, status, iters, resid, y}, tail);
  list_out(tail, ids, n);
  return 0;
#else
  return -1;
#endif
}
// ... and the reduced-native TAIL solver on the same workgroup, on a list of instances (mpmpc_reduced_tail_pair_block_kernel);
// ids2 <- what it leaves
extern "C" int emuw_solve_rn_tail_pair(const mpmpc_config* cfg, const mpmpc_settings* st, const double* qp, int B, double* z, double* u0,
                                       int* status, int* iters, double* resid, double* y, const int* ids, int n_ids, int* ids2, int* n2) {
#if MPMPC_EMU_W == 128
  if (stage_ld(cfg->N) != 256 || !reduced_native_tail(*cfg, *st)) return -1;
  std::vector<int> tail2;
  solve_rn_tail<LWPair>({cfg, st, qp, B}, {z, u0, status, iters, resid, y}, ListOrder(ids, n_ids), tail2);
  list_out(tail2, ids2, n2);
  return 0;
#else
  return -1;
#endif
}

// the kernel the launcher picks for a horizon above 63: the general solver, one instance per workgroup; full weights
// where a weight matrix has off-diagonal entries, the reduced polish where the time state separates.  -1: the horizon does not belong to this width.
extern "C" int emuw_width() { return EMU_W; }
extern "C" int emuw_solve(const mpmpc_config* cfg, const mpmpc_settings* st, const double* qp, int B, double* z, double* u0,
                          int* status, int* iters, double* resid, double* y) {
  if (stage_ld(cfg->N) != EMU_W) return -1;
  const Problem p{cfg, st, qp, B};
  const Outputs o{z, u0, status, iters, resid, y};
  if (full_weights(*cfg)) solve_wide<1>(p, o);
  else if (reduced_native(*cfg, *st)) {
    // the launcher's sequence for the reference's own weights at the default settings: the reduced-native solver on the workgroup
    // first (mpmpc_reduced_block_kernel), then the general one (mode 2) on what that could not certify
    std::vector<int> tail;
    solve_rn<LW>(p, o, tail);
    const ListOrder list(tail);
    solve_wide<2>(p, o, &list);
  } else if (reducible(*cfg, *st)) solve_wide<2>(p, o);      // (the launcher's choice: mpmpc_hip.hip, launch_solve)
  else solve_wide<0>(p, o);
  return 0;
}
