// CPU lock-step emulation of the HIP kernels (TEST INFRASTRUCTURE ONLY).
// Instantiates the lane-generic core of multi-purpose-mpc_amd/csrc/mpmpc_core.hpp with the
// 64-lane emulated wavefront of lane_emu.hpp so the kernel algorithm can be checked against
// the oracle in the GPU-less authoring container.  Never loaded by the product.
#include <cstring>
#include <initializer_list>
// event counters of the solver code (the phase-clock build of the library counts the same events per wave):
// 16 interior-point iterations, 17 active-set rounds, 18 active-set KKT solves - per emulated wave
static long long g_emu_count[32];
#define MPMPC_TICK_BEGIN(i) ((void)0)
#define MPMPC_TICK_END(i) ((void)0)
#define MPMPC_TICK_COUNT(i) (++g_emu_count[i])
#include "lane_emu.hpp"
#include "lane_pair.hpp"
#include "mpmpc_core.hpp"
#include "mpmpc_reduced.hpp"
#include "mpmpc_reduced_t.hpp"
#include "mpmpc_reduced_tail.hpp"
#include "corridor_core.hpp"
#include "rollout_core.hpp"
#include <limits>

using namespace mpmpc;
#include "wave_loop.hpp"

// mode / tail as in mpmpc_solve_kernel: mode 1 appends the instances it leaves UNSOLVED to tail, mode 2 runs one wave per
// instance listed in it
template <int G, int C, bool FQ = false, bool RED = false, bool FREEX = false>
static void solve_g(const Problem& p, const Outputs& o, const int* guess = nullptr, int* act = nullptr, int mode = 0,
                    std::vector<int>* tail = nullptr) {
  using L = LaneEmu<G, C>;
  using S = Solver<L, FQ, RED, FREEX, RED>;
  const int N = p.cfg->N, ld = stage_ld(N);
  double woff7[7];
  weight_offdiag(*p.cfg, woff7);
  const double* woff = FQ ? woff7 : nullptr;
  auto solve = [&](S& s, const VD* fields, const VI& inst, const VI& k) {
    const VI base = mode == 2 ? spent_ipm(o.iters, inst, p.B) : VI(0);
    // (like the device: the packed kernels carry no phase-1 code when they run as the first of two launches)
    if (guess) s.template run<true>(fields, p.B, inst, k, N, make_params(*p.st), mode, warm_guess(guess, ld, inst, k, p.B, N), base, woff);
    else if (mode == 1) s.template run<false, (G == 64)>(fields, p.B, inst, k, N, make_params(*p.st), mode, VI(0), base, woff);
    else s.template run<false, true>(fields, p.B, inst, k, N, make_params(*p.st), mode, VI(0), base, woff);
    s.store(inst, k, p.cfg->wheelbase, o.z, o.u0, o.status, o.iters, o.resid, o.y, act, ld);
  };
  if (mode == 2) wave_loop<S, L>(p, ListOrder(*tail), nullptr, solve);
  else wave_loop<S, L>(p, BatchOrder{}, mode == 1 ? tail : nullptr, solve);
}

// run-time (G, N) -> the <G, C> instantiation the launcher picks for G lanes per instance; -1: no such layout
template <int G_, int C_> struct Layout { static constexpr int G = G_, C = C_; };
template <class F>
static int with_layout(int G, int N, F&& f) {
  const int C = lane_split(G, N);
  if (G == 64 && C == 16) f(Layout<64, 16>{});
  else if (G == 64) f(Layout<64, 32>{});
  else if (G == 32) f(Layout<32, 16>{});
  else if (G == 16) f(Layout<16, 16>{});
  else return -1;
  return 0;
}
// the general kernel in the variant the launcher would pick: reduced polish where the configuration allows it, free e_psi / t
// (one instance per wave only)
static int solve_general(int G, const Problem& p, const Outputs& o, const int* guess = nullptr, int* act = nullptr, int mode = 0,
                         std::vector<int>* tail = nullptr) {
  return with_layout(G, p.cfg->N, [&](auto l) {
    constexpr int g = decltype(l)::G, c = decltype(l)::C;
    if (reducible(*p.cfg, *p.st)) solve_g<g, c, false, true>(p, o, guess, act, mode, tail);
    else if (g == 64 && free_states(*p.cfg)) solve_g<g, c, false, false, (g == 64)>(p, o, guess, act, mode, tail);
    else solve_g<g, c>(p, o, guess, act, mode, tail);
  });
}
// the reduced-native kernel for G lanes per instance (CR = false: the chain-sequential elimination, A/B in the tests)
template <bool CR = true>
static int solve_rn_g(int G, const Problem& p, const Outputs& o, std::vector<int>& tail, const int* guess = nullptr, int* act = nullptr) {
  const int N = p.cfg->N;
  // 16 lanes for more than 16 stages, 64 for more than 64 (mpmpc_reduced_pair_kernel; on the one-stage layout the latter take a
  // workgroup of two, emul_wide.cpp): TWO stages per lane - cold starts only, like the launcher
  if ((G == 16 || G == 64) && N + 1 > G) {
    if (guess || N + 1 > 2 * G) return -1;
    if (G == 16) solve_rn<LanePair<LaneEmu<16, 16>>>(p, o, tail);
    else solve_rn<LanePair<LaneEmu<64, 64>>>(p, o, tail);
    return 0;
  }
  return with_layout(G, N, [&](auto l) { solve_rn<LaneEmu<decltype(l)::G, decltype(l)::C>, CR>(p, o, tail, guess, act); });
}
// ... its twin for a terminal cost on the time state: one instance per wave whatever packing the caller asked for (the launcher
// does the same); horizons 64 .. 127 with two stages per lane (mpmpc_reduced_t_pair_kernel<64>)
template <bool CR = true>
static int solve_rnt_g(const Problem& p, const Outputs& o, std::vector<int>& tail) {
  const int N = p.cfg->N;
  if (N + 1 > 64) {
    if (N + 1 > 128) return -1;
    solve_rnt<LanePair<LaneEmu<64, 64>>>(p, o, tail);
    return 0;
  }
  return with_layout(64, N, [&](auto l) { solve_rnt<LaneEmu<64, decltype(l)::C>, CR>(p, o, tail); });
}

static int g_emu_lean_tail = 1;          // emu_set_lean_tail, like mpmpc_set_tail_kernel: 0 = the general kernel takes the whole
                                         // tail (as before round 4); 1 = the tail solver, TWO instances per wave (32 lanes each,
                                         // three entries per lane: the device's default); 2 = the tail solver, one instance per wave
// the reduced-native tail solver (pair layout: mpmpc_reduced_tail_pair_kernel<64>, horizons 64 .. 127, one instance per emulated
// wavefront) on a list of instances; ids2 <- what it leaves (n2 of them)
extern "C" int emu_solve_rn_tail_pair(const mpmpc_config* cfg, const mpmpc_settings* st, const double* qp, int B, double* z, double* u0,
                                      int* status, int* iters, double* resid, double* y, const int* ids, int n_ids, int* ids2, int* n2) {
  if (cfg->N + 1 <= 64 || cfg->N + 1 > 128 || !reduced_native_tail(*cfg, *st)) return -1;
  std::vector<int> tail2;
  solve_rn_tail<LanePair<LaneEmu<64, 64>>>({cfg, st, qp, B}, {z, u0, status, iters, resid, y}, ListOrder(ids, n_ids), tail2);
  list_out(tail2, ids2, n2);
  return 0;
}
extern "C" void emu_set_lean_tail(int on) { g_emu_lean_tail = on; }
extern "C" int emu_reduced_native_tail(const mpmpc_config* cfg, const mpmpc_settings* st) { return reduced_native_tail(*cfg, *st) ? 1 : 0; }
static int g_emu_tail2 = 0;              // instances the last emu_solve_launch's reduced-native tail solver left to the general kernel
extern "C" int emu_last_tail2() { return g_emu_tail2; }

extern "C" int emu_solve(const mpmpc_config* cfg, const mpmpc_settings* st, int G, const double* qp, int B,
                         double* z, double* u0, int* status, int* iters, double* resid, double* y) {
  const Problem p{cfg, st, qp, B};
  const Outputs o{z, u0, status, iters, resid, y};
  if (cfg->N + 1 > G) return -1;
  if (!full_weights(*cfg)) return solve_general(G, p, o);
  if (G != 64) return -1;          // Q, R or QN with off-diagonal entries: the launcher gives such instances a wave each
  return with_layout(64, cfg->N, [&](auto l) { solve_g<64, decltype(l)::C, true>(p, o); });
}

// what launch_solve does with a packed batch (G < 64 and an early polish attempt): the packed kernel in mode 1, then
// the <64, C> kernel in mode 2 on the instances it left unsolved (phase 1, full ADMM run); otherwise one launch.
extern "C" int emu_solve_launch(const mpmpc_config* cfg, const mpmpc_settings* st, int G, const double* qp, int B,
                                double* z, double* u0, int* status, int* iters, double* resid, double* y, int* n_tail) {
  const Problem p{cfg, st, qp, B};
  const Outputs o{z, u0, status, iters, resid, y};
  if (cfg->N + 1 > G && !(G == 16 && cfg->N + 1 <= 32 && reduced_native(*cfg, *st))) return -1;      // (two stages per lane)
  const bool early = st->polish && st->early_polish > 0 && st->early_polish < st->max_iter;
  if (n_tail) *n_tail = 0;
  std::vector<int> tail;
  if (reduced_native(*cfg, *st) || reduced_native_tt(*cfg, *st)) {
    // the reduced-native kernel for the whole batch (any packing), then the general kernel on its tail
    if (reduced_native_tt(*cfg, *st) ? solve_rnt_g(p, o, tail) : solve_rn_g(G, p, o, tail)) return -1;
    if (n_tail) *n_tail = (int)tail.size();
    if (g_emu_lean_tail && !reduced_native_tt(*cfg, *st) && reduced_native_tail(*cfg, *st)) {
      // the reduced-native tail solver first; the general kernel on what that leaves
      std::vector<int> tail2;
      if (lane_split(64, cfg->N) == 32) solve_rn_tail<LaneEmu<64, 32>>(p, o, tail, tail2);
      else if (g_emu_lean_tail != 2) solve_rn_tail<LaneEmu<32, 16>>(p, o, tail, tail2);
      else solve_rn_tail<LaneEmu<64, 16>>(p, o, tail, tail2);
      tail.swap(tail2);
    }
    g_emu_tail2 = (int)tail.size();
    return solve_general(64, p, o, nullptr, nullptr, 2, &tail);
  }
  if (G == 64 || !early) return emu_solve(cfg, st, G, qp, B, z, u0, status, iters, resid, y);
  if (G != 32 && G != 16) return -1;
  solve_general(G, p, o, nullptr, nullptr, 1, &tail);
  if (n_tail) *n_tail = (int)tail.size();
  return solve_general(64, p, o, nullptr, nullptr, 2, &tail);
}

// the reduced-native kernel alone: what it cannot certify stays UNSOLVED and is counted in *n_tail
template <bool CR>
static int solve_rn_alone(int G, const Problem& p, const Outputs& o, int* n_tail) {
  std::vector<int> tail;
  if (reducible_tt(*p.cfg, *p.st)) {          // the terminal-time kernels (one instance per wave)
    if (solve_rnt_g<CR>(p, o, tail)) return -1;
  } else if (!reducible(*p.cfg, *p.st) || solve_rn_g<CR>(G, p, o, tail)) return -1;
  if (n_tail) *n_tail = (int)tail.size();
  return 0;
}
extern "C" int emu_solve_rn(const mpmpc_config* cfg, const mpmpc_settings* st, int G, const double* qp, int B,
                            double* z, double* u0, int* status, int* iters, double* resid, double* y, int* n_tail) {
  if (cfg->N + 1 > G && !((G == 16 || G == 64) && cfg->N + 1 <= 2 * G && (reducible(*cfg, *st) || (G == 64 && reducible_tt(*cfg, *st))))) return -1;
  return solve_rn_alone<true>(G, {cfg, st, qp, B}, {z, u0, status, iters, resid, y}, n_tail);
}
// the same kernel with the SEQUENTIAL elimination of the chains (the cyclic-reduction form is what ships): A/B in the tests
extern "C" int emu_solve_rn_sequential(const mpmpc_config* cfg, const mpmpc_settings* st, int G, const double* qp, int B,
                                       double* z, double* u0, int* status, int* iters, double* resid, double* y, int* n_tail) {
  if (cfg->N + 1 > G) return -1;
  return solve_rn_alone<false>(G, {cfg, st, qp, B}, {z, u0, status, iters, resid, y}, n_tail);
}
extern "C" int emu_reduced_native(const mpmpc_config* cfg, const mpmpc_settings* st) { return reduced_native(*cfg, *st) ? 1 : 0; }
extern "C" int emu_reduced_native_tt(const mpmpc_config* cfg, const mpmpc_settings* st) { return reduced_native_tt(*cfg, *st) ? 1 : 0; }

// the closed-loop variant: `guess` [B x ld] = active sets to start from (bit 30 = valid), `act` [B x ld] <- the
// active sets of the certified points (what mpmpc_solve_kernel<..., true> reads and writes in a rollout)
extern "C" int emu_solve_warm(const mpmpc_config* cfg, const mpmpc_settings* st, int G, const double* qp, int B,
                              const int* guess, double* z, double* u0, int* status, int* iters, double* resid,
                              double* y, int* act) {
  const Problem p{cfg, st, qp, B};
  const Outputs o{z, u0, status, iters, resid, y};
  if (cfg->N + 1 > G) return -1;
  if (reduced_native(*cfg, *st)) {
    // what the launcher runs in a warm-started closed-loop step: the reduced-native kernel with the guesses, then the
    // general kernel (no guess) on its tail
    std::vector<int> tail;
    if (solve_rn_g(G, p, o, tail, guess, act)) return -1;
    return solve_general(64, p, o, nullptr, nullptr, 2, &tail);
  }
  if (G != 64) return -1;          // the general kernels run one instance per wave
  return solve_general(64, p, o, guess, act);
}

extern "C" int emu_assemble(const mpmpc_config* cfg, int n_wp, const double* kappa, const double* v_ref,
                            const double* ds_next, int n_cols, const double* ub_tab, const double* lb_tab, int B,
                            const int* wp_id, const double* x0, const double* cc, const double* lb,
                            const double* ub, double* qp) {
  using L = LaneEmu<64>;
  PathTables t{kappa, v_ref, ds_next, n_wp, ub_tab, lb_tab, n_cols};
  const int ld = stage_ld(cfg->N);
  const int total = B * ld;
  for (int t0 = 0; t0 < total; t0 += EMU_W) {
    VI inst, k;
    for (int i = 0; i < EMU_W; ++i) { inst.v[i] = (t0 + i) / ld; k.v[i] = (t0 + i) % ld; }
    assemble_lane<L>(*cfg, t, B, ld, inst, k, wp_id, x0, cc, lb, ub, qp);
  }
  return 0;
}

extern "C" int emu_stage_ld(int N) { return stage_ld(N); }
extern "C" void emu_event_counts(long long* out32, int reset) {
  for (int i = 0; i < 32; ++i) { out32[i] = g_emu_count[i]; if (reset) g_emu_count[i] = 0; }
}

// instruction census of everything executed since the last reset (only with -DMPMPC_COUNT_OPS)
// out7: wave instructions by class, all contexts together
extern "C" int emu_op_count(long long* out7, int reset) {
#ifdef MPMPC_COUNT_OPS
  OpCensus& s = op_census();
  for (int i = 0; i < 7; ++i) out7[i] = 0;
  for (int m = 0; m < 3; ++m) {
    const OpCount& c = s.c[m];
    out7[0] += c.fma; out7[1] += c.addmul; out7[2] += c.div; out7[3] += c.sqrt; out7[4] += c.cmpsel; out7[5] += c.shift; out7[6] += c.reduce;
  }
  if (reset) s = OpCensus{};
  return 1;
#else
  (void)out7; (void)reset;
  return 0;
#endif
}
// out4: FP64 flops (FMA = 2) of the wave instructions by context - lane-parallel, lane-parallel in the split layout,
// inside serial sweeps (as executed) - and the flops of ONE step per serial sweep (what a stage needs of it)
extern "C" int emu_op_flops(double* out4, int reset) {
#ifdef MPMPC_COUNT_OPS
  OpCensus& s = op_census();
  out4[0] = double(op_flops(s.c[0])); out4[1] = double(op_flops(s.c[1])); out4[2] = double(op_flops(s.c[2]));
  out4[3] = s.serial_useful;
  if (reset) s = OpCensus{};
  return 1;
#else
  (void)out4; (void)reset;
  return 0;
#endif
}

// Structure-exploiting flop count of the two linear-algebra pieces every iteration is made of, measured on the
// counting build: one factor() and one kkt_solve() of a <64,16> instance of horizon N with unit data.
// out4: factor lane-parallel, factor one-serial-step, kkt_solve lane-parallel, kkt_solve one-step-per-sweep (summed)
extern "C" int emu_census_pieces(int N, double* out4) {
#ifdef MPMPC_COUNT_OPS
  using L = LaneEmu<64, 16>;
  if (N + 1 > 32) return 0;
  Solver<L> s;
  typename L::real fields[MPMPC_NUM_FIELDS];
  for (int f = 0; f < MPMPC_NUM_FIELDS; ++f) fields[f] = VD(f == F_DS ? 0.05 : (f >= F_P ? 1.0 : (f >= F_HI && f < F_Q ? 1.0 : (f >= F_LO && f < F_HI ? -1.0 : 0.01))));
  VI inst(0), k = L::stage() - lane_offset(64, 16, N);
  s.load(fields, 1, inst, k, N);
  VD h[5], rx[5], req[3], xt[5], nu[3];
  for (int j = 0; j < 5; ++j) { h[j] = VD(0.5); rx[j] = VD(1.0); }
  for (int i = 0; i < 3; ++i) req[i] = VD(1.0);
  double o[4];
  op_census() = OpCensus{};
  s.factor(h, VD(1e-3));
  out4[0] = double(op_flops(op_census().c[0])); out4[1] = op_census().serial_useful;
  op_census() = OpCensus{};
  s.kkt_solve(rx, req, xt, nu);
  out4[2] = double(op_flops(op_census().c[0])); out4[3] = op_census().serial_useful;
  op_census() = OpCensus{};
  (void)o;
  return 1;
#else
  (void)N; (void)out4;
  return 0;
#endif
}

// returns the number of start waypoints without a free segment (>= 0), or: -3000 a border cell outside the map,
// -3001 more than COR_MAXSEG free segments on a line (what mpmpc_build_corridor reports as errors), -1000 the two
// forms of the column walk disagree
extern "C" int emu_corridor(int height, int width, const int8_t* data, double ox, double oy, double res, int n_wp,
                            const double* x, const double* y, const double* psi, const double* ds_next, int circular,
                            const double* bub, const double* blb, int n_cols, double min_width, double safety_margin,
                            double* ub_tab, double* lb_tab, int* nseg_out) {
  MapView mv{data, height, width, ox, oy, res};
  std::vector<double> trig((size_t)n_wp * COR_TRIG);
  for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
  PathGeom pg{x, y, psi, ds_next, n_wp, circular, trig.data()};
  for (int i = 0; i < n_wp; ++i) {
    int cx, cy;
    cor_w2m(mv, bub[2 * i], bub[2 * i + 1], cx, cy);
    if (cx < 0 || cx >= width || cy < 0 || cy >= height) return -3000;
    cor_w2m(mv, blb[2 * i], blb[2 * i + 1], cx, cy);
    if (cx < 0 || cx >= width || cy < 0 || cy >= height) return -3000;
  }
  double* segs = new double[(size_t)n_wp * 4 * COR_MAXSEG]();
  int* nseg = new int[n_wp];
  for (int i = 0; i < n_wp; ++i) {
    nseg[i] = cor_free_segments(mv, bub[2 * i], bub[2 * i + 1], blb[2 * i], blb[2 * i + 1], min_width, segs + (size_t)i * 4 * COR_MAXSEG);
    if (nseg[i] < 0) { delete[] segs; delete[] nseg; return -3001; }
    // the staged form the device runs (cells of the line as packed 16-bit pairs, then the scan over the copy) must
    // give the same bits
    {
      int cells[COR_CELL_CAP];
      double seg2[4 * COR_MAXSEG] = {0};
      int ux, uy, lx, ly;
      cor_w2m(mv, bub[2 * i], bub[2 * i + 1], ux, uy);
      cor_w2m(mv, blb[2 * i], blb[2 * i + 1], lx, ly);
      const int n = cor_line_cells(ux, uy, lx, ly, cells, COR_CELL_CAP);
      if (n <= COR_CELL_CAP) {
        const int c2 = cor_scan_cells(mv, ux, uy, lx, ly, min_width, n, [&](int c, int& cx, int& cy) { cor_unpack_cell(cells[c], cx, cy); },
                                      [&](int c) { int cx, cy; cor_unpack_cell(cells[c], cx, cy); return cor_cell_free(mv, cx, cy); }, seg2);
        if (c2 != nseg[i] || std::memcmp(seg2, segs + (size_t)i * 4 * COR_MAXSEG, sizeof(double) * 4 * c2) != 0) {
          delete[] segs; delete[] nseg;
          return -2000;
        }
      }
    }
  }
  double* wpc = new double[(size_t)n_wp * COR_WPC]();
  for (int i = 0; i < n_wp; ++i)
    if (nseg[i] <= 1) cor_forced(pg, segs, nseg, i, safety_margin, wpc + (size_t)i * COR_WPC);
  int bad = 0;
  for (int w = 0; w < n_wp; ++w) {
    if (!cor_select(pg, segs, nseg, w + 1, n_cols, safety_margin, ub_tab + (size_t)w * n_cols, lb_tab + (size_t)w * n_cols, wpc)) {
      ++bad;
      for (int n = 0; n < n_cols; ++n) ub_tab[(size_t)w * n_cols + n] = lb_tab[(size_t)w * n_cols + n] = std::numeric_limits<double>::quiet_NaN();
      continue;
    }
    // the per-column form the device runs (one thread per (start waypoint, column)) must give the same bits
    for (int n = 0; n < n_cols; ++n) {
      double ub, lb;
      if (!cor_select_one(pg, segs, nseg, w + 1, n, safety_margin, wpc, &ub, &lb) || ub != ub_tab[(size_t)w * n_cols + n] ||
          lb != lb_tab[(size_t)w * n_cols + n]) {
        delete[] segs; delete[] nseg; delete[] wpc;
        return -1000;
      }
    }
  }
  if (nseg_out) for (int i = 0; i < n_wp; ++i) nseg_out[i] = nseg[i];
  delete[] segs; delete[] nseg; delete[] wpc;
  return bad;
}

// host runs of the per-car rollout code that the K3 kernels execute per thread
// -> the car's waypoint (-1 past the path's length); *alive (may be NULL) as mpmpc_localise_kernel leaves it for a running car:
// 1, 0 (s past the length) or -2 (the horizon passes the end of an open path)
extern "C" int emu_localise(int n_wp, int N, int circular, const double* cum, const double* gx, const double* gy,
                            const double* gpsi, double s, const double* pose, double* x0, int* alive) {
  int wp = ro_current_waypoint(cum, n_wp, s);
  if (wp >= 0) ro_t2s(pose[0], pose[1], pose[2], gx[wp], gy[wp], gpsi[wp], x0);
  if (alive) *alive = wp < 0 ? 0 : (ro_past_open_end(n_wp, N, circular != 0, wp) ? -2 : 1);
  return wp;
}
extern "C" int emu_advance(int N, double L, double Ts, int status, const double* z, double* cc, int* counter,
                           const double* x0, double kappa_wp, double* pose, double* s, double* u_out) {
  return ro_advance(N, L, Ts, status, z, cc, counter, x0, kappa_wp, pose, s, u_out) ? 1 : 0;
}

// host run of the speed-profile code that mpmpc_speed_profile_kernel executes per thread
#include "speed_core.hpp"
#include <cstring>
#include <vector>
extern "C" int emu_speed_profile(int n, const double* li, const double* kappa, const double* lim5, double eps,
                                 double* v, int* iters) {
  std::vector<double> ws((size_t)SP_ARRAYS * n);
  SpWork W{ws.data(), n, 1};
  SpLimits lim{lim5[0], lim5[1], lim5[2], lim5[3], lim5[4]};
  return sp_solve(n, li, kappa, 1, lim, eps, W, v, 1, iters);
}
// ... and of the code mpmpc_speed_profile_wave_kernel executes per wavefront: the same per-row cyclic reduction, row by row
extern "C" int emu_speed_profile_wave(int n, const double* li, const double* kappa, const double* lim5, double eps,
                                      double* v, int* iters) {
  std::vector<double> ws((size_t)(SP_ARRAYS + sp_cr_arrays(n)) * n);
  SpWork W{ws.data(), n, 1};
  SpCyclicHost pol{{ws.data() + (size_t)SP_ARRAYS * n, n}};
  SpLimits lim{lim5[0], lim5[1], lim5[2], lim5[3], lim5[4]};
  return sp_solve_t(pol, n, li, kappa, 1, lim, eps, W, v, 1, iters);
}
