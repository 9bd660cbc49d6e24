// The contract of a lane backend, primitive by primitive: ONE function that calls the primitive an integer selects on the
// lane's input values and returns what it gives.  Written once, compiled twice: probe.hip on the device backends
// (csrc/lane_gpu.hpp: LaneGpu / LaneBlock, lane_pair.hpp on top), probe_emu.cpp on their twin (csrc/lane_emu.hpp).  Include
// after lane_gpu.hpp or lane_emu.hpp, lane_pair.hpp and mpmpc_core.hpp (the staged sweeps are the Solver's own static members).
// tests/test_lane_backends.py holds the contract itself, in numpy, and compares.
#pragma once

namespace lane_probe {
using namespace mpmpc;

constexpr int K = 20;           // doubles per lane, in and out (a pair backend: 10 values of two stages, stage 2p first half)
enum Kind { WAVE = 0, BLOCK = 1, PAIR = 2 };      // LaneGpu / LaneBlock / LanePair (the twin: LaneEmu of the same G, C)

// backends (tests/test_lane_backends.py: BACKENDS)
enum Backend { G64C16 = 0, G64C32, G32C16, G16C16, G64C64, B128, B256, B128CH128, P16, P64, P128, N_BACKENDS };

#define LANE_PROBE_OPS(X)                                                                                              \
  X(up) X(down) X(mirror) X(cup) X(cdown) X(up_n) X(down_n) X(mirror_n) X(cup_n) X(cdown_n)                            \
  X(rshr) X(rshl) X(cr_elim) X(from_even_row) X(from_odd_row) X(from_upper) X(from_lower) X(bcast15) X(bcast31)        \
  X(cr_low15) X(cr_special) X(cr64_x) X(cr64_special) X(cr_pull) X(cr_push) X(cr_down) X(cr_bcast) X(up1) X(down1)     \
  X(gsum) X(gmax) X(gmin) X(gscan) X(gany) X(gcount) X(wany) X(cold) X(ids) X(again)                                   \
  X(load) X(gather) X(loadi) X(gatheri) X(store) X(storei) X(end_to_mid) X(mid_to_end)                                 \
  X(rcp) X(rsqrt) X(rcp_fast) X(sqrt) X(fma) X(max) X(min) X(max_raw) X(min_raw)                                       \
  X(sweep_staged_in) X(sweep_staged_out) X(sweep_lock_in) X(sweep_lock_out)                                            \
  X(sweep2_staged_in) X(sweep2_staged_out) X(sweep2_lock_in) X(sweep2_lock_out)
enum Op : int {
#define X(n) OP_##n,
  LANE_PROBE_OPS(X)
#undef X
  N_OPS
};
inline const char* op_name(int op) {
  static const char* const names[] = {
#define X(n) #n,
    LANE_PROBE_OPS(X)
#undef X
  };
  return op >= 0 && op < N_OPS ? names[op] : "";
}

// ---- int <-> real of the lane types (the backends have no such conversion: the solver never needs one)
#ifdef MPMPC_LANE_EMU
inline VD to_real(const VI& a) { VD r; for (int i = 0; i < EMU_W; ++i) r.v[i] = double(a.v[i]); return r; }
inline VI to_ival(const VD& a) { VI r; for (int i = 0; i < EMU_W; ++i) r.v[i] = int(a.v[i]); return r; }
#else
MPMPC_HD double to_real(int a) { return double(a); }
MPMPC_HD int to_ival(double a) { return int(a); }
#endif
MPMPC_HD D2 to_real(const I2& a) { return D2(to_real(a.v[0]), to_real(a.v[1])); }
MPMPC_HD I2 to_ival(const D2& a) { return I2(to_ival(a.v[0]), to_ival(a.v[1])); }

template <int V> struct IC { static constexpr int value = V; };
template <class F> MPMPC_HD void with_d(int d, F f) {
  if (d == 1) f(IC<1>{}); else if (d == 2) f(IC<2>{}); else if (d == 4) f(IC<4>{}); else f(IC<8>{});
}

// ---- the sweeps: x <- fma(a, shift(x), b) on NV values per step, the shift through the Solver's own cup_n / cdown_n
template <class L, int NV, int DIR, int MODE>
MPMPC_HD void sweep_step(const typename L::real* a, const typename L::real* b, typename L::real* x) {
  typename L::real sh[NV];
  if constexpr (DIR < 0) Solver<L>::template cup_n<NV, MODE>(x, sh); else Solver<L>::template cdown_n<NV, MODE>(x, sh);
  for (int i = 0; i < NV; ++i) x[i] = fma_(a[i], sh[i], b[i]);
}
// ... and a step that shifts TWICE (two independent recurrences): staged, the two shifts take disjoint edge slots (OFF 0 / NV)
template <class L, int NV, int DIR, int MODE>
MPMPC_HD void sweep_step2(const typename L::real* a, const typename L::real* b, typename L::real* x) {
  typename L::real sh[NV], sh2[NV];
  if constexpr (MODE != 0) {
    L::template chain_shift<NV, DIR, MODE, 0>(x, sh);
    L::template chain_shift<NV, DIR, MODE, NV>(x + NV, sh2);
  } else if constexpr (DIR < 0) {
    Solver<L>::template cup_n<NV>(x, sh); Solver<L>::template cup_n<NV>(x + NV, sh2);
  } else {
    Solver<L>::template cdown_n<NV>(x, sh); Solver<L>::template cdown_n<NV>(x + NV, sh2);
  }
  for (int i = 0; i < NV; ++i) { x[i] = fma_(a[i], sh[i], b[i]); x[NV + i] = fma_(a[NV + i], sh2[i], b[NV + i]); }
}
// in: a = x[0 .. W), b = x[W .. 2 W) (W = NV, or 2 NV for the double step); out: y[0 .. W); the iterate starts at 0 (as in the solver)
template <class L, int NV, int DIR, bool STAGED, bool TWO>
MPMPC_HD bool sweep(int steps, const typename L::real* x, typename L::real* y) {
  using R = typename L::real;
  constexpr int W = TWO ? 2 * NV : NV;
  R v[W];
  for (int i = 0; i < W; ++i) v[i] = R(0.0);
  if constexpr (STAGED) {
    if constexpr (L::staged_sweeps) {
      Solver<L>::template staged_sweep<DIR>(steps, [&](auto mode) {
        if constexpr (TWO) sweep_step2<L, NV, DIR, decltype(mode)::value>(x, x + W, v);
        else sweep_step<L, NV, DIR, decltype(mode)::value>(x, x + W, v);
      });
    } else {
      return false;
    }
  } else {
    for (int s = 0; s < steps; ++s) {
      if constexpr (TWO) sweep_step2<L, NV, DIR, 0>(x, x + W, v); else sweep_step<L, NV, DIR, 0>(x, x + W, v);
    }
  }
  for (int i = 0; i < W; ++i) y[i] = v[i];
  return true;
}
template <class L, int DIR, bool STAGED>
MPMPC_HD bool sweep_nv(int arg, const typename L::real* x, typename L::real* y) {       // arg = 16 steps + NV
  const int nv = arg & 15, steps = arg >> 4;
  if (nv == 1) return sweep<L, 1, DIR, STAGED, false>(steps, x, y);
  if (nv == 3) return sweep<L, 3, DIR, STAGED, false>(steps, x, y);
  if (nv == 9) return sweep<L, 9, DIR, STAGED, false>(steps, x, y);
  return false;
}

// Runs `op` (every lane of the execution group calls it with the same op and arg); false: this backend has no such primitive.
// NX values per lane: K, or K / 2 pairs.  mem / imem: the buffers of load .. storei.
template <class L, int KIND>
MPMPC_HD bool run_op(int op, int arg, const typename L::real* x, typename L::real* y, double* mem, int* imem) {
  using R = typename L::real;
  using Mk = typename L::mask;
  constexpr int NX = KIND == PAIR ? K / 2 : K;
  const R one(1.0), zero(0.0);
  for (int k = 0; k < NX; ++k) y[k] = zero;
  const Mk m = x[0] > 0.5;
  auto real_of = [&](const Mk& b) { return sel(b, one, zero); };
  switch (op) {
    case OP_up: for (int k = 0; k < 2; ++k) y[k] = L::up(x[k]); return true;
    case OP_down: for (int k = 0; k < 2; ++k) y[k] = L::down(x[k]); return true;
    case OP_up_n: Solver<L>::template up_n<3>(x, y); return true;
    case OP_down_n: Solver<L>::template down_n<3>(x, y); return true;
    case OP_mirror: for (int k = 0; k < 2; ++k) y[k] = L::mirror(x[k]); return true;
    case OP_cup: for (int k = 0; k < 2; ++k) y[k] = L::cup(x[k]); return true;
    case OP_cdown: for (int k = 0; k < 2; ++k) y[k] = L::cdown(x[k]); return true;
    case OP_mirror_n: Solver<L>::template mirror_n<3>(x, y); return true;
    case OP_cup_n: Solver<L>::template cup_n<3>(x, y); return true;
    case OP_cdown_n: Solver<L>::template cdown_n<3>(x, y); return true;
    case OP_gsum: y[0] = L::gsum(x[0]); return true;
    case OP_gmax: y[0] = L::gmax(x[0]); return true;
    case OP_gmin: y[0] = L::gmin(x[0]); return true;
    case OP_gscan: y[0] = L::gscan(x[0]); return true;
    case OP_gany: y[0] = real_of(L::gany(m)); return true;
    case OP_gcount: y[0] = L::gcount(m); return true;
    case OP_wany: y[0] = R(L::wany(m) ? 1.0 : 0.0); return true;
    case OP_cold:        // two slots, read back crosswise
      L::cold_put(0, x[0]); L::cold_put(1, x[1]); L::fence();
      y[0] = L::cold_get(1); y[1] = L::cold_get(0);
      return true;
    case OP_ids: y[0] = to_real(L::lane_id()); y[1] = to_real(L::stage()); y[2] = to_real(L::slot()); return true;
    // x[0]: ok, x[1]: index, x[2]: value
    case OP_load: y[0] = L::load(mem, to_ival(x[1]), m, -7.5); return true;
    case OP_gather: y[0] = L::gather(mem, to_ival(x[1]), m, -7.5); return true;
    case OP_loadi: y[0] = to_real(L::loadi(imem, to_ival(x[1]), m, -7)); return true;
    case OP_gatheri: y[0] = to_real(L::gatheri(imem, to_ival(x[1]), m, -7)); return true;
    case OP_store: L::store(mem, to_ival(x[1]), m, x[2]); return true;
    case OP_storei: L::storei(imem, to_ival(x[1]), m, to_ival(x[2])); return true;
    case OP_sqrt: for (int k = 0; k < NX; ++k) y[k] = sqrt_(x[k]); return true;
    case OP_rcp: for (int k = 0; k < NX; ++k) y[k] = rcp_(x[k]); return true;
    case OP_rsqrt: for (int k = 0; k < NX; ++k) y[k] = rsqrt_(x[k]); return true;
    case OP_rcp_fast: for (int k = 0; k < NX; ++k) y[k] = rcp_fast_(x[k]); return true;
    case OP_fma: for (int k = 0; k < NX / 3; ++k) y[k] = fma_(x[k], x[k + NX / 3], x[k + 2 * (NX / 3)]); return true;
    case OP_max: for (int k = 0; k < NX / 2; ++k) y[k] = max_(x[k], x[k + NX / 2]); return true;
    case OP_min: for (int k = 0; k < NX / 2; ++k) y[k] = min_(x[k], x[k + NX / 2]); return true;
    default: break;
  }
  if constexpr (KIND == PAIR) {
    switch (op) {        // the lanes' own one-lane shift underneath the pairs, on both components
      case OP_up1: for (int k = 0; k < 2; ++k) y[k] = R(L::up1(x[k].v[0]), L::up1(x[k].v[1])); return true;
      case OP_down1: for (int k = 0; k < 2; ++k) y[k] = R(L::down1(x[k].v[0]), L::down1(x[k].v[1])); return true;
#ifndef MPMPC_LANE_EMU
      case OP_again: y[1] = to_real(L::stage_again()); y[2] = to_real(L::slot_again()); return true;
#endif
      default: return false;
    }
  } else {
    switch (op) {
      case OP_rshr: with_d(arg, [&](auto d) { for (int k = 0; k < 2; ++k) y[k] = L::template rshr<decltype(d)::value>(x[k]); }); return true;
      case OP_rshl: with_d(arg, [&](auto d) { for (int k = 0; k < 2; ++k) y[k] = L::template rshl<decltype(d)::value>(x[k]); }); return true;
      case OP_cr_elim: with_d(arg, [&](auto d) { y[0] = real_of(L::template cr_elim<decltype(d)::value>()); }); return true;
      case OP_cr64_x: y[0] = real_of(L::cr64_x(arg)); return true;
      case OP_cr64_special: y[0] = real_of(L::cr64_special(arg)); return true;
      case OP_cr_pull: L::template cr_pull<2>(arg, x, y); return true;
      case OP_cr_push: L::template cr_push<2>(arg, x, y); return true;
      case OP_cr_down: L::template cr_down<2>(arg, x, y); return true;
      case OP_cr_bcast: L::template cr_bcast<2>(arg, x, y); return true;
      case OP_sweep_lock_in: if constexpr (L::group == 256) return sweep_nv<L, -1, false>(arg, x, y); return false;
      case OP_sweep_lock_out: if constexpr (L::group == 256) return sweep_nv<L, +1, false>(arg, x, y); return false;
      case OP_sweep2_lock_in: if constexpr (L::group == 256) return sweep<L, 4, -1, false, true>(arg >> 4, x, y); return false;
      case OP_sweep2_lock_out: if constexpr (L::group == 256) return sweep<L, 4, +1, false, true>(arg >> 4, x, y); return false;
#ifndef MPMPC_LANE_EMU
      case OP_sweep_staged_in: if constexpr (L::group == 256) return sweep_nv<L, -1, true>(arg, x, y); return false;
      case OP_sweep_staged_out: if constexpr (L::group == 256) return sweep_nv<L, +1, true>(arg, x, y); return false;
      case OP_sweep2_staged_in: if constexpr (L::group == 256) return sweep<L, 4, -1, true, true>(arg >> 4, x, y); return false;
      case OP_sweep2_staged_out: if constexpr (L::group == 256) return sweep<L, 4, +1, true, true>(arg >> 4, x, y); return false;
      case OP_again: y[0] = to_real(L::lane_again()); y[1] = to_real(L::stage_again()); y[2] = to_real(L::slot_again()); return true;
      case OP_max_raw: for (int k = 0; k < NX / 2; ++k) y[k] = max_raw_(x[k], x[k + NX / 2]); return true;
      case OP_min_raw: for (int k = 0; k < NX / 2; ++k) y[k] = min_raw_(x[k], x[k + NX / 2]); return true;
#endif
      default: break;
    }
  }
  if constexpr (KIND == WAVE) {
    switch (op) {
      case OP_from_even_row: for (int k = 0; k < 2; ++k) y[k] = L::from_even_row(x[k]); return true;
      case OP_from_odd_row: for (int k = 0; k < 2; ++k) y[k] = L::from_odd_row(x[k]); return true;
      case OP_from_upper: for (int k = 0; k < 2; ++k) y[k] = L::from_upper(x[k]); return true;
      case OP_from_lower: for (int k = 0; k < 2; ++k) y[k] = L::from_lower(x[k]); return true;
      case OP_bcast15: for (int k = 0; k < 2; ++k) y[k] = L::bcast15(x[k]); return true;
      case OP_bcast31: for (int k = 0; k < 2; ++k) y[k] = L::bcast31(x[k]); return true;
      case OP_cr_low15: y[0] = real_of(L::cr_low15()); return true;
      case OP_cr_special: y[0] = real_of(L::cr_special()); return true;
#ifndef MPMPC_LANE_EMU
      case OP_end_to_mid: if constexpr (L::junction_moves) { for (int k = 0; k < 2; ++k) y[k] = L::end_to_mid(x[k]); return true; } return false;
      case OP_mid_to_end: if constexpr (L::junction_moves) { for (int k = 0; k < 2; ++k) y[k] = L::mid_to_end(x[k]); return true; } return false;
#endif
      default: break;
    }
  }
  return false;
}

}  // namespace lane_probe
