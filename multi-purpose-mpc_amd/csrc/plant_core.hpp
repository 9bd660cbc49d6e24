// Plant models of the device rollout: the vehicle that differs from the controller's model - gains, a steering bias, a
// scaled wheelbase, first-order actuator lags, a steering rate limit - and reproducible noise on the commands and on the
// pose the controller localises on.  Scalar per-car code that compiles for gfx950 (K3n / K3p, mpmpc_plant.hpp) and for the
// host (tests/emul_plant), like obstacle_motion_core.hpp and rollout_core.hpp.  The build has -ffp-contract=off: every
// product and sum below is rounded on its own, in exactly the order stated.
//
// DRAWS.  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), written out below:
//   multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; Weyl constants W0 = 0x9E3779B9, W1 = 0xBB67AE85; ten rounds, the key
//   bumped by (W0, W1) between rounds (nine times);  one round on the counter (c0, c1, c2, c3) with the key (k0, k1):
//       (hi0, lo0) = M0 * c0     (hi1, lo1) = M1 * c2          (32 x 32 -> 64 bit)
//       (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
//   key     = (seed & 0xffffffff, seed >> 32) of the uint64 seed
//   counter = ((uint32)(car0 + car), j_lo, j_hi, block),  j = k - step0 as a two's-complement int64 (j_lo / j_hi its
//             low / high 32 bits), k the rollout step index the movers use (0-based, counted from mpmpc_rollout_init)
//   One 32-bit word w gives one variate
//       t = (double)((int)(w >> 16) + (int)(w & 0xffff) - 65535) * 2^-16
//   the sum of two independent 16-bit uniforms, centred: triangular on (-1, 1), |t| <= 65535 / 65536, mean 0, standard
//   deviation 1 / sqrt(6).  An integer below 2^17 times a power of two: exact in double, no libm - device and host agree
//   bit for bit.  Block 0 yields (n_v, n_delta, n_x, n_y) from its words 0 .. 3, word 0 of block 1 yields n_psi; the
//   other words of block 1 and all further blocks are reserved.  A draw depends on (seed, car0 + car, j, channel) only -
//   not on B, not on how many steps one call makes, not on what other cars do.  Of the reserved blocks, word 0 of block 2 is
//   the pose estimator's dropout draw (estimator_core.hpp, under the estimator's own seed, car0 and step0).  Blocks 16 .. 527 are
//   the lidar localiser's range noise, four beams a block (localiser_core.hpp, under the localiser's own seed, car0 and step0).
//
// PARAMETERS.  PL_PARAMS = 11 doubles per car (PL_*), identity 1, 1, 0, 1, 1, 1, +inf, 0, 0, 0, 0 (pl_check_params):
//   0 speed_gain g_v (finite)       1 steer_gain g_d (finite)        2 steer_offset b_d [rad] (finite)
//   3 wheelbase_scale (finite, > 0) 4 speed_lag a_v in (0, 1]        5 steer_lag a_d in (0, 1]
//   6 steer_rate [rad / step] (> 0, +inf allowed)                    7 speed_noise A_v [m/s]   8 steer_noise A_d [rad]
//   9 position_noise A_xy [m]       10 heading_noise A_psi [rad]     (7 .. 10 finite, >= 0)
//
// MEASURE (pl_measure), in front of K3a, cars with alive == 1: the pose the controller localises on
//       meas = (x + A_xy * n_x,  y + A_xy * n_y,  psi + A_psi * n_psi)
//   The true pose is not touched.
//
// DRIVE (pl_drive), in place of ro_drive:
//   1  (v_cmd, d_cmd), the counter, u_out (the COMMANDED control) and the N - 1 ending are exactly ro_drive's; a run
//      that ends there returns before anything below: the actuator state, the pose and s stay
//   2  v_t = g_v * v_cmd + A_v * n_v
//   3  d_t = (g_d * d_cmd + b_d) + A_d * n_delta
//   4  v_act <- (a_v == 1) ? v_t : v_act + a_v * (v_t - v_act)
//   5  d_new  = (a_d == 1) ? d_t : d_act + a_d * (d_t - d_act)
//   6  d = d_new - d_act
//   7  d_act <- (|d| > rate) ? d_act + copysign(rate, d) : d_new
//   8  ro_drive's pose update with v_act, d_act and the wheelbase Lp = L * wheelbase_scale:
//        psi0 = psi;  x += (v_act * cos(psi0)) * Ts;  y += (v_act * sin(psi0)) * Ts;  psi += (v_act / Lp * tan(d_act)) * Ts
//   9  s += (1 / (1 - x0[0] * kappa_wp) * v_act * cos(x0[1])) * Ts - ro_drive's s_dot on v_act: wheel odometry sees what
//      the wheels did, through the x0 that K3a computed from the MEASURED pose
//   The selects of 4, 5 and 7 make an identity plant ro_drive bit for bit (1 * v + 0 * n is v, +inf never binds); they
//   are not to be simplified away.
//
// STATISTICS (pl_stats), by the thread that drives the car, on the steps where it is driven (pl_drive returned true),
// from the TRUE pose as the step found it (before step 8) against the step's waypoint w (the one K3a chose):
//       e = cos_w * (y - y_w) - sin_w * (x - x_w)
//   cos_w / sin_w from K0's per-waypoint table (cor_trig_row: the HOST's libm), so that the accumulators hold no
//   device-libm result.  Per car: max |e| (ey_max), sum of e * e in step order (ey_sq), the number of such steps.
#pragma once
#include <cmath>
#include <cstdint>

#include "rollout_core.hpp"

namespace mpmpc {

constexpr int PL_PARAMS = 11;
constexpr int PL_SPEED_GAIN = 0, PL_STEER_GAIN = 1, PL_STEER_OFFSET = 2, PL_WHEELBASE_SCALE = 3, PL_SPEED_LAG = 4, PL_STEER_LAG = 5,
              PL_STEER_RATE = 6, PL_SPEED_NOISE = 7, PL_STEER_NOISE = 8, PL_POSITION_NOISE = 9, PL_HEADING_NOISE = 10;
constexpr int PL_NOISE = 5;      // variates per car and step: n_v, n_delta, n_x, n_y, n_psi

MPMPC_HD void pl_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* out) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;      // (the bump after the tenth round is never read)
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

MPMPC_HD double pl_variate(uint32_t w) { return (double)((int)(w >> 16) + (int)(w & 0xffffu) - 65535) * (1.0 / 65536.0); }

// block 0 of (car id, j): n_v, n_delta, n_x, n_y
MPMPC_HD void pl_noise_drive(uint64_t seed, uint32_t car, long long j, double* n4) {
  uint32_t w[4];
  pl_philox((uint32_t)seed, (uint32_t)(seed >> 32), car, (uint32_t)(unsigned long long)j, (uint32_t)((unsigned long long)j >> 32), 0u, w);
  for (int c = 0; c < 4; ++c) n4[c] = pl_variate(w[c]);
}
// word 0 of block 1: n_psi
MPMPC_HD double pl_noise_heading(uint64_t seed, uint32_t car, long long j) {
  uint32_t w[4];
  pl_philox((uint32_t)seed, (uint32_t)(seed >> 32), car, (uint32_t)(unsigned long long)j, (uint32_t)((unsigned long long)j >> 32), 1u, w);
  return pl_variate(w[0]);
}
// all five, in the order of mpmpc_plant_noise's rows
MPMPC_HD void pl_noise(uint64_t seed, uint32_t car, long long j, double* n5) {
  pl_noise_drive(seed, car, j, n5);
  n5[4] = pl_noise_heading(seed, car, j);
}

// p: the car's parameters, n5: its variates of the step
MPMPC_HD void pl_measure(const double* p, const double* n5, const double* pose, double* meas) {
  meas[0] = pose[0] + p[PL_POSITION_NOISE] * n5[2];
  meas[1] = pose[1] + p[PL_POSITION_NOISE] * n5[3];
  meas[2] = pose[2] + p[PL_HEADING_NOISE] * n5[4];
}

// act [2]: the executed (v, delta), carried from step to step.  Returns false when the run ends (ro_drive's N - 1 ending).
MPMPC_HD bool pl_drive(int N, double L, double Ts, int status, const double* cc, int* counter, const double* x0, double kappa_wp,
                       const double* p, const double* n5, double* act, double* pose, double* s, double* u_out) {
  double v, delta;
  if (ro_usable(status)) {
    v = cc[0];
    delta = cc[1];
    *counter = 0;
  } else {
    const int i = 2 * (*counter + 1);
    v = cc[i];
    delta = cc[i + 1];
    *counter += 1;
  }
  u_out[0] = v;
  u_out[1] = delta;
  if (*counter == N - 1) return false;
  const double v_t = p[PL_SPEED_GAIN] * v + p[PL_SPEED_NOISE] * n5[0];
  const double d_t = (p[PL_STEER_GAIN] * delta + p[PL_STEER_OFFSET]) + p[PL_STEER_NOISE] * n5[1];
  const double a_v = p[PL_SPEED_LAG], a_d = p[PL_STEER_LAG], rate = p[PL_STEER_RATE];
  const double v_act = (a_v == 1.0) ? v_t : act[0] + a_v * (v_t - act[0]);
  const double d_new = (a_d == 1.0) ? d_t : act[1] + a_d * (d_t - act[1]);
  const double d = d_new - act[1];
  const double d_act = (std::fabs(d) > rate) ? act[1] + std::copysign(rate, d) : d_new;
  act[0] = v_act;
  act[1] = d_act;
  const double Lp = L * p[PL_WHEELBASE_SCALE];
  const double psi = pose[2];
  pose[0] += (v_act * std::cos(psi)) * Ts;
  pose[1] += (v_act * std::sin(psi)) * Ts;
  pose[2] += (v_act / Lp * std::tan(d_act)) * Ts;
  const double s_dot = 1.0 / (1.0 - x0[0] * kappa_wp) * v_act * std::cos(x0[1]);
  *s += s_dot * Ts;
  return true;
}

// (x, y): the true position as the step found it; (wx, wy, cos_w, sin_w): the step's waypoint and its row of K0's table
MPMPC_HD void pl_stats(double x, double y, double wx, double wy, double cos_w, double sin_w, double* ey_max, double* ey_sq, int* steps) {
  const double e = cos_w * (y - wy) - sin_w * (x - wx);
  const double a = std::fabs(e);
  if (a > *ey_max) *ey_max = a;
  *ey_sq += e * e;
  *steps += 1;
}

// Host-side validation of mpmpc_rollout_set_plant's parameter block [B][PL_PARAMS] (params != NULL) and of act0 (may be
// NULL).  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline bool pl_finite(double v) { return std::fabs(v) <= 1.7976931348623157e308; }
inline int pl_check_params(int B, int max_batch, const double* params, const double* act0, const char** why) {
  if (B < 1 || B > max_batch) { *why = "B must be in [1, max_batch]"; return -1; }
  for (long i = 0; i < B; ++i) {
    const double* p = params + (long)PL_PARAMS * i;
    if (!pl_finite(p[PL_SPEED_GAIN]) || !pl_finite(p[PL_STEER_GAIN]) || !pl_finite(p[PL_STEER_OFFSET])) {
      *why = "plant: speed_gain, steer_gain and steer_offset must be finite"; return -1;
    }
    if (!(p[PL_WHEELBASE_SCALE] > 0.0) || !pl_finite(p[PL_WHEELBASE_SCALE])) { *why = "plant: wheelbase_scale must be finite and > 0"; return -1; }
    if (!(p[PL_SPEED_LAG] > 0.0 && p[PL_SPEED_LAG] <= 1.0)) { *why = "plant: speed_lag must be in (0, 1]"; return -1; }
    if (!(p[PL_STEER_LAG] > 0.0 && p[PL_STEER_LAG] <= 1.0)) { *why = "plant: steer_lag must be in (0, 1]"; return -1; }
    if (!(p[PL_STEER_RATE] > 0.0)) { *why = "plant: steer_rate must be > 0 (+inf: no limit)"; return -1; }
    for (int c = PL_SPEED_NOISE; c <= PL_HEADING_NOISE; ++c)
      if (!(p[c] >= 0.0) || !pl_finite(p[c])) { *why = "plant: the noise amplitudes must be finite and >= 0"; return -1; }
  }
  if (act0)
    for (long i = 0; i < 2L * B; ++i)
      if (!pl_finite(act0[i])) { *why = "plant: act0 must be finite"; return -1; }
  return 0;
}

}  // namespace mpmpc
