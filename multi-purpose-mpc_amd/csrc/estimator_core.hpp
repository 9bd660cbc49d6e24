// Pose estimator of the device rollout: per car a 3-state extended Kalman filter on the world pose (x, y, psi) that runs in the
// controller's NOMINAL model, between the measurement and the controller.  With it the controller localises on the estimate
// instead of the raw measured pose (K3a without a delay, K3d's starting pose with one); everything that senses or judges the
// car keeps the true pose.  Scalar per-car code that compiles for gfx950 (K3e, mpmpc_estimator.hpp) and for the host
// (tests/emul_estimator), like plant_core.hpp and delay_core.hpp.  The build has -ffp-contract=off: every product and sum
// below is rounded on its own, in exactly the order stated.
//
// STATE per car.  est [3] = (x, y, psi);  cov [6], the upper triangle of the symmetric covariance P in the order
//   Pxx, Pxy, Pxp, Pyy, Pyp, Ppp (p: psi) - the lower triangle is never stored, so P is symmetric by construction;  primed
//   (int, 0 / 1);  the statistics of 4.
//
// PARAMETERS.  ES_PARAMS = 8 doubles per car (ES_*, es_check_params):
//   0 q_xy, 1 q_psi: process variances added per step [m^2], [rad^2] (finite, >= 0)
//   2 r_xy, 3 r_psi: measurement variances (finite, > 0: every innovation variance is > 0, no division needs a guard)
//   4 p0_xy, 5 p0_psi: the variances a car is primed with (finite, >= 0)
//   6 period: an integer >= 1 held in a double; the measurement is scheduled on the steps with j mod period == 0,
//     j = k - step0, the modulus non-negative for negative j
//   7 drop in [0, 1): the probability that a scheduled measurement is lost
//   seed, car0, step0 as the plant's (plant_core.hpp).
//
// AVAILABLE (es_available): scheduled and not dropped.  Dropped: (w >> 8) * 2^-24 < drop, w word 0 of Philox block 2 of
//   (seed, car0 + car, j) (pl_philox; plant_core.hpp reserves the block).  A 24-bit integer times a power of two compared
//   with a double: no rounding, device and host agree bit for bit.
//
// ONE STEP (es_step), at the start of step k, cars with alive == 1, behind K3n and in front of K3d / K3a.  z: the plant's
//   `meas` when a plant is in force, else the true pose.  (v, delta): the command the controller believes reached the wheels in
//   step k - 1 - without a delay the last commanded control (u of the rollout's state), with one entry c of the register as K3q
//   left it, c the car's ASSUMED delay (the register has shifted once since: before the shift it was entry c - 1, or, c = 0,
//   the command itself).  alive only ever leaves 1, so alive == 1 and primed imply that the car was driven in step k - 1.
//   1  not primed:  est = z;  cov = (p0_xy, 0, 0, p0_xy, 0, p0_psi);  primed = 1;  the measurement counts as taken, whatever
//      the schedule says;  go to 4
//   2  time update.   psi0 = est[2]
//        a = -((v * sin(psi0)) * Ts)           b = (v * cos(psi0)) * Ts
//        est <- ro_drive's pose update on est with v, delta, L, Ts (dl_nominal: ro_drive ITSELF, nothing restated)
//        P <- F P F^T + diag(q_xy, q_xy, q_psi),  F = I + [[0, 0, a], [0, 0, b], [0, 0, 0]],  entry by entry from the OLD P:
//        tx  = Pxp + a * Ppp                    ty  = Pyp + b * Ppp
//        Pxx = ((Pxx + a * Pxp) + a * tx) + q_xy
//        Pxy = (Pxy + a * Pyp) + b * tx
//        Pyy = ((Pyy + b * Pyp) + b * ty) + q_xy
//        Pxp = tx        Pyp = ty        Ppp = Ppp + q_psi
//   3  measurement update, if es_available: three sequential scalar updates in the order x, y, psi (H = I and R diagonal:
//      this equals the joint update and needs no 3 x 3 inverse).  Channel i with r_i = (r_xy, r_xy, r_psi):
//        nu = z_i - est_i            (i = psi: wrapped to [-pi, pi) by ro_t2s ITSELF - its e_psi of heading z_psi against est_psi)
//        s  = P_ii + r_i
//        g_j = P_ji / s              j = x, y, psi, from the P before this channel's update
//        est_j = est_j + g_j * nu    j = x, y, psi
//        P_jl = P_jl - g_j * P_il    the six entries j <= l, every P_il the one before this channel's update
//   4  statistics, from the TRUE pose (x, y, psi) as the step finds it:
//        steps += 1;  used += 1 when a measurement was taken (1, or 3 ran)
//        e2 = (est_x - x) * (est_x - x) + (est_y - y) * (est_y - y);   err2_sum += e2;   err2_max = max(err2_max, e2)
//        meas2_sum += (z_x - x) * (z_x - x) + (z_y - y) * (z_y - y)        every step, whether or not the filter saw z
//        h = ro_t2s's e_psi of heading est_psi against psi;   head2_sum += h * h
//
// PROPERTIES.
//   - Off changes no bit: without the setting no kernel's arguments differ from what they were.
//   - Exact when there is nothing to estimate: with an identity or absent plant, no noise, and no delay or c = d and every
//     car driven, 2 applies to est the operations the drive applied to the pose, on the same numbers; every innovation is
//     exactly 0 (the wrap of 0 is fmod(pi, 2 pi) - pi = 0), g * 0 is 0, so est keeps the bits of the true pose for any q, r,
//     period and drop, and the rollout is the rollout without the estimator.
//   - One call equals many: a result depends on (seed, car0 + car, j) and the car's own state only - not on how rollout_step
//     calls split the steps, not on B, not on other cars.
#pragma once
#include "delay_core.hpp"

namespace mpmpc {

constexpr int ES_PARAMS = 8;
constexpr int ES_Q_XY = 0, ES_Q_PSI = 1, ES_R_XY = 2, ES_R_PSI = 3, ES_P0_XY = 4, ES_P0_PSI = 5, ES_PERIOD = 6, ES_DROP = 7;
constexpr int ES_COV = 6;      // Pxx, Pxy, Pxp, Pyy, Pyp, Ppp
constexpr int ES_STATS = 4;    // err2_max, err2_sum, meas2_sum, head2_sum

// ro_t2s's e_psi of heading `a` against heading `b`: a - b wrapped to [-pi, pi)
MPMPC_HD double es_wrap(double a, double b) {
  double x0[3];
  ro_t2s(0.0, 0.0, a, 0.0, 0.0, b, x0);
  return x0[1];
}

// is the measurement of step j = k - step0 scheduled and not dropped
MPMPC_HD bool es_available(const double* p, uint64_t seed, uint32_t car, long long j) {
  const long long period = (long long)p[ES_PERIOD];
  long long m = j % period;
  if (m < 0) m += period;
  if (m != 0) return false;
  uint32_t w[4];
  pl_philox((uint32_t)seed, (uint32_t)(seed >> 32), car, (uint32_t)(unsigned long long)j, (uint32_t)((unsigned long long)j >> 32), 2u, w);
  return !((double)(w[0] >> 8) * (1.0 / 16777216.0) < p[ES_DROP]);
}

// 2: (v, delta) the command believed executed in the last step
MPMPC_HD void es_time_update(const double* p, double L, double Ts, double v, double delta, double* est, double* P) {
  const double psi0 = est[2];
  const double a = -((v * std::sin(psi0)) * Ts), b = (v * std::cos(psi0)) * Ts;
  const double zero[3] = {0.0, 0.0, 0.0};
  double s = 0.0;
  dl_nominal(L, Ts, v, delta, zero, 0.0, est, &s);
  const double tx = P[2] + a * P[5], ty = P[4] + b * P[5];
  P[0] = ((P[0] + a * P[2]) + a * tx) + p[ES_Q_XY];
  P[1] = (P[1] + a * P[4]) + b * tx;
  P[3] = ((P[3] + b * P[4]) + b * ty) + p[ES_Q_XY];
  P[2] = tx;
  P[4] = ty;
  P[5] = P[5] + p[ES_Q_PSI];
}

// 3: one channel.  (pi0, pi1, pi2): row i of P before the update
MPMPC_HD void es_channel(double nu, double r, double pi0, double pi1, double pi2, double pii, double* est, double* P) {
  const double s = pii + r;
  const double g0 = pi0 / s, g1 = pi1 / s, g2 = pi2 / s;
  est[0] = est[0] + g0 * nu;
  est[1] = est[1] + g1 * nu;
  est[2] = est[2] + g2 * nu;
  P[0] = P[0] - g0 * pi0;
  P[1] = P[1] - g0 * pi1;
  P[2] = P[2] - g0 * pi2;
  P[3] = P[3] - g1 * pi1;
  P[4] = P[4] - g1 * pi2;
  P[5] = P[5] - g2 * pi2;
}
MPMPC_HD void es_measurement_update(const double* p, const double* z, double* est, double* P) {
  es_channel(z[0] - est[0], p[ES_R_XY], P[0], P[1], P[2], P[0], est, P);
  es_channel(z[1] - est[1], p[ES_R_XY], P[1], P[3], P[4], P[3], est, P);
  es_channel(es_wrap(z[2], est[2]), p[ES_R_PSI], P[2], P[4], P[5], P[5], est, P);
}

// One car's step.  cmd [2]: (v, delta) of 2 (not read while the car is not primed); pose: the true one; st [ES_STATS]; used /
// steps: the counters.  Returns whether a measurement was taken.
MPMPC_HD bool es_step(const double* p, uint64_t seed, uint32_t car, long long j, double L, double Ts, const double* z, const double* pose,
                      const double* cmd, double* est, double* P, int* primed, double* st, int* used, int* steps) {
  bool took;
  if (!*primed) {
    est[0] = z[0]; est[1] = z[1]; est[2] = z[2];
    P[0] = p[ES_P0_XY]; P[1] = 0.0; P[2] = 0.0; P[3] = p[ES_P0_XY]; P[4] = 0.0; P[5] = p[ES_P0_PSI];
    *primed = 1;
    took = true;
  } else {
    es_time_update(p, L, Ts, cmd[0], cmd[1], est, P);
    took = es_available(p, seed, car, j);
    if (took) es_measurement_update(p, z, est, P);
  }
  *steps += 1;
  if (took) *used += 1;
  const double ex = est[0] - pose[0], ey = est[1] - pose[1];
  const double e2 = ex * ex + ey * ey;
  st[1] += e2;
  if (e2 > st[0]) st[0] = e2;
  const double mx = z[0] - pose[0], my = z[1] - pose[1];
  st[2] += mx * mx + my * my;
  const double hd = es_wrap(est[2], pose[2]);
  st[3] += hd * hd;
  return took;
}

// Host-side validation of mpmpc_rollout_set_estimator: params [B][ES_PARAMS] (not NULL), est0 [B][3] and cov0 [B][ES_COV]
// (both or neither).  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int es_check_params(int B, int max_batch, const double* params, const double* est0, const double* cov0, const char** why) {
  if (B < 1 || B > max_batch) { *why = "B must be in [1, max_batch]"; return -1; }
  if ((est0 != nullptr) != (cov0 != nullptr)) { *why = "estimator: est0 and cov0 are given together or not at all"; return -1; }
  for (long i = 0; i < B; ++i) {
    const double* p = params + (long)ES_PARAMS * i;
    if (!(p[ES_Q_XY] >= 0.0) || !pl_finite(p[ES_Q_XY]) || !(p[ES_Q_PSI] >= 0.0) || !pl_finite(p[ES_Q_PSI])) {
      *why = "estimator: q_xy and q_psi must be finite and >= 0"; return -1;
    }
    if (!(p[ES_R_XY] > 0.0) || !pl_finite(p[ES_R_XY]) || !(p[ES_R_PSI] > 0.0) || !pl_finite(p[ES_R_PSI])) {
      *why = "estimator: r_xy and r_psi must be finite and > 0"; return -1;
    }
    if (!(p[ES_P0_XY] >= 0.0) || !pl_finite(p[ES_P0_XY]) || !(p[ES_P0_PSI] >= 0.0) || !pl_finite(p[ES_P0_PSI])) {
      *why = "estimator: p0_xy and p0_psi must be finite and >= 0"; return -1;
    }
    if (!(p[ES_PERIOD] >= 1.0) || !(p[ES_PERIOD] <= 1073741824.0) || p[ES_PERIOD] != std::floor(p[ES_PERIOD])) {
      *why = "estimator: period must be an integer in [1, 2^30]"; return -1;
    }
    if (!(p[ES_DROP] >= 0.0 && p[ES_DROP] < 1.0)) { *why = "estimator: drop must be in [0, 1)"; return -1; }
  }
  if (est0) {
    for (long i = 0; i < 3L * B; ++i)
      if (!pl_finite(est0[i])) { *why = "estimator: est0 must be finite"; return -1; }
    for (long i = 0; i < (long)ES_COV * B; ++i)
      if (!pl_finite(cov0[i])) { *why = "estimator: cov0 must be finite"; return -1; }
  }
  return 0;
}

}  // namespace mpmpc
