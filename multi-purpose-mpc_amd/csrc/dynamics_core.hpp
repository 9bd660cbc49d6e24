// Dynamic single-track plant of the device rollout: a car with mass, yaw inertia and tyres that slip and saturate, behind a
// speed controller that needs time and traction to reach the commanded speed.  The controller stays the LTV-MPC on the
// kinematic model; the mismatch is the point.  Scalar per-car code that compiles for gfx950 (K3y, mpmpc_dynamics.hpp) and for
// the host (tests/emul_dynamics), like plant_core.hpp and delay_core.hpp.  The build has -ffp-contract=off: every product and
// sum below is rounded on its own, in exactly the order stated; a / b * c is (a / b) * c, a * b * c is (a * b) * c.
//
// PARAMETERS.  DY_PARAMS = 11 doubles per car (DY_*), checked by dy_check_params:
//   0 mass m [kg] (> 0)            1 inertia Iz [kg m^2] (> 0)      2 lf [m]: centre of gravity to the front axle (> 0)
//   3 Cf   4 Cr [N / rad]: cornering stiffness (> 0)                 5 mu: friction coefficient (> 0, +inf: no saturation)
//   6 speed_gain k_a [1 / s] (> 0, +inf: an ideal speed controller)  7 a_drive   8 a_brake [m / s^2] (> 0, +inf allowed)
//   9 v_dyn [m / s]: the switch speed (> 0, +inf: never dynamic)    10 substeps n: an integer in [1, DY_MAX_SUBSTEPS = 64]
//   (0 - 4 finite.)  The plant's wheelbase is Lp = L * wheelbase_scale (plant_core.hpp) and lr = Lp - lf; dy_check_run
//   refuses lf >= Lp.  g = 9.81; the static axle loads are Fzf = m * g * lr / Lp and Fzr = m * g * lf / Lp.
//
// STATE per car, carried from step to step like the plant's act: (vx, vy, r) - the body-frame velocity at the centre of gravity
//   and the yaw rate.  The pose stays the reference's point, the rear axle.
//
// DRIVE (dy_drive; under a delay dy_drive_delay), in place of pl_drive / dl_drive<true>:
//   1  pl_drive's steps 1 - 7 (the command, the counter, u_out, the N - 1 ending, the gains, the noise, the lags, the rate
//      limit) yield v_act, d_act = act; under a delay dl_drive<true>'s steps 1 - 3 come first and what leaves the register is
//      the command.  Nothing of that arithmetic is restated: pl_drive / dl_drive<true> THEMSELVES are called, with a pose and an
//      s of their own that nobody reads (their steps 8 and 9 fall away as dead code), so plant_core.hpp and delay_core.hpp - and
//      with them K3p and K3q - stay as they are.  A run that ends returns before anything below.
//   then dy_move:
//   2  if k_a == +inf: vx = v_act
//   3  KINEMATIC branch, taken when !(vx >= v_dyn):
//        if k_a is finite: a = clamp(k_a * (v_act - vx), -a_brake, a_drive);  vx += a * Ts
//        pl_drive's step 8 with vx in place of v_act:
//          r = vx / Lp * tan(d_act);  x += (vx * cos(psi0)) * Ts;  y += (vx * sin(psi0)) * Ts;  psi += r * Ts
//        vy = lr * r
//   4  DYNAMIC branch, otherwise: sd = sin(d_act), cd = cos(d_act), h = Ts / n, cap_f = mu * Fzf, cap_x = mu * Fzr, and n
//      sub-steps of
//        Fx   = k_a finite ? clamp(m * clamp(k_a * (v_act - vx), -a_brake, a_drive), -cap_x, cap_x) : 0      (rear driven)
//        a_f  = d_act - atan2(vy + lf * r, vx)
//        a_r  = -atan2(vy - lr * r, vx)
//        cap_r = sqrt(max(cap_x * cap_x - Fx * Fx, 0))                                                        (friction ellipse)
//        Fyf  = clamp(Cf * a_f, -cap_f, cap_f);   Fyr = clamp(Cr * a_r, -cap_r, cap_r)
//        t    = Fyf * cd
//        dvx  = (Fx - Fyf * sd) / m + vy * r
//        dvy  = (t + Fyr) / m - vx * r
//        dr   = (lf * t - lr * Fyr) / Iz
//        vx += dvx * h  (only if k_a is finite: an ideal speed controller holds vx = v_act through the step)
//        vy += dvy * h;   r += dr * h
//        then the pose with the NEW velocities, at the rear axle:  w = vy - lr * r
//        x += (vx * cos(psi) - w * sin(psi)) * h;   y += (vx * sin(psi) + w * cos(psi)) * h   (both with the old psi);   psi += r * h
//      clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v).  A clip is continuous: a one-ulp difference between two libms moves
//      nothing by more than an ulp.
//   5  pl_drive's step 9 with the step's final vx: s += (1 / (1 - x0[0] * kappa_wp) * vx * cos(x0[1])) * Ts;
//      under a delay `now` takes the place of x0 and kappa, as in dl_drive.
//   The selects of 2 - 4 are not to be simplified away: v_dyn = +inf with k_a = +inf is pl_drive bit for bit (vx = v_act, the
//   kinematic branch, no acceleration step, the same products in the same order).
//
// ACCUMULATORS (DyAcc), per car, by the thread that drives it, on driven steps only:
//   dyn_steps            steps that took the dynamic branch
//   sat_front, sat_rear  steps in which some sub-step clipped that axle (|Cf * a_f| > cap_f, |Cr * a_r| > cap_r)
//   slip_f, slip_r       max |a_f|, max |a_r| over all sub-steps
//   alat                 max |t + Fyr| / m over all sub-steps
//
// STABILITY.  The sub-step is explicit Euler.  With lambda = max((Cf + Cr) / (m * v_dyn), (lf^2 * Cf + lr^2 * Cr) / (Iz * v_dyn))
//   a run needs lambda * Ts / n <= 1 (dy_check_run; v_dyn = +inf passes: lambda = 0).  It is refused on the host before any
//   kernel is launched, at the first call that knows Ts, the wheelbase and the parameters.
//
// OUT OF SCOPE: the dynamics state in the trace / chain record; load transfer and combined-slip curves beyond the ellipse; a
//   dynamic model inside the controller, in K3d's prediction or in K3e (the estimator's and the localiser's dead reckoning, the
//   delay's prediction and the lookahead stay on the nominal model); sharded fleets; the emulation handles; reverse driving.
#pragma once
#include "delay_core.hpp"

namespace mpmpc {

constexpr int DY_PARAMS = 11;
constexpr int DY_MASS = 0, DY_INERTIA = 1, DY_LF = 2, DY_CF = 3, DY_CR = 4, DY_MU = 5, DY_SPEED_GAIN = 6, DY_A_DRIVE = 7, DY_A_BRAKE = 8,
              DY_V_DYN = 9, DY_SUBSTEPS = 10;
constexpr int DY_STATE = 3;      // vx, vy, r
constexpr int DY_COUNTS = 3;     // dyn_steps, sat_front, sat_rear
constexpr int DY_PEAKS = 3;      // slip_f, slip_r, alat
constexpr int DY_MAX_SUBSTEPS = 64;
constexpr double DY_G = 9.81;

struct DyAcc {
  int dyn_steps, sat_front, sat_rear;
  double slip_f, slip_r, alat;
};

MPMPC_HD bool dy_ideal(double k_a) { return k_a > 1.7976931348623157e308; }      // k_a == +inf
MPMPC_HD double dy_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Steps 2 - 4.  q: the car's DY_PARAMS, read where they are used; st [3] = (vx, vy, r) and pose [3]: read once, written once.
MPMPC_HD void dy_move(double Lp, double Ts, double v_act, double d_act, const double* q, double* st, double* pose, DyAcc* acc) {
  const double m = q[DY_MASS], lf = q[DY_LF], k_a = q[DY_SPEED_GAIN];
  const double lr = Lp - lf;
  const bool ideal = dy_ideal(k_a);
  double vx = st[0], vy = st[1], r = st[2];
  if (ideal) vx = v_act;
  if (!(vx >= q[DY_V_DYN])) {
    if (!ideal) {
      const double a = dy_clamp(k_a * (v_act - vx), -q[DY_A_BRAKE], q[DY_A_DRIVE]);
      vx += a * Ts;
    }
    const double psi = pose[2];
    r = vx / Lp * std::tan(d_act);
    pose[0] += (vx * std::cos(psi)) * Ts;
    pose[1] += (vx * std::sin(psi)) * Ts;
    pose[2] += r * Ts;
    vy = lr * r;
  } else {
    const double Iz = q[DY_INERTIA], Cf = q[DY_CF], Cr = q[DY_CR], mu = q[DY_MU];
    const int n = (int)q[DY_SUBSTEPS];
    const double Fzf = m * DY_G * lr / Lp, Fzr = m * DY_G * lf / Lp;
    const double cap_f = mu * Fzf, cap_x = mu * Fzr;
    const double sd = std::sin(d_act), cd = std::cos(d_act);
    const double h = Ts / n;
    double x = pose[0], y = pose[1], psi = pose[2];
    bool sat_f = false, sat_r = false;
    double slip_f = acc->slip_f, slip_r = acc->slip_r, alat = acc->alat;
    for (int j = 0; j < n; ++j) {
      double Fx = 0.0;
      if (!ideal) Fx = dy_clamp(m * dy_clamp(k_a * (v_act - vx), -q[DY_A_BRAKE], q[DY_A_DRIVE]), -cap_x, cap_x);
      const double a_f = d_act - std::atan2(vy + lf * r, vx);
      const double a_r = -std::atan2(vy - lr * r, vx);
      const double cap_r = std::sqrt(std::fmax(cap_x * cap_x - Fx * Fx, 0.0));
      const double Ff = Cf * a_f, Fr = Cr * a_r;
      const double Fyf = dy_clamp(Ff, -cap_f, cap_f), Fyr = dy_clamp(Fr, -cap_r, cap_r);
      if (std::fabs(Ff) > cap_f) sat_f = true;
      if (std::fabs(Fr) > cap_r) sat_r = true;
      const double t = Fyf * cd;
      const double dvx = (Fx - Fyf * sd) / m + vy * r;
      const double dvy = (t + Fyr) / m - vx * r;
      const double dr = (lf * t - lr * Fyr) / Iz;
      if (std::fabs(a_f) > slip_f) slip_f = std::fabs(a_f);
      if (std::fabs(a_r) > slip_r) slip_r = std::fabs(a_r);
      const double al = std::fabs(t + Fyr) / m;
      if (al > alat) alat = al;
      if (!ideal) vx += dvx * h;
      vy += dvy * h;
      r += dr * h;
      const double w = vy - lr * r;
      const double c = std::cos(psi), s = std::sin(psi);
      x += (vx * c - w * s) * h;
      y += (vx * s + w * c) * h;
      psi += r * h;
    }
    pose[0] = x; pose[1] = y; pose[2] = psi;
    acc->dyn_steps += 1;
    if (sat_f) acc->sat_front += 1;
    if (sat_r) acc->sat_rear += 1;
    acc->slip_f = slip_f; acc->slip_r = slip_r; acc->alat = alat;
  }
  st[0] = vx; st[1] = vy; st[2] = r;
}

// Steps 2 - 5 behind the plant's actuators.  act: what pl_drive left; p: the plant's parameters; q, st, acc: dy_move's.
MPMPC_HD void dy_wheels(double L, double Ts, const double* x0, double kappa_wp, const double* p, const double* q, const double* act,
                        double* st, double* pose, double* s, DyAcc* acc) {
  dy_move(L * p[PL_WHEELBASE_SCALE], Ts, act[0], act[1], q, st, pose, acc);
  const double s_dot = 1.0 / (1.0 - x0[0] * kappa_wp) * st[0] * std::cos(x0[1]);
  *s += s_dot * Ts;
}

// In place of pl_drive.  Returns false when the run ends (ro_drive's N - 1 ending).
MPMPC_HD bool dy_drive(int N, double L, double Ts, int status, const double* cc, int* counter, const double* x0, double kappa_wp,
                       const double* p, const double* n5, const double* q, double* act, double* st, double* pose, double* s, double* u_out,
                       DyAcc* acc) {
  double unread_pose[3] = {0.0, 0.0, 0.0}, unread_s = 0.0;
  if (!pl_drive(N, L, Ts, status, cc, counter, x0, kappa_wp, p, n5, act, unread_pose, &unread_s, u_out)) return false;
  dy_wheels(L, Ts, x0, kappa_wp, p, q, act, st, pose, s, acc);
  return true;
}

// In place of dl_drive<true>: reg is the car's command register, d its delay, now what dl_predict left.
MPMPC_HD bool dy_drive_delay(int N, double L, double Ts, int status, const double* cc, int* counter, const double* now, int d, double* reg,
                             const double* p, const double* n5, const double* q, double* act, double* st, double* pose, double* s,
                             double* u_out, DyAcc* acc) {
  double unread_pose[3] = {0.0, 0.0, 0.0}, unread_s = 0.0;
  if (!dl_drive<true>(N, L, Ts, status, cc, counter, now, d, reg, p, n5, act, unread_pose, &unread_s, u_out)) return false;
  dy_wheels(L, Ts, now, now[2], p, q, act, st, pose, s, acc);
  return true;
}

// Host-side validation of mpmpc_rollout_set_dynamics' parameter block [B][DY_PARAMS] (params != NULL) and of state0 [B][3] (may
// be NULL).  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int dy_check_params(int B, int max_batch, const double* params, const double* state0, const char** why) {
  if (B < 1 || B > max_batch) { *why = "B must be in [1, max_batch]"; return -1; }
  for (long i = 0; i < B; ++i) {
    const double* q = params + (long)DY_PARAMS * i;
    for (int c = DY_MASS; c <= DY_CR; ++c)
      if (!(q[c] > 0.0) || !pl_finite(q[c])) { *why = "dynamics: mass, inertia, lf, Cf and Cr must be finite and > 0"; return -1; }
    for (int c = DY_MU; c <= DY_V_DYN; ++c)
      if (!(q[c] > 0.0)) { *why = "dynamics: mu, speed_gain, a_drive, a_brake and v_dyn must be > 0 (+inf allowed)"; return -1; }
    const double n = q[DY_SUBSTEPS];
    if (!(n >= 1.0 && n <= (double)DY_MAX_SUBSTEPS) || n != std::floor(n)) { *why = "dynamics: substeps must be an integer in [1, 64]"; return -1; }
  }
  if (state0)
    for (long i = 0; i < (long)DY_STATE * B; ++i)
      if (!pl_finite(state0[i])) { *why = "dynamics: state0 must be finite"; return -1; }
  return 0;
}

// ... and of what needs the run: every car's plant wheelbase Lp = L * scale[i] (scale == NULL: L itself) against lf, and the
// explicit sub-step's stability at Ts.  Returns 0 or -1 and the reason.
inline int dy_check_run(int B, double L, const double* scale, double Ts, const double* params, const char** why) {
  for (long i = 0; i < B; ++i) {
    const double* q = params + (long)DY_PARAMS * i;
    const double Lp = scale ? L * scale[i] : L;
    const double lf = q[DY_LF], lr = Lp - lf;
    if (!(lf < Lp)) { *why = "dynamics: lf must be below the plant's wheelbase L * wheelbase_scale"; return -1; }
    const double v = q[DY_V_DYN];
    const double la = (q[DY_CF] + q[DY_CR]) / (q[DY_MASS] * v), lb = (lf * lf * q[DY_CF] + lr * lr * q[DY_CR]) / (q[DY_INERTIA] * v);
    const double lambda = la > lb ? la : lb;
    if (!(lambda * Ts / q[DY_SUBSTEPS] <= 1.0)) {
      *why = "dynamics: the explicit sub-step is unstable - max((Cf + Cr) / (m v_dyn), (lf^2 Cf + lr^2 Cr) / (Iz v_dyn)) * Ts / substeps "
             "must be <= 1 (more substeps, or a higher v_dyn)";
      return -1;
    }
  }
  return 0;
}

}  // namespace mpmpc
