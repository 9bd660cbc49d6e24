// Actuation delay of the device rollout and its compensation: a command issued at step k reaches the wheels at step k + d
// (compute, radio and servo latency), and the controller - which assumes a delay c - predicts, through its own nominal model
// and the commands still in flight, where the car will be when the command it computes now takes effect, and plans from
// there.  Scalar per-car code that compiles for gfx950 (K3d / K3q, mpmpc_delay.hpp) and for the host (tests/emul_delay), like
// plant_core.hpp and rollout_core.hpp.  The build has -ffp-contract=off: every product and sum is rounded on its own.
//
// STATE per car.  delay d and assumed c, integers in [0, DL_MAX], DL_MAX = 8; a shift register q [DL_MAX][2] of issued
//   commands (v, delta): q[0] is the newest, q[i] was issued i + 1 driven steps ago.  The register is always DL_MAX long,
//   whatever d and c are; c > d and c < d are legal (a controller that over- or under-estimates the latency).
//
// PREDICT (dl_predict), in front of K3a and behind K3n, cars with alive == 1.  Input: the pose the controller localises on
//   (the plant's `meas` when a plant is in force, else the true pose) and s; the car's route view as K3a takes it.
//       P = pose, S = s
//       wp = ro_current_waypoint(cum, n_wp, S)
//       if wp < 0: pred = (P, S); `now` is left as it is; return            (K3a ends the car as it does without a delay)
//       x0 = ro_t2s(P, waypoint wp)
//       now = (x0[0], x0[1], kappa[wp]);  now_wp = the global row of wp
//       for i = c - 1 down to 0:                                             (the oldest command in flight first)
//           (v, delta) = q[i]
//           ro_drive's pose update and s update on (P, S) with v, delta, L, Ts, x0, kappa[wp]      (dl_nominal: the NOMINAL
//                                                                                                  model, no plant parameter)
//           if i > 0: wp = ro_current_waypoint(cum, n_wp, S); if wp < 0: break; x0 = ro_t2s(P, waypoint wp)
//       pred_pose = P, pred_s = S
//   K3a then localises on (pred_pose, pred_s): wp_id, x0, the warm start's shift, K0c's corridor, the QP and the plan all
//   belong to the predicted pose.  With c = 0 the loop body never runs: pred is the input bit for bit and `now` is what K3a
//   computes.  A prediction that passes the path's end hands K3a an s past the end: the car finishes (alive = 0) up to c
//   steps early.
//
// DRIVE (dl_drive), in place of ro_drive / pl_drive:
//   1  (v_cmd, d_cmd), the counter, u_out (the COMMANDED control) and the N - 1 ending are exactly ro_drive's; a run that
//      ends there returns before anything below: the register, the actuator state, the pose and s stay
//   2  exec = (d > 0) ? q[d - 1] : cmd
//   3  q[i] = q[i - 1] for i = DL_MAX - 1 down to 1;  q[0] = cmd
//   4  no plant: ro_drive's pose update on exec;  plant: pl_drive's steps 2 - 8 on exec
//   5  the s update (ro_drive's s_dot; step 9 of the plant) with `now` in place of K3a's x0 and kappa[wp_id], which belong
//      to the predicted pose: s stays the odometry of where the car IS
//   Steps 4 and 5 are ro_drive / pl_drive THEMSELVES, called on a usable status with a plan whose entry 0 is exec, x0 = now
//   and kappa_wp = now[2] (dl_nominal, dl_plant): nothing of their arithmetic is restated.  So
//     - d = 0, c = 0 changes no bit: without a plant dl_drive is ro_drive, with one it is pl_drive;
//     - with no plant (or an identity plant), d = c and a car driven on every step in between, pred_pose / pred_s of step k
//       are bit-equal to the true pose / s the car has when step k + c begins: the prediction applies the same operations to
//       the same numbers as the drive will.
//   The selects of 2 are not to be simplified away.
//
// STATISTICS.  With a plant, pl_stats is fed the waypoint of `now` (now_wp), not the predicted one.
#pragma once
#include "plant_core.hpp"

namespace mpmpc {

constexpr int DL_MAX = 8;

// ro_drive's pose and s update alone: ro_drive itself, on a usable status and a plan whose entry 0 is (v, delta).  N = 0
// keeps its N - 1 ending out of reach (the counter it sees is 0, never -1).
MPMPC_HD void dl_nominal(double L, double Ts, double v, double delta, const double* x0, double kappa_wp, double* pose, double* s) {
  const double cmd[2] = {v, delta};
  int counter = 0;
  double u[2];
  (void)ro_drive(0, L, Ts, 1, cmd, &counter, x0, kappa_wp, pose, s, u);
}
// ... and pl_drive's steps 2 - 9, the same way
MPMPC_HD void dl_plant(double L, double Ts, double v, double delta, const double* x0, double kappa_wp, const double* p, const double* n5,
                       double* act, double* pose, double* s) {
  const double cmd[2] = {v, delta};
  int counter = 0;
  double u[2];
  (void)pl_drive(0, L, Ts, 1, cmd, &counter, x0, kappa_wp, p, n5, act, pose, s, u);
}

// cum, gx, gy, gpsi, kappa: the car's route (its first row already added; `first` is that row, for now_wp); q: the car's
// register, read where it is used.  pose / s: what the controller localises on.  Returns the waypoint of `now` (-1: s is past
// the end - pred is the input, now / now_wp are not written).
MPMPC_HD int dl_predict(const double* cum, const double* gx, const double* gy, const double* gpsi, const double* kappa, int n_wp, long first,
                        int c, const double* q, double L, double Ts, const double* pose, double s, double* pred_pose, double* pred_s,
                        double* now, int* now_wp) {
  double P[3] = {pose[0], pose[1], pose[2]};
  double S = s;
  int wp = ro_current_waypoint(cum, n_wp, S);
  const int wp_now = wp;
  if (wp >= 0) {
    double x0[3];
    ro_t2s(P[0], P[1], P[2], gx[wp], gy[wp], gpsi[wp], x0);
    now[0] = x0[0];
    now[1] = x0[1];
    now[2] = kappa[wp];
    *now_wp = (int)(first + wp);
    for (int i = c - 1; i >= 0; --i) {
      dl_nominal(L, Ts, q[2 * i], q[2 * i + 1], x0, kappa[wp], P, &S);
      if (i > 0) {
        wp = ro_current_waypoint(cum, n_wp, S);
        if (wp < 0) break;
        ro_t2s(P[0], P[1], P[2], gx[wp], gy[wp], gpsi[wp], x0);
      }
    }
  }
  pred_pose[0] = P[0];
  pred_pose[1] = P[1];
  pred_pose[2] = P[2];
  *pred_s = S;
  return wp_now;
}

// q: the car's register [DL_MAX][2]; now: what dl_predict left (x0[0], x0[1], kappa of the car's TRUE waypoint).  PLANT: p, n5
// and act are pl_drive's (else unused).  Returns false when the run ends (ro_drive's N - 1 ending).
template <bool PLANT>
MPMPC_HD bool dl_drive(int N, double L, double Ts, int status, const double* cc, int* counter, const double* now, int d, double* q,
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
  const double ev = (d > 0) ? q[2 * (d - 1)] : v;
  const double ed = (d > 0) ? q[2 * (d - 1) + 1] : delta;
  for (int i = DL_MAX - 1; i > 0; --i) {
    q[2 * i] = q[2 * i - 2];
    q[2 * i + 1] = q[2 * i - 1];
  }
  q[0] = v;
  q[1] = delta;
  if (PLANT) dl_plant(L, Ts, ev, ed, now, now[2], p, n5, act, pose, s);
  else dl_nominal(L, Ts, ev, ed, now, now[2], pose, s);
  return true;
}

// Host-side validation of mpmpc_rollout_set_delay: delay [B] (not NULL), assumed [B] or NULL, queue0 [B][DL_MAX][2] or NULL.
// Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int dl_check(int B, int max_batch, const int32_t* delay, const int32_t* assumed, const double* queue0, const char** why) {
  if (B < 1 || B > max_batch) { *why = "B must be in [1, max_batch]"; return -1; }
  for (long i = 0; i < B; ++i) {
    if (delay[i] < 0 || delay[i] > DL_MAX) { *why = "delay: every car's delay must be in [0, 8]"; return -1; }
    if (assumed && (assumed[i] < 0 || assumed[i] > DL_MAX)) { *why = "delay: every car's assumed delay must be in [0, 8]"; return -1; }
  }
  if (queue0)
    for (long i = 0; i < 2L * DL_MAX * B; ++i)
      if (!pl_finite(queue0[i])) { *why = "delay: queue0 must be finite"; return -1; }
  return 0;
}

}  // namespace mpmpc
