// CPU twin of K3d / K3q (mpmpc_delay.hpp): the same delay_core.hpp code, one car after the other.
// Built by tests/emul_delay/Makefile, loaded by tests/delay_twin.py.
#include <cstdint>

#include "delay_core.hpp"

using namespace mpmpc;

extern "C" {

int dl_emu_max() { return DL_MAX; }

// Validation of mpmpc_rollout_set_delay (the library calls the same function): 0 or -1 (E_ARG)
int dl_emu_check(int B, int max_batch, const int32_t* delay, const int32_t* assumed, const double* queue0) {
  const char* why = "";
  return dl_check(B, max_batch, delay, assumed, queue0, &why);
}

// K3d for one car on the route that starts at row `first` of the tables and has n_wp waypoints.  Returns the waypoint of `now`
// (local to the route; -1: s is past the end).
int dl_emu_predict(int n_wp, int first, const double* cum, const double* gx, const double* gy, const double* gpsi, const double* kappa, int c,
                   const double* q, double L, double Ts, const double* pose, double s, double* pred_pose, double* pred_s, double* now,
                   int* now_wp) {
  return dl_predict(cum + first, gx + first, gy + first, gpsi + first, kappa + first, n_wp, first, c, q, L, Ts, pose, s, pred_pose, pred_s,
                    now, now_wp);
}

// K3q<false> for one car: the plan entries as ro_advance writes them, then dl_drive.  Returns 1 (driven) or 0 (the run ends).
int dl_emu_advance(int N, double L, double Ts, int status, const double* z, double* cc, int* counter, const double* now, int d, double* q,
                   double* pose, double* s, double* u_out) {
  if (ro_usable(status))
    for (int k = 0; k < N; ++k) ro_plan_entry(N, L, z, cc, k);
  return dl_drive<false>(N, L, Ts, status, cc, counter, now, d, q, nullptr, nullptr, nullptr, pose, s, u_out) ? 1 : 0;
}

// K3q<true> for one car
int dl_emu_advance_plant(int N, double L, double Ts, int status, const double* z, double* cc, int* counter, const double* now, int d,
                         double* q, const double* p, const double* n5, double* act, double* pose, double* s, double* u_out) {
  if (ro_usable(status))
    for (int k = 0; k < N; ++k) ro_plan_entry(N, L, z, cc, k);
  return dl_drive<true>(N, L, Ts, status, cc, counter, now, d, q, p, n5, act, pose, s, u_out) ? 1 : 0;
}

}  // extern "C"
