// CPU twin of K3y (mpmpc_dynamics.hpp): the same dynamics_core.hpp code, one car after the other.
// Built by tests/emul_dynamics/Makefile, loaded by tests/dynamics_twin.py.
#include <cstdint>

#include "dynamics_core.hpp"

using namespace mpmpc;

namespace {
// the accumulators as the library's getters lay them out: counts [3] = dyn_steps, sat_front, sat_rear; peaks [3] = slip_f, slip_r, alat
DyAcc load(const int* counts, const double* peaks) { return DyAcc{counts[0], counts[1], counts[2], peaks[0], peaks[1], peaks[2]}; }
void store(const DyAcc& a, int* counts, double* peaks) {
  counts[0] = a.dyn_steps; counts[1] = a.sat_front; counts[2] = a.sat_rear;
  peaks[0] = a.slip_f; peaks[1] = a.slip_r; peaks[2] = a.alat;
}
}  // namespace

extern "C" {

int dy_emu_params() { return DY_PARAMS; }

// Validation of mpmpc_rollout_set_dynamics and of the run (the library calls the same functions): 0 or -1
int dy_emu_check(int B, int max_batch, const double* params, const double* state0) {
  const char* why = "";
  return dy_check_params(B, max_batch, params, state0, &why);
}
int dy_emu_check_run(int B, double L, const double* scale, double Ts, const double* params) {
  const char* why = "";
  return dy_check_run(B, L, scale, Ts, params, &why);
}

// steps 2 - 4 for one car: what mpmpc_dynamics_drive does with one command
void dy_emu_move(double Lp, double Ts, double v_act, double d_act, const double* q, double* st, double* pose, int* counts, double* peaks) {
  DyAcc a = load(counts, peaks);
  dy_move(Lp, Ts, v_act, d_act, q, st, pose, &a);
  store(a, counts, peaks);
}

// K3y for one car: the plan entries as ro_advance writes them, then dy_drive.  Returns 1 (driven) or 0 (the run ends).
int dy_emu_advance(int N, double L, double Ts, int status, const double* z, double* cc, int* counter, const double* x0, double kappa_wp,
                   const double* p, const double* n5, const double* q, double* act, double* st, double* pose, double* s, double* u_out,
                   int* counts, double* peaks) {
  if (ro_usable(status))
    for (int k = 0; k < N; ++k) ro_plan_entry(N, L, z, cc, k);
  DyAcc a = load(counts, peaks);
  const bool driven = dy_drive(N, L, Ts, status, cc, counter, x0, kappa_wp, p, n5, q, act, st, pose, s, u_out, &a);
  if (driven) store(a, counts, peaks);
  return driven ? 1 : 0;
}

// K3y under a delay for one car
int dy_emu_advance_delay(int N, double L, double Ts, int status, const double* z, double* cc, int* counter, const double* now, int d,
                         double* reg, const double* p, const double* n5, const double* q, double* act, double* st, double* pose, double* s,
                         double* u_out, int* counts, double* peaks) {
  if (ro_usable(status))
    for (int k = 0; k < N; ++k) ro_plan_entry(N, L, z, cc, k);
  DyAcc a = load(counts, peaks);
  const bool driven = dy_drive_delay(N, L, Ts, status, cc, counter, now, d, reg, p, n5, q, act, st, pose, s, u_out, &a);
  if (driven) store(a, counts, peaks);
  return driven ? 1 : 0;
}

}  // extern "C"
