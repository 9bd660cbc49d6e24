// CPU twin of K3e (mpmpc_estimator.hpp): the same estimator_core.hpp code, one car at a time.
// Built by tests/emul_estimator/Makefile, loaded by tests/estimator_twin.py.
#include <cstdint>

#include "estimator_core.hpp"

using namespace mpmpc;

extern "C" {

int es_emu_params() { return ES_PARAMS; }

// Validation of mpmpc_rollout_set_estimator (the library calls the same function): 0 or -1 (E_ARG)
int es_emu_check(int B, int max_batch, const double* params, const double* est0, const double* cov0) {
  const char* why = "";
  return es_check_params(B, max_batch, params, est0, cov0, &why);
}

// is the measurement of step j = k - step0 available to car `car` (car0 already added)
int es_emu_available(const double* p, uint64_t seed, uint32_t car, int64_t j) { return es_available(p, seed, car, j) ? 1 : 0; }

// K3e for one car.  st [4] = err2_max, err2_sum, meas2_sum, head2_sum.  Returns 1 when a measurement was taken.
int es_emu_step(const double* p, uint64_t seed, uint32_t car, int64_t j, double L, double Ts, const double* z, const double* pose,
                const double* cmd, double* est, double* cov, int* primed, double* st, int* used, int* steps) {
  return es_step(p, seed, car, j, L, Ts, z, pose, cmd, est, cov, primed, st, used, steps) ? 1 : 0;
}

// the drive of a car without a plant and without a delay: ro_drive on a usable status with (v, delta) as its plan's entry 0
void es_emu_drive(double L, double Ts, double v, double delta, const double* x0, double kappa_wp, double* pose, double* s) {
  const double cmd[2] = {v, delta};
  int counter = 0;
  double u[2];
  (void)ro_drive(2, L, Ts, 1, cmd, &counter, x0, kappa_wp, pose, s, u);
}

}  // extern "C"
