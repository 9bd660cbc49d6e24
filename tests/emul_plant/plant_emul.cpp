// CPU twin of K3n / K3p (mpmpc_plant.hpp): the same plant_core.hpp code, one car after the other.
// Built by tests/emul/Makefile (`make plant`), loaded by tests/twins.py.
#include <cstdint>

#include "plant_core.hpp"

using namespace mpmpc;

extern "C" {

// Philox4x32-10 on one counter and key
void pl_emu_philox(const uint32_t* key, const uint32_t* ctr, uint32_t* out) { pl_philox(key[0], key[1], ctr[0], ctr[1], ctr[2], ctr[3], out); }

// out [n][B][5]: the variates of cars car0 .. car0 + B - 1 at j[0 .. n - 1], as mpmpc_plant_noise_kernel computes them
void pl_emu_noise(uint64_t seed, int32_t car0, int B, int n, const int64_t* j, double* out) {
  for (int t = 0; t < n; ++t)
    for (int i = 0; i < B; ++i) pl_noise(seed, (uint32_t)(car0 + i), (long long)j[t], out + ((long)t * B + i) * PL_NOISE);
}

// Validation of mpmpc_rollout_set_plant (the library calls the same function): 0 or -1 (E_ARG)
int pl_emu_check(int B, int max_batch, const double* params, const double* act0) {
  const char* why = "";
  return pl_check_params(B, max_batch, params, act0, &why);
}

// K3n for one car
void pl_emu_measure(const double* p, const double* n5, const double* pose, double* meas) { pl_measure(p, n5, pose, meas); }

// K3p for one car: the plan entries as ro_advance writes them, then pl_drive.  Returns 1 (driven) or 0 (the run ends).
int pl_emu_advance(int N, double L, double Ts, int status, const double* z, double* cc, int* counter, const double* x0, double kappa_wp,
                   const double* p, const double* n5, double* act, double* pose, double* s, double* u_out) {
  if (ro_usable(status))
    for (int k = 0; k < N; ++k) ro_plan_entry(N, L, z, cc, k);
  return pl_drive(N, L, Ts, status, cc, counter, x0, kappa_wp, p, n5, act, pose, s, u_out) ? 1 : 0;
}

// the accumulators of one car, one step
void pl_emu_stats(double x, double y, double wx, double wy, double cos_w, double sin_w, double* ey_max, double* ey_sq, int* steps) {
  pl_stats(x, y, wx, wy, cos_w, sin_w, ey_max, ey_sq, steps);
}

}  // extern "C"
