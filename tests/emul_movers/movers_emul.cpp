// CPU twin of K0m (mpmpc_obstacle_move_kernel): the same obstacle_motion_core.hpp code, one mover after the other.
// Built by tests/emul/Makefile (`make movers`), loaded by tests/twins.py.
#include <cstdint>
#include <vector>

#include "obstacle_motion_core.hpp"

using namespace mpmpc;

extern "C" {

// Validation of mpmpc_rollout_set_movers (the library calls the same function): 0, -1 (E_ARG) or -3 (E_STATE).
// static_B / static_off: the static discs in force (static_B = 0: none).
int mov_emu_check(int B, int max_batch, const int32_t* off, const int32_t* kind, const int32_t* radius, const double* params,
                  int built, int static_B, const int32_t* static_off) {
  const char* why = "";
  return mov_check_movers(B, max_batch, off, kind, radius, params, built != 0, static_B, static_off, &why);
}

// the other direction: mpmpc_rollout_set_obstacles' check of new static discs against the movers in force
int mov_emu_check_combined(int static_B, const int32_t* static_off, int movers_B, const int32_t* movers_off) {
  const char* why = "";
  return mov_check_combined(static_B, static_off, movers_B, movers_off, &why);
}

// combined offsets [B + 1] and the movers' slots, as the library lays them out
void mov_emu_combine(int B, const int32_t* static_off, const int32_t* movers_off, int32_t* off, int32_t* dst) {
  mov_combine(B, static_off, movers_off, off, dst);
}

// discs[n][3] of n movers (params [n][4]), mover q at rollout step k[q]; the trigonometric table is K0's (cor_trig_row)
void mov_emu_discs(int n, const int32_t* kind, const int32_t* radius, const double* params, const int64_t* k, int64_t step0,
                   int map_h, int map_w, double ox, double oy, double res, int n_wp, const double* cum, const double* x,
                   const double* y, const double* psi, int circular, int32_t* discs) {
  const MapView m{nullptr, map_h, map_w, ox, oy, res};
  std::vector<double> trig((size_t)n_wp * COR_TRIG);
  for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
  const MoverPath p{cum, x, y, trig.data(), n_wp, COR_TRIG, circular};
  for (int q = 0; q < n; ++q) {
    const double* a = params + (size_t)MOV_PARAMS * q;
    int d[3];
    mov_disc(m, p, kind[q], radius[q], a[0], a[1], a[2], a[3], (long long)k[q], (long long)step0, d);
    for (int t = 0; t < 3; ++t) discs[3 * q + t] = d[t];
  }
}

}  // extern "C"
