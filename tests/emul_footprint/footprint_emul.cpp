// CPU twin of K0f (mpmpc_footprint_kernel): the same footprint_core.hpp code, one car and one cell after the other in plain
// row order, no early exit, the host's libm for cos and sin.  Built by tests/emul/Makefile (`make footprint`), loaded by tests/twins.py.
#include <cmath>
#include <cstdint>

#include "footprint_core.hpp"

using namespace mpmpc;

extern "C" {

// the argument checks of mpmpc_footprint_audit (the library calls the same function): 0 or -1 (E_ARG); *R <- the window
int fp_emu_check(int height, int width, const int8_t* data, double res, int B, const double* pose, const int32_t* off,
                 const int32_t* discs, double length, double car_width, double reach_m, const int32_t* contact,
                 const double* clearance, int32_t* R) {
  const char* why = "";
  int r = 0;
  const int rc = fp_check_audit(height, width, data, res, B, pose, off, discs, length, car_width, reach_m, contact, clearance, &r, &why);
  if (R) *R = r;
  return rc;
}

// contact [B], clearance [B].  Returns the check's code.
int fp_emu_audit(int height, int width, const int8_t* data, double ox, double oy, double res, int B, const double* pose,
                 const int32_t* off, const int32_t* discs, double length, double car_width, double reach_m, int32_t* contact,
                 double* clearance) {
  const char* why = "";
  int R = 0;
  if (int rc = fp_check_audit(height, width, data, res, B, pose, off, discs, length, car_width, reach_m, contact, clearance, &R, &why))
    return rc;
  const MapView m{data, height, width, ox, oy, res};
  for (int b = 0; b < B; ++b) {
    const double x = pose[3L * b], y = pose[3L * b + 1], psi = pose[3L * b + 2];
    int cx, cy;
    if (!lid_sensor_cell(m, x, y, psi, &cx, &cy)) {
      contact[b] = 0;
      clearance[b] = std::nan("");
      continue;
    }
    const FpCar car = fp_car(x, y, psi, length, car_width);
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    auto disc = [&](int q) { return discs + 3L * (d0 + q); };
    const int i0 = cx - R < 0 ? 0 : cx - R, i1 = cx + R > width - 1 ? width - 1 : cx + R;
    const int j0 = cy - R < 0 ? 0 : cy - R, j1 = cy + R > height - 1 ? height - 1 : cy + R;
    double best = FP_NONE;
    int hit = 0;
    for (int j = j0; j <= j1; ++j)
      for (int i = i0; i <= i1; ++i) {
        if (!lid_occupied(m, i, j, nd, disc)) continue;
        const double g = fp_cell_g(m, car, i, j);
        hit |= g == 0.0;
        best = g < best ? g : best;
      }
    contact[b] = hit;
    clearance[b] = fp_clearance(best, reach_m);
  }
  return 0;
}

}  // extern "C"
