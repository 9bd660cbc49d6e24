// CPU twin of K0l (mpmpc_lidar_scan_kernel): the same lidar_core.hpp code, one car and one cell after the other, the
// host's libm for the atan2 of a cell's interval.  Built by tests/emul/Makefile (`make lidar`), loaded by tests/twins.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "lidar_core.hpp"

using namespace mpmpc;

extern "C" {

// the argument checks of mpmpc_lidar_scan (the library calls the same function): 0 or -1 (E_ARG)
int lid_emu_check(int height, int width, const int8_t* data, double res, int B, const double* pose, const int32_t* off,
                  const int32_t* discs, int n_beams, const double* angles, double range_m, const double* out) {
  const char* why = "";
  return lid_check_scan(height, width, data, res, B, pose, off, discs, n_beams, angles, range_m, out, &why);
}

// ranges [B][n_beams]; skipped [B] (may be NULL): the cells of each scan that step 3 skips; enclosed [B][2] (may be NULL):
// the occupied in-range cells lid_cell_enclosure gives an enclosure for, and those whose interval it does NOT contain
// (K0l's shortcut rests on there being none).  Returns the check's code.
int lid_emu_scan(int height, int width, const int8_t* data, double ox, double oy, double res, int B, const double* pose,
                 const int32_t* off, const int32_t* discs, int n_beams, const double* angles, double range_m, double* ranges,
                 int32_t* skipped, int32_t* enclosed) {
  const char* why = "";
  if (int rc = lid_check_scan(height, width, data, res, B, pose, off, discs, n_beams, angles, range_m, ranges, &why)) return rc;
  const MapView m{data, height, width, ox, oy, res};
  std::vector<int> best((size_t)n_beams);
  for (int b = 0; b < B; ++b) {
    double* out = ranges + (long)b * n_beams;
    if (skipped) skipped[b] = 0;
    if (enclosed) enclosed[2 * b] = enclosed[2 * b + 1] = 0;
    const double psi = pose[3L * b + 2];
    int cx, cy;
    if (!lid_sensor_cell(m, pose[3L * b], pose[3L * b + 1], psi, &cx, &cy)) {
      for (int k = 0; k < n_beams; ++k) out[k] = std::nan("");
      continue;
    }
    const LidWindow w = lid_window(m, cx, cy, range_m);
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    auto disc = [&](int q) { return discs + 3L * (d0 + q); };
    for (int k = 0; k < n_beams; ++k) best[k] = LID_NONE;
    for (int j = w.j0; j <= w.j1; ++j)
      for (int i = w.i0; i <= w.i1; ++i) {
        if (!lid_occupied(m, i, j, nd, disc)) continue;
        int d2;
        if (!lid_in_range(i - cx, j - cy, w.lim, &d2)) continue;
        double mn, mx, lo, hi;
        const bool in = lid_cell_interval(i - cx, j - cy, psi, &mn, &mx);
        if (enclosed && lid_cell_enclosure(i - cx, j - cy, d2, psi, &lo, &hi)) {
          ++enclosed[2 * b];
          if (!(lo <= mn && mx <= hi)) ++enclosed[2 * b + 1];
        }
        if (!in) {
          if (skipped) ++skipped[b];
          continue;
        }
        for (int k = lid_first_beam(angles, n_beams, mn); k < n_beams && angles[k] <= mx; ++k)
          best[k] = d2 < best[k] ? d2 : best[k];
      }
    for (int k = 0; k < n_beams; ++k) out[k] = lid_range(best[k], res, range_m);
  }
  return 0;
}

}  // extern "C"
