// Lidar of a car: what LidarModel(FoV, range, resolution).scan(car, map) of the reference measures (src/lidar_model.py:37-112),
// for one car in its own world - the base map plus the car's disc list.  Scalar code that compiles for gfx950 (K0l,
// mpmpc_lidar_scan_kernel in mpmpc_lidar.hpp) and for the host (tests/emul_lidar), like traffic_core.hpp.
//
// Inputs: the map's frame and grid (MapView: int8, 1 = free, 0 = occupied), the car's discs (cx, cy, r) - at most
// COR_MAX_DISCS, K0c's format, (0, 0, 0) occupies nothing -, a pose (x, y, psi), angles[n] finite and ascending (the
// Python side passes numpy's linspace values; every comparison uses those bits) and range_m > 0.  In exactly this order:
//
//   1 the sensor cell:  qx = floor((x - ox) / res), qy = floor((y - oy) / res)            (cor_w2m's expression)
//       psi not finite, or |qx| or |qy| above 2^30 (a NaN fails this): the whole row is NaN
//       else (cx, cy) = (int)(qx, qy).  The sensor may lie off the grid: the window is clipped, possibly empty.
//   2 the window:  lim = range_m / res,  R = (int)lim      (R > LID_MAX_RANGE_CELLS: MPMPC_E_ARG, checked on the host)
//   3 every cell (i, j) with |i - cx| <= R, |j - cy| <= R, 0 <= i < width, 0 <= j < height that is occupied in the car's
//     world (data[j][i] == 0, or cor_in_disc for one of the discs):
//       nine points  dx = (i - cx) + k / 2,  dy = (j - cy) + l / 2,  k, l in {-1, 0, 1}     (exact in double)
//       a = atan2(dy, dx) - psi
//       a = a < -pi ? -mod(pi + a, 2 pi) + pi : mod(pi + a, 2 pi) - pi       (mod: numpy's, the sign of the divisor)
//       mn, mx = the minimum and the maximum of the nine
//       the cell is SKIPPED when mn < -pi/2 and mx > pi/2 (the reference's branch for such a cell selects no beam)
//       d2 = (cx - i)^2 + (cy - j)^2 (an integer),  d = sqrt((double)d2);  the cell counts only if d < lim
//       every beam b with mn <= angles[b] <= mx:  best[b] = min(best[b], d2)
//   4 ranges[b] = sqrt((double)best[b]) * res where a cell was found, else range_m
//
// The reference updates a beam sequentially with the test d < current / res.  Distinct d2 up to 2 * 2048^2 differ in d by
// more than 6e-8 relative while the round trip (d * res) / res errs by about 1e-16, and equal d2 give the same value
// either way: the result is the minimum over the hit cells IN ANY ORDER - an integer minimum, parallel and deterministic.
//
// THIS IS THE FIRST DEVICE CODE WHERE A LIBM RESULT DECIDES AN OUTPUT: psi is device state and the predicate is the
// reference's own arctan2, so the atan2 of step 3 runs where the scan runs (K0, K0m and the recorder take their
// trigonometry from host-made tables).  Everything after atan2 is +, -, fmod, comparisons, integers and one sqrt, under
// -ffp-contract=off.  Two libms can therefore differ only where an angle ties with a beam, with -+pi/2 or with the +-pi
// wrap to within a few ulp; tests compare implementations outside a 1e-9 rad band around those ties and bit for bit
// everywhere else (tests/test_lidar.py, "the tie rule").
#pragma once
#include <cmath>
#include <cstdint>

#include "obstacle_motion_core.hpp"

namespace mpmpc {

constexpr int LID_MAX_BEAMS = 2048;          // beams of one scan (K0l keeps best[] and angles[] in LDS)
constexpr int LID_MAX_RANGE_CELLS = 2048;    // R: d2 <= 2 R^2 fits an int32 with room to spare
constexpr int LID_NONE = 0x7fffffff;         // best[b] of a beam no cell has hit

// numpy's mod for a positive divisor: fmod, moved into [0, b) by one addition (npy_divmod)
MPMPC_HOST_DEVICE inline double lid_npmod(double a, double b) {
  double m = std::fmod(a, b);
  if (m != 0.0) {
    if (m < 0.0) m += b;
  } else {
    m = 0.0;
  }
  return m;
}

MPMPC_HOST_DEVICE inline double lid_wrap(double a) {
  return a < -COR_PI ? -lid_npmod(COR_PI + a, 2.0 * COR_PI) + COR_PI : lid_npmod(COR_PI + a, 2.0 * COR_PI) - COR_PI;
}

// step 1; false: the row is NaN
MPMPC_HOST_DEVICE inline bool lid_sensor_cell(const MapView& m, double x, double y, double psi, int* cx, int* cy) {
  const double qx = std::floor((x - m.ox) / m.res), qy = std::floor((y - m.oy) / m.res);
  if (!mov_finite(psi) || !(std::fabs(qx) <= MOV_CELL_MAX && std::fabs(qy) <= MOV_CELL_MAX)) return false;
  *cx = (int)qx; *cy = (int)qy;
  return true;
}

// step 2 and the clip of step 3: cells i0 .. i1, j0 .. j1 (empty when i0 > i1 or j0 > j1)
struct LidWindow {
  int i0, i1, j0, j1, R;
  double lim;
};
MPMPC_HOST_DEVICE inline LidWindow lid_window(const MapView& m, int cx, int cy, double range_m) {
  LidWindow w;
  w.lim = range_m / m.res;
  const int R = w.R = (int)w.lim;
  w.i0 = cx - R < 0 ? 0 : cx - R;
  w.i1 = cx + R > m.width - 1 ? m.width - 1 : cx + R;
  w.j0 = cy - R < 0 ? 0 : cy - R;
  w.j1 = cy + R > m.height - 1 ? m.height - 1 : cy + R;
  return w;
}

// a cell of the window (it lies on the grid) in the car's world; disc(j) -> const int* {cx, cy, r}
template <class Disc>
MPMPC_HD bool lid_occupied(const MapView& m, int i, int j, int n_disc, Disc disc) {
  if (m.data[(long long)j * m.width + i] == 0) return true;
  for (int q = 0; q < n_disc; ++q)
    if (cor_in_disc(i, j, disc(q))) return true;
  return false;
}

// the integer half of step 3: d2 of the cell at offset (di, dj) = (i - cx, j - cy), and whether it is in range
MPMPC_HOST_DEVICE inline bool lid_in_range(int di, int dj, double lim, int* d2) {
  *d2 = di * di + dj * dj;
  return std::sqrt((double)*d2) < lim;
}

// the libm half of step 3: the angle interval [mn, mx] of the cell; false: the cell is skipped
MPMPC_HOST_DEVICE inline bool lid_cell_interval(int di, int dj, double psi, double* mn, double* mx) {
  double lo = 0.0, hi = 0.0;
  for (int k = -1; k <= 1; ++k)
    for (int l = -1; l <= 1; ++l) {
      const double dx = (double)di + 0.5 * k, dy = (double)dj + 0.5 * l;
      const double a = lid_wrap(std::atan2(dy, dx) - psi);
      if (k == -1 && l == -1) { lo = a; hi = a; }
      lo = a < lo ? a : lo;
      hi = a > hi ? a : hi;
    }
  *mn = lo; *mx = hi;
  return !(lo < -COR_PI / 2.0 && hi > COR_PI / 2.0);
}

// A cheap enclosure of that interval, for skipping work only (K0l): [lo, hi] contains the nine wrapped angles of the cell,
// from ONE atan2.  The centre is one of the nine points; the others lie within 0.70711 cells of it, so their raw angles
// lie within asin(0.70711 / d) <= 0.712 / d of the centre's for d >= 4, and hw = 0.75 / d leaves 5 % for the rounding of
// both sides - unless the cell lies on atan2's own cut (dj = 0, di < 0: the reference's wrap MIRRORS angles below -pi
// instead of shifting them, so it does not always glue the cut).  Off the cut the wrap is an isometry between its
// breakpoints, and at every breakpoint its value is +-pi: where [a_c - hw, a_c + hw] stays clear of +-pi there is none
// within hw of the centre.
// false: no enclosure (a cell next to the sensor, on the cut, or one whose points may wrap apart).  A cell whose enclosure covers no
// beam with best[b] > d2 cannot change any best[b]: the minimum is order-free, so leaving it out changes no output bit.
constexpr int LID_BOUND_MIN_D2 = 16;
MPMPC_HOST_DEVICE inline bool lid_cell_enclosure(int di, int dj, int d2, double psi, double* lo, double* hi) {
  if (d2 < LID_BOUND_MIN_D2 || (dj == 0 && di < 0)) return false;
  const double ac = lid_wrap(std::atan2((double)dj, (double)di) - psi);
  const double hw = 0.75 / std::sqrt((double)d2);
  if (!(std::fabs(ac) + hw < 3.14)) return false;
  *lo = ac - hw; *hi = ac + hw;
  return true;
}

// the first beam with angles[b] >= mn (n when there is none): comparisons against the table only
MPMPC_HOST_DEVICE inline int lid_first_beam(const double* angles, int n, double mn) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (angles[mid] >= mn) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// step 4
MPMPC_HOST_DEVICE inline double lid_range(int best, double res, double range_m) {
  return best == LID_NONE ? range_m : std::sqrt((double)best) * res;
}

// Host-side validation of mpmpc_lidar_scan / mpmpc_rollout_scan: everything that can be refused before a device call.
// off == NULL: no discs.  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int lid_check_beams(int n_beams, const double* angles, double range_m, double res, const char** why) {
  if (n_beams < 1 || n_beams > LID_MAX_BEAMS) { *why = "n_beams must be in [1, 2048] (LID_MAX_BEAMS)"; return -1; }
  if (!angles) { *why = "angles is NULL"; return -1; }
  for (int b = 0; b < n_beams; ++b) {
    if (!mov_finite(angles[b])) { *why = "a beam angle is not finite"; return -1; }
    if (b > 0 && !(angles[b] >= angles[b - 1])) { *why = "the beam angles must be ascending"; return -1; }
  }
  if (!(range_m > 0.0) || !mov_finite(range_m)) { *why = "the range must be positive and finite"; return -1; }
  if (!(range_m / res <= (double)LID_MAX_RANGE_CELLS)) { *why = "the range is more than 2048 cells (LID_MAX_RANGE_CELLS)"; return -1; }
  return 0;
}
inline int lid_check_discs(int B, const int32_t* off, const int32_t* discs, int map_w, int map_h, const char** why) {
  if (!off) return 0;
  if (off[0] != 0) { *why = "offsets[0] must be 0"; return -1; }
  for (int b = 0; b < B; ++b) {
    const long k = (long)off[b + 1] - off[b];
    if (k < 0) { *why = "offsets must not decrease"; return -1; }
    if (k > COR_MAX_DISCS) { *why = "more than 64 discs for one car (COR_MAX_DISCS)"; return -1; }
  }
  if (off[B] > 0 && !discs) { *why = "discs is NULL"; return -1; }
  for (long j = 0; j < off[B]; ++j) {
    const long cx = discs[3 * j], cy = discs[3 * j + 1], r = discs[3 * j + 2];
    if (r < 0) { *why = "a disc has a negative radius"; return -1; }
    if (cx - r < 0 || cy - r < 0 || cx + r > map_w || cy + r > map_h) { *why = "a disc's square leaves the map"; return -1; }
  }
  return 0;
}
inline int lid_check_scan(int height, int width, const int8_t* data, double res, int B, const double* pose, const int32_t* off,
                          const int32_t* discs, int n_beams, const double* angles, double range_m, const double* out,
                          const char** why) {
  if (height < 1 || width < 1 || !(res > 0.0) || !mov_finite(res)) { *why = "map needs positive size and resolution"; return -1; }
  if (height > COR_MAX_SIDE || width > COR_MAX_SIDE) { *why = "map sides are limited to 65534 cells"; return -1; }
  if (B < 1) { *why = "B must be >= 1"; return -1; }
  if (!data || !pose || !out) { *why = "data, pose and ranges_out must not be NULL"; return -1; }
  if (int rc = lid_check_beams(n_beams, angles, range_m, res, why)) return rc;
  return lid_check_discs(B, off, discs, width, height, why);
}

}  // namespace mpmpc
