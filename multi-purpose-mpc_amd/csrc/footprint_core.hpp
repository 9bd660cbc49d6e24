// Footprint audit of a car: does the car's rectangle, at the car's pose, touch anything in the car's own world - the base
// map plus the car's disc list -, and how close does it get?  Scalar code that compiles for gfx950 (K0f,
// mpmpc_footprint_kernel in mpmpc_footprint.hpp) and for the host (tests/emul_footprint), like lidar_core.hpp.
//
// Inputs: the map's frame and grid (MapView: int8, 1 = free, 0 = occupied), the car's discs (cx, cy, r) - at most
// COR_MAX_DISCS, K0c's format, (0, 0, 0) occupies nothing -, a pose (x, y, psi): the CENTRE of the rectangle, as
// SpatialBicycleModel.show of the reference draws the car (src/spatial_bicycle_models.py), length > 0 along the heading
// and width > 0 across it, reach_m > 0, and the window's half-width in cells, computed on the host:
//       R = (int)((reach_m + 0.5 * sqrt(length^2 + width^2)) / res) + 1     (R > FP_MAX_REACH_CELLS: MPMPC_E_ARG)
// In exactly this order:
//
//   1 the centre cell:  qx = floor((x - ox) / res), qy = floor((y - oy) / res)            (lid_sensor_cell)
//       psi, x or y not finite, or |qx| or |qy| above 2^30: contact = 0, clearance = NaN, and the car IS NOT COUNTED - of a
//       rollout's accumulators only last_contact / last_clearance take these values (fp_accumulate)
//       else (cx, cy) = (int)(qx, qy).  The centre may lie off the grid: the window is clipped, possibly empty.
//   2 c = cos(psi), s = sin(psi), once per car: THE ONLY LIBM CALL
//   3 every cell (i, j) with |i - cx| <= R, |j - cy| <= R, 0 <= i < width, 0 <= j < height that is occupied in the car's
//     world (data[j][i] == 0, or cor_in_disc for one of the discs; off-grid cells count as nothing, as in K0l):
//       px = (i + 0.5) * res + ox,  py = (j + 0.5) * res + oy        (cor_m2w's expression);  dx = px - x,  dy = py - y
//       u = c * dx + s * dy,  v = c * dy - s * dx                    (the car's frame; -ffp-contract=off)
//       du = max(|u| - length / 2, 0),  dv = max(|v| - width / 2, 0),  g = du * du + dv * dv
//       contact |= (g == 0);  best = min(best, g)
//   4 clearance = min(reach_m, sqrt(best)), reach_m when no cell was found
//
// Why this is exact.  A cell outside the window has |i - cx| >= R + 1 or |j - cy| >= R + 1, and the car's centre lies in
// its centre cell: along that axis the outside cell's centre is at least (R + 1 + 0.5 - 1) * res = (R + 0.5) * res from the
// car's centre, and R * res > reach_m + half the rectangle's diagonal (half a cell is left for the rounding of step 1) -
// hence more than reach_m from every point of the rectangle - it could only give clearance = reach_m, which is what is
// reported without it.  The minimum of doubles is order-free, so no output bit depends on the order in which the cells
// are visited or on an early exit: once one cell has g == 0 the answer is (1, 0.0) whatever else is in the window (K0f's
// one shortcut).  contact is the same statement as best == 0, since g >= 0.
// Two libms can differ in c and s by a few ulp, so two implementations can differ in the flag only where an occupied cell's
// centre lies within rounding of the rectangle's boundary, and in the clearance by a few ulp of the distances involved;
// tests compare implementations outside a 1e-9 m band around the boundary (tests/test_footprint.py, "the tie rule").
#pragma once
#include <cmath>
#include <cstdint>

#include "lidar_core.hpp"

namespace mpmpc {

constexpr int FP_MAX_REACH_CELLS = 256;      // R: the window has at most 513^2 cells
constexpr int FP_MODE_OFF = 0, FP_MODE_AUDIT = 1, FP_MODE_STOP = 2;      // mpmpc_rollout_set_audit
constexpr int FP_ALIVE_CONTACT = -5;         // alive of a car that mode 2 ended

// the window's half-width as a double (the host compares it with the cap before it becomes an int)
inline double fp_reach_cells(double length, double width, double reach_m, double res) {
  return std::floor((reach_m + 0.5 * std::sqrt(length * length + width * width)) / res) + 1.0;
}

// step 2 and what step 3 needs of the car
struct FpCar {
  double x, y, c, s, hl, hw;      // centre, cos / sin of the heading, half length, half width
};
MPMPC_HOST_DEVICE inline FpCar fp_car(double x, double y, double psi, double length, double width) {
  return FpCar{x, y, std::cos(psi), std::sin(psi), 0.5 * length, 0.5 * width};
}

// step 3 for one cell: g, the squared distance of the cell's centre from the rectangle (0: inside or on it)
MPMPC_HOST_DEVICE inline double fp_cell_g(const MapView& m, const FpCar& k, int i, int j) {
  const double px = (i + 0.5) * m.res + m.ox, py = (j + 0.5) * m.res + m.oy;
  const double dx = px - k.x, dy = py - k.y;
  const double u = k.c * dx + k.s * dy, v = k.c * dy - k.s * dx;
  const double au = std::fabs(u) - k.hl, av = std::fabs(v) - k.hw;
  const double du = au > 0.0 ? au : 0.0, dv = av > 0.0 ? av : 0.0;
  return du * du + dv * dv;
}

constexpr double FP_NONE = __builtin_inf();     // best of a window without an occupied cell (+inf)

// step 4
MPMPC_HOST_DEVICE inline double fp_clearance(double best, double reach_m) {
  if (!(best <= 1.7976931348623157e308)) return reach_m;
  const double d = std::sqrt(best);
  return d < reach_m ? d : reach_m;
}

// The accumulators of a rollout (mpmpc_rollout_audit), updated with the verdict of step k for one car.  valid: step 1 gave
// a centre cell.  min_clearance starts at reach_m and min_step at -1: a step sets them only when it comes closer.
MPMPC_HOST_DEVICE inline void fp_accumulate(bool valid, int contact, double clearance, int k, int* contact_steps,
                                            int* first_contact, double* min_clearance, int* min_step, int* last_contact,
                                            double* last_clearance) {
  *last_contact = contact;
  *last_clearance = clearance;
  if (!valid) return;
  if (contact) {
    *contact_steps += 1;
    if (*first_contact < 0) *first_contact = k;
  }
  if (clearance < *min_clearance) {
    *min_clearance = clearance;
    *min_step = k;
  }
}

// Host-side validation of mpmpc_footprint_audit / mpmpc_rollout_set_audit: everything that can be refused before a device
// call.  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int fp_check_car(double length, double width, double reach_m, const char** why) {
  if (!(length > 0.0) || !mov_finite(length)) { *why = "the car's length must be positive and finite"; return -1; }
  if (!(width > 0.0) || !mov_finite(width)) { *why = "the car's width must be positive and finite"; return -1; }
  if (!(reach_m > 0.0) || !mov_finite(reach_m)) { *why = "the reach must be positive and finite"; return -1; }
  return 0;
}
// ... and the window; *R <- its half-width
inline int fp_check_reach(double length, double width, double reach_m, double res, int* R, const char** why) {
  const double r = fp_reach_cells(length, width, reach_m, res);
  if (!(r <= (double)FP_MAX_REACH_CELLS)) { *why = "reach plus half the car's diagonal is more than 256 cells (FP_MAX_REACH_CELLS)"; return -1; }
  *R = (int)r;
  return 0;
}
inline int fp_check_audit(int height, int width, const int8_t* data, double res, int B, const double* pose, const int32_t* off,
                          const int32_t* discs, double length, double car_width, double reach_m, const int32_t* contact,
                          const double* clearance, int* R, const char** why) {
  if (height < 1 || width < 1 || !(res > 0.0) || !mov_finite(res)) { *why = "map needs positive size and resolution"; return -1; }
  if (height > COR_MAX_SIDE || width > COR_MAX_SIDE) { *why = "map sides are limited to 65534 cells"; return -1; }
  if (B < 1) { *why = "B must be >= 1"; return -1; }
  if (!data || !pose || !contact || !clearance) { *why = "data, pose, contact_out and clearance_out must not be NULL"; return -1; }
  if (int rc = fp_check_car(length, car_width, reach_m, why)) return rc;
  if (int rc = fp_check_reach(length, car_width, reach_m, res, R, why)) return rc;
  return lid_check_discs(B, off, discs, width, height, why);
}

}  // namespace mpmpc
