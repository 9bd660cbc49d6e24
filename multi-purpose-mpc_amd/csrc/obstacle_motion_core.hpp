// Moving obstacles of the device rollout ("movers"): where a car's moving discs are at rollout step k.  Scalar
// per-mover code that compiles for gfx950 (K0m, mpmpc_obstacle_move_kernel in mpmpc_closed_loop.hpp) and for the host
// (tests/emul_movers), like corridor_core.hpp and rollout_core.hpp.
//
// A mover is a disc of constant radius r (map cells, Map.add_obstacles' ceil(radius / resolution)) whose centre is a
// CLOSED-FORM function of the rollout step index k (0-based, counted from mpmpc_rollout_init), not of accumulated
// state: the discs of any step can be recomputed from its index.  With j = (double)(k - step0), every product and sum
// below rounded on its own (the build has -ffp-contract=off), in exactly this order:
//
//   kind 0 (MOV_LINE), parameters (x0, y0, dx, dy) - world start point and displacement per step [m]:
//       x = x0 + j * dx                  y = y0 + j * dy
//   kind 1 (MOV_PATH), parameters (s0, e, ds, unused) - start arc length, lateral offset (positive = left, the sign
//   of e_y in ro_pred_point), arc length per step:
//       s = s0 + j * ds                  L = cum[n_wp - 1]
//       absent unless s is finite and L > 0
//       circular path:   s = s - L * floor(s / L);  then ONE guard: a result outside [0, L) (rounding at a multiple
//                        of L) becomes 0
//       open path:       absent unless 0 <= s < L
//       i = the largest index with cum[i] <= s, clamped to [0, n_wp - 2]       (binary search)
//       den = cum[i+1] - cum[i];   f = den > 0 ? (s - cum[i]) / den : 0        (an empty segment: its start point)
//       x = (x_i + f * (x_{i+1} - x_i)) - e * sin(psi_i)
//       y = (y_i + f * (y_{i+1} - y_i)) + e * cos(psi_i)
//     sin / cos(psi_i) come from K0's per-waypoint table (cor_trig_row: the HOST's libm), so that - as in K0 and the
//     recorder - no device-libm result decides a cell.
//   the disc:  qx = floor((x - ox) / res), qy = floor((y - oy) / res)          (cor_w2m's expression)
//       absent unless |qx| <= 2^30 and |qy| <= 2^30 (a NaN fails both); (cx, cy) = (int)(qx, qy)
//       absent if cx - r < 0 or cy - r < 0 or cx + r > width or cy + r > height  (cor_check_obstacles' test: the
//       disc's square leaves the grid)
//   An absent mover is the disc (0, 0, 0): by cor_in_disc and cor_disc_meets_box it occupies no cell and meets no box.
#pragma once
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "corridor_core.hpp"

namespace mpmpc {

constexpr int MOV_LINE = 0, MOV_PATH = 1;
constexpr int MOV_PARAMS = 4;                      // doubles per mover
constexpr double MOV_CELL_MAX = 1073741824.0;      // 2^30: cell coordinates beyond it are not converted to int

// what kind 1 reads of the path: the rollout's cumulative lengths and K0's per-waypoint tables
struct MoverPath {
  const double *cum, *x, *y;      // [n_wp]
  const double* trig;             // [n_wp x trig_ld]: cos(psi), sin(psi), ...
  int n_wp, trig_ld, circular;
};
// route fleets: the path moved onto a car's view (corridor_core.hpp) - an along-the-path mover follows its car's route
MPMPC_HD MoverPath route_path(MoverPath p, RouteView v) {
  p.cum += v.first; p.x += v.first; p.y += v.first; p.trig += v.first * p.trig_ld;
  v.lengths(p.n_wp, p.circular);
  return p;
}

MPMPC_HOST_DEVICE inline bool mov_finite(double v) { return std::fabs(v) <= 1.7976931348623157e308; }

// world centre of a mover at j = k - step0; false: absent (kind 1 only)
MPMPC_HD bool mov_centre(const MoverPath& p, int kind, double p0, double p1, double p2, double p3, double j, double* x,
                         double* y) {
  if (kind == MOV_LINE) {
    *x = p0 + j * p2;
    *y = p1 + j * p3;
    return true;
  }
  double s = p0 + j * p2;
  const double L = p.cum[p.n_wp - 1];
  if (!mov_finite(s) || !(L > 0.0)) return false;
  if (p.circular) {
    s = s - L * std::floor(s / L);
    if (!(s >= 0.0 && s < L)) s = 0.0;
  } else if (!(s >= 0.0 && s < L)) {
    return false;
  }
  int lo = 0, hi = p.n_wp;                 // first index with cum > s
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (p.cum[mid] > s) hi = mid; else lo = mid + 1;
  }
  int i = lo - 1;
  i = i < 0 ? 0 : (i > p.n_wp - 2 ? p.n_wp - 2 : i);
  const double den = p.cum[i + 1] - p.cum[i];
  const double f = den > 0.0 ? (s - p.cum[i]) / den : 0.0;
  const double c = p.trig[(long long)i * p.trig_ld], sn = p.trig[(long long)i * p.trig_ld + 1];
  *x = (p.x[i] + f * (p.x[i + 1] - p.x[i])) - p1 * sn;
  *y = (p.y[i] + f * (p.y[i + 1] - p.y[i])) + p1 * c;
  return true;
}

// the disc d = (cx, cy, r) of a mover at rollout step k, or (0, 0, 0) when it is absent
MPMPC_HD void mov_disc(const MapView& m, const MoverPath& p, int kind, int r, double p0, double p1, double p2, double p3,
                       long long k, long long step0, int* d) {
  d[0] = 0; d[1] = 0; d[2] = 0;
  double x, y;
  if (!mov_centre(p, kind, p0, p1, p2, p3, (double)(k - step0), &x, &y)) return;
  const double qx = std::floor((x - m.ox) / m.res), qy = std::floor((y - m.oy) / m.res);
  if (!(std::fabs(qx) <= MOV_CELL_MAX && std::fabs(qy) <= MOV_CELL_MAX)) return;
  const long long cx = (long long)qx, cy = (long long)qy;
  if (cx - r < 0 || cy - r < 0 || cx + r > m.width || cy + r > m.height) return;
  d[0] = (int)cx; d[1] = (int)cy; d[2] = r;
}

// The three per-car settings of a rollout - static discs (mpmpc_rollout_set_obstacles), movers
// (mpmpc_rollout_set_movers) and traffic (mpmpc_rollout_set_traffic, traffic_core.hpp) - share one CSR list per car: the
// static discs first, then one slot per mover, then the car's traffic slots (the same number for every car).  B_x = 0:
// that setting is off.  Returns 0, -1 (MPMPC_E_ARG) or -3 (MPMPC_E_STATE) and the reason.
inline int mov_check_combined(int B_static, const int32_t* off_static, int B_movers, const int32_t* off_movers,
                              const char** why, int B_traffic = 0, int traffic_slots = 0) {
  int B = 0, on = 0;
  for (const int v : {B_static, B_movers, B_traffic}) {
    if (v <= 0) continue;
    if (on > 0 && v != B) { *why = "static obstacles, movers and traffic were set for different numbers of cars"; return -3; }
    B = v;
    ++on;
  }
  if (on < 2) return 0;
  for (int b = 0; b < B; ++b) {
    const long ns = B_static > 0 ? (long)off_static[b + 1] - off_static[b] : 0;
    const long nm = B_movers > 0 ? (long)off_movers[b + 1] - off_movers[b] : 0;
    if (ns + nm + (B_traffic > 0 ? traffic_slots : 0) > COR_MAX_DISCS) {
      *why = "more than 64 static discs, movers and traffic slots together for one car (COR_MAX_DISCS)";
      return -1;
    }
  }
  return 0;
}

// Host-side validation of mpmpc_rollout_set_movers (offsets != NULL); B_static / off_static: the static setting in force,
// B_traffic / traffic_slots: the traffic in force.
inline int mov_check_movers(int B, int max_batch, const int32_t* off, const int32_t* kind, const int32_t* radius,
                            const double* params, bool built, int B_static, const int32_t* off_static, const char** why,
                            int B_traffic = 0, int traffic_slots = 0) {
  if (!built) { *why = "needs mpmpc_build_corridor on the current map and path geometry first"; return -3; }
  if (B < 1 || B > max_batch) { *why = "B must be in [1, max_batch]"; return -1; }
  if (off[0] != 0) { *why = "offsets[0] must be 0"; return -1; }
  for (int b = 0; b < B; ++b) {
    const long n = (long)off[b + 1] - off[b];
    if (n < 0) { *why = "offsets must not decrease"; return -1; }
    if (n > COR_MAX_DISCS) { *why = "more than 64 movers for one car (COR_MAX_DISCS)"; return -1; }
  }
  if (off[B] > 0 && (!kind || !radius || !params)) { *why = "kind, radius_cells or params is NULL"; return -1; }
  for (long j = 0; j < off[B]; ++j) {
    if (kind[j] != MOV_LINE && kind[j] != MOV_PATH) { *why = "unknown mover kind"; return -1; }
    if (radius[j] < 0) { *why = "a mover has a negative radius"; return -1; }
    for (int t = 0; t < MOV_PARAMS; ++t)
      if (!mov_finite(params[MOV_PARAMS * j + t])) { *why = "a mover parameter is not finite"; return -1; }
  }
  return mov_check_combined(B_static, off_static, B, off, why, B_traffic, traffic_slots);
}

// Combined offsets [B + 1] and, per mover, the index of its slot in the combined disc list.  Either offsets may be
// NULL (that setting is off); traffic_slots = 0: no traffic.  Car b's traffic slots are the last traffic_slots entries
// of its list: off[b + 1] - traffic_slots .. off[b + 1] - 1.
inline void mov_combine(int B, const int32_t* off_static, const int32_t* off_movers, int32_t* off, int32_t* dst,
                        int traffic_slots = 0) {
  off[0] = 0;
  for (int b = 0; b < B; ++b) {
    const int ns = off_static ? off_static[b + 1] - off_static[b] : 0;
    const int nm = off_movers ? off_movers[b + 1] - off_movers[b] : 0;
    for (int q = 0; q < nm; ++q) dst[off_movers[b] + q] = off[b] + ns + q;
    off[b + 1] = off[b] + ns + nm + traffic_slots;
  }
}

}  // namespace mpmpc
