// Where is a pose on a route?  Scalar code that compiles for gfx950 (mpmpc_project_kernel in mpmpc_project.hpp) and for the host
// (tests/emul_project).  The reference has no such step - its car is born at waypoint 0 (src/spatial_bicycle_models.py:36-60) -
// but a fleet started from world poses, or a car that changes route while it drives (mpmpc_rollout_reroute), needs it.
//
// The law.  A route is rows 0 .. n - 1 of x, y, psi, cum (the caller offsets the pointers to the route's first row; cum is the
// route's own cumulative length, cum[0] = 0).  For a pose (px, py, ppsi) and every waypoint j:
//   d2[j]    = dx dx + dy dy, dx = px - x[j], dy = py - y[j], every operation rounded on its own (-ffp-contract=off)
//   e_psi[j] = the heading error of ro_t2s: fmod(ppsi - psi[j] + pi, 2 pi), + 2 pi if negative, - pi
//   eligible   |e_psi[j]| <= max_heading   (max_heading >= pi: every waypoint)
//   wp       = the eligible j of the smallest d2, ties to the lowest j; -1 if none is eligible or the pose is not finite
//   dist = sqrt(d2[wp]), x0 = ro_t2s(pose, waypoint wp), s = cum[wp]          (wp = -1: +inf, NaN, NaN)
// s = cum[wp] on purpose: ro_current_waypoint(cum, n, s) then returns wp again for every wp < n - 1, and -1 at wp = n - 1 (the
// car has finished, as the reference's loop guard `car.s < length` decides).
// The search is written for ONE LANE of a wavefront that strides over the waypoints (proj_lane_scan) and for the exchange step of
// the butterfly that follows (proj_merge): both keep the lexicographic minimum of (d2, j), so any split of the waypoints over
// lanes and any order of the merges gives the law's answer.
#pragma once
#include <cmath>

#include "rollout_core.hpp"

namespace mpmpc {

constexpr int PROJ_NONE = 0x7fffffff;      // "no waypoint yet": behind every j
struct ProjBest {
  double d2;
  int j;
};
MPMPC_HD ProjBest proj_none() { return ProjBest{__builtin_inf(), PROJ_NONE}; }
MPMPC_HD bool proj_finite(double v) { return std::fabs(v) <= 1.7976931348623157e308; }      // (false for NaN)
MPMPC_HD double proj_heading_error(double ppsi, double wpsi) {                              // x0[1] of ro_t2s, the same operations
  double t = std::fmod(ppsi - wpsi + RO_PI, 2.0 * RO_PI);
  if (t < 0.0) t += 2.0 * RO_PI;
  return t - RO_PI;
}
// a comes before b: smaller d2, or the same d2 at a lower j.  A NaN d2 comes before nothing.
// (by value, and chosen field by field: a choice between two references would put both in private memory)
MPMPC_HD bool proj_before(ProjBest a, ProjBest b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.j < b.j); }
MPMPC_HD ProjBest proj_merge(ProjBest mine, ProjBest other) {
  const bool take = proj_before(other, mine);
  return ProjBest{take ? other.d2 : mine.d2, take ? other.j : mine.j};
}

// the best of waypoints lane, lane + stride, ... < n (lane 0, stride 1: the whole route)
MPMPC_HD ProjBest proj_lane_scan(const double* x, const double* y, const double* psi, int n, double px, double py, double ppsi,
                                 double max_heading, int lane, int stride) {
  ProjBest best = proj_none();
  if (!(proj_finite(px) && proj_finite(py) && proj_finite(ppsi))) return best;
  for (int j = lane; j < n; j += stride) {
    const double dx = px - x[j], dy = py - y[j];
    const ProjBest c{dx * dx + dy * dy, j};
    if (std::fabs(proj_heading_error(ppsi, psi[j])) <= max_heading && proj_before(c, best)) best = c;
  }
  return best;
}

// the outputs of one (pose, route) pair from the winner
MPMPC_HD void proj_finish(const double* x, const double* y, const double* psi, const double* cum, double px, double py, double ppsi,
                          ProjBest best, int* wp, double* dist, double* x0, double* s) {
  const double nan = __builtin_nan("");
  if (best.j == PROJ_NONE) {
    *wp = -1; *dist = __builtin_inf(); *s = nan;
    x0[0] = x0[1] = x0[2] = nan;
    return;
  }
  *wp = best.j;
  *dist = std::sqrt(best.d2);
  *s = cum[best.j];
  ro_t2s(px, py, ppsi, x[best.j], y[best.j], psi[best.j], x0);
}

// mpmpc_rollout_reroute: does the car take the route it was projected on?
MPMPC_HD bool proj_accept(int wp, double dist, double max_dist) { return wp >= 0 && dist <= max_dist; }

// ---- the argument checks of mpmpc_project (host): 0, or -1 with *why set.  P = 0 or first = null: one route of n_wp rows.
inline int proj_routes_of(int P, const int* first) { return P > 0 && first ? P : 1; }
inline int proj_check_args(int n_wp, const double* x, const double* y, const double* psi, const double* cum, int P, const int* first,
                           int B, const double* pose, int K, const int* cand, double max_heading, const char** why) {
  if (!x || !y || !psi || !cum || !pose) return *why = "project: x, y, psi, cum and pose must not be NULL", -1;
  if (n_wp < 2) return *why = "project: need at least 2 waypoints", -1;
  if (P < 0) return *why = "project: P must be >= 0", -1;
  if (B < 1 || K < 1) return *why = "project: need B >= 1 poses and K >= 1 candidates", -1;
  if ((long long)B * K > 2147483647LL / 3) return *why = "project: more than 2^31 / 3 (pose, route) pairs in one call", -1;
  if (!(max_heading >= 0.0)) return *why = "project: max_heading must be >= 0 (and not NaN)", -1;
  const int routes = proj_routes_of(P, first);
  if (!cand && K != routes) return *why = "project: cand = NULL means every route: K must be the number of routes", -1;
  if (cand)
    for (long long q = 0; q < (long long)B * K; ++q)
      if (cand[q] < 0 || cand[q] >= routes) return *why = "project: candidate route id out of range", -1;
  return 0;
}

}  // namespace mpmpc
