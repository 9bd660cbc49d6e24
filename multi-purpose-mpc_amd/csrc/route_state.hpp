// Route fleets, the host side: which routes a handle's path table is made of, which route every instance of a batch is on, and
// every check that follows from the two (the law: include/mpmpc.h, mpmpc_set_routes).  Host code only - no HIP, no device
// memory: the handle (mpmpc_handle.hpp: TabState) owns one and adds the device copy of the per-instance headers;
// tests/emul_routes drives the same object without a device.  Every function returns MPMPC_OK or an error code with *why set.
#pragma once
#include <cstdint>
#include <vector>

#include "mpmpc.h"

namespace mpmpc {

struct RouteState {
  int n_routes = 0;      // 0: one path
  int car_B = 0;         // instances the car routes were given for (0: not given yet)
  std::vector<int32_t> first, circ, car_route;      // [n_routes + 1], [n_routes], [car_B]
  void clear() { n_routes = car_B = 0; first.clear(); circ.clear(); car_route.clear(); }

  // the arguments of set_routes on their own
  static int check(int n_wp, int P, const int32_t* f, const int32_t* c, const char** why) {
    if (P < 1 || !f || !c) return *why = "routes: need P >= 1, first and circular", MPMPC_E_ARG;
    return check_first(n_wp, P, f, why);
  }
  // ... of `first` alone (mpmpc_project takes routes without their flags)
  static int check_first(int n_wp, int P, const int32_t* f, const char** why) {
    if (f[0] != 0) return *why = "routes: first[0] must be 0", MPMPC_E_ARG;
    for (int p = 0; p < P; ++p) {
      if (f[p + 1] <= f[p]) return *why = "routes: first must be strictly increasing", MPMPC_E_ARG;
      if (f[p + 1] - f[p] < 2) return *why = "routes: every route needs at least 2 waypoints", MPMPC_E_ARG;
    }
    if (f[P] != n_wp) return *why = "routes: first[P] must be the number of waypoints of the path set", MPMPC_E_ARG;
    return MPMPC_OK;
  }
  // P routes on a path of n_wp waypoints (n_wp = 0: no path set); P = 0: one path again.  *changed: the routes are not what they were
  int set_routes(int n_wp, int P, const int32_t* f, const int32_t* c, bool* changed, const char** why) {
    *changed = false;
    if (P < 0) return *why = "routes: P must be >= 0", MPMPC_E_ARG;
    if (P == 0) {
      *changed = n_routes != 0;
      clear();
      return MPMPC_OK;
    }
    if (n_wp == 0) return *why = "no path set (mpmpc_set_path)", MPMPC_E_STATE;
    if (int rc = check(n_wp, P, f, c, why)) return rc;
    clear();
    first.assign(f, f + P + 1);
    circ.assign(c, c + P);
    n_routes = P;
    *changed = true;
    return MPMPC_OK;
  }
  // The route of every instance of the calls on B instances that follow -> hdr [B][2], what gather_stage reads
  // (PathTables::route): {first row, length - negated on an open route}.  Nothing is kept yet: the caller puts hdr on the
  // device and then calls keep_car_routes.
  int car_headers(int max_batch, int B, const int32_t* route, std::vector<int32_t>* hdr, const char** why) const {
    if (!route) return *why = "NULL argument", MPMPC_E_ARG;
    if (n_routes == 0) return *why = "no routes set (mpmpc_set_routes)", MPMPC_E_STATE;
    if (B < 1 || B > max_batch) return *why = "B must be in [1, max_batch]", MPMPC_E_ARG;
    hdr->resize(2 * (size_t)B);
    for (int i = 0; i < B; ++i) {
      const int p = route[i];
      if (p < 0 || p >= n_routes) return *why = "route id out of range", MPMPC_E_ARG;
      const int n = first[p + 1] - first[p];
      (*hdr)[2 * i] = first[p];
      (*hdr)[2 * i + 1] = circ[p] ? n : -n;
    }
    return MPMPC_OK;
  }
  void keep_car_routes(int B, const int32_t* route) { car_route.assign(route, route + B); car_B = B; }
  // Re-route (mpmpc_rollout_reroute): may the cars of a rollout of `rollout_B` cars (0: none in progress) be projected onto
  // route [B] (-1: keep)?  Nothing changes here: the device decides car by car, and `rerouted` then takes its verdicts.
  int check_reroute(int B, const int32_t* route, int rollout_B, const char** why) const {
    if (!route) return *why = "NULL argument", MPMPC_E_ARG;
    if (n_routes == 0) return *why = "no routes set (mpmpc_set_routes)", MPMPC_E_STATE;
    if (B < 1 || car_B != B) return *why = "no car routes for this number of instances (mpmpc_set_car_routes)", MPMPC_E_STATE;
    if (rollout_B != B) return *why = "no rollout in progress on this number of cars (mpmpc_rollout_init)", MPMPC_E_STATE;
    for (int i = 0; i < B; ++i)
      if (route[i] < -1 || route[i] >= n_routes) return *why = "route id out of range (-1 keeps the car's route)", MPMPC_E_ARG;
    return MPMPC_OK;
  }
  // {first row, length - negated on an open route} of every route: what the device writes into an accepted car's header
  void route_headers(std::vector<int32_t>* hdr) const {
    hdr->resize(2 * (size_t)n_routes);
    for (int p = 0; p < n_routes; ++p) {
      const int n = first[p + 1] - first[p];
      (*hdr)[2 * p] = first[p];
      (*hdr)[2 * p + 1] = circ[p] ? n : -n;
    }
  }
  // the cars the device accepted are on their new routes: check_wp_ids and every later call see them
  void rerouted(int B, const int32_t* route, const int32_t* accepted) {
    for (int i = 0; i < B; ++i)
      if (accepted[i]) car_route[i] = route[i];
  }
  // the route every car is on now
  int car_routes(int B, int32_t* route_out, const char** why) const {
    if (!route_out) return *why = "NULL argument", MPMPC_E_ARG;
    if (n_routes == 0) return *why = "no routes set (mpmpc_set_routes)", MPMPC_E_STATE;
    if (B < 1 || car_B != B) return *why = "no car routes for this number of instances (mpmpc_set_car_routes)", MPMPC_E_STATE;
    for (int i = 0; i < B; ++i) route_out[i] = car_route[i];
    return MPMPC_OK;
  }
  // With routes set, a call on B instances needs their routes.  (Without routes: nothing to check.)
  int check_batch(int B, const char** why) const {
    if (n_routes && car_B != B) return *why = "routes are set: call mpmpc_set_car_routes for this number of instances first", MPMPC_E_STATE;
    return MPMPC_OK;
  }
  // The waypoint ids of a batch: 0 <= wp < n, and an open path ends the run when the horizon passes its last waypoint
  // (src/reference_path.py:367-369) - n and the flag of the one path (n_wp, circular), or of every instance's own route
  int check_wp_ids(int B, const int32_t* wp_id, int N, int n_wp, bool circular, const char** why) const {
    if (int rc = check_batch(B, why)) return rc;
    for (int i = 0; i < B; ++i) {
      const int p = n_routes ? car_route[i] : 0;
      const int n = n_routes ? first[p + 1] - first[p] : n_wp;
      const bool closed = n_routes ? circ[p] != 0 : circular;
      if (wp_id[i] < 0 || wp_id[i] >= n) return *why = "wp_id out of range", MPMPC_E_ARG;
      if (!closed && wp_id[i] + N >= n) return *why = "Reached end of path!", MPMPC_E_ARG;
    }
    return MPMPC_OK;
  }
};

}  // namespace mpmpc
