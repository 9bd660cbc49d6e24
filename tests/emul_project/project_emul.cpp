// CPU twin of the pose projection and of the re-route (tests/test_reroute.py): the library's own law (project_core.hpp) on 64
// emulated lanes - every lane strides over the route's waypoints, then the six-step xor butterfly of mpmpc_project_kernel - and
// the handle's route state (route_state.hpp) for the checks and the bookkeeping of mpmpc_rollout_reroute.  Built by
// tests/emul/Makefile (`make project`), loaded by tests/twins.py.
#include <cstdint>
#include <vector>

#include "project_core.hpp"
#include "route_state.hpp"

using namespace mpmpc;

namespace {
constexpr int W = 64;
// one (pose, route) pair as one wavefront does it
void project_pair(const double* x, const double* y, const double* psi, const double* cum, int n, const double* pose, double max_heading,
                  int* wp, double* dist, double* x0, double* s) {
  ProjBest lane[W], next[W];
  for (int l = 0; l < W; ++l) lane[l] = proj_lane_scan(x, y, psi, n, pose[0], pose[1], pose[2], max_heading, l, W);
  for (int m = 1; m < W; m <<= 1) {
    for (int l = 0; l < W; ++l) next[l] = proj_merge(lane[l], lane[l ^ m]);
    for (int l = 0; l < W; ++l) lane[l] = next[l];
  }
  proj_finish(x, y, psi, cum, pose[0], pose[1], pose[2], lane[0], wp, dist, x0, s);
}
}  // namespace

// mpmpc_project without a device: the same checks, the same codes
extern "C" int project_emu(int n_wp, const double* x, const double* y, const double* psi, const double* cum, int P, const int32_t* first,
                           int B, const double* pose, int K, const int32_t* cand, double max_heading, int32_t* wp_out, double* dist_out,
                           double* x0_out, double* s_out, const char** why) {
  if (proj_check_args(n_wp, x, y, psi, cum, P, first, B, pose, K, cand, max_heading, why)) return MPMPC_E_ARG;
  const int32_t one[2] = {0, n_wp};
  if (P > 0 && first) {
    if (int rc = RouteState::check_first(n_wp, P, first, why)) return rc;
  } else {
    first = one;
  }
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < K; ++k) {
      const long q = (long)b * K + k;
      const int p = cand ? cand[q] : k;
      const long f = first[p];
      int wp;
      double dist, s, x0[3];
      project_pair(x + f, y + f, psi + f, cum + f, first[p + 1] - first[p], pose + 3L * b, max_heading, &wp, &dist, x0, &s);
      if (wp_out) wp_out[q] = wp;
      if (dist_out) dist_out[q] = dist;
      if (s_out) s_out[q] = s;
      if (x0_out)
        for (int c = 0; c < 3; ++c) x0_out[3 * q + c] = x0[c];
    }
  return MPMPC_OK;
}

// The handle's side of a re-route without a handle: the route state, the path's length and the rollout in progress (B cars, 0:
// none) stand in for the handle; the cars' device state is the caller's arrays.
struct RerouteTwin {
  RouteState r;
  int n_wp = 0, max_batch = 0, rollout_B = 0;
  const char* why = "";
};
extern "C" RerouteTwin* reroute_twin_new(int n_wp, int max_batch) {
  RerouteTwin* t = new RerouteTwin();
  t->n_wp = n_wp; t->max_batch = max_batch;
  return t;
}
extern "C" void reroute_twin_free(RerouteTwin* t) { delete t; }
extern "C" const char* reroute_twin_why(RerouteTwin* t) { return t->why; }
extern "C" int reroute_twin_set_routes(RerouteTwin* t, int P, const int32_t* first, const int32_t* circular) {
  bool changed = false;
  const int rc = t->r.set_routes(t->n_wp, P, first, circular, &changed, &t->why);
  if (changed) t->rollout_B = 0;      // (routes_change ends a rollout)
  return rc;
}
extern "C" int reroute_twin_set_car_routes(RerouteTwin* t, int B, const int32_t* route, int32_t* hdr_out) {
  std::vector<int32_t> hdr;
  if (int rc = t->r.car_headers(t->max_batch, B, route, &hdr, &t->why)) return rc;
  for (size_t i = 0; i < hdr.size(); ++i) hdr_out[i] = hdr[i];
  t->r.keep_car_routes(B, route);
  t->rollout_B = 0;                   // (mpmpc_set_car_routes ends a rollout)
  return MPMPC_OK;
}
extern "C" int reroute_twin_rollout_init(RerouteTwin* t, int B) {
  if (int rc = t->r.check_batch(B, &t->why)) return rc;
  t->rollout_B = B;
  return MPMPC_OK;
}
extern "C" int reroute_twin_check_upload(RerouteTwin* t, int B, const int32_t* wp_id, int N) {
  return t->r.check_wp_ids(B, wp_id, N, t->n_wp, true, &t->why);
}
extern "C" int reroute_twin_routes(RerouteTwin* t, int B, int32_t* route_out) { return t->r.car_routes(B, route_out, &t->why); }

// mpmpc_rollout_reroute: the entry point's checks in its order, mpmpc_project_kernel and mpmpc_reroute_apply_kernel car by car,
// then the mirror.  hdr [B][2], s [B], wp_id [B], x0 [B][3] are updated in place for accepted cars and left alone otherwise.
extern "C" int reroute_twin_reroute(RerouteTwin* t, int B, const int32_t* route, double max_dist, double max_heading, const double* x,
                                    const double* y, const double* psi, const double* cum, const double* pose, const int32_t* alive,
                                    int32_t* hdr, double* s, int32_t* wp_id, double* x0, int32_t* accepted) {
  if (!route) return t->why = "NULL argument", MPMPC_E_ARG;
  if (!(max_dist >= 0.0)) return t->why = "reroute: max_dist must be >= 0 (and not NaN; +inf: no limit)", MPMPC_E_ARG;
  if (!(max_heading >= 0.0)) return t->why = "reroute: max_heading must be >= 0 (and not NaN)", MPMPC_E_ARG;
  if (int rc = t->r.check_reroute(B, route, t->rollout_B, &t->why)) return rc;
  std::vector<int32_t> rhdr;
  t->r.route_headers(&rhdr);
  for (int i = 0; i < B; ++i) {
    int wp = -1;
    double dist = __builtin_inf(), s_new = 0.0, x0_new[3] = {0.0, 0.0, 0.0};
    const int p = route[i];
    if (p >= 0 && alive[i] == 1) {
      const long f = t->r.first[p];
      project_pair(x + f, y + f, psi + f, cum + f, t->r.first[p + 1] - t->r.first[p], pose + 3L * i, max_heading, &wp, &dist, x0_new, &s_new);
    }
    accepted[i] = proj_accept(wp, dist, max_dist) ? 1 : 0;
    if (!accepted[i]) continue;
    hdr[2 * i] = rhdr[2 * p];
    hdr[2 * i + 1] = rhdr[2 * p + 1];
    s[i] = s_new;
    wp_id[i] = wp;
    for (int c = 0; c < 3; ++c) x0[3 * i + c] = x0_new[c];
  }
  t->r.rerouted(B, route, accepted);
  return MPMPC_OK;
}
