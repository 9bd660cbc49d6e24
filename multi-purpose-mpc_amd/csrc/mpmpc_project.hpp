// Pose projection of libmpmpc.so, part of the one translation unit mpmpc_hip.hip (included there behind mpmpc_footprint.hpp):
// the kernels mpmpc_project_kernel and mpmpc_reroute_apply_kernel and the entry points mpmpc_project (no handle, like
// mpmpc_lidar_scan), mpmpc_rollout_reroute and mpmpc_rollout_routes.  The law: project_core.hpp.
#pragma once

// One WAVEFRONT per (pose, candidate route) pair q.  The lanes stride over the route's waypoints (j = lane, lane + 64, ...:
// consecutive lanes read consecutive doubles of x, y, psi; many pairs share a route, so the tables are served from the L2), each
// keeps the lexicographic minimum of (d2, j) of its own waypoints, a six-step xor butterfly leaves the wave's minimum in every
// lane, and lane 0 forms the outputs (proj_finish).  No LDS, no scratch.
//   cand [n_pairs]  the route of pair q, or null: route q % K ("every route").  An id < 0 skips the pair (wp = -1): the cars a
//                   re-route keeps.
//   alive           null, or [n_pairs / K]: a pair of a car that is not running (alive != 1) is skipped too.
//   first [P + 1]   the routes' first rows (checked on the host: 0 = first[0] < ... < first[P] = rows of the tables).
// Outputs [n_pairs] (x0 [n_pairs][3]); every index is bounded by the host's checks of first and cand.
__global__ __launch_bounds__(64) void mpmpc_project_kernel(int n_pairs, int K, const int* __restrict__ cand, const int* __restrict__ first,
                                                           const double* __restrict__ x, const double* __restrict__ y,
                                                           const double* __restrict__ psi, const double* __restrict__ cum,
                                                           const double* __restrict__ pose, const int* __restrict__ alive,
                                                           double max_heading, int* __restrict__ wp_out, double* __restrict__ dist_out,
                                                           double* __restrict__ x0_out, double* __restrict__ s_out) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= n_pairs) return;      // (uniform)
  const int car = q / K;
  const int p = cand ? cand[q] : q - car * K;
  const bool skip = p < 0 || (alive && alive[car] != 1);      // (uniform)
  const double px = pose[3L * car], py = pose[3L * car + 1], ppsi = pose[3L * car + 2];
  ProjBest best = proj_none();
  long f = 0;
  if (!skip) {
    f = first[p];
    best = proj_lane_scan(x + f, y + f, psi + f, first[p + 1] - first[p], px, py, ppsi, max_heading, lane, 64);
  }
  for (int m = 1; m < 64; m <<= 1) {
    const ProjBest other{__shfl_xor(best.d2, m, 64), __shfl_xor(best.j, m, 64)};
    best = proj_merge(best, other);
  }
  if (lane == 0) proj_finish(x + f, y + f, psi + f, cum + f, px, py, ppsi, best, wp_out + q, dist_out + q, x0_out + 3L * q, s_out + q);
}

// mpmpc_rollout_reroute, after the projection (one thread per car): an accepted car takes its new route's header, s = cum at the
// waypoint it was projected on, and that waypoint and its path-relative state as wp_id / x0 - the batch blocks then hold ids that
// are local to the routes the headers name (a solve on them reads no row outside its route); the next step localises anew.
// rhdr [P][2]: the header of every route (RouteState::route_headers).  Everything else of the car is left as it is.
__global__ __launch_bounds__(256) void mpmpc_reroute_apply_kernel(int B, const int* __restrict__ route, const int* __restrict__ rhdr,
                                                                  const int* __restrict__ wp, const double* __restrict__ dist,
                                                                  const double* __restrict__ x0_new, const double* __restrict__ s_new,
                                                                  double max_dist, int* __restrict__ hdr, double* __restrict__ s,
                                                                  int* __restrict__ wp_id, double* __restrict__ x0,
                                                                  int* __restrict__ accepted) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const bool ok = proj_accept(wp[i], dist[i], max_dist);      // (wp = -1 for a kept car and for one that is not running)
  accepted[i] = ok ? 1 : 0;
  if (!ok) return;
  const int p = route[i];
  hdr[2 * i] = rhdr[2 * p];
  hdr[2 * i + 1] = rhdr[2 * p + 1];
  s[i] = s_new[i];
  wp_id[i] = wp[i];
  x0[3 * i] = x0_new[3 * i]; x0[3 * i + 1] = x0_new[3 * i + 1]; x0[3 * i + 2] = x0_new[3 * i + 2];
}

// device scratch of mpmpc_project, kept between calls like the speed profile's (SpScratch)
static SpScratch g_proj_dev[SP_MAX_DEVICES];

extern "C" {

int mpmpc_project(int32_t device, int32_t n_wp, const double* x, const double* y, const double* psi, const double* cum, int32_t P,
                  const int32_t* first, int32_t B, const double* pose, int32_t K, const int32_t* cand, double max_heading,
                  int32_t* wp_out, double* dist_out, double* x0_out, double* s_out) {
  const char* why = "";
  if (proj_check_args(n_wp, x, y, psi, cum, P, first, B, pose, K, cand, max_heading, &why)) return fail(MPMPC_E_ARG, why);
  const int routes = proj_routes_of(P, first);
  const int32_t one[2] = {0, n_wp};
  if (P > 0 && first) {
    if (int rc = RouteState::check_first(n_wp, P, first, &why)) return fail(rc, why);
  } else {
    first = one;
  }
  const size_t n = (size_t)n_wp, nb = (size_t)B, pairs = nb * K;
  Layout L;
  const auto r_x = L.add<double>(n), r_y = L.add<double>(n), r_psi = L.add<double>(n), r_cum = L.add<double>(n), r_pose = L.add<double>(3 * nb),
             r_dist = L.add<double>(pairs), r_x0 = L.add<double>(3 * pairs), r_s = L.add<double>(pairs);
  const auto r_wp = L.add<int>(pairs), r_first = L.add<int>((size_t)routes + 1), r_cand = L.add<int>(cand ? pairs : 0);
  Scratch sc;
  if (int rc = scratch_acquire(g_proj_dev, device, L.bytes(), "projection", &sc)) return rc;
  hipStream_t stream = sc.stream;
  char* blk = sc.blk;
  HIP_TRY(hipMemcpyAsync(r_x.at(blk), x, r_x.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_y.at(blk), y, r_y.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_psi.at(blk), psi, r_psi.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_cum.at(blk), cum, r_cum.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_pose.at(blk), pose, r_pose.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_first.at(blk), first, r_first.bytes(), hipMemcpyHostToDevice, stream));
  if (cand) HIP_TRY(hipMemcpyAsync(r_cand.at(blk), cand, r_cand.bytes(), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(mpmpc_project_kernel, dim3((unsigned)pairs), dim3(64), 0, stream, (int)pairs, K, cand ? r_cand.at(blk) : nullptr,
                     r_first.at(blk), r_x.at(blk), r_y.at(blk), r_psi.at(blk), r_cum.at(blk), r_pose.at(blk), nullptr, max_heading,
                     r_wp.at(blk), r_dist.at(blk), r_x0.at(blk), r_s.at(blk));
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(stream, wp_out, r_wp.at(blk), pairs));
  HIP_TRY(pull(stream, dist_out, r_dist.at(blk), pairs));
  HIP_TRY(pull(stream, x0_out, r_x0.at(blk), 3 * pairs));
  HIP_TRY(pull(stream, s_out, r_s.at(blk), pairs));
  HIP_TRY(hipStreamSynchronize(stream));
  return MPMPC_OK;
}

int mpmpc_rollout_reroute(mpmpc_handle h, int32_t B, const int32_t* route, double max_dist, double max_heading,
                          int32_t* accepted_out) {
  if (int rc = enter(h, route)) return rc;
  if (!(max_dist >= 0.0)) return fail(MPMPC_E_ARG, "reroute: max_dist must be >= 0 (and not NaN; +inf: no limit)");
  if (!(max_heading >= 0.0)) return fail(MPMPC_E_ARG, "reroute: max_heading must be >= 0 (and not NaN)");
  TabState& t = h->tab;
  const char* why = "";
  if (int rc = t.routes.check_reroute(B, route, h->ro.valid ? h->ro.B : 0, &why)) return fail(rc, why);
  if (h->cor.geom_n != t.n_wp) return fail(MPMPC_E_STATE, "needs mpmpc_set_path_geometry for the path set");
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  // one block of the handle's own, max_batch cars and the routes of the moment wide: route, wp, accepted [mb] ints, the routes'
  // headers and first rows, then dist, s [mb] and x0 [mb][3] doubles
  const size_t mb = (size_t)h->cfg.max_batch, P = (size_t)t.routes.n_routes;
  const size_t o_route = 0, o_wp = o_route + pad8(sizeof(int) * mb), o_acc = o_wp + pad8(sizeof(int) * mb),
               o_rhdr = o_acc + pad8(sizeof(int) * mb), o_first = o_rhdr + pad8(sizeof(int) * 2 * P),
               o_dist = o_first + pad8(sizeof(int) * (P + 1)), o_s = o_dist + sizeof(double) * mb, o_x0 = o_s + sizeof(double) * mb,
               need = o_x0 + sizeof(double) * 3 * mb;
  if (h->ro.reroute.count() < need) HIP_TRY(h->ro.reroute.alloc(need));
  char* blk = h->ro.reroute;
  std::vector<int32_t> rhdr, acc((size_t)B);
  t.routes.route_headers(&rhdr);
  HIP_TRY(hipMemcpyAsync(blk + o_route, route, sizeof(int) * B, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipMemcpyAsync(blk + o_rhdr, rhdr.data(), sizeof(int) * 2 * P, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipMemcpyAsync(blk + o_first, t.routes.first.data(), sizeof(int) * (P + 1), hipMemcpyHostToDevice, sl.stream));
  hipLaunchKernelGGL(mpmpc_project_kernel, dim3(B), dim3(64), 0, sl.stream, B, 1, (const int*)(blk + o_route),
                     (const int*)(blk + o_first), h->cor.gx.get(), h->cor.gy.get(), h->cor.gpsi.get(), h->ro.cum.get(),
                     h->ro.pose.get(), h->ro.alive.get(), max_heading, (int*)(blk + o_wp), (double*)(blk + o_dist),
                     (double*)(blk + o_x0), (double*)(blk + o_s));
  hipLaunchKernelGGL(mpmpc_reroute_apply_kernel, dim3((B + 255) / 256), dim3(256), 0, sl.stream, B, (const int*)(blk + o_route),
                     (const int*)(blk + o_rhdr), (const int*)(blk + o_wp), (const double*)(blk + o_dist),
                     (const double*)(blk + o_x0), (const double*)(blk + o_s), max_dist, t.car_hdr.get(), h->ro.s.get(), h->io.wp_id,
                     h->io.x0, (int*)(blk + o_acc));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(acc.data(), blk + o_acc, sizeof(int) * B, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));      // `rhdr` and `acc` leave scope; the mirror needs the verdicts
  t.routes.rerouted(B, route, acc.data());
  h->tlk.forget();      // (traffic lookahead: a plan track lies on the route it was made on - the whole fleet's start over)
  if (h->cm.B > 0) {    // (commitment: a memory lies on the route it was made on - the accepted cars' are emptied)
    if (int rc = commitment_rerouted(h, sl, B, acc.data())) return rc;
    HIP_TRY(hipStreamSynchronize(sl.stream));
  }
  if (accepted_out) std::memcpy(accepted_out, acc.data(), sizeof(int32_t) * (size_t)B);
  return MPMPC_OK;
}

int mpmpc_rollout_routes(mpmpc_handle h, int32_t B, int32_t* route_out) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  const char* why = "";
  if (int rc = h->tab.routes.car_routes(B, route_out, &why)) return fail(rc, why);
  return MPMPC_OK;
}

}  // extern "C"
