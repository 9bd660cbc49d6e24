// The perception of libmpmpc.so, part of the one translation unit mpmpc_hip.hip (included there behind mpmpc_lidar.hpp): the
// kernel K0s and its entry points - mpmpc_perception_scan (no handle, like mpmpc_lidar_scan_world), mpmpc_rollout_set_perception
// and mpmpc_rollout_perception - and what mpmpc_rollout_step calls of it.  The law: perception_core.hpp.
#pragma once

// K0s: what a scan saw and what the car then knows, one WORKGROUP of 256 lanes per car.  Its scan IS K0l's (k0l_scan_car in
// mpmpc_lidar.hpp, one body: the ranges are K0l's bit for bit); the marking and the knowledge are that body's PER phases.
// PER 1: ranges (may be null) and the seen masks of B poses.  PER 2: a rollout step - no ranges, the knowledge of every car
// and its perceived lists.  Stores are ordinary vector stores; every index is bounded as K0l bounds its own, a slot index by
// COR_MAX_DISCS / COR_MAX_WALLS.
template <bool WALLS, int PER>
__global__ __launch_bounds__(K0L_THREADS) void mpmpc_perception_kernel(MapView map, int B, const double* __restrict__ pose,
                                                                       const int* __restrict__ off,
                                                                       const int* __restrict__ discs, int n_beams,
                                                                       const double* __restrict__ angles, double range_m,
                                                                       double* __restrict__ ranges, WallView wv, K0sArgs pa) {
  k0l_scan_car<WALLS, PER>(map, B, pose, off, discs, n_beams, angles, range_m, ranges, wv, pa);
}

// device scratch of mpmpc_perception_scan (SpScratch: one per device, each behind its own mutex, never freed)
static SpScratch g_per_dev[SP_MAX_DEVICES];

// mpmpc_rollout_step, before it enqueues anything: perception is on - may steps of B cars perceive?  *active: they do (a per-car
// setting is in force; else there is nothing to perceive and the step launches nothing new).  Allocates on first use and resets
// the knowledge where a reset is due.
static int per_check_step(mpmpc_handle h, int B, bool per_car, bool* active) {
  PerState& p = h->per;
  *active = false;
  if (!h->cor.map) return fail(MPMPC_E_STATE, "perception needs mpmpc_set_map first");
  const char* why = "";
  if (lid_check_beams(p.n_beams, p.host_angles.data(), p.range, h->cor.map_res, &why)) return fail(MPMPC_E_ARG, why);
  if (!per_car) return MPMPC_OK;
  const size_t mb = (size_t)h->cfg.max_batch, nb = (size_t)B;
  if (!p.mem) HIP_TRY(p.mem.alloc(K0S_INTS * mb));
  if (p.fresh) {
    hipStream_t st = h->last().stream;
    std::vector<int> counts(2 * nb, 0);
    for (size_t b = 0; b < nb; ++b) {
      if (h->obs.obst_B > 0 && h->obs.st_B > 0) counts[2 * b] = h->obs.st_off[b + 1] - h->obs.st_off[b];
      if (h->obs.obst_B > 0 && h->obs.mv_B > 0) counts[2 * b + 1] = h->obs.mv_off[b + 1] - h->obs.mv_off[b];
    }
    HIP_TRY(hipMemsetAsync(p.mem, 0xff, sizeof(int) * K0S_DISC_KNOWN * mb, st));      // first_seen, last_seen of every slot: -1
    HIP_TRY(hipMemsetAsync(p.mem + K0S_DISC_KNOWN * mb, 0, sizeof(int) * (K0S_INTS - K0S_DISC_KNOWN) * mb, st));
    HIP_TRY(hipMemcpyAsync(p.mem + K0S_COUNTS * mb, counts.data(), sizeof(int) * 2 * nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // `counts` leaves scope
    p.fresh = false;
    p.B = 0;
  }
  *active = true;
  return MPMPC_OK;
}

// K0s of rollout step k on the slot's stream (behind K0t and K0m, in front of K3a and K0c)
static void per_enqueue_step(mpmpc_handle h, Slot& sl, int B, long long k) {
  PerState& p = h->per;
  const bool discs = h->obs.obst_B > 0;
  const K0sArgs pa{h->ro.alive.get(), p.mem.get(), h->cfg.max_batch, (int)k, p.hold};
  if (h->obs.wl_B > 0)
    hipLaunchKernelGGL((mpmpc_perception_kernel<true, 2>), dim3(B), dim3(K0L_THREADS), 0, sl.stream, h->cor.map_view(), B, h->ro.pose.get(),
                       discs ? h->obs.obst_off.get() : nullptr, h->obs.obst_discs.get(), p.n_beams, p.angles.get(), p.range,
                       (double*)nullptr, h->obs.wall_view(), pa);
  else
    hipLaunchKernelGGL((mpmpc_perception_kernel<false, 2>), dim3(B), dim3(K0L_THREADS), 0, sl.stream, h->cor.map_view(), B, h->ro.pose.get(),
                       discs ? h->obs.obst_off.get() : nullptr, h->obs.obst_discs.get(), p.n_beams, p.angles.get(), p.range,
                       (double*)nullptr, WallView{nullptr, nullptr, nullptr}, pa);
}

static const int* per_plan_discs(mpmpc_handle h) { return h->per.mem + (size_t)K0S_DISCS * (size_t)h->cfg.max_batch; }
static const int* per_plan_whdr(mpmpc_handle h) { return h->per.mem + (size_t)K0S_WHDR * (size_t)h->cfg.max_batch; }

extern "C" {

int mpmpc_perception_scan(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                          double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                          const int32_t* wall_offsets, const int32_t* walls, int32_t n_beams, const double* angles, double range_m,
                          double* ranges_out, uint64_t* disc_seen_out, uint32_t* wall_seen_out) {
  const char* why = "";
  if (!disc_seen_out || !wall_seen_out) return fail(MPMPC_E_ARG, "disc_seen_out and wall_seen_out must not be NULL");
  if (lid_check_scan(height, width, data, resolution, B, pose, offsets, discs, n_beams, angles, range_m,
                     ranges_out ? ranges_out : (const double*)disc_seen_out, &why))
    return fail(MPMPC_E_ARG, why);
  if (wall_offsets && wall_check_lists(B, wall_offsets, walls, width, height, &why)) return fail(MPMPC_E_ARG, why);
  if (!mov_finite(origin_x) || !mov_finite(origin_y)) return fail(MPMPC_E_ARG, "the map's origin is not finite");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MPMPC_E_HIP, "no such HIP device");
  if (device >= SP_MAX_DEVICES) return fail(MPMPC_E_ARG, "device ordinal beyond the perception scratch table");
  HIP_TRY(hipSetDevice(device));
  const size_t nb = (size_t)B, n_disc = offsets ? (size_t)offsets[B] : 0;
  const size_t o_pose = 0, o_ang = o_pose + sizeof(double) * 3 * nb, o_out = o_ang + sizeof(double) * (size_t)n_beams,
               o_dseen = o_out + sizeof(double) * nb * (size_t)n_beams, o_wseen = o_dseen + sizeof(uint64_t) * nb,
               o_off = o_wseen + pad8(sizeof(uint32_t) * nb), o_disc = o_off + pad8(sizeof(int) * (nb + 1)),
               o_map = o_disc + pad8(sizeof(int) * 3 * n_disc), o_wall = o_map + pad8((size_t)height * width);
  WallBlock wb = wall_block(o_wall, B, wall_offsets, walls);
  const size_t need = wb.end;
  SpScratch& g = g_per_dev[device];
  std::lock_guard<std::mutex> lock(g.mu);
  if (g.bytes < need) {
    if (g.block) (void)device_free(g.block);
    g.block = nullptr; g.bytes = 0;
    HIP_TRY(device_alloc((void**)&g.block, need));
    g.bytes = need;
  }
  if (!g.stream) HIP_TRY(hipStreamCreate(&g.stream));
  hipStream_t stream = g.stream;
  char* blk = g.block;
  HIP_TRY(hipMemcpyAsync(blk + o_pose, pose, sizeof(double) * 3 * nb, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(blk + o_ang, angles, sizeof(double) * (size_t)n_beams, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(blk + o_map, data, (size_t)height * width, hipMemcpyHostToDevice, stream));
  if (offsets) HIP_TRY(hipMemcpyAsync(blk + o_off, offsets, sizeof(int) * (nb + 1), hipMemcpyHostToDevice, stream));
  if (n_disc > 0) HIP_TRY(hipMemcpyAsync(blk + o_disc, discs, sizeof(int) * 3 * n_disc, hipMemcpyHostToDevice, stream));
  if (int rc = wall_block_enqueue(blk, wb, B, wall_offsets, walls, stream)) return rc;      // K0w first, on the same stream
  const MapView mv{(const int8_t*)(blk + o_map), height, width, origin_x, origin_y, resolution};
  const K0sArgs pa{nullptr, (int*)(blk + o_dseen), B, 0, 0};      // (the walls' masks follow the discs': o_wseen = o_dseen + 8 B)
  double* d_out = ranges_out ? (double*)(blk + o_out) : nullptr;
  if (wall_offsets)
    hipLaunchKernelGGL((mpmpc_perception_kernel<true, 1>), dim3(B), dim3(K0L_THREADS), 0, stream, mv, B, (const double*)(blk + o_pose),
                       offsets ? (const int*)(blk + o_off) : nullptr, (const int*)(blk + o_disc), n_beams,
                       (const double*)(blk + o_ang), range_m, d_out, wall_block_view(blk, wb, wall_offsets), pa);
  else
    hipLaunchKernelGGL((mpmpc_perception_kernel<false, 1>), dim3(B), dim3(K0L_THREADS), 0, stream, mv, B, (const double*)(blk + o_pose),
                       offsets ? (const int*)(blk + o_off) : nullptr, (const int*)(blk + o_disc), n_beams,
                       (const double*)(blk + o_ang), range_m, d_out, WallView{nullptr, nullptr, nullptr}, pa);
  HIP_TRY(hipGetLastError());
  if (ranges_out) HIP_TRY(hipMemcpyAsync(ranges_out, blk + o_out, sizeof(double) * nb * (size_t)n_beams, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(disc_seen_out, blk + o_dseen, sizeof(uint64_t) * nb, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(wall_seen_out, blk + o_wseen, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return wall_block_verdict(wb);
}

int mpmpc_rollout_set_perception(mpmpc_handle h, int32_t n_beams, const double* angles, double range_m, int32_t hold) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  const char* why = "";
  if (angles && per_check_setting(n_beams, angles, range_m, hold, h->cor.map ? h->cor.map_res : HUGE_VAL, &why))
    return fail(MPMPC_E_ARG, why);
  if (int rc = enter(h)) return rc;
  PerState& p = h->per;
  p.forget();
  if (!angles) {
    p.n_beams = 0;
    return MPMPC_OK;
  }
  HIP_TRY(hipSetDevice(h->cfg.device));
  p.n_beams = 0;      // a failure below leaves perception off
  if (!p.angles) HIP_TRY(p.angles.alloc((size_t)LID_MAX_BEAMS));
  p.host_angles.assign(angles, angles + n_beams);
  HIP_TRY(hipMemcpyAsync(p.angles, p.host_angles.data(), sizeof(double) * (size_t)n_beams, hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  p.n_beams = n_beams;
  p.range = range_m;
  p.hold = hold;
  return MPMPC_OK;
}

int mpmpc_rollout_perception(mpmpc_handle h, int32_t B, int32_t* disc_first, int32_t* disc_last, int32_t* wall_first,
                             int32_t* wall_last, uint64_t* disc_known, uint32_t* wall_known) {
  if (int rc = enter(h)) return rc;
  PerState& p = h->per;
  if (p.n_beams == 0) return fail(MPMPC_E_STATE, "perception is off (mpmpc_rollout_set_perception)");
  if (p.fresh || p.B == 0) return fail(MPMPC_E_STATE, "no rollout step has perceived since the knowledge was reset");
  if (B != p.B || B != h->ro.B) return fail(MPMPC_E_STATE, "the rollout perceives for another number of cars");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch, nb = (size_t)B;
  hipStream_t st = h->last().stream;
  const int* mem = p.mem.get();
#define PULL(dst, src, bytes) if (dst) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st))
  PULL(disc_first, mem + K0S_DISC_FIRST * mb, sizeof(int) * COR_MAX_DISCS * nb);
  PULL(disc_last, mem + K0S_DISC_LAST * mb, sizeof(int) * COR_MAX_DISCS * nb);
  PULL(wall_first, mem + K0S_WALL_FIRST * mb, sizeof(int) * COR_MAX_WALLS * nb);
  PULL(wall_last, mem + K0S_WALL_LAST * mb, sizeof(int) * COR_MAX_WALLS * nb);
  PULL(disc_known, mem + K0S_DISC_KNOWN * mb, sizeof(uint64_t) * nb);
  PULL(wall_known, mem + K0S_WALL_KNOWN * mb, sizeof(uint32_t) * nb);
#undef PULL
  HIP_TRY(hipStreamSynchronize(st));
  return MPMPC_OK;
}

}  // extern "C"
