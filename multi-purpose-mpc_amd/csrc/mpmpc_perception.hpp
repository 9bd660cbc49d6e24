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

// K0s of B cars on the stream: `walls` chooses the instantiation, `a` is the kernel's argument list (map .. pa;
// without walls wv is a null view)
template <int PER, class... A>
static void enqueue_perception(hipStream_t stream, int B, bool walls, A... a) {
  if (walls) hipLaunchKernelGGL((mpmpc_perception_kernel<true, PER>), dim3(B), dim3(K0L_THREADS), 0, stream, a...);
  else hipLaunchKernelGGL((mpmpc_perception_kernel<false, PER>), dim3(B), dim3(K0L_THREADS), 0, stream, a...);
}

// device scratch of mpmpc_perception_scan (device_scratch.hpp)
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
  const bool discs = h->obs.obst_B > 0, walls = h->obs.wl_B > 0;
  const K0sArgs pa{h->ro.alive.get(), p.mem.get(), h->cfg.max_batch, (int)k, p.hold};
  enqueue_perception<2>(sl.stream, B, walls, h->cor.map_view(), B, h->ro.pose.get(), discs ? h->obs.obst_off.get() : nullptr,
                        h->obs.obst_discs.get(), p.n_beams, p.angles.get(), p.range, nullptr, h->obs.wall_view(), pa);
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
  const size_t nb = (size_t)B;
  Layout L;
  const auto r_pose = L.add<double>(3 * nb), r_ang = L.add<double>((size_t)n_beams), r_out = L.add<double>(nb * (size_t)n_beams);
  // K0s's memory is ONE region (K0sArgs::mem): the discs' masks [B][2], the walls' [B] right behind them
  const auto r_seen = L.add<int>(3 * nb), r_dseen = r_seen.part(0, 2 * nb), r_wseen = r_seen.part(2 * nb, nb);
  WorldBlock wd = world_block(L, height, width, data, B, offsets, discs, wall_offsets, walls);
  Scratch sc;
  if (int rc = scratch_acquire(g_per_dev, device, L.bytes(), "perception", &sc)) return rc;
  hipStream_t stream = sc.stream;
  char* blk = sc.blk;
  HIP_TRY(hipMemcpyAsync(r_pose.at(blk), pose, r_pose.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_ang.at(blk), angles, r_ang.bytes(), hipMemcpyHostToDevice, stream));
  if (int rc = wd.enqueue(blk, stream)) return rc;
  double* d_out = ranges_out ? r_out.at(blk) : nullptr;
  enqueue_perception<1>(stream, B, wall_offsets != nullptr, wd.map(blk, origin_x, origin_y, resolution), B, r_pose.at(blk),
                        wd.offsets(blk), wd.discs(blk), n_beams, r_ang.at(blk), range_m, d_out, wd.walls.view(blk),
                        K0sArgs{nullptr, r_seen.at(blk), B, 0, 0});
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(stream, ranges_out, r_out.at(blk), r_out.count));
  HIP_TRY(pull(stream, disc_seen_out, (const uint64_t*)r_dseen.at(blk), nb));      // (bit q of the 64: slot q - two ints per car)
  HIP_TRY(pull(stream, wall_seen_out, (const uint32_t*)r_wseen.at(blk), nb));
  HIP_TRY(hipStreamSynchronize(stream));
  return wd.verdict();
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
  HIP_TRY(pull(st, disc_first, mem + K0S_DISC_FIRST * mb, COR_MAX_DISCS * nb));
  HIP_TRY(pull(st, disc_last, mem + K0S_DISC_LAST * mb, COR_MAX_DISCS * nb));
  HIP_TRY(pull(st, wall_first, mem + K0S_WALL_FIRST * mb, COR_MAX_WALLS * nb));
  HIP_TRY(pull(st, wall_last, mem + K0S_WALL_LAST * mb, COR_MAX_WALLS * nb));
  HIP_TRY(pull(st, disc_known, (const uint64_t*)(mem + K0S_DISC_KNOWN * mb), nb));
  HIP_TRY(pull(st, wall_known, (const uint32_t*)(mem + K0S_WALL_KNOWN * mb), nb));
  HIP_TRY(hipStreamSynchronize(st));
  return MPMPC_OK;
}

}  // extern "C"
