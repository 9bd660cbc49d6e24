// The footprint audit of libmpmpc.so, part of the one translation unit mpmpc_hip.hip (included there behind mpmpc_lidar.hpp):
// the kernel K0f, its launch inside mpmpc_rollout_step (aud_enqueue_step, called from mpmpc_rollout_step.hpp) and the entry
// points - mpmpc_footprint_audit (no handle, like mpmpc_lidar_scan), mpmpc_rollout_set_audit and mpmpc_rollout_audit (the
// accumulators of a handle's running rollout).  The law: footprint_core.hpp.
#pragma once

// K0f: the verdict of one car, one WAVEFRONT per car.  The window's cells are numbered row by row, the rows in the order 0,
// +1, -1, +2, -2 ... of their distance from the centre cell's row (nearest first: where there is contact, it is found in the
// first passes) and the lane runs along i inside a row, so that a wave reads consecutive bytes of a grid row (the grid is
// L2-resident: every car of a fleet reads the same few rows).  A pass takes K0F_ROWS * 64 cells: every lane first issues
// its K0F_ROWS byte loads - a lone wave per SIMD is latency-bound, so the loads of several rows are in flight together -
// and then works through them: occupancy in the car's world (the byte, else the car's discs that meet the window,
// compacted into LDS by a ballot; their order does not matter to an OR), g of the cell (fp_cell_g), a running minimum per
// lane.  The one shortcut: when a ballot finds a lane with g == 0 after a pass, the answer is (1, 0.0) and the wave stops,
// uniformly.  At the end a 64-lane butterfly over the 64-bit value gives the minimum (the minimum of doubles is order-free:
// footprint_core.hpp) and lane 0 writes the results with ordinary stores.
// alive != nullptr (the rollout): only cars with alive == 1 are audited, the others keep what they have.  cs != nullptr:
// the rollout's accumulators take step k's verdict (fp_accumulate), and in mode FP_MODE_STOP a car in contact ends with
// alive = FP_ALIVE_CONTACT.  off == nullptr: no discs (the base map).
// Every index is bounded: the window is clipped to the grid, R to FP_MAX_REACH_CELLS and a car's disc count to
// COR_MAX_DISCS (the host refuses more of either); the trip count is at most 513^2 / (64 K0F_ROWS) + 1 passes.
// LDS: 0.8 KB; no scratch, no atomics.
// WALLS: the car's walls whose box meets the window are compacted into LDS like the discs (headers, 384 B) and a cell is
// occupied as wall_core.hpp says (grid, discs, walls); without walls the kernel is the instantiation <false>, the code it
// always was.
constexpr int K0F_ROWS = 4;
template <bool WALLS>
__global__ __launch_bounds__(64) void mpmpc_footprint_kernel(MapView map, int B, const double* __restrict__ pose,
                                                             const int* __restrict__ off, const int* __restrict__ discs,
                                                             double length, double width, double reach_m, int R, int mode, int k,
                                                             int* __restrict__ alive, int* __restrict__ contact_out,
                                                             double* __restrict__ clearance_out, int* __restrict__ cs,
                                                             int* __restrict__ first, double* __restrict__ min_clr,
                                                             int* __restrict__ min_step, WallView wv) {
  __shared__ int s_whdr[WALLS ? WALL_HDR * COR_MAX_WALLS : 1];
  __shared__ int s_disc[3 * COR_MAX_DISCS];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;                                   // (uniform)
  if (alive && alive[b] != 1) return;                   // (uniform)
  R = R > FP_MAX_REACH_CELLS ? FP_MAX_REACH_CELLS : (R < 0 ? 0 : R);
  const double x = pose[3L * b], y = pose[3L * b + 1], psi = pose[3L * b + 2];
  int cx = 0, cy = 0;
  const bool valid = lid_sensor_cell(map, x, y, psi, &cx, &cy);      // (uniform)
  int contact = 0;
  double clearance = __builtin_nan("");
  if (valid) {
    const FpCar car = fp_car(x, y, psi, length, width);
    const int i0 = cx - R < 0 ? 0 : cx - R, i1 = cx + R > map.width - 1 ? map.width - 1 : cx + R;
    const int j0 = cy - R < 0 ? 0 : cy - R, j1 = cy + R > map.height - 1 ? map.height - 1 : cy + R;
    int nd = 0;
    if (off) {
      const int d0 = off[b];
      int n = off[b + 1] - d0;
      n = n > COR_MAX_DISCS ? COR_MAX_DISCS : n;        // (the host refuses more)
      int d[3] = {0, 0, 0};
      bool meets = false;
      if (lane < n) {
        const int* p = discs + 3L * (d0 + lane);
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
        const int box[5] = {0, i0, j0, i1, j1};
        meets = d[2] > 0 && cor_disc_meets_box(d, box);
      }
      const unsigned long long m = __ballot(meets);
      if (meets) {
        const int q = __popcll(m & ((1ull << lane) - 1ull));
        s_disc[3 * q] = d[0]; s_disc[3 * q + 1] = d[1]; s_disc[3 * q + 2] = d[2];
      }
      nd = __popcll(m);
    }
    int nw = 0;
    if (WALLS && wv.off) {
      const int w0 = wv.off[b];
      int n = wv.off[b + 1] - w0;
      n = n > COR_MAX_WALLS ? COR_MAX_WALLS : n;        // (the host refuses more)
      bool meets = false;
      const int* hd = wv.hdr + (long)WALL_HDR * (w0 + (lane < n ? lane : 0));
      if (lane < n) {
        const int box[5] = {0, i0, j0, i1, j1};
        meets = wall_meets_box(hd, box);
      }
      const unsigned long long m = __ballot(meets);
      if (meets) {
        const int q = __popcll(m & ((1ull << lane) - 1ull));
        for (int e = 0; e < WALL_HDR; ++e) s_whdr[WALL_HDR * q + e] = hd[e];
      }
      nw = __popcll(m);
    }
    __syncthreads();
    const int cols = i1 - i0 + 1;
    const int cells = cols > 0 && j0 <= j1 ? cols * (2 * R + 1) : 0;      // at most 513^2
    double best = FP_NONE;
    for (int base = 0; base < cells; base += 64 * K0F_ROWS) {             // (uniform)
      int ci[K0F_ROWS], cj[K0F_ROWS];
      signed char free_[K0F_ROWS];
      bool on[K0F_ROWS];
#pragma unroll
      for (int q = 0; q < K0F_ROWS; ++q) {      // (no branch: every lane loads a byte of the clipped window, used or not)
        const int t = base + 64 * q + lane;
        const int tc = t < cells ? t : cells - 1;
        const int r = tc / cols;
        const int dj = (r & 1) ? (r + 1) / 2 : -(r / 2);
        ci[q] = i0 + (tc - r * cols);
        cj[q] = cy + dj;
        const int jc = cj[q] < j0 ? j0 : (cj[q] > j1 ? j1 : cj[q]);
        on[q] = t < cells && cj[q] == jc;
        free_[q] = map.data[(long long)jc * map.width + ci[q]];
      }
      bool hit = false;
#pragma unroll
      for (int q = 0; q < K0F_ROWS; ++q) {
        if (!on[q]) continue;
        bool occ = free_[q] == 0;
        for (int e = 0; e < nd && !occ; ++e) occ = cor_in_disc(ci[q], cj[q], s_disc + 3 * e);
        if (WALLS)
          for (int e = 0; e < nw && !occ; ++e) occ = wall_on(ci[q], cj[q], s_whdr + WALL_HDR * e, wv.tab);
        if (!occ) continue;
        const double g = fp_cell_g(map, car, ci[q], cj[q]);
        hit = hit || g == 0.0;
        best = g < best ? g : best;
      }
      if (__ballot(hit) != 0ull) { contact = 1; break; }                   // (uniform) the one shortcut
    }
    if (contact) best = 0.0;
    for (int m = 32; m >= 1; m >>= 1) {
      const long long bits = __double_as_longlong(best);
      const int lo = __shfl_xor((int)(unsigned)(bits & 0xffffffffLL), m, 64), hi = __shfl_xor((int)(bits >> 32), m, 64);
      const double o = __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
      best = o < best ? o : best;
    }
    clearance = fp_clearance(best, reach_m);
  }
  if (lane == 0) {
    if (cs) {
      fp_accumulate(valid, contact, clearance, k, cs + b, first + b, min_clr + b, min_step + b, contact_out + b, clearance_out + b);
      if (mode == FP_MODE_STOP && contact) alive[b] = FP_ALIVE_CONTACT;
    } else {
      contact_out[b] = contact;
      clearance_out[b] = clearance;
    }
  }
}

// K0f of B cars on the stream: `walls` chooses the instantiation, `a` is the kernel's argument list (map .. wv; without walls
// wv is WALLS_NONE)
template <class... A>
static void enqueue_footprint(hipStream_t stream, int B, bool walls, A... a) {
  if (walls) hipLaunchKernelGGL(mpmpc_footprint_kernel<true>, dim3(B), dim3(64), 0, stream, a...);
  else hipLaunchKernelGGL(mpmpc_footprint_kernel<false>, dim3(B), dim3(64), 0, stream, a...);
}

// device scratch of mpmpc_footprint_audit (device_scratch.hpp)
static SpScratch g_fp_dev[SP_MAX_DEVICES];

// the accumulators at the start of a run: nothing counted, min_clearance = reach_m, the last verdict (0, NaN)
static int aud_reset(mpmpc_handle h, int B) {
  AudState& a = h->aud;
  a.B = 0;
  if (a.mode == FP_MODE_OFF || B < 1) return MPMPC_OK;
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch, nb = (size_t)B;
  if (!a.ints) HIP_TRY(alloc_all(Want{a.ints, 4 * mb}, Want{a.dbls, 2 * mb}));      // (both or neither)
  std::vector<int> iv(4 * nb, 0);
  std::vector<double> dv(2 * nb, a.reach);
  for (size_t i = 0; i < nb; ++i) {
    iv[nb + i] = -1;                  // first_contact
    iv[2 * nb + i] = -1;              // min_step
    dv[nb + i] = std::nan("");        // last_clearance
  }
  hipStream_t st = h->last().stream;
  for (int q = 0; q < 4; ++q) HIP_TRY(hipMemcpyAsync(a.ints + q * mb, iv.data() + q * nb, sizeof(int) * nb, hipMemcpyHostToDevice, st));
  for (int q = 0; q < 2; ++q) HIP_TRY(hipMemcpyAsync(a.dbls + q * mb, dv.data() + q * nb, sizeof(double) * nb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));      // (iv and dv leave scope)
  a.B = B;
  return MPMPC_OK;
}

// what mpmpc_rollout_step asks before it enqueues anything: can step(s) of B cars be audited?
static int aud_check_step(mpmpc_handle h, int B) {
  AudState& a = h->aud;
  if (a.mode == FP_MODE_OFF) return MPMPC_OK;
  if (!h->cor.map) return fail(MPMPC_E_STATE, "the audit needs mpmpc_set_map first");
  if (a.B != B) return fail(MPMPC_E_STATE, "mpmpc_rollout_set_audit was set up for another number of cars");
  const char* why = "";
  if (fp_check_reach(a.length, a.width, a.reach, h->cor.map_res, &a.R, &why)) return fail(MPMPC_E_ARG, why);
  return MPMPC_OK;
}

// K0f of rollout step k on the slot's stream (behind K0m, in front of K0c: the step's disc lists are complete)
static void aud_enqueue_step(mpmpc_handle h, Slot& sl, int B, long long k, bool per_car) {
  AudState& a = h->aud;
  const size_t mb = (size_t)h->cfg.max_batch;
  const bool discs = per_car && h->obs.obst_B > 0, walls = per_car && h->obs.wl_B > 0;
  enqueue_footprint(sl.stream, B, walls, h->cor.map_view(), B, h->ro.pose.get(), discs ? h->obs.obst_off.get() : nullptr,
                    h->obs.obst_discs.get(), a.length, a.width, a.reach, a.R, a.mode, (int)k, h->ro.alive.get(), a.ints + 3 * mb,
                    a.dbls + mb, a.ints.get(), a.ints + mb, a.dbls.get(), a.ints + 2 * mb, walls ? h->obs.wall_view() : WALLS_NONE);
}

extern "C" {

int mpmpc_footprint_audit(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                          double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                          double length, double car_width, double reach_m, int32_t* contact_out, double* clearance_out) {
  return mpmpc_footprint_audit_world(device, height, width, data, origin_x, origin_y, resolution, B, pose, offsets, discs, nullptr,
                                     nullptr, length, car_width, reach_m, contact_out, clearance_out);
}

int mpmpc_footprint_audit_world(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                                double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                                const int32_t* wall_offsets, const int32_t* walls, double length, double car_width, double reach_m,
                                int32_t* contact_out, double* clearance_out) {
  const char* why = "";
  int R = 0;
  if (fp_check_audit(height, width, data, resolution, B, pose, offsets, discs, length, car_width, reach_m, contact_out, clearance_out,
                     &R, &why))
    return fail(MPMPC_E_ARG, why);
  if (wall_offsets && wall_check_lists(B, wall_offsets, walls, width, height, &why)) return fail(MPMPC_E_ARG, why);
  if (!mov_finite(origin_x) || !mov_finite(origin_y)) return fail(MPMPC_E_ARG, "the map's origin is not finite");
  const size_t nb = (size_t)B;
  Layout L;
  const auto r_pose = L.add<double>(3 * nb), r_clr = L.add<double>(nb);
  const auto r_con = L.add<int>(nb);
  WorldBlock wd = world_block(L, height, width, data, B, offsets, discs, wall_offsets, walls);
  Scratch sc;
  if (int rc = scratch_acquire(g_fp_dev, device, L.bytes(), "footprint", &sc)) return rc;
  hipStream_t stream = sc.stream;
  char* blk = sc.blk;
  HIP_TRY(hipMemcpyAsync(r_pose.at(blk), pose, r_pose.bytes(), hipMemcpyHostToDevice, stream));
  if (int rc = wd.enqueue(blk, stream)) return rc;
  enqueue_footprint(stream, B, wall_offsets != nullptr, wd.map(blk, origin_x, origin_y, resolution), B, r_pose.at(blk), wd.offsets(blk),
                    wd.discs(blk), length, car_width, reach_m, R, FP_MODE_AUDIT, 0, nullptr, r_con.at(blk), r_clr.at(blk), nullptr,
                    nullptr, nullptr, nullptr, wd.walls.view(blk));      // (no alive, no accumulators: the verdicts alone)
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(stream, contact_out, r_con.at(blk), nb));
  HIP_TRY(pull(stream, clearance_out, r_clr.at(blk), nb));
  HIP_TRY(hipStreamSynchronize(stream));
  return wd.verdict();
}

int mpmpc_rollout_set_audit(mpmpc_handle h, int32_t mode, double length, double car_width, double reach_m) {
  if (!h) return fail(MPMPC_E_ARG, "handle is NULL");
  if (mode < FP_MODE_OFF || mode > FP_MODE_STOP) return fail(MPMPC_E_ARG, "mode must be 0 (off), 1 (audit) or 2 (audit and stop on contact)");
  const char* why = "";
  if (mode != FP_MODE_OFF) {
    int R = 0;
    if (fp_check_car(length, car_width, reach_m, &why)) return fail(MPMPC_E_ARG, why);
    if (h->cor.map && fp_check_reach(length, car_width, reach_m, h->cor.map_res, &R, &why)) return fail(MPMPC_E_ARG, why);
  }
  if (int rc = enter(h)) return rc;
  AudState& a = h->aud;
  a.mode = mode;
  a.length = length; a.width = car_width; a.reach = reach_m;
  return aud_reset(h, h->ro.valid ? h->ro.B : 0);      // (a run in progress is audited from here on; else mpmpc_rollout_init resets)
}

int mpmpc_rollout_audit(mpmpc_handle h, int32_t B, int32_t* contact_steps, int32_t* first_contact, double* min_clearance,
                        int32_t* min_step, int32_t* last_contact, double* last_clearance) {
  if (int rc = enter(h)) return rc;
  AudState& a = h->aud;
  if (a.mode == FP_MODE_OFF) return fail(MPMPC_E_STATE, "the audit is off (mpmpc_rollout_set_audit)");
  if (B < 1 || B != a.B) return fail(MPMPC_E_STATE, "mpmpc_rollout_set_audit was set up for another number of cars");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch, nb = (size_t)B;
  hipStream_t st = h->last().stream;
  HIP_TRY(pull(st, contact_steps, a.ints, nb));
  HIP_TRY(pull(st, first_contact, a.ints + mb, nb));
  HIP_TRY(pull(st, min_step, a.ints + 2 * mb, nb));
  HIP_TRY(pull(st, last_contact, a.ints + 3 * mb, nb));
  HIP_TRY(pull(st, min_clearance, a.dbls, nb));
  HIP_TRY(pull(st, last_clearance, a.dbls + mb, nb));
  HIP_TRY(hipStreamSynchronize(st));
  return MPMPC_OK;
}

}  // extern "C"
