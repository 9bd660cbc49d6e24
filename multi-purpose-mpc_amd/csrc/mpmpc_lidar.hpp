// The lidar of libmpmpc.so, part of the one translation unit mpmpc_hip.hip (included there behind mpmpc_closed_loop.hpp): the
// kernel K0l and its two entry points - mpmpc_lidar_scan (no handle, like mpmpc_speed_profile) and mpmpc_rollout_scan (the
// cars of a handle's running rollout in the worlds of its last step).  The law: lidar_core.hpp.
#pragma once

// K0l: one scan per car, one WORKGROUP of 256 lanes per car.  best[n_beams] (int32 d2, LID_NONE = no hit) and a copy of
// angles[] live in LDS (8 + 16 KB at LID_MAX_BEAMS) beside the car's discs that meet the window (compacted by an LDS
// counter; their order does not matter to an OR).  The window is walked in passes of K0L_PASS cells, a row at a time,
// lane along i, so that a wave reads consecutive bytes of a grid row (the grid is L2-resident: every car of a fleet
// reads the same few rows), and the rows in the order 0, +1, -1, +2, -2 ... of their distance from the sensor's: along
// every beam that is near to far.  A pass has two halves with a barrier between them:
//   sift   per cell the integer work - occupancy, d2, the range test - and then the shortcut: one atan2 gives an enclosure
//          of the cell's interval (lid_cell_enclosure), and a cell whose enclosure covers no beam that could still take
//          its d2 is done - behind a wall's front row that is most of the wall.  What is left goes into a queue in LDS.
//   scan   the queued cells, one per lane and the lanes dense: the nine FP64 atan2 of the cell's interval, its beams
//          found in the table itself (a binary search for the first angle >= mn, then a walk while angle <= mx:
//          comparisons against the bits the host passed, never arithmetic on the spacing), LDS atomicMin.
// The queue is what keeps the nine atan2 off the waves that have one open cell among 64 (without it the shortcut saved
// a quarter of the time, not most of it).  best[] only ever decreases, so a stale read can only queue a cell in vain; the
// minimum is order-free (lidar_core.hpp), so no output bit depends on the order of the rows, of the queue, or on the
// shortcut.  A pose with a NaN or a far-off sensor (lid_sensor_cell) gives a NaN row.
// off == nullptr: no discs (the base map).  Every index is bounded: the window is clipped to the grid, a car's disc
// count to COR_MAX_DISCS, the queue to the cells of a pass, n_beams to LID_MAX_BEAMS by the host.
constexpr int K0L_THREADS = 256;
// WALLS: the car's walls whose box meets the window are staged in LDS beside the discs (headers, 384 B) and a cell is
// occupied as wall_core.hpp says (grid, discs, walls); without walls the kernel is the instantiation <false>, the code it
// always was.
constexpr int K0L_PASS = 1024;      // cells per pass = the queue's capacity
// ONE BODY for K0l and for K0s (mpmpc_perception.hpp), which marks what the scan saw: PER 0 is K0l - the code it always was,
// `pa` unused -, PER 1 a scan that also returns the seen masks, PER 2 the perception of a rollout step.  The law of the
// marking: perception_core.hpp.  K0s's two further phases:
//   mark   behind the scan's last barrier best[] is final.  The staged discs and walls keep their SLOT INDEX (s_dslot / s_wslot:
//          the compaction drops the order); for each, the lanes stride over the cells of its box clipped to the window: the
//          integer tests first (cor_in_disc / wall_on, the range), then the enclosure as a filter (no beam in it with best == d2:
//          done), then the exact interval; a cell that owns a beam sets the slot's bit by an LDS atomicOr (two words of discs,
//          one of walls).  A slot whose bit is set is left at once - the OR is order-free.
//   know   (PER 2) lanes 0 .. 63 take the car's disc slots, lanes 64 .. 79 its wall slots: first_seen / last_seen, KNOWN, and
//          the car's perceived discs and wall headers, which K0c reads in place of the true ones.
// A car that does not scan (PER 2: alive != 1 as the step finds it; any PER: a NaN row) sees nothing and still runs `know`.
// K0s's memory is ONE block of ints, `cars` cars wide, its arrays back to back (two pointers in the kernel's arguments where
// eleven made the compiler reserve a stack): PER 1 the seen masks - discs [cars][2] (bit q of the 64: slot q), walls [cars] -,
// PER 2 the arrays below, K0S_* = the array's offset in ints per car.
constexpr int K0S_DISC_FIRST = 0, K0S_DISC_LAST = K0S_DISC_FIRST + COR_MAX_DISCS;       // [cars][COR_MAX_DISCS] each
constexpr int K0S_WALL_FIRST = K0S_DISC_LAST + COR_MAX_DISCS, K0S_WALL_LAST = K0S_WALL_FIRST + COR_MAX_WALLS;      // [cars][COR_MAX_WALLS] each
constexpr int K0S_DISC_KNOWN = K0S_WALL_LAST + COR_MAX_WALLS, K0S_WALL_KNOWN = K0S_DISC_KNOWN + 2;      // [cars][2], [cars]
constexpr int K0S_COUNTS = K0S_WALL_KNOWN + 1;      // [cars][2]: static discs, movers of the car (the slots behind them are traffic)
constexpr int K0S_DISCS = K0S_COUNTS + 2;           // the perceived discs: the layout of `discs` (at most [cars][COR_MAX_DISCS][3])
constexpr int K0S_WHDR = K0S_DISCS + 3 * COR_MAX_DISCS;      // the perceived wall headers: the layout of wv.hdr
constexpr int K0S_INTS = K0S_WHDR + WALL_HDR * COR_MAX_WALLS;
struct K0sArgs {
  const int* alive;      // PER 2
  int* mem;
  int cars;
  int k, hold;           // PER 2
};
template <bool WALLS, int PER>
__device__ __forceinline__ void k0l_scan_car(const MapView& map, int B, const double* __restrict__ pose, const int* __restrict__ off,
                                             const int* __restrict__ discs, int n_beams, const double* __restrict__ angles,
                                             double range_m, double* __restrict__ ranges, const WallView& wv, const K0sArgs& pa) {
  __shared__ int s_whdr[WALLS ? WALL_HDR * COR_MAX_WALLS : 1];
  __shared__ int s_nw;
  __shared__ double s_ang[LID_MAX_BEAMS];
  __shared__ int s_best[LID_MAX_BEAMS];
  __shared__ int s_disc[3 * COR_MAX_DISCS];
  __shared__ int s_nd;
  __shared__ int s_queue[K0L_PASS];      // (di + 2048) | (dj + 2048) << 16: |di|, |dj| <= LID_MAX_RANGE_CELLS
  __shared__ int s_nq;
  __shared__ int s_dslot[PER ? COR_MAX_DISCS : 1], s_wslot[PER ? COR_MAX_WALLS : 1];      // K0s: the staged primitives' slots
  __shared__ unsigned s_seen[3], s_known[3];      // K0s: discs 0 .. 31, discs 32 .. 63, walls
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B || n_beams > LID_MAX_BEAMS) return;      // (uniform)
  double* out = ranges + (long)b * n_beams;
  const double x = pose[3L * b], y = pose[3L * b + 1], psi = pose[3L * b + 2];
  int cx = 0, cy = 0;
  bool scans = PER != 2 || pa.alive[b] == 1;      // (uniform)
  if (PER && tid < 3) { s_seen[tid] = 0u; s_known[tid] = 0u; }      // (the scan's first barrier, or `know`'s, orders these)
  if (scans && !lid_sensor_cell(map, x, y, psi, &cx, &cy)) {      // (uniform)
    if (PER == 0 || ranges)
      for (int k = tid; k < n_beams; k += K0L_THREADS) out[k] = __builtin_nan("");
    if (PER == 0) return;
    scans = false;
  }
  if (PER == 0 || scans) {
  const LidWindow w = lid_window(map, cx, cy, range_m);
  for (int k = tid; k < n_beams; k += K0L_THREADS) {
    s_ang[k] = angles[k];
    s_best[k] = LID_NONE;
  }
  if (tid == 0) { s_nd = 0; s_nq = 0; s_nw = 0; }
  __syncthreads();
  if (WALLS && wv.off) {
    const int w0 = wv.off[b];
    int n = wv.off[b + 1] - w0;
    n = n > COR_MAX_WALLS ? COR_MAX_WALLS : n;      // (the host refuses more)
    if (tid < n) {
      const int* hd = wv.hdr + (long)WALL_HDR * (w0 + tid);
      const int box[5] = {0, w.i0, w.j0, w.i1, w.j1};
      if (wall_meets_box(hd, box)) {
        const int q = atomicAdd(&s_nw, 1);
        for (int e = 0; e < WALL_HDR; ++e) s_whdr[WALL_HDR * q + e] = hd[e];
        if (PER) s_wslot[q] = tid;
      }
    }
  }
  if (off) {
    const int d0 = off[b];
    int nd = off[b + 1] - d0;
    nd = nd > COR_MAX_DISCS ? COR_MAX_DISCS : nd;      // (the host refuses more)
    if (tid < nd) {
      const int* d = discs + 3L * (d0 + tid);
      const int box[5] = {0, w.i0, w.j0, w.i1, w.j1};
      if (d[2] > 0 && cor_disc_meets_box(d, box)) {
        const int q = atomicAdd(&s_nd, 1);
        s_disc[3 * q] = d[0]; s_disc[3 * q + 1] = d[1]; s_disc[3 * q + 2] = d[2];
        if (PER) s_dslot[q] = tid;
      }
    }
  }
  __syncthreads();
  const int nd = s_nd, nw = WALLS ? s_nw : 0;
  auto disc = [&](int q) { return (const int*)(s_disc + 3 * q); };
  auto whdr = [&](int q) { return (const int*)(s_whdr + WALL_HDR * q); };
  const int cols = w.i1 - w.i0 + 1;
  const int cells = cols > 0 && w.j0 <= w.j1 ? cols * (2 * w.R + 1) : 0;      // at most 4097^2
  for (int base = 0; base < cells; base += K0L_PASS) {      // (uniform)
    const int end = base + K0L_PASS < cells ? base + K0L_PASS : cells;
    for (int t = base + tid; t < end; t += K0L_THREADS) {
      const int r = t / cols;
      const int dj = (r & 1) ? (r + 1) / 2 : -(r / 2);
      const int i = w.i0 + (t - r * cols), j = cy + dj;
      if (j < w.j0 || j > w.j1) continue;
      if (!(WALLS ? wall_lid_occupied(map, i, j, nd, disc, nw, whdr, wv.tab) : lid_occupied(map, i, j, nd, disc))) continue;
      int d2;
      if (!lid_in_range(i - cx, dj, w.lim, &d2)) continue;
      double lo, hi;
      if (lid_cell_enclosure(i - cx, dj, d2, psi, &lo, &hi)) {
        bool open = false;
        for (int k = lid_first_beam(s_ang, n_beams, lo); k < n_beams && s_ang[k] <= hi; ++k) open = open || d2 < s_best[k];
        if (!open) continue;
      }
      s_queue[atomicAdd(&s_nq, 1)] = (i - cx + LID_MAX_RANGE_CELLS) | ((dj + LID_MAX_RANGE_CELLS) << 16);
    }
    __syncthreads();
    const int nq = s_nq;
    for (int c = tid; c < nq; c += K0L_THREADS) {
      const int di = (s_queue[c] & 0xffff) - LID_MAX_RANGE_CELLS, dj = (s_queue[c] >> 16) - LID_MAX_RANGE_CELLS;
      const int d2 = di * di + dj * dj;
      double mn, mx;
      if (!lid_cell_interval(di, dj, psi, &mn, &mx)) continue;
      for (int k = lid_first_beam(s_ang, n_beams, mn); k < n_beams && s_ang[k] <= mx; ++k)
        if (d2 < s_best[k]) atomicMin(&s_best[k], d2);
    }
    __syncthreads();
    if (tid == 0) s_nq = 0;      // (every lane has read nq; the barrier below keeps the next sift's appends behind this)
    __syncthreads();
  }
  __syncthreads();
  if (PER == 0 || ranges)
    for (int k = tid; k < n_beams; k += K0L_THREADS) out[k] = lid_range(s_best[k], map.res, range_m);
  if (PER) {      // mark: best[] is final, nothing below writes it
    for (int q = 0; q < nd; ++q) {      // (uniform)
      const int* d = disc(q);
      const int slot = s_dslot[q] & (COR_MAX_DISCS - 1);
      const int x0 = d[0] - d[2] < w.i0 ? w.i0 : d[0] - d[2], x1 = d[0] + d[2] - 1 > w.i1 ? w.i1 : d[0] + d[2] - 1;
      const int y0 = d[1] - d[2] < w.j0 ? w.j0 : d[1] - d[2], y1 = d[1] + d[2] - 1 > w.j1 ? w.j1 : d[1] + d[2] - 1;
      const int bc = x1 - x0 + 1, n = bc > 0 && y1 >= y0 ? bc * (y1 - y0 + 1) : 0;      // (at most 4097^2)
      for (int t = tid; t < n; t += K0L_THREADS) {
        if ((s_seen[slot >> 5] >> (slot & 31)) & 1u) break;
        const int r = t / bc, i = x0 + (t - r * bc), j = y0 + r;
        int d2;
        if (!cor_in_disc(i, j, d) || !lid_in_range(i - cx, j - cy, w.lim, &d2)) continue;
        if (!per_cell_may_own(i - cx, j - cy, d2, psi, s_ang, n_beams, s_best)) continue;
        if (per_cell_owns_beam(i - cx, j - cy, d2, psi, s_ang, n_beams, s_best)) atomicOr(&s_seen[slot >> 5], 1u << (slot & 31));
      }
    }
    for (int q = 0; q < nw; ++q) {      // (uniform)
      const int* hd = whdr(q);
      const int slot = s_wslot[q] & (COR_MAX_WALLS - 1);
      const int x0 = hd[0] < w.i0 ? w.i0 : hd[0], x1 = hd[2] > w.i1 ? w.i1 : hd[2];
      const int y0 = hd[1] < w.j0 ? w.j0 : hd[1], y1 = hd[3] > w.j1 ? w.j1 : hd[3];
      const int bc = x1 - x0 + 1, n = bc > 0 && y1 >= y0 ? bc * (y1 - y0 + 1) : 0;
      for (int t = tid; t < n; t += K0L_THREADS) {
        if ((s_seen[2] >> slot) & 1u) break;
        const int r = t / bc, i = x0 + (t - r * bc), j = y0 + r;
        int d2;
        if (!wall_on(i, j, hd, wv.tab) || !lid_in_range(i - cx, j - cy, w.lim, &d2)) continue;
        if (!per_cell_may_own(i - cx, j - cy, d2, psi, s_ang, n_beams, s_best)) continue;
        if (per_cell_owns_beam(i - cx, j - cy, d2, psi, s_ang, n_beams, s_best)) atomicOr(&s_seen[2], 1u << slot);
      }
    }
  }
  }
  if (PER == 0) return;
  __syncthreads();
  if (PER == 1 && tid == 0) {
    pa.mem[2L * b] = (int)s_seen[0]; pa.mem[2L * b + 1] = (int)s_seen[1];
    pa.mem[2L * pa.cars + b] = (int)s_seen[2];
  }
  if (PER == 2) {      // know
    auto arr = [&](int a) { return pa.mem + (long)a * pa.cars; };
    if (tid < COR_MAX_DISCS) {
      const int d0 = off ? off[b] : 0;
      int n = off ? off[b + 1] - d0 : 0;
      n = n > COR_MAX_DISCS ? COR_MAX_DISCS : n;
      if (tid < n) {
        const long e = (long)COR_MAX_DISCS * b + tid;
        int first = arr(K0S_DISC_FIRST)[e], last = arr(K0S_DISC_LAST)[e];
        per_mark(((s_seen[tid >> 5] >> (tid & 31)) & 1u) != 0, pa.k, &first, &last);
        arr(K0S_DISC_FIRST)[e] = first; arr(K0S_DISC_LAST)[e] = last;
        const bool known = per_known(per_disc_kind(tid, arr(K0S_COUNTS)[2L * b], arr(K0S_COUNTS)[2L * b + 1]), last, pa.k, pa.hold);
        per_disc(known, discs + 3L * (d0 + tid), arr(K0S_DISCS) + 3L * (d0 + tid));
        if (known) atomicOr(&s_known[tid >> 5], 1u << (tid & 31));
      }
    } else if (WALLS && tid < COR_MAX_DISCS + COR_MAX_WALLS && wv.off) {
      const int q = tid - COR_MAX_DISCS, w0 = wv.off[b];
      int n = wv.off[b + 1] - w0;
      n = n > COR_MAX_WALLS ? COR_MAX_WALLS : n;
      if (q < n) {
        const long e = (long)COR_MAX_WALLS * b + q;
        int first = arr(K0S_WALL_FIRST)[e], last = arr(K0S_WALL_LAST)[e];
        per_mark(((s_seen[2] >> q) & 1u) != 0, pa.k, &first, &last);
        arr(K0S_WALL_FIRST)[e] = first; arr(K0S_WALL_LAST)[e] = last;
        const bool known = per_known(PER_WALL, last, pa.k, pa.hold);
        per_wall(known, wv.hdr + (long)WALL_HDR * (w0 + q), arr(K0S_WHDR) + (long)WALL_HDR * (w0 + q));
        if (known) atomicOr(&s_known[2], 1u << q);
      }
    }
    __syncthreads();
    if (tid == 0) {
      arr(K0S_DISC_KNOWN)[2L * b] = (int)s_known[0]; arr(K0S_DISC_KNOWN)[2L * b + 1] = (int)s_known[1];
      arr(K0S_WALL_KNOWN)[b] = (int)s_known[2];
    }
  }
}

template <bool WALLS>
__global__ __launch_bounds__(K0L_THREADS) void mpmpc_lidar_scan_kernel(MapView map, int B, const double* __restrict__ pose,
                                                                       const int* __restrict__ off,
                                                                       const int* __restrict__ discs, int n_beams,
                                                                       const double* __restrict__ angles, double range_m,
                                                                       double* __restrict__ ranges, WallView wv) {
  k0l_scan_car<WALLS, 0>(map, B, pose, off, discs, n_beams, angles, range_m, ranges, wv, K0sArgs{});
}

// K0l of a localising rollout step (mpmpc_rollout_step.hpp): the same scan, of the running cars alone.  A car with alive != 1
// keeps the ranges of its last scan - those K3l matched, the hits noisy -, as K3l keeps everything else of it.
template <bool WALLS>
__global__ __launch_bounds__(K0L_THREADS) void mpmpc_lidar_scan_running_kernel(MapView map, int B, const double* __restrict__ pose,
                                                                               const int* __restrict__ alive,
                                                                               const int* __restrict__ off,
                                                                               const int* __restrict__ discs, int n_beams,
                                                                               const double* __restrict__ angles, double range_m,
                                                                               double* __restrict__ ranges, WallView wv) {
  if ((int)blockIdx.x < B && alive[blockIdx.x] != 1) return;      // (uniform, in front of the scan's first barrier)
  k0l_scan_car<WALLS, 0>(map, B, pose, off, discs, n_beams, angles, range_m, ranges, wv, K0sArgs{});
}

// K0l of B cars on the stream: `walls` chooses the instantiation, `a` is the kernel's argument list (map .. wv;
// without walls wv is a null view)
template <class... A>
static void enqueue_lidar_scan(hipStream_t stream, int B, bool walls, A... a) {
  if (walls) hipLaunchKernelGGL(mpmpc_lidar_scan_kernel<true>, dim3(B), dim3(K0L_THREADS), 0, stream, a...);
  else hipLaunchKernelGGL(mpmpc_lidar_scan_kernel<false>, dim3(B), dim3(K0L_THREADS), 0, stream, a...);
}

// device scratch of mpmpc_lidar_scan (device_scratch.hpp)
static SpScratch g_lid_dev[SP_MAX_DEVICES];

extern "C" {

int mpmpc_lidar_scan(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                     double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                     int32_t n_beams, const double* angles, double range_m, double* ranges_out) {
  return mpmpc_lidar_scan_world(device, height, width, data, origin_x, origin_y, resolution, B, pose, offsets, discs, nullptr, nullptr,
                                n_beams, angles, range_m, ranges_out);
}

int mpmpc_lidar_scan_world(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                           double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                           const int32_t* wall_offsets, const int32_t* walls, int32_t n_beams, const double* angles,
                           double range_m, double* ranges_out) {
  const char* why = "";
  if (lid_check_scan(height, width, data, resolution, B, pose, offsets, discs, n_beams, angles, range_m, ranges_out, &why))
    return fail(MPMPC_E_ARG, why);
  if (wall_offsets && wall_check_lists(B, wall_offsets, walls, width, height, &why)) return fail(MPMPC_E_ARG, why);
  if (!mov_finite(origin_x) || !mov_finite(origin_y)) return fail(MPMPC_E_ARG, "the map's origin is not finite");
  const size_t nb = (size_t)B;
  Layout L;
  const auto r_pose = L.add<double>(3 * nb), r_ang = L.add<double>((size_t)n_beams), r_out = L.add<double>(nb * (size_t)n_beams);
  WorldBlock wd = world_block(L, height, width, data, B, offsets, discs, wall_offsets, walls);
  Scratch sc;
  if (int rc = scratch_acquire(g_lid_dev, device, L.bytes(), "lidar", &sc)) return rc;
  hipStream_t stream = sc.stream;
  char* blk = sc.blk;
  HIP_TRY(hipMemcpyAsync(r_pose.at(blk), pose, r_pose.bytes(), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(r_ang.at(blk), angles, r_ang.bytes(), hipMemcpyHostToDevice, stream));
  if (int rc = wd.enqueue(blk, stream)) return rc;
  enqueue_lidar_scan(stream, B, wall_offsets != nullptr, wd.map(blk, origin_x, origin_y, resolution), B, r_pose.at(blk), wd.offsets(blk),
                     wd.discs(blk), n_beams, r_ang.at(blk), range_m, r_out.at(blk), wd.walls.view(blk));
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(stream, ranges_out, r_out.at(blk), r_out.count));
  HIP_TRY(hipStreamSynchronize(stream));
  return wd.verdict();
}

int mpmpc_rollout_scan(mpmpc_handle h, int32_t B, int32_t n_beams, const double* angles, double range_m, double* ranges_out) {
  if (int rc = enter(h, ranges_out)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B, "the rollout's state was overwritten by an upload / solve / assemble on this handle: "
                              "call mpmpc_rollout_init again")) return rc;
  if (B != h->ro.B) return fail(MPMPC_E_STATE, "the rollout was set up for another number of cars");
  if (!h->cor.map) return fail(MPMPC_E_STATE, "needs mpmpc_set_map first");
  const char* why = "";
  if (lid_check_beams(n_beams, angles, range_m, h->cor.map_res, &why)) return fail(MPMPC_E_ARG, why);
  const bool per_car = h->obs.world_B() > 0, discs = h->obs.obst_B > 0, walls = h->obs.wl_B > 0;
  if (per_car && (!h->obs.car_rows || !h->obs.discs_live || h->obs.world_B() != B))
    return fail(MPMPC_E_STATE, "per-car obstacles / movers / traffic are set, but no rollout step of B cars has used them yet, or they were "
                               "set anew since the last step: the cars' worlds are those of a step (mpmpc_rollout_step)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n_out = (size_t)B * (size_t)n_beams;
  if (h->lid.angles.count() < (size_t)n_beams) HIP_TRY(h->lid.angles.alloc((size_t)LID_MAX_BEAMS));
  if (h->lid.ranges.count() < n_out) HIP_TRY(h->lid.ranges.alloc(n_out));
  HIP_TRY(hipMemcpyAsync(h->lid.angles, angles, sizeof(double) * (size_t)n_beams, hipMemcpyHostToDevice, sl.stream));
  enqueue_lidar_scan(sl.stream, B, walls, h->cor.map_view(), B, h->ro.pose.get(), discs ? h->obs.obst_off.get() : nullptr,
                     h->obs.obst_discs.get(), n_beams, h->lid.angles.get(), range_m, h->lid.ranges.get(),
                     h->obs.wall_view());
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(sl.stream, ranges_out, h->lid.ranges, n_out));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

}  // extern "C"

