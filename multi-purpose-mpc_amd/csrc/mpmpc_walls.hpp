// The walls of libmpmpc.so, part of the one translation unit mpmpc_hip.hip (included there in front of mpmpc_closed_loop.hpp):
// the kernels K0w (the walls' table) and K-world (one car's world as a grid), the layout of a fleet's walls inside a scratch
// block for the entry points that need no handle, and mpmpc_world_grid.  The law: wall_core.hpp.  mpmpc_rollout_set_walls
// lives with the other per-car setters in mpmpc_closed_loop.hpp.
#pragma once

// K0w: one THREAD per wall walks its line once (cor_line_aa: a float32 recurrence, inherently serial) and fills the wall's
// slice of the table - raw [n][4] end cells, hdr [n][WALL_HDR] (the host's wall_layout: the slices are disjoint and lie inside
// the table, which is sized by the sum of the extents).  The thread owns its slice: ordinary stores, no atomics.  ok[j] = 1,
// or 0 when the line does not fit the table's form (wall_raster; the caller then refuses the walls).  Runs when walls are
// set, never per step.
__global__ __launch_bounds__(64) void mpmpc_wall_raster_kernel(int n, const int* __restrict__ raw, const int* __restrict__ hdr,
                                                               int* __restrict__ table, int* __restrict__ ok) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  int w[4], h[WALL_HDR];
  for (int e = 0; e < 4; ++e) w[e] = raw[4L * j + e];
  for (int e = 0; e < WALL_HDR; ++e) h[e] = hdr[(long)WALL_HDR * j + e];
  ok[j] = wall_raster(w, h, table) ? 1 : 0;
}

// K-world: the occupancy of ONE car's world, one thread per cell (1 free / 0 occupied, the grid's own convention), through
// wall_world_occupied - the direct pin of the predicate, and what a plot of a car's world needs.  Discs and headers in LDS.
__global__ __launch_bounds__(256) void mpmpc_world_grid_kernel(MapView map, int nd, const int* __restrict__ discs, int nw,
                                                               const int* __restrict__ hdr, const int* __restrict__ table,
                                                               int8_t* __restrict__ out) {
  __shared__ int s_disc[3 * COR_MAX_DISCS];
  __shared__ int s_whdr[WALL_HDR * COR_MAX_WALLS];
  nd = nd > COR_MAX_DISCS ? COR_MAX_DISCS : nd;      // (the host refuses more of either)
  nw = nw > COR_MAX_WALLS ? COR_MAX_WALLS : nw;
  for (int k = threadIdx.x; k < 3 * nd; k += 256) s_disc[k] = discs[k];
  for (int k = threadIdx.x; k < WALL_HDR * nw; k += 256) s_whdr[k] = hdr[k];
  __syncthreads();
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= (long long)map.height * map.width) return;
  const int y = (int)(c / map.width), x = (int)(c - (long long)y * map.width);
  const bool occ = wall_world_occupied(map, x, y, nd, [&](int q) { return (const int*)(s_disc + 3 * q); }, nw,
                                       [&](int q) { return (const int*)(s_whdr + WALL_HDR * q); }, table);
  out[c] = occ ? 0 : 1;
}

constexpr WallView WALLS_NONE{nullptr, nullptr, nullptr};      // what a kernel instantiated without WALLS is handed

// A fleet's walls inside a scratch block, for the entry points that need no handle: its five arrays, reserved in the block's
// layout (device_scratch.hpp), the caller's lists and the headers (host).  off == nullptr: no walls, and nothing is reserved.
struct WallBlock {
  const int32_t *off = nullptr, *walls = nullptr;
  size_t n = 0;
  Region<int> r_off, r_hdr, r_raw, r_tab, r_ok;
  std::vector<int32_t> hdr, ok;
  // uploads them and runs K0w on the stream, in front of the kernel that reads them; `ok` arrives with the stream's next
  // synchronisation (verdict)
  int enqueue(char* blk, hipStream_t stream) {
    if (!off) return MPMPC_OK;
    HIP_TRY(hipMemcpyAsync(r_off.at(blk), off, r_off.bytes(), hipMemcpyHostToDevice, stream));
    if (n == 0) return MPMPC_OK;
    HIP_TRY(hipMemcpyAsync(r_hdr.at(blk), hdr.data(), r_hdr.bytes(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(r_raw.at(blk), walls, r_raw.bytes(), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(mpmpc_wall_raster_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, (int)n, r_raw.at(blk),
                       r_hdr.at(blk), r_tab.at(blk), r_ok.at(blk));
    HIP_TRY(hipGetLastError());
    HIP_TRY(pull(stream, ok.data(), r_ok.at(blk), n));
    return MPMPC_OK;
  }
  WallView view(char* blk) const {
    if (!off) return WALLS_NONE;
    return WallView{r_off.at(blk), r_hdr.at(blk), r_tab.at(blk)};
  }
  int verdict() const {
    for (size_t j = 0; j < n; ++j)
      if (ok[j] != 1) return fail(MPMPC_E_ARG, "wall " + std::to_string(j) + " does not fit the wall table (csrc/wall_core.hpp, step 3)");
    return MPMPC_OK;
  }
};
static WallBlock wall_block(Layout& L, int B, const int32_t* off, const int32_t* walls) {
  WallBlock w;
  if (!off) return w;
  w.off = off; w.walls = walls;
  w.n = (size_t)off[B];
  w.hdr.assign(WALL_HDR * w.n + 1, 0);
  w.ok.assign(w.n + 1, 1);
  const size_t total = (size_t)wall_layout((long)w.n, walls, w.hdr.data());
  w.r_off = L.add<int>((size_t)B + 1);
  w.r_hdr = L.add<int>(WALL_HDR * w.n);
  w.r_raw = L.add<int>(4 * w.n);
  w.r_tab = L.add<int>(total);
  w.r_ok = L.add<int>(w.n);
  return w;
}

// The worlds of B cars inside a scratch block (mpmpc_lidar_scan_world, mpmpc_footprint_audit_world, mpmpc_perception_scan,
// mpmpc_path_build; mpmpc_world_grid with B = 1): the map, the cars' discs (off == nullptr: none) and their walls.
struct WorldBlock {
  int height = 0, width = 0;
  const int8_t* data = nullptr;
  const int32_t *off = nullptr, *disc_list = nullptr;
  Region<int8_t> r_map;
  Region<int> r_off, r_disc;
  WallBlock walls;
  int upload(char* blk, hipStream_t stream) {
    HIP_TRY(hipMemcpyAsync(r_map.at(blk), data, r_map.bytes(), hipMemcpyHostToDevice, stream));
    if (off) HIP_TRY(hipMemcpyAsync(r_off.at(blk), off, r_off.bytes(), hipMemcpyHostToDevice, stream));
    if (r_disc.count > 0) HIP_TRY(hipMemcpyAsync(r_disc.at(blk), disc_list, r_disc.bytes(), hipMemcpyHostToDevice, stream));
    return MPMPC_OK;
  }
  // everything onto the stream, K0w included: the kernel that reads the worlds comes behind
  int enqueue(char* blk, hipStream_t stream) {
    if (int rc = upload(blk, stream)) return rc;
    return walls.enqueue(blk, stream);
  }
  MapView map(char* blk, double origin_x, double origin_y, double resolution) const {
    return MapView{r_map.at(blk), height, width, origin_x, origin_y, resolution};
  }
  const int* offsets(char* blk) const { return off ? r_off.at(blk) : nullptr; }
  const int* discs(char* blk) const { return r_disc.at(blk); }
  int verdict() const { return walls.verdict(); }
};
static WorldBlock world_block(Layout& L, int height, int width, const int8_t* data, int B, const int32_t* off, const int32_t* discs,
                              const int32_t* wall_off, const int32_t* walls) {
  WorldBlock w;
  w.height = height; w.width = width; w.data = data; w.off = off; w.disc_list = discs;
  w.r_off = L.add<int>((size_t)B + 1);
  w.r_disc = L.add<int>(off ? 3 * (size_t)off[B] : 0);
  w.r_map = L.add<int8_t>((size_t)height * width);
  w.walls = wall_block(L, B, wall_off, walls);
  return w;
}

static SpScratch g_world_dev[SP_MAX_DEVICES];

extern "C" int mpmpc_world_grid(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                                double resolution, int32_t n_discs, const int32_t* discs, int32_t n_walls, const int32_t* walls,
                                int8_t* grid_out) {
  if (height < 1 || width < 1 || !(resolution > 0.0) || !mov_finite(resolution)) return fail(MPMPC_E_ARG, "map needs positive size and resolution");
  if (height > COR_MAX_SIDE || width > COR_MAX_SIDE) return fail(MPMPC_E_ARG, "map sides are limited to 65534 cells");
  if (!data || !grid_out) return fail(MPMPC_E_ARG, "data and grid_out must not be NULL");
  if (!mov_finite(origin_x) || !mov_finite(origin_y)) return fail(MPMPC_E_ARG, "the map's origin is not finite");
  if (n_discs < 0 || n_walls < 0) return fail(MPMPC_E_ARG, "n_discs and n_walls must be >= 0");
  const int32_t d_off[2] = {0, n_discs}, w_off[2] = {0, n_walls};
  const char* why = "";
  if (lid_check_discs(1, d_off, discs, width, height, &why)) return fail(MPMPC_E_ARG, why);
  if (wall_check_lists(1, w_off, walls, width, height, &why)) return fail(MPMPC_E_ARG, why);
  const size_t cells = (size_t)height * width;
  Layout L;
  WorldBlock wd = world_block(L, height, width, data, 1, d_off, discs, w_off, walls);      // one car's world: the lists of a fleet of one
  const auto r_out = L.add<int8_t>(cells);
  Scratch sc;
  if (int rc = scratch_acquire(g_world_dev, device, L.bytes(), "world", &sc)) return rc;
  if (int rc = wd.enqueue(sc.blk, sc.stream)) return rc;
  const WallView wv = wd.walls.view(sc.blk);
  hipLaunchKernelGGL(mpmpc_world_grid_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, sc.stream,
                     wd.map(sc.blk, origin_x, origin_y, resolution), n_discs, wd.discs(sc.blk), n_walls, wv.hdr, wv.tab,
                     r_out.at(sc.blk));
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(sc.stream, grid_out, r_out.at(sc.blk), cells));
  HIP_TRY(hipStreamSynchronize(sc.stream));
  return wd.verdict();
}
