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

// A fleet's walls inside a scratch block (mpmpc_lidar_scan_world, mpmpc_footprint_audit_world, mpmpc_world_grid): where its
// five arrays lie from byte `start` on, the headers (host), and the block's end.
struct WallBlock {
  size_t n = 0, total = 0;
  size_t o_off = 0, o_hdr = 0, o_raw = 0, o_tab = 0, o_ok = 0, end = 0;
  std::vector<int32_t> hdr, ok;
};
static WallBlock wall_block(size_t start, int B, const int32_t* off, const int32_t* walls) {
  WallBlock w;
  w.end = start;
  if (!off) return w;
  w.n = (size_t)off[B];
  w.hdr.assign(WALL_HDR * w.n + 1, 0);
  w.ok.assign(w.n + 1, 1);
  w.total = (size_t)wall_layout((long)w.n, walls, w.hdr.data());
  w.o_off = start;
  w.o_hdr = w.o_off + pad8(sizeof(int) * ((size_t)B + 1));
  w.o_raw = w.o_hdr + pad8(sizeof(int) * WALL_HDR * w.n);
  w.o_tab = w.o_raw + pad8(sizeof(int) * 4 * w.n);
  w.o_ok = w.o_tab + pad8(sizeof(int) * w.total);
  w.end = w.o_ok + pad8(sizeof(int) * w.n);
  return w;
}
// uploads them and runs K0w on the stream, in front of the kernel that reads them; w.ok arrives with the stream's next
// synchronisation (wall_block_verdict)
static int wall_block_enqueue(char* blk, WallBlock& w, int B, const int32_t* off, const int32_t* walls, hipStream_t stream) {
  if (!off) return MPMPC_OK;
  HIP_TRY(hipMemcpyAsync(blk + w.o_off, off, sizeof(int) * ((size_t)B + 1), hipMemcpyHostToDevice, stream));
  if (w.n == 0) return MPMPC_OK;
  HIP_TRY(hipMemcpyAsync(blk + w.o_hdr, w.hdr.data(), sizeof(int) * WALL_HDR * w.n, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(blk + w.o_raw, walls, sizeof(int) * 4 * w.n, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(mpmpc_wall_raster_kernel, dim3((unsigned)((w.n + 63) / 64)), dim3(64), 0, stream, (int)w.n, (const int*)(blk + w.o_raw),
                     (const int*)(blk + w.o_hdr), (int*)(blk + w.o_tab), (int*)(blk + w.o_ok));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(w.ok.data(), blk + w.o_ok, sizeof(int) * w.n, hipMemcpyDeviceToHost, stream));
  return MPMPC_OK;
}
static WallView wall_block_view(char* blk, const WallBlock& w, const int32_t* off) {
  if (!off) return WallView{nullptr, nullptr, nullptr};
  return WallView{(const int*)(blk + w.o_off), (const int*)(blk + w.o_hdr), (const int*)(blk + w.o_tab)};
}
static int wall_block_verdict(const WallBlock& w) {
  for (size_t j = 0; j < w.n; ++j)
    if (w.ok[j] != 1) return fail(MPMPC_E_ARG, "wall " + std::to_string(j) + " does not fit the wall table (csrc/wall_core.hpp, step 3)");
  return MPMPC_OK;
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
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MPMPC_E_HIP, "no such HIP device");
  if (device >= SP_MAX_DEVICES) return fail(MPMPC_E_ARG, "device ordinal beyond the world scratch table");
  HIP_TRY(hipSetDevice(device));
  const size_t cells = (size_t)height * width;
  const size_t o_map = 0, o_out = o_map + pad8(cells), o_disc = o_out + pad8(cells), o_wall = o_disc + pad8(sizeof(int) * 3 * (size_t)n_discs);
  WallBlock wb = wall_block(o_wall, 1, w_off, walls);
  const size_t need = wb.end + 8;
  SpScratch& g = g_world_dev[device];
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
  HIP_TRY(hipMemcpyAsync(blk + o_map, data, cells, hipMemcpyHostToDevice, stream));
  if (n_discs > 0) HIP_TRY(hipMemcpyAsync(blk + o_disc, discs, sizeof(int) * 3 * (size_t)n_discs, hipMemcpyHostToDevice, stream));
  if (int rc = wall_block_enqueue(blk, wb, 1, w_off, walls, stream)) return rc;
  const MapView mv{(const int8_t*)(blk + o_map), height, width, origin_x, origin_y, resolution};
  hipLaunchKernelGGL(mpmpc_world_grid_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, mv, n_discs,
                     (const int*)(blk + o_disc), n_walls, (const int*)(blk + wb.o_hdr), (const int*)(blk + wb.o_tab),
                     (int8_t*)(blk + o_out));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(grid_out, blk + o_out, cells, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return wall_block_verdict(wb);
}
