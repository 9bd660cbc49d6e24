// Reference paths of libmpmpc.so, part of the one translation unit mpmpc_hip.hip (included there behind mpmpc_lidar.hpp):
// the kernel K0p and the entry points mpmpc_path_count (host only) and mpmpc_path_build (no handle, like mpmpc_lidar_scan).
// The law: path_core.hpp.  Steps 1 - 4 run on the host inside the call (path_rows: every libm result of a path is the
// host's); K0p is step 5, the static width.
#pragma once

// K0p: one THREAD per line, 18 lines per waypoint (side-major: lines 0 .. 8 left, 9 .. 17 right), a WORKGROUP of 576 threads =
// 32 waypoints of ONE path (a path's last workgroup may hold fewer; blk[] = (path, first row) per workgroup, rows counted
// over all paths).  A line walk is serial - cor_line_aa's float32 recurrence - and its occupancy reads scatter over a grid
// that stays in the L2; the 18 lines of a waypoint share their start and end within a cell, so the lanes of a wave walk
// lines of nearly one length.  Each thread keeps the first strict minimum of its own line (path_line_min), the 18 results
// meet in LDS, and one thread per side (the first wave: lane = 2 * waypoint + side) reduces its nine (path_side_reduce).
// The path's discs and wall headers are staged in LDS; the world's predicate is wall_world_occupied.
// out [rows][PATH_WP_OUT] doubles, flags [rows][2] ints (a side that probed outside the grid).  Every index is bounded: a
// walk by max_width <= 512 cells (the host's check), the grid reads by cor_cell_free, a path's discs / walls to
// COR_MAX_DISCS / COR_MAX_WALLS, the table reads by the wall's box.
constexpr int K0P_WPS = 32, K0P_LINES = 2 * PATH_LINES, K0P_THREADS = K0P_WPS * K0P_LINES;
__global__ __launch_bounds__(K0P_THREADS) void mpmpc_path_width_kernel(MapView map, int n_blocks, const int* __restrict__ blk,
                                                                       const int* __restrict__ row_off, const double* __restrict__ maxw,
                                                                       const double* __restrict__ xy, const int* __restrict__ cells,
                                                                       const int* __restrict__ d_off, const int* __restrict__ discs,
                                                                       WallView wv, double* __restrict__ out, int* __restrict__ flags) {
  __shared__ int s_disc[3 * COR_MAX_DISCS];
  __shared__ int s_whdr[WALL_HDR * COR_MAX_WALLS];
  __shared__ double s_d[K0P_THREADS];
  __shared__ int s_x[K0P_THREADS], s_y[K0P_THREADS], s_out[K0P_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= n_blocks) return;      // (uniform)
  const int p = blk[2 * b], row0 = blk[2 * b + 1];
  int n = row_off[p + 1] - row0;
  n = n > K0P_WPS ? K0P_WPS : n;
  int nd = 0, nw = 0;
  if (d_off) {
    const int d0 = d_off[p];
    nd = d_off[p + 1] - d0;
    nd = nd > COR_MAX_DISCS ? COR_MAX_DISCS : nd;      // (the host refuses more of either)
    for (int k = tid; k < 3 * nd; k += K0P_THREADS) s_disc[k] = discs[3L * d0 + k];
  }
  if (wv.off) {
    const int w0 = wv.off[p];
    nw = wv.off[p + 1] - w0;
    nw = nw > COR_MAX_WALLS ? COR_MAX_WALLS : nw;
    for (int k = tid; k < WALL_HDR * nw; k += K0P_THREADS) s_whdr[k] = wv.hdr[(long)WALL_HDR * w0 + k];
  }
  __syncthreads();
  const double mw = maxw[p];
  const int w = tid / K0P_LINES, l = tid - w * K0P_LINES, side = l / PATH_LINES;
  PathLineBest r{mw, 0, 0, 0};
  if (w < n) {
    const long row = (long)row0 + w;
    const int* c = cells + PATH_WP_INTS * row;
    int ex, ey;
    path_line_end(c[2 + 2 * side], c[3 + 2 * side], l - side * PATH_LINES, ex, ey);
    r = path_line_min(map, xy[2 * row], xy[2 * row + 1], c[0], c[1], ex, ey, mw, [&](int x, int y) {
      return wall_world_occupied(map, x, y, nd, [&](int q) { return (const int*)(s_disc + 3 * q); }, nw,
                                 [&](int q) { return (const int*)(s_whdr + WALL_HDR * q); }, wv.tab);
    });
  }
  s_d[tid] = r.d; s_x[tid] = r.x; s_y[tid] = r.y; s_out[tid] = r.outside;
  __syncthreads();
  if (tid < 2 * n) {
    const int rw = tid >> 1, rs = tid & 1, base = rw * K0P_LINES + rs * PATH_LINES;
    const long row = (long)row0 + rw;
    const int* c = cells + PATH_WP_INTS * row;
    double o[3];
    path_side_reduce(map, mw, c[2 + 2 * rs], c[3 + 2 * rs], [&](int k, double& d, int& x, int& y) {
      d = s_d[base + k]; x = s_x[base + k]; y = s_y[base + k];
    }, o);
    int outside = 0;
    for (int k = 0; k < PATH_LINES; ++k) outside |= s_out[base + k];
    out[PATH_WP_OUT * row + rs] = o[0];
    out[PATH_WP_OUT * row + 2 + 2 * rs] = o[1];
    out[PATH_WP_OUT * row + 3 + 2 * rs] = o[2];
    flags[2 * row + rs] = outside;
  }
}

// device scratch of mpmpc_path_build, kept between calls like the speed profile's (SpScratch)
static SpScratch g_path_dev[SP_MAX_DEVICES];

static int path_build_impl(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                           double resolution, int32_t P, const int32_t* corner_offsets, const double* corners, const double* spec,
                           const int32_t* ispec, const int32_t* disc_offsets, const int32_t* discs, const int32_t* wall_offsets,
                           const int32_t* walls, int32_t cap, int32_t* n_wp, int32_t* status, double* x, double* y, double* psi,
                           double* kappa, double* ds_next, double* ub, double* lb, double* border, double* length, float* ms) {
  const char* why = "";
  const bool outputs = n_wp && status && x && y && psi && kappa && ds_next && ub && lb && border && length;
  if (path_check_build(height, width, data, origin_x, origin_y, resolution, P, corner_offsets, corners, spec, ispec, disc_offsets,
                       discs, wall_offsets, walls, cap, outputs, &why))
    return fail(MPMPC_E_ARG, why);
  // steps 1 - 4 on the host
  const auto t0 = std::chrono::steady_clock::now();
  const MapView frame{nullptr, height, width, origin_x, origin_y, resolution};
  std::vector<PathRows> tabs((size_t)P);
  std::vector<int32_t> count((size_t)P), stat((size_t)P), row_off((size_t)P + 1, 0), blk;
  for (int p = 0; p < P; ++p) {
    const long long c = path_rows(frame, corner_offsets[p + 1] - corner_offsets[p], corners + 2L * corner_offsets[p], spec[2 * p],
                                    spec[2 * p + 1], ispec[2 * p], ispec[2 * p + 1] != 0, cap, tabs[p]);
    count[p] = c > 2147483647LL ? 2147483647 : (int32_t)c;
    stat[p] = c < 2 ? PATH_E_SHORT : c > cap ? PATH_E_CAP : PATH_OK;
    const int rows = stat[p] == PATH_OK ? count[p] : 0;
    for (int r = 0; r < rows; r += K0P_WPS) { blk.push_back(p); blk.push_back(row_off[p] + r); }
    if ((long long)row_off[p] + rows > 2147483647LL / PATH_WP_OUT) return fail(MPMPC_E_ARG, "more than 2^31 / 6 waypoints in one call");
    row_off[p + 1] = row_off[p] + rows;
  }
  const size_t rows = (size_t)row_off[P], n_blk = blk.size() / 2;
  std::vector<double> xy(2 * rows + 1), maxw((size_t)P), res_out(PATH_WP_OUT * rows + 1);
  std::vector<int32_t> cells(PATH_WP_INTS * rows + 1), flags(2 * rows + 1);
  for (int p = 0; p < P; ++p) {
    maxw[p] = spec[2 * p + 1];
    for (int i = 0; i < row_off[p + 1] - row_off[p]; ++i) {
      const size_t r = (size_t)row_off[p] + i;
      xy[2 * r] = tabs[p].x[i]; xy[2 * r + 1] = tabs[p].y[i];
      for (int e = 0; e < PATH_WP_INTS; ++e) cells[PATH_WP_INTS * r + e] = tabs[p].cells[(size_t)PATH_WP_INTS * i + e];
    }
  }
  if (ms) ms[0] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // step 5 on the device
  // (a call without a row to fill still takes the scratch: the device ordinal is checked whatever the routes are)
  const size_t np = (size_t)P;
  Layout L;
  const auto r_xy = L.add<double>(2 * rows), r_maxw = L.add<double>(np), r_out = L.add<double>(PATH_WP_OUT * rows);
  const auto r_cells = L.add<int>(PATH_WP_INTS * rows), r_flags = L.add<int>(2 * rows), r_blk = L.add<int>(2 * n_blk),
             r_row = L.add<int>(np + 1);
  WorldBlock wd = world_block(L, height, width, data, P, disc_offsets, discs, wall_offsets, walls);
  Scratch sc;
  if (int rc = scratch_acquire(g_path_dev, device, rows > 0 ? L.bytes() : 0, "path", &sc)) return rc;
  if (rows > 0) {
    hipStream_t stream = sc.stream;
    char* dev = sc.blk;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (ms)
      for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipMemcpyAsync(r_xy.at(dev), xy.data(), r_xy.bytes(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(r_maxw.at(dev), maxw.data(), r_maxw.bytes(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(r_cells.at(dev), cells.data(), r_cells.bytes(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(r_blk.at(dev), blk.data(), r_blk.bytes(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(r_row.at(dev), row_off.data(), r_row.bytes(), hipMemcpyHostToDevice, stream));
    if (int rc = wd.upload(dev, stream)) return rc;
    if (ms) HIP_TRY(hipEventRecord(ev[0], stream));
    if (int rc = wd.walls.enqueue(dev, stream)) return rc;      // K0w first, on the same stream
    if (ms) HIP_TRY(hipEventRecord(ev[1], stream));
    hipLaunchKernelGGL(mpmpc_path_width_kernel, dim3((unsigned)n_blk), dim3(K0P_THREADS), 0, stream,
                       wd.map(dev, origin_x, origin_y, resolution), (int)n_blk, r_blk.at(dev), r_row.at(dev), r_maxw.at(dev),
                       r_xy.at(dev), r_cells.at(dev), wd.offsets(dev), wd.discs(dev), wd.walls.view(dev), r_out.at(dev),
                       r_flags.at(dev));
    HIP_TRY(hipGetLastError());
    if (ms) HIP_TRY(hipEventRecord(ev[2], stream));
    HIP_TRY(pull(stream, res_out.data(), r_out.at(dev), r_out.count));
    HIP_TRY(pull(stream, flags.data(), r_flags.at(dev), r_flags.count));
    HIP_TRY(hipStreamSynchronize(stream));
    if (ms) {
      HIP_TRY(hipEventElapsedTime(&ms[1], ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&ms[2], ev[1], ev[2]));
      for (auto& e : ev) HIP_TRY(hipEventDestroy(e));
    }
    if (int rc = wd.verdict()) return rc;
  } else if (ms) {
    ms[1] = ms[2] = 0.0f;
  }
  // the outputs, written only now: a refused call leaves them untouched
  const double nan = std::nan("");
  const size_t all = (size_t)P * (size_t)cap;
  for (double* a : {x, y, psi, kappa, ds_next, ub, lb})
    for (size_t k = 0; k < all; ++k) a[k] = nan;
  for (size_t k = 0; k < 4 * all; ++k) border[k] = nan;
  for (int p = 0; p < P; ++p) {
    n_wp[p] = count[p];
    status[p] = stat[p];
    length[p] = nan;
    if (stat[p] != PATH_OK) continue;
    const PathRows& t = tabs[p];
    const size_t o = (size_t)p * (size_t)cap;
    length[p] = t.length;
    for (int i = 0; i < count[p]; ++i) {
      const size_t r = (size_t)row_off[p] + i;
      x[o + i] = t.x[i]; y[o + i] = t.y[i]; psi[o + i] = t.psi[i]; kappa[o + i] = t.kappa[i]; ds_next[o + i] = t.ds_next[i];
      ub[o + i] = res_out[PATH_WP_OUT * r];
      lb[o + i] = -res_out[PATH_WP_OUT * r + 1];
      for (int e = 0; e < 4; ++e) border[4 * (o + i) + e] = res_out[PATH_WP_OUT * r + 2 + e];
      if (flags[2 * r] | flags[2 * r + 1]) status[p] = PATH_OUTSIDE;
    }
  }
  return MPMPC_OK;
}

extern "C" {

int32_t mpmpc_path_count(int32_t n_corners, const double* corners, double path_resolution, int32_t smoothing) {
  const char* why = "";
  if (path_check_route(n_corners, corners, path_resolution, smoothing, &why)) return fail(MPMPC_E_ARG, why);
  const long long c = path_wp_count(n_corners, corners, path_resolution, smoothing);
  return c > 2147483647LL ? 2147483647 : (int32_t)c;
}

int mpmpc_path_build(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                     double resolution, int32_t P, const int32_t* corner_offsets, const double* corners, const double* spec,
                     const int32_t* ispec, const int32_t* disc_offsets, const int32_t* discs, const int32_t* wall_offsets,
                     const int32_t* walls, int32_t cap, int32_t* n_wp, int32_t* status, double* x, double* y, double* psi,
                     double* kappa, double* ds_next, double* ub, double* lb, double* border, double* length) {
  return path_build_impl(device, height, width, data, origin_x, origin_y, resolution, P, corner_offsets, corners, spec, ispec,
                         disc_offsets, discs, wall_offsets, walls, cap, n_wp, status, x, y, psi, kappa, ds_next, ub, lb, border,
                         length, nullptr);
}

int mpmpc_path_build_timed(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                           double resolution, int32_t P, const int32_t* corner_offsets, const double* corners, const double* spec,
                           const int32_t* ispec, const int32_t* disc_offsets, const int32_t* discs, const int32_t* wall_offsets,
                           const int32_t* walls, int32_t cap, int32_t* n_wp, int32_t* status, double* x, double* y, double* psi,
                           double* kappa, double* ds_next, double* ub, double* lb, double* border, double* length, float* ms) {
  if (!ms) return fail(MPMPC_E_ARG, "ms must not be NULL");
  return path_build_impl(device, height, width, data, origin_x, origin_y, resolution, P, corner_offsets, corners, spec, ispec,
                         disc_offsets, discs, wall_offsets, walls, cap, n_wp, status, x, y, psi, kappa, ds_next, ub, lb, border,
                         length, ms);
}

}  // extern "C"
