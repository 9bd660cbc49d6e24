// CPU twin of the wall kernels: K0w (mpmpc_wall_raster_kernel), K-world (mpmpc_world_grid_kernel) and the WALLS variants of
// K0c, K0l and K0f - the same wall_core.hpp code (and corridor_core / lidar_core / footprint_core beneath it), one wall,
// one car, one cell after the other; K0c's rows: car_rows.hpp.  Built by tests/emul/Makefile (`make walls`), loaded by tests/twins.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../emul_car/car_rows.hpp"
#include "footprint_core.hpp"

using namespace mpmpc;

extern "C" {

// Validation of mpmpc_rollout_set_walls (the library calls the same function): 0, -1 (E_ARG) or -3 (E_STATE).
int wall_emu_check(int B, int max_batch, const int32_t* off, const int32_t* walls, int built, int map_w, int map_h, int other_B) {
  const char* why = "";
  return wall_check_walls(B, max_batch, off, walls, built != 0, map_w, map_h, other_B, &why);
}

// The cells of ONE wall as its table gives them: every cell of the grown box that wall_on accepts, in row order, into
// xs / ys [cap].  Returns their number (possibly more than cap), or -1 when the line does not fit the table.
// props[3] (may be NULL), from cor_line_aa itself: major indices without a cell or cells outside the major range; the
// largest minor span of one major index, -1 if the cells of one are not contiguous; the furthest a cell lies outside the
// end points' minor range.
long wall_emu_cells(const int32_t* wall, int32_t* xs, int32_t* ys, long cap, int32_t* props) {
  Walls w(1, wall);
  if (!w.ok) return -1;
  const int* h = w.hdr.data();
  long n = 0;
  for (int y = h[1]; xs && y <= h[3]; ++y)      // (xs == NULL: the properties only - long lines)
    for (int x = h[0]; x <= h[2]; ++x)
      if (wall_on(x, y, h, w.tab.data())) {
        if (n < cap) { xs[n] = x; ys[n] = y; }
        ++n;
      }
  if (props) {
    const int ext = wall_extent(wall), axis = h[5];
    const int m0 = axis == 0 ? h[0] : h[1];
    const int lo = axis == 0 ? h[1] + 1 : h[0] + 1, hi = axis == 0 ? h[3] - 1 : h[2] - 1;      // the end points' minor range
    std::vector<int> mn((size_t)ext, 1 << 30), mx((size_t)ext, -(1 << 30)), cnt((size_t)ext, 0);
    std::vector<std::vector<int>> seen((size_t)ext);
    int bad = 0, outside = 0;
    cor_line_aa(wall[0], wall[1], wall[2], wall[3], [&](int x, int y) {
      const int k = (axis == 0 ? x : y) - m0, minor = axis == 0 ? y : x;
      if (k < 0 || k >= ext) { ++bad; return; }
      bool dup = false;
      for (int v : seen[k]) dup = dup || v == minor;
      if (!dup) { seen[k].push_back(minor); ++cnt[k]; }
      mn[k] = minor < mn[k] ? minor : mn[k];
      mx[k] = minor > mx[k] ? minor : mx[k];
      const int o = minor < lo ? lo - minor : (minor > hi ? minor - hi : 0);
      outside = o > outside ? o : outside;
    });
    int span = 0;
    for (int k = 0; k < ext; ++k) {
      if (cnt[k] == 0) { ++bad; continue; }
      const int s = mx[k] - mn[k] + 1;
      if (s != cnt[k]) span = -1;
      else if (span >= 0 && s > span) span = s;
    }
    props[0] = bad; props[1] = span; props[2] = outside;
  }
  return n;
}

// K-world: out [h][w] <- 1 free / 0 occupied of the grid with nd discs and nw walls.  Returns 0, or 1 when a wall does not fit.
int wall_emu_world_grid(int h, int w, const int8_t* grid, int nd, const int32_t* discs, int nw, const int32_t* walls, int8_t* out) {
  Walls ws(nw, walls);
  if (!ws.ok) return 1;
  const MapView m{grid, h, w, 0.0, 0.0, 1.0};
  auto disc = [&](int q) { return discs + 3L * q; };
  auto hdr = [&](int q) { return (const int*)(ws.hdr.data() + WALL_HDR * q); };
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) out[(long)y * w + x] = wall_world_occupied(m, x, y, nd, disc, nw, hdr, ws.tab.data()) ? 0 : 1;
  return 0;
}

// K0a's base build on the grid, then K0c<WALLS>'s rows for n_start cars whose waypoint is wp_id[b], whose discs are the CSR
// lists off / discs (off may be NULL: none) and whose walls are the CSR lists woff / walls.  ub / lb [n_start x N] (NaN rows
// unless the verdict is COR_ROW_OK), flag [n_start] = COR_ROW_*.  Returns 0, 1 / 2 when the base build overflows, 3 when a
// wall does not fit the table.
int wall_emu_rows(int h, int w, const int8_t* grid, double ox, double oy, double res, int n_wp, const double* x, const double* y,
                  const double* psi, const double* ds_next, int circular, const double* bub, const double* blb, int N,
                  double min_width, double sm, int n_start, const int32_t* wp_id, const int32_t* off, const int32_t* discs,
                  const int32_t* woff, const int32_t* walls, double* ub, double* lb, int32_t* flag) {
  Walls ws(woff[n_start], walls);
  if (!ws.ok) return 3;
  TwinBase base(h, w, grid, ox, oy, res, n_wp, x, y, psi, ds_next, circular, bub, blb, min_width, sm);
  const RouteView v = route_view(nullptr, 0, n_wp, circular);
  if (int rc = base.build(v)) return rc;
  for (int b = 0; b < n_start; ++b) {
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    const int w0 = woff[b], nw = woff[b + 1] - w0;
    auto hdr = [&](int j) { return (const int*)(ws.hdr.data() + (size_t)WALL_HDR * (w0 + j)); };
    flag[b] = car_rows<true>(base, v, wp_id[b], N, nd, plain_col_disc(discs + 3L * d0), nw, hdr, ws.tab.data(), ub + (size_t)b * N,
                             lb + (size_t)b * N);
  }
  return 0;
}

// K0l<WALLS>: tests/emul_lidar's scan with the walls in the predicate.  ranges [B][n_beams].  Returns the checks' code, 3
// when a wall does not fit the table.
int wall_emu_scan(int height, int width, const int8_t* data, double ox, double oy, double res, int B, const double* pose,
                  const int32_t* off, const int32_t* discs, const int32_t* woff, const int32_t* walls, int n_beams,
                  const double* angles, double range_m, double* ranges) {
  const char* why = "";
  if (int rc = lid_check_scan(height, width, data, res, B, pose, off, discs, n_beams, angles, range_m, ranges, &why)) return rc;
  if (int rc = wall_check_lists(B, woff, walls, width, height, &why)) return rc;
  Walls ws(woff[B], walls);
  if (!ws.ok) return 3;
  const MapView m{data, height, width, ox, oy, res};
  std::vector<int> best((size_t)n_beams);
  for (int b = 0; b < B; ++b) {
    double* out = ranges + (long)b * n_beams;
    const double psi = pose[3L * b + 2];
    int cx, cy;
    if (!lid_sensor_cell(m, pose[3L * b], pose[3L * b + 1], psi, &cx, &cy)) {
      for (int k = 0; k < n_beams; ++k) out[k] = std::nan("");
      continue;
    }
    const LidWindow w = lid_window(m, cx, cy, range_m);
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    auto disc = [&](int q) { return discs + 3L * (d0 + q); };
    const int w0 = woff[b], nw = woff[b + 1] - w0;
    auto hdr = [&](int q) { return (const int*)(ws.hdr.data() + (size_t)WALL_HDR * (w0 + q)); };
    for (int k = 0; k < n_beams; ++k) best[k] = LID_NONE;
    for (int j = w.j0; j <= w.j1; ++j)
      for (int i = w.i0; i <= w.i1; ++i) {
        if (!wall_lid_occupied(m, i, j, nd, disc, nw, hdr, ws.tab.data())) continue;
        int d2;
        if (!lid_in_range(i - cx, j - cy, w.lim, &d2)) continue;
        double mn, mx;
        if (!lid_cell_interval(i - cx, j - cy, psi, &mn, &mx)) continue;
        for (int k = lid_first_beam(angles, n_beams, mn); k < n_beams && angles[k] <= mx; ++k) best[k] = d2 < best[k] ? d2 : best[k];
      }
    for (int k = 0; k < n_beams; ++k) out[k] = lid_range(best[k], res, range_m);
  }
  return 0;
}

// K0f<WALLS>: tests/emul_footprint's audit with the walls in the predicate.  contact [B], clearance [B].
int wall_emu_audit(int height, int width, const int8_t* data, double ox, double oy, double res, int B, const double* pose,
                   const int32_t* off, const int32_t* discs, const int32_t* woff, const int32_t* walls, double length,
                   double car_width, double reach_m, int32_t* contact, double* clearance) {
  const char* why = "";
  int R = 0;
  if (int rc = fp_check_audit(height, width, data, res, B, pose, off, discs, length, car_width, reach_m, contact, clearance, &R, &why))
    return rc;
  if (int rc = wall_check_lists(B, woff, walls, width, height, &why)) return rc;
  Walls ws(woff[B], walls);
  if (!ws.ok) return 3;
  const MapView m{data, height, width, ox, oy, res};
  for (int b = 0; b < B; ++b) {
    const double x = pose[3L * b], y = pose[3L * b + 1], psi = pose[3L * b + 2];
    int cx, cy;
    if (!lid_sensor_cell(m, x, y, psi, &cx, &cy)) {
      contact[b] = 0;
      clearance[b] = std::nan("");
      continue;
    }
    const FpCar car = fp_car(x, y, psi, length, car_width);
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    auto disc = [&](int q) { return discs + 3L * (d0 + q); };
    const int w0 = woff[b], nw = woff[b + 1] - w0;
    auto hdr = [&](int q) { return (const int*)(ws.hdr.data() + (size_t)WALL_HDR * (w0 + q)); };
    const int i0 = cx - R < 0 ? 0 : cx - R, i1 = cx + R > width - 1 ? width - 1 : cx + R;
    const int j0 = cy - R < 0 ? 0 : cy - R, j1 = cy + R > height - 1 ? height - 1 : cy + R;
    double best = FP_NONE;
    int hit = 0;
    for (int j = j0; j <= j1; ++j)
      for (int i = i0; i <= i1; ++i) {
        if (!wall_lid_occupied(m, i, j, nd, disc, nw, hdr, ws.tab.data())) continue;
        const double g = fp_cell_g(m, car, i, j);
        hit |= g == 0.0;
        best = g < best ? g : best;
      }
    contact[b] = hit;
    clearance[b] = fp_clearance(best, reach_m);
  }
  return 0;
}

}  // extern "C"
