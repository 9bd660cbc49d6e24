// CPU twin of the wall kernels: K0w (mpmpc_wall_raster_kernel), K-world (mpmpc_world_grid_kernel) and the WALLS variants of
// K0c, K0l and K0f - the same wall_core.hpp code (and corridor_core / lidar_core / footprint_core beneath it), one wall,
// one car, one cell after the other.  Built by tests/test_walls.py with the flags of tests/test_footprint.py's twin.
#include <cmath>
#include <cstdint>
#include <vector>

#include "footprint_core.hpp"
#include "wall_core.hpp"

using namespace mpmpc;

namespace {

// headers and table of a fleet's walls, as the library lays them out (wall_layout) and K0w fills them; false: a wall
// does not fit the table
struct Walls {
  std::vector<int32_t> hdr, tab;
  bool ok = true;
  Walls(long n, const int32_t* walls) : hdr((size_t)WALL_HDR * n + 1) {
    tab.assign((size_t)wall_layout(n, walls, hdr.data()) + 1, 0);
    for (long j = 0; j < n; ++j) ok = wall_raster(walls + 4 * j, hdr.data() + WALL_HDR * j, tab.data()) && ok;
  }
};

}  // namespace

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
  MapView m{grid, h, w, ox, oy, res};
  std::vector<double> trig((size_t)n_wp * COR_TRIG);
  for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
  PathGeom g{x, y, psi, ds_next, n_wp, circular, trig.data()};
  std::vector<double> segs((size_t)n_wp * 4 * COR_MAXSEG, 0.0), wpc((size_t)n_wp * COR_WPC, 0.0);
  std::vector<int> nseg(n_wp), cells((size_t)n_wp * COR_CELL_CAP), box((size_t)n_wp * COR_LINE_BOX);
  for (int i = 0; i < n_wp; ++i) {           // K0a
    int ux, uy, lx, ly;
    cor_w2m(m, bub[2 * i], bub[2 * i + 1], ux, uy);
    cor_w2m(m, blb[2 * i], blb[2 * i + 1], lx, ly);
    int* c = cells.data() + (size_t)i * COR_CELL_CAP;
    const int n = cor_line_cells(ux, uy, lx, ly, c, COR_CELL_CAP);
    if (n > COR_CELL_CAP) return 1;
    const int cnt = cor_scan_cells(m, ux, uy, lx, ly, min_width, n, [&](int k, int& cx, int& cy) { cor_unpack_cell(c[k], cx, cy); },
                                   [&](int k) { int cx, cy; cor_unpack_cell(c[k], cx, cy); return cor_cell_free(m, cx, cy); },
                                   segs.data() + (size_t)i * 4 * COR_MAXSEG);
    if (cnt < 0) return 2;
    nseg[i] = cnt;
    if (cnt <= 1) cor_forced(g, segs.data(), nseg.data(), i, sm, wpc.data() + (size_t)i * COR_WPC);
    cor_line_box(c, n, (ux + 1) | ((uy + 1) << 16), (lx + 1) | ((ly + 1) << 16), box.data() + (size_t)i * COR_LINE_BOX);
  }
  std::vector<double> col_o((size_t)N * COR_WPC);
  std::vector<int> col_seg((size_t)N * 2 * COR_MAXSEG), col_cnt(N);
  for (int b = 0; b < n_start; ++b) {        // K0c<WALLS>, one car
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    auto disc = [&](int j) { return discs + 3L * (d0 + j); };
    const int w0 = woff[b], nw = woff[b + 1] - w0;
    auto hdr = [&](int j) { return (const int*)(ws.hdr.data() + (size_t)WALL_HDR * (w0 + j)); };
    const int wp = wp_id[b] + 1;
    bool over = false;
    for (int n = 0; n < N; ++n) {
      const int i = cor_wp(g, wp + n);
      const int* bx = box.data() + (size_t)i * COR_LINE_BOX;
      double* o = col_o.data() + (size_t)n * COR_WPC;
      if (wall_car_touches(bx, nd, disc, nw, hdr)) {
        int* cs = col_seg.data() + (size_t)n * 2 * COR_MAXSEG;
        double s0[4] = {0, 0, 0, 0};
        const int cnt = wall_car_scan(m, min_width, cells.data() + (size_t)i * COR_CELL_CAP, bx, nd, disc, nw, hdr, ws.tab.data(),
                                      [&](int q, int sx, int sy, int ex, int ey, double ax, double ay, double bx2, double by) {
                                        cs[2 * q] = (sx + 1) | ((sy + 1) << 16);
                                        cs[2 * q + 1] = (ex + 1) | ((ey + 1) << 16);
                                        if (q == 0) { s0[0] = ax; s0[1] = ay; s0[2] = bx2; s0[3] = by; }
                                      });
        if (cnt < 0) over = true;
        else if (cnt <= 1) cor_forced_seg(g, i, cnt, s0, sm, o);
        col_cnt[n] = cnt < 0 ? cnt : cnt + 1000;
      } else {
        const int cnt = nseg[i];
        if (cnt <= 1)
          for (int k = 0; k < COR_WPC; ++k) o[k] = wpc[(size_t)i * COR_WPC + k];
        col_cnt[n] = cnt;
      }
    }
    auto cnt = [&](int c) { const int v = col_cnt[c]; return v >= 1000 ? v - 1000 : v; };
    auto forced = [&](int c, double* o) { for (int k = 0; k < COR_WPC; ++k) o[k] = col_o[(size_t)c * COR_WPC + k]; };
    auto seg = [&](int c, int k, double* s) {
      if (col_cnt[c] >= 1000) {
        const int* cs = col_seg.data() + (size_t)c * 2 * COR_MAXSEG;
        int cx, cy;
        cor_unpack_cell(cs[2 * k], cx, cy);
        cor_m2w(m, cx, cy, s[0], s[1]);
        cor_unpack_cell(cs[2 * k + 1], cx, cy);
        cor_m2w(m, cx, cy, s[2], s[3]);
      } else {
        const double* sg = segs.data() + (size_t)cor_wp(g, wp + c) * 4 * COR_MAXSEG + 4 * k;
        for (int j = 0; j < 4; ++j) s[j] = sg[j];
      }
    };
    const int verdict = cnt(0) == 0 ? COR_ROW_BLOCKED : (over ? COR_ROW_OVERFLOW : COR_ROW_OK);
    for (int n = 0; n < N; ++n) {
      double u = std::nan(""), l = std::nan("");
      if (verdict == COR_ROW_OK) cor_select_car_one(g, wp, n, sm, cnt, forced, seg, &u, &l);
      ub[(size_t)b * N + n] = u;
      lb[(size_t)b * N + n] = l;
    }
    flag[b] = verdict;
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
