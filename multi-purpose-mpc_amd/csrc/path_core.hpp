// Building a reference path: from corner points to the per-waypoint tables and the static width, what
// ReferencePath.__init__ of the reference computes (src/reference_path.py:110-287).  Steps 1 - 4 are host code (plain
// inline functions: every libm call of a path - atan2, cos, sin - runs here, as cor_trig_row does for the corridor); step 5
// is scalar code that compiles for gfx950 (K0p, mpmpc_path.hpp) and for the host (tests/emul_path), like lidar_core.hpp.
// Every operation is rounded on its own (the builds carry -ffp-contract=off).
//
// One path: corner points (cx[k], cy[k]), path resolution r_p, smoothing distance sd, max_width, circular, and a world -
// the grid frame (ox, oy, res), the path's discs and walls (wall_core.hpp).  In exactly this order:
//
//   1 counts:  cnt[k] = (int)(sqrt(dx * dx + dy * dy) / r_p) per segment; its raw points are i * (d / cnt[k]) + c[k] for
//       i = 0 .. cnt[k] - 1 (numpy's linspace without end point: a multiply, then an add); a segment with cnt == 0 gives
//       nothing; the last corner is appended.
//   2 smoothing:  point j = sum(raw[j .. j + 2 sd]) / (2 sd + 1), the sum in numpy's pairwise order (path_mean); 2 sd + 1
//       <= 127 keeps numpy's recursive split out of it.
//   3 waypoints:  waypoint i = point i up to the second-to-last, n_wp = points - 1.  step = p[i + 1] - p[i], dist =
//       sqrt(sx * sx + sy * sy), psi = atan2(sy, sx); kappa[0] = 0, kappa[i] = wrap(psi[i] - psi[i - 1]) / (dist[i] + 1e-12)
//       (cor_wrap_host); ds_next[i] = dist[i] for i < n_wp - 1, ds_next[n_wp - 1] = the distance back to waypoint 0 if
//       circular, else 0 (ReferencePath.tables()); length = the sequential sum of the n_wp - 1 segment lengths.
//   4 normals:  per waypoint and side s = +1 (left), -1 (right): ang = wrap(psi + s * pi / 2), target (x + max_width *
//       cos(ang), y + max_width * sin(ang)), target cell (tx, ty) = cor_w2m(target), own cell (px, py) = cor_w2m(x, y).
//   5 width:  for di in (-1, 0, 1), outer, dj in (-1, 0, 1), inner: the line cor_line_aa(px, py, tx + di, ty + dj) in
//       skimage's order, the start cell included.  A visited cell that is occupied in the path's world
//       (wall_world_occupied: on the grid, outside it, in a disc, on a wall) is a candidate at d = sqrt((x - qx)^2 + (y -
//       qy)^2) from the waypoint to its centre cor_m2w.  The result is the first candidate in that order with d strictly
//       below everything before it, starting from max_width: width = d, border cell = its centre.  No candidate: width =
//       max_width, border cell = the centre of the last target probed, (tx + 1, ty + 1).  ub = width_left, lb =
//       -width_right.
//     Split: a line keeps its own first strict minimum below max_width (path_line_min); the nine lines of a side are
//     reduced by (smaller d, then lower line index 3 (di + 1) + (dj + 1)) (path_side_reduce) - the same cell.
// A probed cell outside the grid counts as occupied and is reported (status 1): the reference would have raised there,
// or wrapped around at -1.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "lidar_core.hpp"
#include "wall_core.hpp"

namespace mpmpc {

constexpr int PATH_MAX_SMOOTHING = 63;        // 2 sd + 1 <= 127 terms per mean
constexpr int PATH_MAX_WIDTH_CELLS = 512;     // max_width / resolution: bounds a line walk
constexpr int PATH_LINES = 9;                 // lines per side
constexpr int PATH_WP_INTS = 6;               // px, py, tx_left, ty_left, tx_right, ty_right
constexpr int PATH_WP_OUT = 6;                // width_left, width_right, ub_x, ub_y, lb_x, lb_y
constexpr double PATH_CELL_MAX = 1073741824.0;      // corners lie within 2^30 cells of the origin
constexpr int PATH_OK = 0, PATH_OUTSIDE = 1, PATH_E_SHORT = -1, PATH_E_CAP = -2;      // status[p]

// ---------------------------------------------------------------------------------------------- step 5 (host and device)
struct PathLineBest {
  double d;          // max_width: no candidate on this line
  int x, y;          // the candidate's cell
  int outside;       // 1: the line visited a cell outside the grid
};
// one line: its first strict minimum below max_width.  occupied(x, y): the world's predicate.
template <class Occ>
MPMPC_HD PathLineBest path_line_min(const MapView& m, double wx, double wy, int px, int py, int ex, int ey, double max_width,
                                    Occ occupied) {
  PathLineBest b{max_width, 0, 0, 0};
  cor_line_aa(px, py, ex, ey, [&](int x, int y) {
    if ((unsigned)x >= (unsigned)m.width || (unsigned)y >= (unsigned)m.height) b.outside = 1;
    if (!occupied(x, y)) return;
    double qx, qy;
    cor_m2w(m, x, y, qx, qy);
    const double d = std::sqrt((wx - qx) * (wx - qx) + (wy - qy) * (wy - qy));
    if (d < b.d) { b.d = d; b.x = x; b.y = y; }
  });
  return b;
}
// the target cell of line l = 3 (di + 1) + (dj + 1) of a side whose target cell is (tx, ty)
MPMPC_HD void path_line_end(int tx, int ty, int l, int& ex, int& ey) {
  ex = tx + l / 3 - 1;
  ey = ty + l % 3 - 1;
}
// a side from its nine lines (line(l) -> d, x, y of line l): o[0] = width, o[1 .. 2] = the border cell's centre
template <class Line>
MPMPC_HD void path_side_reduce(const MapView& m, double max_width, int tx, int ty, Line line, double* o) {
  double best = max_width;
  int bx = tx + 1, by = ty + 1;      // no candidate: the last target probed
  for (int l = 0; l < PATH_LINES; ++l) {
    double d;
    int x, y;
    line(l, d, x, y);
    if (d < best) { best = d; bx = x; by = y; }
  }
  o[0] = best;
  cor_m2w(m, bx, by, o[1], o[2]);
}

// ---------------------------------------------------------------------------------------------------- steps 1 - 4 (host)
// step 1: points of a segment
inline int path_seg_count(double ax, double ay, double bx, double by, double r_p) {
  const double dx = bx - ax, dy = by - ay;
  const double q = std::sqrt(dx * dx + dy * dy) / r_p;
  return q >= 2147483647.0 ? 2147483647 : (int)q;
}
// waypoints the path will have (<= 1: no path); corners [n][2]
inline long long path_wp_count(int n, const double* c, double r_p, int sd) {
  long long pts = 1;
  for (int k = 0; k + 1 < n; ++k) pts += path_seg_count(c[2 * k], c[2 * k + 1], c[2 * k + 2], c[2 * k + 3], r_p);
  const long long wp = pts - 2LL * sd - 1;
  return wp < 0 ? 0 : wp;
}
// step 2: numpy's mean of n <= 127 terms (add.reduce's pairwise sum below its block size, then one division)
inline double path_mean(const double* a, int n) {
  double res;
  if (n < 8) {
    res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
  } else {
    double r[8];
    for (int t = 0; t < 8; ++t) r[t] = a[t];
    int i = 8;
    for (; i < n - n % 8; i += 8)
      for (int t = 0; t < 8; ++t) r[t] += a[i + t];
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
  }
  return res / (double)n;
}

// the tables of one path, as the host computes them (steps 1 - 4); rows = n_wp
struct PathRows {
  std::vector<double> x, y, psi, kappa, ds_next;
  std::vector<int32_t> cells;      // [n_wp][PATH_WP_INTS]
  double length = 0.0;
};
// -> n_wp (the tables are filled iff 2 <= n_wp <= cap).  m: the grid's frame (data unused).
inline long long path_rows(const MapView& m, int n, const double* c, double r_p, double max_width, int sd, bool circular, int cap,
                             PathRows& t) {
  const long long count = path_wp_count(n, c, r_p, sd);
  if (count < 2 || count > cap) return count;
  const int n_wp = (int)count, terms = 2 * sd + 1, pts = n_wp + 1;
  std::vector<double> rx, ry;
  rx.reserve((size_t)pts + terms);
  ry.reserve((size_t)pts + terms);
  for (int k = 0; k + 1 < n; ++k) {
    const int cnt = path_seg_count(c[2 * k], c[2 * k + 1], c[2 * k + 2], c[2 * k + 3], r_p);
    if (cnt == 0) continue;
    const double sx = (c[2 * k + 2] - c[2 * k]) / (double)cnt, sy = (c[2 * k + 3] - c[2 * k + 1]) / (double)cnt;
    for (int i = 0; i < cnt; ++i) {
      rx.push_back((double)i * sx + c[2 * k]);
      ry.push_back((double)i * sy + c[2 * k + 1]);
    }
  }
  rx.push_back(c[2 * (n - 1)]);
  ry.push_back(c[2 * (n - 1) + 1]);
  std::vector<double> px((size_t)pts), py((size_t)pts), dist((size_t)n_wp);
  for (int j = 0; j < pts; ++j) {
    px[j] = path_mean(rx.data() + j, terms);
    py[j] = path_mean(ry.data() + j, terms);
  }
  t.x.assign(px.begin(), px.begin() + n_wp);
  t.y.assign(py.begin(), py.begin() + n_wp);
  t.psi.resize(n_wp); t.kappa.resize(n_wp); t.ds_next.resize(n_wp);
  t.cells.resize((size_t)PATH_WP_INTS * n_wp);
  t.length = 0.0;
  for (int i = 0; i < n_wp; ++i) {
    const double sx = px[i + 1] - px[i], sy = py[i + 1] - py[i];
    dist[i] = std::sqrt(sx * sx + sy * sy);
    t.psi[i] = std::atan2(sy, sx);
    t.kappa[i] = i == 0 ? 0.0 : cor_wrap_host(t.psi[i] - t.psi[i - 1]) / (dist[i] + 1e-12);
    if (i < n_wp - 1) {
      t.ds_next[i] = dist[i];
      t.length += dist[i];
    }
    double tr[COR_TRIG];
    cor_trig_row(t.psi[i], tr);
    int32_t* cell = t.cells.data() + (size_t)PATH_WP_INTS * i;
    int a, b;
    cor_w2m(m, t.x[i], t.y[i], a, b);
    cell[0] = a; cell[1] = b;
    cor_w2m(m, t.x[i] + max_width * tr[2], t.y[i] + max_width * tr[3], a, b);
    cell[2] = a; cell[3] = b;
    cor_w2m(m, t.x[i] + max_width * tr[4], t.y[i] + max_width * tr[5], a, b);
    cell[4] = a; cell[5] = b;
  }
  if (circular) {
    const double bx = t.x[0] - t.x[n_wp - 1], by = t.y[0] - t.y[n_wp - 1];
    t.ds_next[n_wp - 1] = std::sqrt(bx * bx + by * by);
  } else {
    t.ds_next[n_wp - 1] = 0.0;
  }
  return count;
}

// Host-side validation of mpmpc_path_count's arguments.  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int path_check_route(int n, const double* c, double r_p, int sd, const char** why) {
  if (n < 2) { *why = "a path needs at least 2 corner points"; return -1; }
  if (!c) { *why = "corners is NULL"; return -1; }
  for (int k = 0; k < 2 * n; ++k)
    if (!mov_finite(c[k])) { *why = "a corner point is not finite"; return -1; }
  if (!(r_p > 0.0) || !mov_finite(r_p)) { *why = "the path resolution must be positive and finite"; return -1; }
  if (sd < 0 || sd > PATH_MAX_SMOOTHING) { *why = "the smoothing distance must be in [0, 63] (PATH_MAX_SMOOTHING)"; return -1; }
  return 0;
}
// ... of mpmpc_path_build: everything that is decided before a device call
inline int path_check_build(int height, int width, const int8_t* data, double ox, double oy, double res, int P, const int32_t* coff,
                            const double* corners, const double* spec, const int32_t* ispec, const int32_t* doff,
                            const int32_t* discs, const int32_t* woff, const int32_t* walls, int cap, bool outputs,
                            const char** why) {
  if (height < 1 || width < 1 || !(res > 0.0) || !mov_finite(res)) { *why = "map needs positive size and resolution"; return -1; }
  if (height > COR_MAX_SIDE || width > COR_MAX_SIDE) { *why = "map sides are limited to 65534 cells"; return -1; }
  if (!mov_finite(ox) || !mov_finite(oy)) { *why = "the map's origin is not finite"; return -1; }
  if (P < 1) { *why = "P must be >= 1"; return -1; }
  if (cap < 1) { *why = "cap must be >= 1"; return -1; }
  if (!data || !coff || !corners || !spec || !ispec) { *why = "data, corner_offsets, corners, spec and ispec must not be NULL"; return -1; }
  if (!outputs) { *why = "no output pointer may be NULL"; return -1; }
  if (coff[0] != 0) { *why = "corner_offsets[0] must be 0"; return -1; }
  for (int p = 0; p < P; ++p) {
    if (coff[p + 1] < coff[p]) { *why = "corner_offsets must not decrease"; return -1; }
    const int n = coff[p + 1] - coff[p];
    const double* c = corners + 2L * coff[p];
    if (int rc = path_check_route(n, c, spec[2 * p], ispec[2 * p], why)) return rc;
    for (int k = 0; k < n; ++k)
      if (!(std::fabs((c[2 * k] - ox) / res) <= PATH_CELL_MAX && std::fabs((c[2 * k + 1] - oy) / res) <= PATH_CELL_MAX)) {
        *why = "a corner point lies more than 2^30 cells from the map's origin";
        return -1;
      }
    const double mw = spec[2 * p + 1];
    if (!(mw > 0.0) || !mov_finite(mw)) { *why = "max_width must be positive and finite"; return -1; }
    if (!(mw / res <= (double)PATH_MAX_WIDTH_CELLS)) { *why = "max_width is more than 512 cells (PATH_MAX_WIDTH_CELLS)"; return -1; }
  }
  if (int rc = lid_check_discs(P, doff, discs, width, height, why)) return rc;
  if (woff)
    if (int rc = wall_check_lists(P, woff, walls, width, height, why)) return rc;
  return 0;
}

}  // namespace mpmpc
