// The CPU twin of K0a's line cache and of K0c (mpmpc_car_corridor_kernel), written once: the same corridor_core.hpp / wall_core.hpp
// code as the kernels, one route, one car and one column after the other.  The entry points car_emu_rows, wall_emu_rows,
// look_emu_rows and tlk_emu_rows (tests/emul_car, emul_walls, emul_lookahead, emul_traffic_lookahead) are calls of car_rows.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "wall_core.hpp"

namespace mpmpc {

// headers and table of a fleet's walls, as the library lays them out (wall_layout) and K0w fills them; ok == false: a wall
// does not fit the table
struct Walls {
  std::vector<int32_t> hdr, tab;
  bool ok = true;
  Walls(long n, const int32_t* walls) : hdr((size_t)WALL_HDR * n + 1) {
    tab.assign((size_t)wall_layout(n, walls, hdr.data()) + 1, 0);
    for (long j = 0; j < n; ++j) ok = wall_raster(walls + 4 * j, hdr.data() + WALL_HDR * j, tab.data()) && ok;
  }
};

// K0a on the host: trig rows, line cells, free segments, forced rows and line boxes of the path table's rows, built per route
// when its first car asks (route == NULL: the one path) and indexed by global row.
struct TwinBase {
  MapView m;
  PathGeom whole;
  const double *bub, *blb;
  double min_width, sm;
  std::vector<double> trig, segs, wpc;
  std::vector<int> nseg, cells, box;
  std::vector<char> built;

  TwinBase(int h, int w, const int8_t* grid, double ox, double oy, double res, int n_wp, const double* x, const double* y,
           const double* psi, const double* ds_next, int circular, const double* bub, const double* blb, double min_width, double sm)
      : m{grid, h, w, ox, oy, res}, bub(bub), blb(blb), min_width(min_width), sm(sm), trig((size_t)n_wp * COR_TRIG),
        segs((size_t)n_wp * 4 * COR_MAXSEG, 0.0), wpc((size_t)n_wp * COR_WPC, 0.0), nseg(n_wp), cells((size_t)n_wp * COR_CELL_CAP),
        box((size_t)n_wp * COR_LINE_BOX), built(n_wp, 0) {
    for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
    whole = PathGeom{x, y, psi, ds_next, n_wp, circular, trig.data()};
  }

  // the rows of route v.  Returns 0, or 1 / 2: a line has more cells than the cache holds / more free segments than COR_MAXSEG.
  int build(const RouteView& v) {
    if (built[v.first]) return 0;
    built[v.first] = 1;
    const PathGeom g = route_geom(whole, v);
    for (int i = 0; i < v.n(); ++i) {
      const size_t r = v.first + i;
      int ux, uy, lx, ly;
      cor_w2m(m, bub[2 * r], bub[2 * r + 1], ux, uy);
      cor_w2m(m, blb[2 * r], blb[2 * r + 1], lx, ly);
      int* c = cells.data() + r * COR_CELL_CAP;
      const int n = cor_line_cells(ux, uy, lx, ly, c, COR_CELL_CAP);
      if (n > COR_CELL_CAP) return 1;
      double* const r_segs = segs.data() + (size_t)v.first * 4 * COR_MAXSEG;
      const int cnt = cor_scan_cells(m, ux, uy, lx, ly, min_width, n, [&](int k, int& cx, int& cy) { cor_unpack_cell(c[k], cx, cy); },
                                     [&](int k) { int cx, cy; cor_unpack_cell(c[k], cx, cy); return cor_cell_free(m, cx, cy); },
                                     r_segs + (size_t)i * 4 * COR_MAXSEG);
      if (cnt < 0) return 2;
      nseg[r] = cnt;
      if (cnt <= 1) cor_forced(g, r_segs, nseg.data() + v.first, i, sm, wpc.data() + r * COR_WPC);
      cor_line_box(c, n, (ux + 1) | ((uy + 1) << 16), (lx + 1) | ((ly + 1) << 16), box.data() + r * COR_LINE_BOX);
    }
    return 0;
  }
};

// K0c<WALLS, ...> for one car on route v at local waypoint wp_id: N columns into ub / lb (NaN unless the verdict is COR_ROW_OK);
// returns the verdict COR_ROW_*.  col_disc(n) is the disc accessor j -> const int* of column n over the car's nd discs (plain:
// the same list for every column; look_col_disc / tlk_col_disc: the column's own world).  WALLS: the wall path of the kernel -
// wall_car_touches / wall_car_scan over the car's nw walls hdr(j), table wtab - else nd > 0 && cor_car_touches / cor_car_scan.
template <bool WALLS, class ColDisc, class Hdr>
int car_rows(const TwinBase& base, const RouteView& v, int wp_id, int N, int nd, ColDisc col_disc, int nw, Hdr hdr, const int* wtab,
             double* ub, double* lb) {
  const MapView& m = base.m;
  const PathGeom g = route_geom(base.whole, v);
  const double* const r_segs = base.segs.data() + (size_t)v.first * 4 * COR_MAXSEG;
  const double* const r_wpc = base.wpc.data() + (size_t)v.first * COR_WPC;
  const int* const r_nseg = base.nseg.data() + v.first;
  const int* const r_cells = base.cells.data() + (size_t)v.first * COR_CELL_CAP;
  const int* const r_box = base.box.data() + (size_t)v.first * COR_LINE_BOX;
  std::vector<double> col_o((size_t)N * COR_WPC);
  std::vector<int> col_seg((size_t)N * 2 * COR_MAXSEG), col_cnt(N);
  const int wp = wp_id + 1;
  bool over = false;
  for (int n = 0; n < N; ++n) {              // column n in its own world
    auto disc = col_disc(n);
    const int i = cor_wp(g, wp + n);
    const int* bx = r_box + (size_t)i * COR_LINE_BOX;
    double* o = col_o.data() + (size_t)n * COR_WPC;
    bool touched;
    if constexpr (WALLS) touched = wall_car_touches(bx, nd, disc, nw, hdr);
    else touched = nd > 0 && cor_car_touches(bx, nd, disc);
    if (touched) {
      int* cs = col_seg.data() + (size_t)n * 2 * COR_MAXSEG;
      double s0[4] = {0, 0, 0, 0};
      auto record = [&](int q, int sx, int sy, int ex, int ey, double ax, double ay, double bx2, double by) {
        cs[2 * q] = (sx + 1) | ((sy + 1) << 16);
        cs[2 * q + 1] = (ex + 1) | ((ey + 1) << 16);
        if (q == 0) { s0[0] = ax; s0[1] = ay; s0[2] = bx2; s0[3] = by; }
      };
      const int* line = r_cells + (size_t)i * COR_CELL_CAP;
      int cnt;
      if constexpr (WALLS) cnt = wall_car_scan(m, base.min_width, line, bx, nd, disc, nw, hdr, wtab, record);
      else cnt = cor_car_scan(m, base.min_width, line, bx, nd, disc, record);
      if (cnt < 0) over = true;
      else if (cnt <= 1) cor_forced_seg(g, i, cnt, s0, base.sm, o);
      col_cnt[n] = cnt < 0 ? cnt : cnt + 1000;
    } else {
      const int cnt = r_nseg[i];
      if (cnt <= 1)
        for (int k = 0; k < COR_WPC; ++k) o[k] = r_wpc[(size_t)i * COR_WPC + k];
      col_cnt[n] = cnt;
    }
  }
  auto cnt = [&](int c) { const int q = col_cnt[c]; return q >= 1000 ? q - 1000 : q; };
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
      const double* sg = r_segs + (size_t)cor_wp(g, wp + c) * 4 * COR_MAXSEG + 4 * k;
      for (int j = 0; j < 4; ++j) s[j] = sg[j];
    }
  };
  const int verdict = cnt(0) == 0 ? COR_ROW_BLOCKED : (over ? COR_ROW_OVERFLOW : COR_ROW_OK);
  for (int n = 0; n < N; ++n) {
    double u = std::nan(""), l = std::nan("");
    if (verdict == COR_ROW_OK) cor_select_car_one(g, wp, n, base.sm, cnt, forced, seg, &u, &l);
    ub[n] = u;
    lb[n] = l;
  }
  return verdict;
}

// the disc accessor of every column when the columns share the car's list
inline auto plain_col_disc(const int* dsc) {
  return [dsc](int) { return [dsc](int j) { return dsc + 3 * j; }; };
}

}  // namespace mpmpc
