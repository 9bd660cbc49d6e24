// CPU twin of the lookahead kernels: K0h (mpmpc_mover_horizon_kernel) and K0c<WALLS, LEAD> (mpmpc_car_corridor_kernel) - the
// same lookahead_core.hpp code (and obstacle_motion_core / corridor_core / wall_core beneath it), one car, one mover, one
// column after the other.  Built by tests/test_lookahead.py with the flags of tests/test_movers.py's twin.
#include <cmath>
#include <cstdint>
#include <vector>

#include "lookahead_core.hpp"
#include "wall_core.hpp"

using namespace mpmpc;

// (the car's view of the path - route == NULL: the one path - is the kernels' own: route_view, corridor_core.hpp)

extern "C" {

// Validation of mpmpc_rollout_set_lookahead (the library calls the same function): 0 or -1 (E_ARG).
int look_emu_check(int n_wp, int path_n_wp, const double* seg_time, int max_lead) {
  const char* why = "";
  return look_check_setting(n_wp, path_n_wp, seg_time, max_lead, &why);
}

long long look_emu_table_bytes(long long movers, int N) { return look_table_bytes(movers, N); }

// lead [B][N] of B cars at local waypoints wp_id (K0h's first half)
void look_emu_leads(int B, int N, const int32_t* wp_id, const int32_t* route, int n_wp, int circular, const double* seg_time,
                    double Ts, int max_lead, int32_t* lead) {
  for (int b = 0; b < B; ++b) {
    const RouteView v = route_view(route, b, n_wp, circular);
    const PathGeom g{nullptr, nullptr, nullptr, nullptr, v.n(), v.circular(), nullptr};
    const double* seg = seg_time + v.first;
    look_leads(N, Ts, max_lead, [&](int c) { return seg[look_seg_row(g, wp_id[b], c)]; }, lead + (long)b * N);
  }
}

// tab [movers][N][3]: the fleet's movers (CSR offsets moff [B + 1]; params [n][4]) over their cars' horizons at rollout step
// k, column c of car b at step k + lead[b][c] (K0h's second half); cum / x / y / psi are the path table's global rows
void look_emu_discs(int B, int N, const int32_t* moff, const int32_t* kind, const int32_t* radius, const double* params,
                    int64_t k, int64_t step0, const int32_t* lead, const int32_t* route, int map_h, int map_w, double ox,
                    double oy, double res, int n_wp, const double* cum, const double* x, const double* y, const double* psi,
                    int circular, int32_t* tab) {
  const MapView m{nullptr, map_h, map_w, ox, oy, res};
  std::vector<double> trig((size_t)n_wp * COR_TRIG);
  for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
  for (int b = 0; b < B; ++b) {
    const RouteView v = route_view(route, b, n_wp, circular);
    const MoverPath p = route_path(MoverPath{cum, x, y, trig.data(), n_wp, COR_TRIG, circular}, v);
    for (long j = moff[b]; j < moff[b + 1]; ++j)
      for (int c = 0; c < N; ++c) {
        const double* a = params + (size_t)MOV_PARAMS * j;
        int d[3];
        mov_disc(m, p, kind[j], radius[j], a[0], a[1], a[2], a[3], (long long)k + lead[(long)b * N + c], (long long)step0, d);
        for (int t = 0; t < 3; ++t) tab[(j * N + c) * 3 + t] = d[t];
      }
  }
}

// K0a's base build on the grid (per route), then K0c<WALLS, LEAD>'s rows for n_start cars: waypoint wp_id[b] (local), discs the
// CSR lists off / discs (the lists K0c plans from at the step itself; off may be NULL: none), walls the CSR lists woff / walls,
// route as above.  look_car == NULL: no lookahead (the plain rows).  Else look_car [n_start + 1][2] = {first mover of the car in
// the fleet's list, first mover slot in the car's own list} and hz [movers][N][3] = look_emu_discs' table: column c reads
// look_col_disc.  ub / lb [n_start x N] (NaN rows unless the verdict is COR_ROW_OK), flag [n_start] = COR_ROW_*.  Returns 0,
// 1 / 2 when the base build overflows, 3 when a wall does not fit the table.
int look_emu_rows(int h, int w, const int8_t* grid, double ox, double oy, double res, int n_wp, const double* x, const double* y,
                  const double* psi, const double* ds_next, int circular, const double* bub, const double* blb, int N,
                  double min_width, double sm, int n_start, const int32_t* wp_id, const int32_t* off, const int32_t* discs,
                  const int32_t* woff, const int32_t* walls, const int32_t* route, const int32_t* look_car, const int32_t* hz,
                  double* ub, double* lb, int32_t* flag) {
  const long n_walls = woff ? woff[n_start] : 0;
  std::vector<int32_t> whdr((size_t)WALL_HDR * n_walls + 1), wtab;
  wtab.assign((size_t)wall_layout(n_walls, walls, whdr.data()) + 1, 0);
  for (long j = 0; j < n_walls; ++j)
    if (!wall_raster(walls + 4 * j, whdr.data() + WALL_HDR * j, wtab.data())) return 3;
  MapView m{grid, h, w, ox, oy, res};
  std::vector<double> trig((size_t)n_wp * COR_TRIG);
  for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
  std::vector<double> segs((size_t)n_wp * 4 * COR_MAXSEG, 0.0), wpc((size_t)n_wp * COR_WPC, 0.0);
  std::vector<int> nseg(n_wp), cells((size_t)n_wp * COR_CELL_CAP), box((size_t)n_wp * COR_LINE_BOX);
  std::vector<char> built(n_wp, 0);
  std::vector<double> col_o((size_t)N * COR_WPC);
  std::vector<int> col_seg((size_t)N * 2 * COR_MAXSEG), col_cnt(N);
  for (int b = 0; b < n_start; ++b) {
    const RouteView v = route_view(route, b, n_wp, circular);
    const PathGeom g = route_geom(PathGeom{x, y, psi, ds_next, n_wp, circular, trig.data()}, v);
    double* const r_segs = segs.data() + v.first * 4 * COR_MAXSEG;
    double* const r_wpc = wpc.data() + v.first * COR_WPC;
    int* const r_nseg = nseg.data() + v.first;
    int* const r_cells = cells.data() + v.first * COR_CELL_CAP;
    int* const r_box = box.data() + v.first * COR_LINE_BOX;
    if (!built[v.first]) {                         // K0a on the car's route
      built[v.first] = 1;
      for (int i = 0; i < v.n(); ++i) {
        int ux, uy, lx, ly;
        cor_w2m(m, bub[2 * (v.first + i)], bub[2 * (v.first + i) + 1], ux, uy);
        cor_w2m(m, blb[2 * (v.first + i)], blb[2 * (v.first + i) + 1], lx, ly);
        int* c = r_cells + (size_t)i * COR_CELL_CAP;
        const int n = cor_line_cells(ux, uy, lx, ly, c, COR_CELL_CAP);
        if (n > COR_CELL_CAP) return 1;
        const int cnt = cor_scan_cells(m, ux, uy, lx, ly, min_width, n, [&](int k, int& cx, int& cy) { cor_unpack_cell(c[k], cx, cy); },
                                       [&](int k) { int cx, cy; cor_unpack_cell(c[k], cx, cy); return cor_cell_free(m, cx, cy); },
                                       r_segs + (size_t)i * 4 * COR_MAXSEG);
        if (cnt < 0) return 2;
        r_nseg[i] = cnt;
        cor_line_box(c, n, (ux + 1) | ((uy + 1) << 16), (lx + 1) | ((ly + 1) << 16), r_box + (size_t)i * COR_LINE_BOX);
      }
      for (int i = 0; i < v.n(); ++i)
        if (r_nseg[i] <= 1) cor_forced(g, r_segs, r_nseg, i, sm, r_wpc + (size_t)i * COR_WPC);
    }
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    const int32_t* dsc = discs + 3L * d0;
    int ns = 0, nm = 0;
    const int32_t* car_hz = nullptr;
    if (look_car) {
      const int m0 = look_car[2 * b];
      ns = look_car[2 * b + 1];
      nm = look_car[2 * b + 2] - m0;
      car_hz = hz + (long)m0 * N * 3;
    }
    const int w0 = woff ? woff[b] : 0, nw = woff ? woff[b + 1] - w0 : 0;
    auto hdr = [&](int j) { return (const int*)(whdr.data() + (size_t)WALL_HDR * (w0 + j)); };
    const int wp = wp_id[b] + 1;
    bool over = false;
    for (int n = 0; n < N; ++n) {              // K0c, one car; column n in its own world
      auto disc = [&](int j) { return look_car ? look_col_disc(dsc, j, ns, nm, car_hz, N, n) : (const int*)(dsc + 3 * j); };
      const int i = cor_wp(g, wp + n);
      const int* bx = r_box + (size_t)i * COR_LINE_BOX;
      double* o = col_o.data() + (size_t)n * COR_WPC;
      if (wall_car_touches(bx, nd, disc, nw, hdr)) {
        int* cs = col_seg.data() + (size_t)n * 2 * COR_MAXSEG;
        double s0[4] = {0, 0, 0, 0};
        const int cnt = wall_car_scan(m, min_width, r_cells + (size_t)i * COR_CELL_CAP, bx, nd, disc, nw, hdr, wtab.data(),
                                      [&](int q, int sx, int sy, int ex, int ey, double ax, double ay, double bx2, double by) {
                                        cs[2 * q] = (sx + 1) | ((sy + 1) << 16);
                                        cs[2 * q + 1] = (ex + 1) | ((ey + 1) << 16);
                                        if (q == 0) { s0[0] = ax; s0[1] = ay; s0[2] = bx2; s0[3] = by; }
                                      });
        if (cnt < 0) over = true;
        else if (cnt <= 1) cor_forced_seg(g, i, cnt, s0, sm, o);
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
      if (verdict == COR_ROW_OK) cor_select_car_one(g, wp, n, sm, cnt, forced, seg, &u, &l);
      ub[(size_t)b * N + n] = u;
      lb[(size_t)b * N + n] = l;
    }
    flag[b] = verdict;
  }
  return 0;
}

}  // extern "C"
