// CPU twin of K0a's line cache and of K0c (mpmpc_car_corridor_kernel): the same corridor_core.hpp code, one car and
// one column after the other.  Built by tests/test_car_obstacles.py with the flags of tests/emul/Makefile.
#include <cmath>
#include <cstdint>
#include <vector>

#include "corridor_core.hpp"

using namespace mpmpc;

extern "C" {

// Validation of mpmpc_rollout_set_obstacles (the library calls the same function): 0, -1 (E_ARG) or -3 (E_STATE).
int car_emu_check(int B, int max_batch, const int32_t* off, const int32_t* discs, int built, int map_w, int map_h) {
  const char* why = "";
  return cor_check_obstacles(B, max_batch, off, discs, built != 0, map_w, map_h, &why);
}

// Base build (K0a: segments, forced rows, line cache) on the grid, then K0c's rows for n_start cars whose waypoint is
// wp_id[b] (row = update_path_constraints(wp_id[b] + 1, N, ...)) and whose discs are the CSR lists off / discs.
// ub / lb [n_start x N], flag[n_start] = COR_ROW_*.  Returns 0, or 1 / 2 when the base build overflows.
int car_emu_rows(int h, int w, const int8_t* grid, double ox, double oy, double res, int n_wp, const double* x,
                 const double* y, const double* psi, const double* ds_next, int circular, const double* bub,
                 const double* blb, int N, double min_width, double sm, int n_start, const int32_t* wp_id,
                 const int32_t* off, const int32_t* discs, double* ub, double* lb, int32_t* flag) {
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
  for (int b = 0; b < n_start; ++b) {        // K0c, one car
    const int* dsc = discs + 3L * off[b];
    const int nd = off[b + 1] - off[b];
    auto disc = [&](int j) { return dsc + 3 * j; };
    const int wp = wp_id[b] + 1;
    bool over = false;
    for (int n = 0; n < N; ++n) {
      const int i = cor_wp(g, wp + n);
      const int* bx = box.data() + (size_t)i * COR_LINE_BOX;
      double* o = col_o.data() + (size_t)n * COR_WPC;
      if (nd > 0 && cor_car_touches(bx, nd, disc)) {
        int* cs = col_seg.data() + (size_t)n * 2 * COR_MAXSEG;
        double s0[4] = {0, 0, 0, 0};
        const int cnt = cor_car_scan(m, min_width, cells.data() + (size_t)i * COR_CELL_CAP, bx, nd, disc,
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

}  // extern "C"
