// CPU twin of K0k, the KEEP instantiations of K0c (mpmpc_car_corridor_kernel<WALLS, false, false, true>): the same
// commitment_core.hpp / corridor_core.hpp / wall_core.hpp code as the kernel, one car and one column after the other, on the base
// build of tests/emul_car/car_rows.hpp (TwinBase, Walls).  Built by tests/emul_commitment/Makefile, loaded by
// tests/commitment_twin.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "car_rows.hpp"
#include "commitment_core.hpp"

using namespace mpmpc;

namespace {

// a world to build rows in: the grid (a copy) and K0a's base build of the one path on it
struct Twin {
  std::vector<int8_t> grid;
  std::vector<double> x, y, psi, ds, bub, blb;
  TwinBase base;
  RouteView v;
  int N;
  Twin(int h, int w, const int8_t* g, double ox, double oy, double res, int n_wp, const double* x_, const double* y_, const double* psi_,
       const double* ds_, int circular, const double* bub_, const double* blb_, int N, double min_width, double sm)
      : grid(g, g + (size_t)h * w), x(x_, x_ + n_wp), y(y_, y_ + n_wp), psi(psi_, psi_ + n_wp), ds(ds_, ds_ + n_wp),
        bub(bub_, bub_ + 2 * (size_t)n_wp), blb(blb_, blb_ + 2 * (size_t)n_wp),
        base(h, w, grid.data(), ox, oy, res, n_wp, x.data(), y.data(), psi.data(), ds.data(), circular, bub.data(), blb.data(), min_width, sm),
        v(route_view(nullptr, 0, n_wp, circular)), N(N) {}
};

// K0c<WALLS, false, false, true> for one car at local waypoint wp_id: the column sources as car_rows builds them (car_rows.hpp),
// then cmt_select_car_one per column, the new memory and the three counts.  ub / lb NaN unless the verdict is COR_ROW_OK.
template <bool WALLS, class Hdr>
int keep_rows(const TwinBase& base, const RouteView& v, int wp_id, int N, int nd, const int* dsc, int nw, Hdr hdr, const int* wtab,
              double keep, const int32_t* mem_wp, const double* mem_rows, double* ub, double* lb, int32_t* new_wp, double* new_rows,
              int32_t* counts, long stride) {
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
  auto disc = [dsc](int j) { return dsc + 3 * j; };
  for (int n = 0; n < N; ++n) {
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
  auto mwp = [&](int c) { return (int)mem_wp[c]; };
  auto mem = [&](int i, double* mm) {
    const int c = cmt_find(N, mwp, i);
    if (c < 0) return false;
    for (int k = 0; k < COR_WPC; ++k) mm[k] = mem_rows[(size_t)c * COR_WPC + k];
    return true;
  };
  const int verdict = cnt(0) == 0 ? COR_ROW_BLOCKED : (over ? COR_ROW_OVERFLOW : COR_ROW_OK);
  for (int n = 0; n < N; ++n) {
    double o[COR_WPC] = {0, 0, 0, 0, 0, 0};
    int how = 0;
    if (verdict == COR_ROW_OK) cmt_select_car_one(g, wp, n, base.sm, keep, cnt, forced, seg, mem, o, &how);
    ub[n] = verdict == COR_ROW_OK ? o[0] : std::nan("");
    lb[n] = verdict == COR_ROW_OK ? o[1] : std::nan("");
    const int i = cor_wp(g, wp + n);
    const bool held = verdict == COR_ROW_OK && cnt(n) >= 1;
    new_wp[n] = held ? i : CMT_EMPTY;
    for (int k = 0; k < COR_WPC; ++k) new_rows[(size_t)n * COR_WPC + k] = held ? o[k] : 0.0;
    counts[0] += how & CMT_KEPT ? 1 : 0;
    counts[stride] += how & CMT_SWITCHED ? 1 : 0;
    const int c = cmt_find(N, mwp, i);
    if (c >= 0 && cmt_moved(o[0], o[1], mem_rows[(size_t)c * COR_WPC], mem_rows[(size_t)c * COR_WPC + 1])) ++counts[2 * stride];
  }
  return verdict;
}

}  // namespace

extern "C" {

// validation of mpmpc_rollout_set_commitment (the library calls the same function): 0 or -1 (E_ARG)
int cmt_emu_check(int B, int max_batch, int N, const double* keep, const int32_t* mem_wp, const double* mem_rows) {
  const char* why = "";
  return cmt_check(B, max_batch, N, keep, mem_wp, mem_rows, &why);
}
long long cmt_emu_bytes(long long B, int N) { return cmt_bytes(B, N); }
long long cmt_emu_budget() { return CMT_BUDGET; }

// the world: K0a's base build of the one path on the grid.  NULL when the base build overflows.
void* cmt_twin_new(int h, int w, const int8_t* grid, double ox, double oy, double res, int n_wp, const double* x, const double* y,
                   const double* psi, const double* ds_next, int circular, const double* bub, const double* blb, int N, double min_width,
                   double sm) {
  Twin* t = new Twin(h, w, grid, ox, oy, res, n_wp, x, y, psi, ds_next, circular, bub, blb, N, min_width, sm);
  if (t->base.build(t->v)) { delete t; return nullptr; }
  return t;
}
void cmt_twin_free(void* t) { delete (Twin*)t; }

// One step of K0c<WALLS, false, false, true> for B cars at the local waypoints wp_id[b]: discs off / discs (CSR; off may be
// NULL: none), walls woff / walls (CSR; woff NULL: the instantiation without walls), keep [B], the memory mem_wp [B x N] /
// mem_rows [B x N x 6] it reads.  Out: ub / lb [B x N] (NaN unless the verdict is COR_ROW_OK), flag [B] = COR_ROW_*, the
// memory it writes new_wp / new_rows, and counts [3][B], which it ADDS to.  Returns 0, or 3 when a wall does not fit the table.
int cmt_twin_rows(void* tw, int B, const int32_t* wp_id, const int32_t* off, const int32_t* discs, const int32_t* woff,
                  const int32_t* walls, const double* keep, const int32_t* mem_wp, const double* mem_rows, double* ub, double* lb,
                  int32_t* flag, int32_t* new_wp, double* new_rows, int32_t* counts) {
  const Twin& t = *(const Twin*)tw;
  const int N = t.N;
  Walls ws(woff ? woff[B] : 0, walls);
  if (!ws.ok) return 3;
  for (int b = 0; b < B; ++b) {
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    const size_t at = (size_t)b * N;
    if (woff) {
      const int w0 = woff[b], nw = woff[b + 1] - w0;
      auto hdr = [&](int j) { return (const int*)(ws.hdr.data() + (size_t)WALL_HDR * (w0 + j)); };
      flag[b] = keep_rows<true>(t.base, t.v, wp_id[b], N, nd, discs + 3L * d0, nw, hdr, ws.tab.data(), keep[b], mem_wp + at,
                                mem_rows + at * COR_WPC, ub + at, lb + at, new_wp + at, new_rows + at * COR_WPC, counts + b, B);
    } else {
      auto hdr = [](int) { return (const int*)nullptr; };
      flag[b] = keep_rows<false>(t.base, t.v, wp_id[b], N, nd, discs + 3L * d0, 0, hdr, nullptr, keep[b], mem_wp + at,
                                 mem_rows + at * COR_WPC, ub + at, lb + at, new_wp + at, new_rows + at * COR_WPC, counts + b, B);
    }
  }
  return 0;
}

}  // extern "C"
