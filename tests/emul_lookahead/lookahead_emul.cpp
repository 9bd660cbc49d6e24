// CPU twin of the lookahead kernels: K0h (mpmpc_mover_horizon_kernel) and K0c<WALLS, LEAD> (mpmpc_car_corridor_kernel) - the
// same lookahead_core.hpp code (and obstacle_motion_core / corridor_core / wall_core beneath it), one car, one mover, one
// column after the other; K0c's rows: car_rows.hpp.  Built by tests/emul/Makefile (`make lookahead`), loaded by tests/twins.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../emul_car/car_rows.hpp"
#include "lookahead_core.hpp"

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
  const Walls ws(woff ? woff[n_start] : 0, walls);
  if (!ws.ok) return 3;
  TwinBase base(h, w, grid, ox, oy, res, n_wp, x, y, psi, ds_next, circular, bub, blb, min_width, sm);
  for (int b = 0; b < n_start; ++b) {
    const RouteView v = route_view(route, b, n_wp, circular);
    if (int rc = base.build(v)) return rc;                         // K0a on the car's route
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
    auto hdr = [&](int j) { return (const int*)(ws.hdr.data() + (size_t)WALL_HDR * (w0 + j)); };
    auto col_disc = [&](int n) {                                   // column n in its own world
      return [=](int j) { return look_car ? look_col_disc(dsc, j, ns, nm, car_hz, N, n) : (const int*)(dsc + 3 * j); };
    };
    flag[b] = car_rows<true>(base, v, wp_id[b], N, nd, col_disc, nw, hdr, ws.tab.data(), ub + (size_t)b * N, lb + (size_t)b * N);
  }
  return 0;
}

}  // extern "C"
