// CPU twin of the traffic lookahead kernels: K3t (mpmpc_plan_track_kernel), K0t with its occupants (mpmpc_traffic_kernel<true>),
// K0ht (mpmpc_traffic_horizon_kernel) and K0c<WALLS, true, true> (mpmpc_car_corridor_kernel) - the same
// traffic_lookahead_core.hpp code (and lookahead_core / traffic_core / corridor_core / wall_core beneath it), one car, one
// stage, one column after the other; K0c's rows: car_rows.hpp.  Built by tests/emul/Makefile (`make traffic_lookahead`), loaded by
// tests/twins.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../emul_car/car_rows.hpp"
#include "traffic_lookahead_core.hpp"

using namespace mpmpc;

// (the car's view of the path - route == NULL: the one path - is the kernels' own: route_view, corridor_core.hpp)

extern "C" {

long long tlk_emu_table_bytes(long long B, int S, int N) { return tlk_table_bytes(B, S, N); }
long long tlk_emu_budget() { return LOOK_TABLE_BUDGET; }

// K3t: the tracks of B plans z [B][5 N + 3]; wp_id / status / alive: the state after the step; x / y / psi: global rows
void tlk_emu_tracks(int B, int N, const double* z, const int32_t* wp_id, const int32_t* status, const int32_t* alive,
                    const int32_t* route, int n_wp, int circular, const double* x, const double* y, const double* psi, int map_h,
                    int map_w, double ox, double oy, double res, int32_t* valid, int32_t* cells, double* tm) {
  const MapView m{nullptr, map_h, map_w, ox, oy, res};
  std::vector<double> trig((size_t)n_wp * COR_TRIG);
  for (int i = 0; i < n_wp; ++i) cor_trig_row(psi[i], trig.data() + (size_t)i * COR_TRIG);
  for (int n = 0; n < B; ++n) {
    const RouteView v = route_view(route, n, n_wp, circular);
    const double* zn = z + (size_t)(5 * N + 3) * n;
    valid[n] = tlk_valid(alive[n], status[n]) ? 1 : 0;
    for (int j = 0; j <= N; ++j) {
      const long long w = tlk_stage_row(wp_id[n], j, v.n(), v.circular() != 0, v.first);
      tlk_stage_cell(m, x[w], y[w], trig[w * COR_TRIG], trig[w * COR_TRIG + 1], zn[3 * j], cells + ((size_t)n * (N + 1) + j) * 2);
    }
    tlk_times(N, zn, tm + (size_t)n * (N + 1));
  }
}

// ... and tm alone the way K3t forms it: chunks of 64 keys, an inclusive scan of shifted maxima in each, the carry between them
void tlk_emu_times_scan(int N, const double* z, double* tm) {
  double carry = 0.0;
  for (int j0 = 0; j0 <= N; j0 += 64) {
    double v[64], before[64];
    for (int l = 0; l < 64; ++l) v[l] = j0 + l <= N ? tlk_time_key(j0 + l, z[3 * (j0 + l) + 2]) : -HUGE_VAL;
    for (int s = 1; s < 64; s <<= 1) {
      for (int l = 0; l < 64; ++l) before[l] = l >= s ? v[l - s] : 0.0;
      for (int l = s; l < 64; ++l) v[l] = tlk_time_max(before[l], v[l]);
    }
    for (int l = 0; l < 64; ++l) {
      v[l] = tlk_time_max(carry, v[l]);
      if (j0 + l <= N) tm[j0 + l] = v[l];
    }
    carry = v[63];
  }
}

// K0t with its occupants: out [B][S][3], who [B][S]
int tlk_emu_slots(int B, const double* pose, const int32_t* alive, const int32_t* group, const int32_t* radius, int S,
                  int range_cells, int map_h, int map_w, double ox, double oy, double res, int32_t* out, int32_t* who) {
  const MapView m{nullptr, map_h, map_w, ox, oy, res};
  std::vector<int32_t> dense((size_t)B), goff((size_t)B + 1), members((size_t)B);
  if (tr_layout(B, group, dense.data(), goff.data(), members.data()) < 0) return -1;
  for (int b = 0; b < B; ++b)
    tr_slots_car(m, pose, alive, dense.data(), radius, goff.data(), members.data(), S, range_cells, b, out + 3L * S * b,
                 who + (long)S * b);
  return 0;
}

// K0ht: tz [B][S][N][3] from who [B][S], the slots' discs of step k [B][S][3], lead [B][N] and the tracks
void tlk_emu_discs(int B, int S, int N, double Ts, int map_h, int map_w, const int32_t* who, const int32_t* discs_k,
                   const int32_t* lead, const int32_t* valid, const int32_t* cells, const double* tm, int32_t* tz) {
  const MapView m{nullptr, map_h, map_w, 0.0, 0.0, 1.0};
  for (long b = 0; b < B; ++b)
    for (int t = 0; t < S; ++t)
      for (int c = 0; c < N; ++c)
        tlk_disc(m, discs_k + (b * S + t) * 3, who[b * S + t], lead[b * N + c], Ts, N, valid, cells, tm, tz + ((b * S + t) * N + c) * 3);
}

// K0a's base build on the grid (per route), then the rows of K0c's traffic instantiations for n_start cars: waypoint wp_id[b]
// (local), discs the CSR lists off / discs (the lists K0c plans from at the step itself), walls the CSR lists woff / walls,
// route as above.  look_car [n_start + 1][2] = {first mover of the car in the fleet's list, first mover slot in the car's own
// list} and hz [movers][N][3] (K0h's table; no movers: all zero / NULL); S traffic slots at the end of every list and tz
// [n_start][S][N][3] (K0ht's table): column c reads tlk_col_disc.  tz == NULL: look_col_disc alone (the mover-only LEAD rows),
// look_car == NULL as well: the plain rows.  ub / lb [n_start x N] (NaN rows unless the verdict is COR_ROW_OK), flag [n_start] =
// COR_ROW_*.  Returns 0, 1 / 2 when the base build overflows, 3 when a wall does not fit the table.
int tlk_emu_rows(int h, int w, const int8_t* grid, double ox, double oy, double res, int n_wp, const double* x, const double* y,
                 const double* psi, const double* ds_next, int circular, const double* bub, const double* blb, int N,
                 double min_width, double sm, int n_start, const int32_t* wp_id, const int32_t* off, const int32_t* discs,
                 const int32_t* woff, const int32_t* walls, const int32_t* route, const int32_t* look_car, const int32_t* hz, int S,
                 const int32_t* tz, double* ub, double* lb, int32_t* flag) {
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
      car_hz = hz ? hz + (long)m0 * N * 3 : nullptr;
    }
    const int ts = S < nd ? S : nd;
    const int32_t* tzb = tz ? tz + (long)b * S * N * 3 : nullptr;
    const int w0 = woff ? woff[b] : 0, nw = woff ? woff[b + 1] - w0 : 0;
    auto hdr = [&](int j) { return (const int*)(ws.hdr.data() + (size_t)WALL_HDR * (w0 + j)); };
    auto col_disc = [&](int n) {                                   // column n in its own world
      return [=](int j) {
        if (tz) return tlk_col_disc(dsc, j, ns, nm, car_hz, nd, ts, tzb, N, n);
        return look_car ? look_col_disc(dsc, j, ns, nm, car_hz, N, n) : (const int*)(dsc + 3 * j);
      };
    };
    flag[b] = car_rows<true>(base, v, wp_id[b], N, nd, col_disc, nw, hdr, ws.tab.data(), ub + (size_t)b * N, lb + (size_t)b * N);
  }
  return 0;
}

}  // extern "C"
