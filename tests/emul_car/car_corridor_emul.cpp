// CPU twin of K0a's line cache and of K0c (mpmpc_car_corridor_kernel): the same corridor_core.hpp code, one car and
// one column after the other (car_rows.hpp).  Built by tests/emul/Makefile (`make car_corridor`), loaded by tests/twins.py.
#include <cstdint>

#include "car_rows.hpp"

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
  TwinBase base(h, w, grid, ox, oy, res, n_wp, x, y, psi, ds_next, circular, bub, blb, min_width, sm);
  const RouteView v = route_view(nullptr, 0, n_wp, circular);
  if (int rc = base.build(v)) return rc;
  auto no_wall = [](int) { return (const int*)nullptr; };
  for (int b = 0; b < n_start; ++b)
    flag[b] = car_rows<false>(base, v, wp_id[b], N, off[b + 1] - off[b], plain_col_disc(discs + 3L * off[b]), 0, no_wall, nullptr,
                              ub + (size_t)b * N, lb + (size_t)b * N);
  return 0;
}

}  // extern "C"
