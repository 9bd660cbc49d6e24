// CPU twin of mpmpc_path_build: the host part is the library's own (path_core.hpp: path_check_build, path_rows), the
// width is the per-line code of K0p (path_line_min, path_side_reduce) run in a loop, the walls' table the host's
// wall_raster.  Built by tests/emul/Makefile (`make path`), loaded by tests/twins.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "path_core.hpp"

using namespace mpmpc;

extern "C" {

// mpmpc_path_count; -1 for arguments it refuses
int path_emu_count(int n, const double* corners, double r_p, int sd) {
  const char* why = "";
  if (path_check_route(n, corners, r_p, sd, &why)) return -1;
  const long long c = path_wp_count(n, corners, r_p, sd);
  return c > 2147483647LL ? 2147483647 : (int)c;
}

// numpy's mean of n <= 127 terms, as step 2 takes it
double path_emu_mean(const double* a, int n) { return path_mean(a, n); }

// mpmpc_path_build without the device: the same arguments, outputs and return codes (-1: refused; a wall that does not
// fit its table: -1 as well)
int path_emu_build(int height, int width, const int8_t* data, double ox, double oy, double res, int P, const int32_t* coff,
                   const double* corners, const double* spec, const int32_t* ispec, const int32_t* doff, const int32_t* discs,
                   const int32_t* woff, const int32_t* walls, int cap, int32_t* n_wp, int32_t* status, double* x, double* y,
                   double* psi, double* kappa, double* ds_next, double* ub, double* lb, double* border, double* length) {
  const char* why = "";
  const bool outputs = n_wp && status && x && y && psi && kappa && ds_next && ub && lb && border && length;
  if (int rc = path_check_build(height, width, data, ox, oy, res, P, coff, corners, spec, ispec, doff, discs, woff, walls, cap,
                                outputs, &why))
    return rc;
  const MapView m{data, height, width, ox, oy, res};
  std::vector<int32_t> hdr, table;
  if (woff) {
    hdr.assign((size_t)WALL_HDR * woff[P] + 1, 0);
    table.assign((size_t)wall_layout(woff[P], walls, hdr.data()) + 1, 0);
    for (long j = 0; j < woff[P]; ++j)
      if (!wall_raster(walls + 4 * j, hdr.data() + WALL_HDR * j, table.data())) return -1;
  }
  const double nan = std::nan("");
  const size_t all = (size_t)P * (size_t)cap;
  for (double* a : {x, y, psi, kappa, ds_next, ub, lb})
    for (size_t k = 0; k < all; ++k) a[k] = nan;
  for (size_t k = 0; k < 4 * all; ++k) border[k] = nan;
  for (int p = 0; p < P; ++p) {
    PathRows t;
    const double mw = spec[2 * p + 1];
    const long long c = path_rows(m, coff[p + 1] - coff[p], corners + 2L * coff[p], spec[2 * p], mw, ispec[2 * p], ispec[2 * p + 1] != 0,
                                    cap, t);
    n_wp[p] = c > 2147483647LL ? 2147483647 : (int32_t)c;
    status[p] = c < 2 ? PATH_E_SHORT : c > cap ? PATH_E_CAP : PATH_OK;
    length[p] = nan;
    if (status[p] != PATH_OK) continue;
    length[p] = t.length;
    const int d0 = doff ? doff[p] : 0, nd = doff ? doff[p + 1] - d0 : 0;
    const int w0 = woff ? woff[p] : 0, nw = woff ? woff[p + 1] - w0 : 0;
    auto occupied = [&](int cx, int cy) {
      return wall_world_occupied(m, cx, cy, nd, [&](int q) { return discs + 3L * (d0 + q); }, nw,
                                 [&](int q) { return (const int*)(hdr.data() + (long)WALL_HDR * (w0 + q)); }, (const int*)table.data());
    };
    const size_t o = (size_t)p * (size_t)cap;
    for (int i = 0; i < n_wp[p]; ++i) {
      const int32_t* cell = t.cells.data() + (size_t)PATH_WP_INTS * i;
      x[o + i] = t.x[i]; y[o + i] = t.y[i]; psi[o + i] = t.psi[i]; kappa[o + i] = t.kappa[i]; ds_next[o + i] = t.ds_next[i];
      for (int side = 0; side < 2; ++side) {
        PathLineBest line[PATH_LINES];
        for (int l = 0; l < PATH_LINES; ++l) {
          int ex, ey;
          path_line_end(cell[2 + 2 * side], cell[3 + 2 * side], l, ex, ey);
          line[l] = path_line_min(m, t.x[i], t.y[i], cell[0], cell[1], ex, ey, mw, occupied);
          if (line[l].outside) status[p] = PATH_OUTSIDE;
        }
        double r[3];
        path_side_reduce(m, mw, cell[2 + 2 * side], cell[3 + 2 * side],
                         [&](int l, double& d, int& cx, int& cy) { d = line[l].d; cx = line[l].x; cy = line[l].y; }, r);
        (side == 0 ? ub : lb)[o + i] = side == 0 ? r[0] : -r[0];
        border[4 * (o + i) + 2 * side] = r[1];
        border[4 * (o + i) + 2 * side + 1] = r[2];
      }
    }
  }
  return 0;
}

}  // extern "C"
