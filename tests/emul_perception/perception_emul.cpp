// CPU twin of K0s (mpmpc_perception_kernel): the same perception_core.hpp code (and lidar_core / wall_core beneath it), one car,
// one slot and one cell after the other, the host's libm for the atan2 of a cell's interval.  No sift, no queue, no enclosure:
// every cell of the window is asked directly.  Built by tests/emul/Makefile (`make perception`), loaded by tests/twins.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "perception_core.hpp"

using namespace mpmpc;

extern "C" {

// the argument checks of mpmpc_perception_scan (the library calls the same functions): 0 or -1 (E_ARG)
int per_emu_check_scan(int height, int width, const int8_t* data, double res, int B, const double* pose, const int32_t* off,
                       const int32_t* discs, const int32_t* woff, const int32_t* walls, int n_beams, const double* angles,
                       double range_m, const double* out) {
  const char* why = "";
  if (int rc = lid_check_scan(height, width, data, res, B, pose, off, discs, n_beams, angles, range_m, out, &why)) return rc;
  return woff ? wall_check_lists(B, woff, walls, width, height, &why) : 0;
}
// ... of mpmpc_rollout_set_perception
int per_emu_check_setting(int n_beams, const double* angles, double range_m, int hold, double res) {
  const char* why = "";
  return per_check_setting(n_beams, angles, range_m, hold, res, &why);
}

// ranges [B][n_beams], disc_seen [B], wall_seen [B].  Returns the check's code, or 1 when a wall does not fit the table.
int per_emu_scan(int height, int width, const int8_t* data, double ox, double oy, double res, int B, const double* pose,
                 const int32_t* off, const int32_t* discs, const int32_t* woff, const int32_t* walls, int n_beams,
                 const double* angles, double range_m, double* ranges, uint64_t* disc_seen, uint32_t* wall_seen) {
  if (int rc = per_emu_check_scan(height, width, data, res, B, pose, off, discs, woff, walls, n_beams, angles, range_m, ranges)) return rc;
  const long n_walls = woff ? woff[B] : 0;
  std::vector<int32_t> hdr((size_t)WALL_HDR * n_walls + 1, 0), tab;
  tab.assign((size_t)wall_layout(n_walls, walls, hdr.data()) + 1, 0);
  for (long j = 0; j < n_walls; ++j)
    if (!wall_raster(walls + 4 * j, hdr.data() + WALL_HDR * j, tab.data())) return 1;
  const MapView m{data, height, width, ox, oy, res};
  std::vector<int> best((size_t)n_beams);
  for (int b = 0; b < B; ++b) {
    double* out = ranges + (long)b * n_beams;
    disc_seen[b] = 0;
    wall_seen[b] = 0;
    const double psi = pose[3L * b + 2];
    int cx, cy;
    if (!lid_sensor_cell(m, pose[3L * b], pose[3L * b + 1], psi, &cx, &cy)) {
      for (int k = 0; k < n_beams; ++k) out[k] = std::nan("");
      continue;
    }
    const LidWindow w = lid_window(m, cx, cy, range_m);
    const int d0 = off ? off[b] : 0, nd = off ? off[b + 1] - d0 : 0;
    const int w0 = woff ? woff[b] : 0, nw = woff ? woff[b + 1] - w0 : 0;
    auto disc = [&](int q) { return discs + 3L * (d0 + q); };
    auto whdr = [&](int q) { return (const int*)(hdr.data() + (long)WALL_HDR * (w0 + q)); };
    for (int k = 0; k < n_beams; ++k) best[k] = LID_NONE;
    for (int j = w.j0; j <= w.j1; ++j)
      for (int i = w.i0; i <= w.i1; ++i) {
        if (!wall_lid_occupied(m, i, j, nd, disc, nw, whdr, tab.data())) continue;
        int d2;
        if (!lid_in_range(i - cx, j - cy, w.lim, &d2)) continue;
        double mn, mx;
        if (!lid_cell_interval(i - cx, j - cy, psi, &mn, &mx)) continue;
        for (int k = lid_first_beam(angles, n_beams, mn); k < n_beams && angles[k] <= mx; ++k)
          best[k] = d2 < best[k] ? d2 : best[k];
      }
    for (int k = 0; k < n_beams; ++k) out[k] = lid_range(best[k], res, range_m);
    for (int j = w.j0; j <= w.j1; ++j)
      for (int i = w.i0; i <= w.i1; ++i) {
        int d2;
        if (!lid_in_range(i - cx, j - cy, w.lim, &d2)) continue;
        bool asked = false, owns = false;
        auto cell_owns = [&]() {
          if (!asked) { owns = per_cell_owns_beam(i - cx, j - cy, d2, psi, angles, n_beams, best.data()); asked = true; }
          return owns;
        };
        for (int q = 0; q < nd; ++q)
          if (disc(q)[2] > 0 && cor_in_disc(i, j, disc(q)) && cell_owns()) disc_seen[b] |= (uint64_t)1 << q;
        for (int q = 0; q < nw; ++q)
          if (wall_on(i, j, whdr(q), tab.data()) && cell_owns()) wall_seen[b] |= (uint32_t)1 << q;
      }
  }
  return 0;
}

// the knowledge law (per_step) for one car over a sequence of T steps: seen masks and scanned flags per step; `reset_at` >= 0: every
// slot is reset to -1 in front of that step.  Outputs per step: disc_known [T], wall_known [T]; and the final first / last arrays.
void per_emu_sequence(int T, int n_disc, int n_static, int n_mover, int n_wall, const int32_t* scanned, const uint64_t* disc_seen,
                      const uint32_t* wall_seen, int k0, int hold, int reset_at, uint64_t* disc_known, uint32_t* wall_known,
                      int32_t* disc_first, int32_t* disc_last, int32_t* wall_first, int32_t* wall_last) {
  auto forget = [&]() {
    for (int q = 0; q < COR_MAX_DISCS; ++q) disc_first[q] = disc_last[q] = -1;
    for (int q = 0; q < COR_MAX_WALLS; ++q) wall_first[q] = wall_last[q] = -1;
  };
  forget();
  for (int t = 0; t < T; ++t) {
    if (t == reset_at) forget();
    per_step(n_disc, n_static, n_mover, n_wall, scanned[t] != 0, disc_seen[t], wall_seen[t], k0 + t, hold, disc_first, disc_last,
             wall_first, wall_last, disc_known + t, wall_known + t);
  }
}

// the perceived lists of one car (per_disc, per_wall): discs [n_disc][3] -> out_discs, raw walls [n_wall][4] -> out_hdr [n_wall][6]
void per_emu_lists(int n_disc, const int32_t* discs, uint64_t disc_known, int n_wall, const int32_t* walls, uint32_t wall_known,
                   int32_t* out_discs, int32_t* out_hdr) {
  for (int q = 0; q < n_disc; ++q) per_disc(((disc_known >> q) & 1) != 0, discs + 3 * q, out_discs + 3 * q);
  std::vector<int32_t> hdr((size_t)WALL_HDR * n_wall + 1, 0);
  wall_layout(n_wall, walls, hdr.data());
  for (int q = 0; q < n_wall; ++q) per_wall(((wall_known >> q) & 1) != 0, hdr.data() + WALL_HDR * q, out_hdr + WALL_HDR * q);
}

}  // extern "C"
