// Perception of a car: which primitives of its TRUE world - the discs of corridor_core.hpp, the walls of wall_core.hpp - a lidar
// scan (lidar_core.hpp) saw, and what the car KNOWS of its world from the scans so far: the world its corridor is then built from.
// The reference's Map is "a wrapper around a potential obstacle detection algorithm ... incorporating LiDAR measurements"; here the
// detection is exact (a primitive is seen or it is not) and its memory is per primitive.  Scalar code that compiles for gfx950 (K0s,
// mpmpc_perception.hpp) and for the host (tests/emul_perception), like lidar_core.hpp.
//
// SLOTS.  A car has up to COR_MAX_DISCS disc slots - its combined list in the order mpmpc_rollout_obstacles returns it: static
// discs, then movers, then traffic slots - and up to COR_MAX_WALLS wall slots in the order of mpmpc_rollout_set_walls.  The base
// grid is always known: it is the prior map.
//
// SEEING (one scan: a pose, a true world W = grid + discs + walls):
//   1 best[b] is exactly steps 1 - 3 of lidar_core.hpp in W.  A pose that gives a NaN row sees nothing.
//   2 disc slot q (radius > 0) is SEEN iff there is a cell (i, j) and a beam b with: (i, j) in the clipped window,
//     cor_in_disc(i, j, disc q), lid_in_range, lid_cell_interval does not skip the cell, mn <= angles[b] <= mx, and
//     d2 == best[b] - the FINAL best[b] of step 1  (per_cell_owns_beam).
//   3 wall slot q is SEEN by the same rule with wall_on.
// The rule is order-free: a seen slot occupies a nearest hit cell of some beam.  A cell shared by two primitives sees both; a
// cell that is also occupied on the grid sees the primitive anyway; two cells of different primitives with the same d2 on one
// beam see both; the absent disc (0, 0, 0) and a disc of radius 0 are never seen.
//
// KNOWING (per slot: first_seen, last_seen, int32, -1 = never).  At rollout step k every car with alive == 1 as the step finds
// it scans (pose k, the discs of step k); a seen slot gets last_seen = k, and first_seen = k if it was -1  (per_mark).  A slot is
// KNOWN at step k (per_known):
//   static disc, wall   last_seen >= 0                               (sticky: it is a map)
//   mover               last_seen >= 0 && k - last_seen <= hold      (tracked for `hold` further steps, at its true disc of step k)
//   traffic slot        last_seen == k                               (a slot is not the same car from step to step)
// Cars that do not scan keep what they know.
//
// PLANNING reads the perceived world: the disc list with the same offsets in which an unknown slot is (0, 0, 0), and wall headers in
// which an unknown wall has the empty box {1, 1, 0, 0, 0, 0} - wall_in_box and wall_meets_box are false for it  (per_disc, per_wall).
#pragma once
#include <cstdint>

#include "lidar_core.hpp"
#include "wall_core.hpp"

namespace mpmpc {

constexpr int PER_STATIC = 0, PER_MOVER = 1, PER_TRAFFIC = 2, PER_WALL = 3;      // slot kinds

// the kind of disc slot q of a car with n_static static discs and n_mover movers (what follows them is traffic)
MPMPC_HOST_DEVICE inline int per_disc_kind(int q, int n_static, int n_mover) {
  return q < n_static ? PER_STATIC : (q < n_static + n_mover ? PER_MOVER : PER_TRAFFIC);
}

// (MPMPC_HD: always inlined into K0s - a call would need a stack, and K0s runs without scratch)
// SEEING, rule 2 for one cell at offset (di, dj) from the sensor that belongs to the primitive and is in range with d2: does it
// own a beam - is it a nearest hit cell of one?  best[]: the final minima of the scan.
MPMPC_HD bool per_cell_owns_beam(int di, int dj, int d2, double psi, const double* angles, int n_beams, const int* best) {
  double mn, mx;
  if (!lid_cell_interval(di, dj, psi, &mn, &mx)) return false;
  for (int k = lid_first_beam(angles, n_beams, mn); k < n_beams && angles[k] <= mx; ++k)
    if (best[k] == d2) return true;
  return false;
}
// ... and the filter in front of it (K0s): false only where the cell cannot own a beam - its enclosure (lid_cell_enclosure) holds
// no beam with best == d2.  Skips work, never changes a verdict.
MPMPC_HD bool per_cell_may_own(int di, int dj, int d2, double psi, const double* angles, int n_beams, const int* best) {
  double lo, hi;
  if (!lid_cell_enclosure(di, dj, d2, psi, &lo, &hi)) return true;
  for (int k = lid_first_beam(angles, n_beams, lo); k < n_beams && angles[k] <= hi; ++k)
    if (best[k] == d2) return true;
  return false;
}

// KNOWING
MPMPC_HOST_DEVICE inline void per_mark(bool seen, int k, int* first_seen, int* last_seen) {
  if (!seen) return;
  *last_seen = k;
  if (*first_seen < 0) *first_seen = k;
}
MPMPC_HOST_DEVICE inline bool per_known(int kind, int last_seen, int k, int hold) {
  if (last_seen < 0) return false;
  if (kind == PER_MOVER) return k - last_seen <= hold;
  if (kind == PER_TRAFFIC) return last_seen == k;
  return true;
}

// PLANNING: slot values of the perceived world
MPMPC_HOST_DEVICE inline void per_disc(bool known, const int* d, int* o) {
  o[0] = known ? d[0] : 0; o[1] = known ? d[1] : 0; o[2] = known ? d[2] : 0;
}
MPMPC_HOST_DEVICE inline void per_wall(bool known, const int* h, int* o) {
  static_assert(WALL_HDR == 6, "per_wall writes the six header words one by one");
  o[0] = known ? h[0] : 1; o[1] = known ? h[1] : 1;
  o[2] = known ? h[2] : 0; o[3] = known ? h[3] : 0; o[4] = known ? h[4] : 0; o[5] = known ? h[5] : 0;
}

// One step of one car's knowledge, the whole law in one place (the host's restatement of K0s's third phase): n_disc disc slots
// (n_static static, n_mover movers, the rest traffic) and n_wall wall slots; scanned: the car scanned at step k; seen masks as a
// scan returns them (ignored when it did not scan).  Updates first / last ([COR_MAX_DISCS], [COR_MAX_WALLS]) and returns the masks
// of the slots known at step k.
inline void per_step(int n_disc, int n_static, int n_mover, int n_wall, bool scanned, uint64_t disc_seen, uint32_t wall_seen, int k,
                     int hold, int32_t* disc_first, int32_t* disc_last, int32_t* wall_first, int32_t* wall_last, uint64_t* disc_known,
                     uint32_t* wall_known) {
  uint64_t dk = 0;
  uint32_t wk = 0;
  for (int q = 0; q < n_disc && q < COR_MAX_DISCS; ++q) {
    per_mark(scanned && ((disc_seen >> q) & 1), k, disc_first + q, disc_last + q);
    if (per_known(per_disc_kind(q, n_static, n_mover), disc_last[q], k, hold)) dk |= (uint64_t)1 << q;
  }
  for (int q = 0; q < n_wall && q < COR_MAX_WALLS; ++q) {
    per_mark(scanned && ((wall_seen >> q) & 1), k, wall_first + q, wall_last + q);
    if (per_known(PER_WALL, wall_last[q], k, hold)) wk |= (uint32_t)1 << q;
  }
  *disc_known = dk;
  *wall_known = wk;
}

// Host-side validation of mpmpc_rollout_set_perception (res: the map's resolution, or +inf while there is no map - the step
// checks again).  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int per_check_setting(int n_beams, const double* angles, double range_m, int hold, double res, const char** why) {
  if (hold < 0) { *why = "hold must be >= 0"; return -1; }
  return lid_check_beams(n_beams, angles, range_m, res, why);
}

}  // namespace mpmpc
