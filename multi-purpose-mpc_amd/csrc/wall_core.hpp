// Boundary walls of a car's world: what Map.add_boundary of the reference stamps into the grid (src/map.py:139-155), as a
// second primitive of the per-car worlds beside the discs of corridor_core.hpp.  Scalar code that compiles for gfx950 (K0w
// and the consumers K0c, K0l, K0f, K-world) and for the host (tests/emul_walls), like lidar_core.hpp.
//
// A wall is (x0, y0, x1, y1) in map cells, the w2m of its two end points.  In exactly this order:
//
//   1 the cells:  a wall occupies exactly the cells cor_line_aa(x0, y0, x1, y1, visit(x, y)) produces - skimage's line_aa in
//       the reference's argument order (rr = x, cc = y), the same set the host Map.add_boundary stamps.
//   2 the major axis:  x when |x1 - x0| >= |y1 - y0|, else y.  n = max(|x1 - x0|, |y1 - y0|) + 1 major indices,
//       k = major - min(major end points).
//   3 the table (K0w, once per setting, never per step):  one int32 per major index, 0 = nothing seen yet.  The first cell
//       seen at index k with minor coordinate f gives  base = f - WALL_BASE_BACK,  entry = (base + WALL_BIAS) << 8 | 1 <<
//       WALL_BASE_BACK;  every further cell at k sets bit (minor - base).  No second pass: the bits 0 .. 7 around the first
//       cell hold any run that spans at most 3 cells whichever of them comes first (bits 1 .. 5).  A cell whose major
//       index leaves [0, n) or whose bit leaves [0, 8) makes wall_raster return false - the setter then refuses the wall
//       instead of keeping a table that is not the line (no line among those measured does: DESIGN).
//   4 the header, WALL_HDR ints, computed on the host:  the box x_min, y_min, x_max, y_max of the two end cells GROWN BY ONE
//       CELL IN THE MINOR DIRECTION (anti-aliased neighbours step at most one cell past the end points' minor range, and
//       never past the major one), the wall's offset into the table, the major axis (0: x, 1: y).
//   5 membership of (x, y), O(1) per wall:  outside the box: no.  Else k = major - box_min(major), e = table[offset + k],
//       bit = minor - ((e >> 8) - WALL_BIAS):  on the wall iff 0 <= bit < 8 and (e >> bit) & 1.  One table load.
//
// A cell of a car's world is occupied iff it is occupied on the base grid (off the grid counts as occupied, cor_cell_free), or
// lies in one of the car's discs (cor_in_disc), or on one of the car's walls (wall_on).  Everything is integer: every consumer
// is bit-equal to the same consumer on the grid with the walls stamped in.
// End points are confined to [1, width - 2] x [1, height - 2] (wall_check_lists): every produced cell then lies on the grid.
#pragma once
#include <cstdint>

#include "corridor_core.hpp"

namespace mpmpc {

constexpr int COR_MAX_WALLS = 16;      // walls per car (mpmpc_rollout_set_walls refuses more)
constexpr int WALL_HDR = 6;            // x_min, y_min, x_max, y_max (grown), table offset, major axis
constexpr int WALL_BASE_BACK = 3;      // the mask starts this many cells below the first cell seen
constexpr int WALL_BIAS = 4;           // keeps base + WALL_BIAS positive (base >= -WALL_BASE_BACK)

MPMPC_HOST_DEVICE inline int wall_abs(int a) { return a < 0 ? -a : a; }
// step 2: table entries of a wall
MPMPC_HOST_DEVICE inline int wall_extent(const int* w) {
  const int dx = wall_abs(w[2] - w[0]), dy = wall_abs(w[3] - w[1]);
  return (dx >= dy ? dx : dy) + 1;
}
// step 4
MPMPC_HOST_DEVICE inline void wall_header(const int* w, int table_offset, int* h) {
  const int dx = wall_abs(w[2] - w[0]), dy = wall_abs(w[3] - w[1]);
  const int axis = dx >= dy ? 0 : 1;
  h[0] = (w[0] < w[2] ? w[0] : w[2]) - (axis == 1 ? 1 : 0);
  h[1] = (w[1] < w[3] ? w[1] : w[3]) - (axis == 0 ? 1 : 0);
  h[2] = (w[0] > w[2] ? w[0] : w[2]) + (axis == 1 ? 1 : 0);
  h[3] = (w[1] > w[3] ? w[1] : w[3]) + (axis == 0 ? 1 : 0);
  h[4] = table_offset;
  h[5] = axis;
}
// steps 1 and 3 for one wall: fills table[h[4] .. h[4] + wall_extent(w)).  false: the table cannot hold the line.
MPMPC_HD bool wall_raster(const int* w, const int* h, int* table) {
  const int n = wall_extent(w), axis = h[5];
  int* t = table + h[4];
  for (int k = 0; k < n; ++k) t[k] = 0;
  const int m0 = axis == 0 ? h[0] : h[1];
  bool ok = true;
  cor_line_aa(w[0], w[1], w[2], w[3], [&](int x, int y) {
    const int k = (axis == 0 ? x : y) - m0, minor = axis == 0 ? y : x;
    if (k < 0 || k >= n) { ok = false; return; }
    const int e = t[k];
    if (e == 0) {
      t[k] = ((minor - WALL_BASE_BACK + WALL_BIAS) << 8) | (1 << WALL_BASE_BACK);
    } else {
      const int bit = minor - ((e >> 8) - WALL_BIAS);
      if (bit < 0 || bit > 7) { ok = false; return; }
      t[k] = e | (1 << bit);
    }
  });
  return ok;
}
MPMPC_HD bool wall_in_box(int x, int y, const int* h) { return x >= h[0] && x <= h[2] && y >= h[1] && y <= h[3]; }
// step 5
MPMPC_HD bool wall_on(int x, int y, const int* h, const int* table) {
  if (!wall_in_box(x, y, h)) return false;
  const int k = h[5] == 0 ? x - h[0] : y - h[1], minor = h[5] == 0 ? y : x;
  const int e = table[h[4] + k];
  const int bit = minor - ((e >> 8) - WALL_BIAS);
  return (unsigned)bit < 8u && ((e >> bit) & 1) != 0;
}
// does the wall's box meet a box (K0c's line box layout: box[1 .. 4] = x_min, y_min, x_max, y_max)?
MPMPC_HD bool wall_meets_box(const int* h, const int* box) {
  return h[0] <= box[3] && h[2] >= box[1] && h[1] <= box[4] && h[3] >= box[2];
}
// does anything of a car's world - discs or walls (hdr(j) -> const int* header) - touch the line box?
template <class Disc, class Hdr>
MPMPC_HD bool wall_car_touches(const int* box, int n_disc, Disc disc, int n_wall, Hdr hdr) {
  for (int j = 0; j < n_wall; ++j)
    if (wall_meets_box(hdr(j), box)) return true;
  return cor_car_touches(box, n_disc, disc);
}
// THE predicate: is cell (x, y) occupied in the car's world?
template <class Disc, class Hdr>
MPMPC_HD bool wall_world_occupied(const MapView& m, int x, int y, int n_disc, Disc disc, int n_wall, Hdr hdr, const int* table) {
  if (!cor_cell_free(m, x, y)) return true;
  for (int j = 0; j < n_disc; ++j)
    if (cor_in_disc(x, y, disc(j))) return true;
  for (int j = 0; j < n_wall; ++j)
    if (wall_on(x, y, hdr(j), table)) return true;
  return false;
}
// ... of a packed cell of a cached border line (K0c; cor_car_cell_free with walls)
template <class Disc, class Hdr>
MPMPC_HD bool wall_car_cell_free(const MapView& m, int cell, int n_disc, Disc disc, int n_wall, Hdr hdr, const int* table) {
  int x, y;
  cor_unpack_cell(cell, x, y);
  return !wall_world_occupied(m, x, y, n_disc, disc, n_wall, hdr, table);
}
// ... of a window cell that lies on the grid (K0l, K0f; lid_occupied with walls)
template <class Disc, class Hdr>
MPMPC_HD bool wall_lid_occupied(const MapView& m, int i, int j, int n_disc, Disc disc, int n_wall, Hdr hdr, const int* table) {
  return wall_world_occupied(m, i, j, n_disc, disc, n_wall, hdr, table);
}
// Free segments of a cached line in the car's world with walls (cor_car_scan with walls)
template <class Disc, class Hdr, class Emit>
MPMPC_HD int wall_car_scan(const MapView& m, double min_width, const int* cells, const int* box, int n_disc, Disc disc, int n_wall,
                           Hdr hdr, const int* table, Emit emit) {
  int ux, uy, lx, ly;
  cor_unpack_cell(box[5], ux, uy);
  cor_unpack_cell(box[6], lx, ly);
  return cor_scan_runs(m, ux, uy, lx, ly, min_width, box[0], [&](int k, int& x, int& y) { cor_unpack_cell(cells[k], x, y); },
                       [&](int k) { return wall_car_cell_free(m, cells[k], n_disc, disc, n_wall, hdr, table); }, emit);
}

// what the kernels take of a fleet's walls: CSR offsets per car, the headers, the table (off == nullptr: no walls)
struct WallView {
  const int* off;      // [B + 1]
  const int* hdr;      // [off[B]][WALL_HDR]
  const int* tab;      // sum of the walls' extents
};

// Host side: headers and table offsets of n walls ([n][4]); returns the table's size (the sum of the extents).
inline long wall_layout(long n, const int32_t* walls, int32_t* hdr) {
  long total = 0;
  for (long j = 0; j < n; ++j) {
    wall_header(walls + 4 * j, (int)total, hdr + WALL_HDR * j);
    total += wall_extent(walls + 4 * j);
  }
  return total;
}

// Host-side validation of the wall lists of B cars (off != NULL), everything that is decided before a device call.
// Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int wall_check_lists(int B, const int32_t* off, const int32_t* walls, int map_w, int map_h, const char** why) {
  if (off[0] != 0) { *why = "wall offsets[0] must be 0"; return -1; }
  for (int b = 0; b < B; ++b) {
    const long k = (long)off[b + 1] - off[b];
    if (k < 0) { *why = "wall offsets must not decrease"; return -1; }
    if (k > COR_MAX_WALLS) { *why = "more than 16 walls for one car (COR_MAX_WALLS)"; return -1; }
  }
  if (off[B] > 0 && !walls) { *why = "walls is NULL"; return -1; }
  for (long j = 0; j < off[B]; ++j)
    for (int e = 0; e < 2; ++e) {
      const long x = walls[4 * j + 2 * e], y = walls[4 * j + 2 * e + 1];
      if (x < 1 || x > map_w - 2 || y < 1 || y > map_h - 2) {
        *why = "a wall's end point lies outside [1, width - 2] x [1, height - 2]";
        return -1;
      }
    }
  return 0;
}
// ... of mpmpc_rollout_set_walls.  built: a mpmpc_build_corridor of the current map and geometry exists; other_B: the B of
// the per-car settings in force (0: none).  Returns 0, -1 (MPMPC_E_ARG) or -3 (MPMPC_E_STATE).
inline int wall_check_walls(int B, int max_batch, const int32_t* off, const int32_t* walls, bool built, int map_w, int map_h,
                            int other_B, const char** why) {
  if (!built) { *why = "needs mpmpc_build_corridor on the current map and path geometry first"; return -3; }
  if (B < 1 || B > max_batch) { *why = "B must be in [1, max_batch]"; return -1; }
  if (int rc = wall_check_lists(B, off, walls, map_w, map_h, why)) return rc;
  if (other_B > 0 && other_B != B) { *why = "the walls and the other per-car settings must be for the same number of cars"; return -3; }
  return 0;
}

}  // namespace mpmpc
