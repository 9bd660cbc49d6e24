// Traffic of the device rollout: the cars of a group see each other as discs.  Scalar code that compiles for gfx950 (K0t,
// mpmpc_traffic_kernel in mpmpc_closed_loop.hpp) and for the host (tests/emul_traffic), like obstacle_motion_core.hpp.
//
// The settings of a call (mpmpc_rollout_set_traffic):
//   group[B]         int32; cars with the same non-negative value share a world, a negative value: the car sees nobody
//                    and nobody sees it
//   radius_cells[B]  >= 0: the disc with which car c appears to the others (a disc of radius 0 occupies no cell)
//   slots S          in [1, 64], the same for every car: the discs a car gets of its group
//   range_cells      a car sees no further than this many cells; negative: no limit
// The inputs of a step are pose[B][3] and alive[B] AS THE STEP FINDS THEM - what mpmpc_rollout_state returns before the
// step, what the recorder's snapshot keeps (s, pose: empty when the car had ended) - before K3a changes alive: the host
// loop and a recorded trace can recompute every step's discs from public data.  In exactly this order:
//
//   car c is PRESENT iff alive[c] == 1 and group[c] >= 0 and, with
//       qx = floor((x_c - ox) / res), qy = floor((y_c - oy) / res)              (cor_w2m's expression)
//       |qx| <= 2^30 and |qy| <= 2^30 (mov_disc's guard; a NaN fails both);  then (cx_c, cy_c) = (int)(qx, qy)
//   a present car with r = radius_cells[c] is VISIBLE unless
//       cx - r < 0 or cy - r < 0 or cx + r > width or cy + r > height            (mov_disc's test: the square leaves the grid)
//   A car that has ended (alive -1 .. -4) or finished its lap (alive 0) is taken off the track: it is not seen and it
//   sees nobody.  (Seeing ended cars as wrecks would be another law.)
//
//   the slots of car b:  b not present: all S slots are the absent disc (0, 0, 0).  b present (it need not be visible):
//   its candidates are the visible cars c with  c != b,  group[c] == group[b]  and
//       d2 = (cx_c - cx_b)^2 + (cy_c - cy_b)^2   (int64)   <= range_cells^2      (range_cells < 0: no such condition)
//   ordered by (d2 ascending, car index ascending); the first S fill slots 0, 1, ... as (cx_c, cy_c, r_c), the slots
//   that remain are (0, 0, 0).
// Everything after the two floors is integer arithmetic; no device-libm result enters.  d2 fits: a candidate lies on
// the grid (at most COR_MAX_SIDE cells a side) and b within 2^30 cells, so d2 < 2^62.
//
// The host lays the groups out once per call (tr_layout): a dense group number per car (or -1) and a CSR list of each
// group's members in ascending car index - position in that list orders like the car index, which is what K0t breaks
// ties by.  A group has at most TR_MAX_GROUP members (K0t stages one key per member in LDS).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "obstacle_motion_core.hpp"

namespace mpmpc {

constexpr int TR_MAX_GROUP = 1024;      // members of one group
constexpr int TR_MAX_SLOTS = COR_MAX_DISCS;

// the cell of a car whose alive and group let it be present; false: not present
MPMPC_HOST_DEVICE inline bool tr_cell(const MapView& m, double x, double y, int* cx, int* cy) {
  const double qx = std::floor((x - m.ox) / m.res), qy = std::floor((y - m.oy) / m.res);
  if (!(std::fabs(qx) <= MOV_CELL_MAX && std::fabs(qy) <= MOV_CELL_MAX)) return false;
  *cx = (int)qx; *cy = (int)qy;
  return true;
}

MPMPC_HOST_DEVICE inline bool tr_visible(const MapView& m, int cx, int cy, int r) {
  return !((long long)cx - r < 0 || (long long)cy - r < 0 || (long long)cx + r > m.width || (long long)cy + r > m.height);
}

// d2 of a visible member at (cx, cy) as the present car at (bx, by) sees it, or -1 when it lies out of range
MPMPC_HOST_DEVICE inline long long tr_d2(int bx, int by, int cx, int cy, int range_cells) {
  const long long dx = (long long)cx - bx, dy = (long long)cy - by;
  const long long d2 = dx * dx + dy * dy;
  if (range_cells >= 0 && d2 > (long long)range_cells * range_cells) return -1;
  return d2;
}

// (d2, position) pairs order lexicographically; positions are unique within a group, so the order is total
MPMPC_HOST_DEVICE inline bool tr_less(long long d2a, int ia, long long d2b, int ib) {
  return d2a < d2b || (d2a == d2b && ia < ib);
}

// Dense group numbers (ascending in the group value; -1 for a negative group), the CSR offsets goff[G + 1] and the
// members of every group in ascending car index.  dense / members: [B], goff: [B + 1].  Returns G, or -1 when a group
// has more than TR_MAX_GROUP members.
inline int tr_layout(int B, const int32_t* group, int32_t* dense, int32_t* goff, int32_t* members) {
  std::vector<std::pair<int32_t, int32_t>> order;
  order.reserve((size_t)B);
  for (int c = 0; c < B; ++c) {
    dense[c] = -1;
    if (group[c] >= 0) order.emplace_back(group[c], c);
  }
  std::sort(order.begin(), order.end());
  int G = 0;
  goff[0] = 0;
  for (size_t k = 0; k < order.size(); ++k) {
    if (k > 0 && order[k].first != order[k - 1].first) goff[++G] = (int32_t)k;
    dense[order[k].second] = G;
    members[k] = order[k].second;
    if ((int)k - goff[G] >= TR_MAX_GROUP) return -1;
  }
  if (!order.empty()) goff[++G] = (int32_t)order.size();
  return G;
}

// Host-side validation of mpmpc_rollout_set_traffic (group != NULL) against the other two settings in force (B_x = 0:
// off).  Returns 0, -1 (MPMPC_E_ARG) or -3 (MPMPC_E_STATE) and the reason.
inline int tr_check_traffic(int B, int max_batch, const int32_t* group, const int32_t* radius, int slots, bool built,
                            int B_static, const int32_t* off_static, int B_movers, const int32_t* off_movers,
                            const char** why) {
  if (!built) { *why = "needs mpmpc_build_corridor on the current map and path geometry first"; return -3; }
  if (B < 1 || B > max_batch) { *why = "B must be in [1, max_batch]"; return -1; }
  if (!radius) { *why = "radius_cells is NULL"; return -1; }
  if (slots < 1 || slots > TR_MAX_SLOTS) { *why = "slots must be in [1, 64]"; return -1; }
  for (int c = 0; c < B; ++c)
    if (radius[c] < 0) { *why = "a car has a negative traffic radius"; return -1; }
  std::vector<int32_t> dense((size_t)B), goff((size_t)B + 1), members((size_t)B);
  if (tr_layout(B, group, dense.data(), goff.data(), members.data()) < 0) {
    *why = "a traffic group has more than 1024 members (TR_MAX_GROUP)";
    return -1;
  }
  return mov_check_combined(B_static, off_static, B_movers, off_movers, why, B, slots);
}

// The S slots of car b, one car after the other (the host twin; K0t does the same selection with a wavefront).
// out [S][3]; who [S] (optional): the car index of every slot's occupant, -1 for an empty slot (what K0t writes for the
// traffic lookahead, traffic_lookahead_core.hpp).
inline void tr_slots_car(const MapView& m, const double* pose, const int32_t* alive, const int32_t* dense,
                         const int32_t* radius, const int32_t* goff, const int32_t* members, int S, int range_cells, int b,
                         int32_t* out, int32_t* who = nullptr) {
  for (int k = 0; k < 3 * S; ++k) out[k] = 0;
  for (int t = 0; who && t < S; ++t) who[t] = -1;
  int bx, by;
  if (alive[b] != 1 || dense[b] < 0 || !tr_cell(m, pose[3L * b], pose[3L * b + 1], &bx, &by)) return;
  const int g0 = goff[dense[b]], n = goff[dense[b] + 1] - g0;
  struct Cand { long long d2; int pos, cx, cy; };
  std::vector<Cand> cand;
  for (int p = 0; p < n; ++p) {
    const int c = members[g0 + p];
    int cx, cy;
    if (c == b || alive[c] != 1 || !tr_cell(m, pose[3L * c], pose[3L * c + 1], &cx, &cy)) continue;
    if (!tr_visible(m, cx, cy, radius[c])) continue;
    const long long d2 = tr_d2(bx, by, cx, cy, range_cells);
    if (d2 >= 0) cand.push_back({d2, p, cx, cy});
  }
  std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& c) { return tr_less(a.d2, a.pos, c.d2, c.pos); });
  for (int t = 0; t < S && t < (int)cand.size(); ++t) {
    out[3 * t] = cand[t].cx; out[3 * t + 1] = cand[t].cy; out[3 * t + 2] = radius[members[g0 + cand[t].pos]];
    if (who) who[t] = members[g0 + cand[t].pos];
  }
}

}  // namespace mpmpc
