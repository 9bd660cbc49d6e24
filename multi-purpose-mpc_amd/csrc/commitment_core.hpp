// Corridor commitment (K0k): a car's horizon keeps, waypoint by waypoint, the side of an obstacle it chose in the step before.
// Scalar per-thread code on corridor_core.hpp's accessors that compiles for gfx950 (the KEEP instantiations of K0c,
// mpmpc_closed_loop.hpp) and for the host (tests/emul_commitment), both under -ffp-contract=off.
//
// The reference rebuilds a car's row from nothing at every step (ReferencePath.update_path_constraints: the largest free
// segment at column 0, then the segment nearest the forward projection of the previous column's).  Nothing ties step k's row
// to step k - 1's, so a waypoint can change sides of an obstacle in the step it becomes column 0 - the reference's README
// names this as its second open limitation.  The law below is this library's own; with the setting off it is the reference's.
//
// THE LAW, every operation in its order:
//   Setting.  keep[b], one double per car: 0 - the car is off; a value in [1, +inf] - the car is on, with that switch_ratio;
//     anything else (NaN included) is refused (cmt_check).
//   Memory.  A car has N entries, one per column of the last row K0c built for it.  Entry c holds wp - the route-local
//     waypoint of that column, cor_wp(wp_id + 1 + c), or CMT_EMPTY - and the column's cor_bounds output (COR_WPC doubles: ub,
//     lb and the border cells of the selection without the margin).  An entry is EMPTY (wp = CMT_EMPTY, the doubles 0) when the
//     column had no free segment or the car's row was not COR_ROW_OK.  The memory of waypoint i is the entry with wp == i in
//     the LOWEST column (cmt_find; duplicates: the clamped end columns of an open route, a circular route shorter than N).
//   Choice at column c, waypoint i, cnt >= 2 candidates (cmt_select_car_one):
//     1. the car is on and waypoint i has memory m (cmt_choose_acc): for every candidate s = (ub_x, ub_y, lb_x, lb_y) in order
//          du = sqrt((s0 - m2)(s0 - m2) + (s1 - m3)(s1 - m3)),  dl = sqrt((s2 - m4)(s2 - m4) + (s3 - m5)(s3 - m5)),
//          off = (du + dl) / 2                       - cor_choose_acc's measure against m itself: the waypoint is the same,
//                                                      nothing is projected forward
//          len = sqrt(dx dx + dy dy), dx = s0 - s2, dy = s1 - s3      - column 0's span
//        the kept candidate is the FIRST minimum of off (k == 0 || off < best), the longest the FIRST maximum of len
//        (len > best, from -1: column 0's tie rule); if switch_ratio < +inf and len_longest > switch_ratio * len_kept the
//        longest is taken instead ("switched").  The column is "kept" either way.
//     2. otherwise the reference's rule, unchanged (cor_choose_acc): the largest segment at c = 0, else the candidate nearest
//        the projection of column c - 1's border cells - whatever rule decided column c - 1.
//     Columns with cnt <= 1 are forced, the verdicts COR_ROW_BLOCKED / COR_ROW_OVERFLOW are taken as without the law.
//   Replay.  A column is sequential only through the run of multi-segment columns right before it that rule 2 decides: a
//     column that rule 1 decides does not read its predecessor and starts a replay like a forced column does.
//   Counters, three per car, accumulated over the steps for every car the setting covers, the off cars included:
//     kept      columns decided by rule 1
//     switched  columns where the ratio clause left the nearest candidate
//     moved     columns whose waypoint has memory m where neither (ub, lb) of this step nor (m0, m1) is collapsed
//               (ub == lb: cor_bounds' collapse to 0, 0, and the zero row of a car without a row) and the intervals do not
//               overlap: ub < m1 || lb > m0                                                              (cmt_moved)
#pragma once
#include "corridor_core.hpp"

namespace mpmpc {

constexpr int CMT_EMPTY = -1;                    // wp of an empty entry
constexpr int CMT_COUNTS = 3;                    // kept, switched, moved
constexpr int CMT_KEPT = 1, CMT_SWITCHED = 2;    // bits of how a column was decided
constexpr long long CMT_BUDGET = 256LL << 20;    // bytes of a fleet's commitment block (the lookahead tables' cap)

MPMPC_HD bool cmt_on(double keep) { return keep >= 1.0; }      // (of a checked setting: 0 or [1, +inf])
// the block of B cars with N columns: the setting, the memory twice (a step reads one and writes the other), the counters
inline long long cmt_bytes(long long B, int N) {      // (host)
  return 8 * B + 2 * B * N * (8LL * COR_WPC + 4) + 4LL * CMT_COUNTS * B;
}
// the lowest column of a memory whose waypoint is i (wp(c) -> int), or -1
template <class Wp>
MPMPC_HD int cmt_find(int N, Wp wp, int i) {
  for (int c = 0; c < N; ++c)
    if (wp(c) == i) return c;
  return -1;
}
MPMPC_HD bool cmt_collapsed(double ub, double lb) { return ub == lb; }
MPMPC_HD bool cmt_moved(double ub, double lb, double m_ub, double m_lb) {
  return !cmt_collapsed(ub, lb) && !cmt_collapsed(m_ub, m_lb) && (ub < m_lb || lb > m_ub);
}

// Rule 1 at waypoint i: o <- the cor_bounds output of the chosen candidate; returns CMT_KEPT, | CMT_SWITCHED
template <class Seg>
MPMPC_HD int cmt_choose_acc(const PathGeom& g, int cnt, Seg seg, int i, const double* m, double ratio, double safety_margin,
                            double* o) {
  int best = 0, longest = 0;
  double best_off = 0.0, best_span = 0.0, longest_span = -1.0;
  for (int k = 0; k < cnt; ++k) {
    double s[4];
    seg(k, s);
    const double du = std::sqrt((s[0] - m[2]) * (s[0] - m[2]) + (s[1] - m[3]) * (s[1] - m[3]));
    const double dl = std::sqrt((s[2] - m[4]) * (s[2] - m[4]) + (s[3] - m[5]) * (s[3] - m[5]));
    const double off = (du + dl) / 2;
    const double dx = s[0] - s[2], dy = s[1] - s[3];
    const double len = std::sqrt(dx * dx + dy * dy);
    if (k == 0 || off < best_off) { best_off = off; best = k; best_span = len; }
    if (len > longest_span) { longest_span = len; longest = k; }
  }
  int how = CMT_KEPT;
  if (ratio < __builtin_inf() && longest_span > ratio * best_span) { best = longest; how |= CMT_SWITCHED; }
  double s[4];
  seg(best, s);
  cor_bounds(g.x[i], g.y[i], g.trig + (long)i * COR_TRIG, s[0], s[1], s[2], s[3], safety_margin, o);
  return how;
}

// Column n of the horizon that starts at waypoint wp_id under the law: cor_select_car_one with a memory.
//   cnt / forced / seg    as cor_select_car_one's
//   mem(i, m)             the memory of waypoint i into m[COR_WPC]; false: it has none
// o <- the column's cor_bounds output, *how <- how column n itself was decided (0: forced or rule 2).  Returns
// COR_ROW_BLOCKED when the first column has no free segment, else COR_ROW_OK.
template <class Cnt, class Forced, class Seg, class Mem>
MPMPC_HD int cmt_select_car_one(const PathGeom& g, int wp_id, int n, double safety_margin, double keep, Cnt cnt, Forced forced,
                                Seg seg, Mem mem, double* o, int* how) {
  *how = 0;
  if (cnt(0) == 0) return COR_ROW_BLOCKED;
  const bool on = cmt_on(keep);
  double m[COR_WPC];
  int first = n;               // first column of the run to replay
  bool committed = false;      // ... and rule 1 decides it
  for (;;) {
    if (cnt(first) < 2) break;
    if (on && mem(cor_wp(g, wp_id + first), m)) { committed = true; break; }
    if (first == 0) break;
    --first;
  }
  for (int k = 0; k < COR_WPC; ++k) o[k] = 0.0;
  for (int c = first; c <= n; ++c) {
    const int i = cor_wp(g, wp_id + c);
    if (cnt(c) <= 1) {
      forced(c, o);
    } else if (c == first && committed) {
      const int hw = cmt_choose_acc(g, cnt(c), [&](int k, double* s) { seg(c, k, s); }, i, m, keep, safety_margin, o);
      if (c == n) *how = hw;
    } else {
      double prev[COR_WPC];
      for (int k = 0; k < COR_WPC; ++k) prev[k] = o[k];
      cor_choose_acc(g, cnt(c), [&](int k, double* s) { seg(c, k, s); }, i, cor_wp(g, wp_id + c - 1), c == 0, prev,
                     safety_margin, o);
    }
  }
  return COR_ROW_OK;
}

// Host-side validation of mpmpc_rollout_set_commitment (keep != NULL).  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int cmt_check(int B, int max_batch, int N, const double* keep, const int32_t* mem_wp, const double* mem_rows,
                     const char** why) {
  if (B < 1 || B > max_batch) { *why = "B must be in [1, max_batch]"; return -1; }
  for (int b = 0; b < B; ++b)
    if (!(keep[b] == 0.0 || keep[b] >= 1.0)) { *why = "keep must be 0 (off) or a switch_ratio in [1, +inf] for every car"; return -1; }
  if (cmt_bytes(B, N) > CMT_BUDGET) { *why = "the commitment memory of B cars would exceed 256 MiB"; return -1; }
  if ((mem_wp != nullptr) != (mem_rows != nullptr)) { *why = "mem_wp and mem_rows go together: both or neither"; return -1; }
  if (mem_wp)
    for (long k = 0; k < (long)B * N; ++k)
      if (mem_wp[k] < CMT_EMPTY) { *why = "mem_wp holds waypoints >= 0 or -1 (empty)"; return -1; }
  return 0;
}

}  // namespace mpmpc
