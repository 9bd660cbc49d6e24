// Lookahead for traffic: every column of a car's horizon sees the cars of its group where their own plans put them when the
// car gets there, not where they are now.  Scalar code that compiles for gfx950 (K3t, mpmpc_plan_track_kernel; K0ht,
// mpmpc_traffic_horizon_kernel; the traffic instantiations of K0c - all in mpmpc_closed_loop.hpp) and for the host
// (tests/emul_traffic_lookahead), like the other *_core.hpp.
//
// The setting (mpmpc_rollout_set_lookahead_traffic; fleet-wide, off by default).  It is ACTIVE in a step iff lookahead is set
// (mpmpc_rollout_set_lookahead), traffic is set (mpmpc_rollout_set_traffic) and the flag is on; such a step looks ahead even
// when the fleet has no movers.
//
// The law, in three parts.
//
// 1. PLAN TRACKS (K3t, at the end of a step, behind the plant update).  Every step leaves car n's solved plan in z[n]: stage j
//    holds (e_y, e_psi, t)_j = z[n][3 j .. 3 j + 2] at waypoint wp_id[n] + j, j = 0 .. N, t_j the predicted arrival time.  With
//    the car's route view (first global row f, n_wp rows, circular or open: the one path when the fleet has no routes):
//
//        valid[n] = (alive[n] == 1 after the plant update) && ro_usable(status[n])
//        w_j      = wp_id[n] + j;  if (w_j >= n_wp) w_j = circular ? w_j % n_wp : n_wp - 1;  w_j += f        (ro_record_finish's)
//        (px, py) = ro_pred_point(gx[w_j], gy[w_j], cos psi[w_j], sin psi[w_j], z[n][3 j])     (the recorder's predicted path;
//                   the trigonometry is K0's host table: no device-libm result enters)
//        cells[n][j] = tr_cell(px, py), or OFF = (INT32_MIN, 0) where its guard fails (a NaN, or beyond 2^30 cells)
//        tm[n][0] = 0.0;   tm[n][j] = (t_j > tm[n][j-1]) ? t_j : tm[n][j-1]     with t_j = z[n][3 j + 2]
//
//    The running maximum takes the sub-tolerance non-monotonicity of a 1e-8 solve out, and a NaN is never taken; tm is
//    non-decreasing.  A maximum is exact, so K3t may form it by a wave scan (tlk_time_key / tlk_time_max: leftmost maximum
//    of the sequence 0.0, t_1', t_2', ... where t' is t with a NaN replaced by -inf - associative, the same bits in any
//    grouping).  Tracks are written for every car; valid says whether anybody may read them.
//    mpmpc_rollout_init, mpmpc_rollout_reroute and switching the setting on clear valid for the whole fleet (a stated
//    simplification: every car falls back to the frozen disc for one step).
//
// 2. WHO (K0t).  K0t also writes who[b][t]: the car index of the occupant of traffic slot t of car b, or -1 for an empty slot.
//
// 3. TRAFFIC HORIZON (K0ht, behind K0h, in front of K0c; it reads the leads of step k, who of step k and the tracks step
//    k - 1 left).  For car b, slot t, column c, with n = who[b][t], d = (cx, cy, r) the slot's disc of step k in the TRUE
//    list (as K0t wrote it) and L = lead[b][c] (lookahead_core.hpp):
//
//        tz[b][t][c] = d                                   if n < 0 or L == 0 or !valid[n]
//        otherwise   tau = (double)(L + 1) * Ts            (the plan was made one step ago)
//                    j*  = the largest j in [0, N] with tm[n][j] <= tau       (binary search; tm[n][0] = 0 <= tau)
//                    (cx', cy') = cells[n][j*]
//        tz[b][t][c] = (0, 0, 0)  if that stage is OFF or !tr_visible(map, cx', cy', r),  else (cx', cy', r)
//
//    Consequences: a neighbour is held at its plan's end beyond tm[n][N]; the S slots are chosen by CURRENT distance (K0t,
//    unchanged) - anticipation moves them, it does not re-select; knowing a neighbour means knowing its plan (the same kind
//    of simplification lookahead_core.hpp states for movers).
//
// K0c: the car's last S slots are its traffic slots.  For traffic slot t, if the entry of the list K0c plans from has r > 0,
// the disc of column c is tz[b][t][c], otherwise the staged entry (tlk_col_disc) - the same ONE gate as for movers, so under
// perception a car anticipates exactly the neighbours it currently sees.  The source is used in the touched test and in the
// staged occupancy, nowhere else.
#pragma once
#include <cmath>
#include <cstdint>

#include "lookahead_core.hpp"
#include "rollout_core.hpp"
#include "traffic_core.hpp"

namespace mpmpc {

constexpr int TLK_OFF = INT32_MIN;      // cells[n][j][0] of a stage whose cell failed tr_cell's guard

// bytes of K0ht's table for B cars with S slots each
inline long long tlk_table_bytes(long long B, int S, int N) { return B * S * N * 12; }

MPMPC_HOST_DEVICE inline bool tlk_valid(int alive_after, int status) {
  return alive_after == 1 && (status == 1 || status == 2 || status == -2);      // ro_usable
}

// global row of stage j of a car at local waypoint wp on its route view (ro_record_finish's wrap / clamp)
MPMPC_HOST_DEVICE inline long long tlk_stage_row(int wp, int j, int n_wp, bool circular, long long first) {
  int w = wp + j;
  if (w >= n_wp) w = circular ? w % n_wp : n_wp - 1;
  return first + w;
}

// the cell of a stage with lateral offset e_y at waypoint (wx, wy, cos, sin) -> cell[2]
MPMPC_HOST_DEVICE inline void tlk_stage_cell(const MapView& m, double wx, double wy, double cos_w, double sin_w, double e_y,
                                             int* cell) {
  const double px = wx - e_y * sin_w, py = wy + e_y * cos_w;      // ro_pred_point
  int cx = 0, cy = 0;
  if (tr_cell(m, px, py, &cx, &cy)) { cell[0] = cx; cell[1] = cy; }
  else { cell[0] = TLK_OFF; cell[1] = 0; }
}

// the running maximum: one step of the law's recurrence ...
MPMPC_HOST_DEVICE inline double tlk_time_max(double before, double t) { return t > before ? t : before; }
// ... and what a scan feeds it: stage 0 enters as 0.0, a NaN as -inf (never taken: tm[0] = 0.0 lies to its left)
MPMPC_HOST_DEVICE inline double tlk_time_key(int j, double t) { return j == 0 ? 0.0 : (t == t ? t : -HUGE_VAL); }

// tm[0 .. N] of one plan z (one stage after the other: the host twin; K3t scans)
MPMPC_HOST_DEVICE inline void tlk_times(int N, const double* z, double* tm) {
  tm[0] = 0.0;
  for (int j = 1; j <= N; ++j) tm[j] = tlk_time_max(tm[j - 1], z[3 * j + 2]);
}

// the largest j in [0, N] with tm[j] <= tau (tm non-decreasing, tm[0] = 0 <= tau)
MPMPC_HOST_DEVICE inline int tlk_stage_at(const double* tm, int N, double tau) {
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (tm[mid] <= tau) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// tz[b][t][c]: d the slot's disc of step k in the true list, n its occupant, L the column's lead; valid / cells / tm: the tracks
MPMPC_HOST_DEVICE inline void tlk_disc(const MapView& m, const int* d, int n, int L, double Ts, int N, const int* valid,
                                       const int* cells, const double* tm, int* out) {
  out[0] = d[0]; out[1] = d[1]; out[2] = d[2];
  if (n < 0 || L == 0 || !valid[n]) return;
  const double tau = (double)(L + 1) * Ts;
  const int j = tlk_stage_at(tm + (long long)n * (N + 1), N, tau);
  const int* c = cells + ((long long)n * (N + 1) + j) * 2;
  if (c[0] == TLK_OFF || !tr_visible(m, c[0], c[1], d[2])) { out[0] = out[1] = out[2] = 0; return; }
  out[0] = c[0]; out[1] = c[1];
}

// The disc a column plans with for slot j of the car's list `dsc` of nd entries: look_col_disc for the movers, and for the
// car's last S slots - its traffic slots - K0ht's table tzb [S][N][3] of the car.  The gate: an absent slot stays absent.
MPMPC_HOST_DEVICE inline const int* tlk_col_disc(const int* dsc, int j, int ns, int nm, const int* hz, int nd, int S,
                                                 const int* tzb, int N, int c) {
  const int* d = dsc + 3 * j;
  const int q = j - ns, t = j - (nd - S);
  if (d[2] <= 0) return d;
  if (q >= 0 && q < nm) return hz + ((long long)q * N + c) * 3;
  if (t >= 0) return tzb + ((long long)t * N + c) * 3;
  return d;
}

}  // namespace mpmpc
