// Lookahead of the device rollout: every column of a car's horizon sees the car's movers where they will be when the car
// gets there, not where they are now.  Scalar code that compiles for gfx950 (K0h, mpmpc_mover_horizon_kernel, and the LEAD
// instantiations of K0c in mpmpc_closed_loop.hpp) and for the host (tests/emul_lookahead), like the other *_core.hpp.
//
// The setting (mpmpc_rollout_set_lookahead; fleet-wide, off by default): a table seg_time[n_wp] - entry i is the seconds a
// car is expected to need from waypoint i to waypoint i + 1, indexed by the GLOBAL row of the handle's path table (route
// fleets lay it end to end like the path itself) - and max_lead >= 1 [steps].
//
// The law.  Car b at rollout step k with local waypoint wp_id: column c of its horizon is waypoint
// cor_wp(g, wp_id + 1 + c) on the car's route view g (K0c's own index function: circular wrap and open-route clamping
// are K0c's by construction).  Its LEAD is
//
//     t_-1 = 0;   t_c = t_(c-1) + seg_time[row of cor_wp(g, wp_id + c)]          c = 0 .. N-1
//     q = floor(t_c / Ts)        lead_c = (q < max_lead) ? (int)q : max_lead
//
// The sum is strictly sequential, left to right; every add and the division are rounded on their own (the build has
// -ffp-contract=off), so host and device agree bit for bit.  An infinite t_c saturates lead_c to max_lead (no entry is
// negative or NaN: look_check_setting).  Ts is the rollout's.
//
// Column c is then built in this world:
//   static discs, walls and traffic slots as at step k (lead 0: unchanged; the traffic slots follow their occupants' plans
//   instead when mpmpc_rollout_set_lookahead_traffic is on: traffic_lookahead_core.hpp);
//   mover slot q as mov_disc(..., k + lead_c, step0) on the route view of the owning car, as K0m forms it;
//   ONE gate: a mover whose slot in the list K0c plans from is absent at step k (r == 0: off the grid, or - under
//   perception - not known) is absent in every column.  Under perception a car thus anticipates exactly the movers it
//   currently knows; knowing a mover means knowing its motion law (a simplification: the lidar sees a disc, not a law).
// Nothing else of K0c's law changes: the "touched" box test, the staged occupancy, cor_scan_runs, cor_select_car_one and
// the verdict at column 0 read per-column sources, which now come from per-column worlds.
#pragma once
#include <cmath>
#include <cstdint>

#include "obstacle_motion_core.hpp"

namespace mpmpc {

constexpr int LOOK_MAX_LEAD = 1 << 20;                        // cap of max_lead [steps]
constexpr long long LOOK_TABLE_BUDGET = 256LL << 20;          // bytes of K0h's disc table: movers x N x 12

// lead of one column from its arrival time t [s]
MPMPC_HOST_DEVICE inline int look_lead(double t, double Ts, int max_lead) {
  const double q = std::floor(t / Ts);
  return q < (double)max_lead ? (int)q : max_lead;
}

// The leads of one car's N columns.  seg(c): seg_time[row of cor_wp(g, wp_id + c)] (look_seg_row on the car's route view; K0h
// fetches the N values side by side first, the sum itself stays one lane's).
MPMPC_HD int look_seg_row(const PathGeom& g, int wp_id, int c) { return cor_wp(g, wp_id + c); }
template <class Seg>
MPMPC_HD void look_leads(int N, double Ts, int max_lead, Seg seg, int* lead) {
  double t = 0.0;
  for (int c = 0; c < N; ++c) {
    t = t + seg(c);
    lead[c] = look_lead(t, Ts, max_lead);
  }
}

// The disc a column plans with for slot j of the car's list `dsc` (the list of step k K0c stages): slots
// ns .. ns + nm - 1 are the car's movers, mover q's horizon discs are hz[(q * N + c) * 3 ..] (K0h's table, q counted from
// the car's first mover).  The gate: an absent slot stays absent.
MPMPC_HOST_DEVICE inline const int* look_col_disc(const int* dsc, int j, int ns, int nm, const int* hz, int N, int c) {
  const int* d = dsc + 3 * j;
  const int q = j - ns;
  return (q >= 0 && q < nm && d[2] > 0) ? hz + ((long long)q * N + c) * 3 : d;
}

// Bytes of K0h's disc table for `movers` movers of the fleet
inline long long look_table_bytes(long long movers, int N) { return movers * N * 12; }

// Host-side validation of mpmpc_rollout_set_lookahead (seg_time != NULL).  path_n_wp: the path table's rows (0: none set).
// Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int look_check_setting(int n_wp, int path_n_wp, const double* seg_time, int max_lead, const char** why) {
  if (path_n_wp <= 0 || n_wp != path_n_wp) { *why = "n_wp must equal the path table's (mpmpc_set_path)"; return -1; }
  if (max_lead < 1 || max_lead > LOOK_MAX_LEAD) { *why = "max_lead must be in [1, 1048576] (LOOK_MAX_LEAD)"; return -1; }
  for (int i = 0; i < n_wp; ++i)
    if (!(seg_time[i] >= 0.0)) { *why = "a seg_time entry is negative or NaN"; return -1; }
  return 0;
}

}  // namespace mpmpc
