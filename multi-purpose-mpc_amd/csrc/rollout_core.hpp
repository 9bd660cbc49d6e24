// Closed-loop step around the QP solve, scalar per-instance code that compiles for gfx950 (K3
// kernels in mpmpc_closed_loop.hpp) and for the host (tests/emul).  Replaces, for B cars at once, what
// src/simulation.py:134-140 does per step on the host:
//   localise   SpatialBicycleModel.get_current_waypoint   src/spatial_bicycle_models.py:256-279
//              SpatialBicycleModel.t2s                    src/spatial_bicycle_models.py:183-219
//   advance    MPC.get_control's use of the solution / the infeasibility fallback  src/MPC.py:185-220
//              SpatialBicycleModel.drive                  src/spatial_bicycle_models.py:221-244
#pragma once
#include <cmath>

#include "corridor_core.hpp"      // RouteView

namespace mpmpc {

constexpr double RO_PI = 3.141592653589793;

// Closest of the two waypoints enclosing arc length s (ties to the earlier one).  cum = cumulative
// segment lengths, cum[0] = 0.  Returns -1 when s is past the end of the path (the reference's loop
// guard `car.s < reference_path.length` stops before that).
MPMPC_HD int ro_current_waypoint(const double* cum, int n_wp, double s) {
  int lo = 0, hi = n_wp;                 // first index with cum > s
  while (lo < hi) {
    int mid = (lo + hi) / 2;
    if (cum[mid] > s) hi = mid; else lo = mid + 1;
  }
  const int nxt = lo;
  if (nxt >= n_wp) return -1;
  const int prv = nxt - 1;
  const double c_prev = prv >= 0 ? cum[prv] : cum[n_wp - 1];     // numpy's negative index wraps
  const bool take_next = std::fabs(s - cum[nxt]) < std::fabs(s - c_prev);
  return take_next ? nxt : (prv >= 0 ? prv : n_wp - 1);
}

// True when a car at waypoint wp can no longer be controlled on an OPEN path: the horizon's last stage would read
// waypoint wp + N >= n_wp, where the reference's get_waypoint prints "Reached end of path!" and calls exit(1)
// (src/reference_path.py:367-369, reached from MPC._init_problem, src/MPC.py:93-94).  A circular path never ends.
MPMPC_HD bool ro_past_open_end(int n_wp, int N, bool circular, int wp) { return !circular && wp + N >= n_wp; }

MPMPC_HD void ro_t2s(double px, double py, double ppsi, double wx, double wy, double wpsi, double* x0) {
  x0[0] = std::cos(wpsi) * (py - wy) - std::sin(wpsi) * (px - wx);
  double t = std::fmod(ppsi - wpsi + RO_PI, 2.0 * RO_PI);       // np.mod: result has the divisor's sign
  if (t < 0.0) t += 2.0 * RO_PI;
  x0[1] = t - RO_PI;
  x0[2] = 0.0;
}

// One car, after the solve.  cc [2N] is MPC.current_control (updated in place), z the primal
// solution, x0 / kappa_wp the pre-step spatial state and the curvature of the current waypoint.
// Split in two so that the device can give every plan entry its own thread (ro_plan_entry for k = 0..N-1, then
// ro_drive by the thread that wrote entry 0); ro_advance is the same thing for one thread per car.
MPMPC_HD bool ro_usable(int status) { return status == 1 || status == 2 || status == -2; }
MPMPC_HD void ro_plan_entry(int N, double L, const double* z, double* cc, int k) {
  const double* uu = z + 3 * (N + 1);
  cc[2 * k] = uu[2 * k];
  cc[2 * k + 1] = std::atan(uu[2 * k + 1] * L);
}
// Returns false when the run ends (N-1 consecutive infeasible steps: the reference calls exit(1)).
MPMPC_HD bool ro_drive(int N, double L, double Ts, int status, const double* cc, int* counter, const double* x0,
                       double kappa_wp, double* pose, double* s, double* u_out) {
  double v, delta;
  if (ro_usable(status)) {
    v = cc[0];
    delta = cc[1];
    *counter = 0;
  } else {
    const int i = 2 * (*counter + 1);
    v = cc[i];
    delta = cc[i + 1];
    *counter += 1;
  }
  u_out[0] = v;
  u_out[1] = delta;
  if (*counter == N - 1) return false;
  const double psi = pose[2];
  pose[0] += (v * std::cos(psi)) * Ts;
  pose[1] += (v * std::sin(psi)) * Ts;
  pose[2] += (v / L * std::tan(delta)) * Ts;
  const double s_dot = 1.0 / (1.0 - x0[0] * kappa_wp) * v * std::cos(x0[1]);
  *s += s_dot * Ts;
  return true;
}
MPMPC_HD bool ro_advance(int N, double L, double Ts, int status, const double* z, double* cc, int* counter,
                         const double* x0, double kappa_wp, double* pose, double* s, double* u_out) {
  if (ro_usable(status))
    for (int k = 0; k < N; ++k) ro_plan_entry(N, L, z, cc, k);
  return ro_drive(N, L, Ts, status, cc, counter, x0, kappa_wp, pose, s, u_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Recorder (mpmpc_rollout_record): one record per car and recorded step, written while the cars drive.
//   ro_record_begin    before localise: s, pose and alive as the step finds them (localise / advance overwrite them)
//   ro_record_finish   after advance: everything else, masked by how the step went for the car (include/mpmpc.h)
// Both are written for ONE ENTRY of one car, so that the device gives every entry its own thread (consecutive
// threads store consecutive words) and the host twin (tests/emul_trace) loops over the same code.
// "Empty": NaN for doubles, -1 for wp_id, 0 for status.
constexpr int RO_REC_PLAN = 1, RO_REC_PRED = 2, RO_REC_ROWS = 4, RO_REC_ALL = 7;
constexpr int RO_REC_BEGIN_ENTRIES = 4;      // s, pose[3]
constexpr int RO_REC_FIXED_ENTRIES = 9;      // x0[3], u[2], wp_id, status, counter, alive

// Byte offsets of the fields inside one record of B cars; every field lies as the host arrays of mpmpc_rollout_trace
// do ([B] or [B][len], car-major), so a range of records comes back with one strided copy per field.  -1: not recorded.
struct RoTraceLayout {
  long long s, pose, x0, u, wp_id, status, counter, alive, plan, pred_x, pred_y, ub, lb;
  long long bytes;      // of one record (a multiple of 256)
  int entries;          // per car in ro_record_finish
};
inline RoTraceLayout ro_trace_layout(int N, int B, int fields) {
  RoTraceLayout l;
  long long at = 0;
  auto take = [&](long long per_car) { const long long o = at; at += (per_car * B + 255) / 256 * 256; return o; };
  l.s = take(8); l.pose = take(24); l.x0 = take(24); l.u = take(16);
  l.wp_id = take(4); l.status = take(4); l.counter = take(4); l.alive = take(4);
  l.plan = (fields & RO_REC_PLAN) ? take(16LL * N) : -1;
  l.pred_x = (fields & RO_REC_PRED) ? take(8LL * (N - 2)) : -1;
  l.pred_y = (fields & RO_REC_PRED) ? take(8LL * (N - 2)) : -1;
  l.ub = (fields & RO_REC_ROWS) ? take(8LL * N) : -1;
  l.lb = (fields & RO_REC_ROWS) ? take(8LL * N) : -1;
  l.bytes = at;
  l.entries = RO_REC_FIXED_ENTRIES + ((fields & RO_REC_PLAN) ? 2 * N : 0) + ((fields & RO_REC_PRED) ? 2 * (N - 2) : 0) +
              ((fields & RO_REC_ROWS) ? 2 * N : 0);
  return l;
}

// what a record's fields may hold, from the car's alive before (a_in) and after (a) the step
MPMPC_HD bool ro_rec_state(int a_in) { return a_in == 1; }                                   // s, pose
MPMPC_HD bool ro_rec_input(int a_in, int a) { return a_in == 1 && a != 0; }                  // wp_id, x0
MPMPC_HD bool ro_rec_solved(int a_in, int a) { return a_in == 1 && (a == 1 || a == -1); }    // status, u, plan, rows
MPMPC_HD bool ro_rec_pred(int a_in, int a, int status) { return ro_rec_solved(a_in, a) && ro_usable(status); }
MPMPC_HD double ro_rec_nan() { return __builtin_nan(""); }

// BicycleModel.s2t of (e_y, waypoint), as MPC.update_prediction applies it (src/MPC.py:224-248): world x / y
MPMPC_HD void ro_pred_point(double wx, double wy, double cos_w, double sin_w, double e_y, double* px, double* py) {
  *px = wx - e_y * sin_w;
  *py = wy + e_y * cos_w;
}

// entry c of car i: 0 = s, 1 .. 3 = pose; c == 0 also keeps a_in for ro_record_finish
MPMPC_HD void ro_record_begin(const double* s, const double* pose, const int* alive, int* a_in, char* rec,
                              const RoTraceLayout& l, int i, int c) {
  const int a = alive[i];
  const bool have = ro_rec_state(a);
  if (c == 0) {
    a_in[i] = a;
    ((double*)(rec + l.s))[i] = have ? s[i] : ro_rec_nan();
  } else {
    ((double*)(rec + l.pose))[3LL * i + c - 1] = have ? pose[3LL * i + c - 1] : ro_rec_nan();
  }
}

// what ro_record_finish reads: the rollout's state after advance, the step's solution, the path's tables
struct RoRecSrc {
  const int *alive, *a_in, *wp_id, *status, *counter;
  const double *x0, *u, *cc, *z;            // z [B][5N+3]
  const double *gx, *gy, *trig;             // per waypoint; trig [n_wp][trig_ld] = cos(psi), sin(psi), ...
  const double *row_ub, *row_lb;            // corridor rows: row `wp_id` of the table, or row `car` of the per-car rows
  long long row_ld;
  int per_car, trig_ld, N, n_wp, circular;
  const int* route = nullptr;               // route fleets: {first row, length - negated when open} per car (PathTables::route)
};

// entry e of car i, in the order x0[3], u[2], wp_id, status, counter, alive, then plan / pred_x / pred_y / ub / lb as recorded
MPMPC_HD void ro_record_finish(const RoRecSrc& r, char* rec, const RoTraceLayout& l, int i, int e) {
  const int N = r.N;
  const int a_in = r.a_in[i], a = r.alive[i];
  const bool input = ro_rec_input(a_in, a), solved = ro_rec_solved(a_in, a);
  const double nan = ro_rec_nan();
  if (e < 3) { ((double*)(rec + l.x0))[3LL * i + e] = input ? r.x0[3LL * i + e] : nan; return; }
  if (e < 5) { ((double*)(rec + l.u))[2LL * i + e - 3] = solved ? r.u[2LL * i + e - 3] : nan; return; }
  if (e == 5) { ((int*)(rec + l.wp_id))[i] = input ? r.wp_id[i] : -1; return; }
  if (e == 6) { ((int*)(rec + l.status))[i] = solved ? r.status[i] : 0; return; }
  if (e == 7) { ((int*)(rec + l.counter))[i] = r.counter[i]; return; }
  if (e == 8) { ((int*)(rec + l.alive))[i] = a; return; }
  e -= RO_REC_FIXED_ENTRIES;
  if (l.plan >= 0) {
    if (e < 2 * N) { ((double*)(rec + l.plan))[2LL * N * i + e] = solved ? r.cc[2LL * N * i + e] : nan; return; }
    e -= 2 * N;
  }
  if (l.pred_x >= 0) {
    if (e < 2 * (N - 2)) {
      const bool is_y = e >= N - 2;
      const int k = (is_y ? e - (N - 2) : e) + 2;      // stage 2 .. N-1
      double v = nan;
      if (ro_rec_pred(a_in, a, r.status[i])) {
        // (the car's route: wrap / clamp inside it, its first row added last.  Written out, not route_view: the kernel's
        // instructions change with every form of it - docs/HISTORY.md)
        const int nn = r.route ? r.route[2 * i + 1] : 0;
        const int n = r.route ? (nn > 0 ? nn : -nn) : r.n_wp;
        const bool circular = r.route ? nn > 0 : r.circular != 0;
        int w = r.wp_id[i] + k;
        if (w >= n) w = circular ? w % n : n - 1;
        if (r.route) w += r.route[2 * i];
        double px, py;
        ro_pred_point(r.gx[w], r.gy[w], r.trig[(long long)w * r.trig_ld], r.trig[(long long)w * r.trig_ld + 1],
                      r.z[(5LL * N + 3) * i + 3 * k], &px, &py);
        v = is_y ? py : px;
      }
      ((double*)(rec + (is_y ? l.pred_y : l.pred_x)))[(long long)(N - 2) * i + k - 2] = v;
      return;
    }
    e -= 2 * (N - 2);
  }
  if (l.ub >= 0 && e < 2 * N) {
    const bool is_lb = e >= N;
    const int k = is_lb ? e - N : e;
    const long long row = r.per_car ? i : (solved ? r.wp_id[i] + (int)route_view(r.route, i, r.n_wp, r.circular).first : 0);
    const double* src = is_lb ? r.row_lb : r.row_ub;
    ((double*)(rec + (is_lb ? l.lb : l.ub)))[(long long)N * i + k] = solved ? src[row * r.row_ld + k] : nan;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The pose chain in the record (include/mpmpc.h, MPMPC_REC_PLANT .. MPMPC_REC_SCAN): what the plant, the delay, the estimator and
// the localiser left in their own buffers when the step ended - every value the one the feature's getter would return right
// after the step.  The chain lies BEHIND the record ro_trace_layout describes (RoTraceLayout and the two kernels that take it by
// value do not know of it): its offsets count from the chain's start, which is RoTraceLayout::bytes into the record, and a
// record's stride is the sum of the two.
//   ro_record_chain    after advance, behind ro_record_finish: one ENTRY of one car, like the two above
// "Empty": NaN for doubles, -2 for cand / score / hits (-1 keeps its meanings there), -1 for used.
constexpr int RO_REC_PLANT = 8, RO_REC_DELAY = 16, RO_REC_EST = 32, RO_REC_FIX = 64, RO_REC_SCAN = 128;
constexpr int RO_REC_CHAIN = RO_REC_PLANT | RO_REC_DELAY | RO_REC_EST | RO_REC_FIX | RO_REC_SCAN, RO_REC_EVERY = RO_REC_ALL | RO_REC_CHAIN;
constexpr int RO_CHAIN_QUEUE = 8;      // the command register's entries (DL_MAX of delay_core.hpp, which includes this header)
constexpr int RO_CHAIN_COV = 6;        // the covariance's upper triangle (ES_COV of estimator_core.hpp)

struct RoChainLayout {
  long long act, meas, queue, pred_pose, pred_s, now, est, cov, used, fix, prior, cand, score, hits, ranges;      // -1: not recorded
  long long bytes;      // of the chain of one record (a multiple of 256; 0: no chain bit)
  int entries;          // per car in ro_record_chain
  int n_beams;          // of `ranges`
};
inline RoChainLayout ro_chain_layout(int B, int fields, int n_beams) {
  RoChainLayout l;
  long long at = 0;
  auto take = [&](int bit, long long per_car) {
    if (!(fields & bit)) return -1LL;
    const long long o = at;
    at += (per_car * B + 255) / 256 * 256;
    return o;
  };
  l.act = take(RO_REC_PLANT, 16); l.meas = take(RO_REC_PLANT, 24);
  l.queue = take(RO_REC_DELAY, 16LL * RO_CHAIN_QUEUE); l.pred_pose = take(RO_REC_DELAY, 24); l.pred_s = take(RO_REC_DELAY, 8);
  l.now = take(RO_REC_DELAY, 24);
  l.est = take(RO_REC_EST, 24); l.cov = take(RO_REC_EST, 8LL * RO_CHAIN_COV); l.used = take(RO_REC_EST, 4);
  l.fix = take(RO_REC_FIX, 24); l.prior = take(RO_REC_FIX, 24); l.cand = take(RO_REC_FIX, 4); l.score = take(RO_REC_FIX, 4);
  l.hits = take(RO_REC_FIX, 4);
  l.ranges = take(RO_REC_SCAN, 8LL * n_beams);
  l.bytes = at;
  l.n_beams = (fields & RO_REC_SCAN) ? n_beams : 0;
  l.entries = ((fields & RO_REC_PLANT) ? 5 : 0) + ((fields & RO_REC_DELAY) ? 2 * RO_CHAIN_QUEUE + 7 : 0) +
              ((fields & RO_REC_EST) ? 4 + RO_CHAIN_COV : 0) + ((fields & RO_REC_FIX) ? 9 : 0) + l.n_beams;
  return l;
}

// what ro_record_chain reads: a_in (ro_record_begin kept it) and the features' own buffers as the step leaves them.  A group's
// first pointer is null when its feature is not in force at the step: the whole group is then empty for every car.
struct RoChainSrc {
  const int* a_in;
  const double *act, *meas;                          // plant: [B][2], [B][3]
  const double *queue, *pred_pose, *pred_s, *now;    // delay: [B][RO_CHAIN_QUEUE][2], [B][3], [B], [B][3]
  const double *est, *cov;                           // estimator: [B][3], [B][RO_CHAIN_COV]
  const int* used;                                   //   [B]
  const double *fix, *prior;                         // localiser: [B][3] each
  const int *cand, *score, *hits;                    //   [B] each
  const double* ranges;                              //   [B][n_beams], n_beams the layout's
};

// entry e of car i, in the order act[2], meas[3] / queue[2 RO_CHAIN_QUEUE], pred_pose[3], pred_s, now[3] / est[3], cov[RO_CHAIN_COV], used /
// fix[3], prior[3], cand, score, hits / ranges[n_beams], as recorded.  act, queue and used outlive a step and are recorded for every
// car as they stand; the others are the step's own and K3n, K3d, K3e and K3l write them for the cars the step finds running
// (alive == 1) alone; the scan is the step's where its hits are counted (hits >= 0).
MPMPC_HD void ro_record_chain(const RoChainSrc& r, char* rec, const RoChainLayout& l, int i, int e) {
  const bool ran = ro_rec_state(r.a_in[i]);
  const double nan = ro_rec_nan();
  if (l.act >= 0) {
    if (e < 2) { ((double*)(rec + l.act))[2LL * i + e] = r.act ? r.act[2LL * i + e] : nan; return; }
    if (e < 5) { ((double*)(rec + l.meas))[3LL * i + e - 2] = r.act && ran ? r.meas[3LL * i + e - 2] : nan; return; }
    e -= 5;
  }
  if (l.queue >= 0) {
    const bool have = r.queue && ran;
    constexpr int Q = 2 * RO_CHAIN_QUEUE;
    if (e < Q) { ((double*)(rec + l.queue))[(long long)Q * i + e] = r.queue ? r.queue[(long long)Q * i + e] : nan; return; }
    if (e < Q + 3) { ((double*)(rec + l.pred_pose))[3LL * i + e - Q] = have ? r.pred_pose[3LL * i + e - Q] : nan; return; }
    if (e == Q + 3) { ((double*)(rec + l.pred_s))[i] = have ? r.pred_s[i] : nan; return; }
    if (e < Q + 7) { ((double*)(rec + l.now))[3LL * i + e - Q - 4] = have ? r.now[3LL * i + e - Q - 4] : nan; return; }
    e -= Q + 7;
  }
  if (l.est >= 0) {
    const bool have = r.est && ran;
    if (e < 3) { ((double*)(rec + l.est))[3LL * i + e] = have ? r.est[3LL * i + e] : nan; return; }
    if (e < 3 + RO_CHAIN_COV) {
      ((double*)(rec + l.cov))[(long long)RO_CHAIN_COV * i + e - 3] = have ? r.cov[(long long)RO_CHAIN_COV * i + e - 3] : nan;
      return;
    }
    if (e == 3 + RO_CHAIN_COV) { ((int*)(rec + l.used))[i] = r.est ? r.used[i] : -1; return; }
    e -= 4 + RO_CHAIN_COV;
  }
  if (l.fix >= 0) {
    const bool have = r.fix && ran;
    if (e < 3) { ((double*)(rec + l.fix))[3LL * i + e] = have ? r.fix[3LL * i + e] : nan; return; }
    if (e < 6) { ((double*)(rec + l.prior))[3LL * i + e - 3] = have ? r.prior[3LL * i + e - 3] : nan; return; }
    if (e == 6) { ((int*)(rec + l.cand))[i] = have ? r.cand[i] : -2; return; }
    if (e == 7) { ((int*)(rec + l.score))[i] = have ? r.score[i] : -2; return; }
    if (e == 8) { ((int*)(rec + l.hits))[i] = have ? r.hits[i] : -2; return; }
    e -= 9;
  }
  if (l.ranges >= 0 && e < l.n_beams) {
    const bool have = r.fix && ran && r.hits[i] >= 0;
    ((double*)(rec + l.ranges))[(long long)l.n_beams * i + e] = have ? r.ranges[(long long)l.n_beams * i + e] : nan;
  }
}

}  // namespace mpmpc
