// Lidar localisation of the device rollout: scan matching.  Every scheduled step a running car scans its TRUE world (K0l itself)
// and matches the scan against the map it knows in advance - the BASE map, as a capped squared-distance field (K0d) -, starting
// from dead reckoning; the FIX it finds is what the pose filter (K3e) measures and the controller localises on.  The
// measurement error then depends on what the car can see.  Scalar code that compiles for gfx950 (K0d / K3l,
// mpmpc_localiser.hpp) and for the host (tests/emul_localiser), like estimator_core.hpp.  The build has -ffp-contract=off: every
// product and sum below is rounded on its own, in exactly the order stated.
//
// SETTING, per fleet (LcSet, lc_check_setting): a lidar - n_beams, angles[], range_m under K0l's own checks (lid_check_beams) -;
//   D in [1, 15] cells, the reach of the field;  m >= 1, the translation step in cells;  W in [0, 16] and T in [0, 8], the half
//   widths of the window in translation steps and in heading steps;  step_psi >= 0 rad (> 0 when T > 0);  min_hits >= 1;
//   sigma_r >= 0 m;  period >= 1;  seed, car0, step0 as the plant's (plant_core.hpp);  optional fix0 [B][3], which PRIMES the
//   cars (a resumed run).  (2 T + 1) n_beams <= LC_MAX_ENDPOINTS = 8 192; everything finite.
//
// K0d, THE FIELD of the base map (lc_field_cell), integers only: for a cell (i, j) of the grid
//       F[j][i] = min(cap, min d2),   cap = D * D + 1
//   the inner minimum over the occupied in-grid cells (i', j') with |i' - i| <= D, |j' - j| <= D and d2 = (i' - i)^2 +
//   (j' - j)^2 <= D^2.  One byte per cell (cap <= 226).  A look-up outside the grid returns cap (lc_field_at).
//
// K3l, ONE STEP (lc_step) of a car with alive == 1, at the start of step k, behind K3n and in front of K3e / K3d / K3a.
//   j = k - step0.  (v, delta): the command the controller believes reached the wheels in step k - 1, K3e's rule exactly - u of
//   the rollout's state, or entry c of the delay register, c the car's assumed delay (estimator_core.hpp).
//   1  PRIOR.  Not primed: fix = prior = the true pose as the step finds it; primed = 1; go to 5 (no scan is used).  A setting
//      with fix0 starts the cars primed with it.  Primed: prior = dl_nominal on the last fix with (v, delta) - ro_drive ITSELF.
//   2  SCHEDULE.  j mod period != 0 (the modulus non-negative): fix = prior, no scan is used, go to 5.
//   3  SCAN.  ranges[b]: K0l's own kernel on the TRUE pose in the car's TRUE world of step k.  Beam b is a HIT iff
//      ranges[b] < range_m (a NaN is none).  A hit's range becomes r = ranges[b] + sigma_r * n_b, n_b the plant's variate
//      (pl_variate) of word (b & 3) of Philox block 16 + (b >> 2) of (seed, car0 + car, j); plant_core.hpp reserves blocks
//      16 .. 527 (LID_MAX_BEAMS / 4 of them).  The other beams keep K0l's value.  hits < min_hits, or a prior that is not
//      finite: fix = prior, lost += 1, go to 5.
//   4  MATCH (lc_match).  For t in [-T, T]: psi_t = prior_psi + (double)t * step_psi.  For every hit: th = psi_t + angles[b],
//      ex = prior_x + r * cos(th), ey = prior_y + r * sin(th), (ci, cj) = cor_w2m's floor expression of (ex, ey); an endpoint
//      that is not finite or beyond MOV_CELL_MAX is BAD and scores cap for every translation (lc_endpoint).  For a, c in
//      [-W, W]:   score(a, c, t) = sum over the hits of F(ci + a * m, cj + c * m)     in int32 - translations are integer
//      shifts of the endpoint cells BY DEFINITION, nothing is re-evaluated in floating point.  The winner is the minimum of the
//      key (score, a^2 + c^2, t^2, idx), idx = ((t + T) (2 W + 1) + (c + W)) (2 W + 1) + (a + W) - one 64-bit integer, lc_key -,
//      so where the scan cannot tell the fix stays at dead reckoning.
//          fix = (prior_x + (double)(a * m) * res,  prior_y + (double)(c * m) * res,  psi_t)        the heading left unwrapped
//      matched += 1;  the winner on the window's border (|a| == W > 0, |c| == W > 0 or |t| == T > 0): edge += 1.
//      The half-cell bias between the lidar's cell-centre ranges and the continuous prior is NOT corrected: the capped squared
//      distance absorbs it, and this law is what the twin pins.
//   5  STATISTICS, from the true pose (x, y, psi):  steps += 1;  e2 = (fix_x - x)^2 + (fix_y - y)^2, err2_sum += e2,
//      err2_max = max(err2_max, e2);  head2_sum += es_wrap(fix_psi, psi)^2;  prior2_sum += (prior_x - x)^2 + (prior_y - y)^2 -
//      what dead reckoning alone would have given in that step.
//   What a step leaves besides: prior;  cand = idx of the winner, score = its score (both -1 on a step without a match);
//   hits = the number of hits (-1 on a step without a scan).
//
// PROPERTIES.  Off changes no bit.  The field, the scores, the winner and the counters are integers: the device and the host
//   agree bit for bit wherever their cos / sin put every endpoint into the same cell.  One call equals many: a result depends on
//   (seed, car0 + car, j) and the car's own state only.
//
// WHAT THE SCAN IS.  K0l is the reference's lidar, bit for bit, and that wraps a cell's angle atan2(dy, dx) - psi by MIRRORING it
//   when it is below -pi (lidar_core.hpp, step 3).  At a heading in [-pi, 0] no angle falls below -pi and the scan is geometrically
//   the map's; at a heading above 0 - and at every heading ro_drive has carried beyond +-pi, which it leaves unwrapped - the
//   cells behind the car on its right are reported by the beams behind it on its left, and the match is fed a scan that is not
//   the map's: it then pulls the fix away ("K0d / K3l", has the figures).  The law matches what the sensor reports;
//   it does not repair the sensor.
//
// OUT OF SCOPE: per-car settings; matching against known discs or walls, or against what perception has seen; sub-cell
//   refinement of the winner; one scan shared between perception and the localiser; the fix in the trace; sharded.py; the
//   emulation handles.
#pragma once
#include <vector>

#include "estimator_core.hpp"
#include "lidar_core.hpp"

namespace mpmpc {

constexpr int LC_MAX_D = 15, LC_MAX_W = 16, LC_MAX_T = 8;
constexpr int LC_MAX_ENDPOINTS = 8192;      // (2 T + 1) * n_beams: K3l keeps the endpoint cells in LDS
constexpr int LC_BLOCK0 = 16;               // the first Philox block of the range noise
constexpr int LC_STATS = 4;                 // err2_max, err2_sum, head2_sum, prior2_sum
constexpr int LC_COUNTS = 4;                // steps, matched, lost, edge
constexpr int LC_SKIP = (int)0x80000000, LC_BAD = (int)0x80000001;      // ci of a beam that is no hit / of a BAD endpoint

struct LcSet {
  int D, m, W, T, min_hits;
  double step_psi, sigma_r;
};

MPMPC_HOST_DEVICE inline int lc_cap(int D) { return D * D + 1; }

// K0d for one cell of the grid
MPMPC_HOST_DEVICE inline int lc_field_cell(const MapView& map, int i, int j, int D) {
  int best = lc_cap(D);
  const int j0 = j - D < 0 ? 0 : j - D, j1 = j + D > map.height - 1 ? map.height - 1 : j + D;
  const int i0 = i - D < 0 ? 0 : i - D, i1 = i + D > map.width - 1 ? map.width - 1 : i + D;
  for (int jj = j0; jj <= j1; ++jj)
    for (int ii = i0; ii <= i1; ++ii) {
      const int d2 = (ii - i) * (ii - i) + (jj - j) * (jj - j);
      if (d2 < best && d2 <= D * D && map.data[(long long)jj * map.width + ii] == 0) best = d2;
    }
  return best;
}

MPMPC_HOST_DEVICE inline int lc_field_at(const uint8_t* F, int width, int height, int cap, long long i, long long j) {
  return i >= 0 && i < width && j >= 0 && j < height ? (int)F[j * width + i] : cap;
}

// the noisy range of hit b
MPMPC_HD double lc_noisy(double range, double sigma_r, uint64_t seed, uint32_t car, long long j, int b) {
  uint32_t w[4];
  pl_philox((uint32_t)seed, (uint32_t)(seed >> 32), car, (uint32_t)(unsigned long long)j, (uint32_t)((unsigned long long)j >> 32),
            (uint32_t)(LC_BLOCK0 + (b >> 2)), w);
  const int q = b & 3;      // (selects: a run-time index would put w[] on the stack)
  return range + sigma_r * pl_variate(q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3]);
}

MPMPC_HOST_DEVICE inline bool lc_scheduled(long long j, long long period) {
  long long r = j % period;
  if (r < 0) r += period;
  return r == 0;
}

// the endpoint cell of a hit of range r under the heading psi_t; false: BAD.  (qx, qy): the cell coordinates before the floor
MPMPC_HD bool lc_endpoint(const MapView& map, double px, double py, double psi_t, double angle, double r, int* ci, int* cj, double* qx,
                          double* qy) {
  const double th = psi_t + angle;
  const double ex = px + r * std::cos(th), ey = py + r * std::sin(th);
  *qx = (ex - map.ox) / map.res;
  *qy = (ey - map.oy) / map.res;
  const double fx = std::floor(*qx), fy = std::floor(*qy);
  if (!(std::fabs(fx) <= MOV_CELL_MAX && std::fabs(fy) <= MOV_CELL_MAX)) return false;      // (a NaN fails too)
  *ci = (int)fx; *cj = (int)fy;
  return true;
}

// the key of candidate (a, c, t): score < 2^21 (8 192 endpoints of at most 226), a^2 + c^2 <= 512, t^2 <= 64, idx < 2^15
MPMPC_HOST_DEVICE inline unsigned long long lc_key(int score, int a, int c, int t, int idx) {
  return ((unsigned long long)score << 32) | ((unsigned long long)(a * a + c * c) << 22) | ((unsigned long long)(t * t) << 15) |
         (unsigned long long)idx;
}
MPMPC_HOST_DEVICE inline void lc_candidate(int idx, int W, int T, int* a, int* c, int* t) {
  const int n = 2 * W + 1;
  *a = idx % n - W;
  *c = (idx / n) % n - W;
  *t = idx / (n * n) - T;
}
MPMPC_HOST_DEVICE inline int lc_candidates(int W, int T) { return (2 * T + 1) * (2 * W + 1) * (2 * W + 1); }
MPMPC_HOST_DEVICE inline bool lc_on_edge(int a, int c, int t, int W, int T) {
  return (W > 0 && (a == W || a == -W || c == W || c == -W)) || (T > 0 && (t == T || t == -T));
}
MPMPC_HOST_DEVICE inline bool lc_pose_finite(const double* p) { return mov_finite(p[0]) && mov_finite(p[1]) && mov_finite(p[2]); }

// the fix of candidate (a, c, t)
MPMPC_HOST_DEVICE inline void lc_fix(const double* prior, const LcSet& s, double res, int a, int c, int t, double* fix) {
  fix[0] = prior[0] + (double)((long long)a * s.m) * res;
  fix[1] = prior[1] + (double)((long long)c * s.m) * res;
  fix[2] = prior[2] + (double)t * s.step_psi;
}

// 5.  st [LC_STATS], cnt [LC_COUNTS]: the car's
MPMPC_HD void lc_stats(const double* fix, const double* prior, const double* pose, double* st, int* cnt) {
  cnt[0] += 1;
  const double ex = fix[0] - pose[0], ey = fix[1] - pose[1];
  const double e2 = ex * ex + ey * ey;
  st[1] += e2;
  if (e2 > st[0]) st[0] = e2;
  const double hd = es_wrap(fix[2], pose[2]);
  st[2] += hd * hd;
  const double qx = prior[0] - pose[0], qy = prior[1] - pose[1];
  st[3] += qx * qx + qy * qy;
}

#ifndef __HIPCC__      // (host builds only: the library states the same with a workgroup, mpmpc_localiser.hpp)
// 3 (the hits only) and 4, one car, serially: the host's statement of what K3l's workgroup computes.  r [n_beams]: the ranges
// (a hit's already noisy), hit [n_beams] (null: r[b] < range_m).  fix [3], *cand, *score as a step leaves them; returns the number
// of hits.  min_edge (may be null): the smallest distance, in cells, of a used endpoint's (qx, qy) to a cell boundary - the
// band inside which another libm's cos / sin may choose another cell (+inf when no endpoint was used).
inline int lc_match(const MapView& map, const uint8_t* F, const LcSet& s, int n_beams, const double* angles, double range_m, const double* r,
                    const unsigned char* hit, const double* prior, double* fix, int* cand, int* score, double* min_edge) {
  int hits = 0;
  for (int b = 0; b < n_beams; ++b) hits += (hit ? hit[b] != 0 : r[b] < range_m) ? 1 : 0;
  fix[0] = prior[0]; fix[1] = prior[1]; fix[2] = prior[2];
  *cand = -1; *score = -1;
  if (min_edge) *min_edge = HUGE_VAL;
  if (hits < s.min_hits || !lc_pose_finite(prior)) return hits;
  const int cap = lc_cap(s.D), n = 2 * s.W + 1;
  unsigned long long best = ~0ull;
  for (int t = -s.T; t <= s.T; ++t) {
    const double psi_t = prior[2] + (double)t * s.step_psi;
    for (int c = -s.W; c <= s.W; ++c)
      for (int a = -s.W; a <= s.W; ++a) {
        int sc = 0;
        for (int b = 0; b < n_beams; ++b) {
          if (!(hit ? hit[b] != 0 : r[b] < range_m)) continue;
          int ci, cj;
          double qx, qy;
          if (!lc_endpoint(map, prior[0], prior[1], psi_t, angles[b], r[b], &ci, &cj, &qx, &qy)) { sc += cap; continue; }
          if (min_edge) {
            const double dx = qx - std::floor(qx), dy = qy - std::floor(qy);
            const double d = std::fmin(std::fmin(dx, 1.0 - dx), std::fmin(dy, 1.0 - dy));
            if (d < *min_edge) *min_edge = d;
          }
          sc += lc_field_at(F, map.width, map.height, cap, (long long)ci + (long long)a * s.m, (long long)cj + (long long)c * s.m);
        }
        const int idx = ((t + s.T) * n + (c + s.W)) * n + (a + s.W);
        const unsigned long long key = lc_key(sc, a, c, t, idx);
        if (key < best) best = key;
      }
  }
  int a, c, t;
  *cand = (int)(best & 0x7fffu);
  *score = (int)(best >> 32);
  lc_candidate(*cand, s.W, s.T, &a, &c, &t);
  lc_fix(prior, s, map.res, a, c, t, fix);
  return hits;
}

// One car's step on the host.  ranges [n_beams]: K0l's scan of the step (read on a scheduled step only; hits are made noisy IN
// PLACE).  cmd [2]: (v, delta) of 1.  State: fix [3], *primed, st [LC_STATS], cnt [LC_COUNTS]; the step also leaves prior [3],
// *cand, *score, *hits.
inline void lc_step(const MapView& map, const uint8_t* F, const LcSet& s, long long period, uint64_t seed, uint32_t car, long long j, double L,
                    double Ts, int n_beams, const double* angles, double range_m, double* ranges, const double* pose, const double* cmd,
                    double* fix, double* prior, int* primed, int* cand, int* score, int* hits, double* st, int* cnt) {
  *cand = -1; *score = -1; *hits = -1;
  if (!*primed) {
    for (int e = 0; e < 3; ++e) fix[e] = prior[e] = pose[e];
    *primed = 1;
  } else {
    const double zero[3] = {0.0, 0.0, 0.0};
    double sd = 0.0;
    for (int e = 0; e < 3; ++e) prior[e] = fix[e];
    dl_nominal(L, Ts, cmd[0], cmd[1], zero, 0.0, prior, &sd);
    if (!lc_scheduled(j, period)) {
      for (int e = 0; e < 3; ++e) fix[e] = prior[e];
    } else {
      std::vector<unsigned char> hit((size_t)n_beams);
      for (int b = 0; b < n_beams; ++b) {
        hit[b] = ranges[b] < range_m ? 1 : 0;
        if (hit[b]) ranges[b] = lc_noisy(ranges[b], s.sigma_r, seed, car, j, b);
      }
      *hits = lc_match(map, F, s, n_beams, angles, range_m, ranges, hit.data(), prior, fix, cand, score, nullptr);
      if (*cand < 0) {
        cnt[2] += 1;
      } else {
        int a, c, t;
        lc_candidate(*cand, s.W, s.T, &a, &c, &t);
        cnt[1] += 1;
        if (lc_on_edge(a, c, t, s.W, s.T)) cnt[3] += 1;
      }
    }
  }
  lc_stats(fix, prior, pose, st, cnt);
}

#endif

// Host-side validation of the setting (mpmpc_rollout_set_localiser; mpmpc_scan_match takes period = 1, sigma_r = 0).  res: the
// map's resolution.  Returns 0 or -1 (MPMPC_E_ARG) and the reason.
inline int lc_check_setting(int n_beams, const double* angles, double range_m, double res, const LcSet& s, long long period, int B,
                            const double* fix0, const char** why) {
  if (int rc = lid_check_beams(n_beams, angles, range_m, res, why)) return rc;
  if (s.D < 1 || s.D > LC_MAX_D) { *why = "localiser: D must be in [1, 15] cells"; return -1; }
  if (s.m < 1) { *why = "localiser: the translation step must be >= 1 cell"; return -1; }
  if (s.W < 0 || s.W > LC_MAX_W) { *why = "localiser: the window W must be in [0, 16]"; return -1; }
  if (s.T < 0 || s.T > LC_MAX_T) { *why = "localiser: the headings T must be in [0, 8]"; return -1; }
  if (!(s.step_psi >= 0.0) || !mov_finite(s.step_psi) || (s.T > 0 && !(s.step_psi > 0.0))) {
    *why = "localiser: step_psi must be finite and >= 0, and > 0 when T > 0"; return -1;
  }
  if (s.min_hits < 1) { *why = "localiser: min_hits must be >= 1"; return -1; }
  if (!(s.sigma_r >= 0.0) || !mov_finite(s.sigma_r)) { *why = "localiser: sigma_r must be finite and >= 0"; return -1; }
  if (period < 1) { *why = "localiser: period must be >= 1"; return -1; }
  if ((long long)(2 * s.T + 1) * n_beams > LC_MAX_ENDPOINTS) { *why = "localiser: (2 T + 1) * n_beams must be at most 8192"; return -1; }
  if (fix0)
    for (long i = 0; i < 3L * B; ++i)
      if (!mov_finite(fix0[i])) { *why = "localiser: fix0 must be finite"; return -1; }
  return 0;
}

}  // namespace mpmpc
