// Speed profile of a reference path (K4): per-path code written against an execution policy - one wavefront per
// path on gfx950 (SpWave in mpmpc_speed_profile.hpp: lane-strided loops, shuffle reductions, cyclic reduction for the
// tridiagonal systems), one thread per path for very long paths and on the host (SpSerial; tests/emul).
//
// Replaces ReferencePath.compute_speed_profile (src/reference_path.py:289-354), the reference's second
// OSQP call site:
//     min 1/2 |v|^2 - vmax' v      s.t.  a_min <= (v[i+1] - v[i]) / (2 l_i) <= a_max,   v_min <= v[i] <= vmax_i
// with vmax_i = min(v_max, sqrt(ay_max / (|kappa_i| + eps)))  (src/reference_path.py:326-329), n = n_wp - 1.
// The reference takes whatever OSQP returns at eps = 1e-3; here the problem is solved to a KKT point:
// Mehrotra predictor-corrector on the normal equations - a scalar tridiagonal system, because the
// difference rows couple neighbours only - followed by primal-dual active-set rounds and a KKT
// certificate, the same construction as the polish of K2 (mpmpc_core.hpp).
//
// Workspace: SP_ARRAYS arrays of n doubles per path, element (a, i) of path p at w[(a * n + i) * stride + p]
// (stride = number of paths: consecutive threads touch consecutive addresses).
#pragma once
#include <cmath>

#ifndef MPMPC_HD
#define MPMPC_HD inline
#endif

namespace mpmpc {

enum {
  SP_X, SP_Q, SP_HI, SP_C, SP_SL1, SP_SU1, SP_ZL1, SP_ZU1, SP_SL2, SP_SU2, SP_ZL2, SP_ZU2, SP_RD, SP_MD, SP_ME, SP_DX,
  SP_PL1, SP_PU1, SP_PL2, SP_PU2, SP_RHS, SP_A1, SP_A2, SP_L1, SP_L2, SP_ARRAYS
};

struct SpWork {
  double* w;
  long n, stride;
  MPMPC_HD double& operator()(int a, int i) const { return w[((long)a * n + i) * stride]; }
};

struct SpLimits { double a_min, a_max, v_min, v_max, ay_max; };

constexpr int SP_SOLVED = 1, SP_INACCURATE = 2, SP_BAD_INPUT = -1;

// one row of the interior-point step: slack / multiplier directions from the row's A dx
struct SpRow { double dsl, dsu, dzl, dzu; };
MPMPC_HD SpRow sp_row(double sl, double su, double zl, double zu, double rl, double ru, double rcl, double rcu, double adx) {
  SpRow r;
  r.dsl = adx + rl;
  r.dsu = -adx + ru;
  r.dzl = (-rcl - zl * r.dsl) / sl;
  r.dzu = (-rcu - zu * r.dsu) / su;
  return r;
}
MPMPC_HD double sp_block(double blk, double s, double ds) { return ds < 0.0 ? std::fmax(blk, -ds / s) : blk; }

// Solve M y = rhs in place (rhs in SP_RHS -> solution in SP_DX) with the LDL' factors in SP_MD / SP_ME.
MPMPC_HD void sp_tri_solve(const SpWork& W, int n) {
  W(SP_DX, 0) = W(SP_RHS, 0);
  for (int i = 1; i < n; ++i) W(SP_DX, i) = W(SP_RHS, i) - W(SP_ME, i - 1) * W(SP_DX, i - 1);
  W(SP_DX, n - 1) = W(SP_DX, n - 1) / W(SP_MD, n - 1);
  for (int i = n - 2; i >= 0; --i) W(SP_DX, i) = W(SP_DX, i) / W(SP_MD, i) - W(SP_ME, i) * W(SP_DX, i + 1);
}
// LDL' of the tridiagonal (diag SP_MD, sub-diagonal SP_ME[i] between i and i+1), in place: ME <- l_{i+1}
MPMPC_HD void sp_tri_factor(const SpWork& W, int n) {
  for (int i = 0; i + 1 < n; ++i) {
    const double l = W(SP_ME, i) / W(SP_MD, i);
    W(SP_MD, i + 1) -= l * W(SP_ME, i);
    W(SP_ME, i) = l;
  }
}

// ---- parallel cyclic reduction of the same tridiagonal systems, written per row: at level l (stride s = 2^l) row i
// eliminates its neighbours i - s and i + s, so every row of a level is independent of the others and a policy may run
// the rows of a level in any order - SpWave (mpmpc_speed_profile.hpp) lane-strided on the device, SpCyclicHost below
// one after the other on the host.  "factor" keeps the two multipliers of every row and level and the final reciprocal
// diagonal, "solve" applies them to a right-hand side.  Unlike sp_tri_factor it leaves SP_MD / SP_ME as they were.
// State: sp_cr_arrays(n) arrays of `cap` doubles - A0 B0 C0 A1 B1 C1 (double-buffered rows), D0 D1, BINV, then
// K1[l], K2[l] per level.
constexpr int sp_cr_arrays(int n) {
  int levels = 0;
  for (int s = 1; s < n; s <<= 1) ++levels;
  return 9 + 2 * levels;
}
struct SpCyclic {
  double* x;
  int cap;            // row capacity (n of the launch)
  MPMPC_HD double* arr(int a) const { return x + (long)a * cap; }
};
MPMPC_HD void sp_cr_load_row(const SpWork& W, int n, int i, double* a0, double* b0, double* c0) {
  a0[i] = i > 0 ? W(SP_ME, i - 1) : 0.0;
  b0[i] = W(SP_MD, i);
  c0[i] = i + 1 < n ? W(SP_ME, i) : 0.0;
}
MPMPC_HD void sp_cr_factor_row(int n, int s, int i, const double* a0, const double* b0, const double* c0, double* a1,
                               double* b1, double* c1, double* k1, double* k2) {
  const bool lo = i - s >= 0, hi = i + s < n;
  const double m1 = lo ? a0[i] / b0[i - s] : 0.0, m2 = hi ? c0[i] / b0[i + s] : 0.0;
  k1[i] = m1; k2[i] = m2;
  a1[i] = lo ? -a0[i - s] * m1 : 0.0;
  c1[i] = hi ? -c0[i + s] * m2 : 0.0;
  b1[i] = b0[i] - (lo ? c0[i - s] * m1 : 0.0) - (hi ? a0[i + s] * m2 : 0.0);
}
MPMPC_HD void sp_cr_solve_row(int n, int s, int i, const double* d0, double* d1, const double* k1, const double* k2) {
  d1[i] = d0[i] - (i - s >= 0 ? d0[i - s] * k1[i] : 0.0) - (i + s < n ? d0[i + s] * k2[i] : 0.0);
}
template <class P>
MPMPC_HD void sp_cr_factor(const P& pol, const SpCyclic& cr, const SpWork& W, int n) {
  const int i0 = pol.first(), di = pol.step();
  double *a0 = cr.arr(0), *b0 = cr.arr(1), *c0 = cr.arr(2), *a1 = cr.arr(3), *b1 = cr.arr(4), *c1 = cr.arr(5);
  for (int i = i0; i < n; i += di) sp_cr_load_row(W, n, i, a0, b0, c0);
  pol.sync();
  int l = 0;
  for (int s = 1; s < n; s <<= 1, ++l) {
    double *k1 = cr.arr(9 + 2 * l), *k2 = cr.arr(10 + 2 * l);
    for (int i = i0; i < n; i += di) sp_cr_factor_row(n, s, i, a0, b0, c0, a1, b1, c1, k1, k2);
    pol.sync();
    double* t;
    t = a0; a0 = a1; a1 = t; t = b0; b0 = b1; b1 = t; t = c0; c0 = c1; c1 = t;
  }
  double* binv = cr.arr(8);
  for (int i = i0; i < n; i += di) binv[i] = 1.0 / b0[i];
  pol.sync();
}
// d0 (cr.arr(6)) holds the right-hand side -> the array that holds the solution (d0 or d1)
template <class P>
MPMPC_HD double* sp_cr_apply(const P& pol, const SpCyclic& cr, int n) {
  const int i0 = pol.first(), di = pol.step();
  double *d0 = cr.arr(6), *d1 = cr.arr(7);
  int l = 0;
  for (int s = 1; s < n; s <<= 1, ++l) {
    const double *k1 = cr.arr(9 + 2 * l), *k2 = cr.arr(10 + 2 * l);
    for (int i = i0; i < n; i += di) sp_cr_solve_row(n, s, i, d0, d1, k1, k2);
    pol.sync();
    double* t = d0; d0 = d1; d1 = t;
  }
  const double* binv = cr.arr(8);
  for (int i = i0; i < n; i += di) d0[i] *= binv[i];
  pol.sync();
  return d0;
}
// RHS -> DX, with one step of iterative refinement against the unfactored matrix (SP_MD / SP_ME): the multipliers of the
// reduction are rounded level by level, and on long runs of active acceleration rows (diagonal and off-diagonal of the
// normal equations both ~ z / s, their sum O(1)) the plain solve leaves the interior point a residual floor above its tol.
template <class P>
MPMPC_HD void sp_cr_solve(const P& pol, const SpCyclic& cr, const SpWork& W, int n) {
  const int i0 = pol.first(), di = pol.step();
  double* d0 = cr.arr(6);
  for (int i = i0; i < n; i += di) d0[i] = W(SP_RHS, i);
  pol.sync();
  const double* y = sp_cr_apply(pol, cr, n);
  for (int i = i0; i < n; i += di) W(SP_DX, i) = y[i];
  pol.sync();
  for (int i = i0; i < n; i += di) {
    double r = W(SP_RHS, i) - W(SP_MD, i) * W(SP_DX, i);
    if (i > 0) r -= W(SP_ME, i - 1) * W(SP_DX, i - 1);
    if (i + 1 < n) r -= W(SP_ME, i) * W(SP_DX, i + 1);
    d0[i] = r;
  }
  pol.sync();
  y = sp_cr_apply(pol, cr, n);
  for (int i = i0; i < n; i += di) W(SP_DX, i) += y[i];
  pol.sync();
}

// Execution policy of sp_solve_t.  SpSerial: one thread walks the path (host emulation, and the thread-per-path
// kernel for very long paths).  The device's SpWave (mpmpc_speed_profile.hpp) spreads the elementwise loops over the 64 lanes
// of a wavefront, reduces with shuffles and solves the tridiagonal systems by parallel cyclic reduction.
struct SpSerial {
  MPMPC_HD int first() const { return 0; }
  MPMPC_HD int step() const { return 1; }
  MPMPC_HD void sync() const {}
  MPMPC_HD double rmax(double x) const { return x; }
  MPMPC_HD double rsum(double x) const { return x; }
  MPMPC_HD bool any(bool b) const { return b; }
  MPMPC_HD void tri_factor(const SpWork& W, int n) const { sp_tri_factor(W, n); }
  MPMPC_HD void tri_solve(const SpWork& W, int n) const { sp_tri_solve(W, n); }
};

// The cyclic reduction one row after the other: the host twin of SpWave (tests/emul).  Same per-row arithmetic and the
// same order of levels as the device; only the sums over the path run serially where the device reduces by butterfly.
// `x`: sp_cr_arrays(n) * n doubles.
struct SpCyclicHost {
  SpCyclic cr;
  MPMPC_HD int first() const { return 0; }
  MPMPC_HD int step() const { return 1; }
  MPMPC_HD void sync() const {}
  MPMPC_HD double rmax(double x) const { return x; }
  MPMPC_HD double rsum(double x) const { return x; }
  MPMPC_HD bool any(bool b) const { return b; }
  MPMPC_HD void tri_factor(const SpWork& W, int n) const { sp_cr_factor(*this, cr, W, n); }
  MPMPC_HD void tri_solve(const SpWork& W, int n) const { sp_cr_solve(*this, cr, W, n); }
};

// v[n] <- optimum; returns SP_SOLVED (KKT certificate <= cert_tol), SP_INACCURATE or SP_BAD_INPUT.
// li[i] = |wp[i+1] - wp[i]|, kappa[i], i = 0..n-1; iters (optional) <- interior-point iterations.
// Every loop over the path is elementwise (it reads neighbours only from arrays the loop does not write), so a
// policy may run it strided over several lanes; P.sync() separates the loops.
template <class P>
MPMPC_HD int sp_solve_t(const P& pol, int n, const double* li, const double* kappa, long in_stride, const SpLimits& lim,
                        double eps, const SpWork& W, double* v, long v_stride, int* iters) {
  const int i0 = pol.first(), di = pol.step();
  const double reg = 1e-9, tol = 1e-10, delta = 1e-9, cert_tol = 1e-8;
  if (n < 2 || !(lim.a_min < lim.a_max)) return SP_BAD_INPUT;
  // ---- data
  bool bad_input = false;
  for (int i = i0; i < n; i += di) {
    double hi = lim.v_max;
    const double cap = std::sqrt(lim.ay_max / (std::fabs(kappa[i * in_stride]) + eps));
    if (cap < hi) hi = cap;
    if (!(lim.v_min < hi)) bad_input = true;
    W(SP_HI, i) = hi;
    W(SP_Q, i) = -hi;
    if (i + 1 < n) W(SP_C, i) = 1.0 / (2.0 * li[i * in_stride]);
  }
  if (pol.any(bad_input)) return SP_BAD_INPUT;       // (any() also orders the loop above before the next one)
  const int m1 = n - 1;
  const double nb = 2.0 * (m1 + n);
  // ---- start: x = 0, unit multipliers, slacks at least 1 (as the host solver this replaces)
  for (int i = i0; i < n; i += di) {
    W(SP_X, i) = 0.0;
    W(SP_L2, i) = 0.0;                                   // the iterate of the smallest residual so far (see `best`)
    W(SP_SL2, i) = std::fmax(0.0 - lim.v_min, 1.0); W(SP_SU2, i) = std::fmax(W(SP_HI, i) - 0.0, 1.0);
    W(SP_ZL2, i) = 1.0; W(SP_ZU2, i) = 1.0;
    if (i < m1) {
      W(SP_SL1, i) = std::fmax(0.0 - lim.a_min, 1.0); W(SP_SU1, i) = std::fmax(lim.a_max - 0.0, 1.0);
      W(SP_ZL1, i) = 1.0; W(SP_ZU1, i) = 1.0;
    }
  }
  pol.sync();
  auto ax1 = [&](int a, int k) { return W(SP_C, k) * (W(a, k + 1) - W(a, k)); };
  int it = 0;
  bool converged = false;
  double best = 1e300;
  for (; it < 60; ++it) {
    // ---- residuals, complementarity, normal-equations matrix
    double res = 0.0, musum = 0.0;
    for (int i = i0; i < n; i += di) {
      double rd = W(SP_X, i) + W(SP_Q, i) + (W(SP_ZU2, i) - W(SP_ZL2, i));
      double md = 1.0 + reg + W(SP_ZL2, i) / W(SP_SL2, i) + W(SP_ZU2, i) / W(SP_SU2, i);
      if (i > 0) {
        const double c = W(SP_C, i - 1), w1 = W(SP_ZL1, i - 1) / W(SP_SL1, i - 1) + W(SP_ZU1, i - 1) / W(SP_SU1, i - 1);
        rd += c * (W(SP_ZU1, i - 1) - W(SP_ZL1, i - 1));
        md += w1 * c * c;
      }
      if (i < m1) {
        const double c = W(SP_C, i), w1 = W(SP_ZL1, i) / W(SP_SL1, i) + W(SP_ZU1, i) / W(SP_SU1, i);
        rd -= c * (W(SP_ZU1, i) - W(SP_ZL1, i));
        md += w1 * c * c;
        W(SP_ME, i) = -w1 * c * c;
        const double a = ax1(SP_X, i);
        res = std::fmax(res, std::fmax(std::fabs(a - lim.a_min - W(SP_SL1, i)), std::fabs(lim.a_max - a - W(SP_SU1, i))));
        musum += W(SP_SL1, i) * W(SP_ZL1, i) + W(SP_SU1, i) * W(SP_ZU1, i);
      }
      W(SP_RD, i) = rd;
      W(SP_MD, i) = md;
      res = std::fmax(res, std::fabs(rd));
      res = std::fmax(res, std::fmax(std::fabs(W(SP_X, i) - lim.v_min - W(SP_SL2, i)), std::fabs(W(SP_HI, i) - W(SP_X, i) - W(SP_SU2, i))));
      musum += W(SP_SL2, i) * W(SP_ZL2, i) + W(SP_SU2, i) * W(SP_ZU2, i);
    }
    pol.sync();
    res = pol.rmax(res);
    const double mu = pol.rsum(musum) / nb;
    if (res < tol && mu < tol) { converged = true; break; }
    if (!(res < 1e300)) break;
    // a run that ends without convergence returns its best iterate, not its last (SP_L2 is free until the finish)
    if (res < best) {
      best = res;
      for (int i = i0; i < n; i += di) W(SP_L2, i) = W(SP_X, i);
    }
    pol.tri_factor(W, n);
    double sigmu = 0.0, alpha = 1.0;
    for (int pass = 0; pass < 2; ++pass) {
      // ---- right-hand side  -rd - A' t,  t = (rcl + zl rl) / sl - (rcu + zu ru) / su  per row
      auto t1 = [&](int k) {
        const double a = ax1(SP_X, k), sl = W(SP_SL1, k), su = W(SP_SU1, k), zl = W(SP_ZL1, k), zu = W(SP_ZU1, k);
        const double rcl = sl * zl - sigmu + (pass ? W(SP_PL1, k) : 0.0), rcu = su * zu - sigmu + (pass ? W(SP_PU1, k) : 0.0);
        return (rcl + zl * (a - lim.a_min - sl)) / sl - (rcu + zu * (lim.a_max - a - su)) / su;
      };
      for (int i = i0; i < n; i += di) {
        const double sl = W(SP_SL2, i), su = W(SP_SU2, i), zl = W(SP_ZL2, i), zu = W(SP_ZU2, i), x = W(SP_X, i);
        const double rcl = sl * zl - sigmu + (pass ? W(SP_PL2, i) : 0.0), rcu = su * zu - sigmu + (pass ? W(SP_PU2, i) : 0.0);
        double r = -W(SP_RD, i) - ((rcl + zl * (x - lim.v_min - sl)) / sl - (rcu + zu * (W(SP_HI, i) - x - su)) / su);
        if (i > 0) r -= W(SP_C, i - 1) * t1(i - 1);
        if (i < m1) r += W(SP_C, i) * t1(i);
        W(SP_RHS, i) = r;
      }
      pol.sync();
      pol.tri_solve(W, n);
      // ---- row directions: fraction to the boundary; the predictor also leaves the second-order terms
      double blk = 0.0;
      for (int i = i0; i < n; i += di) {
        {
          const double sl = W(SP_SL2, i), su = W(SP_SU2, i), zl = W(SP_ZL2, i), zu = W(SP_ZU2, i), x = W(SP_X, i);
          const double rcl = sl * zl - sigmu + (pass ? W(SP_PL2, i) : 0.0), rcu = su * zu - sigmu + (pass ? W(SP_PU2, i) : 0.0);
          const SpRow d = sp_row(sl, su, zl, zu, x - lim.v_min - sl, W(SP_HI, i) - x - su, rcl, rcu, W(SP_DX, i));
          blk = sp_block(sp_block(sp_block(sp_block(blk, sl, d.dsl), su, d.dsu), zl, d.dzl), zu, d.dzu);
          if (!pass) { W(SP_PL2, i) = d.dsl * d.dzl; W(SP_PU2, i) = d.dsu * d.dzu; }
        }
        if (i < m1) {
          const double sl = W(SP_SL1, i), su = W(SP_SU1, i), zl = W(SP_ZL1, i), zu = W(SP_ZU1, i), a = ax1(SP_X, i);
          const double rcl = sl * zl - sigmu + (pass ? W(SP_PL1, i) : 0.0), rcu = su * zu - sigmu + (pass ? W(SP_PU1, i) : 0.0);
          const SpRow d = sp_row(sl, su, zl, zu, a - lim.a_min - sl, lim.a_max - a - su, rcl, rcu, ax1(SP_DX, i));
          blk = sp_block(sp_block(sp_block(sp_block(blk, sl, d.dsl), su, d.dsu), zl, d.dzl), zu, d.dzu);
          if (!pass) { W(SP_PL1, i) = d.dsl * d.dzl; W(SP_PU1, i) = d.dsu * d.dzu; }
        }
      }
      pol.sync();
      blk = pol.rmax(blk);
      const double ratio = blk > 0.0 ? 1.0 / blk : 1e300;
      alpha = pass ? std::fmin(1.0, 0.995 * ratio) : std::fmin(1.0, ratio);
      // ---- predictor: centring from the affine complementarity.  corrector: take the step.
      double aff = 0.0;
      for (int i = i0; i < n; i += di) {
        {
          const double sl = W(SP_SL2, i), su = W(SP_SU2, i), zl = W(SP_ZL2, i), zu = W(SP_ZU2, i), x = W(SP_X, i);
          const double rcl = sl * zl - sigmu + (pass ? W(SP_PL2, i) : 0.0), rcu = su * zu - sigmu + (pass ? W(SP_PU2, i) : 0.0);
          const SpRow d = sp_row(sl, su, zl, zu, x - lim.v_min - sl, W(SP_HI, i) - x - su, rcl, rcu, W(SP_DX, i));
          if (!pass) aff += (sl + alpha * d.dsl) * (zl + alpha * d.dzl) + (su + alpha * d.dsu) * (zu + alpha * d.dzu);
          else { W(SP_SL2, i) = sl + alpha * d.dsl; W(SP_SU2, i) = su + alpha * d.dsu; W(SP_ZL2, i) = zl + alpha * d.dzl; W(SP_ZU2, i) = zu + alpha * d.dzu; }
        }
        if (i < m1) {
          const double sl = W(SP_SL1, i), su = W(SP_SU1, i), zl = W(SP_ZL1, i), zu = W(SP_ZU1, i), a = ax1(SP_X, i);
          const double rcl = sl * zl - sigmu + (pass ? W(SP_PL1, i) : 0.0), rcu = su * zu - sigmu + (pass ? W(SP_PU1, i) : 0.0);
          const SpRow d = sp_row(sl, su, zl, zu, a - lim.a_min - sl, lim.a_max - a - su, rcl, rcu, ax1(SP_DX, i));
          if (!pass) aff += (sl + alpha * d.dsl) * (zl + alpha * d.dzl) + (su + alpha * d.dsu) * (zu + alpha * d.dzu);
          else { W(SP_SL1, i) = sl + alpha * d.dsl; W(SP_SU1, i) = su + alpha * d.dsu; W(SP_ZL1, i) = zl + alpha * d.dzl; W(SP_ZU1, i) = zu + alpha * d.dzu; }
        }
      }
      if (!pass) {
        aff = pol.rsum(aff);
        const double s = mu > 0.0 ? (aff / nb) / mu : 0.0;
        sigmu = s * s * s * mu;
      } else {
        // x moves last: the rows above read the old x
        pol.sync();
        for (int i = i0; i < n; i += di) W(SP_X, i) += alpha * W(SP_DX, i);
        pol.sync();
      }
    }
  }
  if (iters && i0 == 0) *iters = it;
  // ---- active-set finish: A1 = -1 / 0 / +1 for a difference row at its lower / no / upper bound, A2 for the boxes.
  // It starts from the interior-point iterate, multipliers included (L = zu - zl).  Where the active rows are linearly
  // dependent - a speed peak exactly on a waypoint: rising rows, falling rows and the boxes at both ends of the stretch -
  // the multipliers are not unique, and the delta-regularised solves below keep the component of their starting point
  // along the dependency.  From zero that component is the minimum-norm one, with wrong signs on a long stretch of rows
  // that the update then releases and re-adds one by one; from the interior point it is the central, strictly signed one.
  for (int i = i0; converged && i < n; i += di) {
    W(SP_A2, i) = W(SP_ZL2, i) > W(SP_SL2, i) ? -1.0 : (W(SP_ZU2, i) > W(SP_SU2, i) ? 1.0 : 0.0);
    W(SP_L2, i) = W(SP_ZU2, i) - W(SP_ZL2, i);
    W(SP_PL2, i) = W(SP_X, i);
    if (i < m1) {
      W(SP_A1, i) = W(SP_ZL1, i) > W(SP_SL1, i) ? -1.0 : (W(SP_ZU1, i) > W(SP_SU1, i) ? 1.0 : 0.0);
      W(SP_L1, i) = W(SP_ZU1, i) - W(SP_ZL1, i);
    }
  }
  pol.sync();
  bool ok = false;
  for (int round = 0; round < 8 && converged && !ok; ++round) {
    // reduced system: boxes by a 1/delta penalty on the diagonal (h), active difference rows through
    // the tridiagonal Schur complement S = A1 diag(h) A1' + delta I  (SP_MD / SP_ME, m1 rows)
    for (int i = i0; i < n; i += di) {
      W(SP_RD, i) = 1.0 / (1.0 + delta + (W(SP_A2, i) != 0.0 ? 1.0 / delta : 0.0));       // h
      if (W(SP_A2, i) == 0.0) W(SP_L2, i) = 0.0;       // (x, lam1, lam2) = (PL2, L1, L2) go on from the round before
      if (i < m1 && W(SP_A1, i) == 0.0) W(SP_L1, i) = 0.0;
    }
    pol.sync();
    for (int k = i0; k < m1; k += di) {
      const double c = W(SP_C, k);
      const bool on = W(SP_A1, k) != 0.0;
      W(SP_MD, k) = on ? c * c * (W(SP_RD, k) + W(SP_RD, k + 1)) + delta : 1.0;
      if (k + 1 < m1) W(SP_ME, k) = (on && W(SP_A1, k + 1) != 0.0) ? -c * W(SP_C, k + 1) * W(SP_RD, k + 1) : 0.0;
    }
    pol.sync();
    pol.tri_factor(W, m1);
    for (int rf = 0; rf < 6; ++rf) {
      // residuals of the KKT system at (x, lam1, lam2) = (PL2, L1, L2); PU2 <- rhs_x, PL1 <- r3
      for (int i = i0; i < n; i += di) {
        double r1 = -W(SP_Q, i) - W(SP_PL2, i) - W(SP_L2, i);
        if (i > 0) r1 -= W(SP_C, i - 1) * W(SP_L1, i - 1);
        if (i < m1) r1 += W(SP_C, i) * W(SP_L1, i);
        const double a2 = W(SP_A2, i);
        const double r3 = a2 != 0.0 ? (a2 > 0.0 ? W(SP_HI, i) : lim.v_min) - W(SP_PL2, i) : 0.0;
        W(SP_PL1, i) = r3;
        W(SP_PU2, i) = r1 + r3 / delta;
      }
      pol.sync();
      for (int k = i0; k < m1; k += di) {
        const double a1 = W(SP_A1, k);
        const double r2 = a1 != 0.0 ? (a1 > 0.0 ? lim.a_max : lim.a_min) - ax1(SP_PL2, k) : 0.0;
        // bv = A1 (h rhs_x) - r2 on the active rows
        const double t0 = W(SP_RD, k) * W(SP_PU2, k), t1 = W(SP_RD, k + 1) * W(SP_PU2, k + 1);
        W(SP_RHS, k) = a1 != 0.0 ? W(SP_C, k) * (t1 - t0) - r2 : 0.0;
      }
      // S dlam = bv  (the tridiagonal solver works on RHS -> DX; m1 rows)
      pol.sync();
      pol.tri_solve(W, m1);
      for (int k = i0; k < m1; k += di) { if (W(SP_A1, k) == 0.0) W(SP_DX, k) = 0.0; W(SP_L1, k) += W(SP_DX, k); }
      pol.sync();
      for (int i = i0; i < n; i += di) {
        double s = 0.0;                                   // (A1' dlam)_i
        if (i > 0) s += W(SP_C, i - 1) * W(SP_DX, i - 1);
        if (i < m1) s -= W(SP_C, i) * W(SP_DX, i);
        const double dx = W(SP_RD, i) * (W(SP_PU2, i) - s);
        if (W(SP_A2, i) != 0.0) W(SP_L2, i) += (dx - W(SP_PL1, i)) / delta;
        W(SP_PU1, i) = dx;                                // parked: DX still holds dlam for the rows below i
      }
      pol.sync();
      for (int i = i0; i < n; i += di) W(SP_PL2, i) += W(SP_PU1, i);
      pol.sync();
    }
    // primal-dual active-set update
    bool changed = false;
    const double t = 1e-9;
    for (int i = i0; i < n; i += di) {
      const double x = W(SP_PL2, i), a2 = W(SP_A2, i), l2 = W(SP_L2, i);
      double n2 = a2;
      if (a2 < 0.0 && l2 > t) n2 = 0.0;
      if (a2 > 0.0 && l2 < -t) n2 = 0.0;
      if (a2 == 0.0 && x < lim.v_min - t) n2 = -1.0;
      if (a2 == 0.0 && x > W(SP_HI, i) + t) n2 = 1.0;
      if (n2 != a2) { W(SP_A2, i) = n2; changed = true; }
      if (i < m1) {
        const double a = ax1(SP_PL2, i), a1 = W(SP_A1, i), l1 = W(SP_L1, i);
        double n1 = a1;
        if (a1 < 0.0 && l1 > t) n1 = 0.0;
        if (a1 > 0.0 && l1 < -t) n1 = 0.0;
        if (a1 == 0.0 && a < lim.a_min - t) n1 = -1.0;
        if (a1 == 0.0 && a > lim.a_max + t) n1 = 1.0;
        if (n1 != a1) { W(SP_A1, i) = n1; changed = true; }
      }
    }
    ok = !pol.any(changed);
  }
  // ---- certificate on the active-set point (or the interior-point iterate when that failed)
  double worst = 1e300;
  if (ok) {
    worst = 0.0;
    for (int i = i0; i < n; i += di) {
      const double x = W(SP_PL2, i);
      double st = x + W(SP_Q, i) + W(SP_L2, i);
      if (i > 0) st += W(SP_C, i - 1) * W(SP_L1, i - 1);
      if (i < m1) st -= W(SP_C, i) * W(SP_L1, i);
      worst = std::fmax(worst, std::fabs(st));
      worst = std::fmax(worst, std::fmax(lim.v_min - x, x - W(SP_HI, i)));
      const double l2 = W(SP_L2, i);
      worst = std::fmax(worst, std::fmax(l2, 0.0) * std::fabs(W(SP_HI, i) - x));
      worst = std::fmax(worst, std::fmax(-l2, 0.0) * std::fabs(x - lim.v_min));
      if (i < m1) {
        const double a = ax1(SP_PL2, i), l1 = W(SP_L1, i);
        worst = std::fmax(worst, std::fmax(lim.a_min - a, a - lim.a_max));
        worst = std::fmax(worst, std::fmax(l1, 0.0) * std::fabs(lim.a_max - a));
        worst = std::fmax(worst, std::fmax(-l1, 0.0) * std::fabs(a - lim.a_min));
      }
    }
  }
  worst = pol.rmax(worst);
  const bool certified = ok && worst <= cert_tol;
  for (int i = i0; i < n; i += di) v[i * v_stride] = certified ? W(SP_PL2, i) : (converged ? W(SP_X, i) : W(SP_L2, i));
  return certified ? SP_SOLVED : SP_INACCURATE;
}

// one thread per path
MPMPC_HD int sp_solve(int n, const double* li, const double* kappa, long in_stride, const SpLimits& lim, double eps,
                      const SpWork& W, double* v, long v_stride, int* iters) {
  return sp_solve_t(SpSerial{}, n, li, kappa, in_stride, lim, eps, W, v, v_stride, iters);
}

}  // namespace mpmpc
