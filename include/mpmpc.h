/* mpmpc -- C ABI of the MI355X-native batched LTV-MPC QP path.
 *
 * The reference (matssteinweg/Multi-Purpose-MPC) has no FFI layer: its hot path is the Python
 * method MPC.get_control() (src/MPC.py:161-222), which rebuilds the horizon-stacked QP in
 * MPC._init_problem() (src/MPC.py:61-159) and hands it to the third-party OSQP solver
 * (src/MPC.py:158-159,183).  This header is the boundary a maintainer binds with ctypes to move
 * that path onto the GPU for B independent controller instances per call.
 *
 * Conventions
 *   - every array is caller-owned, C-contiguous HOST memory (numpy); the library owns all device
 *     memory behind the opaque handle; one handle = one device = one stream; calls on one handle
 *     are not re-entrant; every call that returns data is synchronous.
 *   - functions return 0 on success, <0 on error; mpmpc_last_error() gives the thread-local text.
 *   - all arithmetic is IEEE float64; nx = 3 states (e_y, e_psi, t), nu = 2 inputs (v, kappa).
 *   - decision vector z = [x_0..x_N (3 each), u_0..u_{N-1} (2 each)], n = 5N+3, as in
 *     src/MPC.py:128-147; constraint rows [3(N+1) dynamics ; 3(N+1) state boxes ; 2N input boxes].
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails.
 */
#ifndef MPMPC_H
#define MPMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPMPC_NX 3
#define MPMPC_NU 2
#define MPMPC_MAX_HORIZON 255
#define MPMPC_NUM_FIELDS 27 /* doubles per (instance, stage) of the stage-blocked QP, see below */

/* per-instance status, OSQP's numbering (drives the fallback branch of src/MPC.py:208-216) */
#define MPMPC_SOLVED 1
#define MPMPC_SOLVED_INACCURATE 2
#define MPMPC_MAX_ITER_REACHED (-2)
#define MPMPC_PRIMAL_INFEASIBLE (-3) /* default settings: with a Farkas ray in y; an EMPTY box (lower bound above upper bound,
                                        e.g. the speed cap of src/MPC.py:111-113 below umin[0]) is reported as -3 with a
                                        zero ray - stock OSQP refuses such data at setup */
#define MPMPC_DUAL_INFEASIBLE (-4)
#define MPMPC_UNSOLVED (-10) /* no verdict: the iterate is not finite (NaN / Inf in the inputs) */

/* error codes */
#define MPMPC_OK 0
#define MPMPC_E_ARG (-1)
#define MPMPC_E_HIP (-2)
#define MPMPC_E_STATE (-3)

typedef struct mpmpc_handle_s* mpmpc_handle;

/* Controller constants: what MPC.__init__ stores (src/MPC.py:15-59) plus the model's wheelbase
 * (src/spatial_bicycle_models.py:130) and the path's `circular` flag (src/reference_path.py:96).
 * Q, R, QN hold the DIAGONALS of the reference's weight matrices, Q_offdiag / R_offdiag / QN_offdiag their off-diagonal
 * entries (symmetric; all zero for what src/simulation.py:101-103 builds).  The reference puts the WHOLE Q, R, QN into the
 * Hessian (src/MPC.py:150) while its cost vector uses only diag(Q), diag(R) but the whole QN (src/MPC.py:153-155) - a quirk
 * that is reproduced: with non-diagonal Q or R the minimiser is not the tracking reference even without constraints.
 * A configuration with any off-diagonal weight, like one with bounds on e_psi / t or a cost on t, runs the general kernels,
 * one instance per wavefront (dense 3 x 3 / 2 x 2 stage Hessian blocks); diagonal weights run the reduced-native kernels
 * unchanged.  Q, R, QN must be positive semidefinite.
 * HORIZON: 3 <= N <= MPMPC_MAX_HORIZON (one lane per stage: a wavefront up to N = 63, a workgroup of 2 / 4 wavefronts whose
 * stages talk through LDS beyond that - several times slower per solve; the reference has no
 * upper limit). */
typedef struct {
  int32_t N;          /* horizon, 3 <= N <= MPMPC_MAX_HORIZON (the kappa_pred quirk of MPC.py:86 needs N >= 3); N <= 63: one wavefront
                         (or a part of one) per instance; 64 .. 127 / 128 .. 255: a workgroup of 2 / 4 wavefronts per instance,
                         general kernel (csrc/lane_gpu.hpp: LaneBlock) */
  int32_t max_batch;  /* largest B of any later call */
  int32_t device;     /* HIP device ordinal */
  int32_t circular;   /* ReferencePath.circular */
  double Q[3], R[2], QN[3];
  double xmin[3], xmax[3]; /* StateConstraints 'xmin','xmax' (may be +-inf) */
  double umin[2], umax[2]; /* InputConstraints 'umin','umax' in (v, kappa) */
  double ay_max;           /* MPC.ay_max */
  double wheelbase;        /* model.length */
  double QN_offdiag[3];    /* QN[0][1], QN[0][2], QN[1][2] (= their transposes); all zero for the reference's weights */
  double Q_offdiag[3];     /* Q[0][1], Q[0][2], Q[1][2]: enter the Hessian only (src/MPC.py:150), not the cost vector (153) */
  double R_offdiag[1];     /* R[0][1]: likewise (src/MPC.py:150,155) */
} mpmpc_config;

/* Solver settings: OSQP 0.6.x names and defaults for the ADMM stage (what
 * osqp.OSQP().setup(..., verbose=False) of src/MPC.py:159 runs with), plus the certified polish. */
typedef struct {
  double rho, sigma, alpha;
  double eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
  int32_t max_iter, check_termination, scaling;
  int32_t adaptive_rho, adaptive_rho_interval;
  double adaptive_rho_tolerance;
  int32_t polish;   /* 0: ADMM only (stock OSQP behaviour); 2: interior-point refine + active-set polish + certificate */
  int32_t ipm_max_iter;  /* interior-point iterations per attempt (30) */
  double ipm_tol, ipm_reg; /* the interior point stops at residual, complementarity < ipm_tol (1e-8: it only has to identify the
                            active set, which it reads off its last step; a failed active-set attempt continues it to
                            ipm_tol x 1e-4); primal / dual regularisation of its Newton systems (1e-8) */
  double as_delta;       /* regularisation of the active-set KKT solve, removed by as_refine refinement steps (1e-10, 5) */
  int32_t as_refine, as_rounds;   /* ...; primal-dual active-set rounds per attempt (4) */
  double cert_tol;       /* KKT certificate (unscaled problem): primal violation, stationarity, complementarity <= 1e-8 */
  int32_t early_polish; /* > 0: try the polish after this many ADMM iterations; instances it cannot certify
                           run the full ADMM (to max_iter / termination / infeasibility) and are polished
                           again.  0: polish only after ADMM has terminated (OSQP's order). */
  int32_t early_scaling; /* Ruiz passes done before the early polish attempt (0 or >= scaling: all of them).  The
                            remaining scaling - early_scaling passes are done before the full ADMM run, which
                            therefore sees exactly OSQP's `scaling` passes. */
  int32_t phase1;        /* 1: an instance the early polish attempt cannot certify is first tested for infeasibility -
                            least-squares phase 1 (every inequality row softened, nothing else in the cost) by the same
                            interior-point code; its multipliers are a Farkas ray, checked with OSQP's own
                            primal-infeasibility criterion (at phase1_eps) -> MPMPC_PRIMAL_INFEASIBLE after ~5-10
                            interior-point iterations instead of hundreds or thousands of ADMM iterations; z then holds
                            the least-violation point, y the ray, resid[0] the largest bound violation of z.  What it
                            cannot decide runs the full ADMM as before.  0: OSQP's ADMM decides infeasibility. */
  double ipm_diverged;   /* the interior point gives up when mu exceeds this multiple of its smallest value so far
                            (multipliers blowing up: infeasible, phase 1 decides) */
  double phase1_theta;   /* start value of phase 1's slacks and multipliers (row space) */
  double phase1_eps;     /* eps of OSQP's primal-infeasibility test when it is applied to phase 1's ray (default 1e-6).
                            eps_prim_inf = 1e-4 is calibrated for ADMM's slowly converging dual steps; the interior-point
                            ray satisfies |A'y| <= 1e-7 |y|, so the test can be sharper: an instance whose corridor
                            cannot be met by a few tenths of a millimetre is still proved infeasible instead of being
                            handed to the ADMM iteration (which calls it "solved" at eps = 1e-3; status 2). */
  int32_t reduce;        /* 1 (default): when the time state carries neither cost nor bound (Q[2] = QN[2] = 0, QN_offdiag
                            without t, xmin[1..2] = -inf, xmax[1..2] = +inf, R[0] > 0 - the reference's own tracking weights,
                            src/simulation.py:101-111) the certified polish and phase 1 solve the REDUCED problem: t enters
                            no other state's dynamics and the speed v drives t alone, so the QP separates into
                            v_k = clip(v_ref_k) in closed form, the roll-forward of t, and the QP in (e_y, e_psi, kappa) with
                            2 x 2 blocks - the same optimum (the KKT certificate is evaluated on the FULL problem) for about
                            half the arithmetic.  0: always the full 3-state polish.  The ADMM stage always runs on the
                            full problem (it reproduces OSQP's iterates). */
  double ipm_start_slack; /* the polish attempt that follows the early_polish ADMM iterations (and the retry from phase 1's */
  double ipm_start_mu;    /* point) starts the interior point CENTRED: slacks max(distance to the bound, ipm_start_slack),
                            multipliers ipm_start_mu / slack (row space of the scaled problem) - after one ADMM iteration
                            the multipliers carry no information and small slacks cost 5-7 blocked steps.  ipm_start_mu = 0:
                            warm start from the ADMM multipliers, as the polish after a full ADMM run always does.
                            Defaults 0.1, 0.01. */
  double ipm_start_dual;  /* > 0: the centred start uses mu0 = max(ipm_start_mu, ipm_start_dual x ipm_start_slack x |P x + q|_inf)
                            (scaled problem, start point x): start multipliers commensurate with the dual residual they
                            have to balance (config 3, time-optimal weights: 12.6 -> 11.4 iterations; the stock weights sit on the
                            ipm_start_mu floor).  0: ipm_start_mu alone.  Default 0.2. */
  double as_add_fraction; /* active-set rounds add only the bounds violated by at least this fraction of the round's worst
                            violation (measured on the scaled variable); 0: every violated bound, the plain primal-dual
                            active-set update; the retry after a failed attempt uses at least 0.5.  Default 0.25. */
  int32_t phase1_accept; /* 1 (default): an instance phase 1 proves infeasible by LESS than OSQP's primal termination tolerance
                            (eps_abs + eps_rel max(|Ax|, |z|) at the least-violation point: millimetres at eps = 1e-3) is not
                            reported infeasible - the reference's OSQP call accepts such a problem as "solved" and the
                            reference drives the plan (src/MPC.py:159,183-206).  Its violated boxes are widened to 1.5 times the
                            least violation, the polish solves that problem, and the plan comes back as MPMPC_SOLVED_INACCURATE
                            with the violation in resid[0] (a usable status: no fallback step).  0: every proven infeasibility
                            is reported as MPMPC_PRIMAL_INFEASIBLE however small the margin (batch sweeps that want the verdict).
                            The test is a MODEL of OSQP's, not a run of it: the least-violation point is the limit of OSQP's
                            ADMM iteration (the minimiser of the sum of the squared scaled violations, dynamics rows weighted a
                            thousand times the box rows: Solver::phase1), max(|Ax|, |z|) is taken at that point; what it
                            cannot know is an instance OSQP abandons at max_iter before either of its tests passes (it then
                            returns its iterate: "solved inaccurate"), or one within 0.1 % of the threshold, where OSQP stops
                            an iterate short of its limit.  Validated on the reference's own laps (golden G6s) and
                            on BASELINE's obstacle batches (tests, bench line); mpmpc.stock_settings() runs the restated OSQP
                            itself. */
  int32_t native;        /* 1 (default): where `reduce` applies and the settings are the defaults of the early attempt
                            (early_polish = 1, ipm_start_mu > 0) the batch launches run the REDUCED-NATIVE kernels: a lane
                            never holds the 3-state problem - v in closed form at load time, own Ruiz pass / start / interior
                            point / active-set rounds / KKT certificate on the (e_y, e_psi, kappa) problem, the roll-forward
                            of t at the store - about half the registers of the general kernels, so two wavefronts share a
                            SIMD.  What they cannot certify (infeasible or very hard instances) goes to the general
                            one-instance-per-wave kernel (phase 1, full OSQP run) exactly like the tail of a packed launch.
                            0: the general kernels only.  The closed loop's warm-started launches run the same kernels
                            (template flag WARM).  Weightings with a terminal cost on the time state and none else on it
                            (QN[2] > 0 = Q[2]: BASELINE config 3) have their own reduced-native kernels
                            (csrc/mpmpc_reduced_t.hpp: the speeds stay in the problem, the time cost is one rank-one term;
                            one instance per wave, cold starts). */
  double native_ipm_tol; /* interior-point tolerance of the reduced-native kernels' FIRST attempt (ipm_tol is the general
                            kernels').  The interior point only has to identify the active set - the active-set rounds
                            and the KKT certificate (cert_tol) make the answer - and on the reduced problem it has done
                            so one iteration earlier than at 1e-8 for most instances: measured, config 2 +8 %, configs 4 / 5
                            +2-3 %, B = 65 536 +4 %.  An attempt whose active-set rounds fail is repeated at a hundred
                            times tighter tolerance, twice if need be.  Default 1e-7. */
  int32_t early_start;   /* start of the general kernels' early attempt (early_polish = 1): 1 = OSQP's first iterate (one
                            factorisation + one KKT solve), 0 (default) = x = 0, no OSQP iterate - measured: config 3 takes
                            11.08 instead of 11.43 interior-point iterations from x = 0 and saves the iterate's 11 us per
                            wave.  The reduced-native kernels always start from x = 0.  iters[.][0] = 1 marks the early
                            attempt either way. */
  double phase1_band;    /* phase1_accept: phase 1 leaves at the first iterate whose multipliers are a valid Farkas ray only while
                            that iterate violates a bound by more than phase1_band times OSQP's primal tolerance (eps_abs +
                            eps_rel x the largest finite bound); inside the band it runs to its converged optimum, because the
                            violation of THAT point decides whether the reference's OSQP call would have returned a plan, and
                            it is up to 2.4 times smaller than the early iterate's.  Default 3: measured on config 5 (65 536
                            instances, emulation) the number of instances that take the other branch than the restated stock
                            OSQP is 67 / 34 / 29 / 26 / 26 / 26 at 1.5 / 2 / 2.5 / 3 / 6 / 1000, and config 4 runs 2.1 / 2.7 /
                            3.2 / 4.3 % slower at 2 / 3 / 4 / 6 than at 0 (profiles/r5/branch_agreement.txt). */
} mpmpc_settings;

const char* mpmpc_version(void);
const char* mpmpc_last_error(void);
int mpmpc_device_count(int32_t* count);
void mpmpc_default_settings(mpmpc_settings* s);

/* replaces MPC.__init__ (src/MPC.py:15-59): allocates device buffers for max_batch instances */
int mpmpc_create(const mpmpc_config* cfg, const mpmpc_settings* settings, mpmpc_handle* out);
int mpmpc_destroy(mpmpc_handle h);
int mpmpc_set_settings(mpmpc_handle h, const mpmpc_settings* settings);
/* Lanes given to one QP instance by the solve launches of the reference's own weights (the reduced-native kernels; every
 * packing returns the same answers: parity tests and tuning).  A value the handle's horizon cannot take is MPMPC_E_ARG.
 *     0    (default) chosen per launch.  N <= 63: one instance per 64-lane wavefront up to 1 024 instances, beyond that the
 *          smallest of 32 / 16 lanes that holds the N + 1 stages from 1 025 / 2 049 instances on - from 129 / 257 on for
 *          launches that are one of several in flight (mpmpc_set_pipeline).  N >= 64: two stages per lane (see 64, 128).
 *    64    N <= 63: one instance per wavefront at any batch size.  64 <= N <= 127: TWO stages per lane, the instance in one
 *          wavefront - what 0 selects there.
 *    32    N <= 31: two instances per wavefront at any batch size.
 *    16    N <= 15: four instances per wavefront at any batch size.  16 <= N <= 31: TWO stages per lane, four instances per
 *          wavefront, for the batch launches (cold starts; the closed loop ignores it and keeps one stage per lane).
 *   128    64 <= N <= 127: one stage per lane on a workgroup of two wavefronts instead of the two-stages-per-lane default.
 *          128 <= N <= 255: two stages per lane on a workgroup of two wavefronts - what 0 selects there.
 *   256    128 <= N <= 255: one stage per lane on a workgroup of four wavefronts instead.
 * Configurations the reduction does not apply to (full weights, bounds on e_psi / t, a cost on t) run one instance per
 * wavefront / workgroup whatever is set here. */
int mpmpc_set_packing(mpmpc_handle h, int32_t lanes_per_instance);
/* Which kernel takes the TAIL of a batch launch - the instances the reduced-native kernel could not certify: infeasible,
 * marginally infeasible and very hard ones.  1 (default) = the reduced-native tail kernel first (phase 1 and one more
 * attempt of the certified polish on the (e_y, e_psi, kappa) problem, two wavefronts per SIMD, two instances per wavefront
 * for horizons up to 31, one for horizons 32 .. 63), the general kernel only on what that leaves; 2 = the same with ONE instance per wavefront (the split
 * layout of the general kernel's phase 1: its answers to rounding, 4e-16); 0 = the general kernel on the whole tail (one
 * wavefront per SIMD).  Same statuses in all three; least-violation points and relaxed plans of 1 agree with those of 2 / 0
 * to ~1e-8 (phase 1 converges along another arithmetic path).  Parity tests, A/B timings. */
int mpmpc_set_tail_kernel(mpmpc_handle h, int32_t reduced_native);

/* replaces the per-stage ReferencePath.get_waypoint() / Waypoint.__sub__ reads of
 * src/MPC.py:93-97 (src/reference_path.py:50-57,356-371): per-waypoint kappa, v_ref and the
 * distance to the next waypoint, uploaded once per path. */
int mpmpc_set_path(mpmpc_handle h, int32_t n_wp, const double* kappa, const double* v_ref,
                   const double* ds_next);

/* replaces ReferencePath.update_path_constraints(wp_id+1, N, ...) of src/MPC.py:116-118 for a
 * static map, where it depends on wp_id only (src/reference_path.py:522-648): row w of the
 * [n_wp x n_cols] tables holds ub / lb for the n_cols waypoints after waypoint w. n_cols >= N. */
int mpmpc_set_corridor(mpmpc_handle h, int32_t n_wp, int32_t n_cols, const double* ub,
                       const double* lb);

/* Route fleets: every instance of a batch follows its own reference path.  The tables of mpmpc_set_path (and of
 * mpmpc_set_corridor, mpmpc_set_path_geometry, mpmpc_build_corridor, which keep their signatures) are then the
 * CONCATENATION of P routes: route p is rows first[p] .. first[p + 1] - 1 of every per-waypoint table and has its own
 * circular[p]; the handle-wide mpmpc_config.circular is ignored while routes are set.
 * The law.  For an instance on route p, n = first[p + 1] - first[p]: every waypoint index of the single-path code is
 * formed with n_wp := n and circular := circular[p] on LOCAL waypoint ids 0 .. n - 1 - stage k reads rows wp + k and
 * max(wp + k - 1, 0), wrapped on a circular route (one subtraction when n > N, modulo otherwise), clamped to n - 1 on an
 * open one - and first[p] is added last, at the load.  wp_id is local to the route wherever it crosses this interface:
 * mpmpc_upload / _assemble / _solve / the staged calls take local ids (0 <= wp_id < n, and wp_id + N < n on an open
 * route, per instance), and the corridor-table row an instance reads is global row first[p] + wp_id.
 *   mpmpc_set_routes      after mpmpc_set_path: first [P + 1] with first[0] = 0, strictly increasing, first[P] = n_wp of
 *                         the path set; every route has at least 2 waypoints; circular [P].  P = 0 returns the handle to
 *                         one path.  A new mpmpc_set_path clears the routes.  MPMPC_E_STATE without a path.  When the
 *                         routes change, the corridor table of a handle on which mpmpc_build_corridor has run is void (its
 *                         horizons were walked under the old ones): build it again; a table given by mpmpc_set_corridor
 *                         on a handle that never built one stays.
 *   mpmpc_set_car_routes  route [B]: the route of instance i in every later call with this B, until set again; ids outside
 *                         [0, P) are MPMPC_E_ARG.  With routes set, a call on another number of instances than the last
 *                         mpmpc_set_car_routes returns MPMPC_E_STATE.
 *   Both calls invalidate the batch on the device - its local wp_id were checked against the old routes: upload again before
 *   mpmpc_solve_resident, which returns MPMPC_E_STATE until then.
 *   mpmpc_check_routes    the argument checks of mpmpc_set_routes on their own (no handle, no device).
 * What works with routes: mpmpc_set_corridor, mpmpc_set_path_geometry, mpmpc_build_corridor (the horizon walk of a start
 * waypoint wraps or clamps inside its route; the table comes out concatenated), mpmpc_assemble, mpmpc_upload, mpmpc_solve, the
 * resident and staged solves, at every packing - and the closed loop: mpmpc_rollout_init after mpmpc_set_car_routes for its B,
 * with cum_lengths [n_wp] the routes' own cumulative lengths laid end to end (each route's starts at 0; s is the arc length
 * along the car's route), then mpmpc_rollout_step with every setting: per-car obstacles, walls, movers (an along-the-path
 * mover follows the route of the car that owns it), traffic (a group may span routes: cars of different routes meet),
 * perception, audit, recorder (wp_id local; the predicted path and the corridor row are the route's), scan.  alive = 0 (s past
 * the route's length) and -2 (the horizon passes the end of an OPEN route) are decided per route.  Two differences from one
 * path: the closed-loop warm start is off while routes are set (mpmpc_rollout_warm_start is kept for when they are cleared),
 * and setting routes or car routes ends a rollout in progress (mpmpc_rollout_init again; mpmpc_rollout_reroute below changes
 * the routes of running cars and does not).  Without routes a handle computes what it computed before. */
int mpmpc_check_routes(int32_t n_wp, int32_t P, const int32_t* first, const int32_t* circular);
int mpmpc_set_routes(mpmpc_handle h, int32_t P, const int32_t* first, const int32_t* circular);
int mpmpc_set_car_routes(mpmpc_handle h, int32_t B, const int32_t* route);

/* Where is a pose on a route, and re-routing the cars of a running rollout.
 * The law (csrc/project_core.hpp).  A route is rows first .. first + n - 1 of x, y, psi, cum; cum is the route's own cumulative
 * length starting at 0, what mpmpc_rollout_init takes.  For a pose (px, py, ppsi) and every local waypoint j:
 * d2[j] = dx dx + dy dy with dx = px - x[j], dy = py - y[j] (every operation rounded on its own); e_psi[j] is the heading error
 * of the rollout's localisation, fmod(ppsi - psi[j] + pi, 2 pi), + 2 pi if negative, - pi; j is eligible when
 * |e_psi[j]| <= max_heading (max_heading >= pi: every waypoint - the gate keeps a car on the right branch where routes cross
 * or run back beside themselves).  wp is the eligible j of the smallest d2, ties to the lowest j; -1 when none is eligible or a
 * pose component is not finite.  dist = sqrt(d2[wp]); x0 = (e_y, e_psi, 0) of the pose at waypoint wp, as the rollout forms
 * it; s = cum[wp].  With wp = -1: dist = +inf, x0 and s NaN.  s = cum[wp] on purpose: the rollout's localisation then finds
 * wp again for every wp < n - 1, and "finished" at wp = n - 1.
 *   mpmpc_project          no handle.  The tables are [n_wp]; P = 0 or first = NULL: one route of n_wp rows, else first [P + 1]
 *                          by the rules of mpmpc_check_routes.  pose [B*3].  cand [B*K]: the K candidate routes of every pose
 *                          (ids may repeat); NULL with K = P (K = 1 for one route): every route.  An id outside [0, P),
 *                          max_heading negative or NaN: MPMPC_E_ARG.  Outputs [B*K] (x0_out [B*K*3]), any may be NULL.
 *   mpmpc_rollout_reroute  needs routes, and a rollout in progress on exactly B cars (else MPMPC_E_STATE).  route [B]: the
 *                          route car i is to take, -1: keep; an id outside [-1, P), max_dist or max_heading negative or NaN:
 *                          MPMPC_E_ARG, nothing changes (max_dist may be +inf).  On the device, every RUNNING car (alive = 1)
 *                          with route[i] >= 0 is projected from its current pose onto that route; if wp >= 0 and
 *                          dist <= max_dist the car is on that route from now on with s = cum[wp] of it and accepted = 1, else
 *                          it keeps its route and s and accepted = 0 (as for a car that is not running, or kept).  A car sent
 *                          to the route it is on is treated like any other: s snaps to the nearest waypoint.  Pose, plan,
 *                          u_last, infeasibility counter, alive, audit accumulators, perception memory, recorder and every
 *                          per-car world setting stay as they are; wp_id and x0 of an accepted car become the projection's
 *                          (local to the new route) until the next step localises anew.  The rollout goes on: the call does
 *                          not end it and voids neither the batch nor the corridor table.  The next step localises on the new
 *                          route, an along-the-path mover of the car follows it, and a car put within N waypoints of an open
 *                          route's end gets alive = -2 at its next step.  accepted_out [B] may be NULL.
 *   mpmpc_rollout_routes   route_out [B]: the route every car is on now.  MPMPC_E_STATE without routes or car routes for B. */
int mpmpc_project(int32_t device, int32_t n_wp, const double* x, const double* y, const double* psi, const double* cum,
                  int32_t P, const int32_t* first, int32_t B, const double* pose, int32_t K, const int32_t* cand,
                  double max_heading, int32_t* wp_out, double* dist_out, double* x0_out, double* s_out);
int mpmpc_rollout_reroute(mpmpc_handle h, int32_t B, const int32_t* route, double max_dist, double max_heading,
                          int32_t* accepted_out);
int mpmpc_rollout_routes(mpmpc_handle h, int32_t B, int32_t* route_out);

/* Device-side corridor generation: the three calls below replace, for a map that
 * changes between steps, the host loop of ReferencePath.update_path_constraints + _compute_free_segments
 * + skimage.draw.line_aa + Map.w2m/m2w (src/reference_path.py:466-648, src/map.py:77-101).
 *   mpmpc_set_map           Map.data (int8, 1 free / 0 occupied, row = y), Map.origin, Map.resolution
 *   mpmpc_set_path_geometry per-waypoint x, y, psi and Waypoint.static_border_cells (world coordinates,
 *                           [n_wp*2] each: upper/left border, lower/right border); needs mpmpc_set_path first
 *   mpmpc_build_corridor    update_path_constraints(w+1, n_cols, min_width, safety_margin) for EVERY start
 *                           waypoint w, written into the handle's corridor table (as mpmpc_set_corridor would)
 *                           and optionally copied out ([n_wp x n_cols]; rows whose first horizon waypoint has no
 *                           free segment - the reference raises there - are NaN).  *bad_rows counts those. */
int mpmpc_set_map(mpmpc_handle h, int32_t height, int32_t width, const int8_t* data, double origin_x,
                  double origin_y, double resolution);
int mpmpc_set_path_geometry(mpmpc_handle h, int32_t n_wp, const double* x, const double* y, const double* psi,
                            const double* border_ub, const double* border_lb);
int mpmpc_build_corridor(mpmpc_handle h, int32_t n_cols, double min_width, double safety_margin, double* ub_out,
                         double* lb_out, int32_t* bad_rows);

/* Closed-loop batched rollout on the device: B cars driven through
 * `while car.s < length: u = mpc.get_control(); car.drive(u)` (src/simulation.py:134-140) without a
 * host round trip per step.  Each step = localise + t2s (src/spatial_bicycle_models.py:183-219,256-279)
 * -> K1 -> K2 -> solution use / infeasibility fallback (src/MPC.py:185-220) + drive
 * (src/spatial_bicycle_models.py:221-244).  Needs mpmpc_set_path, mpmpc_set_path_geometry and a corridor
 * table (mpmpc_set_corridor or mpmpc_build_corridor).
 *   init:  Ts = model.Ts; cum_lengths[n_wp] = cumsum(ReferencePath.segment_lengths); s[B] arc lengths;
 *          pose[B*3] = (x, y, psi); cc0[B*2N] previous plans or NULL for zeros (MPC.__init__).
 *   state: any output may be NULL.  alive: 1 running, 0 lap finished (s >= length), -1 ended by the
 *          reference's exit(1) after N-1 consecutive infeasible steps, -2 ended by the reference's exit(1) at
 *          the end of an OPEN path (circular = 0): the car's waypoint has wp_id + N >= n_wp, where
 *          get_waypoint prints "Reached end of path!" (src/reference_path.py:367-369); wp_id and x0 hold the
 *          state of that step, the car is not driven.  A circular path never ends a car with -2.
 *          With per-car obstacles (mpmpc_rollout_set_obstacles) also: -3 the first horizon waypoint of the car's
 *          world has no free segment (the reference raises in update_path_constraints), -4 a border line of the
 *          car's world has more than 8 free segments (COR_MAXSEG, a limit of this library); wp_id and x0 hold
 *          that step's state, the car is not driven, the other cars are unaffected.  The lists K0c reads hold the car's
 *          static discs, its movers (mpmpc_rollout_set_movers) and its traffic slots (mpmpc_rollout_set_traffic): a row
 *          blocked by another car's disc ends the car with -3 in the same way.
 *          With mpmpc_rollout_set_audit in mode 2 also: -5 the car's footprint touched its world at that step's pose.
 * The rollout keeps its plans, waypoint ids and states in the handle's batch blocks: mpmpc_upload / mpmpc_solve /
 * mpmpc_assemble on the SAME handle overwrite them, after which mpmpc_rollout_step / _state / _set_counters return
 * MPMPC_E_STATE until mpmpc_rollout_init is called again.  (mpmpc_download and mpmpc_build_corridor are fine.) */
int mpmpc_rollout_init(mpmpc_handle h, int32_t B, double Ts, const double* cum_lengths, const double* s,
                       const double* pose, const double* cc0);
int mpmpc_rollout_step(mpmpc_handle h, int32_t B, int32_t n_steps);
/* MPC.infeasibility_counter of every car (src/MPC.py:206,215), to resume a recorded run: values in [0, N-2].
 * mpmpc_rollout_init starts every car at 0. */
int mpmpc_rollout_set_counters(mpmpc_handle h, int32_t B, const int32_t* counter);
/* Warm start of the closed loop: each step first tries active-set rounds from the active set the previous step
 * certified for the same car, shifted by the waypoints it advanced; what they cannot certify goes through the
 * normal path.  enable: 0 off, 1 on, 2 (default) on where it pays - fleets of more than 1024 cars (several cars per
 * wavefront) and of at most 16; in between a step ends with its slowest car, and one car in fourteen misses its
 * guess.  The reference cold-starts every step (src/MPC.py:158). */
int mpmpc_rollout_warm_start(mpmpc_handle h, int32_t enable);
int mpmpc_rollout_state(mpmpc_handle h, int32_t B, double* s, double* pose, double* cc, int32_t* wp_id,
                        double* x0, double* u_last, int32_t* status, int32_t* counter, int32_t* alive);
/* Per-car obstacles: a fleet of different worlds in one rollout.  Car b's world is the base map (mpmpc_set_map) with
 * its own circular obstacles added as Map.add_obstacles rasterises them (src/map.py:116-137): disc j of car b is
 * discs[3*(offsets[b] + j) + {0,1,2}] = (cx, cy, r) in map cells, r = ceil(radius / resolution), (cx, cy) = w2m(centre);
 * it occupies (cx+dx, cy+dy) for dx, dy in [-r, r-1] with dx^2 + dy^2 <= r^2.  offsets [B+1] (offsets[0] = 0,
 * non-decreasing, at most 64 discs per car; a car may have none).  Each rollout step then uses, for car b, the row
 * update_path_constraints(wp_id_b + 1, N, min_width, safety_margin) of car b's world (min_width / safety_margin of the
 * last mpmpc_build_corridor), bit-identical to the reference's, built on the device (K0c) - see alive -3 / -4 above.
 *   Needs mpmpc_build_corridor on the current map, path and geometry (it reuses that build's per-waypoint segments):
 *   MPMPC_E_STATE before one, or after mpmpc_set_map / mpmpc_set_path / mpmpc_set_path_geometry; a step after such a
 *   change also fails with MPMPC_E_STATE until the obstacles are set again.  A disc whose square leaves the grid:
 *   MPMPC_E_ARG.  offsets == NULL: back to the shared corridor table (the default).  May be called before
 *   mpmpc_rollout_init or between mpmpc_rollout_step calls: it applies from the next step on and keeps the rollout's
 *   state (worlds that change while the cars drive).  The B of the next step must equal this B. */
int mpmpc_rollout_set_obstacles(mpmpc_handle h, int32_t B, const int32_t* offsets, const int32_t* discs);
/* ub / lb [B x N]: the rows the last rollout step used for each car (per-car obstacles only, else MPMPC_E_STATE), as the
 * reference's update_path_constraints returns them; NaN rows for cars whose row was blocked (-3) or overflowed (-4). */
int mpmpc_rollout_corridor(mpmpc_handle h, int32_t B, double* ub, double* lb);
/* Movers: per-car obstacles that move while the cars drive, advanced on the device (K0m) - a slower vehicle ahead,
 * something crossing the track - so that mpmpc_rollout_step(h, B, n_steps) keeps its point with n_steps > 1.  A mover is a
 * disc of constant radius (map cells, as above) whose centre is a closed-form function of the rollout step index k
 * (0-based, counted from mpmpc_rollout_init: what mpmpc_rollout_recorded returns as n_steps), j = k - step0:
 *   kind 0, params (x0, y0, dx, dy): a straight line, world start point and displacement per step [m]:
 *           (x, y) = (x0 + j dx, y0 + j dy)
 *   kind 1, params (s0, e, ds, 0): along the reference path, start arc length, lateral offset (positive = left, the sign
 *           of e_y) and arc length per step: s = s0 + j ds, wrapped into [0, L) on a circular path (L = the last entry of
 *           mpmpc_rollout_init's cum_lengths); the centre is the point at arc length s of the waypoint polyline, moved by
 *           e along the normal of the segment's first waypoint.
 * The disc of step k is (w2m(x, y), r).  A mover is ABSENT on a step - the disc (0, 0, 0), which occupies no cell - when
 * its square leaves the grid, its centre is not finite or beyond 2^30 cells, or (kind 1, open path) s < 0 or s >= L.
 * The exact operation order is stated in csrc/obstacle_motion_core.hpp; the positions of any step, recorded or not, can
 * be recomputed from its index.
 *   mpmpc_rollout_set_movers   mover q of car b is entry offsets[b] + q of kind[], radius_cells[] and params[][4]
 *                           (offsets [B+1] as for the discs).  offsets == NULL: no movers.  Static discs and movers are
 *                           two independent settings; K0c reads, per car, the static discs followed by the movers' discs
 *                           of the step.  Together at most 64 per car (else MPMPC_E_ARG), and both settings must be for
 *                           the same B (else MPMPC_E_STATE) - mpmpc_rollout_set_obstacles checks the same against the
 *                           movers in force.  Also MPMPC_E_ARG: an unknown kind, a negative radius, a parameter that is
 *                           not finite, offsets that decrease.  A refused call leaves the previous setting as it was.
 *                           Needs mpmpc_build_corridor like the discs, and is void after a change of map, path or
 *                           geometry in the same way.  May be called before mpmpc_rollout_init or between
 *                           mpmpc_rollout_step calls: it applies from the next step on and keeps the rollout's state.
 *                           step0 may be negative: a run resumed from a saved state of step k0 (mpmpc_rollout_init
 *                           restarts k at 0) continues its movers with step0 - k0.
 *   mpmpc_rollout_obstacles the disc lists the LAST rollout step used: offsets_out [B+1], discs_out [offsets_out[B]][3]
 *                           (at most 64 B entries; either pointer may be NULL), per car the static discs, then the
 *                           movers, then the traffic slots (mpmpc_rollout_set_traffic), absent ones as (0, 0, 0).
 *                           MPMPC_E_STATE if that step built no per-car rows (as mpmpc_rollout_corridor), or if any of
 *                           the three settings was changed since.
 * A rollout without movers launches exactly what it launched before. */
int mpmpc_rollout_set_movers(mpmpc_handle h, int32_t B, const int32_t* offsets, const int32_t* kind,
                             const int32_t* radius_cells, const double* params, int64_t step0);
int mpmpc_rollout_obstacles(mpmpc_handle h, int32_t B, int32_t* discs_out, int32_t* offsets_out);
/* Lookahead: every column of a car's horizon sees the car's movers where they will be when the car gets there.  Without it
 * K0c builds all N columns against the movers' discs of the current step k: a car reserves room where a crossing mover is
 * now for its whole horizon, and none where the mover will be.  The setting is fleet-wide and off by default:
 *   seg_time[n_wp]   entry i = the seconds a car is expected to need from waypoint i to i + 1, indexed by the global row of
 *                    the path table (route fleets lay it end to end like the path); ds_next / v_ref is the time model the
 *                    MPC's own time state is linearised around
 *   max_lead         in steps, 1 .. 1048576
 * For car b at step k with local wp_id, column c is waypoint cor_wp(wp_id + 1 + c) of the car's route (K0c's own index:
 * circular wrap, open-route clamping), and its lead is
 *     t_-1 = 0;   t_c = t_(c-1) + seg_time[row of cor_wp(wp_id + c)]     c = 0 .. N-1
 *     q = floor(t_c / Ts)        lead_c = (q < max_lead) ? (int)q : max_lead
 * (a strictly sequential sum, every add and the division rounded on their own; an infinite t_c saturates to max_lead; Ts is
 * mpmpc_rollout_init's).  Column c is built in this world: static discs, walls and traffic slots as at step k; mover slot q
 * as its disc of step k + lead_c (K0h evaluates the movers' closed form once per (mover, column), in front of K0c).  One
 * gate: a mover whose slot in the list K0c plans from is absent at step k - off the grid, or, under
 * mpmpc_rollout_set_perception, not known - is absent in every column.  Under perception a car thus anticipates exactly the
 * movers it currently knows: knowing a mover means knowing its motion law (a simplification).  The exact statement:
 * csrc/lookahead_core.hpp.  Everything else of a step is unchanged: the verdicts -3 / -4 are taken at column 0 of the
 * anticipated row, the audit keeps judging the true world of step k, recorded rows and mpmpc_rollout_corridor are the
 * anticipated rows, mpmpc_rollout_obstacles keeps returning the discs of step k.  Traffic slots are anticipated only with
 * mpmpc_rollout_set_lookahead_traffic (below).
 *   mpmpc_rollout_set_lookahead   seg_time == NULL: off.  MPMPC_E_ARG: n_wp differs from the path table's, an entry is
 *                           negative or NaN (+inf is allowed), max_lead < 1 or above the cap, N > 255, or the movers in
 *                           force times N times 12 bytes exceed 256 MiB (mpmpc_rollout_set_movers then checks the same
 *                           against the lookahead in force).  May be called before mpmpc_rollout_init or between
 *                           mpmpc_rollout_step calls: it applies from the next step on and keeps the rollout's state.
 *                           After a change of map, path, routes or geometry the next step returns MPMPC_E_STATE until it
 *                           is set again, like the per-car settings.
 *   mpmpc_rollout_lookahead what the LAST step's K0h wrote: lead_out [B x N], discs_out [movers of the fleet x N x 3]
 *                           (mover-major, in mpmpc_rollout_set_movers' order; may be NULL), ungated.  MPMPC_E_STATE if that
 *                           step did not look ahead for B cars (lookahead off, no movers), or a setting changed since.
 * A rollout without lookahead, or without movers, launches exactly what it launched before. */
int mpmpc_rollout_set_lookahead(mpmpc_handle h, int32_t n_wp, const double* seg_time, int32_t max_lead);
int mpmpc_rollout_lookahead(mpmpc_handle h, int32_t B, int32_t* lead_out, int32_t* discs_out);
/* Traffic: the cars of a group see each other as discs, from the fleet's own poses, every step on the device (K0t) - cars
 * that react to each other without a host round trip per step.  group[B]: cars with the same non-negative value share a
 * world, a negative value means the car sees nobody and nobody sees it.  radius_cells[B] >= 0: the disc with which car c
 * appears to the others (radius 0 occupies no cell).  slots S in [1, 64], the same for every car; range_cells: a car sees
 * no further (negative: no limit).  A step reads pose and alive AS IT FINDS THEM (what mpmpc_rollout_state returns before
 * the step; what a record holds as pose): car c is present iff alive == 1, group >= 0 and its cell w2m(x, y) lies within
 * 2^30 cells; a present car is visible iff its disc's square stays in the grid.  A car that has ended or finished is
 * taken off the track: it is not seen.  Car b, if present, gets the visible cars c != b of its group with
 * d2 = (cx_c - cx_b)^2 + (cy_c - cy_b)^2 <= range_cells^2, ordered by (d2, car index): the first S as (cx_c, cy_c, r_c), the
 * other slots (0, 0, 0); a car that is not present gets S absent discs.  The exact statement: csrc/traffic_core.hpp.
 *   group == NULL: no traffic.  Traffic is a third independent per-car setting beside the static discs and the movers:
 *   K0c reads, per car, the static discs, then the movers, then the S traffic slots - together at most 64 per car (else
 *   MPMPC_E_ARG), all settings in force for the same B (else MPMPC_E_STATE); the other two setters check the same against
 *   the traffic in force.  Also MPMPC_E_ARG: B outside [1, max_batch], a negative radius, slots outside [1, 64], a group
 *   of more than 1024 cars.  A refused call leaves every setting as it was.  Needs mpmpc_build_corridor like the discs
 *   (else MPMPC_E_STATE) and is void after a change of map, path or geometry in the same way.  May be called before
 *   mpmpc_rollout_init or between mpmpc_rollout_step calls: it applies from the next step on and keeps the rollout's
 *   state.  A rollout without traffic launches exactly what it launched before. */
int mpmpc_rollout_set_traffic(mpmpc_handle h, int32_t B, const int32_t* group, const int32_t* radius_cells, int32_t slots,
                              int32_t range_cells);
/* Lookahead for traffic: every column of a car's horizon sees the cars in its traffic slots where their own plans put them
 * when the car gets there.  Without it K0c plans all N columns against the neighbours' discs of the current step: a car
 * reserves room where a neighbour is now for its whole horizon, and none where it will be.  A fleet-wide flag, off by default,
 * independent of the order in which it, mpmpc_rollout_set_lookahead and mpmpc_rollout_set_traffic are called: a step
 * anticipates traffic iff lookahead is set, traffic is set and the flag is on - and then looks ahead with or without movers
 * (mpmpc_rollout_lookahead then returns the leads of such a step, and no discs when there are no movers).
 *   Tracks (K3t, at the end of such a step): stage j = 0 .. N of car n's solved plan lies at waypoint wp_id + j of its route
 *   (wrapped or clamped like the recorded predicted path) with lateral offset e_y_j = z[3 j] and arrival time t_j = z[3 j + 2]:
 *       valid[n]    = alive[n] == 1 after the step, and its status usable (1, 2, -2)
 *       cells[n][j] = the map cell of the predicted point (the recorder's pred_x / pred_y), or (INT32_MIN, 0) when it is not
 *                     finite or beyond 2^30 cells
 *       tm[n][0] = 0;  tm[n][j] = max(tm[n][j-1], t_j)  (a NaN is never taken)
 *   Who (K0t): who[b][t] = the car in traffic slot t of car b at the step, -1: empty.
 *   Horizon (K0ht, in front of K0c): with n = who[b][t], d the slot's TRUE disc of step k, L = lead[b][c]
 *       discs[b][t][c] = d   if n < 0 or L == 0 or !valid[n]   (valid, cells, tm: the tracks step k - 1 left)
 *       else  j* = the largest j with tm[n][j] <= (L + 1) * Ts;  (cx, cy) = cells[n][j*];
 *             discs[b][t][c] = (0, 0, 0) if that stage has no cell or the square of radius d.r around it leaves the grid,
 *                              else (cx, cy, d.r)
 *   K0c: for a traffic slot whose entry in the list it plans from (under perception: the perceived list) has r > 0, column
 *   c is built against discs[b][t][c]; else against that entry.  A neighbour is held at its plan's end beyond tm[n][N]; the
 *   slots are chosen by current distance (anticipation moves them, it does not re-select); knowing a neighbour means knowing
 *   its plan (a simplification).  mpmpc_rollout_init, mpmpc_rollout_reroute, switching the flag on and every per-car setter
 *   make every track invalid: the first step after them plans against the discs of the step itself.  The exact statement:
 *   csrc/traffic_lookahead_core.hpp.  The audit, mpmpc_rollout_obstacles and mpmpc_rollout_scan keep the true world of step k.
 *   mpmpc_rollout_set_lookahead_traffic   enable != 0: on.  MPMPC_E_ARG: N > 255, or B x slots x N x 12 bytes of the traffic in
 *                           force exceed 256 MiB while lookahead is set - whichever of the three setters comes last refuses,
 *                           and the setting that was in force stays.
 *   mpmpc_rollout_tracks    what the LAST step's K3t left: valid_out [B], cells_out [B x (N + 1) x 2], tm_out [B x (N + 1)]
 *                           (the last two may be NULL).
 *   mpmpc_rollout_lookahead_traffic   what the LAST step's K0t and K0ht wrote: who_out [B x slots], discs_out
 *                           [B x slots x N x 3] (may be NULL), ungated.
 *   Both getters: MPMPC_E_STATE if that step did not anticipate traffic for B cars, or a setting changed since (as
 *   mpmpc_rollout_lookahead).  A rollout with the flag off launches exactly what it launched before. */
int mpmpc_rollout_set_lookahead_traffic(mpmpc_handle h, int32_t enable);
int mpmpc_rollout_tracks(mpmpc_handle h, int32_t B, int32_t* valid_out, int32_t* cells_out, double* tm_out);
int mpmpc_rollout_lookahead_traffic(mpmpc_handle h, int32_t B, int32_t* who_out, int32_t* discs_out);
/* Corridor commitment (K0k): K0c builds a car's row from nothing at every step, as ReferencePath.update_path_constraints does -
 * the largest free segment at column 0, then the segment nearest the projection of the previous column's - so a waypoint can
 * sit on one side of an obstacle while it is a far column and change sides in the step it becomes column 0, next to the
 * obstacle.  With the setting, per car and off by default, a waypoint that was in the car's horizon in the step before chooses,
 * among its free segments, the one nearest to what it chose then:
 *   keep[B]          0: the car is off, its rows are the reference's bit for bit; a value in [1, +inf]: on, with that switch_ratio
 *   memory           per car N entries, one per column of its last row: wp = cor_wp(wp_id + 1 + c), local to the car's route,
 *                    or -1 (empty: the column had no free segment, or the car had no row), and the six numbers cor_bounds gave
 *                    for the column (ub, lb and the border cells of the selection without the margin: x, y of the upper, x, y of
 *                    the lower).  The memory of waypoint i is the entry with wp == i in the lowest column.
 *   choice           at a column of waypoint i with two or more free segments, on a car that is on, when waypoint i has memory m:
 *                    off = (|s_ub - m_ub| + |s_lb - m_lb|) / 2 over the candidates' border cells against the remembered ones -
 *                    the reference's measure without the forward projection - and the first minimum is kept; if switch_ratio is
 *                    finite and the longest candidate (column 0's span and tie rule) is longer than switch_ratio times the kept
 *                    one, the longest is taken instead.  Every other column is decided as without the setting: forced with at
 *                    most one segment, else the largest segment at column 0, else the nearest to the projection of the column
 *                    before - whatever decided that one.
 *   counters         three per car, accumulated for every car of the setting, the off cars included (a fleet is its own A/B):
 *                    kept - columns decided from memory; switched - of those, where the ratio left the nearest candidate; moved -
 *                    columns whose waypoint has memory, neither this step's (ub, lb) nor the remembered one collapsed (ub == lb),
 *                    and ub < lb_mem || lb > ub_mem: the corridor of the waypoint jumped to a disjoint interval.
 * The exact statement: csrc/commitment_core.hpp.  No kernel is added: a committed step runs another instantiation of K0c.  The
 * verdicts -3 / -4, mpmpc_rollout_corridor and the recorder's rows are those of the committed rows.  The per-car world setters
 * keep the memory - worlds that change under a committed car are the point; mpmpc_rollout_init and the setter empty it and zero
 * the counters; mpmpc_rollout_reroute empties the memory of the cars it accepts.
 *   mpmpc_rollout_set_commitment   keep == NULL: off.  mem_wp [B x N] and mem_rows [B x N x 6]: the memory of a resumed run (both
 *                           or neither; NULL: empty).  MPMPC_E_ARG: B outside [1, max_batch], a keep that is neither 0 nor in
 *                           [1, +inf] (NaN included), a mem_wp below -1, only one of the two memory pointers, or a block above
 *                           256 MiB (B x N x 104 + B x 20 bytes).  A refused call leaves the previous setting in force.  May be
 *                           called between mpmpc_rollout_step calls; after a change of map, path, routes or geometry the next
 *                           step returns MPMPC_E_STATE until it is set again, like the per-car settings.  A step under the
 *                           setting returns MPMPC_E_STATE without a per-car world in force for the same B (rows of the shared
 *                           table have no per-car memory; empty disc lists will do) and with mpmpc_rollout_set_lookahead in force.
 *   mpmpc_rollout_commitment   any pointer may be NULL.  counts_out [3][B]: kept, switched, moved; wp_out [B x N], rows_out
 *                           [B x N x 6]: the memory the next step will read.  MPMPC_E_STATE unless a step of B cars ran under the
 *                           setting in force.
 * A rollout without the setting launches exactly what it launched before. */
int mpmpc_rollout_set_commitment(mpmpc_handle h, int32_t B, const double* keep, const int32_t* mem_wp, const double* mem_rows);
int mpmpc_rollout_commitment(mpmpc_handle h, int32_t B, int32_t* counts_out, int32_t* wp_out, double* rows_out);
/* Walls: the second primitive of a car's world beside the discs - Map.add_boundary of the reference (src/map.py:139-155): a
 * line between two world points, stamped with skimage's line_aa.  A wall is (x0, y0, x1, y1) in map cells, the w2m of its
 * two end points, and occupies exactly the cells line_aa(x0, y0, x1, y1) produces (the law: csrc/wall_core.hpp).  A cell
 * of a car's world is occupied iff it is occupied on the grid, lies in one of the car's discs or on one of its walls.
 *   offsets [B+1] / walls [offsets[B]][4]: wall q of car b is entry offsets[b] + q.  offsets == NULL: no walls.  Walls are
 *   a fourth independent per-car setting beside the static discs, the movers and the traffic: K0w rasterises them into a
 *   table once, when they are set (sized by the sum of the walls' longer extents), and K0c, K0l, K0f and the recorder read
 *   them from the next step on.  All settings in force must be for the same B (else MPMPC_E_STATE; the other three
 *   setters check the same against the walls in force).  MPMPC_E_ARG, decided on the host before any device call: B
 *   outside [1, max_batch], more than 16 walls for one car, offsets that decrease, an end point outside [1, width - 2] x
 *   [1, height - 2] (the anti-aliased neighbours may step one cell past an end point; the reference raises or wraps
 *   there).  A wall of one cell is allowed.  A refused call leaves every setting as it was.  Needs mpmpc_build_corridor
 *   like the discs (else MPMPC_E_STATE) and is void after a change of map, path or geometry in the same way.  May be
 *   called before mpmpc_rollout_init or between mpmpc_rollout_step calls: it applies from the next step on and keeps the
 *   rollout's state.  Walls count for every consumer of the world of the last step - mpmpc_rollout_corridor,
 *   mpmpc_rollout_scan, the audit, recorded rows; mpmpc_rollout_obstacles keeps returning the discs only.  A rollout
 *   without walls launches exactly what it launched before. */
int mpmpc_rollout_set_walls(mpmpc_handle h, int32_t B, const int32_t* offsets, const int32_t* walls);
/* Plant: the vehicle that differs from the controller's model, per car and off by default - the sim-to-real question (does
 * this tuning still clear the obstacle with 5 % wheelbase error, a steering bias, a lagging servo, noisy localisation?)
 * without a host round trip per step.  With a plant in force the true vehicle and the controller's knowledge of its pose
 * separate: the TRUE pose stays what mpmpc_rollout_state returns, and K3a localises on a MEASURED pose kept in a buffer of
 * its own (K3n writes it in front of K3a); K3p drives the car in place of K3b.  params [B][11] per car, in this order
 * (identity: 1, 1, 0, 1, 1, 1, +inf, 0, 0, 0, 0):
 *    0 speed_gain       finite              4 speed_lag   in (0, 1]                   7 speed_noise    [m/s]
 *    1 steer_gain       finite              5 steer_lag   in (0, 1]                   8 steer_noise    [rad]
 *    2 steer_offset     finite [rad]        6 steer_rate  > 0 [rad / step], +inf ok   9 position_noise [m]
 *    3 wheelbase_scale  finite, > 0                                                  10 heading_noise  [rad]   (7 .. 10 finite, >= 0)
 * Per step k (0-based, counted from mpmpc_rollout_init - the movers' index), j = k - step0, (n_v, n_d, n_x, n_y, n_psi) the
 * car's five variates of the step:
 *    measure   meas = (x + position_noise n_x, y + position_noise n_y, psi + heading_noise n_psi)      cars with alive == 1
 *    drive     (v_cmd, d_cmd), the infeasibility counter, u (the COMMANDED control) and the N - 1 ending as without a plant;
 *              v_t = speed_gain v_cmd + speed_noise n_v;   d_t = steer_gain d_cmd + steer_offset + steer_noise n_d;
 *              v_act += speed_lag (v_t - v_act);  d_new = d_act + steer_lag (d_t - d_act), its change from d_act limited to
 *              +-steer_rate;  the bicycle step with (v_act, d_act) and the wheelbase L wheelbase_scale;  s advances by the
 *              model's s_dot on v_act and the x0 of the MEASURED pose (wheel odometry: s drifts from the true arc length;
 *              mpmpc_rollout_reroute onto the car's own route relocalises it)
 * The variates are triangular on (-1, 1) (standard deviation 1 / sqrt 6), one 32-bit word of Philox4x32-10 each, key = the
 * seed, counter = (car0 + car, j, block): a draw depends on (seed, car0 + car, j, channel) only - not on B, on the steps per
 * call or on other cars - so the noise of any step can be recomputed from its index (mpmpc_plant_noise), as the movers'
 * positions can.  Gaussian noise is not offered.  The exact operation order, the generator and the variate are stated in
 * csrc/plant_core.hpp; an identity plant reproduces the rollout without one bit for bit.
 * The audit, mpmpc_rollout_scan, perception (K0s), traffic (K0t), the plan tracks, the recorder and mpmpc_rollout_reroute
 * keep reading the true pose: they judge or sense the true car.  x0 (state, recorder) is the measured pose's.
 *   mpmpc_rollout_set_plant  params == NULL: no plant.  act0 [B][2]: the executed (v, delta) the actuators start from, or
 *                           NULL for zeros; the call sets them and zeroes the accumulators.  car0: the index of car 0 in a
 *                           larger fleet.  step0 may be negative: a run resumed from a saved state of step k0 continues its
 *                           noise with step0 = -k0 and act0 = the saved act.  May be called before mpmpc_rollout_init or
 *                           between mpmpc_rollout_step calls: it applies from the next step on and keeps the rollout's
 *                           state.  MPMPC_E_ARG: a parameter outside the table, act0 not finite, B outside [1, max_batch];
 *                           a refused call leaves the previous setting in force.  A step whose B differs returns
 *                           MPMPC_E_STATE.  mpmpc_rollout_init with a plant in force keeps the parameters and zeroes the
 *                           actuator states and the accumulators.
 *   mpmpc_rollout_plant     any pointer may be NULL.  act [B][2]: the executed (v, delta) of the last driven step; meas
 *                           [B][3]: the pose K3a saw in the last step (cars that were running); ey_max / ey_sq / steps [B]:
 *                           max |e|, sum of e^2 and the number of steps over the steps the car was driven, e = the lateral
 *                           offset of the TRUE pose the step found the car at from the step's waypoint (cos / sin from K0's
 *                           host table: no device-libm result).  MPMPC_E_STATE if no step ran under the setting in force.
 *   mpmpc_plant_noise       out [n_steps][B][5] = (n_v, n_d, n_x, n_y, n_psi) of cars car0 .. car0 + B - 1 at j = j0 ..
 *                           j0 + n_steps - 1, computed on the device with plant_core.hpp's code; no handle needed.
 * A rollout without a plant launches exactly what it launched before. */
int mpmpc_rollout_set_plant(mpmpc_handle h, int32_t B, const double* params, uint64_t seed, int32_t car0, int64_t step0,
                            const double* act0);
int mpmpc_rollout_plant(mpmpc_handle h, int32_t B, double* act, double* meas, double* ey_max, double* ey_sq, int32_t* steps);
int mpmpc_plant_noise(int32_t device, uint64_t seed, int32_t car0, int32_t B, int64_t j0, int32_t n_steps, double* out);
/* Actuation delay and its compensation, per car and off by default - the one plant defect feedback alone cannot absorb: compute,
 * radio and servo latency of a few control steps.  Per car: delay d (a command issued at step k reaches the wheels at step
 * k + d) and assumed c (what the controller compensates for), integers in [0, MPMPC_DELAY_MAX]; c > d and c < d are legal.
 * Every car carries a shift register of its last MPMPC_DELAY_MAX issued commands (v, delta), the newest first.
 *    predict (K3d, in front of K3a, behind K3n; cars with alive == 1): from the pose the controller localises on (the plant's
 *              measured pose, else the true one) and s, the controller's NOMINAL model is stepped through the c commands still
 *              in flight, the oldest first, re-localising between the steps; K3a then localises on the predicted pose and s, so
 *              wp_id, x0, the corridor, the QP and the plan belong to where the car will be when the command takes effect.
 *              `now` keeps (e_y, e_psi, kappa) of the waypoint the car IS at.  A prediction that passes the end of the path
 *              finishes the car (alive = 0) up to c steps early.
 *    drive   (K3q, in place of K3b / K3p): the command, the infeasibility counter, u (the COMMANDED control) and the N - 1 ending
 *              as without a delay (a run that ends there leaves the register untouched); exec = d > 0 ? queue[d - 1] : command;
 *              the register shifts by one and takes the command; exec drives the car (through the plant when one is in force);
 *              s advances by the odometry of `now`, not of the predicted x0.
 * The exact operation order is stated in csrc/delay_core.hpp.  d = c = 0 reproduces the rollout without the setting bit for
 * bit (with and without a plant); with no plant, d = c and a car driven on every step, pred_pose / pred_s of step k are
 * bit-equal to pose / s at the beginning of step k + c.
 * The audit, mpmpc_rollout_scan, perception, traffic, the movers, the recorder's pose and mpmpc_rollout_reroute keep reading
 * the true pose; x0 and wp_id (state, recorder) are the predicted pose's.  A step with a delay and a lookahead
 * (mpmpc_rollout_set_lookahead) both in force returns MPMPC_E_STATE: lookahead under delay is not supported.
 *   mpmpc_rollout_set_delay  delay == NULL: off.  assumed == NULL: assumed = delay.  queue0 [B][MPMPC_DELAY_MAX][2]: the
 *                           commands in flight, queue0[b][i] issued i + 1 steps ago (the first d executions are queue0[b][d-1]
 *                           .. queue0[b][0]), or NULL for zeros: the car stands for d steps.  Validated on the host before
 *                           anything is touched - MPMPC_E_ARG: d or c outside [0, MPMPC_DELAY_MAX], queue0 not finite, B outside
 *                           [1, max_batch]; a refused call leaves the previous setting in force.  A step whose B differs returns
 *                           MPMPC_E_STATE.  May be called before mpmpc_rollout_init or between steps; mpmpc_rollout_init with a
 *                           delay in force keeps d and c and zeroes the registers - a resumed run sets the delay (with the saved
 *                           register as queue0) after it.
 *   mpmpc_rollout_delay     any pointer may be NULL.  queue [B][MPMPC_DELAY_MAX][2]: the registers; pred_pose [B][3], pred_s [B]:
 *                           what K3a saw in the last step; now [B][3]: (e_y, e_psi, kappa) of where the car was in the last step
 *                           (cars that were running).  MPMPC_E_STATE unless a step of B cars ran under the setting in force.
 * A rollout without the setting launches exactly what it launched before. */
#define MPMPC_DELAY_MAX 8
int mpmpc_rollout_set_delay(mpmpc_handle h, int32_t B, const int32_t* delay, const int32_t* assumed, const double* queue0);
int mpmpc_rollout_delay(mpmpc_handle h, int32_t B, double* queue, double* pred_pose, double* pred_s, double* now);
/* Dynamic single-track plant, per car and off by default: a car with mass, yaw inertia and tyres that slip and saturate, behind
 * a speed controller that needs time and traction - the questions about grip that a kinematic plant cannot be asked.  The
 * controller, the estimator's and the localiser's dead reckoning, the delay's prediction and the lookahead stay on the nominal
 * kinematic model.  Needs a plant in force for the same B cars (the identity will do; else a step returns MPMPC_E_STATE): K3y
 * drives the car in place of K3p, or of K3q under a delay.  The plant's gains, noise, lags and rate limit yield (v_act, d_act) as
 * before; then, per car with the state (vx, vy, r) - body-frame velocity at the centre of gravity and yaw rate, carried from step
 * to step - below v_dyn the car is kinematic at the speed its speed controller reaches, above it n explicit sub-steps integrate
 * the single-track model with linear tyres clipped to the friction ellipse (rear driven, static axle loads); s advances by the
 * odometry of the step's final vx.  params [B][11] per car, in this order:
 *    0 mass [kg] > 0          3 Cf [N/rad] > 0     6 speed_gain [1/s] > 0, +inf: ideal    9 v_dyn [m/s] > 0, +inf: never dynamic
 *    1 inertia [kg m^2] > 0   4 Cr [N/rad] > 0     7 a_drive [m/s^2] > 0, +inf allowed    10 substeps: an integer in [1, 64]
 *    2 lf [m] in (0, Lp)      5 mu > 0, +inf: none 8 a_brake [m/s^2] > 0, +inf allowed
 * Lp = wheelbase * wheelbase_scale is the plant's wheelbase.  The exact operation order is stated in csrc/dynamics_core.hpp.
 * v_dyn = +inf with speed_gain = +inf reproduces the plant alone bit for bit.  The audit, mpmpc_rollout_scan, perception,
 * traffic, the localiser's scan and the recorder keep the true pose; the plant's statistics go on as under K3p / K3q.
 *   mpmpc_rollout_set_dynamics  params == NULL: off.  state0 [B][3] or NULL for zeros.  Validated on the host before anything is
 *                           touched - MPMPC_E_ARG: a parameter outside its range, state0 not finite, B outside [1, max_batch]; a
 *                           refused call leaves the previous setting in force.  The first step that knows Ts, the plant and the
 *                           parameters returns MPMPC_E_STATE before any kernel is launched if a car's lf is not below its Lp or
 *                           the explicit sub-step is unstable: with lambda = max((Cf + Cr) / (m v_dyn), (lf^2 Cf + lr^2 Cr) /
 *                           (Iz v_dyn)) a run needs lambda * Ts / substeps <= 1 (v_dyn = +inf passes).  May be called before
 *                           mpmpc_rollout_init or between steps; mpmpc_rollout_init keeps the parameters and starts the state
 *                           and the accumulators over - a resumed run sets the dynamics (with the saved state) after it.
 *   mpmpc_rollout_dynamics  any pointer may be NULL.  state [B][3]; counts [3][B]: the steps that took the dynamic branch, and
 *                           those in which some sub-step clipped the front / the rear axle; peaks [3][B]: max |front slip angle|,
 *                           max |rear slip angle| [rad] and max lateral acceleration |Fyf cos(delta) + Fyr| / m over all
 *                           sub-steps (driven steps only).  MPMPC_E_STATE unless a step of B cars ran under the setting in force.
 *   mpmpc_dynamics_drive    without a handle, open loop: B cars from state0 (NULL: zeros) and pose0 [B][3] through
 *                           cmds [n_steps][B][2] = (v_act, d_act) on the wheelbase L - step steer, skidpad, launch.  Out: state
 *                           [B][3], pose [B][3], counts [3][B], peaks [3][B] and trace [n_steps][B][3], the pose after every step
 *                           (each may be NULL).  MPMPC_E_ARG for what the other two refuse, the stability bound included.
 * A rollout without the setting launches exactly what it launched before. */
int mpmpc_rollout_set_dynamics(mpmpc_handle h, int32_t B, const double* params, const double* state0);
int mpmpc_rollout_dynamics(mpmpc_handle h, int32_t B, double* state, int32_t* counts, double* peaks);
int mpmpc_dynamics_drive(int32_t device, int32_t B, int32_t n_steps, double L, double Ts, const double* params, const double* state0,
                         const double* pose0, const double* cmds, double* state, double* pose, int32_t* counts, double* peaks,
                         double* trace);
/* Pose estimator, per car and off by default: a 3-state extended Kalman filter on the world pose (x, y, psi) in the controller's
 * NOMINAL model, between the measurement and the controller (K3e, behind K3n and in front of K3d / K3a; cars with alive == 1).
 * With it everything the controller localises on takes the ESTIMATE instead of the measured (plant) or true pose: K3a without a
 * delay, K3d's starting pose with one.  The audit, mpmpc_rollout_scan, perception, traffic and its tracks, the recorder,
 * mpmpc_rollout_reroute and the plant's statistics keep the true pose.  Per car and step k, j = k - step0, z = the plant's
 * measured pose (else the true one):
 *    not primed:   est = z, cov = diag(p0_xy, p0_xy, p0_psi), primed - whatever the schedule says
 *    time update:  the nominal model's pose step on est with the command the controller believes reached the wheels in step
 *                  k - 1 (without a delay u of the state; with one entry c of the register, c the car's assumed delay);
 *                  P <- F P F^T + diag(q_xy, q_xy, q_psi) with the model's Jacobian F at the heading before the step
 *    measurement:  if j mod period == 0 and the measurement is not dropped (probability drop; a draw of (seed, car0 + car, j)):
 *                  three sequential scalar updates in the order x, y, psi, the heading innovation wrapped to [-pi, pi)
 *    statistics:   from the true pose as the step finds it
 * The exact operation order is stated in csrc/estimator_core.hpp.  With an identity or absent plant, no noise and no delay (or
 * assumed == delay, every car driven) every innovation is exactly 0: est keeps the bits of the true pose and the rollout is the
 * rollout without the estimator, bit for bit.  Results depend on (seed, car0 + car, j) and the car's own state only.
 *   mpmpc_rollout_set_estimator  params == NULL: off.  params [B][MPMPC_ESTIMATOR_PARAMS] = q_xy, q_psi (finite, >= 0), r_xy,
 *                           r_psi (finite, > 0), p0_xy, p0_psi (finite, >= 0), period (an integer >= 1, as a double), drop in
 *                           [0, 1).  est0 [B][3] and cov0 [B][6] (the upper triangle Pxx, Pxy, Pxp, Pyy, Pyp, Ppp): both or
 *                           neither; given, they prime the cars - a saved run is resumed with what mpmpc_rollout_estimator
 *                           returned, step0 = -(the step of the save) and, for the command of the last step, the saved register
 *                           as mpmpc_rollout_set_delay's queue0 (mpmpc_rollout_init zeroes u: without a delay the first time
 *                           update of a resumed run is taken with the command (0, 0)).  Validated on the host before anything
 *                           is touched - MPMPC_E_ARG, and the previous setting stays in force.  A step whose B differs returns
 *                           MPMPC_E_STATE; so does a step under a delay with a car whose assumed delay is MPMPC_DELAY_MAX (the
 *                           command of the last step has left the register).  May be called before mpmpc_rollout_init or
 *                           between steps; mpmpc_rollout_init keeps the parameters, un-primes every car and zeroes the
 *                           statistics - a resumed run sets the estimator after it.
 *   mpmpc_rollout_estimator any pointer may be NULL.  est [B][3], cov [B][6]: as the last step's K3e left them; err2_max, err2_sum
 *                           [B]: maximum and sum over the car's steps of (est_x - x)^2 + (est_y - y)^2; meas2_sum [B]: the same
 *                           sum of z (every step, used or not); head2_sum [B]: the sum of the wrapped heading error of the
 *                           estimate, squared; used, steps [B]: measurements taken (priming included) and K3e steps.
 *                           MPMPC_E_STATE unless a step of B cars ran under the setting in force.
 * A rollout without the setting launches exactly what it launched before. */
#define MPMPC_ESTIMATOR_PARAMS 8
int mpmpc_rollout_set_estimator(mpmpc_handle h, int32_t B, const double* params, uint64_t seed, int32_t car0, int64_t step0,
                                const double* est0, const double* cov0);
int mpmpc_rollout_estimator(mpmpc_handle h, int32_t B, double* est, double* cov, double* err2_max, double* err2_sum, double* meas2_sum,
                            double* head2_sum, int32_t* used, int32_t* steps);
/* Lidar localisation, per fleet and off by default: scan matching (K0d, K3l; the law and the exact operation order:
 * csrc/localiser_core.hpp).  Every scheduled step each running car scans its TRUE world with K0l itself - base map, discs,
 * movers at step k, traffic and walls - and matches the scan against the map it knows in advance, the BASE map, from dead
 * reckoning; the FIX takes the place of the measured pose: the estimator measures it, and the controller localises on the
 * estimate, else on the fix (else on the plant's measured pose, else on the true one).  A plant still measures (its `meas` and
 * mpmpc_rollout_plant are unchanged), but nothing plans on that then.  The audit, mpmpc_rollout_scan, perception, traffic, the
 * recorder and mpmpc_rollout_reroute keep the true pose.
 *    the field    F[j][i] = min(cap, the smallest squared cell distance <= D^2 to an occupied cell of the grid), cap = D^2 + 1,
 *                 one byte per cell; outside the grid: cap
 *    prior        not primed: the true pose (the step counts, no scan is used); else the nominal model's step on the last fix
 *                 with the command believed executed in step k - 1 (the estimator's rule)
 *    schedule     (k - step0) mod period != 0: fix = prior, no scan
 *    scan         beam b is a hit iff ranges[b] < range_m; a hit's range takes sigma_r * n_b, n_b a triangular variate of
 *                 (seed, car0 + car, k - step0, b); fewer than min_hits hits or a prior that is not finite: fix = prior, lost
 *    match        headings psi_t = prior_psi + t * step_psi, t in [-T, T]; every hit's endpoint cell from the prior under psi_t;
 *                 score(a, c, t) = sum over the hits of F(cell + (a, c) * m), a, c in [-W, W]; the winner: the smallest
 *                 (score, a^2 + c^2, t^2, idx), idx = ((t + T)(2W + 1) + (c + W))(2W + 1) + (a + W);
 *                 fix = (prior_x + a m res, prior_y + c m res, psi_t); a winner on the window's border counts as edge
 *    statistics   from the true pose as the step finds it
 *   mpmpc_distance_field   K0d without a handle: data [height][width] (1 free / 0 occupied), D in [1, 15] -> field_out
 *                          [height][width] bytes.
 *   mpmpc_scan_match       scan and match (no noise) of B (prior, scan) pairs without a handle: prior [B][3], ranges
 *                          [B][n_beams] -> fix_out [B][3], score_out, cand_out (idx; both -1 without a match), hits_out [B].
 *   mpmpc_rollout_set_localiser  B = 0: off.  n_beams, angles, range_m under mpmpc_lidar_scan's checks; D in [1, 15]; m >= 1
 *                          cells; W in [0, 16]; T in [0, 8]; step_psi >= 0 (> 0 when T > 0); min_hits >= 1; sigma_r >= 0;
 *                          period >= 1; (2T + 1) n_beams <= 8192; fix0 [B][3] or NULL - given, it primes the cars (a saved run is
 *                          resumed with the fix mpmpc_rollout_localiser returned and step0 = -(the step of the save)).  Validated
 *                          before anything is touched - MPMPC_E_ARG, and the previous setting stays in force.  Needs
 *                          mpmpc_set_map (MPMPC_E_STATE); the field is built by this call, and a step after mpmpc_set_map /
 *                          mpmpc_set_path / mpmpc_set_path_geometry returns MPMPC_E_STATE until it is set again.  So does a step
 *                          whose B differs, and one under a delay with an assumed delay of MPMPC_DELAY_MAX.  May be called
 *                          before mpmpc_rollout_init or between steps; mpmpc_rollout_init keeps the setting, un-primes every car
 *                          and zeroes the statistics - a resumed run sets the localiser after it.
 *   mpmpc_rollout_localiser  any pointer may be NULL.  fix, prior [B][3], cand, score, hits [B] as the car's last step left them
 *                          (cand, score: -1 without a match; hits: -1 without a scan); ranges [B][n_beams]: the scans of the
 *                          last scheduled step, the hits noisy; err2_max, err2_sum [B]: maximum and sum of the fix's squared
 *                          position error; head2_sum: the sum of its wrapped heading error squared; prior2_sum: err2_sum of the
 *                          prior; steps, matched, lost, edge [B].  MPMPC_E_STATE unless a step of B cars ran under the setting.
 * The scan is mpmpc_lidar_scan's, the reference's lidar: at headings above 0 (and unwrapped ones beyond pi) it mirrors the cells
 * behind the car on its right onto the beams behind it on its left, and the match follows what the sensor reports.
 * Out of scope: per-car settings, matching against discs, walls or perceived worlds, sub-cell refinement.  (The fix and the scan of every
 * step: MPMPC_REC_FIX / MPMPC_REC_SCAN of mpmpc_rollout_record.)
 * A rollout without the setting launches exactly what it launched before. */
int mpmpc_distance_field(int32_t device, int32_t height, int32_t width, const int8_t* data, int32_t D, uint8_t* field_out);
int mpmpc_scan_match(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y, double resolution,
                     int32_t B, const double* prior, const double* ranges, int32_t n_beams, const double* angles, double range_m, int32_t D,
                     int32_t m, int32_t W, int32_t T, double step_psi, int32_t min_hits, double* fix_out, int32_t* score_out,
                     int32_t* cand_out, int32_t* hits_out);
int mpmpc_rollout_set_localiser(mpmpc_handle h, int32_t B, int32_t n_beams, const double* angles, double range_m, int32_t D, int32_t m,
                                int32_t W, int32_t T, double step_psi, int32_t min_hits, double sigma_r, int32_t period, uint64_t seed,
                                int32_t car0, int64_t step0, const double* fix0);
int mpmpc_rollout_localiser(mpmpc_handle h, int32_t B, double* fix, double* prior, int32_t* cand, int32_t* score, int32_t* hits, double* ranges,
                            double* err2_max, double* err2_sum, double* head2_sum, double* prior2_sum, int32_t* steps, int32_t* matched,
                            int32_t* lost, int32_t* edge);

/* Recorder: while the cars drive, the rollout appends one record per car and recorded step to a device-resident trace
 * (what src/simulation.py:117-157 logs per step on the host: x_log / y_log / v_log and MPC.current_prediction), and
 * mpmpc_rollout_trace brings any range of records back.  A rollout that does not ask for it launches what it always did.
 *   mpmpc_rollout_record    reserves device memory for `capacity` records of B cars - the basic fields (s, pose, wp_id,
 *                           x0, u, status, counter, alive: 88 bytes per car) plus those selected by `fields` - and switches
 *                           recording on; capacity = 0 switches it off and frees the memory.  Rollout step k (0-based,
 *                           counted from mpmpc_rollout_init) is recorded when k % stride == 0.  May be called before or
 *                           after mpmpc_rollout_init (which keeps the configuration and empties the trace); the B of later
 *                           mpmpc_rollout_init / _step calls must equal this B (MPMPC_E_STATE).  capacity < 0, stride < 1,
 *                           unknown bits in fields, B outside [1, max_batch]: MPMPC_E_ARG; no memory: MPMPC_E_HIP, and
 *                           recording is off.
 *   mpmpc_rollout_step      never overwrites or drops records: a call whose records do not fit into what is left of
 *                           `capacity` returns MPMPC_E_STATE before it launches anything.
 *   mpmpc_rollout_recorded  records held, steps taken since mpmpc_rollout_init (either pointer may be NULL).
 *   mpmpc_rollout_trace     records first .. first + count - 1 into host arrays [count][B][...]: pose 3, x0 3, u 2,
 *                           plan 2N, pred_x / pred_y N-2, ub / lb N.  Any pointer may be NULL; a field that was not
 *                           selected, or records beyond those held: MPMPC_E_STATE.  The trace has its own memory: it stays
 *                           readable after mpmpc_upload / mpmpc_solve on the handle have invalidated the rollout's state,
 *                           until the next mpmpc_rollout_init or mpmpc_rollout_record.
 * A record, with a_in / a the car's `alive` before / after the step ("empty": NaN, wp_id -1, status 0):
 *   s, pose        the state the step STARTED from (the state after the last step is mpmpc_rollout_state's); empty if
 *                  a_in != 1 (the car had ended before)
 *   wp_id, x0      this step's; empty if a_in != 1 or a == 0 (localise found the lap finished)
 *   status, u, plan, ub, lb   this step's solver status, applied control (v, delta), MPC.current_control after the step,
 *                  the corridor row the QP used; empty unless a is 1 or -1 (the solve launch also re-solves ended cars
 *                  on stale inputs: their values are masked here)
 *   pred_x, pred_y the predicted path, MPC.update_prediction (src/MPC.py:224-248): stage k = 2 .. N-1 of the step's
 *                  solution at waypoint w = wp_id + k, x_w - e_y sin(psi_w), y_w + e_y cos(psi_w); empty unless the
 *                  status is usable (1, 2, -2) - on a fallback step the reference keeps DISPLAYING the previous step's
 *                  prediction, the trace holds none
 *   counter, alive as they stand after the step, always */
#define MPMPC_REC_PLAN 1   /* the car's plan after the step: MPC.current_control, [2N]               */
#define MPMPC_REC_PRED 2   /* predicted path of the step, world x / y of stages 2 .. N-1, [N-2] each */
#define MPMPC_REC_ROWS 4   /* the corridor row the step's QP used, ub / lb [N] each                  */
int mpmpc_rollout_record(mpmpc_handle h, int32_t B, int32_t capacity, int32_t fields, int32_t stride);
int mpmpc_rollout_recorded(mpmpc_handle h, int32_t* n_records, int32_t* n_steps);
int mpmpc_rollout_trace(mpmpc_handle h, int32_t B, int32_t first, int32_t count, double* s, double* pose, int32_t* wp_id,
                        double* x0, double* u, int32_t* status, int32_t* counter, int32_t* alive, double* plan,
                        double* pred_x, double* pred_y, double* ub, double* lb);
/* The pose chain in the trace: five more bits for `fields`, each the state of one feature that stands between the car's true pose
 * and the pose its controller plans on.  Every value is the one the matching getter (mpmpc_rollout_plant / _delay / _estimator /
 * _localiser) would return if it were called right after that step, so one multi-step mpmpc_rollout_step yields the time series
 * that otherwise takes one step per call and a download of every getter in between.
 *   bit  macro             per car and record
 *     8  MPMPC_REC_PLANT   act [2], meas [3]
 *    16  MPMPC_REC_DELAY   queue [MPMPC_DELAY_MAX][2], pred_pose [3], pred_s, now [3]
 *    32  MPMPC_REC_EST     est [3], cov [6], used (int32)
 *    64  MPMPC_REC_FIX     fix [3], prior [3], cand, score, hits (int32 each)
 *   128  MPMPC_REC_SCAN    ranges [n_beams]: the localiser's scan of the step, the hits noisy
 * Masks, with a_in the car's `alive` before the step ("empty": NaN for doubles, -2 for cand / score / hits - where -1 keeps its
 * meanings "no match" / "no scan this step" -, -1 for used):
 *   act, queue, used   state that outlives a step: as it stands after the step, for every car, like `counter`
 *   meas, pred_pose, pred_s, now, est, cov, fix, prior, cand, score, hits
 *                      the step's own: empty if a_in != 1 (K3n, K3d, K3e and K3l run for the cars the step finds running)
 *   ranges             empty unless the record's own hits >= 0 (a_in == 1 and the step was a scheduled one)
 *   feature off        a whole group - act and meas, queue .. now, est .. used, fix .. hits and ranges - is empty for every car at
 *                      a step its feature is not in force for; settings may change between mpmpc_rollout_step calls
 * mpmpc_rollout_record with MPMPC_REC_SCAN needs a localiser in force (MPMPC_E_STATE otherwise): a record holds that setting's
 * n_beams ranges per car, and a step under a localiser with another n_beams while such a trace is open returns MPMPC_E_STATE
 * before it launches anything.  Bits above 255: MPMPC_E_ARG.  A rollout that records no chain bit launches what it launched
 * before; one that does gets one more kernel per recorded step, which reads the features' own buffers.
 *   mpmpc_rollout_trace_chain  records first .. first + count - 1 into host arrays [count][B][...], as mpmpc_rollout_trace does
 *                      for the other fields and with the trace's lifetime.  Any pointer may be NULL; a field whose bit was not
 *                      selected, or records beyond those held: MPMPC_E_STATE. */
#define MPMPC_REC_PLANT 8
#define MPMPC_REC_DELAY 16
#define MPMPC_REC_EST 32
#define MPMPC_REC_FIX 64
#define MPMPC_REC_SCAN 128
int mpmpc_rollout_trace_chain(mpmpc_handle h, int32_t B, int32_t first, int32_t count, double* act, double* meas, double* queue,
                              double* pred_pose, double* pred_s, double* now, double* est, double* cov, int32_t* used, double* fix,
                              double* prior, int32_t* cand, int32_t* score, int32_t* hits, double* ranges);

/* replaces MPC._init_problem (src/MPC.py:61-155) for B instances: LTV linearisation
 * (src/spatial_bicycle_models.py:391-417) around waypoints wp_id+0..N-1, offsets, speed cap from
 * the previous plan cc_prev (src/MPC.py:86-87,111-113), box bounds, references, cost vectors.
 *   wp_id[B], x0[B*3] (= model.spatial_state), cc_prev[B*2N] (= MPC.current_control),
 *   lb/ub [B*N]: per-instance corridor, or both NULL to use the table of mpmpc_set_corridor.
 * qp_out (host, may be NULL) receives the stage-blocked QP [MPMPC_NUM_FIELDS][B][LD] with
 * LD = mpmpc_stage_ld(N); field order: ds, a10, a20, b20, beq[3], lo[5], hi[5], q[5], p[5]
 * (A_k = [[1,ds,0],[a10,1,0],[a20,0,1]], B_k = [[0,0],[0,ds],[b20,0]] couple stage k to k+1;
 * beq = rhs of equality block k; lo/hi/q/p over (e_y,e_psi,t,v,kappa) of stage k). */
int mpmpc_assemble(mpmpc_handle h, int32_t B, const int32_t* wp_id, const double* x0,
                   const double* cc_prev, const double* lb, const double* ub, double* qp_out);
int32_t mpmpc_stage_ld(int32_t N);

/* replaces _init_problem + osqp setup/solve + solution extraction (src/MPC.py:180-194) for B
 * instances.  Outputs (any may be NULL): z[B*(5N+3)] primal solution (dec.x), u0[B*2] = (v_0,
 * delta_0 = arctan(kappa_0 * wheelbase)) as returned by get_control, status[B], iters[B*2]
 * (OSQP's iteration counter: 0 = certified from the closed loop's warm-start guess, 1 = the early attempt alone - the general
 * kernels start it from OSQP's first iterate, the reduced-native kernels from x = 0 without any OSQP iterate -, more = the ADMM
 * loop ran; interior-point iterations), resid[B*2] (primal, dual residual, unscaled),
 * y[B*(8N+6)] multipliers in the reference's row order. */
int mpmpc_solve(mpmpc_handle h, int32_t B, const int32_t* wp_id, const double* x0,
                const double* cc_prev, const double* lb, const double* ub, double* z, double* u0,
                int32_t* status, int32_t* iters, double* resid, double* y);

/* Split form of mpmpc_solve for callers that keep inputs resident in HBM (benchmarks, closed
 * loops): upload once, launch any number of times (asynchronous on the handle's stream),
 * synchronise, download.  mpmpc_upload returns as soon as the caller's buffers may be reused; the
 * transfer itself is ordered before everything launched after it on the handle's stream. */
int mpmpc_upload(mpmpc_handle h, int32_t B, const int32_t* wp_id, const double* x0,
                 const double* cc_prev, const double* lb, const double* ub);
/* The outputs of a resident launch are defined after the next mpmpc_sync / mpmpc_download on the handle (the only ways to
 * read them), and only for the LAST launch before it.  Resident launches are pipelined inside the handle (by default three
 * launch slots - stream, output block - used in turn: mpmpc_set_pipeline): launch k + 1, k + 2 run beside launch k, whose
 * outputs stay untouched until launch k + 3; mpmpc_sync / mpmpc_download and every other call on the handle wait for all of them.  The
 * library also uses the freedom the first sentence leaves: the second kernel of a launch (the tail: instances the first kernel could not certify, usually none) is not
 * enqueued while the launches whose outcome the host has seen left no tail; a launch that does leave one has it run inside
 * the next mpmpc_sync / mpmpc_download / mpmpc_upload / mpmpc_set_* call, before that call does anything else. */
int mpmpc_solve_resident(mpmpc_handle h, int32_t B);
/* Do resident launches store the multipliers y (46 % of a solve's output bytes)?  Default 1.  mpmpc_solve decides per
 * call (y == NULL: not stored), the closed-loop rollout never stores them.  mpmpc_download refuses a y the last launch
 * did not produce. */
int mpmpc_set_outputs(mpmpc_handle h, int32_t want_y);
/* Resident launches in flight, 1 .. 8: 3 (default) = pipelined as described above; 1 = every launch on one stream and one output
 * block, each waiting for the one before (what every other entry point does anyway).  Every launch in flight needs a stream of
 * its own, and the HIP runtime spreads the streams of a process over GPU_MAX_HW_QUEUES hardware queues (4 when the variable is
 * absent); streams that share a queue take turns, which costs more than the extra launch gains.  So the handle runs
 *     s = mpmpc_pipeline_streams(depth, mpmpc_hw_queue_budget(getenv("GPU_MAX_HW_QUEUES")))  =  min(depth, queues)
 * launch slots, whatever depth asks for beyond that: the library reads the variable (once per process), it never sets it, and a
 * caller need not know about it.  What a caller may rely on: launch k's outputs stay untouched until launch k + s, 1 <= s <= depth;
 * a slot's launches run in the order they were issued; mpmpc_sync / mpmpc_download see the LAST launch, after waiting for all.
 * The library itself does nothing on the null stream, so that all of the process's queues are there for launch streams (a
 * process that uses the null stream, or streams of its own, beside a handle gives one of them away: depth 3 then fits 4 queues).
 * With depth > 1 (and more than one queue) the batch launches of the handle pack two / four instances into a wavefront from
 * 128 / 256 instances on (instead of 1 024 / 2 048): the handle is after throughput, several launches fill the chip. */
int mpmpc_set_pipeline(mpmpc_handle h, int32_t depth);
/* The two halves of that rule, pure functions (no device, no handle).  mpmpc_hw_queue_budget: the queue count a value of
 * GPU_MAX_HW_QUEUES stands for - NULL (variable absent), text that is not one positive decimal number, zero or a negative
 * number give the runtime's default, 4.  mpmpc_pipeline_streams: launch slots a handle uses for a depth asked of
 * mpmpc_set_pipeline (clamped to 1 .. 8) in a process with hw_queues queues (below 1 counts as 1): min(depth, hw_queues). */
int32_t mpmpc_hw_queue_budget(const char* text);
int32_t mpmpc_pipeline_streams(int32_t depth, int32_t hw_queues);
/* Which solve kernels a launch runs, as the launcher itself decides it - a pure function (no device, no handle, no state;
 * the launcher calls the same code): the plan of a launch of B instances on a handle with this configuration and these
 * settings.  knobs[4] = what the policy reads of the handle: lanes per instance (mpmpc_set_packing), tail kernel
 * (mpmpc_set_tail_kernel: 0 / 1 / 2), launch slots in use (mpmpc_pipeline_streams), warm start (mpmpc_rollout_warm_start:
 * 0 / 1 / 2).  closed_loop: a step of mpmpc_rollout_step.  kind: 0 a launch that is waited for on its own (mpmpc_solve,
 * mpmpc_solve_staged, timed launches, rollout steps), 1 one of several in flight (mpmpc_solve_resident, mpmpc_staged_begin).
 * Returns the number of stages, 1 .. MPMPC_PLAN_MAX_STAGES, in stream order, and writes one row of MPMPC_PLAN_ROW int32 per stage
 * to rows; MPMPC_E_ARG for arguments no handle can hold (horizon, B < 1, a packing mpmpc_set_packing refuses, ...).  A row:
 *    0 family       MPMPC_K_*
 *    1 G            lanes per instance          } template arguments of the instantiation; 0 where the family has none
 *    2 C            chain split of the factorisation }
 *    3 var          general kernels: 0 full problem, 1 full weights, 2 reduced polish, 3 free e_psi / t
 *    4 warm         1: the closed loop's warm-started instantiation
 *    5 mode         general kernels: 0 the whole solve of every instance, 2 the full run on the instances of a list
 *    6 grid         workgroups
 *    7 block        lanes per workgroup
 *    8 reads        MPMPC_LIST_*: the list whose instances the stage takes (none: every instance of the batch)
 *    9 fills        MPMPC_LIST_*: the list it appends what it cannot decide to
 *   10 clear        1: the list it fills is emptied on the stream in front of it
 *   11 deferrable   1: the launcher may hold the stage back while the launches it has seen left the list it reads empty
 *   12 turn         1: the launch takes the slot's next flip list and a new sequence number */
#define MPMPC_PLAN_ROW 13
#define MPMPC_PLAN_MAX_STAGES 3
#define MPMPC_K_GENERAL 0          /* mpmpc_solve_kernel<64, C, warm, var>          one instance per wavefront */
#define MPMPC_K_REDUCED 1          /* mpmpc_reduced_kernel<G, C, warm>              64 / G instances per wavefront */
#define MPMPC_K_REDUCED_T 2        /* mpmpc_reduced_t_kernel<64, C>                 terminal cost on the time state */
#define MPMPC_K_REDUCED_TAIL 3     /* mpmpc_reduced_tail_kernel<G, C>               the tail solver; stamps tail_flag + 1 */
#define MPMPC_K_PAIR 4             /* mpmpc_reduced_pair_kernel<G>                  two stages per lane, G lanes per instance */
#define MPMPC_K_PAIR_T 5           /* mpmpc_reduced_t_pair_kernel<64> */
#define MPMPC_K_PAIR_TAIL 6        /* mpmpc_reduced_tail_pair_kernel<64> */
#define MPMPC_K_BLOCK 7            /* mpmpc_solve_block_kernel<G, var>              one instance per workgroup of G lanes */
#define MPMPC_K_RBLOCK 8           /* mpmpc_reduced_block_kernel<G> */
#define MPMPC_K_PAIR_BLOCK 9       /* mpmpc_reduced_pair_block_kernel               two stages per lane, workgroup of 128 */
#define MPMPC_K_PAIR_BLOCK_TAIL 10 /* mpmpc_reduced_tail_pair_block_kernel */
#define MPMPC_K_PAIR_BLOCK_T 11    /* mpmpc_reduced_t_pair_block_kernel */
#define MPMPC_LIST_NONE 0
#define MPMPC_LIST_THIS 1          /* the list this launch fills */
#define MPMPC_LIST_NEXT 2          /* the list the slot's next launch fills (N <= 63: emptied by this launch's last kernel) */
#define MPMPC_LIST_LEFT 3          /* what the tail solver leaves to the general kernel */
int32_t mpmpc_launch_plan(const mpmpc_config* cfg, const mpmpc_settings* settings, const int32_t* knobs, int32_t B,
                          int32_t closed_loop, int32_t kind, int32_t* rows);
int mpmpc_sync(mpmpc_handle h);
int mpmpc_download(mpmpc_handle h, int32_t B, double* z, double* u0, int32_t* status,
                   int32_t* iters, double* resid, double* y);
/* Zero-copy host path.  mpmpc_solve copies the caller's (pageable) arrays into page-locked staging blocks and the results back
 * out of them - at B = 1 024 those host-side copies are two thirds of the call.  A caller that can build its inputs in place
 * and read the results in place asks for the blocks themselves: mpmpc_staging gives pointers into them, laid out for a batch
 * of B (same shapes as mpmpc_solve's arguments; any out-pointer may be NULL; the pointers stay valid until the handle is
 * destroyed, the layout until a call with another B), mpmpc_solve_staged runs upload + solve + download on them and returns
 * when the outputs are there: u0, status, iters, resid always, z if want_z, z and y if want_y.  with_rows = 0: lb / ub are not
 * read, the corridor table (mpmpc_set_corridor) applies.  Handles whose max_batch needs more than 64 MiB per block have no
 * staging blocks (MPMPC_E_STATE).  The blocks ARE the ones mpmpc_upload / mpmpc_download / mpmpc_solve stage through: a call
 * of those overwrites them, and mpmpc_staging itself first waits for an upload that is still leaving the input block. */
int mpmpc_staging(mpmpc_handle h, int32_t B, int32_t** wp_id, double** x0, double** cc_prev, double** lb, double** ub,
                  double** z, double** u0, int32_t** status, int32_t** iters, double** resid, double** y);
int mpmpc_solve_staged(mpmpc_handle h, int32_t B, int32_t with_rows, int32_t want_z, int32_t want_y);
/* The same call in two halves, for a loop that keeps several handles busy: mpmpc_staged_begin enqueues upload, solve and
 * download on the handle's stream and returns; mpmpc_staged_end waits for them (and runs the rarely needed second kernel of the
 * launch if it turns out to be needed).  Between the two the staging block belongs to the device: do not touch it.  Every other
 * call on the handle ends a begun call first. */
int mpmpc_staged_begin(mpmpc_handle h, int32_t B, int32_t with_rows, int32_t want_z, int32_t want_y);
int mpmpc_staged_end(mpmpc_handle h);
/* one resident pass with HIP events around each kernel on the handle's stream (ms); the launch runs alone on the chip */
int mpmpc_solve_resident_timed(mpmpc_handle h, int32_t B, float* ms_assemble, float* ms_solve);
/* n resident launches issued exactly as mpmpc_solve_resident issues them (double-buffered, see there), each between two
 * HIP events on its own stream: ms_each[n] = duration of every launch with the other slot's launch beside it on the chip,
 * *ms_span (may be NULL) = first start to last end.  What rocprofv3 --kernel-trace reports for the same loop. */
int mpmpc_solve_resident_profile(mpmpc_handle h, int32_t B, int32_t n, float* ms_each, float* ms_span);
/* n launches of the stand-alone assembly kernel K1 (what mpmpc_assemble runs, without its download) back to back on the
 * handle's stream, each between two HIP events: ms_each[n].  mpmpc_solve_resident_timed times K1 right after a solve launch,
 * whose dirty output lines K1's writes then push out of the cache; this is K1 on its own. */
int mpmpc_assemble_resident_timed(mpmpc_handle h, int32_t B, int32_t n, float* ms_each);

/* ---- speed profile (K4): replaces ReferencePath.compute_speed_profile, src/reference_path.py:289-354,
 * the reference's second OSQP call site, for B paths of n + 1 waypoints at once (no handle needed):
 *     min 1/2 |v|^2 - vmax' v   s.t.  a_min <= (v[i+1] - v[i]) / (2 li[i]) <= a_max,  v_min <= v[i] <= vmax[i],
 *     vmax[i] = min(v_max, sqrt(ay_max / (|kappa[i]| + eps)))
 * li [B][n]      distance waypoint i -> i+1            (src/reference_path.py:318)
 * kappa [B][n]   curvature of waypoint i               (src/reference_path.py:320)
 * limits [B][5]  a_min, a_max, v_min, v_max, ay_max    (the Constraints dict, src/reference_path.py:301-307)
 * v [B][n]       <- speed_profile (the caller copies v[n-1] to the last waypoint, src/reference_path.py:351-353)
 * status [B]     <- 1 KKT-certified optimum, 2 interior-point iterate (uncertified), -1 bad input
 * iters [B]      <- interior-point iterations (may be NULL)                                              */
int mpmpc_speed_profile(int32_t device, int32_t B, int32_t n, const double* li, const double* kappa,
                        const double* limits, double eps, double* v, int32_t* status, int32_t* iters);

/* ---- lidar (K0l): replaces LidarModel.scan, src/lidar_model.py:37-112, for B cars at once, each in a world of its own -
 * the grid plus the car's discs.  The law, step by step, is csrc/lidar_core.hpp; a cell's beam interval comes from the
 * DEVICE's atan2 (the first output of this library that a device-libm result decides: two implementations can differ
 * only where an angle ties with a beam, with -+pi/2 or with the +-pi wrap to within a few ulp).
 *   mpmpc_lidar_scan    needs no handle.  data [height][width] int8, 1 free / 0 occupied, with its frame (mpmpc_set_map's
 *                       arguments); pose [B][3] = x, y, psi; offsets [B+1] / discs [offsets[B]][3]: the cars' discs in
 *                       mpmpc_rollout_set_obstacles' format, offsets == NULL: none; angles [n_beams] finite and ascending;
 *                       ranges_out [B][n_beams] <- the distance to the nearest occupied cell each beam hits, range_m where
 *                       it hits none; a row of NaN for a pose that is not finite or further than 2^30 cells from the
 *                       origin.  MPMPC_E_ARG, before any device call: n_beams outside [1, 2048], angles not finite or
 *                       not ascending, range_m not positive and finite or above 2048 cells, offsets that decrease, more
 *                       than 64 discs for a car, a disc whose square leaves the grid.
 *   mpmpc_rollout_scan  every car of the running rollout from the pose its last step left it at, on the handle's resident
 *                       map, in the world mpmpc_rollout_obstacles would return (static discs, movers, traffic slots of
 *                       the last step); without a per-car setting in force: the base map.  Cars are scanned whatever
 *                       their alive.  Nothing but the result passes through the host, and the call writes nothing the
 *                       rollout reads.  MPMPC_E_STATE: no rollout of exactly B cars (or one invalidated by an upload),
 *                       no map, a per-car setting in force that no step has used yet or that was set anew since. */
int mpmpc_lidar_scan(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                     double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                     int32_t n_beams, const double* angles, double range_m, double* ranges_out);
int mpmpc_rollout_scan(mpmpc_handle h, int32_t B, int32_t n_beams, const double* angles, double range_m, double* ranges_out);

/* ---- footprint audit (K0f): did a car touch anything, and how close did it get?  For every car its rectangle - length
 * along the heading, car_width across it, centred at the pose (x, y, psi) - is tested against the car's own world, the grid
 * plus the car's discs.  The law, step by step, is csrc/footprint_core.hpp: over the occupied cells whose centres lie within
 * reach_m of the rectangle, contact = a cell centre inside or on the rectangle, clearance = the smallest distance of a cell
 * centre from the rectangle, reach_m when there is none that near (exact: the window of cells is chosen so that no cell
 * outside it can matter).  cos(psi) and sin(psi) come from the DEVICE's libm: two implementations can differ in the flag
 * only where a cell centre lies on the rectangle's boundary to within rounding, and in the clearance by a few ulp.  A
 * pose that is not finite or lies more than 2^30 cells from the origin gives contact 0, clearance NaN.
 *   mpmpc_footprint_audit    needs no handle.  data [height][width] int8, 1 free / 0 occupied, with its frame (mpmpc_set_map's
 *                            arguments); pose [B][3]; offsets [B+1] / discs [offsets[B]][3]: the cars' discs in
 *                            mpmpc_rollout_set_obstacles' format, offsets == NULL: the base map only; contact_out [B],
 *                            clearance_out [B].  MPMPC_E_ARG, before any device call: length, car_width or reach_m not
 *                            positive and finite, reach_m plus half the rectangle's diagonal above 256 cells, offsets
 *                            that decrease, more than 64 discs for a car, a disc whose square leaves the grid.
 *   mpmpc_rollout_set_audit  mode 0: off (the default; mpmpc_rollout_step launches nothing new), 1: every step audits every
 *                            car that is still running after localisation - pose k in world k: the step's static discs,
 *                            movers and traffic slots, or the base map when no per-car setting is in force -, 2: as 1, and
 *                            a car in contact ends there with alive = -5: it is not driven, its corridor row is still
 *                            built and its solve still runs, as for -3 / -4.  The setting persists across
 *                            mpmpc_rollout_init; the accumulators start over with every mpmpc_rollout_init and every
 *                            call of this function.  Needs mpmpc_set_map: without it mpmpc_rollout_step fails with
 *                            MPMPC_E_STATE (and with MPMPC_E_ARG if the window exceeds 256 cells on the map of the moment).
 *   mpmpc_rollout_audit      the accumulators, [B] each, any pointer may be NULL: contact_steps (audited steps with contact),
 *                            first_contact (step index of the first, counted from mpmpc_rollout_init; -1: none),
 *                            min_clearance (the smallest seen; reach_m at the start), min_step (the first step that reached
 *                            it; -1 while nothing came nearer than reach_m), last_contact / last_clearance (the verdict of
 *                            the car's last audited step; 0 / NaN before the first).  MPMPC_E_STATE: the audit is off, or
 *                            its accumulators were set up for another number of cars. */
int mpmpc_footprint_audit(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                          double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                          double length, double car_width, double reach_m, int32_t* contact_out, double* clearance_out);
int mpmpc_rollout_set_audit(mpmpc_handle h, int32_t mode, double length, double car_width, double reach_m);
int mpmpc_rollout_audit(mpmpc_handle h, int32_t B, int32_t* contact_steps, int32_t* first_contact, double* min_clearance,
                        int32_t* min_step, int32_t* last_contact, double* last_clearance);

/* ---- worlds with walls, no handle needed.  wall_offsets [B+1] / walls [wall_offsets[B]][4] as for mpmpc_rollout_set_walls
 * (NULL: no walls; MPMPC_E_ARG for the same lists it refuses).  K0w rasterises the walls first, on the same stream.
 *   mpmpc_lidar_scan_world / mpmpc_footprint_audit_world   mpmpc_lidar_scan / mpmpc_footprint_audit in worlds of grid, discs
 *                       and walls; the two older entry points are calls of these with NULL.
 *   mpmpc_world_grid    ONE car's world as a grid: grid_out [height][width] int8, 1 free / 0 occupied - data with the
 *                       n_discs discs ([n_discs][3], at most 64) and the n_walls walls ([n_walls][4], at most 16) stamped
 *                       in, through the predicate every kernel uses (K-world).  For plots, and the pin of the predicate. */
int mpmpc_lidar_scan_world(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                           double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                           const int32_t* wall_offsets, const int32_t* walls, int32_t n_beams, const double* angles,
                           double range_m, double* ranges_out);
int mpmpc_footprint_audit_world(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                                double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                                const int32_t* wall_offsets, const int32_t* walls, double length, double car_width, double reach_m,
                                int32_t* contact_out, double* clearance_out);
int mpmpc_world_grid(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                     double resolution, int32_t n_discs, const int32_t* discs, int32_t n_walls, const int32_t* walls,
                     int8_t* grid_out);

/* ---- perception: plan on what the lidar saw (K0s; the law: csrc/perception_core.hpp).  A car has up to 64 disc slots - its
 * combined list in the order mpmpc_rollout_obstacles returns it: static discs, movers, traffic slots - and up to 16 wall slots.
 * A slot is SEEN by a scan iff it occupies a nearest hit cell of some beam.
 *   mpmpc_perception_scan         no handle; arguments, checks (MPMPC_E_ARG before any device call), scratch and stream as for
 *                                 mpmpc_lidar_scan_world.  ranges_out [B][n_beams] may be NULL and is bit-equal to
 *                                 mpmpc_lidar_scan_world's; disc_seen_out [B] uint64, bit q = disc slot q; wall_seen_out [B]
 *                                 uint32, bit q = wall slot q (neither may be NULL).
 *   mpmpc_rollout_set_perception  angles == NULL: off (the default; mpmpc_rollout_step launches what it always did).  Else every
 *                                 step, every car with alive == 1 as the step finds it scans its TRUE world of that step from
 *                                 its pose; seen slots get last_seen = k (steps count from mpmpc_rollout_init) and first_seen
 *                                 = k if it was -1.  The step's corridor rows (K0c) are then built in the PERCEIVED world: the
 *                                 base map plus the KNOWN slots - a static disc or a wall once seen, a mover for `hold` further
 *                                 steps after it was last seen (at its true disc of the step), a traffic slot in the step it is
 *                                 seen.  mpmpc_rollout_corridor, recorded rows and the verdicts -3 / -4 report that world; the
 *                                 audit, mpmpc_rollout_scan, mpmpc_rollout_obstacles and traffic stay in the true one.
 *                                 MPMPC_E_ARG: what mpmpc_lidar_scan refuses of n_beams, angles and range_m; hold < 0.  The
 *                                 setting persists across mpmpc_rollout_init and may be changed between steps; this call,
 *                                 mpmpc_rollout_init and each of the four per-car setters reset every slot of every car to
 *                                 "never seen".  A step with perception on needs mpmpc_set_map (else MPMPC_E_STATE); while no
 *                                 per-car setting is in force there is nothing to perceive and the step launches nothing new.
 *   mpmpc_rollout_perception      what the cars know: disc_first / disc_last [B][64], wall_first / wall_last [B][16] (step
 *                                 indices, -1: never seen, and for unused slots), disc_known [B] uint64 / wall_known [B]
 *                                 uint32: the masks the last step planned with.  Any pointer may be NULL.  MPMPC_E_STATE:
 *                                 perception is off, no step has perceived since a reset, or B is not the rollout's. */
int mpmpc_perception_scan(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                          double resolution, int32_t B, const double* pose, const int32_t* offsets, const int32_t* discs,
                          const int32_t* wall_offsets, const int32_t* walls, int32_t n_beams, const double* angles, double range_m,
                          double* ranges_out, uint64_t* disc_seen_out, uint32_t* wall_seen_out);
int mpmpc_rollout_set_perception(mpmpc_handle h, int32_t n_beams, const double* angles, double range_m, int32_t hold);
int mpmpc_rollout_perception(mpmpc_handle h, int32_t B, int32_t* disc_first, int32_t* disc_last, int32_t* wall_first,
                             int32_t* wall_last, uint64_t* disc_known, uint32_t* wall_known);

/* ---- reference paths (K0p): replaces ReferencePath.__init__, src/reference_path.py:110-287, for P paths at once, each in a
 * world of its own - from corner points to the per-waypoint tables and the static width.  The law, step by step, is
 * csrc/path_core.hpp.  Counts, smoothing, waypoints and the normals' target cells are host code inside the call - every libm
 * result of a path (atan2, cos, sin) is the HOST's, as for mpmpc_set_path_geometry -; the width, 18 anti-aliased lines per
 * waypoint through the world's predicate, is the kernel.  No handle is needed.
 *   mpmpc_path_count   host only: the number of waypoints a path of these corner points ([n_corners][2]) will have; 1 or less:
 *                      there is no path.  Callers size `cap` with it.  MPMPC_E_ARG (a negative value): fewer than 2 corners, a
 *                      corner or a resolution that is not finite (and positive), smoothing outside [0, 63].
 *   mpmpc_path_build   data [height][width] int8, 1 free / 0 occupied, with its frame (mpmpc_set_map's arguments);
 *                      corner_offsets [P+1] / corners [corner_offsets[P]][2]: the paths' corner points; spec [P][2] =
 *                      path_resolution, max_width; ispec [P][2] = smoothing, circular; disc_offsets / discs and wall_offsets /
 *                      walls: the paths' worlds in the formats of mpmpc_rollout_set_obstacles / mpmpc_rollout_set_walls
 *                      (Map.obstacle_discs, Map.boundary_walls), NULL offsets: the base map; K0w rasterises the walls first,
 *                      on the same stream.  n_wp [P], status [P], length [P]; x, y, psi, kappa, ds_next, ub, lb [P][cap];
 *                      border [P][cap][4] = ub_x, ub_y, lb_x, lb_y, the static border cells mpmpc_set_path_geometry takes.
 *                      Rows from n_wp[p] on, and every row (and the length) of a path with a negative status, are NaN.
 *                      status[p]   0  built
 *                                  1  built, and some probed cell lay outside the grid: it counted as occupied (the reference
 *                                     would have raised there, or wrapped around)
 *                                 -1  fewer than 2 waypoints
 *                                 -2  n_wp[p] > cap (n_wp[p] still says how many)
 *                      A path with a negative status does not disturb the others.  MPMPC_E_ARG, decided on the host before any
 *                      device call and with every output untouched: P < 1, cap < 1, offsets that do not start at 0 or that
 *                      decrease, a path with fewer than 2 corners, a corner, resolution or max_width that is not finite (and
 *                      positive), a corner further than 2^30 cells from the origin, smoothing outside [0, 63], max_width /
 *                      resolution above 512 cells, a map side above 65534, and what mpmpc_lidar_scan_world refuses of disc
 *                      and wall lists (64 discs and 16 walls per path, squares or walls leaving the grid).
 *   mpmpc_path_build_timed   the same call, and ms [3] <- the host part (steps 1 - 4, host clock), the wall rasterisation and
 *                      the width kernel (device events), in milliseconds. */
int32_t mpmpc_path_count(int32_t n_corners, const double* corners, double path_resolution, int32_t smoothing);
int mpmpc_path_build(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                     double resolution, int32_t P, const int32_t* corner_offsets, const double* corners, const double* spec,
                     const int32_t* ispec, const int32_t* disc_offsets, const int32_t* discs, const int32_t* wall_offsets,
                     const int32_t* walls, int32_t cap, int32_t* n_wp, int32_t* status, double* x, double* y, double* psi,
                     double* kappa, double* ds_next, double* ub, double* lb, double* border, double* length);
int mpmpc_path_build_timed(int32_t device, int32_t height, int32_t width, const int8_t* data, double origin_x, double origin_y,
                           double resolution, int32_t P, const int32_t* corner_offsets, const double* corners, const double* spec,
                           const int32_t* ispec, const int32_t* disc_offsets, const int32_t* discs, const int32_t* wall_offsets,
                           const int32_t* walls, int32_t cap, int32_t* n_wp, int32_t* status, double* x, double* y, double* psi,
                           double* kappa, double* ds_next, double* ub, double* lb, double* border, double* length, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* MPMPC_H */
