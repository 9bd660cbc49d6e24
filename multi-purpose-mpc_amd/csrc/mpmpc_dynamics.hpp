// Dynamic single-track plant of the rollout, part of the one translation unit mpmpc_hip.hip (included behind mpmpc_delay.hpp and
// in front of mpmpc_closed_loop.hpp; the step loop of mpmpc_rollout_step.hpp launches the kernel): K3y (mpmpc_advance_plant_kernel
// / mpmpc_advance_delay_kernel<true> with the dynamic car in place of the kinematic one), the open-loop drive without a handle,
// and the entry points mpmpc_rollout_set_dynamics / mpmpc_rollout_dynamics / mpmpc_dynamics_drive.  The law: dynamics_core.hpp.
// The state: the sub-state dy of the handle (mpmpc_handle.hpp).
#pragma once

// what K3y takes of the dynamics besides K3p's / K3q's arguments
struct DynView {
  const double* prm;      // [B][DY_PARAMS]
  double* state;          // [B][DY_STATE]
  int* counts;            // [DY_COUNTS][stride]: dyn_steps, sat_front, sat_rear
  double* peaks;          // [DY_PEAKS][stride]: slip_f, slip_r, alat
  long stride;
};

// a car's accumulators, read from and written to memory where they are used (no private array)
__device__ inline DyAcc dyn_load(const DynView& y, int i) {
  return DyAcc{y.counts[i], y.counts[y.stride + i], y.counts[2 * y.stride + i], y.peaks[i], y.peaks[y.stride + i], y.peaks[2 * y.stride + i]};
}
__device__ inline void dyn_store(const DynView& y, int i, const DyAcc& a) {
  y.counts[i] = a.dyn_steps; y.counts[y.stride + i] = a.sat_front; y.counts[2 * y.stride + i] = a.sat_rear;
  y.peaks[i] = a.slip_f; y.peaks[y.stride + i] = a.slip_r; y.peaks[2 * y.stride + i] = a.alat;
}

// K3y: K3p (DELAY = false) or K3q<true> (true) with the dynamic plant.  Their thread layout - one thread per (car, plan entry),
// the N arctangents of a car's new plan side by side - and the thread of entry 0 then draws the step's variates, drives the car
// (dy_drive / dy_drive_delay: n serial sub-steps of FP64 atan2 / sin / cos) and, if it was driven, accumulates the plant's
// tracking statistics as K3p / K3q do.  No LDS, no scratch: the state, the parameters and the accumulators are scalars read from
// memory where they are used.
template <bool DELAY>
__global__ __launch_bounds__(256) void mpmpc_advance_dynamics_kernel(int B, int N, double L, double Ts, const double* __restrict__ kappa,
                                                                     const int* __restrict__ wp_id, const double* __restrict__ x0,
                                                                     const int* __restrict__ status, const double* __restrict__ z,
                                                                     double* __restrict__ cc, int* __restrict__ counter,
                                                                     int* __restrict__ alive, double* __restrict__ pose,
                                                                     double* __restrict__ s, double* __restrict__ u_last,
                                                                     const int* __restrict__ route, DelayView dv, PlantView pv, DynView yv) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int i = g / N, k = g - i * N;
  if (i >= B || alive[i] != 1) return;
  const int n = 5 * N + 3;
  const int st = status[i];
  if (ro_usable(st)) ro_plan_entry(N, L, z + (long)i * n, cc + (long)i * 2 * N, k);
  if (k != 0) return;
  double n4[4];
  pl_noise_drive(pv.seed, (uint32_t)(pv.car0 + i), pv.j, n4);
  const double px = pose[3L * i], py = pose[3L * i + 1];
  DyAcc acc = dyn_load(yv, i);
  long w;
  bool driven;
  if (DELAY) {
    w = dv.now_wp[i];
    driven = dy_drive_delay(N, L, Ts, st, cc + (long)i * 2 * N, counter + i, dv.now + 3L * i, dv.delay[i], dv.queue + 2L * DL_MAX * i,
                            pv.prm + (long)PL_PARAMS * i, n4, yv.prm + (long)DY_PARAMS * i, pv.act + 2L * i, yv.state + (long)DY_STATE * i,
                            pose + 3L * i, s + i, u_last + 2L * i, &acc);
  } else {
    w = wp_id[i] + (int)route_view(route, i, 0, 0).first;      // (the global row; the route's length is not needed)
    driven = dy_drive(N, L, Ts, st, cc + (long)i * 2 * N, counter + i, x0 + 3L * i, kappa[w], pv.prm + (long)PL_PARAMS * i, n4,
                      yv.prm + (long)DY_PARAMS * i, pv.act + 2L * i, yv.state + (long)DY_STATE * i, pose + 3L * i, s + i, u_last + 2L * i, &acc);
  }
  if (!driven) {
    alive[i] = -1;
    return;
  }
  dyn_store(yv, i, acc);
  pl_stats(px, py, pv.gx[w], pv.gy[w], pv.trig[w * COR_TRIG], pv.trig[w * COR_TRIG + 1], pv.ey_max + i, pv.ey_sq + i, pv.steps + i);
}

// the open-loop drive of mpmpc_dynamics_drive: one thread per car, n_steps commands (v_act, d_act) one after the other through
// dy_move; trace (may be null) [n_steps][B][3] takes the pose after every step
__global__ __launch_bounds__(256) void mpmpc_dynamics_drive_kernel(int B, int n_steps, double Lp, double Ts, const double* __restrict__ prm,
                                                                   const double* __restrict__ cmds, double* __restrict__ state,
                                                                   double* __restrict__ pose, int* __restrict__ counts,
                                                                   double* __restrict__ peaks, double* __restrict__ trace) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const DynView yv{prm, state, counts, peaks, (long)B};
  DyAcc acc = dyn_load(yv, i);
  for (int t = 0; t < n_steps; ++t) {
    const double* c = cmds + 2 * ((long)t * B + i);
    dy_move(Lp, Ts, c[0], c[1], prm + (long)DY_PARAMS * i, state + (long)DY_STATE * i, pose + 3L * i, &acc);
    if (trace) {
      double* o = trace + 3 * ((long)t * B + i);
      o[0] = pose[3L * i]; o[1] = pose[3L * i + 1]; o[2] = pose[3L * i + 2];
    }
  }
  dyn_store(yv, i, acc);
}

// the states (state0, or zeros) and the accumulators of B cars start over, on the slot's stream
static int dynamics_reset(mpmpc_handle h, Slot& sl, int B, const double* state0) {
  const size_t mb = (size_t)h->cfg.max_batch;
  if (state0) HIP_TRY(hipMemcpyAsync(h->dy.state, state0, sizeof(double) * DY_STATE * B, hipMemcpyHostToDevice, sl.stream));
  else HIP_TRY(hipMemsetAsync(h->dy.state, 0, sizeof(double) * DY_STATE * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->dy.counts, 0, sizeof(int) * DY_COUNTS * mb, sl.stream));
  HIP_TRY(hipMemsetAsync(h->dy.peaks, 0, sizeof(double) * DY_PEAKS * mb, sl.stream));
  h->dy.ran = false;
  return MPMPC_OK;
}

static DynView dynamics_view(mpmpc_handle h) {
  return DynView{h->dy.prm, h->dy.state, h->dy.counts, h->dy.peaks, (long)h->cfg.max_batch};
}

// What plan_step asks of a step under dynamics, before any kernel is launched: a plant in force for the same cars, and - once
// per (setting, plant, Ts) - every car's lf against its plant wheelbase and the sub-step's stability.
static int dynamics_check_step(mpmpc_handle h, int B) {
  if (h->dy.B != B) return fail(MPMPC_E_STATE, "the dynamics were set for another number of cars (mpmpc_rollout_set_dynamics)");
  if (h->pl.B != B) return fail(MPMPC_E_STATE, "dynamics need a plant in force for the same cars (mpmpc_rollout_set_plant; the identity will do)");
  if (h->dy.verified) return MPMPC_OK;
  const char* why = "";
  if (dy_check_run(B, h->cfg.wheelbase, h->pl.host_scale.data(), h->ro.Ts, h->dy.host_prm.data(), &why)) return fail(MPMPC_E_STATE, why);
  h->dy.verified = true;
  return MPMPC_OK;
}

// device scratch of mpmpc_dynamics_drive, kept between calls like the plant noise's
static SpScratch g_dynamics_dev[SP_MAX_DEVICES];
constexpr long DY_DRIVE_MAX_ROWS = 1L << 26;      // n_steps x B of one call

extern "C" {

int mpmpc_rollout_set_dynamics(mpmpc_handle h, int32_t B, const double* params, const double* state0) {
  if (int rc = enter(h)) return rc;
  if (!params) {      // no dynamics: the plant (if any) drives the kinematic car
    h->dy.B = 0;
    h->dy.ran = false;
    return MPMPC_OK;
  }
  const char* why = "";
  if (dy_check_params(B, h->cfg.max_batch, params, state0, &why)) return fail(MPMPC_E_ARG, why);
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->dy.prm)      // (all four or none; a failure leaves "no dynamics", which is what was in force)
    HIP_TRY(alloc_all(Want{h->dy.prm, DY_PARAMS * mb}, Want{h->dy.state, DY_STATE * mb}, Want{h->dy.counts, DY_COUNTS * mb},
                      Want{h->dy.peaks, DY_PEAKS * mb}));
  HIP_TRY(hipMemcpyAsync(h->dy.prm, params, sizeof(double) * DY_PARAMS * B, hipMemcpyHostToDevice, sl.stream));
  if (int rc = dynamics_reset(h, sl, B, state0)) return rc;
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the caller's arrays have been read
  h->dy.host_prm.assign(params, params + (size_t)DY_PARAMS * B);      // (the step's stability check needs Ts and the plant's wheelbase)
  h->dy.verified = false;
  h->dy.B = B;
  return MPMPC_OK;
}

int mpmpc_rollout_dynamics(mpmpc_handle h, int32_t B, double* state, int32_t* counts, double* peaks) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B)) return rc;
  if (h->dy.B != B || !h->dy.ran)
    return fail(MPMPC_E_STATE, "no rollout step of B cars ran under the dynamics in force (mpmpc_rollout_set_dynamics)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch, nb = (size_t)B;
  HIP_TRY(pull(sl.stream, state, h->dy.state, DY_STATE * nb));
  for (size_t c = 0; c < (size_t)DY_COUNTS; ++c)
    HIP_TRY(pull(sl.stream, counts ? counts + c * nb : nullptr, h->dy.counts + c * mb, nb));
  for (size_t c = 0; c < (size_t)DY_PEAKS; ++c)
    HIP_TRY(pull(sl.stream, peaks ? peaks + c * nb : nullptr, h->dy.peaks + c * mb, nb));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

int mpmpc_dynamics_drive(int32_t device, int32_t B, int32_t n_steps, double L, double Ts, const double* params, const double* state0,
                         const double* pose0, const double* cmds, double* state, double* pose, int32_t* counts, double* peaks,
                         double* trace) {
  if (B < 1 || n_steps < 0) return fail(MPMPC_E_ARG, "dynamics drive needs B >= 1 and n_steps >= 0");
  if (!params || !pose0 || (n_steps > 0 && !cmds)) return fail(MPMPC_E_ARG, "params, pose0 and cmds must not be NULL");
  if (!(L > 0) || !pl_finite(L) || !(Ts > 0) || !pl_finite(Ts)) return fail(MPMPC_E_ARG, "dynamics drive needs finite L > 0 and Ts > 0");
  const long total = (long)B * n_steps;
  if (total > DY_DRIVE_MAX_ROWS) return fail(MPMPC_E_ARG, "dynamics drive: more than 2^26 (step, car) rows in one call");
  const char* why = "";
  if (dy_check_params(B, B, params, state0, &why)) return fail(MPMPC_E_ARG, why);
  if (dy_check_run(B, L, nullptr, Ts, params, &why)) return fail(MPMPC_E_ARG, why);
  for (long i = 0; i < 3L * B; ++i)
    if (!pl_finite(pose0[i])) return fail(MPMPC_E_ARG, "dynamics drive: pose0 must be finite");
  for (long i = 0; i < 2 * total; ++i)
    if (!pl_finite(cmds[i])) return fail(MPMPC_E_ARG, "dynamics drive: cmds must be finite");
  const size_t nb = (size_t)B;
  Layout lay;
  const auto r_prm = lay.add<double>(DY_PARAMS * nb), r_cmd = lay.add<double>(2 * (size_t)total), r_state = lay.add<double>(DY_STATE * nb),
             r_pose = lay.add<double>(3 * nb), r_peaks = lay.add<double>(DY_PEAKS * nb), r_trace = lay.add<double>(trace ? 3 * (size_t)total : 0);
  const auto r_counts = lay.add<int>(DY_COUNTS * nb);
  Scratch sc;
  if (int rc = scratch_acquire(g_dynamics_dev, device, lay.bytes(), "dynamics", &sc)) return rc;
  HIP_TRY(hipMemcpyAsync(r_prm.at(sc.blk), params, r_prm.bytes(), hipMemcpyHostToDevice, sc.stream));
  if (total > 0) HIP_TRY(hipMemcpyAsync(r_cmd.at(sc.blk), cmds, r_cmd.bytes(), hipMemcpyHostToDevice, sc.stream));
  if (state0) HIP_TRY(hipMemcpyAsync(r_state.at(sc.blk), state0, r_state.bytes(), hipMemcpyHostToDevice, sc.stream));
  else HIP_TRY(hipMemsetAsync(r_state.at(sc.blk), 0, r_state.bytes(), sc.stream));
  HIP_TRY(hipMemcpyAsync(r_pose.at(sc.blk), pose0, r_pose.bytes(), hipMemcpyHostToDevice, sc.stream));
  HIP_TRY(hipMemsetAsync(r_peaks.at(sc.blk), 0, r_peaks.bytes(), sc.stream));
  HIP_TRY(hipMemsetAsync(r_counts.at(sc.blk), 0, r_counts.bytes(), sc.stream));
  hipLaunchKernelGGL(mpmpc_dynamics_drive_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, sc.stream, (int)B, (int)n_steps, L, Ts,
                     r_prm.at(sc.blk), r_cmd.at(sc.blk), r_state.at(sc.blk), r_pose.at(sc.blk), r_counts.at(sc.blk), r_peaks.at(sc.blk),
                     trace ? r_trace.at(sc.blk) : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(sc.stream, state, r_state.at(sc.blk), r_state.count));
  HIP_TRY(pull(sc.stream, pose, r_pose.at(sc.blk), r_pose.count));
  HIP_TRY(pull(sc.stream, counts, r_counts.at(sc.blk), r_counts.count));
  HIP_TRY(pull(sc.stream, peaks, r_peaks.at(sc.blk), r_peaks.count));
  HIP_TRY(pull(sc.stream, trace, r_trace.at(sc.blk), r_trace.count));
  HIP_TRY(hipStreamSynchronize(sc.stream));
  return MPMPC_OK;
}

}  // extern "C"
