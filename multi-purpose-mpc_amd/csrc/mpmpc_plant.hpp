// Plant models of the rollout, part of the one translation unit mpmpc_hip.hip (included in front of mpmpc_closed_loop.hpp; the
// step loop of mpmpc_rollout_step.hpp launches the two kernels): K3n (the measured poses K3a localises on), K3p (mpmpc_advance_kernel with the plant in
// place of ro_drive), the noise table without a handle, and the entry points mpmpc_rollout_set_plant / mpmpc_rollout_plant /
// mpmpc_plant_noise.  The law: plant_core.hpp.  The state: the sub-state pl of the handle (mpmpc_handle.hpp).
#pragma once

// what K3p takes of the plant besides mpmpc_advance_kernel's arguments
struct PlantView {
  unsigned long long seed;
  int car0;
  long long j;                    // k - step0 of the step
  const double* prm;              // [B][PL_PARAMS]
  double* act;                    // [B][2]
  const double *gx, *gy, *trig;   // per waypoint (global rows); trig [n_wp][COR_TRIG] = cos(psi), sin(psi), ...
  double *ey_max, *ey_sq;         // [B] each
  int* steps;                     // [B]
};

// K3n: the pose every running car's controller localises on (one thread per car), launched in front of K3a - which then reads
// `meas` in place of the true poses - and, with perception on, behind K0s, which senses from the true pose.  Ten Philox rounds
// twice and three multiply-adds per car; no LDS, no scratch, no libm.
__global__ __launch_bounds__(256) void mpmpc_plant_measure_kernel(int B, unsigned long long seed, int car0, long long j,
                                                                  const double* __restrict__ prm, const double* __restrict__ pose,
                                                                  const int* __restrict__ alive, double* __restrict__ meas) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B || alive[i] != 1) return;
  double n5[PL_NOISE];
  pl_noise(seed, (uint32_t)(car0 + i), j, n5);
  double m[3];
  pl_measure(prm + (long)PL_PARAMS * i, n5, pose + 3L * i, m);
  meas[3L * i] = m[0]; meas[3L * i + 1] = m[1]; meas[3L * i + 2] = m[2];
}

// K3p: K3b with a plant.  The thread layout and the route handling are mpmpc_advance_kernel's - one thread per (car, plan
// entry), the N arctangents of a car's new plan side by side - and the thread of entry 0 then draws the step's variates,
// drives the car (pl_drive) and, if it was driven, accumulates the tracking statistics from the pose the step found it at.
__global__ __launch_bounds__(256) void mpmpc_advance_plant_kernel(int B, int N, double L, double Ts, const double* __restrict__ kappa,
                                                                  const int* __restrict__ wp_id, const double* __restrict__ x0,
                                                                  const int* __restrict__ status, const double* __restrict__ z,
                                                                  double* __restrict__ cc, int* __restrict__ counter,
                                                                  int* __restrict__ alive, double* __restrict__ pose,
                                                                  double* __restrict__ s, double* __restrict__ u_last,
                                                                  const int* __restrict__ route, PlantView pv) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int i = g / N, k = g - i * N;
  if (i >= B || alive[i] != 1) return;
  const int n = 5 * N + 3;
  const int st = status[i];
  if (ro_usable(st)) ro_plan_entry(N, L, z + (long)i * n, cc + (long)i * 2 * N, k);
  if (k != 0) return;
  const long w = wp_id[i] + (int)route_view(route, i, 0, 0).first;      // (the global row; the route's length is not needed)
  double n4[4];
  pl_noise_drive(pv.seed, (uint32_t)(pv.car0 + i), pv.j, n4);
  const double px = pose[3L * i], py = pose[3L * i + 1];
  if (!pl_drive(N, L, Ts, st, cc + (long)i * 2 * N, counter + i, x0 + 3L * i, kappa[w], pv.prm + (long)PL_PARAMS * i, n4, pv.act + 2L * i,
                pose + 3L * i, s + i, u_last + 2L * i)) {
    alive[i] = -1;
    return;
  }
  pl_stats(px, py, pv.gx[w], pv.gy[w], pv.trig[w * COR_TRIG], pv.trig[w * COR_TRIG + 1], pv.ey_max + i, pv.ey_sq + i, pv.steps + i);
}

// the noise table of mpmpc_plant_noise: one thread per (step, car), out [n_steps][B][PL_NOISE]
__global__ __launch_bounds__(256) void mpmpc_plant_noise_kernel(long total, int B, unsigned long long seed, int car0, long long j0,
                                                                double* __restrict__ out) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const long t = g / B;
  const int i = (int)(g - t * B);
  double n5[PL_NOISE];
  pl_noise(seed, (uint32_t)(car0 + i), j0 + t, n5);
  for (int c = 0; c < PL_NOISE; ++c) out[PL_NOISE * g + c] = n5[c];
}

// the actuator states (act0, or zeros) and the accumulators of B cars start over, on the slot's stream
static int plant_reset(mpmpc_handle h, Slot& sl, int B, const double* act0) {
  const size_t mb = (size_t)h->cfg.max_batch;
  if (act0) HIP_TRY(hipMemcpyAsync(h->pl.act, act0, sizeof(double) * 2 * B, hipMemcpyHostToDevice, sl.stream));
  else HIP_TRY(hipMemsetAsync(h->pl.act, 0, sizeof(double) * 2 * B, sl.stream));
  HIP_TRY(hipMemsetAsync(h->pl.ey, 0, sizeof(double) * 2 * mb, sl.stream));
  HIP_TRY(hipMemsetAsync(h->pl.steps, 0, sizeof(int) * mb, sl.stream));
  h->pl.ran = false;
  return MPMPC_OK;
}

// K3n of step k on the slot's stream
static void plant_enqueue_measure(mpmpc_handle h, Slot& sl, int B, long long k) {
  hipLaunchKernelGGL(mpmpc_plant_measure_kernel, dim3((B + 255) / 256), dim3(256), 0, sl.stream, B, h->pl.seed, h->pl.car0, k - h->pl.step0,
                     h->pl.prm.get(), h->ro.pose.get(), h->ro.alive.get(), h->pl.meas.get());
}
static PlantView plant_view(mpmpc_handle h, long long k) {
  const size_t mb = (size_t)h->cfg.max_batch;
  return PlantView{h->pl.seed, h->pl.car0, k - h->pl.step0, h->pl.prm, h->pl.act, h->cor.gx, h->cor.gy, h->cor.gtrig,
                   h->pl.ey, h->pl.ey + mb, h->pl.steps};
}

// device scratch of mpmpc_plant_noise, kept between calls like the speed profile's (SpScratch)
static SpScratch g_plant_dev[SP_MAX_DEVICES];
constexpr long PL_NOISE_MAX_ROWS = 1L << 26;      // n_steps x B of one call (2.5 GiB of output)

extern "C" {

int mpmpc_rollout_set_plant(mpmpc_handle h, int32_t B, const double* params, uint64_t seed, int32_t car0, int64_t step0,
                            const double* act0) {
  if (int rc = enter(h)) return rc;
  if (!params) {      // no plant: the cars drive the controller's own model
    h->pl.B = 0;
    h->pl.ran = false;
    return MPMPC_OK;
  }
  const char* why = "";
  if (pl_check_params(B, h->cfg.max_batch, params, act0, &why)) return fail(MPMPC_E_ARG, why);
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->pl.prm) {      // (all five or none; a failure leaves "no plant", which is what was in force)
    HIP_TRY(alloc_all(Want{h->pl.prm, PL_PARAMS * mb}, Want{h->pl.act, 2 * mb}, Want{h->pl.meas, 3 * mb}, Want{h->pl.ey, 2 * mb},
                      Want{h->pl.steps, mb}));
    HIP_TRY(hipMemsetAsync(h->pl.meas, 0, sizeof(double) * 3 * mb, sl.stream));
  }
  HIP_TRY(hipMemcpyAsync(h->pl.prm, params, sizeof(double) * PL_PARAMS * B, hipMemcpyHostToDevice, sl.stream));
  if (int rc = plant_reset(h, sl, B, act0)) return rc;
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the caller's arrays have been read
  h->pl.host_scale.resize((size_t)B);
  for (int i = 0; i < B; ++i) h->pl.host_scale[(size_t)i] = params[(long)PL_PARAMS * i + PL_WHEELBASE_SCALE];
  h->dy.verified = false;      // (the dynamics' lf and stability are checked against the plant's wheelbase)
  h->pl.B = B;
  h->pl.seed = seed;
  h->pl.car0 = car0;
  h->pl.step0 = step0;
  return MPMPC_OK;
}

int mpmpc_rollout_plant(mpmpc_handle h, int32_t B, double* act, double* meas, double* ey_max, double* ey_sq, int32_t* steps) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B)) return rc;
  if (h->pl.B != B || !h->pl.ran)
    return fail(MPMPC_E_STATE, "no rollout step of B cars ran under the plant in force (mpmpc_rollout_set_plant)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch, nb = (size_t)B;
  HIP_TRY(pull(sl.stream, act, h->pl.act, 2 * nb));
  HIP_TRY(pull(sl.stream, meas, h->pl.meas, 3 * nb));
  HIP_TRY(pull(sl.stream, ey_max, h->pl.ey, nb));
  HIP_TRY(pull(sl.stream, ey_sq, h->pl.ey + mb, nb));
  HIP_TRY(pull(sl.stream, steps, h->pl.steps, nb));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

int mpmpc_plant_noise(int32_t device, uint64_t seed, int32_t car0, int32_t B, int64_t j0, int32_t n_steps, double* out) {
  if (B < 1 || n_steps < 0) return fail(MPMPC_E_ARG, "plant noise needs B >= 1 and n_steps >= 0");
  if (!out) return fail(MPMPC_E_ARG, "out must not be NULL");
  const long total = (long)B * n_steps;
  if (total > PL_NOISE_MAX_ROWS) return fail(MPMPC_E_ARG, "plant noise: more than 2^26 (step, car) rows in one call");
  if (total == 0) return MPMPC_OK;
  Layout L;
  const auto r_out = L.add<double>(PL_NOISE * (size_t)total);
  Scratch sc;
  if (int rc = scratch_acquire(g_plant_dev, device, L.bytes(), "plant", &sc)) return rc;
  hipLaunchKernelGGL(mpmpc_plant_noise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, sc.stream, total, (int)B,
                     (unsigned long long)seed, (int)car0, (long long)j0, r_out.at(sc.blk));
  HIP_TRY(hipGetLastError());
  HIP_TRY(pull(sc.stream, out, r_out.at(sc.blk), r_out.count));
  HIP_TRY(hipStreamSynchronize(sc.stream));
  return MPMPC_OK;
}

}  // extern "C"
