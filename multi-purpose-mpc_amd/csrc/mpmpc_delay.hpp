// Actuation delay of the rollout and its compensation, part of the one translation unit mpmpc_hip.hip (included behind
// mpmpc_plant.hpp and in front of mpmpc_closed_loop.hpp; the step loop of mpmpc_rollout_step.hpp launches the two kernels): K3d
// (the predicted pose and s K3a localises on), K3q (mpmpc_advance_kernel / mpmpc_advance_plant_kernel with the command register
// between the plan and the wheels), and the entry points mpmpc_rollout_set_delay / mpmpc_rollout_delay.  The law:
// delay_core.hpp.  The state: the sub-state dl of the handle (mpmpc_handle.hpp).
#pragma once
static_assert(DL_MAX == MPMPC_DELAY_MAX, "include/mpmpc.h and delay_core.hpp disagree on the register's length");

// what K3q takes of the delay besides mpmpc_advance_plant_kernel's arguments
struct DelayView {
  const int* delay;       // [B]
  double* queue;          // [B][DL_MAX][2]
  const double* now;      // [B][3]: x0[0], x0[1] and kappa of the waypoint the car IS at (K3d)
  const int* now_wp;      // [B]: that waypoint's global row
};

// K3d: where every running car will be when the command computed now takes effect (one thread per car), launched behind K3n -
// whose measured poses it then starts from - and in front of K3a, which reads pred_pose / pred_s in place of the poses and s.
// The register is read from memory where it is used (a private array indexed by c would go to scratch).  No LDS.
__global__ __launch_bounds__(256) void mpmpc_delay_predict_kernel(int B, int n_wp, double L, double Ts, const double* __restrict__ cum,
                                                                  const double* __restrict__ gx, const double* __restrict__ gy,
                                                                  const double* __restrict__ gpsi, const double* __restrict__ kappa,
                                                                  const double* __restrict__ s, const double* __restrict__ pose,
                                                                  const int* __restrict__ alive, const int* __restrict__ assumed,
                                                                  const double* __restrict__ queue, double* __restrict__ pred_pose,
                                                                  double* __restrict__ pred_s, double* __restrict__ now,
                                                                  int* __restrict__ now_wp, const int* __restrict__ route) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B || alive[i] != 1) return;
  long first = 0;
  if (route) {      // route fleets: the car's slice of the tables and its route's length, as K3a takes them
    const RouteView v = route_header(route, i);
    first = v.first;
    cum += first; gx += first; gy += first; gpsi += first; kappa += first;
    n_wp = v.n();
  }
  (void)dl_predict(cum, gx, gy, gpsi, kappa, n_wp, first, assumed[i], queue + 2L * DL_MAX * i, L, Ts, pose + 3L * i, s[i], pred_pose + 3L * i,
                   pred_s + i, now + 3L * i, now_wp + i);
}

// K3q: K3b (PLANT = false) or K3p (true) with the register.  Their thread layout - one thread per (car, plan entry), the N
// arctangents of a car's new plan side by side - and the thread of entry 0 then draws the step's variates (PLANT), drives the car
// (dl_drive: the command goes into the register, what leaves it reaches the wheels) and, if it was driven under a plant,
// accumulates the tracking statistics against the waypoint the car is at.
template <bool PLANT>
__global__ __launch_bounds__(256) void mpmpc_advance_delay_kernel(int B, int N, double L, double Ts, const int* __restrict__ status,
                                                                  const double* __restrict__ z, double* __restrict__ cc,
                                                                  int* __restrict__ counter, int* __restrict__ alive,
                                                                  double* __restrict__ pose, double* __restrict__ s,
                                                                  double* __restrict__ u_last, DelayView dv, PlantView pv) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int i = g / N, k = g - i * N;
  if (i >= B || alive[i] != 1) return;
  const int n = 5 * N + 3;
  const int st = status[i];
  if (ro_usable(st)) ro_plan_entry(N, L, z + (long)i * n, cc + (long)i * 2 * N, k);
  if (k != 0) return;
  double n4[4] = {0.0, 0.0, 0.0, 0.0};
  if (PLANT) pl_noise_drive(pv.seed, (uint32_t)(pv.car0 + i), pv.j, n4);
  const double px = pose[3L * i], py = pose[3L * i + 1];
  if (!dl_drive<PLANT>(N, L, Ts, st, cc + (long)i * 2 * N, counter + i, dv.now + 3L * i, dv.delay[i], dv.queue + 2L * DL_MAX * i,
                       PLANT ? pv.prm + (long)PL_PARAMS * i : nullptr, n4, PLANT ? pv.act + 2L * i : nullptr, pose + 3L * i, s + i,
                       u_last + 2L * i)) {
    alive[i] = -1;
    return;
  }
  if (PLANT) {
    const long w = dv.now_wp[i];
    pl_stats(px, py, pv.gx[w], pv.gy[w], pv.trig[w * COR_TRIG], pv.trig[w * COR_TRIG + 1], pv.ey_max + i, pv.ey_sq + i, pv.steps + i);
  }
}

// the registers of B cars start over (queue0, or zeros: the car stands for d steps), on the slot's stream
static int delay_reset(mpmpc_handle h, Slot& sl, int B, const double* queue0) {
  if (queue0) HIP_TRY(hipMemcpyAsync(h->dl.queue, queue0, sizeof(double) * 2 * DL_MAX * B, hipMemcpyHostToDevice, sl.stream));
  else HIP_TRY(hipMemsetAsync(h->dl.queue, 0, sizeof(double) * 2 * DL_MAX * B, sl.stream));
  h->dl.ran = false;
  return MPMPC_OK;
}

static DelayView delay_view(mpmpc_handle h) { return DelayView{h->dl.delay, h->dl.queue, h->dl.now, h->dl.now_wp}; }

extern "C" {

int mpmpc_rollout_set_delay(mpmpc_handle h, int32_t B, const int32_t* delay, const int32_t* assumed, const double* queue0) {
  if (int rc = enter(h)) return rc;
  if (!delay) {      // no delay: a command reaches the wheels in the step that issues it
    h->dl.B = 0;
    h->dl.ran = false;
    return MPMPC_OK;
  }
  const char* why = "";
  if (dl_check(B, h->cfg.max_batch, delay, assumed, queue0, &why)) return fail(MPMPC_E_ARG, why);
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->dl.delay) {      // (all seven or none; a failure leaves "no delay", which is what was in force)
    HIP_TRY(alloc_all(Want{h->dl.delay, mb}, Want{h->dl.assumed, mb}, Want{h->dl.queue, 2 * DL_MAX * mb}, Want{h->dl.pred_pose, 3 * mb},
                      Want{h->dl.pred_s, mb}, Want{h->dl.now, 3 * mb}, Want{h->dl.now_wp, mb}));
    HIP_TRY(hipMemsetAsync(h->dl.pred_pose, 0, sizeof(double) * 3 * mb, sl.stream));
    HIP_TRY(hipMemsetAsync(h->dl.pred_s, 0, sizeof(double) * mb, sl.stream));
    HIP_TRY(hipMemsetAsync(h->dl.now, 0, sizeof(double) * 3 * mb, sl.stream));
    HIP_TRY(hipMemsetAsync(h->dl.now_wp, 0, sizeof(int) * mb, sl.stream));
  }
  HIP_TRY(hipMemcpyAsync(h->dl.delay, delay, sizeof(int) * B, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipMemcpyAsync(h->dl.assumed, assumed ? assumed : delay, sizeof(int) * B, hipMemcpyHostToDevice, sl.stream));
  if (int rc = delay_reset(h, sl, B, queue0)) return rc;
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the caller's arrays have been read
  h->dl.B = B;
  h->dl.max_assumed = 0;      // (kept on the host: a step under an estimator refuses c = DL_MAX)
  for (int i = 0; i < B; ++i) {
    const int c = (assumed ? assumed : delay)[i];
    if (c > h->dl.max_assumed) h->dl.max_assumed = c;
  }
  return MPMPC_OK;
}

int mpmpc_rollout_delay(mpmpc_handle h, int32_t B, double* queue, double* pred_pose, double* pred_s, double* now) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B)) return rc;
  if (h->dl.B != B || !h->dl.ran)
    return fail(MPMPC_E_STATE, "no rollout step of B cars ran under the delay in force (mpmpc_rollout_set_delay)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t nb = (size_t)B;
  HIP_TRY(pull(sl.stream, queue, h->dl.queue, 2 * DL_MAX * nb));
  HIP_TRY(pull(sl.stream, pred_pose, h->dl.pred_pose, 3 * nb));
  HIP_TRY(pull(sl.stream, pred_s, h->dl.pred_s, nb));
  HIP_TRY(pull(sl.stream, now, h->dl.now, 3 * nb));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

}  // extern "C"
