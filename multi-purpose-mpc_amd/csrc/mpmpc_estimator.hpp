// Pose estimator of the rollout, part of the one translation unit mpmpc_hip.hip (included behind mpmpc_delay.hpp and in front of
// mpmpc_closed_loop.hpp; the step loop of mpmpc_rollout_step.hpp launches the kernel): K3e (the estimated poses K3a - or, under
// a delay, K3d - then starts from) and the entry points mpmpc_rollout_set_estimator / mpmpc_rollout_estimator.  The law:
// estimator_core.hpp.  The state: the sub-state es of the handle (mpmpc_handle.hpp).
#pragma once
static_assert(ES_PARAMS == MPMPC_ESTIMATOR_PARAMS, "include/mpmpc.h and estimator_core.hpp disagree on the parameter block");

// what K3e takes of the estimator
struct EstView {
  unsigned long long seed;
  int car0;
  long long j;             // k - step0 of the step
  const double* prm;       // [B][ES_PARAMS]
  double *est, *cov;       // [B][3], [B][ES_COV]
  int* primed;             // [B]
  double* stats;           // [ES_STATS][ld]: err2_max, err2_sum, meas2_sum, head2_sum
  int *used, *steps;       // [B] each
  long ld;                 // max_batch
};

// K3e: one filter step of every running car (one thread per car), launched behind K3n - whose measured poses it filters - and
// in front of K3d / K3a, which then start from `est`.  z: the measured poses (plant) or the true ones; pose: the true ones
// (statistics).  The command of the last step: u [B][2] (queue == null), or - under a delay - entry assumed[i] of the car's
// register, read from memory where it lies.  No LDS.
__global__ __launch_bounds__(256) void mpmpc_estimate_kernel(int B, double L, double Ts, const double* __restrict__ z,
                                                             const double* __restrict__ pose, const int* __restrict__ alive,
                                                             const double* __restrict__ u, const double* __restrict__ queue,
                                                             const int* __restrict__ assumed, EstView ev) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B || alive[i] != 1) return;
  const double* cmd = queue ? queue + 2L * DL_MAX * i + 2 * assumed[i] : u + 2L * i;      // (assumed < DL_MAX: plan_step)
  double est[3] = {ev.est[3L * i], ev.est[3L * i + 1], ev.est[3L * i + 2]};
  double P[ES_COV], st[ES_STATS];
  for (int c = 0; c < ES_COV; ++c) P[c] = ev.cov[(long)ES_COV * i + c];
  for (int c = 0; c < ES_STATS; ++c) st[c] = ev.stats[c * ev.ld + i];
  int primed = ev.primed[i], used = ev.used[i], steps = ev.steps[i];
  const double zz[3] = {z[3L * i], z[3L * i + 1], z[3L * i + 2]};
  const double pp[3] = {pose[3L * i], pose[3L * i + 1], pose[3L * i + 2]};
  const double cc[2] = {cmd[0], cmd[1]};
  (void)es_step(ev.prm + (long)ES_PARAMS * i, ev.seed, (uint32_t)(ev.car0 + i), ev.j, L, Ts, zz, pp, cc, est, P, &primed, st, &used, &steps);
  for (int c = 0; c < 3; ++c) ev.est[3L * i + c] = est[c];
  for (int c = 0; c < ES_COV; ++c) ev.cov[(long)ES_COV * i + c] = P[c];
  for (int c = 0; c < ES_STATS; ++c) ev.stats[c * ev.ld + i] = st[c];
  ev.primed[i] = primed;
  ev.used[i] = used;
  ev.steps[i] = steps;
}

// every car un-primed (or primed with est0 / cov0) and the statistics zero, on the slot's stream
static int est_reset(mpmpc_handle h, Slot& sl, int B, const double* est0, const double* cov0) {
  const size_t mb = (size_t)h->cfg.max_batch;
  HIP_TRY(hipMemsetAsync(h->es.est, 0, sizeof(double) * 3 * mb, sl.stream));
  HIP_TRY(hipMemsetAsync(h->es.cov, 0, sizeof(double) * ES_COV * mb, sl.stream));
  HIP_TRY(hipMemsetAsync(h->es.primed, 0, sizeof(int) * mb, sl.stream));
  if (est0) {
    const std::vector<int> ones((size_t)B, 1);
    HIP_TRY(hipMemcpyAsync(h->es.est, est0, sizeof(double) * 3 * B, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemcpyAsync(h->es.cov, cov0, sizeof(double) * ES_COV * B, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemcpyAsync(h->es.primed, ones.data(), sizeof(int) * B, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));      // (`ones` has been read)
  }
  HIP_TRY(hipMemsetAsync(h->es.stats, 0, sizeof(double) * ES_STATS * mb, sl.stream));
  HIP_TRY(hipMemsetAsync(h->es.count, 0, sizeof(int) * 2 * mb, sl.stream));
  h->es.ran = false;
  return MPMPC_OK;
}

static EstView est_view(mpmpc_handle h, long long k) {
  const size_t mb = (size_t)h->cfg.max_batch;
  return EstView{h->es.seed, h->es.car0, k - h->es.step0, h->es.prm, h->es.est, h->es.cov, h->es.primed, h->es.stats,
                 h->es.count, h->es.count + mb, (long)mb};
}

extern "C" {

int mpmpc_rollout_set_estimator(mpmpc_handle h, int32_t B, const double* params, uint64_t seed, int32_t car0, int64_t step0,
                                const double* est0, const double* cov0) {
  if (int rc = enter(h)) return rc;
  if (!params) {      // no estimator: the controller localises on the measured pose (plant) or the true one
    h->es.B = 0;
    h->es.ran = false;
    return MPMPC_OK;
  }
  const char* why = "";
  if (es_check_params(B, h->cfg.max_batch, params, est0, cov0, &why)) return fail(MPMPC_E_ARG, why);
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t mb = (size_t)h->cfg.max_batch;
  if (!h->es.prm)      // (all six or none; a failure leaves "no estimator", which is what was in force)
    HIP_TRY(alloc_all(Want{h->es.prm, ES_PARAMS * mb}, Want{h->es.est, 3 * mb}, Want{h->es.cov, ES_COV * mb}, Want{h->es.primed, mb},
                      Want{h->es.stats, ES_STATS * mb}, Want{h->es.count, 2 * mb}));
  HIP_TRY(hipMemcpyAsync(h->es.prm, params, sizeof(double) * ES_PARAMS * B, hipMemcpyHostToDevice, sl.stream));
  if (int rc = est_reset(h, sl, B, est0, cov0)) return rc;
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the caller's arrays have been read
  h->es.B = B;
  h->es.seed = seed;
  h->es.car0 = car0;
  h->es.step0 = step0;
  return MPMPC_OK;
}

int mpmpc_rollout_estimator(mpmpc_handle h, int32_t B, double* est, double* cov, double* err2_max, double* err2_sum, double* meas2_sum,
                            double* head2_sum, int32_t* used, int32_t* steps) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B)) return rc;
  if (h->es.B != B || !h->es.ran)
    return fail(MPMPC_E_STATE, "no rollout step of B cars ran under the estimator in force (mpmpc_rollout_set_estimator)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const size_t mb = (size_t)h->cfg.max_batch, nb = (size_t)B;
  HIP_TRY(pull(sl.stream, est, h->es.est, 3 * nb));
  HIP_TRY(pull(sl.stream, cov, h->es.cov, ES_COV * nb));
  HIP_TRY(pull(sl.stream, err2_max, h->es.stats, nb));
  HIP_TRY(pull(sl.stream, err2_sum, h->es.stats + mb, nb));
  HIP_TRY(pull(sl.stream, meas2_sum, h->es.stats + 2 * mb, nb));
  HIP_TRY(pull(sl.stream, head2_sum, h->es.stats + 3 * mb, nb));
  HIP_TRY(pull(sl.stream, used, h->es.count, nb));
  HIP_TRY(pull(sl.stream, steps, h->es.count + mb, nb));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

}  // extern "C"
