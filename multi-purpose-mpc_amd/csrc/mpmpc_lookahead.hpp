// Lookahead of the rollout, part of the one translation unit mpmpc_hip.hip (included behind mpmpc_closed_loop.hpp, which holds
// K0h and the LEAD instantiations of K0c): the setting, the layout of K0h's tables for the movers in force, K0h's launch and
// the getter.  The law: lookahead_core.hpp.  The state: the sub-state look of the handle (mpmpc_handle.hpp).
#pragma once

// May steps of B cars run with the lookahead that is set?  *active: they look ahead (the fleet has movers) - then look.car and
// look.tab fit the per-car settings in force when this returns.
static int look_check_step(mpmpc_handle h, int B, int movers, bool* active) {
  LookState& lk = h->look;
  *active = false;
  if (lk.gen != h->cor.base_gen)
    return fail(MPMPC_E_STATE, "map, path, routes or geometry changed since mpmpc_rollout_set_lookahead");
  if (movers <= 0) return MPMPC_OK;
  *active = true;
  if (lk.laid) return MPMPC_OK;
  const int N = h->cfg.N;
  if (look_table_bytes(movers, N) > LOOK_TABLE_BUDGET) return fail(MPMPC_E_ARG, LOOK_OVER_BUDGET);      // (the setters refuse it first)
  const size_t mb = (size_t)h->cfg.max_batch, want = (size_t)movers * N * 3;
  if (!lk.lead) HIP_TRY(alloc_all(Want{lk.lead, mb * N}, Want{lk.car, 2 * (mb + 1)}));      // (both or neither)
  if (want > lk.tab.count()) HIP_TRY(lk.tab.alloc(want));
  lk.host_car.assign(2 * ((size_t)B + 1), 0);
  for (int b = 0; b <= B; ++b) {
    lk.host_car[2 * (size_t)b] = h->obs.mv_off[b];
    lk.host_car[2 * (size_t)b + 1] = b < B && h->obs.st_B > 0 ? h->obs.st_off[b + 1] - h->obs.st_off[b] : 0;
  }
  HIP_TRY(hipMemcpyAsync(lk.car, lk.host_car.data(), sizeof(int) * lk.host_car.size(), hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  lk.laid = true;
  return MPMPC_OK;
}

// K0h of rollout step k on the slot's stream (behind K3a, in front of K0c)
static void look_enqueue_step(mpmpc_handle h, Slot& sl, int B, long long k, int movers, const MapView& mv, const PathGeom& pg,
                              const MoverPath& mp, const int* route) {
  const double* mv_p = (const double*)h->obs.mv_block.get();
  const int* mv_i = (const int*)(mv_p + (size_t)MOV_PARAMS * movers);
  hipLaunchKernelGGL(mpmpc_mover_horizon_kernel, dim3(B), dim3(64), 0, sl.stream, h->cfg.N, k, h->obs.mv_step0, h->ro.Ts, h->look.max_lead, mv,
                     pg, mp, h->look.seg.get(), h->io.wp_id, movers, mv_i, mv_i + movers, mv_p, h->look.car.get(), h->look.lead.get(),
                     h->look.tab.get(), route);
}

extern "C" {

int mpmpc_rollout_set_lookahead(mpmpc_handle h, int32_t n_wp, const double* seg_time, int32_t max_lead) {
  if (int rc = enter(h)) return rc;
  LookState& lk = h->look;
  if (!seg_time) {      // off
    lk.max_lead = 0;
    lk.ran_B = 0;
    return MPMPC_OK;
  }
  const char* why = "";
  if (look_check_setting(n_wp, h->tab.n_wp, seg_time, max_lead, &why)) return fail(MPMPC_E_ARG, why);
  if (h->cfg.N > 255) return fail(MPMPC_E_ARG, "lookahead needs N <= 255");
  if (h->obs.mv_B > 0 && look_table_bytes(h->obs.mv_n, h->cfg.N) > LOOK_TABLE_BUDGET) return fail(MPMPC_E_ARG, LOOK_OVER_BUDGET);
  HIP_TRY(hipSetDevice(h->cfg.device));
  lk.max_lead = 0;      // a failure below leaves "off"
  lk.ran_B = 0;
  if (int rc = upload_table(h, lk.seg, seg_time, (size_t)n_wp)) return rc;
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  lk.max_lead = max_lead;
  lk.gen = h->cor.base_gen;
  return MPMPC_OK;
}

int mpmpc_rollout_lookahead(mpmpc_handle h, int32_t B, int32_t* lead_out, int32_t* discs_out) {
  if (int rc = enter(h, lead_out != nullptr)) return rc;
  const LookState& lk = h->look;
  if (B < 1 || lk.ran_B != B || !h->ro.valid)
    return fail(MPMPC_E_STATE, "the last rollout step did not look ahead for B cars (mpmpc_rollout_set_lookahead with movers in the fleet), "
                               "or a per-car setting, the lookahead or the rollout was set anew since");
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t N = (size_t)h->cfg.N;
  HIP_TRY(hipMemcpyAsync(lead_out, lk.lead, sizeof(int) * (size_t)B * N, hipMemcpyDeviceToHost, sl.stream));
  if (discs_out) HIP_TRY(hipMemcpyAsync(discs_out, lk.tab, sizeof(int) * 3 * N * (size_t)lk.ran_n, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

}  // extern "C"
