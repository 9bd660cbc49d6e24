// Lookahead of the rollout, part of the one translation unit mpmpc_hip.hip (included behind mpmpc_closed_loop.hpp, which holds
// K0h and the LEAD instantiations of K0c): the setting, the layout of K0h's tables for the movers in force, K0h's launch and
// the getter (the step loop that calls look_* / tlk_*: mpmpc_rollout_step.hpp).  The law: lookahead_core.hpp.  The state: the sub-state look of the handle (mpmpc_handle.hpp).
// Lookahead for traffic (the law: traffic_lookahead_core.hpp; the state: the sub-state tlk): the flag, the memory of the plan
// tracks and of K0t's / K0ht's tables, the launches of K0ht and K3t and the two getters.
#pragma once

// The tracks and tables of a step of B cars that anticipates traffic (S slots per car): allocated on first use, who and tz grow.
static int tlk_lay_out(mpmpc_handle h, int B, int S) {
  TlkState& tk = h->tlk;
  const size_t mb = (size_t)h->cfg.max_batch, N = (size_t)h->cfg.N;
  if (tlk_table_bytes(B, S, (int)N) > LOOK_TABLE_BUDGET) return fail(MPMPC_E_ARG, TLK_OVER_BUDGET);      // (the setters refuse it first)
  if (!tk.valid) {      // (all three or none)
    HIP_TRY(alloc_all(Want{tk.valid, mb}, Want{tk.cells, 2 * (N + 1) * mb}, Want{tk.tm, (N + 1) * mb}));
    tk.tracks_live = false;
  }
  if ((size_t)B * S > tk.who.count()) HIP_TRY(tk.who.alloc((size_t)B * S));
  if ((size_t)B * S * N * 3 > tk.tz.count()) HIP_TRY(tk.tz.alloc((size_t)B * S * N * 3));
  return MPMPC_OK;
}

// May steps of B cars run with the lookahead that is set?  *active: they look ahead (the fleet has movers, or the step
// anticipates traffic: *ahead_traffic) - then look.car and look.tab, and the tracks and tables of tlk, fit the per-car settings
// in force when this returns.
static int look_check_step(mpmpc_handle h, int B, int movers, bool traffic, bool* active, bool* ahead_traffic) {
  LookState& lk = h->look;
  *active = *ahead_traffic = false;
  if (lk.gen != h->cor.base_gen)
    return fail(MPMPC_E_STATE, "map, path, routes or geometry changed since mpmpc_rollout_set_lookahead");
  const bool tlk = h->tlk.on && traffic;
  if (movers <= 0 && !tlk) return MPMPC_OK;
  if (tlk) {
    if (int rc = tlk_lay_out(h, B, h->obs.tr_S)) return rc;
  }
  *active = true;
  *ahead_traffic = tlk;
  if (lk.laid) return MPMPC_OK;
  const int N = h->cfg.N;
  if (look_table_bytes(movers, N) > LOOK_TABLE_BUDGET) return fail(MPMPC_E_ARG, LOOK_OVER_BUDGET);      // (the setters refuse it first)
  const size_t mb = (size_t)h->cfg.max_batch, want = (size_t)movers * N * 3;
  if (!lk.lead) HIP_TRY(alloc_all(Want{lk.lead, mb * N}, Want{lk.car, 2 * (mb + 1)}));      // (both or neither)
  if (want > lk.tab.count()) HIP_TRY(lk.tab.alloc(want));
  lk.host_car.assign(2 * ((size_t)B + 1), 0);
  for (int b = 0; b <= B; ++b) {
    lk.host_car[2 * (size_t)b] = movers > 0 ? h->obs.mv_off[b] : 0;
    lk.host_car[2 * (size_t)b + 1] = b < B && h->obs.st_B > 0 ? h->obs.st_off[b + 1] - h->obs.st_off[b] : 0;
  }
  HIP_TRY(hipMemcpyAsync(lk.car, lk.host_car.data(), sizeof(int) * lk.host_car.size(), hipMemcpyHostToDevice, h->last().stream));
  HIP_TRY(hipStreamSynchronize(h->last().stream));
  lk.laid = true;
  return MPMPC_OK;
}

// K0h of rollout step k on the slot's stream (behind K3a, in front of K0c)
static void look_enqueue_step(mpmpc_handle h, Slot& sl, int B, long long k, const MapView& mv, const PathGeom& pg, const MoverPath& mp,
                              const int* route) {
  const MoverView m = h->obs.mover_view();
  hipLaunchKernelGGL(mpmpc_mover_horizon_kernel, dim3(B), dim3(64), 0, sl.stream, h->cfg.N, k, m.step0, h->ro.Ts, h->look.max_lead, mv, pg, mp,
                     h->look.seg.get(), h->io.wp_id, m.n, m.kind, m.radius, m.prm, h->look.car.get(), h->look.lead.get(), h->look.tab.get(),
                     route);
}

// K0ht of a rollout step on the slot's stream (behind K0h, in front of K0c): the true lists, K0t's who, K0h's leads, the tracks
static void tlk_enqueue_horizon(mpmpc_handle h, Slot& sl, int B, const MapView& mv) {
  hipLaunchKernelGGL(mpmpc_traffic_horizon_kernel, dim3(B), dim3(64), 0, sl.stream, h->cfg.N, h->obs.tr_S, h->ro.Ts, mv, h->obs.obst_off.get(),
                     h->obs.obst_discs.get(), h->tlk.who.get(), h->look.lead.get(), h->tlk.valid.get(), h->tlk.cells.get(), h->tlk.tm.get(),
                     h->tlk.tz.get());
}

// K3t of a rollout step on the slot's stream (behind K3b): the step's plans become the tracks
static void tlk_enqueue_tracks(mpmpc_handle h, Slot& sl, int B, const MapView& mv, const int* route) {
  hipLaunchKernelGGL(mpmpc_plan_track_kernel, dim3(B), dim3(64), 0, sl.stream, B, h->cfg.N, mv, h->cor.gx.get(), h->cor.gy.get(),
                     h->cor.gtrig.get(), h->tab.n_wp, h->cfg.circular ? 1 : 0, h->io.wp_id, h->ro.alive.get(), sl.status, sl.z, route,
                     h->tlk.valid.get(), h->tlk.cells.get(), h->tlk.tm.get());
}

extern "C" {

int mpmpc_rollout_set_lookahead_traffic(mpmpc_handle h, int32_t enable) {
  if (int rc = enter(h)) return rc;
  TlkState& tk = h->tlk;
  if (enable && h->look.max_lead > 0 && h->obs.tr_B > 0 && tlk_table_bytes(h->obs.tr_B, h->obs.tr_S, h->cfg.N) > LOOK_TABLE_BUDGET)
    return fail(MPMPC_E_ARG, TLK_OVER_BUDGET);
  if (enable && h->cfg.N > 255) return fail(MPMPC_E_ARG, "lookahead needs N <= 255");
  if ((enable != 0) != tk.on) tk.forget();      // (switched on: no track is the last step's; off: the last step's tables are nobody's)
  tk.on = enable != 0;
  return MPMPC_OK;
}

int mpmpc_rollout_tracks(mpmpc_handle h, int32_t B, int32_t* valid_out, int32_t* cells_out, double* tm_out) {
  if (int rc = enter(h, valid_out != nullptr)) return rc;
  const TlkState& tk = h->tlk;
  if (B < 1 || tk.ran_B != B || !tk.tracks_live || !h->ro.valid)
    return fail(MPMPC_E_STATE, "the last rollout step left no plan tracks for B cars (mpmpc_rollout_set_lookahead_traffic with lookahead "
                               "and traffic set), or a per-car setting, a route or the rollout was set anew since");
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t n1 = (size_t)h->cfg.N + 1;
  HIP_TRY(hipMemcpyAsync(valid_out, tk.valid, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, sl.stream));
  if (cells_out) HIP_TRY(hipMemcpyAsync(cells_out, tk.cells, sizeof(int) * 2 * n1 * (size_t)B, hipMemcpyDeviceToHost, sl.stream));
  if (tm_out) HIP_TRY(hipMemcpyAsync(tm_out, tk.tm, sizeof(double) * n1 * (size_t)B, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

int mpmpc_rollout_lookahead_traffic(mpmpc_handle h, int32_t B, int32_t* who_out, int32_t* discs_out) {
  if (int rc = enter(h, who_out != nullptr)) return rc;
  const TlkState& tk = h->tlk;
  if (B < 1 || tk.ran_B != B || !h->ro.valid)
    return fail(MPMPC_E_STATE, "the last rollout step did not anticipate traffic for B cars (mpmpc_rollout_set_lookahead_traffic with "
                               "lookahead and traffic set), or a per-car setting, the lookahead or the rollout was set anew since");
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  const size_t slots = (size_t)B * tk.ran_S;
  HIP_TRY(hipMemcpyAsync(who_out, tk.who, sizeof(int) * slots, hipMemcpyDeviceToHost, sl.stream));
  if (discs_out) HIP_TRY(hipMemcpyAsync(discs_out, tk.tz, sizeof(int) * 3 * (size_t)h->cfg.N * slots, hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

int mpmpc_rollout_set_lookahead(mpmpc_handle h, int32_t n_wp, const double* seg_time, int32_t max_lead) {
  if (int rc = enter(h)) return rc;
  LookState& lk = h->look;
  if (!seg_time) {      // off
    lk.max_lead = 0;
    lk.ran_B = 0;
    h->tlk.forget();
    return MPMPC_OK;
  }
  const char* why = "";
  if (look_check_setting(n_wp, h->tab.n_wp, seg_time, max_lead, &why)) return fail(MPMPC_E_ARG, why);
  if (h->cfg.N > 255) return fail(MPMPC_E_ARG, "lookahead needs N <= 255");
  if (h->obs.mv_B > 0 && look_table_bytes(h->obs.mv_n, h->cfg.N) > LOOK_TABLE_BUDGET) return fail(MPMPC_E_ARG, LOOK_OVER_BUDGET);
  if (h->tlk.on && h->obs.tr_B > 0 && tlk_table_bytes(h->obs.tr_B, h->obs.tr_S, h->cfg.N) > LOOK_TABLE_BUDGET)
    return fail(MPMPC_E_ARG, TLK_OVER_BUDGET);
  HIP_TRY(hipSetDevice(h->cfg.device));
  lk.max_lead = 0;      // a failure below leaves "off"
  lk.ran_B = 0;
  h->tlk.ran_B = 0;      // (the leads change: the last step's traffic horizon is no step's of this setting; the tracks stay)
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
