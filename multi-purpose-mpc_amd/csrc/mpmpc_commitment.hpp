// Corridor commitment of the rollout (K0k), part of the one translation unit mpmpc_hip.hip (included behind mpmpc_localiser.hpp and
// in front of mpmpc_closed_loop.hpp, whose K0c has the KEEP instantiations; the step loop of mpmpc_rollout_step.hpp chooses them):
// the view K0c takes, what a step and the resets need of the sub-state cm of the handle (mpmpc_handle.hpp), and the entry points
// mpmpc_rollout_set_commitment / mpmpc_rollout_commitment.  The law: commitment_core.hpp.
#pragma once

// what the KEEP instantiations of K0c take of the commitment (the others: the empty KeepNone)
struct KeepNone {};
struct KeepView {
  const double* keep;        // [B]: 0 off, else the switch_ratio
  const int* wp_old;         // [B][N]: the memory the step reads ...
  const double* rows_old;    // [B][N][COR_WPC]
  int* wp_new;               // ... and the one it writes
  double* rows_new;
  int* counts;               // [CMT_COUNTS][stride]: kept, switched, moved
  long stride;
};

// cars b0 .. b1 - 1 of the memory a step would read forget their rows (every entry empty), on the slot's stream
static int commitment_forget(mpmpc_handle h, Slot& sl, int b0, int b1) {
  const CmtState& c = h->cm;
  const size_t N = (size_t)h->cfg.N, n = (size_t)(b1 - b0) * N;
  HIP_TRY(hipMemsetAsync(c.wp(c.cur, (int)N) + (size_t)b0 * N, 0xff, sizeof(int) * n, sl.stream));      // CMT_EMPTY
  HIP_TRY(hipMemsetAsync(c.rows(c.cur, (int)N) + (size_t)b0 * N * COR_WPC, 0, sizeof(double) * COR_WPC * n, sl.stream));
  return MPMPC_OK;
}

// mpmpc_rollout_init under a commitment in force: the setting stays, the memory is emptied and the counters start over
static int commitment_reset(mpmpc_handle h, Slot& sl) {
  CmtState& c = h->cm;
  if (int rc = commitment_forget(h, sl, 0, c.B)) return rc;
  HIP_TRY(hipMemsetAsync(c.counts(h->cfg.N), 0, sizeof(int) * CMT_COUNTS * (size_t)c.B, sl.stream));
  c.ran = false;
  return MPMPC_OK;
}

// mpmpc_rollout_reroute under a commitment in force: the cars it accepted are on another route - their memory is emptied
static int commitment_rerouted(mpmpc_handle h, Slot& sl, int B, const int32_t* accepted) {
  const int n = B < h->cm.B ? B : h->cm.B;
  for (int b = 0; b < n;) {      // (one pair of memsets per run of accepted cars)
    if (!accepted[b]) { ++b; continue; }
    int e = b;
    while (e < n && accepted[e]) ++e;
    if (int rc = commitment_forget(h, sl, b, e)) return rc;
    b = e;
  }
  return MPMPC_OK;
}

// What plan_step asks of a step under a commitment: the setting's B, nothing the setting was made on changed, a per-car world
// in force and no lookahead.
static int commitment_check_step(mpmpc_handle h, int B, bool per_car) {
  if (h->cm.B != B) return fail(MPMPC_E_STATE, "the commitment was set for another number of cars (mpmpc_rollout_set_commitment)");
  if (h->cm.gen != h->cor.base_gen)
    return fail(MPMPC_E_STATE, "map, path, routes or geometry changed since mpmpc_rollout_set_commitment: set the commitment again");
  if (!per_car)
    return fail(MPMPC_E_STATE, "a commitment needs a per-car world in force for the same cars: rows of the shared table have no per-car "
                               "memory (mpmpc_rollout_set_obstacles with empty lists will do)");
  if (h->look.max_lead > 0)
    return fail(MPMPC_E_STATE, "a commitment and a lookahead are both in force: commitment under lookahead is not supported "
                               "(mpmpc_rollout_set_commitment / mpmpc_rollout_set_lookahead: switch one off)");
  return MPMPC_OK;
}

// what K0c<., false, false, true> takes of the commitment in a step; the step writes the other buffer, which is the memory then
static KeepView commitment_view_and_swap(mpmpc_handle h) {
  CmtState& c = h->cm;
  const int N = h->cfg.N, old = c.cur;
  c.cur ^= 1;
  return KeepView{c.keep(), c.wp(old, N), c.rows(old, N), c.wp(c.cur, N), c.rows(c.cur, N), c.counts(N), (long)c.B};
}

extern "C" {

int mpmpc_rollout_set_commitment(mpmpc_handle h, int32_t B, const double* keep, const int32_t* mem_wp, const double* mem_rows) {
  if (int rc = enter(h)) return rc;
  if (!keep) {      // no commitment: K0c builds every row from nothing, as the reference does
    h->cm = CmtState{};
    return MPMPC_OK;
  }
  const int N = h->cfg.N;
  const char* why = "";
  if (cmt_check(B, h->cfg.max_batch, N, keep, mem_wp, mem_rows, &why)) return fail(MPMPC_E_ARG, why);
  HIP_TRY(hipSetDevice(h->cfg.device));
  Slot& sl = h->last();
  // a refused call leaves the old setting: the new block is built on its own and moved in at the end
  CmtState c;
  c.B = B;
  if (c.block.alloc((size_t)cmt_bytes(B, N))) {
    (void)hipGetLastError();
    return fail(MPMPC_E_HIP, "no device memory for the commitment of " + std::to_string(B) + " cars");
  }
  const size_t nb = (size_t)B, cells = nb * (size_t)N;
  HIP_TRY(hipMemcpyAsync(c.keep(), keep, sizeof(double) * nb, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipMemsetAsync(c.rows(0, N), 0, sizeof(double) * 2 * COR_WPC * cells, sl.stream));
  HIP_TRY(hipMemsetAsync(c.wp(0, N), 0xff, sizeof(int) * 2 * cells, sl.stream));      // CMT_EMPTY
  HIP_TRY(hipMemsetAsync(c.counts(N), 0, sizeof(int) * CMT_COUNTS * nb, sl.stream));
  if (mem_wp) {      // the saved memory of a resumed run
    HIP_TRY(hipMemcpyAsync(c.wp(0, N), mem_wp, sizeof(int) * cells, hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemcpyAsync(c.rows(0, N), mem_rows, sizeof(double) * COR_WPC * cells, hipMemcpyHostToDevice, sl.stream));
  }
  HIP_TRY(hipStreamSynchronize(sl.stream));      // the caller's arrays have been read
  c.gen = h->cor.base_gen;
  h->cm = std::move(c);
  return MPMPC_OK;
}

int mpmpc_rollout_commitment(mpmpc_handle h, int32_t B, int32_t* counts_out, int32_t* wp_out, double* rows_out) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  if (int rc = h->ro.check(B)) return rc;
  const CmtState& c = h->cm;
  if (c.B != B || !c.ran)
    return fail(MPMPC_E_STATE, "no rollout step of B cars ran under the commitment in force (mpmpc_rollout_set_commitment)");
  HIP_TRY(hipSetDevice(h->cfg.device));
  const int N = h->cfg.N;
  const size_t cells = (size_t)B * N;
  HIP_TRY(pull(sl.stream, counts_out, c.counts(N), CMT_COUNTS * (size_t)B));
  HIP_TRY(pull(sl.stream, wp_out, c.wp(c.cur, N), cells));
  HIP_TRY(pull(sl.stream, rows_out, c.rows(c.cur, N), COR_WPC * cells));
  HIP_TRY(hipStreamSynchronize(sl.stream));
  return MPMPC_OK;
}

}  // extern "C"
