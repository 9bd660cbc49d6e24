// The handle of libmpmpc.so: the error channel, the sub-states a handle is made of - each with its buffers (device_buf.hpp: the
// handle's destructor frees them), its counts and flags and the views the kernels take - the launch slots, and settle / drain.
// Part of the one translation unit mpmpc_hip.hip (included there after the solve kernels); host code only.
// Field names: a field drops the prefix that names its own sub-state (ro.s, rec.cap); every other name is kept.
#pragma once
#include "device_buf.hpp"
#include "device_scratch.hpp"
#include "route_state.hpp"

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
// (expr: a HIP call, or an allocation of device_buf.hpp, which returns the runtime's code as an int)
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = static_cast<hipError_t>(expr);                                                 \
    if (e_ != hipSuccess)                                                                          \
      return fail(MPMPC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
  } while (0)

// An entry point without a handle takes its scratch (device_scratch.hpp) here: `table` is the entry point's own, `word` names it
// in the message.  One order for all of them: the device count, the two range checks, the device is set, the scratch locked,
// grown to `need` bytes and given its stream.  The lock is held while `Scratch` lives - declare it where the call should end.
struct Scratch {
  std::unique_lock<std::mutex> lock;
  char* blk = nullptr;
  hipStream_t stream = nullptr;
};
static int scratch_acquire(SpScratch* table, int device, size_t need, const char* word, Scratch* out) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MPMPC_E_HIP, "no such HIP device");
  if (device >= SP_MAX_DEVICES) return fail(MPMPC_E_ARG, std::string("device ordinal beyond the ") + word + " scratch table");
  HIP_TRY(hipSetDevice(device));
  SpScratch& g = table[device];
  out->lock = std::unique_lock<std::mutex>(g.mu);
  HIP_TRY(grow(g, need));
  if (!g.stream) HIP_TRY(hipStreamCreate(&g.stream));
  out->blk = g.block;
  out->stream = g.stream;
  return MPMPC_OK;
}

// `count` elements of T, device -> host, on the stream; a getter's output that the caller left NULL is skipped.  The byte count
// comes from T: where a block is read as another type than it is kept in, the cast stands at the call.
// (`src` takes no part in deducing T, so that a Buf<T> converts)
template <class T>
static hipError_t pull(hipStream_t stream, T* dst, const typename std::common_type<T>::type* src, size_t count) {
  return dst ? hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, stream) : hipSuccess;
}

// path and corridor tables
struct TabState {
  Buf<double> kappa, v_ref, ds_next, ub_tab, lb_tab;
  int n_wp = 0, n_cols = 0;
  // Route fleets (mpmpc_set_routes / mpmpc_set_car_routes): what the routes are and which one every instance is on
  // (route_state.hpp: host only), and the device form of the latter, max_batch wide - the {first row, length, negated when
  // open} pairs that gather_stage reads (PathTables::route).
  RouteState routes;
  Buf<int> car_hdr;
  PathTables path_tables() const {
    PathTables t{kappa, v_ref, ds_next, n_wp, ub_tab, lb_tab, n_cols};
    if (routes.n_routes) t.route = car_hdr;
    return t;
  }
};

// corridor generation on the device: grid, per-waypoint geometry, per-waypoint free segments
struct CorState {
  Buf<int8_t> map;
  int map_h = 0, map_w = 0;
  double map_ox = 0, map_oy = 0, map_res = 0;
  Buf<double> gx, gy, gpsi, bub, blb, segs, gtrig;
  Buf<int> nseg, bad;      // bad[0]: start waypoints without a free segment, bad[1]: K0a overflow code
  int geom_n = 0;
  std::vector<double> host_bub, host_blb;   // border points, kept to validate them against the map of the moment
  // per-car obstacles (K0c): cached border lines of the last build, and what that build was made from
  Buf<int> line_cells, line_box;      // [n_wp x COR_CELL_CAP], [n_wp x COR_LINE_BOX]
  unsigned base_gen = 1;        // bumped by mpmpc_set_path / _set_map / _set_path_geometry
  unsigned built_gen = 0;       // base_gen of the last successful mpmpc_build_corridor (0: none)
  double built_min_width = 0, built_sm = 0;
  MapView map_view() const { return MapView{map, map_h, map_w, map_ox, map_oy, map_res}; }
  PathGeom path_geom(const TabState& tab, int circular) const { return PathGeom{gx, gy, gpsi, tab.ds_next, tab.n_wp, circular, gtrig}; }
  double* forced_rows(const TabState& tab) const { return segs.get() + (size_t)4 * COR_MAXSEG * tab.n_wp; }      // cor_forced rows behind the segments
  // the corridor is built for the current map and path
  bool built(const TabState& tab) const { return built_gen == base_gen && built_gen != 0 && tab.n_cols > 0 && line_cells; }
};

// what K0m / K0h take of the movers' block and K0t of the traffic block (host-side decodings of ObsState's two blocks)
struct MoverView {
  int n;                            // movers of the fleet (0: none in force)
  long long step0;
  const double* prm;                // [MOV_PARAMS][n]
  const int *kind, *radius, *dst;   // [n] each; dst: the mover's slot in the cars' disc lists
};
struct TrafficView {
  int S, range;                     // slots per car, range [cells]
  const int *dense, *radius, *members, *goff;      // [tr_B] each, then the groups' offsets
};

// per-car discs, movers and traffic
struct ObsState {
  Buf<int> obst_off, obst_discs, ro_flag;   // CSR lists on the device, per-car row verdicts
  int obst_B = 0;               // > 0: the rollout's cars carry their own discs (mpmpc_rollout_set_obstacles)
  unsigned obst_gen = 0;        // base_gen the discs were validated against
  bool car_rows = false;        // the last rollout step built per-car rows
  // The three per-car settings, kept on the host: static discs (mpmpc_rollout_set_obstacles; st_B > 0: set; obst_gen),
  // movers (mpmpc_rollout_set_movers; mv_B > 0: set; mv_gen) and traffic (mpmpc_rollout_set_traffic; tr_B > 0: set;
  // tr_gen).  Whichever setter is called lays out ONE CSR list per car on the device (obst_off / obst_discs, what K0c
  // reads: the static discs, then a slot per mover that K0m fills every step, then tr_S traffic slots that K0t fills
  // every step) - sync_disc_lists; obst_B is the B of whichever is set.
  std::vector<int32_t> st_off, st_discs, mv_off, comb_off;
  int st_B = 0, mv_B = 0, mv_n = 0;      // mv_n: movers of the fleet
  unsigned mv_gen = 0;          // base_gen the movers were set against
  long long mv_step0 = 0;
  Buf<char> mv_block;           // [4][mv_n] doubles (parameters), then [mv_n] ints each: kind, radius, slot; only grows
  int tr_B = 0, tr_S = 0, tr_range = -1;      // traffic: cars, slots per car, range [cells]
  unsigned tr_gen = 0;          // base_gen the traffic was set against
  Buf<int> tr_block;            // [4 max_batch + 1]: dense group, radius, members (each [tr_B]), group offsets
  bool discs_live = false;      // obst_discs hold the lists the last rollout step used (mpmpc_rollout_obstacles)
  // The fourth per-car setting: walls (mpmpc_rollout_set_walls; wl_B > 0: set; wl_gen).  Not discs: a CSR list of its own
  // (wl_off / wl_hdr, WALL_HDR ints per wall) and the walls' table (wl_tab, sized by the sum of the walls' extents), filled by
  // K0w when the walls are set.  wl_raw / wl_ok: K0w's input ([n][4]) and its per-wall verdict.  A new setting is built in buffers of its own
  // and moved in when K0w has accepted every wall (a refused call leaves the old one).
  Buf<int> wl_off, wl_hdr, wl_tab, wl_raw, wl_ok;
  int wl_B = 0, wl_n = 0;
  unsigned wl_gen = 0;          // base_gen the walls were set against
  // B of the per-car worlds in force (0: none - the shared table), and what the kernels take of the walls
  int world_B() const { return obst_B > 0 ? obst_B : wl_B; }
  WallView wall_view() const { return wl_B > 0 ? WallView{wl_off, wl_hdr, wl_tab} : WallView{nullptr, nullptr, nullptr}; }
  MoverView mover_view() const {
    const int n = obst_B > 0 && mv_B > 0 ? mv_n : 0;
    const double* p = (const double*)mv_block.get();
    const int* i = (const int*)(p + (size_t)MOV_PARAMS * n);
    return MoverView{n, mv_step0, p, i, i + n, i + 2 * (size_t)n};
  }
  TrafficView traffic_view() const {
    const int* t = tr_block.get();
    const size_t nb = (size_t)tr_B;
    return TrafficView{tr_S, tr_range, t, t + nb, t + 2 * nb, t + 3 * nb};
  }
};

// closed-loop rollout state
struct RoState {
  Buf<double> cum, s, pose, u;
  Buf<int> counter, alive, act, shift;      // act, shift: warm start - certified active sets [B x ld], waypoints advanced [B]
  Buf<char> reroute;      // mpmpc_rollout_reroute's block (mpmpc_project.hpp): the request, the projection, the verdicts
  int warm = 2;      // 0 off, 1 on, 2 where it pays (see plan_solve)
  double Ts = 0;
  int B = 0;
  bool valid = false;      // the batch blocks still hold the rollout's plans / waypoint ids / states
  // Does the handle hold the state of a rollout of at least B cars?  `overwritten`: the entry point's own text for a state
  // that an upload has overwritten (none given: the short form serves for both)
  int check(int B_, const char* overwritten = "call mpmpc_rollout_init for at least B cars first") const {
    if (B_ < 1 || B_ > B) return fail(MPMPC_E_STATE, "call mpmpc_rollout_init for at least B cars first");
    return valid ? MPMPC_OK : fail(MPMPC_E_STATE, overwritten);
  }
};

// recorder (mpmpc_rollout_record): the trace has its own memory, [cap] records of rec_bytes() each
struct RecState {
  Buf<char> buf;
  Buf<int> ain;             // [B] alive before the step being recorded
  RoTraceLayout lay{};
  RoChainLayout chain{};    // the pose chain behind it (chain.bytes == 0: no chain bit selected)
  size_t rec_bytes() const { return (size_t)lay.bytes + (size_t)chain.bytes; }      // a record's stride
  int cap = 0, B = 0, fields = 0, stride = 1;
  int count = 0;            // records held
  long long ro_steps = 0;   // rollout steps since mpmpc_rollout_init
  // records that steps ro_steps .. ro_steps + n_steps - 1 add (every stride-th step counted from mpmpc_rollout_init)
  long long records_of(long long n_steps) const { return (ro_steps + n_steps + stride - 1) / stride - (ro_steps + stride - 1) / stride; }
};

// lidar of the rollout (mpmpc_rollout_scan): memory of its own - a scan writes nothing the rollout reads
struct LidState {
  Buf<double> angles, ranges;      // [LID_MAX_BEAMS], [B x n_beams] of the largest scan so far
};

// footprint audit of the rollout (mpmpc_rollout_set_audit): the setting and the per-car accumulators, memory of their own
struct AudState {
  int mode = 0;             // FP_MODE_*: 0 off, 1 audit, 2 audit and stop on contact
  double length = 0, width = 0, reach = 0;
  int R = 0;                // the window's half-width on the map of the moment (aud_check_step)
  int B = 0;                // cars the accumulators were reset for (0: not since the setting changed)
  Buf<int> ints;            // [4][max_batch]: contact_steps, first_contact, min_step, last_contact
  Buf<double> dbls;         // [2][max_batch]: min_clearance, last_clearance
};

// perception of the rollout (mpmpc_rollout_set_perception; the law: perception_core.hpp): the setting, what every car knows of
// its world and the perceived lists K0c reads, memory of their own, sized by max_batch on first use
struct PerState {
  int n_beams = 0;          // 0: off
  double range = 0;
  int hold = 0;
  std::vector<double> host_angles;      // kept to check the range against the map of the moment
  Buf<double> angles;       // [LID_MAX_BEAMS]
  Buf<int> mem;             // K0s's block, max_batch cars wide (K0S_* in mpmpc_lidar.hpp): first_seen / last_seen of every slot, the masks
                            // the last step planned with, static discs and movers per car, and the perceived lists K0c reads (the
                            // layouts of obs.obst_discs and obs.wl_hdr)
  bool fresh = true;        // every slot is to be reset to -1 in front of the next perceiving step
  int B = 0;                // cars of the perceiving steps since the last reset (0: none yet)
  void forget() { fresh = true; B = 0; }
};

// lookahead of the rollout (mpmpc_rollout_set_lookahead; the law: lookahead_core.hpp): the setting, and what K0h writes every
// step for the LEAD instantiations of K0c - memory of its own, laid out for the movers in force in front of the first step that
// needs it (mpmpc_lookahead.hpp)
struct LookState {
  int max_lead = 0;         // 0: off
  unsigned gen = 0;         // base_gen the setting was made against
  Buf<double> seg;          // seg_time [n_wp]
  Buf<int> lead;            // [max_batch x N] the leads of the last step
  Buf<int> car;             // [B + 1][2]: a car's first mover in the fleet's list, its first mover slot in its own disc list
  Buf<int> tab;             // [movers of the fleet][N][3] the horizon discs of the last step; only grows
  std::vector<int32_t> host_car;
  bool laid = false;        // car and tab fit the per-car settings in force
  int ran_B = 0, ran_n = 0; // cars and movers K0h ran for in the last step (0: it did not run)
};

// lookahead for traffic (mpmpc_rollout_set_lookahead_traffic; the law: traffic_lookahead_core.hpp): the flag, the plan tracks
// K3t leaves at the end of every step that anticipates traffic, and what K0t and K0ht write in front of K0c - memory of its
// own, sized in front of the first step that needs it (mpmpc_lookahead.hpp)
struct TlkState {
  bool on = false;          // the flag; a step anticipates traffic iff it is on, lookahead is set and traffic is set
  Buf<int> valid;           // [max_batch]: may the car's track be read
  Buf<int> cells;           // [max_batch][N + 1][2]: the cell of every stage of the car's plan (TLK_OFF: none)
  Buf<double> tm;           // [max_batch][N + 1]: the running maximum of the plan's times
  Buf<int> who;             // [B][S] the occupants of the traffic slots of the last step; only grows
  Buf<int> tz;              // [B][S][N][3] the horizon discs of the traffic slots of the last step; only grows
  bool tracks_live = false; // the tracks are those of the rollout's last step (else valid is cleared in front of the next reader)
  int ran_B = 0, ran_S = 0; // cars and slots K0ht ran for in the last step (0: it did not run)
  void forget() { tracks_live = false; ran_B = 0; }
};

// plant models of the rollout (mpmpc_rollout_set_plant; the law: plant_core.hpp): the setting, the cars' actuator states, the
// measured poses K3a localises on and the tracking accumulators - memory of its own, sized by max_batch when first set
struct PlantState {
  int B = 0;                // > 0: a plant is in force for B cars
  unsigned long long seed = 0;
  int car0 = 0;
  long long step0 = 0;
  Buf<double> prm;          // [max_batch][PL_PARAMS]
  Buf<double> act;          // [max_batch][2]: the executed (v, delta) of the last driven step
  Buf<double> meas;         // [max_batch][3]: the pose K3a saw in the last step
  Buf<double> ey;           // [2][max_batch]: ey_max, ey_sq
  Buf<int> steps;           // [max_batch]
  bool ran = false;         // a step ran under the setting in force (mpmpc_rollout_plant)
  std::vector<double> host_scale;      // [B]: every car's wheelbase_scale (host copy: the dynamics' check of a step)
};

// dynamic single-track plant of the rollout (mpmpc_rollout_set_dynamics; the law: dynamics_core.hpp): the setting, the cars'
// velocity states and the accumulators - memory of its own, sized by max_batch when first set
struct DynState {
  int B = 0;                // > 0: dynamics are in force for B cars
  Buf<double> prm;          // [max_batch][DY_PARAMS]
  Buf<double> state;        // [max_batch][DY_STATE]: (vx, vy, r) after the last driven step
  Buf<int> counts;          // [DY_COUNTS][max_batch]: dyn_steps, sat_front, sat_rear
  Buf<double> peaks;        // [DY_PEAKS][max_batch]: slip_f, slip_r, alat
  bool ran = false;         // a step ran under the setting in force (mpmpc_rollout_dynamics)
  std::vector<double> host_prm;      // [B][DY_PARAMS] (host copy: the check of a step needs Ts and the plant's wheelbase)
  bool verified = false;    // dy_check_run passed for the setting, the plant and the Ts in force
};

// actuation delay of the rollout and its compensation (mpmpc_rollout_set_delay; the law: delay_core.hpp): the setting, the cars'
// command registers, the predicted poses and arc lengths K3a localises on and the spatial state of where the cars are - memory
// of its own, sized by max_batch when first set
struct DelayState {
  int B = 0;                // > 0: a delay is in force for B cars
  Buf<int> delay, assumed;  // [max_batch] each: d and c
  Buf<double> queue;        // [max_batch][DL_MAX][2]: the issued (v, delta), the newest first
  Buf<double> pred_pose;    // [max_batch][3]: the pose K3a saw in the last step
  Buf<double> pred_s;       // [max_batch]: ... and the arc length
  Buf<double> now;          // [max_batch][3]: x0[0], x0[1] and kappa of the waypoint the car was at in the last step
  Buf<int> now_wp;          // [max_batch]: that waypoint's global row
  bool ran = false;         // a step ran under the setting in force (mpmpc_rollout_delay)
  int max_assumed = 0;      // the largest c of the cars the setting is in force for (host copy: plan_step)
};

// pose estimator of the rollout (mpmpc_rollout_set_estimator; the law: estimator_core.hpp): the setting, every car's estimate,
// covariance and statistics - memory of its own, sized by max_batch when first set
struct EstState {
  int B = 0;                // > 0: an estimator is in force for B cars
  unsigned long long seed = 0;
  int car0 = 0;
  long long step0 = 0;
  Buf<double> prm;          // [max_batch][ES_PARAMS]
  Buf<double> est;          // [max_batch][3]: the pose the controller localises on
  Buf<double> cov;          // [max_batch][ES_COV]: the upper triangle Pxx, Pxy, Pxp, Pyy, Pyp, Ppp
  Buf<int> primed;          // [max_batch]
  Buf<double> stats;        // [ES_STATS][max_batch]: err2_max, err2_sum, meas2_sum, head2_sum
  Buf<int> count;           // [2][max_batch]: used, steps
  bool ran = false;         // a step ran under the setting in force (mpmpc_rollout_estimator)
};

// lidar localisation of the rollout (mpmpc_rollout_set_localiser; the law: localiser_core.hpp): the setting - per fleet -, the
// distance field of the base map it was made on, every car's fix and statistics - memory of its own, sized by max_batch, the
// map and the beams when set
struct LocState {
  int B = 0;                // > 0: the localiser is in force for B cars
  unsigned gen = 0;         // base_gen the field was built against
  LcSet set{};
  int n_beams = 0;
  double range = 0;
  long long period = 1;
  unsigned long long seed = 0;
  int car0 = 0;
  long long step0 = 0;
  Buf<uint8_t> field;       // [map_h][map_w]: K0d's capped squared distances
  Buf<double> angles;       // [LID_MAX_BEAMS]
  Buf<double> ranges;       // [max_batch][n_beams]: K0l's scans of the last scheduled step, the hits noisy
  Buf<double> fix, prior;   // [max_batch][3] each: the pose the controller localises on, and dead reckoning's
  Buf<int> primed;          // [max_batch]
  Buf<int> out;             // [3][max_batch]: cand, score, hits of the last step
  Buf<double> stats;        // [LC_STATS][max_batch]: err2_max, err2_sum, head2_sum, prior2_sum
  Buf<int> count;           // [LC_COUNTS][max_batch]: steps, matched, lost, edge
  bool ran = false;         // a step ran under the setting in force (mpmpc_rollout_localiser)
};

// corridor commitment of the rollout (mpmpc_rollout_set_commitment; the law: commitment_core.hpp): the setting, every car's memory
// of its last row - twice: a step of K0c<., ., ., true> reads buffer `cur` and writes the other, then they swap - and the counters;
// one block of its own, sized by the setting's B
struct CmtState {
  int B = 0;                // > 0: the commitment is in force for B cars
  unsigned gen = 0;         // base_gen the setting was made against
  Buf<char> block;          // keep [B] doubles, rows [2][B][N][COR_WPC] doubles, wp [2][B][N] ints, counts [CMT_COUNTS][B] ints
  int cur = 0;              // the buffer that holds the memory of the last step
  bool ran = false;         // a step ran under the setting in force (mpmpc_rollout_commitment)
  double* keep() const { return (double*)block.get(); }
  double* rows(int which, int N) const { return keep() + B + (size_t)which * B * N * COR_WPC; }
  int* wp(int which, int N) const { return (int*)(keep() + B + (size_t)2 * B * N * COR_WPC) + (size_t)which * B * N; }
  int* counts(int N) const { return wp(0, N) + (size_t)2 * B * N; }
};

// per-batch inputs and host staging
struct IoState {
  // the inputs of a batch lie back to back in ONE device block (wp_id, x0, cc, lb, ub, laid out for the batch size
  // of the last upload), and so do the outputs of every launch slot (Slot::out_block: u0, resid, status, iters, z, y): an upload
  // or a download through the pinned staging buffers is then a single copy instead of five or six - what a single-car call is made of
  Buf<char> in_block;
  int* wp_id = nullptr;       // pointers into it (lay_out):
  double *x0 = nullptr, *cc = nullptr, *lb = nullptr, *ub = nullptr;
  bool have_rows = false;     // per-instance corridor rows uploaded (else: table)
  int uploaded = 0, laid_out = 0;
  Buf<double> qp;      // stage-blocked QP
  // pinned host staging for mpmpc_upload / mpmpc_download (small copies from pageable memory are
  // synchronous and slow; empty above STAGE_LIMIT bytes: large batches amortise the direct path)
  Buf<char, Mem::Pinned> stage_in, stage_out;
  hipEvent_t ev_in = nullptr;      // the last staged upload has left the pinned buffer
  bool in_flight = false;
  // ... above that limit an upload goes through a small page-locked bounce buffer in two halves (allocated by the first such
  // upload): the device copy of one half runs while the host fills the other, and the call returns when the caller's buffers
  // have been read - not when the device has them.  (A copy from pageable memory is synchronous: one process feeding several
  // devices - sharded.py - would otherwise serve them one after the other)
  Buf<char, Mem::Pinned> bounce;
  hipEvent_t ev_bounce[2] = {nullptr, nullptr};
  bool bounce_busy[2] = {false, false};
  int bounce_turn = 0;
  // what the solve kernels and K1 read of a batch
  AssembleIn inputs(const TabState& tab) const { return AssembleIn{tab.path_tables(), wp_id, x0, cc, have_rows ? lb : nullptr, have_rows ? ub : nullptr}; }
  size_t staged_bytes = 0;  // mpmpc_staged_begin without its mpmpc_staged_end: bytes of the output block on their way back
  bool staged_async = true; // mpmpc_staged_begin was called as such (not as the first half of mpmpc_solve_staged)
};

struct mpmpc_handle_s {
  mpmpc_config cfg;
  mpmpc_settings st;
  int ld = 0, n = 0, m = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  TabState tab;
  CorState cor;
  ObsState obs;
  RoState ro;
  RecState rec;
  LidState lid;
  AudState aud;
  PerState per;
  LookState look;
  TlkState tlk;
  PlantState pl;
  DelayState dl;
  DynState dy;
  EstState es;
  LocState lc;
  CmtState cm;
  IoState io;
  // ---- Launch slots: what ONE solve launch in flight owns - its stream, its output block, its tail lists and its deferred-tail
  // state.  slot[0] is made by mpmpc_create (its stream before anything else touches the device) and is all a handle needs that
  // never pipelines; slot[1 .. n_slots - 1] are made by the first pipelined resident launch (next_slot).  `cur` is the slot of the
  // LAST launch, and everything in this library that is not a resident launch - uploads, downloads, the staged calls, corridor build,
  // rollout, recorder, timed launches - works on last(): its stream, its outputs.  A resident launch first moves `cur` one slot on
  // (round robin over the `pipeline` slots in use), so that launches k + 1 .. k + pipeline - 1 run beside launch k, each on its
  // own stream, writing its own outputs.  A function that acts on a slot is handed it; nothing is copied between slots.
  struct Slot {
    hipStream_t stream = nullptr;
    Buf<char> out_block;      // pointers into it (lay_out):
    double *z = nullptr, *u0 = nullptr, *resid = nullptr, *y = nullptr;
    int *status = nullptr, *iters = nullptr;
    bool y_valid = false;     // the slot's last solve launch stored y
    bool busy = false;        // resident launches in flight on the slot's stream that nothing has waited for yet
    // instances the early pass of a packed (2 or 4 per wave) launch could not certify: [0] = count, [1..] = ids
    Buf<int> tail;
    int tail_flip = 0;          // which of the two lists the next reduced-native launch fills
    // Deferred tail (batch launches of the reduced-native kernels, not the closed loop).  Launching the tail kernel costs
    // 4.8 us even when its list is empty - 10 % of a 1 024-instance step - so when the last launch whose outcome the host
    // has SEEN left no tail, the next launches do not enqueue one: the reduced-native kernel stamps its sequence number into
    // tail_flag (host memory) if it appends anything, and every entry point through which results or state can be observed
    // or changed (sync, download, upload, set_*, rollout, timed launches) first drains the stream, looks at the stamp and
    // runs the tail of the slot's LAST launch if it left one (observe_tail).  A launch that is followed by another launch on
    // the slot without such a call in between has unobservable results either way (same output buffers).
    Buf<unsigned, Mem::Pinned> tail_flag;         // page-locked, device-visible
    unsigned seq = 0;                   // sequence number of the last reduced-native launch
    bool tail_expect_empty = false;     // the last observed launch left no tail
    bool tail_ran_late = false;         // the last observe_tail had to run a deferred tail
    // Second level (reduced_native_tail configurations): the tail goes to the reduced-native tail kernel first, which appends
    // what IT leaves to a third list (tail + 2 (max_batch + 1)) and stamps tail_flag[1]; the general kernel on that list is
    // deferred by the same rule.
    bool tail2_expect_empty = false;
    // The slot's last solve launch: its plan (mpmpc_launch_plan.hpp), the first stage not yet enqueued, and what the stages
    // still to come need of the launch they belong to - the batch size, whether y is stored, the solver parameters, the lists
    // by role (MPMPC_LIST_*).  (The handle's input buffers and path tables are read when a stage is enqueued: every call that
    // changes them settles first.)
    SolvePlan plan{};
    int next_stage = 0;
    int launch_B = 0;
    bool want_y = false;
    SolverParams prm{};
    int* list[4] = {nullptr, nullptr, nullptr, nullptr};
    bool deferred() const { return next_stage < plan.n; }      // stages of the last launch were held back
  };
  static constexpr int MAX_PIPELINE = 8;
  Slot slot[MAX_PIPELINE];
  int n_slots = 0;          // slots allocated: slot[0 .. n_slots - 1]
  int cur = 0;              // the slot of the last launch
  Slot& last() { return slot[cur]; }
  int pipeline = 3;         // launch slots in use = resident launches in flight (1 = one slot only): what mpmpc_set_pipeline asked
                            // for, three by default, but never more than the process has hardware queues (launch_streams:
                            // GPU_MAX_HW_QUEUES, 4 if unset) - two streams on one queue take turns.  Measured, config 2, four
                            // queues: depth 4 = 68.7 M solves/s with the four launch streams on four queues, 39.5 M while a
                            // synchronous memset of this library had made the null stream hold one of them (two launch streams
                            // shared a queue: 2.0 instead of 3.85 solve kernels on the chip; profiles/hw_queues/)
  hipEvent_t ev_order = nullptr;
  bool order_pending = false;      // asynchronous work other than resident solves is queued on last().stream: the next resident launch
                                   // goes to ANOTHER stream and has to wait for it (uploads, closed-loop steps: they write what solves read)
  int force_lanes = 0;      // mpmpc_set_packing: 0 = chosen from the batch size
  // mpmpc_set_tail_kernel (MPMPC_LEAN_TAIL=0 in the environment: off from the start, for A/B timings of whole programs)
  bool lean_tail = !(std::getenv("MPMPC_LEAN_TAIL") && std::atoi(std::getenv("MPMPC_LEAN_TAIL")) == 0);
  bool lean_tail_single = std::getenv("MPMPC_LEAN_TAIL") && std::atoi(std::getenv("MPMPC_LEAN_TAIL")) == 2;      // ONE tail instance per wave
  bool resident_y = true;   // mpmpc_set_outputs: do resident launches store the multipliers y (46 % of the output bytes)?
};
using Slot = mpmpc_handle_s::Slot;

static int observe_tail(mpmpc_handle h, Slot& s);
// The other slots' launches are drained and their deferred tails, if any, are run (the slot of the last launch is left as it
// is: what follows on its stream is ordered behind it anyway).
static int settle_other_slots(mpmpc_handle h) {
  for (int i = 0; i < h->n_slots; ++i) {
    Slot& s = h->slot[i];
    if (i == h->cur || (!s.busy && !s.deferred())) continue;
    if (int rc = observe_tail(h, s)) return rc;
  }
  return MPMPC_OK;
}
// ... and then the slot of the last launch: every launch of the handle is done, deferred tails included
static int drain(mpmpc_handle h) {
  if (int rc = settle_other_slots(h)) return rc;
  return observe_tail(h, h->last());
}
// first statement of every entry point that reads results or changes what a launch in flight - or a deferred tail launch -
// works on: `if (int rc = settle(h)) return rc;`
static int settle(mpmpc_handle h) {
  if (int rc = mpmpc_staged_end(h)) return rc;      // (of a staged call that was begun, if any)
  if (int rc = settle_other_slots(h)) return rc;
  if (h->last().deferred()) {
    if (int rc = observe_tail(h, h->last())) return rc;
  }
  h->order_pending = true;
  return MPMPC_OK;
}
// ... of an entry point whose only pointer is the handle: `if (int rc = enter(h)) return rc;`
static int enter(mpmpc_handle h) { return h ? settle(h) : fail(MPMPC_E_ARG, "handle is NULL"); }
// ... and of one with further pointers that must not be null: `if (int rc = enter(h, a && b)) return rc;`
static int enter(mpmpc_handle h, bool others) { return h && others ? settle(h) : fail(MPMPC_E_ARG, "NULL argument"); }
