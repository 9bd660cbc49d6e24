// mpmpc_rollout_step of libmpmpc.so, part of the one translation unit mpmpc_hip.hip (included there behind every feature of a
// step: mpmpc_closed_loop.hpp - the kernels K0c, K0m, K0t, K3a, K3b, K3r -, mpmpc_plant.hpp, mpmpc_delay.hpp, mpmpc_estimator.hpp, mpmpc_localiser.hpp, mpmpc_commitment.hpp, mpmpc_lookahead.hpp, mpmpc_lidar.hpp,
// mpmpc_perception.hpp and mpmpc_footprint.hpp).  A step is decided once (plan_step: every check and lay-out, in a fixed order),
// then its kernels are enqueued in stream order, each from the one enqueue_* function that launches it, then the handle
// remembers what ran (step_ran).  DESIGN.md section 4, "A rollout step", is the same list.
#pragma once

// What the step loop needs, and nothing else (host only).
struct StepPlan {
  bool per_car, discs, walls, traffic, perceiving, plant, delaying, dynamic, estimating, localising, auditing, looking, ahead_traffic, keeping, recording;
  int movers;
  MapView map;
  PathGeom geom;
  MoverPath path;
  const int* plan_discs;      // the world K0c plans in: the true lists, or - perceiving - the lists K0s writes in front of it
  WallView plan_walls;
  const int* route;           // route fleets: the cars' {first row, length} headers (null: one path)
  size_t car_lds;             // K0c's dynamic LDS
  LookTrafficView look;       // K0h's and K0ht's tables (LookView: its first two members)
};

// Every check and lay-out of a step of B cars, in this order (the first refusal that applies is the call's): the rollout's
// state, n_steps, the per-car settings' B, stale generations, the recorder's B and capacity, the plant's B, the delay's B, the
// dynamics' B, plant and stability, the estimator's B, the localiser's B, map and generation, the beams of a recorded scan, the audit, perception, the routes, the lookahead, the delay under a
// lookahead, the estimator and the localiser under an assumed delay of DL_MAX, the commitment.
static int plan_step(mpmpc_handle h, int B, int n_steps, StepPlan& p) {
  if (int rc = h->ro.check(B, "the rollout's state was overwritten by an upload / solve / assemble on this handle: "
                              "call mpmpc_rollout_init again (or use a second handle for single solves)")) return rc;
  if (n_steps < 0) return fail(MPMPC_E_ARG, "n_steps must be >= 0");
  const ObsState& o = h->obs;
  p.per_car = o.world_B() > 0;
  p.discs = o.obst_B > 0;
  p.walls = o.wl_B > 0;
  if (p.per_car) {
    if (o.world_B() != B || (p.walls && o.wl_B != B)) return fail(MPMPC_E_STATE, "the per-car obstacles were set for another number of cars");
    if ((o.st_B > 0 && o.obst_gen != h->cor.base_gen) || (o.mv_B > 0 && o.mv_gen != h->cor.base_gen) ||
        (o.tr_B > 0 && o.tr_gen != h->cor.base_gen) || (p.walls && o.wl_gen != h->cor.base_gen) || h->cor.built_gen != h->cor.base_gen)
      return fail(MPMPC_E_STATE, "map, path or geometry changed since mpmpc_rollout_set_obstacles / mpmpc_build_corridor");
  }
  p.recording = h->rec.cap > 0;
  if (p.recording) {
    if (h->rec.B != B) return fail(MPMPC_E_STATE, "mpmpc_rollout_record was set up for another number of cars");
    if (h->rec.count + h->rec.records_of(n_steps) > h->rec.cap)
      return fail(MPMPC_E_STATE, "the trace is full: " + std::to_string(h->rec.count) + " of " + std::to_string(h->rec.cap) +
                                     " records held, this call would add " + std::to_string(h->rec.records_of(n_steps)));
  }
  p.plant = h->pl.B > 0;
  if (p.plant && h->pl.B != B) return fail(MPMPC_E_STATE, "the plant was set for another number of cars (mpmpc_rollout_set_plant)");
  p.delaying = h->dl.B > 0;
  if (p.delaying && h->dl.B != B) return fail(MPMPC_E_STATE, "the delay was set for another number of cars (mpmpc_rollout_set_delay)");
  p.dynamic = h->dy.B > 0;
  if (p.dynamic) {
    if (int rc = dynamics_check_step(h, B)) return rc;
  }
  p.estimating = h->es.B > 0;
  if (p.estimating && h->es.B != B)
    return fail(MPMPC_E_STATE, "the estimator was set for another number of cars (mpmpc_rollout_set_estimator)");
  p.localising = h->lc.B > 0;
  if (p.localising) {
    if (h->lc.B != B) return fail(MPMPC_E_STATE, "the localiser was set for another number of cars (mpmpc_rollout_set_localiser)");
    if (!h->cor.map) return fail(MPMPC_E_STATE, "the localiser needs mpmpc_set_map first");
    if (h->lc.gen != h->cor.base_gen)      // (the field is the map's of the setting)
      return fail(MPMPC_E_STATE, "map, path or geometry changed since mpmpc_rollout_set_localiser: set the localiser again");
    if (p.recording && h->rec.chain.ranges >= 0 && h->lc.n_beams != h->rec.chain.n_beams)
      return fail(MPMPC_E_STATE, "the trace records scans of " + std::to_string(h->rec.chain.n_beams) + " beams, the localiser in force has " +
                                     std::to_string(h->lc.n_beams) + " (mpmpc_rollout_record with MPMPC_REC_SCAN: set it up again)");
  }
  if (int rc = aud_check_step(h, B)) return rc;
  p.auditing = h->aud.mode != FP_MODE_OFF;
  HIP_TRY(hipSetDevice(h->cfg.device));
  p.perceiving = false;
  if (h->per.n_beams > 0) {
    if (int rc = per_check_step(h, B, p.per_car, &p.perceiving)) return rc;
  }
  p.plan_discs = p.perceiving ? per_plan_discs(h) : o.obst_discs.get();
  p.plan_walls = o.wall_view();
  if (p.perceiving && p.walls) p.plan_walls.hdr = per_plan_whdr(h);
  const int N = h->cfg.N;
  p.car_lds = sizeof(double) * COR_WPC * N + sizeof(int) * (2 * COR_MAXSEG + 3) * N + sizeof(int) * 3 * COR_MAX_DISCS +
              (sizeof(int) + 1) * COR_CELL_CAP + (p.walls ? sizeof(int) * WALL_HDR * COR_MAX_WALLS : 0);
  p.map = h->cor.map_view();
  p.geom = h->cor.path_geom(h->tab, h->cfg.circular);
  h->io.have_rows = p.per_car;     // K1 / K2 read the per-instance rows K0c writes (else: the table)
  p.movers = p.discs ? o.mover_view().n : 0;
  p.path = MoverPath{h->ro.cum, h->cor.gx, h->cor.gy, h->cor.gtrig, h->tab.n_wp, COR_TRIG, h->cfg.circular ? 1 : 0};
  p.traffic = p.discs && o.tr_B > 0;
  if (int rc = check_car_routes(h, B)) return rc;
  p.route = h->tab.path_tables().route;
  p.looking = p.ahead_traffic = false;
  if (h->look.max_lead > 0) {
    if (int rc = look_check_step(h, B, p.movers, p.traffic, &p.looking, &p.ahead_traffic)) return rc;
  }
  p.look = LookTrafficView{h->look.car.get(), h->look.tab.get(), h->tlk.tz.get(), o.tr_S};
  if (p.delaying && h->look.max_lead > 0)      // (column leads and plan tracks would have to be offset by c: out of scope)
    return fail(MPMPC_E_STATE, "a delay and a lookahead are both in force: lookahead under delay is not supported "
                               "(mpmpc_rollout_set_delay / mpmpc_rollout_set_lookahead: switch one off)");
  if (p.estimating && p.delaying && h->dl.max_assumed >= DL_MAX)      // (K3e reads entry c of the register, which has DL_MAX entries)
    return fail(MPMPC_E_STATE, "an estimator is in force and a car's assumed delay is " + std::to_string(DL_MAX) +
                               ": the command that reached the wheels in the last step has left the register by then "
                               "(mpmpc_rollout_set_estimator / mpmpc_rollout_set_delay: assume at most " + std::to_string(DL_MAX - 1) + ")");
  if (p.localising && p.delaying && h->dl.max_assumed >= DL_MAX)      // (K3l reads the same entry)
    return fail(MPMPC_E_STATE, "a localiser is in force and a car's assumed delay is " + std::to_string(DL_MAX) +
                               ": the command that reached the wheels in the last step has left the register by then "
                               "(mpmpc_rollout_set_localiser / mpmpc_rollout_set_delay: assume at most " + std::to_string(DL_MAX - 1) + ")");
  p.keeping = h->cm.B > 0;
  if (p.keeping) {
    if (int rc = commitment_check_step(h, B, p.per_car)) return rc;
    p.car_lds += sizeof(int) * N;      // (the waypoints of the car's memory)
  }
  return MPMPC_OK;
}

// One function per kernel of the step, each the kernel's only launch site; all on the slot's stream.  k: the step's index.

// K3r, snapshot: s, pose and alive as the step finds them
static void enqueue_record_snapshot(mpmpc_handle h, Slot& sl, int B, char* rec) {
  hipLaunchKernelGGL(mpmpc_record_snapshot_kernel, dim3((unsigned)(((long)B * RO_REC_BEGIN_ENTRIES + 255) / 256)), dim3(256), 0, sl.stream, B,
                     h->ro.s, h->ro.pose, h->ro.alive, h->rec.ain, rec, h->rec.lay);
}

// K0t; a step that anticipates traffic also keeps the slots' occupants (K0ht reads them)
template <bool WHO, class Who>
static void launch_traffic(mpmpc_handle h, Slot& sl, int B, const StepPlan& p, Who who) {
  const TrafficView t = h->obs.traffic_view();
  hipLaunchKernelGGL(mpmpc_traffic_kernel<WHO>, dim3(B), dim3(64), 0, sl.stream, B, t.S, t.range, p.map, h->ro.pose.get(), h->ro.alive.get(),
                     t.dense, t.radius, t.members, t.goff, h->obs.obst_off.get(), h->obs.obst_discs.get(), who);
}
static void enqueue_traffic(mpmpc_handle h, Slot& sl, int B, const StepPlan& p) {
  if (p.ahead_traffic) launch_traffic<true>(h, sl, B, p, h->tlk.who.get());
  else launch_traffic<false>(h, sl, B, p, LookNone{});
}

// K0m: in front of K0s when the step perceives (K0s reads alive as the step finds it, K0m reads nothing K3a writes) and in front
// of K0l when it localises (the scan sees the movers of step k), else behind K3a
static void enqueue_movers(mpmpc_handle h, Slot& sl, int B, long long k, const StepPlan& p) {
  const MoverView m = h->obs.mover_view();
  hipLaunchKernelGGL(mpmpc_obstacle_move_kernel, dim3((m.n + 255) / 256), dim3(256), 0, sl.stream, m.n, k, m.step0, p.map, p.path, m.kind,
                     m.radius, m.prm, m.dst, h->obs.obst_discs.get(), h->obs.obst_off.get(), B, p.route);
}

// what measures the pose: K3l's fix, else the pose K3n measured (plant), else the true one
static const double* measured_pose(mpmpc_handle h, const StepPlan& p) {
  return p.localising ? h->lc.fix.get() : p.plant ? h->pl.meas.get() : h->ro.pose.get();
}
// what the controller localises on: the estimate, else that
static const double* localise_pose(mpmpc_handle h, const StepPlan& p) {
  return p.estimating ? h->es.est.get() : measured_pose(h, p);
}

// K0l of a scheduled localising step: every running car's TRUE pose in its TRUE world of step k (behind K0t and K0m), into the
// localiser's ranges; a car that is not running keeps its last scan
template <bool WALLS>
static void launch_localiser_scan(mpmpc_handle h, Slot& sl, int B, const StepPlan& p, WallView wv) {
  hipLaunchKernelGGL(mpmpc_lidar_scan_running_kernel<WALLS>, dim3(B), dim3(K0L_THREADS), 0, sl.stream, p.map, B, h->ro.pose.get(),
                     h->ro.alive.get(), p.discs ? h->obs.obst_off.get() : nullptr, h->obs.obst_discs.get(), h->lc.n_beams,
                     h->lc.angles.get(), h->lc.range, h->lc.ranges.get(), wv);
}
static void enqueue_localiser_scan(mpmpc_handle h, Slot& sl, int B, const StepPlan& p) {
  if (p.walls) launch_localiser_scan<true>(h, sl, B, p, h->obs.wall_view());
  else launch_localiser_scan<false>(h, sl, B, p, WallView{nullptr, nullptr, nullptr});
}

// K3l: the fix of every running car; the last step's command is u or - delaying - in the register, as K3e takes it
static void enqueue_scan_localise(mpmpc_handle h, Slot& sl, int B, const StepPlan& p, const LocView& lv) {
  hipLaunchKernelGGL(mpmpc_scan_localise_kernel, dim3(B), dim3(LC_THREADS), loc_lds(lv.set.T, lv.n_beams), sl.stream, p.map, B,
                     h->cfg.wheelbase, h->ro.Ts, h->ro.pose.get(), h->ro.alive.get(), h->ro.u.get(), p.delaying ? h->dl.queue.get() : nullptr,
                     p.delaying ? h->dl.assumed.get() : nullptr, lv);
}

// K3e: filters K3l's fixes, else the poses K3n measured (plant), else the true ones; the last step's command is u or - delaying -
// in the register
static void enqueue_estimate(mpmpc_handle h, Slot& sl, int B, long long k, const StepPlan& p) {
  hipLaunchKernelGGL(mpmpc_estimate_kernel, dim3((B + 255) / 256), dim3(256), 0, sl.stream, B, h->cfg.wheelbase, h->ro.Ts,
                     measured_pose(h, p), h->ro.pose.get(), h->ro.alive.get(), h->ro.u.get(),
                     p.delaying ? h->dl.queue.get() : nullptr, p.delaying ? h->dl.assumed.get() : nullptr, est_view(h, k));
}

// K3d: from the estimate, else K3l's fix, else the poses K3n measured (plant), else the true ones, through the commands in flight
static void enqueue_delay_predict(mpmpc_handle h, Slot& sl, int B, const StepPlan& p) {
  hipLaunchKernelGGL(mpmpc_delay_predict_kernel, dim3((B + 255) / 256), dim3(256), 0, sl.stream, B, h->tab.n_wp, h->cfg.wheelbase, h->ro.Ts,
                     h->ro.cum.get(), h->cor.gx.get(), h->cor.gy.get(), h->cor.gpsi.get(), h->tab.kappa.get(), h->ro.s.get(),
                     localise_pose(h, p), h->ro.alive.get(), h->dl.assumed.get(), h->dl.queue.get(),
                     h->dl.pred_pose.get(), h->dl.pred_s.get(), h->dl.now.get(), h->dl.now_wp.get(), p.route);
}

// K3a; with a plant it localises on the poses K3n measured, with a localiser on K3l's fixes, with an estimator on K3e's estimate
// of either, with a delay on what K3d predicted from any of them
static void enqueue_localise(mpmpc_handle h, Slot& sl, int B, const StepPlan& p) {
  const double* s = p.delaying ? h->dl.pred_s.get() : h->ro.s.get();
  const double* pose = p.delaying ? h->dl.pred_pose.get() : localise_pose(h, p);
  hipLaunchKernelGGL(mpmpc_localise_kernel, dim3((B + 255) / 256), dim3(256), 0, sl.stream, B, h->tab.n_wp, h->cfg.N, h->cfg.circular ? 1 : 0,
                     h->ro.cum, h->cor.gx, h->cor.gy, h->cor.gpsi, s, pose, h->ro.alive, h->io.wp_id, h->io.x0, h->ro.shift, p.route);
}

// K0c: one argument pack, and one choice of its eight instantiations by (walls, looking, ahead_traffic, keeping); a step that
// keeps swaps the two buffers of the commitment's memory
template <bool WALLS, bool LEAD, bool TRAF, bool KEEP = false, class Look, class Keep = KeepNone>
static void launch_car_corridor(mpmpc_handle h, Slot& sl, int B, const StepPlan& p, Look lk, Keep km = KeepNone{}) {
  hipLaunchKernelGGL((mpmpc_car_corridor_kernel<WALLS, LEAD, TRAF, KEEP>), dim3(B), dim3(64), p.car_lds, sl.stream, p.map, p.geom, h->cfg.N,
                     h->cor.built_min_width, h->cor.built_sm, h->cor.segs, h->cor.nseg, h->cor.forced_rows(h->tab), h->cor.line_cells,
                     h->cor.line_box, p.discs ? h->obs.obst_off.get() : nullptr /* a world of walls only */, p.plan_discs, h->io.wp_id,
                     h->ro.alive.get(), h->obs.ro_flag.get(), h->io.lb, h->io.ub, p.plan_walls, p.route, lk, km);
}
static void enqueue_car_corridor(mpmpc_handle h, Slot& sl, int B, const StepPlan& p) {
  const LookView lk{p.look.car, p.look.tab};
  if (p.ahead_traffic) p.walls ? launch_car_corridor<true, true, true>(h, sl, B, p, p.look) : launch_car_corridor<false, true, true>(h, sl, B, p, p.look);
  else if (p.looking) p.walls ? launch_car_corridor<true, true, false>(h, sl, B, p, lk) : launch_car_corridor<false, true, false>(h, sl, B, p, lk);
  else if (p.keeping) {
    const KeepView km = commitment_view_and_swap(h);
    p.walls ? launch_car_corridor<true, false, false, true>(h, sl, B, p, LookNone{}, km) : launch_car_corridor<false, false, false, true>(h, sl, B, p, LookNone{}, km);
  }
  else p.walls ? launch_car_corridor<true, false, false>(h, sl, B, p, LookNone{}) : launch_car_corridor<false, false, false>(h, sl, B, p, LookNone{});
}

// K3q, in place of K3b (PLANT = false) or K3p (true)
template <bool PLANT>
static void enqueue_advance_delay(mpmpc_handle h, Slot& sl, int B, const PlantView& pv) {
  hipLaunchKernelGGL(mpmpc_advance_delay_kernel<PLANT>, dim3((B * h->cfg.N + 255) / 256), dim3(256), 0, sl.stream, B, h->cfg.N, h->cfg.wheelbase,
                     h->ro.Ts, sl.status, sl.z, h->io.cc, h->ro.counter.get(), h->ro.alive.get(), h->ro.pose.get(), h->ro.s.get(), h->ro.u.get(),
                     delay_view(h), pv);
}

// K3y, in place of K3p (DELAY = false) or K3q<true> (true)
template <bool DELAY>
static void enqueue_advance_dynamics(mpmpc_handle h, Slot& sl, int B, long long k, const StepPlan& p) {
  hipLaunchKernelGGL(mpmpc_advance_dynamics_kernel<DELAY>, dim3((B * h->cfg.N + 255) / 256), dim3(256), 0, sl.stream, B, h->cfg.N,
                     h->cfg.wheelbase, h->ro.Ts, h->tab.kappa.get(), h->io.wp_id, h->io.x0, sl.status, sl.z, h->io.cc, h->ro.counter.get(),
                     h->ro.alive.get(), h->ro.pose.get(), h->ro.s.get(), h->ro.u.get(), p.route, DELAY ? delay_view(h) : DelayView{},
                     plant_view(h, k), dynamics_view(h));
}

// K3b, or - with a plant - K3p in its place, or - with a delay - K3q in place of either, or - with dynamics - K3y in place of K3p / K3q
static void enqueue_advance(mpmpc_handle h, Slot& sl, int B, long long k, const StepPlan& p) {
  if (p.dynamic) {
    p.delaying ? enqueue_advance_dynamics<true>(h, sl, B, k, p) : enqueue_advance_dynamics<false>(h, sl, B, k, p);
    return;
  }
  const dim3 grid((B * h->cfg.N + 255) / 256);
  if (p.delaying)
    p.plant ? enqueue_advance_delay<true>(h, sl, B, plant_view(h, k)) : enqueue_advance_delay<false>(h, sl, B, PlantView{});
  else if (p.plant)
    hipLaunchKernelGGL(mpmpc_advance_plant_kernel, grid, dim3(256), 0, sl.stream, B, h->cfg.N, h->cfg.wheelbase, h->ro.Ts, h->tab.kappa.get(),
                       h->io.wp_id, h->io.x0, sl.status, sl.z, h->io.cc, h->ro.counter.get(), h->ro.alive.get(), h->ro.pose.get(), h->ro.s.get(),
                       h->ro.u.get(), p.route, plant_view(h, k));
  else
    hipLaunchKernelGGL(mpmpc_advance_kernel, grid, dim3(256), 0, sl.stream, B, h->cfg.N, h->cfg.wheelbase, h->ro.Ts, h->tab.kappa, h->io.wp_id,
                       h->io.x0, sl.status, sl.z, h->io.cc, h->ro.counter, h->ro.alive, h->ro.pose, h->ro.s, h->ro.u, p.route);
}

// K3r, write: everything else of the record, after the cars drove
static void enqueue_record_write(mpmpc_handle h, Slot& sl, int B, const StepPlan& p, char* rec) {
  const int N = h->cfg.N;
  const RoRecSrc src{h->ro.alive, h->rec.ain, h->io.wp_id, sl.status, h->ro.counter, h->io.x0, h->ro.u, h->io.cc, sl.z, h->cor.gx, h->cor.gy,
                     h->cor.gtrig, p.per_car ? h->io.ub : h->tab.ub_tab, p.per_car ? h->io.lb : h->tab.lb_tab,
                     p.per_car ? (long long)N : (long long)h->tab.n_cols, p.per_car ? 1 : 0, COR_TRIG, N, h->tab.n_wp, h->cfg.circular ? 1 : 0,
                     p.route};
  hipLaunchKernelGGL(mpmpc_record_write_kernel, dim3((unsigned)(((long)B * h->rec.lay.entries + 255) / 256)), dim3(256), 0, sl.stream, B, src,
                     rec, h->rec.lay);
}

// K3r, chain: the pose chain of the step behind the record, from the buffers of the features in force at this step (the others'
// groups are empty: a null first pointer); only when a chain bit is selected
static void enqueue_record_chain(mpmpc_handle h, Slot& sl, int B, const StepPlan& p, char* chain) {
  const size_t mb = (size_t)h->cfg.max_batch;
  RoChainSrc src{};
  src.a_in = h->rec.ain;
  if (p.plant) { src.act = h->pl.act; src.meas = h->pl.meas; }
  if (p.delaying) { src.queue = h->dl.queue; src.pred_pose = h->dl.pred_pose; src.pred_s = h->dl.pred_s; src.now = h->dl.now; }
  if (p.estimating) { src.est = h->es.est; src.cov = h->es.cov; src.used = h->es.count; }
  if (p.localising) {
    src.fix = h->lc.fix; src.prior = h->lc.prior; src.ranges = h->lc.ranges;
    src.cand = h->lc.out; src.score = h->lc.out + mb; src.hits = h->lc.out + 2 * mb;
  }
  hipLaunchKernelGGL(mpmpc_record_chain_kernel, dim3((unsigned)(((long)B * h->rec.chain.entries + 255) / 256)), dim3(256), 0, sl.stream, B, src,
                     chain, h->rec.chain);
}

// what the handle remembers of a call that ran at least one step
static void step_ran(mpmpc_handle h, int B, const StepPlan& p) {
  h->obs.car_rows = h->obs.discs_live = p.per_car;
  if (p.perceiving) h->per.B = B;
  if (p.plant) h->pl.ran = true;
  if (p.delaying) h->dl.ran = true;
  if (p.dynamic) h->dy.ran = true;
  if (p.estimating) h->es.ran = true;
  if (p.localising) h->lc.ran = true;
  if (p.keeping) h->cm.ran = true;
  h->look.ran_B = p.looking ? B : 0;
  h->look.ran_n = p.looking ? p.movers : 0;
  h->tlk.ran_B = p.ahead_traffic ? B : 0;
  h->tlk.ran_S = p.ahead_traffic ? h->obs.tr_S : 0;
  h->tlk.tracks_live = p.ahead_traffic;
}

extern "C" int mpmpc_rollout_step(mpmpc_handle h, int32_t B, int32_t n_steps) {
  if (int rc = enter(h)) return rc;
  Slot& sl = h->last();
  StepPlan p;
  if (int rc = plan_step(h, B, n_steps, p)) return rc;
  if (p.ahead_traffic && !h->tlk.tracks_live && n_steps > 0)      // no track is the last step's: every car is a frozen disc for one step
    HIP_TRY(hipMemsetAsync(h->tlk.valid, 0, sizeof(int) * (size_t)h->cfg.max_batch, sl.stream));
  for (int t = 0; t < n_steps; ++t) {
    const long long k = h->rec.ro_steps;
    char* rec = p.recording && k % h->rec.stride == 0 ? h->rec.buf + h->rec.rec_bytes() * (size_t)h->rec.count : nullptr;
    if (rec) enqueue_record_snapshot(h, sl, B, rec);                                       // K3r snapshot
    if (p.traffic) enqueue_traffic(h, sl, B, p);                                           // K0t: pose and alive as the step finds them
    const bool movers_first = p.perceiving || p.localising;
    if (movers_first && p.movers > 0) enqueue_movers(h, sl, B, k, p);                      // K0m
    if (p.perceiving) per_enqueue_step(h, sl, B, k);                                       // K0s
    if (p.plant) plant_enqueue_measure(h, sl, B, k);                                       // K3n
    if (p.localising) {
      const LocView lv = loc_view(h, k);
      if (lv.scheduled) enqueue_localiser_scan(h, sl, B, p);                               // K0l: pose k in world k
      enqueue_scan_localise(h, sl, B, p, lv);                                              // K3l
    }
    if (p.estimating) enqueue_estimate(h, sl, B, k, p);                                    // K3e
    if (p.delaying) enqueue_delay_predict(h, sl, B, p);                                    // K3d
    enqueue_localise(h, sl, B, p);                                                         // K3a
    if (!movers_first && p.movers > 0) enqueue_movers(h, sl, B, k, p);                     // K0m
    if (p.auditing) aud_enqueue_step(h, sl, B, k, p.per_car);                              // K0f: pose k in world k
    if (p.looking) look_enqueue_step(h, sl, B, k, p.map, p.geom, p.path, p.route);         // K0h
    if (p.ahead_traffic) tlk_enqueue_horizon(h, sl, B, p.map);                             // K0ht
    if (p.per_car) enqueue_car_corridor(h, sl, B, p);                                      // K0c
    if (int rc = launch_solve(h, sl, B, true, false)) return rc;                           // (the plant step reads z and the status only)
    enqueue_advance(h, sl, B, k, p);                                                       // K3b / K3p / K3q / K3y
    if (p.ahead_traffic) tlk_enqueue_tracks(h, sl, B, p.map, p.route);                     // K3t: this step's plans, for the next one's K0ht
    if (rec) {
      enqueue_record_write(h, sl, B, p, rec);                                              // K3r write
      if (h->rec.chain.bytes > 0) enqueue_record_chain(h, sl, B, p, rec + h->rec.lay.bytes);  // K3r chain
      ++h->rec.count;
    }
    ++h->rec.ro_steps;
  }
  HIP_TRY(hipGetLastError());
  if (n_steps > 0) step_ran(h, B, p);
  return MPMPC_OK;
}
