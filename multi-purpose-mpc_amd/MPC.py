"""Model predictive controller on the GPU QP path.

`MPC` keeps the constructor, attributes and `get_control()` contract of the reference's
src/MPC.py:14-257 so that src/simulation.py's body runs against it unchanged:

    mpc = MPC(car, N, Q, R, QN, StateConstraints, InputConstraints, ay_max)
    u = mpc.get_control()            # np.array([v, delta]); u[0], u[1]
    mpc.show_prediction()

On an open path (ReferencePath(..., circular=False)) `get_control()` ends the run where the reference does: when the
horizon would read past the last waypoint (wp_id + N >= n_wp) it prints "Reached end of path!" and raises
SystemExit(1) (src/reference_path.py:367-369), before any solve and whichever corridor the controller uses.

What changed is where the work happens.  The reference rebuilds dense A/B, scipy.sparse P/A and a
fresh OSQP workspace every step (src/MPC.py:61-159) and solves on one CPU thread
(src/MPC.py:183).  Here the per-waypoint tables are uploaded once, and every step sends
(waypoint id, spatial state, previous plan, corridor) through the C ABI of libmpmpc.so, where one
HIP kernel assembles the stage-blocked QP and a second one solves it (OSQP-style ADMM + certified
polish).  There is no CPU solver behind this class: without the library / a device it raises.

`BatchMPC` is the one API extension: B independent controller instances per call (scenario
sweeps, Monte-Carlo initial poses) on one device.

Weights: Q, R, QN may be any symmetric positive semidefinite matrices (scipy sparse or dense).  Like
the reference, the Hessian takes the whole matrices (src/MPC.py:150) while the cost vector uses
diag(Q), diag(R) and the whole QN (src/MPC.py:153-155).  Diagonal weights (src/simulation.py:101-103)
run the reduced-native kernels; anything else the general kernels.  3 <= N <= mpmpc.MAX_HORIZON.
"""
from __future__ import annotations

import numpy as np

import mpmpc
from spatial_bicycle_models import current_waypoint_batch, t2s_batch

PREDICTION = '#BA4A00'


def _symmetric(M, n, name):
    """a weight matrix (scipy sparse or dense) as a dense symmetric positive semidefinite array - anything else is refused"""
    D = M.toarray() if hasattr(M, "toarray") else np.asarray(M, float)
    D = np.atleast_2d(D).astype(float)
    if D.shape != (n, n):
        raise ValueError("%s must be %dx%d" % (name, n, n))
    if not np.array_equal(D, D.T):
        raise ValueError("%s must be symmetric" % name)
    if not np.all(np.isfinite(D)) or np.linalg.eigvalsh(D).min() < -1e-12 * (1.0 + np.abs(D).max()):
        raise ValueError("%s must be finite and positive semidefinite" % name)
    return D


def _make_config(model, N, Q, R, QN, StateConstraints, InputConstraints, ay_max, max_batch, device):
    rp = model.reference_path
    return mpmpc.make_config(N, _symmetric(Q, 3, "Q"), _symmetric(R, 2, "R"), _symmetric(QN, 3, "QN"),
                             StateConstraints['xmin'], StateConstraints['xmax'],
                             InputConstraints['umin'], InputConstraints['umax'], ay_max, model.length,
                             circular=rp.circular, max_batch=max_batch, device=device)


class MPC:
    def __init__(self, model, N, Q, R, QN, StateConstraints, InputConstraints, ay_max,
                 settings=None, device=0, backend=None, corridor="host"):
        """`corridor`: "host" calls ReferencePath.update_path_constraints every step like the reference
        (src/MPC.py:116-118; 5 ms of Python here, 17 ms there, and it refreshes the plotted border cells);
        "device" keeps the table of all start waypoints on the GPU (K0, rebuilt when the map's grid changes)
        and the step sends no bounds at all - the whole get_control() is then ~0.3 ms."""
        if corridor not in ("host", "device"):
            raise ValueError("corridor must be 'host' or 'device'")
        self.corridor = corridor
        self._map_version = None
        self.N = N
        self.Q, self.R, self.QN = Q, R, QN
        self.model = model
        self.nx = self.model.n_states
        self.nu = 2
        self.state_constraints = StateConstraints
        self.input_constraints = InputConstraints
        self.ay_max = ay_max
        self.current_prediction = None
        self.infeasibility_counter = 0
        self.current_control = np.zeros(self.nu * self.N)
        self.settings = settings or mpmpc.default_settings()
        self._cfg = _make_config(model, N, Q, R, QN, StateConstraints, InputConstraints, ay_max, 1, device)
        # `backend`: anything with set_path / solve like mpmpc.Handle (the tests inject the CPU
        # emulation of the kernels); the product default is the HIP library and nothing else
        self.optimizer = backend if backend is not None else mpmpc.Handle(self._cfg, self.settings)
        self._path_version = None
        self._path_stamp = None
        self.last_status = None
        self.last_solution = None

    # -- path tables follow the ReferencePath (v_ref is filled by compute_speed_profile after
    #    the controller is constructed, src/simulation.py:112-119)
    def _sync_path(self):
        rp = self.model.reference_path
        # cheap check first: compute_speed_profile bumps the version; a path without one (v_ref assigned by hand,
        # as some tests do) is compared by content
        stamp = (id(rp), getattr(rp, "tables_version", None))
        if stamp[1] is not None and stamp == self._path_stamp:
            return
        kappa, v_ref, ds = rp.tables()
        key = (kappa.tobytes(), v_ref.tobytes(), ds.tobytes())
        if key != self._path_version:
            if np.any(np.isnan(v_ref)):
                raise RuntimeError("reference path has no speed profile (call compute_speed_profile first)")
            self.optimizer.set_path(kappa, v_ref, ds)
            self._path_version = key
        self._path_stamp = stamp

    def _init_problem(self):
        """Inputs of this step's QP (the arithmetic of src/MPC.py:61-155 happens in K1 on the device)."""
        rp, m = self.model.reference_path, self.model
        self._sync_path()
        x0 = np.array(m.spatial_state[:], dtype=float)
        head = (np.array([m.wp_id], dtype=np.int32), x0[None, :], np.asarray(self.current_control, float)[None, :])
        if self.corridor == "device":
            self._sync_corridor()
            return head + (None, None)
        ub, lb, _ = rp.update_path_constraints(m.wp_id + 1, self.N, 2 * m.safety_margin, m.safety_margin)
        return head + (np.asarray(lb, float)[None, :], np.asarray(ub, float)[None, :])

    def _sync_corridor(self):
        """Device corridor table (row w = update_path_constraints(w + 1, N, 2 sm, sm)) follows the map: it is
        rebuilt (two small launches) whenever the occupancy grid differs from the one it was built from."""
        rp, grid = self.model.reference_path, self.model.reference_path.map
        version = grid.data.tobytes()
        if version == self._map_version:
            return
        if not hasattr(self.optimizer, "build_corridor"):
            raise RuntimeError("corridor='device' needs the HIP library (mpmpc.Handle)")
        wps = rp.waypoints
        self.optimizer.set_map(grid.data, grid.origin, grid.resolution)
        self.optimizer.set_path_geometry([w.x for w in wps], [w.y for w in wps], [w.psi for w in wps],
                                         [w.static_border_cells[0] for w in wps], [w.static_border_cells[1] for w in wps])
        sm = self.model.safety_margin
        self.optimizer.build_corridor(self.N, 2 * sm, sm, want_tables=False)
        self._map_version = version

    def get_control(self):
        nx, nu = self.model.n_states, 2
        self.model.get_current_waypoint()
        self.model.spatial_state = self.model.t2s(reference_state=self.model.temporal_state,
                                                  reference_waypoint=self.model.current_waypoint)
        rp = self.model.reference_path
        if not rp.circular and self.model.wp_id + self.N >= rp.n_waypoints:
            # the horizon passes the last waypoint of an open path: the reference's get_waypoint exits here
            # (src/reference_path.py:367-369 via src/MPC.py:93-94), whichever way the corridor is computed
            print('Reached end of path!')
            raise SystemExit(1)
        wp, x0, cc, lb, ub = self._init_problem()
        sol = self.optimizer.solve(wp, x0, cc, lb, ub)
        self.last_solution = sol
        self.last_status = int(sol.status[0])
        # stock OSQP hands back a usable x for "solved", "solved inaccurate" and "max iter reached";
        # only an infeasibility verdict makes the reference take its fallback branch (src/MPC.py:208)
        if self.last_status in (mpmpc.SOLVED, mpmpc.SOLVED_INACCURATE, mpmpc.MAX_ITER_REACHED):
            z = sol.z[0]
            plan = np.array(z[-self.N * nu:])
            plan[1::2] = np.arctan(plan[1::2] * self.model.length)
            self.current_control = plan
            self.current_prediction = self.update_prediction(np.reshape(z[:(self.N + 1) * nx], (self.N + 1, nx)))
            u = np.array([plan[0], plan[1]])
            self.infeasibility_counter = 0
        else:
            print('Infeasible problem. Previously predicted control signal used!')
            i = nu * (self.infeasibility_counter + 1)
            u = np.array(self.current_control[i:i + 2])
            self.infeasibility_counter += 1
        if self.infeasibility_counter == (self.N - 1):
            print('No control signal computed!')
            raise SystemExit(1)
        return u

    def update_prediction(self, spatial_state_prediction):
        """Predicted e_y per stage -> world x, y for plotting (stages 2..N-1, src/MPC.py:224-248)."""
        rp, wp0 = self.model.reference_path, self.model.wp_id
        xs, ys = [], []
        for n in range(2, self.N):
            w = rp.get_waypoint(wp0 + n)
            p = self.model.s2t(w, spatial_state_prediction[n, :])
            xs.append(p.x)
            ys.append(p.y)
        return xs, ys

    def show_prediction(self):
        if self.current_prediction is not None:
            import matplotlib.pyplot as plt
            plt.scatter(self.current_prediction[0], self.current_prediction[1], c=PREDICTION, s=30)


def _spatial_states(rp, s, poses):
    """(wp_id[B], x0[B,3]) of cars at arc lengths s and world poses on the reference path rp"""
    wp = current_waypoint_batch(rp.segment_lengths, s)
    wx = np.array([w.x for w in rp.waypoints])[wp]
    wy = np.array([w.y for w in rp.waypoints])[wp]
    wpsi = np.array([w.psi for w in rp.waypoints])[wp]
    poses = np.asarray(poses, float)
    return wp.astype(np.int32), t2s_batch(poses[:, 0], poses[:, 1], poses[:, 2], wx, wy, wpsi)


class BatchMPC:
    """B independent controllers sharing one path, weights and limits; one launch per call.  The map is shared too, except
    in rollout(..., obstacles=...), where every car adds its own obstacles to it.  set_routes gives the controller several
    paths, one per car: get_control_batch(..., routes=...) and rollout(..., routes=...)."""

    def __init__(self, model, N, Q, R, QN, StateConstraints, InputConstraints, ay_max, max_batch,
                 settings=None, device=0, corridor=None):
        self.N, self.model = N, model
        self.settings = settings or mpmpc.default_settings()
        self._cfg = _make_config(model, N, Q, R, QN, StateConstraints, InputConstraints, ay_max, max_batch, device)
        self.handle = mpmpc.Handle(self._cfg, self.settings)
        kappa, v_ref, ds = model.reference_path.tables()
        if np.any(np.isnan(v_ref)):
            raise RuntimeError("reference path has no speed profile (call compute_speed_profile first)")
        self.handle.set_path(kappa, v_ref, ds)
        self._path = model.reference_path
        self._routes = None               # set_routes: the ReferencePath of every route, else None - the one path
        self.corridor_cols = None
        self._corridor_tables = None      # host copies of a static corridor table (for the further handles of get_control_stream)
        self._stream = None
        self._ring = []                   # the further handles of get_control_stream (built like self.handle, kept in step with it)
        self._packing, self._tail_kernel = None, None
        if isinstance(corridor, str) and corridor == "device":
            self.update_corridor_from_map()
        elif corridor is not None:        # (ub, lb) tables [n_wp x >=N] of a static map
            self.handle.set_corridor(*corridor)
            self._corridor_tables = corridor

    def _handles(self):
        return [self.handle] + list(self._ring)

    def _corridor_from_map(self, h, n_cols):
        rp, m = self._path, self._path.map
        h.set_map(m.data, m.origin, m.resolution)
        if self._routes is not None:      # the concatenated geometry of the routes (set_routes)
            g = self._route_geometry
            h.set_path_geometry(g["x"], g["y"], g["psi"], g["border_ub"], g["border_lb"])
        else:
            wps = rp.waypoints
            h.set_path_geometry([w.x for w in wps], [w.y for w in wps], [w.psi for w in wps],
                                [w.static_border_cells[0] for w in wps], [w.static_border_cells[1] for w in wps])
        sm = self.model.safety_margin
        return h.build_corridor(n_cols, 2 * sm, sm, want_tables=False)[2]

    # Everything that changes what a handle solves goes through these, so that the ring of get_control_stream never works on a
    # stale corridor or stale settings (a call on `self.handle` alone reaches only the first handle of the ring).
    def _quiesce_stream(self):
        """nothing of a stream may still be in flight on a handle whose settings, packing, tail kernel or corridor change: the
        C side would settle the staged call (`settle` in mpmpc_handle.hpp) and a live get_control_stream generator would then yield fewer or
        stale batches - what is in flight is waited for and dropped, the generator ends at its next step"""
        if self._stream is not None:
            self._stream.discard()

    def set_settings(self, settings):
        self._quiesce_stream()
        self.settings = settings
        for h in self._handles():
            h.set_settings(settings)

    def set_packing(self, lanes_per_instance=0):
        self._quiesce_stream()
        self._packing = lanes_per_instance
        for h in self._handles():
            h.set_packing(lanes_per_instance)

    def set_tail_kernel(self, reduced_native=True):
        self._quiesce_stream()
        self._tail_kernel = reduced_native
        for h in self._handles():
            h.set_tail_kernel(reduced_native)

    def set_corridor(self, ub, lb):
        """a static corridor table [n_wp x >= N] for every handle of this controller"""
        self._quiesce_stream()
        for h in self._handles():
            h.set_corridor(ub, lb)
        self._corridor_tables, self.corridor_cols = (ub, lb), None

    def _close_ring(self):
        if self._stream is not None:
            self._stream.discard()
        for h in self._ring:
            h.close()
        self._ring, self._stream = [], None

    def close(self):
        self._close_ring()
        self.handle.close()

    def update_corridor_from_map(self, n_cols=None):
        """(Re)build the corridor table on the device from the path's map as it is NOW (obstacles
        added since the last call included): update_path_constraints(w + 1, n_cols, 2*sm, sm) for every
        start waypoint w (src/MPC.py:116-118, src/reference_path.py:522-648), without leaving the GPU.
        Returns the number of start waypoints whose first horizon waypoint is fully blocked.  Every handle of this
        controller - the ring of get_control_stream included - gets the new table."""
        n_cols = int(n_cols or self.N)
        if self._stream is not None:
            self._stream.discard()        # nothing of a stream may still be in flight on a handle whose table changes
        bad = [self._corridor_from_map(h, n_cols) for h in self._handles()][0]
        self.corridor_cols = n_cols
        self._corridor_tables = None
        return bad

    # --- route fleets: every car of a batch follows its own reference path (mpmpc.Handle.set_routes)
    def set_routes(self, paths, n_cols=None):
        """paths: a list of ReferencePath objects on this controller's map, each with its speed profile - the handle's path
        tables become their concatenation, and get_control_batch(..., routes=route_of_car) solves every car on its own route
        (wp_id local to it).  With corridor='device' the table is rebuilt from the map for all routes at once (a start
        waypoint's horizon stays inside its route); otherwise give set_corridor the concatenated table.  None or an empty
        list returns the controller to the one path it was made with.  rollout(..., routes=route_of_car) drives the fleet in closed
        loop, every car on its route (s is the arc length along it, wp_id comes back local to it; the warm start is off).
        get_control_stream stays single-path: it raises while routes are set."""
        self._close_ring()
        had_device_table = self.corridor_cols is not None
        if not paths:
            self._routes = None
            self.handle.set_path(*self._path.tables())          # (clears the routes)
            if had_device_table:
                self.update_corridor_from_map(n_cols or self.corridor_cols)
            return None
        tabs = []
        for rp in paths:
            kappa, v_ref, ds = rp.tables()
            if np.any(np.isnan(v_ref)):
                raise RuntimeError("a route has no speed profile (call compute_speed_profile first)")
            wps = rp.waypoints
            tabs.append(dict(kappa=kappa, v_ref=v_ref, ds_next=ds, x=[w.x for w in wps], y=[w.y for w in wps], psi=[w.psi for w in wps],
                             border_ub=[w.static_border_cells[0] for w in wps], border_lb=[w.static_border_cells[1] for w in wps]))
        cat, first = mpmpc.concat_routes(tabs)
        h = self.handle
        h.set_path(cat["kappa"], cat["v_ref"], cat["ds_next"])
        h.set_routes(first, [1 if rp.circular else 0 for rp in paths])
        self._routes, self._route_geometry, self._corridor_tables = list(paths), cat, None
        self._route_first = first
        if had_device_table:
            return self.update_corridor_from_map(n_cols or self.corridor_cols)
        h.set_path_geometry(cat["x"], cat["y"], cat["psi"], cat["border_ub"], cat["border_lb"])      # (the closed loop localises on it)
        return None

    def spatial_states(self, s, poses, routes=None):
        """(wp_id[B], x0[B,3]) from arc lengths and world poses, as get_control does per car.  routes (with set_routes): the
        route of every car - s is the arc length along it, wp_id comes out local to it."""
        if routes is not None:
            if self._routes is None:
                raise ValueError("routes need set_routes first")
            routes, s, poses = np.asarray(routes), np.asarray(s, float), np.asarray(poses, float)
            wp, x0 = np.zeros(s.size, np.int32), np.zeros((s.size, 3))
            for p in np.unique(routes):
                idx = np.flatnonzero(routes == p)
                wp[idx], x0[idx] = _spatial_states(self._routes[int(p)], s[idx], poses[idx])
            return wp, x0
        return _spatial_states(self._path, s, poses)

    # --- where poses are on the routes, and re-routing the cars of a rollout (mpmpc.project / mpmpc.Handle.rollout_reroute)
    def project(self, poses, routes=None, max_heading=np.pi / 2):
        """Project world poses [B, 3] onto the routes of set_routes, or onto the one path: the nearest waypoint whose heading
        differs from the pose's by at most max_heading, on the device.  routes: None - every route; [B] or [B, K] - the
        candidate route(s) of every pose.  -> mpmpc.project's dict: wp (local to the route, -1: none), dist, x0, s, each
        [B, K, ...]; s is the arc length rollout takes."""
        if self._routes is not None:
            g = self._route_geometry
            x, y, psi, first = g["x"], g["y"], g["psi"], self._route_first
            cum = np.concatenate([np.cumsum(p.segment_lengths) for p in self._routes])
        else:
            if routes is not None:
                raise ValueError("routes need set_routes first")
            wps = self._path.waypoints
            x, y, psi, first = [w.x for w in wps], [w.y for w in wps], [w.psi for w in wps], None
            cum = np.cumsum(self._path.segment_lengths)
        poses = np.asarray(poses, float).reshape(-1, 3)
        cand = None if routes is None else np.asarray(routes, np.int32).reshape(poses.shape[0], -1)
        return mpmpc.project(x, y, psi, cum, poses, first=first, cand=cand, max_heading=max_heading, device=self._cfg.device)

    def reroute(self, routes, max_dist=np.inf, max_heading=np.pi / 2):
        """Re-route the cars of the rollout the handle holds (after rollout(..., routes=...), before further
        handle.rollout_step calls): routes[i] >= 0 puts running car i on that route of set_routes, at the waypoint its pose
        projects on, if that lies within max_dist and max_heading; -1 keeps its route.  The rollout's state stays on the
        device and the rollout goes on.  -> accepted, bool [B]."""
        if self._routes is None:
            raise ValueError("reroute needs set_routes first")
        return self.handle.rollout_reroute(routes, max_dist, max_heading)

    def rollout(self, s, poses, n_steps, cc0=None, obstacles=None, record=None, movers=None, traffic=None, audit=None,
                walls=None, perception=None, routes=None, lookahead=None, plant=None, delay=None, estimator=None, localiser=None,
                dynamics=None, commitment=None):
        """Drive B cars `n_steps` control steps on the device (localise, assemble, solve, fallback,
        plant update: the loop of src/simulation.py:134-140) and return the final state dict
        (s, pose, cc, wp_id, x0, u, status, counter, alive).  Needs a corridor table.
        s: the cars' arc lengths, or None - every car starts where its pose projects on its route (project with
        max_heading = pi / 2: s is the arc length of that waypoint); a car that projects on no waypoint raises ValueError.
        obstacles: None (every car drives the path's map) or a length-B list of lists of Obstacle - car b drives the
        path's map with ITS obstacles added (Map.add_obstacles), its corridor rebuilt on the device every step; needs
        corridor='device' (the last update_corridor_from_map's map is the base every car's obstacles are added to).
        movers: None or a length-B list of lists of movers.Mover - car b's moving obstacles (a straight line, or along the
        reference path, at a constant speed), advanced on the device every step; combines with `obstacles` (together at
        most 64 per car) and needs corridor='device' as well.  movers.mover_discs gives their discs at any step index.
        traffic: None or a traffic.Traffic - the cars of a group see each other as discs (the nearest `slots` cars within
        `range`), from the fleet's own poses, every step on the device; combines with `obstacles` and `movers` (together at
        most 64 per car) and needs corridor='device' as well.  traffic.traffic_discs gives the discs of any state.
        walls: None or a length-B list of lists of boundaries ((x0, y0), (x1, y1)) in world coordinates - car b drives the
        path's map with ITS boundaries added (Map.add_boundary); combines with the other three (at most 16 walls per car)
        and needs corridor='device' as well.
        alive: 1 running, 0 lap finished (s >= length), -1 ended after N - 1 consecutive infeasible steps
        (src/MPC.py:218-220), -2 ended at the end of an open path (wp_id + N >= n_wp, where the reference's
        get_waypoint exits: src/reference_path.py:367-369; wp_id and x0 are that step's, the car is not driven),
        -3 (obstacles) no free segment at the first horizon waypoint of the car's world (the reference raises in
        update_path_constraints), -4 (obstacles) a border line of the car's world has more than 8 free segments (a
        limit of this library); for -3 / -4 too wp_id and x0 are that step's and the car is not driven, -5 (audit with
        stop=True) the car's footprint touched its world at that step's pose; the car is not driven either.
        audit: None - no audit; a footprint.Footprint - every step tests the rectangle of every running car, at the pose the
        step finds it at, against the car's world of that step (the map of corridor='device' plus its obstacles, movers and
        traffic discs) on the device, and the returned dict also holds "audit": rollout_audit().
        perception: None - every car knows its whole world from step 0; a perception.Perception - every step every running
        car scans its true world with the lidar (K0s) and its corridor is built from the base map plus what it has seen so
        far (static obstacles and walls once seen, a mover for `hold` steps after it was last seen, traffic while seen);
        the audit and rollout_scan keep judging the true world.  Needs corridor='device'; the returned dict also holds
        "perception": rollout_perception() (None when no step perceived: no per-car world, or n_steps = 0).
        lookahead: None - every column of a car's horizon is built against its movers' discs of the current step; a
        lookahead.Lookahead - column c sees them at step k + lead_c, lead_c = min(floor(t_c / Ts), max_lead) with t_c the
        expected arrival time summed over the waypoints in between (default table: ds_next / v_ref of the path or routes in
        force), K0h on the device every step.  Static obstacles and walls are not anticipated; under perception a
        car anticipates the movers it currently knows.  Needs corridor='device'; handle.rollout_lookahead() returns the
        last step's leads and discs.  Lookahead(..., traffic=True) together with `traffic`: column c also sees the cars in the
        car's traffic slots where their own plans of the step before put them at step k + lead_c (K3t, K0ht;
        csrc/traffic_lookahead_core.hpp); handle.rollout_tracks() and handle.rollout_lookahead_traffic() return the plan
        tracks and the slots' horizon discs of the last step.
        plant: None - every car drives the controller's own model, exactly; a plant.Plant - the true vehicle of every car
        (gains, steering offset, wheelbase scale, actuator lags, steering rate limit, noise on the commands and on the pose
        the controller localises on; per car, K3n / K3p on the device, csrc/plant_core.hpp).  Needs no corridor='device'.  The
        controllers see the MEASURED pose: wp_id / x0, and through them the plan and s (wheel odometry on the measured
        spatial state - s drifts from the true arc length; `reroute` onto a car's own route relocalises it).  Everything
        else keeps the TRUE pose, "pose" of the returned dict: the audit, rollout_scan, perception, traffic and its plan
        tracks, the recorder's pose and `reroute`.  The returned dict also holds "plant": handle.rollout_plant() - act, meas,
        ey_max, ey_sq, steps (None when n_steps = 0).
        delay: None - a command reaches the wheels in the step that issues it; a delay.Delay - per car, the command issued at
        step k reaches the wheels at step k + steps, and the controller predicts its pose through the `assumed` commands in
        flight with its own model and plans from there (K3d / K3q on the device, csrc/delay_core.hpp).  Combines with `plant`
        (the prediction starts from the measured pose, the delayed command drives the plant); not with `lookahead`
        (ValueError).  wp_id / x0 of the returned dict belong to the PREDICTED pose, "pose" and everything that senses or
        judges the car stay true.  The returned dict also holds "delay": handle.rollout_delay() - queue, pred_pose, pred_s, now
        (None when n_steps = 0).
        dynamics: None - the plant (if any) drives a kinematic car; a dynamics.Dynamics - per car, mass, yaw inertia, tyres with
        slip and a friction limit and a speed controller with a gain and traction (K3y on the device, csrc/dynamics_core.hpp),
        behind the plant's actuators; without `plant` an identity plant.Plant() is put in force (and "plant" is returned too).
        Combines with `delay`; the controller, the estimator and the delay's prediction keep the kinematic model.  The returned
        dict also holds "dynamics": handle.rollout_dynamics() - state, dyn_steps, sat_front, sat_rear, slip_max, alat_max (None
        with n_steps = 0).  A later rollout without it has none again.
        commitment: None - every step builds a car's corridor row from nothing, as the reference does; a commitment.Commitment -
        per car, a waypoint that was in the car's horizon in the step before chooses, among its free segments, the one nearest
        to what it chose then (K0k: the KEEP instantiations of K0c, csrc/commitment_core.hpp), so that the car does not change
        sides of an obstacle in the step it reaches it.  Needs corridor='device'; with no per-car world given an empty list of
        obstacles per car is put in force (the rows then are the table's, built per car).  Not with `lookahead` (ValueError).
        The returned dict also holds "commitment": handle.rollout_commitment() - kept, switched, moved, wp, rows (None with
        n_steps = 0).  A later rollout without it has none again.
        estimator: None - the controller localises on the measured pose (plant) or the true one; an estimator.Estimator - per
        car a 3-state extended Kalman filter on the world pose in the controller's nominal model, with a measurement schedule
        (period, random dropouts), between the measurement and the controller (K3e on the device, csrc/estimator_core.hpp):
        every step it takes the model's step with the command believed executed in the last step and, when the measurement is
        available, the measured pose; the controller localises on the ESTIMATE (under `delay` it predicts from it).  Combines
        with every other option (not with an assumed delay of 8: ValueError); with no noise and nothing to estimate the
        estimate keeps the bits of the true pose.  "pose" and everything that senses or judges the car stay true.  The returned
        dict also holds "estimator": handle.rollout_estimator() - est, cov, err2_max, err2_sum, meas2_sum, head2_sum, used,
        steps (None when n_steps = 0).
        localiser: None - the pose is measured by the plant's noise model or not at all; a localiser.Localiser - one setting for
        the fleet: every scheduled step each running car scans its TRUE world with the lidar (K0l: base map, obstacles, movers,
        traffic, walls) and matches the scan against the distance field of the BASE map around dead reckoning (K0d, K3l on the
        device, csrc/localiser_core.hpp); the FIX is what `estimator` measures and what the controller localises on (the
        estimate, else the fix; under `delay` it predicts from it), so the measurement error depends on what the car can see.
        Needs corridor='device'; composes with `plant`, `delay`, `estimator`, `perception` and `routes` (not with an assumed delay
        of 8: ValueError).  A plant still measures, but nothing plans on that.  "pose" and everything that senses or judges the car
        stay true.  The returned dict also holds "localiser": handle.rollout_localiser() - fix, prior, cand, score, hits, ranges,
        err2_max, err2_sum, head2_sum, prior2_sum, steps, matched, lost, edge (None when n_steps = 0).
        record: None - nothing is recorded; True or a dict of mpmpc.Handle.rollout_record's keyword arguments (capacity,
        plan, prediction, rows, stride, plant, delay, estimator, fix, scan, chain; capacity defaults to the records `n_steps`
        yields) - the run is recorded on the device and the returned dict also holds "trace": mpmpc.Handle.rollout_trace() of
        the whole run, arrays [records, B, ...] with the state every recorded step started from, its control, status, ...
        (what src/simulation.py:117-157 logs per step).  The pose chain of every recorded step, each value what the feature's
        getter would return right after that step: plant - act, meas; delay - queue, pred_pose, pred_s, now; estimator - est,
        cov, used; fix - fix, prior, cand, score, hits; chain=True - these four; scan - ranges, the localiser's scan (needs
        `localiser`).  A group is empty (NaN; cand / score / hits -2, used -1) where its feature is off."""
        rp = self._path
        fleet = getattr(self, "_routes", None)      # (getattr: tests call rollout on stand-ins without __init__)
        if (fleet is None) != (routes is None):
            raise ValueError("rollout(routes=...) goes with set_routes: both or neither")
        if fleet is not None:
            if len(routes) != (np.asarray(s).size if s is not None else np.asarray(poses).size // 3):
                raise ValueError("routes must hold one route id per car")
            cum = np.concatenate([np.cumsum(p.segment_lengths) for p in fleet])      # each route's own, from 0, laid end to end
        else:
            cum = None      # (the one path's, taken where the rollout starts: the argument checks below come first)
        if s is None:
            on = self.project(poses, routes=None if fleet is None else np.asarray(routes).reshape(-1, 1))
            lost = np.flatnonzero(on["wp"][:, 0] < 0)
            if lost.size:
                raise ValueError("rollout(s=None): cars %s project on no waypoint of their routes" % lost[:8].tolist())
            s = on["s"][:, 0]
        if obstacles is not None:
            if self.corridor_cols is None:
                raise ValueError("per-car obstacles need corridor='device' (update_corridor_from_map)")
            if len(obstacles) != np.asarray(s).size:
                raise ValueError("obstacles must hold one list of Obstacle per car")
            discs = [rp.map.obstacle_discs(obs) for obs in obstacles]
        if movers is not None:
            if self.corridor_cols is None:
                raise ValueError("movers need corridor='device' (update_corridor_from_map)")
            if len(movers) != np.asarray(s).size:
                raise ValueError("movers must hold one list of Mover per car")
            rows = [np.array([m.row(self.model.Ts, rp.map.resolution) for m in car], float).reshape(-1, 6) for car in movers]
        if traffic is not None:
            if self.corridor_cols is None:
                raise ValueError("traffic needs corridor='device' (update_corridor_from_map)")
            if traffic.group.size != np.asarray(s).size:
                raise ValueError("traffic must hold one group per car")
        if walls is not None:
            if self.corridor_cols is None:
                raise ValueError("walls need corridor='device' (update_corridor_from_map)")
            if len(walls) != np.asarray(s).size:
                raise ValueError("walls must hold one list of boundaries per car")
            wall_cells = [rp.map.boundary_walls(w) for w in walls]
        if commitment is not None:
            if self.corridor_cols is None:
                raise ValueError("commitment needs corridor='device' (update_corridor_from_map): the rows are built per car")
            if lookahead is not None:
                raise ValueError("commitment and lookahead cannot be combined: the anticipating instantiations of the corridor "
                                 "kernel keep no memory")
            keep = commitment.keep(np.asarray(s).size)
            if all(v is None for v in (obstacles, movers, traffic, walls)):      # (a per-car world with nothing in it)
                obstacles = [[] for _ in range(np.asarray(s).size)]
                discs = [rp.map.obstacle_discs(obs) for obs in obstacles]
        if perception is not None and self.corridor_cols is None:
            raise ValueError("perception needs corridor='device' (update_corridor_from_map): the map lives on the device")
        if lookahead is not None and self.corridor_cols is None:
            raise ValueError("lookahead needs corridor='device' (update_corridor_from_map): it anticipates movers")
        if delay is not None and lookahead is not None:
            raise ValueError("delay and lookahead cannot be combined: the column leads would have to be offset by the assumed delay")
        if estimator is not None and delay is not None and np.any(delay.arrays(np.asarray(s).size)[1] >= 8):
            raise ValueError("estimator and an assumed delay of 8 cannot be combined: the command that reached the wheels in the "
                             "last step has left the register by then")
        if localiser is not None and self.corridor_cols is None:
            raise ValueError("localiser needs corridor='device' (update_corridor_from_map): the map lives on the device")
        if localiser is not None and delay is not None and np.any(delay.arrays(np.asarray(s).size)[1] >= 8):
            raise ValueError("localiser and an assumed delay of 8 cannot be combined: the command that reached the wheels in the "
                             "last step has left the register by then")
        if isinstance(record, dict) and record.get("scan") and localiser is None:
            raise ValueError("record=dict(scan=True) needs a localiser: the scan recorded is the localiser's")
        if fleet is not None:
            self.handle.set_car_routes(routes)      # (the routes' geometry went up with set_routes)
        elif getattr(self.handle, "_n_wp", None) != rp.n_waypoints:
            wps = rp.waypoints
            self.handle.set_path_geometry([w.x for w in wps], [w.y for w in wps], [w.psi for w in wps],
                                          [w.static_border_cells[0] for w in wps],
                                          [w.static_border_cells[1] for w in wps])
        self.handle.rollout_set_perception(None)      # (off first, like the other settings)
        self.handle.rollout_set_obstacles(None)       # (all off first: the settings must agree on B while they are on)
        self.handle.rollout_set_movers(None)
        self.handle.rollout_set_traffic(None)
        self.handle.rollout_set_walls(None)
        if walls is not None:
            self.handle.rollout_set_walls(wall_cells)
        if obstacles is not None:
            self.handle.rollout_set_obstacles(discs)
        if movers is not None:
            self.handle.rollout_set_movers(rows, step0=0)
        if traffic is not None:
            self.handle.rollout_set_traffic(*traffic.cells(rp.map.resolution))
        if audit is None:
            self.handle.rollout_set_audit(0)          # (off, like the other world settings)
        else:
            if self.corridor_cols is None:
                raise ValueError("the audit needs corridor='device' (update_corridor_from_map): the map lives on the device")
            self.handle.rollout_set_audit(audit.mode, audit.length, audit.width, audit.reach)
        if perception is not None:
            self.handle.rollout_set_perception(perception.angles, perception.range, perception.hold)
        if lookahead is not None:
            _, v_ref, ds = (self._route_geometry[k] for k in ("kappa", "v_ref", "ds_next")) if fleet is not None else rp.tables()
            self.handle.rollout_set_lookahead(lookahead.table(ds, v_ref), lookahead.max_lead)
            self._lookahead_set = True
        elif getattr(self, "_lookahead_set", False):      # (off again; a controller that never looked ahead calls nothing new)
            self.handle.rollout_set_lookahead(None)
            self._lookahead_set = False
        ahead_traffic = lookahead is not None and getattr(lookahead, "traffic", False)
        if ahead_traffic or getattr(self, "_lookahead_traffic_set", False):      # (the same rule for the flag)
            self.handle.rollout_set_lookahead_traffic(ahead_traffic)
            self._lookahead_traffic_set = ahead_traffic
        if dynamics is not None and plant is None:      # (K3y drives the plant's actuators: the identity plant changes no bit)
            from plant import Plant
            plant = Plant()
        if dynamics is not None:
            self.handle.rollout_set_dynamics(dynamics.params(np.asarray(s).size))
            self._dynamics_set = True
        elif getattr(self, "_dynamics_set", False):      # (off again; a controller that never had dynamics calls nothing new)
            self.handle.rollout_set_dynamics(None)
            self._dynamics_set = False
        if plant is not None:
            self.handle.rollout_set_plant(plant.params(np.asarray(s).size), plant.seed, plant.car0, plant.step0)
            self._plant_set = True
        elif getattr(self, "_plant_set", False):      # (off again; a controller that never had a plant calls nothing new)
            self.handle.rollout_set_plant(None)
            self._plant_set = False
        delay_arrays = None if delay is None else delay.arrays(np.asarray(s).size)
        est_args = None if estimator is None else (estimator.params(np.asarray(s).size), estimator.seed, estimator.car0, estimator.step0)
        if cum is None:
            cum = np.cumsum(rp.segment_lengths)
        perceived = perception is not None and int(n_steps) > 0 and any(
            v is not None for v in (obstacles, movers, traffic, walls))
        if record is None or record is False:
            self.handle.rollout_init(self.model.Ts, cum, s, poses, cc0)
            self._set_delay(delay_arrays)
            self._set_estimator(est_args)
            self._set_localiser(localiser, np.asarray(s).size)
            self._set_commitment(None if commitment is None else keep)
            self.handle.rollout_step(n_steps)
            out = self.handle.rollout_state()
            if audit is not None:
                out["audit"] = self.handle.rollout_audit()
            if perception is not None:
                out["perception"] = self.handle.rollout_perception() if perceived else None
            if plant is not None:
                out["plant"] = self.handle.rollout_plant() if int(n_steps) > 0 else None
            if delay is not None:
                out["delay"] = self.handle.rollout_delay() if int(n_steps) > 0 else None
            if dynamics is not None:
                out["dynamics"] = self.handle.rollout_dynamics() if int(n_steps) > 0 else None
            if commitment is not None:
                out["commitment"] = self.handle.rollout_commitment() if int(n_steps) > 0 else None
            if estimator is not None:
                out["estimator"] = self.handle.rollout_estimator() if int(n_steps) > 0 else None
            if localiser is not None:
                out["localiser"] = self.handle.rollout_localiser() if int(n_steps) > 0 else None
            return out
        kw = dict(record) if isinstance(record, dict) else {}
        stride = int(kw.get("stride", 1))
        kw.setdefault("capacity", max(1, -(-int(n_steps) // max(stride, 1))))
        if kw.get("scan"):      # (the record's layout takes the n_beams of the localiser in force; set again behind rollout_init)
            self._set_localiser(localiser, np.asarray(s).size)
        self.handle.rollout_record(B=np.asarray(s).size, **kw)
        try:
            self.handle.rollout_init(self.model.Ts, cum, s, poses, cc0)
            self._set_delay(delay_arrays)
            self._set_estimator(est_args)
            self._set_localiser(localiser, np.asarray(s).size)
            self._set_commitment(None if commitment is None else keep)
            self.handle.rollout_step(n_steps)
            out = self.handle.rollout_state()
            out["trace"] = self.handle.rollout_trace()
            if audit is not None:
                out["audit"] = self.handle.rollout_audit()
            if perception is not None:
                out["perception"] = self.handle.rollout_perception() if perceived else None
            if plant is not None:
                out["plant"] = self.handle.rollout_plant() if int(n_steps) > 0 else None
            if delay is not None:
                out["delay"] = self.handle.rollout_delay() if int(n_steps) > 0 else None
            if dynamics is not None:
                out["dynamics"] = self.handle.rollout_dynamics() if int(n_steps) > 0 else None
            if commitment is not None:
                out["commitment"] = self.handle.rollout_commitment() if int(n_steps) > 0 else None
            if estimator is not None:
                out["estimator"] = self.handle.rollout_estimator() if int(n_steps) > 0 else None
            if localiser is not None:
                out["localiser"] = self.handle.rollout_localiser() if int(n_steps) > 0 else None
        finally:
            self.handle.rollout_record(0, B=np.asarray(s).size)      # later rollouts are unrecorded again
        return out

    def _set_commitment(self, keep):
        """behind rollout_init, which empties the memory: the commitment of this run (Commitment.keep), or - None - off again"""
        if keep is not None:
            self.handle.rollout_set_commitment(keep)
            self._commitment_set = True
        elif getattr(self, "_commitment_set", False):      # (off again; a controller that never committed calls nothing new)
            self.handle.rollout_set_commitment(None)
            self._commitment_set = False

    def _set_delay(self, arrays):
        """behind rollout_init, which zeroes the registers: the delay of this run (Delay.arrays) with its commands in flight, or
        - None - off again"""
        if arrays is not None:
            self.handle.rollout_set_delay(*arrays)
            self._delay_set = True
        elif getattr(self, "_delay_set", False):      # (off again; a controller that never had a delay calls nothing new)
            self.handle.rollout_set_delay(None)
            self._delay_set = False

    def _set_estimator(self, args):
        """behind rollout_init, like the delay: the estimator of this run (params, seed, car0, step0), or - None - off again"""
        if args is not None:
            self.handle.rollout_set_estimator(*args)
            self._estimator_set = True
        elif getattr(self, "_estimator_set", False):      # (off again; a controller that never had an estimator calls nothing new)
            self.handle.rollout_set_estimator(None)
            self._estimator_set = False

    def _set_localiser(self, localiser, B):
        """behind rollout_init and every map or path setter, like the estimator: the localiser of this run, or - None - off again"""
        if localiser is not None:
            self.handle.rollout_set_localiser(B, **localiser.setting())
            self._localiser_set = True
        elif getattr(self, "_localiser_set", False):      # (off again; a controller that never localised calls nothing new)
            self.handle.rollout_set_localiser(0)
            self._localiser_set = False

    def rollout_scan(self, lidar):
        """Lidar scans of the cars of the last `rollout`, where it left them and in the worlds of its last step (the map
        of corridor='device' plus each car's obstacles, movers and traffic discs): lidar is a lidar_model.LidarModel ->
        ranges [B, lidar.n_measurements].  The rollout's state is untouched."""
        return self.handle.rollout_scan(lidar.measurements[0], lidar.range)

    def rollout_perception(self):
        """What the cars of the last `rollout(..., perception=Perception)` know (mpmpc.Handle.rollout_perception)."""
        return self.handle.rollout_perception()

    def rollout_audit(self):
        """The audit of the last `rollout(..., audit=Footprint)` -> dict of [B] arrays: contact_steps, first_contact,
        min_clearance, min_step, last_contact, last_clearance (mpmpc.Handle.rollout_audit)."""
        return self.handle.rollout_audit()

    def staging(self, B):
        """numpy views of the handle's page-locked staging blocks for a batch of B (mpmpc.Handle.staging): a caller that builds
        wp_id / x0 / cc_prev (/ lb / ub) in place and reads u0 / status / z in place skips the host-side copies, which are two
        thirds of get_control_batch at B = 1 024."""
        return self.handle.staging(B)

    def get_control_staged(self, B, with_rows=True, want_plan=True):
        """get_control_batch on the staging views: -> (u [B,2] = (v, delta), status [B]) as views into the staging block; the
        plan is in staging(B)["z"] (kappa entries, not yet delta) when want_plan."""
        self.handle.solve_staged(B, with_rows=with_rows, want_z=want_plan, want_y=False)
        st = self.handle.staging(B)
        return st["u0"], st["status"]

    def get_control_stream(self, batches, depth=3, want_plan=True):
        """A stream of get_control_batch calls from host buffers with `depth` of them in flight on this device
        (streamed.StreamedBatches: upload, launch and download of consecutive batches overlap).  batches: iterable of
        (wp_id, x0, cc_prev[, lb, ub]); yields (u [B,2] = (v, delta), plan [B,2N] with delta entries or None, status [B]) per
        batch, in order.  The corridor comes with each batch (lb / ub) or from the table this controller was given or built
        (corridor=(ub, lb), corridor="device" / update_corridor_from_map: every handle of the ring holds it).  Settings,
        packing and tail kernel follow this controller's set_settings / set_packing / set_tail_kernel."""
        import streamed
        if self._routes is not None:
            raise NotImplementedError("get_control_stream follows one path: routes are set (set_routes(None) returns to it)")
        if depth < 1:
            raise ValueError("depth must be >= 1")
        if self._stream is None or self._stream.depth != depth:
            # (the first handle of the ring is this controller's own; the others are built like it and carry its corridor,
            #  settings, packing and tail kernel; a ring of another depth is closed first: each handle holds output blocks and
            #  pinned staging)
            self._close_ring()
            for _ in range(depth - 1):
                h = mpmpc.Handle(self._cfg, self.settings)
                h.set_path(*self._path.tables())
                if self._corridor_tables is not None:
                    h.set_corridor(*self._corridor_tables)
                elif self.corridor_cols is not None:
                    self._corridor_from_map(h, self.corridor_cols)
                if self._packing is not None:
                    h.set_packing(self._packing)
                if self._tail_kernel is not None:
                    h.set_tail_kernel(self._tail_kernel)
                self._ring.append(h)
            self._stream = streamed.StreamedBatches(handles=self._handles())
        for sol in self._stream.map(batches, want_z=want_plan):
            plan = None
            if want_plan:
                plan = sol.z[:, -2 * self.N:].copy()
                plan[:, 1::2] = np.arctan(plan[:, 1::2] * self.model.length)
            yield sol.u0, plan, sol.status

    def get_control_batch(self, wp_id, x0, cc_prev, lb=None, ub=None, routes=None):
        """-> (u [B,2] = (v, delta), plan [B,2N] with delta entries, status [B], Solution).  routes (with set_routes): the route
        of every car, wp_id local to it; None keeps the routes of the last call."""
        if routes is not None:
            self.handle.set_car_routes(routes)
        sol = self.handle.solve(wp_id, x0, cc_prev, lb, ub)
        plan = sol.z[:, -2 * self.N:].copy()
        plan[:, 1::2] = np.arctan(plan[:, 1::2] * self.model.length)
        return sol.u0, plan, sol.status, sol
