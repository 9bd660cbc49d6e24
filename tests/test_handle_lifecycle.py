"""One handle through grow, shrink and re-set: every table, list and trace of a handle is set up small, then larger, then
small again on the SAME handle, and after each phase three rollout steps on it must equal, bit for bit, those of a fresh
handle that was given only that phase's set-up.  A plain solve on the reused handle closes it (the batch blocks after the
rollout has had them).

Phase 2 is the doubled lap: the Sim_Track lap twice as one circular path of 2 n_wp waypoints (every per-waypoint table tiled
twice, the cumulative lengths continued by the lap's length), on the map padded with occupied cells on its high-index sides,
a corridor table of N + 3 columns, three movers per car and a trace of six records."""
import numpy as np
import pytest

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
import scenarios
from map import Map, Obstacle

N, B, STEPS, TS = 10, 6, 3, 0.05
OBSTACLES = [(0.0, 0.0, 0.05), (-0.8, -0.5, 0.08), (-0.7, -1.5, 0.05), (-0.3, -1.0, 0.08), (0.27, -1.0, 0.05), (0.78, -1.47, 0.05)]


def _phase(large):
    """the whole set-up of a phase, as plain arrays"""
    tr = scenarios.sim_track()
    g1 = np.load(M.GOLDEN + "/g1_path_sim_track.npz")
    gh, gw = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:gh * gw].reshape(gh, gw).astype(np.int8))
    origin, res = tuple(g1["origin"]), float(g1["resolution"][0])
    n = g1["x"].size
    cum = np.cumsum(g1["segment_lengths"])
    path = dict(kappa=tr.kappa, v_ref=tr.v_ref, ds_next=tr.ds_next)
    geom = {k: g1[k] for k in ("x", "y", "psi", "border_ub", "border_lb")}
    starts = np.arange(B) * (n // B) + 2
    if large:
        path = {k: np.tile(v, 2) for k, v in path.items()}
        geom = {k: np.concatenate([v, v]) for k, v in geom.items()}
        cum = np.concatenate([cum, cum[-1] + tr.ds_next[-1] + cum])
        grid = np.ascontiguousarray(np.pad(grid, ((0, 7), (0, 5)), constant_values=0))      # 0 = occupied
        starts = starts + n * (np.arange(B) % 2)                                             # every other car on the second lap
    n_wp = cum.size
    assert np.all(np.diff(cum) >= 0)
    static = [Map.from_grid(grid, origin, res).obstacle_discs([Obstacle(*OBSTACLES[b])]) for b in range(B)]
    r = int(np.ceil(0.04 / res))

    def along(b, ahead, e_y, speed):
        w0 = int(starts[b])
        return (1, r, cum[(w0 + ahead) % n_wp], e_y, speed * path["v_ref"][w0] * TS, 0.0)

    def line(b, ahead):
        w = (int(starts[b]) + ahead) % n_wp
        nx, ny = -np.sin(geom["psi"][w]), np.cos(geom["psi"][w])
        return (0, r, geom["x"][w] - 0.3 * nx, geom["y"][w] - 0.3 * ny, 0.6 * nx / STEPS, 0.6 * ny / STEPS)
    if large:
        movers = [np.array([along(b, 8, 0.03, 0.5), along(b, 15, -0.04, 0.4), line(b, 12)], float) for b in range(B)]
    else:
        movers = [np.array([along(b, 8, 0.03, 0.5)], float) if b in (1, 4) else np.zeros((0, 6)) for b in range(B)]
    poses = np.stack([geom["x"][starts], geom["y"][starts], geom["psi"][starts]], 1)
    return dict(path=path, geom=geom, grid=grid, origin=origin, res=res, n_cols=N + 3 if large else N, static=static,
                movers=movers, capacity=6 if large else 3, cum=cum, s0=cum[starts], poses=poses)


def _run(h, p):
    """a phase's set-up on `h` (fresh or used), three rollout steps, everything the handle reports"""
    sm = T.safety_margin("sim")
    h.set_path(p["path"]["kappa"], p["path"]["v_ref"], p["path"]["ds_next"])
    h.set_map(p["grid"], p["origin"], p["res"])
    g = p["geom"]
    h.set_path_geometry(g["x"], g["y"], g["psi"], g["border_ub"], g["border_lb"])
    h.rollout_warm_start(False)
    h.build_corridor(p["n_cols"], 2 * sm, sm, want_tables=False)
    h.rollout_record(p["capacity"], plan=True, prediction=True, rows=True, B=B)
    h.rollout_set_obstacles(p["static"])
    h.rollout_set_movers(p["movers"])
    h.rollout_init(TS, p["cum"], p["s0"], p["poses"])
    h.rollout_step(STEPS)
    ub, lb = h.rollout_corridor()
    assert h.rollout_recorded() == (STEPS, STEPS)
    return dict(state=h.rollout_state(), ub=ub, lb=lb, discs=h.rollout_obstacles(), trace=h.rollout_trace())


def _fresh():
    return mpmpc.Handle(T.stock_config(N, max_batch=B), mpmpc.default_settings())


def _assert_same(got, ref, phase):
    for k, v in ref["state"].items():
        assert np.array_equal(got["state"][k], v), (phase, "state", k)
    assert np.array_equal(got["ub"], ref["ub"], equal_nan=True) and np.array_equal(got["lb"], ref["lb"], equal_nan=True), phase
    assert len(got["discs"]) == len(ref["discs"]) == B
    for a, b in zip(got["discs"], ref["discs"]):
        assert np.array_equal(a, b), (phase, "discs")
    assert set(got["trace"]) == set(ref["trace"])
    for k, v in ref["trace"].items():
        assert v.shape[0] == STEPS and np.array_equal(got["trace"][k], v, equal_nan=v.dtype.kind == "f"), (phase, "trace", k)


@pytest.mark.gpu
def test_one_handle_through_grow_shrink_and_reset_equals_fresh_handles():
    small, large = _phase(False), _phase(True)
    assert large["cum"].size == 2 * small["cum"].size and large["grid"].shape > small["grid"].shape
    h = _fresh()
    handles = [h]
    try:
        for phase, p in (("small", small), ("large", large), ("small again", small)):
            got = _run(h, p)
            f = _fresh()
            handles.append(f)
            ref = _run(f, p)
            f.close()
            # the phase is a rollout worth comparing: cars drive, the per-car rows are real, the movers are in the lists
            assert np.sum(ref["state"]["alive"] == 1) * 2 >= B and np.any(ref["state"]["status"] > 0), (phase, ref["state"])
            assert np.any(np.isfinite(ref["ub"])) and [len(d) for d in ref["discs"]] == [1 + len(m) for m in p["movers"]]
            _assert_same(got, ref, phase)
        # a plain solve on the handle the rollouts have used (its batch blocks were theirs), against the last fresh set-up
        tr = scenarios.sim_track()
        sc = scenarios.make(2, tr, B=B, N=N)
        f = _fresh()
        handles.append(f)
        _run(f, small)
        a = h.solve(sc.wp_id, sc.x0, sc.cc_prev, want_y=True)
        b = f.solve(sc.wp_id, sc.x0, sc.cc_prev, want_y=True)
        assert np.any(b.status > 0)
        for k in ("z", "u0", "status", "iters", "resid", "y"):
            assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), ("solve", k)
    finally:
        for x in handles:
            x.close()
