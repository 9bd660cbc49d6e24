"""Pose projection (mpmpc_project) and re-routing the cars of a running rollout (mpmpc_rollout_reroute / mpmpc_rollout_routes).

The oracle of the projection is the numpy restatement below (np_project): neither csrc/project_core.hpp nor its CPU twin.  It
forms dx*dx + dy*dy unfused, masks with np.where and takes np.argmin, which returns the first minimum.

Tolerances.  wp, dist and s are compared array_equal: + - * sqrt and fmod are exact or correctly rounded on both sides, s is a
table entry.  x0 to 1e-12: e_y = cos * dy - sin * dx with host and device libm a few ulp apart and |dx|, |dy| of at most tens of
metres bounds the difference near 1e-14; 1e-12 is that with two decades of margin.  A rollout after a re-route against the host
detour: wp_id, status, alive, counter equal, every real to 1e-8 - the device-against-host rollout bound of DESIGN (K3).

Fixture routes as in tests/test_routes.py, from the committed Sim_Track lap: L = the lap (200 waypoints, circular), A = rows
0 .. 119 (open), Bo = rows 100 .. 199 (open), S = rows 0 .. 19 (circular); Real_Track's open 302-waypoint path; crafted routes
on integer coordinates, where d2 is exact and ties are real ties."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import scenarios
import twins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = -1, -3
PI = np.pi


_d, _i = T._d, T._i


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def twin():
    """The CPU twin of the projection and of the re-route (tests/emul_project)."""
    return twins.project()


SPANS = {"L": (0, 200, 1), "A": (0, 120, 0), "Bo": (100, 200, 0), "S": (0, 20, 1)}      # rows [lo, hi) of the lap, circular


class Routes:
    """Some of the fixture routes (the helper of tests/test_routes.py, restated): each route's own tables and their concatenation."""

    def __init__(self, track, names, n_cols=30):
        self.names = list(names)
        self.P = len(self.names)
        self.circular = np.array([SPANS[k][2] for k in self.names], np.int32)
        self.own = []
        for k in self.names:
            lo, hi, _ = SPANS[k]
            cum = np.cumsum(track.segment_lengths)[lo:hi]
            self.own.append(dict(kappa=track.kappa[lo:hi].copy(), v_ref=track.v_ref[lo:hi].copy(), ds_next=track.ds_next[lo:hi].copy(),
                                 ub=np.ascontiguousarray(track.ub_free[lo:hi, :n_cols]), lb=np.ascontiguousarray(track.lb_free[lo:hi, :n_cols]),
                                 x=track.x[lo:hi].copy(), y=track.y[lo:hi].copy(), psi=track.psi[lo:hi].copy(), cum_lengths=cum - cum[0]))
        self.all, self.first = mpmpc.concat_routes(self.own)
        self.n = np.diff(self.first)


@pytest.fixture(scope="module")
def track():
    return scenarios.sim_track()


@pytest.fixture(scope="module")
def real():
    t = scenarios.real_track()
    return dict(x=np.ascontiguousarray(t.x), y=np.ascontiguousarray(t.y), psi=np.ascontiguousarray(t.psi),
                cum_lengths=np.cumsum(t.segment_lengths))


# ------------------------------------------------------------------------------------------------------------ the oracle
def np_project(tab, poses, max_heading):
    """The law of include/mpmpc.h for ONE route (dict x, y, psi, cum_lengths) and poses [B, 3] -> dict wp, dist, x0, s ([B, ...])"""
    x, y, psi, cum = (np.asarray(tab[k], float) for k in ("x", "y", "psi", "cum_lengths"))
    poses = np.asarray(poses, float).reshape(-1, 3)
    px, py, pp = poses[:, 0:1], poses[:, 1:2], poses[:, 2:3]
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = px - x[None], py - y[None]
        d2 = dx * dx + dy * dy
        t = np.fmod(pp - psi[None] + PI, 2 * PI)
        t = np.where(t < 0, t + 2 * PI, t)
        e = t - PI
        ok = (np.abs(e) <= max_heading) & np.isfinite(poses).all(1)[:, None]
        wp = np.argmin(np.where(ok, d2, np.inf), 1)
        none = ~ok.any(1)
        r = np.arange(poses.shape[0])
        e_y = np.cos(psi[wp]) * (poses[:, 1] - y[wp]) - np.sin(psi[wp]) * (poses[:, 0] - x[wp])
        out = dict(wp=np.where(none, -1, wp).astype(np.int32), dist=np.where(none, np.inf, np.sqrt(d2[r, wp])),
                   x0=np.where(none[:, None], np.nan, np.stack([e_y, e[r, wp], np.zeros(r.size)], 1)), s=np.where(none, np.nan, cum[wp]))
    return out


def same_projection(got, want, where):
    assert np.array_equal(got["wp"], want["wp"]), (where, np.flatnonzero(got["wp"] != want["wp"])[:8])
    assert np.array_equal(got["dist"], want["dist"]), where
    assert np.array_equal(got["s"], want["s"], equal_nan=True), where
    assert np.array_equal(np.isnan(got["x0"]), np.isnan(want["x0"])), where
    d = np.abs(got["x0"] - want["x0"])
    assert not d.size or np.isnan(d).all() or np.nanmax(d) <= 1e-12, (where, np.nanmax(d))


def twin_project(twin, tab, poses, first=None, cand=None, max_heading=PI):
    """mpmpc.project's signature and result on the CPU twin; raises mpmpc.MpmpcError with the library's code"""
    x, y, psi, cum = (np.ascontiguousarray(tab[k], float) for k in ("x", "y", "psi", "cum_lengths"))
    poses = np.ascontiguousarray(poses, float).reshape(-1, 3)
    B = poses.shape[0]
    f = None if first is None else np.ascontiguousarray(first, np.int32)
    P = 0 if f is None else f.size - 1
    c = None if cand is None else np.ascontiguousarray(cand, np.int32).reshape(B, -1)
    K = max(P, 1) if c is None else c.shape[1]
    out = dict(wp=np.zeros((B, K), np.int32), dist=np.zeros((B, K)), x0=np.zeros((B, K, 3)), s=np.zeros((B, K)))
    why = C.c_char_p(b"")
    rc = twin.project_emu(x.size, _d(x), _d(y), _d(psi), _d(cum), P, _i(f), B, _d(poses), K, _i(c), max_heading, _i(out["wp"]),
                          _d(out["dist"]), _d(out["x0"]), _d(out["s"]), C.byref(why))
    if rc != 0:
        raise mpmpc.MpmpcError("mpmpc error %d: %s" % (rc, why.value.decode()))
    return out


def device_project(_, tab, poses, first=None, cand=None, max_heading=PI):
    return mpmpc.project(tab["x"], tab["y"], tab["psi"], tab["cum_lengths"], poses, first=first, cand=cand, max_heading=max_heading)


def solo(out):
    """[B, 1, ...] of a one-route call -> [B, ...]"""
    return {k: v[:, 0] for k, v in out.items()}


BACKENDS = [pytest.param(twin_project, id="twin"), pytest.param(device_project, id="device", marks=pytest.mark.gpu)]


# ------------------------------------------------------------------------------------------------------------ test 1: the law
def track_poses(tab, seed):
    """every waypoint displaced laterally by 0, +-0.1, +-0.3 m with heading noise of +-0.3 rad, then 64 uniform poses over the
    map and beyond it (far from any route)"""
    rng = np.random.default_rng(seed)
    x, y, psi = tab["x"], tab["y"], tab["psi"]
    poses = [np.stack([x - e * np.sin(psi), y + e * np.cos(psi), psi + rng.uniform(-0.3, 0.3, x.size)], 1) for e in (0.0, 0.1, -0.1, 0.3, -0.3)]
    w, h = x.max() - x.min(), y.max() - y.min()
    poses.append(np.stack([rng.uniform(x.min() - w, x.max() + w, 64), rng.uniform(y.min() - h, y.max() + h, 64), rng.uniform(-4, 4, 64)], 1))
    return np.concatenate(poses)


@pytest.mark.parametrize("project", BACKENDS)
def test_projection_law_against_numpy(project, twin, track, real):
    """Test 1: L (circular lap) and Real_Track (open), gates pi and pi / 2."""
    for name, tab in (("L", Routes(track, ["L"]).own[0]), ("Real_Track", real)):
        poses = track_poses(tab, 5)
        for gate in (PI, PI / 2):
            got, want = solo(project(twin, tab, poses, max_heading=gate)), np_project(tab, poses, gate)
            print("%s, gate %.3f: %d poses, %d on no waypoint, max dist %.3f" % (name, gate, poses.shape[0], (want["wp"] < 0).sum(),
                                                                            want["dist"][want["wp"] >= 0].max()))
            same_projection(got, want, (name, gate))
            assert (want["wp"] >= 0).sum() > poses.shape[0] // 2
        # the undisplaced waypoints project on themselves, at distance 0, with s the table entry
        n = tab["x"].size
        on = np_project(tab, poses[:n], PI)
        assert np.array_equal(on["wp"], np.arange(n)) and not on["dist"].any() and np.array_equal(on["s"], tab["cum_lengths"])


# ------------------------------------------------------------------------------------------------------------ test 2: crafted shapes
def line_route(n):
    """waypoints 2 j along the x axis, heading 0: neighbours 2 apart"""
    j = np.arange(n, dtype=float)
    return dict(x=2 * j, y=np.zeros(n), psi=np.zeros(n), cum_lengths=2 * j)


def rows_route(n):
    """64 waypoints per row, rows 4 apart: waypoints j and j + 64 are vertical neighbours"""
    j = np.arange(n)
    return dict(x=2.0 * (j % 64), y=4.0 * (j // 64), psi=np.zeros(n), cum_lengths=2.0 * j)


def hairpin_route(n):
    """the line with its last waypoint moved next to the first"""
    t = line_route(n)
    t["x"][n - 1], t["y"][n - 1] = 0.0, 4.0
    return t


@pytest.mark.parametrize("project", BACKENDS)
def test_ties_go_to_the_lowest_index(project, twin):
    """Test 2: poses equidistant from two waypoints - neighbouring lanes (j, j + 1; 63 and 64 among them: the last lane of one stride
    and the first of the next), the same lane in successive strides (j, j + 64), and 0 and n - 1 - at n = 2, 63, 64, 65, 128, 130."""
    for n in (2, 63, 64, 65, 128, 130):
        tab = line_route(n)
        j = np.arange(n - 1)
        poses = np.stack([2.0 * j + 1, np.zeros(j.size), np.zeros(j.size)], 1)
        got = solo(project(twin, tab, poses))
        assert np.array_equal(got["wp"], j) and np.array_equal(got["dist"], np.ones(j.size)) and np.array_equal(got["s"], 2.0 * j), n
        same_projection(got, np_project(tab, poses, PI), ("line", n))
        if n > 64:
            tab = rows_route(n)
            j = np.arange(n - 64)
            poses = np.stack([tab["x"][j], tab["y"][j] + 2.0, np.zeros(j.size)], 1)
            got = solo(project(twin, tab, poses))
            assert np.array_equal(got["wp"], j) and np.array_equal(got["dist"], np.full(j.size, 2.0)), n
            same_projection(got, np_project(tab, poses, PI), ("rows", n))
        tab = hairpin_route(n)
        got = solo(project(twin, tab, np.array([[0.0, 2.0, 0.0]])))
        assert got["wp"].tolist() == [0] and got["dist"].tolist() == [2.0], n
        same_projection(got, np_project(tab, [[0.0, 2.0, 0.0]], PI), ("hairpin", n))
        # ... and nearer to the last waypoint it wins: the tie was real
        assert solo(project(twin, tab, np.array([[0.0, 2.5, 0.0]])))["wp"].tolist() == [n - 1], n


def crossing_route(k=40):
    """two branches that cross at (0, 0): along the x axis with heading 0 (waypoints 0 .. 2 k), then along the y axis with
    heading 2 (waypoints 2 k + 1 .. 4 k + 1).  The crossing is waypoint k of the first and k of the second."""
    a = np.arange(-k, k + 1, dtype=float)
    n = a.size
    return dict(x=np.concatenate([a, np.zeros(n)]), y=np.concatenate([np.zeros(n), a]), psi=np.concatenate([np.zeros(n), np.full(n, 2.0)]),
                cum_lengths=np.arange(2 * n, dtype=float)), k, n + k


@pytest.mark.parametrize("project", BACKENDS)
def test_heading_gate_and_pose_that_is_nowhere(project, twin):
    """Test 2: a route that crosses itself - at the crossing the pose's heading picks the branch at pi / 2 and the lower index wins at
    pi; a heading that fails the gate everywhere, NaN and inf pose components give wp = -1, dist = +inf, x0 = s = NaN."""
    tab, first_branch, second_branch = crossing_route()
    poses = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0]])
    assert solo(project(twin, tab, poses, max_heading=PI / 2))["wp"].tolist() == [first_branch, second_branch]
    assert solo(project(twin, tab, poses, max_heading=PI))["wp"].tolist() == [first_branch, first_branch]
    for gate in (PI / 2, PI):
        same_projection(solo(project(twin, tab, poses, max_heading=gate)), np_project(tab, poses, gate), ("crossing", gate))
    line = line_route(65)
    assert solo(project(twin, line, [[7.0, 1.0, 0.0]], max_heading=0.0))["wp"].tolist() == [3]          # |0| <= 0: eligible
    bad = [[7.0, 1.0, 3.0]] + [[v if c == 0 else 7.0, v if c == 1 else 1.0, v if c == 2 else 0.0] for v in (np.nan, np.inf, -np.inf) for c in range(3)]
    got = solo(project(twin, line, np.array(bad), max_heading=0.5))
    assert (got["wp"] == -1).all() and np.isposinf(got["dist"]).all() and np.isnan(got["x0"]).all() and np.isnan(got["s"]).all()
    same_projection(got, np_project(line, bad, 0.5), "nowhere")


@pytest.mark.parametrize("project", BACKENDS)
def test_several_candidates_per_pose(project, twin, track):
    """Test 2: K = 3 on the concatenation of L, A, Bo (cand = NULL: every route) and a cand with repeated ids that differs from car to
    car - every pair equals the solo call on that route's own tables."""
    R = Routes(track, ["L", "A", "Bo"])
    poses = track_poses(R.own[0], 9)[::7]
    B = poses.shape[0]
    alone = [solo(project(twin, R.own[p], poses, max_heading=PI / 2)) for p in range(3)]
    every = project(twin, R.all, poses, first=R.first, max_heading=PI / 2)
    assert every["wp"].shape == (B, 3) and every["x0"].shape == (B, 3, 3)
    rng = np.random.default_rng(3)
    cand = rng.integers(0, 3, (B, 4)).astype(np.int32)
    cand[::5] = cand[::5, :1]                                    # some cars name one route four times
    ragged = project(twin, R.all, poses, first=R.first, cand=cand, max_heading=PI / 2)
    for p in range(3):
        for k in every:
            assert np.array_equal(every[k][:, p], alone[p][k], equal_nan=True), (p, k)
            for c in range(4):
                m = cand[:, c] == p
                assert np.array_equal(ragged[k][m, c], alone[p][k][m], equal_nan=True), (p, k, c)
        same_projection(alone[p], np_project(R.own[p], poses, PI / 2), R.names[p])
    # row j of A for j = 100 .. 119 is Bo's local j - 100, at distance 0; A's rows below 100 lie at least a segment away
    A, Bo = R.own[1], R.own[2]
    on = np_project(Bo, np.stack([A["x"], A["y"], A["psi"]], 1), PI / 2)
    assert np.array_equal(on["wp"][100:], np.arange(20)) and not on["dist"][100:].any() and on["dist"][:100].min() >= 0.0355


# ------------------------------------------------------------------------------------------------------------ test 3: argument checks
def test_project_argument_checks_without_a_device(built_library, twin, track):
    """Test 3: what mpmpc_project refuses before it touches a device, through the C ABI (the library loads without a GPU) and on
    the twin, which runs the same checks."""
    lib = mpmpc.load_library()
    R = Routes(track, ["L", "A", "Bo"])
    t = R.all
    x, y, psi, cum = (np.ascontiguousarray(t[k], float) for k in ("x", "y", "psi", "cum_lengths"))
    pose = np.zeros((2, 3))
    out = np.zeros(8, np.int32)

    def call(n_wp=420, P=3, first=R.first, B=2, K=3, cand=None, gate=1.0, x=x):
        f = None if first is None else np.ascontiguousarray(first, np.int32)
        c = None if cand is None else np.ascontiguousarray(cand, np.int32)
        why = C.c_char_p(b"")
        rc_twin = twin.project_emu(n_wp, _d(x), _d(y), _d(psi), _d(cum), P, _i(f), B, _d(pose), K, _i(c), gate, _i(out), None, None, None, C.byref(why))
        rc = lib.mpmpc_project(0, n_wp, _d(x), _d(y), _d(psi), _d(cum), P, _i(f), B, _d(pose), K, _i(c), gate, _i(out), None, None, None)
        assert rc == rc_twin == E_ARG, (rc, rc_twin)
        assert lib.mpmpc_last_error() == why.value
        return why.value

    assert b"first[0]" in call(first=[1, 200, 320, 420])
    assert b"strictly increasing" in call(first=[0, 200, 200, 420])
    assert b"first[P]" in call(first=[0, 200, 320, 421])
    assert b"at least 2 waypoints" in call(first=[0, 200, 201, 420])
    assert b"out of range" in call(K=2, cand=[0, 1, 2, 3]) and b"out of range" in call(K=2, cand=[0, -1, 2, 1])
    assert b"out of range" in call(P=0, first=None, K=1, cand=[0, 1])          # one route: id 0 only
    assert b"every route" in call(K=2) and b"every route" in call(P=0, first=None, K=3)
    assert b"max_heading" in call(gate=-0.1) and b"max_heading" in call(gate=np.nan)
    assert b"NULL" in call(x=None)
    assert b"B >= 1" in call(B=0) and b"B >= 1" in call(K=0, cand=[0])
    assert b"2 waypoints" in call(n_wp=1, P=0, first=None, K=1)
    assert lib.mpmpc_rollout_reroute(None, 1, _i(out), 1.0, 1.0, None) == E_ARG and lib.mpmpc_rollout_routes(None, 1, _i(out)) == E_ARG
    with pytest.raises(mpmpc.MpmpcError):
        mpmpc.project(x, y, psi, cum, pose, first=R.first, cand=[[3], [0]])
    with pytest.raises(ValueError):
        mpmpc.project(x, y, psi[:-1], cum, pose)


class Twin:
    """the handle's side of a re-route on the CPU: route state + the cars' arrays"""

    def __init__(self, lib, R, max_batch=32):
        self.lib, self.R = lib, R
        self.t = lib.reroute_twin_new(int(R.first[-1]), max_batch)
        self.hdr = np.zeros(2 * max_batch, np.int32)

    def close(self):
        self.lib.reroute_twin_free(self.t)

    def why(self):
        return self.lib.reroute_twin_why(self.t)

    def set_routes(self):
        return self.lib.reroute_twin_set_routes(self.t, self.R.P, _i(self.R.first), _i(self.R.circular))

    def set_car_routes(self, route):
        r = np.ascontiguousarray(route, np.int32)
        return self.lib.reroute_twin_set_car_routes(self.t, r.size, _i(r), _i(self.hdr))

    def routes(self, B):
        out = np.full(B, -9, np.int32)
        return self.lib.reroute_twin_routes(self.t, B, _i(out)), out

    def reroute(self, route, pose, alive, s, wp_id, x0, max_dist=np.inf, max_heading=PI / 2):
        r = None if route is None else np.ascontiguousarray(route, np.int32)
        acc = np.full(alive.size, -9, np.int32)
        a = self.R.all
        rc = self.lib.reroute_twin_reroute(self.t, alive.size if r is None else r.size, _i(r), max_dist, max_heading, _d(a["x"]), _d(a["y"]), _d(a["psi"]), _d(a["cum_lengths"]),
                                           _d(pose), _i(alive), _i(self.hdr), _d(s), _i(wp_id), _d(x0), _i(acc))
        return rc, acc


def test_reroute_state_checks_without_a_device(twin, track):
    """Test 3: mpmpc_rollout_reroute's and mpmpc_rollout_routes' checks on the route state the handle owns (csrc/route_state.hpp):
    no routes, no car routes, no rollout, another B, a route id of -2 or P, negative or NaN max_dist / max_heading - and a refused call
    changes nothing."""
    R = Routes(track, ["L", "A", "Bo"])
    t = Twin(twin, R)
    B = 4
    pose, alive, s = np.zeros((B, 3)), np.ones(B, np.int32), np.zeros(B)
    wp, x0 = np.zeros(B, np.int32), np.zeros((B, 3))
    go = lambda route, **kw: t.reroute(route, pose, alive, s, wp, x0, **kw)[0]
    try:
        assert go([1] * B) == E_STATE and b"no routes set" in t.why() and t.routes(B)[0] == E_STATE
        assert t.set_routes() == 0
        assert go([1] * B) == E_STATE and b"mpmpc_set_car_routes" in t.why() and t.routes(B)[0] == E_STATE
        assert t.set_car_routes([1] * B) == 0
        assert go([1] * B) == E_STATE and b"no rollout in progress" in t.why()
        assert t.routes(B)[0] == 0 and t.routes(B)[1].tolist() == [1] * B and t.routes(B - 1)[0] == E_STATE
        assert twin.reroute_twin_rollout_init(t.t, B) == 0
        assert go([1] * (B - 1)) == E_STATE                                                  # another B
        hdr0 = t.hdr.copy()
        for bad in ([1, 2, -2, 0], [1, 3, 0, 0]):
            assert go(bad) == E_ARG and b"route id out of range" in t.why(), bad
        for kw in (dict(max_dist=-1.0), dict(max_dist=np.nan), dict(max_heading=-0.1), dict(max_heading=np.nan)):
            assert go([2] * B, **kw) == E_ARG and (b"max_dist" in t.why() or b"max_heading" in t.why()), kw
        assert go(None) == E_ARG
        assert np.array_equal(t.hdr, hdr0) and t.routes(B)[1].tolist() == [1] * B and not s.any()          # nothing changed
        assert go([-1] * B) == 0 and go([2] * B, max_dist=np.inf) == 0                       # +inf is a distance
        assert t.set_car_routes([1] * B) == 0 and go([2] * B) == E_STATE                     # set_car_routes ends the rollout
    finally:
        t.close()


def test_reroute_on_the_twin(twin, track):
    """The re-route's law without a device: 30 cars on A's rows 90 .. 119 (at the waypoints), asked onto Bo with max_dist = 0.03 -
    rows 100 .. 119 are accepted at Bo's local row - 100 with s = cum of it, rows below 100 (at least a segment, 0.0355 m, away) are
    refused and unchanged; -1 keeps; a car that is not running (every alive code) is untouched; the mirror reports the mix and
    ids local to the new routes pass the upload's check."""
    R = Routes(track, ["L", "A", "Bo"])
    A, Bo = R.own[1], R.own[2]
    t = Twin(twin, R)
    rows = np.arange(90, 120)
    B = rows.size
    try:
        assert t.set_routes() == 0 and t.set_car_routes([1] * B) == 0 and twin.reroute_twin_rollout_init(t.t, B) == 0
        pose = np.ascontiguousarray(np.stack([A["x"][rows], A["y"][rows], A["psi"][rows]], 1))
        s, wp, x0 = A["cum_lengths"][rows].copy(), rows.astype(np.int32), np.full((B, 3), 7.0)
        alive = np.ones(B, np.int32)
        dead = {12: 0, 14: -1, 16: -2, 18: -3, 20: -4, 22: -5}          # car -> alive code (rows 102 .. 112: they would be accepted)
        for i, a in dead.items():
            alive[i] = a
        route = np.full(B, 2, np.int32)
        route[[11, 13]] = -1                                              # rows 101, 103 keep A
        s0, hdr0 = s.copy(), t.hdr.copy()
        rc, acc = t.reroute(route, pose, alive, s, wp, x0, max_dist=0.03)
        assert rc == 0
        want = (rows >= 100) & (route >= 0) & (alive == 1)
        assert np.array_equal(acc, want.astype(np.int32)) and want.sum() == 12
        on = np.flatnonzero(want)
        assert np.array_equal(wp[on], rows[on] - 100) and np.array_equal(s[on], Bo["cum_lengths"][rows[on] - 100])
        assert np.array_equal(t.hdr[:2 * B].reshape(B, 2)[on], np.tile([320, -100], (on.size, 1)))
        assert np.abs(x0[on]).max() <= 1e-12                              # on the waypoint, along it
        off = np.flatnonzero(~want)
        assert np.array_equal(s[off], s0[off]) and np.array_equal(wp[off], rows[off]) and (x0[off] == 7.0).all()
        assert np.array_equal(t.hdr[:2 * B].reshape(B, 2)[off], hdr0[:2 * B].reshape(B, 2)[off])
        rc, now = t.routes(B)
        assert rc == 0 and np.array_equal(now, np.where(want, 2, 1))
        # ids local to the new routes: 85 is on Bo (85 + 10 < 100) and on A, 105 on A only
        N = 10
        assert twin.reroute_twin_check_upload(t.t, B, _i(np.where(want, 85, 105).astype(np.int32)), N) == 0
        assert twin.reroute_twin_check_upload(t.t, B, _i(np.full(B, 105, np.int32)), N) == E_ARG
        # a car sent to the route it is on snaps to its nearest waypoint
        pose[0, :2] += 0.01
        s[0] += 0.02
        rc, acc = t.reroute(np.where(np.arange(B) == 0, 1, -1).astype(np.int32), pose, alive, s, wp, x0)
        assert rc == 0 and acc.tolist() == [1] + [0] * (B - 1) and s[0] == A["cum_lengths"][90] and wp[0] == 90
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------------------ GPU: re-route
N_RO = 10


def _handle(R, B, N=N_RO):
    h = mpmpc.Handle(T.stock_config(N, max_batch=B, circular=False), mpmpc.default_settings())
    a = R.all
    h.set_path(a["kappa"], a["v_ref"], a["ds_next"])
    h.set_corridor(a["ub"], a["lb"])
    h.set_routes(R.first, R.circular)
    n = int(R.first[-1])
    h.set_path_geometry(a["x"], a["y"], a["psi"], np.zeros((n, 2)), np.zeros((n, 2)))
    return h


def _start(R, route, wp):
    o = [R.own[p] for p in route]
    s = np.array([t["cum_lengths"][w] for t, w in zip(o, wp)])
    poses = np.array([[t["x"][w], t["y"][w], t["psi"][w]] for t, w in zip(o, wp)])
    return s, poses


INT_KEYS = ("wp_id", "status", "alive", "counter")


def _same_state(a, b, idx, where):
    for k in a:
        if k in INT_KEYS:
            assert np.array_equal(a[k][idx], b[k][idx]), (where, k, a[k][idx], b[k][idx])
        else:
            d = np.abs(a[k][idx] - b[k][idx]).max() if idx.size else 0.0
            assert d <= 1e-8, (where, k, d)


@pytest.mark.gpu
def test_reroute_against_the_host_detour(track):
    """Test 4: 16 cars on A at waypoints 60 .. 105, N = 10, 5 steps, re-routed onto Bo or kept (mixed) with max_dist = 0.03, 10 more
    steps - against what a user did before: rollout_state, the numpy projection, set_car_routes, rollout_init with those s, the
    poses and plans, rollout_set_counters, 10 steps.  Cars that fail max_dist (A's rows below 100 are at least a segment from Bo)
    are refused and unchanged."""
    R = Routes(track, ["L", "A", "Bo"], n_cols=N_RO)
    B = 16
    route0 = np.ones(B, np.int32)
    wp0 = np.linspace(60, 105, B).astype(int)
    s0, poses0 = _start(R, route0, wp0)
    ask = np.where(np.arange(B) % 3 == 2, -1, 2).astype(np.int32)
    h = _handle(R, B)
    try:
        h.set_car_routes(route0)
        h.rollout_init(0.05, R.all["cum_lengths"], s0, poses0)
        h.rollout_step(5)
        before = h.rollout_state()
        acc = h.rollout_reroute(ask, max_dist=0.03)
        after = h.rollout_state()
        now = h.rollout_routes()
        h.rollout_step(10)
        got = h.rollout_state()
        # the same decision from the numpy projection of the poses the device held
        on = np_project(R.own[2], before["pose"], PI / 2)
        running = before["alive"] == 1
        want = running & (ask >= 0) & (on["wp"] >= 0) & (on["dist"] <= 0.03)
        print("alive at the re-route %s, asked %s, accepted %s, dist %s" % (before["alive"].tolist(), ask.tolist(), acc.astype(int).tolist(),
                                                                        np.round(on["dist"], 4).tolist()))
        assert np.array_equal(acc, want) and want.any() and (running & (ask >= 0) & ~want).any() and running.sum() >= B - 2
        assert np.array_equal(now, np.where(want, 2, 1))
        assert np.array_equal(after["s"][want], on["s"][want]) and np.array_equal(after["wp_id"][want], on["wp"][want])
        assert np.abs(after["x0"][want] - on["x0"][want]).max() <= 1e-12
        refused = ~want
        for k in before:          # refused, kept and not running: unchanged; accepted: everything but s, wp_id, x0
            keep = refused if k in ("s", "wp_id", "x0") else np.ones(B, bool)
            assert np.array_equal(before[k][keep], after[k][keep]), k
        # the detour on the same handle
        h.set_car_routes(route0)
        h.rollout_init(0.05, R.all["cum_lengths"], s0, poses0)
        h.rollout_step(5)
        st = h.rollout_state()
        _same_state(st, before, np.arange(B), "the same five steps")
        h.set_car_routes(np.where(want, 2, 1).astype(np.int32))
        h.rollout_init(0.05, R.all["cum_lengths"], np.where(want, on["s"], st["s"]), st["pose"], st["cc"])
        h.rollout_set_counters(st["counter"])
        h.rollout_step(10)
        detour = h.rollout_state()
    finally:
        h.close()
    _same_state(got, detour, np.flatnonzero(running), "re-route against the detour")
    assert (got["wp_id"][want] < 100).all() and (got["alive"][want] == 1).all()          # on Bo, under way
    for k in got:          # a car that was not running is where it was
        assert np.array_equal(got[k][~running], before[k][~running]), k


@pytest.mark.gpu
def test_hand_over_to_the_next_open_route(track):
    """Test 5: cars on A's rows 99 .. 106 end with alive = -2 on A.  Re-routed onto Bo after two steps (on A's rows 100 .. 109, Bo's first
    rows) they run on and finish Bo; two of them keep A.  mpmpc_rollout_routes reports the mix, and an upload with ids local to the
    new routes passes the check."""
    R = Routes(track, ["L", "A", "Bo"], n_cols=N_RO)
    B = 8
    route0 = np.ones(B, np.int32)
    s0, poses0 = _start(R, route0, np.arange(99, 99 + B))
    ask = np.where(np.arange(B) % 4 == 3, -1, 2).astype(np.int32)
    h = _handle(R, B)
    try:
        h.set_car_routes(route0)
        h.rollout_init(0.05, R.all["cum_lengths"], s0, poses0)
        h.rollout_step(40)
        end = h.rollout_state()
        assert (end["alive"] == -2).all() and (end["wp_id"] + N_RO >= 120).all()
        h.rollout_init(0.05, R.all["cum_lengths"], s0, poses0)
        h.rollout_step(2)          # (wp_id is what the last step localised, before it drove)
        mid = h.rollout_state()
        assert (mid["alive"] == 1).all() and (mid["wp_id"] >= 100).all() and (mid["wp_id"] <= 109).all()
        acc = h.rollout_reroute(ask)
        assert np.array_equal(acc, ask >= 0)
        assert np.array_equal(h.rollout_routes(), np.where(ask >= 0, 2, 1))
        h.rollout_step(150)
        end = h.rollout_state()
        on_bo = ask >= 0
        print("wp_id at the end %s, alive %s" % (end["wp_id"].tolist(), end["alive"].tolist()))
        assert (end["alive"] == -2).all()
        assert (end["wp_id"][on_bo] + N_RO >= 100).all() and (end["wp_id"][on_bo] < 100).all()          # Bo's end
        assert (end["wp_id"][~on_bo] + N_RO >= 120).all()                                               # A's end
        assert (end["s"][on_bo] > R.own[2]["cum_lengths"][85]).all()
        x0, cc = np.zeros((B, 3)), np.zeros((B, 2 * N_RO))
        h.upload(np.where(on_bo, 85, 105).astype(np.int32), x0, cc)
        with pytest.raises(mpmpc.MpmpcError, match="Reached end of path|out of range"):
            h.upload(np.full(B, 105, np.int32), x0, cc)
    finally:
        h.close()


def _world():
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "g1_path_sim_track.npz"))
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "g3_corridor.npz"))
    hh, ww = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:hh * ww].reshape(hh, ww).astype(np.int8))
    return g1, grid, float(g3["safety_margin"][0])


def _eq(a, b):
    """array_equal, NaN (an audit field of a car that was never audited) equal to NaN"""
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f")


def _close(a, b):
    """integers equal; reals NaN where the other is and within 1e-8, the rollout bound (the cars share launches with the re-routed
    ones: an instance's answer may depend on its neighbours in a packed wave, to rounding)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and (not a.size or np.isnan(a).all() or np.nanmax(np.abs(a - b)) <= 1e-8)


@pytest.mark.gpu
def test_what_a_reroute_keeps(track):
    """Test 6: audit and recorder on, the corridor built on the device.  A re-route in the middle of 8 steps leaves the audit's
    accumulators where they were and accumulating, the trace continuous (n_records unbroken, the records before it bit-equal
    to a run without it, all records of the cars that kept their route equal to it within the rollout bound), the infeasibility counters as they were, and the
    cars that are not running (alive 0 and -2 here; every code on the twin) untouched."""
    g1, grid, sm = _world()
    names = ["L", "A", "Bo"]
    R = Routes(track, names, n_cols=N_RO)
    own = []
    for k in names:
        lo, hi, _ = SPANS[k]
        own.append({key: np.ascontiguousarray(g1[key][lo:hi], float) for key in ("border_ub", "border_lb")})
    bub, blb = np.concatenate([o["border_ub"] for o in own]), np.concatenate([o["border_lb"] for o in own])
    B = 12
    route0 = np.array([1] * 10 + [0, 1], np.int32)
    wp0 = np.array(list(range(94, 104)) + [199, 108])
    s0, poses0 = _start(R, route0, wp0)
    s0[10] = R.own[0]["cum_lengths"][-1] + 0.04          # the lap is over with the first step: alive = 0
    ask = np.array([2, -1] * 5 + [2, 2], np.int32)        # car 11 reaches A's end before the re-route: alive = -2
    a = R.all

    def run(reroute):
        h = mpmpc.Handle(T.stock_config(N_RO, max_batch=B, circular=False), mpmpc.default_settings())
        try:
            h.set_path(a["kappa"], a["v_ref"], a["ds_next"])
            h.set_routes(R.first, R.circular)
            h.set_map(grid, (-1.0, -2.0), 0.005)
            h.set_path_geometry(a["x"], a["y"], a["psi"], bub, blb)
            assert h.build_corridor(N_RO, 2 * sm, sm, want_tables=False)[2] == 0
            h.set_car_routes(route0)
            h.rollout_set_audit(1, 0.12, 0.06, 0.1)
            h.rollout_record(8, plan=True, B=B)
            h.rollout_init(0.05, a["cum_lengths"], s0, poses0)
            h.rollout_step(4)
            out = dict(acc=None)
            if reroute:
                counters = np.array([3, 0, 2, 1] * 3, np.int32)
                before = h.rollout_state()
                h.rollout_set_counters(counters)
                out["audit_before"] = h.rollout_audit()
                out["acc"] = h.rollout_reroute(ask)
                out["audit_after"], after = h.rollout_audit(), h.rollout_state()
                assert np.array_equal(after["counter"], counters)
                for k in ("pose", "cc", "u", "status", "alive"):
                    assert np.array_equal(before[k], after[k]), k
                out["alive_mid"] = after["alive"]
                h.rollout_set_counters(before["counter"])          # (as the other run has them)
            assert h.rollout_recorded() == (4, 4)
            h.rollout_step(4)
            assert h.rollout_recorded() == (8, 8)
            out.update(state=h.rollout_state(), audit=h.rollout_audit(), trace=h.rollout_trace())
            return out
        finally:
            h.close()

    with_, without = run(True), run(False)
    alive_mid = with_["alive_mid"]
    assert alive_mid[10] == 0 and alive_mid[11] == -2 and (alive_mid[:10] == 1).all()
    assert np.array_equal(with_["acc"], (ask >= 0) & (alive_mid == 1)) and with_["acc"].sum() == 5
    for k in with_["audit_before"]:
        assert _eq(with_["audit_before"][k], with_["audit_after"][k]), k          # not reset
    moved = with_["acc"]
    for k, v in with_["trace"].items():
        assert v.shape[0] == 8
        assert np.array_equal(v[:4], without["trace"][k][:4], equal_nan=True), k
        assert _close(v[:, ~moved], without["trace"][k][:, ~moved]), k
    assert (with_["trace"]["wp_id"][4:, moved] < 20).all() and (with_["trace"]["alive"][4:, moved] == 1).all()          # on Bo's first rows
    au = with_["audit"]
    print("last_clearance at the re-route %s, at the end %s" % (with_["audit_before"]["last_clearance"].tolist(), au["last_clearance"].tolist()))
    assert (au["min_clearance"][alive_mid == 1] <= with_["audit_before"]["min_clearance"][alive_mid == 1]).all()
    assert (au["contact_steps"] >= with_["audit_before"]["contact_steps"]).all()
    for k in au:          # the cars that kept their route: as without a re-route
        assert _close(au[k][~moved], without["audit"][k][~moved]), k
    for k, v in with_["state"].items():
        assert _close(v[~moved], without["state"][k][~moved]), k


# ------------------------------------------------------------------------------------------------------------ test 7: BatchMPC
class _Waypoint:
    def __init__(self, x, y, psi, ub, lb):
        self.x, self.y, self.psi, self.static_border_cells = x, y, psi, (ub, lb)


class _CutPath:
    """rows lo .. hi - 1 of the committed lap with what BatchMPC reads of a ReferencePath"""

    def __init__(self, g1, track, name):
        lo, hi, circ = SPANS[name]
        self.circular, self.n_waypoints = bool(circ), hi - lo
        self._tables = (track.kappa[lo:hi].copy(), track.v_ref[lo:hi].copy(), track.ds_next[lo:hi].copy())
        self.segment_lengths = np.concatenate([[0.0], track.segment_lengths[lo + 1:hi]])
        self.waypoints = [_Waypoint(float(g1["x"][j]), float(g1["y"][j]), float(g1["psi"][j]), g1["border_ub"][j], g1["border_lb"][j])
                          for j in range(lo, hi)]
        self.length = float(self.segment_lengths.sum())

    def tables(self):
        return self._tables


@pytest.mark.gpu
def test_batch_mpc_rollout_starts_where_the_poses_project(track):
    """Test 7: BatchMPC.rollout(None, poses, ...) on L, A, Bo equals the same call with the numpy-projected s; BatchMPC.project and
    BatchMPC.reroute reach the same kernels; a pose that projects nowhere raises."""
    from MPC import BatchMPC
    from scipy import sparse
    g1, _, sm = _world()
    names = ["L", "A", "Bo"]
    R = Routes(track, names, n_cols=N_RO)
    paths = [_CutPath(g1, track, k) for k in names]
    model = types.SimpleNamespace(reference_path=paths[0], length=0.12, safety_margin=sm, Ts=0.05)
    Q, Rw, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / 0.12]), 'umax': np.array([1.0, np.tan(0.66) / 0.12])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B = 24
    rng = np.random.default_rng(12)
    route = (np.arange(B) % 3).astype(np.int32)
    wp = np.array([rng.integers(0, int(R.n[p]) - N_RO - 12) for p in route])
    e = rng.uniform(-0.02, 0.02, B)
    poses = np.array([[R.own[p]["x"][w] - d * np.sin(R.own[p]["psi"][w]), R.own[p]["y"][w] + d * np.cos(R.own[p]["psi"][w]),
                       R.own[p]["psi"][w] + 0.05] for p, w, d in zip(route, wp, e)])
    tabs = [dict(R.own[p], cum_lengths=np.cumsum(paths[p].segment_lengths)) for p in range(3)]          # (cum as BatchMPC forms it)
    want = [np_project(tabs[p], poses[i:i + 1], PI / 2) for i, p in enumerate(route)]
    s, wp = np.array([w["s"][0] for w in want]), np.array([w["wp"][0] for w in want])
    assert (wp >= 0).all()
    fleet = BatchMPC(model, N_RO, Q, Rw, QN, sc, ic, 4.0, max_batch=B, corridor=(np.ascontiguousarray(track.ub_free[:, :N_RO]), np.ascontiguousarray(track.lb_free[:, :N_RO])))
    try:
        fleet.set_routes(paths)
        fleet.set_corridor(R.all["ub"], R.all["lb"])
        on = fleet.project(poses, routes=route)
        assert np.array_equal(on["wp"][:, 0], wp) and np.array_equal(on["s"][:, 0], s)
        assert fleet.project(poses)["wp"].shape == (B, 3)
        given = fleet.rollout(s, poses, 6, routes=route)
        found = fleet.rollout(None, poses, 6, routes=route)
        assert sorted(found) == sorted(given)          # no new key
        for k in given:
            assert np.array_equal(given[k], found[k]), k
        assert (found["alive"] == 1).all()
        acc = fleet.reroute(np.where(route == 1, 0, -1))          # A's cars onto the lap they are cut from
        assert np.array_equal(acc, route == 1) and np.array_equal(fleet.handle.rollout_routes(), np.where(route == 1, 0, route))
        lost = poses.copy()
        lost[3, 0] = np.nan                                       # nowhere
        with pytest.raises(ValueError, match=r"\[3\]"):
            fleet.rollout(None, lost, 1, routes=route)
        fleet.set_routes(None)
        fleet.set_corridor(np.ascontiguousarray(track.ub_free[:, :N_RO]), np.ascontiguousarray(track.lb_free[:, :N_RO]))
        lap = np.flatnonzero(route == 0)
        one = fleet.rollout(None, poses[lap], 3)
        ref = fleet.rollout(s[lap], poses[lap], 3)
        for k in ref:
            assert np.array_equal(one[k], ref[k]), k
    finally:
        fleet.close()
