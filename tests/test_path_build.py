"""Reference paths on the device (K0p, mpmpc_path_count / mpmpc_path_build): from corner points to the tables and the static
width, for many paths at once, each in a world of its own.

CPU: the host twin (tests/emul_path: the library's own path_core.hpp, the width as the kernel's per-line code in a loop)
against the reference's own paths (golden G1, both tracks), a numpy restatement of the law - written here from the header
csrc/path_core.hpp - against the twin on seeded routes, the twin against the host class ReferencePath on the same routes and
on small crafted grids, the argument checks through the C ABI.  GPU: the device against G1, against the twin, against the
host class on the crafted grids, one ragged call, per-path worlds, ReferencePath.on_device into a device corridor.

Tolerances.  x, y, ds_next, the widths and the border cells are compared bit for bit.  psi comes from atan2 and kappa divides
a difference of two psi by ~0.05 .. 0.3: against G1 and against the host class (numpy's libm against glibc's) they get the
1e-15 / 1e-13 (length: 1e-12) that tests/test_host_path.py already uses for the host class against the same fixture.  The
device against the twin runs the same libm on the same machine: bit-equal, psi and kappa included.
A SIDE is tie-sensitive when a coordinate of its target, (t - o) / res, lies within TIE = 1e-9 cells of an integer (numpy's
cos / sin against glibc's can then move the target cell).  Computed by the restatement alone; a condition, not a tolerance."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import twins
from map import Map, Obstacle, line_aa
from reference_path import ReferencePath

bp = C.POINTER(C.c_int8)
E_ARG = -1
TIE = 1e-9
TABLES = ("x", "y", "psi", "kappa", "ds_next", "ub", "lb")
TRACKS = {"sim": dict(r_p=0.05, sd=5, mw=0.23, circular=True, n_wp=200), "real": dict(r_p=0.20, sd=5, mw=1.50, circular=False, n_wp=302)}


_d, _i, _g1 = T._d, T._i, T.g1_world


# ------------------------------------------------------------------------------------------------ fixtures and callers
def _route(track):
    g1 = _g1(track)[0]
    return np.ascontiguousarray(np.stack([g1["wp_x"], g1["wp_y"]], 1), float)


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of mpmpc_path_build (tests/emul_path)."""
    return twins.path()


def _call(fn, grid, origin, res, routes, r_p, sd, mw, circular, discs=None, walls=None, cap=None, fill=-7.0, device=None, count=None):
    """One call of mpmpc_path_build (device = an ordinal) or of the twin's path_emu_build (device = None) with full [P][cap]
    outputs, pre-filled with `fill` -> (rc, dict).  cap None: sized by `count` (the entry's own count function)."""
    lists = [np.ascontiguousarray(r, float).reshape(-1, 2) for r in routes]
    P = len(lists)
    Pa = max(P, 1)      # (a refused call with P = 0 or cap = 0 still gets arrays of one row)
    coff = np.zeros(Pa + 1, np.int32)
    coff[1:P + 1] = np.cumsum([a.shape[0] for a in lists])
    corners = np.ascontiguousarray(np.concatenate(lists)) if P else np.zeros((1, 2))
    spec = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(r_p, float), (Pa,)), np.broadcast_to(np.asarray(mw, float), (Pa,))], 1))
    ispec = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(sd), (Pa,)), np.broadcast_to(np.asarray(circular), (Pa,))], 1).astype(np.int32))
    if cap is None:
        cap = max(1, max(count(a.shape[0], _d(a), float(spec[p, 0]), int(ispec[p, 0])) for p, a in enumerate(lists)))
    doff, dflat = T.csr(discs, 3, n=P)
    woff, wflat = T.csr(walls, 4, n=P)
    rows = max(cap, 1)
    o = dict(n_wp=np.full(Pa, -7, np.int32), status=np.full(Pa, -7, np.int32), border=np.full((Pa, rows, 4), fill), length=np.full(Pa, fill))
    o.update({k: np.full((Pa, rows), fill) for k in TABLES})
    grid = np.ascontiguousarray(grid, np.int8)
    args = [grid.shape[0], grid.shape[1], grid.ctypes.data_as(bp), float(origin[0]), float(origin[1]), float(res), P, _i(coff),
            _d(corners), _d(spec), _i(ispec), _i(doff), _i(dflat), _i(woff), _i(wflat), int(cap), _i(o["n_wp"]), _i(o["status"])] + \
           [_d(o[k]) for k in TABLES] + [_d(o["border"]), _d(o["length"])]
    rc = fn(*args) if device is None else fn(int(device), *args)
    return rc, o


def _twin_build(twin, *a, **kw):
    rc, o = _call(twin.path_emu_build, *a, count=twin.path_emu_count, **kw)
    assert rc == 0
    return o


def _dev_build(*a, **kw):
    lib = mpmpc.load_library()
    rc, o = _call(lib.mpmpc_path_build, *a, count=lib.mpmpc_path_count, device=0, **kw)
    assert rc == 0, lib.mpmpc_last_error()
    return o


def _same(a, b, p=None, q=None):
    """path p of a and path q of b (None: every path of both) bit for bit over the rows both have, NaN beyond them"""
    pa, qb = (range(len(a["n_wp"])) if p is None else [p]), (range(len(b["n_wp"])) if q is None else [q])
    assert len(pa) == len(qb)
    for i, j in zip(pa, qb):
        for k in TABLES + ("border",):
            u, v = a[k][i], b[k][j]
            n = min(len(u), len(v))
            assert np.array_equal(u[:n], v[:n], equal_nan=True) and np.all(np.isnan(u[n:])) and np.all(np.isnan(v[n:])), (i, j, k)
        assert a["n_wp"][i] == b["n_wp"][j] and a["status"][i] == b["status"][j], (i, j)
        assert np.array_equal(a["length"][i], b["length"][j], equal_nan=True), (i, j)


def _against_g1(o, track):
    """T1's comparison: everything bit-equal but psi (1e-15), kappa (1e-13), length (1e-12)"""
    g1 = _g1(track)[0]
    n = TRACKS[track]["n_wp"]
    assert o["n_wp"][0] == n and o["status"][0] == 0
    for k, gk in (("x", "x"), ("y", "y"), ("ub", "ub_static"), ("lb", "lb_static")):
        assert np.array_equal(o[k][0, :n], g1[gk]), k
    m = n if TRACKS[track]["circular"] else n - 1
    assert np.array_equal(o["ds_next"][0, :m], g1["ds_next"][:m])
    assert np.array_equal(o["border"][0, :n, :2], g1["border_ub"]) and np.array_equal(o["border"][0, :n, 2:], g1["border_lb"])
    assert np.max(np.abs(o["psi"][0, :n] - g1["psi"])) <= 1e-15
    assert np.max(np.abs(o["kappa"][0, :n] - g1["kappa"])) <= 1e-13 and o["kappa"][0, 0] == 0.0
    assert abs(o["length"][0] - g1["length"][0]) <= 1e-12


# ------------------------------------------------------------------------------- the law, restated from the header
def _law(grid, origin, res, route, r_p, sd, mw, circular):
    """csrc/path_core.hpp steps 1 - 5 for one path on the base map, with numpy's own linspace-free arithmetic, mean, arctan2,
    mod, cos, sin and floor -> dict of the tables plus `tie` [n_wp, 2] (tie-sensitive sides) and `outside` (a probed cell lay
    outside the grid)"""
    H, W = grid.shape
    route = np.asarray(route, float)
    xs, ys = [], []
    for k in range(len(route) - 1):                                                            # step 1
        dx, dy = route[k + 1, 0] - route[k, 0], route[k + 1, 1] - route[k, 1]
        cnt = int(math.sqrt(dx * dx + dy * dy) / r_p)
        if cnt == 0:
            continue
        xs.extend((np.arange(cnt) * (dx / cnt) + route[k, 0]).tolist())
        ys.extend((np.arange(cnt) * (dy / cnt) + route[k, 1]).tolist())
    xs.append(float(route[-1, 0]))
    ys.append(float(route[-1, 1]))
    px = np.array([np.mean(xs[j:j + 2 * sd + 1]) for j in range(len(xs) - 2 * sd)])            # step 2
    py = np.array([np.mean(ys[j:j + 2 * sd + 1]) for j in range(len(ys) - 2 * sd)])
    n = len(px) - 1                                                                            # step 3
    sx, sy = px[1:] - px[:-1], py[1:] - py[:-1]
    dist = np.sqrt(sx * sx + sy * sy)
    psi = np.arctan2(sy, sx)
    kappa = np.zeros(n)
    kappa[1:] = (np.mod(psi[1:] - psi[:-1] + math.pi, 2 * math.pi) - math.pi) / (dist[1:] + 1e-12)
    ds = dist.copy()
    bx, by = px[0] - px[n - 1], py[0] - py[n - 1]
    ds[n - 1] = math.sqrt(bx * bx + by * by) if circular else 0.0
    length = 0.0
    for v in dist[:n - 1]:
        length += float(v)
    o = dict(n_wp=n, x=px[:n], y=py[:n], psi=psi, kappa=kappa, ds_next=ds, length=length, ub=np.zeros(n), lb=np.zeros(n),
             border=np.zeros((n, 4)), tie=np.zeros((n, 2), bool), outside=False)
    for i in range(n):
        x, y = px[i], py[i]
        cx, cy = int(np.floor((x - origin[0]) / res)), int(np.floor((y - origin[1]) / res))
        for side, s in enumerate((1.0, -1.0)):                                                 # step 4
            ang = np.mod(psi[i] + s * math.pi / 2 + math.pi, 2 * math.pi) - math.pi
            fx, fy = (x + mw * np.cos(ang) - origin[0]) / res, (y + mw * np.sin(ang) - origin[1]) / res
            o["tie"][i, side] = abs(fx - round(fx)) <= TIE or abs(fy - round(fy)) <= TIE
            tx, ty = int(np.floor(fx)), int(np.floor(fy))
            best, cell = mw, None                                                              # step 5
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    lx, ly, _ = line_aa(cx, cy, tx + di, ty + dj)
                    for qx, qy in zip(lx.tolist(), ly.tolist()):
                        out = not (0 <= qx < W and 0 <= qy < H)
                        o["outside"] = o["outside"] or out
                        if out or grid[qy, qx] == 0:
                            wx, wy = (qx + 0.5) * res + origin[0], (qy + 0.5) * res + origin[1]
                            d = math.sqrt((x - wx) * (x - wx) + (y - wy) * (y - wy))
                            if d < best:
                                best, cell = d, (wx, wy)
            if cell is None:
                cell = ((tx + 1 + 0.5) * res + origin[0], (ty + 1 + 0.5) * res + origin[1])
            (o["ub"] if side == 0 else o["lb"])[i] = best if side == 0 else -best
            o["border"][i, 2 * side:2 * side + 2] = cell
    return o


# ------------------------------------------------------------------------------------------------ the seeded routes
N_ROUTES = 12


def _seeded_routes():
    """Real_Track's corners jittered by up to 0.4 m, cut to a stretch around its second leg so that a path keeps at most 60
    waypoints: path resolution in [0.15, 0.3], sd in {0, 2, 3, 4, 7}, width in [0.8, 2.0], both circular flags"""
    c = _route("real")
    rng = np.random.default_rng(20261)
    out = []
    for k in range(N_ROUTES):
        r_p = float(rng.uniform(0.15, 0.3))
        sd = int((0, 2, 3, 4, 7)[k % 5])
        mw = float(rng.uniform(0.8, 2.0))
        want = r_p * (int(rng.integers(24, 40)) + 2 * sd)              # raw length in metres
        rest = max(want - float(np.linalg.norm(c[2] - c[1])), 2.0)
        a = c[1] + (c[0] - c[1]) / np.linalg.norm(c[0] - c[1]) * rest * 0.5
        b = c[2] + (c[3] - c[2]) / np.linalg.norm(c[3] - c[2]) * rest * 0.5
        route = np.array([a, c[1], c[2], b]) + rng.uniform(-0.4, 0.4, (4, 2))
        out.append(dict(route=route, r_p=r_p, sd=sd, mw=mw, circular=bool(k % 2)))
    return out


@pytest.fixture(scope="module")
def seeded(twin):
    """the routes, the twin's build of each (one call), the restatement of each: computed once, never changed"""
    _, grid, origin, res = _g1("real")
    rs = _seeded_routes()
    tw = _twin_build(twin, grid, origin, res, [r["route"] for r in rs], [r["r_p"] for r in rs], [r["sd"] for r in rs],
                     [r["mw"] for r in rs], [r["circular"] for r in rs])
    laws = [_law(grid, origin, res, r["route"], r["r_p"], r["sd"], r["mw"], r["circular"]) for r in rs]
    return rs, tw, laws


# ------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("track", ["sim", "real"])
def test_twin_matches_reference_paths(track, twin):
    """T1: the twin against G1, nothing left out (Real_Track: 165 sides meet nothing - the last probed target)"""
    g1, grid, origin, res = _g1(track)
    t = TRACKS[track]
    o = _twin_build(twin, grid, origin, res, [_route(track)], t["r_p"], t["sd"], t["mw"], t["circular"])
    _against_g1(o, track)
    if track == "real":
        assert int(np.sum(o["ub"][0] == t["mw"]) + np.sum(o["lb"][0] == -t["mw"])) == 165


def test_mean_is_numpys(twin):
    """step 2's sum order against np.mean on lists of every length the law admits"""
    rng = np.random.default_rng(5)
    for n in list(range(1, 128)) * 3:
        a = np.ascontiguousarray(rng.uniform(-30, 30, n) * 10.0 ** rng.integers(-3, 3))
        assert twin.path_emu_mean(_d(a), n) == np.mean(a.tolist()), n


def test_restatement_matches_twin_on_seeded_routes(seeded):
    """T2: bit-equal on everything but psi / kappa (T1's tolerances: numpy's atan2 against glibc's)"""
    rs, tw, laws = seeded
    for p, law in enumerate(laws):
        n = law["n_wp"]
        assert 2 <= n <= 60 and tw["n_wp"][p] == n and tw["status"][p] == (1 if law["outside"] else 0), p
        for k in ("x", "y", "ds_next", "ub", "lb", "border"):
            assert np.array_equal(tw[k][p, :n], law[k]), (p, k)
            assert np.all(np.isnan(tw[k][p, n:])), (p, k)
        assert tw["length"][p] == law["length"]
        assert np.max(np.abs(tw["psi"][p, :n] - law["psi"])) <= 1e-15 and np.max(np.abs(tw["kappa"][p, :n] - law["kappa"])) <= 1e-13
    assert sum(int(np.sum(law["ub"] == r["mw"])) for r, law in zip(rs, laws)) > 0      # some side met nothing


def test_twin_matches_host_class_on_seeded_routes(seeded):
    """T3: the twin against ReferencePath(...) - widths and border cells bit-equal on every side the restatement does not flag as
    tie-sensitive; at most 1 side in 1 000 may be flagged, no route may probe outside the grid"""
    rs, tw, laws = seeded
    _, grid, origin, res = _g1("real")
    m = Map.from_grid(grid, origin=list(origin), resolution=res)
    sides = flagged = 0
    for p, (r, law) in enumerate(zip(rs, laws)):
        assert not law["outside"] and tw["status"][p] == 0
        rp = ReferencePath(m, list(r["route"][:, 0]), list(r["route"][:, 1]), r["r_p"], r["sd"], r["mw"], r["circular"])
        n = rp.n_waypoints
        assert n == tw["n_wp"][p]
        assert np.array_equal(tw["x"][p, :n], [w.x for w in rp.waypoints]) and np.array_equal(tw["y"][p, :n], [w.y for w in rp.waypoints])
        assert np.max(np.abs(tw["ds_next"][p, :n] - rp.tables()[2])) <= 1e-15
        assert np.max(np.abs(tw["psi"][p, :n] - [w.psi for w in rp.waypoints])) <= 1e-15
        assert np.max(np.abs(tw["kappa"][p, :n] - [float(w.kappa) for w in rp.waypoints])) <= 1e-13
        assert abs(tw["length"][p] - rp.length) <= 1e-12
        keep = ~law["tie"]
        sides += keep.size
        flagged += int(law["tie"].sum())
        width = np.array([[w.ub, -w.lb] for w in rp.waypoints])
        cells = np.array([[w.static_border_cells[0], w.static_border_cells[1]] for w in rp.waypoints])      # [n, side, 2]
        got_w = np.stack([tw["ub"][p, :n], -tw["lb"][p, :n]], 1)
        got_c = tw["border"][p, :n].reshape(n, 2, 2)
        assert np.array_equal(got_w[keep], width[keep]) and np.array_equal(got_c[keep], cells[keep]), p
    assert flagged * 1000 <= sides, (flagged, sides)


def _bad_calls():
    """(name, keyword changes, expected words of the reason) of every MPMPC_E_ARG case of mpmpc_path_build"""
    return [("P < 1", dict(routes=[]), "P must"),
            ("fewer than 2 corners", dict(routes=[[[0.5, 0.5]]]), "at least 2 corner"),
            ("corner not finite", dict(routes=[[[0.5, 0.5], [np.nan, 0.5]]]), "not finite"),
            ("corner far off", dict(routes=[[[0.5, 0.5], [2.0 ** 31, 0.5]]]), "2^30"),
            ("path resolution", dict(r_p=0.0), "path resolution"),
            ("path resolution inf", dict(r_p=np.inf), "path resolution"),
            ("max_width", dict(mw=-1.0), "max_width"),
            ("max_width nan", dict(mw=np.nan), "max_width"),
            ("max_width cells", dict(mw=0.1 * 512.5), "512"),
            ("smoothing low", dict(sd=-1), "smoothing"),
            ("smoothing high", dict(sd=64), "smoothing"),
            ("65 discs", dict(discs=[np.tile([5, 5, 1], (65, 1))]), "64 discs"),
            ("disc leaves", dict(discs=[[[1, 1, 3]]]), "leaves the map"),
            ("17 walls", dict(walls=[np.tile([2, 2, 9, 9], (17, 1))]), "16 walls"),
            ("wall leaves", dict(walls=[[[0, 2, 9, 9]]]), "outside"),
            ("cap", dict(cap=0), "cap")]


def test_argument_checks_through_the_abi(built_library, twin):
    """T4: each MPMPC_E_ARG case is refused on the host, with a reason and the outputs untouched; mpmpc_path_count"""
    lib = mpmpc.load_library()
    grid = np.ones((32, 32), np.int8)
    base = dict(routes=[[[0.5, 0.5], [2.5, 0.6]]], r_p=0.1, sd=1, mw=0.4, circular=True, cap=64)
    for name, change, words in _bad_calls():
        kw = dict(base, **change)
        rc, o = _call(lib.mpmpc_path_build, grid, (0.0, 0.0), 0.1, device=0, **kw)
        assert rc == E_ARG and words in lib.mpmpc_last_error().decode(), (name, lib.mpmpc_last_error())
        for k, v in o.items():
            assert np.all(v == -7), (name, k)
        assert _call(twin.path_emu_build, grid, (0.0, 0.0), 0.1, **kw)[0] == E_ARG, name
    # the map's own limits, offsets that do not start at 0 or that decrease
    args = lambda coff, h=32, w=32, res=0.1: (0, h, w, grid.ctypes.data_as(bp), 0.0, 0.0, res, 2, _i(np.array(coff, np.int32)),      # noqa: E731
                                              _d(np.array([0.5, 0.5, 2.5, 0.6, 0.5, 1.5, 2.5, 1.6])), _d(np.array([0.1, 0.4, 0.1, 0.4])),
                                              _i(np.array([1, 1, 1, 0], np.int32)), None, None, None, None, 8, _i(np.zeros(2, np.int32)),
                                              _i(np.zeros(2, np.int32)), *[_d(np.zeros(64)) for _ in range(9)])
    for a, words in ((args([1, 2, 4]), "corner_offsets[0]"), (args([0, 4, 2]), "decrease"), (args([0, 2, 4], h=65535), "65534"),
                     (args([0, 2, 4], res=0.0), "resolution"), (args([0, 2, 4], res=np.nan), "resolution")):
        assert lib.mpmpc_path_build(*a) == E_ARG and words in lib.mpmpc_last_error().decode(), words
    # mpmpc_path_count: the two tracks, a route too short for its smoothing, arguments it refuses
    for track, t in TRACKS.items():
        c = _route(track)
        assert lib.mpmpc_path_count(c.shape[0], _d(c), t["r_p"], t["sd"]) == t["n_wp"] == twin.path_emu_count(c.shape[0], _d(c), t["r_p"], t["sd"])
        assert mpmpc.path_count(c, t["r_p"], t["sd"]) == t["n_wp"]
    short = np.array([[0.0, 0.0], [1.05, 0.0]])
    assert lib.mpmpc_path_count(2, _d(short), 0.1, 0) == 10 and lib.mpmpc_path_count(2, _d(short), 0.1, 4) == 2
    assert lib.mpmpc_path_count(2, _d(short), 0.1, 5) == 0 and lib.mpmpc_path_count(2, _d(short), 0.1, 63) == 0
    assert lib.mpmpc_path_count(2, _d(short), 2.0, 0) == 0      # no segment long enough: the last corner alone
    for bad in ((1, short, 0.1, 0), (2, short, 0.0, 0), (2, short, 0.1, 64), (2, np.array([[0.0, np.inf], [1.0, 0.0]]), 0.1, 0)):
        assert lib.mpmpc_path_count(bad[0], _d(bad[1]), bad[2], bad[3]) == E_ARG and lib.mpmpc_last_error()


# ------------------------------------------------------------------------------------------------ crafted grids (T7)
CRAFT_RES, CRAFT_ROW = 0.125, 2.03      # cells of 1/8 m from (0, 0): every cell centre is exact; the route runs inside row 16


def _crafted(case):
    """-> (grid [32, 32], route, r_p, sd, max_width): a straight route along +x whose waypoint i stands on the centre of cell
    (4 + i, 16) in x, 16 waypoints (psi = 0: the normals are +-y)"""
    grid = np.ones((32, 32), np.int8)
    route, mw = np.array([[0.5625, CRAFT_ROW], [2.5625, CRAFT_ROW]]), 0.6
    if case == "narrow":            # max_width below one cell: every line is a single cell or a step to a neighbour
        mw = 0.04
        grid[17, 8] = grid[15, 9] = grid[16, 12] = 0
    elif case == "standing":        # waypoint 6 stands on an occupied cell
        grid[16, 10] = 0
    elif case == "tie":             # waypoint 6: (9, 19) and (11, 19) at exactly one distance, on the lines di = -1 and di = +1
        grid[19, 9] = grid[19, 11] = 0
    elif case == "tie_late":        # the later of the two alone: it is a candidate of its own
        grid[19, 11] = 0
    elif case == "leaves":          # the left probes leave the grid above row 31
        route = route + [0.0, 1.75]
    return grid, route, 0.125, 0, mw


def _host_class(grid, route, r_p, sd, mw):
    m = Map.from_grid(grid, origin=[0.0, 0.0], resolution=CRAFT_RES)
    rp = ReferencePath(m, list(route[:, 0]), list(route[:, 1]), r_p, sd, mw, True)
    # the fixture is off the ties of the normals' targets: numpy's and glibc's cos / sin cannot disagree on a target cell
    for w in rp.waypoints:
        for s in (1, -1):
            f = np.array([w.x, w.y + s * mw]) / CRAFT_RES
            assert np.min(np.abs(f - np.round(f))) > 1e-3
    width = np.array([[w.ub, -w.lb] for w in rp.waypoints])
    cells = np.array([[w.static_border_cells[0], w.static_border_cells[1]] for w in rp.waypoints]).reshape(-1, 4)
    return rp, width, cells


def _check_crafted(build, case):
    grid, route, r_p, sd, mw = _crafted(case)
    o = build(grid, (0.0, 0.0), CRAFT_RES, [route], r_p, sd, mw, True)
    assert o["n_wp"][0] == 16
    if case == "leaves":
        assert o["status"][0] == 1
        assert np.all(o["border"][0, :, 1] > 32 * CRAFT_RES) and np.all(o["ub"][0] < mw)      # the cell outside is the border
        assert np.all(o["lb"][0] == -mw) and np.all(o["border"][0, :, 3] < 32 * CRAFT_RES)
        return o
    rp, width, cells = _host_class(grid, route, r_p, sd, mw)
    assert o["status"][0] == 0 and rp.n_waypoints == 16
    assert np.array_equal(o["x"][0], [w.x for w in rp.waypoints]) and np.array_equal(o["y"][0], [w.y for w in rp.waypoints])
    assert np.array_equal(np.stack([o["ub"][0], -o["lb"][0]], 1), width) and np.array_equal(o["border"][0], cells)
    centre = lambda cx, cy: ((cx + 0.5) * CRAFT_RES, (cy + 0.5) * CRAFT_RES)      # noqa: E731
    if case == "narrow":
        assert np.sum(width < mw) >= 1 and np.sum(width == mw) >= 28
    if case == "standing":
        assert tuple(cells[6, :2]) == tuple(cells[6, 2:]) == centre(10, 16) and width[6, 0] == width[6, 1] < CRAFT_RES
    if case == "tie":
        # the host class says it is a tie, and which cell the reference's order meets first
        late = _host_class(*_crafted("tie_late"))
        assert tuple(late[2][6, :2]) == centre(11, 19) and late[1][6, 0] == width[6, 0] < mw
        assert tuple(cells[6, :2]) == centre(9, 19)
    return o


@pytest.mark.parametrize("case", ["narrow", "standing", "tie", "leaves"])
def test_twin_on_crafted_grids(case, twin):
    """T7 on the CPU: the twin against the host class on 32 x 32 grids"""
    _check_crafted(lambda *a: _twin_build(twin, *a), case)


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("track", ["sim", "real"])
def test_device_matches_reference_paths(track, twin):
    """T5: the device against G1, as T1, and against the twin bit for bit"""
    g1, grid, origin, res = _g1(track)
    t = TRACKS[track]
    o = _dev_build(grid, origin, res, [_route(track)], t["r_p"], t["sd"], t["mw"], t["circular"])
    _against_g1(o, track)
    _same(o, _twin_build(twin, grid, origin, res, [_route(track)], t["r_p"], t["sd"], t["mw"], t["circular"]))


@pytest.mark.gpu
def test_device_matches_twin_on_seeded_routes(seeded):
    """T5: every output bit-equal, psi and kappa included, no exclusions"""
    rs, tw, _ = seeded
    _, grid, origin, res = _g1("real")
    o = _dev_build(grid, origin, res, [r["route"] for r in rs], [r["r_p"] for r in rs], [r["sd"] for r in rs], [r["mw"] for r in rs],
                   [r["circular"] for r in rs])
    _same(o, tw)


def _leg(n_wp, sd, r_p=0.2):
    """a straight route along Real_Track's first leg that gives exactly n_wp waypoints (half a step off the count's ties)"""
    c = _route("real")
    u = (c[1] - c[0]) / np.linalg.norm(c[1] - c[0])
    return np.array([c[0], c[0] + u * (n_wp + 2 * sd + 0.5) * r_p])


@pytest.mark.gpu
def test_ragged_call(twin):
    """T6: 8 paths in one call - n_wp 2, 3, 31, 32, 33 (both sides of a workgroup's 32 waypoints) and 302, sd 0 and 63, both
    circular flags, one path too short (-1), one beyond cap (-2): each built path equals its solo build, failed rows are NaN"""
    _, grid, origin, res = _g1("real")
    t = TRACKS["real"]
    paths = [(_leg(2, 63), 0.2, 63, 1.5, True, 2, 0), (_leg(1, 5), 0.2, 5, 1.5, True, 1, -1), (_leg(3, 0), 0.2, 0, 1.0, False, 3, 0),
             (_leg(31, 5), 0.2, 5, 1.5, True, 31, 0), (_route("real"), 0.1, 5, 1.5, False, None, -2), (_leg(32, 0), 0.2, 0, 2.0, False, 32, 0),
             (_leg(33, 2), 0.2, 2, 1.2, True, 33, 0), (_route("real"), t["r_p"], t["sd"], t["mw"], t["circular"], 302, 0)]
    cols = list(zip(*paths))
    o = _dev_build(grid, origin, res, list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), list(cols[4]), cap=302)
    _same(o, _twin_build(twin, grid, origin, res, list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), list(cols[4]), cap=302))
    for p, (route, r_p, sd, mw, circ, n, status) in enumerate(paths):
        assert o["status"][p] == status, p
        if status < 0:
            assert all(np.all(np.isnan(o[k][p])) for k in TABLES + ("border",)) and np.isnan(o["length"][p])
            assert o["n_wp"][p] == (1 if status == -1 else mpmpc.path_count(route, r_p, sd)) and (status == -1 or o["n_wp"][p] > 302)
            continue
        assert o["n_wp"][p] == n
        solo = _dev_build(grid, origin, res, [route], r_p, sd, mw, circ)
        assert solo["x"].shape[1] == n
        _same(o, solo, p, 0)
        assert all(np.all(np.isnan(o[k][p, n:])) for k in TABLES + ("border",)) and not np.any(np.isnan(o["ub"][p, :n]))
    _against_g1({k: v[7:8] for k, v in o.items()}, "real")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["narrow", "standing", "tie", "leaves"])
def test_device_on_crafted_grids(case, twin):
    """T7: the device against the host class on 32 x 32 grids (a line that leaves the grid: against the twin, status 1)"""
    o = _check_crafted(_dev_build, case)
    grid, route, r_p, sd, mw = _crafted(case)
    _same(o, _twin_build(twin, grid, (0.0, 0.0), CRAFT_RES, [route], r_p, sd, mw, True))


def _sim_world():
    g1, grid, origin, res = _g1("sim")
    m = Map.from_grid(grid, origin=list(origin), resolution=res)
    discs = m.obstacle_discs([Obstacle(cx=c[0], cy=c[1], radius=c[2]) for c in g1["obstacles"]])
    walls = m.boundary_walls([((-0.5, -1.7), (-0.5, -1.3)), ((-0.45, -1.0), (-0.05, -1.02))])
    return discs, walls


@pytest.mark.gpu
def test_worlds(twin):
    """T8: Sim_Track's route with the G1 obstacle discs and two walls across the track as per-path lists = the same route on the
    grid mpmpc.world_grid returns for those lists; a second path of the same call with empty lists = the base-map build"""
    _, grid, origin, res = _g1("sim")
    t = TRACKS["sim"]
    discs, walls = _sim_world()
    route = _route("sim")
    o = _dev_build(grid, origin, res, [route, route], t["r_p"], t["sd"], t["mw"], True, discs=[discs, np.zeros((0, 3), np.int32)],
                   walls=[walls, np.zeros((0, 4), np.int32)])
    world = mpmpc.world_grid(grid, origin, res, discs=discs, walls=walls)
    assert int(np.sum(world != grid)) > 100
    stamped = _dev_build(world, origin, res, [route], t["r_p"], t["sd"], t["mw"], True)
    _same(o, stamped, 0, 0)
    _same(o, _dev_build(grid, origin, res, [route], t["r_p"], t["sd"], t["mw"], True), 1, 0)
    assert np.sum(o["ub"][0] != o["ub"][1]) + np.sum(o["lb"][0] != o["lb"][1]) >= 10      # the world is felt
    _same(o, _twin_build(twin, grid, origin, res, [route, route], t["r_p"], t["sd"], t["mw"], True,
                         discs=[discs, np.zeros((0, 3), np.int32)], walls=[walls, np.zeros((0, 4), np.int32)]))


@pytest.mark.gpu
def test_on_device_feeds_the_device_corridor():
    """T9: ReferencePath.on_device on Sim_Track -> set_path_geometry -> build_corridor on the obstacle grid, bit-equal to the
    corridor from the host constructor's tables on the same machine"""
    g1, grid, origin, res = _g1("sim")
    h_, w_ = g1["grid_shape"]
    obst = np.ascontiguousarray(np.unpackbits(g1["grid_obstacles"])[:h_ * w_].reshape(h_, w_).astype(np.int8))
    t = TRACKS["sim"]
    m = Map.from_grid(grid, origin=list(origin), resolution=res)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dev = ReferencePath.on_device(m, list(g1["wp_x"]), list(g1["wp_y"]), t["r_p"], t["sd"], t["mw"], True)
    host = ReferencePath(m, list(g1["wp_x"]), list(g1["wp_y"]), t["r_p"], smoothing_distance=t["sd"], max_width=t["mw"], circular=True)
    assert dev.n_waypoints == host.n_waypoints == 200 and dev.resolution == host.resolution and dev.smoothing_distance == host.smoothing_distance
    assert isinstance(dev.waypoints[0].kappa, int) and dev.waypoints[0].kappa == 0 and dev.circular is True
    assert [w.ub for w in dev.waypoints] == [w.ub for w in host.waypoints] and [w.lb for w in dev.waypoints] == [w.lb for w in host.waypoints]
    for a, b in zip(dev.waypoints, host.waypoints):
        assert tuple(map(tuple, a.static_border_cells)) == tuple(map(tuple, b.static_border_cells))
        assert tuple(map(tuple, a.dynamic_border_cells)) == tuple(map(tuple, b.static_border_cells))
    sm = 0.06 / math.sqrt(2)      # the car of the Sim_Track scenario (width 0.06): golden G3's safety margin
    rows = []
    for rp in (dev, host):
        x, y, psi = (np.array([getattr(w, k) for w in rp.waypoints], float) for k in ("x", "y", "psi"))
        bu = np.array([w.static_border_cells[0] for w in rp.waypoints], float)
        bl = np.array([w.static_border_cells[1] for w in rp.waypoints], float)
        kappa, _, ds = rp.tables()
        h = mpmpc.Handle(T.stock_config(30, max_batch=4))
        h.set_path(kappa, np.ones(x.size), ds)
        h.set_map(obst, origin, res)
        h.set_path_geometry(x, y, psi, bu, bl)
        ub, lb, bad = h.build_corridor(30, 2 * sm, sm)
        h.close()
        assert bad == 0
        rows.append((ub, lb))
    assert np.array_equal(rows[0][0], rows[1][0], equal_nan=True) and np.array_equal(rows[0][1], rows[1][1], equal_nan=True)
    with pytest.raises(ValueError):
        ReferencePath.on_device(m, [0.0, 0.1], [0.0, 0.0], 0.05, 5, 0.23, True)
