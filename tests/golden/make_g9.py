"""Generate G9 (lidar scans) by IMPORTING the reference's LidarModel, like make_golden.py (same interpreter, cwd = the
reference's src/):

    cd <reference>/src && MPLBACKEND=Agg python3.9 -W ignore <this repository>/tests/golden/make_g9.py

Everything written is DATA: g9_lidar.npz holds, per scan, the track, the pose, the sensor's three parameters, the
reference's `measurements` [2 x n] after scan(car, map), and per track the obstacle discs (map cells) that were added to
the map - the grids are G1 / G1r `grid_free` plus those discs (checked here against the reference's map.data).

Every scan is checked against a numpy evaluation of the law of csrc/lidar_core.hpp and its TIE MARGIN is computed: how
close an angle of an occupied in-range cell comes to a beam, to -+pi/2 (the skip test) or to the +-pi wrap.  A scan below
1e-9 rad is refused: there two libms could differ.  (Axis-aligned headings such as psi = 0 tie exactly.)
"""
import contextlib
import io
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets up the reference's flat imports)

import numpy as np  # noqa: E402
from lidar_model import LidarModel  # noqa: E402
from map import Map, Obstacle  # noqa: E402

MARGIN = 1e-9

# (track, x, y, psi, FoV, range, resolution): the coverage named beside each
SCANS = [
    ("sim", -0.75, -1.5, 0.3, 180, 0.3, 1),
    ("sim", -0.25, -1.0, 1.47, 270, 0.25, 0.5),         # a fractional resolution
    ("sim", -0.62, -1.48, 3.3, 360, 0.2, 2),            # psi above pi
    ("sim", -0.99, -1.99, -4.0, 90, 0.3, 1),            # psi below -pi; the window clipped at the map's corner
    ("sim", 0.2, -0.6, 0.9, 180, 0.3, 1),
    ("sim", 0.0, 0.0, 0.7, 360, 0.2, 1),                # the sensor inside an occupied cell (an obstacle's centre)
    ("sim", -0.25, -0.75, 1.2, 180, 0.04, 0.7),         # no beam hits
    ("sim", 1.2, -0.7, -2.1, 270, 0.3, 1.5),
    ("real", -4.9, -5.0, 0.9, 180, 5, 1),
    ("real", -1.0, -5.0, 2.0, 120, 3, 1.5),
    ("real", -6.3, -11.1, -0.4, 360, 3, 1),             # inside an obstacle
    ("real", 6.5, 5.0, 3.9, 90, 4, 0.5),
    ("real", -29.9, -23.9, 0.8, 180, 5, 1),             # the window clipped at the map's corner
    ("real", -31.0, -25.0, 0.5, 180, 3, 1),             # the sensor off the grid
]


class Car:
    def __init__(self, x, y, psi):
        self.x, self.y, self.psi = x, y, psi


def discs_of(m, obstacles):
    out = []
    for cx, cy, rad in obstacles:
        out.append(m.w2m(cx, cy) + (int(np.ceil(rad / m.resolution)),))
    return np.array(out, np.int32).reshape(-1, 3)


def with_discs(grid, discs):
    g = np.array(grid, np.int8)
    for cx, cy, r in np.asarray(discs).tolist():
        yy, xx = np.ogrid[-r:r, -r:r]
        g[cy - r:cy + r, cx - r:cx + r][xx ** 2 + yy ** 2 <= r ** 2] = 0
    return g


def law(grid, origin, res, pose, angles, rng):
    """-> ranges, tie margin [rad], occupied in-range cells, skipped cells: the four steps of csrc/lidar_core.hpp"""
    H, W = grid.shape
    n = angles.size
    cx, cy = int(np.floor((pose[0] - origin[0]) / res)), int(np.floor((pose[1] - origin[1]) / res))
    lim = rng / res
    R = int(lim)
    i0, i1, j0, j1 = max(cx - R, 0), min(cx + R, W - 1), max(cy - R, 0), min(cy + R, H - 1)
    out = np.full(n, float(rng))
    if i0 > i1 or j0 > j1:
        return out, np.inf, 0, 0
    jj, ii = np.nonzero(grid[j0:j1 + 1, i0:i1 + 1] == 0)
    ii, jj = ii + i0, jj + j0
    d2 = (cx - ii) ** 2 + (cy - jj) ** 2
    keep = np.sqrt(d2.astype(float)) < lim
    ii, jj, d2 = ii[keep], jj[keep], d2[keep]
    if ii.size == 0:
        return out, np.inf, 0, 0
    ks = np.array([-0.5, 0.0, 0.5])
    dx = np.broadcast_to(((ii - cx)[:, None, None] + ks[None, :, None]), (ii.size, 3, 3))
    dy = np.broadcast_to(((jj - cy)[:, None, None] + ks[None, None, :]), (ii.size, 3, 3))
    raw = (np.arctan2(dy, dx) - pose[2]).reshape(ii.size, 9)
    a = np.where(raw < -math.pi, -np.mod(math.pi + raw, 2 * math.pi) + math.pi, np.mod(math.pi + raw, 2 * math.pi) - math.pi)
    mn, mx = a.min(1), a.max(1)
    skip = (mn < -math.pi / 2) & (mx > math.pi / 2)
    hit = (~skip)[:, None] & (mn[:, None] <= angles[None, :]) & (angles[None, :] <= mx[:, None])
    big = np.iinfo(np.int64).max
    best = np.where(hit, d2[:, None], big).min(0)
    out[best < big] = np.sqrt(best[best < big].astype(float)) * res
    margin = min(np.abs(mn[:, None] - angles[None, :]).min(), np.abs(mx[:, None] - angles[None, :]).min(),
                 np.abs(mn + math.pi / 2).min(), np.abs(mx - math.pi / 2).min(), np.abs(raw + math.pi).min(),
                 np.abs(np.abs(a) - math.pi).min())
    return out, float(margin), int(ii.size), int(skip.sum())


def main():
    worlds = {}
    m = Map(file_path='maps/sim_map.png', origin=[-1, -2], resolution=0.005)
    worlds["sim"] = (m, discs_of(m, G.OBSTACLES), "g1_path_sim_track.npz")
    G.add_obstacles(m)
    m = Map(**G.REAL_MAP)
    worlds["real"] = (m, discs_of(m, G.REAL_OBSTACLES), "g1_path_real_track.npz")
    m.add_obstacles([Obstacle(cx=c[0], cy=c[1], radius=c[2]) for c in G.REAL_OBSTACLES])
    out = {}
    for name, (m, discs, g1_file) in worlds.items():
        g1 = np.load(os.path.join(HERE, g1_file))
        h, w = g1["grid_shape"]
        base = np.unpackbits(g1["grid_free"])[:h * w].reshape(h, w).astype(np.int8)
        assert np.array_equal(with_discs(base, discs), m.data), name      # the test's grid IS the reference's
        out["discs_" + name] = discs
    seen = dict(clipped=0, inside=0, skipped=0, no_hit=0, wide_psi=0, fractional=0)
    for k, (name, x, y, psi, fov, rng, reso) in enumerate(SCANS):
        m = worlds[name][0]
        sensor = LidarModel(FoV=fov, range=rng, resolution=reso)
        with contextlib.redirect_stdout(io.StringIO()):
            sensor.scan(Car(x, y, psi), m)
        ranges, margin, n_occ, n_skip = law(np.asarray(m.data), m.origin, m.resolution, (x, y, psi), sensor.measurements[0], rng)
        assert np.array_equal(ranges, sensor.measurements[1]), (k, "the law does not restate the reference")
        if margin < MARGIN:
            raise SystemExit("scan %d: tie margin %.3g rad is below %.0e - choose another pose" % (k, margin, MARGIN))
        cx, cy = m.w2m(x, y)
        R = int(rng / m.resolution)
        inside = 0 <= cx < m.width and 0 <= cy < m.height
        seen["clipped"] += cx - R < 0 or cy - R < 0 or cx + R >= m.width or cy + R >= m.height
        seen["inside"] += bool(inside and m.data[cy, cx] == 0)
        seen["skipped"] += n_skip > 0
        seen["no_hit"] += bool(np.all(sensor.measurements[1] == rng))
        seen["wide_psi"] += abs(psi) > math.pi
        seen["fractional"] += reso != int(reso)
        out["measurements_%d" % k] = sensor.measurements.copy()
        print("G9 scan %2d %-4s pose (%g, %g, %g) FoV %g range %g res %g: %d beams, %d hit, %d cells, %d skipped, margin %.3g"
              % (k, name, x, y, psi, fov, rng, reso, sensor.n_measurements, int((sensor.measurements[1] < rng).sum()), n_occ,
                 n_skip, margin))
    assert all(v > 0 for v in seen.values()), seen
    assert {s[4] for s in SCANS} >= {90, 180, 270, 360}
    np.savez_compressed(os.path.join(HERE, "g9_lidar.npz"), n_scans=np.array([len(SCANS)]),
                        track=np.array([s[0] for s in SCANS]), pose=np.array([s[1:4] for s in SCANS], float),
                        sensor=np.array([s[4:7] for s in SCANS], float), **out)


if __name__ == "__main__":
    main()
