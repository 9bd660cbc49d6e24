"""Moving obstacles of the device rollout (host side): `Mover`, what `BatchMPC.rollout(..., movers=...)` takes per car, and
`mover_discs`, a numpy evaluation of the motion law the device applies every step (K0m, csrc/obstacle_motion_core.hpp) -
a mover's disc is a closed-form function of the rollout step index, so the discs of any step of a recorded trace can be
recomputed from that index alone, e.g. for plotting.
"""
from __future__ import annotations

import math

import numpy as np

LINE, ALONG_PATH = 0, 1


class Mover:
    """A circular obstacle [m] that moves at a constant rate: along a straight line, or along the reference path."""

    def __init__(self, kind, radius, params):
        self.kind, self.radius, self.params = int(kind), float(radius), tuple(float(p) for p in params)

    @classmethod
    def line(cls, x, y, vx, vy, radius):
        """starts at the world point (x, y) and moves with the velocity (vx, vy) [m/s]"""
        return cls(LINE, radius, (x, y, vx, vy))

    @classmethod
    def along_path(cls, s, e_y, v, radius):
        """starts at arc length s of the reference path, e_y to the left of it (negative: to the right), and moves along
        it at v [m/s]; on a circular path it laps, on an open path it is gone past either end"""
        return cls(ALONG_PATH, radius, (s, e_y, v, 0.0))

    def row(self, Ts, resolution):
        """-> (kind, radius in cells, p0, p1, p2, p3) as mpmpc.Handle.rollout_set_movers takes it: the speeds become the
        displacement per control step of Ts seconds (one multiplication, here), the radius Map.add_obstacles' cell count"""
        p = self.params
        r = int(np.ceil(self.radius / resolution))
        if self.kind == LINE:
            return (LINE, r, p[0], p[1], p[2] * Ts, p[3] * Ts)
        return (ALONG_PATH, r, p[0], p[1], p[2] * Ts, 0.0)


def mover_discs_rows(rows, j, origin, resolution, width, height, cum=None, x=None, y=None, psi=None, circular=True):
    """Discs (cx, cy, r), int32 [n, 3], of n movers given as rows (kind, radius in cells, p0 .. p3) at j = k - step0 rollout
    steps (a number, or one per mover).  cum / x / y / psi: the path's cumulative segment lengths and waypoints (kind 1).
    Same operations in the same order as the device's (csrc/obstacle_motion_core.hpp); an absent mover is (0, 0, 0)."""
    rows = np.asarray(rows, float).reshape(-1, 6)
    n = rows.shape[0]
    kind, r = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
    p0, p1, p2, p3 = (rows[:, c] for c in (2, 3, 4, 5))
    j = np.broadcast_to(np.asarray(j, float), (n,))
    with np.errstate(all="ignore"):
        wx, wy = p0 + j * p2, p1 + j * p3
        present = np.ones(n, bool)
        on_path = kind == ALONG_PATH
        if on_path.any():
            cum, x, y = (np.asarray(a, float) for a in (cum, x, y))
            sin = np.array([math.sin(a) for a in np.asarray(psi, float)])        # libm, as the device's tables
            cos = np.array([math.cos(a) for a in np.asarray(psi, float)])
            s = p0 + j * p2
            L = cum[-1]
            ok = np.isfinite(s) & (L > 0.0)
            if circular:
                s = s - L * np.floor(s / L)
                s = np.where((s >= 0.0) & (s < L), s, 0.0)
            else:
                ok &= (s >= 0.0) & (s < L)
            s = np.where(ok, s, 0.0)
            i = np.clip(np.searchsorted(cum, s, side="right") - 1, 0, cum.size - 2)
            den = cum[i + 1] - cum[i]
            f = np.where(den > 0.0, (s - cum[i]) / np.where(den > 0.0, den, 1.0), 0.0)
            px = (x[i] + f * (x[i + 1] - x[i])) - p1 * sin[i]
            py = (y[i] + f * (y[i + 1] - y[i])) + p1 * cos[i]
            wx, wy = np.where(on_path, px, wx), np.where(on_path, py, wy)
            present &= ~on_path | ok
        qx, qy = np.floor((wx - origin[0]) / resolution), np.floor((wy - origin[1]) / resolution)
        present &= (np.abs(qx) <= 2.0 ** 30) & (np.abs(qy) <= 2.0 ** 30)
        cx, cy = np.where(present, qx, 0.0).astype(np.int64), np.where(present, qy, 0.0).astype(np.int64)
    present &= ~((cx - r < 0) | (cy - r < 0) | (cx + r > width) | (cy + r > height))
    out = np.stack([cx, cy, r], 1)
    out[~present] = 0
    return out.astype(np.int32)


def mover_discs(movers, k, Ts, map, path=None, step0=0):
    """Discs (cx, cy, r), int32 [n, 3], of a list of Mover at rollout step k (0-based; `Ts` the control period, `map` the
    Map the cars drive on, `path` its ReferencePath - needed by movers along the path).  Stack them under a car's static
    Map.obstacle_discs to get the world that car saw at step k."""
    rows = [m.row(Ts, map.resolution) for m in movers]
    kw = {}
    if path is not None:
        wps = path.waypoints
        kw = dict(cum=np.cumsum(path.segment_lengths), x=[w.x for w in wps], y=[w.y for w in wps],
                  psi=[w.psi for w in wps], circular=path.circular)
    return mover_discs_rows(rows, float(int(k) - int(step0)), map.origin, map.resolution, map.width, map.height, **kw)
