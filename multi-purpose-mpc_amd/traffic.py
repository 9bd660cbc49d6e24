"""Traffic of the device rollout (host side): `Traffic`, what `BatchMPC.rollout(..., traffic=...)` takes, and
`traffic_discs`, a numpy evaluation of the law the device applies every step (K0t, csrc/traffic_core.hpp) - the cars of a
group see each other as discs, computed from the poses and `alive` the step finds, so the discs of any step of a recorded
trace can be recomputed from that record alone (`trace_discs`), e.g. for plotting.
"""
from __future__ import annotations

import math

import numpy as np


class Traffic:
    """Who sees whom, in metres: group [B] ints (the same non-negative value: one world; negative: the car sees nobody and
    nobody sees it), radius [B] or one number - the disc with which a car appears to the others -, slots - how many of the
    nearest cars of its group a car sees -, range - how far it sees (None: no limit)."""

    def __init__(self, group, radius, slots, range=None):
        self.group = np.asarray(group, dtype=np.int64).reshape(-1)
        self.radius = np.broadcast_to(np.asarray(radius, dtype=float), self.group.shape).copy()
        self.slots = int(slots)
        self.range = None if range is None else float(range)

    def cells(self, resolution):
        """-> (group, radius_cells, slots, range_cells) as mpmpc.Handle.rollout_set_traffic takes them: the radius becomes
        Map.add_obstacles' cell count ceil(radius / resolution), the range floor(range / resolution) (-1: no limit)"""
        rad = np.ceil(self.radius / resolution).astype(np.int32)
        rng = -1 if self.range is None else int(math.floor(self.range / resolution))
        return self.group.astype(np.int32), rad, self.slots, rng


def traffic_discs(pose, alive, group, radius_cells, slots, range_cells, origin, resolution, width, height):
    """Slots (cx, cy, r), int32 [B, S, 3], of every car for the state (pose [B, 3], alive [B]) a rollout step finds.  Same
    operations in the same order as the device's (csrc/traffic_core.hpp); an empty slot is (0, 0, 0)."""
    pose = np.asarray(pose, float).reshape(-1, 3)
    B, S = pose.shape[0], int(slots)
    alive, group, r = (np.asarray(a).astype(np.int64).reshape(B) for a in (alive, group, radius_cells))
    with np.errstate(all="ignore"):
        qx, qy = np.floor((pose[:, 0] - origin[0]) / resolution), np.floor((pose[:, 1] - origin[1]) / resolution)
        present = (alive == 1) & (group >= 0) & (np.abs(qx) <= 2.0 ** 30) & (np.abs(qy) <= 2.0 ** 30)
        cx, cy = np.where(present, qx, 0.0).astype(np.int64), np.where(present, qy, 0.0).astype(np.int64)
    visible = present & ~((cx - r < 0) | (cy - r < 0) | (cx + r > width) | (cy + r > height))
    out = np.zeros((B, S, 3), np.int64)
    cars = np.nonzero(group >= 0)[0]
    cars = cars[np.argsort(group[cars], kind="stable")]            # group by group, ascending car index within each
    sizes = np.unique(group[cars], return_counts=True)[1]
    first = np.cumsum(sizes) - sizes
    none = np.iinfo(np.int64).max                                  # (d2 < 2^62: a candidate lies on the grid)
    for n in np.unique(sizes):                                     # all groups of n cars at once: [G, n(b), n(c)]
        idx = cars[first[sizes == n][:, None] + np.arange(n)[None, :]]
        x, y = cx[idx], cy[idx]
        d2 = (x[:, None, :] - x[:, :, None]) ** 2 + (y[:, None, :] - y[:, :, None]) ** 2
        ok = visible[idx][:, None, :] & present[idx][:, :, None] & ~np.eye(n, dtype=bool)[None]
        if range_cells >= 0:
            ok &= d2 <= int(range_cells) ** 2
        key = np.where(ok, d2, none)
        pick = np.argsort(key, axis=2, kind="stable")[:, :, :S]    # (stable: ties stay in car-index order)
        took = np.take_along_axis(ok, pick, 2)
        c = np.take_along_axis(np.broadcast_to(idx[:, None, :], key.shape), pick, 2)
        out[idx[:, :, None], np.arange(pick.shape[2])[None, None, :]] = np.where(took[..., None], np.stack([cx[c], cy[c], r[c]], 3), 0)
    return out.astype(np.int32)


def trace_discs(trace, k, group, radius_cells, slots, range_cells, origin, resolution, width, height):
    """The traffic slots, int32 [B, S, 3], of record k of a mpmpc.Handle.rollout_trace() dict: a record holds the pose
    its step started from, empty (NaN) when the car had ended - so "present" is "the pose is finite"."""
    pose = np.asarray(trace["pose"][k], float)
    alive = np.all(np.isfinite(pose), 1).astype(np.int32)
    return traffic_discs(np.where(alive[:, None] == 1, pose, 0.0), alive, group, radius_cells, slots, range_cells, origin,
                         resolution, width, height)
