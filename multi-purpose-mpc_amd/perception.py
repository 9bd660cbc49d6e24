"""Perception for device rollouts: plan on what the lidar saw (K0s; the law is csrc/perception_core.hpp).

`Perception(lidar, hold=0)` wraps a `lidar_model.LidarModel` - the sensor every car of the fleet carries - and is what
`MPC.BatchMPC.rollout(..., perception=...)` takes: every step every running car scans its TRUE world, and its corridor is
built from the base map plus what it has seen so far.  The reference's Map is "a wrapper around a potential obstacle
detection algorithm ... incorporating LiDAR measurements"; this is that loop on the device, exact and per primitive:

    static obstacle, wall   known from the step it is first seen (a map)
    mover                   known for `hold` further steps after it was last seen, at its true position
    traffic                 known in the steps it is seen

`Perception.scan` is the sensor alone: the scans of a fleet and the primitives each car saw (mpmpc.perception_scan).
"""
from __future__ import annotations

import numpy as np

import mpmpc


class Perception:
    def __init__(self, lidar, hold=0):
        """lidar: a lidar_model.LidarModel (FoV, range, resolution); hold: steps a mover stays known after it was last seen"""
        for attr in ("measurements", "range"):
            if not hasattr(lidar, attr):
                raise TypeError("Perception needs a lidar_model.LidarModel")
        if int(hold) != hold or hold < 0:
            raise ValueError("hold must be a non-negative integer")
        self.lidar = lidar
        self.hold = int(hold)

    @property
    def angles(self):
        return np.ascontiguousarray(self.lidar.measurements[0], dtype=np.float64)

    @property
    def range(self):
        return float(self.lidar.range)

    def scan(self, poses, map, discs=None, walls=None):
        """poses [B, 3] on `map` (map.data, .origin, .resolution), discs / walls per car as for LidarModel.scan_batch ->
        (ranges [B, n], disc_seen [B] uint64, wall_seen [B] uint32)"""
        return mpmpc.perception_scan(map.data, map.origin, map.resolution, poses, self.angles, self.range, discs=discs,
                                     walls=walls, device=getattr(self.lidar, "device", 0))

    @staticmethod
    def slots(mask, n):
        """a seen / known mask -> bool [n]: slot q of the car's list"""
        return ((int(mask) >> np.arange(n, dtype=object)) & 1).astype(bool)
