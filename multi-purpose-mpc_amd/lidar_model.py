"""Lidar sensor on the device (same public surface as the reference's src/lidar_model.py:10-129:
`LidarModel(FoV, range, resolution)`, `.n_measurements`, `.measurements` [2 x n] = angles, ranges, `scan(car, map)`,
`plot_scan(car)`).

`scan` runs the reference's cell loops as one kernel launch (K0l, mpmpc.lidar_scan; the law is csrc/lidar_core.hpp) and
prints nothing; `scan_batch` scans a fleet, each car in its own world.  There is no CPU fallback.  The scans of a running
device rollout are `mpmpc.Handle.rollout_scan` / `MPC.BatchMPC.rollout_scan`.
"""
from __future__ import annotations

import math

import numpy as np

import mpmpc

SCAN = '#5DADE2'


def _pose(car):
    """x, y, psi of what the reference calls `car`: an object with those attributes, or a model with a temporal_state"""
    st = car if hasattr(car, "psi") else car.temporal_state
    return float(st.x), float(st.y), float(st.psi)


class LidarModel:
    def __init__(self, FoV, range, resolution, device=0):
        """FoV: field of view in degrees, range in metres, resolution in degrees (src/lidar_model.py:14-35)"""
        self.FoV = FoV
        self.range = range
        self.resolution = resolution
        self.device = device
        self.n_measurements = int(self.FoV / self.resolution + 1)
        angles = np.linspace(-math.pi / 360 * self.FoV, math.pi / 360 * self.FoV, self.n_measurements)
        ranges = np.ones(self.n_measurements) * self.range
        self.measurements = np.stack((angles, ranges), axis=0)

    def scan_batch(self, poses, map, discs=None, walls=None):
        """poses [B, 3] = x, y, psi on `map` (map.data, .origin, .resolution); discs: per car an int [k, 3] array of
        (cx, cy, r) map cells on top of map.data (Map.obstacle_discs), or None; walls: per car an int [k, 4] array of
        (x0, y0, x1, y1) map cells (Map.boundary_walls), or None -> ranges [B, n_measurements]"""
        return mpmpc.lidar_scan(map.data, map.origin, map.resolution, poses, self.measurements[0], self.range, discs,
                                device=self.device, walls=walls)

    def scan(self, car, map):
        """updates self.measurements[1] with the scan of one car on map.data"""
        self.measurements[1, :] = self.scan_batch([_pose(car)], map)[0]

    def plot_scan(self, car):
        import matplotlib.pyplot as plt
        x, y, psi = _pose(car)
        beam_end_x = self.measurements[1, :] * np.cos(self.measurements[0, :] + psi)
        beam_end_y = self.measurements[1, :] * np.sin(self.measurements[0, :] + psi)
        for i in range(self.n_measurements):
            plt.plot((x, x + beam_end_x[i]), (y, y + beam_end_y[i]), c=SCAN)
