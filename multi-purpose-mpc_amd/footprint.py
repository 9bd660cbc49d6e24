"""Footprint audit on the device: did a car touch anything, and how close did it get?

`Footprint(length, width, reach=None, stop=False)` is the car's rectangle - `length` along the heading, `width` across it,
centred at the pose, as SpatialBicycleModel.show of the reference draws it - and how far clearances are measured (`reach`,
by default the car's length).  `audit_batch` gives the verdict for a fleet of poses, each car in its own world, as one
kernel launch (K0f, mpmpc.footprint_audit; the law is csrc/footprint_core.hpp); `audit` is the same for one car.  Passed to
`MPC.BatchMPC.rollout(..., audit=...)` it audits every step of a device rollout; with `stop` a car in contact ends there
(alive = -5).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

import mpmpc
from lidar_model import _pose


class Footprint:
    def __init__(self, length, width, reach=None, stop=False, device=0):
        """length, width, reach in metres; reach defaults to the car's length"""
        self.length = float(length)
        self.width = float(width)
        self.reach = float(length if reach is None else reach)
        self.stop = bool(stop)
        self.device = device
        self.contact = False             # the verdict of the last `audit`
        self.clearance = self.reach

    @property
    def mode(self):
        """mpmpc.Handle.rollout_set_audit's mode: 1 audit, 2 audit and stop on contact"""
        return 2 if self.stop else 1

    def audit_batch(self, poses, map, discs=None, walls=None):
        """poses [B, 3] = x, y, psi on `map` (map.data, .origin, .resolution); discs: per car an int [k, 3] array of
        (cx, cy, r) map cells on top of map.data (Map.obstacle_discs), or None; walls: per car an int [k, 4] array of
        (x0, y0, x1, y1) map cells (Map.boundary_walls), or None -> (contact [B] bool, clearance [B])"""
        contact, clearance = mpmpc.footprint_audit(map.data, map.origin, map.resolution, poses, self.length, self.width,
                                                   self.reach, discs, device=self.device, walls=walls)
        return contact.astype(bool), clearance

    def audit(self, car, map):
        """one car (an object with x, y, psi, or a model with a temporal_state) on map.data -> (contact, clearance); also
        kept in self.contact / self.clearance"""
        contact, clearance = self.audit_batch([_pose(car)], map)
        self.contact, self.clearance = bool(contact[0]), float(clearance[0])
        return self.contact, self.clearance
