"""Lookahead of the device rollout (host side): `Lookahead`, what `BatchMPC.rollout(..., lookahead=...)` takes, and numpy
restatements of the law the device applies every step (K0h, csrc/lookahead_core.hpp): `leads` - at which later step every
column of a car's horizon sees the car's movers - and `discs` - where the movers are then.
"""
from __future__ import annotations

import numpy as np

from movers import mover_discs_rows

MAX_LEAD_CAP = 1 << 20


class Lookahead:
    """max_lead [steps] bounds how far ahead a column looks; seg_time [n_wp] is the seconds a car is expected to need from
    waypoint i to i + 1 (by global row of the path table; None: BatchMPC.rollout builds seg_time_of(ds_next, v_ref) from the
    path or routes in force)."""

    def __init__(self, max_lead, seg_time=None):
        self.max_lead = int(max_lead)
        if not 1 <= self.max_lead <= MAX_LEAD_CAP:
            raise ValueError("max_lead must be in [1, %d]" % MAX_LEAD_CAP)
        self.seg_time = None if seg_time is None else np.ascontiguousarray(seg_time, float).ravel()

    @staticmethod
    def seg_time_of(ds_next, v_ref):
        """ds_next / v_ref, inf where v_ref <= 0: the time model the MPC's own time state is linearised around"""
        ds, v = np.asarray(ds_next, float), np.asarray(v_ref, float)
        with np.errstate(all="ignore"):
            return np.where(v > 0.0, ds / np.where(v > 0.0, v, 1.0), np.inf)

    def table(self, ds_next, v_ref):
        return self.seg_time if self.seg_time is not None else self.seg_time_of(ds_next, v_ref)


def column_rows(wp_id, N, n_wp, circular, shift):
    """local waypoint of cor_wp(wp_id + shift + c), c = 0 .. N-1, per car: wp_id [B] -> [B, N] (n_wp / circular: a number or
    one per car - the car's route)"""
    i = np.asarray(wp_id, np.int64).reshape(-1, 1) + int(shift) + np.arange(int(N))[None, :]
    n = np.broadcast_to(np.asarray(n_wp, np.int64).reshape(-1, 1), i.shape)
    circ = np.broadcast_to(np.asarray(circular, bool).reshape(-1, 1), i.shape)
    return np.where(i >= n, np.where(circ, i % n, n - 1), i)


def leads(wp_id, N, seg_time, Ts, max_lead, n_wp=None, circular=True, first=0):
    """lead int32 [B, N] of cars at local waypoints wp_id [B]: t_c = t_(c-1) + seg_time[first + cor_wp(wp_id + c)] summed
    strictly left to right, lead_c = floor(t_c / Ts) if that is below max_lead, else max_lead.  n_wp / circular / first: the
    length, flag and first global row of every car's route (numbers or [B]; n_wp None: the whole table, one path)."""
    seg = np.asarray(seg_time, float)
    wp = np.asarray(wp_id, np.int64).ravel()
    n_wp = seg.size if n_wp is None else n_wp
    rows = column_rows(wp, N, n_wp, circular, 0) + np.asarray(first, np.int64).reshape(-1, 1)
    out = np.zeros(rows.shape, np.int32)
    t = np.zeros(wp.size)
    with np.errstate(all="ignore"):
        for c in range(int(N)):
            t = t + seg[rows[:, c]]
            q = np.floor(t / float(Ts))
            out[:, c] = np.where(q < max_lead, np.where(q < max_lead, q, 0.0), max_lead).astype(np.int32)
    return out


def discs(rows, k, lead, step0, origin, resolution, width, height, **path):
    """int32 [n, N, 3]: the discs of n movers (rows [n, 6] as mpmpc.Handle.rollout_set_movers takes them) over the horizons
    of their cars at rollout step k - column c of mover q at step k + lead[q, c] (lead [n, N]: the row of the car that
    owns the mover; [N]: one car's movers); **path: cum, x, y, psi, circular of the route the movers follow
    (movers.mover_discs_rows)."""
    rows = np.asarray(rows, float).reshape(-1, 6)
    lead = np.asarray(lead, np.int64)
    lead = np.broadcast_to(lead.reshape(-1, lead.shape[-1]), (rows.shape[0], lead.shape[-1]))
    N = lead.shape[1]
    j = (int(k) + lead - int(step0)).astype(float).ravel()
    return mover_discs_rows(np.repeat(rows, N, axis=0), j, origin, resolution, width, height, **path).reshape(rows.shape[0], N, 3)
