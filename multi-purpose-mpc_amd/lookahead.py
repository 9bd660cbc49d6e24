"""Lookahead of the device rollout (host side): `Lookahead`, what `BatchMPC.rollout(..., lookahead=...)` takes, and numpy
restatements of the law the device applies every step (K0h, csrc/lookahead_core.hpp): `leads` - at which later step every
column of a car's horizon sees the car's movers - and `discs` - where the movers are then.  Lookahead for traffic
(K3t / K0ht, csrc/traffic_lookahead_core.hpp): `plan_tracks` - the cells and times of every car's solved plan - and
`traffic_discs` - where the cars in a car's traffic slots are, by their own plans, when the car reaches each column.
"""
from __future__ import annotations

import math

import numpy as np

from movers import mover_discs_rows

MAX_LEAD_CAP = 1 << 20
TRACK_OFF = -2 ** 31      # cells[n, j, 0] of a plan stage without a cell


class Lookahead:
    """max_lead [steps] bounds how far ahead a column looks; seg_time [n_wp] is the seconds a car is expected to need from
    waypoint i to i + 1 (by global row of the path table; None: BatchMPC.rollout builds seg_time_of(ds_next, v_ref) from the
    path or routes in force).  traffic: also anticipate the cars in the traffic slots from their own plans (needs
    BatchMPC.rollout(..., traffic=...) to have any effect)."""

    def __init__(self, max_lead, seg_time=None, traffic=False):
        self.traffic = bool(traffic)
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


def plan_tracks(z, wp_id, status, alive, x, y, psi, origin, resolution, n_wp=None, circular=True, first=0):
    """The plan tracks a step leaves (K3t) -> dict(valid bool [B], cells int32 [B, N + 1, 2], tm [B, N + 1]).  z [B, 5 N + 3]:
    the step's primal solutions (mpmpc.Handle.download), stage j = (e_y, e_psi, t) at z[:, 3 j : 3 j + 3]; wp_id, status, alive
    [B]: the rollout's state AFTER the step; x, y, psi: the path table by global row; n_wp / circular / first: the length,
    flag and first global row of every car's route (numbers or [B]; n_wp None: the whole table, one path).
      valid = alive == 1 and status in (1, 2, -2)
      stage j lies at waypoint wp_id + j, wrapped on a circular route and clamped to the last waypoint of an open one; its
      point is (x - e_y sin psi, y + e_y cos psi) there (libm's sin / cos, as the device's tables), its cell
      floor((p - origin) / resolution), or (TRACK_OFF, 0) where that is not finite or beyond 2^30
      tm[0] = 0, tm[j] = t_j if t_j > tm[j - 1] else tm[j - 1]        (a NaN is never taken)"""
    z = np.asarray(z, float)
    B = z.shape[0]
    N = (z.shape[1] - 3) // 5
    x, y, psi = (np.asarray(a, float) for a in (x, y, psi))
    sin = np.array([math.sin(a) for a in psi])
    cos = np.array([math.cos(a) for a in psi])
    n = np.broadcast_to(np.asarray(x.size if n_wp is None else n_wp, np.int64), (B,))
    circ = np.broadcast_to(np.asarray(circular, bool), (B,))
    f = np.broadcast_to(np.asarray(first, np.int64), (B,))
    w = np.asarray(wp_id, np.int64).reshape(B, 1) + np.arange(N + 1)[None, :]
    w = np.where(w >= n[:, None], np.where(circ[:, None], w % n[:, None], n[:, None] - 1), w) + f[:, None]
    e_y = z[:, 0:3 * (N + 1):3]
    with np.errstate(all="ignore"):
        px, py = x[w] - e_y * sin[w], y[w] + e_y * cos[w]
        qx, qy = np.floor((px - origin[0]) / resolution), np.floor((py - origin[1]) / resolution)
        ok = (np.abs(qx) <= 2.0 ** 30) & (np.abs(qy) <= 2.0 ** 30)
    cells = np.stack([np.where(ok, qx, TRACK_OFF), np.where(ok, qy, 0)], 2).astype(np.int64).astype(np.int32)
    t = z[:, 2:3 * (N + 1):3]
    tm = np.zeros((B, N + 1))
    for j in range(1, N + 1):
        with np.errstate(invalid="ignore"):
            tm[:, j] = np.where(t[:, j] > tm[:, j - 1], t[:, j], tm[:, j - 1])
    st = np.asarray(status).reshape(B)
    valid = (np.asarray(alive).reshape(B) == 1) & ((st == 1) | (st == 2) | (st == -2))
    return dict(valid=valid, cells=cells, tm=tm)


def traffic_discs(who, discs_k, lead, tracks, Ts, width, height):
    """The traffic slots over the horizons (K0ht) -> int32 [B, S, N, 3].  who [B, S]: the car in every slot at step k (-1:
    empty); discs_k [B, S, 3]: the slots' discs of step k (the TRUE lists: traffic.traffic_discs); lead [B, N]: the leads of
    step k (`leads`); tracks: `plan_tracks` of step k - 1 (valid all False: none).  Slot t of car b at column c, with
    n = who[b, t], d = discs_k[b, t], L = lead[b, c]:  d  if n < 0 or L == 0 or not valid[n];  else with j* the largest j with
    tm[n, j] <= (L + 1) * Ts and (cx, cy) = cells[n, j*]:  (0, 0, 0) if that stage has no cell or the square cx -+ r, cy -+ r
    leaves the grid (traffic_core.hpp's visibility test), else (cx, cy, d.r)."""
    who = np.asarray(who, np.int64)
    B, S = who.shape
    lead = np.asarray(lead, np.int64)
    N = lead.shape[1]
    d = np.asarray(discs_k, np.int64).reshape(B, S, 3)
    valid, cells, tm = np.asarray(tracks["valid"], bool), np.asarray(tracks["cells"], np.int64), np.asarray(tracks["tm"], float)
    out = np.repeat(d[:, :, None, :], N, 2)
    n = np.where(who >= 0, who, 0)
    tau = (lead + 1).astype(float) * float(Ts)                                        # [B, N]
    # j*: tm is non-decreasing with tm[:, 0] = 0 <= tau, so it is the count of entries <= tau, less one
    j = np.sum(tm[n][:, :, None, :] <= tau[:, None, :, None], 3) - 1                   # [B, S, N]
    c = cells[n[:, :, None], j]                                                        # [B, S, N, 2]
    r = d[:, :, None, 2]
    cx, cy = c[..., 0], c[..., 1]
    gone = (c[..., 0] == TRACK_OFF) | (cx - r < 0) | (cy - r < 0) | (cx + r > width) | (cy + r > height)
    moved = np.stack([np.where(gone, 0, cx), np.where(gone, 0, cy), np.where(gone, 0, np.broadcast_to(r, cx.shape))], 3)
    use = ((who >= 0) & valid[n])[:, :, None] & (lead[:, None, :] != 0)
    return np.where(use[..., None], moved, out).astype(np.int32)
