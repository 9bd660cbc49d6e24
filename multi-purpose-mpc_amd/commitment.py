"""Corridor commitment of the device rollout (host side): `Commitment`, what `BatchMPC.rollout(..., commitment=...)` takes - per
car, whether the waypoints of its horizon keep the side of an obstacle they chose in the step before, and the ratio at which a
much longer free segment is taken instead - and a restatement of what the device does with it in every step (the KEEP
instantiations of K0c, csrc/commitment_core.hpp): `row`, one car's corridor row, its new memory and what it adds to the
counters.  On python floats with the C library's sqrt / cos / sin / fmod, in the header's order, operation for operation.
"""
from __future__ import annotations

import math

import numpy as np

EMPTY = -1                      # wp of an empty memory entry
MAX_SEGMENTS = 8                # COR_MAXSEG: more free segments on one border line are an overflow
ROW_OK, ROW_BLOCKED, ROW_OVERFLOW = 0, 1, 2
BUDGET = 256 << 20              # bytes of a fleet's commitment block


def block_bytes(B, N):
    """cmt_bytes: the setting, the memory twice, the counters"""
    return 8 * B + 2 * B * N * (8 * 6 + 4) + 4 * 3 * B


class Commitment:
    """switch_ratio: a scalar or one value per car - 0: the car is off (its rows are the reference's); a value in [1, inf]: the
    car is on and leaves the candidate nearest its memory only for one more than switch_ratio times as long (inf: never)."""

    def __init__(self, switch_ratio=math.inf):
        self.switch_ratio = switch_ratio

    def keep(self, B):
        """-> float64 [B]: what mpmpc.Handle.rollout_set_commitment takes"""
        k = np.asarray(self.switch_ratio, float)
        if k.ndim == 0:
            k = np.full(int(B), float(k))
        k = np.ascontiguousarray(k.reshape(-1))
        if k.size != int(B):
            raise ValueError("switch_ratio must be a scalar or hold one value per car")
        if not np.all((k == 0.0) | (k >= 1.0)):      # (NaN fails both)
            raise ValueError("switch_ratio must be 0 (off) or in [1, inf] for every car")
        return k


def wp_index(i, n_wp, circular):
    """cor_wp"""
    return (i % n_wp if circular else n_wp - 1) if i >= n_wp else i


def _wrap(a):
    t = math.fmod(a + math.pi, 2.0 * math.pi)
    if t < 0.0:
        t += 2.0 * math.pi
    return t - math.pi


def trig_row(psi):
    """cor_trig_row"""
    au, al = _wrap(math.pi / 2 + psi), _wrap(-math.pi / 2 + psi)
    return (math.cos(psi), math.sin(psi), math.cos(au), math.sin(au), math.cos(al), math.sin(al))


def _side(wx, wy, cpsi, spsi, px, py):
    dx, dy = px - wx, py - wy
    cross = cpsi * dy - spsi * dx
    if cross > 0.0:
        return 1.0
    if cross < 0.0:
        return -1.0
    return -1.0 if (cpsi * dx + spsi * dy) < 0.0 else 0.0


def bounds(wx, wy, tr, s, sm):
    """cor_bounds of the candidate s = (ub_x, ub_y, lb_x, lb_y) -> (ub, lb, cell_ux, cell_uy, cell_lx, cell_ly)"""
    su, sl = _side(wx, wy, tr[0], tr[1], s[0], s[1]), _side(wx, wy, tr[0], tr[1], s[2], s[3])
    ub = su * math.sqrt((s[0] - wx) * (s[0] - wx) + (s[1] - wy) * (s[1] - wy))
    lb = sl * math.sqrt((s[2] - wx) * (s[2] - wx) + (s[3] - wy) * (s[3] - wy))
    ub -= sm
    lb += sm
    if ub < lb:
        ub, lb = 0.0, 0.0
    return (ub, lb, wx + (ub + sm) * tr[2], wy + (ub + sm) * tr[3], wx - (lb - sm) * tr[4], wy - (lb - sm) * tr[5])


def _span(s):
    dx, dy = s[0] - s[2], s[1] - s[3]
    return math.sqrt(dx * dx + dy * dy)


def _offset(s, ux, uy, lx, ly):
    du = math.sqrt((s[0] - ux) * (s[0] - ux) + (s[1] - uy) * (s[1] - uy))
    dl = math.sqrt((s[2] - lx) * (s[2] - lx) + (s[3] - ly) * (s[3] - ly))
    return (du + dl) / 2


def _first_min(v):
    best = 0
    for k in range(1, len(v)):
        if v[k] < v[best]:
            best = k
    return best


def _first_max(v):
    best = 0
    for k in range(1, len(v)):
        if v[k] > v[best]:
            best = k
    return best


def find(mem_wp, i):
    """cmt_find: the lowest column of the memory whose waypoint is i, or -1"""
    for c, w in enumerate(mem_wp):
        if w == i:
            return c
    return -1


def moved(ub, lb, m_ub, m_lb):
    """cmt_moved"""
    return ub != lb and m_ub != m_lb and (ub < m_lb or lb > m_ub)


def row(x, y, psi, ds_next, circular, wp_id, N, segments, sm, keep, mem_wp, mem_rows):
    """One car's step.  x, y, psi, ds_next: its route's waypoints; wp_id: its local waypoint (the row starts at wp_id + 1);
    segments(i) -> the free segments of waypoint i in the car's world, [(ub_x, ub_y, lb_x, lb_y), ...] in the scan's order;
    sm: the safety margin; keep: 0 or the switch_ratio; mem_wp [N], mem_rows [N][6]: the car's memory.
    -> (verdict, ub [N], lb [N], new mem_wp, new mem_rows, (kept, switched, moved)); without a row (verdict != ROW_OK) ub and lb
    are NaN, the new memory is empty and nothing is counted."""
    n_wp = len(x)
    on = keep >= 1.0
    idx = [wp_index(wp_id + 1 + c, n_wp, circular) for c in range(N)]
    segs = [list(segments(i)) for i in idx]
    verdict = ROW_BLOCKED if not segs[0] else (ROW_OVERFLOW if any(len(s) > MAX_SEGMENTS for s in segs) else ROW_OK)
    if verdict != ROW_OK:
        return verdict, [math.nan] * N, [math.nan] * N, [EMPTY] * N, [[0.0] * 6 for _ in range(N)], (0, 0, 0)
    out, kept, switched, n_moved = [], 0, 0, 0
    for c, i in enumerate(idx):
        cand = segs[c]
        tr = trig_row(psi[i])
        at = find(mem_wp, i)
        if len(cand) == 0:
            pick = (x[i], y[i], x[i], y[i])
        elif len(cand) == 1:
            pick = cand[0]
        elif on and at >= 0:                                   # rule 1
            m = mem_rows[at]
            k = _first_min([_offset(s, m[2], m[3], m[4], m[5]) for s in cand])
            spans = [_span(s) for s in cand]
            longest = _first_max(spans)
            kept += 1
            if keep < math.inf and spans[longest] > keep * spans[k]:
                k = longest
                switched += 1
            pick = cand[k]
        elif c == 0:                                           # rule 2: the largest segment
            pick = cand[_first_max([_span(s) for s in cand])]
        else:                                                  # ... or the nearest to the projection of the column before
            ip = wp_index(wp_id + c, n_wp, circular)
            shift, cp, sp = ds_next[ip], math.cos(psi[ip]), math.sin(psi[ip])
            prev = out[c - 1]
            qux, quy, qlx, qly = prev[2] + shift * cp, prev[3] + shift * cp, prev[4] + shift * sp, prev[5] + shift * sp
            pick = cand[_first_min([_offset(s, qux, quy, qlx, qly) for s in cand])]
        o = bounds(x[i], y[i], tr, pick, sm)
        out.append(o)
        if at >= 0 and moved(o[0], o[1], mem_rows[at][0], mem_rows[at][1]):
            n_moved += 1
    new_wp = [i if segs[c] else EMPTY for c, i in enumerate(idx)]
    new_rows = [list(out[c]) if segs[c] else [0.0] * 6 for c in range(N)]
    return ROW_OK, [o[0] for o in out], [o[1] for o in out], new_wp, new_rows, (kept, switched, n_moved)
