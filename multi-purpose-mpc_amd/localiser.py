"""Lidar localisation of the device rollout (host side): `Localiser`, what `BatchMPC.rollout(..., localiser=...)` takes - every
scheduled step each car scans its true world and matches the scan against the map it knows in advance, the base map, starting
from dead reckoning - and restatements of what the device does with it (K0d, K3l; csrc/localiser_core.hpp): the distance field
(`Localiser.field`), the match (`Localiser.match`), the range noise (`Localiser.noisy`) and the step (`fresh` /
`Localiser.update`), for host loops.  Endpoints are computed one after the other on python floats with the C library's cos / sin,
in the header's order, operation for operation; scores are integers.

The law (csrc/localiser_core.hpp is the specification).  The field: F[j][i] = min(cap, the smallest (i' - i)^2 + (j' - j)^2 <= D^2
over the occupied cells of the grid), cap = D^2 + 1; outside the grid: cap.  A step of a car, from the true pose, the last fix
and (v, delta), the command the controller believes reached the wheels in step k - 1 (the estimator's rule):
  1  not primed: fix = prior = the true pose, primed, no scan is used
  2  else prior = the nominal model's step on the last fix; (k - step0) mod period != 0: fix = prior, no scan is used
  3  else the scan: beam b is a hit iff ranges[b] < range; a hit's range takes sigma_r * n_b, n_b the plant's variate of word b & 3
     of Philox block 16 + (b >> 2) of (seed, car0 + car, k - step0); fewer than min_hits hits or a prior that is not finite:
     fix = prior, lost
  4  else the match: psi_t = prior_psi + t * step_psi, t in [-T, T]; a hit's endpoint (prior_x + r cos(psi_t + angle), prior_y +
     r sin(psi_t + angle)) and its cell (floor((e - origin) / res)); score(a, c, t) = the sum over the hits of F(ci + a m,
     cj + c m), a, c in [-W, W]; the winner is the smallest (score, a^2 + c^2, t^2, idx), idx = ((t + T)(2W + 1) + (c + W))(2W + 1) +
     (a + W); fix = (prior_x + (a m) res, prior_y + (c m) res, psi_t); a winner on the window's border counts as edge
  5  statistics from the true pose: steps, matched, lost, edge, err2_sum / err2_max of the fix's position error, head2_sum of its
     wrapped heading error squared, prior2_sum of the prior's position error.
"""
from __future__ import annotations

import math

import numpy as np

from delay import nominal
from estimator import wrap
from plant import philox4x32, variate

CELL_MAX = 1073741824.0      # MOV_CELL_MAX
STATS = ("err2_max", "err2_sum", "head2_sum", "prior2_sum")
COUNTS = ("steps", "matched", "lost", "edge")


def fresh(B, n_beams=0):
    """-> the state a run of B cars starts from: nobody primed, the statistics zero"""
    B = int(B)
    out = dict(fix=np.zeros((B, 3)), prior=np.zeros((B, 3)), primed=np.zeros(B, np.int32), cand=np.full(B, -1, np.int32),
               score=np.full(B, -1, np.int32), hits=np.full(B, -1, np.int32), ranges=np.zeros((B, int(n_beams))))
    out.update({k: np.zeros(B) for k in STATS})
    out.update({k: np.zeros(B, np.int32) for k in COUNTS})
    return out


class Localiser:
    """The scan matcher of a rollout, one setting for the fleet.  lidar: a lidar_model.LidarModel (its angles and range; anything
    with `measurements[0]` and `range`);  D in [1, 15]: the reach of the distance field in cells;  step_cells >= 1: the
    translation step m in cells;  window in [0, 16] and headings in [0, 8]: the half widths W and T of the search window, in
    translation steps and in heading steps of step_psi [rad];  min_hits: fewer hits and the car is lost for the step;  sigma_r
    [m]: the amplitude of the triangular range noise;  period: the car scans on the steps with (k - step0) mod period == 0;
    seed, car0, step0: the noise is a function of (seed, car0 + car, k - step0, beam)."""

    def __init__(self, lidar, D, step_cells, window, headings, step_psi, min_hits=3, sigma_r=0.0, period=1, seed=0, car0=0, step0=0):
        self.angles = np.ascontiguousarray(np.asarray(lidar.measurements)[0], dtype=np.float64)
        self.range = float(lidar.range)
        self.D, self.m, self.W, self.T = int(D), int(step_cells), int(window), int(headings)
        self.step_psi, self.min_hits, self.sigma_r, self.period = float(step_psi), int(min_hits), float(sigma_r), int(period)
        self.seed, self.car0, self.step0 = int(seed), int(car0), int(step0)
        if not 1 <= self.D <= 15:
            raise ValueError("localiser: D must be in [1, 15] cells")
        if self.m < 1:
            raise ValueError("localiser: the translation step must be >= 1 cell")
        if not 0 <= self.W <= 16:
            raise ValueError("localiser: the window W must be in [0, 16]")
        if not 0 <= self.T <= 8:
            raise ValueError("localiser: the headings T must be in [0, 8]")
        if not (math.isfinite(self.step_psi) and self.step_psi >= 0.0) or (self.T > 0 and not self.step_psi > 0.0):
            raise ValueError("localiser: step_psi must be finite and >= 0, and > 0 when T > 0")
        if self.min_hits < 1:
            raise ValueError("localiser: min_hits must be >= 1")
        if not (math.isfinite(self.sigma_r) and self.sigma_r >= 0.0):
            raise ValueError("localiser: sigma_r must be finite and >= 0")
        if self.period < 1:
            raise ValueError("localiser: period must be >= 1")
        if (2 * self.T + 1) * self.angles.size > 8192:
            raise ValueError("localiser: (2 T + 1) * n_beams must be at most 8192")

    @property
    def cap(self):
        return self.D * self.D + 1

    @property
    def n_candidates(self):
        return (2 * self.T + 1) * (2 * self.W + 1) ** 2

    def candidate(self, idx):
        """idx -> (a, c, t)"""
        n = 2 * self.W + 1
        return int(idx) % n - self.W, (int(idx) // n) % n - self.W, int(idx) // (n * n) - self.T

    def setting(self):
        """-> the keyword arguments of mpmpc.Handle.rollout_set_localiser (without B and fix0)"""
        return dict(angles=self.angles, range_m=self.range, D=self.D, m=self.m, W=self.W, T=self.T, step_psi=self.step_psi,
                    min_hits=self.min_hits, sigma_r=self.sigma_r, period=self.period, seed=self.seed, car0=self.car0, step0=self.step0)

    def car(self, i):
        """-> the Localiser of car i alone (car0 moved): what a host loop that drives one car at a time uses"""
        out = Localiser.__new__(Localiser)
        out.__dict__.update(self.__dict__)
        out.car0 = self.car0 + int(i)
        return out

    def scheduled(self, k):
        return (int(k) - self.step0) % self.period == 0      # (python's modulus is non-negative)

    # --- K0d
    def field(self, grid):
        """grid [H, W] (1 free / 0 occupied; a map.Map's `data`) -> uint8 [H, W], K0d's field, by brute force: one shifted copy of
        the occupancy per offset of the disc of radius D"""
        occ = np.asarray(getattr(grid, "data", grid)) == 0
        H, W_ = occ.shape
        D = self.D
        F = np.full((H, W_), self.cap, np.int32)
        pad = np.zeros((H + 2 * D, W_ + 2 * D), bool)
        pad[D:D + H, D:D + W_] = occ
        for dj in range(-D, D + 1):
            for di in range(-D, D + 1):
                d2 = di * di + dj * dj
                if d2 <= D * D:
                    F = np.where(pad[D + dj:D + dj + H, D + di:D + di + W_], np.minimum(F, d2), F)
        return F.astype(np.uint8)

    # --- the range noise of step 3
    def variates(self, k, B):
        """-> float64 [B, n_beams]: n_b of cars car0 .. car0 + B - 1 at rollout step k"""
        n = self.angles.size
        nblk = (n + 3) // 4
        ju = (int(k) - self.step0) & 0xFFFFFFFFFFFFFFFF      # two's complement
        seed = self.seed & 0xFFFFFFFFFFFFFFFF
        ctr = np.zeros((int(B), nblk, 4), np.uint64)
        ctr[..., 0] = np.array([(self.car0 + i) & 0xFFFFFFFF for i in range(int(B))], np.uint64)[:, None]
        ctr[..., 1], ctr[..., 2] = ju & 0xFFFFFFFF, ju >> 32
        ctr[..., 3] = 16 + np.arange(nblk, dtype=np.uint64)[None, :]
        w = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
        return variate(w).reshape(int(B), 4 * nblk)[:, :n]

    def noisy(self, k, ranges):
        """ranges [B, n_beams], K0l's scans of step k -> (the ranges with every hit's made noisy, hit [B, n_beams] bool)"""
        r = np.array(ranges, dtype=np.float64).reshape(-1, self.angles.size)
        hit = r < self.range
        return np.where(hit, r + self.sigma_r * self.variates(k, r.shape[0]), r), hit

    # --- steps 3 (the hits) and 4
    def match(self, grid, origin, resolution, priors, ranges, hit=None, field=None):
        """(prior, scan) pairs on the map `grid` [H, W] with its origin and resolution: priors [B, 3], ranges [B, n_beams] (a hit's
        already noisy), hit [B, n_beams] bool (None: ranges < range) -> dict(fix [B, 3], cand, score, hits [B], min_edge [B]: the
        smallest distance, in cells, of a used endpoint to a cell boundary, +inf without one).  cand = score = -1 and fix = prior
        without a match."""
        F = self.field(grid) if field is None else np.asarray(field)
        H, W_ = F.shape
        ox, oy, res = float(origin[0]), float(origin[1]), float(resolution)
        priors = np.asarray(priors, float).reshape(-1, 3)
        ranges = np.asarray(ranges, float).reshape(priors.shape[0], self.angles.size)
        hit = ranges < self.range if hit is None else np.asarray(hit, bool).reshape(ranges.shape)
        B = priors.shape[0]
        out = dict(fix=priors.copy(), cand=np.full(B, -1, np.int32), score=np.full(B, -1, np.int32), hits=hit.sum(1).astype(np.int32),
                   min_edge=np.full(B, np.inf))
        W, T, m, cap = self.W, self.T, self.m, self.cap
        shift = np.arange(-W, W + 1, dtype=np.int64) * m
        Fp = np.full((H + 1, W_ + 1), cap, np.int64)      # (row H / column W_: every look-up outside the grid)
        Fp[:H, :W_] = F
        for i in range(B):
            px, py, ppsi = (float(v) for v in priors[i])
            if out["hits"][i] < self.min_hits or not all(math.isfinite(v) for v in (px, py, ppsi)):
                continue
            beams = np.nonzero(hit[i])[0]
            best = None
            for t in range(-T, T + 1):
                psi_t = ppsi + float(t) * self.step_psi
                ci, cj, bad = [], [], 0
                for b in beams:
                    th = psi_t + float(self.angles[b])
                    r = float(ranges[i, b])
                    ex, ey = px + r * math.cos(th), py + r * math.sin(th)
                    qx, qy = (ex - ox) / res, (ey - oy) / res
                    if not (math.isfinite(qx) and math.isfinite(qy)) or not (abs(math.floor(qx)) <= CELL_MAX and abs(math.floor(qy)) <= CELL_MAX):
                        bad += 1
                        continue
                    fx, fy = math.floor(qx), math.floor(qy)
                    out["min_edge"][i] = min(out["min_edge"][i], qx - fx, 1.0 - (qx - fx), qy - fy, 1.0 - (qy - fy))
                    ci.append(fx)
                    cj.append(fy)
                ci, cj = np.array(ci, np.int64), np.array(cj, np.int64)
                ii = ci[None, :] + shift[:, None]                       # [a, hit]
                jj = cj[None, :] + shift[:, None]                       # [c, hit]
                ii = np.where((ii >= 0) & (ii < W_), ii, W_)
                jj = np.where((jj >= 0) & (jj < H), jj, H)
                sc = Fp[jj[:, None, :], ii[None, :, :]].sum(-1) + bad * cap      # [c, a]
                for c in range(-W, W + 1):
                    for a in range(-W, W + 1):
                        idx = ((t + T) * (2 * W + 1) + (c + W)) * (2 * W + 1) + (a + W)
                        key = (int(sc[c + W, a + W]), a * a + c * c, t * t, idx)
                        if best is None or key < best:
                            best = key
            a, c, t = self.candidate(best[3])
            out["cand"][i], out["score"][i] = best[3], best[0]
            out["fix"][i] = (px + float(a * m) * res, py + float(c * m) * res, ppsi + float(t) * self.step_psi)
        return out

    # --- K3l
    def update(self, k, pose, cmd, ranges, state, grid, origin, resolution, length, Ts, field=None):
        """K3l of step k for B cars: pose [B, 3] the true poses, cmd [B, 2] the commands (v, delta) believed executed in step k - 1
        (not read for a car that is not primed), ranges [B, n_beams] K0l's scans of the step in the cars' true worlds (read on a
        scheduled step only; may be None otherwise), state: fresh(B) or what update returned.  -> the new state; nothing is
        changed in place."""
        pose, cmd = np.asarray(pose, float).reshape(-1, 3), np.asarray(cmd, float).reshape(-1, 2)
        B = pose.shape[0]
        out = {key: np.array(v, copy=True) for key, v in state.items()}
        out["cand"][:], out["score"][:], out["hits"][:] = -1, -1, -1
        primed = out["primed"].astype(bool)
        prior = pose.copy()
        for i in np.nonzero(primed)[0]:
            prior[i] = nominal(tuple(float(v) for v in out["fix"][i]), 0.0, float(cmd[i, 0]), float(cmd[i, 1]), 0.0, 0.0, 0.0, length, Ts)[0]
        fix = prior.copy()
        if self.scheduled(k) and primed.any():
            noisy, hit = self.noisy(k, ranges)
            m = self.match(grid, origin, resolution, prior, noisy, hit, field)
            for i in np.nonzero(primed)[0]:
                out["hits"][i] = m["hits"][i]
                out["ranges"][i] = noisy[i]
                if m["cand"][i] < 0:
                    out["lost"][i] += 1
                    continue
                fix[i], out["cand"][i], out["score"][i] = m["fix"][i], m["cand"][i], m["score"][i]
                out["matched"][i] += 1
                a, c, t = self.candidate(m["cand"][i])
                if (self.W > 0 and (abs(a) == self.W or abs(c) == self.W)) or (self.T > 0 and abs(t) == self.T):
                    out["edge"][i] += 1
        out["primed"][:] = 1
        out["fix"], out["prior"] = fix, prior
        out["steps"] += 1
        for i in range(B):
            ex, ey = float(fix[i, 0] - pose[i, 0]), float(fix[i, 1] - pose[i, 1])
            e2 = ex * ex + ey * ey
            out["err2_sum"][i] += e2
            out["err2_max"][i] = max(float(out["err2_max"][i]), e2)
            hd = wrap(float(fix[i, 2]), float(pose[i, 2]))
            out["head2_sum"][i] += hd * hd
            qx, qy = float(prior[i, 0] - pose[i, 0]), float(prior[i, 1] - pose[i, 1])
            out["prior2_sum"][i] += qx * qx + qy * qy
        return out
