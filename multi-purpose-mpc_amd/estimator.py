"""Pose estimator of the device rollout (host side): `Estimator`, what `BatchMPC.rollout(..., estimator=...)` takes - per
car a 3-state extended Kalman filter on the world pose (x, y, psi) in the controller's nominal model, with a measurement
schedule (period, random dropouts) - and restatements of what the device does with it every step (K3e,
csrc/estimator_core.hpp): the schedule (`Estimator.available`), the filter step (`Estimator.update`) and the step around a
controller, composed with plant.Plant and delay.Delay (`Estimator.apply`), for host loops.  One car after the other on python
floats with the C library's cos / sin / tan / fmod, in the header's order, operation for operation.

The law (csrc/estimator_core.hpp is the specification).  State per car: est [3]; cov [6], the upper triangle Pxx, Pxy, Pxp, Pyy,
Pyp, Ppp; primed.  At the start of step k, from z (the plant's measured pose, else the true pose) and (v, delta), the command the
controller believes reached the wheels in step k - 1:
  1  not primed: est = z, cov = (p0_xy, 0, 0, p0_xy, 0, p0_psi), primed; the measurement counts as taken
  2  else the time update: psi0 = est[2]; a = -((v sin psi0) Ts), b = (v cos psi0) Ts; est takes the nominal model's step;
     tx = Pxp + a Ppp, ty = Pyp + b Ppp; Pxx = ((Pxx + a Pxp) + a tx) + q_xy; Pxy = (Pxy + a Pyp) + b tx;
     Pyy = ((Pyy + b Pyp) + b ty) + q_xy; Pxp = tx; Pyp = ty; Ppp = Ppp + q_psi
  3  and, if the measurement is available (j = k - step0 a multiple of period, and not dropped: (w >> 8) 2^-24 >= drop, w word 0
     of Philox block 2 of (seed, car0 + car, j)), three scalar updates in the order x, y, psi: nu = z_i - est_i (psi: wrapped),
     s = P_ii + r_i, g_j = P_ji / s, est_j += g_j nu, P_jl -= g_j P_il
  4  statistics from the true pose: steps, used, err2_sum / err2_max of (est_x - x)^2 + (est_y - y)^2, meas2_sum the same of z,
     head2_sum of the wrapped heading error squared.
"""
from __future__ import annotations

import math

import numpy as np

from delay import nominal, t2s
from plant import philox4x32

NAMES = ("q_xy", "q_psi", "r_xy", "r_psi", "p0_xy", "p0_psi", "period", "drop")
STATS = ("err2_max", "err2_sum", "meas2_sum", "head2_sum")


def wrap(a, b):
    """ro_t2s's e_psi of heading a against heading b: a - b wrapped to [-pi, pi)"""
    return t2s((0.0, 0.0, a), 0.0, 0.0, b)[1]


def fresh(B):
    """-> the state a run of B cars starts from: nobody primed, the statistics zero"""
    B = int(B)
    return dict(est=np.zeros((B, 3)), cov=np.zeros((B, 6)), primed=np.zeros(B, np.int32), err2_max=np.zeros(B), err2_sum=np.zeros(B),
                meas2_sum=np.zeros(B), head2_sum=np.zeros(B), used=np.zeros(B, np.int32), steps=np.zeros(B, np.int32))


class Estimator:
    """The pose filter of a rollout, per car: each parameter a scalar (every car) or one value per car.
    q_xy [m^2], q_psi [rad^2]: process variances added per step (>= 0);  r_xy, r_psi: measurement variances (> 0);  p0_xy,
    p0_psi: the variances a car is primed with (None: r_xy, r_psi - it is primed with a measurement);  period: the measurement
    arrives on the steps with (k - step0) mod period == 0 (an integer >= 1);  drop in [0, 1): the probability that a scheduled
    measurement is lost.  seed, car0, step0: a dropout is a function of (seed, car0 + car, k - step0), k the rollout step index."""

    def __init__(self, q_xy, q_psi, r_xy, r_psi, p0_xy=None, p0_psi=None, period=1, drop=0.0, seed=0, car0=0, step0=0):
        self.values = (q_xy, q_psi, r_xy, r_psi, r_xy if p0_xy is None else p0_xy, r_psi if p0_psi is None else p0_psi, period, drop)
        self.seed, self.car0, self.step0 = int(seed), int(car0), int(step0)

    @classmethod
    def matched(cls, plant, q_xy=1e-6, q_psi=1e-6, **kw):
        """-> the Estimator whose measurement variances are those of `plant`'s pose noise: r = A^2 / 6, the variance of the
        triangular noise of amplitude A (position_noise, heading_noise; both must be > 0)"""
        a_xy, a_psi = (np.asarray(plant.values[c], float) for c in (9, 10))
        if np.any(a_xy <= 0) or np.any(a_psi <= 0):
            raise ValueError("estimator: matched needs a plant with position_noise > 0 and heading_noise > 0")
        return cls(q_xy, q_psi, a_xy * a_xy / 6.0, a_psi * a_psi / 6.0, **kw)

    def params(self, B):
        """-> float64 [B, 8], the block mpmpc.Handle.rollout_set_estimator takes"""
        out = np.empty((int(B), len(NAMES)))
        for c, (name, v) in enumerate(zip(NAMES, self.values)):
            v = np.asarray(v, float)
            if v.ndim > 1 or (v.ndim == 1 and v.size != int(B)):
                raise ValueError("estimator parameter %s must be a scalar or hold one value per car" % name)
            out[:, c] = v
        if np.any(out[:, 6] != np.floor(out[:, 6])) or np.any(out[:, 6] < 1):
            raise ValueError("estimator: period must be an integer >= 1")
        return out

    def car(self, i):
        """-> the Estimator of car i alone (B = 1, car0 moved): what a host loop that drives one car at a time uses"""
        vals = [float(np.asarray(v, float).reshape(-1)[i if np.ndim(v) else 0]) for v in self.values]
        return Estimator(*vals, seed=self.seed, car0=self.car0 + int(i), step0=self.step0)

    def available(self, k, B=None):
        """-> bool [B]: does car i's filter see the measurement of rollout step k (scheduled and not dropped).  B: the number of
        cars (None: that of the per-car parameters, or 1)"""
        B = max([1] + [np.size(v) for v in self.values if np.ndim(v)]) if B is None else int(B)
        p = self.params(B)
        j = int(k) - self.step0
        ju = j & 0xFFFFFFFFFFFFFFFF      # two's complement
        seed = self.seed & 0xFFFFFFFFFFFFFFFF
        ctr = np.zeros((B, 4), np.uint64)
        ctr[:, 0] = [(self.car0 + i) & 0xFFFFFFFF for i in range(B)]
        ctr[:, 1], ctr[:, 2], ctr[:, 3] = ju & 0xFFFFFFFF, ju >> 32, 2
        w = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))[:, 0]
        dropped = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 < p[:, 7]
        scheduled = np.array([j % int(p[i, 6]) == 0 for i in range(B)])      # (python's modulus is non-negative)
        return scheduled & ~dropped

    def update(self, k, z, pose, cmd, state, length, Ts):
        """K3e of step k for B cars: z [B, 3] what the filters measure (the plant's measured poses, else the true ones), pose
        [B, 3] the true poses (statistics), cmd [B, 2] the commands (v, delta) believed executed in step k - 1 (not read for a
        car that is not primed), state: fresh(B) or what update returned.  -> the new state (fresh's keys, and took [B]: a
        measurement was taken); nothing is changed in place."""
        z, pose, cmd = (np.asarray(a, float).reshape(-1, w) for a, w in ((z, 3), (pose, 3), (cmd, 2)))
        B = z.shape[0]
        p, avail = self.params(B), self.available(k, B)
        out = {key: np.array(v, copy=True) for key, v in state.items() if key != "took"}
        out["took"] = np.zeros(B, bool)
        for i in range(B):
            q_xy, q_psi, r_xy, r_psi, p0_xy, p0_psi = (float(v) for v in p[i, :6])
            zi = [float(v) for v in z[i]]
            if not out["primed"][i]:
                est, P, took = list(zi), [p0_xy, 0.0, 0.0, p0_xy, 0.0, p0_psi], True
                out["primed"][i] = 1
            else:
                est, P = [float(v) for v in out["est"][i]], [float(v) for v in out["cov"][i]]
                v, delta = float(cmd[i, 0]), float(cmd[i, 1])
                psi0 = est[2]
                a, b = -((v * math.sin(psi0)) * Ts), (v * math.cos(psi0)) * Ts
                est = list(nominal(tuple(est), 0.0, v, delta, 0.0, 0.0, 0.0, length, Ts)[0])
                tx, ty = P[2] + a * P[5], P[4] + b * P[5]
                P = [((P[0] + a * P[2]) + a * tx) + q_xy, (P[1] + a * P[4]) + b * tx, tx, ((P[3] + b * P[4]) + b * ty) + q_xy, ty,
                     P[5] + q_psi]
                took = bool(avail[i])
                if took:
                    for ch in range(3):
                        row = ((P[0], P[1], P[2]), (P[1], P[3], P[4]), (P[2], P[4], P[5]))[ch]
                        nu = wrap(zi[2], est[2]) if ch == 2 else zi[ch] - est[ch]
                        s = row[ch] + (r_psi if ch == 2 else r_xy)
                        g = [row[0] / s, row[1] / s, row[2] / s]
                        est = [est[0] + g[0] * nu, est[1] + g[1] * nu, est[2] + g[2] * nu]
                        P = [P[0] - g[0] * row[0], P[1] - g[0] * row[1], P[2] - g[0] * row[2], P[3] - g[1] * row[1], P[4] - g[1] * row[2],
                             P[5] - g[2] * row[2]]
            out["est"][i], out["cov"][i], out["took"][i] = est, P, took
            out["steps"][i] += 1
            out["used"][i] += int(took)
            x, y, psi = (float(v) for v in pose[i])
            ex, ey = est[0] - x, est[1] - y
            e2 = ex * ex + ey * ey
            out["err2_sum"][i] += e2
            out["err2_max"][i] = max(float(out["err2_max"][i]), e2)
            mx, my = zi[0] - x, zi[1] - y
            out["meas2_sum"][i] += mx * mx + my * my
            hd = wrap(est[2], psi)
            out["head2_sum"][i] += hd * hd
        return out

    def apply(self, k, pose, s, state, u_last, control, length, Ts, plant=None, act=None, delay=None, queue=None, path=None):
        """One closed-loop step of B cars around a controller, composed with plant.Plant.apply's and delay.Delay.apply's:
        z = plant.measure(k, pose) (no plant: the pose); state = update(k, z, pose, cmd, state) with cmd = u_last [B, 2], the
        controls commanded in the last step (no delay), or queue[:, assumed] (delay: a delay.Delay with queue [B, 8, 2] and path
        a delay.Path); then
          no delay: (u, x0, kappa) = control(est) as Plant.apply's control - the commanded controls [B, 2] with the spatial
                    states and waypoint curvatures they were computed from - and the drive (plant.drive, else the nominal model);
          delay:    pred = delay.predict(est, s, queue); u = control(pred_pose, pred_s) as Delay.apply's control; delay.drive.
        -> dict(pose, s, act, queue, state, meas, u, est) and, under a delay, (executed, pred_pose, pred_s, now)."""
        pose = np.asarray(pose, float).reshape(-1, 3)
        B = pose.shape[0]
        s = np.asarray(s, float).reshape(B)
        meas = pose if plant is None else plant.measure(k, pose)
        if delay is None:
            cmd = np.asarray(u_last, float).reshape(B, 2)
        else:
            queue = np.asarray(queue, float).reshape(B, -1, 2)
            cmd = queue[np.arange(B), np.minimum(delay.arrays(B)[1], queue.shape[1] - 1)]
        state = self.update(k, meas, pose, cmd, state, length, Ts)
        est = state["est"]
        if delay is not None:
            pr = delay.predict(est, s, queue, path, length, Ts)
            u = np.asarray(control(pr["pred_pose"], pr["pred_s"]), float).reshape(-1, 2)
            out = delay.drive(u, pose, s, queue, pr["now"], length, Ts, plant=plant, k=k, act=act)
            out.update(pred_pose=pr["pred_pose"], pred_s=pr["pred_s"], now=pr["now"])
        else:
            u, x0, kappa = control(est)
            u, x0, kappa = np.asarray(u, float).reshape(B, 2), np.asarray(x0, float).reshape(B, -1), np.asarray(kappa, float).reshape(B)
            if plant is not None:
                new, s1, act1 = plant.drive(k, u, pose, s, np.zeros((B, 2)) if act is None else act, x0, kappa, length, Ts)
            else:
                new, s1 = np.zeros((B, 3)), np.zeros(B)
                for i in range(B):
                    new[i], s1[i] = nominal(tuple(float(v) for v in pose[i]), float(s[i]), float(u[i, 0]), float(u[i, 1]), float(x0[i, 0]),
                                            float(x0[i, 1]), float(kappa[i]), length, Ts)
                act1 = u.copy()
            out = dict(pose=new, s=s1, act=act1, queue=None)
        out.update(state=state, meas=meas, u=u, est=est)
        return out
