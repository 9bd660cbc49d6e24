"""Actuation delay of the device rollout and its compensation (host side): `Delay`, what `BatchMPC.rollout(..., delay=...)`
takes - per car, how many control steps a command needs to reach the wheels and how many the controller assumes - and
restatements of what the device does with it every step (K3d / K3q, csrc/delay_core.hpp): the prediction through the
commands in flight (`Delay.predict`), the step of the command register and the car (`Delay.drive`) and both around a
controller (`Delay.apply`, with or without a plant.Plant), for host loops.  One car after the other on python floats with
the C library's cos / sin / tan / fmod, in the header's order, operation for operation.
"""
from __future__ import annotations

import math

import numpy as np

DELAY_MAX = 8


def current_waypoint(cum, s):
    """csrc/rollout_core.hpp's ro_current_waypoint: the closer of the two waypoints enclosing s (ties: the earlier), -1 past the end"""
    n = len(cum)
    nxt = int(np.searchsorted(cum, s, side="right"))      # first index with cum > s
    if nxt >= n:
        return -1
    prv = nxt - 1
    c_prev = cum[prv] if prv >= 0 else cum[n - 1]
    if abs(s - cum[nxt]) < abs(s - c_prev):
        return nxt
    return prv if prv >= 0 else n - 1


def t2s(pose, wx, wy, wpsi):
    """ro_t2s -> (e_y, e_psi)"""
    e_y = math.cos(wpsi) * (pose[1] - wy) - math.sin(wpsi) * (pose[0] - wx)
    t = math.fmod(pose[2] - wpsi + math.pi, 2.0 * math.pi)
    if t < 0.0:
        t += 2.0 * math.pi
    return e_y, t - math.pi


def nominal(pose, s, v, delta, e_y, e_psi, kappa, length, Ts):
    """ro_drive's pose update and s update -> (pose, s)"""
    psi = pose[2]
    new = (pose[0] + (v * math.cos(psi)) * Ts, pose[1] + (v * math.sin(psi)) * Ts, pose[2] + (v / length * math.tan(delta)) * Ts)
    s_dot = 1.0 / (1.0 - e_y * kappa) * v * math.cos(e_psi)
    return new, s + s_dot * Ts


class Path:
    """The tables K3d reads: cum (cumulative segment lengths), x, y, psi, kappa per waypoint; for route fleets all routes laid
    end to end with first [B] / n_wp [B], every car's first row and its route's length (None: one path for every car)."""

    def __init__(self, cum, x, y, psi, kappa, first=None, n_wp=None):
        self.cum, self.x, self.y, self.psi, self.kappa = (np.asarray(a, float).reshape(-1) for a in (cum, x, y, psi, kappa))
        self.first = None if first is None else np.asarray(first, int).reshape(-1)
        self.n_wp = None if n_wp is None else np.asarray(n_wp, int).reshape(-1)

    def car(self, i):
        """-> (first row, number of waypoints) of car i"""
        return (0, self.cum.size) if self.first is None else (int(self.first[i]), int(self.n_wp[i]))


class Delay:
    """The latency of a rollout, per car: steps - the control steps a command needs to reach the wheels (d, 0 .. 8); assumed -
    what the controller compensates for (c, 0 .. 8; None: c = d; 0: no compensation); each a scalar (every car) or one value
    per car.  queue0 [B, 8, 2] (or [8, 2] for every car): the commands (v, delta) in flight when the run starts, queue0[:, i]
    issued i + 1 steps before it - the first d executions are queue0[:, d - 1] .. queue0[:, 0]; None: zeros, the car stands for
    d steps."""

    def __init__(self, steps, assumed=None, queue0=None):
        self.steps, self.assumed, self.queue0 = steps, assumed, queue0

    def arrays(self, B):
        """-> (delay int32 [B], assumed int32 [B], queue0 float64 [B, 8, 2] or None): what mpmpc.Handle.rollout_set_delay takes"""
        B = int(B)
        out = []
        for name, v in (("steps", self.steps), ("assumed", self.steps if self.assumed is None else self.assumed)):
            v = np.asarray(v)
            if v.ndim > 1 or (v.ndim == 1 and v.size != B):
                raise ValueError("delay: %s must be a scalar or hold one value per car" % name)
            if not np.array_equal(v, np.floor(v)) or np.any(v < 0) or np.any(v > DELAY_MAX):
                raise ValueError("delay: %s must be integers in [0, %d]" % (name, DELAY_MAX))
            out.append(np.ascontiguousarray(np.broadcast_to(v.astype(np.int32), (B,))))
        q = None
        if self.queue0 is not None:
            q = np.asarray(self.queue0, float)
            if q.shape == (DELAY_MAX, 2):
                q = np.broadcast_to(q, (B, DELAY_MAX, 2))
            if q.shape != (B, DELAY_MAX, 2):
                raise ValueError("delay: queue0 must be [B, 8, 2] or [8, 2]")
            q = np.ascontiguousarray(q)
        return out[0], out[1], q

    def queue(self, B):
        """-> the registers a run of B cars starts from, float64 [B, 8, 2]"""
        q = self.arrays(B)[2]
        return np.zeros((int(B), DELAY_MAX, 2)) if q is None else q.copy()

    def car(self, i):
        """-> the Delay of car i alone (B = 1): what a host loop that drives one car at a time uses"""
        pick = lambda v: None if v is None else int(np.asarray(v).reshape(-1)[i if np.ndim(v) else 0])
        q = None if self.queue0 is None else np.asarray(self.queue0, float)
        if q is not None and q.ndim == 3:
            q = q[i]
        return Delay(pick(self.steps), pick(self.assumed), q)

    def predict(self, pose, s, queue, path, length, Ts):
        """K3d for B cars: pose [B, 3] the poses the controllers localise on (the measured ones under a plant), s [B], queue
        [B, 8, 2] the registers, path a delay.Path.  -> dict(pred_pose [B, 3], pred_s [B], now [B, 3], now_wp [B], wp [B]): what
        the controllers plan from; (e_y, e_psi, kappa) of the waypoint the car is at and that waypoint's row in the tables; the
        same waypoint within the car's route (-1: s is past the end - pred is the input, now is NaN, now_wp -1)."""
        pose = np.asarray(pose, float).reshape(-1, 3)
        B = pose.shape[0]
        s, queue = np.asarray(s, float).reshape(B), np.asarray(queue, float).reshape(B, DELAY_MAX, 2)
        _, assumed, _ = self.arrays(B)
        out = dict(pred_pose=np.zeros((B, 3)), pred_s=np.zeros(B), now=np.full((B, 3), np.nan), now_wp=np.full(B, -1), wp=np.full(B, -1))
        for i in range(B):
            first, n = path.car(i)
            cum = path.cum[first:first + n]
            P, S = tuple(float(v) for v in pose[i]), float(s[i])
            wp = current_waypoint(cum, S)
            out["wp"][i] = wp
            if wp >= 0:
                r = first + wp
                e_y, e_psi = t2s(P, path.x[r], path.y[r], path.psi[r])
                out["now"][i] = (e_y, e_psi, path.kappa[r])
                out["now_wp"][i] = r
                for j in range(int(assumed[i]) - 1, -1, -1):      # the oldest command in flight first
                    P, S = nominal(P, S, float(queue[i, j, 0]), float(queue[i, j, 1]), e_y, e_psi, float(path.kappa[first + wp]), length, Ts)
                    if j > 0:
                        wp = current_waypoint(cum, S)
                        if wp < 0:
                            break
                        r = first + wp
                        e_y, e_psi = t2s(P, path.x[r], path.y[r], path.psi[r])
            out["pred_pose"][i], out["pred_s"][i] = P, S
        return out

    def drive(self, u, pose, s, queue, now, length, Ts, plant=None, k=0, act=None):
        """K3q's steps 2 - 5 for B driven cars: u [B, 2] the commanded (v, delta), pose [B, 3] and s [B] the TRUE poses and the
        arc lengths, queue [B, 8, 2], now [B, 3] predict's.  plant: a plant.Plant with k (the step) and act [B, 2], or None.
        -> dict(pose, s, queue, executed [B, 2], act); nothing is changed in place."""
        u, pose = np.asarray(u, float).reshape(-1, 2), np.asarray(pose, float).reshape(-1, 3)
        B = pose.shape[0]
        s, queue, now = np.asarray(s, float).reshape(B), np.asarray(queue, float).reshape(B, DELAY_MAX, 2), np.asarray(now, float).reshape(B, 3)
        d = self.arrays(B)[0]
        ex = np.array([queue[i, d[i] - 1] if d[i] > 0 else u[i] for i in range(B)]).reshape(B, 2)
        new_q = np.concatenate([u[:, None, :], queue[:, :-1]], axis=1)
        if plant is not None:
            new_pose, new_s, new_act = plant.drive(k, ex, pose, s, np.zeros((B, 2)) if act is None else act, now[:, :2], now[:, 2], length, Ts)
            return dict(pose=new_pose, s=new_s, queue=new_q, executed=ex, act=new_act)
        new_pose, new_s = np.zeros((B, 3)), np.zeros(B)
        for i in range(B):
            new_pose[i], new_s[i] = nominal(tuple(float(v) for v in pose[i]), float(s[i]), float(ex[i, 0]), float(ex[i, 1]), float(now[i, 0]),
                                            float(now[i, 1]), float(now[i, 2]), length, Ts)
        return dict(pose=new_pose, s=new_s, queue=new_q, executed=ex, act=ex.copy())

    def apply(self, k, pose, s, queue, control, path, length, Ts, plant=None, act=None):
        """One closed-loop step of B cars around a controller, composed with plant.Plant.apply's: meas = plant.measure(k, pose)
        (no plant: the pose); pred = predict(meas, s, queue); u = control(pred_pose, pred_s), the commanded controls [B, 2] of
        controllers that localise on the prediction; then drive.
        -> dict(pose, s, queue, act, meas, u, executed, pred_pose, pred_s, now)."""
        pose = np.asarray(pose, float).reshape(-1, 3)
        meas = pose if plant is None else plant.measure(k, pose)
        pr = self.predict(meas, s, queue, path, length, Ts)
        u = np.asarray(control(pr["pred_pose"], pr["pred_s"]), float).reshape(-1, 2)
        out = self.drive(u, pose, s, queue, pr["now"], length, Ts, plant=plant, k=k, act=act)
        out.update(meas=meas, u=u, pred_pose=pr["pred_pose"], pred_s=pr["pred_s"], now=pr["now"])
        return out
