"""Dynamic single-track plant of the device rollout (host side): `Dynamics`, what `BatchMPC.rollout(..., dynamics=...)` takes -
per car, the mass, yaw inertia, tyres and speed controller of a vehicle that slips and saturates - and a restatement of what
the device does with it every step (K3y, csrc/dynamics_core.hpp): `Dynamics.step`, for host loops, and `Dynamics.drive`, the
plant step around it (plant.Plant.drive's place).  One car after the other on python floats with the C library's sin / cos / tan
/ atan2 / sqrt, in the header's order, operation for operation.
"""
from __future__ import annotations

import math

import numpy as np

NAMES = ("mass", "inertia", "lf", "Cf", "Cr", "mu", "speed_gain", "a_drive", "a_brake", "v_dyn", "substeps")
G = 9.81
MAX_SUBSTEPS = 64
ACC_FIELDS = ("dyn_steps", "sat_front", "sat_rear", "slip_max", "alat_max")


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def new_acc(B):
    """-> the accumulators of B cars before their first step"""
    B = int(B)
    return dict(dyn_steps=np.zeros(B, np.int32), sat_front=np.zeros(B, np.int32), sat_rear=np.zeros(B, np.int32),
                slip_max=np.zeros((B, 2)), alat_max=np.zeros(B))


class Dynamics:
    """The dynamic plant of a rollout, per car: each parameter a scalar (every car) or one value per car.
    mass [kg], inertia [kg m^2] (yaw), lf [m] (centre of gravity to the front axle; lr = the plant's wheelbase - lf), Cf / Cr
    [N / rad] (cornering stiffness), mu (friction coefficient; inf: the tyres never saturate), speed_gain [1 / s] (the speed
    controller's gain; inf: the commanded speed IS the speed, the reference's assumption), a_drive / a_brake [m / s^2] (its
    limits; inf: none), v_dyn [m / s] (below it the car is kinematic; inf: always), substeps (1 .. 64 explicit sub-steps per
    control step).  Dynamics(v_dyn=inf, speed_gain=inf) is the plant alone, bit for bit."""

    def __init__(self, mass=1.0, inertia=0.0025, lf=0.06, Cf=50.0, Cr=50.0, mu=np.inf, speed_gain=np.inf, a_drive=np.inf,
                 a_brake=np.inf, v_dyn=0.5, substeps=16):
        self.values = (mass, inertia, lf, Cf, Cr, mu, speed_gain, a_drive, a_brake, v_dyn, substeps)

    def params(self, B):
        """-> float64 [B, 11], the block mpmpc.Handle.rollout_set_dynamics takes"""
        out = np.empty((int(B), len(NAMES)))
        for c, (name, v) in enumerate(zip(NAMES, self.values)):
            v = np.asarray(v, float)
            if v.ndim > 1 or (v.ndim == 1 and v.size != int(B)):
                raise ValueError("dynamics parameter %s must be a scalar or hold one value per car" % name)
            out[:, c] = v
        n = out[:, 10]
        if not np.all((n >= 1) & (n <= MAX_SUBSTEPS) & (n == np.floor(n))):
            raise ValueError("dynamics: substeps must be integers in [1, %d]" % MAX_SUBSTEPS)
        return out

    def car(self, i):
        """-> the Dynamics of car i alone (B = 1): what a host loop that drives one car at a time uses"""
        return Dynamics(*[float(np.asarray(v, float).reshape(-1)[i if np.ndim(v) else 0]) for v in self.values])

    def stability(self, B, Lp, Ts):
        """-> lambda * Ts / substeps per car [B] (a run needs <= 1), lambda = max((Cf + Cr) / (m v_dyn), (lf^2 Cf + lr^2 Cr) /
        (Iz v_dyn)); Lp: the plant's wheelbase, a scalar or [B]"""
        p = self.params(B)
        Lp = np.broadcast_to(np.asarray(Lp, float), (int(B),))
        lf, lr = p[:, 2], Lp - p[:, 2]
        lam = np.maximum((p[:, 3] + p[:, 4]) / (p[:, 0] * p[:, 9]), (lf * lf * p[:, 3] + lr * lr * p[:, 4]) / (p[:, 1] * p[:, 9]))
        return lam * Ts / p[:, 10]

    def step(self, v_act, d_act, state, pose, Lp, Ts, acc=None, probe=None):
        """Steps 2 - 4 of the header for B cars: v_act, d_act [B] what the actuators do, state [B, 3] = (vx, vy, r), pose [B, 3]
        the true poses, Lp the plant's wheelbase (a scalar or [B]).  acc: new_acc(B) or what an earlier step returned (None:
        new).  probe: None, or dict(switch [B], clip [B]) that is lowered in place to the smallest |vx - v_dyn| at a branch
        decision and the smallest relative distance | |F| - cap | / cap of a tyre force from its clip (the two lateral forces,
        and the traction force that sets the rear cap; finite caps only) - how far the car stayed from its decisions.
        -> (state, pose, acc, dynamic [B] bool: which branch was taken); nothing else is changed in place."""
        state, pose = np.array(state, float).reshape(-1, 3), np.array(pose, float).reshape(-1, 3)
        B = pose.shape[0]
        v_act, d_act = (np.broadcast_to(np.asarray(a, float), (B,)) for a in (v_act, d_act))
        Lps = np.broadcast_to(np.asarray(Lp, float), (B,))
        prm = self.params(B)
        acc = new_acc(B) if acc is None else {k: np.array(v) for k, v in acc.items()}
        dynamic = np.zeros(B, bool)
        Ts = float(Ts)
        for i in range(B):
            m, Iz, lf, Cf, Cr, mu, k_a, a_drive, a_brake, v_dyn, n = (float(v) for v in prm[i])
            Lp_i, va, da = float(Lps[i]), float(v_act[i]), float(d_act[i])
            lr = Lp_i - lf
            ideal = k_a == math.inf
            vx, vy, r = (float(v) for v in state[i])
            x, y, psi = (float(v) for v in pose[i])
            if ideal:
                vx = va
            if probe is not None:
                probe["switch"][i] = min(probe["switch"][i], abs(vx - v_dyn))
            if not vx >= v_dyn:
                if not ideal:
                    vx += _clamp(k_a * (va - vx), -a_brake, a_drive) * Ts
                r = vx / Lp_i * math.tan(da)
                x, y, psi = x + (vx * math.cos(psi)) * Ts, y + (vx * math.sin(psi)) * Ts, psi + r * Ts
                vy = lr * r
            else:
                dynamic[i] = True
                n = int(n)
                Fzf, Fzr = m * G * lr / Lp_i, m * G * lf / Lp_i
                cap_f, cap_x = mu * Fzf, mu * Fzr
                sd, cd = math.sin(da), math.cos(da)
                h = Ts / n
                sat_f = sat_r = False
                slip_f, slip_r, alat = float(acc["slip_max"][i, 0]), float(acc["slip_max"][i, 1]), float(acc["alat_max"][i])
                for _ in range(n):
                    Fraw = 0.0 if ideal else m * _clamp(k_a * (va - vx), -a_brake, a_drive)
                    Fx = _clamp(Fraw, -cap_x, cap_x)      # (0 stays 0)
                    a_f = da - math.atan2(vy + lf * r, vx)
                    a_r = -math.atan2(vy - lr * r, vx)
                    cap_r = math.sqrt(max(cap_x * cap_x - Fx * Fx, 0.0))
                    Ff, Fr = Cf * a_f, Cr * a_r
                    Fyf, Fyr = _clamp(Ff, -cap_f, cap_f), _clamp(Fr, -cap_r, cap_r)
                    sat_f, sat_r = sat_f or abs(Ff) > cap_f, sat_r or abs(Fr) > cap_r
                    if probe is not None:
                        for F, cap in ((Ff, cap_f), (Fr, cap_r)) + (() if ideal else ((Fraw, cap_x),)):
                            if cap < math.inf:      # (a cap of 0 - all grip spent on traction - clips whatever is not 0)
                                gap = abs(abs(F) - cap) / cap if cap > 0.0 else (math.inf if F != 0.0 else 0.0)
                                probe["clip"][i] = min(probe["clip"][i], gap)
                    t = Fyf * cd
                    dvx = (Fx - Fyf * sd) / m + vy * r
                    dvy = (t + Fyr) / m - vx * r
                    dr = (lf * t - lr * Fyr) / Iz
                    slip_f, slip_r, alat = max(slip_f, abs(a_f)), max(slip_r, abs(a_r)), max(alat, abs(t + Fyr) / m)
                    if not ideal:
                        vx += dvx * h
                    vy += dvy * h
                    r += dr * h
                    w = vy - lr * r
                    c, s = math.cos(psi), math.sin(psi)
                    x, y, psi = x + (vx * c - w * s) * h, y + (vx * s + w * c) * h, psi + r * h
                acc["dyn_steps"][i] += 1
                acc["sat_front"][i] += int(sat_f)
                acc["sat_rear"][i] += int(sat_r)
                acc["slip_max"][i] = (slip_f, slip_r)
                acc["alat_max"][i] = alat
            state[i], pose[i] = (vx, vy, r), (x, y, psi)
        return state, pose, acc, dynamic

    def drive(self, plant, k, u, pose, s, act, state, x0, kappa, length, Ts, acc=None, probe=None):
        """The dynamic plant step of step k for B cars, plant.Plant.drive's place: the plant's steps 2 - 7 on u (its gains,
        noise, lags and rate limit: Plant.drive's own, evaluated on a scratch pose), then `step` with the plant's wheelbase,
        then the wheel odometry on the step's final vx.  -> dict(pose, s, act, state, acc, dynamic)."""
        pose = np.asarray(pose, float).reshape(-1, 3)
        B = pose.shape[0]
        s, kappa = np.asarray(s, float).reshape(B), np.asarray(kappa, float).reshape(B)
        x0 = np.asarray(x0, float).reshape(B, -1)
        act1 = plant.drive(k, u, np.zeros((B, 3)), np.zeros(B), act, np.zeros((B, 2)), np.zeros(B), length, Ts)[2]
        Lp = length * plant.params(B)[:, 3]
        st, new, acc, dynamic = self.step(act1[:, 0], act1[:, 1], state, pose, Lp, Ts, acc, probe)
        s1 = np.array([float(s[i]) + (1.0 / (1.0 - float(x0[i, 0]) * float(kappa[i])) * float(st[i, 0]) * math.cos(float(x0[i, 1]))) * float(Ts)
                       for i in range(B)])
        return dict(pose=new, s=s1, act=act1, state=st, acc=acc, dynamic=dynamic)
