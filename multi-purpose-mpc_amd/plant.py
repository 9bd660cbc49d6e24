"""Plant models of the device rollout (host side): `Plant`, what `BatchMPC.rollout(..., plant=...)` takes - the vehicle that
differs from the controller's model, per car - and numpy restatements of what the device does with it every step (K3n / K3p,
csrc/plant_core.hpp): the draws (`Plant.noise`), the measured pose (`Plant.measure`), the plant step (`Plant.drive`) and both
around a controller (`Plant.apply`), for host loops.  A draw is a function of (seed, car0 + car, k - step0, channel) alone, so
the noise of any step of a run can be recomputed from its index, e.g. to replay one car on the host.
"""
from __future__ import annotations

import numpy as np

NAMES = ("speed_gain", "steer_gain", "steer_offset", "wheelbase_scale", "speed_lag", "steer_lag", "steer_rate",
         "speed_noise", "steer_noise", "position_noise", "heading_noise")
IDENTITY = (1.0, 1.0, 0.0, 1.0, 1.0, 1.0, np.inf, 0.0, 0.0, 0.0, 0.0)
CHANNELS = ("n_v", "n_delta", "n_x", "n_y", "n_psi")

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10 on arrays: counter [..., 4], key [..., 2] (32-bit words held in uint64) -> uint32 [..., 4]."""
    c = [np.asarray(counter, np.uint64)[..., i] & _LO for i in range(4)]
    k = [np.asarray(key, np.uint64)[..., i] & _LO for i in range(2)]
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _LO, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _LO]
        k = [(k[0] + _W0) & _LO, (k[1] + _W1) & _LO]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def variate(w):
    """one 32-bit word -> the sum of its two 16-bit halves, centred and scaled: triangular on (-1, 1), exact in double"""
    w = np.asarray(w, np.uint32).astype(np.int64)
    return ((w >> 16) + (w & 0xFFFF) - 65535).astype(np.float64) * 2.0 ** -16


def noise(seed, car0, B, j):
    """(n_v, n_delta, n_x, n_y, n_psi) of cars car0 .. car0 + B - 1 at j = k - step0 (an int or an array of them)
    -> float64 [len(j), B, 5].  The device's draws (csrc/plant_core.hpp), bit for bit."""
    j = np.atleast_1d(np.asarray(j, dtype=object))
    ju = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in j], np.uint64)      # two's complement
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    car = np.array([(int(car0) + i) & 0xFFFFFFFF for i in range(int(B))], np.uint64)
    ctr = np.zeros((ju.size, car.size, 4), np.uint64)
    ctr[..., 0] = car[None, :]
    ctr[..., 1] = (ju & _LO)[:, None]
    ctr[..., 2] = (ju >> _S32)[:, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    b0 = philox4x32(ctr, key)
    ctr[..., 3] = 1
    b1 = philox4x32(ctr, key)
    return np.concatenate([variate(b0), variate(b1[..., :1])], -1)


class Plant:
    """The true vehicle of a rollout, per car: each parameter a scalar (every car) or one value per car.
    speed_gain / steer_gain / steer_offset [rad]: v = gain * v_cmd, delta = gain * delta_cmd + offset;  wheelbase_scale: the
    true wheelbase over the model's;  speed_lag / steer_lag in (0, 1]: act += lag * (target - act) per control step (1: no
    lag);  steer_rate [rad / step]: the most the steering angle changes in one step (inf: no limit);  speed_noise [m/s],
    steer_noise [rad], position_noise [m], heading_noise [rad]: amplitudes of the triangular noise on (-1, 1) (standard
    deviation amplitude / sqrt 6) added to the commands and to the pose the controller localises on.
    seed, car0, step0: a draw is a function of (seed, car0 + car, k - step0, channel), k the rollout step index."""

    def __init__(self, speed_gain=1.0, steer_gain=1.0, steer_offset=0.0, wheelbase_scale=1.0, speed_lag=1.0, steer_lag=1.0,
                 steer_rate=np.inf, speed_noise=0.0, steer_noise=0.0, position_noise=0.0, heading_noise=0.0, seed=0, car0=0,
                 step0=0):
        self.values = (speed_gain, steer_gain, steer_offset, wheelbase_scale, speed_lag, steer_lag, steer_rate, speed_noise,
                       steer_noise, position_noise, heading_noise)
        self.seed, self.car0, self.step0 = int(seed), int(car0), int(step0)

    def params(self, B):
        """-> float64 [B, 11], the block mpmpc.Handle.rollout_set_plant takes"""
        out = np.empty((int(B), len(NAMES)))
        for c, (name, v) in enumerate(zip(NAMES, self.values)):
            v = np.asarray(v, float)
            if v.ndim > 1 or (v.ndim == 1 and v.size != int(B)):
                raise ValueError("plant parameter %s must be a scalar or hold one value per car" % name)
            out[:, c] = v
        return out

    def car(self, i):
        """-> the Plant of car i alone (B = 1, car0 moved): what a host loop that drives one car at a time uses"""
        vals = [float(np.asarray(v, float).reshape(-1)[i if np.ndim(v) else 0]) for v in self.values]
        return Plant(*vals, seed=self.seed, car0=self.car0 + int(i), step0=self.step0)

    def noise(self, B, steps):
        """The draws of rollout steps k = 0 .. steps - 1 (an int) or of the step indices `steps` (an array)
        -> float64 [len, B, 5] = (n_v, n_delta, n_x, n_y, n_psi)."""
        k = range(int(steps)) if np.ndim(steps) == 0 else [int(v) for v in np.asarray(steps, dtype=object).reshape(-1)]
        return noise(self.seed, self.car0, B, [v - self.step0 for v in k])

    def measure(self, k, pose):
        """-> the poses [B, 3] the controllers localise on at step k, from the true poses"""
        pose = np.asarray(pose, float).reshape(-1, 3)
        p, n = self.params(pose.shape[0]), self.noise(pose.shape[0], [k])[0]
        return np.stack([pose[:, 0] + p[:, 9] * n[:, 2], pose[:, 1] + p[:, 9] * n[:, 3], pose[:, 2] + p[:, 10] * n[:, 4]], 1)

    def drive(self, k, u, pose, s, act, x0, kappa, length, Ts):
        """The plant step of step k for B cars: u [B, 2] the commanded (v, delta), pose [B, 3] and s [B] the true poses and
        the arc lengths, act [B, 2] the executed (v, delta) so far, x0 [B, >= 2] and kappa [B] the controllers' spatial states
        (of the measured poses) and the curvatures of their waypoints, length the model's wheelbase.
        -> (pose, s, act) after the step; nothing is changed in place.  csrc/plant_core.hpp's order, operation for operation."""
        u, pose, act = (np.asarray(a, float).reshape(-1, w) for a, w in ((u, 2), (pose, 3), (act, 2)))
        B = pose.shape[0]
        s, kappa = np.asarray(s, float).reshape(B), np.asarray(kappa, float).reshape(B)
        x0 = np.asarray(x0, float).reshape(B, -1)
        p, n = self.params(B), self.noise(B, [k])[0]
        with np.errstate(invalid="ignore"):      # (inf - inf in the branch an infinite rate never takes)
            v_t = p[:, 0] * u[:, 0] + p[:, 7] * n[:, 0]
            d_t = (p[:, 1] * u[:, 1] + p[:, 2]) + p[:, 8] * n[:, 1]
            v_act = np.where(p[:, 4] == 1.0, v_t, act[:, 0] + p[:, 4] * (v_t - act[:, 0]))
            d_new = np.where(p[:, 5] == 1.0, d_t, act[:, 1] + p[:, 5] * (d_t - act[:, 1]))
            d = d_new - act[:, 1]
            d_act = np.where(np.abs(d) > p[:, 6], act[:, 1] + np.copysign(p[:, 6], d), d_new)
        Lp = length * p[:, 3]
        psi = pose[:, 2]
        new = np.stack([pose[:, 0] + (v_act * np.cos(psi)) * Ts, pose[:, 1] + (v_act * np.sin(psi)) * Ts,
                        pose[:, 2] + (v_act / Lp * np.tan(d_act)) * Ts], 1)
        s_dot = 1.0 / (1.0 - x0[:, 0] * kappa) * v_act * np.cos(x0[:, 1])
        return new, s + s_dot * Ts, np.stack([v_act, d_act], 1)

    def apply(self, k, pose, s, act, control, length, Ts):
        """One closed-loop step of B cars around a controller: meas = measure(k, pose); (u, x0, kappa) = control(meas), the
        commanded controls [B, 2] with the spatial states and waypoint curvatures they were computed from; then drive.
        -> dict(pose, s, act, meas, u)."""
        meas = self.measure(k, pose)
        u, x0, kappa = control(meas)
        new, s1, act1 = self.drive(k, u, pose, s, act, x0, kappa, length, Ts)
        return dict(pose=new, s=s1, act=act1, meas=meas, u=np.asarray(u, float).reshape(-1, 2))
