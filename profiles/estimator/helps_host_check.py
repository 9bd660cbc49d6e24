"""Do the inputs of tests/test_estimator.py::test_the_estimator_helps satisfy its two inequalities?  Checked without a GPU: the
reference's loop with the project's host classes on the CPU emulation of the solve, one car at a time, around Estimator.apply
(with the estimator) and Plant.apply (without); the lateral error is taken against the waypoint the controller chose.

    python profiles/estimator/helps_host_check.py      # a few minutes"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in ("multi-purpose-mpc_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import mpmpc_testlib as T                                  # noqa: E402
import test_estimator as TE                                # noqa: E402
from estimator import fresh                                # noqa: E402
from spatial_bicycle_models import TemporalState           # noqa: E402

N, B, steps = TE.HELPS["N"], TE.HELPS["B"], TE.HELPS["steps"]
w, s0, poses, plant, est = TE._helps_inputs()
total, worst, not_one = {"with": 0.0, "without": 0.0}, 0.0, 0
for i in range(B):
    for name in ("with", "without"):
        m, rp, car = T.build_world(obstacles=False)
        mpc = T.make_mpc(car, N, backend="emu")
        one_p, one_e = plant.car(i), est.car(i)
        st = dict(pose=poses[i:i + 1].copy(), s=np.array([float(s0[i])]), act=np.zeros((1, 2)), state=fresh(1), u=np.zeros((1, 2)))

        def control(pose_in):
            global not_one
            car.s = float(st["s"][0])
            car.temporal_state = TemporalState(*pose_in[0])
            u = mpc.get_control()
            not_one += int(mpc.last_status != 1)
            return u, [[car.spatial_state.e_y, car.spatial_state.e_psi]], [car.current_waypoint.kappa]
        for k in range(steps):
            before = st["pose"][0].copy()
            if name == "with":
                st = one_e.apply(k, st["pose"], st["s"], st["state"], st["u"], control, car.length, car.Ts, plant=one_p, act=st["act"])
            else:
                st = one_p.apply(k, st["pose"], st["s"], st["act"], control, car.length, car.Ts)
            wp = car.current_waypoint      # (pl_stats: the true pose the step found against the step's waypoint)
            e = np.cos(wp.psi) * (before[1] - wp.y) - np.sin(wp.psi) * (before[0] - wp.x)
            total[name] += e * e
        if name == "with":
            worst = max(worst, st["state"]["err2_sum"][0] / st["state"]["meas2_sum"][0])
print("summed ey^2 with %.4f, without %.4f; worst err2_sum / meas2_sum %.3f; host statuses other than 1: %d" %
      (total["with"], total["without"], worst, not_one))
