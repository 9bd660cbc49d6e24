"""MPC.get_control() host logic (src/MPC.py:161-222) against the reference's own closed loop
(golden G6: src/simulation.py's while-loop driven through the reference classes, teacher-forced
per step).  The solver behind the controller is the CPU emulation of the HIP kernels here; the
-m gpu twin runs the same lap through libmpmpc.so."""
import numpy as np
import pytest

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
from MPC import MPC
from spatial_bicycle_models import TemporalState

G = M.GOLDEN


@pytest.mark.parametrize("N,stride", [(10, 1), (30, 3)])
def test_get_control_reproduces_reference_lap(N, stride):
    """The reference's own loop with a solver that returns the CERTIFIED optimum and reports every proven infeasibility
    (golden G6: stand-in = the oracle with polish and phase 1): controls, plans, predictions, counters, step by step.
    phase1_accept = 0 is that solver's verdict semantics; the default (marginal infeasibility -> usable plan, like the
    reference's OSQP call at eps = 1e-3) is pinned by the STOCK lap below."""
    g = np.load(G + "/g6_closed_loop_N%d.npz" % N)
    m, rp, car = T.build_world()
    mpc = T.make_mpc(car, N, "emu", settings=mpmpc.default_settings(phase1_accept=0))
    steps = range(0, g["s"].size, stride)
    n_inf = 0
    for t in steps:
        car.s = float(g["s"][t])
        car.temporal_state = TemporalState(*g["pose"][t])
        mpc.current_control = g["cc_prev"][t].copy()
        mpc.infeasibility_counter = int(g["counter"][t - 1]) if t > 0 else 0
        u = mpc.get_control()
        assert car.wp_id == g["wp_id"][t]
        assert np.allclose(np.array(car.spatial_state[:]), g["x0"][t], atol=1e-13)
        assert mpc.infeasibility_counter == g["counter"][t]
        ref_ok = g["status"][t] > 0
        assert (mpc.last_status > 0) == ref_ok, (t, mpc.last_status, g["status"][t])
        assert np.max(np.abs(u - g["u"][t])) <= 1e-6, (t, u, g["u"][t])
        if ref_ok:
            d = np.abs(mpc.current_control - g["cc_next"][t])
            d[-1] = 0.0                                   # kappa_{N-1} is cost free
            assert d.max() <= 1e-6
            # MPC.update_prediction (src/MPC.py:224-248): the reference's own (x_pred, y_pred) of this step
            px, py = mpc.current_prediction
            assert len(px) == len(py) == N - 2
            assert np.max(np.abs(np.array(px) - g["pred_x"][t])) <= 1e-6 and np.max(np.abs(np.array(py) - g["pred_y"][t])) <= 1e-6
        else:
            n_inf += 1
            assert np.array_equal(mpc.current_control, g["cc_prev"][t])
    assert n_inf > 0           # the fallback branch (src/MPC.py:208-216) was exercised


@pytest.mark.parametrize("N,stride", [(10, 1), (30, 1)])
def test_default_path_takes_the_branch_stock_osqp_takes(N, stride):
    """golden G6s is the reference's loop run with the restated OSQP at ITS DEFAULTS (eps 1e-3, no
    polish, no phase 1: the arithmetic of src/MPC.py:159,183).  Every recorded step, teacher-forced through
    MPC.get_control with the build's DEFAULT settings, must take the same branch of src/MPC.py:185-220 - fresh plan or
    fallback - and keep the same infeasibility counter.  (OSQP at 1e-3 accepts corridor violations of millimetres; the
    default path returns MPMPC_SOLVED_INACCURATE for those instead of a Farkas verdict: mpmpc_settings::phase1_accept.)"""
    g = np.load(G + "/g6s_stock_loop_N%d.npz" % N)
    m, rp, car = T.build_world()
    mpc = T.make_mpc(car, N, "emu")
    seen = set()
    for t in range(0, g["s"].size, stride):
        car.s = float(g["s"][t])
        car.temporal_state = TemporalState(*g["pose"][t])
        mpc.current_control = g["cc_prev"][t].copy()
        mpc.infeasibility_counter = int(g["counter"][t - 1]) if t > 0 else 0
        u = mpc.get_control()
        assert car.wp_id == g["wp_id"][t]
        assert np.allclose(np.array(car.spatial_state[:]), g["x0"][t], atol=1e-13)
        assert (mpc.last_status > 0) == (g["status"][t] > 0), (t, mpc.last_status, g["status"][t])
        assert mpc.infeasibility_counter == g["counter"][t], t
        seen.add(int(mpc.last_status))
        if g["status"][t] > 0:
            assert abs(u[0] - g["u"][t][0]) <= 5e-3      # the speed channel is well conditioned: OSQP at 1e-3 has it
        else:
            assert np.array_equal(u, g["u"][t])          # the replayed entry of the previous plan
    assert 2 in seen           # marginal instances occurred and were handed back as usable plans
    if N == 30:
        assert -3 in seen      # ... and the ones OSQP itself refuses are still refused


def test_exit_after_n_minus_one_infeasible_steps():
    """src/MPC.py:218-220: the reference's lap at N=10 ends with exit(1); so does ours."""
    g = np.load(G + "/g6_closed_loop_N10.npz")
    assert bool(g["exited"][0])
    m, rp, car = T.build_world()
    mpc = T.make_mpc(car, 10, "emu")
    t = g["s"].size - 1
    # replay the recorded last good state, then drive freely: the run must stop with SystemExit
    car.s = float(g["s"][t])
    car.temporal_state = TemporalState(*g["pose"][t])
    mpc.current_control = g["cc_prev"][t].copy()
    mpc.infeasibility_counter = int(g["counter"][t - 1])
    with pytest.raises(SystemExit):
        for _ in range(12):
            u = mpc.get_control()
            car.drive(u)


def test_rejects_unsupported_weights_and_missing_profile():
    m, rp, car = T.build_world()
    from scipy import sparse
    ic = {'umin': np.array([0.0, -1.0]), 'umax': np.array([1.0, 1.0])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    Qbad = np.array([[1.0, 0.1, 0], [0.1, 0, 0], [0, 0, 0]])          # indefinite: 1 x 0 - 0.01 < 0
    with pytest.raises(ValueError):
        MPC(car, 10, Qbad, sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0, 0]), sc, ic, 4.0, backend=object())
    with pytest.raises(ValueError):                                    # not symmetric
        MPC(car, 10, np.array([[1.0, 0.1, 0], [0.2, 1, 0], [0, 0, 0]]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0, 0]), sc, ic, 4.0,
            backend=object())
    # a symmetric positive semidefinite Q / R with off-diagonal entries is taken, like in the reference (src/MPC.py:150)
    mpc = MPC(car, 10, np.array([[1.0, 0.1, 0], [0.1, 0.5, 0], [0, 0, 0]]), np.array([[0.5, 0.05], [0.05, 0.1]]), sparse.diags([1.0, 0, 0]),
              sc, ic, 4.0, backend=object())
    assert list(mpc._cfg.Q_offdiag) == [0.1, 0.0, 0.0] and list(mpc._cfg.R_offdiag) == [0.05] and list(mpc._cfg.Q) == [1.0, 0.5, 0.0]
    with pytest.raises(ValueError):
        MPC(car, 2, sparse.diags([1.0, 0, 0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0, 0]), sc, ic, 4.0,
            backend=object())


def test_product_fails_loudly_without_device():
    """No CPU fallback behind the product classes: constructing the controller without a HIP
    device (this container) must raise, not silently compute elsewhere."""
    if mpmpc.device_count() > 0:
        pytest.skip("a GPU is present")
    m, rp, car = T.build_world()
    with pytest.raises((mpmpc.MpmpcError, RuntimeError)):
        T.make_mpc(car, 10, backend=None)
