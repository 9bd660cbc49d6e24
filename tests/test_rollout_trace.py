"""The recorder of the device rollout (mpmpc_rollout_record / _recorded / _trace): one record per car and recorded step,
written by two small kernels around the step, with the predicted path (MPC.update_prediction) computed on the device.

CPU: the record code of csrc/rollout_core.hpp on the host (tests/emul_trace) against the reference's own per-step records
(golden G6: z, wp_id, status -> pred_x / pred_y) and against the masking table of include/mpmpc.h.  GPU: the trace of a
rollout against the reference (G6, G6o, G6r teacher-forced) and, bit for bit, against rollout_step(1) + rollout_state()
in a host loop on a second handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mpc_np as M
import mpmpc
import mpmpc_testlib as T
import scenarios
import twins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ip = C.POINTER(C.c_int32)
E_ARG, E_STATE = -1, -3
PLAN, PRED, ROWS = 1, 2, 4
BASIC = ("s", "pose", "wp_id", "x0", "u", "status", "counter", "alive")
ALL = BASIC + ("plan", "pred_x", "pred_y", "ub", "lb")
INTS = ("wp_id", "status", "counter", "alive")


_d, _i = T._d, T._i


def _usable(status):
    return np.isin(status, (1, 2, -2))


def _eq(a, b):
    """bit-equal, NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))


@pytest.fixture(scope="module")
def twin():
    """The CPU twin of the recorder kernels (tests/emul_trace)."""
    return twins.trace()


def _twin_record(twin, N, fields, g1, circular, s, pose, a_in, alive, wp_id, status, counter, x0, u, cc, z, row_ub, row_lb,
                 per_car=False):
    B = np.asarray(s).size
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    gx, gy, gpsi = f64(g1["x"]), f64(g1["y"]), f64(g1["psi"])
    row_ub, row_lb = f64(row_ub), f64(row_lb)
    shape = dict(s=(), pose=(3,), wp_id=(), x0=(3,), u=(2,), status=(), counter=(), alive=(), plan=(2 * N,),
                 pred_x=(N - 2,), pred_y=(N - 2,), ub=(N,), lb=(N,))
    have = set(BASIC) | ({"plan"} if fields & PLAN else set()) | ({"pred_x", "pred_y"} if fields & PRED else set()) | \
        ({"ub", "lb"} if fields & ROWS else set())
    out = {k: (np.full((B,) + shape[k], 77, np.int32) if k in INTS else np.full((B,) + shape[k], 77.0)) for k in have}
    o = {k: (_i(out[k]) if k in INTS else _d(out[k])) if k in out else None for k in shape}
    ins = [f64(s), f64(pose), i32(a_in), i32(alive), i32(wp_id), i32(status), i32(counter), f64(x0), f64(u), f64(cc), f64(z)]
    rc = twin.trace_emu_record(N, B, fields, gx.size, int(circular), _d(ins[0]), _d(ins[1]), _i(ins[2]), _i(ins[3]), _i(ins[4]),
                               _i(ins[5]), _i(ins[6]), _d(ins[7]), _d(ins[8]), _d(ins[9]), _d(ins[10]), _d(gx), _d(gy), _d(gpsi),
                               _d(row_ub), _d(row_lb), row_ub.shape[1], int(per_car), o["s"], o["pose"], o["wp_id"], o["x0"],
                               o["u"], o["status"], o["counter"], o["alive"], o["plan"], o["pred_x"], o["pred_y"], o["ub"], o["lb"])
    assert rc == 0
    return out


def _sim():
    return np.load(M.GOLDEN + "/g1_path_sim_track.npz"), np.load(M.GOLDEN + "/g3_corridor.npz")


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("N,n_usable,n_fallback", [(10, 90, 10), (30, 188, 22)])
def test_twin_reproduces_the_reference_predictions(twin, N, n_usable, n_fallback):
    """G6 holds MPC.current_prediction of every step of the reference's lap: from the same z, wp_id and status the record
    code gives the same world points (<= 1e-12: the C library's sine / cosine against numpy's) and nothing on a fallback."""
    g = np.load(M.GOLDEN + "/g6_closed_loop_N%d.npz" % N)
    g1, g3 = _sim()
    Tn = g["s"].size
    ones = np.ones(Tn, np.int32)
    rec = _twin_record(twin, N, PLAN | PRED | ROWS, g1, True, g["s"], g["pose"], ones, ones, g["wp_id"], g["status"], g["counter"],
                       g["x0"], g["u"], g["cc_next"], np.nan_to_num(g["z"]), g3["ub_obstacles"], g3["lb_obstacles"])
    ok = _usable(g["status"])
    assert ok.sum() == n_usable and (~ok).sum() == n_fallback
    dx, dy = np.abs(rec["pred_x"][ok] - g["pred_x"][ok]), np.abs(rec["pred_y"][ok] - g["pred_y"][ok])
    print("N = %d: max |pred - golden| = %.3e, %.3e over %d steps" % (N, dx.max(), dy.max(), ok.sum()))
    assert dx.max() <= 1e-12 and dy.max() <= 1e-12
    assert np.all(np.isnan(rec["pred_x"][~ok])) and np.all(np.isnan(rec["pred_y"][~ok]))
    # the numpy restatement of the formula, same operation order
    k = np.arange(2, N)
    w = (g["wp_id"][:, None] + k[None, :]) % g1["x"].size
    e_y = np.nan_to_num(g["z"])[:, 3 * k]
    px, py = g1["x"][w] - e_y * np.sin(g1["psi"][w]), g1["y"][w] + e_y * np.cos(g1["psi"][w])
    assert np.max(np.abs(rec["pred_x"][ok] - px[ok])) <= 1e-12 and np.max(np.abs(rec["pred_y"][ok] - py[ok])) <= 1e-12
    # the other fields of a step that solved and advanced: passed through
    assert _eq(rec["s"], g["s"]) and _eq(rec["pose"], g["pose"]) and _eq(rec["wp_id"], g["wp_id"]) and _eq(rec["x0"], g["x0"])
    assert _eq(rec["status"], g["status"]) and _eq(rec["u"], g["u"]) and _eq(rec["plan"], g["cc_next"])
    assert _eq(rec["counter"], g["counter"]) and np.all(rec["alive"] == 1)
    assert _eq(rec["ub"], g["ub"]) and _eq(rec["lb"], g["lb"])          # the table's row wp_id IS the reference's row


def _expected_record(N, s, pose, a_in, alive, wp_id, status, counter, x0, u, cc, rows_ub, rows_lb):
    """the table of include/mpmpc.h, restated with numpy masks (pred: only WHERE it is valid)"""
    state = a_in == 1
    inp = state & (alive != 0)
    solved = state & np.isin(alive, (1, -1))
    nan = np.nan
    m = lambda mask, v: np.where(mask.reshape((-1,) + (1,) * (np.ndim(v) - 1)), v, nan)
    return dict(s=m(state, s), pose=m(state, pose), wp_id=np.where(inp, wp_id, -1), x0=m(inp, x0),
                status=np.where(solved, status, 0), u=m(solved, u), plan=m(solved, cc), ub=m(solved, rows_ub),
                lb=m(solved, rows_lb), counter=counter, alive=alive), solved & _usable(status)


def test_twin_masks_every_row_of_the_table(twin):
    g1, g3 = _sim()
    N = 30
    #        a_in: ended before (5 kinds) | running: lap over, -2, -3, -4, -1, then 1 with every status class
    a_in = np.array([0, -1, -2, -3, -4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], np.int32)
    alive = np.array([0, -1, -2, -3, -4, 0, -2, -3, -4, -1, 1, 1, 1, 1, 1, 1], np.int32)
    status = np.array([1, 1, -3, 2, 1, 1, 1, 1, 2, -3, 1, 2, -2, -3, -4, -10], np.int32)
    B = a_in.size
    rng = np.random.default_rng(5)
    s, pose, x0, u = rng.normal(size=B), rng.normal(size=(B, 3)), rng.normal(size=(B, 3)), rng.normal(size=(B, 2))
    cc, z = rng.normal(size=(B, 2 * N)), rng.normal(size=(B, 5 * N + 3))
    wp_id = rng.integers(0, 200, B).astype(np.int32)
    wp_id[10] = 195                                                       # the horizon wraps around the lap
    counter = rng.integers(0, N - 1, B).astype(np.int32)
    for per_car in (False, True):
        rows_ub = rng.normal(size=(B, N)) if per_car else g3["ub_obstacles"]
        rows_lb = rng.normal(size=(B, N)) if per_car else g3["lb_obstacles"]
        rec = _twin_record(twin, N, PLAN | PRED | ROWS, g1, True, s, pose, a_in, alive, wp_id, status, counter, x0, u, cc, z,
                           rows_ub, rows_lb, per_car=per_car)
        want, pred_ok = _expected_record(N, s, pose, a_in, alive, wp_id, status, counter, x0, u, cc,
                                         rows_ub if per_car else rows_ub[wp_id][:, :N], rows_lb if per_car else rows_lb[wp_id][:, :N])
        for k in want:
            assert _eq(rec[k], want[k]), (k, per_car)
        assert list(np.flatnonzero(pred_ok)) == [10, 11, 12]
        for key in ("pred_x", "pred_y"):
            assert np.all(np.isfinite(rec[key][pred_ok])) and np.all(np.isnan(rec[key][~pred_ok])), key
        k = np.arange(2, N)
        w = (wp_id[:, None] + k[None, :]) % 200
        px = g1["x"][w] - z[:, 3 * k] * np.sin(g1["psi"][w])
        assert np.max(np.abs(rec["pred_x"][pred_ok] - px[pred_ok])) <= 1e-12
    # only the fields selected are laid out; the basic ones are 88 bytes per car
    assert twin.trace_emu_record_bytes(N, 256, 0) == 88 * 256
    assert twin.trace_emu_record_bytes(N, 256, PLAN | PRED | ROWS) == 1496 * 256
    assert twin.trace_emu_entries(N, 256, 0) == 9 and twin.trace_emu_entries(N, 256, PLAN | PRED | ROWS) == 9 + 60 + 56 + 60
    basic = _twin_record(twin, N, 0, g1, True, s, pose, a_in, alive, wp_id, status, counter, x0, u, cc, z,
                         g3["ub_obstacles"], g3["lb_obstacles"])
    assert sorted(basic) == sorted(BASIC) and all(_eq(basic[k], want[k]) for k in BASIC)


def test_abi_declares_exports_and_guards_the_recorder(built_library):
    names = ("mpmpc_rollout_record", "mpmpc_rollout_recorded", "mpmpc_rollout_trace")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpmpc.h")).read(), flags=re.S)
    lib = mpmpc.load_library(built_library)
    for n in names:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in mpmpc.EXPORTS and hasattr(lib, n), n
    for macro, val in (("MPMPC_REC_PLAN", 1), ("MPMPC_REC_PRED", 2), ("MPMPC_REC_ROWS", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), text), macro
    assert (mpmpc.REC_PLAN, mpmpc.REC_PRED, mpmpc.REC_ROWS) == (1, 2, 4)
    lib.mpmpc_rollout_record.argtypes = [C.c_void_p] + [C.c_int32] * 4
    lib.mpmpc_rollout_recorded.argtypes = [C.c_void_p, ip, ip]
    lib.mpmpc_rollout_trace.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] * 13
    n = C.c_int32(0)
    for rc in (lib.mpmpc_rollout_record(None, 1, 1, 0, 1), lib.mpmpc_rollout_recorded(None, C.byref(n), C.byref(n)),
               lib.mpmpc_rollout_trace(None, 1, 0, 0, *([None] * 13))):
        assert rc == E_ARG and b"handle is NULL" in lib.mpmpc_last_error()


# ------------------------------------------------------------------------------------------------------------ GPU
def _sim_handle(N, B, settings=None, key="obstacles"):
    g1, g3 = _sim()
    tr = scenarios.sim_track()
    h = mpmpc.Handle(T.stock_config(N, max_batch=B), settings or mpmpc.default_settings())
    h.set_path(tr.kappa, tr.v_ref, tr.ds_next)
    h.set_corridor(g3["ub_" + key], g3["lb_" + key])
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    return h, np.cumsum(g1["segment_lengths"]), g1, g3


def _check_against_table(rec, before, after, rows_ub, rows_lb, N, where=""):
    """one record against the states around its step (rollout_state() before / after), bit for bit"""
    want, pred_ok = _expected_record(N, before["s"], before["pose"], before["alive"], after["alive"], after["wp_id"],
                                     after["status"], after["counter"], after["x0"], after["u"], after["cc"], rows_ub, rows_lb)
    for k in want:
        if k in rec:
            assert _eq(rec[k], want[k]), (k, where)
    for key in ("pred_x", "pred_y"):
        if key in rec:
            assert np.all(np.isfinite(rec[key][pred_ok])) and np.all(np.isnan(rec[key][~pred_ok])), (key, where)
    return pred_ok


@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 30])
def test_trace_of_the_teacher_forced_reference_lap(N):
    """tests/test_rollout.py's replay of G6 (every recorded step one car, ONE rollout step) with everything recorded."""
    g = np.load(M.GOLDEN + "/g6_closed_loop_N%d.npz" % N)
    Tn = g["s"].size
    h, cum, g1, g3 = _sim_handle(N, Tn, mpmpc.default_settings(phase1_accept=0))
    h.rollout_warm_start(False)
    h.rollout_record(1, plan=True, prediction=True, rows=True, B=Tn)
    h.rollout_init(0.05, cum, g["s"], g["pose"], cc0=g["cc_prev"])
    h.rollout_set_counters(np.concatenate([[0], g["counter"][:-1]]).astype(np.int32))
    h.rollout_step(1)
    assert h.rollout_recorded() == (1, 1)
    tr = h.rollout_trace()
    st = h.rollout_state()
    h.close()
    assert sorted(tr) == sorted(ALL) and all(v.shape[:2] == (1, Tn) for v in tr.values())
    r = {k: v[0] for k, v in tr.items()}
    assert np.array_equal(r["s"], g["s"]) and np.array_equal(r["pose"], g["pose"])
    assert np.array_equal(r["wp_id"], g["wp_id"])
    assert np.max(np.abs(r["x0"] - g["x0"])) <= 1e-13
    ok = g["status"] > 0
    assert np.array_equal(r["status"] > 0, ok) and (~ok).sum() >= 5
    assert np.array_equal(r["counter"], g["counter"])
    assert np.max(np.abs(r["u"] - g["u"])) <= 1e-6
    d = np.abs(r["plan"] - g["cc_next"])
    d[:, -1] = 0.0                                                              # kappa_{N-1} is cost free
    assert d.max() <= 1e-6
    assert np.all(r["alive"] == 1)
    use = _usable(r["status"])
    assert np.array_equal(use, _usable(g["status"]))
    dx, dy = np.abs(r["pred_x"][use] - g["pred_x"][use]), np.abs(r["pred_y"][use] - g["pred_y"][use])
    print("N = %d: max |pred - golden| = %.3e, %.3e" % (N, dx.max(), dy.max()))
    assert dx.max() <= 1e-6 and dy.max() <= 1e-6
    assert np.all(np.isnan(r["pred_x"][~use])) and np.all(np.isnan(r["pred_y"][~use]))
    assert np.array_equal(r["ub"], g["ub"]) and np.array_equal(r["lb"], g["lb"])
    # ... and the record agrees with what the rollout itself reports after the step
    for k in ("wp_id", "x0", "u", "status", "counter", "alive"):
        assert np.array_equal(r[k], st[k]), k
    assert np.array_equal(r["plan"], st["cc"])


def _free_run(N, B, steps, warm, with_z):
    g1, g3 = _sim()
    rng = np.random.default_rng(17)
    starts = np.sort(rng.integers(0, g1["x"].size, B))
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    poses[:, 2] += rng.uniform(-0.03, 0.03, B)
    # run A: recorded, one call
    ha, cum, _, _ = _sim_handle(N, B)
    if warm is not None:
        ha.rollout_warm_start(warm)
    ha.rollout_record(steps, plan=True, prediction=True, rows=True, B=B)
    ha.rollout_init(0.05, cum, cum[starts], poses)
    ha.rollout_step(steps)
    assert ha.rollout_recorded() == (steps, steps)
    tr = ha.rollout_trace()
    fin_a = ha.rollout_state()
    ha.close()
    # run B: never recorded, one step per call, the state read back around each
    hb, cum, _, _ = _sim_handle(N, B)
    if warm is not None:
        hb.rollout_warm_start(warm)
    hb.rollout_init(0.05, cum, cum[starts], poses)
    snaps, zs = [hb.rollout_state()], []
    for _ in range(steps):
        hb.rollout_step(1)
        snaps.append(hb.rollout_state())
        if with_z:
            zs.append(hb.download(B).z)
    hb.close()
    ub_tab, lb_tab = g3["ub_obstacles"][:, :N], g3["lb_obstacles"][:, :N]
    k = np.arange(2, N)
    worst = 0.0
    for t in range(steps):
        before, after = snaps[t], snaps[t + 1]
        rec = {key: v[t] for key, v in tr.items()}
        pred_ok = _check_against_table(rec, before, after, ub_tab[after["wp_id"]], lb_tab[after["wp_id"]], N, where=t)
        if with_z and pred_ok.any():
            # the prediction from run B's solution of the same step (numpy's sine / cosine: an ulp of the C library's)
            w = (after["wp_id"][:, None] + k[None, :]) % g1["x"].size
            e_y = zs[t][:, 3 * k]
            px, py = g1["x"][w] - e_y * np.sin(g1["psi"][w]), g1["y"][w] + e_y * np.cos(g1["psi"][w])
            worst = max(worst, np.max(np.abs(rec["pred_x"][pred_ok] - px[pred_ok])), np.max(np.abs(rec["pred_y"][pred_ok] - py[pred_ok])))
    assert worst <= 1e-12, worst
    fin_b = snaps[-1]
    run = fin_b["alive"] == 1
    for key in fin_b:
        assert np.array_equal(fin_a[key][run], fin_b[key][run]), key
    for key in ("s", "pose", "cc", "counter", "alive"):
        assert np.array_equal(fin_a[key], fin_b[key]), key
    return tr, snaps


@pytest.mark.gpu
def test_free_run_is_recorded_faithfully_and_unperturbed():
    """64 cars, 270 steps in ONE call with every field recorded, against a second handle that never records and is stepped
    and read back one step at a time: every entry of the trace is bit-equal to those snapshots or empty where the table
    says so, and the two runs end in the same state."""
    steps = 270
    tr, snaps = _free_run(30, 64, steps, None, with_z=True)
    alive = tr["alive"]
    finished = np.any((alive[:-1] == 1) & (alive[1:] == 0), axis=0)
    assert finished.sum() >= 1
    b = int(np.flatnonzero(finished)[0])
    t = int(np.flatnonzero((alive[:-1, b] == 1) & (alive[1:, b] == 0))[0]) + 1
    assert np.isfinite(tr["s"][t, b]) and tr["wp_id"][t, b] == -1 and tr["status"][t, b] == 0       # the step that found the lap over
    assert np.all(np.isnan(tr["s"][t + 1:, b])) and np.all(alive[t + 1:, b] == 0)                   # ... and the ones after it
    assert np.array_equal(tr["s"][0], snaps[0]["s"])


@pytest.mark.gpu
def test_free_run_of_a_packed_fleet_with_the_warm_start():
    """2 048 cars: several cars share a wavefront and the (default, automatic) warm start is on."""
    _free_run(30, 2048, 8, None, with_z=False)


@pytest.mark.gpu
def test_records_of_cars_that_end():
    # ---- -1: the reference's lap at N = 10 exits after N - 1 consecutive infeasible steps
    g = np.load(M.GOLDEN + "/g6_closed_loop_N10.npz")
    N, t = 10, g["s"].size - 1
    h, cum, g1, g3 = _sim_handle(N, 1, mpmpc.default_settings(phase1_accept=0))
    h.rollout_record(12, plan=True, prediction=True, rows=True, B=1)
    h.rollout_init(0.05, cum, g["s"][t:t + 1], g["pose"][t:t + 1], cc0=g["cc_prev"][t:t + 1])
    h.rollout_set_counters(g["counter"][t - 1:t])
    h.rollout_step(12)
    tr = {k: v[:, 0] for k, v in h.rollout_trace().items()}
    st = h.rollout_state()
    h.close()
    assert st["alive"][0] == -1 and st["counter"][0] == 9
    e = int(np.flatnonzero(tr["alive"] == -1)[0])
    assert np.all(tr["alive"][:e] == 1) and np.all(tr["alive"][e:] == -1) and e < 11
    assert np.array_equal(tr["s"][0], g["s"][t]) and np.array_equal(tr["pose"][0], g["pose"][t])
    # the ending step: solved (no usable status), the fallback control applied, not driven; the plan and the row are there
    assert np.isfinite(tr["s"][e]) and np.all(np.isfinite(tr["pose"][e])) and tr["wp_id"][e] >= 0 and np.all(np.isfinite(tr["x0"][e]))
    assert tr["status"][e] != 0 and not _usable(tr["status"][e]) and tr["counter"][e] == 9
    assert np.all(np.isfinite(tr["u"][e])) and np.all(np.isfinite(tr["plan"][e]))
    assert np.array_equal(tr["u"][e], tr["plan"][e][2 * 9:2 * 9 + 2])              # cc[2 * counter], src/MPC.py:210-214
    assert np.all(np.isnan(tr["pred_x"][e])) and np.all(np.isnan(tr["pred_y"][e]))
    assert np.array_equal(tr["ub"][e], g3["ub_obstacles"][tr["wp_id"][e], :N]) and np.array_equal(tr["lb"][e], g3["lb_obstacles"][tr["wp_id"][e], :N])
    assert tr["s"][e] == st["s"][0] and np.array_equal(tr["pose"][e], st["pose"][0])
    # the steps after it: empty, counter and alive as they stand
    for k in ("s", "pose", "x0", "u", "plan", "pred_x", "pred_y", "ub", "lb"):
        assert np.all(np.isnan(tr[k][e + 1:])), k
    assert np.all(tr["wp_id"][e + 1:] == -1) and np.all(tr["status"][e + 1:] == 0) and np.all(tr["counter"][e + 1:] == 9)
    # ---- -2: the state at which the reference's run on the open Real_Track exited
    g = np.load(M.GOLDEN + "/g6_closed_loop_real_N30.npz")
    g1 = np.load(M.GOLDEN + "/g1_path_real_track.npz")
    g3r = np.load(M.GOLDEN + "/g3_corridor_real.npz")
    rtrack = scenarios.real_track()
    N = 30
    h = mpmpc.Handle(T.stock_config(N, max_batch=1, track=rtrack), mpmpc.default_settings(phase1_accept=0))
    h.set_path(rtrack.kappa, rtrack.v_ref, rtrack.ds_next)
    h.set_corridor(g3r["ub_free"], g3r["lb_free"])
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h.rollout_record(3, plan=True, prediction=True, rows=True, B=1)
    h.rollout_init(0.05, np.cumsum(g1["segment_lengths"]), g["exit_s"], g["exit_pose"][None, :], cc0=g["exit_cc_prev"][None, :])
    h.rollout_set_counters(g["exit_counter"].astype(np.int32))
    h.rollout_step(3)
    tr = {k: v[:, 0] for k, v in h.rollout_trace().items()}
    h.close()
    assert np.all(tr["alive"] == -2) and np.all(tr["counter"] == g["exit_counter"][0])
    assert tr["s"][0] == g["exit_s"][0] and np.array_equal(tr["pose"][0], g["exit_pose"])
    assert tr["wp_id"][0] == g["exit_wp_id"][0] and np.max(np.abs(tr["x0"][0] - g["exit_x0"])) <= 1e-13
    assert tr["status"][0] == 0
    for k in ("u", "plan", "pred_x", "pred_y", "ub", "lb"):
        assert np.all(np.isnan(tr[k])), k
    for k in ("s", "pose", "x0"):
        assert np.all(np.isnan(tr[k][1:])), k
    assert np.all(tr["wp_id"][1:] == -1) and np.all(tr["status"] == 0)


@pytest.mark.gpu
def test_rows_of_per_car_obstacle_worlds():
    """G6o teacher-forced as tests/test_car_obstacles.py does it, rows recorded: the rows K0c wrote for each car."""
    g = np.load(M.GOLDEN + "/g6o_closed_loop_N30.npz")
    g1 = np.load(M.GOLDEN + "/g1_path_sim_track.npz")
    sm = float(np.load(M.GOLDEN + "/g3o_sim_obstacles.npz")["safety_margin"][0])
    N, Tn = 30, g["s"].size
    gh, gw = g1["grid_shape"]
    grid = np.ascontiguousarray(np.unpackbits(g1["grid_free"])[:gh * gw].reshape(gh, gw).astype(np.int8))
    origin = tuple(g1["origin"]) if "origin" in g1 else (-1.0, -2.0)
    res = float(g1["resolution"][0]) if "resolution" in g1 else 0.005
    tr_ = scenarios.sim_track()
    h = mpmpc.Handle(T.stock_config(N, max_batch=Tn), mpmpc.default_settings(phase1_accept=0))
    h.set_path(tr_.kappa, tr_.v_ref, tr_.ds_next)
    h.set_map(grid, origin, res)
    h.set_path_geometry(g1["x"], g1["y"], g1["psi"], g1["border_ub"], g1["border_lb"])
    h.rollout_warm_start(False)
    h.build_corridor(N, 2 * sm, sm, want_tables=False)
    world = g["world"]
    counter_prev = np.zeros(Tn, np.int32)
    for t in range(1, Tn):
        counter_prev[t] = g["counter"][t - 1] if world[t] == world[t - 1] else 0
    h.rollout_record(2, rows=True, B=Tn)
    h.rollout_set_obstacles([g["discs_%d" % w] for w in world])
    h.rollout_init(0.05, np.cumsum(g1["segment_lengths"]), g["s"], g["pose"], cc0=g["cc_prev"])
    h.rollout_set_counters(counter_prev)
    h.rollout_step(1)
    tr = h.rollout_trace()
    assert sorted(tr) == sorted(BASIC + ("ub", "lb"))
    assert np.array_equal(tr["ub"][0], g["ub"]) and np.array_equal(tr["lb"][0], g["lb"])
    assert np.array_equal(tr["wp_id"][0], g["wp_id"]) and np.all(tr["alive"][0] == 1)
    h.rollout_step(1)
    last = h.rollout_trace(first=1, count=1)
    ub, lb = h.rollout_corridor()
    alive = h.rollout_state()["alive"]
    h.close()
    ok = np.isin(alive, (1, -1))
    assert ok.sum() > Tn // 2
    assert np.array_equal(last["ub"][0][ok], ub[ok]) and np.array_equal(last["lb"][0][ok], lb[ok])


@pytest.mark.gpu
def test_bookkeeping_of_the_trace():
    N, B = 30, 16
    g1, g3 = _sim()
    starts = np.arange(B) * 12
    poses = np.stack([g1["x"][starts], g1["y"][starts], g1["psi"][starts]], 1)
    h, cum, _, _ = _sim_handle(N, B)
    every = dict(plan=True, prediction=True, rows=True)

    def fresh():
        h.rollout_init(0.05, cum, cum[starts], poses)

    # a run that never recorded
    fresh()
    h.rollout_step(20)
    plain = h.rollout_state()
    # step(7) + step(13) = step(20)
    h.rollout_record(20, **every)
    fresh()
    assert h.rollout_recorded() == (0, 0)
    h.rollout_step(7)
    assert h.rollout_recorded() == (7, 7)
    h.rollout_step(13)
    assert h.rollout_recorded() == (20, 20)
    split = h.rollout_trace()
    part = h.rollout_trace(first=5, count=4, fields=["pose", "alive", "pred_y"])
    assert sorted(part) == ["alive", "pose", "pred_y"] and all(_eq(part[k], split[k][5:9]) for k in part)
    # the trace is full: the call is refused as a whole, nothing moves
    st0 = h.rollout_state()
    with pytest.raises(mpmpc.MpmpcError, match="error -3"):
        h.rollout_step(1)
    st1 = h.rollout_state()
    assert h.rollout_recorded() == (20, 20) and all(np.array_equal(st0[k], st1[k]) for k in st0)
    assert all(np.array_equal(st0[k], plain[k]) for k in plain)            # recording did not perturb the run
    with pytest.raises(mpmpc.MpmpcError, match="error -3"):
        h.rollout_trace(first=15, count=6)                                 # beyond the records held
    fresh()                                                                # rollout_init keeps the configuration, empties the trace
    assert h.rollout_recorded() == (0, 0)
    h.rollout_step(20)
    whole = h.rollout_trace()
    assert sorted(whole) == sorted(ALL) and all(_eq(whole[k], split[k]) for k in whole)
    assert np.all(whole["alive"] == 1) and np.all(np.isfinite(whole["pred_x"][_usable(whole["status"])]))
    # every 4th step
    h.rollout_record(5, stride=4, **every)
    fresh()
    h.rollout_step(20)
    assert h.rollout_recorded() == (5, 20)
    strided = h.rollout_trace()
    assert all(_eq(strided[k], whole[k][0::4]) for k in whole)
    with pytest.raises(mpmpc.MpmpcError, match="error -3"):
        h.rollout_step(1)                                                  # step 20 is a recorded one, and the trace is full
    # a field that was not recorded
    h.rollout_record(20, plan=True)
    fresh()
    h.rollout_step(3)
    assert sorted(h.rollout_trace()) == sorted(BASIC + ("plan",))
    with pytest.raises(mpmpc.MpmpcError, match="error -3"):
        h.rollout_trace(fields=["pred_x"])
    with pytest.raises(mpmpc.MpmpcError, match="error -1"):
        h.rollout_record(4, stride=0)
    # the trace survives what invalidates the rollout's state
    h.rollout_record(8, **every)
    fresh()
    h.rollout_step(5)
    a = h.rollout_trace()
    g = np.load(M.GOLDEN + "/g6_closed_loop_N30.npz")
    h.solve(g["wp_id"][:2].astype(np.int32), g["x0"][:2], g["cc_prev"][:2], g["lb"][:2], g["ub"][:2])
    with pytest.raises(mpmpc.MpmpcError, match="rollout_init"):
        h.rollout_step(1)
    b = h.rollout_trace()
    assert h.rollout_recorded()[0] == 5 and all(_eq(a[k], b[k]) for k in a) and all(_eq(a[k], whole[k][:5]) for k in a)
    # capacity 0: recording off, the rollout is the one that never recorded
    h.rollout_record(0)
    fresh()
    h.rollout_step(20)
    off = h.rollout_state()
    assert all(np.array_equal(off[k], plain[k]) for k in plain)
    with pytest.raises(mpmpc.MpmpcError):
        h.rollout_trace()
    # the B of a recorded rollout is the recorder's
    h.rollout_record(4, B=B - 1)
    with pytest.raises(mpmpc.MpmpcError, match="error -3"):
        fresh()
    h.close()


@pytest.mark.gpu
def test_batch_mpc_rollout_returns_the_trace():
    from MPC import BatchMPC
    from scipy import sparse
    m, rp, car = T.build_world()
    Q, R, QN = sparse.diags([1.0, 0.0, 0.0]), sparse.diags([0.5, 0.0]), sparse.diags([1.0, 0.0, 0.0])
    ic = {'umin': np.array([0.0, -np.tan(0.66) / car.length]), 'umax': np.array([1.0, np.tan(0.66) / car.length])}
    sc = {'xmin': np.array([-np.inf] * 3), 'xmax': np.array([np.inf] * 3)}
    B, steps = 8, 12
    bm = BatchMPC(car, 30, Q, R, QN, sc, ic, 4.0, max_batch=B, corridor="device")
    starts = np.arange(B) * 20
    cum = np.cumsum(rp.segment_lengths)
    poses = np.array([[rp.waypoints[w].x, rp.waypoints[w].y, rp.waypoints[w].psi] for w in starts])
    plain = bm.rollout(cum[starts], poses, steps)
    assert "trace" not in plain
    rec = bm.rollout(cum[starts], poses, steps, record=True)
    tr = rec.pop("trace")
    assert sorted(rec) == sorted(plain) and all(np.array_equal(rec[k], plain[k]) for k in plain)
    assert sorted(tr) == sorted(BASIC) and tr["pose"].shape == (steps, B, 3)
    assert np.array_equal(tr["pose"][0], poses) and np.array_equal(tr["s"][0], cum[starts])
    full = bm.rollout(cum[starts], poses, steps, record=dict(prediction=True, stride=3))
    assert full["trace"]["pred_x"].shape == (4, B, 28) and np.array_equal(full["trace"]["pose"], tr["pose"][0::3])
    assert all(np.array_equal(full[k], plain[k]) for k in plain)
    again = bm.rollout(cum[starts], poses, steps)                         # a later rollout is unrecorded again
    assert "trace" not in again and all(np.array_equal(again[k], plain[k]) for k in plain)
