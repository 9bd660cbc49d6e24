"""Speed profile (K4) on acceleration-limited paths: every execution policy of sp_solve_t (csrc/speed_core.hpp) - the serial
emulation, the host twin of the wave kernel's cyclic reduction, and on the device the wave kernel and the thread-per-path kernel -
against the exact reference of tests/speed_profile_cases.py, on the named path families there at sizes around the wave width, the
levels of the reduction, the LDS limit of the wave kernel (384) and beyond it (385, 420).

Bars: 1e-8 on v against the reference (the project's bar against an oracle, test_host_path.py), 1e-9 between two runs of the same
code (device / emulation / twin), status 1 everywhere; the interior-point iteration counts of the two policies differ by at most 2
(a residual floor of the cyclic reduction above the loop's tolerance shows up there long before the loop's cap of 60)."""
import os
import warnings

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import speed_profile_cases as S

G = os.path.join(T.ROOT, "tests", "golden")
_runs = {}


def _emulated(entry, n):
    """(v [9, n], status, iters) of one emulation entry point on the nine families at size n; computed once."""
    if (entry, n) not in _runs:
        LI, KA, LIM, _ = S.batch(n)
        out = getattr(T, entry)(LI, KA, LIM)
        for a in out:
            a.setflags(write=False)
        _runs[entry, n] = out
    return _runs[entry, n]


# ---- the reference itself
@pytest.mark.parametrize("n", S.SIZES)
def test_recorded_reference_is_the_optimum(n):
    """kkt() on the recorded v of every case, with the inputs generated now: feasible and stationary to 1e-10 (measured: violation
    <= 1.5e-11 - tiny_li, whose rows carry c = 500 -, stationarity <= 5e-13), a hundred times below the bar the kernels are held to."""
    for f in S.FAMILIES:
        li, kappa, lim = S.make(f, n)
        viol, stat = S.kkt(li, kappa, lim, S.recorded(f, n))
        print(S.case_id(f, n), viol, stat)
        assert viol <= 1e-10 and stat <= 1e-10, (f, n, viol, stat)


@pytest.mark.parametrize("n", [m for m in S.SIZES if m <= 129])
def test_reference_reproduces_the_record(n):
    for f in S.FAMILIES:
        d = np.max(np.abs(S.reference(*S.make(f, n)) - S.recorded(f, n)))
        print(S.case_id(f, n), d)
        assert d <= 1e-10, (f, n, d)


@pytest.mark.parametrize("g1,g2", [("g1_path_sim_track.npz", "g2_speed_profile.npz"),
                                   ("g1_path_real_track.npz", "g2_speed_profile_real.npz")])
def test_reference_against_certified_fixtures(g1, g2):
    """reference() on the two shipped tracks against the certified optimum of G2: the distances in the docstring of
    speed_profile_cases, at least ten times below the 1e-8 bar with and without the refinement step."""
    g1, g2 = np.load(os.path.join(G, g1)), np.load(os.path.join(G, g2))
    n = g2["x"].size
    li, kappa = g1["ds_next"][:n], g1["kappa"][:n].astype(float)
    for refine in (False, True):
        d = np.max(np.abs(S.reference(li, kappa, g2["constraints"], refine=refine) - g2["x"]))
        print("refine", refine, "n", n, "distance", d)
        assert d <= 1e-9, (refine, d)


def test_cases_have_long_active_acceleration_runs():
    S.recorded("hairpin", 384)
    assert len(S.ACCEL_RUNS) == len(S.CASES) == len(S.FAMILIES) * len(S.SIZES)
    assert max(S.ACCEL_RUNS.values()) >= 150
    # ... and in each of the two kernels: on the largest wave launch, and on the thread-per-path kernel
    assert max(S.ACCEL_RUNS[S.case_id(f, 384)] for f in S.FAMILIES) >= 150
    assert max(S.ACCEL_RUNS[S.case_id(f, 385)] for f in S.FAMILIES) >= 150


# ---- the kernels' code on the host
@pytest.mark.parametrize("n", S.SIZES)
def test_serial_emulation_against_reference(n):
    v, status, iters = _emulated("emu_speed_profile", n)
    VREF = S.batch(n)[3]
    for p, f in enumerate(S.FAMILIES):
        print(S.case_id(f, n), status[p], iters[p], np.max(np.abs(v[p] - VREF[p])))
    assert np.all(status == 1), dict(zip(S.FAMILIES, status))
    assert np.max(np.abs(v - VREF)) <= 1e-8


@pytest.mark.parametrize("n", S.SIZES_WAVE)
def test_wave_twin_against_reference_and_serial(n):
    v, status, iters = _emulated("emu_speed_profile_wave", n)
    vs, ss, its = _emulated("emu_speed_profile", n)
    VREF = S.batch(n)[3]
    for p, f in enumerate(S.FAMILIES):
        print(S.case_id(f, n), status[p], iters[p], its[p], np.max(np.abs(v[p] - VREF[p])), np.max(np.abs(v[p] - vs[p])))
    assert np.all(status == 1), dict(zip(S.FAMILIES, status))
    assert np.max(np.abs(v - VREF)) <= 1e-8
    assert np.array_equal(status, ss) and np.max(np.abs(v - vs)) <= 1e-9
    assert np.max(np.abs(iters.astype(int) - its)) <= 2, (iters, its)


# ---- what the host class does with the status
@pytest.fixture(scope="module")
def path():
    from map import Map
    from reference_path import ReferencePath
    g1 = np.load(os.path.join(G, "g1_path_sim_track.npz"))
    h, w = g1["grid_shape"]
    m = Map.from_grid(np.unpackbits(g1["grid_free"])[:h * w].reshape(h, w).astype(np.int8), origin=[-1, -2], resolution=0.005)
    return ReferencePath.from_tables(m, g1["x"], g1["y"], g1["psi"], g1["kappa"], circular=True,
                                     border_ub=g1["border_ub"], border_lb=g1["border_lb"])


CONS = dict(a_min=-0.1, a_max=0.5, v_min=0.0, v_max=1.0, ay_max=4.0)


def _stub(status, fill=0.5):
    def solver(li, kappa, limits, eps=1e-12):
        return np.full((1, len(li)), fill), np.array([status], np.int32), np.zeros(1, np.int32)
    return solver


def test_compute_speed_profile_warns_on_status_2(path):
    with pytest.warns(UserWarning, match="status 2"):
        path.compute_speed_profile(CONS, solver=_stub(2, 0.25))
    assert all(w.v_ref == 0.25 for w in path.waypoints)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        path.compute_speed_profile(CONS, solver=_stub(1))
    assert all(w.v_ref == 0.5 for w in path.waypoints)


def test_compute_speed_profile_refuses_what_is_not_a_profile(path):
    path.compute_speed_profile(CONS, solver=_stub(1))
    for fill in (np.nan, np.inf):
        for status in (1, 2):
            with pytest.raises(ValueError, match="not finite"):
                path.compute_speed_profile(CONS, solver=_stub(status, fill))
    with pytest.raises(ValueError, match="inconsistent"):
        path.compute_speed_profile(CONS, solver=_stub(-1))
    assert all(w.v_ref == 0.5 for w in path.waypoints)          # a refused profile changes nothing


# ---- the device
@pytest.mark.gpu
@pytest.mark.parametrize("n", S.SIZES)
def test_device_families(n):
    """One path per family in one launch: the wave kernel up to n = 384 (its whole LDS budget), the thread-per-path kernel beyond."""
    LI, KA, LIM, VREF = S.batch(n)
    v, status, iters = mpmpc.speed_profile(LI, KA, LIM)
    ve, se, ie = _emulated("emu_speed_profile_wave" if n <= 384 else "emu_speed_profile", n)
    for p, f in enumerate(S.FAMILIES):
        print(S.case_id(f, n), status[p], se[p], iters[p], ie[p], np.max(np.abs(v[p] - ve[p])), np.max(np.abs(v[p] - VREF[p])))
    assert np.array_equal(status, se) and np.all(status == 1)
    assert np.max(np.abs(v - ve)) <= 1e-9
    assert np.max(np.abs(v - VREF)) <= 1e-8


@pytest.mark.gpu
def test_thread_per_path_kernel_across_blocks():
    """n = 385, B = 130: two full blocks and one of two lanes, the families in turn.  The code is serial per thread and only the
    stride of its path-minor workspace differs from a launch of one path: bit-equal rows."""
    n, B = 385, 130
    LI, KA, LIM, _ = S.batch(n)
    rep = np.arange(B) % len(S.FAMILIES)
    v, status, iters = mpmpc.speed_profile(LI[rep], KA[rep], LIM[rep])
    ve, se, _ = _emulated("emu_speed_profile", n)
    assert np.array_equal(status, se[rep]) and np.all(status == 1)
    assert np.max(np.abs(v - ve[rep])) <= 1e-9
    for p in range(len(S.FAMILIES)):
        v1, s1, i1 = mpmpc.speed_profile(LI[p], KA[p], LIM[p])
        assert s1[0] == 1
        for row in np.flatnonzero(rep == p):
            assert np.array_equal(v[row], v1[0]) and iters[row] == i1[0], (p, row)


@pytest.mark.gpu
def test_wave_kernel_mixed_batch_at_the_lds_limit():
    n = 384
    fam = ("hairpin", "tiny_li", "sawtooth", "vmin_positive", "iid")
    LI, KA, LIM, VREF = S.batch(n, fam)
    bad = LIM.copy()
    bad[2] = [0.5, -0.1, 0.0, 1.0, 4.0]                    # a_min > a_max: refused
    v, status, _ = mpmpc.speed_profile(LI, KA, bad)
    keep = np.array([0, 1, 3, 4])
    assert status[2] == -1 and np.all(status[keep] == 1)
    v4, s4, _ = mpmpc.speed_profile(LI[keep], KA[keep], LIM[keep])
    assert np.all(s4 == 1) and np.array_equal(v[keep], v4)
    assert np.max(np.abs(v4 - VREF[keep])) <= 1e-8


@pytest.mark.gpu
def test_scratch_regrowth_leaves_results_alone():
    """The per-device scratch grows for the thread-per-path launch (its workspace is in HBM) and is reused, larger than needed, by
    the launches after it."""
    first = None
    for B, n in ((9, 64), (130, 385), (9, 384), (9, 64)):
        LI, KA, LIM, VREF = S.batch(n)
        rep = np.arange(B) % len(S.FAMILIES)
        v, status, iters = mpmpc.speed_profile(LI[rep], KA[rep], LIM[rep])
        assert np.all(status == 1) and np.max(np.abs(v - VREF[rep])) <= 1e-8
        if first is None:
            first = (v, status, iters)
    assert all(np.array_equal(a, b) for a, b in zip(first, (v, status, iters)))
