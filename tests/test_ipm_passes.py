"""The predictor and corrector passes of the interior points are compiled straight-line (ReducedSolver::ipm3, the terminal-time
interior point of mpmpc_reduced_t.hpp, Solver::ipm where its kernels' register budget allows): the same operations in the same
order on the same operands, so no output bit may move.  tests/golden/ipm_passes_parent.npz holds what the emulation of the
headers BEFORE that change returned for the solves of tests/ipm_passes_cases.py (recorded by that file)."""
import numpy as np
import pytest

import ipm_passes_cases as cases
import mpmpc
import mpmpc_testlib as T


@pytest.fixture(scope="module")
def parent():
    return cases.load()


def test_fixture_reaches_every_interior_point(parent):
    """The recorded solves run what they are there for: interior-point iterations in every case, and in the obstacle
    corridor both certified optima and refusals - the latter leave through the tail kernel's phase 1, ipm3<SOFT>."""
    for name, (cfgid, B, N, _, _) in cases.CASES.items():
        p = parent[name]
        assert p["z"].shape == (B, 5 * N + 3) and p["u0"].shape == (B, 2) and p["status"].shape == (B,)
        assert p["iters"].shape == (B, 2) and p["resid"].shape == (B, 2)
        assert p["z"].dtype == p["u0"].dtype == p["resid"].dtype == np.float64 and p["status"].dtype == p["iters"].dtype == np.int32
        assert np.all(p["iters"][:, 1] >= 3), name
    st = parent["cfg4_B64_N30_auto"]["status"]
    assert (st == mpmpc.PRIMAL_INFEASIBLE).sum() >= 1 and (st == 1).sum() >= 1
    assert mpmpc.PRIMAL_INFEASIBLE == -3
    for name in ("cfg2_B5_N30_g32", "cfg2_B5_N30_g64", "cfg2_B3_N12_g16", "cfg3_B3_N50_auto"):
        assert np.all(parent[name]["status"] == 1), name
    # (every packing returns the same bits: the two layouts of the same five instances)
    for f in cases.FIELDS:
        assert np.array_equal(parent["cfg2_B5_N30_g32"][f], parent["cfg2_B5_N30_g64"][f])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_emulation_reproduces_the_parent_byte_for_byte(name, parent, emu, track):
    now = cases.emulate(name, emu, track)
    for f in cases.FIELDS:
        a, b = np.ascontiguousarray(now[f]), np.ascontiguousarray(parent[name][f])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, f)


def test_flagship_iteration_has_no_inner_loop(built_library):
    """Static census of the shipped code object (profiles/ipm_passes/census.py): the interior-point iteration of the flagship's
    kernel holds no loop - the unroll pragma is a hint, this is the check - and no more VALU instructions than were counted
    when the passes were made straight-line (1 652; as a loop of two trips: 1 313 + a second trip of 491)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ipm_passes"))
    import census
    it = census.iteration(built_library, "mpmpc_reduced_kernel<32, 16, false>")
    assert it["inner"] == [] and 1000 <= it["valu"] <= 1652, it


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_gives_the_parents_results(name, parent, track):
    """The device against the recorded emulation, with the tolerances of the device-against-emulation tests of
    tests/test_gpu_parity.py: statuses and both iteration counters equal, z and u0 of certified optima to 1e-9
    (test_randomised_horizons_weights_and_batches_against_emulation), z of every instance - least-violation points of refused
    ones included - to 1e-4 (test_two_tail_instances_per_wave_on_device); resid with the only residual tolerance those tests
    have, rtol 1e-6 / atol 1e-9 (same test)."""
    cfgid, B, N, _, packing = cases.CASES[name]
    sc = cases.scenario(name, track)
    h = mpmpc.Handle(T.stock_config(sc.N, sc.weights, max_batch=B), mpmpc.default_settings())
    h.set_path(track.kappa, track.v_ref, track.ds_next)
    h.set_packing(packing)
    dev = h.solve(sc.wp_id, sc.x0, sc.cc_prev, sc.lb, sc.ub)
    h.close()
    ref = parent[name]
    ok = ref["status"] == 1
    print(name, "status equal", np.array_equal(dev.status, ref["status"]), "iters equal", np.array_equal(dev.iters, ref["iters"]),
          "max|dz| certified %.3e all %.3e" % (np.abs(dev.z - ref["z"])[ok].max(), np.abs(dev.z - ref["z"]).max()),
          "max|du0| certified %.3e all %.3e" % (np.abs(dev.u0 - ref["u0"])[ok].max(), np.abs(dev.u0 - ref["u0"]).max()),
          "max|dresid| %.3e" % np.abs(dev.resid - ref["resid"]).max(),
          "max rel dresid %.3e" % (np.abs(dev.resid - ref["resid"]) / np.maximum(np.abs(ref["resid"]), 1e-300)).max())
    assert np.array_equal(dev.status, ref["status"]) and np.array_equal(dev.iters, ref["iters"])
    assert np.abs(dev.z - ref["z"])[ok].max() < 1e-9 and np.abs(dev.u0 - ref["u0"])[ok].max() < 1e-9
    assert np.abs(dev.z - ref["z"]).max() <= 1e-4 and np.abs(dev.u0 - ref["u0"]).max() <= 1e-4
    np.testing.assert_allclose(dev.resid, ref["resid"], rtol=1e-6, atol=1e-9)
