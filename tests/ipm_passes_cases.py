"""The solves of tests/test_ipm_passes.py and the recorder of their fixture, tests/golden/ipm_passes_parent.npz.

The fixture holds what the lock-step emulation returned for these solves BEFORE the predictor and corrector passes of the
interior points (ReducedSolver::ipm3, the terminal-time interior point, Solver::ipm) were made compile-time: z, u0, status,
iters and resid of the launcher's sequence of kernels, array by array as the emulation wrote them (np.savez keeps the bits).
It was recorded from the parent commit's headers and is not to be re-recorded from later ones: the test asks that the
arithmetic of those routines never moves.

    python tests/ipm_passes_cases.py            # writes the fixture from the tree's emulation (run on the commit to pin)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ipm_passes_parent.npz")
FIELDS = ("z", "u0", "status", "iters", "resid")

# name: (config of scenarios.make, B, N, lanes per instance in the emulation, mpmpc_set_packing on the device - 0 = automatic)
# A waited-for launch of up to 1 024 instances runs one instance per wave (mpmpc_launch_plan.hpp), so "automatic" is 64 lanes.
CASES = {
    # an odd batch: the last wave of <32,16> carries one instance and one "none"
    "cfg2_B5_N30_g32": (2, 5, 30, 32, 32),
    # the same instances on <64,16>
    "cfg2_B5_N30_g64": (2, 5, 30, 64, 64),
    # <16,16>: four instances per wave, the wave partly filled
    "cfg2_B3_N12_g16": (2, 3, 12, 16, 16),
    # the obstacle corridor: infeasible instances reach the tail kernel, phase 1 and with it ipm3<SOFT>
    "cfg4_B64_N30_auto": (4, 64, 30, 64, 0),
    # the terminal-time kernel (mpmpc_reduced_t.hpp)
    "cfg3_B3_N50_auto": (3, 3, 50, 64, 0),
}


def scenario(name, track):
    import scenarios
    cfgid, B, N, _, _ = CASES[name]
    return scenarios.make(cfgid, track, B=B, N=N)


def emulate(name, emu, track):
    """-> {field: array} of the launcher's sequence of kernels on the emulation"""
    import mpmpc
    import mpmpc_testlib as T
    sc = scenario(name, track)
    cfg = T.stock_config(sc.N, sc.weights)
    qp = emu.assemble(cfg, track, (sc.wp_id, sc.x0, sc.cc_prev, sc.lb, sc.ub))
    sol, _ = emu.solve_launch(cfg, mpmpc.default_settings(), qp, G=CASES[name][3])
    return {f: getattr(sol, f) for f in FIELDS}


def load():
    with np.load(FIXTURE) as g:
        return {name: {f: g[name + "." + f] for f in FIELDS} for name in CASES}


if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    for p in (HERE, os.path.join(ROOT, "multi-purpose-mpc_amd"), os.path.join(ROOT, "oracle"), ROOT):
        sys.path.insert(0, p)
    import mpmpc_testlib as T
    import scenarios
    emu, track = T.Emul(), scenarios.sim_track()
    out = {}
    for name in CASES:
        for f, a in emulate(name, emu, track).items():
            out[name + "." + f] = a
        print(name, "status", np.unique(out[name + ".status"], return_counts=True), "ipm iterations", out[name + ".iters"][:, 1].tolist()[:8])
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
