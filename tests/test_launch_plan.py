"""Which solve kernels a launch runs (csrc/mpmpc_launch_plan.hpp, read through mpmpc_launch_plan): the policy, on the CPU.

Every packing returns the same bits, so a launcher that picks the wrong kernel passes every answer test and is merely slower.
The expected stages below are written out by hand from the policy (packing thresholds, warm start, tail solver, deferral, the
long-horizon sequences); nothing here computes them with the code under test.  The sweeps at the end run the whole parameter
space and assert what must hold everywhere - and that the knobs a rule does not name do not move its plan, which ties the
rest of the space to the literal cases."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import mpmpc
import mpmpc_testlib as T
import scenarios
from mpmpc import (K_BLOCK, K_GENERAL, K_PAIR, K_PAIR_BLOCK, K_PAIR_BLOCK_T, K_PAIR_BLOCK_TAIL, K_PAIR_T, K_PAIR_TAIL, K_RBLOCK,
                   K_REDUCED, K_REDUCED_T, K_REDUCED_TAIL, LIST_LEFT, LIST_NEXT, LIST_NONE, LIST_THIS)

HORIZONS = (3, 10, 15, 16, 30, 31, 32, 50, 63, 64, 100, 127, 128, 200, 255)
BATCHES = (16, 17, 128, 129, 256, 257, 1024, 1025, 2048, 2049)      # both sides of every threshold
PACKINGS = (0, 16, 32, 64, 128, 256)
CONFIGS = ("stock", "full", "bounded", "free", "tt")


@pytest.fixture(scope="module")
def lib(built_library):
    return mpmpc.load_library()


def config(name, N):
    """stock: the reference's weights (reduced-native); full: off-diagonal weights; bounded: a bound on e_psi and t; free: a cost
    on t, no bound on e_psi / t; tt: a terminal cost on t and none else on it (the terminal-time kernels)"""
    if name == "full":
        return mpmpc.make_config(N, scenarios.Q_FULL, scenarios.R_FULL, scenarios.QN_FULL, scenarios.XMIN, scenarios.XMAX, scenarios.UMIN,
                                 scenarios.UMAX, scenarios.AY_MAX, scenarios.CAR_LENGTH)
    cfg = T.stock_config(N, "time_optimal" if name == "tt" else "stock")
    if name == "bounded":
        cfg.xmin[1], cfg.xmax[1], cfg.xmax[2] = -1.0, 1.0, 50.0
    if name == "free":
        cfg.Q[2] = 0.1
    return cfg


def plan(name, N, B, **kw):
    return mpmpc.launch_plan(config(name, N), mpmpc.default_settings(), B, **kw)


def stage(family, G, C, grid, block=64, reads=LIST_NONE, fills=LIST_NONE, var=0, warm=0, mode=0, clear=0, deferrable=0, turn=0):
    return dict(family=family, G=G, C=C, var=var, warm=warm, mode=mode, grid=grid, block=block, reads=reads, fills=fills, clear=clear,
                deferrable=deferrable, turn=turn)


def first(G, C, grid, warm=0):
    """the reduced-native batch kernel: fills this launch's list, opens a new turn of the flip lists"""
    return stage(K_REDUCED, G, C, grid, fills=LIST_THIS, warm=warm, turn=1)


def tail_solver(G, C, grid):
    return stage(K_REDUCED_TAIL, G, C, grid, reads=LIST_THIS, fills=LIST_LEFT, deferrable=1)


def general_tail(C, grid, reads, var=2, deferrable=1):
    return stage(K_GENERAL, 64, C, grid, reads=reads, var=var, mode=2, deferrable=deferrable)


THROUGHPUT = dict(kind=1, pipeline=3)

SHORT_STOCK = [
    # ---- N + 1 <= 32: 32 lanes from 1 025 instances on; from 129 on for one of several launches in flight
    (30, 1024, {}, [first(64, 16, 1024), tail_solver(32, 16, 512), general_tail(16, 1024, LIST_LEFT)]),
    (30, 1025, {}, [first(32, 16, 513), tail_solver(32, 16, 513), general_tail(16, 1025, LIST_LEFT)]),
    (30, 128, THROUGHPUT, [first(64, 16, 128), tail_solver(32, 16, 64), general_tail(16, 128, LIST_LEFT)]),
    (30, 129, THROUGHPUT, [first(32, 16, 65), tail_solver(32, 16, 65), general_tail(16, 129, LIST_LEFT)]),
    (30, 129, dict(kind=1, pipeline=1), [first(64, 16, 129), tail_solver(32, 16, 65), general_tail(16, 129, LIST_LEFT)]),
    (30, 129, dict(kind=0, pipeline=3), [first(64, 16, 129), tail_solver(32, 16, 65), general_tail(16, 129, LIST_LEFT)]),
    (30, 2049, {}, [first(32, 16, 1025), tail_solver(32, 16, 1025), general_tail(16, 2049, LIST_LEFT)]),      # 31 stages never fit 16 lanes
    (16, 2049, {}, [first(32, 16, 1025), tail_solver(32, 16, 1025), general_tail(16, 2049, LIST_LEFT)]),
    (31, 1025, {}, [first(32, 16, 513), tail_solver(32, 16, 513), general_tail(16, 1025, LIST_LEFT)]),
    (31, 1024, {}, [first(64, 16, 1024), tail_solver(32, 16, 512), general_tail(16, 1024, LIST_LEFT)]),
    # ---- N + 1 <= 16: 16 lanes from 2 049 on; from 257 on under throughput
    (15, 1024, {}, [first(64, 16, 1024), tail_solver(32, 16, 512), general_tail(16, 1024, LIST_LEFT)]),
    (15, 1025, {}, [first(32, 16, 513), tail_solver(32, 16, 513), general_tail(16, 1025, LIST_LEFT)]),
    (15, 2048, {}, [first(32, 16, 1024), tail_solver(32, 16, 1024), general_tail(16, 2048, LIST_LEFT)]),
    (15, 2049, {}, [first(16, 16, 513), tail_solver(32, 16, 1025), general_tail(16, 2049, LIST_LEFT)]),
    (15, 128, THROUGHPUT, [first(64, 16, 128), tail_solver(32, 16, 64), general_tail(16, 128, LIST_LEFT)]),
    (15, 129, THROUGHPUT, [first(32, 16, 65), tail_solver(32, 16, 65), general_tail(16, 129, LIST_LEFT)]),
    (15, 256, THROUGHPUT, [first(32, 16, 128), tail_solver(32, 16, 128), general_tail(16, 256, LIST_LEFT)]),
    (15, 257, THROUGHPUT, [first(16, 16, 65), tail_solver(32, 16, 129), general_tail(16, 257, LIST_LEFT)]),
    (10, 2049, {}, [first(16, 16, 513), tail_solver(32, 16, 1025), general_tail(16, 2049, LIST_LEFT)]),
    (3, 257, THROUGHPUT, [first(16, 16, 65), tail_solver(32, 16, 129), general_tail(16, 257, LIST_LEFT)]),
    # ---- 33 .. 64 stages: one instance per wave, chains split at 32, the tail solver one instance per wave
    (32, 2049, THROUGHPUT, [first(64, 32, 2049), tail_solver(64, 32, 2049), general_tail(32, 2049, LIST_LEFT)]),
    (50, 2049, {}, [first(64, 32, 2049), tail_solver(64, 32, 2049), general_tail(32, 2049, LIST_LEFT)]),
    (63, 129, THROUGHPUT, [first(64, 32, 129), tail_solver(64, 32, 129), general_tail(32, 129, LIST_LEFT)]),
    # ---- the tail: one instance per wave on request (below 32 stages only), or the general kernel on all of it
    (30, 203, dict(tail_kernel=2), [first(64, 16, 203), tail_solver(64, 16, 203), general_tail(16, 203, LIST_LEFT)]),
    (50, 203, dict(tail_kernel=2), [first(64, 32, 203), tail_solver(64, 32, 203), general_tail(32, 203, LIST_LEFT)]),
    (30, 203, dict(tail_kernel=0), [first(64, 16, 203), general_tail(16, 203, LIST_THIS)]),
    (50, 1025, dict(tail_kernel=0), [first(64, 32, 1025), general_tail(32, 1025, LIST_THIS)]),
    # ---- mpmpc_set_packing wins where the lanes hold the stages
    (30, 8, dict(packing=32), [first(32, 16, 4), tail_solver(32, 16, 4), general_tail(16, 8, LIST_LEFT)]),
    (30, 5000, dict(packing=64, **THROUGHPUT), [first(64, 16, 5000), tail_solver(32, 16, 2500), general_tail(16, 5000, LIST_LEFT)]),
    (10, 8, dict(packing=16), [first(16, 16, 2), tail_solver(32, 16, 4), general_tail(16, 8, LIST_LEFT)]),
    (15, 9, dict(packing=16), [first(16, 16, 3), tail_solver(32, 16, 5), general_tail(16, 9, LIST_LEFT)]),
    (10, 8, dict(packing=32), [first(32, 16, 4), tail_solver(32, 16, 4), general_tail(16, 8, LIST_LEFT)]),
    (50, 5000, dict(packing=64), [first(64, 32, 5000), tail_solver(64, 32, 5000), general_tail(32, 5000, LIST_LEFT)]),
    # ---- 16 lanes for 17 .. 32 stages: two stages per lane, four instances per wave - outside the closed loop
    (30, 203, dict(packing=16), [stage(K_PAIR, 16, 0, 51, fills=LIST_THIS, turn=1), tail_solver(32, 16, 102), general_tail(16, 203, LIST_LEFT)]),
    (16, 203, dict(packing=16), [stage(K_PAIR, 16, 0, 51, fills=LIST_THIS, turn=1), tail_solver(32, 16, 102), general_tail(16, 203, LIST_LEFT)]),
    (31, 4, dict(packing=16, tail_kernel=0), [stage(K_PAIR, 16, 0, 1, fills=LIST_THIS, turn=1), general_tail(16, 4, LIST_THIS)]),
    (30, 2049, dict(packing=16, closed_loop=True), [first(32, 16, 1025, warm=1), general_tail(16, 2049, LIST_THIS, deferrable=0)]),
    (30, 203, dict(packing=16, closed_loop=True), [first(64, 16, 203), general_tail(16, 203, LIST_THIS, deferrable=0)]),
    # ---- the closed loop: never lean, never deferred, never "throughput"; warm where it is asked for or pays
    (30, 17, dict(closed_loop=True), [first(64, 16, 17), general_tail(16, 17, LIST_THIS, deferrable=0)]),
    (30, 16, dict(closed_loop=True), [first(64, 16, 16, warm=1), general_tail(16, 16, LIST_THIS, deferrable=0)]),
    (30, 16, dict(closed_loop=True, warm_start=0), [first(64, 16, 16), general_tail(16, 16, LIST_THIS, deferrable=0)]),
    (30, 17, dict(closed_loop=True, warm_start=1), [first(64, 16, 17, warm=1), general_tail(16, 17, LIST_THIS, deferrable=0)]),
    (30, 1025, dict(closed_loop=True), [first(32, 16, 513, warm=1), general_tail(16, 1025, LIST_THIS, deferrable=0)]),
    (30, 1025, dict(closed_loop=True, warm_start=0), [first(32, 16, 513), general_tail(16, 1025, LIST_THIS, deferrable=0)]),
    (30, 1024, dict(closed_loop=True, **THROUGHPUT), [first(64, 16, 1024), general_tail(16, 1024, LIST_THIS, deferrable=0)]),
    (30, 17, dict(closed_loop=True, packing=32), [first(32, 16, 9, warm=1), general_tail(16, 17, LIST_THIS, deferrable=0)]),
    (50, 16, dict(closed_loop=True), [first(64, 32, 16, warm=1), general_tail(32, 16, LIST_THIS, deferrable=0)]),
    (15, 2049, dict(closed_loop=True), [first(16, 16, 513, warm=1), general_tail(16, 2049, LIST_THIS, deferrable=0)]),
]


@pytest.mark.parametrize("N,B,kw,want", SHORT_STOCK)
def test_short_horizons_reference_weights(lib, N, B, kw, want):
    assert plan("stock", N, B, **kw) == want


def tt_first(C, grid):
    return stage(K_REDUCED_T, 64, C, grid, fills=LIST_THIS, turn=1)


SHORT_OTHER = [
    # ---- a terminal cost on t: one instance per wave whatever is set, never lean, never warm; the general kernel takes its tail
    ("tt", 50, 4096, {}, [tt_first(32, 4096), general_tail(32, 4096, LIST_THIS, var=3)]),
    ("tt", 30, 5000, dict(packing=32, **THROUGHPUT), [tt_first(16, 5000), general_tail(16, 5000, LIST_THIS, var=3)]),
    ("tt", 15, 2049, dict(tail_kernel=2), [tt_first(16, 2049), general_tail(16, 2049, LIST_THIS, var=3)]),
    ("tt", 63, 16, dict(closed_loop=True, warm_start=1), [tt_first(32, 16), general_tail(32, 16, LIST_THIS, var=3, deferrable=0)]),
    # ---- everything else: the general kernel alone, one instance per wave, the whole solve
    ("full", 30, 1000, {}, [stage(K_GENERAL, 64, 16, 1000, var=1)]),
    ("full", 50, 2049, dict(packing=64, **THROUGHPUT), [stage(K_GENERAL, 64, 32, 2049, var=1)]),
    ("bounded", 30, 2049, THROUGHPUT, [stage(K_GENERAL, 64, 16, 2049, var=0)]),
    ("bounded", 63, 7, {}, [stage(K_GENERAL, 64, 32, 7, var=0)]),
    ("free", 15, 2049, dict(packing=16), [stage(K_GENERAL, 64, 16, 2049, var=3)]),
    ("free", 32, 1, {}, [stage(K_GENERAL, 64, 32, 1, var=3)]),
    ("full", 30, 16, dict(closed_loop=True), [stage(K_GENERAL, 64, 16, 16, var=1, warm=1)]),
    ("full", 30, 17, dict(closed_loop=True), [stage(K_GENERAL, 64, 16, 17, var=1)]),
    ("bounded", 50, 17, dict(closed_loop=True, warm_start=1), [stage(K_GENERAL, 64, 32, 17, var=0, warm=1)]),
    ("free", 30, 16, dict(closed_loop=True, warm_start=0), [stage(K_GENERAL, 64, 16, 16, var=3)]),
    ("free", 30, 2049, dict(closed_loop=True), [stage(K_GENERAL, 64, 16, 2049, var=3)]),      # never packed: not warm where "it pays"
]


@pytest.mark.parametrize("name,N,B,kw,want", SHORT_OTHER)
def test_short_horizons_other_configurations(lib, name, N, B, kw, want):
    assert plan(name, N, B, **kw) == want


def block(G, B, reads, var):
    return stage(K_BLOCK, G, 0, B, block=G, reads=reads, var=var, mode=2 if reads else 0)


def long_pair(B):
    return [stage(K_PAIR, 64, 0, B, fills=LIST_THIS, clear=1), stage(K_PAIR_TAIL, 64, 0, B, reads=LIST_THIS, fills=LIST_NEXT),
            block(128, B, LIST_NEXT, 2)]


def long_pair_block(B):
    return [stage(K_PAIR_BLOCK, 128, 0, B, block=128, fills=LIST_THIS, clear=1),
            stage(K_PAIR_BLOCK_TAIL, 128, 0, B, block=128, reads=LIST_THIS, fills=LIST_NEXT, clear=1), block(256, B, LIST_NEXT, 2)]


LONG = [
    # ---- 65 .. 128 stages, reference weights: two stages per lane in one wave, its tail solver, the workgroup kernel on the last list
    ("stock", 64, 300, {}, long_pair(300)),
    ("stock", 100, 203, {}, long_pair(203)),
    ("stock", 127, 2049, dict(packing=64, closed_loop=True, **THROUGHPUT), long_pair(2049)),
    ("stock", 100, 203, dict(tail_kernel=0), [stage(K_PAIR, 64, 0, 203, fills=LIST_THIS, clear=1), block(128, 203, LIST_THIS, 2)]),
    ("stock", 100, 203, dict(packing=128), [stage(K_RBLOCK, 128, 0, 203, block=128, fills=LIST_THIS, clear=1), block(128, 203, LIST_THIS, 2)]),
    ("stock", 127, 5, dict(packing=128, tail_kernel=0), [stage(K_RBLOCK, 128, 0, 5, block=128, fills=LIST_THIS, clear=1), block(128, 5, LIST_THIS, 2)]),
    # ---- more than 128 stages: the same on a workgroup of two waves; the tail solver's list is emptied in front of it
    ("stock", 128, 300, {}, long_pair_block(300)),
    ("stock", 200, 203, dict(packing=128), long_pair_block(203)),
    ("stock", 255, 17, dict(closed_loop=True, tail_kernel=2), long_pair_block(17)),
    ("stock", 200, 203, dict(tail_kernel=0), [stage(K_PAIR_BLOCK, 128, 0, 203, block=128, fills=LIST_THIS, clear=1), block(256, 203, LIST_THIS, 2)]),
    ("stock", 200, 203, dict(packing=256), [stage(K_RBLOCK, 256, 0, 203, block=256, fills=LIST_THIS, clear=1), block(256, 203, LIST_THIS, 2)]),
    ("stock", 128, 1, dict(packing=256), [stage(K_RBLOCK, 256, 0, 1, block=256, fills=LIST_THIS, clear=1), block(256, 1, LIST_THIS, 2)]),
    # ---- a terminal cost on t: its pair kernel, then the workgroup kernel; with the forcing knob the workgroup kernel alone
    ("tt", 100, 203, {}, [stage(K_PAIR_T, 64, 0, 203, fills=LIST_THIS, clear=1), block(128, 203, LIST_THIS, 0)]),
    ("tt", 64, 16, dict(closed_loop=True, warm_start=1), [stage(K_PAIR_T, 64, 0, 16, fills=LIST_THIS, clear=1), block(128, 16, LIST_THIS, 0)]),
    ("tt", 200, 203, {}, [stage(K_PAIR_BLOCK_T, 128, 0, 203, block=128, fills=LIST_THIS, clear=1), block(256, 203, LIST_THIS, 0)]),
    ("tt", 100, 203, dict(packing=128), [block(128, 203, LIST_NONE, 0)]),
    ("tt", 200, 203, dict(packing=256), [block(256, 203, LIST_NONE, 0)]),
    # ---- full weights or not reducible: the workgroup kernel alone, over every instance (no variant for free states here)
    ("full", 100, 203, {}, [block(128, 203, LIST_NONE, 1)]),
    ("full", 255, 2049, THROUGHPUT, [block(256, 2049, LIST_NONE, 1)]),
    ("bounded", 64, 203, {}, [block(128, 203, LIST_NONE, 0)]),
    ("bounded", 128, 203, dict(packing=256), [block(256, 203, LIST_NONE, 0)]),
    ("free", 127, 16, dict(closed_loop=True), [block(128, 16, LIST_NONE, 0)]),
    ("free", 200, 203, {}, [block(256, 203, LIST_NONE, 0)]),
]


@pytest.mark.parametrize("name,N,B,kw,want", LONG)
def test_long_horizons(lib, name, N, B, kw, want):
    assert plan(name, N, B, **kw) == want


def test_settings_that_rule_the_reduced_native_kernels_out(lib):
    """native = 0, or a polish that is off: the general kernel alone (variant 2 only while the reduced polish applies);
    phase1 = 0: no tail solver"""
    cfg = config("stock", 30)
    assert mpmpc.launch_plan(cfg, mpmpc.default_settings(native=0), 2049, **THROUGHPUT) == [stage(K_GENERAL, 64, 16, 2049, var=2)]
    assert mpmpc.launch_plan(cfg, mpmpc.stock_settings(), 2049) == [stage(K_GENERAL, 64, 16, 2049, var=3)]
    assert mpmpc.launch_plan(cfg, mpmpc.default_settings(phase1=0), 203) == [first(64, 16, 203), general_tail(16, 203, LIST_THIS)]
    assert mpmpc.launch_plan(config("stock", 100), mpmpc.default_settings(phase1=0), 203) == \
        [stage(K_PAIR, 64, 0, 203, fills=LIST_THIS, clear=1), block(128, 203, LIST_THIS, 2)]
    assert mpmpc.launch_plan(config("stock", 100), mpmpc.default_settings(native=0), 203) == [block(128, 203, LIST_NONE, 2)]


# ---- the whole space
def packing_fits(N, g):
    """what mpmpc_set_packing accepts, by hand: 16 / 32 up to 32 stages (16 lanes: two stages per lane from 17 on), 64 up to 128
    stages (two per lane from 65 on), 128 from 65 stages on, 256 from 129 on"""
    return {0: True, 16: N <= 31, 32: N <= 31, 64: N <= 127, 128: N >= 64, 256: N >= 128}[g]


class Raw:
    """mpmpc_launch_plan without the dictionaries: -> a tuple of rows (tuples), or the error code"""

    def __init__(self, lib):
        self.lib, self.st = lib, mpmpc.default_settings()
        self.knobs, self.rows = (C.c_int32 * 4)(), (C.c_int32 * (3 * len(mpmpc.PLAN_FIELDS)))()
        self.cfg = {(name, N): config(name, N) for name in CONFIGS for N in HORIZONS}

    def __call__(self, name, N, B, closed=0, kind=0, packing=0, tail=1, pipeline=3, warm=2):
        self.knobs[:] = [packing, tail, pipeline, warm]
        n = self.lib.mpmpc_launch_plan(C.byref(self.cfg[name, N]), C.byref(self.st), self.knobs, B, closed, kind, self.rows)
        w = len(mpmpc.PLAN_FIELDS)
        return n if n < 0 else tuple(tuple(self.rows[i * w:(i + 1) * w]) for i in range(n))


F = {f: i for i, f in enumerate(mpmpc.PLAN_FIELDS)}


@pytest.mark.parametrize("name", CONFIGS)
def test_what_holds_for_every_plan(lib, name):
    raw = Raw(lib)
    rn = name in ("stock", "tt")
    for N, B, closed, packing in itertools.product(HORIZONS, BATCHES, (0, 1), PACKINGS):
        if not packing_fits(N, packing):
            assert raw(name, N, B, closed, packing=packing) == -1, (N, packing)      # MPMPC_E_ARG, as mpmpc_set_packing answers
            continue
        seen = {}
        for kind, pipeline, warm, tail in itertools.product((0, 1), (1, 3), (0, 1, 2), (0, 1, 2)):
            p = raw(name, N, B, closed, kind, packing, tail, pipeline, warm)
            seen[kind, pipeline, warm, tail] = p
            where = (name, N, B, closed, kind, packing, tail, pipeline, warm)
            assert 1 <= len(p) <= 3, where
            for i, s in enumerate(p):
                # deferral: stages 2 and 3 of a launch outside the closed loop at N + 1 <= 64, nothing else
                assert s[F["deferrable"]] == (1 if rn and i > 0 and not closed and N <= 63 else 0), where
                # warm: the closed loop's first stage at N + 1 <= 64 only, never the terminal-time kernels
                if s[F["warm"]]:
                    assert closed and i == 0 and N <= 63 and name != "tt" and warm != 0, where
                # a new turn of the flip lists: the reduced-native first stage of the short horizons, once
                assert s[F["turn"]] == (1 if rn and i == 0 and N <= 63 else 0), where
                assert s[F["grid"]] >= 1 and s[F["block"]] in (64, 128, 256), where
                # a stage reads what an earlier stage filled; the first list of a long horizon is emptied on the stream
                assert s[F["reads"]] == LIST_NONE or any(q[F["fills"]] == s[F["reads"]] for q in p[:i]), where
                assert s[F["clear"]] in (0, 1) and (not s[F["clear"]] or (N >= 64 and s[F["fills"]] != LIST_NONE)), where
            assert p[-1][F["fills"]] == LIST_NONE and p[-1][F["family"]] in (K_GENERAL, K_BLOCK), where
            assert N <= 63 or not rn or len(p) == 1 or p[0][F["clear"]] == 1, where
        base = seen[0, 1, 2, 1]
        for (kind, pipeline, warm, tail), p in seen.items():
            # "throughput" is kind 1 AND more than one slot AND not the closed loop; and only the first stage's packing sees it
            if not (kind == 1 and pipeline == 3 and not closed):
                assert p == seen[0, 1, warm, tail], (name, N, B, closed, kind, pipeline)
            assert p[1:] == seen[0, 1, warm, tail][1:]
            # the warm-start knob is the closed loop's
            if not closed:
                assert p == seen[kind, pipeline, 2, tail]
            # the tail kernel is not the closed loop's at N + 1 <= 64, and nobody's where the reduction does not apply
            if (closed and N <= 63) or name != "stock":
                assert p == seen[kind, pipeline, warm, 1]
            # long horizons: neither the entry point nor the closed loop nor the batch size (beyond the grid) moves the plan
            if N >= 64:
                assert p == seen[0, 1, 2, tail] == raw(name, N, B, 1 - closed, 0, packing, tail, 1, 2)
                assert [s[:F["grid"]] + s[F["block"]:] for s in p] == [s[:F["grid"]] + s[F["block"]:] for s in raw(name, N, 7, 0, 0, packing, tail)]
                assert all(s[F["grid"]] == B for s in p)
            # configurations the reduction does not apply to: one stage, whatever the packing
            if not rn:
                assert len(p) == 1 and p == raw(name, N, B, closed, 0, 0, 1, 1, warm)
        assert base == raw(name, N, B, closed, 0, packing, 1, 1, 2)          # the same answer every time


def test_arguments_no_handle_can_hold_are_refused(lib):
    raw = Raw(lib)
    assert raw("stock", 30, 0) == -1 and raw("stock", 30, -5) == -1 and raw("stock", 30, 8, kind=2) == -1
    assert raw("stock", 30, 8, tail=3) == -1 and raw("stock", 30, 8, pipeline=0) == -1 and raw("stock", 30, 8, pipeline=9) == -1
    assert raw("stock", 30, 8, warm=3) == -1 and raw("stock", 30, 8, packing=48) == -1
    assert b"knobs" in lib.mpmpc_last_error()
    cfg = config("stock", 30)
    cfg.N = 256
    rows = (C.c_int32 * 39)()
    assert lib.mpmpc_launch_plan(C.byref(cfg), C.byref(mpmpc.default_settings()), (C.c_int32 * 4)(0, 1, 3, 2), 8, 0, 0, rows) == -1
    assert lib.mpmpc_launch_plan(None, None, None, 8, 0, 0, None) == -1
    with pytest.raises(mpmpc.MpmpcError):
        plan("stock", 50, 8, packing=16)


def test_the_plan_is_pure(lib, monkeypatch):
    """No device, no handle, no state: the same rows on repeated calls, rows beyond the plan's stages left alone, the environment
    neither read (MPMPC_LEAN_TAIL belongs to the handle, MPMPC_RN_OCC to the enqueue path) nor written."""
    libc = C.CDLL(None)
    libc.getenv.restype = C.c_char_p
    names = (b"MPMPC_LEAN_TAIL", b"MPMPC_RN_OCC", b"GPU_MAX_HW_QUEUES")
    want = plan("stock", 30, 2049, **THROUGHPUT)
    assert len(want) == 3
    for value in (None, "0", "2"):
        for n in names[:2]:
            if value is None:
                monkeypatch.delenv(n.decode(), raising=False)
            else:
                monkeypatch.setenv(n.decode(), value)
        env, raw_env = dict(os.environ), [libc.getenv(n) for n in names]
        for _ in range(3):
            assert plan("stock", 30, 2049, **THROUGHPUT) == want
        assert dict(os.environ) == env and [libc.getenv(n) for n in names] == raw_env
    rows = np.full((3, len(mpmpc.PLAN_FIELDS)), -7, np.int32)
    n = lib.mpmpc_launch_plan(C.byref(config("full", 30)), C.byref(mpmpc.default_settings()), (C.c_int32 * 4)(0, 1, 3, 2), 8, 0, 0,
                              rows.ctypes.data_as(C.POINTER(C.c_int32)))
    assert n == 1 and (rows[1:] == -7).all() and dict(zip(mpmpc.PLAN_FIELDS, rows[0].tolist())) == stage(K_GENERAL, 64, 16, 8, var=1)
