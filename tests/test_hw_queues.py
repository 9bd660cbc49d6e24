"""Launch streams against hardware queues: the policy (CPU) and what it buys on the device (-m gpu, fresh child processes).

The HIP runtime maps the streams of a process onto GPU_MAX_HW_QUEUES hardware queues (4 when the variable is absent) and two
streams on one queue take turns.  A handle therefore never drives more launch streams than the process has queues
(mpmpc_pipeline_streams), and the library keeps off the null stream, which would take a queue of its own."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import mpmpc
import mpmpc_testlib as T

CHILD = os.path.join(T.ROOT, "tests", "hw_queue_child.py")


@pytest.fixture(scope="module")
def lib(built_library):
    return mpmpc.load_library()


@pytest.mark.parametrize("budget", [4, 8, 16])
def test_never_more_launch_streams_than_hardware_queues(lib, budget):
    for depth in range(1, 9):
        s = lib.mpmpc_pipeline_streams(depth, budget)
        assert 1 <= s <= min(depth, budget)
        assert s == min(depth, budget)          # ... and no fewer than the budget carries
    # depths outside 1 .. 8 (mpmpc_set_pipeline refuses them) and budgets below one queue still give a usable answer
    assert lib.mpmpc_pipeline_streams(0, budget) == 1 and lib.mpmpc_pipeline_streams(-3, budget) == 1
    assert lib.mpmpc_pipeline_streams(100, budget) == min(8, budget)
    assert lib.mpmpc_pipeline_streams(4, 0) == 1 and lib.mpmpc_pipeline_streams(4, -1) == 1


def test_policy_on_small_budgets(lib):
    assert [lib.mpmpc_pipeline_streams(d, 1) for d in range(1, 9)] == [1] * 8
    assert [lib.mpmpc_pipeline_streams(d, 3) for d in range(1, 9)] == [1, 2, 3, 3, 3, 3, 3, 3]
    assert [lib.mpmpc_pipeline_streams(d, 4) for d in range(1, 9)] == [1, 2, 3, 4, 4, 4, 4, 4]


@pytest.mark.parametrize("text,want", [
    (None, 4),                                            # variable absent: the runtime's default
    (b"4", 4), (b"8", 8), (b"16", 16), (b"1", 1), (b"32", 32), (b" 8", 8), (b"8 ", 8), (b"+8", 8),
    (b"", 4), (b" ", 4), (b"eight", 4), (b"8x", 4), (b"8.5", 4), (b"0x10", 4), (b"4,8", 4),      # not one decimal number
    (b"0", 4), (b"-1", 4), (b"-8", 4),                                                            # not a queue count
    (b"99999999999999999999999", 4),                                                              # out of range
])
def test_queue_budget_from_the_environment_text(lib, text, want):
    assert lib.mpmpc_hw_queue_budget(text) == want


def test_the_policy_symbols_are_pure(lib):
    """No device, no handle, no state: callable on a box without a GPU, same answer every time, and the environment of the
    process is left as it was (the library reads GPU_MAX_HW_QUEUES, it never writes it)."""
    before = os.environ.get("GPU_MAX_HW_QUEUES")
    libc = C.CDLL(None)
    libc.getenv.restype = C.c_char_p
    raw_before = libc.getenv(b"GPU_MAX_HW_QUEUES")
    for _ in range(3):
        assert lib.mpmpc_pipeline_streams(4, lib.mpmpc_hw_queue_budget(b"4")) == 4
        assert lib.mpmpc_pipeline_streams(6, lib.mpmpc_hw_queue_budget(None)) == 4
        assert lib.mpmpc_pipeline_streams(6, lib.mpmpc_hw_queue_budget(b"16")) == 6
    assert os.environ.get("GPU_MAX_HW_QUEUES") == before and libc.getenv(b"GPU_MAX_HW_QUEUES") == raw_before


def test_library_source_never_writes_the_environment_or_uses_the_null_stream():
    """the library's translation unit: the .hip and every header beside it (host code lives in headers too)"""
    csrc = os.path.join(T.ROOT, "multi-purpose-mpc_amd", "csrc")
    files = ["mpmpc_hip.hip"] + sorted(f for f in os.listdir(csrc) if f.endswith(".hpp"))
    assert len(files) > 1
    for name in files:
        src = open(os.path.join(csrc, name)).read()
        for word in ("setenv(", "putenv(", "hipMemset(", "hipMemcpy(", "hipDeviceSynchronize("):
            assert word not in src, (name, word)


def _child(mode, limit):
    """a fresh process with four hardware queues, under its own time limit; -> the JSON line it printed"""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, CHILD, mode], env=env, capture_output=True, text=True,
                       timeout=limit + 30)
    assert r.returncode == 0, "child %s ended with %d:\n%s" % (mode, r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    assert out["GPU_MAX_HW_QUEUES"] == "4" and out["streams_at_depth4"] == 4
    return out


@pytest.mark.gpu
def test_depth_four_on_four_queues_returns_the_bytes_of_depth_one():
    """config 2, B = 1 024: nine resident launches through four slots, then the same through one"""
    out = _child("equal", 120)
    assert out["instances"] == 1024 and out["solved"] > 0
    assert all(out["same"].values()), out["same"]


@pytest.mark.gpu
def test_depth_four_on_four_queues_is_not_slower_than_depth_three():
    """config 2, B = 1 024, GPU_MAX_HW_QUEUES=4: median rate of nine 200-step regions per depth, the depths in turn, after
    bench.py's clock ramp.  The bar is 1.0: with two launch streams on one queue the fourth launch costs a quarter of the rate
    (0.74 = 36.1 / 49.0 M solves/s, profiles/r4/depth_sweep.txt), with four streams on four queues it adds a quarter
    (1.25 = 61.5 / 49.0 on eight queues)."""
    out = _child("rate", 180)
    print("depth 3: %.2f M solves/s, depth 4: %.2f M solves/s, ratio %.3f" %
          (out["solves_per_s_depth3"] / 1e6, out["solves_per_s_depth4"] / 1e6, out["ratio_depth4_over_depth3"]))
    assert out["ratio_depth4_over_depth3"] >= 1.0, out
