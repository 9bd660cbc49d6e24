"""The block layout and the scratch of the entry points without a handle (csrc/device_scratch.hpp): a stand-alone program with
the address and undefined-behaviour sanitizers (tests/scratch/scratch_check.cpp, built by tests/emul/Makefile), run here once.
The layout: regions start on multiples of 8, ascend and do not overlap, the block ends with the last one, a region of no
elements changes nothing, the parts of a combined region lie back to back, and the lidar's world block is written out for two
shapes.  grow, for every k of small -> larger -> smaller -> larger again with the k-th allocation failing: the old block is
freed exactly once, a failed grow leaves the scratch empty and the next call allocates, a need that fits allocates nothing, one
block per scratch is live at the end (the program frees it itself; the sanitizer's leak check ends it with another status)."""
import os
import re
import subprocess

import mpmpc_testlib as T

ALLOCATIONS = 6      # of the scenario: two scratches, each small, larger, larger again (smaller and the repeat fit)


def test_layout_and_scratch_under_a_failing_allocator():
    out = os.path.join(T.ROOT, "tests", "_build", "scratch_check")
    subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "tests", "emul"), out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"(\d+) scenarios, (\d+) allocations in the scenario, (\d+) failures, (\d+) blocks live", r.stdout)
    assert m, r.stdout
    assert [int(g) for g in m.groups()] == [ALLOCATIONS + 1, ALLOCATIONS, 0, 0]      # one run without a failure, one per allocation
