"""The owner of the handle's buffers (csrc/device_buf.hpp) under an allocator whose k-th allocation fails: a stand-alone program
with the address and undefined-behaviour sanitizers (tests/device_buf/device_buf_check.cpp, built by tests/emul/Makefile), run
here once.  It checks, for every k of its scenario: alloc over a held buffer frees the old block, a failed alloc leaves the buffer
empty, moves leave the source empty and free the destination's old block once, alloc_all is all or nothing, nothing is live at
the end (its own count; the sanitizer's leak check ends the program with another status)."""
import os
import re
import subprocess

import mpmpc_testlib as T

ALLOCATIONS = 10      # of the scenario: 2 + 1 + 2 + 2 single ones, 3 in the group


def test_buffer_owner_under_a_failing_allocator():
    out = os.path.join(T.ROOT, "tests", "_build", "device_buf_check")
    subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "tests", "emul"), out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"(\d+) scenarios, (\d+) allocations in the scenario, (\d+) failures, (\d+) blocks live", r.stdout)
    assert m, r.stdout
    assert [int(g) for g in m.groups()] == [ALLOCATIONS + 1, ALLOCATIONS, 0, 0]      # one run without a failure, one per allocation
