"""The CPU twin of the recorder's chain kernel (tests/emul_chain: ro_chain_layout / ro_record_chain of csrc/rollout_core.hpp
compiled for the host): a cached loader that has tests/emul_chain/Makefile build the library (rebuilt only when a source or a
header changed), loads it and declares every entry point's ctypes signature - here and nowhere else."""
import ctypes as C
import functools
import os
import subprocess

import mpmpc_testlib as T      # (first: it puts the package on sys.path)

dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
# chain_emu_layout's `out`, and the fields with their per-car shapes (n: n_beams) in chain_emu_record's order
LAYOUT = ("act", "meas", "queue", "pred_pose", "pred_s", "now", "est", "cov", "used", "fix", "prior", "cand", "score", "hits", "ranges",
          "bytes", "entries", "n_beams")
FIELDS = LAYOUT[:15]
INTS = ("used", "cand", "score", "hits")


@functools.lru_cache(None)
def chain():
    subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "tests", "emul_chain")], check=True)
    lib = C.CDLL(os.path.join(T.ROOT, "tests", "_build", "libchain_emul.so"))
    lib.chain_emu_layout.argtypes = [C.c_int, C.c_int, C.c_int, lp]
    lib.chain_emu_layout.restype = None
    io = [ip if f in INTS else dp for f in FIELDS]
    lib.chain_emu_record.argtypes = [C.c_int, C.c_int, C.c_int, ip] + io + io
    return lib
