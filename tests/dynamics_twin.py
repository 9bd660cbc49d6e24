"""The CPU twin of K3y (tests/emul_dynamics: csrc/dynamics_core.hpp compiled for the host): a cached loader that has
tests/emul_dynamics/Makefile build the library (rebuilt only when a source or a header changed), loads it and declares every
entry point's ctypes signature - here and nowhere else."""
import ctypes as C
import functools
import os
import subprocess

import mpmpc_testlib as T      # (first: it puts the package on sys.path)

dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@functools.lru_cache(None)
def dynamics():
    subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "tests", "emul_dynamics")], check=True)
    lib = C.CDLL(os.path.join(T.ROOT, "tests", "_build", "libdynamics_emul.so"))
    lib.dy_emu_params.argtypes = []
    lib.dy_emu_check.argtypes = [C.c_int, C.c_int, dp, dp]
    lib.dy_emu_check_run.argtypes = [C.c_int, C.c_double, dp, C.c_double, dp]
    lib.dy_emu_move.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, dp, dp, dp, ip, dp]
    lib.dy_emu_move.restype = None
    lib.dy_emu_advance.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int), dp, C.c_double, dp, dp, dp, dp, dp,
                                   dp, dp, dp, ip, dp]
    lib.dy_emu_advance_delay.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int), dp, C.c_int, dp, dp, dp, dp,
                                         dp, dp, dp, dp, dp, ip, dp]
    return lib
