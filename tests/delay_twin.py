"""The CPU twin of K3d / K3q (tests/emul_delay: csrc/delay_core.hpp compiled for the host): a cached loader that has
tests/emul_delay/Makefile build the library (rebuilt only when a source or a header changed), loads it and declares every entry
point's ctypes signature - here and nowhere else."""
import ctypes as C
import functools
import os
import subprocess

import mpmpc_testlib as T      # (first: it puts the package on sys.path)

dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@functools.lru_cache(None)
def delay():
    subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "tests", "emul_delay")], check=True)
    lib = C.CDLL(os.path.join(T.ROOT, "tests", "_build", "libdelay_emul.so"))
    lib.dl_emu_max.argtypes = []
    lib.dl_emu_check.argtypes = [C.c_int, C.c_int, ip, ip, dp]
    lib.dl_emu_predict.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, dp, C.c_int, dp, C.c_double, C.c_double, dp, C.c_double, dp, dp, dp,
                                   C.POINTER(C.c_int)]
    lib.dl_emu_advance.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int), dp, C.c_int, dp, dp, dp, dp]
    lib.dl_emu_advance_plant.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int), dp, C.c_int, dp, dp, dp, dp,
                                         dp, dp, dp]
    return lib
