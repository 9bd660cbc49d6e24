"""The CPU twin of K3e (tests/emul_estimator: csrc/estimator_core.hpp compiled for the host): a cached loader that has
tests/emul_estimator/Makefile build the library (rebuilt only when a source or a header changed), loads it and declares every
entry point's ctypes signature - here and nowhere else."""
import ctypes as C
import functools
import os
import subprocess

import mpmpc_testlib as T      # (first: it puts the package on sys.path)

dp, cip = C.POINTER(C.c_double), C.POINTER(C.c_int)


@functools.lru_cache(None)
def estimator():
    subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "tests", "emul_estimator")], check=True)
    lib = C.CDLL(os.path.join(T.ROOT, "tests", "_build", "libestimator_emul.so"))
    lib.es_emu_params.argtypes = []
    lib.es_emu_check.argtypes = [C.c_int, C.c_int, dp, dp, dp]
    lib.es_emu_available.argtypes = [dp, C.c_uint64, C.c_uint32, C.c_int64]
    lib.es_emu_step.argtypes = [dp, C.c_uint64, C.c_uint32, C.c_int64, C.c_double, C.c_double, dp, dp, dp, dp, dp, cip, dp, cip, cip]
    lib.es_emu_drive.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, dp, C.c_double, dp, dp]
    lib.es_emu_drive.restype = None
    return lib
