"""The CPU twin of K0d / K3l (tests/emul_localiser: csrc/localiser_core.hpp compiled for the host): a cached loader that has
tests/emul_localiser/Makefile build the library (rebuilt only when a source or a header changed), loads it and declares every
entry point's ctypes signature - here and nowhere else."""
import ctypes as C
import functools
import os
import subprocess

import mpmpc_testlib as T      # (first: it puts the package on sys.path)

dp, cip = C.POINTER(C.c_double), C.POINTER(C.c_int)
i8p, u8p = C.POINTER(C.c_int8), C.POINTER(C.c_uint8)


@functools.lru_cache(None)
def localiser():
    subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "tests", "emul_localiser")], check=True)
    lib = C.CDLL(os.path.join(T.ROOT, "tests", "_build", "liblocaliser_emul.so"))
    lib.lc_emu_check.argtypes = [C.c_int, dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double,
                                 C.c_longlong, C.c_int, dp, C.POINTER(C.c_char_p)]
    lib.lc_emu_field.argtypes = [C.c_int, C.c_int, i8p, C.c_int, u8p]
    lib.lc_emu_field.restype = None
    lib.lc_emu_field_at.argtypes = [u8p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong]
    lib.lc_emu_noise.argtypes = [C.c_double, C.c_uint64, C.c_uint32, C.c_int64, C.c_int, C.c_double, dp, u8p]
    lib.lc_emu_noise.restype = None
    lib.lc_emu_match.argtypes = [C.c_int, C.c_int, i8p, u8p, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, u8p, C.c_int, dp,
                                 C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, cip, cip, cip, dp]
    lib.lc_emu_match.restype = None
    lib.lc_emu_step.argtypes = [C.c_int, C.c_int, i8p, u8p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_double, C.c_int, C.c_double, C.c_longlong, C.c_uint64, C.c_uint32, C.c_int64, C.c_double, C.c_double,
                                C.c_int, dp, C.c_double, dp, dp, dp, dp, dp, cip, cip, cip, cip, dp, cip]
    lib.lc_emu_step.restype = None
    return lib
