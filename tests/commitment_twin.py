"""The CPU twin of K0k (tests/emul_commitment: csrc/commitment_core.hpp and csrc/corridor_core.hpp compiled for the host): a cached
loader that has tests/emul_commitment/Makefile build the library (rebuilt only when a source or a header changed), loads it and
declares every entry point's ctypes signature - here and nowhere else."""
import ctypes as C
import functools
import os
import subprocess

import mpmpc_testlib as T      # (first: it puts the package on sys.path)

dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int8)


@functools.lru_cache(None)
def commitment():
    subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "tests", "emul_commitment")], check=True)
    lib = C.CDLL(os.path.join(T.ROOT, "tests", "_build", "libcommitment_emul.so"))
    lib.cmt_emu_check.argtypes = [C.c_int, C.c_int, C.c_int, dp, ip, dp]
    lib.cmt_emu_bytes.argtypes = [C.c_longlong, C.c_int]
    lib.cmt_emu_bytes.restype = C.c_longlong
    lib.cmt_emu_budget.restype = C.c_longlong
    lib.cmt_twin_new.restype = C.c_void_p
    lib.cmt_twin_new.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, dp, dp,
                                 C.c_int, C.c_double, C.c_double]
    lib.cmt_twin_free.argtypes = [C.c_void_p]
    lib.cmt_twin_free.restype = None
    lib.cmt_twin_rows.argtypes = [C.c_void_p, C.c_int, ip, ip, ip, ip, ip, dp, ip, dp, dp, dp, ip, ip, dp, ip]
    return lib
