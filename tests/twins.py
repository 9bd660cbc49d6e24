"""The CPU twins of the rollout's features (tests/emul_*/: the library's own *_core.hpp headers compiled for the host), one
cached loader per library.  A loader has tests/emul/Makefile build its library (`make <name>`: the emulation's flags, rebuilt
only when a source or a header changed), loads it and declares every entry point's ctypes signature - here and nowhere else."""
import ctypes as C
import functools
import os
import subprocess

import mpmpc_testlib as T      # (first: it puts the package on sys.path)
import mpmpc

dp, ip, bp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int8), C.POINTER(C.c_int64)
up, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def _load(name):
    subprocess.run(["make", "-s", "-j4", "-C", os.path.join(T.ROOT, "tests", "emul"), name], check=True)
    return C.CDLL(os.path.join(T.ROOT, "tests", "_build", "lib%s_emul.so" % name))


@functools.lru_cache(None)
def car():
    """K0a's line cache and K0c (tests/emul_car)"""
    lib = _load("car_corridor")
    lib.car_emu_check.argtypes = [C.c_int, C.c_int, ip, ip, C.c_int, C.c_int, C.c_int]
    lib.car_emu_rows.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double, C.c_int,
                                 dp, dp, dp, dp, C.c_int, dp, dp, C.c_int, C.c_double, C.c_double, C.c_int, ip, ip, ip,
                                 dp, dp, ip]
    return lib


@functools.lru_cache(None)
def walls():
    """K0w, K-world and the WALLS variants of K0c, K0l, K0f (tests/emul_walls)"""
    lib = _load("walls")
    lib.wall_emu_check.argtypes = [C.c_int, C.c_int, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.wall_emu_cells.argtypes = [ip, ip, ip, C.c_long, ip]
    lib.wall_emu_cells.restype = C.c_long
    lib.wall_emu_world_grid.argtypes = [C.c_int, C.c_int, bp, C.c_int, ip, C.c_int, ip, bp]
    lib.wall_emu_rows.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, dp, dp,
                                  C.c_int, C.c_double, C.c_double, C.c_int, ip, ip, ip, ip, ip, dp, dp, ip]
    lib.wall_emu_scan.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, ip, ip, ip, ip, C.c_int, dp,
                                  C.c_double, dp]
    lib.wall_emu_audit.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, ip, ip, ip, ip, C.c_double,
                                   C.c_double, C.c_double, ip, dp]
    return lib


@functools.lru_cache(None)
def lookahead():
    """K0h and K0c<WALLS, LEAD> (tests/emul_lookahead)"""
    lib = _load("lookahead")
    lib.look_emu_check.argtypes = [C.c_int, C.c_int, dp, C.c_int]
    lib.look_emu_table_bytes.argtypes = [C.c_longlong, C.c_int]
    lib.look_emu_table_bytes.restype = C.c_longlong
    lib.look_emu_leads.argtypes = [C.c_int, C.c_int, ip, ip, C.c_int, C.c_int, dp, C.c_double, C.c_int, ip]
    lib.look_emu_leads.restype = None
    lib.look_emu_discs.argtypes = [C.c_int, C.c_int, ip, ip, ip, dp, C.c_int64, C.c_int64, ip, ip, C.c_int, C.c_int, C.c_double,
                                   C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, ip]
    lib.look_emu_discs.restype = None
    lib.look_emu_rows.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, dp, dp,
                                  C.c_int, C.c_double, C.c_double, C.c_int, ip, ip, ip, ip, ip, ip, ip, ip, dp, dp, ip]
    return lib


@functools.lru_cache(None)
def traffic_lookahead():
    """K3t, K0t<true>, K0ht and K0c<WALLS, true, true> (tests/emul_traffic_lookahead)"""
    lib = _load("traffic_lookahead")
    lib.tlk_emu_table_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.tlk_emu_table_bytes.restype = C.c_longlong
    lib.tlk_emu_budget.restype = C.c_longlong
    lib.tlk_emu_tracks.argtypes = [C.c_int, C.c_int, dp, ip, ip, ip, ip, C.c_int, C.c_int, dp, dp, dp, C.c_int, C.c_int, C.c_double,
                                   C.c_double, C.c_double, ip, ip, dp]
    lib.tlk_emu_tracks.restype = None
    lib.tlk_emu_times_scan.argtypes = [C.c_int, dp, dp]
    lib.tlk_emu_times_scan.restype = None
    lib.tlk_emu_slots.argtypes = [C.c_int, dp, ip, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, ip, ip]
    lib.tlk_emu_discs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, ip, ip, ip, ip, ip, dp, ip]
    lib.tlk_emu_discs.restype = None
    lib.tlk_emu_rows.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, dp, dp,
                                 C.c_int, C.c_double, C.c_double, C.c_int, ip, ip, ip, ip, ip, ip, ip, ip, C.c_int, ip, dp, dp, ip]
    return lib


@functools.lru_cache(None)
def movers():
    """K0m (tests/emul_movers)"""
    lib = _load("movers")
    lib.mov_emu_check.argtypes = [C.c_int, C.c_int, ip, ip, ip, dp, C.c_int, C.c_int, ip]
    lib.mov_emu_check_combined.argtypes = [C.c_int, ip, C.c_int, ip]
    lib.mov_emu_combine.argtypes = [C.c_int, ip, ip, ip, ip]
    lib.mov_emu_combine.restype = None
    lib.mov_emu_discs.argtypes = [C.c_int, ip, ip, dp, lp, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                  C.c_int, dp, dp, dp, dp, C.c_int, ip]
    lib.mov_emu_discs.restype = None
    return lib


@functools.lru_cache(None)
def traffic():
    """K0t (tests/emul_traffic)"""
    lib = _load("traffic")
    lib.tr_emu_check.argtypes = [C.c_int, C.c_int, ip, ip, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip]
    lib.tr_emu_check_combined.argtypes = [C.c_int, ip, C.c_int, ip, C.c_int, C.c_int]
    lib.tr_emu_check_movers.argtypes = [C.c_int, C.c_int, ip, ip, ip, dp, C.c_int, C.c_int, ip, C.c_int, C.c_int]
    lib.tr_emu_layout.argtypes = [C.c_int, ip, ip, ip, ip]
    lib.tr_emu_combine.argtypes = [C.c_int, ip, ip, C.c_int, ip, ip]
    lib.tr_emu_combine.restype = None
    lib.tr_emu_slots.argtypes = [C.c_int, dp, ip, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                 C.c_double, ip]
    return lib


@functools.lru_cache(None)
def lidar():
    """K0l (tests/emul_lidar)"""
    lib = _load("lidar")
    lib.lid_emu_check.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_int, dp, ip, ip, C.c_int, dp, C.c_double, dp]
    lib.lid_emu_scan.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, ip, ip, C.c_int, dp,
                                 C.c_double, dp, ip, ip]
    return lib


@functools.lru_cache(None)
def footprint():
    """K0f (tests/emul_footprint)"""
    lib = _load("footprint")
    lib.fp_emu_check.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_int, dp, ip, ip, C.c_double, C.c_double, C.c_double, ip, dp, ip]
    lib.fp_emu_audit.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, ip, ip, C.c_double,
                                 C.c_double, C.c_double, ip, dp]
    return lib


@functools.lru_cache(None)
def perception():
    """K0s (tests/emul_perception)"""
    lib = _load("perception")
    lib.per_emu_check_scan.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_int, dp, ip, ip, ip, ip, C.c_int, dp, C.c_double, dp]
    lib.per_emu_check_setting.argtypes = [C.c_int, dp, C.c_double, C.c_int, C.c_double]
    lib.per_emu_scan.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, ip, ip, ip, ip, C.c_int, dp,
                                 C.c_double, dp, u64p, up]
    lib.per_emu_sequence.argtypes = [C.c_int] * 5 + [ip, u64p, up, C.c_int, C.c_int, C.c_int, u64p, up, ip, ip, ip, ip]
    lib.per_emu_sequence.restype = None
    lib.per_emu_lists.argtypes = [C.c_int, ip, C.c_uint64, C.c_int, ip, C.c_uint32, ip, ip]
    lib.per_emu_lists.restype = None
    return lib


@functools.lru_cache(None)
def path():
    """mpmpc_path_count / mpmpc_path_build (tests/emul_path)"""
    lib = _load("path")
    lib.path_emu_count.argtypes = [C.c_int, dp, C.c_double, C.c_int]
    lib.path_emu_mean.argtypes = [dp, C.c_int]
    lib.path_emu_mean.restype = C.c_double
    lib.path_emu_build.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, ip, dp, dp, ip, ip, ip, ip, ip,
                                   C.c_int, ip, ip] + [dp] * 9
    return lib


@functools.lru_cache(None)
def routes():
    """the route view of K1, the waypoint arithmetic, mpmpc_build_corridor and the routes' state (tests/emul_routes)"""
    lib = _load("routes")
    lib.routes_emu_fields.argtypes = [C.POINTER(mpmpc.Config), C.c_int, dp, dp, dp, C.c_int, dp, dp, ip, C.c_int, C.c_int, C.c_int,
                                      ip, dp, dp, dp]
    lib.routes_emu_current_waypoint.argtypes = [dp, C.c_int, C.c_int, C.c_double]
    lib.routes_emu_past_open_end.argtypes = [C.c_int] * 4
    lib.routes_emu_corridor.argtypes = [C.c_int, C.c_int, bp, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int,
                                        ip, ip, dp, dp, C.c_int, C.c_double, C.c_double, dp, dp]
    lib.routes_state_new.restype = C.c_void_p
    lib.routes_state_new.argtypes = [C.c_int] * 3
    lib.routes_state_free.argtypes = [C.c_void_p]
    lib.routes_state_why.restype = C.c_char_p
    lib.routes_state_why.argtypes = [C.c_void_p]
    lib.routes_state_set_path.argtypes = [C.c_void_p, C.c_int]
    lib.routes_state_set_routes.argtypes = [C.c_void_p, C.c_int, ip, ip, ip]
    lib.routes_state_set_car_routes.argtypes = [C.c_void_p, C.c_int, ip, ip]
    lib.routes_state_check_upload.argtypes = [C.c_void_p, C.c_int, ip]
    lib.routes_state_check_batch.argtypes = [C.c_void_p, C.c_int]
    return lib


@functools.lru_cache(None)
def project():
    """mpmpc_project and the re-route of a running rollout (tests/emul_project)"""
    lib = _load("project")
    lib.project_emu.argtypes = [C.c_int, dp, dp, dp, dp, C.c_int, ip, C.c_int, dp, C.c_int, ip, C.c_double, ip, dp, dp, dp,
                                C.POINTER(C.c_char_p)]
    lib.reroute_twin_new.restype = C.c_void_p
    lib.reroute_twin_new.argtypes = [C.c_int, C.c_int]
    lib.reroute_twin_free.argtypes = [C.c_void_p]
    lib.reroute_twin_why.restype = C.c_char_p
    lib.reroute_twin_why.argtypes = [C.c_void_p]
    lib.reroute_twin_set_routes.argtypes = [C.c_void_p, C.c_int, ip, ip]
    lib.reroute_twin_set_car_routes.argtypes = [C.c_void_p, C.c_int, ip, ip]
    lib.reroute_twin_rollout_init.argtypes = [C.c_void_p, C.c_int]
    lib.reroute_twin_check_upload.argtypes = [C.c_void_p, C.c_int, ip, C.c_int]
    lib.reroute_twin_routes.argtypes = [C.c_void_p, C.c_int, ip]
    lib.reroute_twin_reroute.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_double, dp, dp, dp, dp, dp, ip, ip, dp, ip, dp, ip]
    return lib


@functools.lru_cache(None)
def trace():
    """the recorder kernels (tests/emul_trace)"""
    lib = _load("trace")
    lib.trace_emu_record_bytes.restype = C.c_longlong
    lib.trace_emu_record_bytes.argtypes = [C.c_int] * 3
    lib.trace_emu_entries.argtypes = [C.c_int] * 3
    lib.trace_emu_record.argtypes = ([C.c_int] * 5 + [dp, dp, ip, ip, ip, ip, ip, dp, dp, dp, dp, dp, dp, dp, dp, dp,
                                                      C.c_longlong, C.c_int] + [dp, dp, ip, dp, dp, ip, ip, ip, dp, dp, dp, dp, dp])
    return lib


@functools.lru_cache(None)
def plant():
    """K3n / K3p (tests/emul_plant)"""
    lib = _load("plant")
    lib.pl_emu_philox.argtypes = [up, up, up]
    lib.pl_emu_philox.restype = None
    lib.pl_emu_noise.argtypes = [C.c_uint64, C.c_int32, C.c_int, C.c_int, lp, dp]
    lib.pl_emu_noise.restype = None
    lib.pl_emu_check.argtypes = [C.c_int, C.c_int, dp, dp]
    lib.pl_emu_measure.argtypes = [dp, dp, dp, dp]
    lib.pl_emu_measure.restype = None
    lib.pl_emu_advance.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int), dp, C.c_double, dp, dp, dp,
                                   dp, dp, dp]
    lib.pl_emu_stats.argtypes = [C.c_double] * 6 + [dp, dp, C.POINTER(C.c_int)]
    lib.pl_emu_stats.restype = None
    return lib
