"""ctypes binding of the C ABI declared in include/mpmpc.h (libmpmpc.so, HIP kernels for gfx950).

This is the only place Python touches the device library.  There is no CPU fallback: if the
shared library is missing or no HIP device is present, construction of a `Handle` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libmpmpc.so")

NX, NU = 3, 2
NUM_FIELDS = 27
MAX_HORIZON = 255

SOLVED, SOLVED_INACCURATE = 1, 2
MAX_ITER_REACHED, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, UNSOLVED = -2, -3, -4, -10
REC_PLAN, REC_PRED, REC_ROWS = 1, 2, 4      # optional fields of a rollout record (mpmpc_rollout_record)
REC_PLANT, REC_DELAY, REC_EST, REC_FIX, REC_SCAN = 8, 16, 32, 64, 128      # ... and the pose chain (mpmpc_rollout_trace_chain)


class Config(C.Structure):
    """mpmpc_config"""
    _fields_ = [("N", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32), ("circular", C.c_int32),
                ("Q", C.c_double * 3), ("R", C.c_double * 2), ("QN", C.c_double * 3),
                ("xmin", C.c_double * 3), ("xmax", C.c_double * 3),
                ("umin", C.c_double * 2), ("umax", C.c_double * 2),
                ("ay_max", C.c_double), ("wheelbase", C.c_double), ("QN_offdiag", C.c_double * 3),
                ("Q_offdiag", C.c_double * 3), ("R_offdiag", C.c_double * 1)]


class Settings(C.Structure):
    """mpmpc_settings (OSQP 0.6.x names/defaults for the ADMM stage + certified polish)"""
    _fields_ = [("rho", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double),
                ("eps_abs", C.c_double), ("eps_rel", C.c_double),
                ("eps_prim_inf", C.c_double), ("eps_dual_inf", C.c_double),
                ("max_iter", C.c_int32), ("check_termination", C.c_int32), ("scaling", C.c_int32),
                ("adaptive_rho", C.c_int32), ("adaptive_rho_interval", C.c_int32),
                ("adaptive_rho_tolerance", C.c_double),
                ("polish", C.c_int32), ("ipm_max_iter", C.c_int32),
                ("ipm_tol", C.c_double), ("ipm_reg", C.c_double), ("as_delta", C.c_double),
                ("as_refine", C.c_int32), ("as_rounds", C.c_int32), ("cert_tol", C.c_double),
                ("early_polish", C.c_int32), ("early_scaling", C.c_int32), ("phase1", C.c_int32),
                ("ipm_diverged", C.c_double), ("phase1_theta", C.c_double), ("phase1_eps", C.c_double),
                ("reduce", C.c_int32),
                ("ipm_start_slack", C.c_double), ("ipm_start_mu", C.c_double),
                ("ipm_start_dual", C.c_double), ("as_add_fraction", C.c_double), ("phase1_accept", C.c_int32), ("native", C.c_int32),
                ("native_ipm_tol", C.c_double), ("early_start", C.c_int32), ("phase1_band", C.c_double)]


def default_settings(**kw) -> Settings:
    s = Settings(rho=0.1, sigma=1e-6, alpha=1.6, eps_abs=1e-3, eps_rel=1e-3, eps_prim_inf=1e-4,
                 eps_dual_inf=1e-4, max_iter=4000, check_termination=25, scaling=10, adaptive_rho=1,
                 adaptive_rho_interval=50, adaptive_rho_tolerance=5.0, polish=2, ipm_max_iter=30,
                 ipm_tol=1e-8, ipm_reg=1e-8, as_delta=1e-10, as_refine=5, as_rounds=4, cert_tol=1e-8, early_polish=1,
                 early_scaling=1, phase1=1, ipm_diverged=1e2, phase1_theta=1.0, phase1_eps=1e-6, reduce=1,
                 ipm_start_slack=0.1, ipm_start_mu=0.01, ipm_start_dual=0.2, as_add_fraction=0.25, phase1_accept=1, native=1, native_ipm_tol=1e-7, early_start=0, phase1_band=3.0)
    for k, v in kw.items():
        if not hasattr(s, k):
            raise TypeError("unknown solver setting %r" % k)
        setattr(s, k, v)
    return s


def stock_settings(**kw) -> Settings:
    """The reference's own solver call (src/MPC.py:158-159,183): OSQP at its defaults and nothing else - no polish, no
    phase 1; statuses and iterates are those of the restated OSQP (eps = 1e-3: up to ~1 rad away from the optimum in
    delta_0 on this problem family)."""
    return default_settings(polish=0, early_polish=0, phase1=0, reduce=0, **kw)


def make_config(N, Q, R, QN, xmin, xmax, umin, umax, ay_max, wheelbase, circular=True, max_batch=1,
                device=0) -> Config:
    if not 3 <= int(N) <= MAX_HORIZON:
        raise ValueError("horizon N must satisfy 3 <= N <= %d" % MAX_HORIZON)
    c = Config(N=int(N), max_batch=int(max_batch), device=int(device), circular=int(bool(circular)),
               ay_max=float(ay_max), wheelbase=float(wheelbase))
    # The reference puts the WHOLE weight matrices into the Hessian (src/MPC.py:150): a matrix argument is split into its
    # diagonal and its off-diagonal entries; a vector argument is a diagonal.
    def split(M, n, name):
        M = np.asarray(M.toarray() if hasattr(M, "toarray") else M, float)
        if M.shape != (n, n):
            return M, None
        if not np.array_equal(M, M.T):
            raise ValueError("%s must be symmetric" % name)
        return np.diag(M).copy(), [M[i, j] for i in range(n) for j in range(i + 1, n)]
    QN, off = split(QN, 3, "QN")
    if off is not None:
        c.QN_offdiag = (C.c_double * 3)(*off)
    Q, off = split(Q, 3, "Q")
    if off is not None:
        c.Q_offdiag = (C.c_double * 3)(*off)
    R, off = split(R, 2, "R")
    if off is not None:
        c.R_offdiag = (C.c_double * 1)(*off)
    for name, val, n in (("Q", Q, 3), ("R", R, 2), ("QN", QN, 3), ("xmin", xmin, 3), ("xmax", xmax, 3),
                         ("umin", umin, 2), ("umax", umax, 2)):
        a = np.asarray(val, float).ravel()
        if a.size != n:
            raise ValueError("%s must have %d entries" % (name, n))
        setattr(c, name, (C.c_double * n)(*a))
    return c


def stage_ld(N: int) -> int:
    for ld in (16, 32, 64, 128):
        if N + 1 <= ld:
            return ld
    return 256


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


_lib = None


def load_library(path: str | None = None):
    """dlopen libmpmpc.so and declare every entry point of include/mpmpc.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError("mpmpc: %s not found - build it with `python __graft_entry__.py` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
    lib = C.CDLL(p)
    h = C.c_void_p
    lib.mpmpc_version.restype = C.c_char_p
    lib.mpmpc_last_error.restype = C.c_char_p
    lib.mpmpc_device_count.argtypes = [_ip]
    lib.mpmpc_default_settings.argtypes = [C.POINTER(Settings)]
    lib.mpmpc_default_settings.restype = None
    lib.mpmpc_create.argtypes = [C.POINTER(Config), C.POINTER(Settings), C.POINTER(h)]
    lib.mpmpc_destroy.argtypes = [h]
    lib.mpmpc_set_settings.argtypes = [h, C.POINTER(Settings)]
    lib.mpmpc_set_packing.argtypes = [h, C.c_int32]
    lib.mpmpc_set_tail_kernel.argtypes = [h, C.c_int32]
    lib.mpmpc_set_pipeline.argtypes = [h, C.c_int32]
    lib.mpmpc_hw_queue_budget.argtypes = [C.c_char_p]
    lib.mpmpc_hw_queue_budget.restype = C.c_int32
    lib.mpmpc_pipeline_streams.argtypes = [C.c_int32, C.c_int32]
    lib.mpmpc_pipeline_streams.restype = C.c_int32
    lib.mpmpc_launch_plan.argtypes = [C.POINTER(Config), C.POINTER(Settings), _ip, C.c_int32, C.c_int32, C.c_int32, _ip]
    lib.mpmpc_launch_plan.restype = C.c_int32
    lib.mpmpc_set_path.argtypes = [h, C.c_int32, _dp, _dp, _dp]
    lib.mpmpc_set_corridor.argtypes = [h, C.c_int32, C.c_int32, _dp, _dp]
    lib.mpmpc_check_routes.argtypes = [C.c_int32, C.c_int32, _ip, _ip]
    lib.mpmpc_set_routes.argtypes = [h, C.c_int32, _ip, _ip]
    lib.mpmpc_set_car_routes.argtypes = [h, C.c_int32, _ip]
    lib.mpmpc_project.argtypes = [C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, C.c_int32, _ip, C.c_int32, _dp, C.c_int32, _ip,
                                  C.c_double, _ip, _dp, _dp, _dp]
    lib.mpmpc_rollout_reroute.argtypes = [h, C.c_int32, _ip, C.c_double, C.c_double, _ip]
    lib.mpmpc_rollout_routes.argtypes = [h, C.c_int32, _ip]
    lib.mpmpc_set_map.argtypes = [h, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double]
    lib.mpmpc_set_path_geometry.argtypes = [h, C.c_int32, _dp, _dp, _dp, _dp, _dp]
    lib.mpmpc_build_corridor.argtypes = [h, C.c_int32, C.c_double, C.c_double, _dp, _dp, _ip]
    lib.mpmpc_rollout_init.argtypes = [h, C.c_int32, C.c_double, _dp, _dp, _dp, _dp]
    lib.mpmpc_rollout_step.argtypes = [h, C.c_int32, C.c_int32]
    lib.mpmpc_rollout_set_counters.argtypes = [h, C.c_int32, _ip]
    lib.mpmpc_rollout_warm_start.argtypes = [h, C.c_int32]
    lib.mpmpc_rollout_state.argtypes = [h, C.c_int32, _dp, _dp, _dp, _ip, _dp, _dp, _ip, _ip, _ip]
    lib.mpmpc_rollout_set_obstacles.argtypes = [h, C.c_int32, _ip, _ip]
    lib.mpmpc_rollout_corridor.argtypes = [h, C.c_int32, _dp, _dp]
    lib.mpmpc_rollout_set_movers.argtypes = [h, C.c_int32, _ip, _ip, _ip, _dp, C.c_int64]
    lib.mpmpc_rollout_obstacles.argtypes = [h, C.c_int32, _ip, _ip]
    lib.mpmpc_rollout_set_lookahead.argtypes = [h, C.c_int32, _dp, C.c_int32]
    lib.mpmpc_rollout_lookahead.argtypes = [h, C.c_int32, _ip, _ip]
    lib.mpmpc_rollout_set_lookahead_traffic.argtypes = [h, C.c_int32]
    lib.mpmpc_rollout_tracks.argtypes = [h, C.c_int32, _ip, _ip, _dp]
    lib.mpmpc_rollout_lookahead_traffic.argtypes = [h, C.c_int32, _ip, _ip]
    lib.mpmpc_rollout_set_traffic.argtypes = [h, C.c_int32, _ip, _ip, C.c_int32, C.c_int32]
    lib.mpmpc_rollout_set_walls.argtypes = [h, C.c_int32, _ip, _ip]
    lib.mpmpc_rollout_set_plant.argtypes = [h, C.c_int32, _dp, C.c_uint64, C.c_int32, C.c_int64, _dp]
    lib.mpmpc_rollout_plant.argtypes = [h, C.c_int32, _dp, _dp, _dp, _dp, _ip]
    lib.mpmpc_plant_noise.argtypes = [C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _dp]
    lib.mpmpc_rollout_set_delay.argtypes = [h, C.c_int32, _ip, _ip, _dp]
    lib.mpmpc_rollout_delay.argtypes = [h, C.c_int32, _dp, _dp, _dp, _dp]
    lib.mpmpc_rollout_set_commitment.argtypes = [h, C.c_int32, _dp, _ip, _dp]
    lib.mpmpc_rollout_commitment.argtypes = [h, C.c_int32, _ip, _ip, _dp]
    lib.mpmpc_rollout_set_dynamics.argtypes = [h, C.c_int32, _dp, _dp]
    lib.mpmpc_rollout_dynamics.argtypes = [h, C.c_int32, _dp, _ip, _dp]
    lib.mpmpc_dynamics_drive.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp]
    lib.mpmpc_rollout_set_estimator.argtypes = [h, C.c_int32, _dp, C.c_uint64, C.c_int32, C.c_int64, _dp, _dp]
    lib.mpmpc_rollout_estimator.argtypes = [h, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip]
    _i8p, _u8p = C.POINTER(C.c_int8), C.POINTER(C.c_uint8)
    lib.mpmpc_distance_field.argtypes = [C.c_int32, C.c_int32, C.c_int32, _i8p, C.c_int32, _u8p]
    lib.mpmpc_scan_match.argtypes = [C.c_int32, C.c_int32, C.c_int32, _i8p, C.c_double, C.c_double, C.c_double, C.c_int32, _dp, _dp,
                                     C.c_int32, _dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                     _dp, _ip, _ip, _ip]
    lib.mpmpc_rollout_set_localiser.argtypes = [h, C.c_int32, C.c_int32, _dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.c_int32, C.c_int64, _dp]
    lib.mpmpc_rollout_localiser.argtypes = [h, C.c_int32, _dp, _dp, _ip, _ip, _ip, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip, _ip]
    lib.mpmpc_rollout_record.argtypes = [h, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.mpmpc_rollout_recorded.argtypes = [h, _ip, _ip]
    lib.mpmpc_rollout_trace.argtypes = [h, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _ip, _dp, _dp, _ip, _ip, _ip, _dp, _dp, _dp, _dp, _dp]
    lib.mpmpc_rollout_trace_chain.argtypes = [h, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _ip,
                                              _ip, _ip, _dp]
    lib.mpmpc_assemble.argtypes = [h, C.c_int32, _ip, _dp, _dp, _dp, _dp, _dp]
    lib.mpmpc_stage_ld.argtypes = [C.c_int32]
    lib.mpmpc_stage_ld.restype = C.c_int32
    lib.mpmpc_solve.argtypes = [h, C.c_int32, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _dp]
    lib.mpmpc_upload.argtypes = [h, C.c_int32, _ip, _dp, _dp, _dp, _dp]
    lib.mpmpc_solve_resident.argtypes = [h, C.c_int32]
    lib.mpmpc_set_outputs.argtypes = [h, C.c_int32]
    lib.mpmpc_sync.argtypes = [h]
    lib.mpmpc_download.argtypes = [h, C.c_int32, _dp, _dp, _ip, _ip, _dp, _dp]
    lib.mpmpc_solve_resident_timed.argtypes = [h, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mpmpc_solve_resident_profile.argtypes = [h, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mpmpc_assemble_resident_timed.argtypes = [h, C.c_int32, C.c_int32, C.POINTER(C.c_float)]
    lib.mpmpc_speed_profile.argtypes = [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, C.c_double, _dp, _ip, _ip]
    lib.mpmpc_lidar_scan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double,
                                     C.c_int32, _dp, _ip, _ip, C.c_int32, _dp, C.c_double, _dp]
    lib.mpmpc_rollout_scan.argtypes = [h, C.c_int32, C.c_int32, _dp, C.c_double, _dp]
    lib.mpmpc_footprint_audit.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double,
                                          C.c_int32, _dp, _ip, _ip, C.c_double, C.c_double, C.c_double, _ip, _dp]
    lib.mpmpc_rollout_set_audit.argtypes = [h, C.c_int32, C.c_double, C.c_double, C.c_double]
    lib.mpmpc_rollout_audit.argtypes = [h, C.c_int32, _ip, _ip, _dp, _ip, _ip, _dp]
    lib.mpmpc_lidar_scan_world.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double,
                                           C.c_int32, _dp, _ip, _ip, _ip, _ip, C.c_int32, _dp, C.c_double, _dp]
    lib.mpmpc_footprint_audit_world.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double,
                                                C.c_int32, _dp, _ip, _ip, _ip, _ip, C.c_double, C.c_double, C.c_double, _ip, _dp]
    lib.mpmpc_world_grid.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double,
                                     C.c_int32, _ip, C.c_int32, _ip, C.POINTER(C.c_int8)]
    lib.mpmpc_perception_scan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double,
                                          C.c_int32, _dp, _ip, _ip, _ip, _ip, C.c_int32, _dp, C.c_double, _dp,
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.mpmpc_rollout_set_perception.argtypes = [h, C.c_int32, _dp, C.c_double, C.c_int32]
    lib.mpmpc_rollout_perception.argtypes = [h, C.c_int32, _ip, _ip, _ip, _ip, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.mpmpc_path_count.argtypes = [C.c_int32, _dp, C.c_double, C.c_int32]
    lib.mpmpc_path_count.restype = C.c_int32
    lib.mpmpc_path_build.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double,
                                     C.c_int32, _ip, _dp, _dp, _ip, _ip, _ip, _ip, _ip, C.c_int32, _ip, _ip] + [_dp] * 9
    lib.mpmpc_path_build_timed.argtypes = lib.mpmpc_path_build.argtypes + [C.POINTER(C.c_float)]
    _ipp, _dpp = C.POINTER(_ip), C.POINTER(_dp)
    lib.mpmpc_staging.argtypes = [h, C.c_int32, _ipp, _dpp, _dpp, _dpp, _dpp, _dpp, _dpp, _ipp, _ipp, _dpp, _dpp]
    lib.mpmpc_solve_staged.argtypes = [h, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.mpmpc_staged_begin.argtypes = [h, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.mpmpc_staged_end.argtypes = [h]
    if path is None:
        _lib = lib
    return lib


EXPORTS = ["mpmpc_version", "mpmpc_last_error", "mpmpc_device_count", "mpmpc_default_settings",
           "mpmpc_create", "mpmpc_destroy", "mpmpc_set_settings", "mpmpc_set_packing", "mpmpc_set_tail_kernel", "mpmpc_set_path", "mpmpc_set_corridor",
           "mpmpc_set_map", "mpmpc_set_path_geometry", "mpmpc_build_corridor", "mpmpc_rollout_init",
           "mpmpc_rollout_step", "mpmpc_rollout_set_counters", "mpmpc_rollout_warm_start", "mpmpc_rollout_state", "mpmpc_rollout_set_obstacles", "mpmpc_rollout_corridor",
           "mpmpc_rollout_set_movers", "mpmpc_rollout_obstacles", "mpmpc_rollout_set_traffic",
           "mpmpc_rollout_set_lookahead", "mpmpc_rollout_lookahead",
           "mpmpc_rollout_set_lookahead_traffic", "mpmpc_rollout_tracks", "mpmpc_rollout_lookahead_traffic",
           "mpmpc_rollout_record", "mpmpc_rollout_recorded", "mpmpc_rollout_trace", "mpmpc_rollout_trace_chain", "mpmpc_assemble", "mpmpc_stage_ld", "mpmpc_solve", "mpmpc_upload", "mpmpc_solve_resident", "mpmpc_set_outputs", "mpmpc_set_pipeline", "mpmpc_hw_queue_budget", "mpmpc_pipeline_streams", "mpmpc_launch_plan",
           "mpmpc_sync", "mpmpc_download", "mpmpc_solve_resident_timed", "mpmpc_solve_resident_profile", "mpmpc_assemble_resident_timed", "mpmpc_speed_profile", "mpmpc_lidar_scan", "mpmpc_rollout_scan",
           "mpmpc_footprint_audit", "mpmpc_rollout_set_audit", "mpmpc_rollout_audit", "mpmpc_rollout_set_walls",
           "mpmpc_lidar_scan_world", "mpmpc_footprint_audit_world", "mpmpc_world_grid", "mpmpc_staging",
           "mpmpc_perception_scan", "mpmpc_rollout_set_perception", "mpmpc_rollout_perception",
           "mpmpc_path_count", "mpmpc_path_build", "mpmpc_path_build_timed",
           "mpmpc_check_routes", "mpmpc_set_routes", "mpmpc_set_car_routes",
           "mpmpc_project", "mpmpc_rollout_reroute", "mpmpc_rollout_routes",
           "mpmpc_rollout_set_plant", "mpmpc_rollout_plant", "mpmpc_plant_noise",
           "mpmpc_rollout_set_delay", "mpmpc_rollout_delay",
           "mpmpc_rollout_set_dynamics", "mpmpc_rollout_dynamics", "mpmpc_dynamics_drive",
           "mpmpc_rollout_set_estimator", "mpmpc_rollout_estimator",
           "mpmpc_distance_field", "mpmpc_scan_match", "mpmpc_rollout_set_localiser", "mpmpc_rollout_localiser",
           "mpmpc_rollout_set_commitment", "mpmpc_rollout_commitment",
           "mpmpc_solve_staged", "mpmpc_staged_begin", "mpmpc_staged_end"]


class MpmpcError(RuntimeError):
    pass


# mpmpc_launch_plan: the fields of a row, kernel families and list roles (include/mpmpc.h)
PLAN_FIELDS = ("family", "G", "C", "var", "warm", "mode", "grid", "block", "reads", "fills", "clear", "deferrable", "turn")
PLAN_MAX_STAGES = 3
(K_GENERAL, K_REDUCED, K_REDUCED_T, K_REDUCED_TAIL, K_PAIR, K_PAIR_T, K_PAIR_TAIL, K_BLOCK, K_RBLOCK, K_PAIR_BLOCK,
 K_PAIR_BLOCK_TAIL, K_PAIR_BLOCK_T) = range(12)
LIST_NONE, LIST_THIS, LIST_NEXT, LIST_LEFT = range(4)


def launch_plan(config: Config, settings: Settings, B: int, closed_loop=False, kind=0, packing=0, tail_kernel=1, pipeline=3,
                warm_start=2):
    """The stages of a solve launch of B instances as the launcher decides them (no device needed): a list of dicts keyed by
    PLAN_FIELDS.  packing / tail_kernel / pipeline / warm_start: what mpmpc_set_packing, mpmpc_set_tail_kernel,
    mpmpc_pipeline_streams and mpmpc_rollout_warm_start leave in a handle; kind 1: one of several launches in flight."""
    lib = load_library()
    knobs = np.array([packing, tail_kernel, pipeline, warm_start], np.int32)
    rows = np.zeros((PLAN_MAX_STAGES, len(PLAN_FIELDS)), np.int32)
    n = lib.mpmpc_launch_plan(C.byref(config), C.byref(settings), _i(knobs), int(B), int(bool(closed_loop)), int(kind), _i(rows))
    if n < 0:
        raise MpmpcError("mpmpc error %d: %s" % (n, lib.mpmpc_last_error().decode()))
    return [dict(zip(PLAN_FIELDS, (int(v) for v in rows[i]))) for i in range(n)]


class Solution:
    """Outputs of one batched solve (host arrays)."""
    __slots__ = ("z", "u0", "status", "iters", "resid", "y")

    def __init__(self, z, u0, status, iters, resid, y):
        self.z, self.u0, self.status, self.iters, self.resid, self.y = z, u0, status, iters, resid, y


class _StagingView(np.ndarray):
    """ndarray view into a handle's staging block; carries a reference to the Handle that owns the memory"""
    _owner = None

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)


class Handle:
    """One device context: controller constants, path tables, device buffers for max_batch QPs."""

    def __init__(self, config: Config, settings: Settings | None = None):
        self.lib = load_library()
        self.cfg = config
        self.N = config.N
        self.n = 5 * self.N + 3
        self.m = 8 * self.N + 6
        self.settings = settings or default_settings()
        self._h = C.c_void_p()
        self._check(self.lib.mpmpc_create(C.byref(self.cfg), C.byref(self.settings), C.byref(self._h)))
        self._have_table = False

    def _check(self, rc):
        if rc != 0:
            raise MpmpcError("mpmpc error %d: %s" % (rc, self.lib.mpmpc_last_error().decode()))

    def close(self):
        if self._h:
            self.lib.mpmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_settings(self, settings: Settings):
        self.settings = settings
        self._check(self.lib.mpmpc_set_settings(self._h, C.byref(settings)))

    def set_packing(self, lanes_per_instance: int = 0):
        """0 = automatic; 64 / 32 / 16 force that many lanes of a wavefront per instance (tests, tuning).  16 at horizons
        16 .. 31: two stages per lane, four instances per wavefront (measured slower than 32: never automatic).  Horizons above
        63: 128 (N <= 127) / 256 (N >= 128) select the one-stage workgroup kernels instead of the two-stages-per-lane default."""
        self._check(self.lib.mpmpc_set_packing(self._h, int(lanes_per_instance)))

    def set_tail_kernel(self, reduced_native: bool = True):
        """True / 1 (default): the reduced-native tail kernel takes the tail of a batch launch first, two instances per wavefront;
        2: the same, one instance per wavefront; False / 0: the general kernel takes all of it (parity tests, A/B timings)."""
        self._check(self.lib.mpmpc_set_tail_kernel(self._h, int(reduced_native)))

    def set_path(self, kappa, v_ref, ds_next):
        k, v, d = (np.ascontiguousarray(a, dtype=np.float64) for a in (kappa, v_ref, ds_next))
        if not (k.size == v.size == d.size):
            raise ValueError("path tables must have equal length")
        self._check(self.lib.mpmpc_set_path(self._h, k.size, _d(k), _d(v), _d(d)))

    def set_corridor(self, ub, lb):
        ub = np.ascontiguousarray(ub, dtype=np.float64)
        lb = np.ascontiguousarray(lb, dtype=np.float64)
        if ub.shape != lb.shape or ub.ndim != 2:
            raise ValueError("corridor tables must be equal-shape [n_wp x n_cols]")
        self._check(self.lib.mpmpc_set_corridor(self._h, ub.shape[0], ub.shape[1], _d(ub), _d(lb)))
        self._have_table = True

    # --- route fleets: the path tables are the concatenation of several routes, every instance is on one of them
    def set_routes(self, first, circular):
        """After set_path: route p is rows first[p] .. first[p + 1] - 1 of every per-waypoint table (first[0] = 0, first[-1] =
        the path's length; concat_routes returns it) with its own circular[p].  wp_id is then local to an instance's route in
        every call.  An empty `circular` (P = 0) returns the handle to one path; a new set_path clears the routes."""
        f = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        c = np.ascontiguousarray(circular, dtype=np.int32).reshape(-1)
        if c.size and f.size != c.size + 1:
            raise ValueError("first needs one entry more than circular")
        self._check(self.lib.mpmpc_set_routes(self._h, c.size, _i(f) if c.size else None, _i(c) if c.size else None))

    def set_car_routes(self, route):
        """route[i]: the route of instance i in every later call on len(route) instances, until set again."""
        r = np.ascontiguousarray(route, dtype=np.int32).reshape(-1)
        self._check(self.lib.mpmpc_set_car_routes(self._h, r.size, _i(r)))
        self._route_B = r.size

    # --- corridor generation on the device (dynamic maps)
    def set_map(self, data, origin, resolution):
        grid = np.ascontiguousarray(data, dtype=np.int8)
        if grid.ndim != 2:
            raise ValueError("map grid must be 2-D [height, width]")
        self._check(self.lib.mpmpc_set_map(self._h, grid.shape[0], grid.shape[1],
                                           grid.ctypes.data_as(C.POINTER(C.c_int8)), float(origin[0]),
                                           float(origin[1]), float(resolution)))

    def set_path_geometry(self, x, y, psi, border_ub, border_lb):
        x, y, psi = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, psi))
        bu = np.ascontiguousarray(border_ub, dtype=np.float64).reshape(x.size, 2)
        bl = np.ascontiguousarray(border_lb, dtype=np.float64).reshape(x.size, 2)
        self._check(self.lib.mpmpc_set_path_geometry(self._h, x.size, _d(x), _d(y), _d(psi), _d(bu), _d(bl)))
        self._n_wp = x.size

    def build_corridor(self, n_cols, min_width, safety_margin, want_tables=True):
        """update_path_constraints(w + 1, n_cols, ...) for every start waypoint w, on the device; the
        handle then uses the result like a table given to set_corridor.  -> (ub, lb, bad_rows)"""
        n = self._n_wp
        ub = np.zeros((n, n_cols)) if want_tables else None
        lb = np.zeros((n, n_cols)) if want_tables else None
        bad = C.c_int32(0)
        self._check(self.lib.mpmpc_build_corridor(self._h, int(n_cols), float(min_width), float(safety_margin),
                                                  _d(ub), _d(lb), C.byref(bad)))
        self._have_table = True
        return ub, lb, bad.value

    # --- closed-loop rollout on the device
    def rollout_init(self, Ts, cum_lengths, s, poses, cc0=None):
        cum = np.ascontiguousarray(cum_lengths, dtype=np.float64)
        s = np.ascontiguousarray(s, dtype=np.float64).ravel()
        B = s.size
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(B, 3)
        if cc0 is not None:
            cc0 = np.ascontiguousarray(cc0, dtype=np.float64).reshape(B, 2 * self.N)
        self._check(self.lib.mpmpc_rollout_init(self._h, B, float(Ts), _d(cum), _d(s), _d(poses), _d(cc0)))
        self._ro_B = B
        return B

    def rollout_set_counters(self, counters):
        """MPC.infeasibility_counter of every car (to resume a recorded run)"""
        c = np.ascontiguousarray(counters, dtype=np.int32).ravel()
        self._check(self.lib.mpmpc_rollout_set_counters(self._h, c.size, _i(c)))

    def rollout_reroute(self, route, max_dist=np.inf, max_heading=np.pi / 2):
        """Route fleets, between rollout_step calls: route[i] >= 0 projects running car i from its current pose onto that route
        (nearest waypoint whose heading differs by at most max_heading) and, if it lies within max_dist, puts the car on it with
        s at that waypoint; -1 keeps the car's route.  Everything else of the rollout stays, on the device (include/mpmpc.h).
        -> accepted, bool [B]."""
        r = np.ascontiguousarray(route, dtype=np.int32).reshape(-1)
        acc = np.zeros(r.size, np.int32)
        self._check(self.lib.mpmpc_rollout_reroute(self._h, r.size, _i(r), float(max_dist), float(max_heading), _i(acc)))
        return acc != 0

    def rollout_routes(self):
        """-> the route every car of the last set_car_routes is on now (rollout_reroute moves cars), int32 [B]."""
        out = np.zeros(getattr(self, "_route_B", 0), np.int32)
        self._check(self.lib.mpmpc_rollout_routes(self._h, out.size, _i(np.zeros(1, np.int32)) if out.size == 0 else _i(out)))
        return out

    def rollout_warm_start(self, enable=True):
        """closed loop: try the previous step's shifted active set first.  True / False force it on / off, "auto"
        (the handle's default) uses it for fleets of more than 1024 or at most 16 cars, where it pays."""
        self._check(self.lib.mpmpc_rollout_warm_start(self._h, 2 if enable == "auto" else int(bool(enable))))

    def rollout_step(self, n_steps=1):
        self._check(self.lib.mpmpc_rollout_step(self._h, self._ro_B, int(n_steps)))

    def rollout_state(self):
        """-> dict(s, pose, cc, wp_id, x0, u, status, counter, alive) of the rollout's cars.  alive: 1 running, 0 lap
        finished, -1 ended after N - 1 consecutive infeasible steps, -2 ended at the end of an open path, -3 / -4 (per-car
        obstacles) no free segment at the first horizon waypoint of the car's world / more than 8 free segments on a border
        line of it (include/mpmpc.h)."""
        B, N = self._ro_B, self.N
        out = dict(s=np.zeros(B), pose=np.zeros((B, 3)), cc=np.zeros((B, 2 * N)), wp_id=np.zeros(B, np.int32),
                   x0=np.zeros((B, 3)), u=np.zeros((B, 2)), status=np.zeros(B, np.int32),
                   counter=np.zeros(B, np.int32), alive=np.zeros(B, np.int32))
        self._check(self.lib.mpmpc_rollout_state(self._h, B, _d(out["s"]), _d(out["pose"]), _d(out["cc"]),
                                                 _i(out["wp_id"]), _d(out["x0"]), _d(out["u"]), _i(out["status"]),
                                                 _i(out["counter"]), _i(out["alive"])))
        return out

    def rollout_set_obstacles(self, discs):
        """Per-car obstacle worlds: discs = one int [k_b, 3] array of (cx, cy, r) map cells per car (Map.obstacle_discs;
        k_b may be 0, at most 64), or None for the shared corridor table.  Needs build_corridor on the current map; may be
        called between rollout_step calls (applies from the next step, keeps the rollout's state)."""
        if discs is None:
            self._check(self.lib.mpmpc_rollout_set_obstacles(self._h, 0, None, None))
            return
        lists = [np.asarray(d, dtype=np.int32).reshape(-1, 3) for d in discs]
        off = np.zeros(len(lists) + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in lists])
        flat = np.ascontiguousarray(np.concatenate(lists) if off[-1] else np.zeros((0, 3), np.int32), dtype=np.int32)
        self._check(self.lib.mpmpc_rollout_set_obstacles(self._h, len(lists), _i(off), _i(flat) if flat.size else None))

    def rollout_corridor(self):
        """-> (ub, lb) [B, N]: the rows the last rollout step used per car (per-car obstacles); NaN rows for alive -3 / -4"""
        B, N = self._ro_B, self.N
        ub, lb = np.zeros((B, N)), np.zeros((B, N))
        self._check(self.lib.mpmpc_rollout_corridor(self._h, B, _d(ub), _d(lb)))
        return ub, lb

    def rollout_set_movers(self, movers, step0=0):
        """Per-car moving obstacles, advanced on the device every step (K0m): movers = one [k_b, 6] array per car of rows
        (kind, radius in cells, p0, p1, p2, p3) - movers.Mover.row() - or None for no movers.  kind 0: (x0, y0, dx, dy), a
        straight line; kind 1: (s0, e_y, ds, 0), along the reference path; displacements are per rollout step, counted from
        step0 (which may be negative: resuming a run).  Combines with rollout_set_obstacles (together at most 64 per car,
        the same number of cars); needs build_corridor on the current map; may be called between rollout_step calls."""
        if movers is None:
            self._check(self.lib.mpmpc_rollout_set_movers(self._h, 0, None, None, None, None, 0))
            self._n_movers = 0
            return
        lists = [np.asarray(m, dtype=np.float64).reshape(-1, 6) for m in movers]
        off = np.zeros(len(lists) + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in lists])
        flat = np.concatenate(lists) if off[-1] else np.zeros((0, 6))
        if not np.array_equal(flat[:, :2], np.floor(flat[:, :2])) or np.any(np.abs(flat[:, :2]) > 2 ** 30):
            raise ValueError("mover kind and radius (cells) must be integers")
        kind, rad = (np.ascontiguousarray(flat[:, c], dtype=np.int32) for c in (0, 1))
        prm = np.ascontiguousarray(flat[:, 2:], dtype=np.float64)
        self._check(self.lib.mpmpc_rollout_set_movers(self._h, len(lists), _i(off), _i(kind), _i(rad), _d(prm), int(step0)))
        self._n_movers = int(off[-1])      # (rollout_lookahead sizes its disc table by it)

    def rollout_set_lookahead(self, seg_time, max_lead=1):
        """Lookahead (K0h; the law: csrc/lookahead_core.hpp): column c of every car's horizon sees the car's movers at step
        k + lead_c, lead_c = min(floor(t_c / Ts), max_lead) with t_c the running sum of seg_time [n_wp] (seconds from
        waypoint i to i + 1, by global row of the path table; lookahead.Lookahead.seg_time_of gives ds_next / v_ref) from the
        car's waypoint on.  None switches it off (the default).  May be called between rollout_step calls; void after a
        change of map, path, routes or geometry like the per-car settings."""
        if seg_time is None:
            self._check(self.lib.mpmpc_rollout_set_lookahead(self._h, 0, None, 0))
            return
        t = np.ascontiguousarray(seg_time, dtype=np.float64).ravel()
        self._check(self.lib.mpmpc_rollout_set_lookahead(self._h, t.size, _d(t), int(max_lead)))

    def rollout_lookahead(self):
        """-> (lead int32 [B, N], discs int32 [movers, N, 3]): what the last step's K0h wrote - every column's lead and
        every mover's disc at every column of its car (mover-major, rollout_set_movers' order; ungated: K0c drops the
        columns of a mover whose slot is absent at the step itself)."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        lead = np.zeros((max(B, 1), self.N), np.int32)
        discs = np.zeros((int(getattr(self, "_n_movers", 0)), self.N, 3), np.int32)
        self._check(self.lib.mpmpc_rollout_lookahead(self._h, B, _i(lead), _i(discs) if discs.size else None))
        return lead[:B], discs

    def rollout_set_lookahead_traffic(self, enable=True):
        """Lookahead for traffic (K3t, K0ht; the law: csrc/traffic_lookahead_core.hpp): while rollout_set_lookahead and
        rollout_set_traffic are both in force, column c of a car's horizon sees the cars in its traffic slots where their own
        plans of the step before put them at step k + lead_c (a neighbour without a valid plan, or a column with lead 0: where
        it is now).  A fleet-wide flag, off by default, independent of the order of the three calls; such a step looks ahead
        with or without movers.  rollout_init, rollout_reroute and switching it on make every plan invalid for one step."""
        self._check(self.lib.mpmpc_rollout_set_lookahead_traffic(self._h, 1 if enable else 0))

    def rollout_tracks(self):
        """-> dict(valid bool [B], cells int32 [B, N + 1, 2], tm [B, N + 1]): the plan tracks the last step left - the map cell
        of every stage of every car's plan ((INT32_MIN, 0): none) and the running maximum of its arrival times; valid: the
        next step may read the car's track (the car is running and its solve was usable).  lookahead.plan_tracks restates it."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        n = max(B, 1)
        valid, cells, tm = np.zeros(n, np.int32), np.zeros((n, self.N + 1, 2), np.int32), np.zeros((n, self.N + 1))
        self._check(self.lib.mpmpc_rollout_tracks(self._h, B, _i(valid), _i(cells), _d(tm)))
        return dict(valid=valid[:B] != 0, cells=cells[:B], tm=tm[:B])

    def rollout_lookahead_traffic(self):
        """-> (who int32 [B, S], discs int32 [B, S, N, 3]): what the last step's K0t and K0ht wrote - the car in every traffic
        slot (-1: empty) and the slot's disc at every column of its car (ungated: K0c keeps the staged entry of a slot that is
        absent in the list it plans from).  lookahead.traffic_discs restates it."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        S = int(getattr(self, "_tr_S", 0))
        who, discs = np.zeros((max(B, 1), max(S, 1)), np.int32), np.zeros((max(B, 1), max(S, 1), self.N, 3), np.int32)
        self._check(self.lib.mpmpc_rollout_lookahead_traffic(self._h, B, _i(who), _i(discs)))
        return who[:B, :S], discs[:B, :S]

    def rollout_set_traffic(self, group, radius_cells=None, slots=1, range_cells=-1):
        """Traffic: the cars of a group see each other as discs, from the fleet's own poses, every step on the device (K0t).
        group [B] ints (the same non-negative value: one world; negative: sees nobody, is seen by nobody), radius_cells [B]
        the disc of each car as the others see it, slots the discs a car gets (the nearest, ties by car index),
        range_cells how far it sees (negative: no limit); None switches traffic off.  Combines with rollout_set_obstacles
        and rollout_set_movers (together at most 64 per car, the same number of cars); needs build_corridor on the current
        map; may be called between rollout_step calls.  traffic.traffic_discs gives the slots of any state."""
        if group is None:
            self._check(self.lib.mpmpc_rollout_set_traffic(self._h, 0, None, None, 0, -1))
            self._tr_S = 0
            return
        grp, rad = (np.asarray(a) for a in (group, radius_cells))
        if grp.ndim != 1 or rad.shape != grp.shape:
            raise ValueError("group and radius_cells must be [B]")
        for a in (grp, rad):
            if a.size and (not np.array_equal(a, np.floor(a)) or np.any(np.abs(a) > 2 ** 30)):
                raise ValueError("group and radius_cells must be integers")
        grp, rad = (np.ascontiguousarray(a, dtype=np.int32) for a in (grp, rad))
        self._check(self.lib.mpmpc_rollout_set_traffic(self._h, grp.size, _i(grp), _i(rad), int(slots), int(range_cells)))
        self._tr_S = int(slots)      # (rollout_lookahead_traffic sizes its arrays by it)

    def rollout_set_walls(self, walls):
        """Per-car boundary walls (Map.add_boundary on the device; the law: csrc/wall_core.hpp): walls = one int [k_b, 4]
        array of (x0, y0, x1, y1) map cells per car (Map.boundary_walls; k_b may be 0, at most 16), or None for no walls.
        A fourth setting beside rollout_set_obstacles / _movers / _traffic (the same number of cars); needs build_corridor
        on the current map; may be called between rollout_step calls (applies from the next step, keeps the rollout's
        state).  rollout_corridor, rollout_scan, the audit and recorded rows see the walls; rollout_obstacles returns discs."""
        if walls is None:
            self._check(self.lib.mpmpc_rollout_set_walls(self._h, 0, None, None))
            return
        off, flat = _wall_csr(walls)
        self._check(self.lib.mpmpc_rollout_set_walls(self._h, off.size - 1, _i(off), _i(flat) if flat.size else None))

    def rollout_obstacles(self):
        """-> one int32 [k_b, 3] array of (cx, cy, r) per car: the discs the last rollout step used - the car's static discs,
        then its movers where that step had them, then its traffic slots (rollout_set_traffic); an absent mover (off the
        map, past the end of an open path) or an empty slot is (0, 0, 0)"""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        off = np.zeros(B + 1, np.int32)
        self._check(self.lib.mpmpc_rollout_obstacles(self._h, B, None, _i(off)))
        flat = np.zeros((int(off[-1]), 3), np.int32)
        self._check(self.lib.mpmpc_rollout_obstacles(self._h, B, _i(flat) if flat.size else None, None))
        return [flat[off[b]:off[b + 1]] for b in range(B)]

    def rollout_scan(self, angles, range_m):
        """Lidar scans of every car of the running rollout (K0l), from the pose its last step left it at, in the world that
        step gave it - the resident map plus the discs rollout_obstacles() returns (the base map when no per-car setting is
        in force).  angles [n] ascending (lidar_model.LidarModel.measurements[0]), range_m in metres -> ranges [B, n].
        Changes nothing the rollout reads."""
        ang = np.ascontiguousarray(angles, dtype=np.float64).ravel()
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        out = np.zeros((B, ang.size))
        self._check(self.lib.mpmpc_rollout_scan(self._h, B, ang.size, _d(ang), float(range_m), _d(out)))
        return out

    # --- perception of the rollout: plan on what the lidar saw (K0s; the law: csrc/perception_core.hpp)
    def rollout_set_perception(self, angles, range_m=0.0, hold=0):
        """Every step of the rollouts that follow, every running car scans its TRUE world (angles [n] ascending,
        lidar_model.LidarModel.measurements[0]; range_m in metres) and its corridor is built from what it KNOWS: the base map,
        static discs and walls once seen, a mover for `hold` further steps after it was last seen, a traffic slot while
        seen.  None switches perception off (the default).  Needs set_map; the setting outlives rollout_init, the
        knowledge starts over with it, with this call and with every per-car setter.  The audit, rollout_scan and
        rollout_obstacles stay in the true world; rollout_corridor and recorded rows are the perceived world's."""
        if angles is None:
            self._check(self.lib.mpmpc_rollout_set_perception(self._h, 0, None, 0.0, 0))
            return
        ang = np.ascontiguousarray(angles, dtype=np.float64).ravel()
        self._check(self.lib.mpmpc_rollout_set_perception(self._h, ang.size, _d(ang), float(range_m), int(hold)))

    def rollout_perception(self):
        """-> dict: disc_first, disc_last [B, 64], wall_first, wall_last [B, 16] (the step a slot was first / last seen at, -1:
        never, and for unused slots; disc slots in rollout_obstacles' order), disc_known [B] uint64, wall_known [B] uint32
        (bit q = slot q: the masks the last step planned with)"""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        out = dict(disc_first=np.zeros((B, 64), np.int32), disc_last=np.zeros((B, 64), np.int32),
                   wall_first=np.zeros((B, 16), np.int32), wall_last=np.zeros((B, 16), np.int32),
                   disc_known=np.zeros(B, np.uint64), wall_known=np.zeros(B, np.uint32))
        self._check(self.lib.mpmpc_rollout_perception(self._h, B, _i(out["disc_first"]), _i(out["disc_last"]), _i(out["wall_first"]),
                                                      _i(out["wall_last"]), out["disc_known"].ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      out["wall_known"].ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    # --- plant models of the rollout: the vehicle that differs from the controller's model, per car
    PLANT_FIELDS = ("act", "meas", "ey_max", "ey_sq", "steps")

    def rollout_set_plant(self, params, seed=0, car0=0, step0=0, act0=None):
        """The true vehicle of the rollouts that follow (K3n / K3p; the law: csrc/plant_core.hpp): params [B, 11] per car -
        plant.Plant.params(B): speed_gain, steer_gain, steer_offset, wheelbase_scale, speed_lag, steer_lag, steer_rate,
        speed_noise, steer_noise, position_noise, heading_noise - or None for no plant (the default: every car drives the
        controller's own model).  A draw of the noise depends on (seed, car0 + car, k - step0, channel) only.  act0 [B, 2]: the
        executed (v, delta) the actuators start from (None: zeros).  The true pose stays rollout_state()["pose"] - what the
        audit, rollout_scan, perception, traffic, the recorder and rollout_reroute read; the controllers localise on the
        measured pose (rollout_plant()["meas"]).  May be called before rollout_init or between rollout_step calls."""
        if params is None:
            self._check(self.lib.mpmpc_rollout_set_plant(self._h, 0, None, 0, 0, 0, None))
            return
        p = np.ascontiguousarray(params, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 11:
            raise ValueError("plant parameters must be [B, 11] (plant.Plant.params)")
        a = None if act0 is None else np.ascontiguousarray(act0, dtype=np.float64).reshape(p.shape[0], 2)
        self._check(self.lib.mpmpc_rollout_set_plant(self._h, p.shape[0], _d(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(car0), int(step0),
                                                     _d(a)))

    def rollout_plant(self):
        """-> dict of the plant's per-car state: act [B, 2] the executed (v, delta) of the last driven step, meas [B, 3] the
        pose the controller saw in the last step, ey_max / ey_sq / steps [B]: max |e|, sum of e^2 and the number of steps over
        the steps the car was driven - e the lateral offset of the TRUE pose from the step's waypoint."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        out = dict(act=np.zeros((B, 2)), meas=np.zeros((B, 3)), ey_max=np.zeros(B), ey_sq=np.zeros(B), steps=np.zeros(B, np.int32))
        self._check(self.lib.mpmpc_rollout_plant(self._h, B, _d(out["act"]), _d(out["meas"]), _d(out["ey_max"]), _d(out["ey_sq"]),
                                                 _i(out["steps"])))
        return out

    # --- actuation delay of the rollout and its compensation, per car
    DELAY_FIELDS = ("queue", "pred_pose", "pred_s", "now")

    def rollout_set_delay(self, delay, assumed=None, queue0=None):
        """The latency of the rollouts that follow (K3d / K3q; the law: csrc/delay_core.hpp): delay [B] ints in [0, 8] - the
        command a car's controller issues at step k reaches its wheels at step k + delay - or None for no delay (the default);
        assumed [B] ints in [0, 8]: the delay the controller compensates for by predicting its pose through the commands in
        flight (None: assumed = delay; zeros: no compensation); queue0 [B, 8, 2]: the commands (v, delta) in flight, queue0[:, i]
        issued i + 1 steps ago (None: zeros, the car stands for `delay` steps).  delay.Delay.arrays(B) gives all three.  The true
        pose stays rollout_state()["pose"]; wp_id and x0 are those of the predicted pose (rollout_delay()["pred_pose"]).  Not
        together with a lookahead.  May be called before rollout_init or between rollout_step calls; rollout_init zeroes the
        registers, so a resumed run sets the delay after it."""
        if delay is None:
            self._check(self.lib.mpmpc_rollout_set_delay(self._h, 0, None, None, None))
            return
        d = np.asarray(delay)
        a = d if assumed is None else np.asarray(assumed)
        if d.ndim != 1 or a.shape != d.shape:
            raise ValueError("delay and assumed must be [B]")
        for v in (d, a):
            if v.size and (not np.array_equal(v, np.floor(v)) or np.any(np.abs(v) > 2 ** 30)):
                raise ValueError("delay and assumed must be integers")
        d, a = (np.ascontiguousarray(v, dtype=np.int32) for v in (d, a))
        q = None if queue0 is None else np.ascontiguousarray(queue0, dtype=np.float64).reshape(d.size, 8, 2)
        self._check(self.lib.mpmpc_rollout_set_delay(self._h, d.size, _i(d), _i(a), _d(q)))

    def rollout_delay(self):
        """-> dict of the delay's per-car state: queue [B, 8, 2] the issued (v, delta), the newest first; pred_pose [B, 3] and
        pred_s [B] what the controller localised on in the last step; now [B, 3] = (e_y, e_psi, kappa) of the waypoint the car
        was at in the last step."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        out = dict(queue=np.zeros((B, 8, 2)), pred_pose=np.zeros((B, 3)), pred_s=np.zeros(B), now=np.zeros((B, 3)))
        self._check(self.lib.mpmpc_rollout_delay(self._h, B, _d(out["queue"]), _d(out["pred_pose"]), _d(out["pred_s"]), _d(out["now"])))
        return out

    # --- dynamic single-track plant of the rollout, per car
    DYNAMICS_FIELDS = ("state", "dyn_steps", "sat_front", "sat_rear", "slip_max", "alat_max")

    def rollout_set_dynamics(self, params, state0=None):
        """The dynamic plant of the rollouts that follow (K3y; the law: csrc/dynamics_core.hpp): params [B, 11] per car -
        dynamics.Dynamics.params(B): mass, inertia, lf, Cf, Cr, mu, speed_gain, a_drive, a_brake, v_dyn, substeps - or None for
        none (the default).  state0 [B, 3]: the (vx, vy, r) the cars start from (None: zeros).  Needs a plant in force for the
        same cars at the step (rollout_set_plant; plant.Plant() is the identity).  The controller keeps its kinematic model;
        everything that senses or judges the car keeps the true pose.  May be called before rollout_init or between
        rollout_step calls; rollout_init starts the state over, so a resumed run sets the dynamics after it."""
        if params is None:
            self._check(self.lib.mpmpc_rollout_set_dynamics(self._h, 0, None, None))
            return
        p = np.ascontiguousarray(params, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 11:
            raise ValueError("dynamics parameters must be [B, 11] (dynamics.Dynamics.params)")
        s0 = None if state0 is None else np.ascontiguousarray(state0, dtype=np.float64).reshape(p.shape[0], 3)
        self._check(self.lib.mpmpc_rollout_set_dynamics(self._h, p.shape[0], _d(p), _d(s0)))

    def rollout_dynamics(self):
        """-> dict of the dynamics' per-car state: state [B, 3] = (vx, vy, r) after the last driven step; dyn_steps / sat_front
        / sat_rear [B]: the driven steps that took the dynamic branch and those in which a sub-step clipped the front / rear
        axle; slip_max [B, 2]: max |front|, |rear| slip angle [rad]; alat_max [B]: max lateral acceleration [m/s^2]."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        state, counts, peaks = np.zeros((B, 3)), np.zeros((3, B), np.int32), np.zeros((3, B))
        self._check(self.lib.mpmpc_rollout_dynamics(self._h, B, _d(state), _i(counts), _d(peaks)))
        return _dynamics_dict(state, counts, peaks)

    # --- corridor commitment of the rollout, per car
    COMMITMENT_FIELDS = ("kept", "switched", "moved", "wp", "rows")

    def rollout_set_commitment(self, keep, memory=None):
        """The corridor commitment of the rollouts that follow (K0k; the law: csrc/commitment_core.hpp): keep [B] per car -
        commitment.Commitment.keep(B): 0 off, else the switch_ratio in [1, inf] - or None for none (the default).  A car that is
        on lets every waypoint that was in its horizon in the step before choose, among its free segments, the one nearest to
        what it chose then.  memory: None (empty) or (wp [B, N], rows [B, N, 6]) - rollout_commitment()'s of the run that is
        resumed.  Needs a per-car world in force for the same cars at the step (rollout_set_obstacles with empty lists will
        do); not together with rollout_set_lookahead.  May be called between rollout_step calls; rollout_init empties the
        memory, so a resumed run sets the commitment after it."""
        if keep is None:
            self._check(self.lib.mpmpc_rollout_set_commitment(self._h, 0, None, None, None))
            return
        k = np.ascontiguousarray(keep, dtype=np.float64).reshape(-1)
        wp = rows = None
        if memory is not None:
            wp = np.ascontiguousarray(memory[0], dtype=np.int32).reshape(k.size, self.cfg.N)
            rows = np.ascontiguousarray(memory[1], dtype=np.float64).reshape(k.size, self.cfg.N, 6)
        self._check(self.lib.mpmpc_rollout_set_commitment(self._h, k.size, _d(k), _i(wp), _d(rows)))

    def rollout_commitment(self):
        """-> dict of the commitment's per-car state: kept / switched / moved [B] - the columns decided from memory, those of
        them where the ratio left the nearest candidate, and the columns whose corridor jumped to a disjoint interval, summed
        over the steps since the setting or rollout_init; wp [B, N], rows [B, N, 6]: the memory the next step reads (wp -1: an
        empty entry)."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        N = self.cfg.N
        counts, wp, rows = np.zeros((3, B), np.int32), np.zeros((B, N), np.int32), np.zeros((B, N, 6))
        self._check(self.lib.mpmpc_rollout_commitment(self._h, B, _i(counts), _i(wp), _d(rows)))
        return dict(kept=counts[0], switched=counts[1], moved=counts[2], wp=wp, rows=rows)

    # --- pose estimator of the rollout, per car
    ESTIMATOR_FIELDS = ("est", "cov", "err2_max", "err2_sum", "meas2_sum", "head2_sum", "used", "steps")

    def rollout_set_estimator(self, params, seed=0, car0=0, step0=0, est0=None, cov0=None):
        """The pose filter of the rollouts that follow (K3e; the law: csrc/estimator_core.hpp): params [B, 8] = q_xy, q_psi
        (process variances per step, >= 0), r_xy, r_psi (measurement variances, > 0), p0_xy, p0_psi (the variances a car is
        primed with, >= 0), period (the measurement is scheduled when (k - step0) mod period == 0; an integer >= 1), drop in
        [0, 1) (the probability that a scheduled measurement is lost; a draw of (seed, car0 + car, k - step0)) - or None for no
        estimator (the default).  estimator.Estimator.params(B) gives the block.  Per step every running car's filter takes the
        nominal model's step with the command believed executed in the last step, then - if available - the measurement (the
        plant's measured pose, else the true one), and the controller localises on the ESTIMATE (under a delay: predicts from
        it); the true pose stays rollout_state()["pose"].  est0 [B, 3] and cov0 [B, 6] (Pxx, Pxy, Pxp, Pyy, Pyp, Ppp), both or
        neither: the cars start primed with them (a resumed run).  May be called before rollout_init or between rollout_step
        calls; rollout_init un-primes every car and zeroes the statistics, so a resumed run sets the estimator after it.  Not
        together with an assumed delay of 8."""
        if params is None:
            self._check(self.lib.mpmpc_rollout_set_estimator(self._h, 0, None, 0, 0, 0, None, None))
            return
        p = np.ascontiguousarray(params, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 8:
            raise ValueError("estimator params must be [B, 8]")
        B = p.shape[0]
        e0 = None if est0 is None else np.ascontiguousarray(est0, dtype=np.float64).reshape(B, 3)
        c0 = None if cov0 is None else np.ascontiguousarray(cov0, dtype=np.float64).reshape(B, 6)
        self._check(self.lib.mpmpc_rollout_set_estimator(self._h, B, _d(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(car0), int(step0),
                                                         _d(e0), _d(c0)))

    def rollout_estimator(self):
        """-> dict of the estimator's per-car state: est [B, 3] and cov [B, 6] (the upper triangle Pxx, Pxy, Pxp, Pyy, Pyp, Ppp)
        as the last step left them - est is what the controller localised on in that step; err2_max and err2_sum, maximum and
        sum over the car's steps of the squared position error of the estimate against the true pose; meas2_sum, the same sum
        for what was measured (every step, whether or not the filter saw it); head2_sum, the sum of the squared wrapped heading
        error of the estimate; used, the measurements taken (priming included); steps, the filter's steps."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        out = dict(est=np.zeros((B, 3)), cov=np.zeros((B, 6)), err2_max=np.zeros(B), err2_sum=np.zeros(B), meas2_sum=np.zeros(B),
                   head2_sum=np.zeros(B), used=np.zeros(B, np.int32), steps=np.zeros(B, np.int32))
        self._check(self.lib.mpmpc_rollout_estimator(self._h, B, _d(out["est"]), _d(out["cov"]), _d(out["err2_max"]), _d(out["err2_sum"]),
                                                     _d(out["meas2_sum"]), _d(out["head2_sum"]), _i(out["used"]), _i(out["steps"])))
        return out

    # --- lidar localisation of the rollout, per fleet
    LOCALISER_FIELDS = ("fix", "prior", "cand", "score", "hits", "ranges", "err2_max", "err2_sum", "head2_sum", "prior2_sum", "steps",
                        "matched", "lost", "edge")

    def rollout_set_localiser(self, B, angles=None, range_m=0.0, D=1, m=1, W=0, T=0, step_psi=0.0, min_hits=1, sigma_r=0.0, period=1,
                              seed=0, car0=0, step0=0, fix0=None):
        """The scan matcher of the rollouts that follow (K0d, K3l; the law: csrc/localiser_core.hpp), one setting for the B cars -
        or B = 0 / None for none (the default).  localiser.Localiser.setting() gives the keyword arguments.  Every step with
        (k - step0) mod period == 0 each running car scans its TRUE world (angles [n] ascending, range_m in metres) and matches
        the scan against the distance field of the BASE map (reach D cells, built by this call: needs set_map) around dead
        reckoning: headings t * step_psi, t in [-T, T], translations (a, c) * m cells, a, c in [-W, W]; fewer than min_hits hits
        and the car keeps dead reckoning; a hit's range takes sigma_r times a triangular variate of (seed, car0 + car,
        k - step0, beam).  The FIX is what the estimator measures and what the controller localises on (the estimate, else
        the fix); the true pose stays rollout_state()["pose"].  fix0 [B, 3]: the cars start primed with it (a resumed run).
        May be called before rollout_init or between rollout_step calls; rollout_init un-primes every car and zeroes the
        statistics.  After set_map / set_path / set_path_geometry it must be set again.  Not together with an assumed delay
        of 8."""
        if not B or angles is None:
            self._check(self.lib.mpmpc_rollout_set_localiser(self._h, 0, 0, None, 0.0, 0, 0, 0, 0, 0.0, 0, 0.0, 0, 0, 0, 0, None))
            self._lc_beams = 0
            return
        ang = np.ascontiguousarray(angles, dtype=np.float64).ravel()
        f0 = None if fix0 is None else np.ascontiguousarray(fix0, dtype=np.float64).reshape(int(B), 3)
        self._check(self.lib.mpmpc_rollout_set_localiser(self._h, int(B), ang.size, _d(ang), float(range_m), int(D), int(m), int(W), int(T),
                                                         float(step_psi), int(min_hits), float(sigma_r), int(period),
                                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(car0), int(step0), _d(f0)))
        self._lc_beams = ang.size

    def rollout_localiser(self):
        """-> dict of the localiser's per-car state: fix, prior [B, 3], cand, score, hits [B] as the car's last step left them
        (cand, the winner's index, and score: -1 on a step without a match; hits: -1 on a step without a scan); ranges
        [B, n_beams], the scans of the last scheduled step with the hits noisy; err2_max and err2_sum, maximum and sum over the
        car's steps of the squared position error of the fix against the true pose; head2_sum, the sum of its squared wrapped
        heading error; prior2_sum, err2_sum of the prior - dead reckoning alone; steps, matched, lost, edge: the counters."""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        n = int(getattr(self, "_lc_beams", 0))
        out = dict(fix=np.zeros((B, 3)), prior=np.zeros((B, 3)), cand=np.zeros(B, np.int32), score=np.zeros(B, np.int32),
                   hits=np.zeros(B, np.int32), ranges=np.zeros((B, n)), err2_max=np.zeros(B), err2_sum=np.zeros(B), head2_sum=np.zeros(B),
                   prior2_sum=np.zeros(B), steps=np.zeros(B, np.int32), matched=np.zeros(B, np.int32), lost=np.zeros(B, np.int32),
                   edge=np.zeros(B, np.int32))
        self._check(self.lib.mpmpc_rollout_localiser(self._h, B, _d(out["fix"]), _d(out["prior"]), _i(out["cand"]), _i(out["score"]),
                                                     _i(out["hits"]), _d(out["ranges"]) if out["ranges"].size else None, _d(out["err2_max"]),
                                                     _d(out["err2_sum"]), _d(out["head2_sum"]), _d(out["prior2_sum"]), _i(out["steps"]),
                                                     _i(out["matched"]), _i(out["lost"]), _i(out["edge"])))
        return out

    # --- footprint audit of the rollout: contact and clearance of every car, every step, accumulated on the device
    AUDIT_FIELDS = ("contact_steps", "first_contact", "min_clearance", "min_step", "last_contact", "last_clearance")

    def rollout_set_audit(self, mode, length=0.0, width=0.0, reach=0.0):
        """Audit the cars of the rollouts that follow (K0f; the law: csrc/footprint_core.hpp): every step tests the
        length x width rectangle of every running car, centred at the pose the step finds it at, against the car's world of
        that step (the resident map plus its static discs, movers and traffic slots).  mode 0 / None: off, 1: audit,
        2: audit, and a car in contact ends there with alive = -5.  reach [m]: clearances are exact up to it.  Needs
        set_map; the setting outlives rollout_init, the accumulators (rollout_audit) start over with it and with this call."""
        mode = int(mode or 0)
        self._check(self.lib.mpmpc_rollout_set_audit(self._h, mode, float(length), float(width), float(reach)))

    def rollout_audit(self):
        """-> dict of [B] arrays: contact_steps (audited steps with contact), first_contact (step index, -1: none),
        min_clearance (reach at the start), min_step (first step that reached it, -1: none came nearer than reach),
        last_contact, last_clearance (the verdict of the car's last audited step)"""
        B = int(getattr(self, "_ro_B", 0))      # (0 before the first rollout_init: the library refuses it)
        out = {k: np.zeros(B, np.float64 if k.endswith("clearance") else np.int32) for k in self.AUDIT_FIELDS}
        self._check(self.lib.mpmpc_rollout_audit(self._h, B, _i(out["contact_steps"]), _i(out["first_contact"]),
                                                 _d(out["min_clearance"]), _i(out["min_step"]), _i(out["last_contact"]),
                                                 _d(out["last_clearance"])))
        return out

    # --- recorder of the rollout: one record per car and recorded step, kept on the device
    TRACE_BASIC = ("s", "pose", "wp_id", "x0", "u", "status", "counter", "alive")

    def rollout_record(self, capacity, plan=False, prediction=False, rows=False, stride=1, B=None, plant=False, delay=False,
                       estimator=False, fix=False, scan=False, chain=False):
        """Record every `stride`-th step of the rollouts that follow into a device-resident trace of `capacity` records:
        always s, pose (the state the step started from), wp_id, x0, u, status, counter, alive; optionally the plan after
        the step, the predicted path (world x / y of stages 2 .. N-1, MPC.update_prediction) and the corridor row the QP
        used; and optionally the pose chain, each value the one the feature's getter would return right after the step:
        plant (act, meas), delay (queue, pred_pose, pred_s, now), estimator (est, cov, used), fix (fix, prior, cand, score,
        hits), scan (ranges: needs a localiser in force now, whose n_beams the records take); chain=True selects the first
        four.  capacity = 0 switches recording off and frees the memory.  B: cars per record (default: the rollout's, so
        before the first rollout_init it must be given).  A rollout_step that would overflow the trace raises and does
        nothing; rollout_init keeps the configuration and empties the trace."""
        B = int(B if B is not None else getattr(self, "_ro_B", 0))
        if B < 1:
            raise ValueError("rollout_record before rollout_init needs B")
        fields = (REC_PLAN if plan else 0) | (REC_PRED if prediction else 0) | (REC_ROWS if rows else 0) | \
            (REC_PLANT if plant or chain else 0) | (REC_DELAY if delay or chain else 0) | (REC_EST if estimator or chain else 0) | \
            (REC_FIX if fix or chain else 0) | (REC_SCAN if scan else 0)
        self._check(self.lib.mpmpc_rollout_record(self._h, B, int(capacity), fields, int(stride)))
        self._rec = (B, fields, int(getattr(self, "_lc_beams", 0)) if fields & REC_SCAN else 0) if capacity else None

    def rollout_recorded(self):
        """-> (records held, rollout steps taken since rollout_init)"""
        n, k = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.mpmpc_rollout_recorded(self._h, C.byref(n), C.byref(k)))
        return n.value, k.value

    # the pose chain's fields by the bit that records them, in mpmpc_rollout_trace_chain's order
    TRACE_CHAIN = ((REC_PLANT, ("act", "meas")), (REC_DELAY, ("queue", "pred_pose", "pred_s", "now")), (REC_EST, ("est", "cov", "used")),
                   (REC_FIX, ("fix", "prior", "cand", "score", "hits")), (REC_SCAN, ("ranges",)))

    def rollout_trace(self, first=0, count=None, fields=None):
        """Records first .. first + count - 1 (default: all from `first`) -> dict of arrays [count, B, ...]: s, pose [.., 3],
        wp_id, x0 [.., 3], u [.., 2], status, counter, alive, and - where recorded - plan [.., 2N], pred_x / pred_y [.., N-2],
        ub / lb [.., N], and the pose chain: act [.., 2], meas [.., 3], queue [.., 8, 2], pred_pose [.., 3], pred_s, now [.., 3],
        est [.., 3], cov [.., 6], used, fix / prior [.., 3], cand, score, hits, ranges [.., n_beams].  fields: names to fetch
        (default: everything recorded; asking for one that was not raises).  Entries a step did not produce for a car are
        empty - NaN, wp_id -1, status 0, cand / score / hits -2, used -1 (include/mpmpc.h has the tables)."""
        if getattr(self, "_rec", None) is None:
            raise MpmpcError("mpmpc error -3: recording is off (rollout_record)")
        B, rec, n_beams = self._rec
        N = self.N
        if count is None:
            count = self.rollout_recorded()[0] - int(first)
        count = int(count)
        names = list(self.TRACE_BASIC) + (["plan"] if rec & REC_PLAN else []) + (["pred_x", "pred_y"] if rec & REC_PRED else []) + \
            (["ub", "lb"] if rec & REC_ROWS else []) + [k for bit, group in self.TRACE_CHAIN if rec & bit for k in group]
        if fields is not None:
            names = list(fields)
        shape = dict(s=(), pose=(3,), wp_id=(), x0=(3,), u=(2,), status=(), counter=(), alive=(), plan=(2 * N,),
                     pred_x=(N - 2,), pred_y=(N - 2,), ub=(N,), lb=(N,))
        chain = dict(act=(2,), meas=(3,), queue=(8, 2), pred_pose=(3,), pred_s=(), now=(3,), est=(3,), cov=(6,), used=(),
                     fix=(3,), prior=(3,), cand=(), score=(), hits=(), ranges=(n_beams,))
        ints = ("wp_id", "status", "counter", "alive", "used", "cand", "score", "hits")
        for k in names:
            if k not in shape and k not in chain:
                raise ValueError("unknown trace field %r" % (k,))
        out = {k: np.zeros((max(count, 0), B) + (shape[k] if k in shape else chain[k]), np.int32 if k in ints else np.float64) for k in names}
        a = {k: (_i(out[k]) if k in ints else _d(out[k])) if k in out else None for k in list(shape) + list(chain)}
        if any(k in shape for k in names) or not names:
            self._check(self.lib.mpmpc_rollout_trace(self._h, B, int(first), count, a["s"], a["pose"], a["wp_id"], a["x0"], a["u"],
                                                     a["status"], a["counter"], a["alive"], a["plan"], a["pred_x"], a["pred_y"],
                                                     a["ub"], a["lb"]))
        if any(k in chain for k in names):
            if "ranges" in out and not (rec & REC_SCAN):      # (no beams to size the array by: the library's own refusal)
                raise MpmpcError("mpmpc error -3: a field was asked for that mpmpc_rollout_record did not select")
            self._check(self.lib.mpmpc_rollout_trace_chain(self._h, B, int(first), count, a["act"], a["meas"], a["queue"], a["pred_pose"],
                                                           a["pred_s"], a["now"], a["est"], a["cov"], a["used"], a["fix"], a["prior"],
                                                           a["cand"], a["score"], a["hits"], a["ranges"]))
        return out

    def _inputs(self, wp_id, x0, cc_prev, lb, ub):
        wp = np.ascontiguousarray(wp_id, dtype=np.int32).ravel()
        B = wp.size
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(B, 3)
        cc = np.ascontiguousarray(cc_prev, dtype=np.float64).reshape(B, 2 * self.N)
        if (lb is None) != (ub is None):
            raise ValueError("lb and ub must both be given or both be None")
        if lb is not None:
            lb = np.ascontiguousarray(lb, dtype=np.float64).reshape(B, self.N)
            ub = np.ascontiguousarray(ub, dtype=np.float64).reshape(B, self.N)
        elif not self._have_table:
            raise ValueError("no per-instance corridor given and no corridor table set")
        return B, wp, x0, cc, lb, ub

    def assemble(self, wp_id, x0, cc_prev, lb=None, ub=None):
        """Stage-blocked QP [NUM_FIELDS, B, LD] as K1 leaves it in HBM."""
        B, wp, x0, cc, lb, ub = self._inputs(wp_id, x0, cc_prev, lb, ub)
        qp = np.zeros((NUM_FIELDS, B, stage_ld(self.N)))
        self._check(self.lib.mpmpc_assemble(self._h, B, _i(wp), _d(x0), _d(cc), _d(lb), _d(ub), _d(qp)))
        return qp

    def _outputs(self, B, want_y):
        return (np.zeros((B, self.n)), np.zeros((B, 2)), np.zeros(B, np.int32), np.zeros((B, 2), np.int32),
                np.zeros((B, 2)), np.zeros((B, self.m)) if want_y else None)

    def solve(self, wp_id, x0, cc_prev, lb=None, ub=None, want_y=False) -> Solution:
        B, wp, x0, cc, lb, ub = self._inputs(wp_id, x0, cc_prev, lb, ub)
        z, u0, st, it, rs, y = self._outputs(B, want_y)
        self._check(self.lib.mpmpc_solve(self._h, B, _i(wp), _d(x0), _d(cc), _d(lb), _d(ub), _d(z), _d(u0),
                                         _i(st), _i(it), _d(rs), _d(y)))
        return Solution(z, u0, st, it, rs, y)

    # --- zero-copy host form: numpy views of the handle's page-locked staging blocks
    def staging(self, B):
        """-> dict of numpy views (wp_id [B], x0 [B,3], cc_prev [B,2N], lb / ub [B,N]; z [B,n], u0 [B,2], status [B], iters [B,2],
        resid [B,2], y [B,m]) laid out for a batch of B: fill the inputs in place, call solve_staged(B), read the outputs."""
        N = self.cfg.N
        pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        wp, st, it = pi(), pi(), pi()
        x0, cc, lb, ub, z, u0, rs, y = (pd() for _ in range(8))
        self._check(self.lib.mpmpc_staging(self._h, B, C.byref(wp), C.byref(x0), C.byref(cc), C.byref(lb), C.byref(ub), C.byref(z),
                                           C.byref(u0), C.byref(st), C.byref(it), C.byref(rs), C.byref(y)))
        def view(p, shape):
            # (the views point into the handle's page-locked blocks: they keep the Handle alive - its close() / __del__ frees them)
            v = np.ctypeslib.as_array(p, shape=shape).view(_StagingView)
            v._owner = self
            return v
        return dict(wp_id=view(wp, (B,)), x0=view(x0, (B, 3)), cc_prev=view(cc, (B, 2 * N)), lb=view(lb, (B, N)), ub=view(ub, (B, N)),
                    z=view(z, (B, self.n)), u0=view(u0, (B, 2)), status=view(st, (B,)), iters=view(it, (B, 2)), resid=view(rs, (B, 2)),
                    y=view(y, (B, self.m)))

    def solve_staged(self, B, with_rows=True, want_z=True, want_y=False):
        self._check(self.lib.mpmpc_solve_staged(self._h, B, int(with_rows), int(want_z), int(want_y)))

    def staged_begin(self, B, with_rows=True, want_z=True, want_y=False):
        """solve_staged in two halves (a loop that keeps several handles busy): enqueue, return; staged_end() waits."""
        self._check(self.lib.mpmpc_staged_begin(self._h, B, int(with_rows), int(want_z), int(want_y)))

    def staged_end(self):
        self._check(self.lib.mpmpc_staged_end(self._h))

    # --- resident (benchmark / closed loop) form
    def upload(self, wp_id, x0, cc_prev, lb=None, ub=None):
        B, wp, x0, cc, lb, ub = self._inputs(wp_id, x0, cc_prev, lb, ub)
        self._check(self.lib.mpmpc_upload(self._h, B, _i(wp), _d(x0), _d(cc), _d(lb), _d(ub)))
        return B

    def solve_resident(self, B):
        self._check(self.lib.mpmpc_solve_resident(self._h, B))

    def set_outputs(self, want_y=True):
        """resident launches store the multipliers y (default) or skip them (46 % of the output bytes)"""
        self._check(self.lib.mpmpc_set_outputs(self._h, int(bool(want_y))))

    def set_pipeline(self, depth=3):
        """resident launches in flight, 1 .. 8: 3 (default) = pipelined inside the handle (launch k + 1, k + 2 run beside
        launch k), 1 = one stream, one output block.  Every launch in flight has a stream of its own and streams that share a
        hardware queue take turns, so the handle uses s = min(depth, GPU_MAX_HW_QUEUES of this process; 4 if unset) launch
        slots (mpmpc_pipeline_streams): results of launch k stay untouched until launch k + s.  The library reads the variable,
        never sets it, and keeps off the null stream, so depth 4 runs four launches side by side on the runtime's default"""
        self._check(self.lib.mpmpc_set_pipeline(self._h, int(depth)))

    def sync(self):
        self._check(self.lib.mpmpc_sync(self._h))

    def download(self, B, want_y=False) -> Solution:
        z, u0, st, it, rs, y = self._outputs(B, want_y)
        self._check(self.lib.mpmpc_download(self._h, B, _d(z), _d(u0), _i(st), _i(it), _d(rs), _d(y)))
        return Solution(z, u0, st, it, rs, y)

    def solve_resident_timed(self, B):
        a, s = C.c_float(), C.c_float()
        self._check(self.lib.mpmpc_solve_resident_timed(self._h, B, C.byref(a), C.byref(s)))
        return a.value, s.value

    def solve_resident_profile(self, B, n):
        """n resident launches as solve_resident issues them (double-buffered), HIP events around each on its own stream
        -> (durations [n] in ms, span from the first start to the last end in ms)"""
        each = np.zeros(n, np.float32)
        span = C.c_float()
        self._check(self.lib.mpmpc_solve_resident_profile(self._h, B, n, each.ctypes.data_as(C.POINTER(C.c_float)), C.byref(span)))
        return each.astype(float), span.value

    def assemble_timed(self, B, n):
        """n launches of the stand-alone assembly kernel K1 back to back, HIP events around each -> durations [n] in ms"""
        each = np.zeros(n, np.float32)
        self._check(self.lib.mpmpc_assemble_resident_timed(self._h, B, n, each.ctypes.data_as(C.POINTER(C.c_float))))
        return each.astype(float)


def device_count() -> int:
    n = C.c_int32(0)
    rc = load_library().mpmpc_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def speed_profile(li, kappa, limits, eps=1e-12, device=0):
    """Speed profiles of B paths on the device (K4, replaces compute_speed_profile's OSQP call,
    src/reference_path.py:289-354).  li, kappa [B, n] (or [n]); limits [B, 5] (or [5]) =
    (a_min, a_max, v_min, v_max, ay_max).  -> (v [B, n], status [B], iters [B])."""
    lib = load_library()
    li = np.atleast_2d(np.ascontiguousarray(li, float))
    kappa = np.atleast_2d(np.ascontiguousarray(kappa, float))
    B, n = li.shape
    if kappa.shape != (B, n):
        raise ValueError("li and kappa must have the same shape")
    limits = np.ascontiguousarray(np.broadcast_to(np.atleast_2d(np.asarray(limits, float)), (B, 5)))
    v = np.zeros((B, n))
    status, iters = np.zeros(B, np.int32), np.zeros(B, np.int32)
    rc = lib.mpmpc_speed_profile(device, B, n, _d(li), _d(kappa), _d(limits), float(eps), _d(v), _i(status), _i(iters))
    if rc != 0:
        raise MpmpcError("mpmpc_speed_profile: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    return v, status, iters


def plant_noise(seed, car0, B, j0, n_steps, device=0):
    """The plant's draws (csrc/plant_core.hpp) of cars car0 .. car0 + B - 1 at j = j0 .. j0 + n_steps - 1, computed on the
    device -> float64 [n_steps, B, 5] = (n_v, n_delta, n_x, n_y, n_psi).  plant.Plant.noise is the numpy evaluation."""
    lib = load_library()
    out = np.zeros((int(n_steps), int(B), 5))
    rc = lib.mpmpc_plant_noise(device, int(seed) & 0xFFFFFFFFFFFFFFFF, int(car0), int(B), int(j0), int(n_steps),
                               _d(out) if out.size else _d(np.zeros(1)))
    if rc != 0:
        raise MpmpcError("mpmpc_plant_noise: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    return out


def _dynamics_dict(state, counts, peaks):
    return dict(state=state, dyn_steps=counts[0].copy(), sat_front=counts[1].copy(), sat_rear=counts[2].copy(),
                slip_max=np.ascontiguousarray(peaks[:2].T), alat_max=peaks[2].copy())


def dynamics_drive(params, cmds, length, Ts, state0=None, pose0=None, trace=False, device=0):
    """The dynamic plant open loop on the device (csrc/dynamics_core.hpp, steps 2 - 4): params [B, 11]
    (dynamics.Dynamics.params), cmds [n_steps, B, 2] = (v_act, d_act) what the actuators do at every step, length the wheelbase,
    state0 [B, 3] / pose0 [B, 3] (None: zeros) -> dict(state, pose, dyn_steps, sat_front, sat_rear, slip_max, alat_max) after the
    last step and - trace - "trace" [n_steps, B, 3], the pose after every step.  dynamics.Dynamics.step is the host evaluation."""
    lib = load_library()
    p = np.ascontiguousarray(params, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 11:
        raise ValueError("dynamics parameters must be [B, 11] (dynamics.Dynamics.params)")
    B = p.shape[0]
    c = np.ascontiguousarray(cmds, dtype=np.float64)
    if c.ndim != 3 or c.shape[1:] != (B, 2):
        raise ValueError("cmds must be [n_steps, B, 2]")
    n = c.shape[0]
    s0 = None if state0 is None else np.ascontiguousarray(state0, dtype=np.float64).reshape(B, 3)
    p0 = np.zeros((B, 3)) if pose0 is None else np.ascontiguousarray(pose0, dtype=np.float64).reshape(B, 3)
    state, pose, counts, peaks = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((3, B), np.int32), np.zeros((3, B))
    tr = np.zeros((n, B, 3)) if trace else None
    rc = lib.mpmpc_dynamics_drive(int(device), B, n, float(length), float(Ts), _d(p), _d(s0), _d(p0), _d(c) if c.size else _d(np.zeros(2)),
                                  _d(state), _d(pose), _i(counts), _d(peaks), _d(tr) if trace and tr.size else None)
    if rc != 0:
        raise MpmpcError("mpmpc_dynamics_drive: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    out = _dynamics_dict(state, counts, peaks)
    out["pose"] = pose
    if trace:
        out["trace"] = tr
    return out


def distance_field(grid, D, device=0):
    """The capped squared-distance field of a grid on the device (K0d; the law: csrc/localiser_core.hpp): grid [H, W] int8 (1 free /
    0 occupied), D in [1, 15] cells -> uint8 [H, W], min(D^2 + 1, the smallest squared cell distance <= D^2 to an occupied cell).
    localiser.Localiser.field is the numpy evaluation."""
    lib = load_library()
    grid = np.ascontiguousarray(grid, dtype=np.int8)
    if grid.ndim != 2:
        raise ValueError("map grid must be 2-D [height, width]")
    out = np.zeros(grid.shape, np.uint8)
    rc = lib.mpmpc_distance_field(int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)), int(D),
                                  out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise MpmpcError("mpmpc_distance_field: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    return out


def scan_match(grid, origin, resolution, priors, ranges, angles, range_m, D, m, W, T, step_psi, min_hits=1, device=0):
    """Scan matching of B (prior, scan) pairs on the device (K0d, then K3l's match; the law: csrc/localiser_core.hpp, steps 3 -
    the hits, no noise - and 4): grid [H, W] int8 with its origin and resolution, priors [B, 3], ranges [B, n] of the beams
    angles [n] (ascending) with range_m -> dict(fix [B, 3], score, cand, hits [B]); cand = score = -1 and fix = prior where there
    is no match.  localiser.Localiser.match is the numpy evaluation."""
    lib = load_library()
    grid = np.ascontiguousarray(grid, dtype=np.int8)
    if grid.ndim != 2:
        raise ValueError("map grid must be 2-D [height, width]")
    priors = np.ascontiguousarray(priors, dtype=np.float64).reshape(-1, 3)
    ang = np.ascontiguousarray(angles, dtype=np.float64).ravel()
    B = priors.shape[0]
    rg = np.ascontiguousarray(ranges, dtype=np.float64).reshape(B, ang.size)
    out = dict(fix=np.zeros((B, 3)), score=np.zeros(B, np.int32), cand=np.zeros(B, np.int32), hits=np.zeros(B, np.int32))
    rc = lib.mpmpc_scan_match(int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)), float(origin[0]),
                              float(origin[1]), float(resolution), B, _d(priors), _d(rg), ang.size, _d(ang), float(range_m), int(D),
                              int(m), int(W), int(T), float(step_psi), int(min_hits), _d(out["fix"]), _i(out["score"]), _i(out["cand"]),
                              _i(out["hits"]))
    if rc != 0:
        raise MpmpcError("mpmpc_scan_match: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    return out


def _wall_csr(walls, B=None):
    """one int [k_b, 4] array per car -> (offsets [B + 1], walls [n, 4]) as the C ABI takes them"""
    lists = [np.asarray(w, dtype=np.int32).reshape(-1, 4) for w in walls]
    if B is not None and len(lists) != B:
        raise ValueError("walls must hold one list per car")
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([a.shape[0] for a in lists])
    flat = np.ascontiguousarray(np.concatenate(lists) if off[-1] else np.zeros((0, 4), np.int32), dtype=np.int32)
    return off, flat


def world_grid(grid, origin, resolution, discs=None, walls=None, device=0):
    """ONE car's world as a grid (K-world): grid [H, W] int8 (1 free / 0 occupied) with discs [k, 3] (Map.obstacle_discs) and
    walls [k, 4] (Map.boundary_walls) stamped in by the predicate every kernel uses -> int8 [H, W]; what Map.add_obstacles
    and Map.add_boundary leave in Map.data."""
    lib = load_library()
    grid = np.ascontiguousarray(grid, dtype=np.int8)
    if grid.ndim != 2:
        raise ValueError("map grid must be 2-D [height, width]")
    d = np.ascontiguousarray(np.asarray(discs if discs is not None else [], dtype=np.int32).reshape(-1, 3))
    w = np.ascontiguousarray(np.asarray(walls if walls is not None else [], dtype=np.int32).reshape(-1, 4))
    out = np.zeros_like(grid)
    rc = lib.mpmpc_world_grid(int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)), float(origin[0]),
                              float(origin[1]), float(resolution), d.shape[0], _i(d) if d.size else None, w.shape[0],
                              _i(w) if w.size else None, out.ctypes.data_as(C.POINTER(C.c_int8)))
    if rc != 0:
        raise MpmpcError("mpmpc_world_grid: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    return out


def lidar_scan(grid, origin, resolution, poses, angles, range_m, discs=None, device=0, walls=None):
    """Lidar scans of B cars on the device (K0l, replaces LidarModel.scan's loops, src/lidar_model.py:37-112; the law:
    csrc/lidar_core.hpp).  grid [H, W] int8 (1 free / 0 occupied) with its origin and resolution, poses [B, 3] = x, y, psi,
    angles [n] ascending, range_m in metres, discs: one int [k_b, 3] array of (cx, cy, r) map cells per car
    (Map.obstacle_discs; at most 64) or None.  -> ranges [B, n]."""
    lib = load_library()
    grid = np.ascontiguousarray(grid, dtype=np.int8)
    if grid.ndim != 2:
        raise ValueError("map grid must be 2-D [height, width]")
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    ang = np.ascontiguousarray(angles, dtype=np.float64).ravel()
    B = poses.shape[0]
    off = flat = None
    if discs is not None:
        lists = [np.asarray(d, dtype=np.int32).reshape(-1, 3) for d in discs]
        if len(lists) != B:
            raise ValueError("discs must hold one list per car")
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in lists])
        flat = np.ascontiguousarray(np.concatenate(lists) if off[-1] else np.zeros((0, 3), np.int32), dtype=np.int32)
    out = np.zeros((B, ang.size))
    if walls is not None:
        woff, wflat = _wall_csr(walls, B)
        rc = lib.mpmpc_lidar_scan_world(int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)),
                                        float(origin[0]), float(origin[1]), float(resolution), B, _d(poses), _i(off),
                                        _i(flat) if flat is not None and flat.size else None, _i(woff),
                                        _i(wflat) if wflat.size else None, ang.size, _d(ang), float(range_m), _d(out))
        if rc != 0:
            raise MpmpcError("mpmpc_lidar_scan_world: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
        return out
    rc = lib.mpmpc_lidar_scan(int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)),
                              float(origin[0]), float(origin[1]), float(resolution), B, _d(poses), _i(off),
                              _i(flat) if flat is not None and flat.size else None, ang.size, _d(ang), float(range_m), _d(out))
    if rc != 0:
        raise MpmpcError("mpmpc_lidar_scan: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    return out


def path_count(route, path_resolution, smoothing_distance):
    """The number of waypoints ReferencePath would give a route of corner points [k, 2] (host only, mpmpc_path_count);
    1 or less: there is no path."""
    lib = load_library()
    c = np.ascontiguousarray(route, dtype=np.float64).reshape(-1, 2)
    n = lib.mpmpc_path_count(c.shape[0], _d(c), float(path_resolution), int(smoothing_distance))
    if n < 0:
        raise MpmpcError("mpmpc_path_count: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), n))
    return n


def path_build(grid, origin, resolution, routes, path_resolution, smoothing_distance, max_width, circular=True, discs=None,
               walls=None, device=0, timings=None):
    """Reference paths of P routes on the device (K0p, replaces ReferencePath.__init__, src/reference_path.py:110-287; the
    law: csrc/path_core.hpp).  grid [H, W] int8 (1 free / 0 occupied) with its origin and resolution; routes: a list of [k, 2]
    arrays of corner points; path_resolution, smoothing_distance, max_width, circular: scalars or one value per route;
    discs / walls: one int [k_p, 3] / [k_p, 4] array per route (Map.obstacle_discs / Map.boundary_walls) or None for the
    base map.  The rows per path are sized by mpmpc_path_count.  timings: a list that receives the call's (host, wall
    rasterisation, width kernel) milliseconds.
    -> one dict per route: n_wp, status (0 built, 1 built but probed outside the grid, -1 fewer than 2 waypoints), x, y, psi,
    kappa, ds_next, ub, lb [n_wp], border_ub, border_lb [n_wp, 2], length (empty / NaN for status < 0)."""
    lib = load_library()
    grid = np.ascontiguousarray(grid, dtype=np.int8)
    if grid.ndim != 2:
        raise ValueError("map grid must be 2-D [height, width]")
    lists = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 2) for r in routes]
    P = len(lists)
    if P < 1:
        raise ValueError("routes must hold at least one route")
    coff = np.zeros(P + 1, np.int32)
    coff[1:] = np.cumsum([a.shape[0] for a in lists])
    corners = np.ascontiguousarray(np.concatenate(lists))
    spec = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(path_resolution, float), (P,)),
                                          np.broadcast_to(np.asarray(max_width, float), (P,))], 1))
    ispec = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(smoothing_distance), (P,)),
                                           np.broadcast_to(np.asarray(circular), (P,))], 1).astype(np.int32))
    cap = 1
    for p in range(P):
        n = lib.mpmpc_path_count(lists[p].shape[0], _d(lists[p]), float(spec[p, 0]), int(ispec[p, 0]))
        if n < 0:
            raise MpmpcError("mpmpc_path_count: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), n))
        cap = max(cap, int(n))
    doff = dflat = woff = wflat = None
    if discs is not None:
        dl = [np.asarray(d, dtype=np.int32).reshape(-1, 3) for d in discs]
        if len(dl) != P:
            raise ValueError("discs must hold one list per route")
        doff = np.zeros(P + 1, np.int32)
        doff[1:] = np.cumsum([a.shape[0] for a in dl])
        dflat = np.ascontiguousarray(np.concatenate(dl) if doff[-1] else np.zeros((0, 3), np.int32), dtype=np.int32)
    if walls is not None:
        woff, wflat = _wall_csr(walls, P)
    n_wp, status = np.zeros(P, np.int32), np.zeros(P, np.int32)
    tab = {k: np.zeros((P, cap)) for k in ("x", "y", "psi", "kappa", "ds_next", "ub", "lb")}
    border, length = np.zeros((P, cap, 4)), np.zeros(P)
    args = [int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)), float(origin[0]), float(origin[1]),
            float(resolution), P, _i(coff), _d(corners), _d(spec), _i(ispec), _i(doff),
            _i(dflat) if dflat is not None and dflat.size else None, _i(woff), _i(wflat) if wflat is not None and wflat.size else None,
            cap, _i(n_wp), _i(status)] + [_d(tab[k]) for k in ("x", "y", "psi", "kappa", "ds_next", "ub", "lb")] + [_d(border), _d(length)]
    if timings is None:
        rc = lib.mpmpc_path_build(*args)
    else:
        ms = (C.c_float * 3)()
        rc = lib.mpmpc_path_build_timed(*args, ms)
        timings[:] = [float(v) for v in ms]
    if rc != 0:
        raise MpmpcError("mpmpc_path_build: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    out = []
    for p in range(P):
        n = int(n_wp[p]) if status[p] >= 0 else 0
        rec = {k: v[p, :n].copy() for k, v in tab.items()}
        rec.update(n_wp=int(n_wp[p]), status=int(status[p]), border_ub=border[p, :n, :2].copy(), border_lb=border[p, :n, 2:].copy(),
                   length=float(length[p]))
        out.append(rec)
    return out


def concat_routes(routes):
    """The tables of several routes laid end to end, for a handle with routes (Handle.set_routes).  routes: one dict of
    per-waypoint arrays per route - what path_build returns, or any dict with at least kappa - or the
    (kappa, v_ref, ds_next) tuple of ReferencePath.tables().  -> (tables, first): every key that all routes hold as
    an array with one row per waypoint, concatenated in route order, and first [P + 1], the row each route starts at.
    `cum_lengths` is re-based so that each route's starts at 0; everything else is copied as it is."""
    routes = [dict(zip(("kappa", "v_ref", "ds_next"), r)) if isinstance(r, (tuple, list)) else r for r in routes]
    if not routes:
        raise ValueError("concat_routes needs at least one route")
    n = [int(np.asarray(r["kappa"]).shape[0]) for r in routes]
    first = np.zeros(len(routes) + 1, np.int32)
    first[1:] = np.cumsum(n)
    tables = {}
    for key in routes[0]:
        parts = [np.asarray(r[key]) if key in r else None for r in routes]
        if any(a is None or a.ndim < 1 or a.shape[0] != k for a, k in zip(parts, n)):
            continue
        if key == "cum_lengths":
            parts = [np.asarray(a, float) - float(a[0]) for a in parts]
        tables[key] = np.ascontiguousarray(np.concatenate(parts))
    return tables, first


def check_routes(n_wp, first, circular):
    """The argument checks of Handle.set_routes on their own (no handle, no device): raises MpmpcError as it would."""
    lib = load_library()
    f = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
    c = np.ascontiguousarray(circular, dtype=np.int32).reshape(-1)
    if f.size != c.size + 1:
        raise ValueError("first needs one entry more than circular")
    rc = lib.mpmpc_check_routes(int(n_wp), c.size, _i(f), _i(c) if c.size else None)
    if rc != 0:
        raise MpmpcError("mpmpc error %d: %s" % (rc, lib.mpmpc_last_error().decode()))


def project(x, y, psi, cum, poses, first=None, cand=None, max_heading=np.pi, device=0):
    """Where are B world poses on routes (mpmpc_project_kernel; the law: csrc/project_core.hpp, include/mpmpc.h)?  x, y, psi,
    cum: the waypoints' tables, cum every route's own cumulative length from 0 (concat_routes re-bases it); first [P + 1]: the
    routes' first rows (None: one route); poses [B, 3]; cand [B, K]: the candidate routes of every pose (None: every route);
    a waypoint counts when the pose's heading differs from its by at most max_heading.
    -> dict(wp [B, K] local to the route, -1: none; dist [B, K]; x0 [B, K, 3] = (e_y, e_psi, 0); s [B, K] = cum at wp)."""
    lib = load_library()
    x, y, psi, cum = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (x, y, psi, cum))
    if not (x.size == y.size == psi.size == cum.size):
        raise ValueError("x, y, psi and cum must have equal length")
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    B = poses.shape[0]
    f = None if first is None else np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
    P = 0 if f is None else f.size - 1
    if cand is None:
        c, K = None, max(P, 1)
    else:
        c = np.ascontiguousarray(cand, dtype=np.int32).reshape(B, -1)
        K = c.shape[1]
    out = dict(wp=np.zeros((B, K), np.int32), dist=np.zeros((B, K)), x0=np.zeros((B, K, 3)), s=np.zeros((B, K)))
    rc = lib.mpmpc_project(int(device), x.size, _d(x), _d(y), _d(psi), _d(cum), P, _i(f), B, _d(poses), K, _i(c), float(max_heading),
                           _i(out["wp"]), _d(out["dist"]), _d(out["x0"]), _d(out["s"]))
    if rc != 0:
        raise MpmpcError("mpmpc error %d: %s" % (rc, lib.mpmpc_last_error().decode()))
    return out


def perception_scan(grid, origin, resolution, poses, angles, range_m, discs=None, walls=None, device=0):
    """Lidar scans of B cars and WHAT THEY SAW (K0s; the law: csrc/perception_core.hpp): the arguments of lidar_scan ->
    (ranges [B, n] - lidar_scan's bit for bit -, disc_seen [B] uint64, wall_seen [B] uint32): bit q is set iff disc / wall q of
    the car's list occupies a nearest hit cell of some beam."""
    lib = load_library()
    grid = np.ascontiguousarray(grid, dtype=np.int8)
    if grid.ndim != 2:
        raise ValueError("map grid must be 2-D [height, width]")
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    ang = np.ascontiguousarray(angles, dtype=np.float64).ravel()
    B = poses.shape[0]
    off = flat = woff = wflat = None
    if discs is not None:
        lists = [np.asarray(d, dtype=np.int32).reshape(-1, 3) for d in discs]
        if len(lists) != B:
            raise ValueError("discs must hold one list per car")
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in lists])
        flat = np.ascontiguousarray(np.concatenate(lists) if off[-1] else np.zeros((0, 3), np.int32), dtype=np.int32)
    if walls is not None:
        woff, wflat = _wall_csr(walls, B)
    out, dseen, wseen = np.zeros((B, ang.size)), np.zeros(B, np.uint64), np.zeros(B, np.uint32)
    rc = lib.mpmpc_perception_scan(int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)),
                                   float(origin[0]), float(origin[1]), float(resolution), B, _d(poses), _i(off),
                                   _i(flat) if flat is not None and flat.size else None, _i(woff),
                                   _i(wflat) if wflat is not None and wflat.size else None, ang.size, _d(ang), float(range_m),
                                   _d(out), dseen.ctypes.data_as(C.POINTER(C.c_uint64)), wseen.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != 0:
        raise MpmpcError("mpmpc_perception_scan: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    return out, dseen, wseen


def footprint_audit(grid, origin, resolution, poses, length, width, reach, discs=None, device=0, walls=None):
    """Contact and clearance of B cars on the device (K0f; the law: csrc/footprint_core.hpp): the length x width rectangle of
    each car, centred at its pose, against its own world.  grid [H, W] int8 (1 free / 0 occupied) with its origin and
    resolution, poses [B, 3] = x, y, psi, reach in metres, discs: one int [k_b, 3] array of (cx, cy, r) map cells per car
    (Map.obstacle_discs; at most 64) or None for the base map.  -> (contact [B] int32, clearance [B]): clearance is the exact
    distance of the nearest occupied cell centre from the rectangle, capped at reach; NaN for a pose that is not finite."""
    lib = load_library()
    grid = np.ascontiguousarray(grid, dtype=np.int8)
    if grid.ndim != 2:
        raise ValueError("map grid must be 2-D [height, width]")
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    B = poses.shape[0]
    off = flat = None
    if discs is not None:
        lists = [np.asarray(d, dtype=np.int32).reshape(-1, 3) for d in discs]
        if len(lists) != B:
            raise ValueError("discs must hold one list per car")
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in lists])
        flat = np.ascontiguousarray(np.concatenate(lists) if off[-1] else np.zeros((0, 3), np.int32), dtype=np.int32)
    contact, clearance = np.zeros(B, np.int32), np.zeros(B)
    if walls is not None:
        woff, wflat = _wall_csr(walls, B)
        rc = lib.mpmpc_footprint_audit_world(int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)),
                                             float(origin[0]), float(origin[1]), float(resolution), B, _d(poses), _i(off),
                                             _i(flat) if flat is not None and flat.size else None, _i(woff),
                                             _i(wflat) if wflat.size else None, float(length), float(width), float(reach),
                                             _i(contact), _d(clearance))
        if rc != 0:
            raise MpmpcError("mpmpc_footprint_audit_world: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
        return contact, clearance
    rc = lib.mpmpc_footprint_audit(int(device), grid.shape[0], grid.shape[1], grid.ctypes.data_as(C.POINTER(C.c_int8)),
                                   float(origin[0]), float(origin[1]), float(resolution), B, _d(poses), _i(off),
                                   _i(flat) if flat is not None and flat.size else None, float(length), float(width),
                                   float(reach), _i(contact), _d(clearance))
    if rc != 0:
        raise MpmpcError("mpmpc_footprint_audit: %s (rc=%d)" % (lib.mpmpc_last_error().decode(), rc))
    return contact, clearance
