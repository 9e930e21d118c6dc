"""ctypes binding of lib/libtmpc_hip.so (C ABI: include/tmpc.h).

This is the only route from the Python classes to the solver: there is no CPU
fall-back.  A missing library raises at import of the first solve/setup call.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (TMPC_LIB: another build of the same library, e.g. a diagnostic variant -- developers' A/B runs; default: the in-tree build)
LIB_PATH = os.environ.get("TMPC_LIB") or os.path.join(_PKG, "lib", "libtmpc_hip.so")
ABI_VERSION = 5

_PTR_FIELDS = ["A", "B", "Q", "R", "P", "T", "K", "K_anc",
               "Hx", "hx", "Hu", "hu", "HT", "hT", "HZ", "hZ", "HZW", "hZW", "HTP", "hTP"]
_INT_FIELDS = ["nx", "nu", "N", "rx", "ru", "rT", "rZ", "rZW",
               "fixed_x0", "extended", "literal_terminal_row", "max_iter"]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint8)


class TmpcProblem(C.Structure):
    """Field-for-field include/tmpc.h: tmpc_problem."""
    _fields_ = ([(n, C.c_int32) for n in _INT_FIELDS] + [("tol", C.c_double)]
                + [(n, _dp) for n in _PTR_FIELDS] + [("rTP", C.c_int32), ("terminal_equality", C.c_int32)])


_REG_INT_FIELDS = ["nx", "nu", "N", "rx", "ru", "rf", "rZ", "tube", "max_iter"]
_REG_PTR_FIELDS = ["A", "B", "Q", "R", "P", "K", "Hx", "hx", "Hu", "hu", "Hf", "hf", "HZ", "hZ"]


class TmpcRegulatorProblem(C.Structure):
    """Field-for-field include/tmpc.h: tmpc_regulator_problem."""
    _fields_ = ([(n, C.c_int32) for n in _REG_INT_FIELDS] + [("tol", C.c_double)]
                + [(n, _dp) for n in _REG_PTR_FIELDS])


_lib = None


def _share_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so with the same SONAME as the system one.
    Two HIP runtimes cannot both own the GPU in one process, and whichever is loaded first
    wins the SONAME.  When torch is installed (bench.py and the multi-GPU driver use it for
    device buffers and RCCL) bind this library to torch's copy, so that tensors, RCCL and the
    solve kernels share one runtime regardless of import order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_PKG, 'csrc')}` "
                "(or __graft_entry__.build()).  There is no CPU solve path.")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.tmpc_abi_version.restype = C.c_int
        if L.tmpc_abi_version() != ABI_VERSION:
            raise RuntimeError("libtmpc_hip.so ABI version mismatch")
        L.tmpc_last_error.argtypes = [C.c_void_p]
        L.tmpc_last_error.restype = C.c_char_p
        L.tmpc_create.argtypes = [C.POINTER(TmpcProblem), C.c_int, C.POINTER(C.c_void_p)]
        L.tmpc_create.restype = C.c_int
        L.tmpc_destroy.argtypes = [C.c_void_p]
        L.tmpc_destroy.restype = None
        sig = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tmpc_solve_batch.argtypes = sig
        L.tmpc_solve_batch.restype = C.c_int
        L.tmpc_solve_batch_device.argtypes = sig
        L.tmpc_solve_batch_device.restype = C.c_int
        L.tmpc_set_kernel_path.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_set_kernel_path.restype = C.c_int
        L.tmpc_get_kernel_path.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_get_kernel_path.restype = C.c_int
        L.tmpc_kernel_name.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_kernel_name.restype = C.c_char_p
        L.tmpc_mc_run.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int] + [C.c_void_p] * 8 + [C.c_int32] + [C.c_void_p] * 6
        L.tmpc_mc_set_capture.argtypes = [C.c_void_p, C.c_int64]
        L.tmpc_mc_set_capture.restype = C.c_int
        L.tmpc_mc_get_capture.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tmpc_mc_get_capture.restype = C.c_int
        L.tmpc_set_solve_timing.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_set_solve_timing.restype = C.c_int
        L.tmpc_get_solve_ticks.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.tmpc_get_solve_ticks.restype = C.c_int
        L.tmpc_mc_get_solve_ticks.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.tmpc_mc_get_solve_ticks.restype = C.c_int
        L.tmpc_mc_set_device_rng.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_int64, C.c_void_p]
        L.tmpc_mc_set_device_rng.restype = C.c_int
        L.tmpc_mc_get_physics_error.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.tmpc_mc_get_physics_error.restype = C.c_int
        L.tmpc_mc_set_warm_start.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_mc_set_warm_start.restype = C.c_int
        L.tmpc_mc_set_fused.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_mc_set_fused.restype = C.c_int
        L.tmpc_mc_last_fused.argtypes = [C.c_void_p]
        L.tmpc_mc_last_fused.restype = C.c_int
        L.tmpc_mc_run.restype = C.c_int
        L.tmpc_mc_open.argtypes = ([C.c_void_p, C.c_int64, C.c_int32, C.c_int] + [C.c_void_p] * 7 + [C.c_int32]
                                   + [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 2 + [C.c_int32])
        L.tmpc_mc_open.restype = C.c_int
        L.tmpc_mc_step_device.argtypes = [C.c_void_p] * 4
        L.tmpc_mc_step_device.restype = C.c_int
        L.tmpc_mc_step.argtypes = [C.c_void_p] * 3
        L.tmpc_mc_step.restype = C.c_int
        L.tmpc_mc_set_reference_table.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.tmpc_mc_set_reference_table.restype = C.c_int
        L.tmpc_mc_step_device_ref.argtypes = [C.c_void_p] * 5
        L.tmpc_mc_step_device_ref.restype = C.c_int
        L.tmpc_mc_step_ref.argtypes = [C.c_void_p] * 4
        L.tmpc_mc_step_ref.restype = C.c_int
        L.tmpc_mc_set_channel.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        L.tmpc_mc_set_channel.restype = C.c_int
        L.tmpc_mc_get_channel.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.tmpc_mc_get_channel.restype = C.c_int
        L.tmpc_mc_get_link_stats.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        L.tmpc_mc_get_link_stats.restype = C.c_int
        L.tmpc_mc_set_series.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_mc_set_series.restype = C.c_int
        L.tmpc_mc_set_law.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64]
        L.tmpc_mc_get_law_stats.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tmpc_mc_get_law_misses.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("tmpc_mc_set_law", "tmpc_mc_get_law_stats", "tmpc_mc_get_law_misses"):
            getattr(L, name).restype = C.c_int
        L.tmpc_mc_get_series.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.tmpc_mc_get_series.restype = C.c_int
        L.tmpc_mc_series_stats.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p] + [C.c_void_p] * 16
        L.tmpc_mc_series_stats.restype = C.c_int
        L.tmpc_series_stats.argtypes = [C.c_int, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p] + [C.c_void_p] * 16
        L.tmpc_series_stats.restype = C.c_int
        L.tmpc_mc_close.argtypes = [C.c_void_p] * 9
        L.tmpc_mc_close.restype = C.c_int
        L.tmpc_mc_replay.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int] + [C.c_void_p] * 8
        L.tmpc_mc_replay.restype = C.c_int
        L.tmpc_mc_set_actuator.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_mc_set_actuator.restype = C.c_int
        L.tmpc_mc_set_plant.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int]
        L.tmpc_mc_set_plant.restype = C.c_int
        L.tmpc_mc_set_plant_models.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int]
        L.tmpc_mc_set_plant_models.restype = C.c_int
        L.tmpc_plant_step_device.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.tmpc_plant_step_device.restype = C.c_int
        L.tmpc_mc_run_plants.argtypes = ([C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
                                         + ([C.c_void_p] * 2 + [C.c_int32]) * 3 + [C.c_void_p] * 9)
        L.tmpc_mc_run_plants.restype = C.c_int
        L.tmpc_lp_batch.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tmpc_lp_batch.restype = C.c_int
        L.tmpc_order_statistics.argtypes = [C.c_int, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tmpc_order_statistics.restype = C.c_int
        L.tmpc_estimate_w.argtypes = ([C.c_int, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_int32]
                                      + [C.c_void_p] * 3 + [C.c_uint64, C.c_int64, C.c_int32, C.c_void_p, C.c_double] + [C.c_void_p] * 10)
        L.tmpc_estimate_w.restype = C.c_int
        L.tmpc_estimate_w_models.argtypes = ([C.c_int, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32]
                                             + [C.c_void_p] * 3 + [C.c_uint64, C.c_int64, C.c_int32, C.c_void_p, C.c_double] + [C.c_void_p] * 10)
        L.tmpc_estimate_w_models.restype = C.c_int
        L.tmpc_synchronize.argtypes = [C.c_void_p]
        L.tmpc_synchronize.restype = C.c_int
        L.tmpc_set_call_overlap.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_set_call_overlap.restype = C.c_int
        L.tmpc_debug_lane_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
        L.tmpc_debug_lane_counters.restype = C.c_int
        if hasattr(L, "tmpc_set_call_lanes"):      # (an older build loaded through TMPC_LIB for an A/B has none of these)
            L.tmpc_set_call_lanes.argtypes = [C.c_void_p, C.c_int]
            L.tmpc_set_call_lanes.restype = C.c_int
            L.tmpc_get_call_lanes.argtypes = [C.c_void_p]
            L.tmpc_get_call_lanes.restype = C.c_int
            L.tmpc_debug_lane_counters_n.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
            L.tmpc_debug_lane_counters_n.restype = C.c_int
            L.tmpc_debug_elastic_grid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            L.tmpc_debug_elastic_grid.restype = C.c_int
            L.tmpc_debug_surplus_yields.argtypes = [C.c_uint32, C.c_int32]
            L.tmpc_debug_surplus_yields.restype = C.c_int
            L.tmpc_debug_plan_lanes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            L.tmpc_debug_plan_lanes.restype = C.c_int
            L.tmpc_debug_busy_union.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
            L.tmpc_debug_busy_union.restype = C.c_double
        L.tmpc_debug_calls_conflict.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p), C.c_int64, C.POINTER(C.c_void_p)]
        L.tmpc_debug_calls_conflict.restype = C.c_int
        L.tmpc_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.tmpc_last_kernel_ms.restype = C.c_int
        L.tmpc_kernel_ms_total.argtypes = [C.c_void_p, C.POINTER(C.c_float), _ip, C.c_int]
        L.tmpc_kernel_ms_total.restype = C.c_int
        L.tmpc_get_dims.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip]
        L.tmpc_get_dims.restype = C.c_int
        L.tmpc_get_factoring.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip]
        L.tmpc_get_factoring.restype = C.c_int
        L.tmpc_get_condensed.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
        L.tmpc_get_condensed.restype = C.c_int
        L.tmpc_create_regulator.argtypes = [C.POINTER(TmpcRegulatorProblem), C.c_int, C.POINTER(C.c_void_p)]
        L.tmpc_create_regulator.restype = C.c_int
        L.tmpc_reg_run.argtypes = ([C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 2
                                   + [C.c_int32] + [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 8 + [C.c_int64]
                                   + [C.c_void_p] * 3)
        L.tmpc_reg_run.restype = C.c_int
        jac = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_double] + [C.c_void_p] * 4
        vjp = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_double] + [C.c_void_p] * 4
        for name, sig in (("tmpc_sens_jacobian", jac), ("tmpc_sens_jacobian_device", jac), ("tmpc_sens_vjp", vjp), ("tmpc_sens_vjp_device", vjp)):
            getattr(L, name).argtypes = sig
            getattr(L, name).restype = C.c_int
        L.tmpc_sens_get_model.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.tmpc_sens_get_model.restype = C.c_int
        if hasattr(L, "tmpc_sens_vjp_weights"):     # (an older build loaded through TMPC_LIB for an A/B has none of these)
            vjpw = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_double] + [C.c_void_p] * 8
            for name in ("tmpc_sens_vjp_weights", "tmpc_sens_vjp_weights_device"):
                getattr(L, name).argtypes = vjpw
                getattr(L, name).restype = C.c_int
            L.tmpc_sens_weight_map.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
            L.tmpc_sens_weight_map.restype = C.c_int
            L.tmpc_qp_sensitivity_data.argtypes = ([C.c_int] + [C.c_int32] * 4 + [C.c_void_p] * 7 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_double]
                                                   + [C.c_void_p] * 7)
            L.tmpc_qp_sensitivity_data.restype = C.c_int
        L.tmpc_qp_sensitivity.argtypes = ([C.c_int] + [C.c_int32] * 4 + [C.c_void_p] * 7 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_double, C.c_int]
                                          + [C.c_void_p] * 5)
        L.tmpc_qp_sensitivity.restype = C.c_int
        law = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 8
        for name in ("tmpc_law_eval", "tmpc_law_eval_device", "tmpc_law_solve", "tmpc_law_solve_device"):
            getattr(L, name).argtypes = law
            getattr(L, name).restype = C.c_int
        L.tmpc_law_add.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
        L.tmpc_law_learn.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_double] + [C.c_void_p] * 2
        L.tmpc_law_get_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tmpc_law_reorder.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_law_clear.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_law_get_region.argtypes = [C.c_void_p, C.c_int, C.c_int32] + [C.c_void_p] * 5
        L.tmpc_get_param_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tmpc_qp_law_eval.argtypes = ([C.c_int] + [C.c_int32] * 4 + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                                                            C.c_void_p, C.c_int] + [C.c_void_p] * 3)
        L.tmpc_qp_law_eval_hops.argtypes = L.tmpc_qp_law_eval.argtypes + [C.c_int, C.c_void_p]
        L.tmpc_law_set_hops.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_law_get_hops.argtypes = [C.c_void_p, C.c_void_p]
        L.tmpc_law_get_hop_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tmpc_law_clear_hop_stats.argtypes = [C.c_void_p, C.c_int]
        L.tmpc_law_find_key.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
        for name in ("tmpc_law_add", "tmpc_law_learn", "tmpc_law_get_stats", "tmpc_law_reorder", "tmpc_law_clear", "tmpc_law_get_region", "tmpc_get_param_rows",
                     "tmpc_qp_law_eval", "tmpc_qp_law_eval_hops", "tmpc_law_set_hops", "tmpc_law_get_hops", "tmpc_law_get_hop_stats",
                     "tmpc_law_clear_hop_stats", "tmpc_law_find_key"):
            getattr(L, name).restype = C.c_int
        _lib = L
    return _lib


def pack_problem(d: dict):
    """dict (TubeTrackingMPC._problem_dict) -> (TmpcProblem, keep-alive list)."""
    p = TmpcProblem()
    keep = []
    nx, nu = int(d["nx"]), int(d["nu"])
    p.nx, p.nu, p.N = nx, nu, int(d["N"])
    p.fixed_x0 = int(d.get("fixed_x0", 0))
    p.extended = int(d.get("extended", 0))
    p.literal_terminal_row = int(d.get("literal_terminal_row", 1))
    p.max_iter = int(d.get("max_iter", 0))
    p.tol = float(d.get("tol", 0.0))
    square = {"A": (nx, nx), "B": (nx, nu), "Q": (nx, nx), "R": (nu, nu), "P": (nx, nx), "T": (nx, nx),
              "K": (nu, nx), "K_anc": (nu, nx)}
    widths = {"Hx": nx, "Hu": nu, "HT": 2 * nx + nu, "HZ": nx, "HZW": nx, "HTP": nx + nu}
    rows = {}
    for name in _PTR_FIELDS:
        v = d.get(name)
        if v is None:
            setattr(p, name, _dp())
            continue
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
        if name in square:
            if a.size != square[name][0] * square[name][1]:
                raise ValueError(f"{name} has {a.size} entries, expected shape {square[name]}")
            a = np.ascontiguousarray(a.reshape(square[name]))
        elif name in widths:
            if a.ndim != 2 or a.shape[1] != widths[name]:
                raise ValueError(f"{name} must have {widths[name]} columns, got shape {a.shape}")
            rows[name] = a.shape[0]
        else:                                   # right-hand sides
            a = np.ascontiguousarray(a.reshape(-1))
            rows[name] = a.shape[0]
        keep.append(a)
        setattr(p, name, a.ctypes.data_as(_dp))
    for hk, Hk in (("hx", "Hx"), ("hu", "Hu"), ("hT", "HT"), ("hZ", "HZ"), ("hZW", "HZW"), ("hTP", "HTP")):
        if rows.get(hk, 0) != rows.get(Hk, 0):
            raise ValueError(f"{Hk} has {rows.get(Hk, 0)} rows but {hk} has {rows.get(hk, 0)} entries")
    p.rx, p.ru, p.rT = rows.get("Hx", 0), rows.get("Hu", 0), rows.get("HT", 0)
    p.rZ, p.rZW = rows.get("HZ", 0), rows.get("HZW", 0)
    p.rTP = rows.get("HTP", 0)
    p.terminal_equality = int(d.get("terminal_equality", 0))
    return p, keep


def pack_regulator_problem(d: dict):
    """dict (RegulatorMPC._regulator_dict) -> (TmpcRegulatorProblem, keep-alive list).  Absent sets (None) get 0 rows."""
    p = TmpcRegulatorProblem()
    keep = []
    nx, nu = int(d["nx"]), int(d["nu"])
    p.nx, p.nu, p.N = nx, nu, int(d["N"])
    p.tube = int(d.get("tube", 0))
    p.max_iter = int(d.get("max_iter", 0))
    p.tol = float(d.get("tol", 0.0))
    square = {"A": (nx, nx), "B": (nx, nu), "Q": (nx, nx), "R": (nu, nu), "P": (nx, nx), "K": (nu, nx)}
    widths = {"Hx": nx, "Hu": nu, "Hf": nx, "HZ": nx}
    rows = {}
    for name in _REG_PTR_FIELDS:
        v = d.get(name)
        if v is None:
            setattr(p, name, _dp())
            continue
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
        if name in square:
            if a.size != square[name][0] * square[name][1]:
                raise ValueError(f"{name} has {a.size} entries, expected shape {square[name]}")
            a = np.ascontiguousarray(a.reshape(square[name]))
        elif name in widths:
            if a.ndim != 2 or a.shape[1] != widths[name]:
                raise ValueError(f"{name} must have {widths[name]} columns, got shape {a.shape}")
            rows[name] = a.shape[0]
        else:
            a = np.ascontiguousarray(a.reshape(-1))
            rows[name] = a.shape[0]
        keep.append(a)
        setattr(p, name, a.ctypes.data_as(_dp))
    for hk, Hk in (("hx", "Hx"), ("hu", "Hu"), ("hf", "Hf"), ("hZ", "HZ")):
        if rows.get(hk, 0) != rows.get(Hk, 0):
            raise ValueError(f"{Hk} has {rows.get(Hk, 0)} rows but {hk} has {rows.get(hk, 0)} entries")
    p.rx, p.ru, p.rf, p.rZ = rows.get("Hx", 0), rows.get("Hu", 0), rows.get("Hf", 0), rows.get("HZ", 0)
    return p, keep


class Handle:
    def __init__(self, ptr, nx, nu, N, nvariants, regulator: bool = False):
        self.ptr, self.nx, self.nu, self.N, self.nvariants = ptr, nx, nu, N, nvariants
        self.regulator = regulator
        self.series_shape = None     # (B, T) of the per-step record the last loop left (series=True), for mc_series_stats

    def error(self) -> str:
        return lib().tmpc_last_error(self.ptr).decode()


def create(problem: dict, device: int = 0) -> Handle:
    L = lib()
    p, _keep = pack_problem(problem)
    h = C.c_void_p()
    rc = L.tmpc_create(C.byref(p), int(device), C.byref(h))
    if rc != 0:
        raise RuntimeError(f"tmpc_create failed ({rc}): {L.tmpc_last_error(None).decode()}")
    return Handle(h, p.nx, p.nu, p.N, 2 if p.extended else 1)


def create_regulator(problem: dict, device: int = 0) -> Handle:
    """include/tmpc.h: tmpc_create_regulator (device < 0: host-only handle, for tmpc_get_condensed)."""
    L = lib()
    p, _keep = pack_regulator_problem(problem)
    h = C.c_void_p()
    rc = L.tmpc_create_regulator(C.byref(p), int(device), C.byref(h))
    if rc != 0:
        raise RuntimeError(f"tmpc_create_regulator failed ({rc}): {L.tmpc_last_error(None).decode()}")
    return Handle(h, p.nx, p.nu, p.N, 1, regulator=True)


def destroy(h: Handle):
    if h is not None and h.ptr:
        lib().tmpc_destroy(h.ptr)
        h.ptr = None


def get_dims(h: Handle, variant: int = 0):
    nv, nc, npar = C.c_int32(), C.c_int32(), C.c_int32()
    if lib().tmpc_get_dims(h.ptr, variant, C.byref(nv), C.byref(nc), C.byref(npar)) != 0:
        raise RuntimeError("tmpc_get_dims failed")
    return nv.value, nc.value, npar.value


def get_factoring(h: Handle, variant: int = 0):
    """include/tmpc.h: tmpc_get_factoring -> (general rows, rows of the factored block, its rank)."""
    nd, ncc, kc = C.c_int32(), C.c_int32(), C.c_int32()
    if lib().tmpc_get_factoring(h.ptr, variant, C.byref(nd), C.byref(ncc), C.byref(kc)) != 0:
        raise RuntimeError("tmpc_get_factoring failed")
    return nd.value, ncc.value, kc.value


def get_condensed(h: Handle, variant: int = 0) -> dict:
    nv, nc, _ = get_dims(h, variant)
    out = dict(H=np.empty((nv, nv)), F1=np.empty((nv, h.nx)), F2=np.empty((nv, h.nx)),
               G=np.empty((nc, nv)), g0=np.empty(nc), E=np.empty((nc, h.nx)))
    rc = lib().tmpc_get_condensed(h.ptr, variant, *[out[k].ctypes.data_as(_dp) for k in ("H", "F1", "F2", "G", "g0", "E")])
    if rc != 0:
        raise RuntimeError("tmpc_get_condensed failed")
    return out


TICK_SECONDS = 1e-8      # s_memrealtime: constant 100 MHz (include/tmpc.h, tmpc_set_solve_timing)


def solve_batch(h: Handle, x, r, variant=None, want_traj: bool = True, timing: bool = False) -> dict:
    """Host-pointer entry (tmpc_solve_batch): numpy in, numpy out.  timing: also `solve_time` (B,), the seconds every
    instance spent in its wavefront / workgroup (tmpc_set_solve_timing)."""
    B = x.shape[0]
    if lib().tmpc_set_solve_timing(h.ptr, int(bool(timing))) != 0:
        raise RuntimeError(h.error())
    nx, nu, N = h.nx, h.nu, h.N
    out = dict(u_nom=np.empty((B, N, nu)), x_nom0=np.empty((B, nx)), xu_ss=np.empty((B, nx + nu)),
               x_nom=np.empty((B, N + 1, nx)) if want_traj else None,
               status=np.empty(B, np.int32), iters=np.empty(B, np.int32))
    vptr = None
    if variant is not None:
        var = np.ascontiguousarray(np.broadcast_to(np.asarray(variant, dtype=np.uint8).reshape(-1), (B,)))
        vptr = var.ctypes.data
    rc = lib().tmpc_solve_batch(h.ptr, B, x.ctypes.data, r.ctypes.data, vptr,
                                out["u_nom"].ctypes.data, out["x_nom0"].ctypes.data, out["xu_ss"].ctypes.data,
                                out["x_nom"].ctypes.data if want_traj else None,
                                out["status"].ctypes.data, out["iters"].ctypes.data)
    if rc != 0:
        raise RuntimeError(f"tmpc_solve_batch failed ({rc}): {h.error()}")
    out["x_ss"] = out["xu_ss"][:, :nx]
    out["u_ss"] = out["xu_ss"][:, nx:]
    if timing:
        ticks = np.empty(B, np.int64)
        if lib().tmpc_get_solve_ticks(h.ptr, B, ticks.ctypes.data) != 0:
            raise RuntimeError(h.error())
        out["solve_time"] = ticks * TICK_SECONDS
    return out


def solve_regulator_batch(h: Handle, x, want_traj: bool = True) -> dict:
    """tmpc_solve_batch on a regulator handle: x (B, nx) -> u_nom (B, N, nu), x_nom0 (B, nx) (x_0: a decision variable of
    the tube regulator, x_k for the plain one), x_nom (B, N+1, nx), status, iters; NaN rows where status >= INFEASIBLE."""
    B = x.shape[0]
    if lib().tmpc_set_solve_timing(h.ptr, 0) != 0:
        raise RuntimeError(h.error())
    nx, nu, N = h.nx, h.nu, h.N
    out = dict(u_nom=np.empty((B, N, nu)), x_nom0=np.empty((B, nx)), x_nom=np.empty((B, N + 1, nx)) if want_traj else None,
               status=np.empty(B, np.int32), iters=np.empty(B, np.int32))
    rc = lib().tmpc_solve_batch(h.ptr, B, x.ctypes.data, None, None, out["u_nom"].ctypes.data, out["x_nom0"].ctypes.data, None,
                                out["x_nom"].ctypes.data if want_traj else None, out["status"].ctypes.data, out["iters"].ctypes.data)
    if rc != 0:
        raise RuntimeError(f"tmpc_solve_batch failed ({rc}): {h.error()}")
    return out


def solve_batch_device(h: Handle, B: int, x_ptr, r_ptr, var_ptr, u_ptr, x0_ptr, ss_ptr, xn_ptr, st_ptr, it_ptr):
    """Device-pointer entry (tmpc_solve_batch_device): raw addresses (e.g. tensor.data_ptr())."""
    rc = lib().tmpc_solve_batch_device(h.ptr, int(B), x_ptr, r_ptr, var_ptr, u_ptr, x0_ptr, ss_ptr, xn_ptr, st_ptr, it_ptr)
    if rc != 0:
        raise RuntimeError(f"tmpc_solve_batch_device failed ({rc}): {h.error()}")


def synchronize(h: Handle):
    if lib().tmpc_synchronize(h.ptr) != 0:
        raise RuntimeError(h.error())


def set_call_overlap(h: Handle, on: bool = True):
    """include/tmpc.h: tmpc_set_call_overlap -- independent tmpc_solve_batch_device calls of the handle may run side by side (default) or not."""
    if lib().tmpc_set_call_overlap(h.ptr, int(bool(on))) != 0:
        raise RuntimeError(h.error())


def lane_counters(h: Handle, reset: bool = False):
    """include/tmpc.h: tmpc_debug_lane_counters -> ((device-pointer calls by the parity of the lane changes: with two lanes, those enqueued on
    lane 0, on lane 1), calls that had to wait for another lane), since the handle was created or the counters were last reset."""
    calls, waits = (C.c_int64 * 2)(), C.c_int64()
    if lib().tmpc_debug_lane_counters(h.ptr, calls, C.byref(waits), int(reset)) != 0:
        raise RuntimeError(h.error())
    return (int(calls[0]), int(calls[1])), int(waits.value)


MAX_LANES = 4


def set_call_lanes(h: Handle, n: int):
    """include/tmpc.h: tmpc_set_call_lanes -- the launch lanes (1 ... MAX_LANES) the handle's independent calls rotate over."""
    if lib().tmpc_set_call_lanes(h.ptr, int(n)) != 0:
        raise RuntimeError(h.error())


def get_call_lanes(h: Handle) -> int:
    """include/tmpc.h: tmpc_get_call_lanes -- the lanes in use now."""
    return int(lib().tmpc_get_call_lanes(h.ptr))


def lane_counters_n(h: Handle, reset: bool = False):
    """include/tmpc.h: tmpc_debug_lane_counters_n -> ((device-pointer calls enqueued on each of the MAX_LANES lanes), calls that had to
    wait for another lane)."""
    calls, waits = (C.c_int64 * MAX_LANES)(), C.c_int64()
    if lib().tmpc_debug_lane_counters_n(h.ptr, calls, C.byref(waits), int(reset)) != 0:
        raise RuntimeError(h.error())
    return tuple(int(c) for c in calls), int(waits.value)


def elastic_grid(h: Handle, n_cu: int, lanes: int, wpb: int, B: int):
    """include/tmpc.h: tmpc_debug_elastic_grid -> (core workgroups, whether a launch over B instances would be elastic).  No device is touched."""
    core, el = C.c_int32(), C.c_int32()
    if lib().tmpc_debug_elastic_grid(h.ptr, n_cu, lanes, wpb, int(B), C.byref(core), C.byref(el)) != 0:
        raise RuntimeError("tmpc_debug_elastic_grid: invalid argument")
    return int(core.value), bool(el.value)


def surplus_yields(followers: int, lanes: int) -> bool:
    """include/tmpc.h: tmpc_debug_surplus_yields -- the decision of a surplus workgroup of an elastic launch."""
    return bool(lib().tmpc_debug_surplus_yields(int(followers), int(lanes)))


def plan_lanes(nx: int, nu: int, N: int, lanes: int, calls):
    """include/tmpc.h: tmpc_debug_plan_lanes.  calls: [(B, {argument name (SOLVE_POINTERS): address})] -> (lane, wait mask, followers) per
    call, for a script none of whose calls finishes.  No device is touched."""
    n = len(calls)
    B = (C.c_int64 * max(n, 1))(*[int(b) for b, _ in calls])
    ptrs = (C.c_void_p * (9 * max(n, 1)))(*[a.get(k) for _, a in calls for k in SOLVE_POINTERS])
    lane, waited, fol = ((C.c_int32 * max(n, 1))() for _ in range(3))
    if lib().tmpc_debug_plan_lanes(nx, nu, N, int(lanes), n, B, ptrs, lane, waited, fol) != 0:
        raise RuntimeError("tmpc_debug_plan_lanes: invalid argument")
    return [(int(lane[i]), int(waited[i]), int(fol[i])) for i in range(n)]


def busy_union(lanes, start, end) -> float:
    """include/tmpc.h: tmpc_debug_busy_union -- tmpc_kernel_ms_total's arithmetic on calls given in call order."""
    n = len(lanes)
    la = (C.c_int32 * max(n, 1))(*[int(x) for x in lanes])
    s = (C.c_double * max(n, 1))(*[float(x) for x in start])
    e = (C.c_double * max(n, 1))(*[float(x) for x in end])
    return float(lib().tmpc_debug_busy_union(n, la, s, e))


SOLVE_POINTERS = ("x_k", "ref", "variant", "u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters")


def calls_conflict(nx: int, nu: int, N: int, B_a: int, a: dict, B_b: int, b: dict) -> bool:
    """include/tmpc.h: tmpc_debug_calls_conflict -- whether the later of two tmpc_solve_batch_device calls must stay behind the
    earlier one.  a, b: {argument name (SOLVE_POINTERS): address}; a missing name or None is a NULL pointer.  No device is touched."""
    pa = (C.c_void_p * 9)(*[a.get(k) for k in SOLVE_POINTERS])
    pb = (C.c_void_p * 9)(*[b.get(k) for k in SOLVE_POINTERS])
    rc = lib().tmpc_debug_calls_conflict(nx, nu, N, int(B_a), pa, int(B_b), pb)
    if rc < 0:
        raise RuntimeError("tmpc_debug_calls_conflict: invalid argument")
    return bool(rc)


def last_kernel_ms(h: Handle) -> float:
    ms = C.c_float()
    if lib().tmpc_last_kernel_ms(h.ptr, C.byref(ms)) != 0:
        raise RuntimeError(h.error())
    return float(ms.value)


def kernel_ms_total(h: Handle, reset: bool = True):
    """(sum of per-call device ms, number of calls) since the last reset."""
    ms, cnt = C.c_float(), C.c_int32()
    if lib().tmpc_kernel_ms_total(h.ptr, C.byref(ms), C.byref(cnt), int(reset)) != 0:
        raise RuntimeError(h.error())
    return float(ms.value), int(cnt.value)


def kernel_name(h: Handle, variant: int = 0) -> str:
    """Name of the kernel instantiation that solves `variant` (as in a rocprofv3 kernel trace)."""
    return lib().tmpc_kernel_name(h.ptr, int(variant)).decode()


KERNEL_PATHS = {"auto": 0, "wave": 1, "block": 2}


def set_kernel_path(h: Handle, path):
    """include/tmpc.h: tmpc_set_kernel_path ('auto' | 'wave' | 'block')."""
    code = KERNEL_PATHS[path] if isinstance(path, str) else int(path)
    if lib().tmpc_set_kernel_path(h.ptr, code) != 0:
        raise RuntimeError(h.error())


def get_kernel_path(h: Handle, variant: int = 0) -> str:
    code = lib().tmpc_get_kernel_path(h.ptr, int(variant))
    if code < 0:
        raise RuntimeError("tmpc_get_kernel_path failed")
    return {v: k for k, v in KERNEL_PATHS.items()}[code]


def mc_set_actuator(h: Handle, smart: bool):
    """include/tmpc.h: tmpc_mc_set_actuator (False: consistent actuator, True: plain smart actuator of the R-MPC loop)."""
    if lib().tmpc_mc_set_actuator(h.ptr, 1 if smart else 0) != 0:
        raise RuntimeError(h.error())


def mc_set_plant(h: Handle, plant=None, Th: float = 0.02, substeps: int = 10):
    """include/tmpc.h: tmpc_mc_set_plant.  plant: None / 'linear', or 'cartpole' (workloads.CARTPOLE_PARAMS)."""
    if plant in (None, "linear"):
        rc = lib().tmpc_mc_set_plant(h.ptr, 0, None, 0)
    elif plant == "cartpole":
        from .workloads import CARTPOLE_PARAMS as P
        par = (C.c_double * 7)(P["M"], P["m"], P["b"], P["I"], P["g"], P["l"], float(Th))
        rc = lib().tmpc_mc_set_plant(h.ptr, 1, par, int(substeps))
    else:
        raise ValueError(f"unknown plant {plant!r}")
    if rc != 0:
        raise RuntimeError(h.error())


def mc_set_plant_models(h: Handle, kind, models=None, substeps: int = 10):
    """include/tmpc.h: tmpc_mc_set_plant_models -- a plant per trajectory of the next tmpc_reg_run of a regulator handle.  kind
    'linear': models (B, nx, nx + nu), rows [A_b[i, :] | B_b[i, :]].  models None clears them.  Returns the models' batch size (None
    when cleared)."""
    if models is None:
        if lib().tmpc_mc_set_plant_models(h.ptr, 0, 0, None, 0) != 0:
            raise RuntimeError(h.error())
        return None
    if kind not in ("linear", "cartpole"):
        raise ValueError(f"unknown plant {kind!r}")
    m = np.ascontiguousarray(np.asarray(models, dtype=np.float64))
    want = (7,) if kind == "cartpole" else (h.nx, h.nx + h.nu)
    if m.ndim != len(want) + 1 or m.shape[1:] != want:
        raise ValueError(f"mc_set_plant_models: {kind} models are (B,) + {want}, got {m.shape}")
    rc = lib().tmpc_mc_set_plant_models(h.ptr, PLANT_KIND[kind], m.shape[0], m.ctypes.data, int(substeps))
    if rc != 0:
        raise RuntimeError(f"tmpc_mc_set_plant_models failed ({rc}): {h.error()}")
    return m.shape[0]


def mc_set_reference(h: Handle, table=None, ref_id=None, B=None):
    """include/tmpc.h: tmpc_mc_set_reference_table -- full-state reference schedules of the next closed loops.  table
    (K, T_tab, nx) (or (T_tab, nx): K = 1); ref_id (B,) ints in [0, K) or None (K == 1: schedule 0 for everybody, K == B: schedule
    b); B: the batch of the loops (default: len(ref_id), else K).  table None clears the setting."""
    if table is None:
        if lib().tmpc_mc_set_reference_table(h.ptr, 0, 0, None, 0, None) != 0:
            raise RuntimeError(h.error())
        return
    table = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
    if table.ndim == 2:
        table = table[None]
    if table.ndim != 3 or table.shape[2] != h.nx:
        raise ValueError(f"mc_set_reference: table must be (K, T_tab, nx = {h.nx}), got {table.shape}")
    K, T_tab = table.shape[:2]
    ids = None
    if ref_id is not None:
        ids = np.ascontiguousarray(np.asarray(ref_id).reshape(-1), dtype=np.int32)
        if not np.array_equal(ids, np.asarray(ref_id).reshape(-1)):
            raise ValueError("mc_set_reference: ref_id must hold integers")
        if B is not None and int(B) != ids.shape[0]:
            raise ValueError("mc_set_reference: ref_id must have B entries")
    Bv = int(B) if B is not None else (ids.shape[0] if ids is not None else K)
    rc = lib().tmpc_mc_set_reference_table(h.ptr, K, T_tab, table.ctypes.data, Bv, None if ids is None else ids.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"tmpc_mc_set_reference_table failed ({rc}): {h.error()}")


def reference_form(nx: int, who: str, ref, B: int, T, ref_id, flatten_legacy: bool = False):
    """The `ref` forms of the closed loops -> (legacy (T,) array or None, table (K, T, nx) or None, T): (T,) legacy; (nx,) with
    T > nx, or (1, nx) with any T: constant full state; (T, nx): one schedule; (B, T, nx): one per trajectory; (K, T, nx) with
    ref_id (B,): K shared schedules.  flatten_legacy (the stepped loop, which has always flattened its `ref`): a scalar, and a 2-D
    array that is no full-state form -- one row or one column, the other extent not nx -- are the legacy reference flattened.
    The one place that tells the forms apart."""
    ref = np.ascontiguousarray(np.asarray(ref, dtype=np.float64))
    if flatten_legacy and ref_id is None and (ref.ndim == 0 or (ref.ndim == 2 and 1 in ref.shape and ref.shape[1] != nx)):
        ref = ref.reshape(-1)
    if ref.ndim == 2 and ref.shape == (1, nx) and T is not None and ref_id is None:
        ref = np.broadcast_to(ref[None], (1, int(T), nx))          # the constant form for every T (T <= nx included)
    if ref.ndim == 1:
        # (nx,) is the constant form where it cannot be the legacy one: T is given and the array does not cover T steps
        if not (T is not None and ref.shape[0] == nx and ref.shape[0] < int(T)):
            if ref_id is not None:
                raise ValueError(f"{who}: ref_id selects among (K, T, nx) schedules")
            return ref, None, ref.shape[0]
        ref = np.broadcast_to(ref, (1, int(T), nx))
    elif ref.ndim == 2:
        ref = ref[None]
    if ref.ndim != 3 or ref.shape[2] != nx:
        raise ValueError(f"{who}: ref must be (T,), (nx,) with T > nx or (1, nx) with T, (T, nx), (B, T, nx) or (K, T, nx) with ref_id; "
                         f"got {ref.shape} (nx = {nx})")
    if ref_id is None and ref.shape[0] not in (1, B):
        raise ValueError(f"{who}: ref holds {ref.shape[0]} schedules for B = {B} trajectories and no ref_id")
    return None, ref, (ref.shape[1] if T is None else int(T))


def _loop_reference(h: Handle, who: str, ref, B: int, T, ref_id, flatten_legacy: bool = False):
    """reference_form applied to the handle: the table set for the full-state forms, cleared for the legacy one (so that a
    handle's earlier setting never leaks into a legacy call) -> (the legacy (T,) array or None, T)."""
    legacy, table, T = reference_form(h.nx, who, ref, B, T, ref_id, flatten_legacy)
    mc_set_reference(h, table, ref_id if table is not None else None, B=B if table is not None else None)
    return legacy, T


def mc_set_channel(h: Handle, channel=None, B=None):
    """include/tmpc.h: tmpc_mc_set_channel -- the Gilbert-Elliott loss channel of the next closed loops.  channel: a dict with
    p_gb, p_bg, e_g, e_b (montecarlo.burst_channel returns one) or these four in a sequence, each a scalar or (B,); B: the batch of
    the loops (default: the longest parameter).  None clears the setting: independent losses with probability p_loss.  Returns the
    channel's batch size (None when cleared)."""
    if channel is None:
        if lib().tmpc_mc_set_channel(h.ptr, 0, None, None, None, None) != 0:
            raise RuntimeError(h.error())
        return None
    from .montecarlo import channel_parameters
    par = channel_parameters(channel, B)
    rc = lib().tmpc_mc_set_channel(h.ptr, par[0].shape[0], *[v.ctypes.data for v in par])
    if rc != 0:
        raise RuntimeError(f"tmpc_mc_set_channel failed ({rc}): {h.error()}")
    return par[0].shape[0]


def loop_batch(who: str, p_loss, channel, th_u=None, x0=None, ref_id=None, nx=None):
    """The batch of a closed loop and its loss model -> (p_loss (B,) or None, the channel's four (B,) arrays or None, B).  Without a
    channel p_loss gives B.  With one p_loss is not used, and B comes from p_loss if given, else from the rows of th_u, of x0, the
    length of ref_id, or the longest channel parameter; a channel of scalars with none of these has no batch: ValueError.  Nothing is
    set on a handle here: the loops set the channel once their other arguments have been checked."""
    from .montecarlo import channel_parameters
    if channel is None:
        if p_loss is None:
            raise ValueError(f"{who}: p_loss or channel")
        p_loss = np.ascontiguousarray(np.asarray(p_loss, dtype=np.float64))
        return p_loss, None, p_loss.shape[0] if p_loss.ndim else 1
    B = None
    if p_loss is not None:
        B = np.asarray(p_loss).size
    elif th_u is not None:
        B = np.shape(th_u)[0]
    elif x0 is not None:
        B = np.asarray(x0).reshape(-1, nx).shape[0] if nx else np.shape(x0)[0]
    elif ref_id is not None:
        B = np.asarray(ref_id).size
    par = channel_parameters(channel, B)
    if B is None and par[0].shape[0] == 1 and all(np.ndim(v) == 0 for v in (channel.values() if isinstance(channel, dict) else channel)):
        raise ValueError(f"{who}: a channel of scalars does not say how many trajectories to run: give p_loss, th_u, x0 or ref_id, or "
                         "one of the channel's parameters per trajectory")
    return None, par, par[0].shape[0]


def mc_get_channel(h: Handle, B: int):
    """include/tmpc.h: tmpc_mc_get_channel -- the thresholds (B, 2, 3) of the channel that is set, as the device compares them."""
    thr = np.empty((int(B), 2, 3))
    if lib().tmpc_mc_get_channel(h.ptr, int(B), thr.ctypes.data) != 0:
        raise RuntimeError(h.error())
    return thr


def mc_link_stats(h: Handle, B: int) -> dict:
    """include/tmpc.h: tmpc_mc_get_link_stats -- lost_up, lost_down, max_gap, overrun (B,) int32 of the last loop."""
    out = {k: np.empty(int(B), np.int32) for k in ("lost_up", "lost_down", "max_gap", "overrun")}
    if lib().tmpc_mc_get_link_stats(h.ptr, int(B), *[v.ctypes.data for v in out.values()]) != 0:
        raise RuntimeError(h.error())
    return out


def mc_get_series(h: Handle, B: int, T: int) -> dict:
    """include/tmpc.h: tmpc_mc_get_series -- the per-step record of the last loop run with series=True: e (T, B) float64, word (T, B)
    uint32, and the word's fields decoded (montecarlo.unpack_series_word): alive, lost_up, lost_down, adopted, tube, not_optimal,
    overrun (bool), iters, age (int32)."""
    from .montecarlo import decode_series
    e, word = np.empty((int(T), int(B))), np.empty((int(T), int(B)), np.uint32)
    if lib().tmpc_mc_get_series(h.ptr, int(B), int(T), e.ctypes.data, word.ctypes.data) != 0:
        raise RuntimeError(h.error())
    return decode_series(e, word)


def _series_tables(who: str, B: int, T: int, group, q, G):
    """The arguments of a reduction as the C ABI takes them and its output tables -> (group or None, G, q, tables, pointers in ABI order)."""
    from .montecarlo import SERIES_INT_TABLES
    if group is not None:
        group = np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(-1))
        if group.size != B:
            raise ValueError(f"{who}: group holds {group.size} entries, the record {B} trajectories")
    G = (int(group.max()) + 1 if group is not None and group.size else 1) if G is None else int(G)
    q = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1))
    shape = (max(int(T), 0), max(G, 0))
    out = {k: np.empty(shape, np.int64 if k.endswith("_sum") else np.int32) for k in SERIES_INT_TABLES}
    out["e_sum"], out["e_max"], out["e_q"] = np.empty(shape), np.empty(shape), np.empty(shape + (q.size,))
    return group, G, q, out, [v.ctypes.data for v in out.values()]


def mc_series_stats(h: Handle, group=None, q=(0.5, 0.95), G=None, B=None, T=None) -> dict:
    """include/tmpc.h: tmpc_mc_series_stats -- the ensemble statistics of the record the last series=True loop left on the device, per
    time step and group: (T, G) tables n_alive, n_nan, lost_up, lost_down, adopted, tube, not_optimal, overrun, age_max, age_sum,
    iters_max, iters_sum, e_sum, e_max and e_q (T, G, len(q)); kernel_ms, the reduction's device time.  group (B,): ids in [0, G) or -1
    (None: everybody in one group); q: quantiles -- the element of rank floor(q (n - 1)) of the sorted values, no interpolation
    (montecarlo.series_stats is the numpy twin).  B, T: the record's shape (default: that of the handle's last loop)."""
    if B is None or T is None:
        if getattr(h, "series_shape", None) is None:
            raise RuntimeError("mc_series_stats: the handle's last loop kept no per-step record (series=True)")
        B, T = h.series_shape
    B, T = int(B), int(T)
    group, G, q, out, ptrs = _series_tables("mc_series_stats", B, T, group, q, G)
    ms = C.c_float(0.0)
    rc = lib().tmpc_mc_series_stats(h.ptr, B, T, G, _ptr(group), q.size, q.ctypes.data, *ptrs, C.addressof(ms))
    if rc != 0:
        raise RuntimeError(f"tmpc_mc_series_stats failed ({rc}): {h.error()}")
    out["kernel_ms"] = float(ms.value)
    return out


def series_stats(e, word, group=None, q=(0.5, 0.95), G=None, device: int = 0) -> dict:
    """include/tmpc.h: tmpc_series_stats -- the reduction of mc_series_stats on host arrays e, word (T, B), without a handle."""
    e = np.ascontiguousarray(np.asarray(e, dtype=np.float64))
    word = np.ascontiguousarray(np.asarray(word, dtype=np.uint32))
    if e.ndim != 2 or word.shape != e.shape:
        raise ValueError("series_stats: e and word are (T, B)")
    T, B = e.shape
    group, G, q, out, ptrs = _series_tables("series_stats", B, T, group, q, G)
    ms = C.c_float(0.0)
    rc = lib().tmpc_series_stats(int(device), B, T, e.ctypes.data, word.ctypes.data, G, _ptr(group), q.size, q.ctypes.data, *ptrs, C.addressof(ms))
    if rc != 0:
        raise RuntimeError(f"tmpc_series_stats failed ({rc}): {lib().tmpc_last_error(None).decode()}")
    out["kernel_ms"] = float(ms.value)
    return out


MC_FUSED = {"off": 0, "on": 1, "auto": 2, False: 0, True: 1, None: 2}      # include/tmpc.h: TMPC_MC_FUSED_*


def _contiguous(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _law_setting(law):
    """(on, max_tries, miss_capacity) of the `law` argument of mc_run / mc_run_plants / mc_open: None or False -- off; True -- every
    candidate, no miss log; an int -- max_tries; a dict with max_tries (default 0: all) and miss_capacity (default 0) -- and optionally
    max_hops, the handle-wide setting of tmpc_law_set_hops, which `_law_hops` reads."""
    if law is None or law is False:
        return 0, 0, 0
    if law is True:
        return 1, 0, 0
    if isinstance(law, dict):
        extra = set(law) - {"max_tries", "miss_capacity", "max_hops"}
        if extra:
            raise ValueError(f"law: unknown keys {sorted(extra)} (max_tries, miss_capacity, max_hops)")
        return 1, int(law.get("max_tries", 0)), int(law.get("miss_capacity", 0))
    return 1, int(law), 0


def _law_hops(law):
    """max_hops of the `law` argument where it is a dict that names it, else None: the loop runs with the handle's setting (tmpc_law_set_hops)."""
    return int(law["max_hops"]) if isinstance(law, dict) and "max_hops" in law else None


def _restore_law_hops(h: Handle):
    """Puts back the handle's tmpc_law_set_hops value that a loop's law=dict(max_hops=) replaced (a session's: at its close -- the setter
    is refused while it is open)."""
    before = getattr(h, "law_hops_before", None)
    if before is not None:
        h.law_hops_before = None
        law_set_hops(h, before)


def mc_law_stats(h: Handle, B: int) -> dict:
    """include/tmpc.h: tmpc_mc_get_law_stats -- per trajectory of the last loop run through the explicit law: hits (B,) int32, tries (B,)
    int64, region (B,) int32 (the region of the last step taken, -1: a miss)."""
    out = dict(hits=np.empty(B, np.int32), tries=np.empty(B, np.int64), region=np.empty(B, np.int32))
    if lib().tmpc_mc_get_law_stats(h.ptr, B, out["hits"].ctypes.data, out["tries"].ctypes.data, out["region"].ctypes.data) != 0:
        raise RuntimeError(h.error())
    return out


def mc_law_misses(h: Handle, capacity=None) -> dict:
    """include/tmpc.h: tmpc_mc_get_law_misses -- the miss log of the last loop run through the explicit law: n_total (the misses of the
    run), x_k (n, nx), ref (n, nx), variant (n,) uint8 of the n = min(n_total, miss_capacity, capacity) rows kept (capacity None: all
    that were kept).  The order of the rows is not defined."""
    n_total = C.c_int64(0)
    if lib().tmpc_mc_get_law_misses(h.ptr, 0, C.addressof(n_total), None, None, None) != 0:
        raise RuntimeError(h.error())
    n = min(int(n_total.value), int(getattr(h, "law_miss_capacity", 0)))
    if capacity is not None:
        n = min(n, int(capacity))
    x, r, v = np.empty((n, h.nx)), np.empty((n, h.nx)), np.empty(n, np.uint8)
    if n and lib().tmpc_mc_get_law_misses(h.ptr, n, None, x.ctypes.data, r.ctypes.data, v.ctypes.data) != 0:
        raise RuntimeError(h.error())
    return dict(n_total=int(n_total.value), x_k=x, ref=r, variant=v)


def _set_loop_options(h: Handle, timing, warm_start, capture, fused="keep", series: bool = False, law=None):
    """The per-call settings of a tracking loop (mc_run, mc_open): tmpc_set_solve_timing, tmpc_mc_set_warm_start, tmpc_mc_set_capture,
    tmpc_mc_set_series and -- mc_run; a session has one launch form and leaves the setting alone -- tmpc_mc_set_fused.  THE place where
    a new per-call loop option is set."""
    calls = [(lib().tmpc_set_solve_timing, int(bool(timing))), (lib().tmpc_mc_set_warm_start, int(bool(warm_start))),
             (lib().tmpc_mc_set_capture, -1 if capture is None else int(capture)), (lib().tmpc_mc_set_series, int(bool(series)))]
    if fused != "keep":
        calls.insert(1, (lib().tmpc_mc_set_fused, MC_FUSED[fused]))
    for call, arg in calls:
        if call(h.ptr, arg) != 0:
            raise RuntimeError(h.error())
    on, max_tries, miss_capacity = _law_setting(law)
    if lib().tmpc_mc_set_law(h.ptr, on, max_tries, miss_capacity) != 0:
        raise RuntimeError(h.error())
    _restore_law_hops(h)                     # (a loop that failed before its end)
    if _law_hops(law) is not None:           # for this loop alone: the handle's own value comes back at its end (_tracking_result)
        before = law_get_hops(h)
        law_set_hops(h, _law_hops(law))
        h.law_hops_before = before
    h.law_miss_capacity = miss_capacity      # (mc_law_misses: how many rows the loop's log can hold)


def _set_device_rng(h: Handle, device_rng=None, draws_w: bool = True):
    """tmpc_mc_set_device_rng: on with device_rng = (seed, first_trajectory, w_bound), off with None.  draws_w False (the session: w is
    the plant's): (seed, first_trajectory[, ignored])."""
    args = (0, 0, 0, None)
    if device_rng is not None:
        seed, first, w_bound = device_rng if draws_w else (device_rng[0], device_rng[1], None)
        wb = None if w_bound is None else _contiguous(w_bound).reshape(h.nx)
        args = (1, int(seed), int(first), _ptr(wb))
    if lib().tmpc_mc_set_device_rng(h.ptr, *args) != 0:
        raise RuntimeError(h.error())


def _check_set(P, dim: int, who: str):
    """(H, h, rows) of a check polytope, or (None, None, 0)."""
    if P is None:
        return None, None, 0
    HA, hb = _contiguous(P.A), _contiguous(P.b).reshape(-1)
    if HA.ndim != 2 or HA.shape[1] != dim or hb.size != HA.shape[0]:
        raise ValueError(f"{who}: a check set has the wrong dimension")
    return HA, hb, HA.shape[0]


def _tracking_result(h: Handle, out: dict, B: int, T: int, steps: int, loop_mode: int, capture, timing, series: bool = False, law=None) -> dict:
    """Completes the result of a tracking loop (mc_run, mc_close) over the `steps` steps taken of T: the recorded trajectory, the
    solve times, the link statistics and the derived statistics.  THE place where a new loop output is fetched."""
    _restore_law_hops(h)
    n = steps
    if capture is not None:
        xt, xn, ut = np.empty((T, h.nx)), np.empty((T, h.nx)), np.empty((T, h.nu))
        if lib().tmpc_mc_get_capture(h.ptr, T, xt.ctypes.data, xn.ctypes.data, ut.ctypes.data) != 0:
            raise RuntimeError(h.error())
        out["x_traj"], out["x_nom_traj"], out["u_traj"] = xt[:n], xn[:n], ut[:n]
    if timing:
        tsum, tmax = np.empty(B, np.int64), np.empty(B, np.int64)
        if lib().tmpc_mc_get_solve_ticks(h.ptr, B, tsum.ctypes.data, tmax.ctypes.data) != 0:
            raise RuntimeError(h.error())
        out["solve_time_mean"], out["solve_time_max"] = tsum * (TICK_SECONDS / max(n, 1)), tmax * TICK_SECONDS
    out["link_stats"] = mc_link_stats(h, B)
    out.update(out["link_stats"])
    h.series_shape = (B, T) if series else None
    if series:
        out["series"] = mc_get_series(h, B, T)       # (T, B) arrays; rows of steps a session did not take are zero
    if _law_setting(law)[0]:
        st = mc_law_stats(h, B)
        out["law_hits"], out["law_tries"], out["law_region"] = st["hits"], st["tries"], st["region"]
        out["law_misses"] = lambda capacity=None: mc_law_misses(h, capacity)      # (valid until the handle's next loop)
    out["loop_mode"] = loop_mode      # 1: one launch per sweep; 2: one launch per problem and step; 0: solve launches + a state-machine launch per step
    out["fused"] = loop_mode == 1
    out["tracking_error"] = np.sqrt(out["err2"]) / max(n, 1)
    out["consistent_estimate_error"] = float(out["consistent"].max()) if B else 0.0
    out["iters_mean"] = float(out["iters_sum"].sum()) / max(B * n, 1)            # interior-point iterations per solve
    return out


def mc_run(h: Handle, p_loss, ref, th_u, ga_u, w, x0=None, Z=None, extended: bool = False, warm_start: bool = False,
           capture=None, timing: bool = False, physics_substeps: int = 0, device_rng=None, fused=None, ref_id=None, T=None,
           channel=None, series: bool = False, law=None) -> dict:
    """include/tmpc.h: tmpc_mc_run -- the closed loop over the lossy network, resident on the device.
    warm_start: tmpc_mc_set_warm_start for this call; capture: index of a trajectory to record (tmpc_mc_set_capture) ->
    x_traj (T, nx), x_nom_traj (T, nx), u_traj (T, nu) in the result; timing: per trajectory the mean and the maximum
    time of its T solves in seconds (solve_time_mean, solve_time_max; tmpc_set_solve_timing); physics_substeps > 0 (a
    nonlinear plant was set with that many steps per sampling period): tracking_error_physics, the scripts' tracking error
    over the physics-rate trajectory (tmpc_mc_get_physics_error, results_nonlinear_system.py:361).
    device_rng = (seed, first_trajectory, w_bound): the realisations are drawn on the device (tmpc_mc_set_device_rng;
    montecarlo.draw_realisations_philox gives the same numbers on the host); th_u, ga_u, w are then ignored and may be None,
    the batch is len(p_loss) x len(ref).
    fused: "on" / "off" / "auto" (None) -- tmpc_mc_set_fused: one launch for all T steps, a launch pair per step, or the library's
    choice; the result's "fused" says what ran.
    ref: (T,) position reference of the whole batch (the solve gets [ref_t, 0, ..]); or full-state references through
    tmpc_mc_set_reference_table -- (T, nx) one schedule, (B, T, nx) one per trajectory, (K, T, nx) with ref_id (B,) K shared
    schedules, (nx,) together with T (more than nx steps) a constant full state; the tracking error is then |x_t - r_t| over
    all states.  A (T,) call clears an earlier table.  T: the steps (default: the draws' or the reference's).
    channel: the Gilbert-Elliott loss channel of this call (mc_set_channel; None: independent losses with probability p_loss, and
    an earlier channel is cleared); p_loss is then not read and may be None.  The result carries the link statistics lost_up,
    lost_down, max_gap, overrun (also as the dict link_stats) with either loss model.
    series: keep the per-step record (tmpc_mc_set_series) -> result["series"], a dict of (T, B) arrays: e, the error term of every
    step, word, and the word's fields alive, lost_up, lost_down, adopted, tube, not_optimal, overrun, iters, age; mc_series_stats then
    reduces it on the device.  Such a loop runs per time step (loop_mode 0, whatever `fused` says).
    law: the loop looks every step up in the handle's explicit-law table first and solves the misses only (tmpc_mc_set_law) -- True, an
    int (max_tries) or a dict(max_tries=, miss_capacity=, max_hops=); max_hops replaces the handle's tmpc_law_set_hops for this loop alone; the result gains law_hits, law_tries, law_region (B,) and law_misses(), a
    function that fetches the miss log (mc_law_misses)."""
    _set_loop_options(h, timing, warm_start, capture, fused, series, law)
    c, ptr = _contiguous, _ptr
    p_loss, ch_par, n_traj = loop_batch("mc_run", p_loss, channel, None if device_rng is not None else th_u, x0, ref_id, h.nx)
    if T is None and device_rng is None and th_u is not None:
        T = np.shape(th_u)[1]
    ref, T_ref = _loop_reference(h, "mc_run", ref, n_traj, T, ref_id)
    _set_device_rng(h, device_rng)
    if device_rng is not None:
        th_u = ga_u = w = None
        B, T = n_traj, T_ref
    else:
        th_u, ga_u, w = c(th_u), c(ga_u), c(w)
        B, T = th_u.shape
        if ch_par is not None and ch_par[0].shape[0] != B:
            raise ValueError(f"mc_run: the channel holds {ch_par[0].shape[0]} trajectories, the draws {B}")
        if ga_u.shape != (B, T) or w.shape != (B, T, h.nx) or (p_loss is not None and p_loss.shape != (B,)) or (ref is not None and ref.shape != (T,)) or T_ref < T:
            raise ValueError("mc_run: inconsistent shapes" + (f" (a constant full-state reference over T <= nx = {h.nx} steps is (1, nx): "
                                                              "(nx,) is then read as the legacy (T,) form)" if ref is not None and ref.shape == (h.nx,) else ""))
    x0c = None if x0 is None else c(x0).reshape(B, h.nx)
    HZ, hZ, rZ = _check_set(Z, h.nx, "mc_run")
    out = dict(err2=np.empty(B), tube_violations=np.empty(B, np.int32), not_optimal=np.empty(B, np.int32),
               x_final=np.empty((B, h.nx)), consistent=np.empty(B), iters_sum=np.empty(B, np.int32))
    mc_set_channel(h, ch_par)            # (None clears an earlier one; set last, so that no refused call leaves its channel behind)
    rc = lib().tmpc_mc_run(h.ptr, B, T, int(bool(extended)), ptr(p_loss), ptr(ref), ptr(th_u), ptr(ga_u), ptr(w), ptr(x0c),
                           ptr(HZ), ptr(hZ), rZ, ptr(out["err2"]), ptr(out["tube_violations"]), ptr(out["not_optimal"]),
                           ptr(out["x_final"]), ptr(out["consistent"]), ptr(out["iters_sum"]))
    if rc != 0:
        msg = h.error()
        mc_set_channel(h, None)          # a refused loop leaves no channel behind
        raise RuntimeError(f"tmpc_mc_run failed ({rc}): {msg}")
    if physics_substeps > 0:
        out["err2_physics"] = np.empty(B)
        if lib().tmpc_mc_get_physics_error(h.ptr, B, ptr(out["err2_physics"])) != 0:
            raise RuntimeError(h.error())
        out["tracking_error_physics"] = np.sqrt(out["err2_physics"]) / (T * physics_substeps)
    return _tracking_result(h, out, B, T, T, int(lib().tmpc_mc_last_fused(h.ptr)), capture, timing, series, law)


def _family_models(who: str, plant, nx: int, nu: int, B=None):
    """(kind id, models, substeps) of a montecarlo.PlantFamily as the C ABI takes it; the family must fit (nx, nu) and hold B plants."""
    kind = getattr(plant, "kind", None)
    if kind not in ("linear", "cartpole"):
        raise ValueError(f"{who}: plant is a montecarlo.PlantFamily (plant_family, sample_cartpole)")
    m = np.ascontiguousarray(np.asarray(plant.models, dtype=np.float64))
    want = (7,) if kind == "cartpole" else (nx, nx + nu)
    if m.ndim != len(want) + 1 or m.shape[1:] != want or (kind == "cartpole" and (nx, nu) != (4, 1)):
        raise ValueError(f"{who}: {kind} models are (B,) + {want} for nx = {nx}, nu = {nu}; got {m.shape}")
    if B is not None and m.shape[0] != B:
        raise ValueError(f"{who}: the plant family holds {m.shape[0]} plants, the loop {B} trajectories")
    return PLANT_KIND[kind], m, int(plant.substeps)


def plant_step(plant, x, u, w=None, x_plus=None, stream=None):
    """include/tmpc.h: tmpc_plant_step_device -- one launch that advances the plants of a montecarlo.PlantFamily by one period:
    x_plus[b] = f_b(x[b], u[b]) + w[b].  x (B, nx), u (B, nu), w (B, nx) or None, x_plus (B, nx) or None (a new tensor): contiguous
    float64 CUDA tensors; plant.models may be such a tensor too (a family kept on the device), else it is uploaded.  Enqueued on
    `stream` (an integer hipStream_t; None: torch's current stream) without synchronising; returns x_plus, which must not overlap x."""
    import torch
    who = "plant_step"
    for name, a in (("x", x), ("u", u), ("w", w), ("x_plus", x_plus)):
        if a is not None and not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float64 and a.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous float64 CUDA tensor")
    if x.dim() != 2 or u.dim() != 2 or u.shape[0] != x.shape[0]:
        raise ValueError(f"{who}: x is (B, nx) and u is (B, nu)")
    B, nx = x.shape
    nu = u.shape[1]
    models = plant.models
    if isinstance(models, torch.Tensor):
        kind, sub = PLANT_KIND[plant.kind], int(plant.substeps)
        if not (models.is_cuda and models.dtype == torch.float64 and models.is_contiguous()) or models.shape[0] != B:
            raise ValueError(f"{who}: models on the device are a contiguous float64 CUDA tensor of B = {B} plants")
    else:
        kind, m, sub = _family_models(who, plant, nx, nu, B)
        models = torch.as_tensor(m, device=x.device)
    if x_plus is None:
        x_plus = torch.empty_like(x)
    for name, a in (("w", w), ("x_plus", x_plus)):
        if a is not None and tuple(a.shape) != (B, nx):
            raise ValueError(f"{who}: {name} must be (B, nx) = {(B, nx)}")
    if stream is None:
        stream = torch.cuda.current_stream(x.device).cuda_stream
    rc = lib().tmpc_plant_step_device(x.device.index, kind, nx, nu, B, models.data_ptr(), sub, x.data_ptr(), u.data_ptr(),
                                      None if w is None else w.data_ptr(), x_plus.data_ptr(), int(stream) if stream else None)
    if rc != 0:
        raise RuntimeError(f"tmpc_plant_step_device failed ({rc}): {lib().tmpc_last_error(None).decode()}")
    return x_plus


def mc_run_plants(h: Handle, plant, p_loss, ref, th_u=None, ga_u=None, w=None, x0=None, Z=None, X=None, U=None, extended: bool = False,
                  warm_start: bool = False, capture=None, timing: bool = False, device_rng=None, ref_id=None, T=None, channel=None,
                  series: bool = False, law=None) -> dict:
    """include/tmpc.h: tmpc_mc_run_plants -- the closed loop of mc_run with a plant per trajectory: `plant` is a montecarlo.PlantFamily of
    B plants, cart-poles or linear models; the stepped session and the plant kernel alternate on the device for T steps.  The arguments
    are mc_run's (`fused` does not apply) plus the check sets X, U of mc_open; the result has mc_run's keys -- with
    tracking_error_physics for a cart-pole family -- plus x_violations and u_violations.  series, law: as in mc_run."""
    _set_loop_options(h, timing, warm_start, capture, series=series, law=law)
    c, ptr = _contiguous, _ptr
    p_loss, ch_par, n_traj = loop_batch("mc_run_plants", p_loss, channel, None if device_rng is not None else th_u, x0, ref_id, h.nx)
    if T is None and device_rng is None and th_u is not None:
        T = np.shape(th_u)[1]
    ref, T_ref = _loop_reference(h, "mc_run_plants", ref, n_traj, T, ref_id)
    _set_device_rng(h, device_rng)
    if device_rng is not None:
        th_u = ga_u = w = None
        B, T = n_traj, T_ref
    else:
        th_u, ga_u, w = c(th_u), c(ga_u), c(w)
        B, T = th_u.shape
        if ch_par is not None and ch_par[0].shape[0] != B:
            raise ValueError(f"mc_run_plants: the channel holds {ch_par[0].shape[0]} trajectories, the draws {B}")
        if ga_u.shape != (B, T) or w.shape != (B, T, h.nx) or (p_loss is not None and p_loss.shape != (B,)) or (ref is not None and ref.shape != (T,)) or T_ref < T:
            raise ValueError("mc_run_plants: inconsistent shapes")
    kind, models, substeps = _family_models("mc_run_plants", plant, h.nx, h.nu, B)
    x0c = None if x0 is None else c(x0).reshape(B, h.nx)
    sets = [v for P, dim in ((Z, h.nx), (X, h.nx), (U, h.nu)) for v in _check_set(P, dim, "mc_run_plants")]
    out = dict(err2=np.empty(B), tube_violations=np.empty(B, np.int32), x_violations=np.empty(B, np.int32), u_violations=np.empty(B, np.int32),
               not_optimal=np.empty(B, np.int32), x_final=np.empty((B, h.nx)), consistent=np.empty(B), iters_sum=np.empty(B, np.int32))
    cart = kind == PLANT_KIND["cartpole"]
    if cart:
        out["err2_physics"] = np.empty(B)
    mc_set_channel(h, ch_par)            # (as in mc_run: last)
    rc = lib().tmpc_mc_run_plants(h.ptr, B, T, int(bool(extended)), kind, models.ctypes.data, substeps, ptr(p_loss), ptr(ref), ptr(th_u), ptr(ga_u),
                                  ptr(w), ptr(x0c), *[ptr(a) if isinstance(a, np.ndarray) or a is None else a for a in sets],
                                  *[ptr(out[k]) for k in ("err2", "tube_violations", "x_violations", "u_violations", "not_optimal", "x_final",
                                                          "consistent", "iters_sum")], ptr(out.get("err2_physics")))
    if rc != 0:
        msg = h.error()
        mc_set_channel(h, None)          # a refused loop leaves no channel behind
        raise RuntimeError(f"tmpc_mc_run_plants failed ({rc}): {msg}")
    if cart:
        out["tracking_error_physics"] = np.sqrt(out["err2_physics"]) / (T * substeps)
    return _tracking_result(h, out, B, T, T, int(lib().tmpc_mc_last_fused(h.ptr)), capture, timing, series, law)


def mc_open(h: Handle, p_loss, ref, th_u=None, ga_u=None, x0=None, T=None, Z=None, X=None, U=None, extended: bool = False,
            warm_start: bool = False, capture=None, timing: bool = False, device_rng=None, ref_id=None, channel=None,
            series: bool = False, law=None) -> dict:
    """include/tmpc.h: tmpc_mc_open -- opens the stepped closed loop around a plant of the caller's.  p_loss (B,), ref (T,)
    or a full-state form (mc_run; (nx,) together with T: a constant full state -- the table of a session steered by ref_next),
    th_u / ga_u (B, T) loss uniforms (None with device_rng = (seed, first_trajectory[, ignored]): Philox block 0, the draws of
    mc_run), x0 (B, nx) or None; T: steps the session may take (default: len(ref)); Z / X / U: tube cross-section and the check
    sets for x_t / u_t (polytopes or None).  No disturbance is drawn: w is the plant's.  channel: the Gilbert-Elliott loss channel of
    the session (mc_run; p_loss may then be None).  series: the session keeps its per-step record (mc_run), which mc_close returns.
    law: the session's steps go through the explicit law (mc_run); mc_close returns its counters and miss log.
    Returns what mc_close needs."""
    c, ptr = _contiguous, _ptr
    p_loss, ch_par, B = loop_batch("mc_open", p_loss, channel, None if device_rng is not None else th_u, x0, ref_id, h.nx)
    if p_loss is not None:
        p_loss = p_loss.reshape(-1)
        B = p_loss.shape[0]
    ref, T_ref = _loop_reference(h, "mc_open", ref, B, T, ref_id, flatten_legacy=True)
    T = T_ref if T is None else int(T)
    if (ref.shape[0] if ref is not None else T_ref) < T:
        raise ValueError("mc_open: ref must cover the T steps of the session")
    _set_loop_options(h, timing, warm_start, capture, series=series, law=law)
    _set_device_rng(h, device_rng, draws_w=False)
    if device_rng is not None:
        th_u = ga_u = None
    else:
        th_u, ga_u = c(th_u), c(ga_u)
        if th_u.shape != (B, T) or ga_u.shape != (B, T):
            raise ValueError(f"mc_open: th_u and ga_u must be (B, T) = {(B, T)}")
    x0c = None if x0 is None else c(x0).reshape(B, h.nx)
    HZ, hZ, rZ = _check_set(Z, h.nx, "mc_open")
    HX, hX, rX = _check_set(X, h.nx, "mc_open")
    HU, hU, rU = _check_set(U, h.nu, "mc_open")
    mc_set_channel(h, ch_par)            # (as in mc_run: last)
    rc = lib().tmpc_mc_open(h.ptr, B, T, int(bool(extended)), ptr(p_loss), ptr(ref), ptr(th_u), ptr(ga_u), ptr(x0c),
                            ptr(HZ), ptr(hZ), rZ, ptr(HX), ptr(hX), rX, ptr(HU), ptr(hU), rU)
    if rc != 0:
        msg = h.error()
        mc_set_channel(h, None)          # (no session was opened: the setter is free)
        raise RuntimeError(f"tmpc_mc_open failed ({rc}): {msg}")
    return dict(B=B, T=T, capture=capture, timing=bool(timing), full_ref=ref is None, series=bool(series), law=law)


def mc_step(h: Handle, info: dict, x, u=None, stream=None, ref_next=None):
    """One step of the open session `info` = mc_open(...) describes.  x, u numpy (B, nx) / (B, nu): tmpc_mc_step, returns u when
    u_t is in place.  x, u integers: DEVICE addresses of B * nx / B * nu doubles for tmpc_mc_step_device, with `stream` the
    caller's hipStream_t as an integer (None / 0: the caller synchronises on both sides); returns without synchronising.
    ref_next (sessions opened with a full-state reference): the reference of the NEXT solve, (B, nx) numpy with numpy x, a device
    address with a device x (tmpc_mc_step_ref / tmpc_mc_step_device_ref); None: the next row of the schedule."""
    if ref_next is not None and not info.get("full_ref", True):
        raise RuntimeError("mc_step: ref_next needs a session opened with a full-state reference (a reference table: the (nx,) + T, "
                           "(T, nx), (B, T, nx) or (K, T, nx) forms of `ref`)")
    call = "tmpc_mc_step"
    if isinstance(x, np.ndarray):
        B = info["B"]
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.size != B * h.nx:           # (the library copies B * nx entries out of x)
            raise ValueError(f"mc_step: x must hold B * nx = {B * h.nx} entries, got {x.size}")
        if u is None:
            u = np.empty((B, h.nu))
        if not (isinstance(u, np.ndarray) and u.dtype == np.float64 and u.flags.c_contiguous and u.size == B * h.nu):
            raise ValueError("mc_step: u must be a contiguous float64 array of B * nu entries")
        if ref_next is None:
            rc = lib().tmpc_mc_step(h.ptr, x.ctypes.data, u.ctypes.data)
        else:
            r = np.ascontiguousarray(ref_next, dtype=np.float64)
            if r.size != B * h.nx:
                raise ValueError(f"mc_step: ref_next must hold B * nx = {B * h.nx} entries, got {r.size}")
            call = "tmpc_mc_step_ref"
            rc = lib().tmpc_mc_step_ref(h.ptr, x.ctypes.data, u.ctypes.data, r.ctypes.data)
    elif ref_next is None:
        call = "tmpc_mc_step_device"
        rc = lib().tmpc_mc_step_device(h.ptr, int(x), int(u), int(stream) if stream else None)
    else:
        call = "tmpc_mc_step_device_ref"
        rc = lib().tmpc_mc_step_device_ref(h.ptr, int(x), int(u), int(ref_next), int(stream) if stream else None)
    if rc != 0:
        raise RuntimeError(f"{call} failed ({rc}): {h.error()}")
    return u


def mc_close(h: Handle, info: dict) -> dict:
    """include/tmpc.h: tmpc_mc_close -- ends the session `info` = mc_open(...) describes and returns its statistics over the
    steps taken: the keys of mc_run (without x_final: the caller has it) plus x_violations, u_violations, steps."""
    B, T = info["B"], info["T"]
    out = dict(err2=np.empty(B), tube_violations=np.empty(B, np.int32), x_violations=np.empty(B, np.int32),
               u_violations=np.empty(B, np.int32), not_optimal=np.empty(B, np.int32), consistent=np.empty(B),
               iters_sum=np.empty(B, np.int32))
    steps = C.c_int32(0)
    rc = lib().tmpc_mc_close(h.ptr, *[out[k].ctypes.data for k in ("err2", "tube_violations", "x_violations", "u_violations",
                                                                   "not_optimal", "consistent", "iters_sum")], C.addressof(steps))
    if rc != 0:
        raise RuntimeError(f"tmpc_mc_close failed ({rc}): {h.error()}")
    out["steps"] = int(steps.value)
    return _tracking_result(h, out, B, T, out["steps"], 0, info.get("capture"), info.get("timing"), info.get("series", False), info.get("law"))


def reg_run(h: Handle, x0, T: int, w=None, device_rng=None, X=None, U=None, Z=None, capture=None, plant=None) -> dict:
    """include/tmpc.h: tmpc_reg_run -- the closed loop of a regulator handle on the device.  x0 (B, nx); w (B, T, nx) or None;
    device_rng = (seed, first_trajectory, w_bound): w drawn on the device (tmpc_mc_set_device_rng; the w of
    montecarlo.draw_realisations_philox); neither: no disturbance.  X, U, Z: check sets (polytopes) or None.  capture: index of
    a trajectory whose x_traj (T+1, nx), x_nom_traj (T, nx), u_traj (T, nu) are returned.  plant: None -- the model's (A, B); or a
    linear montecarlo.PlantFamily, a plant per trajectory (tmpc_mc_set_plant_models)."""
    c, ptr = _contiguous, _ptr
    if plant is not None and getattr(plant, "kind", None) != "linear":
        raise ValueError("reg_run: plant is None or a linear plant family")
    mc_set_plant_models(h, "linear", None if plant is None else plant.models)      # (None clears what an earlier call left)
    x0 = c(x0).reshape(-1, h.nx)
    B, T = x0.shape[0], int(T)
    if w is not None:
        w = c(w)
        if w.shape != (B, T, h.nx):
            raise ValueError(f"reg_run: w must be (B, T, nx) = {(B, T, h.nx)}, got {w.shape}")
    _set_device_rng(h, None if w is not None else device_rng)
    sets = [v for P, dim in ((X, h.nx), (U, h.nu), (Z, h.nx)) for v in _check_set(P, dim, "reg_run")]
    out = dict(cost=np.empty(B), x_viol=np.empty(B, np.int32), u_viol=np.empty(B, np.int32), tube_viol=np.empty(B, np.int32),
               not_optimal=np.empty(B, np.int32), fail_step=np.empty(B, np.int32), x_final=np.empty((B, h.nx)),
               iters_sum=np.empty(B, np.int32))
    cap = -1 if capture is None else int(capture)
    cx, cxn, cu = (np.empty((T + 1, h.nx)), np.empty((T, h.nx)), np.empty((T, h.nu))) if cap >= 0 else (None, None, None)
    args = [ptr(a) if isinstance(a, np.ndarray) or a is None else a for a in sets]
    rc = lib().tmpc_reg_run(h.ptr, B, T, ptr(x0), ptr(w), *args, ptr(out["cost"]), ptr(out["x_viol"]), ptr(out["u_viol"]),
                            ptr(out["tube_viol"]), ptr(out["not_optimal"]), ptr(out["fail_step"]), ptr(out["x_final"]),
                            ptr(out["iters_sum"]), cap, ptr(cx), ptr(cxn), ptr(cu))
    if rc != 0:
        raise RuntimeError(f"tmpc_reg_run failed ({rc}): {h.error()}")
    if cap >= 0:
        out["x_traj"], out["x_nom_traj"], out["u_traj"] = cx, cxn, cu
    return out


def mc_replay(h: Handle, U, theta, gamma, w, xn0=None, x0=None, extended: bool = False, smart: bool = False) -> dict:
    """include/tmpc.h: tmpc_mc_replay -- the device-side estimator / actuator state machines driven by GIVEN controller
    packets (no QP is solved).  U (B, T, N+1, nu): packets, terminal column last; theta, gamma (B, T): arrival flags;
    w (B, T, nx); xn0 (B, T, nx) for the extended controller.  Returns per step x (state after the step), x_hat (estimate
    after the step), x_nom (nominal state in the plant's packet), u (applied input), s, Theta, q."""
    c, ptr = _contiguous, _ptr
    U, w = c(U), c(w)
    B, T = U.shape[:2]
    if U.shape != (B, T, h.N + 1, h.nu) or w.shape != (B, T, h.nx):
        raise ValueError("mc_replay: inconsistent shapes")
    th = np.ascontiguousarray(np.asarray(theta).reshape(B, T) != 0, dtype=np.uint8)
    ga = np.ascontiguousarray(np.asarray(gamma).reshape(B, T) != 0, dtype=np.uint8)
    xn0c = None if xn0 is None else c(xn0).reshape(B, T, h.nx)
    x0c = None if x0 is None else c(x0).reshape(B, h.nx)
    tf = np.empty((B, T, 3 * h.nx + h.nu))
    ti = np.empty((B, T, 3), np.int32)
    mc_set_actuator(h, smart)
    try:
        rc = lib().tmpc_mc_replay(h.ptr, B, T, int(bool(extended)), ptr(U), ptr(xn0c), ptr(th), ptr(ga), ptr(w), ptr(x0c), ptr(tf), ptr(ti))
    finally:
        mc_set_actuator(h, False)
    if rc != 0:
        raise RuntimeError(f"tmpc_mc_replay failed ({rc}): {h.error()}")
    nx = h.nx
    return dict(x=tf[:, :, :nx], x_hat=tf[:, :, nx:2 * nx], x_nom=tf[:, :, 2 * nx:3 * nx], u=tf[:, :, 3 * nx:],
                s=ti[:, :, 0], Theta=ti[:, :, 1], q=ti[:, :, 2])


def lp_batch(H, h, Cmat, relax=None, relax_by: float = 1.0, device: int = 0, want_x: bool = False) -> dict:
    """Batch of support-function LPs over one polytope (include/tmpc.h: tmpc_lp_batch):
    val[b] = max Cmat[b] . x  s.t.  H x <= h, row relax[b] of h raised by relax_by."""
    L = lib()
    H = np.ascontiguousarray(H, dtype=np.float64)
    h = np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
    Cm = np.ascontiguousarray(np.atleast_2d(Cmat), dtype=np.float64)
    nr, d = H.shape
    if h.size != nr or Cm.shape[1] != d:
        raise ValueError("lp_batch: shapes of H (nr x d), h (nr), C (B x d) do not agree")
    B = Cm.shape[0]
    rel = None if relax is None else np.ascontiguousarray(relax, dtype=np.int32).reshape(-1)
    if rel is not None and rel.size != B:
        raise ValueError("lp_batch: relax needs one row index per objective")
    val = np.empty(B)
    x = np.empty((B, d)) if want_x else None
    st = np.empty(B, dtype=np.int32)
    it = np.empty(B, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.tmpc_lp_batch(int(device), d, nr, ptr(H), ptr(h), B, ptr(Cm), ptr(rel), float(relax_by),
                         ptr(val), ptr(x), ptr(st), ptr(it))
    if rc != 0:
        raise RuntimeError(f"tmpc_lp_batch failed ({rc}): {L.tmpc_last_error(None).decode()}")
    out = {"val": val, "status": st, "iters": it}
    if want_x:
        out["x"] = x
    return out


def order_statistics(data, ranks, device: int = 0) -> dict:
    """Exact order statistics of the columns of `data` (n x ncol, or n values), selected on the device (include/tmpc.h:
    tmpc_order_statistics): out[c, r] = numpy.partition(data[:, c], ranks[r])[ranks[r]] over the values that are not NaN (NaN where
    there are fewer); n_nonfinite[c] counts NaN and +-inf."""
    L = lib()
    d = np.asarray(data, dtype=np.float64)
    d = d.reshape(-1, 1) if d.ndim == 1 else d
    cols = np.ascontiguousarray(d.T)                      # column-major: one column after the other
    ncol, n = cols.shape
    rk = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
    out = np.empty((ncol, rk.size))
    nf = np.empty(ncol, dtype=np.int64)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.tmpc_order_statistics(int(device), n, ncol, ptr(cols), rk.size, ptr(rk), ptr(out), ptr(nf))
    if rc != 0:
        raise RuntimeError(f"tmpc_order_statistics failed ({rc}): {L.tmpc_last_error(None).decode()}")
    return {"order_stats": out, "n_nonfinite": nf}


PLANT_KIND = {None: 0, "linear": 0, "cartpole": 1}         # include/tmpc.h: TMPC_PLANT_*


def estimate_w(A, B, K, T: int, x0=None, x0_box=None, n_traj=None, seed: int = 0, first: int = 0, ranks=(), settle_tol: float = 1e-3,
               plant="cartpole", Th: float = 0.02, substeps: int = 10, device: int = 0, want_samples: bool = False, par=None) -> dict:
    """Closed loops u = -K x on the nonlinear plant, the samples w_k = x_k - (A - B K) x_{k-1} and their order statistics, all on the
    device (include/tmpc.h: tmpc_estimate_w).  Initial states: the array x0 (n_traj x nx), or drawn on the device from
    x0_box = (lo, hi) for trajectories first .. first + n_traj - 1 of the stream `seed`.  par: (n_traj, 7) rows {M, m, b, I, g, l, Th},
    a cart-pole per trajectory (tmpc_estimate_w_models), or None: workloads.CARTPOLE_PARAMS and Th for everybody."""
    from .workloads import CARTPOLE_PARAMS as P
    L = lib()
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    K = np.ascontiguousarray(K, dtype=np.float64)
    nx, nu = B.shape
    if A.shape != (nx, nx) or K.size != nu * nx:
        raise ValueError("estimate_w: shapes of A (nx x nx), B (nx x nu), K (nu x nx) do not agree")
    lo = hi = None
    if x0 is not None:
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, nx)
        n_traj = x0.shape[0]
    elif x0_box is not None and n_traj is not None:
        lo = np.ascontiguousarray(x0_box[0], dtype=np.float64).reshape(nx)
        hi = np.ascontiguousarray(x0_box[1], dtype=np.float64).reshape(nx)
    else:
        raise ValueError("estimate_w: give x0, or x0_box and n_traj")
    n_traj, T = int(n_traj), int(T)
    if plant not in PLANT_KIND:
        raise ValueError(f"unknown plant {plant!r}")
    par_traj = None
    if par is not None:
        par_traj = np.ascontiguousarray(par, dtype=np.float64)
        if par_traj.shape != (n_traj, 7):
            raise ValueError(f"estimate_w: par is (n_traj, 7) = {(n_traj, 7)}, got {par_traj.shape}")
    par = np.array([P["M"], P["m"], P["b"], P["I"], P["g"], P["l"], float(Th)])
    rk = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
    nper = max(T - 1, 0)
    stats = np.empty((nx, rk.size))
    wmin, wmax = np.empty(nx), np.empty(nx)
    nf = np.empty(nx, dtype=np.int64)
    ns, bad = C.c_int64(0), C.c_int64(0)
    worst = C.c_double(0.0)
    x0u = np.empty((max(n_traj, 0), nx))
    smp = np.empty((nx, nper, max(n_traj, 0))) if want_samples else None
    ms = (C.c_float * 2)()
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tail = (ptr(x0), ptr(lo), ptr(hi), int(seed), int(first), rk.size, ptr(rk), float(settle_tol),
            ptr(stats), ptr(wmin), ptr(wmax), C.cast(C.byref(ns), C.c_void_p), ptr(nf), C.cast(C.byref(bad), C.c_void_p),
            C.cast(C.byref(worst), C.c_void_p), ptr(x0u), ptr(smp), C.cast(ms, C.c_void_p))
    if par_traj is None:
        rc = L.tmpc_estimate_w(int(device), nx, nu, ptr(A), ptr(B), ptr(K), PLANT_KIND[plant], ptr(par), int(substeps), n_traj, T, *tail)
    else:
        rc = L.tmpc_estimate_w_models(int(device), nx, nu, ptr(A), ptr(B), ptr(K), PLANT_KIND[plant], ptr(par), ptr(par_traj), int(substeps),
                                      n_traj, T, *tail)
    if rc != 0:
        raise RuntimeError(f"tmpc_estimate_w failed ({rc}): {L.tmpc_last_error(None).decode()}")
    out = {"order_stats": stats, "w_min": wmin, "w_max": wmax, "n_samples": ns.value, "n_nonfinite": nf, "not_settled": bad.value,
           "x_final_norm_max": worst.value, "x0_used": x0u, "rollout_ms": float(ms[0]), "selection_ms": float(ms[1])}
    if want_samples:
        out["samples"] = smp
    return out


# ---- sensitivity of the solution (include/tmpc.h: tmpc_sens_*, tmpc_qp_sensitivity; csrc/tmpc_sens.hip)
SENS_SKIPPED, SENS_DEPENDENT, SENS_WEAK, SENS_NOT_KKT = 1, 2, 4, 8
_SENS_RC = {-1: ValueError, -2: NotImplementedError}


def _sens_fail(name: str, rc: int, msg: str):
    raise _SENS_RC.get(rc, RuntimeError)(f"{name} failed ({rc}): {msg}")


def sens_active_words(h: Handle) -> int:
    """Words per instance of the `active` output: ceil(nc_max / 32) over the handle's variants."""
    return (max(get_dims(h, k)[1] for k in range(h.nvariants)) + 31) // 32


def sens_get_model(h: Handle, variant: int = 0) -> dict:
    """include/tmpc.h: tmpc_sens_get_model -> F (nv, 2nx), Ebar (nc, 2nx), Y (ny, nv), Yp (ny, 2nx), Rec (nv, ny + 2nx)."""
    nv, nc, _ = get_dims(h, variant)
    ny, npar = h.N * h.nu + 2 * h.nx + h.nu, 2 * h.nx
    out = dict(F=np.zeros((nv, npar)), Ebar=np.zeros((nc, npar)), Y=np.zeros((ny, nv)), Yp=np.zeros((ny, npar)), Rec=np.zeros((nv, ny + npar)))
    rc = lib().tmpc_sens_get_model(h.ptr, int(variant), *[out[k].ctypes.data for k in ("F", "Ebar", "Y", "Yp", "Rec")])
    if rc != 0:
        _sens_fail("tmpc_sens_get_model", rc, h.error())
    return out


def _sens_inputs(h: Handle, x, ref, variant, sol: dict):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, h.nx))
    B = x.shape[0]
    ref = np.ascontiguousarray(np.broadcast_to(np.asarray(ref, dtype=np.float64).reshape(-1, h.nx), (B, h.nx)))
    var = None if variant is None else np.ascontiguousarray(np.broadcast_to(np.asarray(variant, dtype=np.uint8).reshape(-1), (B,)))
    u = np.ascontiguousarray(np.asarray(sol["u_nom"], dtype=np.float64).reshape(B, h.N * h.nu))
    x0 = np.ascontiguousarray(np.asarray(sol["x_nom0"], dtype=np.float64).reshape(B, h.nx))
    ss = np.ascontiguousarray(np.asarray(sol["xu_ss"], dtype=np.float64).reshape(B, h.nx + h.nu))
    st = None if sol.get("status") is None else np.ascontiguousarray(np.asarray(sol["status"], dtype=np.int32).reshape(B))
    return B, x, ref, var, u, x0, ss, st


def sens_jacobian(h: Handle, x, ref, sol: dict, variant=None, act_tol: float = 0.0) -> dict:
    """Host-pointer entry (tmpc_sens_jacobian): the Jacobians of y = [u_nom | x_nom0 | xu_ss] with respect to [x_k | ref] at the
    solutions `sol` (u_nom, x_nom0, xu_ss, status of a preceding solve) -> J (B, ny, 2nx), flag, n_active, active (B, words)."""
    B, x, ref, var, u, x0, ss, st = _sens_inputs(h, x, ref, variant, sol)
    ny = h.N * h.nu + 2 * h.nx + h.nu
    out = dict(J=np.empty((B, ny, 2 * h.nx)), flag=np.empty(B, np.int32), n_active=np.empty(B, np.int32),
               active=np.zeros((B, sens_active_words(h)), np.uint32))
    rc = lib().tmpc_sens_jacobian(h.ptr, B, x.ctypes.data, ref.ctypes.data, _ptr(var), u.ctypes.data, x0.ctypes.data, ss.ctypes.data, _ptr(st),
                                  float(act_tol), out["J"].ctypes.data, out["flag"].ctypes.data, out["n_active"].ctypes.data, out["active"].ctypes.data)
    if rc != 0:
        _sens_fail("tmpc_sens_jacobian", rc, h.error())
    return out


def sens_vjp(h: Handle, x, ref, sol: dict, ybar, variant=None, act_tol: float = 0.0) -> dict:
    """Host-pointer entry (tmpc_sens_vjp): pbar[b] = J_b' ybar[b] -> pbar (B, 2nx), flag, n_active."""
    B, x, ref, var, u, x0, ss, st = _sens_inputs(h, x, ref, variant, sol)
    ny = h.N * h.nu + 2 * h.nx + h.nu
    ybar = np.ascontiguousarray(np.asarray(ybar, dtype=np.float64).reshape(B, ny))
    out = dict(pbar=np.empty((B, 2 * h.nx)), flag=np.empty(B, np.int32), n_active=np.empty(B, np.int32))
    rc = lib().tmpc_sens_vjp(h.ptr, B, x.ctypes.data, ref.ctypes.data, _ptr(var), u.ctypes.data, x0.ctypes.data, ss.ctypes.data, _ptr(st),
                             float(act_tol), ybar.ctypes.data, out["pbar"].ctypes.data, out["flag"].ctypes.data, out["n_active"].ctypes.data)
    if rc != 0:
        _sens_fail("tmpc_sens_vjp", rc, h.error())
    return out


def sens_jacobian_device(h: Handle, B: int, x_ptr, r_ptr, var_ptr, u_ptr, x0_ptr, ss_ptr, st_ptr, act_tol, J_ptr, flag_ptr, nact_ptr, act_ptr):
    """Device-pointer entry (tmpc_sens_jacobian_device): raw addresses; returns without synchronising."""
    rc = lib().tmpc_sens_jacobian_device(h.ptr, int(B), x_ptr, r_ptr, var_ptr, u_ptr, x0_ptr, ss_ptr, st_ptr, float(act_tol), J_ptr, flag_ptr, nact_ptr, act_ptr)
    if rc != 0:
        _sens_fail("tmpc_sens_jacobian_device", rc, h.error())


def sens_vjp_device(h: Handle, B: int, x_ptr, r_ptr, var_ptr, u_ptr, x0_ptr, ss_ptr, st_ptr, act_tol, ybar_ptr, pbar_ptr, flag_ptr, nact_ptr):
    """Device-pointer entry (tmpc_sens_vjp_device): raw addresses; returns without synchronising."""
    rc = lib().tmpc_sens_vjp_device(h.ptr, int(B), x_ptr, r_ptr, var_ptr, u_ptr, x0_ptr, ss_ptr, st_ptr, float(act_tol), ybar_ptr, pbar_ptr, flag_ptr, nact_ptr)
    if rc != 0:
        _sens_fail("tmpc_sens_vjp_device", rc, h.error())


def qp_sensitivity(H, F, G, g0, Ebar, Y, Yp, P, Z, status=None, act_tol: float = 0.0, mode: str = "jacobian", ybar=None, device: int = 0) -> dict:
    """include/tmpc.h: tmpc_qp_sensitivity -- the sensitivity kernel on raw condensed data, without a handle; arguments and result as
    LinearMPCOverNetworks.sensitivity.qp_sensitivity, its numpy twin (without `lam`)."""
    H, F, G, g0, Ebar, Y, Yp = (_contiguous(a) for a in (H, F, G, g0, Ebar, Y, Yp))
    nv, npar = F.shape
    nc, ny = g0.shape[0], Y.shape[0]
    P = _contiguous(P).reshape(-1, npar)
    Z = _contiguous(Z).reshape(-1, nv)
    B = P.shape[0]
    vjp = mode == "vjp"
    st = None if status is None else np.ascontiguousarray(np.asarray(status, dtype=np.int32).reshape(B))
    yb = _contiguous(ybar).reshape(B, ny) if vjp else None
    out = dict(out=np.empty((B, npar) if vjp else (B, ny, npar)), flag=np.empty(B, np.int32), n_active=np.empty(B, np.int32),
               active=np.zeros((B, (nc + 31) // 32), np.uint32))
    rc = lib().tmpc_qp_sensitivity(int(device), nv, nc, npar, ny, H.ctypes.data, F.ctypes.data, G.ctypes.data if nc else None,
                                   g0.ctypes.data if nc else None, Ebar.ctypes.data if nc else None, Y.ctypes.data, Yp.ctypes.data, B,
                                   P.ctypes.data, Z.ctypes.data, _ptr(st), float(act_tol), 1 if vjp else 0, _ptr(yb), out["out"].ctypes.data,
                                   out["flag"].ctypes.data, out["n_active"].ctypes.data, out["active"].ctypes.data if nc else None)
    if rc != 0:
        _sens_fail("tmpc_qp_sensitivity", rc, lib().tmpc_last_error(None).decode())
    return out


# ---- gradients with respect to the weights Q, R, P, T (include/tmpc.h: tmpc_sens_vjp_weights*, tmpc_sens_weight_map, tmpc_qp_sensitivity_data)
def _weight_outputs(h: Handle) -> dict:
    return dict(Qbar=np.empty((h.nx, h.nx)), Rbar=np.empty((h.nu, h.nu)), Pbar=np.empty((h.nx, h.nx)), Tbar=np.empty((h.nx, h.nx)))


def sens_vjp_weights(h: Handle, x, ref, sol: dict, ybar, variant=None, act_tol: float = 0.0) -> dict:
    """Host-pointer entry (tmpc_sens_vjp_weights): the vector-Jacobian products of tmpc_sens_vjp and the gradients of the same scalar with
    respect to the four weights, summed over the batch -> pbar (B, 2nx), Qbar, Rbar, Pbar, Tbar (symmetric), flag, n_active."""
    B, x, ref, var, u, x0, ss, st = _sens_inputs(h, x, ref, variant, sol)
    ny = h.N * h.nu + 2 * h.nx + h.nu
    ybar = np.ascontiguousarray(np.asarray(ybar, dtype=np.float64).reshape(B, ny))
    out = dict(pbar=np.empty((B, 2 * h.nx)), flag=np.empty(B, np.int32), n_active=np.empty(B, np.int32), **_weight_outputs(h))
    rc = lib().tmpc_sens_vjp_weights(h.ptr, B, x.ctypes.data, ref.ctypes.data, _ptr(var), u.ctypes.data, x0.ctypes.data, ss.ctypes.data, _ptr(st),
                                     float(act_tol), ybar.ctypes.data, out["pbar"].ctypes.data, out["Qbar"].ctypes.data, out["Rbar"].ctypes.data,
                                     out["Pbar"].ctypes.data, out["Tbar"].ctypes.data, out["flag"].ctypes.data, out["n_active"].ctypes.data)
    if rc != 0:
        _sens_fail("tmpc_sens_vjp_weights", rc, h.error())
    return out


def sens_vjp_weights_device(h: Handle, B: int, x_ptr, r_ptr, var_ptr, u_ptr, x0_ptr, ss_ptr, st_ptr, act_tol, ybar_ptr, pbar_ptr, flag_ptr, nact_ptr) -> dict:
    """Device-pointer entry (tmpc_sens_vjp_weights_device): raw addresses for the per-instance arrays; the four gradients are numpy arrays
    on the host.  Returns them once they are in place: the call has synchronised its own launch lane, pbar / flag / n_active are complete."""
    out = _weight_outputs(h)
    rc = lib().tmpc_sens_vjp_weights_device(h.ptr, int(B), x_ptr, r_ptr, var_ptr, u_ptr, x0_ptr, ss_ptr, st_ptr, float(act_tol), ybar_ptr, pbar_ptr,
                                            out["Qbar"].ctypes.data, out["Rbar"].ctypes.data, out["Pbar"].ctypes.data, out["Tbar"].ctypes.data,
                                            flag_ptr, nact_ptr)
    if rc != 0:
        _sens_fail("tmpc_sens_vjp_weights_device", rc, h.error())
    return out


def sens_weight_map(h: Handle, Hbar, Fbar, variant: int = 0) -> dict:
    """include/tmpc.h: tmpc_sens_weight_map -- the adjoint of the condensing's cost assembly on the host (works on a host-only handle):
    Hbar (nv, nv), Fbar (nv, 2nx) -> Qbar, Rbar, Pbar, Tbar (symmetric)."""
    nv = get_dims(h, variant)[0]
    Hbar = _contiguous(Hbar).reshape(nv, nv)
    Fbar = _contiguous(Fbar).reshape(nv, 2 * h.nx)
    out = _weight_outputs(h)
    rc = lib().tmpc_sens_weight_map(h.ptr, int(variant), Hbar.ctypes.data, Fbar.ctypes.data, *[out[k].ctypes.data for k in ("Qbar", "Rbar", "Pbar", "Tbar")])
    if rc != 0:
        _sens_fail("tmpc_sens_weight_map", rc, h.error())
    return out


def qp_sensitivity_data(H, F, G, g0, Ebar, Y, Yp, P, Z, ybar, status=None, act_tol: float = 0.0, device: int = 0) -> dict:
    """include/tmpc.h: tmpc_qp_sensitivity_data -- the reverse mode on raw condensed data with the gradients with respect to H and F, summed
    over the batch; arguments and result as LinearMPCOverNetworks.sensitivity.qp_sensitivity_data, its numpy twin:
    -> pbar (B, np), Hbar (nv, nv), Fbar (nv, np), adj (B, nv), flag, n_active."""
    H, F, G, g0, Ebar, Y, Yp = (_contiguous(a) for a in (H, F, G, g0, Ebar, Y, Yp))
    nv, npar = F.shape
    nc, ny = g0.shape[0], Y.shape[0]
    P = _contiguous(P).reshape(-1, npar)
    Z = _contiguous(Z).reshape(-1, nv)
    B = P.shape[0]
    st = None if status is None else np.ascontiguousarray(np.asarray(status, dtype=np.int32).reshape(B))
    yb = _contiguous(ybar).reshape(B, ny)
    out = dict(pbar=np.empty((B, npar)), Hbar=np.empty((nv, nv)), Fbar=np.empty((nv, npar)), adj=np.empty((B, nv)), flag=np.empty(B, np.int32),
               n_active=np.empty(B, np.int32))
    rc = lib().tmpc_qp_sensitivity_data(int(device), nv, nc, npar, ny, H.ctypes.data, F.ctypes.data, G.ctypes.data if nc else None,
                                        g0.ctypes.data if nc else None, Ebar.ctypes.data if nc else None, Y.ctypes.data, Yp.ctypes.data, B,
                                        P.ctypes.data, Z.ctypes.data, _ptr(st), float(act_tol), yb.ctypes.data, out["pbar"].ctypes.data,
                                        out["Hbar"].ctypes.data, out["Fbar"].ctypes.data, out["adj"].ctypes.data, out["flag"].ctypes.data,
                                        out["n_active"].ctypes.data)
    if rc != 0:
        _sens_fail("tmpc_qp_sensitivity_data", rc, lib().tmpc_last_error(None).decode())
    return out


# ---- the explicit control law (include/tmpc.h: tmpc_law_*, tmpc_qp_law_eval; csrc/tmpc_law.hip)
LAW_FEAS_TOL, LAW_MULT_TOL = 1e-10, 1e-10      # include/tmpc.h: TMPC_LAW_*_TOL; csrc/tmpc_law.hpp


def _law_check(name: str, rc: int, h: Handle = None):
    if rc != 0:
        _sens_fail(name, rc, h.error() if h is not None else lib().tmpc_last_error(None).decode())


def get_param_rows(h: Handle, variant: int = 0) -> dict:
    """include/tmpc.h: tmpc_get_param_rows -> gp0 (npar,), Ep (npar, nx): the rows 0 <= gp0 + Ep x_k."""
    npar = get_dims(h, variant)[2]
    out = dict(gp0=np.zeros(npar), Ep=np.zeros((npar, h.nx)))
    _law_check("tmpc_get_param_rows", lib().tmpc_get_param_rows(h.ptr, int(variant), out["gp0"].ctypes.data, out["Ep"].ctypes.data), h)
    return out


def law_add(h: Handle, words, variant: int = 0):
    """include/tmpc.h: tmpc_law_add -- words (n, ceil(nc / 32)) uint32 -> the region ids (n,), -1 for a refused set."""
    nw = (get_dims(h, variant)[1] + 31) // 32
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32).reshape(-1, nw) if nw else np.zeros((len(words), 0), np.uint32))
    ids = np.full(w.shape[0], -1, np.int32)
    _law_check("tmpc_law_add", lib().tmpc_law_add(h.ptr, int(variant), w.shape[0], w.ctypes.data if w.size else ids.ctypes.data, ids.ctypes.data), h)
    return ids


def law_learn(h: Handle, x, ref, sol: dict, variant=None, act_tol: float = 0.0):
    """include/tmpc.h: tmpc_law_learn -- the working sets of the solutions `sol` of a preceding solve -> (ids (B,), number of new regions)."""
    B, x, ref, var, u, x0, ss, st = _sens_inputs(h, x, ref, variant, sol)
    ids, n_new = np.full(B, -1, np.int32), C.c_int64(0)
    rc = lib().tmpc_law_learn(h.ptr, B, x.ctypes.data, ref.ctypes.data, _ptr(var), u.ctypes.data, x0.ctypes.data, ss.ctypes.data, _ptr(st), float(act_tol),
                              ids.ctypes.data, C.addressof(n_new))
    _law_check("tmpc_law_learn", rc, h)
    return ids, int(n_new.value)


def _law_call(name: str, h: Handle, x, ref, variant, hint, max_tries: int, want_traj: bool) -> dict:
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, h.nx))
    B, nx, nu, N = x.shape[0], h.nx, h.nu, h.N
    ref = np.ascontiguousarray(np.broadcast_to(np.asarray(ref, dtype=np.float64).reshape(-1, nx), (B, nx)))
    var = None if variant is None else np.ascontiguousarray(np.broadcast_to(np.asarray(variant, dtype=np.uint8).reshape(-1), (B,)))
    hint = None if hint is None else np.ascontiguousarray(np.broadcast_to(np.asarray(hint, dtype=np.int32).reshape(-1), (B,)))
    out = dict(u_nom=np.empty((B, N, nu)), x_nom0=np.empty((B, nx)), xu_ss=np.empty((B, nx + nu)), x_nom=np.empty((B, N + 1, nx)) if want_traj else None,
               status=np.empty(B, np.int32), iters=np.empty(B, np.int32), region=np.empty(B, np.int32), tries=np.empty(B, np.int32))
    rc = getattr(lib(), name)(h.ptr, B, x.ctypes.data, ref.ctypes.data, _ptr(var), _ptr(hint), int(max_tries),
                              *[_ptr(out[k]) for k in ("u_nom", "x_nom0", "xu_ss", "x_nom", "status", "iters", "region", "tries")])
    _law_check(name, rc, h)
    out["x_ss"], out["u_ss"] = out["xu_ss"][:, :nx], out["xu_ss"][:, nx:]
    return out


def law_eval(h: Handle, x, ref, variant=None, hint=None, max_tries: int = 0, want_traj: bool = True) -> dict:
    """Host-pointer entry (tmpc_law_eval): the law kernel alone -> the outputs of solve_batch plus region, tries; a miss is NaN, status 3."""
    return _law_call("tmpc_law_eval", h, x, ref, variant, hint, max_tries, want_traj)


def law_solve(h: Handle, x, ref, variant=None, hint=None, max_tries: int = 0, want_traj: bool = True) -> dict:
    """Host-pointer entry (tmpc_law_solve): the law, and the handle's solve for the misses, in one call."""
    return _law_call("tmpc_law_solve", h, x, ref, variant, hint, max_tries, want_traj)


def _law_device(name: str, h: Handle, B: int, ptrs):
    x, r, var, hint, max_tries = ptrs[:5]
    _law_check(name, getattr(lib(), name)(h.ptr, int(B), x, r, var, hint, int(max_tries), *ptrs[5:]), h)


def law_eval_device(h: Handle, B: int, x_ptr, r_ptr, var_ptr, hint_ptr, max_tries, u_ptr, x0_ptr, ss_ptr, xn_ptr, st_ptr, it_ptr, region_ptr, tries_ptr):
    """Device-pointer entry (tmpc_law_eval_device): raw addresses; returns without synchronising."""
    _law_device("tmpc_law_eval_device", h, B, (x_ptr, r_ptr, var_ptr, hint_ptr, max_tries, u_ptr, x0_ptr, ss_ptr, xn_ptr, st_ptr, it_ptr, region_ptr, tries_ptr))


def law_solve_device(h: Handle, B: int, x_ptr, r_ptr, var_ptr, hint_ptr, max_tries, u_ptr, x0_ptr, ss_ptr, xn_ptr, st_ptr, it_ptr, region_ptr, tries_ptr):
    """Device-pointer entry (tmpc_law_solve_device): raw addresses; returns without synchronising."""
    _law_device("tmpc_law_solve_device", h, B, (x_ptr, r_ptr, var_ptr, hint_ptr, max_tries, u_ptr, x0_ptr, ss_ptr, xn_ptr, st_ptr, it_ptr, region_ptr, tries_ptr))


def law_stats(h: Handle, variant: int = 0):
    """include/tmpc.h: tmpc_law_get_stats -> the hit counters (R,) int64."""
    R = C.c_int32(0)
    _law_check("tmpc_law_get_stats", lib().tmpc_law_get_stats(h.ptr, int(variant), C.addressof(R), None), h)
    hits = np.zeros(R.value, np.int64)
    if R.value:
        _law_check("tmpc_law_get_stats", lib().tmpc_law_get_stats(h.ptr, int(variant), None, hits.ctypes.data), h)
    return hits


def law_reorder(h: Handle, variant: int = 0):
    _law_check("tmpc_law_reorder", lib().tmpc_law_reorder(h.ptr, int(variant)), h)


def law_clear(h: Handle, variant: int = 0):
    _law_check("tmpc_law_clear", lib().tmpc_law_clear(h.ptr, int(variant)), h)


def law_get_region(h: Handle, i: int, variant: int = 0) -> dict:
    """include/tmpc.h: tmpc_law_get_region -> words, Ky (ny, 2nx), ky (ny,), S (nrow, 2nx), s (nrow,) as uploaded."""
    _, nc, npar = get_dims(h, variant)
    ny, npp, nrow = h.N * h.nu + 2 * h.nx + h.nu, 2 * h.nx, nc + npar
    out = dict(words=np.zeros((nc + 31) // 32, np.uint32), Ky=np.zeros((ny, npp)), ky=np.zeros(ny), S=np.zeros((nrow, npp)), s=np.zeros(nrow))
    rc = lib().tmpc_law_get_region(h.ptr, int(variant), int(i), *[_ptr(out[k]) for k in ("words", "Ky", "ky", "S", "s")])
    _law_check("tmpc_law_get_region", rc, h)
    return out


def law_set_hops(h: Handle, max_hops: int):
    """include/tmpc.h: tmpc_law_set_hops -- the handle-wide bound of the hops of a search (0: none)."""
    _law_check("tmpc_law_set_hops", lib().tmpc_law_set_hops(h.ptr, int(max_hops)), h)


def law_get_hops(h: Handle) -> int:
    n = C.c_int(0)
    _law_check("tmpc_law_get_hops", lib().tmpc_law_get_hops(h.ptr, C.addressof(n)), h)
    return int(n.value)


HOP_STATS = ("chain_hits", "chain_tests", "ended_absent", "ended_cap", "ended_cycle", "ended_param_row")


def law_hop_stats(h: Handle, variant: int = 0, clear: bool = False):
    """include/tmpc.h: tmpc_law_get_hop_stats -> the six counters (6,) int64, in the order of HOP_STATS; clear: tmpc_law_clear_hop_stats after."""
    st = np.zeros(6, np.int64)
    _law_check("tmpc_law_get_hop_stats", lib().tmpc_law_get_hop_stats(h.ptr, int(variant), st.ctypes.data), h)
    if clear:
        _law_check("tmpc_law_clear_hop_stats", lib().tmpc_law_clear_hop_stats(h.ptr, int(variant)), h)
    return st


def law_find_key(h: Handle, key: int, variant: int = 0) -> int:
    """include/tmpc.h: tmpc_law_find_key -> the id stored under the key (explicit_law.signature_key) in the table's hash, or -1."""
    i = C.c_int32(-1)
    _law_check("tmpc_law_find_key", lib().tmpc_law_find_key(h.ptr, int(variant), C.c_uint64(int(key)), C.addressof(i)), h)
    return int(i.value)


def qp_law_eval(H, F, G, g0, Ebar, Y, Yp, words, order, P, hint=None, max_tries: int = 0, device: int = 0, max_hops=None, want_stats: bool = False) -> dict:
    """include/tmpc.h: tmpc_qp_law_eval -- the law kernel on raw condensed data, without a handle -> y (B, ny), region, tries; arguments as
    LinearMPCOverNetworks.explicit_law.locate on a table of region_law(model, decode(words[i])).  max_hops not None: tmpc_qp_law_eval_hops,
    with want_stats the six counters as `stats` (6,) int64."""
    H, F, G, g0, Ebar, Y, Yp = (_contiguous(a) for a in (H, F, G, g0, Ebar, Y, Yp))
    nv, npar = F.shape
    nc, ny = g0.shape[0], Y.shape[0]
    nw = (nc + 31) // 32
    words = np.ascontiguousarray(np.asarray(words, dtype=np.uint32).reshape(-1, nw) if nw else np.zeros((len(words), 0), np.uint32))
    order = np.ascontiguousarray(np.asarray(order, dtype=np.int32).reshape(-1))
    P = _contiguous(P).reshape(-1, npar)
    B = P.shape[0]
    hint = None if hint is None else np.ascontiguousarray(np.broadcast_to(np.asarray(hint, dtype=np.int32).reshape(-1), (B,)))
    out = dict(y=np.empty((B, ny)), region=np.empty(B, np.int32), tries=np.empty(B, np.int32))
    args = (int(device), nv, nc, npar, ny, H.ctypes.data, F.ctypes.data, G.ctypes.data if nc else None, g0.ctypes.data if nc else None,
            Ebar.ctypes.data if nc else None, Y.ctypes.data, Yp.ctypes.data, words.shape[0], words.ctypes.data if words.size else None,
            order.shape[0], order.ctypes.data if order.size else None, B, P.ctypes.data, _ptr(hint), int(max_tries),
            out["y"].ctypes.data, out["region"].ctypes.data, out["tries"].ctypes.data)
    if max_hops is None:
        _law_check("tmpc_qp_law_eval", lib().tmpc_qp_law_eval(*args))
    else:
        if want_stats:
            out["stats"] = np.zeros(6, np.int64)
        _law_check("tmpc_qp_law_eval_hops", lib().tmpc_qp_law_eval_hops(*args, int(max_hops), out["stats"].ctypes.data if want_stats else None))
    return out
