"""ctypes binding of the C ABI (include/autogp_hip.h) + the call sites of the reference that
it replaces, under the reference's own names:

  compute_cov_matrix_vectorized(node, noise, ts)          src/GP.jl:666-668
  eval_cov(node, ts)                                      src/GP.jl:54-61
  mvnormal_logpdf / GPEngine.logpdf_batch                 src/Model.jl:134-136 (xs ~ mvnormal(0, K))
  MvNormal(node, noise, ts, xs, ts_pred; noise_pred, mean) src/GP.jl:731-758
  quantile(dist, p)                                       src/GP.jl:1006-1012

There is NO CPU fallback: if the HIP library is missing, or no gfx950 device is visible,
construction raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import gp as _gp

_PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = _PKG_DIR / "lib" / "libautogp_hip.so"

EXPORTED_SYMBOLS = [
    "agp_init", "agp_destroy", "agp_last_error", "agp_version", "agp_set_data", "agp_logpdf",
    "agp_logpdf_batch", "agp_logpdf_grad_batch", "agp_logpdf_grad", "agp_logpdf_batch_device", "agp_predict_batch", "agp_infer_gp_sum", "agp_cov_matrix",
    "agp_debug_cholesky", "agp_debug_mfma_probe", "agp_debug_mfma_peak", "agp_debug_math", "agp_set_profiling", "agp_get_timing", "agp_get_launch_times",
    "agp_set_workspace_limit", "agp_set_coalesce_window", "agp_get_coalesce_stats", "agp_get_dedup_stats",
    "agp_shard_range", "agp_comm_get_unique_id", "agp_comm_init_rank", "agp_comm_info", "agp_init_multi", "agp_set_data_multi",
    "agp_allgather_logweights", "agp_allgather_logweights_device", "agp_logpdf_batch_multi", "agp_logpdf_batch_extend_multi",
    "agp_debug_compact_shards", "agp_logpdf_batch_extend", "agp_extend_stats", "agp_extend_reset", "agp_extend_reserve",
    "agp_predict_reuse_stats", "agp_grad_reuse_stats", "agp_set_factor_cache", "agp_wait", "agp_comm_count", "agp_get_lag_stats", "agp_get_lattice_stats", "agp_get_compact_stats", "agp_set_lattice", "agp_probe_lattice", "agp_probe_program", "agp_get_eval_stats", "agp_set_reference_arithmetic", "agp_shard_plan", "agp_get_coalesce_timing", "agp_set_lag_tables", "agp_set_grad_lag_domain", "agp_get_grad_lag_domain_stats", "agp_get_grad_toeplitz_stats", "agp_get_grad_structured_stats", "agp_get_predict_structured_stats", "agp_get_toeplitz_stats", "agp_set_lag_rank_tables", "agp_get_lag_rank_stats", "agp_get_lag_predict_stats", "agp_get_poison_stats",
    "agp_logpdf_grad_batch_multi", "agp_predict_batch_multi", "agp_extend_stats2", "agp_predict_logpdf_batch",
    "agp_mixture_quantile", "agp_predict_quantile_batch", "agp_infer_gp_sum_batch", "agp_predict_sum_batch",
    "agp_predict_sample_batch", "agp_mixture_moments", "agp_predict_mixture_batch", "agp_get_mixture_stats",
    "agp_remove_data", "agp_get_remove_stats", "agp_set_remove_update", "agp_remove_data_multi",
    "agp_debug_factor_batch", "agp_logpdf_series_batch", "agp_debug_series_factor", "agp_logpdf_grad_series_batch",
    "agp_predict_series_batch", "agp_debug_remove_factor", "agp_predict_quantile_series_batch",
    "agp_predict_logpdf_series_batch", "agp_predict_sample_series_batch", "agp_predict_sum_series_batch",
    "agp_debug_toeplitz", "agp_debug_cov_sweep", "agp_hmc_series_batch", "agp_logpdf_long_series_batch",
    "agp_debug_long_series_factor", "agp_predict_long_series_batch", "agp_predict_quantile_long_series_batch",
    "agp_predict_logpdf_long_series_batch",
]
COMM_ID_BYTES = 128
SERIES_MAX_N = 176      # AGP_SERIES_MAX_N of include/autogp_hip.h: the longest series of logpdf_series_batch
LONG_SERIES_MAX_N = 512     # AGP_LONG_SERIES_MAX_N: the longest series of logpdf_long_series_batch
LONG_SERIES_ALL = 1         # AGP_LONG_SERIES_ALL: every non-empty series takes the long kernel


class AGPError(RuntimeError):
    pass


class PosDefException(ArithmeticError):
    """Mirror of LinearAlgebra.PosDefException raised by the reference on a non-PD matrix."""

    def __init__(self, info, particle=None):
        where = "" if particle is None else f" (particle {particle})"
        super().__init__(f"matrix is not positive definite; Cholesky factorization failed at minor {info}{where}")
        self.info = int(info)
        self.particle = particle


_lib = None


def _preload_shared_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  Two HIP runtimes
    in one process cannot both own the GPU, so when PyTorch is installed but not yet imported we map
    ITS runtime first; the engine then binds to it and a later `import torch` reuses the same copy.
    Without PyTorch the engine uses the system ROCm runtime from its RUNPATH."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
        if cand.exists():
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load_library(path=None):
    """dlopen the engine. Raises AGPError (never falls back) when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("AUTOGP_HIP_LIB", LIB_PATH))   # same override as AutoGPHIP.jl
    if not p.exists():
        raise AGPError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _preload_shared_hip_runtime()
    lib = C.CDLL(str(p))
    dp, ip, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    vp = C.c_void_p
    lib.agp_init.argtypes = [C.POINTER(vp), C.c_int]; lib.agp_init.restype = C.c_int
    lib.agp_destroy.argtypes = [vp]; lib.agp_destroy.restype = None
    lib.agp_last_error.argtypes = [vp]; lib.agp_last_error.restype = C.c_char_p
    lib.agp_version.argtypes = []; lib.agp_version.restype = C.c_char_p
    lib.agp_set_data.argtypes = [vp, dp, dp, C.c_int64]; lib.agp_set_data.restype = C.c_int
    lib.agp_logpdf.argtypes = [vp, C.c_int64, u8p, C.c_int32, dp, C.c_int32, C.c_double, dp, ip]
    lib.agp_logpdf.restype = C.c_int
    lib.agp_logpdf_batch.argtypes = [vp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, ip]
    lib.agp_logpdf_batch.restype = C.c_int
    lib.agp_logpdf_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.c_int32, ip, ip, u8p, ip, dp, dp, dp, ip]
    lib.agp_logpdf_series_batch.restype = C.c_int
    lib.agp_logpdf_long_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.c_int32, ip, ip, u8p, ip, dp, dp, C.c_int32, dp, ip]
    lib.agp_logpdf_long_series_batch.restype = C.c_int
    lib.agp_logpdf_grad_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.c_int32, ip, ip, u8p, ip, dp, dp, dp, dp, dp, ip]
    lib.agp_logpdf_grad_series_batch.restype = C.c_int
    lib.agp_hmc_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.c_int32, ip, ip, u8p, ip, dp, dp, ip, C.c_int32, dp,
                                         C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_int32,
                                         C.POINTER(C.c_uint64), C.c_int32, dp, dp, dp, dp, dp, ip, ip, dp]
    lib.agp_hmc_series_batch.restype = C.c_int
    lib.agp_predict_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.POINTER(C.c_int64), dp, C.c_int32, ip, ip, u8p,
                                             ip, dp, dp, dp, dp, dp, C.POINTER(C.c_int64), dp, ip]
    lib.agp_predict_series_batch.restype = C.c_int
    lib.agp_predict_quantile_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.POINTER(C.c_int64), dp, C.c_int32, ip, ip,
                                                      u8p, ip, dp, dp, dp, dp, dp, dp, dp, C.c_int64, C.c_double, C.c_int64, dp, ip, ip,
                                                      dp, dp, dp, ip]
    lib.agp_predict_quantile_series_batch.restype = C.c_int
    lib.agp_predict_long_series_batch.argtypes = lib.agp_predict_series_batch.argtypes + [C.c_uint32]
    lib.agp_predict_long_series_batch.restype = C.c_int
    lib.agp_predict_quantile_long_series_batch.argtypes = lib.agp_predict_quantile_series_batch.argtypes + [C.c_uint32]
    lib.agp_predict_quantile_long_series_batch.restype = C.c_int
    lib.agp_predict_logpdf_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.POINTER(C.c_int64), dp, dp, C.c_int32, ip,
                                                    ip, u8p, ip, dp, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_int64), dp, ip]
    lib.agp_predict_logpdf_series_batch.restype = C.c_int
    lib.agp_predict_logpdf_long_series_batch.argtypes = lib.agp_predict_logpdf_series_batch.argtypes + [C.c_uint32]
    lib.agp_predict_logpdf_long_series_batch.restype = C.c_int
    lib.agp_predict_sample_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.POINTER(C.c_int64), dp, C.c_int32, ip, ip,
                                                    u8p, ip, dp, dp, dp, dp, dp, dp, C.c_int64, C.POINTER(C.c_uint64), ip, dp, dp, ip,
                                                    dp, C.POINTER(C.c_int64), dp, C.POINTER(C.c_int64), ip]
    lib.agp_predict_sample_series_batch.restype = C.c_int
    lib.agp_predict_sum_series_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), dp, dp, C.POINTER(C.c_int64), dp, C.c_int32, C.c_int32,
                                                 ip, ip, u8p, ip, dp, dp, dp, dp, dp, dp, C.c_int64, dp, dp, dp, C.POINTER(C.c_int64), dp, ip]
    lib.agp_predict_sum_series_batch.restype = C.c_int
    lib.agp_logpdf_grad_batch.argtypes = [vp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, ip]
    lib.agp_logpdf_grad_batch.restype = C.c_int
    lib.agp_logpdf_grad.argtypes = [vp, C.c_int64, u8p, C.c_int32, dp, C.c_int32, C.c_double, dp, dp, dp, ip]
    lib.agp_logpdf_grad.restype = C.c_int
    lib.agp_logpdf_batch_device.argtypes = [vp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, vp, vp, vp]
    lib.agp_logpdf_batch_device.restype = C.c_int
    lib.agp_predict_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp,
                                      dp, dp, dp, ip]
    lib.agp_predict_batch.restype = C.c_int
    lib.agp_predict_logpdf_batch.argtypes = [vp, C.c_int64, dp, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, dp, ip]
    lib.agp_predict_logpdf_batch.restype = C.c_int
    lib.agp_mixture_quantile.argtypes = [vp, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_int64, C.c_double, C.c_int64, dp, ip, ip]
    lib.agp_mixture_quantile.restype = C.c_int
    lib.agp_predict_quantile_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, dp,
                                               C.c_double, C.c_double, dp, C.c_int64, C.c_double, C.c_int64, dp, ip, ip, ip]
    lib.agp_predict_quantile_batch.restype = C.c_int
    lib.agp_predict_sample_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, dp,
                                             C.c_double, C.c_double, C.c_int64, C.c_uint64, ip, dp, dp, ip, ip]
    lib.agp_predict_sample_batch.restype = C.c_int
    lib.agp_mixture_moments.argtypes = [vp, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_int32, dp, dp, dp]
    lib.agp_mixture_moments.restype = C.c_int
    lib.agp_predict_mixture_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, dp,
                                              C.c_double, C.c_double, C.c_int32, dp, dp, dp, ip]
    lib.agp_predict_mixture_batch.restype = C.c_int
    lib.agp_infer_gp_sum.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, C.c_double, C.c_double, dp, dp, ip]
    lib.agp_infer_gp_sum.restype = C.c_int
    lib.agp_infer_gp_sum_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, dp, ip]
    lib.agp_infer_gp_sum_batch.restype = C.c_int
    lib.agp_predict_sum_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, C.c_int32, ip, u8p, ip, dp, dp, dp, C.c_double,
                                          C.c_double, dp, C.c_int64, dp, dp, ip]
    lib.agp_predict_sum_batch.restype = C.c_int
    lib.agp_cov_matrix.argtypes = [vp, dp, C.c_int64, u8p, C.c_int32, dp, C.c_int32, C.c_double, dp]
    lib.agp_cov_matrix.restype = C.c_int
    lib.agp_debug_cholesky.argtypes = [vp, dp, C.c_int64, dp, ip]; lib.agp_debug_cholesky.restype = C.c_int
    lib.agp_debug_factor_batch.argtypes = [vp, dp, dp, C.c_int64, C.c_int32, C.c_int32, dp, dp, dp, ip]; lib.agp_debug_factor_batch.restype = C.c_int
    lib.agp_debug_series_factor.argtypes = [vp, dp, dp, C.c_int64, C.c_int32, dp, dp, dp, dp, ip]; lib.agp_debug_series_factor.restype = C.c_int
    lib.agp_debug_long_series_factor.argtypes = lib.agp_debug_series_factor.argtypes; lib.agp_debug_long_series_factor.restype = C.c_int
    lib.agp_debug_mfma_probe.argtypes = [vp, dp, dp, dp]; lib.agp_debug_mfma_probe.restype = C.c_int
    lib.agp_debug_mfma_peak.argtypes = [vp, C.c_int32, C.c_int32, dp, dp]; lib.agp_debug_mfma_peak.restype = C.c_int
    lib.agp_debug_math.argtypes = [vp, C.c_int32, dp, dp, dp, C.c_int32]; lib.agp_debug_math.restype = C.c_int
    if hasattr(lib, "agp_debug_gemm_variant"):      # measurement build only (libautogp_hip_exp.so)
        lib.agp_debug_gemm_variant.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp]; lib.agp_debug_gemm_variant.restype = C.c_int
    lib.agp_set_profiling.argtypes = [vp, C.c_int]; lib.agp_set_profiling.restype = C.c_int
    lib.agp_get_timing.argtypes = [vp, dp, C.c_int32]; lib.agp_get_timing.restype = C.c_int
    lib.agp_get_launch_times.argtypes = [vp, C.c_int32, dp, C.c_int32]; lib.agp_get_launch_times.restype = C.c_int
    lib.agp_set_workspace_limit.argtypes = [vp, C.c_int64]; lib.agp_set_workspace_limit.restype = C.c_int
    lib.agp_set_coalesce_window.argtypes = [vp, C.c_int32]; lib.agp_set_coalesce_window.restype = C.c_int
    lib.agp_get_coalesce_timing.argtypes = [vp, dp]; lib.agp_get_coalesce_timing.restype = C.c_int
    lib.agp_get_coalesce_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]; lib.agp_get_coalesce_stats.restype = C.c_int
    lib.agp_get_dedup_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]; lib.agp_get_dedup_stats.restype = C.c_int
    lib.agp_get_mixture_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]; lib.agp_get_mixture_stats.restype = C.c_int
    lib.agp_logpdf_batch_extend.argtypes = [vp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, ip]
    lib.agp_logpdf_batch_extend.restype = C.c_int
    if hasattr(lib, "agp_debug_flow_trace"):
        lib.agp_debug_flow_trace.argtypes = [vp, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]; lib.agp_debug_flow_trace.restype = C.c_int
    lib.agp_debug_compact_shards.argtypes = [vp, dp, C.c_int32, C.c_int32, dp]; lib.agp_debug_compact_shards.restype = C.c_int
    lib.agp_extend_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_extend_stats.restype = C.c_int
    lib.agp_extend_reset.argtypes = [vp, C.c_int]; lib.agp_extend_reset.restype = C.c_int
    lib.agp_extend_stats2.argtypes = [vp, C.POINTER(C.c_int64), C.c_int32]; lib.agp_extend_stats2.restype = C.c_int
    lib.agp_remove_data.argtypes = [vp, C.POINTER(C.c_int64), C.c_int64]; lib.agp_remove_data.restype = C.c_int
    lib.agp_debug_remove_factor.argtypes = [vp, dp, dp, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.c_int64, dp, dp, dp, dp, ip]
    lib.agp_debug_remove_factor.restype = C.c_int
    lib.agp_debug_toeplitz.argtypes = [vp, C.c_int32, C.c_int64, C.c_int64, C.c_int32, dp, dp, ip, dp, dp, dp, dp, dp, C.c_int32, C.c_double,
                                       C.c_double, C.c_double, C.c_int32, C.c_int32, dp, ip, dp, dp, dp, dp]
    lib.agp_debug_toeplitz.restype = C.c_int
    if hasattr(lib, "agp_debug_cov_sweep"):          # (absent from an older library that an A/B tool drives through AUTOGP_HIP_LIB; build() checks EXPORTED_SYMBOLS)
        lib.agp_debug_cov_sweep.argtypes = [vp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, C.c_int32, C.c_int32, dp, ip, ip, dp, dp]
        lib.agp_debug_cov_sweep.restype = C.c_int
    lib.agp_get_remove_stats.argtypes = [vp, C.POINTER(C.c_int64), C.c_int32]; lib.agp_get_remove_stats.restype = C.c_int
    lib.agp_set_remove_update.argtypes = [vp, C.c_int32]; lib.agp_set_remove_update.restype = C.c_int
    lib.agp_remove_data_multi.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(C.c_int64), C.c_int64]; lib.agp_remove_data_multi.restype = C.c_int
    lib.agp_predict_reuse_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_predict_reuse_stats.restype = C.c_int
    lib.agp_grad_reuse_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_grad_reuse_stats.restype = C.c_int
    lib.agp_set_factor_cache.argtypes = [vp, C.c_int32]; lib.agp_set_factor_cache.restype = C.c_int
    lib.agp_extend_reserve.argtypes = [vp, C.c_int64, C.c_int32]; lib.agp_extend_reserve.restype = C.c_int
    i32p = C.POINTER(C.c_int32)
    lib.agp_shard_range.argtypes = [C.c_int32, C.c_int32, C.c_int32, i32p, i32p]; lib.agp_shard_range.restype = None
    lib.agp_comm_get_unique_id.argtypes = [vp]; lib.agp_comm_get_unique_id.restype = C.c_int
    lib.agp_comm_init_rank.argtypes = [vp, vp, C.c_int32, C.c_int32]; lib.agp_comm_init_rank.restype = C.c_int
    lib.agp_shard_plan.argtypes = [C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, i32p, dp, dp]
    lib.agp_shard_plan.restype = C.c_int
    lib.agp_comm_info.argtypes = [vp, i32p, i32p]; lib.agp_comm_info.restype = C.c_int
    lib.agp_comm_count.argtypes = [vp, i32p]; lib.agp_comm_count.restype = C.c_int
    lib.agp_wait.argtypes = [vp]; lib.agp_wait.restype = C.c_int
    lib.agp_get_lag_stats.argtypes = [vp, i32p, C.POINTER(C.c_int64)]; lib.agp_get_lag_stats.restype = C.c_int
    lib.agp_set_lag_tables.argtypes = [vp, C.c_int32]; lib.agp_set_lag_tables.restype = C.c_int
    lib.agp_get_lattice_stats.argtypes = [vp, i32p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]; lib.agp_get_lattice_stats.restype = C.c_int
    lib.agp_get_compact_stats.argtypes = [vp, i32p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]; lib.agp_get_compact_stats.restype = C.c_int
    lib.agp_set_lattice.argtypes = [vp, C.c_int32]; lib.agp_set_lattice.restype = C.c_int
    lib.agp_get_poison_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]; lib.agp_get_poison_stats.restype = C.c_int
    lib.agp_set_reference_arithmetic.argtypes = [vp, C.c_int32]; lib.agp_set_reference_arithmetic.restype = C.c_int
    lib.agp_probe_lattice.argtypes = [dp, C.c_int64, i32p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int64)]; lib.agp_probe_lattice.restype = C.c_int
    lib.agp_probe_program.argtypes = [C.POINTER(C.c_uint8), C.c_int32, dp, C.c_int32, i32p, i32p, i32p, i32p]; lib.agp_probe_program.restype = C.c_int
    lib.agp_get_eval_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]; lib.agp_get_eval_stats.restype = C.c_int
    lib.agp_set_grad_lag_domain.argtypes = [vp, C.c_int32]; lib.agp_set_grad_lag_domain.restype = C.c_int
    lib.agp_set_lag_rank_tables.argtypes = [vp, C.c_int32]; lib.agp_set_lag_rank_tables.restype = C.c_int
    lib.agp_get_lag_rank_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_get_lag_rank_stats.restype = C.c_int
    lib.agp_get_lag_predict_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_get_lag_predict_stats.restype = C.c_int
    lib.agp_get_grad_lag_domain_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_get_grad_lag_domain_stats.restype = C.c_int
    lib.agp_get_grad_toeplitz_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_get_grad_toeplitz_stats.restype = C.c_int
    lib.agp_get_toeplitz_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_get_toeplitz_stats.restype = C.c_int
    lib.agp_get_grad_structured_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_get_grad_structured_stats.restype = C.c_int
    lib.agp_get_predict_structured_stats.argtypes = [vp, C.POINTER(C.c_int64)]; lib.agp_get_predict_structured_stats.restype = C.c_int
    lib.agp_init_multi.argtypes = [C.POINTER(vp), i32p, C.c_int32]; lib.agp_init_multi.restype = C.c_int
    lib.agp_set_data_multi.argtypes = [C.POINTER(vp), C.c_int32, dp, dp, C.c_int64]; lib.agp_set_data_multi.restype = C.c_int
    lib.agp_allgather_logweights.argtypes = [vp, dp, C.c_int32]; lib.agp_allgather_logweights.restype = C.c_int
    lib.agp_allgather_logweights_device.argtypes = [vp, vp, C.c_int32, vp, vp]; lib.agp_allgather_logweights_device.restype = C.c_int
    lib.agp_logpdf_batch_multi.argtypes = [C.POINTER(vp), C.c_int32, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, ip]
    lib.agp_logpdf_batch_multi.restype = C.c_int
    lib.agp_logpdf_batch_extend_multi.argtypes = lib.agp_logpdf_batch_multi.argtypes
    lib.agp_logpdf_batch_extend_multi.restype = C.c_int
    lib.agp_logpdf_grad_batch_multi.argtypes = [C.POINTER(vp), C.c_int32, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, ip, ip]
    lib.agp_logpdf_grad_batch_multi.restype = C.c_int
    lib.agp_predict_batch_multi.argtypes = [C.POINTER(vp), C.c_int32, C.c_int64, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp,
                                            dp, dp, dp, ip, ip]
    lib.agp_predict_batch_multi.restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _raise_first_bad(info, check):
    """PosDefException for the first particle with info > 0, when `check`."""
    if check and (info > 0).any():
        p = int(np.argmax(info > 0))
        raise PosDefException(int(info[p]), p)


def _series_ctypes(packed, queries=None):
    """The ctypes arguments the four many-series entries share, in the entries' order, from series_call_args' (and pack_queries')
    results, with a one-element stand-in for every empty array: S, pt_off, ts, xs, [q_off, ts_pred,] P, series, op_off, ops,
    prm_off, prm, noise [, noise_pred]."""
    pt_off, ts, xs, (op_off, ops, prm_off, prm), P, noises, sidx = packed
    i64 = C.POINTER(C.c_int64)
    some = lambda a: _dp(a if a.size else np.zeros(1))
    data = (pt_off.shape[0] - 1, pt_off.ctypes.data_as(i64), some(ts), some(xs))
    particles = (P, _ip(sidx), _ip(op_off), _u8(ops), _ip(prm_off), some(prm), _dp(noises))
    if queries is None:
        return data + particles
    q_off, ts_pred, noise_pred = queries
    return data + (q_off.ctypes.data_as(i64), some(ts_pred)) + particles + (_dp(noise_pred),)


def pack_series(series, max_n=SERIES_MAX_N):
    """Concatenate a sequence of (ts, xs) pairs for logpdf_series_batch: (pt_off int64[S+1], ts, xs), series s at
    [pt_off[s], pt_off[s+1]).  Raises ValueError on unequal lengths, input that is not 1-D, or a series of more than max_n points
    (SERIES_MAX_N; logpdf_long_series_batch passes LONG_SERIES_MAX_N); a series may be empty."""
    pt_off = np.zeros(len(series) + 1, dtype=np.int64)
    tss, xss = [], []
    for s, (ts, xs) in enumerate(series):
        ts, xs = _f64(ts), _f64(xs)
        if ts.ndim != 1 or xs.ndim != 1:
            raise ValueError(f"series {s}: ts and xs must be vectors")
        if ts.shape != xs.shape:
            raise ValueError(f"series {s}: ts and xs must have equal lengths ({ts.shape[0]} and {xs.shape[0]})")
        if ts.shape[0] > max_n:
            name = "LONG_SERIES_MAX_N" if max_n == LONG_SERIES_MAX_N else "SERIES_MAX_N" if max_n == SERIES_MAX_N else "max_n"
            raise ValueError(f"series {s} has {ts.shape[0]} points, more than {name} ({max_n})")
        pt_off[s + 1] = pt_off[s] + ts.shape[0]
        tss.append(ts); xss.append(xs)
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0)
    return pt_off, cat(tss), cat(xss)


def series_call_args(series, nodes, noises, series_index, programs=None, max_n=SERIES_MAX_N):
    """The validated arguments the two many-series entries share: (pt_off, ts, xs, (op_off, ops, prm_off, prm), P, noises, sidx).
    Raises ValueError (pack_series' checks, one noise and one series index per particle) before any library call."""
    pt_off, ts, xs = pack_series(series, max_n)
    programs = programs if programs is not None else _gp.encode_batch(nodes)
    P = programs[0].shape[0] - 1
    noises = _f64(noises)
    if noises.shape != (P,):
        raise ValueError("one noise per particle required")
    sidx = np.ascontiguousarray(np.asarray(series_index, dtype=np.int32))
    if sidx.shape != (P,):
        raise ValueError("one series index per particle required")
    return pt_off, ts, xs, programs, P, noises, sidx


def pack_queries(queries, n_series, noise_pred=None, P=None):
    """The query side of predict_series_batch: (q_off int64[S+1], ts_pred, noise_pred or None) from one vector of query times per
    series (a vector may be empty).  Raises ValueError when the number of query vectors differs from the number of series, when one
    is not 1-D, or when noise_pred is not one value per particle — before any library call."""
    if len(queries) != n_series:
        raise ValueError(f"one vector of query times per series required ({len(queries)} for {n_series} series)")
    q_off = np.zeros(n_series + 1, dtype=np.int64)
    parts = []
    for s, q in enumerate(queries):
        q = _f64(q)
        if q.ndim != 1:
            raise ValueError(f"series {s}: the query times must be a vector")
        q_off[s + 1] = q_off[s] + q.shape[0]
        parts.append(q)
    ts_pred = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0)
    if noise_pred is not None:
        noise_pred = _f64(noise_pred)
        if noise_pred.shape != (P,):
            raise ValueError("one noise_pred per particle required")
    return q_off, ts_pred, noise_pred


def pack_series_mixture(series_index, S, weights=None, log_weights=None):
    """The mixtures of predict_quantile_series_batch: (lists, weights) — lists[s] the particles p with series_index[p] == s in
    ascending p (int64; empty for a series without particles), and weights (P,) float64, particle p's weight inside ITS series'
    mixture.  Exactly one of `weights` (returned as given) and `log_weights` (normalised per series by a max-shifted softmax:
    exp(lw - max lw_s) / sum over the series) must be given.  Raises ValueError on anything but one vector of P entries each, on a
    series index outside [0, S), and when both or neither of weights / log_weights are given."""
    if (weights is None) == (log_weights is None):
        raise ValueError("exactly one of weights and log_weights required")
    sidx = np.asarray(series_index)
    if sidx.ndim != 1 or (sidx.size and sidx.dtype.kind not in "iu"):
        raise ValueError("series_index must be a vector of integers")
    sidx = sidx.astype(np.int64)
    S = int(S)
    if S < 0 or (sidx.size and (sidx.min() < 0 or sidx.max() >= S)):
        raise ValueError(f"series indexes must lie in [0, {S})")
    given = _f64(weights if weights is not None else log_weights)
    if given.shape != sidx.shape:
        raise ValueError(f"{'weights' if weights is not None else 'log_weights'} has shape {given.shape}, expected {sidx.shape}")
    lists = [np.flatnonzero(sidx == s) for s in range(S)]
    if weights is not None:
        return lists, given.copy()
    w = np.zeros(sidx.shape[0])
    for sel in lists:
        if sel.size:
            e = np.exp(given[sel] - given[sel].max())
            w[sel] = e / e.sum()
    return lists, w


SeriesBand = collections.namedtuple("SeriesBand", "x converged iters mean var logpdf info")


def _series_transforms(y_transforms, S):
    """(slope, intercept) of a series wrapper's y_transforms, one contiguous (S,) vector each — (None, None) for None (the library's
    (1, 0)).  Raises ValueError on anything but one (slope, intercept) pair per series."""
    if y_transforms is None:
        return None, None
    yt = _f64(y_transforms)
    if yt.shape != (S, 2):
        raise ValueError(f"y_transforms has shape {yt.shape}, expected ({S}, 2): one (slope, intercept) per series")
    return np.ascontiguousarray(yt[:, 0]), np.ascontiguousarray(yt[:, 1])


def _particle_weights(weights, P):
    """A series wrapper's mixture weights as float64, one per particle (ValueError otherwise)."""
    weights = _f64(weights)
    if weights.shape != (P,):
        raise ValueError(f"weights has shape {weights.shape}, expected ({P},)")
    return weights


def _particle_noise_pred(noise_pred, P):
    """A series wrapper's noise_pred: a scalar serves every particle; anything else (None, one per particle) is pack_queries' to
    check.  (predict_quantile_series_batch broadcasts with np.broadcast_to instead, and so also takes a length-1 vector: its own line.)"""
    return np.full(P, float(noise_pred)) if noise_pred is not None and np.ndim(noise_pred) == 0 else noise_pred


def pack_heldout(heldout, q_off, y_transforms=None):
    """The held-out side of predict_logpdf_series_batch: (y_pred, slope or None) from one vector of RAW held-out values per series,
    series s's as long as its vector of query times (q_off: pack_queries').  y_transforms: one (slope, intercept) per series
    (scaled = slope * raw + intercept; None: the values are passed as they are); y_pred is the concatenation of the SCALED values —
    the space xs is in — and slope what the library's Jacobian term needs.  Raises ValueError on anything but one vector per series
    of the query vector's length, and on a y_transforms that is not (S, 2) — before any library call."""
    S = q_off.shape[0] - 1
    if len(heldout) != S:
        raise ValueError(f"one vector of held-out values per series required ({len(heldout)} for {S} series)")
    slope, icpt = _series_transforms(y_transforms, S)
    parts = []
    for s, y in enumerate(heldout):
        y = _f64(y)
        m = int(q_off[s + 1] - q_off[s])
        if y.ndim != 1 or y.shape[0] != m:
            raise ValueError(f"series {s}: {m} held-out values required, one per query time (got shape {y.shape})")
        parts.append(y if slope is None else slope[s] * y + icpt[s])
    y_pred = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0)
    return y_pred, slope


SeriesScores = collections.namedtuple("SeriesScores", "logpdf terms series_logp info")
SeriesSamples = collections.namedtuple("SeriesSamples", "x component mean cov info")
SeriesSums = collections.namedtuple("SeriesSums", "mean var x logpdf info")


def check_remove_indexes(indexes, n_max):
    """The positions of remove_data as a contiguous int64 vector: distinct, ascending, inside [0, n_max) and not empty (the
    reference's "No such time points"); raises ValueError before any library call."""
    raw = np.asarray(indexes)
    if raw.ndim != 1 or raw.size == 0:
        raise ValueError("no such time points: indexes must be a non-empty vector of positions")
    if raw.dtype.kind not in "iu":
        raise ValueError("indexes must be integers")
    idx = np.ascontiguousarray(raw, dtype=np.int64)
    if idx[0] < 0 or idx[-1] >= int(n_max) or (idx.size > 1 and (np.diff(idx) <= 0).any()) or (idx < 0).any() or (idx >= int(n_max)).any():
        raise ValueError(f"indexes must be distinct ascending positions in [0, {int(n_max)})")
    return idx


class GPEngine:
    """One engine context per GPU (the C ABI's agp_ctx)."""

    def __init__(self, device: int = 0, _ctx=None):
        self._lib = load_library()
        if _ctx is not None:          # a context created by agp_init_multi
            self._ctx = _ctx
        else:
            self._ctx = C.c_void_p()
            rc = self._lib.agp_init(C.byref(self._ctx), int(device))
            if rc != 0:
                msg = self._lib.agp_last_error(None)
                raise AGPError(f"agp_init failed ({rc}): {msg.decode() if msg else ''}")
        self.device = int(device)
        self.n_max = 0

    # -- multi-GPU: communicator + the log-weight all-gather (RCCL behind the C ABI) ----------
    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte RCCL id created on rank 0; hand it to the other ranks over any host channel."""
        lib = load_library()
        buf = C.create_string_buffer(COMM_ID_BYTES)
        rc = lib.agp_comm_get_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            msg = lib.agp_last_error(None)
            raise AGPError(f"agp_comm_get_unique_id failed ({rc}): {msg.decode() if msg else ''}")
        return buf.raw

    def comm_init_rank(self, comm_id: bytes, n_ranks: int, rank: int):
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError("communicator id must be 128 bytes")
        buf = C.create_string_buffer(comm_id, COMM_ID_BYTES)
        self._check(self._lib.agp_comm_init_rank(self._ctx, C.cast(buf, C.c_void_p), int(n_ranks), int(rank)))

    def comm_info(self):
        r = C.c_int32(); n = C.c_int32()
        has = self._lib.agp_comm_info(self._ctx, C.byref(r), C.byref(n))
        return bool(has), r.value, n.value

    def comm_count(self):
        """Ranks RCCL reports for this context's communicator (ncclCommCount); 0 without one."""
        n = C.c_int32()
        self._check(self._lib.agp_comm_count(self._ctx, C.byref(n)))
        return n.value

    def wait(self):
        """agp_wait: block until every asynchronously enqueued sweep has completed; raises on a latched kernel timeout."""
        self._check(self._lib.agp_wait(self._ctx))

    def allgather_logweights(self, lw):
        """Host form: `lw` (P float64) with this rank's block filled; returns the complete vector."""
        lw = np.ascontiguousarray(np.asarray(lw, dtype=np.float64)).copy()
        self._check(self._lib.agp_allgather_logweights(self._ctx, _dp(lw), lw.shape[0]))
        return lw

    def allgather_logweights_device(self, d_local_ptr, P, d_all_ptr, stream_ptr=0):
        self._check(self._lib.agp_allgather_logweights_device(self._ctx, C.c_void_p(d_local_ptr), int(P),
                                                              C.c_void_p(d_all_ptr), C.c_void_p(stream_ptr)))

    # -- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.agp_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.agp_last_error(self._ctx)
            raise AGPError(f"engine call failed ({rc}): {msg.decode() if msg else ''}")

    @property
    def version(self):
        return self._lib.agp_version().decode()

    # -- data ------------------------------------------------------------------------------
    def set_data(self, ts, xs):
        ts, xs = _f64(ts), _f64(xs)
        if ts.shape != xs.shape or ts.ndim != 1:
            raise ValueError("ts and xs must be equal-length vectors")
        self._check(self._lib.agp_set_data(self._ctx, _dp(ts), _dp(xs), ts.shape[0]))
        self.n_max = ts.shape[0]

    def remove_data(self, indexes):
        """remove_data! (src/api.jl:449-468): delete the observations at the given 0-based ascending positions of the resident series.
        Resident factors that contain removed positions are updated on the device (or dropped where refactoring is cheaper), so
        logpdf_batch_extend at the new n_max starts from them.  Returns the new n_max."""
        idx = check_remove_indexes(indexes, getattr(self, "n_max", 0))
        self._check(self._lib.agp_remove_data(self._ctx, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size))
        self.n_max -= int(idx.size)
        return self.n_max

    def remove_stats(self):
        """dict(updated, dropped, rows_removed, panel_steps) of remove_data since the engine was created (agp_get_remove_stats)."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.agp_get_remove_stats(self._ctx, out, 4))
        return dict(zip(("updated", "dropped", "rows_removed", "panel_steps"), [int(v) for v in out]))

    def set_remove_update(self, on):
        """0: remove_data always drops the factors it touches; 1: the admission rule decides; 2: always updates (measurement)
        (env AGP_REMOVE_UPDATE)."""
        self._check(self._lib.agp_set_remove_update(self._ctx, int(on)))

    # -- value path (src/Model.jl:135-136) ---------------------------------------------------
    def logpdf(self, node, noise, n=None, check=True):
        ops, prm = _gp.encode(node)
        n = self.n_max if n is None else int(n)
        out = C.c_double(); info = C.c_int32()
        prm_arg = prm if prm.size else np.zeros(1)
        self._check(self._lib.agp_logpdf(self._ctx, n, _u8(ops), ops.size, _dp(prm_arg), prm.size, float(noise),
                                         C.byref(out), C.byref(info)))
        if check and info.value > 0:
            raise PosDefException(info.value)
        return out.value

    def logpdf_grad(self, node, noise, n=None, check=True):
        """(logpdf, d logpdf / d theta in encode(node) parameter order, d logpdf / d noise) of ONE particle — the call a
        per-thread differentiating caller (Gen.choice_gradients) makes; concurrent callers are coalesced."""
        ops, prm = _gp.encode(node)
        n = self.n_max if n is None else int(n)
        out = C.c_double(); gn = C.c_double(); info = C.c_int32()
        prm_arg = prm if prm.size else np.zeros(1)
        grad = np.zeros(max(1, prm.size))
        self._check(self._lib.agp_logpdf_grad(self._ctx, n, _u8(ops), ops.size, _dp(prm_arg), prm.size, float(noise),
                                              C.byref(out), _dp(grad), C.byref(gn), C.byref(info)))
        if check and info.value > 0:
            raise PosDefException(info.value)
        return out.value, grad[:prm.size], gn.value

    def logpdf_batch(self, nodes, noises, n=None, check=True, programs=None):
        """log N(xs[1:n]; 0, K_p + noise_p I) for every particle p.  Returns (logpdf[P], info[P])."""
        n = self.n_max if n is None else int(n)
        op_off, ops, prm_off, prm = programs if programs is not None else _gp.encode_batch(nodes)
        P = op_off.shape[0] - 1
        noises = _f64(noises)
        if noises.shape != (P,):
            raise ValueError("one noise per particle required")
        out = np.empty(P, dtype=np.float64); info = np.empty(P, dtype=np.int32)
        self._check(self._lib.agp_logpdf_batch(self._ctx, n, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                               _dp(noises), _dp(out), _ip(info)))
        _raise_first_bad(info, check)
        return out, info

    def logpdf_series_batch(self, series, nodes, noises, series_index, check=True, programs=None):
        """agp_logpdf_series_batch: many short series (a sequence of (ts, xs) pairs of at most SERIES_MAX_N points each) scored in one
        fused launch — particle p scores series[series_index[p]]: log N(xs_s; 0, K_p(ts_s) + noise_p I).  Needs no set_data and leaves
        the resident series, the factor store and every counter alone.  Returns (logpdf[P], info[P])."""
        packed = series_call_args(series, nodes, noises, series_index, programs)
        P = packed[4]
        out = np.empty(P, dtype=np.float64); info = np.empty(P, dtype=np.int32)
        self._check(self._lib.agp_logpdf_series_batch(self._ctx, *_series_ctypes(packed), _dp(out), _ip(info)))
        _raise_first_bad(info, check)
        return out, info

    def logpdf_long_series_batch(self, series, nodes, noises, series_index, all_long=False, check=True, programs=None):
        """agp_logpdf_long_series_batch: logpdf_series_batch for series of at most LONG_SERIES_MAX_N points — same arguments, same
        statelessness, one call for a mixed family such as 135, 143 and 442 points.  A series of at most SERIES_MAX_N points runs in
        logpdf_series_batch's kernel (bit-identical results); a longer one in the long-series kernel, which keeps the factor in an
        HBM workspace (bounded by set_workspace_limit; more long particles than fit are split into several launches).  all_long:
        every non-empty series takes the long kernel.  Returns (logpdf[P], info[P])."""
        packed = series_call_args(series, nodes, noises, series_index, programs, max_n=LONG_SERIES_MAX_N)
        P = packed[4]
        out = np.empty(P, dtype=np.float64); info = np.empty(P, dtype=np.int32)
        self._check(self._lib.agp_logpdf_long_series_batch(self._ctx, *_series_ctypes(packed), LONG_SERIES_ALL if all_long else 0,
                                                           _dp(out), _ip(info)))
        _raise_first_bad(info, check)
        return out, info

    def logpdf_grad_series_batch(self, series, nodes, noises, series_index, check=True, programs=None):
        """agp_logpdf_grad_series_batch: value and gradient of many short series in one fused launch — logpdf_series_batch's twin, same
        arguments, same statelessness.  Returns (logpdf[P], grads, grad_noise[P], info[P]); grads[p] is d logpdf / d theta in the order
        of gp.encode(node)[1], as in logpdf_grad_batch; logpdf is bit-identical to logpdf_series_batch's."""
        packed = series_call_args(series, nodes, noises, series_index, programs)
        prm_off, P = packed[3][2], packed[4]
        out = np.empty(P, dtype=np.float64); info = np.empty(P, dtype=np.int32); gn = np.empty(P, dtype=np.float64)
        grad = np.zeros(max(1, int(prm_off[-1])))
        self._check(self._lib.agp_logpdf_grad_series_batch(self._ctx, *_series_ctypes(packed), _dp(out), _dp(grad), _dp(gn), _ip(info)))
        _raise_first_bad(info, check)
        return out, [grad[prm_off[i]:prm_off[i + 1]] for i in range(P)], gn, info

    def hmc_series_batch(self, series, nodes, z, z_noise, prm_class, tf, series_index, n_hmc, seeds, noise_class=0, noise_jitter=1e-5,
                         L_param=10, eps_param=0.02, L_noise=10, eps_noise=0.02, n_exit=None, want_trace=False, flags=0, check=True,
                         programs=None):
        """agp_hmc_series_batch: the reference's rejuvenate_particle_parameters for every (series, particle) of a family of short
        series in one call — n_hmc iterations of an HMC move on the kernel parameters and one on the noise, in the latent space
        (theta = transform(z; tf[class])), the whole chain of a particle in one workgroup.  `nodes` (or `programs`) give the
        STRUCTURE only (their parameter values are not read); z: one vector per particle in the order of gp.encode(node)[1] (a
        slot of class < 0 holds the FIXED parameter value); prm_class: one int32 vector per particle; tf: (C, 3) rows
        (mu, sigma, scale); seeds: one uint64 per particle; n_exit: None = n_hmc (the reference's default), <= 0 = never.
        Returns a SimpleNamespace: z, prm (lists of per-particle vectors), z_noise[P], noise[P], logpdf[P] (bit-identical to
        logpdf_series_batch of (prm, noise)), counts[P, 4] (parameter moves accepted, tried, noise moves accepted, trajectories
        rejected as not positive definite), info[P], trace[P, n_hmc, 2, 2] of (alpha, log u) or None."""
        from types import SimpleNamespace
        pt_off, ts, xs = pack_series(series)
        op_off, ops, prm_off, _ = programs if programs is not None else _gp.encode_batch(nodes)
        P = op_off.shape[0] - 1
        nt = int(prm_off[-1])
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=dt).ravel() for a in parts]) if len(parts) else np.zeros(0, dtype=dt))
        zc = cat(z, np.float64); cls = cat(prm_class, np.int32)
        if zc.shape != (nt,) or cls.shape != (nt,):
            raise ValueError("z and prm_class need one entry per program parameter")
        zn = _f64(z_noise); sidx = np.ascontiguousarray(np.asarray(series_index, dtype=np.int32))
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        if zn.shape != (P,) or sidx.shape != (P,) or seeds.shape != (P,):
            raise ValueError("one z_noise, one series index and one seed per particle required")
        tf = _f64(tf)
        if tf.ndim != 2 or tf.shape[1] != 3:
            raise ValueError("tf must have shape (C, 3): (mu, sigma, scale) per class")
        n_hmc = int(n_hmc)
        out_z = np.zeros(max(1, nt)); out_prm = np.zeros(max(1, nt)); out_zn = np.empty(P); out_nz = np.empty(P); lp = np.empty(P)
        counts = np.zeros((P, 4), dtype=np.int32); info = np.zeros(P, dtype=np.int32)
        trace = np.empty((P, max(0, n_hmc), 2, 2)) if want_trace else None
        some = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)
        self._check(self._lib.agp_hmc_series_batch(
            self._ctx, pt_off.shape[0] - 1, pt_off.ctypes.data_as(C.POINTER(C.c_int64)), _dp(some(ts)), _dp(some(xs)), P, _ip(some(sidx)),
            _ip(op_off), _u8(some(ops)), _ip(prm_off), _dp(some(zc)), _dp(some(zn)), _ip(some(cls)), tf.shape[0], _dp(some(tf)), int(noise_class),
            float(noise_jitter), n_hmc, int(L_param), float(eps_param), int(L_noise), float(eps_noise), int(n_hmc if n_exit is None else n_exit),
            some(seeds).ctypes.data_as(C.POINTER(C.c_uint64)), int(flags), _dp(out_z), _dp(some(out_zn)), _dp(out_prm), _dp(some(out_nz)),
            _dp(some(lp)), _ip(some(counts.reshape(-1))), _ip(some(info)), _dp(some(trace.reshape(-1))) if want_trace else None))
        _raise_first_bad(info, check)
        split = lambda a: [a[prm_off[i]:prm_off[i + 1]] for i in range(P)]
        return SimpleNamespace(z=split(out_z), prm=split(out_prm), z_noise=out_zn, noise=out_nz, logpdf=lp, counts=counts, info=info, trace=trace)

    def predict_series_batch(self, series, queries, nodes, noises, series_index, noise_pred=None, want_logpdf=False, check=True,
                             programs=None):
        """agp_predict_series_batch: forecasts of many short series in one fused launch — logpdf_series_batch's predictive twin, same
        series / particle arguments and statelessness.  queries[s] holds series s's own query times; particle p predicts on
        series[series_index[p]]: mean = K21 K11^-1 x, var = diag(K22 - K21 K11^-1 K12) + noise_pred[p] (None: the particle's noise).
        Returns (means, vars, info), or (means, vars, logpdf, info) with want_logpdf (the training log marginal likelihood,
        bit-identical to logpdf_series_batch's); means[p] / vars[p] are views of length len(queries[series_index[p]]) into one
        particle-major array, so np.stack of the adjacent particles of one series is the block mixture_quantile takes."""
        return self._predict_series("agp_predict_series_batch", (), SERIES_MAX_N, series, queries, nodes, noises, series_index,
                                    noise_pred, want_logpdf, check, programs)

    def predict_long_series_batch(self, series, queries, nodes, noises, series_index, noise_pred=None, want_logpdf=False, all_long=False,
                                  check=True, programs=None):
        """agp_predict_long_series_batch: predict_series_batch for series of at most LONG_SERIES_MAX_N points — same arguments, same
        returns, same statelessness, one call for a mixed family such as 135, 143 and 442 points.  A series of at most SERIES_MAX_N
        points runs in predict_series_batch's kernel (bit-identical results); a longer one in the long-series predictive kernel, which
        keeps the factor and the solved query blocks in an HBM workspace (bounded by set_workspace_limit; more long particles than
        fit are split into several launches).  all_long: every non-empty series takes the long kernel.  logpdf (want_logpdf) is
        bit-identical to logpdf_long_series_batch's under the same all_long."""
        return self._predict_series("agp_predict_long_series_batch", (LONG_SERIES_ALL if all_long else 0,), LONG_SERIES_MAX_N,
                                    series, queries, nodes, noises, series_index, noise_pred, want_logpdf, check, programs)

    def _predict_series(self, entry, tail, max_n, series, queries, nodes, noises, series_index, noise_pred, want_logpdf, check, programs):
        """The forecast entries' one call: the library's `entry` (by name: the shape checks below come before the library is touched)
        with the shared arguments and outputs, then `tail` (the long entry's flags)."""
        packed = series_call_args(series, nodes, noises, series_index, programs, max_n=max_n)
        S, P, sidx = packed[0].shape[0] - 1, packed[4], packed[6]
        qpack = pack_queries(queries, S, noise_pred, P)
        m_s = np.diff(qpack[0])
        total = int(sum(m_s[i] for i in sidx if 0 <= i < S))      # (an index outside is the library's to report)
        mean = np.empty(max(1, total)); var = np.empty(max(1, total))
        out_off = np.zeros(P + 1, dtype=np.int64)
        lp = np.empty(P, dtype=np.float64) if want_logpdf else None
        info = np.empty(P, dtype=np.int32)
        self._check(getattr(self._lib, entry)(self._ctx, *_series_ctypes(packed, qpack), _dp(mean), _dp(var),
                                              out_off.ctypes.data_as(C.POINTER(C.c_int64)), _dp(lp), _ip(info), *tail))
        _raise_first_bad(info, check)
        means = [mean[out_off[p]:out_off[p + 1]] for p in range(P)]
        vars_ = [var[out_off[p]:out_off[p + 1]] for p in range(P)]
        return (means, vars_, lp, info) if want_logpdf else (means, vars_, info)

    def predict_quantile_series_batch(self, series, queries, nodes, noises, series_index, weights, q, y_transforms=None, noise_pred=None,
                                      tol=1e-5, max_iter=10**6, want_moments=False, want_logpdf=False, check=True, programs=None):
        """agp_predict_quantile_series_batch: the forecast bands of many short series in one call — predict_series_batch, then on the
        device the quantiles q (a scalar or a vector) of every series' own mixture of its particles' raw-space predictives, and with
        want_moments that mixture's marginal mean and variance.  weights[p] is particle p's weight inside the mixture of
        series[series_index[p]] (each series' weights sum to 1; pack_series_mixture normalises log-weights); y_transforms: one
        (slope, intercept) pair per series (None: (1, 0)).  Returns SeriesBand(x, converged, iters, mean, var, logpdf, info): x,
        converged and iters are lists over the series, each shaped as mixture_quantile returns it — (m_s, nq), or (m_s,) for a scalar
        q (views into one array per output, as predict_series_batch's); mean / var (lists of (m_s,) arrays) and logpdf (P,) are None
        unless asked for.  A series without particles, or with a
        particle whose info != 0 (PosDefException when check), gets NaN and converged False."""
        return self._predict_quantile_series("agp_predict_quantile_series_batch", (), SERIES_MAX_N, series, queries, nodes, noises,
                                             series_index, weights, q, y_transforms, noise_pred, tol, max_iter, want_moments, want_logpdf,
                                             check, programs)

    def predict_quantile_long_series_batch(self, series, queries, nodes, noises, series_index, weights, q, y_transforms=None,
                                           noise_pred=None, tol=1e-5, max_iter=10**6, want_moments=False, want_logpdf=False,
                                           all_long=False, check=True, programs=None):
        """agp_predict_quantile_long_series_batch: predict_quantile_series_batch for series of at most LONG_SERIES_MAX_N points — same
        arguments and returns; the predictive launches are predict_long_series_batch's (routing, workspace, all_long), the read-out
        kernels behind them are predict_quantile_series_batch's, unchanged."""
        return self._predict_quantile_series("agp_predict_quantile_long_series_batch", (LONG_SERIES_ALL if all_long else 0,),
                                             LONG_SERIES_MAX_N, series, queries, nodes, noises, series_index, weights, q, y_transforms,
                                             noise_pred, tol, max_iter, want_moments, want_logpdf, check, programs)

    def _predict_quantile_series(self, entry, tail, max_n, series, queries, nodes, noises, series_index, weights, q, y_transforms,
                                 noise_pred, tol, max_iter, want_moments, want_logpdf, check, programs):
        """The band entries' one call: the library's `entry` (by name, as in _predict_series) with the shared arguments and outputs,
        then `tail` (the long entry's flags)."""
        packed = series_call_args(series, nodes, noises, series_index, programs, max_n=max_n)
        S, P = packed[0].shape[0] - 1, packed[4]
        qpack = pack_queries(queries, S, None if noise_pred is None else np.broadcast_to(noise_pred, (P,)), P)
        q_off = qpack[0]
        weights = _particle_weights(weights, P)
        slope, icpt = _series_transforms(y_transforms, S)
        qa = _f64(np.atleast_1d(q)); nq = qa.shape[0]
        Q = int(q_off[-1])
        x = np.empty(max(1, nq * Q)); conv = np.zeros(max(1, nq * Q), dtype=np.int32); iters = np.zeros(max(1, nq * Q), dtype=np.int32)
        mean = np.empty(max(1, Q)) if want_moments else None
        var = np.empty(max(1, Q)) if want_moments else None
        lp = np.empty(P, dtype=np.float64) if want_logpdf else None
        info = np.zeros(max(1, P), dtype=np.int32)
        self._check(getattr(self._lib, entry)(
            self._ctx, *_series_ctypes(packed, qpack), _dp(weights), _dp(slope), _dp(icpt), _dp(qa), nq, float(tol), int(max_iter),
            _dp(x), _ip(conv), _ip(iters), _dp(mean), _dp(var), _dp(lp), _ip(info), *tail))
        info = info[:P]
        _raise_first_bad(info, check)
        # series s's (nq, m_s) row-major block, seen as (m_s, nq) — or (m_s,) for a scalar q: views into the call's arrays
        conv = conv.astype(bool)
        lo = (nq * q_off).tolist(); qo = q_off.tolist()
        if np.ndim(q) == 0:
            blocks = lambda a: [a[lo[s]:lo[s + 1]] for s in range(S)]
        else:
            blocks = lambda a: [a[lo[s]:lo[s + 1]].reshape(nq, qo[s + 1] - qo[s]).T for s in range(S)]
        cut = lambda a: None if a is None else [a[qo[s]:qo[s + 1]] for s in range(S)]
        return SeriesBand(blocks(x), blocks(conv), blocks(iters), cut(mean), cut(var), lp, info)

    def predict_logpdf_series_batch(self, series, queries, heldout, nodes, noises, series_index, weights=None, y_transforms=None,
                                    noise_pred=None, want_terms=False, check=True, programs=None):
        """agp_predict_logpdf_series_batch: the held-out scores of many short series in one fused launch — predict_logpdf_batch's twin
        for callers that hold one model per short series, with predict_series_batch's series / query / particle arguments and
        statelessness.  heldout[s] holds the RAW values observed at queries[s]; particle p scores them under its posterior predictive
        on series[series_index[p]] (len(series[s]) + len(queries[s]) <= SERIES_MAX_N).  y_transforms: one (slope, intercept) per
        series (scaled = slope * raw + intercept, the space the series' xs are in; None: (1, 0)) — the values are scaled here, as
        predict_proba does, and the density of the raw values gains m log|slope|.  weights[p] (optional) is particle p's weight inside
        the mixture of ITS series (pack_series_mixture).  Returns SeriesScores(logpdf, terms, series_logp, info): logpdf (P,); terms
        (want_terms) a list of views, terms[p][j] the log-density of held-out point j given the training data and the points before
        it, summing to logpdf[p]; series_logp (S,) with weights — the log of each series' mixture density at its held-out vector
        (NaN for a series without particles or with a failed particle, 0 where nothing is held out) — else None."""
        return self._predict_logpdf_series("agp_predict_logpdf_series_batch", (), SERIES_MAX_N, series, queries, heldout, nodes, noises,
                                           series_index, weights, y_transforms, noise_pred, want_terms, check, programs)

    def predict_logpdf_long_series_batch(self, series, queries, heldout, nodes, noises, series_index, weights=None, y_transforms=None,
                                         noise_pred=None, want_terms=False, all_long=False, check=True, programs=None):
        """agp_predict_logpdf_long_series_batch: predict_logpdf_series_batch for len(series[s]) + len(queries[s]) of at most
        LONG_SERIES_MAX_N joint points — same arguments, same returns.  A series whose joint length is at most SERIES_MAX_N runs in
        predict_logpdf_series_batch's kernel (bit-identical logpdf, terms, mixtures and info); a longer one runs in the long kernel
        on the joint points, its factor in an HBM workspace (bounded by set_workspace_limit; more long particles than fit are split
        into several launches).  all_long: every particle with held-out points takes the long kernel.  A series with held-out points
        and a joint length above LONG_SERIES_MAX_N is a ValueError that names it, before any library call."""
        return self._predict_logpdf_series("agp_predict_logpdf_long_series_batch", (LONG_SERIES_ALL if all_long else 0,),
                                           LONG_SERIES_MAX_N, series, queries, heldout, nodes, noises, series_index, weights, y_transforms,
                                           noise_pred, want_terms, check, programs)

    def _predict_logpdf_series(self, entry, tail, max_n, series, queries, heldout, nodes, noises, series_index, weights, y_transforms,
                               noise_pred, want_terms, check, programs):
        """the two held-out entries: `entry` with the trailing arguments `tail` behind agp_predict_logpdf_series_batch's; max_n: the
        cap pack_series applies per series and, in the long entry, the cap on the joint length of a series with held-out points"""
        packed = series_call_args(series, nodes, noises, series_index, programs, max_n=max_n)
        S, P, sidx = packed[0].shape[0] - 1, packed[4], packed[6]
        qpack = pack_queries(queries, S, _particle_noise_pred(noise_pred, P), P)
        if max_n == LONG_SERIES_MAX_N:      # (the short entry's joint cap is the library's to report, as it always was)
            for s, (n_s, m_s) in enumerate(zip(np.diff(packed[0]), np.diff(qpack[0]))):
                if m_s > 0 and n_s + m_s > max_n:
                    raise ValueError(f"series {s} has {n_s} training and {m_s} held-out points, together more than "
                                     f"LONG_SERIES_MAX_N ({max_n})")
        y_pred, slope = pack_heldout(heldout, qpack[0], y_transforms)
        if weights is not None:
            weights = _particle_weights(weights, P)
        m_s = np.diff(qpack[0])
        total = int(sum(m_s[i] for i in sidx if 0 <= i < S))      # (an index outside is the library's to report)
        lp = np.empty(max(1, P), dtype=np.float64); info = np.zeros(max(1, P), dtype=np.int32)
        terms = np.empty(max(1, total)) if want_terms else None
        out_off = np.zeros(P + 1, dtype=np.int64)
        mix = np.empty(max(1, S)) if weights is not None else None
        a = _series_ctypes(packed, qpack)      # (.., q_off, ts_pred | P, ..): the held-out values travel between the two
        self._check(getattr(self._lib, entry)(
            self._ctx, *a[:6], _dp(y_pred if y_pred.size else np.zeros(1)), *a[6:], _dp(slope), _dp(weights), _dp(lp), _dp(terms),
            out_off.ctypes.data_as(C.POINTER(C.c_int64)), _dp(mix), _ip(info), *tail))
        lp, info = lp[:P], info[:P]
        _raise_first_bad(info, check)
        cut = None if terms is None else [terms[out_off[p]:out_off[p + 1]] for p in range(P)]
        return SeriesScores(lp, cut, None if mix is None else mix[:S], info)

    def predict_sample_series_batch(self, series, queries, nodes, noises, series_index, weights, n_samples, seeds=None, y_transforms=None,
                                    noise_pred=None, component=None, z=None, want_moments=False, check=True, programs=None):
        """agp_predict_sample_series_batch: sample paths of many short series in one fused launch — predict_sample_batch's twin for
        callers that hold one model per short series, with predict_logpdf_series_batch's series / query / particle arguments and
        statelessness (len(series[s]) + len(queries[s]) <= SERIES_MAX_N).  weights[p] is particle p's weight inside the mixture of
        ITS series (pack_series_mixture); n_samples (R >= 0) samples are drawn per series, series s under seeds[s] exactly as
        predict_sample_batch draws under that seed (seeds: one unsigned 64-bit integer per series; None: 0, 1, ..).  y_transforms:
        one (slope, intercept) per series (scaled = slope * raw + intercept; None: (1, 0)); every output is in raw space.
        component (S, R) of global particle indices and z (a list over the series of (m_s, R) arrays of normals) replace the draws.
        Returns SeriesSamples(x, component, mean, cov, info): x a list over the series of (m_s, R) arrays, column j being sample j;
        component (S, R); with want_moments mean / cov, lists over the PARTICLES of (m_s,) / (m_s, m_s) arrays — the components of
        predict_mvn's mixture of every series — else None; info (P,).  A series with a failed particle is NaN in x (PosDefException
        with check)."""
        packed = series_call_args(series, nodes, noises, series_index, programs)
        S, P, sidx = packed[0].shape[0] - 1, packed[4], packed[6]
        qpack = pack_queries(queries, S, _particle_noise_pred(noise_pred, P), P)
        qo = qpack[0]
        m_s = np.diff(qo)
        R = int(n_samples)
        slope, icpt = _series_transforms(y_transforms, S)
        weights = _particle_weights(weights, P)
        seeds = np.arange(S, dtype=np.uint64) if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        if seeds.shape != (S,):
            raise ValueError(f"seeds has shape {seeds.shape}, expected ({S},): one per series")
        Rp = max(R, 0)
        if component is not None:
            component = np.ascontiguousarray(np.asarray(component, dtype=np.int32))
            if component.shape != (S, Rp):
                raise ValueError(f"component has shape {component.shape}, expected ({S}, {Rp})")
        if z is not None:
            if len(z) != S:
                raise ValueError(f"one array of normals per series required ({len(z)} for {S} series)")
            parts = []
            for s, zs in enumerate(z):
                zs = np.asarray(zs, dtype=np.float64)
                if zs.shape != (int(m_s[s]), Rp):
                    raise ValueError(f"series {s}: z has shape {zs.shape}, expected ({int(m_s[s])}, {Rp})")
                parts.append(zs.T.ravel())      # sample j is the column of m_s values at j * m_s
            z = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0)
        in_range = [i for i in sidx if 0 <= i < S]      # (an index outside is the library's to report)
        n_mean = int(sum(m_s[i] for i in in_range)); n_cov = int(sum(m_s[i] * m_s[i] for i in in_range))
        x = np.empty(max(1, Rp * int(qo[-1]))); comp = np.zeros(max(1, S * Rp), dtype=np.int32)
        info = np.zeros(max(1, P), dtype=np.int32)
        mean = np.empty(max(1, n_mean)) if want_moments else None
        cov = np.empty(max(1, n_cov)) if want_moments else None
        out_off = np.zeros(P + 1, dtype=np.int64); cov_off = np.zeros(P + 1, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        self._check(self._lib.agp_predict_sample_series_batch(
            self._ctx, *_series_ctypes(packed, qpack), _dp(slope), _dp(icpt), _dp(weights), R,
            (seeds if S else np.zeros(1, dtype=np.uint64)).ctypes.data_as(C.POINTER(C.c_uint64)), _ip(component),
            _dp(z if z is None or z.size else np.zeros(1)), _dp(x), _ip(comp), _dp(mean), out_off.ctypes.data_as(i64), _dp(cov),
            cov_off.ctypes.data_as(i64), _ip(info)))
        info = info[:P]
        _raise_first_bad(info, check)
        xs_ = [x[Rp * qo[s]:Rp * qo[s + 1]].reshape(Rp, qo[s + 1] - qo[s]).T for s in range(S)]
        if want_moments:
            mean = [mean[out_off[p]:out_off[p + 1]] for p in range(P)]
            cov = [cov[cov_off[p]:cov_off[p + 1]].reshape(len(mean[p]), len(mean[p])).T for p in range(P)]
        return SeriesSamples(xs_, comp[:S * Rp].reshape(S, Rp), mean, cov, info)

    def predict_sum_series_batch(self, series, queries, split_nodes, noises, series_index, q=(), y_transforms=None, noise_pred=None,
                                 want_var=False, want_logpdf=False, check=True, programs=None):
        """agp_predict_sum_series_batch: the decompositions of many short series in one fused launch — predict_sum_batch's twin for
        callers that hold one model per short series, with predict_series_batch's series / query arguments and statelessness.
        split_nodes holds each particle's M component kernels (P lists of M nodes, e.g. split_kernel_sop of its kernel); particle p
        decomposes series[series_index[p]] at queries[series_index[p]].  q: the quantiles (a sequence, possibly empty);
        y_transforms: one (slope, intercept) per series (scaled = slope * raw + intercept; None: (1, 0)); noise_pred: None (each
        particle's noise), a scalar or one per particle — it goes on the observable rows only.  Returns SeriesSums(mean, var, x,
        logpdf, info): mean[p] ((M+1) m_s,) the raw means of the rows F_1 .. F_M, X with predict_mvn_sum's intercept correction on
        F_1, var[p] their raw variances (want_var, else None), x[p] ((M+1) m_s, nq) their Normal quantiles — views cut from the
        particle-major arrays, so np.stack of the adjacent particles of one series is the block mixture_quantile takes — logpdf (P,)
        with want_logpdf; info (P,): a bad pivot, or n_s + j for the first joint row j (1-based) without a raw marginal.
        programs: the components encoded beforehand — gp.encode_batch of the P M component kernels, particle by particle — in
        place of split_nodes (then ignored)."""
        noises = _f64(noises)
        if programs is not None:
            P = noises.shape[0] if noises.ndim == 1 else -1
            M, rest = divmod(programs[0].shape[0] - 1, P) if P > 0 else (1, programs[0].shape[0] - 1)
            if rest != 0 or M < 1:
                raise ValueError("programs must hold the same number (>= 1) of components for every particle")
        else:
            split_nodes = [list(c) for c in split_nodes]
            P = len(split_nodes)
            M = len(split_nodes[0]) if P else 1
            if M < 1 or any(len(c) != M for c in split_nodes):
                raise ValueError("every particle must have the same number (>= 1) of components")
            programs = _gp.encode_batch([nd for c in split_nodes for nd in c]) if P else (np.zeros(1, np.int32), np.zeros(1, np.uint8),
                                                                                         np.zeros(1, np.int32), np.zeros(1))
        pt_off, ts, xs = pack_series(series)
        S = pt_off.shape[0] - 1
        if noises.shape != (P,):
            raise ValueError("one noise per particle required")
        sidx = np.ascontiguousarray(np.asarray(series_index, dtype=np.int32))
        if sidx.shape != (P,):
            raise ValueError("one series index per particle required")
        qpack = pack_queries(queries, S, _particle_noise_pred(noise_pred, P), P)
        slope, icpt = _series_transforms(y_transforms, S)
        qa = _f64(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        if qa.ndim != 1:
            raise ValueError("q must be a sequence of quantiles")
        nq = qa.shape[0]
        m_s = np.diff(qpack[0])
        total = (M + 1) * int(sum(m_s[i] for i in sidx if 0 <= i < S))      # (an index outside is the library's to report)
        mean = np.empty(max(1, total)); var = np.empty(max(1, total)) if want_var else None
        x = np.empty(max(1, total * nq)) if nq else None
        out_off = np.zeros(P + 1, dtype=np.int64)
        lp = np.empty(max(1, P), dtype=np.float64) if want_logpdf else None
        info = np.zeros(max(1, P), dtype=np.int32)
        a = _series_ctypes((pt_off, ts, xs, programs, P, noises, sidx), qpack)      # (.., ts_pred | P | series, ..): M travels behind P
        self._check(self._lib.agp_predict_sum_series_batch(
            self._ctx, *a[:7], M, *a[7:], _dp(slope), _dp(icpt), _dp(qa) if nq else None, nq, _dp(mean), _dp(var), _dp(x),
            out_off.ctypes.data_as(C.POINTER(C.c_int64)), _dp(lp), _ip(info)))
        info = info[:P]
        _raise_first_bad(info, check)
        oo = out_off.tolist()
        cut = lambda arr: [arr[oo[p]:oo[p + 1]] for p in range(P)]
        xs_ = [x[nq * oo[p]:nq * oo[p + 1]].reshape(oo[p + 1] - oo[p], nq) if nq else np.empty((oo[p + 1] - oo[p], 0)) for p in range(P)]
        return SeriesSums(cut(mean), cut(var) if want_var else None, xs_, lp[:P] if want_logpdf else None, info)

    def logpdf_batch_extend(self, nodes, noises, n=None, check=True, programs=None):
        """agp_logpdf_batch_extend: like logpdf_batch, but the factors stay resident and a later call on a longer
        prefix of the same data only computes the new tile rows (data annealing, add_data!)."""
        n = self.n_max if n is None else int(n)
        op_off, ops, prm_off, prm = programs if programs is not None else _gp.encode_batch(nodes)
        P = op_off.shape[0] - 1
        noises = _f64(noises)
        if noises.shape != (P,):
            raise ValueError("one noise per particle required")
        out = np.empty(P, dtype=np.float64); info = np.empty(P, dtype=np.int32)
        self._check(self._lib.agp_logpdf_batch_extend(self._ctx, n, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                                      _dp(noises), _dp(out), _ip(info)))
        _raise_first_bad(info, check)
        return out, info

    def extend_stats(self):
        """dict(extended, from_scratch, tile_rows_reused, tile_rows_total, evicted_before_reuse, slots, callers, occupied,
        capacity_tile_rows, growth_copies) (agp_extend_stats2)."""
        out = (C.c_int64 * 10)()
        self._check(self._lib.agp_extend_stats2(self._ctx, out, 10))
        return dict(zip(("extended", "from_scratch", "tile_rows_reused", "tile_rows_total", "evicted_before_reuse", "slots", "callers", "occupied",
                         "capacity_tile_rows", "growth_copies"), [int(v) for v in out]))

    def predict_reuse_stats(self):
        """dict(reused, factored): particles a predictive pass served from a resident factor / factored itself."""
        out = (C.c_int64 * 2)()
        self._check(self._lib.agp_predict_reuse_stats(self._ctx, out))
        return {"reused": int(out[0]), "factored": int(out[1])}

    def grad_reuse_stats(self):
        """dict(reused, factored): particles a gradient sweep served from a resident factor / factored itself."""
        out = (C.c_int64 * 2)()
        self._check(self._lib.agp_grad_reuse_stats(self._ctx, out))
        return {"reused": int(out[0]), "factored": int(out[1])}

    def lag_stats(self):
        """(resident series is a regular grid and the lag-table path is on, sweeps that took it)."""
        r = C.c_int32(); k = C.c_int64()
        self._check(self._lib.agp_get_lag_stats(self._ctx, C.byref(r), C.byref(k)))
        return bool(r.value), int(k.value)

    def eval_stats(self):
        """How the particles of the last batch sweep got their covariance tiles (agp_get_eval_stats): dict(one_node, chain, stack:
        evaluated inside the factorisation kernels as one-node programs / as chains in place / by the stack interpreter; prebuilt:
        tiles from the tile builder; prebuilt_chain: the multi-node chains among those, which the builder evaluates without a stack)."""
        out = (C.c_int64 * 5)()
        self._check(self._lib.agp_get_eval_stats(self._ctx, out))
        return dict(zip(("one_node", "chain", "stack", "prebuilt", "prebuilt_chain"), (int(v) for v in out)))

    def lattice_stats(self):
        """dict(kind, n_lattice, spacing) of the resident series: kind 0 irregular (general path), 1 regular grid, 2 lattice with
        gaps (calendar-indexed series: table-driven sweeps over n_lattice lags), 3 a longer lattice served by compact tables."""
        k = C.c_int32(); g = C.c_int64(); h = C.c_double()
        self._check(self._lib.agp_get_lattice_stats(self._ctx, C.byref(k), C.byref(g), C.byref(h)))
        return {"kind": int(k.value), "n_lattice": int(g.value), "spacing": float(h.value)}

    def compact_stats(self):
        """dict(lags_per_ordinal, table_entries, sweeps): compact lag tables of a long calendar lattice (agp_get_compact_stats)."""
        w = C.c_int32(); e = C.c_int64(); k = C.c_int64()
        self._check(self._lib.agp_get_compact_stats(self._ctx, C.byref(w), C.byref(e), C.byref(k)))
        return {"lags_per_ordinal": int(w.value), "table_entries": int(e.value), "sweeps": int(k.value)}

    def poison_stats(self):
        """dict(bytes, fills): device / pinned memory this context filled with NaN bits so far (AGP_POISON=1 at construction)."""
        b = C.c_int64(); f = C.c_int64()
        self._check(self._lib.agp_get_poison_stats(self._ctx, C.byref(b), C.byref(f)))
        return {"bytes": int(b.value), "fills": int(f.value)}

    def set_lattice(self, on):
        """Admit lattices with gaps at the next set_data (off: regular grids only)."""
        self._check(self._lib.agp_set_lattice(self._ctx, 1 if on else 0))

    def set_reference_arithmetic(self):
        """ONE arithmetic whatever the call order / batch / store state (agp_set_reference_arithmetic); call before set_data."""
        self._check(self._lib.agp_set_reference_arithmetic(self._ctx, 1))

    def set_lag_tables(self, on):
        """Switch the regular-grid lag-table path (takes effect at the next set_data)."""
        self._check(self._lib.agp_set_lag_tables(self._ctx, (1 if on else 0) if isinstance(on, bool) else int(on)))

    def set_lag_rank_tables(self, on):
        """Switch the rank lag tables of caller-order sweeps on a regular grid (prefixes, gradient sweeps)."""
        self._check(self._lib.agp_set_lag_rank_tables(self._ctx, 1 if on else 0))

    def lag_rank_sweeps(self):
        """Sweeps that read stationary subtrees from rank lag tables so far."""
        k = C.c_int64()
        self._check(self._lib.agp_get_lag_rank_stats(self._ctx, C.byref(k)))
        return int(k.value)

    def lag_predict_passes(self):
        """Predictive passes whose query points sat on the series' lattice (rank tables) so far."""
        k = C.c_int64()
        self._check(self._lib.agp_get_lag_predict_stats(self._ctx, C.byref(k)))
        return int(k.value)

    def set_grad_lag_domain(self, on):
        """Switch the lag-domain gradient contraction of regular grids (takes effect at the next gradient sweep)."""
        self._check(self._lib.agp_set_grad_lag_domain(self._ctx, (2 if on else 0) if isinstance(on, bool) else int(on)))

    def grad_lag_domain_particles(self):
        """Particles whose gradient was contracted in the lag domain so far."""
        k = C.c_int64()
        self._check(self._lib.agp_get_grad_lag_domain_stats(self._ctx, C.byref(k)))
        return int(k.value)

    def toeplitz_particles(self):
        """Particles scored by the structured (Toeplitz + rank 2, Schur algorithm) value sweep so far (set_lag_tables(2))."""
        k = C.c_int64()
        self._check(self._lib.agp_get_toeplitz_stats(self._ctx, C.byref(k)))
        return int(k.value)

    def predict_structured_particles(self):
        """Particles of predictive passes served without a dense factor (joint Schur recursion) so far."""
        k = C.c_int64()
        self._check(self._lib.agp_get_predict_structured_stats(self._ctx, C.byref(k)))
        return int(k.value)

    def grad_structured_particles(self):
        """... of which: without any dense factor (Schur recursion + backward substitution; AGP_GRAD_FFT >= 3)."""
        k = C.c_int64()
        self._check(self._lib.agp_get_grad_structured_stats(self._ctx, C.byref(k)))
        return int(k.value)

    def grad_toeplitz_particles(self):
        """... of which: lag sums of K^-1 from the Toeplitz solves (the sweep's points were consecutive grid points)."""
        k = C.c_int64()
        self._check(self._lib.agp_get_grad_toeplitz_stats(self._ctx, C.byref(k)))
        return int(k.value)

    def set_factor_cache(self, on):
        """Whether coalesced agp_logpdf batches leave their factors in the store (default on)."""
        self._check(self._lib.agp_set_factor_cache(self._ctx, 1 if on else 0))

    def extend_reset(self, release_memory=False):
        self._check(self._lib.agp_extend_reset(self._ctx, 1 if release_memory else 0))

    def extend_reserve(self, n_cap, n_slots):
        self._check(self._lib.agp_extend_reserve(self._ctx, int(n_cap), int(n_slots)))

    def logpdf_grad_batch(self, nodes, noises, n=None, check=True, programs=None):
        """(logpdf[P], grads, grad_noise[P], info[P]); grads[p] is d logpdf / d theta in the order of
        gp.encode(node)[1] (transformed parameters; ChangePoint contributes location, scale)."""
        n = self.n_max if n is None else int(n)
        op_off, ops, prm_off, prm = programs if programs is not None else _gp.encode_batch(nodes)
        P = op_off.shape[0] - 1
        noises = _f64(noises)
        out = np.empty(P); info = np.empty(P, dtype=np.int32); gn = np.empty(P)
        grad = np.zeros(max(1, int(prm_off[-1])))
        self._check(self._lib.agp_logpdf_grad_batch(self._ctx, n, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm), _dp(noises),
                                                    _dp(out), _dp(grad), _dp(gn), _ip(info)))
        _raise_first_bad(info, check)
        return out, [grad[prm_off[i]:prm_off[i + 1]] for i in range(P)], gn, info

    def logpdf_batch_device(self, programs, noises, n, d_out_ptr, d_info_ptr, stream_ptr=0):
        """Results stay in device memory (raw pointers, e.g. torch tensors' data_ptr())."""
        op_off, ops, prm_off, prm = programs
        P = op_off.shape[0] - 1
        noises = _f64(noises)
        self._check(self._lib.agp_logpdf_batch_device(self._ctx, int(n), P, _ip(op_off), _u8(ops), _ip(prm_off),
                                                      _dp(prm), _dp(noises), C.c_void_p(d_out_ptr),
                                                      C.c_void_p(d_info_ptr), C.c_void_p(stream_ptr)))

    # -- predictive path (src/GP.jl:731-758) -------------------------------------------------
    def _predict_args(self, nodes, noises, ts_pred, n, noise_pred, mean_train, mean_pred):
        """What the resident predict_* methods hand to the library: (n, programs, P, noises, ts_pred, m, noise_pred per particle or None,
        mean_train, mean_pred)."""
        n = self.n_max if n is None else int(n)
        programs = _gp.encode_batch(nodes)
        P = programs[0].shape[0] - 1
        noises = _f64(noises); ts_pred = _f64(ts_pred)
        npred = None if noise_pred is None else _f64(np.broadcast_to(noise_pred, (P,)))
        mt = None if mean_train is None else _f64(mean_train)
        mp_ = None if mean_pred is None else _f64(mean_pred)
        return n, programs, P, noises, ts_pred, ts_pred.shape[0], npred, mt, mp_

    def predict_batch(self, nodes, noises, ts_pred, n=None, noise_pred=None, mean_train=None, mean_pred=None,
                      want_cov=False, check=True):
        n, (op_off, ops, prm_off, prm), P, noises, ts_pred, m, npred, mt, mp_ = self._predict_args(nodes, noises, ts_pred, n, noise_pred,
                                                                                                   mean_train, mean_pred)
        mean = np.empty((P, m)); var = np.empty((P, m))
        cov = np.empty((P, m, m)) if want_cov else None
        info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_predict_batch(self._ctx, n, _dp(ts_pred), m, P, _ip(op_off), _u8(ops),
                                                _ip(prm_off), _dp(prm), _dp(noises), _dp(npred), _dp(mt), _dp(mp_),
                                                _dp(mean), _dp(var), _dp(cov), _ip(info)))
        _raise_first_bad(info, check)
        return mean, var, cov, info

    def predict_logpdf_batch(self, nodes, noises, ts_pred, y_pred, n=None, noise_pred=None, mean_train=None, mean_pred=None,
                             check=True):
        """logpdf(MvNormal(node, noise, ts[1:n], xs[1:n], ts_pred; noise_pred, mean), y_pred) per particle (src/api.jl:693,
        test/experiment_hmc.jl:125) without forming the predictive covariance.  Returns (logp[P], info[P]); info = n + k: the
        predictive covariance's leading minor k is not positive definite (logp NaN wherever info != 0)."""
        n, (op_off, ops, prm_off, prm), P, noises, ts_pred, m, npred, mt, mp_ = self._predict_args(nodes, noises, ts_pred, n, noise_pred,
                                                                                                   mean_train, mean_pred)
        y_pred = _f64(y_pred)
        if y_pred.shape != (m,):
            raise ValueError(f"y_pred has shape {y_pred.shape}, ts_pred {ts_pred.shape}")
        logp = np.empty(P); info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_predict_logpdf_batch(self._ctx, n, _dp(ts_pred), _dp(y_pred), m, P, _ip(op_off), _u8(ops),
                                                       _ip(prm_off), _dp(prm), _dp(noises), _dp(npred), _dp(mt), _dp(mp_),
                                                       _dp(logp), _ip(info)))
        _raise_first_bad(info, check)
        return logp, info

    # -- mixture quantiles (src/api.jl:547-596) -----------------------------------------------
    def mixture_quantile(self, means, vars, weights, q, tol=1e-5, max_iter=10**6):
        """Statistics.quantile(::MixtureModel, q; tol, max_iter) (src/api.jl:559-596) per point: means / vars of shape (P, m) (the
        layout predict_batch returns), weights (P,), q a scalar or a vector.  Returns (x, converged, iters), each of shape (m, nq)
        — (m,) for a scalar q; the reference's `success` is converged.all()."""
        means = _f64(means); vars = _f64(vars); weights = _f64(weights)
        if means.ndim != 2 or vars.shape != means.shape or weights.shape != (means.shape[0],):
            raise ValueError(f"means {means.shape}, vars {vars.shape}, weights {weights.shape}: expected (P, m), (P, m), (P,)")
        P, m = means.shape
        qa = _f64(np.atleast_1d(q)); nq = qa.shape[0]
        x = np.empty((nq, m)); conv = np.zeros((nq, m), dtype=np.int32); iters = np.zeros((nq, m), dtype=np.int32)
        self._check(self._lib.agp_mixture_quantile(self._ctx, m, P, _dp(means), _dp(vars), _dp(weights), _dp(qa), nq, float(tol),
                                                   int(max_iter), _dp(x), _ip(conv), _ip(iters)))
        return _quantile_shape(q, x, conv, iters)

    def predict_quantile_batch(self, nodes, noises, ts_pred, weights, q, n=None, noise_pred=None, mean_train=None, mean_pred=None,
                               y_transform=(1.0, 0.0), tol=1e-5, max_iter=10**6, check=True):
        """predict_quantile (src/api.jl:547-557) on the resident series: the mixture, with `weights`, of every particle's marginal
        predictive mapped to the raw space of y_transform = (slope, intercept), searched per point by the device.  Returns (x,
        converged, iters, info), x / converged / iters shaped as mixture_quantile's; info = n + j: the raw marginal variance at
        query j (1-based) is negative or NaN.  If any info != 0, x is NaN (PosDefException when check)."""
        n, (op_off, ops, prm_off, prm), P, noises, ts_pred, m, npred, mt, mp_ = self._predict_args(nodes, noises, ts_pred, n, noise_pred,
                                                                                                   mean_train, mean_pred)
        weights = _f64(weights)
        if weights.shape != (P,):
            raise ValueError(f"weights has shape {weights.shape}, expected ({P},)")
        slope, intercept = (float(v) for v in y_transform)
        qa = _f64(np.atleast_1d(q)); nq = qa.shape[0]
        x = np.empty((nq, m)); conv = np.zeros((nq, m), dtype=np.int32); iters = np.zeros((nq, m), dtype=np.int32)
        info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_predict_quantile_batch(self._ctx, n, _dp(ts_pred), m, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                                         _dp(noises), _dp(npred), _dp(mt), _dp(mp_), _dp(weights), slope, intercept,
                                                         _dp(qa), nq, float(tol), int(max_iter), _dp(x), _ip(conv), _ip(iters),
                                                         _ip(info)))
        _raise_first_bad(info, check)
        return _quantile_shape(q, x, conv, iters) + (info,)

    # -- posterior predictive samples (src/api.jl:497-522 + Distributions' rand) -------------------------------------------
    def predict_sample_batch(self, nodes, noises, ts_pred, weights, n_samples, seed=0, n=None, noise_pred=None, mean_train=None,
                             mean_pred=None, y_transform=(1.0, 0.0), component=None, z=None, check=True):
        """rand(MixtureModel(MvNormal_p, weights), n_samples) of every particle's predictive at ts_pred on the resident series, in the
        raw space of y_transform = (slope, intercept) (agp_predict_sample_batch).  component (n_samples,) and z (m, n_samples) are
        optional: the components / standard normals to use instead of the seeded draws.  Returns (x, component, info): x of shape
        (m, n_samples) (column s is sample s), the component of each sample, info[P] (n + k: leading minor k of a predictive covariance
        is not positive definite; x is NaN everywhere if any info != 0, PosDefException when check)."""
        n, (op_off, ops, prm_off, prm), P, noises, ts_pred, m, npred, mt, mp_ = self._predict_args(nodes, noises, ts_pred, n, noise_pred,
                                                                                                   mean_train, mean_pred)
        weights = _f64(weights)
        S = int(n_samples)
        if weights.shape != (P,):
            raise ValueError(f"weights has shape {weights.shape}, expected ({P},)")
        cin = None if component is None else np.ascontiguousarray(component, dtype=np.int32)
        if cin is not None and cin.shape != (S,):
            raise ValueError(f"component has shape {cin.shape}, expected ({S},)")
        zin = None
        if z is not None:
            z = np.asarray(z, dtype=np.float64)
            if z.shape != (m, S):
                raise ValueError(f"z has shape {z.shape}, expected ({m}, {S})")
            zin = np.ascontiguousarray(z.T)          # (sample s's m normals contiguous)
        slope, intercept = (float(v) for v in y_transform)
        xt = np.empty((max(S, 0), m)); comp = np.zeros(max(S, 0), dtype=np.int32); info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_predict_sample_batch(self._ctx, n, _dp(ts_pred), m, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                                       _dp(noises), _dp(npred), _dp(mt), _dp(mp_), _dp(weights), slope, intercept,
                                                       S, int(seed) & (2**64 - 1), _ip(cin), _dp(zin), _dp(xt), _ip(comp), _ip(info)))
        _raise_first_bad(info, check)
        return xt.T, comp, info

    # -- mixture moments (Distributions.mean / var / cov of predict_mvn's MixtureModel) ------------------------------------
    def mixture_moments(self, means, weights, vars=None, covs=None, space=0, want_cov=None):
        """mean / var / cov of MixtureModel(components, weights) (agp_mixture_moments): means (P, m), and either vars (P, m) (marginal
        moments) or covs (P, m, m).  space 0: normal components; 1: MvLogNormal(N(means, covs)) components.  Returns (mean (m,),
        var (m,), cov (m, m) or None); cov when covs is given unless want_cov=False."""
        means = _f64(means); weights = _f64(weights)
        if means.ndim != 2 or weights.shape != (means.shape[0],):
            raise ValueError(f"means {means.shape}, weights {weights.shape}: expected (P, m), (P,)")
        P, m = means.shape
        if covs is not None:
            covs = _f64(covs)
            if covs.shape != (P, m, m):
                raise ValueError(f"covs has shape {covs.shape}, expected ({P}, {m}, {m})")
        if vars is not None:
            vars = _f64(vars)
            if vars.shape != (P, m):
                raise ValueError(f"vars has shape {vars.shape}, expected ({P}, {m})")
        want_cov = covs is not None if want_cov is None else bool(want_cov)
        mean = np.empty(m); var = np.empty(m); cov = np.empty((m, m)) if want_cov else None
        self._check(self._lib.agp_mixture_moments(self._ctx, m, P, _dp(means), _dp(vars), _dp(covs), _dp(weights), int(space),
                                                  _dp(mean), _dp(var), _dp(cov)))
        return mean, var, cov

    def predict_mixture_batch(self, nodes, noises, ts_pred, weights, n=None, noise_pred=None, mean_train=None, mean_pred=None,
                              y_transform=(1.0, 0.0), space=0, want_cov=False, check=True):
        """mean / var / cov of predict_mvn's MixtureModel on the resident series (agp_predict_mixture_batch), in the raw space of
        y_transform = (slope, intercept); space 1: of its MvLogNormal re-wrap.  want_cov: the fused covariance pass (no per-particle
        covariance leaves the device).  Returns (mean (m,), var (m,), cov (m, m) or None, info (P,)); everything is NaN if any info != 0
        (PosDefException when check)."""
        n, (op_off, ops, prm_off, prm), P, noises, ts_pred, m, npred, mt, mp_ = self._predict_args(nodes, noises, ts_pred, n, noise_pred,
                                                                                                   mean_train, mean_pred)
        weights = _f64(weights)
        if weights.shape != (P,):
            raise ValueError(f"weights has shape {weights.shape}, expected ({P},)")
        slope, intercept = (float(v) for v in y_transform)
        mean = np.empty(m); var = np.empty(m); cov = np.empty((m, m)) if want_cov else None
        info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_predict_mixture_batch(self._ctx, n, _dp(ts_pred), m, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                                        _dp(noises), _dp(npred), _dp(mt), _dp(mp_), _dp(weights), slope, intercept,
                                                        int(space), _dp(mean), _dp(var), _dp(cov), _ip(info)))
        _raise_first_bad(info, check)
        return mean, var, cov, info

    # -- sum-of-GPs posterior (src/GP.jl:904-993) ---------------------------------------------
    def infer_gp_sum(self, nodes, noise, ts_pred, n=None, noise_pred=None, check=True):
        """Returns (mean[(M+1)p], cov[(M+1)p, (M+1)p], indexes_F (list of slices), indexes_X (slice))."""
        n = self.n_max if n is None else int(n)
        op_off, ops, prm_off, prm = _gp.encode_batch(nodes)
        M = len(nodes); ts_pred = _f64(ts_pred); p = ts_pred.shape[0]
        ma = (M + 1) * p
        mean = np.empty(ma); cov = np.empty((ma, ma)); info = C.c_int32()
        npred = float(noise) if noise_pred is None else float(noise_pred)
        self._check(self._lib.agp_infer_gp_sum(self._ctx, n, _dp(ts_pred), p, M, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                               float(noise), npred, _dp(mean), _dp(cov), C.byref(info)))
        if check and info.value > 0:
            raise PosDefException(info.value)
        return mean, cov, [slice(i * p, (i + 1) * p) for i in range(M)], slice(M * p, ma)

    def _sum_batch_args(self, split_nodes, noises, ts_pred, n, noise_pred):
        """CSR programs of P particles x M components (split_nodes: P lists of M nodes), noises, ts_pred, noise_pred per particle."""
        split_nodes = [list(c) for c in split_nodes]
        P = len(split_nodes)
        M = len(split_nodes[0]) if P else 0
        if any(len(c) != M for c in split_nodes):
            raise ValueError("every particle must have the same number of components")
        op_off, ops, prm_off, prm = _gp.encode_batch([nd for c in split_nodes for nd in c])
        noises = _f64(noises)
        if noises.shape != (P,):
            raise ValueError(f"noises has shape {noises.shape}, expected ({P},)")
        npred = None if noise_pred is None else _f64(np.broadcast_to(noise_pred, (P,)))
        n = self.n_max if n is None else int(n)
        return n, P, M, op_off, ops, prm_off, prm, noises, _f64(ts_pred), npred

    def infer_gp_sum_batch(self, split_nodes, noises, ts_pred, n=None, noise_pred=None, want_cov=False, check=True):
        """GP.infer_gp_sum per particle (src/GP.jl:904-993) in one call: split_nodes holds each particle's M component kernels (e.g.
        split_kernel_sop of its kernel), noises its noise; noise_pred None = each particle's own noise.  Returns (mean (P, (M+1)p),
        var (P, (M+1)p), cov (P, (M+1)p, (M+1)p) or None, info (P,), indexes_F (list of slices), indexes_X (slice))."""
        n, P, M, op_off, ops, prm_off, prm, noises, ts_pred, npred = self._sum_batch_args(split_nodes, noises, ts_pred, n, noise_pred)
        p = ts_pred.shape[0]; ma = (M + 1) * p
        mean = np.empty((P, ma)); var = np.empty((P, ma)); cov = np.empty((P, ma, ma)) if want_cov else None
        info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_infer_gp_sum_batch(self._ctx, n, _dp(ts_pred), p, P, M, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                                     _dp(noises), _dp(npred), _dp(mean), _dp(var), _dp(cov), _ip(info)))
        _raise_first_bad(info, check)
        return mean, var, cov, info, [slice(i * p, (i + 1) * p) for i in range(M)], slice(M * p, ma)

    def predict_sum_batch(self, split_nodes, noises, ts_pred, q=(), n=None, noise_pred=None, y_transform=(1.0, 0.0), check=True):
        """predict_sum's numbers (src/api.jl:898-1034) per particle: raw means of the rows (F_1 .. F_M, X) with predict_mvn_sum's
        intercept correction on F_1, and their marginal quantiles, computed on the device.  y_transform = (slope, intercept).
        Returns (mean (P, (M+1)p), x (P, (M+1)p, nq), info (P,)); info = n + j: joint row j (1-based) has no raw marginal."""
        n, P, M, op_off, ops, prm_off, prm, noises, ts_pred, npred = self._sum_batch_args(split_nodes, noises, ts_pred, n, noise_pred)
        p = ts_pred.shape[0]; ma = (M + 1) * p
        qa = _f64(np.atleast_1d(np.asarray(q, dtype=np.float64))); nq = qa.shape[0]
        slope, intercept = (float(v) for v in y_transform)
        mean = np.empty((P, ma)); x = np.empty((P, ma, nq)); info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_predict_sum_batch(self._ctx, n, _dp(ts_pred), p, P, M, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                                    _dp(noises), _dp(npred), slope, intercept, _dp(qa) if nq else None, nq, _dp(mean),
                                                    _dp(x) if nq else None, _ip(info)))
        _raise_first_bad(info, check)
        return mean, x, info

    # -- matrix assembly (src/GP.jl:666-668) -------------------------------------------------
    def cov_matrix(self, node, noise, ts):
        ts = _f64(ts); n = ts.shape[0]
        ops, prm = _gp.encode(node)
        out = np.empty((n, n), dtype=np.float64, order="F")
        prm_arg = prm if prm.size else np.zeros(1)
        self._check(self._lib.agp_cov_matrix(self._ctx, _dp(ts), n, _u8(ops), ops.size, _dp(prm_arg), prm.size,
                                             float(noise), _dp(out)))
        return np.asarray(out)

    # -- measurement / debug hooks -----------------------------------------------------------
    def debug_cholesky(self, K):
        K = np.asfortranarray(np.asarray(K, dtype=np.float64)); n = K.shape[0]
        L = np.empty((n, n), dtype=np.float64, order="F"); info = C.c_int32()
        self._check(self._lib.agp_debug_cholesky(self._ctx, _dp(K), n, _dp(L), C.byref(info)))
        return np.asarray(L), info.value

    def debug_factor_batch(self, K, y=None, schedule=-1):
        """Factor the symmetric matrices K (P, n, n) with one schedule of the batched Cholesky (agp_debug_factor_batch: 0 mixed
        per-column launches, 1 split, 2 right-looking, 3 hybrid, 4 dataflow, -1 logpdf_batch's choice) -> L (P, n, n) lower,
        beta = L^-1 y (P, n), partial (P, 2) = [log det, beta'beta], info (P)."""
        K = np.ascontiguousarray(K, dtype=np.float64)
        if K.ndim != 3 or K.shape[1] != K.shape[2]:
            raise ValueError("K must have shape (P, n, n)")
        P, n = K.shape[0], K.shape[1]
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            if y.shape != (P, n):
                raise ValueError("y must have shape (P, n)")
        Lt = np.empty((P, n, n), dtype=np.float64); beta = np.empty((P, n), dtype=np.float64)
        part = np.empty((P, 2), dtype=np.float64); info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_debug_factor_batch(self._ctx, _dp(K), _dp(y), n, P, int(schedule), _dp(Lt), _dp(beta), _dp(part),
                                                     _ip(info)))
        # (column-major blocks: the transpose of each block is the row-major lower factor)
        return np.ascontiguousarray(Lt.transpose(0, 2, 1)), beta, part, info

    def debug_series_factor(self, K, y=None):
        """Factor the matrices K (P, n, n), 1 <= n <= SERIES_MAX_N (lower triangles read), with the Cholesky of logpdf_series_batch's
        kernel (agp_debug_series_factor: the kernel's probe instantiation — the production statements on caller matrices) ->
        L (P, n, n) lower, alpha = L^-1 y (P, n), partial (P, 2) = [2 sum log L_ii, alpha'alpha], logpdf (P), info (P)."""
        return self._series_factor(self._lib.agp_debug_series_factor, K, y)

    def debug_long_series_factor(self, K, y=None):
        """Factor the matrices K (P, n, n), 1 <= n <= LONG_SERIES_MAX_N, P <= 256 (lower triangles read), with the block Cholesky of
        logpdf_long_series_batch's long kernel (agp_debug_long_series_factor: the kernel's probe instantiation — the production
        statements on caller matrices, the factor in the HBM workspace) -> what debug_series_factor returns:
        L (P, n, n) lower, alpha = L^-1 y (P, n), partial (P, 2) = [2 sum log L_ii, alpha'alpha], logpdf (P), info (P)."""
        return self._series_factor(self._lib.agp_debug_long_series_factor, K, y)

    def _series_factor(self, entry, K, y):
        K = np.ascontiguousarray(K, dtype=np.float64)
        if K.ndim != 3 or K.shape[1] != K.shape[2]:
            raise ValueError("K must have shape (P, n, n)")
        P, n = K.shape[0], K.shape[1]
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            if y.shape != (P, n):
                raise ValueError("y must have shape (P, n)")
        L = np.empty((P, n, n), dtype=np.float64); alpha = np.empty((P, n), dtype=np.float64)
        part = np.empty((P, 2), dtype=np.float64); lp = np.empty(P, dtype=np.float64); info = np.zeros(P, dtype=np.int32)
        self._check(entry(self._ctx, _dp(K), _dp(y), n, P, _dp(L), _dp(alpha), _dp(part), _dp(lp), _ip(info)))
        return L, alpha, part, lp, info

    def debug_remove_factor(self, L0, alpha0, idx):
        """The update of remove_data on the caller's factors L0 (P, n, n; lower triangles read) and forward-solve vectors alpha0
        (P, n) or None (zeros), positions idx ascending (agp_debug_remove_factor: the production host function and kernels on
        arrays of the store's layout, partials and inverse blocks seeded with the sentinel -7) -> with n' = n - len(idx),
        nt' = ceil(n' / 128), np' = 128 nt': L (P, np', np') the padded factor as it lies in the tiles, alpha (P, np'),
        partial (P, nt', 2) = [2 sum log L_ii, sum alpha_i^2] per tile column, winv (P, nt', 8, 16, 16) the inverses of the pivot
        blocks as matrices, info (P)."""
        L0 = np.ascontiguousarray(L0, dtype=np.float64)
        if L0.ndim != 3 or L0.shape[1] != L0.shape[2]:
            raise ValueError("L0 must have shape (P, n, n)")
        P, n = L0.shape[0], L0.shape[1]
        if alpha0 is not None:
            alpha0 = np.ascontiguousarray(alpha0, dtype=np.float64)
            if alpha0.shape != (P, n):
                raise ValueError("alpha0 must have shape (P, n)")
        idx = np.ascontiguousarray(idx, dtype=np.int64).ravel()
        nt = max(1, -(-(n - idx.size) // 128)); npad = 128 * nt
        L = np.empty((P, npad, npad), dtype=np.float64); alpha = np.empty((P, npad), dtype=np.float64)
        part = np.empty((P, nt, 2), dtype=np.float64); winv = np.empty((P, nt, 8, 16, 16), dtype=np.float64)
        info = np.zeros(P, dtype=np.int32)
        self._check(self._lib.agp_debug_remove_factor(self._ctx, _dp(L0), _dp(alpha0), n, P, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      idx.size, _dp(L), _dp(alpha), _dp(part), _dp(winv), _ip(info)))
        # (column-major blocks: the transpose of each is the inverse as a matrix)
        return L, alpha, part, np.ascontiguousarray(winv.transpose(0, 1, 2, 4, 3)), info

    def debug_toeplitz(self, mode, r, x, noise, m_future=0, r2=None, const=None, wn=None, lin=None, rank0=0, grid_h=1.0, grid_mid=0.0,
                       t_ref=0.0, raw=None):
        """The structured sweeps' launcher on caller first columns (agp_debug_toeplitz: launch_toep_logpdf itself, programs and
        rank-layout tables built from the arguments, every output seeded with the sentinel -7).  mode 0 value, 1 gradient,
        2 predictive; r (P, N) first columns without noise, N = n + m_future (mode 2) or n = len(x); noise (P).  Per particle,
        None = absent: r2 = (mask (P) bool, rows (mask.sum(), N)) second tables of the masked particles (the kernel adds the two
        tables entry by entry), const / wn (P) values with NaN = no leaf, lin a list of P lists of up to two (centre, bias, amp);
        raw = (particle, opcode) plants one more leaf.  -> dict(lp, info; modes 1, 2: Lcols (P, n(n+1)/2 + 16) packed columns
        and their guard, fwd, sol (P, 4, ldv); mode 2: pacc (P, 4, pstride))."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        if r.ndim != 2:
            raise ValueError("r must have shape (P, N)")
        P, N = r.shape
        n = x.size
        if mode == 2:
            if N != n + m_future:
                raise ValueError("r must have n + m_future columns")
        elif N != n or m_future:
            raise ValueError("r must have n columns (m_future belongs to mode 2)")
        noise = np.ascontiguousarray(np.broadcast_to(np.asarray(noise, dtype=np.float64), (P,)))
        leaves = np.zeros(P, dtype=np.int32)
        r2a = None
        if r2 is not None:
            mask, rows = r2
            mask = np.asarray(mask, dtype=bool)
            r2a = np.zeros((P, N)); r2a[mask] = rows
            leaves[mask] |= 1
        cv = wv = None
        if const is not None:
            cv = np.ascontiguousarray(const, dtype=np.float64); leaves[~np.isnan(cv)] |= 2
        if wn is not None:
            wv = np.ascontiguousarray(wn, dtype=np.float64); leaves[~np.isnan(wv)] |= 4
        la = None
        if lin is not None:
            la = np.zeros((P, 2, 3))
            for p, ls in enumerate(lin):
                if len(ls) > 2:
                    raise ValueError("at most two Linear leaves per particle")
                for q, l3 in enumerate(ls):
                    la[p, q] = l3
                leaves[p] |= len(ls) << 3
        rp, ro = (-1, 0) if raw is None else raw
        ldv = 128 * -(-n // 128); pstride = max(128, 128 * -(-(N - n) // 128))
        out = dict(lp=np.empty(P), info=np.zeros(P, dtype=np.int32))
        if mode >= 1:
            out.update(Lcols=np.empty((P, n * (n + 1) // 2 + 16)), fwd=np.empty((P, 4, ldv)), sol=np.empty((P, 4, ldv)))
        if mode == 2:
            out["pacc"] = np.empty((P, 4, pstride))
        self._check(self._lib.agp_debug_toeplitz(self._ctx, int(mode), n, N if mode == 2 else 0, P, _dp(r), _dp(r2a), _ip(leaves), _dp(cv),
                                                 _dp(wv), _dp(la), _dp(noise), _dp(x), int(rank0), float(grid_h), float(grid_mid),
                                                 float(t_ref), int(rp), int(ro), _dp(out["lp"]), _ip(out["info"]), _dp(out.get("Lcols")),
                                                 _dp(out.get("fwd")), _dp(out.get("sol")), _dp(out.get("pacc"))))
        return out

    COV_SWEEP_MODES = ("general", "sorted_lag", "rank", "compact_whole", "compact_sorted")
    COV_SWEEP_DECODES = ("one_node", "chain", "stack")

    def debug_cov_sweep(self, nodes, noises, n=None, for_gradient=False, allow_tables=True, want_tables=True, programs=None):
        """The covariance tiles of a sweep over the first n resident points, on whichever table path that sweep takes
        (agp_debug_cov_sweep: the sweep's own stages up to its covariance launch with every tile from the tile builder, tiles and
        tables seeded with the sentinel -7, no factorisation).  -> dict(K (P, n_pad, n_pad) the padded lower tiles as they lie (-7
        where no tile is stored), order (n) the caller's position of sweep row i, mode (one of COV_SWEEP_MODES), tab_units,
        tab_gstride, n_tables, logdt (the GammaExponential leaves read the log|dt| table), depth (4 or 8), decode (P names of
        COV_SWEEP_DECODES); with want_tables also tab (n_tables, entries per table) or None and rep (the entries' times) or None)."""
        n = self.n_max if n is None else int(n)
        op_off, ops, prm_off, prm = programs if programs is not None else _gp.encode_batch(nodes)
        P = op_off.shape[0] - 1
        noises = _f64(noises)
        if noises.shape != (P,):
            raise ValueError("one noise per particle required")
        mode = np.zeros(8 + max(P, 0), dtype=np.int32)

        def call(K, order, tab, rep):
            self._check(self._lib.agp_debug_cov_sweep(self._ctx, n, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm), _dp(noises),
                                                      1 if for_gradient else 0, 1 if allow_tables else 0, _dp(K), _ip(order), _ip(mode),
                                                      _dp(tab), _dp(rep)))
        tab = rep = None
        if want_tables:
            call(None, None, None, None)          # (the sizing call)
            if mode[3] > 0 and mode[4] > 0:
                tab = np.empty((int(mode[3]), int(mode[4]))); rep = np.empty(int(mode[5]))
        npad = 128 * -(-n // 128)
        K = np.empty((P, npad, npad)); order = np.empty(n, dtype=np.int32)
        call(K, order, tab, rep)
        return dict(K=K, order=order, mode=self.COV_SWEEP_MODES[int(mode[0])], tab_units=int(mode[1]), tab_gstride=int(mode[2]),
                    n_tables=int(mode[3]), logdt=bool(mode[6]), depth=int(mode[7]),
                    decode=[self.COV_SWEEP_DECODES[int(v)] for v in mode[8:8 + P]], tab=tab, rep=rep)

    def debug_mfma_probe(self, A, B):
        A = _f64(A).reshape(16, 4); B = _f64(B).reshape(4, 16); D = np.empty((16, 16))
        self._check(self._lib.agp_debug_mfma_probe(self._ctx, _dp(A), _dp(B), _dp(D)))
        return D

    def debug_mfma_peak(self, iters=20000, wg_per_cu=2):
        tf = C.c_double(); ghz = C.c_double()
        self._check(self._lib.agp_debug_mfma_peak(self._ctx, int(iters), int(wg_per_cu), C.byref(tf), C.byref(ghz)))
        return tf.value, ghz.value

    def debug_math(self, which, x, g=None):
        x = _f64(x); y = np.empty_like(x)
        g = None if g is None else _f64(g)
        self._check(self._lib.agp_debug_math(self._ctx, int(which), _dp(x), _dp(g), _dp(y), x.size))
        return y

    def _measurement_only(self, name):
        if not hasattr(self._lib, name):
            raise AGPError(f"{name} exists in the measurement build only: python __graft_entry__.py --experiments, then "
                           f"AUTOGP_HIP_LIB=autogp.jl_amd/lib/libautogp_hip_exp.so")

    def debug_gemm_variant(self, P, nt, k, variant, reps=5):
        self._measurement_only("agp_debug_gemm_variant")
        ms = C.c_double()
        self._check(self._lib.agp_debug_gemm_variant(self._ctx, P, nt, k, variant, reps, C.byref(ms)))
        return ms.value

    def flow_trace(self, enable, max_items):
        """agp_debug_flow_trace: enable=True starts recording; enable=False returns an (items, 8) int64 array."""
        self._measurement_only("agp_debug_flow_trace")
        if enable:
            self._check(self._lib.agp_debug_flow_trace(self._ctx, 1, int(max_items), None))
            return None
        out = np.zeros((int(max_items), 8), dtype=np.int64)
        self._check(self._lib.agp_debug_flow_trace(self._ctx, 0, int(max_items), out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def debug_compact_shards(self, padded, P, n_ranks):
        padded = _f64(padded); out = np.empty(int(P))
        self._check(self._lib.agp_debug_compact_shards(self._ctx, _dp(padded), int(P), int(n_ranks), _dp(out)))
        return out

    def set_profiling(self, on: bool):
        self._check(self._lib.agp_set_profiling(self._ctx, 1 if on else 0))

    def timing(self):
        out = np.zeros(16)
        self._check(self._lib.agp_get_timing(self._ctx, _dp(out), 16))
        keys = ["total_ms", "cov_build_ms", "chol_update_ms", "chol_trsm_ms", "finish_ms", "n_update_launches",
                "n_trsm_launches", "h2d_ms", "grad_trtri_ms", "grad_kinv_ms", "grad_contract_ms", "grad_alpha_finish_ms",
                "sample_normals_ms", "sample_readout_ms", "mixture_pass_ms", "mixture_accumulate_ms"]
        return dict(zip(keys, out.tolist()))

    def launch_times(self, which=0, n=64):
        out = np.zeros(n)
        cnt = self._lib.agp_get_launch_times(self._ctx, which, _dp(out), n)
        return out[:max(0, min(cnt, n))]

    def set_coalesce_window(self, microseconds: int):
        self._check(self._lib.agp_set_coalesce_window(self._ctx, int(microseconds)))

    def coalesce_stats(self):
        a = C.c_int64(); b = C.c_int64()
        self._check(self._lib.agp_get_coalesce_stats(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def dedup_stats(self):
        """(particles submitted, particles evaluated) over the host-output batch calls so far."""
        a = C.c_int64(); b = C.c_int64()
        self._check(self._lib.agp_get_dedup_stats(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def mixture_stats(self):
        """(mixture-moment passes finished, chunks of components their running sums took in) so far."""
        a = C.c_int64(); b = C.c_int64()
        self._check(self._lib.agp_get_mixture_stats(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_workspace_limit(self, nbytes: int):
        self._check(self._lib.agp_set_workspace_limit(self._ctx, int(nbytes)))


def shard_range(P: int, rank: int, n_ranks: int):
    """agp_shard_range: block [lo, hi) of rank `rank` (the C ABI's partition; equals dist.shard_range)."""
    lo = C.c_int32(); hi = C.c_int32()
    load_library().agp_shard_range(int(P), int(rank), int(n_ranks), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def shard_plan(programs, noises, n, n_ranks, sweep=1, regular_grid=True, m_future=0, lattice_kind=None):
    """agp_shard_plan: (owner[P], cost[P], rank_cost[n_ranks]) — cost-aware, duplicate-aware assignment of particles to ranks.
    lattice_kind: 0 irregular, 1 regular grid, 2 lattice with gaps (GPEngine.lattice_stats()["kind"]); the older boolean
    `regular_grid` is used when it is None."""
    op_off, ops, prm_off, prm = programs
    P = op_off.shape[0] - 1
    noises = _f64(noises)
    owner = np.zeros(max(P, 1), dtype=np.int32); cost = np.zeros(max(P, 1)); rc = np.zeros(n_ranks)
    r = load_library().agp_shard_plan(int(n), P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm if prm.size else np.zeros(1)), _dp(noises),
                                      int(sweep), int(lattice_kind) if lattice_kind is not None else (1 if regular_grid else 0), int(m_future), int(n_ranks),
                                      owner.ctypes.data_as(C.POINTER(C.c_int32)), _dp(cost), _dp(rc))
    if r != 0:
        raise AGPError(f"agp_shard_plan failed ({r})")
    return owner[:P], cost[:P], rc


def _ctx_array(engines):
    arr = (C.c_void_p * len(engines))()
    for i, e in enumerate(engines):
        arr[i] = e._ctx.value
    return arr


def logpdf_grad_batch_multi(engines, nodes, noises, n=None, check=True, programs=None, want_owner=False):
    """agp_logpdf_grad_batch_multi over a list of GPEngine objects holding the same data (one per device — or several contexts of one
    device): GPEngine.logpdf_grad_batch's results, the population split by the cost-aware plan inside the entry."""
    lib = load_library()
    n = engines[0].n_max if n is None else int(n)
    op_off, ops, prm_off, prm = programs if programs is not None else _gp.encode_batch(nodes)
    P = op_off.shape[0] - 1
    noises = _f64(noises)
    out = np.empty(P); info = np.empty(P, dtype=np.int32); gn = np.empty(P); owner = np.zeros(max(P, 1), dtype=np.int32)
    grad = np.zeros(max(1, int(prm_off[-1])))
    rc = lib.agp_logpdf_grad_batch_multi(_ctx_array(engines), len(engines), n, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm), _dp(noises),
                                         _dp(out), _dp(grad), _dp(gn), _ip(info), _ip(owner))
    engines[0]._check(rc)
    _raise_first_bad(info, check)
    res = (out, [grad[prm_off[i]:prm_off[i + 1]] for i in range(P)], gn, info)
    return res + (owner[:P],) if want_owner else res


def predict_batch_multi(engines, nodes, noises, ts_pred, n=None, noise_pred=None, mean_train=None, mean_pred=None, want_cov=False,
                        check=True, want_owner=False):
    """agp_predict_batch_multi over a list of GPEngine objects holding the same data: GPEngine.predict_batch's results."""
    lib = load_library()
    n = engines[0].n_max if n is None else int(n)
    op_off, ops, prm_off, prm = _gp.encode_batch(nodes)
    P = op_off.shape[0] - 1
    noises = _f64(noises); ts_pred = _f64(ts_pred); m = ts_pred.shape[0]
    npred = None if noise_pred is None else _f64(np.broadcast_to(noise_pred, (P,)))
    mt = None if mean_train is None else _f64(mean_train)
    mp_ = None if mean_pred is None else _f64(mean_pred)
    mean = np.empty((P, m)); var = np.empty((P, m))
    cov = np.empty((P, m, m)) if want_cov else None
    info = np.zeros(P, dtype=np.int32); owner = np.zeros(max(P, 1), dtype=np.int32)
    rc = lib.agp_predict_batch_multi(_ctx_array(engines), len(engines), n, _dp(ts_pred), m, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                                     _dp(noises), _dp(npred), _dp(mt), _dp(mp_), _dp(mean), _dp(var), _dp(cov), _ip(info), _ip(owner))
    engines[0]._check(rc)
    _raise_first_bad(info, check)
    res = (mean, var, cov, info)
    return res + (owner[:P],) if want_owner else res


def probe_lattice(ts):
    """agp_probe_lattice: the admission test of agp_set_data on its own (host code, no device).  Returns
    dict(kind, n_lattice, spacing, index): kind 0 irregular, 1 regular grid, 2 lattice with gaps; index = per-point lattice index."""
    ts = np.ascontiguousarray(ts, dtype=np.float64)
    k = C.c_int32(); g = C.c_int64(); h = C.c_double()
    idx = np.empty(len(ts), dtype=np.int64)
    rc = load_library().agp_probe_lattice(_dp(ts), len(ts), C.byref(k), C.byref(g), C.byref(h), idx.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise AGPError(f"agp_probe_lattice failed ({rc})")
    return {"kind": int(k.value), "n_lattice": int(g.value), "spacing": float(h.value), "index": idx}


def probe_program(node):
    """agp_probe_program: one kernel tree as a table-driven sweep compiles it (host code, no device).  Returns dict(n_compiled, chain,
    depth, n_tables): length of the compiled postfix program, whether it is a chain (leaf (leaf binop)*: evaluated without a stack),
    its evaluation stack need and its table leaves."""
    ops, prm = _gp.encode(node)
    prm_arg = prm if prm.size else np.zeros(1)
    n = C.c_int32(); ch = C.c_int32(); d = C.c_int32(); nt = C.c_int32()
    rc = load_library().agp_probe_program(_u8(ops), ops.size, _dp(prm_arg), prm.size, C.byref(n), C.byref(ch), C.byref(d), C.byref(nt))
    if rc != 0:
        raise AGPError(f"agp_probe_program failed ({rc})")
    return {"n_compiled": int(n.value), "chain": bool(ch.value), "depth": int(d.value), "n_tables": int(nt.value)}


def _quantile_shape(q, x, conv, iters):
    """(nq, m) C-order results of the quantile entries -> (m, nq), or (m,) for a scalar q."""
    x, conv, iters = x.T.copy(), conv.T.astype(bool), iters.T.copy()
    if np.ndim(q) == 0:
        return x[:, 0], conv[:, 0], iters[:, 0]
    return x, conv, iters


def raw_components(mean, var, info, n, y_transform=(1.0, 0.0)):
    """agp_predict_quantile_batch's step between its two passes, on the host: predict_mvn's raw-space transform (src/api.jl:513-520)
    mean (P, m) -> (mean - intercept) / slope, var -> (1 / slope^2) * var, and info = n + j (1-based) where a particle's raw
    variance at query j is negative or NaN or its raw mean not finite.  Returns (mean_raw, var_raw, info)."""
    slope, intercept = (float(v) for v in y_transform)
    mr = (np.asarray(mean, dtype=np.float64) - intercept) / slope
    vr = (1.0 / (slope * slope)) * np.asarray(var, dtype=np.float64)
    info = np.array(info, dtype=np.int32, copy=True)
    bad = ~(np.isfinite(mr) & (vr >= 0.0))
    for p in np.flatnonzero((info == 0) & bad.any(axis=1)):
        info[p] = int(n) + int(np.argmax(bad[p])) + 1
    return mr, vr, info


def predict_quantile_multi(multi, nodes, noises, ts_pred, weights, q, n=None, noise_pred=None, mean_train=None, mean_pred=None,
                           y_transform=(1.0, 0.0), tol=1e-5, max_iter=10**6, check=True):
    """GPEngine.predict_quantile_batch over several devices: the marginal pass split by agp_predict_batch_multi, the components
    gathered on the host and searched on the first device (agp_mixture_quantile).  Same results."""
    engines = multi.engines if isinstance(multi, GPEngineMulti) else list(multi)
    n = engines[0].n_max if n is None else int(n)
    for v in np.atleast_1d(q):
        if not 0.0 < float(v) < 1.0:
            raise AGPError("quantile must be in (0, 1)")
    mean, var, _, info = predict_batch_multi(engines, nodes, noises, ts_pred, n=n, noise_pred=noise_pred, mean_train=mean_train,
                                             mean_pred=mean_pred, check=False)
    mr, vr, info = raw_components(mean, var, info, n, y_transform)
    _raise_first_bad(info, check)
    if (info != 0).any():
        shape = (len(ts_pred),) + (() if np.ndim(q) == 0 else (len(np.atleast_1d(q)),))
        return np.full(shape, np.nan), np.zeros(shape, dtype=bool), np.zeros(shape, dtype=np.int32), info
    return engines[0].mixture_quantile(mr, vr, weights, q, tol=tol, max_iter=max_iter) + (info,)


class GPEngineMulti:
    """One host process driving several GPUs (agp_init_multi): what a single Julia process would hold.
    `engines[i]` is the per-device GPEngine (rank i of the node communicator)."""

    def __init__(self, device_ids):
        self._lib = load_library()
        ids = np.ascontiguousarray(np.asarray(device_ids, dtype=np.int32))
        self._n = int(ids.shape[0])
        self._arr = (C.c_void_p * self._n)()
        rc = self._lib.agp_init_multi(self._arr, _ip(ids), self._n)
        if rc != 0:
            msg = self._lib.agp_last_error(None)
            raise AGPError(f"agp_init_multi failed ({rc}): {msg.decode() if msg else ''}")
        self.engines = [GPEngine(int(d), _ctx=C.c_void_p(self._arr[i])) for i, d in enumerate(ids)]
        self.n_max = 0

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.agp_last_error(C.c_void_p(self._arr[0]))
            raise AGPError(f"engine call failed ({rc}): {msg.decode() if msg else ''}")

    def set_data(self, ts, xs):
        ts, xs = _f64(ts), _f64(xs)
        self._check(self._lib.agp_set_data_multi(self._arr, self._n, _dp(ts), _dp(xs), ts.shape[0]))
        self.n_max = ts.shape[0]
        for e in self.engines:
            e.n_max = self.n_max

    def remove_data(self, indexes):
        """GPEngine.remove_data on every device (agp_remove_data_multi).  Returns the new n_max."""
        idx = check_remove_indexes(indexes, getattr(self, "n_max", 0))
        self._check(self._lib.agp_remove_data_multi(self._arr, self._n, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size))
        self.n_max -= int(idx.size)
        for e in self.engines:
            e.n_max = self.n_max
        return self.n_max

    def logpdf_batch(self, nodes, noises, n=None, check=True, programs=None, extend=False):
        """extend=True: every device runs its shard as an extension sweep (agp_logpdf_batch_extend_multi)."""
        n = self.n_max if n is None else int(n)
        op_off, ops, prm_off, prm = programs if programs is not None else _gp.encode_batch(nodes)
        P = op_off.shape[0] - 1
        noises = _f64(noises)
        out = np.empty(P); info = np.empty(P, dtype=np.int32)
        fn = self._lib.agp_logpdf_batch_extend_multi if extend else self._lib.agp_logpdf_batch_multi
        self._check(fn(self._arr, self._n, n, P, _ip(op_off), _u8(ops), _ip(prm_off), _dp(prm),
                       _dp(noises), _dp(out), _ip(info)))
        _raise_first_bad(info, check)
        return out, info

    def logpdf_grad_batch(self, nodes, noises, n=None, check=True, programs=None, want_owner=False):
        """agp_logpdf_grad_batch_multi over the node's devices (cost-aware split inside the entry)."""
        return logpdf_grad_batch_multi(self.engines, nodes, noises, n=n, check=check, programs=programs, want_owner=want_owner)

    def predict_batch(self, nodes, noises, ts_pred, **kw):
        """agp_predict_batch_multi over the node's devices."""
        return predict_batch_multi(self.engines, nodes, noises, ts_pred, **kw)

    def predict_quantile_batch(self, nodes, noises, ts_pred, weights, q, **kw):
        """GPEngine.predict_quantile_batch over the node's devices (predict_quantile_multi)."""
        return predict_quantile_multi(self, nodes, noises, ts_pred, weights, q, **kw)


# ------------------------------------------------------------------------------------------
# module-level functions with the reference's names; they use a lazily created default engine
# ------------------------------------------------------------------------------------------
_default_engine = None


def default_engine() -> GPEngine:
    global _default_engine
    if _default_engine is None:
        _default_engine = GPEngine(int(os.environ.get("AGP_DEVICE", "0")))
    return _default_engine


def compute_cov_matrix_vectorized(node, noise, ts, engine=None):
    """K = eval_cov(node, ts) + noise*I  (src/GP.jl:666-668), evaluated on the GPU."""
    return (engine or default_engine()).cov_matrix(node, noise, ts)


def eval_cov(node, ts, engine=None):
    """eval_cov(node, ts::Vector{Float64}) (src/GP.jl:55), evaluated on the GPU."""
    return (engine or default_engine()).cov_matrix(node, 0.0, ts)


def mvnormal_logpdf(node, noise, ts, xs, engine=None):
    """Score of `xs ~ mvnormal(zeros(n), compute_cov_matrix_vectorized(node, noise, ts))`
    (src/Model.jl:135-136).  Raises PosDefException like the reference."""
    eng = engine or default_engine()
    eng.set_data(ts, xs)
    return eng.logpdf(node, noise)


class MvNormal:
    """Posterior predictive of src/GP.jl:731-758 (mean / cov of Distributions.MvNormal)."""

    def __init__(self, node, noise, ts, xs, ts_pred, noise_pred=None, mean=None, engine=None):
        eng = engine or default_engine()
        ts = _f64(ts); xs = _f64(xs); ts_pred = _f64(ts_pred)
        eng.set_data(ts, xs)
        mt = mp_ = None
        if mean is not None:
            mt = np.array([mean(t) for t in ts], dtype=np.float64)
            mp_ = np.array([mean(t) for t in ts_pred], dtype=np.float64)
        mu, var, cov, _ = eng.predict_batch([node], [noise], ts_pred, noise_pred=noise_pred, mean_train=mt,
                                            mean_pred=mp_, want_cov=True)
        self.mu, self.var, self.Sigma = mu[0], var[0], cov[0]
        self._score = (eng, node, float(noise), ts, xs, ts_pred, noise_pred, mt, mp_)

    @classmethod
    def from_moments(cls, mu, Sigma):
        """An MvNormal(mu, Sigma) of given moments (predict_mvn_sum's components); it has no logpdf route."""
        d = cls.__new__(cls)
        d.mu = np.asarray(mu, dtype=np.float64); d.Sigma = np.asarray(Sigma, dtype=np.float64)
        d.var = np.diagonal(d.Sigma).copy()
        d._score = None
        return d

    def mean(self):
        return self.mu

    def cov(self):
        return self.Sigma

    def rand(self, n_samples=None, seed=0):
        """rand(d) / rand(d, n_samples) on the GPU (agp_predict_sample_batch with one particle of weight 1): one vector of length m for
        n_samples=None, else (m, n_samples), column s being sample s.  With empty ts / xs this is the prior MvNormal the tutorials
        sample synthetic data from.  The draws are not Julia's RNG stream; the distribution is the contract.  Raises
        PosDefException like the reference."""
        if self._score is None:
            raise NotImplementedError("rand of an MvNormal built from its moments")
        eng, node, noise, ts, xs, ts_pred, noise_pred, mt, mp_ = self._score
        eng.set_data(ts, xs)
        x, _, _ = eng.predict_sample_batch([node], [noise], ts_pred, [1.0], 1 if n_samples is None else n_samples, seed=seed,
                                           noise_pred=noise_pred, mean_train=mt, mean_pred=mp_)
        return x[:, 0].copy() if n_samples is None else x

    def logpdf(self, y):
        """Distributions.logpdf(d, y) (src/api.jl:693), on the GPU from the joint factorisation (agp_predict_logpdf_batch).
        Raises PosDefException like the reference."""
        if self._score is None:
            raise NotImplementedError("logpdf of an MvNormal built from its moments")
        eng, node, noise, ts, xs, ts_pred, noise_pred, mt, mp_ = self._score
        eng.set_data(ts, xs)
        lp, _ = eng.predict_logpdf_batch([node], [noise], ts_pred, y, noise_pred=noise_pred, mean_train=mt, mean_pred=mp_)
        return float(lp[0])


def predict_proba(engine, nodes, noises, log_weights, ts_pred, y, y_transform=(1.0, 0.0), noise_pred=None):
    """AutoGP.predict_proba(model, ds, y) (src/api.jl:686-699) on the engine's resident (scaled) series: per particle its
    normalised weight and the log-density of the RAW observations y at ts_pred (already in the engine's time scale) under the
    un-transformed predictive.  y_transform = (slope, intercept) of the series' linear transform (scaled = slope * raw +
    intercept); the predictive of the raw values is the scaled one mapped back, whose density gains m log|slope|.
    Returns a dict of arrays {"particle", "weight", "logp"} (the reference's DataFrame columns)."""
    slope, intercept = (float(v) for v in y_transform)
    y = _f64(y)
    lp, _ = engine.predict_logpdf_batch(nodes, noises, ts_pred, slope * y + intercept, noise_pred=noise_pred)
    lw = _f64(log_weights)
    w = np.exp(lw - lw.max()); w /= w.sum()
    return {"particle": np.arange(1, len(nodes) + 1), "weight": w, "logp": lp + y.shape[0] * np.log(abs(slope))}


def predict_quantile(engine, nodes, noises, log_weights, ts_pred, q, y_transform=(1.0, 0.0), noise_pred=None, tol=1e-5,
                     max_iter=10**6):
    """AutoGP.predict_quantile(model, ds, q; noise_pred, tol, max_iter) (src/api.jl:547-596) on the engine's resident (scaled)
    series: the quantile q of the weighted mixture of every particle's posterior predictive at ts_pred (already in the engine's
    time scale), in the RAW space of y_transform = (slope, intercept) (scaled = slope * raw + intercept).  Weights are the
    particle_weights route: exp of Gen.normalize_weights(log_weights).  `engine` is a GPEngine or a GPEngineMulti.
    Returns (x, success): x of shape (m,) and a bool for a scalar q; (m, nq) and an (nq,) bool array for a vector q.  Raises
    PosDefException when a particle has no predictive (as predict_batch)."""
    from .dist import normalize_weights
    w = np.exp(normalize_weights(log_weights)[1])
    npred = None if noise_pred is None else float(noise_pred)
    x, conv, _, _ = engine.predict_quantile_batch(nodes, noises, ts_pred, w, q, noise_pred=npred, y_transform=y_transform, tol=tol,
                                                  max_iter=max_iter)
    return x, (bool(conv.all()) if np.ndim(q) == 0 else conv.all(axis=0))


def predict_quantile_series(engine, series, queries, nodes, noises, series_index, log_weights, q, y_transforms=None, noise_pred=None,
                            tol=1e-5, max_iter=10**6, max_n=SERIES_MAX_N, all_long=False):
    """predict_quantile for callers that hold one model per short series: particle p belongs to the model of
    series[series_index[p]], whose mixture weighs it by the softmax of log_weights over THAT series' particles
    (pack_series_mixture); one call of GPEngine.predict_quantile_series_batch serves every series.  y_transforms: one (slope,
    intercept) per series.  Returns a list over the series of (x, success), each as predict_quantile returns them: x of shape (m_s,)
    and a bool for a scalar q; (m_s, nq) and an (nq,) bool array for a vector q.  Raises PosDefException when a particle has no
    predictive.  max_n=LONG_SERIES_MAX_N (or all_long=True: every non-empty series in the long kernel) takes
    GPEngine.predict_quantile_long_series_batch instead: series of up to LONG_SERIES_MAX_N points; any other max_n is a ValueError."""
    if max_n not in (SERIES_MAX_N, LONG_SERIES_MAX_N):
        raise ValueError(f"max_n must be SERIES_MAX_N ({SERIES_MAX_N}) or LONG_SERIES_MAX_N ({LONG_SERIES_MAX_N})")
    _, w = pack_series_mixture(series_index, len(series), log_weights=log_weights)
    if all_long or max_n == LONG_SERIES_MAX_N:
        band = engine.predict_quantile_long_series_batch(series, queries, nodes, noises, series_index, w, q, y_transforms=y_transforms,
                                                         noise_pred=noise_pred, tol=tol, max_iter=max_iter, all_long=all_long)
    else:
        band = engine.predict_quantile_series_batch(series, queries, nodes, noises, series_index, w, q, y_transforms=y_transforms,
                                                    noise_pred=noise_pred, tol=tol, max_iter=max_iter)
    return [(x, (bool(c.all()) if np.ndim(q) == 0 else c.all(axis=0))) for x, c in zip(band.x, band.converged)]


def predict_proba_series(engine, series, queries, heldout, nodes, noises, series_index, log_weights, y_transforms=None, noise_pred=None,
                         max_n=SERIES_MAX_N, all_long=False):
    """predict_proba for callers that hold one model per short series: particle p belongs to the model of series[series_index[p]],
    which weighs it by the softmax of log_weights over THAT series' particles (pack_series_mixture); heldout[s] are the RAW values
    observed at queries[s]; one call of GPEngine.predict_logpdf_series_batch serves every series.  Returns a list over the series of
    dicts with the reference's three columns {"particle", "weight", "logp"} — "particle" the 1-based positions inside the series'
    model, as predict_proba numbers them — plus "mixture_logp", the log-density of the held-out vector under the model's mixture.
    Raises PosDefException when a particle has no predictive.  max_n=LONG_SERIES_MAX_N (or all_long=True: every particle with held-out
    points in the long kernel) takes GPEngine.predict_logpdf_long_series_batch instead: training and held-out points of a series
    together up to LONG_SERIES_MAX_N; any other max_n is a ValueError."""
    if max_n not in (SERIES_MAX_N, LONG_SERIES_MAX_N):
        raise ValueError(f"max_n must be SERIES_MAX_N ({SERIES_MAX_N}) or LONG_SERIES_MAX_N ({LONG_SERIES_MAX_N})")
    lists, w = pack_series_mixture(series_index, len(series), log_weights=log_weights)
    if all_long or max_n == LONG_SERIES_MAX_N:
        sc = engine.predict_logpdf_long_series_batch(series, queries, heldout, nodes, noises, series_index, weights=w,
                                                     y_transforms=y_transforms, noise_pred=noise_pred, all_long=all_long)
    else:
        sc = engine.predict_logpdf_series_batch(series, queries, heldout, nodes, noises, series_index, weights=w,
                                                y_transforms=y_transforms, noise_pred=noise_pred)
    return [{"particle": np.arange(1, sel.size + 1), "weight": w[sel], "logp": sc.logpdf[sel], "mixture_logp": float(sc.series_logp[s])}
            for s, sel in enumerate(lists)]


def predict_rand(engine, nodes, noises, log_weights, ts_pred, n_samples=None, seed=0, y_transform=(1.0, 0.0), noise_pred=None):
    """rand(predict_mvn(model, ds; noise_pred), n_samples) (src/api.jl:497-522 + Distributions' rand) on the engine's resident (scaled)
    series: samples of the weighted mixture of every particle's posterior predictive at ts_pred (already in the engine's time scale),
    in the RAW space of y_transform = (slope, intercept) (scaled = slope * raw + intercept).  Weights are the particle_weights route:
    exp of Gen.normalize_weights(log_weights).  Returns one vector of length m for n_samples=None, else (m, n_samples).  The draws are
    a counter-based stream of `seed` (not Julia's RNG); the distribution is the contract.  Raises PosDefException when a particle has
    no predictive (the reference throws building its MvNormal)."""
    from .dist import normalize_weights
    w = np.exp(normalize_weights(log_weights)[1])
    npred = None if noise_pred is None else float(noise_pred)
    x, _, _ = engine.predict_sample_batch(nodes, noises, ts_pred, w, 1 if n_samples is None else n_samples, seed=seed,
                                          noise_pred=npred, y_transform=y_transform)
    return x[:, 0].copy() if n_samples is None else x


class MixtureModel:
    """The Distributions.MixtureModel that AutoGP.predict_mvn(model, ds; noise_pred) returns (src/api.jl:497-522), on the engine's
    resident (scaled) series: components = every particle's posterior predictive MvNormal at ts_pred mapped to the RAW space of
    y_transform, probs = the normalised particle weights.  mean / var / cov are reduced over the particles on the device
    (agp_predict_mixture_batch) when first asked for."""

    def __init__(self, engine, nodes, noises, log_weights, ts_pred, y_transform=(1.0, 0.0), noise_pred=None, space=0):
        from .dist import normalize_weights
        self._engine = engine
        self._nodes = list(nodes); self._noises = _f64(noises); self._log_weights = _f64(log_weights)
        self._ts_pred = _f64(ts_pred)
        self._y_transform = tuple(float(v) for v in y_transform)
        self._noise_pred = None if noise_pred is None else float(noise_pred)
        self._space = int(space)
        self._components = None
        self.probs = np.exp(normalize_weights(self._log_weights)[1])
        self._marginal = None       # (mean, var)
        self._full = None           # (mean, var, cov)

    @classmethod
    def from_components(cls, components, probs, engine=None, space=0):
        """MixtureModel(components, probs) of given MvNormal moments (predict_mvn_sum's return value): its moments come from
        agp_mixture_moments."""
        d = cls.__new__(cls)
        d._engine = engine or default_engine()
        d._components = list(components)
        d.probs = _f64(probs)
        d._space = int(space)
        d._nodes = None
        d._marginal = d._full = None
        return d

    def _moments(self, want_cov):
        if self._full is None and (want_cov or self._marginal is None):
            if self._components is not None:
                mu = np.stack([np.asarray(cm.mu, dtype=np.float64) for cm in self._components])
                S = np.stack([np.asarray(cm.Sigma, dtype=np.float64) for cm in self._components])
                mean, var, cov = self._engine.mixture_moments(mu, self.probs, covs=S, space=self._space, want_cov=want_cov)
            else:
                mean, var, cov, _ = self._engine.predict_mixture_batch(self._nodes, self._noises, self._ts_pred, self.probs,
                                                                       noise_pred=self._noise_pred, y_transform=self._y_transform,
                                                                       space=self._space, want_cov=want_cov)
            if want_cov:
                self._full = (mean, var, cov)
            else:
                self._marginal = (mean, var)
        return self._full if self._full is not None else self._marginal

    def mean(self):
        return self._moments(False)[0]

    def var(self):
        return self._moments(False)[1]

    def cov(self):
        return self._moments(True)[2]

    def lognormal(self):
        """MixtureModel(MvLogNormal.(components), probs): the direct-space view of a model fitted on log(y)
        (docs/src/tutorials/iclaims.md); its mean / var / cov are the log-normal mixture's (space = 1)."""
        if self._components is not None:
            return MixtureModel.from_components(self._components, self.probs, engine=self._engine, space=1)
        return MixtureModel(self._engine, self._nodes, self._noises, self._log_weights, self._ts_pred, self._y_transform,
                            self._noise_pred, space=1)

    def _resident(self, what):
        if self._nodes is None or self._space != 0:
            raise NotImplementedError(f"{what} of a MixtureModel built from moments or of its log-normal view")

    def logpdf(self, y):
        """Distributions.logpdf(d, y): logsumexp over the particles of log w_p + logpdf(component_p, y) (predict_proba's columns)."""
        self._resident("logpdf")
        r = predict_proba(self._engine, self._nodes, self._noises, self._log_weights, self._ts_pred, y, y_transform=self._y_transform,
                          noise_pred=self._noise_pred)
        keep = r["weight"] > 0.0
        t = np.log(r["weight"][keep]) + r["logp"][keep]
        hi = t.max()
        return float(hi + np.log(np.exp(t - hi).sum())) if np.isfinite(hi) else float(hi)

    def quantile(self, q, tol=1e-5, max_iter=10**6):
        """predict_quantile's (x, success)."""
        self._resident("quantile")
        return predict_quantile(self._engine, self._nodes, self._noises, self._log_weights, self._ts_pred, q,
                                y_transform=self._y_transform, noise_pred=self._noise_pred, tol=tol, max_iter=max_iter)

    def rand(self, n_samples=None, seed=0):
        """predict_rand's samples."""
        self._resident("rand")
        return predict_rand(self._engine, self._nodes, self._noises, self._log_weights, self._ts_pred, n_samples=n_samples, seed=seed,
                            y_transform=self._y_transform, noise_pred=self._noise_pred)


def predict_mvn(engine, nodes, noises, log_weights, ts_pred, y_transform=(1.0, 0.0), noise_pred=None):
    """AutoGP.predict_mvn(model, ds; noise_pred) (src/api.jl:497-522) on the engine's resident (scaled) series: the MixtureModel of
    every particle's posterior predictive at ts_pred (already in the engine's time scale) in the RAW space of y_transform = (slope,
    intercept) (scaled = slope * raw + intercept), weighted by exp of Gen.normalize_weights(log_weights)."""
    return MixtureModel(engine, nodes, noises, log_weights, ts_pred, y_transform=y_transform, noise_pred=noise_pred)


def predict_rand_series(engine, series, queries, nodes, noises, series_index, log_weights, n_samples, seeds, y_transforms=None,
                        noise_pred=None):
    """predict_rand for callers that hold one model per short series: particle p belongs to the model of series[series_index[p]],
    whose mixture weighs it by the softmax of log_weights over THAT series' particles (pack_series_mixture); series s draws its
    n_samples paths under seeds[s], as predict_rand does under that seed on the resident series; one call of
    GPEngine.predict_sample_series_batch serves every series.  Returns one (m_s, n_samples) array per series, raw space.  Raises
    PosDefException when a particle has no predictive."""
    _, w = pack_series_mixture(series_index, len(series), log_weights=log_weights)
    return engine.predict_sample_series_batch(series, queries, nodes, noises, series_index, w, n_samples, seeds=seeds,
                                              y_transforms=y_transforms, noise_pred=noise_pred).x


class SeriesMixtureModel(MixtureModel):
    """predict_mvn_series' return value for one series: a MixtureModel of given components (mean / var / cov through
    agp_mixture_moments) that also knows the short series it came from, so that logpdf, quantile and rand go through the
    many-series entries instead of the resident series.  Built by from_series; an object made by from_components alone has no
    series behind it, and its logpdf / quantile / rand raise NotImplementedError as the base class's do for a model built from moments."""

    _series_model = None

    @classmethod
    def from_series(cls, engine, components, probs, ts, xs, queries, nodes, noises, log_weights, y_transform=None, noise_pred=None):
        """components / probs as from_components; the rest is the one-series model the other routes are asked with: its (ts, xs),
        query times, particles, their log-weights, the series' (slope, intercept) or None, noise_pred (None, scalar or per particle)"""
        d = cls.from_components(components, probs, engine=engine)
        d._series_model = (ts, xs, queries, list(nodes), noises, log_weights, y_transform, noise_pred)
        return d

    def _one(self):
        if self._series_model is None:
            raise NotImplementedError("logpdf / quantile / rand of a SeriesMixtureModel built from moments alone")
        ts, xs, q, nodes, noises, lw, yt, npred = self._series_model
        return ([(ts, xs)], [q], nodes, noises, np.zeros(len(nodes), dtype=np.int32), lw, None if yt is None else [yt], npred)

    def logpdf(self, y):
        series, queries, nodes, noises, sidx, lw, yts, npred = self._one()
        return predict_proba_series(self._engine, series, queries, [y], nodes, noises, sidx, lw, y_transforms=yts,
                                    noise_pred=npred)[0]["mixture_logp"]

    def quantile(self, q, tol=1e-5, max_iter=10**6):
        series, queries, nodes, noises, sidx, lw, yts, npred = self._one()
        return predict_quantile_series(self._engine, series, queries, nodes, noises, sidx, lw, q, y_transforms=yts, noise_pred=npred,
                                       tol=tol, max_iter=max_iter)[0]

    def rand(self, n_samples=None, seed=0):
        series, queries, nodes, noises, sidx, lw, yts, npred = self._one()
        x = predict_rand_series(self._engine, series, queries, nodes, noises, sidx, lw, 1 if n_samples is None else n_samples, [seed],
                                y_transforms=yts, noise_pred=npred)[0]
        return x[:, 0].copy() if n_samples is None else x


def predict_mvn_series(engine, series, queries, nodes, noises, series_index, log_weights, y_transforms=None, noise_pred=None):
    """predict_mvn for callers that hold one model per short series: one MixtureModel per series (None for a series without
    particles), its components the posterior predictive MvNormals of the series' particles in raw space — mean and m_s x m_s
    covariance from ONE call of GPEngine.predict_sample_series_batch (no samples drawn) — and its probs the softmax of log_weights
    over the series' particles.  mean / var / cov / logpdf / quantile / rand work as on predict_mvn's result.  Raises
    PosDefException when a particle has no predictive."""
    S = len(series)
    lists, w = pack_series_mixture(series_index, S, log_weights=log_weights)
    r = engine.predict_sample_series_batch(series, queries, nodes, noises, series_index, w, 0, y_transforms=y_transforms,
                                           noise_pred=noise_pred, want_moments=True)
    lw = _f64(log_weights); noises = _f64(noises)
    out = []
    for s, sel in enumerate(lists):
        if sel.size == 0:
            out.append(None)
            continue
        npred = None if noise_pred is None else (float(noise_pred) if np.ndim(noise_pred) == 0 else _f64(noise_pred)[sel])
        out.append(SeriesMixtureModel.from_series(engine, [MvNormal.from_moments(r.mean[p], r.cov[p]) for p in sel], w[sel],
                                                  series[s][0], series[s][1], queries[s], [nodes[p] for p in sel], noises[sel], lw[sel],
                                                  None if y_transforms is None else tuple(y_transforms[s]), npred))
    return out


def infer_gp_sum(nodes, noise, ts, xs, ts_pred, noise_pred=None, engine=None):
    """GP.infer_gp_sum(nodes, noise, ts, xs, ts_pred; noise_pred) (src/GP.jl:904-993) on the GPU.
    Returns (mean, cov, indexes) with indexes = {"F": [slice...], "X": slice} like the reference's tuple."""
    eng = engine or default_engine()
    eng.set_data(ts, xs)
    mean, cov, iF, iX = eng.infer_gp_sum(nodes, noise, ts_pred, noise_pred=noise_pred)
    return mean, cov, {"F": iF, "X": iX}


def predict_mvn_sum(engine, nodes, noises, log_weights, ts_pred, LeafType, y_transform=(1.0, 0.0), noise_pred=None):
    """AutoGP.predict_mvn_sum(model, ds, T; noise_pred) (src/api.jl:978-1034) on the engine's resident (scaled) series: each particle's
    kernel split by split_kernel_sop(node, LeafType), infer_gp_sum of the two parts (one batched call), mapped to the RAW space of
    y_transform = (slope, intercept) with the intercept counted once (on F_1).  Returns (components, weights, indexes): one
    MvNormal per particle, the normalised particle weights, and {"Y": slice, "F": [slice, slice]}."""
    from .dist import normalize_weights
    slope, intercept = (float(v) for v in y_transform)
    split = [_gp.split_kernel_sop(nd, LeafType) for nd in nodes]
    npred = None if noise_pred is None else float(noise_pred)
    mean, _, cov, _, iF, iX = engine.infer_gp_sum_batch(split, noises, ts_pred, noise_pred=npred, want_cov=True)
    comps = []
    for mu, S in zip(mean, cov):
        mr = (mu - intercept) / slope
        mr[iF[0]] += intercept / slope
        comps.append(MvNormal.from_moments(mr, (1.0 / (slope * slope)) * S))
    w = np.exp(normalize_weights(log_weights)[1])
    return comps, w, {"Y": iX, "F": iF}


def predict_sum(engine, nodes, noises, log_weights, ts_pred, LeafType, y_transform=(1.0, 0.0), noise_pred=None, quantiles=(),
                ds=None):
    """AutoGP.predict_sum(model, ds, T; quantiles, noise_pred) (src/api.jl:898-936): the columns ds, y_mean, component, particle,
    weight, y_<q> of the reference's DataFrame (a dict of arrays), in its row order — per particle, component 0 (the observable),
    then 1 (the addends with a LeafType factor), then 2 (the others).  Means and quantiles come from the device read-out
    (GPEngine.predict_sum_batch).  `ds` labels the rows (default: ts_pred)."""
    from .dist import normalize_weights
    split = [_gp.split_kernel_sop(nd, LeafType) for nd in nodes]
    npred = None if noise_pred is None else float(noise_pred)
    qs = [float(v) for v in quantiles]
    ts_pred = _f64(ts_pred); p = ts_pred.shape[0]
    mean, x, _ = engine.predict_sum_batch(split, noises, ts_pred, q=qs, noise_pred=npred, y_transform=y_transform)
    P = len(nodes)
    w = np.exp(normalize_weights(log_weights)[1])
    blocks = [slice(2 * p, 3 * p), slice(0, p), slice(p, 2 * p)]         # Y, F_1, F_2
    rows = [(k, c, blk) for k in range(P) for c, blk in enumerate(blocks)]
    labels = ts_pred if ds is None else np.asarray(ds)
    out = {
        "ds": np.concatenate([labels for _ in rows]) if rows else labels[:0],
        "y_mean": np.concatenate([mean[k, blk] for k, _, blk in rows]) if rows else np.zeros(0),
        "component": np.repeat([c for _, c, _ in rows], p).astype(np.int64),
        "particle": np.repeat([k + 1 for k, _, _ in rows], p).astype(np.int64),
        "weight": np.repeat([w[k] for k, _, _ in rows], p),
    }
    for j, qv in enumerate(qs):
        out[f"y_{qv!r}"] = np.concatenate([x[k, blk, j] for k, _, blk in rows]) if rows else np.zeros(0)
    return out


def predict_sum_series(engine, series, queries, nodes, noises, series_index, log_weights, LeafType, y_transforms=None, noise_pred=None,
                       quantiles=()):
    """predict_sum for callers that hold one model per short series: particle p belongs to the model of series[series_index[p]],
    whose mixture weighs it by the softmax of log_weights over THAT series' particles (pack_series_mixture); every particle's
    kernel is split by split_kernel_sop(node, LeafType) and ONE call of GPEngine.predict_sum_series_batch decomposes them all.
    Returns one dict of columns per series — ds, y_mean, component, particle, weight, y_<q> — in predict_sum's row order: per
    particle of the series (numbered from 1 within it), component 0 (the observable), then 1 (the addends with a LeafType factor),
    then 2 (the others); a series without particles gives empty columns.  Raises PosDefException when a particle has no result."""
    S = len(series)
    lists, w = pack_series_mixture(series_index, S, log_weights=log_weights)
    split = [_gp.split_kernel_sop(nd, LeafType) for nd in nodes]
    qs = [float(v) for v in quantiles]
    r = engine.predict_sum_series_batch(series, queries, split, noises, series_index, q=qs, y_transforms=y_transforms,
                                        noise_pred=noise_pred)
    out = []
    for s, sel in enumerate(lists):
        tq = _f64(queries[s]); m = tq.shape[0]
        blocks = [slice(2 * m, 3 * m), slice(0, m), slice(m, 2 * m)]         # Y, F_1, F_2
        rows = [(k, int(p), c, blk) for k, p in enumerate(sel) for c, blk in enumerate(blocks)]
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
        d = {
            "ds": cat([tq for _ in rows]),
            "y_mean": cat([r.mean[p][blk] for _, p, _, blk in rows]),
            "component": np.repeat([c for _, _, c, _ in rows], m).astype(np.int64),
            "particle": np.repeat([k + 1 for k, _, _, _ in rows], m).astype(np.int64),
            "weight": np.repeat([w[p] for _, p, _, _ in rows], m),
        }
        for j, qv in enumerate(qs):
            d[f"y_{qv!r}"] = cat([r.x[p][blk, j] for _, p, _, blk in rows])
        out.append(d)
    return out


def with_params(node, params):
    """A copy of a kernel tree with the numeric parameters replaced by `params`, in the order of gp.encode(node)[1]."""
    it = iter(float(v) for v in params)

    def rec(nd):
        if isinstance(nd, _gp.LeafNode):
            return type(nd)(*[next(it) for _ in nd.params()])
        left, right = rec(nd.left), rec(nd.right)
        if isinstance(nd, _gp.ChangePoint):
            return _gp.ChangePoint(left, right, next(it), next(it))
        return type(nd)(left, right)
    out = rec(node)
    if next(it, None) is not None:
        raise ValueError("more parameters than the tree has")
    return out


def mcmc_parameters_series(engine, series, nodes, noises, series_index, n_hmc, seeds, hmc_config=None, prior=None, infer_noise=True,
                           want_trace=False, check=True):
    """mcmc_parameters! / rejuvenate_particle_parameters (src/inference_smc_anneal_data.jl:33-76) for callers that hold one model
    per short series: every particle's kernel parameters and noise are untransformed to the latent z of the reference's prior
    (prior: GPConfig.prior's entries "gamma", "period", "wildcard"; ChangePoint scales stay fixed), ONE call of
    GPEngine.hmc_series_batch runs n_hmc HMC iterations on all of them, and the new trees and noises come back — ready for
    predict_*_series.  hmc_config: the reference's keys L_param, eps_param, L_noise, eps_noise, n_exit; infer_noise=False skips the
    noise moves.  Returns (nodes, noises, counts[P, 4], result) with `result` the engine call's namespace (logpdf, z, trace ...)."""
    from . import prior as _prior
    cfg = dict(hmc_config or {})
    tf = _prior.hmc_transform_table(prior)
    cls = [_prior.hmc_classes(nd) for nd in nodes]
    z = [np.array([_prior.hmc_untransform(v, c, tf) for v, c in zip(_gp.encode(nd)[1], k)]) for nd, k in zip(nodes, cls)]
    zn = np.array([_prior.hmc_untransform(float(v) - _prior.JITTER, _prior.HMC_CLASS_WILDCARD, tf) for v in noises])
    r = engine.hmc_series_batch(series, nodes, z, zn, cls, tf, series_index, n_hmc, seeds, noise_class=_prior.HMC_CLASS_WILDCARD,
                                noise_jitter=_prior.JITTER, L_param=cfg.get("L_param", 10), eps_param=cfg.get("eps_param", 0.02),
                                L_noise=cfg.get("L_noise", 10) if infer_noise else 0, eps_noise=cfg.get("eps_noise", 0.02),
                                n_exit=cfg.get("n_exit", None), want_trace=want_trace, check=check)
    return [with_params(nd, q) for nd, q in zip(nodes, r.prm)], r.noise.copy(), r.counts, r


def quantile(dist: MvNormal, p):
    """Marginal quantiles mu + sqrt(diag(cov)) * Phi^-1(p): m x len(p)  (src/GP.jl:1006-1012)."""
    from statistics import NormalDist
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    z = np.array([NormalDist().inv_cdf(float(v)) for v in p])
    return dist.mu[:, None] + np.sqrt(dist.var)[:, None] * z[None, :]
