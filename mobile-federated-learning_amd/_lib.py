"""ctypes binding of the native libraries ``build.BUILT_LIBS`` describes (the C ABI
in include/*.h): a signature table each, one loader and one status check.

There is no fallback: if a HIP library is missing or does not export the
declared entry points, every product call raises ``FedAvgLibraryError``.
"""
from __future__ import annotations

import ctypes
import functools
import threading
from pathlib import Path

from .build import (BY_KEY, CLIENTADAM_LIB_PATH, CLIENTLOOP_LIB_PATH, CLIENTSTEP_LIB_PATH, CLIENTVEC_LIB_PATH, DESCRIBED,
                    EXTRA_BY_KEY, FUSEDVEC_LIB_PATH, LIB_PATH, PROBE_LIB_PATH, SEGVEC_LIB_PATH, NativeLib)

_c_i64 = ctypes.c_int64
_c_int = ctypes.c_int
_vp = ctypes.c_void_p
_c_float = ctypes.c_float

# name -> (restype, argtypes); mirrors include/fedavg_amd.h
SIGNATURES = {
    "fedavg_abi_version": (_c_int, []),
    "fedavg_last_error": (ctypes.c_char_p, []),
    "fedavg_reduce_f32": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp]),
    "fedavg_reduce_f32_timed": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp]),
    "fedavg_reduce_ptrs_f32": (_c_int, [_vp, _c_i64, _c_i64, _vp, _vp, _vp]),
    "fedavg_reduce_f64": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp]),
    "fedavg_reduce_f16": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp]),
    "fedavg_reduce_bf16": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp]),
    "fedavg_reduce_splitk_f32": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_int, _vp]),
    "fedavg_weights_f32": (_c_int, [_vp, _c_i64, _vp]),
    "fedavg_pack_rows": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_int]),
    "fedavg_pack_rows_device_workspace": (_c_i64, [_c_i64]),
    "fedavg_segments_workspace": (_c_i64, [_c_i64, _c_i64]),
    "fedavg_segments_partials": (_c_i64, [_vp, _c_i64, _c_i64]),
    "fedavg_reduce_segments_f32": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _vp]),
    "fedavg_client_sqdist_segments_f32": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _vp,
                                                   _vp, _c_i64, _vp]),
    "fedavg_reduce_sqdist_segments_partials": (_c_i64, [_c_i64]),
    "fedavg_reduce_sqdist_segments_f32": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp,
                                                   _vp, _vp, _c_i64, _vp]),
    "fedavg_pack_rows_device": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _vp]),
    "fedavg_device_round_workspace": (_c_i64, [_c_i64, _c_i64]),
    "fedavg_device_round_scratch": (_c_i64, [_vp, _vp, _c_i64, _c_i64]),
    "fedavg_device_round_f32": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp,
                                         _vp, _c_i64, _vp, _vp, _c_i64, _vp]),
    "fedavg_round_f32": (_c_int, [_vp, _c_i64, _vp, _vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_int,
                                  _vp]),
    "fedavg_client_sqdist_workspace": (_c_i64, [_c_i64, _c_i64]),
    "fedavg_client_sqdist_f32": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _vp]),
    "fedavg_client_sqdist_workspace_elems": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "fedavg_reduce_sqdist_workspace": (_c_i64, [_c_i64, _c_i64]),
    "fedavg_fused_plan_of": (_c_i64, [_c_i64, _c_i64]),
    "fedavg_reduce_sqdist_f32": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp]),
    "fedavg_client_sqdist_f64": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _vp]),
    "fedavg_client_sqdist_f16": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _vp]),
    "fedavg_client_sqdist_bf16": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _vp]),
    "fedavg_fpf_set_rows_f32": (_c_int, [_vp, _c_i64, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp]),
    "fedavg_fpf_workspace": (_c_i64, [_c_i64]),
    "fedavg_fpf_end_round_f32": (_c_int, [_vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _c_float, _vp, _c_i64,
                                          _vp]),
    "fedavg_fpf_update_g": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_float, _c_int, _c_float, _vp]),
    "fedavg_fpf_index_f32": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp]),
    "fedavg_fpf_index_lru": (_c_int, [_vp, _vp, _c_i64, _vp, _vp]),
    "fedavg_fpf_cat_diff": (_c_int, [_vp, _c_i64, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _vp, _c_i64, _c_int, _vp]),
    "fedavg_fpf_end_round_promoted": (_c_int, [_vp, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _c_int, _c_float, _vp,
                                               _c_i64, _vp]),
    "fedavg_fpf_index_f64": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp]),
    "fedavg_copy_to_host": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp]),
    "fedavg_upload_shard": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_i64, _c_i64, _vp]),
    "fedavg_f32_schedule": (_c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _vp]),
    "fedavg_f32_schedule_ld": (_c_int, [_c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp]),
    "fedavg_client_stats_workspace": (_c_i64, [_c_i64]),
    "fedavg_client_stats_partials": (_c_i64, [_vp, _c_i64]),
    "fedavg_client_stats_f32": (_c_int, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _vp, _vp,
                                         _c_i64, _vp]),
    "fedavg_client_track": (_c_int, [_vp, _vp, _vp, ctypes.c_double, _vp]),
}

# exported only by libfedavg_amd_probe.so (include/fedavg_amd_tuning.h)
TUNING_SIGNATURES = {
    "fedavg_reduce_f32_buf": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _vp]),
    "fedavg_reduce_segments_f32_variant": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _c_i64,
                                                    _c_int, _c_int, _c_int, _vp]),
    "fedavg_client_sqdist_segments_f32_variant": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp,
                                                           _vp, _vp, _c_i64, _c_int, _c_int, _vp]),
    "fedavg_device_round_phases": (_c_int, [_vp, _c_int]),
    "fedavg_fpf_index_workspace": (_c_i64, [_c_i64, _c_i64]),
    "fedavg_fpf_index_variant": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _c_int, _c_int,
                                          _c_int, _vp]),
    "fedavg_probe_cvt16": (_c_int, [_vp, _c_i64, _c_int, _vp, _vp]),
    "fedavg_reduce_f32_tuned": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_int, _c_int, _vp]),
    "fedavg_reduce_f32_variant": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_int, _c_int, _c_int, _c_int,
                                           _c_int, _vp]),
    "fedavg_reduce_half_variant": (_c_int, [_c_int, _vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_int, _c_int, _c_int,
                                            _vp]),
    "fedavg_half_schedule": (_c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _vp]),
    "fedavg_client_sqdist_variant": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _c_int,
                                              _c_int, _vp]),
    "fedavg_client_sqdist_buf": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _c_int,
                                          _c_int, _vp]),
    "fedavg_reduce_sqdist_f32_variant": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _c_int,
                                                  _c_int, _vp]),
    "fedavg_reduce_vec_buf": (_c_int, [_c_int, _vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_int, _c_int, _c_int, _vp]),
    "fedavg_probe_busy_copy": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _vp]),
    "fedavg_probe_clock": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp]),
    "fedavg_stream_create_masked": (_c_int, [_c_int, _c_int, _vp]),
    "fedavg_stream_destroy": (_c_int, [_vp]),
    "fedavg_reduce_f32_xcd": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_int, _vp]),
    "fedavg_probe_read_f32x4": (_c_int, [_vp, _c_i64, _c_int, _c_int, _c_int, _vp, _vp]),
    "fedavg_reduce_tiled_f32": (_c_int, [_vp, _c_i64, _c_i64, _vp, _vp, _c_int, _vp]),
}

# libfedavg_amd_fusedvec.so (include/fedavg_amd_fusedvec.h)
FUSEDVEC_SIGNATURES = {
    "fedavg_fusedvec_abi_version": (_c_int, []),
    "fedavg_fusedvec_last_error": (ctypes.c_char_p, []),
    "fedavg_reduce_sqdist_vec_workspace": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "fedavg_fused_vec_plan_of": (_c_i64, [_c_i64, _c_i64, _c_i64, _c_int]),
    "fedavg_reduce_sqdist_f64": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp]),
    "fedavg_reduce_sqdist_f16": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp]),
    "fedavg_reduce_sqdist_bf16": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp]),
}

# libfedavg_amd_segvec.so (include/fedavg_amd_segvec.h)
_SEGVEC_ROUND = (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp])
SEGVEC_SIGNATURES = {
    "fedavg_segvec_abi_version": (_c_int, []),
    "fedavg_segvec_last_error": (ctypes.c_char_p, []),
    "fedavg_device_round_vec_workspace": (_c_i64, [_c_i64, _c_i64]),
    "fedavg_device_round_vec_partials": (_c_i64, [_c_i64, _c_i64]),
    "fedavg_device_round_vec_plan_of": (_c_i64, [_c_i64, _c_i64, _c_int]),
    "fedavg_device_round_f64": _SEGVEC_ROUND,
    "fedavg_device_round_f16": _SEGVEC_ROUND,
    "fedavg_device_round_bf16": _SEGVEC_ROUND,
}

# libfedavg_amd_clientvec.so (include/fedavg_amd_clientvec.h)
_CLIENTVEC_STATS = (_c_int, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp])
_CLIENTVEC_TRACK = (_c_int, [_vp, _vp, _vp, ctypes.c_double, _vp])
CLIENTVEC_SIGNATURES = {
    "fedavg_clientvec_abi_version": (_c_int, []),
    "fedavg_clientvec_last_error": (ctypes.c_char_p, []),
    "fedavg_client_stats_vec_span": (_c_i64, [_c_i64]),
    "fedavg_client_stats_vec_workspace": (_c_i64, [_c_i64]),
    "fedavg_client_stats_vec_partials": (_c_i64, [_vp, _c_i64, _c_i64]),
    "fedavg_client_stats_bf16": _CLIENTVEC_STATS,
    "fedavg_client_stats_f16": _CLIENTVEC_STATS,
    "fedavg_client_stats_f64": _CLIENTVEC_STATS,
    "fedavg_client_track_bf16": _CLIENTVEC_TRACK,
    "fedavg_client_track_f16": _CLIENTVEC_TRACK,
    "fedavg_client_track_f64": _CLIENTVEC_TRACK,
}

# libfedavg_amd_clientstep.so (include/fedavg_amd_clientstep.h)
_CLIENTSTEP_STEP = (_c_int, [_vp, _vp, _vp, _c_i64, ctypes.c_double, _c_int, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp])
CLIENTSTEP_SIGNATURES = {
    "fedavg_clientstep_abi_version": (_c_int, []),
    "fedavg_clientstep_last_error": (ctypes.c_char_p, []),
    "fedavg_client_step_span": (_c_i64, [_c_i64]),
    "fedavg_client_step_workspace": (_c_i64, [_c_i64]),
    "fedavg_client_step_partials": (_c_i64, [_vp, _c_i64, _c_i64]),
    "fedavg_client_sgd_step_f32": _CLIENTSTEP_STEP,
    "fedavg_client_sgd_step_bf16": _CLIENTSTEP_STEP,
    "fedavg_client_sgd_step_f16": _CLIENTSTEP_STEP,
    "fedavg_client_sgd_step_f64": _CLIENTSTEP_STEP,
}

# libfedavg_amd_clientadam.so (include/fedavg_amd_clientadam.h)
_CLIENTADAM_STEP = (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _c_int, _c_int, _vp, _c_i64, _vp, _vp, _vp,
                             _c_i64, _vp])
CLIENTADAM_SIGNATURES = {
    "fedavg_clientadam_abi_version": (_c_int, []),
    "fedavg_clientadam_last_error": (ctypes.c_char_p, []),
    "fedavg_client_adam_span": (_c_i64, [_c_i64]),
    "fedavg_client_adam_workspace": (_c_i64, [_c_i64]),
    "fedavg_client_adam_partials": (_c_i64, [_vp, _c_i64, _c_i64]),
    "fedavg_client_adam_step_f32": _CLIENTADAM_STEP,
    "fedavg_client_adam_step_bf16": _CLIENTADAM_STEP,
    "fedavg_client_adam_step_f16": _CLIENTADAM_STEP,
    "fedavg_client_adam_step_f64": _CLIENTADAM_STEP,
}

# libfedavg_amd_clientloop.so (include/fedavg_amd_clientloop.h): the steps' arguments, then g_stats, gate, state, loss
_CLIENTLOOP_GUARD = (_c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, _c_i64, _vp])
_CLIENTLOOP_SGD = (_c_int, _CLIENTSTEP_STEP[1] + [_vp, _vp, _vp, _vp])
_CLIENTLOOP_ADAM = (_c_int, _CLIENTADAM_STEP[1] + [_vp, _vp, _vp, _vp])
CLIENTLOOP_SIGNATURES = {
    "fedavg_clientloop_abi_version": (_c_int, []),
    "fedavg_clientloop_last_error": (ctypes.c_char_p, []),
    "fedavg_client_loop_span": (_c_i64, [_c_i64]),
    "fedavg_client_loop_workspace": (_c_i64, [_c_i64, _c_int]),
    "fedavg_client_loop_partials": (_c_i64, [_vp, _c_i64, _c_i64]),
    "fedavg_client_guard_f32": _CLIENTLOOP_GUARD,
    "fedavg_client_guard_bf16": _CLIENTLOOP_GUARD,
    "fedavg_client_guard_f64": _CLIENTLOOP_GUARD,
    "fedavg_client_sgd_step_gated_f32": _CLIENTLOOP_SGD,
    "fedavg_client_sgd_step_gated_bf16": _CLIENTLOOP_SGD,
    "fedavg_client_sgd_step_gated_f64": _CLIENTLOOP_SGD,
    "fedavg_client_adam_step_gated_f32": _CLIENTLOOP_ADAM,
    "fedavg_client_adam_step_gated_bf16": _CLIENTLOOP_ADAM,
    "fedavg_client_adam_step_gated_f64": _CLIENTLOOP_ADAM,
}

ABI_VERSION = BY_KEY["product"].abi[1]
FUSEDVEC_ABI_VERSION = BY_KEY["fusedvec"].abi[1]
SEGVEC_ABI_VERSION = BY_KEY["segvec"].abi[1]
CLIENTVEC_ABI_VERSION = BY_KEY["clientvec"].abi[1]
CLIENTSTEP_ABI_VERSION = BY_KEY["clientstep"].abi[1]
CLIENTADAM_ABI_VERSION = DESCRIBED["clientadam"].abi[1]
CLIENTLOOP_ABI_VERSION = EXTRA_BY_KEY["clientloop"].abi[1]

FEDAVG_EINVAL = -10001
FEDAVG_EALIGN = -10002
FEDAVG_EMODE = -10003


class FpfGroups(ctypes.Structure):
    """fedavg_fpf_groups (include/fedavg_amd.h): row 0 of each dtype group,
    its row stride in elements, its kind (0 fp32, 1 fp64, 2 fp16, 3 bf16)."""

    _fields_ = [("base", ctypes.c_void_p * 4), ("ld", ctypes.c_int64 * 4), ("kind", ctypes.c_int32 * 4)]


class FedAvgLibraryError(RuntimeError):
    """A native library is missing, stale, or a call into it failed."""


# description key -> (its signature tables, the module-level name of its path, the module-level name of its cache
# slot).  _load reads both names when it runs, so a test that patches them is served.
_BINDING = {
    "product": ((SIGNATURES,), "LIB_PATH", "_lib"),
    "probe": ((SIGNATURES, TUNING_SIGNATURES), "PROBE_LIB_PATH", "_probe"),
    "fusedvec": ((FUSEDVEC_SIGNATURES,), "FUSEDVEC_LIB_PATH", "_fusedvec"),
    "segvec": ((SEGVEC_SIGNATURES,), "SEGVEC_LIB_PATH", "_segvec"),
    "clientvec": ((CLIENTVEC_SIGNATURES,), "CLIENTVEC_LIB_PATH", "_clientvec"),
    "clientstep": ((CLIENTSTEP_SIGNATURES,), "CLIENTSTEP_LIB_PATH", "_clientstep"),
    "clientadam": ((CLIENTADAM_SIGNATURES,), "CLIENTADAM_LIB_PATH", "_clientadam"),
}
# the same for the libraries of build.EXTRA_BY_KEY (a new one goes here)
_EXTRA_BINDING = {
    "clientloop": ((CLIENTLOOP_SIGNATURES,), "CLIENTLOOP_LIB_PATH", "_clientloop"),
}

_lock = threading.Lock()
_lib = None
_probe = None
_fusedvec = None
_segvec = None
_clientvec = None
_clientstep = None
_clientadam = None
_clientloop = None


def library_path() -> Path:
    return LIB_PATH


def _load(d: NativeLib) -> ctypes.CDLL:
    """Load (once), type and version-check the library ``d`` describes.  No
    fallback: a missing, unloadable or stale library raises ``FedAvgLibraryError``."""
    tables, path_name, slot = _BINDING[d.key] if d.key in _BINDING else _EXTRA_BINDING[d.key]
    g = globals()
    if g[slot] is not None:
        return g[slot]
    if d.needs:
        _load(DESCRIBED[d.needs] if d.needs in DESCRIBED else EXTRA_BY_KEY[d.needs])
    with _lock:
        if g[slot] is not None:
            return g[slot]
        path = g[path_name]
        if not path.exists():
            raise FedAvgLibraryError(f"{path} not built: run __graft_entry__.build(){d.no_fallback}")
        try:
            lib = ctypes.CDLL(str(path))
        except OSError as e:
            raise FedAvgLibraryError(f"{path} does not load: {e}") from e
        for table in tables:
            for name, (res, args) in table.items():
                try:
                    fn = getattr(lib, name)
                except AttributeError as e:
                    raise FedAvgLibraryError(f"{path} does not export {name}") from e
                fn.restype = res
                fn.argtypes = args
        symbol, expected = d.abi
        ver = getattr(lib, symbol)()
        if ver != expected:
            raise FedAvgLibraryError(f"ABI version {ver} != expected {expected}; rebuild the library")
        g[slot] = lib
    return lib


def _check(d: NativeLib, rc: int, what: str) -> None:
    """Raise on a non-zero status of a call into ``d``'s library, with that library's own message."""
    if rc != 0:
        msg = getattr(_load(d), d.last_error)().decode(errors="replace")
        raise FedAvgLibraryError(f"{what} failed (rc={rc}): {msg}")


# The loaders.  Warm, each reads its own module-level slot and returns it: load() runs once per product call.
def load() -> ctypes.CDLL:
    """The product library (include/fedavg_amd.h)."""
    return _lib if _lib is not None else _load(BY_KEY["product"])


def load_probe() -> ctypes.CDLL:
    """The probe library (product entry points + the tuning hooks of
    include/fedavg_amd_tuning.h).  Scripts and variant tests only; the
    product path never loads it."""
    return _probe if _probe is not None else _load(BY_KEY["probe"])


def load_fusedvec() -> ctypes.CDLL:
    """The fused aggregate + :291 library for fp64 / fp16 / bf16 rows
    (include/fedavg_amd_fusedvec.h); loads the product library first."""
    return _fusedvec if _fusedvec is not None else _load(BY_KEY["fusedvec"])


def load_segvec() -> ctypes.CDLL:
    """The zero-copy device-round library for fp64 / fp16 / bf16 groups (include/fedavg_amd_segvec.h)."""
    return _segvec if _segvec is not None else _load(BY_KEY["segvec"])


def load_clientvec() -> ctypes.CDLL:
    """The client-statistics library for bf16 / fp16 / fp64 models (include/fedavg_amd_clientvec.h)."""
    return _clientvec if _clientvec is not None else _load(BY_KEY["clientvec"])


def load_clientstep() -> ctypes.CDLL:
    """The fused client SGD step library for fp32 / bf16 / fp16 / fp64 models (include/fedavg_amd_clientstep.h)."""
    return _clientstep if _clientstep is not None else _load(BY_KEY["clientstep"])


def load_clientadam() -> ctypes.CDLL:
    """The fused client Adam step library for fp32 / bf16 / fp16 / fp64 models (include/fedavg_amd_clientadam.h)."""
    return _clientadam if _clientadam is not None else _load(DESCRIBED["clientadam"])


def load_clientloop() -> ctypes.CDLL:
    """The device-side guard and gated step library for fp32 / bf16 / fp64 models (include/fedavg_amd_clientloop.h)."""
    return _clientloop if _clientloop is not None else _load(EXTRA_BY_KEY["clientloop"])


check_fusedvec = functools.partial(_check, BY_KEY["fusedvec"])
check_segvec = functools.partial(_check, BY_KEY["segvec"])
check_clientvec = functools.partial(_check, BY_KEY["clientvec"])
check_clientstep = functools.partial(_check, BY_KEY["clientstep"])


def check_clientadam(rc: int, what: str) -> None:
    """``_check`` for the Adam step library (its description read at call time, as the loaders read theirs)."""
    _check(DESCRIBED["clientadam"], rc, what)


def check_clientloop(rc: int, what: str) -> None:
    """``_check`` for the guard and gated step library (its description read at call time)."""
    _check(EXTRA_BY_KEY["clientloop"], rc, what)


def check(rc: int, what: str, lib: ctypes.CDLL = None) -> None:
    """Raise on a non-zero status; the message comes from the library that
    made the call (``lib``; default: the product library, or the probe
    library when only that one is loaded)."""
    if rc != 0:
        src = lib if lib is not None else (_lib if _lib is not None or _probe is None else _probe)
        if src is None:
            src = load()
        msg = src.fedavg_last_error().decode(errors="replace")
        raise FedAvgLibraryError(f"{what} failed (rc={rc}): {msg}")


def f32_schedule(K: int, P: int, ld: int = 0) -> dict:
    """The schedule fedavg_reduce_f32 picks for an aligned [K, P] problem
    (P columns of rows with stride ld, when given)."""
    vals = [ctypes.c_int() for _ in range(4)]
    if ld:
        check(load().fedavg_f32_schedule_ld(K, P, ld, *[ctypes.byref(v) for v in vals]), "fedavg_f32_schedule_ld")
    else:
        check(load().fedavg_f32_schedule(K, P, *[ctypes.byref(v) for v in vals]), "fedavg_f32_schedule")
    sc = dict(zip(("unroll", "cols", "nontemporal", "launches"), (v.value for v in vals)))
    # report_production (csrc/fedavg_reduce.hip, the plan of csrc/reduce_plan.hpp
    # through the walk launch_production takes): nontemporal == 2 marks
    # the per-row buffer-descriptor kernel (nontemporal loads), 1 / 0 the
    # global-pointer variant kernel with / without them; 256-thread workgroups
    sc["kernel"] = "reduce_f32x4_buf_kernel" if sc["nontemporal"] == 2 else "reduce_f32x4_var_kernel"
    sc["block"] = 256
    return sc
