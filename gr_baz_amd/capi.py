"""ctypes binding of the C-ABI declared in include/baz_music_hip.h.

This is the same binding a maintainer of the reference would write on the python side if the
SWIG module were bypassed; the GNU Radio host block binds the same symbols
from C++.  There is no fallback: a missing library raises ImportError at first use, a missing
gfx950 device raises MusicError from Context().
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libbaz_music_hip.so")
# the same sources built with -DBAZ_MUSIC_LAB: reads the lab switches (ablations, geometry overrides, older kernels) the
# release library does not contain.  Only tests/lab and the A/B tests ask for it (Context(..., lab=True)).
LAB_LIB_PATH = os.path.join(_HERE, "csrc", "libbaz_music_hip_lab.so")

OK = 0
E_INVALID, E_NOMEM, E_HIP, E_UNSUPPORTED, E_NODEVICE = -1, -2, -3, -4, -5
STAGE_COV, STAGE_EVD, STAGE_SCAN, STAGE_MERGE, NUM_STAGES = 0, 1, 2, 3, 4
MAX_M, MAX_N = 64, 63     # BAZ_MUSIC_MAX_M / _MAX_N (specialised kernels up to m = 16, run-time-m kernels above)

# every symbol include/baz_music_hip.h declares (tests/test_abi.py checks the .so exports them all)
SYMBOLS = [
    "baz_music_create", "baz_music_destroy", "baz_music_set_table", "baz_music_process",
    "baz_music_process_device", "baz_music_process_device_on", "baz_music_set_stream", "baz_music_sync", "baz_music_reserve",
    "baz_music_profile", "baz_music_stage_ms", "baz_music_stage_name", "baz_music_debug_cov",
    "baz_music_debug_evd", "baz_music_debug_q", "baz_music_q_stride", "baz_music_bytes_per_item", "baz_music_strerror",
    "baz_music_last_hip_error", "baz_music_version", "baz_music_device_count", "baz_music_device", "baz_music_set_peak_mode", "baz_music_refined_items",
    "baz_music_refined_values", "baz_music_debug_coarse_margin", "baz_music_debug_coarse_fired",
    "baz_music_host_register", "baz_music_set_host_pinning", "baz_music_host_unregister_all", "baz_music_host_pinned_bytes",
    "baz_music_debug_i8_margin", "baz_music_debug_i8_stats", "baz_music_uses_i8_scan", "baz_music_debug_i8_image",
    "baz_music_debug_i8_nsplit", "baz_music_debug_sort_state", "baz_music_last_retune_ms", "baz_music_debug_table_image", "baz_music_debug_host_table_image",
    "baz_music_debug_guard_check", "baz_music_debug_guard_active", "baz_music_debug_live_buffers",
    "baz_music_set_smoothing", "baz_music_get_smoothing", "baz_music_smoothing_check",
    "baz_music_set_order_mode", "baz_music_get_order_mode", "baz_music_last_orders", "baz_music_last_orders_device",
    "baz_music_order_estimate",
    "baz_music_set_refine_mode", "baz_music_get_refine_mode", "baz_music_last_refine_offsets", "baz_music_refine_estimate",
    "baz_music_set_power_mode", "baz_music_get_power_mode", "baz_music_last_powers", "baz_music_power_estimate",
    "baz_music_set_beam_mode", "baz_music_get_beam_mode", "baz_music_last_beams", "baz_music_last_beams_device",
    "baz_music_last_beam_weights", "baz_music_beam_weights",
    "baz_music_set_calibration", "baz_music_get_calibration", "baz_music_calibration_apply",
    "baz_music_calibrate", "baz_music_calibrate_device", "baz_music_calibration_estimate",
    "baz_music_set_averaging", "baz_music_get_averaging", "baz_music_reset_averaging", "baz_music_averaging_weights",
    "baz_music_debug_average",
    "baz_music_set_estimator", "baz_music_get_estimator", "baz_music_spectrum_estimate",
    "baz_music_set_noise_covariance", "baz_music_get_noise_covariance", "baz_music_whitening_factor", "baz_music_whiten_table",
    "baz_music_debug_whiten", "baz_music_mean_covariance", "baz_music_mean_covariance_device",
    "baz_music_set_beamspace", "baz_music_get_beamspace", "baz_music_debug_beamspace", "baz_music_beamspace_apply",
    "baz_music_beamspace_design",
    "baz_music_set_subbands", "baz_music_set_subband_tables", "baz_music_get_subbands", "baz_music_debug_subbands",
    "baz_music_debug_subband_combine",
    "baz_music_subband_twiddles", "baz_music_subband_apply",
]
MAX_SUBBANDS = 32                   # BAZ_MUSIC_MAX_SUBBANDS
SUBBAND_HARMONIC, SUBBAND_ARITHMETIC = 0, 1   # BAZ_MUSIC_SUBBAND_*
ESTIMATOR_MUSIC, ESTIMATOR_CAPON, ESTIMATOR_BARTLETT = 0, 1, 2   # BAZ_MUSIC_ESTIMATOR_*
MAX_AVG_WINDOW = 64                 # BAZ_MUSIC_MAX_AVG_WINDOW
ORDER_MODES = {None: 0, "mdl": 1, "aic": 2}   # baz_music_set_order_mode: criterion by name
SMOOTH_WORKSPACE_BYTES = 128 << 20  # BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES: re-stacked items per chunk while smoothing is on

_vp = ctypes.c_void_p
_u32 = ctypes.c_uint32
_f32p = ctypes.POINTER(ctypes.c_float)

_lib = None
_lab_lib = None


class MusicError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        msg = "%s failed: %s (%d)" % (where, lib().baz_music_strerror(code).decode(), code)
        if detail:
            msg += " [" + detail + "]"
        super().__init__(msg)


def lib(lab=False):
    """Loads libbaz_music_hip.so (built in-tree by gr_baz_amd.build); never falls back.  lab=True: the -DBAZ_MUSIC_LAB form."""
    global _lib, _lab_lib
    if lab:
        if _lab_lib is None:
            path = LAB_LIB_PATH
            if os.environ.get("BAZ_MUSIC_LAB_LIB") == "quick":      # tests/lab iterations: python -m gr_baz_amd.build --quick
                path = os.path.join(os.path.dirname(LAB_LIB_PATH), "libbaz_music_hip_quick.so")
            if not os.path.exists(path):
                raise ImportError("gr_baz_amd: %s is missing - run `python -m gr_baz_amd.build`" % path)
            _lab_lib = _bind(ctypes.CDLL(path))
        return _lab_lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("gr_baz_amd: %s is missing - run `python -m gr_baz_amd.build` "
                          "(there is no CPU fallback for the MUSIC-DoA path)" % LIB_PATH)
    _lib = _bind(ctypes.CDLL(LIB_PATH))
    return _lib


def _bind(L):
    L.baz_music_create.restype = ctypes.c_int
    L.baz_music_create.argtypes = [ctypes.POINTER(_vp), _u32, _u32, _u32, _u32, _f32p, ctypes.c_int]
    L.baz_music_destroy.restype = None
    L.baz_music_destroy.argtypes = [_vp]
    L.baz_music_set_table.restype = ctypes.c_int
    L.baz_music_set_table.argtypes = [_vp, _f32p]
    L.baz_music_process.restype = ctypes.c_int
    L.baz_music_process.argtypes = [_vp, _f32p, _u32, _f32p, _f32p, _f32p]
    L.baz_music_process_device.restype = ctypes.c_int
    L.baz_music_process_device.argtypes = [_vp, _vp, _u32, _vp, _vp, _vp]
    L.baz_music_process_device_on.restype = ctypes.c_int
    L.baz_music_process_device_on.argtypes = [_vp, _vp, _vp, _u32, _vp, _vp, _vp]
    L.baz_music_set_stream.restype = ctypes.c_int
    L.baz_music_set_stream.argtypes = [_vp, _vp]
    L.baz_music_sync.restype = ctypes.c_int
    L.baz_music_sync.argtypes = [_vp]
    L.baz_music_reserve.restype = ctypes.c_int
    L.baz_music_reserve.argtypes = [_vp, _u32]
    L.baz_music_profile.restype = ctypes.c_int
    L.baz_music_profile.argtypes = [_vp, ctypes.c_int]
    L.baz_music_stage_ms.restype = ctypes.c_int
    L.baz_music_stage_ms.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_uint64)]
    L.baz_music_stage_name.restype = ctypes.c_char_p
    L.baz_music_stage_name.argtypes = [_vp, ctypes.c_int]
    L.baz_music_debug_cov.restype = ctypes.c_int
    L.baz_music_debug_cov.argtypes = [_vp, _vp, _u32, _vp]
    L.baz_music_debug_evd.restype = ctypes.c_int
    L.baz_music_debug_evd.argtypes = [_vp, _vp, _u32, _vp]
    L.baz_music_debug_q.restype = ctypes.c_int
    L.baz_music_debug_q.argtypes = [_vp, _vp, _u32, _vp]
    L.baz_music_q_stride.restype = _u32
    L.baz_music_q_stride.argtypes = [_u32]
    L.baz_music_bytes_per_item.restype = ctypes.c_uint64
    L.baz_music_bytes_per_item.argtypes = [_vp, ctypes.c_int]
    L.baz_music_strerror.restype = ctypes.c_char_p
    L.baz_music_strerror.argtypes = [ctypes.c_int]
    L.baz_music_last_hip_error.restype = ctypes.c_char_p
    L.baz_music_last_hip_error.argtypes = [_vp]
    L.baz_music_version.restype = ctypes.c_char_p
    L.baz_music_version.argtypes = []
    L.baz_music_device_count.restype = ctypes.c_int
    L.baz_music_device_count.argtypes = []
    L.baz_music_device.restype = ctypes.c_int
    L.baz_music_device.argtypes = [_vp]
    L.baz_music_refined_items.restype = ctypes.c_int64
    L.baz_music_refined_items.argtypes = [_vp]
    L.baz_music_refined_values.restype = ctypes.c_int64
    L.baz_music_refined_values.argtypes = [_vp]
    L.baz_music_debug_coarse_fired.restype = ctypes.c_int64
    L.baz_music_debug_coarse_fired.argtypes = [_vp]
    L.baz_music_debug_coarse_margin.restype = ctypes.c_int
    L.baz_music_debug_coarse_margin.argtypes = [_vp, _vp, _u32, ctypes.POINTER(ctypes.c_float)]
    L.baz_music_set_peak_mode.restype = ctypes.c_int
    L.baz_music_set_peak_mode.argtypes = [_vp, ctypes.c_int]
    L.baz_music_host_register.restype = ctypes.c_int
    L.baz_music_host_register.argtypes = [_vp, _vp, ctypes.c_size_t]
    L.baz_music_set_host_pinning.restype = ctypes.c_int
    L.baz_music_set_host_pinning.argtypes = [_vp, ctypes.c_int]
    L.baz_music_host_unregister_all.restype = ctypes.c_int
    L.baz_music_host_unregister_all.argtypes = [_vp]
    L.baz_music_host_pinned_bytes.restype = ctypes.c_uint64
    L.baz_music_host_pinned_bytes.argtypes = [_vp]
    L.baz_music_debug_i8_margin.restype = ctypes.c_int
    L.baz_music_debug_i8_margin.argtypes = [_vp, _vp, _u32, ctypes.POINTER(ctypes.c_float)]   # float worst[3]
    L.baz_music_debug_i8_stats.restype = ctypes.c_int
    L.baz_music_debug_i8_stats.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.baz_music_uses_i8_scan.restype = ctypes.c_int
    L.baz_music_uses_i8_scan.argtypes = [_vp]
    L.baz_music_debug_i8_nsplit.restype = _u32
    L.baz_music_debug_i8_nsplit.argtypes = [_u32, _u32, _u32]
    L.baz_music_debug_i8_image.restype = ctypes.c_size_t
    L.baz_music_debug_i8_image.argtypes = [_u32, _u32, _f32p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_double)]
    L.baz_music_debug_guard_check.restype = ctypes.c_int
    L.baz_music_debug_guard_check.argtypes = []
    L.baz_music_debug_live_buffers.restype = None
    L.baz_music_debug_live_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    L.baz_music_debug_guard_active.restype = ctypes.c_int
    L.baz_music_debug_guard_active.argtypes = []
    L.baz_music_debug_sort_state.restype = ctypes.c_int
    L.baz_music_debug_sort_state.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64)]
    L.baz_music_last_retune_ms.restype = ctypes.c_int
    L.baz_music_last_retune_ms.argtypes = [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.baz_music_debug_table_image.restype = ctypes.c_size_t
    L.baz_music_debug_table_image.argtypes = [_vp, ctypes.c_int, _vp, ctypes.c_size_t]
    L.baz_music_debug_host_table_image.restype = ctypes.c_size_t
    L.baz_music_debug_host_table_image.argtypes = [_u32, _u32, _u32, _f32p, ctypes.c_int, _vp, ctypes.c_size_t]
    L.baz_music_set_smoothing.restype = ctypes.c_int
    L.baz_music_set_smoothing.argtypes = [_vp, _u32, ctypes.c_int]
    L.baz_music_get_smoothing.restype = ctypes.c_int
    L.baz_music_get_smoothing.argtypes = [_vp, ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_int)]
    L.baz_music_smoothing_check.restype = ctypes.c_int
    L.baz_music_set_order_mode.restype = ctypes.c_int
    L.baz_music_set_order_mode.argtypes = [_vp, ctypes.c_int]
    L.baz_music_get_order_mode.restype = ctypes.c_int
    L.baz_music_get_order_mode.argtypes = [_vp, ctypes.POINTER(ctypes.c_int)]
    L.baz_music_last_orders.restype = ctypes.c_int
    L.baz_music_last_orders.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint8), _u32]
    L.baz_music_last_orders_device.restype = _vp
    L.baz_music_last_orders_device.argtypes = [_vp]
    L.baz_music_set_refine_mode.restype = ctypes.c_int
    L.baz_music_set_refine_mode.argtypes = [_vp, ctypes.c_int]
    L.baz_music_get_refine_mode.restype = ctypes.c_int
    L.baz_music_get_refine_mode.argtypes = [_vp, ctypes.POINTER(ctypes.c_int)]
    L.baz_music_last_refine_offsets.restype = ctypes.c_int
    L.baz_music_last_refine_offsets.argtypes = [_vp, ctypes.POINTER(ctypes.c_double), _u32]
    L.baz_music_set_power_mode.restype = ctypes.c_int
    L.baz_music_set_power_mode.argtypes = [_vp, ctypes.c_int]
    L.baz_music_get_power_mode.restype = ctypes.c_int
    L.baz_music_get_power_mode.argtypes = [_vp, ctypes.POINTER(ctypes.c_int)]
    L.baz_music_last_powers.restype = ctypes.c_int
    L.baz_music_last_powers.argtypes = [_vp, ctypes.POINTER(ctypes.c_double), _u32]
    L.baz_music_power_estimate.restype = ctypes.c_int
    L.baz_music_power_estimate.argtypes = [_u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), _u32,
                                           ctypes.POINTER(ctypes.c_double)]
    L.baz_music_set_beam_mode.restype = ctypes.c_int
    L.baz_music_set_beam_mode.argtypes = [_vp, ctypes.c_int, ctypes.c_double]
    L.baz_music_set_estimator.restype = ctypes.c_int
    L.baz_music_set_estimator.argtypes = [_vp, ctypes.c_int]
    L.baz_music_get_estimator.restype = ctypes.c_int
    L.baz_music_get_estimator.argtypes = [_vp, ctypes.POINTER(ctypes.c_int)]
    L.baz_music_spectrum_estimate.restype = ctypes.c_int
    L.baz_music_spectrum_estimate.argtypes = [ctypes.c_int, _u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), _u32,
                                              ctypes.POINTER(ctypes.c_double)]
    L.baz_music_get_beam_mode.restype = ctypes.c_int
    L.baz_music_get_beam_mode.argtypes = [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
    L.baz_music_last_beams.restype = ctypes.c_int
    L.baz_music_last_beams.argtypes = [_vp, ctypes.POINTER(ctypes.c_float), _u32]
    L.baz_music_last_beams_device.restype = ctypes.c_int
    L.baz_music_last_beams_device.argtypes = [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_u32)]
    L.baz_music_last_beam_weights.restype = ctypes.c_int
    L.baz_music_last_beam_weights.argtypes = [_vp, ctypes.POINTER(ctypes.c_double), _u32]
    L.baz_music_beam_weights.restype = ctypes.c_int
    L.baz_music_beam_weights.argtypes = [_u32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), _u32, ctypes.c_double,
                                         ctypes.POINTER(ctypes.c_double)]
    L.baz_music_refine_estimate.restype = ctypes.c_int
    L.baz_music_refine_estimate.argtypes = [ctypes.POINTER(ctypes.c_double), _u32, ctypes.POINTER(ctypes.c_double)]
    L.baz_music_order_estimate.restype = ctypes.c_int
    L.baz_music_order_estimate.argtypes = [_u32, _u32, _u32, ctypes.c_int, ctypes.POINTER(ctypes.c_double), _u32,
                                           ctypes.POINTER(ctypes.c_uint8)]
    L.baz_music_smoothing_check.argtypes = [_u32, _u32, _f32p, _u32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8)]
    L.baz_music_set_averaging.restype = ctypes.c_int
    L.baz_music_set_averaging.argtypes = [_vp, _u32, ctypes.c_double]
    L.baz_music_get_averaging.restype = ctypes.c_int
    L.baz_music_get_averaging.argtypes = [_vp, ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_double)]
    L.baz_music_reset_averaging.restype = ctypes.c_int
    L.baz_music_reset_averaging.argtypes = [_vp]
    L.baz_music_averaging_weights.restype = ctypes.c_int
    L.baz_music_averaging_weights.argtypes = [_u32, ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_double)]
    L.baz_music_debug_average.restype = ctypes.c_int
    L.baz_music_debug_average.argtypes = [_vp, _vp, _u32, _vp]
    _f64p = ctypes.POINTER(ctypes.c_double)
    L.baz_music_set_calibration.restype = ctypes.c_int
    L.baz_music_set_calibration.argtypes = [_vp, _f32p]
    L.baz_music_get_calibration.restype = ctypes.c_int
    L.baz_music_get_calibration.argtypes = [_vp, _f32p, ctypes.POINTER(ctypes.c_int)]
    L.baz_music_calibration_apply.restype = ctypes.c_int
    L.baz_music_calibration_apply.argtypes = [_u32, _u32, _f32p, _f32p, _f32p]
    L.baz_music_calibrate.restype = ctypes.c_int
    L.baz_music_calibrate.argtypes = [_vp, _f32p, _u32, _f32p, _f64p, _f64p, _f64p]
    L.baz_music_calibrate_device.restype = ctypes.c_int
    L.baz_music_calibrate_device.argtypes = [_vp, _vp, _u32, _f32p, _f64p, _f64p, _f64p]
    L.baz_music_calibration_estimate.restype = ctypes.c_int
    L.baz_music_calibration_estimate.argtypes = [_u32, _f64p, _f32p, _f64p, _f64p]
    L.baz_music_set_noise_covariance.restype = ctypes.c_int
    L.baz_music_set_noise_covariance.argtypes = [_vp, _f64p]
    L.baz_music_get_noise_covariance.restype = ctypes.c_int
    L.baz_music_get_noise_covariance.argtypes = [_vp, _f64p, ctypes.POINTER(ctypes.c_int)]
    L.baz_music_whitening_factor.restype = ctypes.c_int
    L.baz_music_whitening_factor.argtypes = [_u32, _f64p, _f64p]
    L.baz_music_whiten_table.restype = ctypes.c_int
    L.baz_music_whiten_table.argtypes = [_u32, _u32, _f32p, _f64p, _f32p]
    L.baz_music_debug_whiten.restype = ctypes.c_int
    L.baz_music_debug_whiten.argtypes = [_vp, _vp, _u32, _vp]
    L.baz_music_mean_covariance.restype = ctypes.c_int
    L.baz_music_mean_covariance.argtypes = [_vp, _f32p, _u32, _f64p]
    L.baz_music_mean_covariance_device.restype = ctypes.c_int
    L.baz_music_mean_covariance_device.argtypes = [_vp, _vp, _u32, _f64p]
    L.baz_music_set_beamspace.restype = ctypes.c_int
    L.baz_music_set_beamspace.argtypes = [_vp, _u32, _f64p, ctypes.c_int]
    L.baz_music_get_beamspace.restype = ctypes.c_int
    L.baz_music_get_beamspace.argtypes = [_vp, ctypes.POINTER(_u32), _f64p, ctypes.POINTER(ctypes.c_int)]
    L.baz_music_debug_beamspace.restype = ctypes.c_int
    L.baz_music_debug_beamspace.argtypes = [_vp, _vp, _u32, _vp]
    L.baz_music_beamspace_apply.restype = ctypes.c_int
    L.baz_music_beamspace_apply.argtypes = [_u32, _u32, _f64p, ctypes.c_int, _f32p, _u32, _f32p]
    L.baz_music_beamspace_design.restype = ctypes.c_int
    L.baz_music_beamspace_design.argtypes = [_u32, _u32, _f32p, _u32, _u32, _u32, _f64p, _f64p]
    _u32p = ctypes.POINTER(_u32)
    L.baz_music_set_subbands.restype = ctypes.c_int
    L.baz_music_set_subbands.argtypes = [_vp, _u32, _u32, _u32p, _f32p, ctypes.c_int]
    L.baz_music_set_subband_tables.restype = ctypes.c_int
    L.baz_music_set_subband_tables.argtypes = [_vp, _f32p]
    L.baz_music_get_subbands.restype = ctypes.c_int
    L.baz_music_get_subbands.argtypes = [_vp, _u32p, _u32p, _u32p, ctypes.POINTER(ctypes.c_int)]
    L.baz_music_debug_subbands.restype = ctypes.c_int
    L.baz_music_debug_subbands.argtypes = [_vp, _vp, _u32, _vp]
    L.baz_music_debug_subband_combine.restype = ctypes.c_int
    L.baz_music_debug_subband_combine.argtypes = [_vp, _vp, _u32, _vp]
    L.baz_music_subband_twiddles.restype = ctypes.c_int
    L.baz_music_subband_twiddles.argtypes = [_u32, _u32, _u32p, _f64p]
    L.baz_music_subband_apply.restype = ctypes.c_int
    L.baz_music_subband_apply.argtypes = [_u32, _u32, _u32, _f64p, _f32p, _u32, _f32p]
    return L


def _table_f32(table, res, m):
    t = np.ascontiguousarray(np.asarray(table, dtype=np.complex64))
    if t.shape != (res, m):
        raise ValueError("array_response must be resolution x m = %dx%d, got %s" % (res, m, t.shape))
    return t


class Context:
    """One baz_music_ctx: the device-side state of one baz_music_doa block instance."""

    def __init__(self, m, n, nsamples, resolution, table, device_id=-1, lab=None):
        # lab=None: the lab form of the library where BAZ_MUSIC_LAB_LIB is set (lab / quick: tests/lab harnesses whose switches
        # the release form does not read), else the release form
        if lab is None:
            lab = bool(os.environ.get("BAZ_MUSIC_LAB_LIB"))
        L = self._L = lib(lab)
        self.m, self.n, self.nsamples, self.res = int(m), int(n), int(nsamples), int(resolution)
        t = _table_f32(table, self.res, self.m) if (self.res > 0 and self.m > 0) else \
            np.zeros((1, 1), np.complex64)
        h = _vp()
        r = L.baz_music_create(ctypes.byref(h), self.m, self.n, self.nsamples, self.res,
                               t.view(np.float32).ctypes.data_as(_f32p), int(device_id))
        if r != OK:
            raise MusicError(r, "baz_music_create")
        self._h = h

    def _chk(self, r, where):
        if r < 0:
            raise MusicError(r, where, self._L.baz_music_last_hip_error(self._h).decode())
        return r

    def close(self):
        if getattr(self, "_h", None):
            self._L.baz_music_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_table(self, table):
        t = _table_f32(table, self.res, self.m)
        self._chk(self._L.baz_music_set_table(self._h, t.view(np.float32).ctypes.data_as(_f32p)),
                  "baz_music_set_table")

    def debug_sort_state(self):
        """{"sorted_calls", "unsorted_calls", "fired", "walked", "last_sorted"} of the gated scan's sorting policy (synchronises)."""
        v = (ctypes.c_uint64 * 5)()
        self._chk(self._L.baz_music_debug_sort_state(self._h, v), "baz_music_debug_sort_state")
        return {"sorted_calls": int(v[0]), "unsorted_calls": int(v[1]), "fired": int(v[2]), "walked": int(v[3]), "last_sorted": bool(v[4])}

    def last_retune_ms(self):
        """(wall milliseconds of the last set_table, milliseconds of it spent waiting for / holding the lock shared with process)."""
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._chk(self._L.baz_music_last_retune_ms(self._h, ctypes.byref(a), ctypes.byref(b)), "baz_music_last_retune_ms")
        return float(a.value), float(b.value)

    def debug_table_image(self, which):
        """Image `which` of the table in force, copied back from the device (uint8 array), or None when the configuration has none."""
        n = int(self._L.baz_music_debug_table_image(self._h, int(which), None, 0))
        if n == 0:
            return None
        out = np.zeros(n, np.uint8)
        got = int(self._L.baz_music_debug_table_image(self._h, int(which), _vp(out.ctypes.data), n))
        if got != n:
            raise MusicError(E_HIP, "baz_music_debug_table_image")
        return out

    def process(self, items, want_lvl=True, want_spectrum=True, out=None):
        """items: (batch, nsamples) complex64 host array -> (ang, lvl|None, spectrum|None).
        out: optional (ang, lvl|None, spectrum|None) float32 C-contiguous arrays to write into (a scheduler's
        persistent buffers; page-locked ones are handed to the DMA engines without staging)."""
        x = np.ascontiguousarray(np.asarray(items, dtype=np.complex64))
        if x.ndim == 1:
            x = x[None, :]
        if x.shape[1] != self.nsamples:
            raise ValueError("items must be (batch, %d) complex64" % self.nsamples)
        B = x.shape[0]
        if out is not None:
            ang, lvl, spec = out
            want_lvl, want_spectrum = lvl is not None, spec is not None
            for a, cols in ((ang, self.n), (lvl, self.n), (spec, self.res)):
                if a is not None and (a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"] or a.shape != (B, cols)):
                    raise ValueError("out arrays must be C-contiguous float32 of shape (batch, n|n|resolution)")
        else:
            ang = np.zeros((B, self.n), np.float32)
            lvl = np.zeros((B, self.n), np.float32) if want_lvl else None
            spec = np.zeros((B, self.res), np.float32) if want_spectrum else None
        r = self._L.baz_music_process(
            self._h, x.view(np.float32).ctypes.data_as(_f32p), B, ang.ctypes.data_as(_f32p),
            lvl.ctypes.data_as(_f32p) if want_lvl else None,
            spec.ctypes.data_as(_f32p) if want_spectrum else None)
        self._chk(r, "baz_music_process")
        return ang, lvl, spec

    # ---- device-resident path (pointers are plain integers, e.g. torch.Tensor.data_ptr()) ----
    def process_device(self, d_in, batch, d_ang, d_lvl=None, d_spec=None, stream=None):
        """Enqueues one batch.  stream=None: on the context's stream, unordered against other streams (the caller
        orders: set_stream(), sync(), or a device-wide synchronize).  stream=<hipStream_t as int, 0 = the legacy
        default stream, e.g. torch.cuda.current_stream().cuda_stream>: with stream semantics relative to it."""
        if stream is None:
            r = self._L.baz_music_process_device(self._h, _vp(d_in), int(batch), _vp(d_ang),
                                               _vp(d_lvl) if d_lvl else None, _vp(d_spec) if d_spec else None)
        else:
            r = self._L.baz_music_process_device_on(self._h, _vp(stream) if stream else None, _vp(d_in), int(batch),
                                                  _vp(d_ang), _vp(d_lvl) if d_lvl else None,
                                                  _vp(d_spec) if d_spec else None)
        self._chk(r, "baz_music_process_device")

    def refined_values(self):
        """(item, bin) VALUES of the last process call that were recomputed in the reference's literal form (near-null
        bins, extreme SNR) -- not items: one item can contribute up to `resolution` of them.  On the wide path counted by the
        matrix-core scan only (17 <= m <= 64, n <= 8), else 0."""
        return int(self._L.baz_music_refined_values(self._h))

    refined_items = refined_values      # the round-1 name of the same statistic (kept for callers; the unit is values)

    def debug_coarse_fired(self):
        """Lab statistic (context created under BAZ_MUSIC_COARSE_STATS=1): exact tile evaluations since the last read."""
        return int(self._L.baz_music_debug_coarse_fired(self._h))

    def debug_coarse_margin(self, d_in, batch):
        """Worst observed |coarse - exact| / allowance of the coarse-gated scan over every (item, bin) of the batch
        (baz_music_debug_coarse_margin; the gate is sound below 1)."""
        w = ctypes.c_float(0.0)
        self._chk(self._L.baz_music_debug_coarse_margin(self._h, _vp(d_in), int(batch), ctypes.byref(w)),
                  "baz_music_debug_coarse_margin")
        return float(w.value)

    def uses_i8_scan(self):
        """True when this context's scan runs on the int8 matrix core (6 <= m <= 16, n <= 4, not BAZ_MUSIC_EXACT=1)."""
        return bool(self._L.baz_music_uses_i8_scan(self._h))

    def debug_i8_margin(self, d_in, batch):
        """(worst |d5 - d| / E5, worst |d7 - d| / allowance, worst |d4 - d| / E4) of the int8 scan's five-, seven- and
        four-digit forms over every (item, bin) of the batch, against the fp64 form (the bounds hold below 1)."""
        w = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
        self._chk(self._L.baz_music_debug_i8_margin(self._h, _vp(d_in), int(batch), w), "baz_music_debug_i8_margin")
        return float(w[0]), float(w[1]), float(w[2])

    def debug_i8_stats(self):
        """(wave tiles -- 16 items x 16 bins -- that ran the refined form, wave tiles walked) of the int8 scan since the last read; resets."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._chk(self._L.baz_music_debug_i8_stats(self._h, ctypes.byref(a), ctypes.byref(b)), "baz_music_debug_i8_stats")
        return int(a.value), int(b.value)

    # ---- page-locking of caller buffers that live across calls (a scheduler's stream buffers) ----
    def host_register(self, array):
        """Page-locks a numpy array's memory for this context (the array must outlive the registration: call
        host_unregister_all() or close() before dropping it).  Returns the library's code: 0 = locked (or already was)."""
        return int(self._L.baz_music_host_register(self._h, _vp(array.ctypes.data), array.nbytes))

    def set_host_pinning(self, enable):
        """process() page-locks the ranges of every call the first time it sees them (persistent buffers only)."""
        self._chk(self._L.baz_music_set_host_pinning(self._h, 1 if enable else 0), "baz_music_set_host_pinning")

    def host_unregister_all(self):
        self._chk(self._L.baz_music_host_unregister_all(self._h), "baz_music_host_unregister_all")

    def host_pinned_bytes(self):
        return int(self._L.baz_music_host_pinned_bytes(self._h))

    def set_peak_mode(self, mode):
        """0: the reference's n strongest bins (default); 1: n strongest local maxima (opt-in extension)."""
        self._chk(self._L.baz_music_set_peak_mode(self._h, int(mode)), "baz_music_set_peak_mode")

    def set_smoothing(self, subarray, forward_backward=False):
        """Opt-in extension (not reference behaviour): forward-backward averaging and/or spatial smoothing over subarrays of
        `subarray` elements (include/baz_music_hip.h).  set_smoothing(m, False) switches it off."""
        self._chk(self._L.baz_music_set_smoothing(self._h, int(subarray), 1 if forward_backward else 0),
                  "baz_music_set_smoothing")

    def get_smoothing(self):
        """(subarray, forward_backward) in force; (m, False) while the mode is off."""
        ms, fb = _u32(0), ctypes.c_int(0)
        self._chk(self._L.baz_music_get_smoothing(self._h, ctypes.byref(ms), ctypes.byref(fb)), "baz_music_get_smoothing")
        return int(ms.value), bool(fb.value)

    def set_order_mode(self, criterion):
        """Opt-in extension (not reference behaviour): per-item emitter count by "mdl" or "aic"; the context's n becomes the
        largest count and every item reports its own count of pairs, then (0, 0) (include/baz_music_hip.h).  None: off."""
        if criterion not in ORDER_MODES:
            raise ValueError("order mode must be 'mdl', 'aic' or None, not %r" % (criterion,))
        self._chk(self._L.baz_music_set_order_mode(self._h, ORDER_MODES[criterion]), "baz_music_set_order_mode")

    def get_order_mode(self):
        """"mdl", "aic" or None (off)."""
        crit = ctypes.c_int(0)
        self._chk(self._L.baz_music_get_order_mode(self._h, ctypes.byref(crit)), "baz_music_get_order_mode")
        return {v: k for k, v in ORDER_MODES.items()}[int(crit.value)]

    def last_orders(self, count):
        """Emitter counts (uint8) of the first `count` items of the last process*() call; n for a call made with the mode off."""
        out = np.zeros(max(int(count), 1), np.uint8)
        r = self._L.baz_music_last_orders(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), int(count))
        if r < 0:
            self._chk(r, "baz_music_last_orders")
        return out[:r].copy()

    def last_orders_device(self):
        """Device address of the same bytes (0 before the first call); valid until the next process*() call."""
        return int(self._L.baz_music_last_orders_device(self._h) or 0)

    def set_refine_mode(self, mode):
        """Opt-in extension (not reference behaviour): 1 moves every reported angle off the grid by a parabolic fit of the MUSIC
        denominator at its bin and the two neighbours (include/baz_music_hip.h); 0 (default): the reference's grid angles."""
        self._chk(self._L.baz_music_set_refine_mode(self._h, int(mode)), "baz_music_set_refine_mode")

    def get_refine_mode(self):
        mode = ctypes.c_int(0)
        self._chk(self._L.baz_music_get_refine_mode(self._h, ctypes.byref(mode)), "baz_music_get_refine_mode")
        return int(mode.value)

    def last_refine_offsets(self, count):
        """Sub-bin offsets (float64, in bins) of the first `count` (item, slot) entries of the last process*() call; zeros for a
        call made with the mode off."""
        out = np.zeros(max(int(count), 1), np.float64)
        r = self._L.baz_music_last_refine_offsets(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(count))
        if r < 0:
            self._chk(r, "baz_music_last_refine_offsets")
        return out[:r].copy()

    def set_averaging(self, window, forgetting=1.0):
        """Opt-in extension (not reference behaviour): every item's covariance becomes the weighted mean over the last `window`
        items of this context's stream, weights forgetting ** age (include/baz_music_hip.h).  window 1: off."""
        self._chk(self._L.baz_music_set_averaging(self._h, int(window), float(forgetting)), "baz_music_set_averaging")

    def get_averaging(self):
        """(window, forgetting) in force; (1, 1.0) for a context never set."""
        w, b = _u32(0), ctypes.c_double(0.0)
        self._chk(self._L.baz_music_get_averaging(self._h, ctypes.byref(w), ctypes.byref(b)), "baz_music_get_averaging")
        return int(w.value), float(b.value)

    def reset_averaging(self):
        """Forgets the averaging history: the next item is the first of its stream."""
        self._chk(self._L.baz_music_reset_averaging(self._h), "baz_music_reset_averaging")

    def debug_average(self, d_R_in, batch, d_R_out):
        """The averaging stage alone on `batch` caller-supplied covariances (device pointers); advances the history like a
        process call of `batch` items."""
        self._chk(self._L.baz_music_debug_average(self._h, _vp(d_R_in), int(batch), _vp(d_R_out)), "baz_music_debug_average")

    def set_power_mode(self, mode):
        """Opt-in extension (not reference behaviour): 1 computes a Capon power estimate 1 / Re(a^H R^-1 a) per reported entry
        (last_powers; every port unchanged), 2 additionally puts (float)P on the lvl port (include/baz_music_hip.h); 0 (default): off."""
        self._chk(self._L.baz_music_set_power_mode(self._h, int(mode)), "baz_music_set_power_mode")

    def get_power_mode(self):
        mode = ctypes.c_int(0)
        self._chk(self._L.baz_music_get_power_mode(self._h, ctypes.byref(mode)), "baz_music_get_power_mode")
        return int(mode.value)

    def last_powers(self, count):
        """Capon powers (float64, in the units of R) of the first `count` (item, slot) entries of the last process*() call; zeros for
        a call made with the mode off."""
        out = np.zeros(max(int(count), 1), np.float64)
        r = self._L.baz_music_last_powers(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(count))
        if r < 0:
            self._chk(r, "baz_music_last_powers")
        return out[:r].copy()

    def set_estimator(self, kind):
        """Opt-in extension (not reference behaviour): the spectrum estimator -- ESTIMATOR_MUSIC (0, the default: the reference),
        ESTIMATOR_CAPON (1) or ESTIMATOR_BARTLETT (2): powers in the units of R for every bin, ang / lvl picked from the float32
        spectrum (include/baz_music_hip.h)."""
        self._chk(self._L.baz_music_set_estimator(self._h, int(kind)), "baz_music_set_estimator")

    def get_estimator(self):
        kind = ctypes.c_int(0)
        self._chk(self._L.baz_music_get_estimator(self._h, ctypes.byref(kind)), "baz_music_get_estimator")
        return int(kind.value)

    def set_beam_mode(self, mode, loading=0.0):
        """Opt-in extension (not reference behaviour): 1 computes the MVDR weights w = R^-1 a / (a^H R^-1 a) of every reported entry
        and the beam y = w^H X over the item's snapshots (last_beams, last_beam_weights; every port unchanged); `loading` adds
        loading * mean diagonal to R's diagonal (include/baz_music_hip.h); 0 (default): off."""
        self._chk(self._L.baz_music_set_beam_mode(self._h, int(mode), float(loading)), "baz_music_set_beam_mode")

    def get_beam_mode(self):
        """(mode, loading) in force."""
        mode, loading = ctypes.c_int(0), ctypes.c_double(0.0)
        self._chk(self._L.baz_music_get_beam_mode(self._h, ctypes.byref(mode), ctypes.byref(loading)), "baz_music_get_beam_mode")
        return int(mode.value), float(loading.value)

    def last_beams(self, items):
        """Beams (complex64, shape (items, n, K)) of the first `items` items of the last process*() call; zeros for a call made with
        the mode off."""
        K = self.nsamples // self.m
        out = np.zeros((max(int(items), 1), self.n, K), np.complex64)
        r = self._L.baz_music_last_beams(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(items))
        if r < 0:
            self._chk(r, "baz_music_last_beams")
        return out[:r].copy()

    def last_beam_weights(self, items):
        """MVDR weights (complex128, shape (items, n, m)) of the first `items` items of the last process*() call; zeros for a call
        made with the mode off."""
        out = np.zeros((max(int(items), 1), self.n, self.m), np.complex128)
        r = self._L.baz_music_last_beam_weights(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(items))
        if r < 0:
            self._chk(r, "baz_music_last_beam_weights")
        return out[:r].copy()

    def last_beams_device(self):
        """(device pointer, items) of the buffer behind last_beams, [item][slot][K] complex64: ordered on the context's stream, valid
        until the next process*(), set_* or destroy; (0, 0) after a call made with the mode off.  Does not synchronise."""
        p, items = _vp(None), _u32(0)
        self._chk(self._L.baz_music_last_beams_device(self._h, ctypes.byref(p), ctypes.byref(items)), "baz_music_last_beams_device")
        return int(p.value or 0), int(items.value)

    def set_calibration(self, gamma):
        """Opt-in extension (not reference behaviour): the table in force becomes gamma_r * a_r(bin) for the m complex gains `gamma`
        (every one finite and nonzero), across later set_table calls too (include/baz_music_hip.h); None (default): off."""
        if gamma is None:
            self._chk(self._L.baz_music_set_calibration(self._h, None), "baz_music_set_calibration")
            return
        g = np.ascontiguousarray(np.asarray(gamma, dtype=np.complex64).reshape(-1))
        if g.shape != (self.m,):
            raise ValueError("gamma must hold m = %d complex values" % self.m)
        self._chk(self._L.baz_music_set_calibration(self._h, g.view(np.float32).ctypes.data_as(_f32p)), "baz_music_set_calibration")

    def get_calibration(self):
        """The m complex64 gains in force, or None while the mode is off."""
        g, on = np.zeros(self.m, np.complex64), ctypes.c_int(0)
        self._chk(self._L.baz_music_get_calibration(self._h, g.view(np.float32).ctypes.data_as(_f32p), ctypes.byref(on)),
                  "baz_music_get_calibration")
        return g if on.value else None

    def _calibrate(self, call, where, inp, batch, ref, want_rbar):
        p = np.ascontiguousarray(np.asarray(ref, dtype=np.complex64).reshape(-1))
        if p.shape != (self.m,):
            raise ValueError("ref must hold m = %d complex values" % self.m)
        g, q = np.zeros(self.m, np.complex128), ctypes.c_double(0.0)
        rbar = np.zeros((self.m, self.m), np.complex128) if want_rbar else None
        f64p = ctypes.POINTER(ctypes.c_double)
        self._chk(call(self._h, inp, int(batch), p.view(np.float32).ctypes.data_as(_f32p), g.view(np.float64).ctypes.data_as(f64p),
                       ctypes.byref(q), rbar.view(np.float64).ctypes.data_as(f64p) if want_rbar else None), where)
        return (g, float(q.value), rbar) if want_rbar else (g, float(q.value))

    def calibrate(self, items, ref, want_rbar=False):
        """Estimates the gains from pilot items ((batch, nsamples) complex64 host array) and the pilot's ideal response `ref` (m complex):
        (gamma complex128[m], quality[, Rbar complex128[m, m]]).  Does not apply them: set_calibration(gamma.astype(complex64))."""
        x = np.ascontiguousarray(np.asarray(items, dtype=np.complex64))
        if x.ndim == 1:
            x = x[None, :]
        if x.shape[1] != self.nsamples:
            raise ValueError("items must be (batch, %d) complex64" % self.nsamples)
        return self._calibrate(self._L.baz_music_calibrate, "baz_music_calibrate", x.view(np.float32).ctypes.data_as(_f32p), x.shape[0],
                               ref, want_rbar)

    def calibrate_device(self, d_in, batch, ref, want_rbar=False):
        """calibrate() on `batch` items in device memory (d_in: a plain integer pointer); blocks, the results are host arrays."""
        return self._calibrate(self._L.baz_music_calibrate_device, "baz_music_calibrate_device", _vp(d_in), batch, ref, want_rbar)

    def set_noise_covariance(self, rn):
        """Opt-in extension (not reference behaviour): noise pre-whitening with the m x m noise covariance `rn` (Hermitian positive
        definite; its lower triangle is read).  The EVD decomposes W R W^H and the table in force becomes W a, W the inverse of rn's
        Cholesky factor, across later set_table / set_calibration calls too (include/baz_music_hip.h); None (default): off."""
        if rn is None:
            self._chk(self._L.baz_music_set_noise_covariance(self._h, None), "baz_music_set_noise_covariance")
            return
        R = np.ascontiguousarray(np.asarray(rn, dtype=np.complex128))
        if R.shape != (self.m, self.m):
            raise ValueError("rn must be an m x m = %d x %d complex matrix" % (self.m, self.m))
        self._chk(self._L.baz_music_set_noise_covariance(self._h, R.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                  "baz_music_set_noise_covariance")

    def get_noise_covariance(self):
        """The noise covariance in force (m x m complex128, as given), or None while the mode is off."""
        R, on = np.zeros((self.m, self.m), np.complex128), ctypes.c_int(0)
        self._chk(self._L.baz_music_get_noise_covariance(self._h, R.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                         ctypes.byref(on)), "baz_music_get_noise_covariance")
        return R if on.value else None

    def debug_whiten(self, d_R_in, batch, d_R_out):
        """The whitening stage alone on `batch` caller-supplied covariances (device pointers, m*m complex128 each, not overlapping)."""
        self._chk(self._L.baz_music_debug_whiten(self._h, _vp(d_R_in), int(batch), _vp(d_R_out)), "baz_music_debug_whiten")

    def set_beamspace(self, T, normalise=False):
        """Opt-in extension (not reference behaviour): beamspace MUSIC.  `T` (m x B complex, 2 <= B <= min(m, 16), n < B) projects every
        snapshot onto B beams, y = T^H x, and an inner context of B antennas on the table T^H a does the rest -- with every opt-in
        mode, also for 17 .. 64 antennas (include/baz_music_hip.h).  None: off (the default)."""
        if T is None:
            self._chk(self._L.baz_music_set_beamspace(self._h, 0, None, 0), "baz_music_set_beamspace")
            return
        t = np.ascontiguousarray(np.asarray(T, dtype=np.complex128))
        if t.ndim != 2 or t.shape[0] != self.m or t.shape[1] < 1:
            raise ValueError("T must be m x B = %d x B complex" % self.m)
        self._chk(self._L.baz_music_set_beamspace(self._h, t.shape[1], t.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  1 if normalise else 0), "baz_music_set_beamspace")

    def get_beamspace(self):
        """(T, normalise) in force (T: m x B complex128, as given), or None while the mode is off."""
        B, nrm = _u32(0), ctypes.c_int(0)
        self._chk(self._L.baz_music_get_beamspace(self._h, ctypes.byref(B), None, ctypes.byref(nrm)), "baz_music_get_beamspace")
        if not B.value:
            return None
        t = np.zeros((self.m, B.value), np.complex128)
        self._chk(self._L.baz_music_get_beamspace(self._h, ctypes.byref(B), t.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  ctypes.byref(nrm)), "baz_music_get_beamspace")
        return t, bool(nrm.value)

    def debug_beamspace(self, d_in, batch, d_out):
        """The projection alone: `batch` items (device pointer, m K complex64 each) -> batch K B complex64 at d_out (not overlapping)."""
        self._chk(self._L.baz_music_debug_beamspace(self._h, _vp(d_in), int(batch), _vp(d_out)), "baz_music_debug_beamspace")

    def _subband_tables(self, tables, S):
        t = np.ascontiguousarray(np.asarray(tables, dtype=np.complex64))
        if t.shape != (S, self.res, self.m):
            raise ValueError("tables must be S x resolution x m = %d x %d x %d complex" % (S, self.res, self.m))
        return t

    def set_subbands(self, F, bins=None, tables=None, combine=SUBBAND_HARMONIC):
        """Opt-in extension (not reference behaviour): wideband (subband) MUSIC.  Every item is cut into blocks of `F` samples, an F-point
        DFT per antenna separates the subbands `bins` (distinct DFT indices below F), an inner context per subband runs on
        `tables[s]` (S x resolution x m complex) and the S spectra are combined (`combine`: SUBBAND_HARMONIC, the sum of the MUSIC
        denominators, or SUBBAND_ARITHMETIC) into the row the pickers read (include/baz_music_hip.h).  F None or 0: off (the default)."""
        if not F:
            self._chk(self._L.baz_music_set_subbands(self._h, 0, 0, None, None, 0), "baz_music_set_subbands")
            return
        b = np.ascontiguousarray(np.asarray(bins, dtype=np.int64).reshape(-1))
        if b.size < 1 or (b < 0).any() or (b > 0xffffffff).any():
            raise ValueError("bins must be a non-empty list of DFT indices")
        b = b.astype(np.uint32)
        t = self._subband_tables(tables, b.size)
        self._chk(self._L.baz_music_set_subbands(self._h, int(F), b.size, b.ctypes.data_as(ctypes.POINTER(_u32)),
                                                 t.view(np.float32).ctypes.data_as(_f32p), int(combine)), "baz_music_set_subbands")

    def set_subband_tables(self, tables):
        """Retunes all S subband tables at once (S x resolution x m complex): a batch sees all old tables or all new ones."""
        cur = self.get_subbands()
        if cur is None:
            raise MusicError(E_UNSUPPORTED, "baz_music_set_subband_tables: the subband mode is off")
        t = self._subband_tables(tables, len(cur[1]))
        self._chk(self._L.baz_music_set_subband_tables(self._h, t.view(np.float32).ctypes.data_as(_f32p)), "baz_music_set_subband_tables")

    def get_subbands(self):
        """(F, bins, combine) in force, or None while the mode is off."""
        F, S, cmb = _u32(0), _u32(0), ctypes.c_int(0)
        self._chk(self._L.baz_music_get_subbands(self._h, ctypes.byref(F), ctypes.byref(S), None, ctypes.byref(cmb)), "baz_music_get_subbands")
        if not F.value:
            return None
        bins = np.zeros(MAX_SUBBANDS, np.uint32)
        self._chk(self._L.baz_music_get_subbands(self._h, ctypes.byref(F), ctypes.byref(S), bins.ctypes.data_as(ctypes.POINTER(_u32)),
                                                 ctypes.byref(cmb)), "baz_music_get_subbands")
        return int(F.value), [int(k) for k in bins[:S.value]], int(cmb.value)

    def debug_subbands(self, d_in, batch, d_out):
        """The channeliser alone: `batch` items (device pointer, m K complex64 each) -> S batch (K/F) m complex64 at d_out, laid out
        [subband][item][block][antenna] (not overlapping)."""
        self._chk(self._L.baz_music_debug_subbands(self._h, _vp(d_in), int(batch), _vp(d_out)), "baz_music_debug_subbands")

    def debug_subband_combine(self, d_spectra, batch, d_out):
        """The combine alone under the S and the rule in force: S batch resolution float32 ([subband][item][bin], device pointer) ->
        batch resolution float32 at d_out (not overlapping)."""
        self._chk(self._L.baz_music_debug_subband_combine(self._h, _vp(d_spectra), int(batch), _vp(d_out)), "baz_music_debug_subband_combine")

    def mean_covariance(self, items):
        """The mean covariance Rbar (m x m complex128) of items ((batch, nsamples) complex64 host array): calibrate()'s Rbar without
        a pilot -- of a noise-only capture, an estimate of the noise covariance for set_noise_covariance.  Blocks; changes nothing."""
        x = np.ascontiguousarray(np.asarray(items, dtype=np.complex64))
        if x.ndim == 1:
            x = x[None, :]
        if x.shape[1] != self.nsamples:
            raise ValueError("items must be (batch, %d) complex64" % self.nsamples)
        R = np.zeros((self.m, self.m), np.complex128)
        self._chk(self._L.baz_music_mean_covariance(self._h, x.view(np.float32).ctypes.data_as(_f32p), x.shape[0],
                                                    R.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                  "baz_music_mean_covariance")
        return R

    def mean_covariance_device(self, d_in, batch):
        """mean_covariance() on `batch` items in device memory (d_in: a plain integer pointer); blocks, the result is a host array."""
        R = np.zeros((self.m, self.m), np.complex128)
        self._chk(self._L.baz_music_mean_covariance_device(self._h, _vp(d_in), int(batch),
                                                           R.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                  "baz_music_mean_covariance_device")
        return R

    def set_stream(self, hip_stream):
        self._chk(self._L.baz_music_set_stream(self._h, _vp(hip_stream) if hip_stream else None),
                  "baz_music_set_stream")

    def sync(self):
        self._chk(self._L.baz_music_sync(self._h), "baz_music_sync")

    def reserve(self, max_batch):
        self._chk(self._L.baz_music_reserve(self._h, int(max_batch)), "baz_music_reserve")

    def profile(self, enable):
        """enable: False/0 off, True/1 every stage, 2 only the scan stage (cheapest)."""
        self._chk(self._L.baz_music_profile(self._h, int(enable)), "baz_music_profile")

    def stage_ms(self, stage):
        ms = ctypes.c_double(0.0)
        cnt = ctypes.c_uint64(0)
        self._chk(self._L.baz_music_stage_ms(self._h, stage, ctypes.byref(ms), ctypes.byref(cnt)),
                  "baz_music_stage_ms")
        return ms.value, cnt.value

    def stage_name(self, stage):
        return self._L.baz_music_stage_name(self._h, stage).decode()

    def debug_cov(self, d_in, batch, d_R):
        self._chk(self._L.baz_music_debug_cov(self._h, _vp(d_in), int(batch), _vp(d_R)), "baz_music_debug_cov")

    def debug_evd(self, d_R, batch, d_Q):
        self._chk(self._L.baz_music_debug_evd(self._h, _vp(d_R), int(batch), _vp(d_Q)), "baz_music_debug_evd")

    def debug_q(self, d_in, batch, d_Q):
        self._chk(self._L.baz_music_debug_q(self._h, _vp(d_in), int(batch), _vp(d_Q)), "baz_music_debug_q")

    def bytes_per_item(self, with_spectrum=True):
        return int(self._L.baz_music_bytes_per_item(self._h, 1 if with_spectrum else 0))


def debug_i8_image(m, resolution, table):
    """HOST-ONLY: (image bytes as a uint8 array -- [step][tile][block][digit 0..4][lane][16] followed by the same with
    [digit 5, 6] --, params dict) that the library builds for the int8 scan from `table`, or (None, None) when the table has
    no image.  Needs no device."""
    t = _table_f32(table, int(resolution), int(m))
    tp = t.view(np.float32).ctypes.data_as(_f32p)
    n = lib().baz_music_debug_i8_image(int(m), int(resolution), tp, None, 0, None)
    if n == 0:
        return None, None
    img = np.zeros(n, np.uint8)
    par = np.zeros(16, np.float64)
    lib().baz_music_debug_i8_image(int(m), int(resolution), tp, img.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n,
                                   par.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return img, {"wt": par[:7].copy(), "sq": par[7], "t_acc": par[8], "e_bound": par[9], "e_refined": par[10],
                 "ns": int(par[11]), "nd": int(par[12]), "e4_bound": par[13], "t4": par[14]}


def smoothing_check(m, resolution, table, subarray, forward_backward=False):
    """HOST-ONLY: the structure checks of baz_music_set_smoothing on `table` (needs no device).  Returns the involution of the
    subarray's elements (uint8 array, the identity without FB) when the table passes, None when it does not."""
    t = _table_f32(table, int(resolution), int(m))
    perm = np.zeros(max(int(subarray), 1), np.uint8)
    r = lib().baz_music_smoothing_check(int(m), int(resolution), t.view(np.float32).ctypes.data_as(_f32p), int(subarray),
                                        1 if forward_backward else 0, perm.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return perm if r == OK else None


def order_estimate(m, nsnap, n_max, criterion, eigvals_ascending):
    """HOST-ONLY: the emitter counts the kernels' decision routine gives for rows of m ascending eigenvalues (needs no
    device).  criterion "mdl" / "aic"; returns a uint8 array, one count per row."""
    ev = np.ascontiguousarray(eigvals_ascending, dtype=np.float64).reshape(-1, int(m))
    out = np.zeros(max(ev.shape[0], 1), np.uint8)
    crit = ORDER_MODES.get(criterion, criterion) if not isinstance(criterion, int) else criterion
    r = lib().baz_music_order_estimate(int(m), int(nsnap), int(n_max), int(crit or 0),
                                       ev.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ev.shape[0],
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if r != OK:
        raise ValueError("baz_music_order_estimate: %s" % lib().baz_music_strerror(r).decode())
    return out[:ev.shape[0]].copy()


def averaging_weights(window, forgetting=1.0):
    """HOST-ONLY: (w[window], inv_norm[window + 1], n_eff) of baz_music_set_averaging(window, forgetting): the table the library
    hands its averaging kernel (needs no device).  inv_norm[c] normalises an item with c taps; inv_norm[0] is 0."""
    W = int(window)
    w = np.zeros(max(W, 1), np.float64)
    inv = np.zeros(max(W, 1) + 1, np.float64)
    ne = ctypes.c_double(0.0)
    dp = ctypes.POINTER(ctypes.c_double)
    r = lib().baz_music_averaging_weights(W, float(forgetting), w.ctypes.data_as(dp), inv.ctypes.data_as(dp), ctypes.byref(ne))
    if r != OK:
        raise ValueError("baz_music_averaging_weights: %s" % lib().baz_music_strerror(r).decode())
    return w[:W].copy(), inv[:W + 1].copy(), float(ne.value)


def power_estimate(R, a):
    """HOST-ONLY: the Capon powers 1 / Re(a^H R^-1 a) the library's definition gives for one covariance R (m x m complex) and the
    steering rows a (count x m complex64) (needs no device).  Returns a float64 array, one power per row."""
    R = np.ascontiguousarray(R, dtype=np.complex128)
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError("power_estimate: R must be a square matrix")
    m = R.shape[0]
    a = np.ascontiguousarray(a, dtype=np.complex64).reshape(-1, m) if m else np.zeros((0, 0), np.complex64)
    out = np.zeros(max(a.shape[0], 1), np.float64)
    r = lib().baz_music_power_estimate(m, R.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.shape[0],
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if r != OK:
        raise ValueError("baz_music_power_estimate: %s" % lib().baz_music_strerror(r).decode())
    return out[:a.shape[0]].copy()


def spectrum_estimate(kind, R, rows):
    """HOST-ONLY: the Capon (kind 1) or Bartlett (kind 2) spectrum values the library's definition gives for one covariance R
    (m x m complex) and the steering rows (count x m complex64) (needs no device).  Returns a float64 array, one value per row."""
    R = np.ascontiguousarray(R, dtype=np.complex128)
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError("spectrum_estimate: R must be a square matrix")
    m = R.shape[0]
    a = np.ascontiguousarray(rows, dtype=np.complex64).reshape(-1, m) if m else np.zeros((0, 0), np.complex64)
    out = np.zeros(max(a.shape[0], 1), np.float64)
    r = lib().baz_music_spectrum_estimate(int(kind), m, R.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                          a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.shape[0],
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if r != OK:
        raise ValueError("baz_music_spectrum_estimate: %s" % lib().baz_music_strerror(r).decode())
    return out[:a.shape[0]].copy()


def beam_weights(R, a, loading=0.0):
    """HOST-ONLY: the MVDR weights w = R_l^-1 a / (a^H R_l^-1 a) the library's definition gives for one covariance R (m x m complex),
    the steering rows a (count x m complex64) and the diagonal loading (needs no device).  Returns a complex128 array (count, m)."""
    R = np.ascontiguousarray(R, dtype=np.complex128)
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError("beam_weights: R must be a square matrix")
    m = R.shape[0]
    a = np.ascontiguousarray(a, dtype=np.complex64).reshape(-1, m) if m else np.zeros((0, 0), np.complex64)
    out = np.zeros((max(a.shape[0], 1), max(m, 1)), np.complex128)
    r = lib().baz_music_beam_weights(m, R.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                     a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.shape[0], float(loading),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if r != OK:
        raise ValueError("baz_music_beam_weights: %s" % lib().baz_music_strerror(r).decode())
    return out[:a.shape[0]].copy()


def calibration_apply(table, gamma):
    """HOST-ONLY: the calibrated table gamma_r * a_r(bin) the library's definition gives (resolution x m complex64; needs no device)."""
    t = np.ascontiguousarray(np.asarray(table, dtype=np.complex64))
    if t.ndim != 2:
        raise ValueError("calibration_apply: table must be resolution x m")
    g = np.ascontiguousarray(np.asarray(gamma, dtype=np.complex64).reshape(-1))
    if t.size and g.shape != (t.shape[1],):
        raise ValueError("calibration_apply: gamma must hold m = %d complex values" % t.shape[1])
    out = np.zeros(t.shape if t.size else (1, 1), np.complex64)
    r = lib().baz_music_calibration_apply(t.shape[1], t.shape[0], t.view(np.float32).ctypes.data_as(_f32p),
                                          g.view(np.float32).ctypes.data_as(_f32p), out.view(np.float32).ctypes.data_as(_f32p))
    if r != OK:
        raise ValueError("baz_music_calibration_apply: %s" % lib().baz_music_strerror(r).decode())
    return out


def whitening_factor(rn):
    """HOST-ONLY: W = L^-1 (m x m complex128, lower triangular, real positive diagonal) of the Cholesky factor rn = L L^H, by the
    routine set_noise_covariance runs; ValueError where the setter would refuse (a non-finite entry, a pivot at or below the floor)."""
    R = np.ascontiguousarray(rn, dtype=np.complex128)
    if R.ndim != 2 or R.shape[0] != R.shape[1] or R.shape[0] < 1:
        raise ValueError("whitening_factor: rn must be a square matrix")
    W = np.zeros_like(R)
    f64p = ctypes.POINTER(ctypes.c_double)
    r = lib().baz_music_whitening_factor(R.shape[0], R.view(np.float64).ctypes.data_as(f64p), W.view(np.float64).ctypes.data_as(f64p))
    if r != OK:
        raise ValueError("baz_music_whitening_factor: %s" % lib().baz_music_strerror(r).decode())
    return W


def whiten_table(table, w):
    """HOST-ONLY: the whitened table a'_r(bin) = fl32(sum_{k<=r} W_rk a_k(bin)) the library's definition gives (resolution x m
    complex64; the device kernel's own routine, bit for bit; needs no device)."""
    t = np.ascontiguousarray(np.asarray(table, dtype=np.complex64))
    if t.ndim != 2 or not t.size:
        raise ValueError("whiten_table: table must be resolution x m")
    W = np.ascontiguousarray(w, dtype=np.complex128)
    if W.shape != (t.shape[1], t.shape[1]):
        raise ValueError("whiten_table: w must be m x m = %d x %d" % (t.shape[1], t.shape[1]))
    out = np.zeros(t.shape, np.complex64)
    r = lib().baz_music_whiten_table(t.shape[1], t.shape[0], t.view(np.float32).ctypes.data_as(_f32p),
                                     W.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                     out.view(np.float32).ctypes.data_as(_f32p))
    if r != OK:
        raise ValueError("baz_music_whiten_table: %s" % lib().baz_music_strerror(r).decode())
    return out


def beamspace_apply(T, x, normalise=False):
    """HOST-ONLY: rows of m complex64 (`x`: (..., m); items and tables alike) -> rows of B complex64, y = fl32(T^H x) by the library's
    definition (the projection kernel's own routine, bit for bit; needs no device).  normalise: every row scaled to unit norm."""
    t = np.ascontiguousarray(np.asarray(T, dtype=np.complex128))
    if t.ndim != 2:
        raise ValueError("beamspace_apply: T must be m x B")
    v = np.ascontiguousarray(np.asarray(x, dtype=np.complex64))
    if v.ndim < 1 or v.shape[-1] != t.shape[0]:
        raise ValueError("beamspace_apply: the last axis of x must hold m = %d entries" % t.shape[0])
    cols = v.size // t.shape[0]
    out = np.zeros(v.shape[:-1] + (t.shape[1],), np.complex64)
    r = lib().baz_music_beamspace_apply(t.shape[0], t.shape[1], t.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        1 if normalise else 0, v.view(np.float32).ctypes.data_as(_f32p), cols,
                                        out.view(np.float32).ctypes.data_as(_f32p))
    if r != OK:
        raise ValueError("baz_music_beamspace_apply: %s" % lib().baz_music_strerror(r).decode())
    return out


def subband_twiddles(F, bins):
    """HOST-ONLY: the twiddles W (S x F complex128) of the subband mode for block length F and the DFT indices `bins`:
    W[s][t] = exp(-2 pi i ((k_s t) mod F) / F) / sqrt(F) by the library's definition; needs no device."""
    b = np.asarray(bins, dtype=np.int64).reshape(-1)
    if int(F) < 0 or int(F) > 0xffffffff or (b < 0).any() or (b > 0xffffffff).any():
        raise ValueError("subband_twiddles: negative argument")
    b = np.ascontiguousarray(b.astype(np.uint32))
    W = np.zeros((max(b.size, 1), max(int(F), 1)), np.complex128)
    r = lib().baz_music_subband_twiddles(int(F), b.size, b.ctypes.data_as(ctypes.POINTER(_u32)),
                                         W.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if r != OK:
        raise ValueError("baz_music_subband_twiddles: %s" % lib().baz_music_strerror(r).decode())
    return W


def subband_apply(W, x):
    """HOST-ONLY: the channeliser of the subband mode by the library's definition (the kernel's own routine, bit for bit; needs no
    device).  `W`: S x F complex128; `x`: (..., F, m) complex64, blocks of F snapshots of m antennas.  Returns (S, ..., m) complex64:
    y[s, ..., r] = fl32(sum_t W[s, t] x[..., t, r])."""
    w = np.ascontiguousarray(np.asarray(W, dtype=np.complex128))
    if w.ndim != 2:
        raise ValueError("subband_apply: W must be S x F")
    v = np.ascontiguousarray(np.asarray(x, dtype=np.complex64))
    if v.ndim < 2 or v.shape[-2] != w.shape[1]:
        raise ValueError("subband_apply: x must be (..., F, m) with F = %d" % w.shape[1])
    m = v.shape[-1]
    blocks = v.size // max(w.shape[1] * m, 1)
    out = np.zeros((w.shape[0],) + v.shape[:-2] + (m,), np.complex64)
    r = lib().baz_music_subband_apply(m, w.shape[1], w.shape[0], w.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                      v.view(np.float32).ctypes.data_as(_f32p), blocks, out.view(np.float32).ctypes.data_as(_f32p))
    if r != OK:
        raise ValueError("baz_music_subband_apply: %s" % lib().baz_music_strerror(r).decode())
    return out


def beamspace_design(table, bin_lo, bin_count, B):
    """HOST-ONLY: (T, captured) for the sector of `bin_count` bins from `bin_lo` (wrapping) of `table` (resolution x m): T (m x B
    complex128) = the B principal eigenvectors of sum a a^H over the sector, orthonormal; captured = their share of the trace."""
    t = np.ascontiguousarray(np.asarray(table, dtype=np.complex64))
    if t.ndim != 2 or not t.size:
        raise ValueError("beamspace_design: table must be resolution x m")
    if int(B) < 0 or int(bin_lo) < 0 or int(bin_count) < 0:
        raise ValueError("beamspace_design: negative argument")
    T, cap = np.zeros((t.shape[1], max(int(B), 1)), np.complex128), ctypes.c_double(0.0)
    r = lib().baz_music_beamspace_design(t.shape[1], t.shape[0], t.view(np.float32).ctypes.data_as(_f32p), int(bin_lo), int(bin_count),
                                         int(B), T.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(cap))
    if r != OK:
        raise ValueError("baz_music_beamspace_design: %s" % lib().baz_music_strerror(r).decode())
    return T, float(cap.value)


def calibration_estimate(rbar, ref):
    """HOST-ONLY: (gamma complex128[m], quality) the library's definition gives for a mean covariance Rbar (m x m complex) and the
    pilot's ideal response `ref` (m complex64); needs no device."""
    R = np.ascontiguousarray(rbar, dtype=np.complex128)
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError("calibration_estimate: Rbar must be a square matrix")
    m = R.shape[0]
    p = np.ascontiguousarray(np.asarray(ref, dtype=np.complex64).reshape(-1))
    if p.shape != (m,):
        raise ValueError("calibration_estimate: ref must hold m = %d complex values" % m)
    g, q = np.zeros(max(m, 1), np.complex128), ctypes.c_double(0.0)
    f64p = ctypes.POINTER(ctypes.c_double)
    r = lib().baz_music_calibration_estimate(m, R.view(np.float64).ctypes.data_as(f64p), p.view(np.float32).ctypes.data_as(_f32p),
                                             g.view(np.float64).ctypes.data_as(f64p), ctypes.byref(q))
    if r != OK:
        raise ValueError("baz_music_calibration_estimate: %s" % lib().baz_music_strerror(r).decode())
    return g[:m].copy(), float(q.value)


def refine_estimate(y3):
    """HOST-ONLY: the sub-bin offsets the kernel's decision routine gives for rows (d(b-1), d(b), d(b+1)) (needs no device).
    Returns a float64 array, one offset per row."""
    y = np.ascontiguousarray(y3, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(max(y.shape[0], 1), np.float64)
    r = lib().baz_music_refine_estimate(y.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), y.shape[0],
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if r != OK:
        raise ValueError("baz_music_refine_estimate: %s" % lib().baz_music_strerror(r).decode())
    return out[:y.shape[0]].copy()


TABLE_IMAGES = {0: "FB", 1: "TB", 2: "coarse", 3: "i8", 4: "a2p", 5: "TA", 6: "a2", 7: "params", 8: "i8 packed (m <= 4)"}


def debug_host_table_image(m, n, resolution, table, which, lab=None):
    """HOST-ONLY: image `which` of `table` as the round-4 host routines build it (uint8 array), or None.  Needs no device.
    lab=None: the lab form of the library where BAZ_MUSIC_LAB_LIB is set (like Context); image 8 -- the level-packed int8 operands of
    2 .. 4 antennas -- exists in the lab form only."""
    if lab is None:
        lab = bool(os.environ.get("BAZ_MUSIC_LAB_LIB"))
    t = _table_f32(table, int(resolution), int(m))
    tp = t.view(np.float32).ctypes.data_as(_f32p)
    L = lib(lab)
    nb = int(L.baz_music_debug_host_table_image(int(m), int(n), int(resolution), tp, int(which), None, 0))
    if nb == 0:
        return None
    out = np.zeros(nb, np.uint8)
    L.baz_music_debug_host_table_image(int(m), int(n), int(resolution), tp, int(which), _vp(out.ctypes.data), nb)
    return out


def guard_active(lab=True):
    """True when the (lab) library allocates with guard zones: lab build and BAZ_MUSIC_GUARD=1 in the environment at load time."""
    return bool(lib(lab).baz_music_debug_guard_active())


def guard_check(lab=True):
    """Guard zones found overwritten since the process started (lab library under BAZ_MUSIC_GUARD=1; synchronises the device); 0 otherwise."""
    return int(lib(lab).baz_music_debug_guard_check())


def live_buffers(lab=None):
    """(device, page-locked) allocations of the library that are live in this process (baz_music_debug_live_buffers).
    lab=None: the form of the library a Context() loads (the lab form where BAZ_MUSIC_LAB_LIB is set)."""
    if lab is None:
        lab = bool(os.environ.get("BAZ_MUSIC_LAB_LIB"))
    out = (ctypes.c_uint64 * 2)()
    lib(lab).baz_music_debug_live_buffers(out)
    return int(out[0]), int(out[1])


def q_stride(batch):
    return int(lib().baz_music_q_stride(int(batch)))


def device_count():
    """Usable gfx950 devices (0 on a CPU-only box)."""
    return int(lib().baz_music_device_count())


def version():
    return lib().baz_music_version().decode()
