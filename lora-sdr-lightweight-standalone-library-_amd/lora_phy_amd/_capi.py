"""ctypes binding of the C-ABI in include/lora_mi355x.h (liblora_mi355x.so).

The shared library is built in-tree (``make -C lora-sdr-lightweight-standalone-library-_amd``
or ``__graft_entry__.build()``) into ``lora_phy_amd/lib/``.  There is no CPU fallback:
if the library or a GPU is missing, the product API raises.
"""
from __future__ import annotations

import ctypes as C
import os

# LORA_MI355X_LIB: development A/B of an alternative in-tree build of the same library.
LIB_PATH = os.environ.get("LORA_MI355X_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                             "liblora_mi355x.so")

LORA_OK = 0
LORA_EIO = -5
LORA_ENOMEM = -12
LORA_EINVAL = -22
LORA_ERANGE = -34

LORA_WINDOW_NONE = 0
LORA_WINDOW_HANN = 1
LORA_MODE_LEGACY = 0
LORA_MODE_API = 1
LORA_MODE_RAW = 2
# raw sample formats of the banks' raw entries (int16, int8, uint8 I, Q pairs)
LORA_IQ_CS16 = 1
LORA_IQ_CS8 = 2
LORA_IQ_CU8 = 3

# lora_demod_last_kernels bits
KERNEL_BITS = {"frame_max": 1, "estimate": 2, "demod": 4, "generic": 16, "frame_max_wave": 32, "spec": 64}

# Every symbol include/lora_mi355x.h declares (checked by tests/test_capi_symbols.py).
EXPORTED_SYMBOLS = (
    "lora_demod_plan_create",
    "lora_demod_plan_destroy",
    "lora_demod_symbols_per_frame",
    "lora_demod_workspace_bytes",
    "lora_demod_batch",
    "lora_demod_metrics_batch",
    "lora_demod_soft_bits_batch",
    "lora_demod_soft_bits_frame_batch",
    "lora_detect_scan_windows",
    "lora_detect_scan_batch",
    "lora_find_frames_tile",
    "lora_find_frames_batch",
    "lora_find_candidates_batch",
    "lora_select_frames_batch",
    "lora_preamble_tables",
    "lora_detect_scan_acc_windows",
    "lora_detect_scan_acc_batch",
    "lora_find_preamble_batch",
    "lora_select_preamble_batch",
    "lora_channelize_outputs",
    "lora_channelize_batch",
    "lora_resample_outputs",
    "lora_resample_channelize_batch",
    "lora_channelize_raw_batch",
    "lora_resample_channelize_raw_batch",
    "lora_synthesize_outputs",
    "lora_synthesize_batch",
    "lora_synthesize_raw_batch",
    "lora_impair_batch",
    "lora_impair_raw_batch",
    "lora_propagate_batch",
    "lora_mod_batch",
    "lora_estimate_offsets_batch",
    "lora_compensate_offsets_batch",
    "lora_decode_batch",
    "lora_encode_batch",
    "lora_decode_chain_batch",
    "lora_decode_chain_soft_batch",
    "lora_encode_chain_batch",
    "lora_chain_symbols",
    "lora_frame_symbols",
    "lora_encode_frame_batch",
    "lora_decode_frame_batch",
    "lora_decode_frame_soft_batch",
    "lora_gather_frames_batch",
    "lora_demod_profile_enable",
    "lora_demod_profile_read",
    "lora_demod_last_kernels",
    "lora_demod_spec_recomputed",
    "lora_demod_spec_trace",
    "lora_demod_plan_set_pipeline",
    "lora_aql_last_profile",
    "lora_last_error",
    "lora_version",
)


class DemodParams(C.Structure):
    _fields_ = [
        ("sf", C.c_uint),
        ("osr", C.c_uint),
        ("bw_hz", C.c_uint),
        ("window", C.c_int),
        ("dechirp", C.c_int),
        ("mode", C.c_int),
        ("device", C.c_int),
        ("precision", C.c_int),
    ]


class DemodOutputs(C.Structure):
    _fields_ = [
        ("symbols", C.c_void_p),
        ("sym_stride", C.c_int64),
        ("sync", C.c_void_p),
        ("cfo", C.c_void_p),
        ("time_offset", C.c_void_p),
        ("max_amp", C.c_void_p),
    ]


class SymbolMetrics(C.Structure):
    """lora_symbol_metrics: the detector's per-symbol outputs (any pointer may be NULL)."""

    _fields_ = [
        ("power", C.c_void_p),
        ("power_avg", C.c_void_p),
        ("f_index", C.c_void_p),
        ("index", C.c_void_p),
        ("stride", C.c_int64),
    ]


class SpecTraceOut(C.Structure):
    """lora_spec_trace_out: the caller's host buffers of lora_demod_spec_trace."""

    _fields_ = [
        ("fp_spec", C.c_void_p),
        ("fp", C.c_void_p),
        ("max_slot", C.c_void_p),
        ("entries", C.c_void_p),
        ("list", C.c_void_p),
        ("frame_cap", C.c_int64),
        ("sym_cap", C.c_int64),
        ("list_cap", C.c_int64),
    ]


class FindParams(C.Structure):
    """lora_find_params: the frame finder's geometry, threshold and device."""

    _fields_ = [
        ("sf", C.c_uint),
        ("osr", C.c_uint),
        ("sync", C.c_uint),
        ("thresh_db", C.c_float),
        ("hop", C.c_int64),
        ("frame_symbols", C.c_int64),
        ("device", C.c_int),
    ]


class PreambleParams(C.Structure):
    """lora_preamble_params: the preamble finder's geometry, thresholds and device."""

    _fields_ = [
        ("sf", C.c_uint),
        ("osr", C.c_uint),
        ("hop", C.c_int64),
        ("acc_up", C.c_int),
        ("thresh_up_db", C.c_float),
        ("thresh_dn_db", C.c_float),
        ("max_cfo_bins", C.c_int),
        ("device", C.c_int),
    ]


# windows per tile of the finder kernel's pass (lora_find_frames_tile; tests/test_find_capi.py
# holds the two together)
FIND_TILE = 4096


class LoraError(RuntimeError):
    """Raised for negative return codes of the C-ABI (reference: -1 / 0 returns)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"{msg} (code {code})")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    """Load liblora_mi355x.so once; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()')")
    L = C.CDLL(LIB_PATH)
    L.lora_demod_plan_create.restype = C.c_int
    L.lora_demod_plan_create.argtypes = [C.POINTER(DemodParams), C.POINTER(C.c_void_p)]
    L.lora_demod_plan_destroy.restype = C.c_int
    L.lora_demod_plan_destroy.argtypes = [C.c_void_p]
    L.lora_demod_symbols_per_frame.restype = C.c_int64
    L.lora_demod_symbols_per_frame.argtypes = [C.c_void_p, C.c_int64]
    L.lora_demod_workspace_bytes.restype = C.c_size_t
    L.lora_demod_workspace_bytes.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.lora_demod_batch.restype = C.c_int64
    L.lora_demod_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                   C.POINTER(DemodOutputs), C.c_void_p, C.c_size_t, C.c_void_p]
    L.lora_demod_metrics_batch.restype = C.c_int64
    L.lora_demod_metrics_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SymbolMetrics),
                                           C.c_void_p]
    L.lora_demod_soft_bits_batch.restype = C.c_int64
    L.lora_demod_soft_bits_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_void_p]
    L.lora_demod_soft_bits_frame_batch.restype = C.c_int64
    L.lora_demod_soft_bits_frame_batch.argtypes = (L.lora_demod_soft_bits_batch.argtypes[:10] +
                                                   [C.c_int64, C.c_int64, C.c_void_p])
    L.lora_detect_scan_windows.restype = C.c_int64
    L.lora_detect_scan_windows.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.lora_detect_scan_batch.restype = C.c_int64
    L.lora_detect_scan_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                         C.POINTER(SymbolMetrics), C.c_void_p]
    # the frame finder (csrc/lora_find.hip)
    L.lora_find_frames_tile.restype = C.c_int64
    L.lora_find_frames_tile.argtypes = []
    L.lora_find_frames_batch.restype = C.c_int64
    L.lora_find_frames_batch.argtypes = [C.POINTER(FindParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    # the finder of self-describing frames: candidates listed, then selected by their headers
    L.lora_find_candidates_batch.restype = C.c_int64
    L.lora_find_candidates_batch.argtypes = [C.POINTER(FindParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
    L.lora_select_frames_batch.restype = C.c_int64
    L.lora_select_frames_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                           C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    # preambled frames: the tables (host arithmetic), the accumulating scan (csrc/lora_scan.hip),
    # the preamble finder and the selection with a tail and a carried word (csrc/lora_find.hip)
    L.lora_preamble_tables.restype = C.c_int64
    L.lora_preamble_tables.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_int64, C.c_void_p, C.c_void_p]
    L.lora_detect_scan_acc_windows.restype = C.c_int64
    L.lora_detect_scan_acc_windows.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    L.lora_detect_scan_acc_batch.restype = C.c_int64
    L.lora_detect_scan_acc_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                             C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_void_p]
    L.lora_find_preamble_batch.restype = C.c_int64
    L.lora_find_preamble_batch.argtypes = [C.POINTER(PreambleParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
    L.lora_select_preamble_batch.restype = C.c_int64
    L.lora_select_preamble_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                             C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p]
    # the down-converter bank (csrc/lora_channelize.hip)
    L.lora_channelize_outputs.restype = C.c_int64
    L.lora_channelize_outputs.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    L.lora_channelize_batch.restype = C.c_int64
    L.lora_channelize_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int32),
                                        C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    # the rational-rate bank (csrc/lora_resample.hip): interp goes before decim
    L.lora_resample_outputs.restype = C.c_int64
    L.lora_resample_outputs.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64]
    L.lora_resample_channelize_batch.restype = C.c_int64
    L.lora_resample_channelize_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                 C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                                 C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_void_p,
                                                 C.c_int64, C.c_int, C.c_void_p]
    # the raw entries: their float counterparts with (iq, format, scale) in place of iq
    L.lora_channelize_raw_batch.restype = C.c_int64
    L.lora_channelize_raw_batch.argtypes = [C.c_void_p, C.c_int, C.c_float] + L.lora_channelize_batch.argtypes[1:]
    L.lora_resample_channelize_raw_batch.restype = C.c_int64
    L.lora_resample_channelize_raw_batch.argtypes = ([C.c_void_p, C.c_int, C.c_float] +
                                                     L.lora_resample_channelize_batch.argtypes[1:])
    # the synthesis bank (csrc/lora_synth.hip): steps and gains are host arrays; the raw entry has
    # (out, format, inv_scale) in place of out
    L.lora_synthesize_outputs.restype = C.c_int64
    L.lora_synthesize_outputs.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    L.lora_synthesize_batch.restype = C.c_int64
    L.lora_synthesize_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_float), C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                        C.c_void_p]
    L.lora_synthesize_raw_batch.restype = C.c_int64
    L.lora_synthesize_raw_batch.argtypes = (L.lora_synthesize_batch.argtypes[:14] + [C.c_int, C.c_float] +
                                            L.lora_synthesize_batch.argtypes[14:])
    # the channel impairment stage (csrc/lora_impair.hip): gain, fcw, phase and sigma are device
    # arrays (any may be NULL); the raw entry has (out, format, inv_scale) in place of out
    L.lora_impair_batch.restype = C.c_int64
    L.lora_impair_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint64,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                    C.c_void_p]
    L.lora_impair_raw_batch.restype = C.c_int64
    L.lora_impair_raw_batch.argtypes = (L.lora_impair_batch.argtypes[:12] + [C.c_int, C.c_float] +
                                        L.lora_impair_batch.argtypes[12:])
    # the propagation stage (csrc/lora_propagate.hip): delay, gain, sfo, table, fcw, rate and phase
    # are device arrays (sfo, fcw, rate and phase may be NULL)
    L.lora_propagate_batch.restype = C.c_int64
    L.lora_propagate_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                       C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                       C.c_void_p]
    L.lora_mod_batch.restype = C.c_int64
    L.lora_mod_batch.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_uint8, C.c_void_p,
                                 C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.lora_estimate_offsets_batch.restype = C.c_int64
    L.lora_estimate_offsets_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lora_compensate_offsets_batch.restype = C.c_int64
    L.lora_compensate_offsets_batch.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_int64,
                                                C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_void_p, C.c_void_p]
    # the payload codec (csrc/lora_codec.hip)
    L.lora_decode_batch.restype = C.c_int64
    L.lora_decode_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.lora_encode_batch.restype = C.c_int64
    L.lora_encode_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                    C.c_int64, C.c_int, C.c_void_p]
    L.lora_decode_chain_batch.restype = C.c_int64
    L.lora_decode_chain_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.lora_decode_chain_soft_batch.restype = C.c_int64
    L.lora_decode_chain_soft_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.lora_encode_chain_batch.restype = C.c_int64
    L.lora_encode_chain_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.lora_chain_symbols.restype = C.c_int64
    L.lora_chain_symbols.argtypes = [C.c_int, C.c_int, C.c_int64]
    # self-describing frames (csrc/lora_codec.hip) and the frame gather (csrc/lora_gather.hip)
    L.lora_frame_symbols.restype = C.c_int64
    L.lora_frame_symbols.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int]
    L.lora_encode_frame_batch.restype = C.c_int64
    L.lora_encode_frame_batch.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.lora_decode_frame_batch.restype = C.c_int64
    L.lora_decode_frame_batch.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    # (llr for symbols; corrected, hdr_flips and max_flips for errors)
    L.lora_decode_frame_soft_batch.restype = C.c_int64
    L.lora_decode_frame_soft_batch.argtypes = (L.lora_decode_frame_batch.argtypes[:12] + [C.c_void_p, C.c_int] +
                                               L.lora_decode_frame_batch.argtypes[12:])
    L.lora_gather_frames_batch.restype = C.c_int64
    L.lora_gather_frames_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.lora_demod_profile_enable.restype = C.c_int
    L.lora_demod_profile_enable.argtypes = [C.c_void_p, C.c_int]
    L.lora_demod_profile_read.restype = C.c_int
    L.lora_demod_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.lora_demod_last_kernels.restype = C.c_int
    L.lora_demod_last_kernels.argtypes = [C.c_void_p]
    L.lora_demod_spec_recomputed.restype = C.c_int64
    L.lora_demod_spec_recomputed.argtypes = [C.c_void_p]
    L.lora_demod_spec_trace.restype = C.c_int64
    L.lora_demod_spec_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64,
                                        C.POINTER(SpecTraceOut), C.c_void_p]
    L.lora_demod_plan_set_pipeline.restype = C.c_int
    L.lora_demod_plan_set_pipeline.argtypes = [C.c_void_p, C.c_int]
    L.lora_aql_last_profile.restype = C.c_int
    L.lora_aql_last_profile.argtypes = [C.POINTER(C.c_double), C.c_int]
    L.lora_last_error.restype = C.c_char_p
    L.lora_version.restype = C.c_char_p
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        msg = lib().lora_last_error().decode(errors="replace")
        raise LoraError(int(rc), msg or "lora_mi355x error")
    return int(rc)
