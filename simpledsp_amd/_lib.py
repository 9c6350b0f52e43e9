"""ctypes binding of libsdsp_hip.so -- the C ABI declared in include/sdsp_hip.h.

The library is the product: if it cannot be loaded this module raises.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / "lib" / "libsdsp_hip.so"

F32, F64 = 0, 1
F32_F64STATE = 2  # IIR banks: float samples, double state / recurrence
FORWARD, REVERSE = 1, -1
FILTER_NONE, FILTER_LOW_PASS, FILTER_HIGH_PASS, FILTER_BAND_PASS = 0, 1, 2, 3
FILTER_BAND_STOP = 4
IIR_GENERIC, IIR_LP, IIR_HP, IIR_BP = 0, 1, 2, 3
MAX_SECTIONS = 16

OK, ERR_INVALID_SIZE, ERR_UNSUPPORTED, ERR_HIP, ERR_NO_DEVICE, ERR_INVALID_ARG, ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6


class SdspHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"sdsp_hip error {code}: {message}")
        self.code = code
        self.message = message


class PlanInfo(C.Structure):
    _fields_ = [
        ("n", C.c_uint32), ("radix", C.c_int), ("direction", C.c_int), ("precision", C.c_int),
        ("device", C.c_int), ("hbm_passes", C.c_int), ("algorithmic_bytes", C.c_uint64),
        ("workspace_bytes", C.c_uint64), ("twiddle_bytes", C.c_uint64), ("kernel", C.c_char * 64),
        ("stage_radix", C.c_int),
    ]


class FftColsPlanInfo(C.Structure):
    _fields_ = [
        ("n", C.c_uint32), ("width", C.c_uint64), ("direction", C.c_int), ("precision", C.c_int), ("output", C.c_int),
        ("shift", C.c_int), ("windowed", C.c_int), ("device", C.c_int), ("variant", C.c_int), ("tile_columns", C.c_uint32),
        ("threads", C.c_uint32), ("lds_bytes", C.c_uint32), ("algorithmic_bytes", C.c_uint64), ("kernel", C.c_char * 64),
    ]


FFT_COLS_COMPLEX, FFT_COLS_POWER = 0, 1
FFT_COLS_MIN_N, FFT_COLS_MAX_N = 8, 1024


class FirPlanInfo(C.Structure):
    _fields_ = [
        ("taps", C.c_uint32), ("precision", C.c_int), ("device", C.c_int), ("method", C.c_int),
        ("fft_n", C.c_uint32), ("hop", C.c_uint32), ("workspace_bytes", C.c_uint64), ("kernel", C.c_char * 64),
    ]


FIR_DIRECT, FIR_FFT = 0, 1


class ResamplePlanInfo(C.Structure):
    _fields_ = [
        ("taps", C.c_uint32), ("up", C.c_uint32), ("down", C.c_uint32), ("hist", C.c_uint32), ("precision", C.c_int),
        ("device", C.c_int), ("kernel", C.c_char * 64),
    ]


RESAMPLE_MAX_FACTOR = 1024


class StftPlanInfo(C.Structure):
    _fields_ = [
        ("n_fft", C.c_uint32), ("hop", C.c_uint32), ("bins", C.c_uint32), ("hist", C.c_uint32), ("output", C.c_int),
        ("precision", C.c_int), ("device", C.c_int), ("workspace_bytes", C.c_uint64), ("kernel", C.c_char * 64),
    ]


STFT_COMPLEX, STFT_POWER, STFT_MAGNITUDE = 0, 1, 2
WINDOW_RECT, WINDOW_HANN, WINDOW_HAMMING, WINDOW_BLACKMAN = 0, 1, 2, 3


class IstftPlanInfo(C.Structure):
    _fields_ = [
        ("n_fft", C.c_uint32), ("hop", C.c_uint32), ("bins", C.c_uint32), ("hist", C.c_uint32), ("norm", C.c_int),
        ("precision", C.c_int), ("device", C.c_int), ("workspace_bytes", C.c_uint64), ("kernel", C.c_char * 64),
        ("env_min", C.c_double), ("env_max", C.c_double),
    ]


ISTFT_NORMALIZED, ISTFT_RAW = 0, 1


class FiltfiltPlanInfo(C.Structure):
    _fields_ = [
        ("sections", C.c_uint32), ("padlen", C.c_uint32), ("kind", C.c_int), ("padtype", C.c_int), ("precision", C.c_int),
        ("device", C.c_int), ("variant", C.c_int), ("workspace_bytes", C.c_uint64), ("slice_channels", C.c_uint64),
        ("kernel", C.c_char * 64),
    ]


PAD_NONE, PAD_ODD, PAD_EVEN, PAD_CONSTANT = 0, 1, 2, 3


class WelchPlanInfo(C.Structure):
    _fields_ = [
        ("n_fft", C.c_uint32), ("hop", C.c_uint32), ("bins", C.c_uint32), ("hist", C.c_uint32), ("detrend", C.c_int),
        ("scaling", C.c_int), ("fs", C.c_double), ("precision", C.c_int), ("device", C.c_int), ("workspace_bytes", C.c_uint64),
        ("kernel", C.c_char * 64),
    ]


class CsdPlanInfo(C.Structure):
    _fields_ = [
        ("n_fft", C.c_uint32), ("hop", C.c_uint32), ("bins", C.c_uint32), ("hist", C.c_uint32), ("detrend", C.c_int),
        ("scaling", C.c_int), ("fs", C.c_double), ("precision", C.c_int), ("device", C.c_int), ("channels", C.c_uint64),
        ("npairs", C.c_uint64), ("column_bytes", C.c_uint64), ("slice_columns", C.c_uint64), ("workspace_bytes", C.c_uint64),
        ("kernel", C.c_char * 64),
    ]


class PfbPlanInfo(C.Structure):
    _fields_ = [
        ("channels_m", C.c_uint32), ("taps_per_channel", C.c_uint32), ("hop", C.c_uint32), ("bins", C.c_uint32), ("hist", C.c_uint32),
        ("input_kind", C.c_int), ("phase", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("workspace_bytes", C.c_uint64),
        ("kernel", C.c_char * 64), ("fold", C.c_char * 16),
    ]


class PfbSynthPlanInfo(C.Structure):
    _fields_ = [
        ("channels_m", C.c_uint32), ("taps_per_channel", C.c_uint32), ("hop", C.c_uint32), ("bins", C.c_uint32), ("hist", C.c_uint32),
        ("output_kind", C.c_int), ("phase", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("workspace_bytes", C.c_uint64),
        ("kernel", C.c_char * 64), ("unfold", C.c_char * 16),
    ]


class DdcBand(C.Structure):
    _fields_ = [("src", C.c_uint32), ("fcw", C.c_uint32), ("phase0", C.c_uint32)]


class DdcPlanInfo(C.Structure):
    _fields_ = [
        ("taps", C.c_uint32), ("down", C.c_uint32), ("channels", C.c_uint32), ("bands", C.c_uint32), ("hist", C.c_uint32),
        ("block_out", C.c_uint32), ("input_kind", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("kernel", C.c_char * 64),
    ]


class DucBand(C.Structure):
    _fields_ = [("dst", C.c_uint32), ("fcw", C.c_uint32), ("phase0", C.c_uint32)]


class DucPlanInfo(C.Structure):
    _fields_ = [
        ("taps", C.c_uint32), ("up", C.c_uint32), ("channels", C.c_uint32), ("bands", C.c_uint32), ("hist", C.c_uint32),
        ("block_in", C.c_uint32), ("output_kind", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("kernel", C.c_char * 64),
    ]


class ArbPlanInfo(C.Structure):
    _fields_ = [
        ("phases", C.c_uint32), ("taps", C.c_uint32), ("hist", C.c_uint32), ("block_out", C.c_uint32), ("max_step", C.c_uint64),
        ("input_kind", C.c_int), ("interp", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("kernel", C.c_char * 64),
    ]


class CicPlanInfo(C.Structure):
    _fields_ = [
        ("order", C.c_uint32), ("down", C.c_uint32), ("delay", C.c_uint32), ("hist", C.c_uint32), ("in_bits", C.c_uint32),
        ("growth", C.c_uint32), ("reg_bits", C.c_uint32), ("chunk", C.c_uint32), ("segment", C.c_uint32), ("in_type", C.c_int),
        ("input_kind", C.c_int), ("out_kind", C.c_int), ("device", C.c_int), ("scale", C.c_double), ("kernel", C.c_char * 64),
    ]


class CicInterpPlanInfo(C.Structure):
    _fields_ = [
        ("order", C.c_uint32), ("up", C.c_uint32), ("delay", C.c_uint32), ("hist", C.c_uint32), ("in_bits", C.c_uint32),
        ("growth", C.c_uint32), ("reg_bits", C.c_uint32), ("chunk", C.c_uint32), ("segment", C.c_uint32), ("in_type", C.c_int),
        ("input_kind", C.c_int), ("out_kind", C.c_int), ("device", C.c_int), ("scale", C.c_double), ("kernel", C.c_char * 64),
    ]


class BeamEntry(C.Structure):
    _fields_ = [("beam", C.c_uint32), ("sensor", C.c_uint32), ("delay", C.c_uint32)]


class BeamPlanInfo(C.Structure):
    _fields_ = [
        ("sensors", C.c_uint32), ("beams", C.c_uint32), ("groups", C.c_uint32), ("taps", C.c_uint32), ("entries", C.c_uint32),
        ("max_delay", C.c_uint32), ("hist", C.c_uint32), ("block_out", C.c_uint32), ("chunks", C.c_uint32), ("max_spread", C.c_uint32),
        ("lds_line_bytes", C.c_uint32), ("kind", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("variant", C.c_int),
        ("kernel", C.c_char * 64),
    ]


class LmsPlanInfo(C.Structure):
    _fields_ = [
        ("channels", C.c_uint64), ("taps", C.c_uint32), ("block", C.c_uint32), ("lds_bytes", C.c_uint32), ("eps", C.c_double),
        ("kind", C.c_int), ("precision", C.c_int), ("mode", C.c_int), ("device", C.c_int), ("variant", C.c_int),
        ("kernel", C.c_char * 64),
    ]


class RankPlanInfo(C.Structure):
    _fields_ = [
        ("channels", C.c_uint64), ("window", C.c_uint32), ("rank", C.c_uint32), ("padded", C.c_uint32), ("out_index", C.c_uint32),
        ("run", C.c_uint32), ("last_run", C.c_uint32), ("block", C.c_uint32), ("lds_bytes", C.c_uint32), ("departing", C.c_int),
        ("precision", C.c_int), ("device", C.c_int), ("variant", C.c_int), ("kernel", C.c_char * 64),
    ]


class CfarDesc(C.Structure):
    _fields_ = [
        ("train", C.c_uint32), ("guard", C.c_uint32), ("mode", C.c_int), ("rank", C.c_uint32), ("input", C.c_int), ("alpha", C.c_double),
    ]


class CfarPlanInfo(C.Structure):
    _fields_ = [
        ("channels", C.c_uint64), ("train", C.c_uint32), ("guard", C.c_uint32), ("half", C.c_uint32), ("window", C.c_uint32),
        ("lag_shift", C.c_uint32), ("rank", C.c_uint32), ("padded", C.c_uint32), ("run", C.c_uint32), ("last_run", C.c_uint32),
        ("block", C.c_uint32), ("lds_bytes", C.c_uint32), ("alpha", C.c_double), ("scale", C.c_double), ("mode", C.c_int),
        ("input", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("variant", C.c_int), ("kernel", C.c_char * 64),
    ]


class Cfar2dDesc(C.Structure):
    _fields_ = [
        ("train_d", C.c_uint32), ("guard_d", C.c_uint32), ("train_r", C.c_uint32), ("guard_r", C.c_uint32), ("edge", C.c_int),
        ("peak", C.c_int), ("alpha", C.c_double),
    ]


class Cfar2dPlanInfo(C.Structure):
    _fields_ = [
        ("D", C.c_uint32), ("R", C.c_uint32), ("max_maps", C.c_uint64), ("train_d", C.c_uint32), ("guard_d", C.c_uint32),
        ("train_r", C.c_uint32), ("guard_r", C.c_uint32), ("cells", C.c_uint32), ("edge", C.c_int), ("peak", C.c_int),
        ("tabled", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("variant", C.c_int), ("alpha", C.c_double),
        ("tile_rows", C.c_uint32), ("tile_cols", C.c_uint32), ("threads", C.c_uint32), ("lds_bytes", C.c_uint32),
        ("workspace_bytes", C.c_uint64), ("kernel", C.c_char * 64),
    ]


class PllPlanInfo(C.Structure):
    _fields_ = [
        ("channels", C.c_uint64), ("block", C.c_uint32), ("waves", C.c_uint32), ("lds_bytes", C.c_uint32), ("max_dev", C.c_double),
        ("precision", C.c_int), ("mode", C.c_int), ("device", C.c_int), ("variant", C.c_int), ("kernel", C.c_char * 64),
    ]


class TimingPlanInfo(C.Structure):
    _fields_ = [
        ("channels", C.c_uint64), ("step0", C.c_uint64), ("phases", C.c_uint32), ("taps", C.c_uint32), ("block", C.c_uint32),
        ("waves", C.c_uint32), ("lds_bytes", C.c_uint32), ("max_dev", C.c_double),
        ("precision", C.c_int), ("mode", C.c_int), ("device", C.c_int), ("variant", C.c_int), ("kernel", C.c_char * 64),
    ]


class ViterbiPlanInfo(C.Structure):
    _fields_ = [
        ("k", C.c_uint32), ("n", C.c_uint32), ("generators", C.c_uint32 * 3), ("states", C.c_uint32), ("block", C.c_uint32),
        ("depth", C.c_uint32), ("delay", C.c_uint32), ("chunk", C.c_uint32), ("threads", C.c_uint32), ("waves", C.c_uint32),
        ("lds_bytes", C.c_uint32), ("ring_in_lds", C.c_uint32), ("max_channels", C.c_uint64), ("state_bytes", C.c_uint64),
        ("scale", C.c_float), ("in_kind", C.c_int), ("out_kind", C.c_int), ("device", C.c_int), ("variant", C.c_int),
        ("kernel", C.c_char * 64),
    ]


class RsPlanInfo(C.Structure):
    _fields_ = [
        ("field_poly", C.c_uint32), ("fcr", C.c_uint32), ("prim", C.c_uint32), ("nroots", C.c_uint32), ("n", C.c_uint32),
        ("interleave", C.c_uint32), ("k", C.c_uint32), ("t", C.c_uint32), ("threads", C.c_uint32), ("waves", C.c_uint32),
        ("lds_bytes", C.c_uint32), ("out_kind", C.c_int), ("device", C.c_int), ("variant", C.c_int), ("kernel", C.c_char * 64),
    ]


class FsyncPlanInfo(C.Structure):
    _fields_ = [
        ("marker", C.c_uint64), ("marker_bits", C.c_uint32), ("payload_bytes", C.c_uint32), ("period", C.c_uint32), ("tol", C.c_uint32),
        ("verify", C.c_uint32), ("flywheel", C.c_uint32), ("ring_words", C.c_uint32), ("row_words", C.c_uint32), ("has_pn", C.c_uint32),
        ("max_channels", C.c_uint64), ("max_bits", C.c_uint64), ("max_frames", C.c_uint64), ("state_bytes", C.c_uint64),
        ("workspace_bytes", C.c_uint64), ("polarity", C.c_int), ("in_kind", C.c_int), ("device", C.c_int), ("variant", C.c_int),
        ("kernel", C.c_char * 64),
    ]


class LdpcPlanInfo(C.Structure):
    _fields_ = [
        ("mb", C.c_uint32), ("nb", C.c_uint32), ("z", C.c_uint32), ("n", C.c_uint32), ("m", C.c_uint32), ("edges", C.c_uint32),
        ("max_row_degree", C.c_uint32), ("norm", C.c_uint32), ("beta", C.c_uint32), ("out_bits", C.c_uint32), ("group", C.c_uint32),
        ("threads", C.c_uint32), ("lds_bytes", C.c_uint32), ("codewords_per_cu", C.c_uint32), ("piece", C.c_uint64),
        ("workspace_bytes", C.c_uint64), ("scale", C.c_float), ("early_stop", C.c_int), ("in_kind", C.c_int), ("out_kind", C.c_int),
        ("device", C.c_int), ("variant", C.c_int), ("kernel", C.c_char * 64),
    ]


TIMING_GARDNER, TIMING_ZC_QPSK, TIMING_ZC_BPSK = 0, 1, 2
LDPC_I8, LDPC_F32 = 0, 1
LDPC_BYTES, LDPC_PACKED = 0, 1
LDPC_MAX_Z, LDPC_MAX_MB, LDPC_MAX_NB, LDPC_MAX_N, LDPC_MAX_ROW_DEGREE, LDPC_MAX_ITER = 512, 64, 128, 16384, 32, 255
FSYNC_BYTES, FSYNC_PACKED = 0, 1
FSYNC_NORMAL, FSYNC_EITHER = 0, 1
FSYNC_SEARCH, FSYNC_VERIFY, FSYNC_LOCK = 0, 1, 2
FSYNC_MAX_PAYLOAD, FSYNC_CCSDS_ASM = 8192, 0x1ACFFC1D
RS_FULL, RS_DATA = 0, 1
RS_MAX_NROOTS, RS_MAX_INTERLEAVE = 64, 16
VITERBI_I8, VITERBI_F32 = 0, 1
VITERBI_BYTES, VITERBI_PACKED = 0, 1
VITERBI_MIN_K, VITERBI_MAX_K, VITERBI_MAX_BLOCK, VITERBI_MAX_DEPTH, VITERBI_START_METRIC = 3, 9, 1024, 4096, -(1 << 20)
TIMING_MAX_PHASES, TIMING_MAX_TAPS, TIMING_MAX_TABLE = 128, 64, 4096
PLL_CROSS, PLL_BPSK, PLL_QPSK = 0, 1, 2
CFAR_CA, CFAR_GO, CFAR_SO, CFAR_OS = 0, 1, 2, 3
CFAR_POWER, CFAR_IQ = 0, 1
CFAR_MAX_TRAIN, CFAR_MAX_GUARD = 128, 255
CFAR2D_EDGE_MARK, CFAR2D_EDGE_CLIP = 0, 1
CFAR2D_MAX_R, CFAR2D_MAX_TRAIN_D, CFAR2D_MAX_GUARD_D, CFAR2D_MAX_D = 64, 32, 16, 1 << 20
CIC_REAL, CIC_COMPLEX = 0, 1
CIC_I16, CIC_I32 = 0, 1
CIC_OUT_INT, CIC_OUT_F32 = 0, 1
CIC_MAX_ORDER, CIC_MAX_DOWN, CIC_MAX_HISTORY = 8, 16384, 65536
ARB_REAL, ARB_COMPLEX = 0, 1
ARB_NEAREST, ARB_LINEAR = 0, 1
ARB_MAX_PHASES, ARB_MIN_STEP, ARB_MAX_STEP = 1024, 1 << 22, 1 << 42
DDC_REAL, DDC_COMPLEX = 0, 1
DDC_MAX_BANDS = 65536
DUC_REAL, DUC_COMPLEX = 0, 1
DUC_MAX_BANDS = 65536
BEAM_REAL, BEAM_COMPLEX = 0, 1
BEAM_MAX_TAPS, BEAM_MAX_DELAY, BEAM_MAX_ROWS, BEAM_MAX_ENTRIES = 256, 65535, 4096, 1 << 20
LMS_REAL, LMS_COMPLEX = 0, 1
LMS_LMS, LMS_NLMS = 0, 1
LMS_MAX_TAPS, LMS_MAX_TAPS_F64_COMPLEX = 64, 32
RANK_MAX_WINDOW, RANK_MAX_WINDOW_F64 = 255, 127
PFB_REAL, PFB_COMPLEX = 0, 1
PFB_PHASE_FRAME, PFB_PHASE_TIME = 0, 1
PFB_MAX_TAPS_PER_CHANNEL, PFB_MAX_TAPS = 64, 1 << 20

DETREND_NONE, DETREND_CONSTANT, DETREND_LINEAR = 0, 1, 2
SCALING_DENSITY, SCALING_SPECTRUM = 0, 1
CSD_CROSS, CSD_COHERENCE = 0, 1


# name -> (restype, argtypes); every symbol include/sdsp_hip.h declares
_vp, _u32, _u64, _i, _d, _sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double, C.c_size_t
_pp = C.POINTER(C.c_void_p)
SIGNATURES = {
    "sdsp_hip_last_error_string": (C.c_char_p, []),
    "sdsp_hip_version": (C.c_char_p, []),
    "sdsp_hip_device_count": (_i, [C.POINTER(_i)]),
    "sdsp_hip_malloc": (_i, [_pp, _sz, _i]),
    "sdsp_hip_free": (_i, [_vp, _i]),
    "sdsp_hip_memcpy_h2d": (_i, [_vp, _vp, _sz, _i]),
    "sdsp_hip_memcpy_d2h": (_i, [_vp, _vp, _sz, _i]),
    "sdsp_hip_device_synchronize": (_i, [_i]),
    "sdsp_hip_log2": (C.c_uint, [C.c_uint]),
    "sdsp_hip_log4": (C.c_uint, [C.c_uint]),
    "sdsp_hip_is_power_of_2": (_i, [C.c_uint]),
    "sdsp_hip_is_power_of_4": (_i, [C.c_uint]),
    "sdsp_hip_digit_reverse": (C.c_uint, [C.c_uint, C.c_uint, C.c_uint]),
    "sdsp_hip_calc_twiddles": (_i, [C.c_uint, _i, _vp]),
    "sdsp_hip_fft_plan_create": (_i, [_pp, _u32, _i, _i, _i, _u64, _i]),
    "sdsp_hip_rfft_plan_create": (_i, [_pp, _u32, _i, _i, _u64, _i]),
    "sdsp_hip_rfft_plan_create_p": (_i, [_pp, _u32, _i, _i, _i, _u64, _i]),
    "sdsp_hip_fft_plan_destroy": (_i, [_vp]),
    "sdsp_hip_fft_exec": (_i, [_vp, _vp, _u64, _vp]),
    "sdsp_hip_fft_exec_host": (_i, [_vp, _vp, _u64]),
    "sdsp_hip_fft_exec_sharded": (_i, [_pp, _i, _vp, _u64]),
    "sdsp_hip_fft_convolve": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "sdsp_hip_fft_plan_get_info": (_i, [_vp, C.POINTER(PlanInfo)]),
    "sdsp_hip_fft_plan_get_twiddles": (_i, [_vp, _vp]),
    "sdsp_hip_fft_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_fft_plan_status": (_i, [_vp]),
    "sdsp_hip_fft_plan_set_wait_limit": (_i, [_vp, _u64]),
    "sdsp_hip_fft_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_fft_cols_plan_create": (_i, [_pp, _u32, _u64, _i, _i, _i, _i, _vp, _i]),
    "sdsp_hip_fft_cols_plan_destroy": (_i, [_vp]),
    "sdsp_hip_fft_cols_exec": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "sdsp_hip_fft_cols_exec_host": (_i, [_vp, _vp, _vp, _u64]),
    "sdsp_hip_fft_cols_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_fft_cols_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_fft_cols_plan_get_info": (_i, [_vp, C.POINTER(FftColsPlanInfo)]),
    "sdsp_hip_set_launch_piece_bytes": (_i, [_u64]),
    "sdsp_hip_get_launch_piece_bytes": (_i, [C.POINTER(_u64)]),
    "sdsp_hip_iir_design_lp": (_i, [_u32, _d, _d, _d, _vp, _vp, C.POINTER(_d)]),
    "sdsp_hip_iir_design_hp": (_i, [_u32, _d, _d, _d, _vp, _vp, C.POINTER(_d)]),
    "sdsp_hip_iir_design_bp": (_i, [_u32, _d, _d, _d, _d, _vp, _vp, C.POINTER(_d)]),
    "sdsp_hip_iir_design_bs": (_i, [_u32, _d, _d, _d, _d, _vp, _vp, C.POINTER(_d)]),
    "sdsp_hip_iir_preload": (_i, [_u32, _i, _vp, _vp, _d, _d, _vp]),
    "sdsp_hip_iir_plan_create": (_i, [_pp, _u32, _i, _vp, _vp, _d, _i, _i]),
    "sdsp_hip_iir_plan_destroy": (_i, [_vp]),
    "sdsp_hip_iir_process": (_i, [_vp, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_iir_process_interleaved": (_i, [_vp, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_iir_process_host": (_i, [_vp, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_iir_process_sharded": (_i, [_pp, _i, _vp, _u64, _u64]),
    "sdsp_hip_iir_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_iir_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_iir_plan_kernel": (_i, [_vp, _vp, _u64, _u64, _u64, C.c_char_p, _sz]),
    "sdsp_hip_fir_design": (_i, [_u32, _i, _d, _d, _d, _d, _vp]),
    "sdsp_hip_fir_plan_create": (_i, [_pp, _u32, _vp, _i, _i]),
    "sdsp_hip_fir_plan_destroy": (_i, [_vp]),
    "sdsp_hip_fir_process": (_i, [_vp, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_fir_process_host": (_i, [_vp, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_fir_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_fir_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_fir_fft_size": (_i, [_u32, _i, C.POINTER(_u32)]),
    "sdsp_hip_fir_fft_plan_create": (_i, [_pp, _u32, _vp, _i, _u32, _u64, _i]),
    "sdsp_hip_fir_plan_get_info": (_i, [_vp, C.POINTER(FirPlanInfo)]),
    "sdsp_hip_fir_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_resample_design": (_i, [_u32, _u32, _u32, _vp]),
    "sdsp_hip_resample_out_samples": (_i, [_u32, _u32, _u64, C.POINTER(_u64)]),
    "sdsp_hip_resample_plan_create": (_i, [_pp, _u32, _vp, _u32, _u32, _i, _i]),
    "sdsp_hip_resample_plan_destroy": (_i, [_vp]),
    "sdsp_hip_resample_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_resample_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_resample_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_resample_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_resample_plan_get_info": (_i, [_vp, C.POINTER(ResamplePlanInfo)]),
    "sdsp_hip_stft_window": (_i, [_i, _u32, _vp]),
    "sdsp_hip_stft_frames": (_i, [_u32, _u64, C.POINTER(_u64)]),
    "sdsp_hip_stft_plan_create": (_i, [_pp, _u32, _u32, _vp, _i, _i, _u64, _i]),
    "sdsp_hip_stft_plan_destroy": (_i, [_vp]),
    "sdsp_hip_stft_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_stft_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_stft_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_stft_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_stft_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_stft_plan_get_info": (_i, [_vp, C.POINTER(StftPlanInfo)]),
    "sdsp_hip_istft_synthesis_window": (_i, [_u32, _u32, _vp, _i, _vp]),
    "sdsp_hip_istft_plan_create": (_i, [_pp, _u32, _u32, _vp, _i, _i, _u64, _i]),
    "sdsp_hip_istft_plan_destroy": (_i, [_vp]),
    "sdsp_hip_istft_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_istft_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_istft_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_istft_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_istft_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_istft_plan_get_info": (_i, [_vp, C.POINTER(IstftPlanInfo)]),
    "sdsp_hip_iir_steady_state": (_i, [_u32, _i, _vp, _vp, _d, _vp]),
    "sdsp_hip_filtfilt_default_padlen": (_i, [_u32, _i, _vp, _vp, C.POINTER(_u32)]),
    "sdsp_hip_filtfilt_plan_create": (_i, [_pp, _u32, _i, _vp, _vp, _d, _i, _i, C.c_int64, _u64, _i]),
    "sdsp_hip_filtfilt_plan_destroy": (_i, [_vp]),
    "sdsp_hip_filtfilt_process": (_i, [_vp, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_filtfilt_process_host": (_i, [_vp, _vp, _u64, _u64, _u64]),
    "sdsp_hip_filtfilt_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_filtfilt_plan_kernel": (_i, [_vp, _vp, _u64, _u64, _u64, C.c_char_p, _sz]),
    "sdsp_hip_filtfilt_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_filtfilt_plan_get_info": (_i, [_vp, C.POINTER(FiltfiltPlanInfo)]),
    "sdsp_hip_welch_frames": (_i, [_u32, _u32, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_welch_plan_create": (_i, [_pp, _u32, _u32, _vp, _i, _i, _d, _i, _u64, _i]),
    "sdsp_hip_welch_plan_destroy": (_i, [_vp]),
    "sdsp_hip_welch_process": (_i, [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _vp, _u64, _vp]),
    "sdsp_hip_welch_process_host": (_i, [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _vp, _u64]),
    "sdsp_hip_welch_finalize": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _vp]),
    "sdsp_hip_welch_finalize_host": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64]),
    "sdsp_hip_welch_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_welch_plan_launches": (_i, [_vp, _u64, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_welch_plan_get_info": (_i, [_vp, C.POINTER(WelchPlanInfo)]),
    "sdsp_hip_csd_plan_create": (_i, [_pp, _u32, _u32, _vp, _i, _i, _d, _i, _u64, _u64, _vp, _u64, _i]),
    "sdsp_hip_csd_plan_destroy": (_i, [_vp]),
    "sdsp_hip_csd_process": (_i, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _u64, _vp]),
    "sdsp_hip_csd_process_host": (_i, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _u64]),
    "sdsp_hip_csd_finalize": (_i, [_vp, _i, _vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp]),
    "sdsp_hip_csd_finalize_host": (_i, [_vp, _i, _vp, _u64, _vp, _u64, _u64, _vp, _u64]),
    "sdsp_hip_csd_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_csd_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_csd_plan_get_info": (_i, [_vp, C.POINTER(CsdPlanInfo)]),
    "sdsp_hip_pfb_prototype": (_i, [_i, _u32, _u32, _vp]),
    "sdsp_hip_pfb_frames": (_i, [_u32, _u64, C.POINTER(_u64)]),
    "sdsp_hip_pfb_plan_create": (_i, [_pp, _u32, _u32, _u32, _vp, _i, _i, _i, _u64, _i]),
    "sdsp_hip_pfb_plan_destroy": (_i, [_vp]),
    "sdsp_hip_pfb_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_pfb_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _u64, _vp]),
    "sdsp_hip_pfb_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_pfb_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_pfb_plan_set_fold_form": (_i, [_vp, _i]),
    "sdsp_hip_pfb_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_pfb_plan_get_info": (_i, [_vp, C.POINTER(PfbPlanInfo)]),
    "sdsp_hip_pfb_dual_prototype": (_i, [_u32, _u32, _u32, _vp, _vp]),
    "sdsp_hip_pfb_synth_plan_create": (_i, [_pp, _u32, _u32, _u32, _vp, _i, _i, _i, _u64, _i]),
    "sdsp_hip_pfb_synth_plan_destroy": (_i, [_vp]),
    "sdsp_hip_pfb_synth_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_pfb_synth_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _u64, _vp]),
    "sdsp_hip_pfb_synth_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_pfb_synth_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_pfb_synth_plan_set_unfold_form": (_i, [_vp, _i]),
    "sdsp_hip_pfb_synth_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_pfb_synth_plan_get_info": (_i, [_vp, C.POINTER(PfbSynthPlanInfo)]),
    "sdsp_hip_arb_step": (_i, [_d, C.POINTER(_u64)]),
    "sdsp_hip_arb_out_samples": (_i, [_u64, _u64, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "sdsp_hip_arb_design": (_i, [_u32, _u32, _d, _vp]),
    "sdsp_hip_arb_tables": (_i, [_u32, _u32, _vp, _vp, _vp]),
    "sdsp_hip_arb_plan_create": (_i, [_pp, _u32, _u32, _vp, _u64, _i, _i, _i, _i]),
    "sdsp_hip_arb_plan_destroy": (_i, [_vp]),
    "sdsp_hip_arb_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_arb_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _u64, _u64, _vp]),
    "sdsp_hip_arb_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_arb_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_arb_plan_launches": (_i, [_vp, _u64, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_arb_plan_get_info": (_i, [_vp, C.POINTER(ArbPlanInfo)]),
    "sdsp_hip_cic_growth": (_i, [_u32, _u32, _u32, C.POINTER(_u32)]),
    "sdsp_hip_cic_out_samples": (_i, [_u32, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_cic_unity_scale": (_i, [_u32, _u32, _u32, C.POINTER(_d)]),
    "sdsp_hip_cic_taps": (_i, [_u32, _u32, _u32, _vp]),
    "sdsp_hip_cic_plan_create": (_i, [_pp, _u32, _u32, _u32, _i, _u32, _i, _i, _d, _i]),
    "sdsp_hip_cic_plan_destroy": (_i, [_vp]),
    "sdsp_hip_cic_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_cic_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _u64, _vp]),
    "sdsp_hip_cic_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_cic_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_cic_plan_set_segment": (_i, [_vp, _u32]),
    "sdsp_hip_cic_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_cic_plan_get_info": (_i, [_vp, C.POINTER(CicPlanInfo)]),
    "sdsp_hip_cic_interp_growth": (_i, [_u32, _u32, _u32, C.POINTER(_u32)]),
    "sdsp_hip_cic_interp_unity_scale": (_i, [_u32, _u32, _u32, C.POINTER(_d)]),
    "sdsp_hip_cic_interp_plan_create": (_i, [_pp, _u32, _u32, _u32, _i, _u32, _i, _i, _d, _i]),
    "sdsp_hip_cic_interp_plan_destroy": (_i, [_vp]),
    "sdsp_hip_cic_interp_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_cic_interp_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_cic_interp_state_bytes": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_cic_interp_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_cic_interp_plan_set_segment": (_i, [_vp, _u32]),
    "sdsp_hip_cic_interp_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_cic_interp_plan_get_info": (_i, [_vp, C.POINTER(CicInterpPlanInfo)]),
    "sdsp_hip_ddc_phase_word": (_i, [_d, C.POINTER(_u32)]),
    "sdsp_hip_ddc_band_taps": (_i, [_u32, _vp, _u32, _vp]),
    "sdsp_hip_ddc_oscillator": (_i, [_vp, _vp]),
    "sdsp_hip_ddc_out_samples": (_i, [_u32, _u64, C.POINTER(_u64)]),
    "sdsp_hip_ddc_plan_create": (_i, [_pp, _u32, _vp, _u32, _u32, _u32, _vp, _i, _i, _i]),
    "sdsp_hip_ddc_plan_destroy": (_i, [_vp]),
    "sdsp_hip_ddc_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_ddc_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_ddc_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_ddc_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_ddc_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_ddc_plan_get_info": (_i, [_vp, C.POINTER(DdcPlanInfo)]),
    "sdsp_hip_duc_out_samples": (_i, [_u32, _u64, C.POINTER(_u64)]),
    "sdsp_hip_duc_plan_create": (_i, [_pp, _u32, _vp, _u32, _u32, _u32, _vp, _i, _i, _i]),
    "sdsp_hip_duc_plan_destroy": (_i, [_vp]),
    "sdsp_hip_duc_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sdsp_hip_duc_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp]),
    "sdsp_hip_duc_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_duc_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_duc_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_duc_plan_get_info": (_i, [_vp, C.POINTER(DucPlanInfo)]),
    "sdsp_hip_beam_delay_taps": (_i, [_d, _d, _u32, _d, C.POINTER(_u32), _vp]),
    "sdsp_hip_beam_plan_create": (_i, [_pp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _i, _i, _i]),
    "sdsp_hip_beam_plan_destroy": (_i, [_vp]),
    "sdsp_hip_beam_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _vp, _vp]),
    "sdsp_hip_beam_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _vp]),
    "sdsp_hip_beam_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_beam_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_beam_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_beam_plan_get_info": (_i, [_vp, C.POINTER(BeamPlanInfo)]),
    "sdsp_hip_lms_plan_create": (_i, [_pp, _u64, _u32, _i, _i, _i, _d, _i]),
    "sdsp_hip_lms_plan_destroy": (_i, [_vp]),
    "sdsp_hip_lms_process": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _u64, _d, _vp, _vp]),
    "sdsp_hip_lms_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _u64, _d, _vp]),
    "sdsp_hip_lms_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_lms_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_lms_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_lms_plan_get_info": (_i, [_vp, C.POINTER(LmsPlanInfo)]),
    "sdsp_hip_rank_plan_create": (_i, [_pp, _u64, _u32, _u32, _i, _i]),
    "sdsp_hip_rank_plan_destroy": (_i, [_vp]),
    "sdsp_hip_rank_process": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _vp, _vp]),
    "sdsp_hip_rank_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _vp]),
    "sdsp_hip_rank_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_rank_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_rank_plan_set_run": (_i, [_vp, _u64]),
    "sdsp_hip_rank_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_rank_plan_get_info": (_i, [_vp, C.POINTER(RankPlanInfo)]),
    "sdsp_hip_cfar_plan_create": (_i, [_pp, _u64, C.POINTER(CfarDesc), _i, _i]),
    "sdsp_hip_cfar_plan_destroy": (_i, [_vp]),
    "sdsp_hip_cfar_process": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _u64, _vp, _vp]),
    "sdsp_hip_cfar_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _u64, _vp]),
    "sdsp_hip_cfar_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_cfar_plan_set_alpha": (_i, [_vp, _d]),
    "sdsp_hip_cfar_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_cfar_plan_set_run": (_i, [_vp, _u64]),
    "sdsp_hip_cfar_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_cfar_plan_get_info": (_i, [_vp, C.POINTER(CfarPlanInfo)]),
    "sdsp_hip_cfar2d_plan_create": (_i, [_pp, _u32, _u32, _u64, C.POINTER(Cfar2dDesc), _vp, _i, _i]),
    "sdsp_hip_cfar2d_plan_destroy": (_i, [_vp]),
    "sdsp_hip_cfar2d_process": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    "sdsp_hip_cfar2d_process_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64]),
    "sdsp_hip_cfar2d_plan_set_alpha": (_i, [_vp, _d]),
    "sdsp_hip_cfar2d_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_cfar2d_plan_launches": (_i, [_vp, _i, _i, C.POINTER(_u64)]),
    "sdsp_hip_cfar2d_plan_get_info": (_i, [_vp, C.POINTER(Cfar2dPlanInfo)]),
    "sdsp_hip_cfar2d_scale": (_i, [_u32, _u32, C.POINTER(Cfar2dDesc), _d, _vp]),
    "sdsp_hip_pll_oscillator": (_i, [_vp, _vp]),
    "sdsp_hip_pll_gains": (_i, [_d, _d, _d, _i, C.POINTER(_d), C.POINTER(_d)]),
    "sdsp_hip_pll_plan_create": (_i, [_pp, _u64, _i, _i, C.POINTER(_u32), _u64, _d, _i]),
    "sdsp_hip_pll_plan_destroy": (_i, [_vp]),
    "sdsp_hip_pll_process": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _u64, _d, _d, _vp, _vp]),
    "sdsp_hip_pll_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _u64, _d, _d, _vp]),
    "sdsp_hip_pll_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_pll_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_pll_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_pll_plan_get_info": (_i, [_vp, C.POINTER(PllPlanInfo)]),
    "sdsp_hip_timing_step": (_i, [_d, C.POINTER(_u64)]),
    "sdsp_hip_timing_max_out_for": (_i, [_u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_timing_gains": (_i, [_d, _d, _d, _d, C.POINTER(_d), C.POINTER(_d)]),
    "sdsp_hip_timing_design": (_i, [_u32, _u32, _d, _d, _vp]),
    "sdsp_hip_timing_plan_create": (_i, [_pp, _u64, _i, _i, _u32, _u32, _vp, _u64, _d, _i]),
    "sdsp_hip_timing_plan_destroy": (_i, [_vp]),
    "sdsp_hip_timing_process": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _d, _d, _vp, _vp]),
    "sdsp_hip_timing_process_host": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _d, _d, _vp]),
    "sdsp_hip_timing_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_timing_max_out": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_timing_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_timing_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_timing_plan_get_info": (_i, [_vp, C.POINTER(TimingPlanInfo)]),
    "sdsp_hip_viterbi_delay": (_i, [_u32, _u32, C.POINTER(_u32)]),
    "sdsp_hip_conv_encode": (_i, [_u32, _u32, C.POINTER(_u32), _vp, _u64, _i, _vp]),
    "sdsp_hip_viterbi_plan_create": (_i, [_pp, _u32, _u32, C.POINTER(_u32), _u32, _u32, _i, _i, C.c_float, _u64, _i]),
    "sdsp_hip_viterbi_plan_destroy": (_i, [_vp]),
    "sdsp_hip_viterbi_process": (_i, [_vp, _vp, _vp, _u64, _u64, _vp]),
    "sdsp_hip_viterbi_process_host": (_i, [_vp, _vp, _vp, _u64, _u64]),
    "sdsp_hip_viterbi_plan_reset": (_i, [_vp, _i]),
    "sdsp_hip_viterbi_plan_get_metrics": (_i, [_vp, _vp, _u64]),
    "sdsp_hip_viterbi_plan_set_metrics": (_i, [_vp, _vp, _u64]),
    "sdsp_hip_viterbi_plan_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_viterbi_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_viterbi_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_viterbi_plan_get_info": (_i, [_vp, C.POINTER(ViterbiPlanInfo)]),
    "sdsp_hip_rs_generator": (_i, [_u32, _u32, _u32, _u32, _vp]),
    "sdsp_hip_rs_encode": (_i, [_u32, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp]),
    "sdsp_hip_rs_plan_create": (_i, [_pp, _u32, _u32, _u32, _u32, _u32, _u32, _i, _i]),
    "sdsp_hip_rs_plan_destroy": (_i, [_vp]),
    "sdsp_hip_rs_process": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "sdsp_hip_rs_process_host": (_i, [_vp, _vp, _vp, _vp, _vp, _u64]),
    "sdsp_hip_rs_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_rs_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_rs_plan_get_info": (_i, [_vp, C.POINTER(RsPlanInfo)]),
    "sdsp_hip_fsync_ccsds_pn": (_i, [_vp, _u64]),
    "sdsp_hip_fsync_attach": (_i, [_u64, _u32, _u32, _vp, _vp, _u64, _i, _vp]),
    "sdsp_hip_fsync_max_frames": (_i, [_u32, _u32, _u64, C.POINTER(_u64)]),
    "sdsp_hip_fsync_plan_create": (_i, [_pp, _u64, _u32, _u32, _u32, _u32, _u32, _i, _vp, _i, _u64, _u64, _i]),
    "sdsp_hip_fsync_plan_destroy": (_i, [_vp]),
    "sdsp_hip_fsync_process": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    "sdsp_hip_fsync_process_host": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64]),
    "sdsp_hip_fsync_plan_reset": (_i, [_vp]),
    "sdsp_hip_fsync_plan_get_state": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64]),
    "sdsp_hip_fsync_plan_state_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "sdsp_hip_fsync_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_fsync_plan_launches": (_i, [_vp, _u64, _u64, C.POINTER(_u64)]),
    "sdsp_hip_fsync_plan_get_info": (_i, [_vp, C.POINTER(FsyncPlanInfo)]),
    "sdsp_hip_ldpc_parity_matrix": (_i, [_vp, _u32, _u32, _u32, _vp]),
    "sdsp_hip_ldpc_encode": (_i, [_vp, _u32, _u32, _u32, _vp, _u64, _vp]),
    "sdsp_hip_ldpc_plan_create": (_i, [_pp, _vp, _u32, _u32, _u32, _u32, _u32, _i, _i, C.c_float, _i, _u32, _i]),
    "sdsp_hip_ldpc_plan_destroy": (_i, [_vp]),
    "sdsp_hip_ldpc_process": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "sdsp_hip_ldpc_process_host": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _u32]),
    "sdsp_hip_ldpc_plan_set_variant": (_i, [_vp, _i]),
    "sdsp_hip_ldpc_plan_launches": (_i, [_vp, _u64, C.POINTER(_u64)]),
    "sdsp_hip_ldpc_plan_get_info": (_i, [_vp, C.POINTER(LdpcPlanInfo)]),
}

_lib = None


class StaleLibraryError(RuntimeError):
    """libsdsp_hip.so does not match the sources beside it"""


def built_hash(lib) -> str:
    """the source hash the library was built from (sdsp_hip_version() ends in "src:<hash>")"""
    lib.sdsp_hip_version.restype = C.c_char_p
    v = lib.sdsp_hip_version().decode()
    return v.rsplit("src:", 1)[1] if "src:" in v else "unhashed"


def _open(path, fresh: bool = False) -> C.CDLL:
    if fresh:  # dlopen caches by path: load the rebuilt file through a private copy
        import shutil
        import tempfile
        tmp = Path(tempfile.mkdtemp(prefix="sdsp_hip_")) / path.name
        shutil.copy2(path, tmp)
        path = tmp
    return C.CDLL(str(path))


def _bind(lib) -> C.CDLL:
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


def load(build_if_missing: bool = True) -> C.CDLL:
    """Load libsdsp_hip.so (building it with hipcc first if it is not there)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1.  A process must end up
    # with ONE HIP runtime: if torch is going to be used (it is our device-memory plumbing), it has
    # to be loaded first so that this library binds to the same copy by soname.  Loading ours first
    # leaves two HSA runtimes in the process and the second one finds no device.
    if os.environ.get("SDSP_HIP_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    from .build import build_library, source_hash
    if not LIB_PATH.exists():
        if not build_if_missing:
            raise FileNotFoundError(f"{LIB_PATH} is missing: run `python -m simpledsp_amd.build`")
        build_library()
    lib = _open(LIB_PATH)
    # a library built from other sources than the ones beside it (an edited header whose object was not rebuilt, a .so
    # left over from another checkout) must not be what gets tested and benched: rebuild, or refuse
    want = source_hash()
    if built_hash(lib) != want:
        if not build_if_missing or os.environ.get("SDSP_HIP_NO_REBUILD") == "1":
            raise StaleLibraryError(f"{LIB_PATH} was built from other sources (library {built_hash(lib)}, tree {want}): "
                                    "run `python -m simpledsp_amd.build`")
        print(f"simpledsp_amd: {LIB_PATH.name} is stale ({built_hash(lib)} != {want}), rebuilding", file=sys.stderr)
        build_library()
        lib = _open(LIB_PATH, fresh=True)
        if built_hash(lib) != want:
            raise StaleLibraryError(f"{LIB_PATH} still reports {built_hash(lib)} after a rebuild (tree {want})")
    _lib = _bind(lib)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise SdspHipError(rc, load().sdsp_hip_last_error_string().decode(errors="replace"))
