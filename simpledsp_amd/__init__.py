"""simpledsp_amd -- MI355X-native batched FFT + cascaded-biquad engine behind simpledsp's sdsp:: surface.

The product is the HIP library (csrc/ -> lib/libsdsp_hip.so) behind the C ABI in include/sdsp_hip.h;
this package is its Python host mirror.  Importing does not touch the GPU; any compute call without
the library or without a HIP device raises (there is no CPU path here).
"""
from ._lib import (F32, F64, F32_F64STATE, FORWARD, REVERSE, IIR_GENERIC, IIR_LP, IIR_HP, IIR_BP, FILTER_NONE,
                   FILTER_LOW_PASS, FILTER_HIGH_PASS, FILTER_BAND_PASS, FILTER_BAND_STOP, FIR_DIRECT, FIR_FFT, PAD_NONE, PAD_ODD, PAD_EVEN,
                   PAD_CONSTANT, DETREND_NONE, DETREND_CONSTANT, DETREND_LINEAR, SCALING_DENSITY, SCALING_SPECTRUM, CSD_CROSS, CSD_COHERENCE, PFB_REAL, PFB_COMPLEX,
                   PFB_PHASE_FRAME, PFB_PHASE_TIME, DDC_REAL, DDC_COMPLEX, ARB_REAL, ARB_COMPLEX, ARB_NEAREST, ARB_LINEAR, CIC_REAL, CIC_COMPLEX, CIC_I16, CIC_I32, CIC_OUT_INT, CIC_OUT_F32, DUC_REAL, DUC_COMPLEX,
                   BEAM_REAL, BEAM_COMPLEX,
                   LMS_REAL, LMS_COMPLEX, LMS_LMS, LMS_NLMS,
                   CFAR_CA, CFAR_GO, CFAR_SO, CFAR_OS, CFAR_POWER, CFAR_IQ,
                   PLL_CROSS, PLL_BPSK, PLL_QPSK,
                   TIMING_GARDNER, TIMING_ZC_QPSK, TIMING_ZC_BPSK,
                   FFT_COLS_COMPLEX, FFT_COLS_POWER,
                   CFAR2D_EDGE_MARK, CFAR2D_EDGE_CLIP,
                   VITERBI_I8, VITERBI_F32, VITERBI_BYTES, VITERBI_PACKED,
                   RS_FULL, RS_DATA,
                   FSYNC_BYTES, FSYNC_PACKED, FSYNC_NORMAL, FSYNC_EITHER, FSYNC_SEARCH, FSYNC_VERIFY, FSYNC_LOCK,
                   LDPC_I8, LDPC_F32, LDPC_BYTES, LDPC_PACKED,
                   SdspHipError, load)
from .fft import (FftPlan, RfftPlan, fft_radix2, fft_radix4, forward_fft, reverse_fft, log2, log4, isPowerOf2,
                  isPowerOf4, digit_reverse, calc_swap_lookup, calc_twiddles, calc_wCoeffs)
from .fft_cols import FftColsPlan, fft2, ifft2
from .iir import casc_2o_iir, casc_2o_iir_lp, casc_2o_iir_hp, casc_2o_iir_bp
from .fir import fir_filter, fft_fir_filter, fir_fft_size
from .resample import fir_resampler
from .stft import stft_bank, stft_window
from .istft import istft_bank, synthesis_window as istft_synthesis_window
from .filtfilt import filtfilt_plan, sosfiltfilt, steady_state as iir_steady_state, default_padlen as filtfilt_default_padlen
from .welch import welch_bank, welch
from .csd import csd_bank, csd, coherence
from .pfb import pfb_bank, pfb_prototype
from .pfb_synth import pfb_synthesis_bank, pfb_dual_prototype
from .ddc import ddc_bank, ddc_phase_word
from .arb_resample import arb_resampler, arb_step
from .cic import cic_decimator, cic_growth, cic_unity_scale, cic_taps
from .cic_interp import cic_interpolator, cic_interp_growth, cic_interp_unity_scale
from .duc import duc_bank
from .beamformer import beamformer_bank, beam_delay_taps, plane_wave_delays
from .lms import lms_bank
from .rank_filter import rank_filter_bank, medfilt
from .cfar import cfar_bank, cfar_alpha, cfar
from .cfar2d import cfar2d_plan, cfar2d, cfar2d_scale, range_doppler_detect, Cfar2dHits, Cfar2dResult
from .pll import pll_bank, pll_gains
from .timing import timing_bank, timing_step, timing_max_out, timing_gains, timing_design
from .viterbi import viterbi_bank, viterbi_delay, viterbi_decode, conv_encode
from .rs import rs_decoder, rs_decode, rs_encode, rs_generator
from .fsync import frame_sync_bank, ccsds_pn, attach_sync, fsync_max_frames, CCSDS_ASM
from .ldpc import ldpc_decoder, ldpc_decode, ldpc_encode, ldpc_parity_matrix


def set_launch_piece_bytes(nbytes: int) -> None:
    """Process-wide launch granularity (include/sdsp_hip.h: sdsp_hip_set_launch_piece_bytes); 0 = never split."""
    from ._lib import check
    check(load().sdsp_hip_set_launch_piece_bytes(int(nbytes)))


def get_launch_piece_bytes() -> int:
    import ctypes
    from ._lib import check
    v = ctypes.c_uint64(0)
    check(load().sdsp_hip_get_launch_piece_bytes(ctypes.byref(v)))
    return v.value


class filter_type:  # filter_type.h:6
    none, low_pass, high_pass, band_pass = 0, 1, 2, 3
    band_stop = 4  # not in the reference's enum (README.md:15 TODO)
