"""Double-precision reference of the cross-spectral density contract (include/sdsp_hip.h, sdsp_hip_csd_*): the Welch reference's
segments, history, detrend and window (tests/welch_ref.py), conj(X_a) X_b summed per pair and |X_c|^2 per channel, then the one-sided
scaling or the coherence ratio.  Shared by tests/test_csd_host.py and tests/test_gpu_csd.py, with the
channels and pairs both use."""
import numpy as np
import scipy.signal

from welch_ref import detrend_segments, welch_frames, welch_scale

PAIRS = [(0, 1), (0, 3), (2, 1), (3, 3), (1, 0)]


def csd_inputs(n_fft, S, seed, dtype=np.float64):
    """the GPU tests' four channels: noise + 0.8 x a shared noise row + a linear trend; channel 3 = a short FIR of channel 0 + a
    little noise, so that the pair (0, 3) is highly coherent.  The trend runs from -2 to 3 over sqrt(n_fft): an undetrended
    segment's bin 0 grows with (mean n_fft)^2 and the noise bins with n_fft, so this keeps bin 0 a few times the noise level at
    every n_fft -- enough for the detrenders to have something to remove, and no auto spectrum falls below 1e-4 of its peak
    (tests/test_csd_host.py checks that for the shapes of the GPU tests)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((4, S)) + 0.8 * rng.standard_normal(S) + np.linspace(-2, 3, S) / np.sqrt(n_fft)
    x[3] = scipy.signal.lfilter([0.5, 0.3, -0.2], 1, x[0]) + 0.05 * rng.standard_normal(S)
    return x.astype(dtype)


def csd_ref(x, pairs, n_fft, hop, window, detrend="constant", position=0, hist=None, acc_xy=None, acc_auto=None):
    """x: (channels, S) block at stream position `position`; pairs: (npairs, 2) channel indices; hist: (channels, N - 1) newest
    first (None: zeros, only meaningful at position 0); acc_xy: (npairs, bins) complex sums so far and acc_auto: (channels, bins)
    (None: zeros).  Returns (acc_xy, acc_auto, segments counted, new history)."""
    x = np.asarray(x, dtype=np.float64)
    C, S = x.shape
    H = n_fft - 1
    bins = n_fft // 2 + 1
    pairs = np.asarray(pairs).reshape(-1, 2)
    w = np.asarray(window, dtype=np.float64)
    hist2 = np.zeros((C, H)) if hist is None else np.asarray(hist, dtype=np.float64).reshape(C, H)
    xy = np.zeros((len(pairs), bins), dtype=np.complex128) if acc_xy is None else np.array(acc_xy, dtype=np.complex128)
    au = np.zeros((C, bins)) if acc_auto is None else np.array(acc_auto, dtype=np.float64)
    full = np.concatenate([hist2[:, ::-1], x], axis=1)  # full[:, p] = stream sample position - H + p
    F = welch_frames(n_fft, hop, position, S)
    if F:
        first = 0 if position < n_fft else (position - n_fft) // hop + 1
        starts = first * hop - position + H + np.arange(F) * hop
        seg = full[:, starts[:, None] + np.arange(n_fft)[None, :]]  # (C, F, N)
        y = np.fft.rfft(detrend_segments(seg, detrend) * w, axis=-1)
        xy = xy + (np.conj(y[pairs[:, 0]]) * y[pairs[:, 1]]).sum(axis=1)
        au = au + (y.real * y.real + y.imag * y.imag).sum(axis=1)
    state = full[:, ::-1][:, :H].copy()
    return xy, au, F, state


def _m(bins):
    m = np.full(bins, 2.0)
    m[0] = m[-1] = 1.0
    return m


def csd_density(acc_xy, frames, window, fs=1.0, scaling="density"):
    """out = acc_xy c_k, c_k = m_k scale / frames (m_k = 2 between bins 0 and N / 2)"""
    acc_xy = np.asarray(acc_xy)
    return acc_xy * (_m(acc_xy.shape[-1]) * welch_scale(window, fs, scaling) / frames)


def csd_coherence(acc_xy, acc_auto, pairs):
    """|sum conj(X_a) X_b|^2 / (sum |X_a|^2 sum |X_b|^2): scale and segment count cancel"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    acc_xy, acc_auto = np.asarray(acc_xy), np.asarray(acc_auto)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (acc_xy.real ** 2 + acc_xy.imag ** 2) / (acc_auto[pairs[:, 0]] * acc_auto[pairs[:, 1]])
