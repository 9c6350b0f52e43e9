"""Double-precision reference of the Welch PSD contract (include/sdsp_hip.h, sdsp_hip_welch_*): scipy's segments m hop .. m hop + N
counted by the call in which they end, the history newest first, detrend, window, |rfft|^2 summed per channel, then the one-sided
scaling.  Shared by tests/test_welch_host.py and tests/test_gpu_welch.py."""
import numpy as np


def welch_frames(n_fft, hop, position, samples):
    """segments m >= 0 with position < m hop + n_fft <= position + samples"""
    def ended(p):
        return 0 if p < n_fft else (p - n_fft) // hop + 1
    return ended(position + samples) - ended(position)


def detrend_segments(seg, detrend):
    """seg: (..., N) in double; scipy.signal.detrend's 'constant' / 'linear' in the contract's closed form"""
    if detrend in ("none", None, False):
        return seg
    n = seg.shape[-1]
    mu = seg.sum(axis=-1, keepdims=True) / n
    if detrend == "constant":
        return seg - mu
    t = np.arange(n) - (n - 1) / 2
    beta = (seg * t).sum(axis=-1, keepdims=True) / (n * (n * n - 1) / 12)
    return seg - (mu + beta * t)


def welch_ref(x, n_fft, hop, window, detrend="constant", position=0, hist=None, acc=None):
    """x: (channels, S) block at stream position `position`; hist: (channels, N - 1) newest first (None: zeros, only meaningful at
    position 0); acc: (channels, bins) sums so far (None: zeros).  Returns (acc, segments counted, new history)."""
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x2 = x[None, :] if one else x
    C, S = x2.shape
    H = n_fft - 1
    w = np.asarray(window, dtype=np.float64)
    hist2 = np.zeros((C, H)) if hist is None else np.asarray(hist, dtype=np.float64).reshape(C, H)
    acc2 = np.zeros((C, n_fft // 2 + 1)) if acc is None else np.array(acc, dtype=np.float64).reshape(C, -1)
    full = np.concatenate([hist2[:, ::-1], x2], axis=1)  # full[:, p] = stream sample position - H + p
    F = welch_frames(n_fft, hop, position, S)
    if F:
        first = 0 if position < n_fft else (position - n_fft) // hop + 1
        starts = first * hop - position + H + np.arange(F) * hop
        seg = full[:, starts[:, None] + np.arange(n_fft)[None, :]]  # (C, F, N)
        y = np.fft.rfft(detrend_segments(seg, detrend) * w, axis=-1)
        acc2 = acc2 + (y.real * y.real + y.imag * y.imag).sum(axis=1)
    state = full[:, ::-1][:, :H].copy()
    if one:
        return acc2[0], F, state[0]
    return acc2, F, state


def welch_scale(window, fs=1.0, scaling="density"):
    w = np.asarray(window, dtype=np.float64)
    return 1.0 / (fs * (w * w).sum()) if scaling == "density" else 1.0 / w.sum() ** 2


def welch_psd(acc, frames, window, fs=1.0, scaling="density"):
    """out = acc c_k, c_k = m_k scale / frames (m_k = 2 between bins 0 and N / 2)"""
    acc = np.asarray(acc, dtype=np.float64)
    bins = acc.shape[-1]
    m = np.full(bins, 2.0)
    m[0] = m[-1] = 1.0
    return acc * (m * welch_scale(window, fs, scaling) / frames)
