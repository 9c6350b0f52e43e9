"""Double-precision reference of the STFT contract (include/sdsp_hip.h, sdsp_hip_stft_process): x = the channel's history followed
by the block, frame j = rfft(x[j hop : j hop + N] * w), history newest first.  Shared by tests/test_stft_host.py and
tests/test_gpu_stft.py."""
import numpy as np


def stft_ref(x, n_fft, hop, window, hist=None, output="complex"):
    """x: (S,) or (channels, S), S a multiple of hop; hist: (hist,) or (channels, hist) newest first, or None (zeros).
    Returns (out (channels?, F, N/2+1), new_state (channels?, hist))."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(window, dtype=np.float64)
    one = x.ndim == 1
    x2 = x[None, :] if one else x
    C, S = x2.shape
    H = n_fft - hop
    assert S % hop == 0 and w.size == n_fft
    F = S // hop
    if hist is None:
        hist2 = np.zeros((C, H))
    else:
        hist2 = np.asarray(hist, dtype=np.float64).reshape(C, H)
    full = np.concatenate([hist2[:, ::-1], x2], axis=1)  # oldest first
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]
    frames = full[:, idx] * w  # (C, F, N)
    y = np.fft.rfft(frames, axis=-1)
    if output == "power":
        y = y.real * y.real + y.imag * y.imag
    elif output == "magnitude":
        y = np.sqrt(y.real * y.real + y.imag * y.imag)
    state = full[:, ::-1][:, :H].copy()  # newest first
    if one:
        return y[0], state[0]
    return y, state
