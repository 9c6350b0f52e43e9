"""Double-precision reference of the inverse STFT contract (include/sdsp_hip.h, sdsp_hip_istft_process): z_j = irfft(X_j), the
pending sums first, then fl(g z_j) added into positions j hop .. j hop + N - 1 in ascending j.  Shared by tests/test_istft_host.py
and tests/test_gpu_istft.py."""
import numpy as np


def synthesis_window_ref(window, n_fft, hop, normalized=True):
    """g = w / env[n mod hop], env[r] = sum over ascending k of w[r + k hop]^2 (None where NOLA fails); RAW: g = w"""
    w = np.asarray(window, dtype=np.float64)
    if not normalized:
        return w.copy()
    env = np.zeros(hop)
    for i in range(n_fft):
        env[i % hop] += w[i] * w[i]
    if not env.min() > 1e-10 * env.max():
        return None
    return w / env[np.arange(n_fft) % hop]


def istft_ref(X, n_fft, hop, g, pending=None):
    """X: (F, N/2+1) or (channels, F, N/2+1) complex; g: the synthesis window; pending: (hist,) or (channels, hist) in time order,
    or None (zeros).  Returns (y (channels?, F hop), new pending (channels?, hist))."""
    X = np.asarray(X, dtype=np.complex128)
    one = X.ndim == 2
    X3 = X[None] if one else X
    Cn, F, bins = X3.shape
    assert bins == n_fft // 2 + 1
    H = n_fft - hop
    X3 = X3.copy()
    X3[..., 0] = X3[..., 0].real  # irfft ignores these imaginary parts
    X3[..., -1] = X3[..., -1].real
    z = np.fft.irfft(X3, n=n_fft, axis=-1) * np.asarray(g, dtype=np.float64)  # (C, F, N)
    a = np.zeros((Cn, F * hop + H))
    if pending is not None:
        a[:, :H] = np.asarray(pending, dtype=np.float64).reshape(Cn, H)
    for j in range(F):
        a[:, j * hop:j * hop + n_fft] += z[:, j]
    y, state = a[:, :F * hop].copy(), a[:, F * hop:].copy()
    if one:
        return y[0], state[0]
    return y, state
