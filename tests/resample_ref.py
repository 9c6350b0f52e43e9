"""Double-precision reference of the polyphase resampler contract (include/sdsp_hip.h, sdsp_hip_resample_process), in the
contract's summation order: each output sums exactly its own taps in ascending k, a plain multiply first, then one multiply and
one add per tap (numpy never fuses).  Shared by tests/test_resample_host.py and tests/test_gpu_resample.py."""
from math import gcd

import numpy as np

GRID_UD = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 8), (2, 1), (3, 1), (4, 1), (2, 3), (3, 2), (5, 7), (160, 147), (147, 160)]
GRID_T = [1, 2, 16, 17, 64, 65, 255, 1024]


def q_of(up, down):
    return down // gcd(up, down)


def hist_of(taps, up):
    return (taps - 1) // up


def resample_ref(h, x, up, down, hist=None):
    """x: (S,) or (channels, S); hist: (H,) or (channels, H) newest first, or None (zeros).  Returns (y, new_state)."""
    h = np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x2 = x[None, :] if one else x
    C, S = x2.shape
    T, H = h.size, hist_of(h.size, up)
    assert S % q_of(up, down) == 0
    M = S * up // down
    if hist is None:
        hs = np.zeros((C, H))
    else:
        hs = np.asarray(hist, dtype=np.float64).reshape(C, -1)[:, :H]
    ext = np.concatenate([hs[:, ::-1], x2], axis=1)  # ext[:, H + i] = x[:, i]; ext[:, H - 1 - j] = hist[:, j]
    n = np.arange(M, dtype=np.int64) * down
    p, b = n % up, n // up
    tp = np.where(p < T, (T - 1 - p) // up + 1, 0)
    y = np.zeros((C, M))
    for j in range(int(tp.max()) if M else 0):
        sel = np.nonzero(tp > j)[0]
        term = h[p[sel] + j * up][None, :] * ext[:, H + b[sel] - j]
        y[:, sel] = term if j == 0 else y[:, sel] + term
    state = ext[:, ext.shape[1] - H:][:, ::-1].copy() if H else np.zeros((C, 0))
    return (y[0], state[0]) if one else (y, state)


def phase_tap_sums(h, up, down, m):
    """sum of the taps of output m's phase, per output, ascending k"""
    p = (np.asarray(m, dtype=np.int64) * down) % up
    out = np.zeros(p.shape)
    for i, pi in enumerate(p):
        s = 0.0
        for k in range(int(pi), h.size, up):
            s = s + h[k]
        out[i] = s
    return out
