"""Double-precision reference of the polyphase filter-bank contract (include/sdsp_hip.h, sdsp_hip_pfb_process): x = the stream's
history followed by the block, u_j[r] = sum_p x[j D + p M + r] h[p M + r] in ascending p, FRAME: Y_j = fft(u_j); TIME: u_j rotated by
s_j = (position + j D - hist) mod M first.  Real input keeps bins 0 .. M / 2.  History newest first.  Shared by
tests/test_pfb_host.py and tests/test_gpu_pfb.py."""
import numpy as np


def pfb_fold_ref(x, m, p, hop, taps, hist=None):
    """the folded frames (streams, F, M) before any rotation, and the new state"""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    x2 = x.astype(np.complex128 if cplx else np.float64)
    h = np.asarray(taps, dtype=np.float64)
    Cn, S = x2.shape
    L = m * p
    H = L - hop
    assert S % hop == 0 and h.size == L
    F = S // hop
    hist2 = np.zeros((Cn, H), dtype=x2.dtype) if hist is None else np.asarray(hist, dtype=x2.dtype).reshape(Cn, H)
    full = np.concatenate([hist2[:, ::-1], x2], axis=1)  # oldest first
    idx = np.arange(F)[:, None] * hop + np.arange(L)[None, :]
    prod = (full[:, idx] * h).reshape(Cn, F, p, m)
    u = np.zeros((Cn, F, m), dtype=x2.dtype)
    if F:
        u = prod[:, :, 0, :].copy()
        for q in range(1, p):  # ascending p
            u = u + prod[:, :, q, :]
    state = full[:, ::-1][:, :H].copy()  # newest first
    return u, state


def pfb_shifts(m, p, hop, frames, position):
    """s_j = (position + j hop - hist) mod m"""
    return (position + np.arange(frames) * hop - (m * p - hop)) % m


def pfb_ref(x, m, p, hop, taps, hist=None, phase="time", position=0):
    """x: (S,) or (streams, S), real or complex, S a multiple of hop; hist: (hist,) or (streams, hist) newest first, or None (zeros).
    Returns (out (streams?, F, bins), new_state (streams?, hist))."""
    x = np.asarray(x)
    one = x.ndim == 1
    x2 = x[None, :] if one else x
    u, state = pfb_fold_ref(x2, m, p, hop, taps, None if hist is None else np.asarray(hist).reshape(x2.shape[0], -1))
    F = u.shape[1]
    if phase == "time":
        s = pfb_shifts(m, p, hop, F, position)
        v = np.empty_like(u)
        for j in range(F):
            v[:, j] = np.roll(u[:, j], int(s[j]), axis=-1)
    else:
        assert phase == "frame"
        v = u
    y = np.fft.fft(v, axis=-1) if np.iscomplexobj(x2) else np.fft.rfft(v, axis=-1)
    if one:
        return y[0], state[0]
    return y, state
