"""Double-precision reference of the polyphase synthesis contract (include/sdsp_hip.h, sdsp_hip_pfb_synth_process): v_j = ifft / irfft of
frame j, u_j[r] = v_j[(r + s_j) mod M] (TIME; s_j from pfb_ref.pfb_shifts) or v_j (FRAME), the pending sums first, then
g[n] u_j[n mod M] added into positions j D .. j D + L - 1 in ascending j.  Shared by tests/test_pfb_synth_host.py and
tests/test_gpu_pfb_synth.py."""
import numpy as np

from pfb_ref import pfb_shifts


def pfb_synth_frames_ref(X, m, p, hop, phase="time", position=0, cplx=None):
    """u (streams, F, M): the reverse transforms, un-rolled for TIME"""
    X = np.asarray(X, dtype=np.complex128)
    cplx = X.shape[-1] == m if cplx is None else cplx
    if cplx:
        v = np.fft.ifft(X, axis=-1)
    else:
        assert X.shape[-1] == m // 2 + 1
        X = X.copy()
        X[..., 0] = X[..., 0].real  # irfft ignores these imaginary parts
        X[..., -1] = X[..., -1].real
        v = np.fft.irfft(X, n=m, axis=-1)
    F = X.shape[1]
    if phase == "time":
        s = pfb_shifts(m, p, hop, F, position)
        u = np.empty_like(v)
        for j in range(F):
            u[:, j] = np.roll(v[:, j], -int(s[j]), axis=-1)  # u[r] = v[(r + s) mod M]
        return u
    assert phase == "frame"
    return v


def pfb_synth_ref(X, m, p, hop, g, pending=None, phase="time", position=0, cplx=None):
    """X: (F, bins) or (streams, F, bins) complex, bins = M (complex output) or M / 2 + 1 (real output); g: the synthesis prototype
    (L,); pending: (hist,) or (streams, hist) in time order, or None (zeros).  Returns (y (streams?, F D), new pending (streams?, hist))."""
    X = np.asarray(X, dtype=np.complex128)
    one = X.ndim == 2
    X3 = X[None] if one else X
    Cn, F, _ = X3.shape
    Lt = m * p
    H = Lt - hop
    u = pfb_synth_frames_ref(X3, m, p, hop, phase, position, cplx)
    z = np.tile(u, (1, 1, p)) * np.asarray(g, dtype=np.float64)  # (C, F, L): g[n] u_j[n mod M]
    a = np.zeros((Cn, F * hop + H), dtype=z.dtype)
    if pending is not None:
        a[:, :H] = np.asarray(pending, dtype=z.dtype).reshape(Cn, H)
    for j in range(F):  # ascending j
        a[:, j * hop:j * hop + Lt] += z[:, j]
    y, state = a[:, :F * hop].copy(), a[:, F * hop:].copy()
    if one:
        return y[0], state[0]
    return y, state


def dual_systems(h, m, p, hop):
    """the perfect-reconstruction conditions per residue t0 < D: (index vector of the unknowns g[t0 + i D], A, b) with the rows that
    are identically zero dropped"""
    h = np.asarray(h, dtype=np.float64)
    Lt = m * p
    out = []
    for t0 in range(hop):
        idx = np.arange(t0, Lt, hop)
        rows, rhs = [], []
        for k in range(1 - p, p):
            q = idx + k * m
            ok = (q >= 0) & (q < Lt)
            row = np.where(ok, h[np.clip(q, 0, Lt - 1)], 0.0)
            if np.any(row != 0.0):
                rows.append(row)
                rhs.append(1.0 if k == 0 else 0.0)
        out.append((idx, np.array(rows).reshape(len(rows), idx.size), np.array(rhs)))
    return out
