"""numpy reference of the arbitrary-ratio polyphase resampler bank (include/sdsp_hip.h: sdsp_hip_arb_*) in
exactly the contract's operation order, and the grids the resampler tests share.

Time is exact: Python integers for a call's bounds, uint64 for the per-output times (every valid t is below 2^63).  The tables are
made here in double and rounded with astype, as the plan rounds them, so the reference needs neither the library nor a device.  f64
follows the order literally (numpy never contracts); an f32 fmaf is ddc_ref._fma32.  Vectorised over outputs, one loop over k."""
import numpy as np

from ddc_ref import _fma32

SPLIT = [0, 1, 7, 0, 300, 592]   # a stream of 900 samples in calls of these lengths
BLOCKS = [0, 1, 3, 0, 7, 1, 11]  # the GPU tests' call lengths, in units derived from the plan's block_out
SHAPES = [(1, 1), (1, 5), (4, 5), (32, 16), (128, 12)]  # (L, T)
RATIOS = [0.7317, 1.0000131, 2.37, 37.5, 1 / 3.0001]
ONE = 1 << 32


def step_of(ratio):
    """round(ratio 2^32), ties to even, on an exact product"""
    return round(ratio * 2.0 ** 32)


def real_dtype(precision):
    return np.float64 if precision == "f64" else np.float32


def out_samples(step, time, samples):
    """(n_out, next_time) in Python integers"""
    end = samples << 32
    n = 0 if time >= end else -((time - end) // step)  # ceil((end - time) / step)
    return n, time + n * step - end


def tables(h, L, T):
    """(H, Dt), (L, T) doubles: H[p][k] = h[k L + p], Dt[p][k] = hext[k L + p + 1] - h[k L + p], hext = h followed by zeros"""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    assert h.size == L * T
    hext = np.concatenate([h, [0.0]])
    return h.reshape(T, L).T.copy(), (hext[1:] - h).reshape(T, L).T.copy()


def _plane(Ht, Dt, ext, Hn, i, p, mu, linear, dt):
    """one real plane: ext[Hn + n] = x[n]"""
    a = Ht[p, 0] * ext[Hn + i]  # a plain multiply
    b = Dt[p, 0] * ext[Hn + i]
    for k in range(1, Ht.shape[1]):
        xk = ext[Hn + i - k]
        if dt == np.float32:
            a = _fma32(Ht[p, k], xk, a)
            b = _fma32(Dt[p, k], xk, b) if linear else b
        else:
            a = a + Ht[p, k] * xk
            b = b + Dt[p, k] * xk if linear else b
    if not linear:
        return a
    return _fma32(mu, b, a) if dt == np.float32 else a + mu * b


def arb_ref(h, L, T, x, step, time=0, hist=None, interp="linear", precision="f64"):
    """x: (channels, S) real or complex; hist: (channels, T - 1) newest first, or None for zero history.  Returns (y, state,
    next_time): y (channels, n_out) of the input kind and precision, state (channels, T - 1)."""
    dt = real_dtype(precision)
    cdt = np.complex128 if precision == "f64" else np.complex64
    x = np.atleast_2d(np.asarray(x))
    cplx = np.iscomplexobj(x)
    x = x.astype(cdt if cplx else dt)
    channels, S = x.shape
    Hn = T - 1
    lb = L.bit_length() - 1
    assert 1 << lb == L
    if hist is None:
        hist = np.zeros((channels, Hn), dtype=x.dtype)
    hist = np.asarray(hist).astype(x.dtype).reshape(channels, Hn)
    ext = np.concatenate([hist[:, ::-1], x], axis=1)  # ext[:, Hn + n] = x[n]
    state = ext[:, ::-1][:, :Hn].copy()
    n_out, next_time = out_samples(int(step), int(time), S)
    Hd, Dd = tables(h, L, T)
    Ht, Dt = Hd.astype(dt), Dd.astype(dt)
    t = np.uint64(time) + np.arange(n_out, dtype=np.uint64) * np.uint64(step)
    i = (t >> np.uint64(32)).astype(np.int64)
    f = t & np.uint64(0xffffffff)
    p = (f >> np.uint64(32 - lb)).astype(np.int64)
    r = (f & np.uint64((1 << (32 - lb)) - 1)).astype(np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        mu = r.astype(dt) * dt(2.0 ** -(32 - lb))  # the conversion rounds to nearest even; the scaling is exact
        linear = interp == "linear"
        y = np.zeros((channels, n_out), dtype=x.dtype)
        for c in range(channels):
            if cplx:
                y[c].real = _plane(Ht, Dt, np.ascontiguousarray(ext[c].real), Hn, i, p, mu, linear, dt)
                y[c].imag = _plane(Ht, Dt, np.ascontiguousarray(ext[c].imag), Hn, i, p, mu, linear, dt)
            else:
                y[c] = _plane(Ht, Dt, ext[c], Hn, i, p, mu, linear, dt)
    return y, state, next_time


def textbook(h, L, T, x, step, time, kernel=None):
    """sum over k of hc((k + f / 2^32) L) x[i - k] in double with zero history: hc is the piecewise-linear prototype (h followed by
    a zero, joined by straight lines), or `kernel`, a function of the real-valued tap position"""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    x = np.asarray(x)
    S = x.size
    n_out, _ = out_samples(int(step), int(time), S)
    hext = np.concatenate([h, [0.0]])
    ext = np.concatenate([np.zeros(T - 1, dtype=x.dtype), x])
    y = np.zeros(n_out, dtype=np.complex128 if np.iscomplexobj(x) else np.float64)
    for m in range(n_out):
        t = int(time) + m * int(step)
        i, f = t >> 32, t & 0xffffffff
        u = (np.arange(T) + f / 2.0 ** 32) * L
        w = kernel(u) if kernel else np.interp(u, np.arange(L * T + 1), hext)
        y[m] = np.dot(w, ext[T - 1 + i - np.arange(T)])
    return y


def hamming_sinc(L, T, max_ratio):
    """the continuous kernel sdsp_hip_arb_design samples: L firwin(L T, min(1, 1 / max_ratio) / L) as a function of a real tap position"""
    N = L * T
    cutoff = min(1.0, 1.0 / max_ratio) / L
    alpha = 0.5 * (N - 1)

    def v(u):
        return cutoff * np.sinc(cutoff * (u - alpha)) * (0.54 - 0.46 * np.cos(2 * np.pi * u / (N - 1)))

    scale = L / v(np.arange(N)).sum()
    return lambda u: scale * v(np.asarray(u, dtype=np.float64))
