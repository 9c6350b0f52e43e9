"""numpy reference of the LMS / NLMS adaptive filter bank (include/sdsp_hip.h: sdsp_hip_lms_*) in exactly the
contract's operation order, vectorised over the channels with a Python loop over samples and taps, and what the LMS tests share.

mu and eps are host doubles rounded here with the precision's type, as the library rounds them, so the reference needs no device.  f64
follows the order literally (numpy never contracts).  f32: products, sums and quotients are np.float32 arithmetic (each correctly
rounded); one fmaf is the exact float64 product (24 x 24 bits fit) added to the accumulator with a single rounding to f32 -- the float64
sum is made round-to-odd from its exact error term first, so that the second rounding, to f32, cannot differ from one rounding of the
exact value (53 bits >= 24 + 2): the construction of tests/beam_ref.py, written out again here."""
import numpy as np

BLOCKS = [0, 1, 3, 0, 7, 1, 11]  # beam_ref.py's split pattern, in units the test chooses; empty calls included


def real_dtype(precision):
    return np.float64 if precision == "f64" else np.float32


def row_dtype(precision, cplx):
    if cplx:
        return np.complex128 if precision == "f64" else np.complex64
    return real_dtype(precision)


def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: exact product, one rounding"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = c + p
        bb = s - c
        err = (c - (s - bb)) + (p - bb)  # TwoSum: s + err = c + p exactly
        bits = s.view(np.int64)
        fix = (err != 0) & np.isfinite(s) & ((bits & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)  # round to odd
    return s.astype(np.float32)


def _mul_add(g, x, z):
    """z = g x + z"""
    if z.dtype == np.float32:
        return _fma32(g, x, z)
    with np.errstate(invalid="ignore", over="ignore"):
        return z + g * x


def _mul_sub(g, x, z):
    """z = -(g x) + z"""
    if z.dtype == np.float32:
        return _fma32(-g, x, z)
    with np.errstate(invalid="ignore", over="ignore"):
        return z - g * x


def lms_ref(x, d, n_taps, mu, mode="lms", eps=0.0, weights=None, hist=None, precision="f64"):
    """x, d: (channels, S) real or complex; weights: (channels, n_taps) or None for zero weights; hist: (channels, n_taps - 1) newest
    first or None for zero history.  Returns (y, e, weights, history): the a-priori output and error (channels, S), the final weights and
    the final history, all of x's kind in the precision."""
    x = np.atleast_2d(np.asarray(x))
    d = np.atleast_2d(np.asarray(d))
    cplx = np.iscomplexobj(x) or np.iscomplexobj(d) or (weights is not None and np.iscomplexobj(weights))
    dt = real_dtype(precision)
    rt = row_dtype(precision, cplx)
    x, d = x.astype(rt), d.astype(rt)
    C, S = x.shape
    T = n_taps
    assert d.shape == (C, S) and mode in ("lms", "nlms")
    mu, eps = dt(mu), dt(eps)
    w = np.zeros((C, T), dtype=rt) if weights is None else np.array(weights).astype(rt).reshape(C, T)
    h = np.zeros((C, T - 1), dtype=rt) if hist is None else np.asarray(hist).astype(rt).reshape(C, T - 1)
    ext = np.concatenate([h[:, ::-1], x], axis=1)  # ext[:, T - 1 + n] = x[n]
    wr, wi = np.ascontiguousarray(w.real).astype(dt), np.ascontiguousarray(w.imag).astype(dt)
    xr, xi = np.ascontiguousarray(ext.real).astype(dt), np.ascontiguousarray(ext.imag).astype(dt)
    dr, di = np.ascontiguousarray(d.real).astype(dt), np.ascontiguousarray(d.imag).astype(dt)
    y = np.zeros((C, S), dtype=rt)
    e = np.zeros((C, S), dtype=rt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for n in range(S):
            yr, yi, p = np.zeros(C, dtype=dt), np.zeros(C, dtype=dt), np.zeros(C, dtype=dt)  # +0
            for t in range(T):
                vr = xr[:, T - 1 + n - t]
                if cplx:
                    vi = xi[:, T - 1 + n - t]
                    yr = _mul_add(wr[:, t], vr, yr)
                    yr = _mul_sub(wi[:, t], vi, yr)
                    yi = _mul_add(wr[:, t], vi, yi)
                    yi = _mul_add(wi[:, t], vr, yi)
                else:
                    yr = _mul_add(wr[:, t], vr, yr)
            er = dr[:, n] - yr
            ei = di[:, n] - yi if cplx else yi
            gr = mu * er
            gi = mu * ei if cplx else ei
            if mode == "nlms":
                for t in range(T):
                    vr = xr[:, T - 1 + n - t]
                    p = _mul_add(vr, vr, p)
                    if cplx:
                        vi = xi[:, T - 1 + n - t]
                        p = _mul_add(vi, vi, p)
                q = eps + p
                gr = gr / q
                if cplx:
                    gi = gi / q
            assert gr.dtype == dt and er.dtype == dt
            for t in range(T):
                vr = xr[:, T - 1 + n - t]
                if cplx:
                    vi = xi[:, T - 1 + n - t]
                    wr[:, t] = _mul_add(gr, vr, wr[:, t])
                    wr[:, t] = _mul_add(gi, vi, wr[:, t])
                    wi[:, t] = _mul_add(gi, vr, wi[:, t])
                    wi[:, t] = _mul_sub(gr, vi, wi[:, t])
                else:
                    wr[:, t] = _mul_add(gr, vr, wr[:, t])
            if cplx:
                y[:, n].real, y[:, n].imag = yr, yi
                e[:, n].real, e[:, n].imag = er, ei
            else:
                y[:, n], e[:, n] = yr, er
    if cplx:
        w_out = np.empty((C, T), dtype=rt)
        w_out.real, w_out.imag = wr, wi
    else:
        w_out = wr
    return y, e, w_out, ext[:, ::-1][:, :T - 1].copy()


def lms_ref_stream(x, d, n_taps, calls, mode="lms", eps=0.0, weights=None, hist=None, precision="f64"):
    """the reference fed call by call: calls = [(samples, mu)]; returns (y, e, weights, history) with y, e over all the calls"""
    ys, es, s0 = [], [], 0
    for n, mu in calls:
        y, e, weights, hist = lms_ref(x[:, s0:s0 + n], d[:, s0:s0 + n], n_taps, mu, mode, eps, weights, hist, precision)
        ys.append(y)
        es.append(e)
        s0 += n
    return np.concatenate(ys, axis=1), np.concatenate(es, axis=1), weights, hist
