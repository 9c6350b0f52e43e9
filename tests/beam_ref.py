"""numpy reference of the time-delay beamformer bank (include/sdsp_hip.h: sdsp_hip_beam_*) in exactly the
contract's operation order, and what the beamformer tests share.

Taps are host doubles rounded here with astype, as the plan rounds them, so the reference needs no device.  f64 follows the order
literally (numpy never contracts).  f32: one fmaf is the exact float64 product (24 x 24 bits fit) added to the accumulator with a single
rounding to f32 -- the float64 sum is made round-to-odd from its exact error term first, so that the second rounding, to f32, cannot
differ from one rounding of the exact value (53 bits >= 24 + 2): the construction of tests/ddc_ref.py, written out again here."""
import numpy as np

BLOCKS = [0, 1, 3, 0, 7, 1, 11]  # a split pattern, in units the test chooses; an empty call included


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


def _mul_add(g, x, z, dt):
    if dt == np.float32:
        return _fma32(np.full(x.shape, g, dtype=dt), x, z)
    with np.errstate(invalid="ignore", over="ignore"):
        return z + g * x


def _mul_sub(g, x, z, dt):
    if dt == np.float32:
        return _fma32(np.full(x.shape, -g, dtype=dt), x, z)
    with np.errstate(invalid="ignore", over="ignore"):
        return z - g * x


def hist_len(entries, n_taps):
    return max([int(e[2]) for e in entries], default=0) + n_taps - 1


def beam_ref(entries, x, sensors, beams, n_taps, groups=1, hist=None, precision="f64"):
    """entries: [(beam, sensor, delay, taps)] in the contract's order; x: (groups * sensors, S) real or complex; hist:
    (groups * sensors, H) newest first with H = max delay + n_taps - 1, or None for zero history.  Returns (y, state): y
    (groups * beams, S) and state (groups * sensors, H), both of x's kind in the precision."""
    x = np.atleast_2d(np.asarray(x))
    cplx = np.iscomplexobj(x)
    dt = real_dtype(precision)
    x = x.astype(row_dtype(precision, cplx))
    rows, S = x.shape
    assert rows == groups * sensors
    H = hist_len(entries, n_taps)
    if hist is None:
        hist = np.zeros((rows, H), dtype=x.dtype)
    hist = np.asarray(hist).astype(x.dtype).reshape(rows, H)
    ext = np.concatenate([hist[:, ::-1], x], axis=1)  # ext[:, H + n] = x[n]
    state = ext[:, ::-1][:, :H].copy()
    y = np.zeros((groups * beams, S), dtype=x.dtype)
    n = np.arange(S, dtype=np.int64)
    for grp in range(groups):
        zr = np.zeros((beams, S), dtype=dt)  # +0
        zi = np.zeros((beams, S), dtype=dt)
        for (b, c, d, g) in entries:
            g = np.asarray(g).reshape(-1)
            assert g.size == n_taps
            gr = g.real.astype(dt)
            gi = g.imag.astype(dt) if cplx else None
            for t in range(n_taps):
                xk = ext[grp * sensors + c, H + n - int(d) - t]
                if cplx:
                    xr, xi = xk.real.astype(dt), xk.imag.astype(dt)
                    zr[b] = _mul_add(gr[t], xr, zr[b], dt)
                    zr[b] = _mul_sub(gi[t], xi, zr[b], dt)
                    zi[b] = _mul_add(gr[t], xi, zi[b], dt)
                    zi[b] = _mul_add(gi[t], xr, zi[b], dt)
                else:
                    zr[b] = _mul_add(gr[t], xk, zr[b], dt)
        if cplx:
            y[grp * beams:(grp + 1) * beams].real = zr
            y[grp * beams:(grp + 1) * beams].imag = zi
        else:
            y[grp * beams:(grp + 1) * beams] = zr
    return y, state


def delay_taps_formula(tau, weight, n_taps, beta):
    """the contract's designer in numpy (np.sinc, np.i0): (delay, taps)"""
    if n_taps == 1:
        return int(np.floor(tau + 0.5)), np.array([float(weight)])
    d = int(np.floor(tau))
    mu = tau - d
    c0 = (n_taps - 1) // 2
    u = np.arange(n_taps) - c0 - mu
    w = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (u / ((n_taps + 1) / 2.0)) ** 2))) / np.i0(beta)
    g = np.sinc(u) * w
    return d, g / g.sum() * weight


def response(g, f):
    """H(f) = sum g[t] e^(-2 pi i f t) for an array of frequencies in cycles per sample"""
    t = np.arange(len(g))
    return np.exp(-2j * np.pi * np.outer(np.atleast_1d(f), t)) @ np.asarray(g, dtype=np.float64)
