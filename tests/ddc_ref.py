"""numpy reference of the digital down-converter bank (include/sdsp_hip.h: sdsp_hip_ddc_*) in exactly the
contract's operation order, and the grids the DDC tests share.

The band taps and the oscillator tables come from the library's host helpers (doubles) and are rounded here with astype, as the plan
rounds them, so the reference needs no device and does not rely on two libm's agreeing.  f64 follows the order literally (numpy never
contracts).  f32: one fmaf is the exact float64 product (24 x 24 bits fit) added to the accumulator with a single rounding to f32 --
the float64 sum is made round-to-odd from its exact error term first, so that the second rounding, to f32, cannot differ from one
rounding of the exact value (53 bits >= 24 + 2)."""
import ctypes as C

import numpy as np

import simpledsp_amd as sd

GRID_T = [1, 17, 64, 255]
GRID_D = [1, 3, 4, 16, 50]
GRID_FCW = [0, 1 << 31, 0x12345678, (1 << 32) - 0x01000001]
BLOCKS = [0, 1, 3, 0, 7, 1, 11]  # in units of D


def real_dtype(precision):
    return np.float64 if precision == "f64" else np.float32


def band_taps(h, fcw):
    """the library's g[k] = h[k] e^(+2 pi i (k fcw mod 2^32) / 2^32) as a (T, 2) double array, before rounding"""
    h = np.ascontiguousarray(h, dtype=np.float64)
    g = np.zeros((h.size, 2))
    assert sd.load().sdsp_hip_ddc_band_taps(h.size, h.ctypes.data, int(fcw), g.ctypes.data) == 0
    return g


_TABLES = None


def oscillator():
    """(C, F): the library's two (65536, 2) double tables, before rounding"""
    global _TABLES
    if _TABLES is None:
        c, f = np.zeros((65536, 2)), np.zeros((65536, 2))
        assert sd.load().sdsp_hip_ddc_oscillator(c.ctypes.data, f.ctypes.data) == 0
        _TABLES = (c, f)
    return _TABLES


def phase_word(f):
    w = C.c_uint32(0)
    assert sd.load().sdsp_hip_ddc_phase_word(float(f), C.byref(w)) == 0
    return w.value


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
        return _fma32(g, x, z)
    return z + g * x


def _mul_sub(g, x, z, dt):
    if dt == np.float32:
        return _fma32(-g, x, z)
    return z - g * x


def _cmul(ar, ai, br, bi):
    """a (x) b: two products and one sum or difference, each rounded on its own (numpy never contracts)"""
    return ar * br - ai * bi, ar * bi + ai * br


def ddc_ref(h, x, down, bands, position=0, hist=None, precision="f64"):
    """x: (channels, S) real or complex input, S a multiple of down; bands: [(src, fcw, phase0)] with integer phase words; hist:
    (channels, T - 1) newest first, or None for zero history.  Returns (y, state): y (bands, S / down) complex of the precision, state
    (channels, T - 1) of the input kind."""
    dt = real_dtype(precision)
    cdt = np.complex128 if precision == "f64" else np.complex64
    x = np.atleast_2d(np.asarray(x))
    cplx = np.iscomplexobj(x)
    x = x.astype(cdt if cplx else dt)
    channels, S = x.shape
    T = len(h)
    H = T - 1
    assert S % down == 0
    M = S // down
    if hist is None:
        hist = np.zeros((channels, H), dtype=x.dtype)
    hist = np.asarray(hist).astype(x.dtype).reshape(channels, H)
    ext = np.concatenate([hist[:, ::-1], x], axis=1)  # ext[:, H + n] = x[n]
    state = ext[:, ::-1][:, :H].copy()
    Cd, Fd = oscillator()
    Ct, Ft = Cd.astype(dt), Fd.astype(dt)
    y = np.zeros((len(bands), M), dtype=cdt)
    n = np.arange(M, dtype=np.int64) * down
    for i, (src, fcw, phase0) in enumerate(bands):
        g = band_taps(h, fcw).astype(dt)
        zr, zi = np.zeros(M, dtype=dt), np.zeros(M, dtype=dt)
        for k in range(T):
            xk = ext[src, H + n - k]
            gr, gi = np.full(M, g[k, 0], dtype=dt), np.full(M, g[k, 1], dtype=dt)
            if cplx:
                xr, xi = xk.real.astype(dt), xk.imag.astype(dt)
                zr = _mul_add(gr, xr, zr, dt)
                zr = _mul_sub(gi, xi, zr, dt)
                zi = _mul_add(gr, xi, zi, dt)
                zi = _mul_add(gi, xr, zi, dt)
            else:
                zr = _mul_add(gr, xk, zr, dt)
                zi = _mul_add(gi, xk, zi, dt)
        j = (int(phase0) + int(fcw) * ((int(position) + n.astype(object)))) % (1 << 32)  # exact integers
        j = np.array(j, dtype=np.int64)
        a, b = j >> 16, j & 0xffff
        with np.errstate(invalid="ignore", over="ignore"):
            wr, wi = _cmul(Ct[a, 0], Ct[a, 1], Ft[b, 0], Ft[b, 1])
            yr, yi = _cmul(zr, zi, wr, wi)
        y[i].real, y[i].imag = yr, yi
    return y, state


def textbook(h, x, down, fcw, phase0=0, position=0):
    """mix in double with an oscillator computed directly, FIR, keep every down-th sample: scipy.signal.upfirdn on the mixed stream
    (zero history), cut to S / down outputs"""
    import scipy.signal
    x = np.asarray(x)
    S = x.size
    n = np.arange(S, dtype=object) + int(position)
    j = np.array((int(phase0) + int(fcw) * n) % (1 << 32), dtype=np.float64)
    osc = np.exp(-2j * np.pi * j / 2.0 ** 32)
    full = scipy.signal.upfirdn(np.asarray(h, dtype=np.float64), x.astype(np.complex128) * osc, 1, down)
    return full[:S // down]
