"""numpy reference of the carrier-recovery PLL / Costas loop bank (include/sdsp_hip.h: sdsp_hip_pll_*) in
exactly the contract's operation order, vectorised over the channels with a Python loop over the samples, and what the PLL tests share.

The oscillator tables come from the library's host helper (doubles) and are rounded here with astype, as the plan rounds them, so the
reference needs no device and does not rely on two libm's agreeing.  alpha, beta and max_dev are host doubles rounded here with the
precision's type, as the library rounds them.  f64 follows the order literally (numpy never contracts); in f32 one fmaf is
lms_ref._fma32 (exact double product, round-to-odd sum, one rounding to f32)."""
import numpy as np

import simpledsp_amd as sd
from ddc_ref import _cmul
from lms_ref import BLOCKS, _fma32  # noqa: F401  (BLOCKS is re-exported for the tests)

MODES = ("cross", "bpsk", "qpsk")

_TABLES = None


def real_dtype(precision):
    return np.float64 if precision == "f64" else np.float32


def row_dtype(precision):
    return np.complex128 if precision == "f64" else np.complex64


def oscillator():
    """(C, F): the library's two (2048, 2) double tables, before rounding: C[a] = e^(-2 pi i a / 2^11), F[a] = e^(-2 pi i a / 2^22)"""
    global _TABLES
    if _TABLES is None:
        c, f = np.zeros((2048, 2)), np.zeros((2048, 2))
        assert sd.load().sdsp_hip_pll_oscillator(c.ctypes.data, f.ctypes.data) == 0
        _TABLES = (c, f)
    return _TABLES


def _ma(a, b, c):
    """ma(a, b, c) = a b + c: one fmaf in f32, a multiply then an add in f64"""
    if c.dtype == np.float32:
        return _fma32(np.broadcast_to(a, c.shape), b, c)
    return a * b + c


def _flip_sign_where_negative(v, s):
    """v with its sign bit flipped where the sign bit of s is set: bit operations, -0 counts as negative"""
    u = np.uint64 if v.dtype == np.float64 else np.uint32
    top = u(1) << u(8 * v.dtype.itemsize - 1)
    return (v.view(u) ^ (s.view(u) & top)).view(v.dtype)


def pll_ref(x, fcw0, alpha, beta, mode="cross", max_dev=0.5, integ=None, theta=None, precision="f64"):
    """x: (channels, S) complex; fcw0: uint32 words, (channels,) or one shared word; integ: (channels,) reals or None for zeros;
    theta: (channels,) uint32 or None for zeros.  Returns (y, err, freq, integ, theta): the de-rotated rows (channels, S) complex, the
    detector output and the integrator (channels, S) real, and the final state."""
    assert mode in MODES
    dt, rt = real_dtype(precision), row_dtype(precision)
    x = np.atleast_2d(np.asarray(x)).astype(rt)
    C, S = x.shape
    fcw = np.broadcast_to(np.asarray(fcw0, dtype=np.uint32).reshape(-1), (C,)).astype(np.int64)
    alpha, beta, dev = dt(alpha), dt(beta), dt(max_dev)
    integ = np.zeros(C, dtype=dt) if integ is None else np.array(integ, dtype=dt).reshape(C)
    th = np.zeros(C, dtype=np.int64) if theta is None else np.array(theta, dtype=np.uint32).reshape(C).astype(np.int64)
    Cd, Fd = oscillator()
    Ct, Ft = Cd.astype(dt), Fd.astype(dt)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    y = np.zeros((C, S), dtype=rt)
    err, freq = np.zeros((C, S), dtype=dt), np.zeros((C, S), dtype=dt)
    lo, hi = dt(-2.0 ** 31), dt(2.0 ** 31 - (128 if precision == "f32" else 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(S):
            a, b = th >> 21, (th >> 10) & 0x7ff
            wr, wi = _cmul(Ct[a, 0], Ct[a, 1], Ft[b, 0], Ft[b, 1])
            yr, yi = _cmul(xr[:, n], xi[:, n], wr, wi)
            if mode == "cross":
                e = yi
            elif mode == "bpsk":
                e = yr * yi
            else:
                e = _flip_sign_where_negative(yi, yr) - _flip_sign_where_negative(yr, yi)
            integ = _ma(beta, e, integ)
            integ = np.where(integ < -dev, -dev, np.where(integ > dev, dev, integ))
            v = _ma(alpha, e, integ)
            t = v * dt(2.0 ** 32)
            t = np.where(t < lo, lo, np.where(t > hi, hi, t))
            t = np.where(np.isnan(t), dt(0), t)
            assert t.dtype == dt and e.dtype == dt and integ.dtype == dt
            th = (th + fcw + np.rint(t).astype(np.int64)) & 0xffffffff
            y[:, n].real, y[:, n].imag = yr, yi
            err[:, n], freq[:, n] = e, integ
    return y, err, freq, integ, th.astype(np.uint32)


def pll_ref_stream(x, fcw0, calls, mode="cross", max_dev=0.5, integ=None, theta=None, precision="f64"):
    """the reference fed call by call: calls = [(samples, alpha, beta)]; returns what pll_ref returns, over all the calls"""
    ys, es, fs, s0 = [], [], [], 0
    for n, alpha, beta in calls:
        y, e, f, integ, theta = pll_ref(x[:, s0:s0 + n], fcw0, alpha, beta, mode, max_dev, integ, theta, precision)
        ys.append(y)
        es.append(e)
        fs.append(f)
        s0 += n
    return np.concatenate(ys, axis=1), np.concatenate(es, axis=1), np.concatenate(fs, axis=1), integ, theta


# ---- the lock test's signals (tests/test_pll_host.py on the reference, tests/test_gpu_pll.py on the device)
LOCK_CHANNELS, LOCK_SAMPLES, LOCK_TAIL, LOCK_F0, LOCK_NOISE = 8, 6000, 1000, 0.1, 0.05
LOCK_ORDER = {"cross": 1, "bpsk": 2, "qpsk": 4}


def lock_signal(mode, bn, seed=0):
    """(x, sym, df): LOCK_CHANNELS carriers at LOCK_F0 + df cycles per sample, df uniform in +-0.4 bn, random start phase, unit
    amplitude, the mode's symbols (one per sample) and complex Gaussian noise of LOCK_NOISE per component; complex128"""
    rng = np.random.default_rng(1000 * MODES.index(mode) + int(round(bn * 1e4)) + seed)
    C, S = LOCK_CHANNELS, LOCK_SAMPLES
    df = rng.uniform(-0.4 * bn, 0.4 * bn, C)
    ph = rng.uniform(0.0, 2 * np.pi, C)
    if mode == "cross":
        sym = np.ones((C, S), dtype=np.complex128)
    elif mode == "bpsk":
        sym = (2.0 * rng.integers(0, 2, (C, S)) - 1.0).astype(np.complex128)
    else:
        sym = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, (C, S))))
    n = np.arange(S)
    x = sym * np.exp(1j * (2 * np.pi * (LOCK_F0 + df)[:, None] * n + ph[:, None]))
    x = x + LOCK_NOISE * (rng.standard_normal((C, S)) + 1j * rng.standard_normal((C, S)))
    return x, sym, df


def lock_figures(mode, y, freq, sym, df):
    """(max |mean(freq) - df|, max |angle(mean((y / sym)^M))|) over the last LOCK_TAIL samples, in double"""
    M = LOCK_ORDER[mode]
    tail = slice(LOCK_SAMPLES - LOCK_TAIL, LOCK_SAMPLES)
    f = np.abs(freq[:, tail].astype(np.float64).mean(axis=1) - df).max()
    z = (y[:, tail].astype(np.complex128) / sym[:, tail]) ** M
    return f, np.abs(np.angle(z.mean(axis=1))).max()
