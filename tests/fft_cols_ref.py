"""The contract of the column FFT plans (include/sdsp_hip.h: sdsp_hip_fft_cols_*) in numpy: what tests/test_gpu_fft_cols.py holds the
kernels to and tests/test_fft_cols_host.py holds to the oracle.  A plain module, not a conftest.

x: (batch, n, width) complex.  The window and the inputs are rounded to the precision and multiplied in that precision (one product
per component); the transform itself runs in complex128 along axis -2; then come the shift and the power."""
import numpy as np

EPS64 = np.finfo(np.float64).eps
TOL32 = 1e-6  # normwise, the row plans' (tests/test_gpu_fft.py)


def tol(n, f64):
    """f64: 4 n eps of max |X| of the column (tests/test_gpu_fft.py: _tol64); f32: TOL32"""
    return 4 * n * EPS64 if f64 else TOL32


def dtypes(f64):
    return (np.complex128, np.float64) if f64 else (np.complex64, np.float32)


def hann(n):
    """the periodic Hann window: zero at p = 0"""
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


def windowed(x, window, f64):
    """v[p] = x[p] w[p] in the precision, as complex128"""
    cplx, real = dtypes(f64)
    v = np.asarray(x).astype(cplx)
    if window is not None:
        w = np.asarray(window, dtype=np.float64).astype(real)[:, None]
        v = (v.real * w + 1j * (v.imag * w)).astype(cplx)  # two real products of the precision
    return v.astype(np.complex128)


def fft_cols(x, f64=False, reverse=False, window=None, shift=False, power=False):
    """(batch, n, width) -> the plan's output in double: complex128, or float64 for power"""
    assert not (reverse and (window is not None or power))
    v = windowed(x, window, f64)
    n = v.shape[-2]
    if reverse:
        if shift:
            v = np.roll(v, -(n // 2), axis=-2)  # x[p] is read from row (p + n/2) mod n
        return np.fft.ifft(v, axis=-2)
    X = np.fft.fft(v, axis=-2)
    if shift:
        X = np.roll(X, n // 2, axis=-2)  # X[k] goes to row (k + n/2) mod n
    return X.real ** 2 + X.imag ** 2 if power else X


def fft2(x, reverse=False):
    """rows then columns, each a 1-D transform of the contract: what simpledsp_amd.fft2 / ifft2 compute"""
    a = np.asarray(x).astype(np.complex128)
    f = np.fft.ifft if reverse else np.fft.fft
    return f(f(a, axis=-1), axis=-2)


def col_err(got, want, f64):
    """the worst column's error in the tolerance's own metric: f64 max |d| / max |X| of the column, f32 normwise"""
    d = np.abs(np.asarray(got).astype(np.complex128) - want)
    if f64:
        den = np.abs(want).max(axis=-2)
        return float((d.max(axis=-2) / np.where(den == 0, 1.0, den)).max())
    den = np.sqrt((np.abs(want) ** 2).sum(axis=-2))
    return float((np.sqrt((d ** 2).sum(axis=-2)) / np.where(den == 0, 1.0, den)).max())


def power_excess(got, want_power, want_max, n, f64):
    """the worst |P - P_ref| in units of its bound (2 tol + tol^2) max |X|^2 + 4 ulp, which follows from |X - X_ref| <= tol max |X|;
    want_max: max |X| per column, (batch, 1, width)"""
    t = tol(n, f64)
    ulp = np.finfo(np.float64 if f64 else np.float32).eps
    bound = (2 * t + t * t) * want_max ** 2 + 4 * ulp * want_power
    return float((np.abs(np.asarray(got).astype(np.float64) - want_power) / bound).max())
