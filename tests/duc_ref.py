"""numpy reference of the digital up-converter bank (include/sdsp_hip.h: sdsp_hip_duc_*) in exactly the
contract's operation order, the textbook form it is pinned to, and the grids the DUC tests share.

The oscillator tables come from the library's host helper (doubles) and are rounded here with astype, as the plan rounds them; the
taps are rounded the same way.  f64 follows the order literally (numpy never contracts); f32 uses ddc_ref's _fma32, one rounding per
multiply-add."""
import numpy as np

from ddc_ref import GRID_FCW as DDC_FCW
from ddc_ref import _fma32, oscillator, phase_word, real_dtype  # noqa: F401  (phase_word: re-exported for the tests)

GRID_T = [1, 17, 64, 255]
GRID_U = [1, 3, 4, 16, 50, 96]  # 96: a wave of 64 consecutive outputs is shorter than one input step
GRID_FCW = DDC_FCW + [0x40000001]
BLOCKS = [0, 1, 3, 0, 7, 1, 11]  # input samples per band


def hist_len(taps, up):
    return (taps - 1) // up


def duc_ref(h, x, up, bands, channels, kind="complex", position=0, hist=None, precision="f64"):
    """x: (nb, S) complex input, row i = band i; bands: [(dst, fcw, phase0)] with integer phase words; hist: (nb, H) newest first, or
    None for zero history.  Returns (y, state): y (channels, S * up) complex, or real for kind "real", of the precision; state (nb, H)
    complex."""
    dt = real_dtype(precision)
    cdt = np.complex128 if precision == "f64" else np.complex64
    x = np.atleast_2d(np.asarray(x)).astype(cdt)
    nb, S = x.shape
    assert nb == len(bands)
    T = len(h)
    H = hist_len(T, up)
    if hist is None:
        hist = np.zeros((nb, H), dtype=cdt)
    hist = np.asarray(hist).astype(cdt).reshape(nb, H)
    ext = np.concatenate([hist[:, ::-1], x], axis=1)  # ext[:, H + m] = x[m]
    state = ext[:, ::-1][:, :H].copy()
    ht = np.asarray(h, dtype=np.float64).astype(dt)
    Cd, Fd = oscillator()
    Ct, Ft = Cd.astype(dt), Fd.astype(dt)
    R = S * up
    r = np.arange(R, dtype=np.int64)
    m, p = r // up, r % up
    n = (int(position) * up + r.astype(object)) % (1 << 32)  # exact integers
    acc_r = np.zeros((channels, R), dtype=dt)
    acc_i = np.zeros((channels, R), dtype=dt)
    for i, (dst, fcw, phase0) in enumerate(bands):  # ascending band index within every channel
        xr, xi = ext[i].real.astype(dt), ext[i].imag.astype(dt)
        zr, zi = np.zeros(R, dtype=dt), np.zeros(R, dtype=dt)
        for q in range(H + 1):
            k = q * up + p
            on = k < T  # a phase never gets a tap it does not have
            g = ht[np.where(on, k, 0)]
            xq_r, xq_i = xr[H + m - q], xi[H + m - q]
            if dt == np.float32:
                nr, ni = _fma32(g, xq_r, zr), _fma32(g, xq_i, zi)
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    nr, ni = zr + g * xq_r, zi + g * xq_i
            zr, zi = np.where(on, nr, zr), np.where(on, ni, zi)
        j = np.array((int(phase0) + int(fcw) * n) % (1 << 32), dtype=np.int64)
        a, b = j >> 16, j & 0xffff
        with np.errstate(invalid="ignore", over="ignore"):
            wr = Ct[a, 0] * Ft[b, 0] - Ct[a, 1] * Ft[b, 1]
            wi = -(Ct[a, 0] * Ft[b, 1] + Ct[a, 1] * Ft[b, 0])  # the conjugate: an exact sign flip
            acc_r[dst] = acc_r[dst] + (zr * wr - zi * wi)
            if kind == "complex":
                acc_i[dst] = acc_i[dst] + (zr * wi + zi * wr)
    if kind == "real":
        return acc_r, state
    y = np.zeros((channels, R), dtype=cdt)
    y.real, y.imag = acc_r, acc_i
    return y, state


def textbook(h, x, up, bands, channels, kind="complex", position=0):
    """scipy.signal.upfirdn(h, x, up) per band (zero history), zero-padded or cut to S * up outputs, times e^(+2 pi i j / 2^32)
    computed directly in double, summed per channel"""
    import scipy.signal
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    S = x.shape[1]
    R = S * up
    n = np.arange(R, dtype=object) + int(position) * up
    y = np.zeros((channels, R), dtype=np.complex128)
    for i, (dst, fcw, phase0) in enumerate(bands):
        full = scipy.signal.upfirdn(np.asarray(h, dtype=np.float64), x[i], up) if S else np.zeros(0, dtype=np.complex128)
        z = np.zeros(R, dtype=np.complex128)
        z[:min(R, full.size)] = full[:R]
        j = np.array((int(phase0) + int(fcw) * n) % (1 << 32), dtype=np.float64)
        y[dst] += z * np.exp(2j * np.pi * j / 2.0 ** 32)
    return y.real.copy() if kind == "real" else y
