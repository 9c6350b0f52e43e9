"""CPU-side checks of the column FFT plans: the numpy contract (tests/fft_cols_ref.py) against the oracle's radix-2 transform of the
transposed columns, the shift against numpy's fftshift, fft2 against numpy, and every argument error of sdsp_hip_fft_cols_* -- all of
which come back before a device is looked for; a valid plan then fails loudly without one (there is no CPU path)."""
import ctypes as C

import numpy as np
import pytest

import fft_cols_ref as ref

import simpledsp_amd as sd
from simpledsp_amd import _lib as L

NS = (8, 16, 32, 64, 128, 256, 512, 1024)


def _cube(rng, batch, n, width):
    return rng.standard_normal((batch, n, width)) + 1j * rng.standard_normal((batch, n, width))


@pytest.mark.parametrize("n", NS)
def test_reference_equals_the_oracle_on_transposed_columns(oracle, n):
    rng = np.random.default_rng(n)
    x = _cube(rng, 2, n, 5)
    for reverse in (False, True):
        want = oracle.fft(np.ascontiguousarray(x.transpose(0, 2, 1)), 2, reverse).transpose(0, 2, 1)
        got = ref.fft_cols(x, f64=True, reverse=reverse)
        assert ref.col_err(got, want, True) < 1e-12, (n, reverse)
    # the window multiplies before the transform, in the precision
    w = ref.hann(n)
    want = oracle.fft(np.ascontiguousarray((x * w[:, None]).transpose(0, 2, 1)), 2).transpose(0, 2, 1)
    assert ref.col_err(ref.fft_cols(x, f64=True, window=w), want, True) < 1e-12
    x32 = x.astype(np.complex64)
    w32 = w.astype(np.float32)
    v = ((x32.real * w32[:, None]) + 1j * (x32.imag * w32[:, None])).astype(np.complex64)  # rounded products
    assert np.array_equal(ref.windowed(x, w, False), v.astype(np.complex128))


@pytest.mark.parametrize("n", (8, 64, 1024))
def test_shift_is_fftshift_and_reverse_undoes_forward(n):
    rng = np.random.default_rng(3)
    x = _cube(rng, 2, n, 3)
    plain = ref.fft_cols(x, f64=True)
    shifted = ref.fft_cols(x, f64=True, shift=True)
    assert np.array_equal(shifted, np.fft.fftshift(plain, axes=-2))
    for k in (0, 1, n // 2, n - 1):
        assert np.array_equal(shifted[:, (k + n // 2) % n], plain[:, k])
    back = ref.fft_cols(shifted, f64=True, reverse=True, shift=True)
    assert np.abs(back - x).max() < 1e-12
    assert np.abs(ref.fft_cols(plain, f64=True, reverse=True) - x).max() < 1e-12
    p = ref.fft_cols(x, f64=True, shift=True, power=True)
    assert p.dtype == np.float64 and np.allclose(p, np.abs(shifted) ** 2, rtol=1e-14, atol=0)


def test_fft2_reference_equals_numpy():
    rng = np.random.default_rng(5)
    for n, m in ((8, 16), (64, 64), (32, 128)):
        x = _cube(rng, 3, n, m)
        assert np.abs(ref.fft2(x) - np.fft.fft2(x)).max() < 1e-11 * np.abs(np.fft.fft2(x)).max()
        assert np.abs(ref.fft2(x, reverse=True) - np.fft.ifft2(x)).max() < 1e-12


def _create(n, width, direction=L.FORWARD, precision=L.F32, output=L.FFT_COLS_COMPLEX, shift=0, window=None, out=True):
    lib = sd.load()
    h = C.c_void_p()
    w = None if window is None else np.ascontiguousarray(window, dtype=np.float64)
    rc = lib.sdsp_hip_fft_cols_plan_create(C.byref(h) if out else None, n, width, direction, precision, output, shift,
                                           None if w is None else w.ctypes.data, 0)
    assert h.value is None or rc == L.OK
    if h.value:
        lib.sdsp_hip_fft_cols_plan_destroy(h)
    return rc


def test_argument_errors_come_before_the_device():
    ok = (L.OK, L.ERR_NO_DEVICE)  # whatever machine this runs on, an argument error is never one of these
    assert _create(64, 33) in ok
    for n in (0, 1, 4, 12, 48, 100, 2048, 1 << 20):
        assert _create(n, 33) == L.ERR_INVALID_SIZE, n
    assert _create(64, 0) == L.ERR_INVALID_SIZE
    assert _create(64, (1 << 40) // 64) == L.ERR_INVALID_SIZE  # n width = 2^40
    assert _create(64, (1 << 40) // 64 - 1) in ok
    assert _create(64, 33, out=False) == L.ERR_INVALID_ARG
    for direction in (0, 2, -2):
        assert _create(64, 33, direction=direction) == L.ERR_INVALID_ARG
    for precision in (-1, L.F32_F64STATE, 3):
        assert _create(64, 33, precision=precision) == L.ERR_INVALID_ARG
    for output in (-1, 2):
        assert _create(64, 33, output=output) == L.ERR_INVALID_ARG
    w = ref.hann(64)
    assert _create(64, 33, direction=L.REVERSE, window=w) == L.ERR_INVALID_ARG
    assert _create(64, 33, direction=L.REVERSE, output=L.FFT_COLS_POWER) == L.ERR_INVALID_ARG
    for bad in (np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[17] = bad
        for precision in (L.F32, L.F64):
            assert _create(64, 33, precision=precision, window=wb) == L.ERR_INVALID_ARG
    wb = w.copy()
    wb[5] = 1e300  # finite in double, infinite once rounded to float
    assert _create(64, 33, precision=L.F32, window=wb) == L.ERR_INVALID_ARG
    assert _create(64, 33, precision=L.F64, window=wb) in ok
    # the null-plan forms of the other entries
    lib = sd.load()
    n = C.c_uint64(0)
    assert lib.sdsp_hip_fft_cols_plan_destroy(None) == L.OK
    assert lib.sdsp_hip_fft_cols_exec(None, None, None, 1, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_fft_cols_exec_host(None, None, None, 1) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_fft_cols_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_fft_cols_plan_launches(None, 1, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_fft_cols_plan_get_info(None, None) == L.ERR_INVALID_ARG


def test_every_valid_combination_needs_a_device():
    """without a device every valid combination is ERR_NO_DEVICE (there is no CPU path); with one, every one of them is a plan"""
    count = C.c_int(0)
    have = sd.load().sdsp_hip_device_count(C.byref(count)) == L.OK and count.value > 0
    want = L.OK if have else L.ERR_NO_DEVICE
    w = ref.hann(8)
    for n in NS:
        for precision in (L.F32, L.F64):
            for shift in (0, 1):
                assert _create(n, 17, L.REVERSE, precision, L.FFT_COLS_COMPLEX, shift) == want
                for output in (L.FFT_COLS_COMPLEX, L.FFT_COLS_POWER):
                    for window in (None, np.resize(w, n)):
                        assert _create(n, 17, L.FORWARD, precision, output, shift, window) == want
    if not have:
        with pytest.raises(sd.SdspHipError) as e:
            sd.FftColsPlan(64, 33)
        assert e.value.code == L.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        sd.FftColsPlan(64, 33, output="magnitude")
    with pytest.raises(ValueError):
        sd.FftColsPlan(64, 33, window=np.ones(63))
