"""CPU checks of the digital down-converter bank (include/sdsp_hip.h: sdsp_hip_ddc_*): the host helpers
against numpy, the numpy reference the GPU tests use (tests/ddc_ref.py) against the textbook form through scipy.signal.upfirdn,
block-wise streaming and the 2^32 periodicity of that reference, and plan creation without a device."""
import ctypes as C

import numpy as np
import pytest

from ddc_ref import BLOCKS, GRID_D, GRID_FCW, GRID_T, band_taps, ddc_ref, oscillator, phase_word, textbook

import simpledsp_amd as sd
from simpledsp_amd import _lib as L


def test_phase_word_is_the_rounded_scaled_frequency():
    rng = np.random.default_rng(1)
    for f in [0.0, 0.25, -0.25, 0.5, -0.5, 2.0 ** -33, 3 * 2.0 ** -33, *rng.uniform(-0.5, 0.5, 20)]:
        assert phase_word(f) == round(f * 2 ** 32) % 2 ** 32, f  # Python's round: ties to even, on an exact product
    assert phase_word(0.25) == 1 << 30 and phase_word(-0.25) == 3 << 30 and phase_word(0.5) == phase_word(-0.5) == 1 << 31
    lib = sd.load()
    w = C.c_uint32(7)
    for bad in (0.5000001, -0.6, float("nan"), float("inf")):
        assert lib.sdsp_hip_ddc_phase_word(bad, C.byref(w)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_ddc_phase_word(0.1, None) == L.ERR_INVALID_ARG
    assert sd.ddc_phase_word(0.25) == 1 << 30
    with pytest.raises(sd.SdspHipError):
        sd.ddc_phase_word(0.75)


def _unit(a):
    """e^(+2 pi i a / 2^32) of integer phase words with numpy's cos and sin on the library's exactly reduced angle: the quadrant from the
    top two bits, the rest folded to [0, pi / 4]"""
    a = np.asarray(a, dtype=np.int64)
    quad, r = a >> 30, a & 0x3fffffff
    low = r <= 0x20000000
    t = 2 * np.pi / 2.0 ** 32 * np.where(low, r, 0x40000000 - r)
    c = np.where(low, np.cos(t), np.sin(t))
    s = np.where(low, np.sin(t), np.cos(t))
    re = np.choose(quad, [c, -s, -c, s])
    im = np.choose(quad, [s, c, -s, -c])
    return re, im


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_oscillator_tables_against_numpy():
    c, f = oscillator()
    a = np.arange(65536)
    for tab, words in ((c, a << 16), (f, a)):
        re, im = _unit(words)
        assert _ulps(tab[:, 0], re).max() <= 2 and _ulps(tab[:, 1], -im).max() <= 2
    # the axes are exact, and |w| = 1 to rounding everywhere
    assert tuple(c[0]) == (1.0, 0.0) and tuple(c[16384]) == (0.0, -1.0) and tuple(c[32768]) == (-1.0, 0.0) and tuple(c[49152]) == (0.0, 1.0)
    assert not np.signbit(c[32768, 1])  # (-1, +0): what test_gpu_ddc's fcw = 2^31 case relies on
    assert np.abs(np.hypot(c[:, 0], c[:, 1]) - 1).max() < 3e-16 and np.abs(np.hypot(f[:, 0], f[:, 1]) - 1).max() < 3e-16
    assert sd.load().sdsp_hip_ddc_oscillator(None, f.ctypes.data) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("fcw", GRID_FCW + [1, 0x40000000, 0xdeadbeef])
def test_band_taps_against_numpy(fcw):
    rng = np.random.default_rng(fcw % 1000)
    h = rng.standard_normal(255)
    g = band_taps(h, fcw)
    re, im = _unit((np.arange(255, dtype=np.int64) * fcw) % 2 ** 32)
    assert _ulps(g[:, 0], h * re)[re != 0].max(initial=0) <= 2 and _ulps(g[:, 1], h * im)[im != 0].max(initial=0) <= 2
    assert np.all(g[re == 0, 0] == 0) and np.all(g[im == 0, 1] == 0)
    lib = sd.load()
    assert lib.sdsp_hip_ddc_band_taps(0, h.ctypes.data, fcw, g.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_ddc_band_taps(4097, h.ctypes.data, fcw, g.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_ddc_band_taps(255, None, fcw, g.ctypes.data) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("down", GRID_D)
@pytest.mark.parametrize("taps", GRID_T)
def test_reference_against_the_textbook_form(taps, down):
    """f64 within 1e-12 sum|h| max|x| of mix -> upfirdn, f32 within 1e-6 normwise (max error over max magnitude); the margins are in
    DESIGN.md section 5.19"""
    rng = np.random.default_rng(taps * 131 + down)
    S = down * (40 + -(-taps // down))  # at least T + 40 D samples: every tap meets the block in every cell
    h = rng.standard_normal(taps)
    for cplx in (False, True):
        x = rng.standard_normal(S) + (1j * rng.standard_normal(S) if cplx else 0)
        for fcw in GRID_FCW:
            phase0 = int(rng.integers(0, 1 << 32))
            position = int(rng.integers(0, 1 << 20)) * down
            want = textbook(h, x, down, fcw, phase0, position)
            y64, _ = ddc_ref(h, x, down, [(0, fcw, phase0)], position, None, "f64")
            e64 = np.abs(y64[0] - want).max() / (np.abs(h).sum() * np.abs(x).max())
            x32 = x.astype(np.complex64 if cplx else np.float32)
            want32 = textbook(h.astype(np.float32), x32, down, fcw, phase0, position)
            y32, _ = ddc_ref(h, x32, down, [(0, fcw, phase0)], position, None, "f32")
            e32 = np.abs(y32[0] - want32).max() / np.abs(want32).max()
            print(f"T {taps} D {down} cplx {cplx} fcw {fcw:#x}: f64 {e64:.2e} of 1e-12, f32 {e32:.2e} of 1e-6")
            assert e64 <= 1e-12
            assert e32 <= 1e-6


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True])
def test_reference_blockwise_equals_one_call(precision, cplx):
    rng = np.random.default_rng(7)
    for taps, down in [(1, 3), (17, 4), (64, 1), (255, 16)]:
        blocks = [b * down for b in BLOCKS]
        S = sum(blocks)
        x = rng.standard_normal((2, S)) + (1j * rng.standard_normal((2, S)) if cplx else 0)
        hist0 = rng.standard_normal((2, taps - 1)) + (1j * rng.standard_normal((2, taps - 1)) if cplx else 0)
        h = rng.standard_normal(taps)
        bands = [(0, 0x12345678, 99), (1, GRID_FCW[3], 0), (0, 0, 1 << 31)]
        pos0 = 12345 * down
        want, want_state = ddc_ref(h, x, down, bands, pos0, hist0, precision)
        got, state, s0 = [], hist0, 0
        for b in blocks:
            y, state = ddc_ref(h, x[:, s0:s0 + b], down, bands, pos0 + s0, state, precision)
            got.append(y)
            s0 += b
        assert np.array_equal(np.concatenate(got, axis=1), want)
        assert np.array_equal(state, want_state)


def test_reference_position_is_periodic_in_2_to_the_32():
    rng = np.random.default_rng(3)
    h, x = rng.standard_normal(17), rng.standard_normal((1, 64))
    bands = [(0, 0x12345678, 5), (0, GRID_FCW[3], 0)]
    for position in (0, 2 ** 32 - 12, 4 * 1000):
        a, _ = ddc_ref(h, x, 4, bands, position, None, "f32")
        b, _ = ddc_ref(h, x, 4, bands, position + 2 ** 32, None, "f32")
        assert np.array_equal(a, b)


def test_out_samples():
    lib = sd.load()
    n = C.c_uint64(0)
    for down, S, want in [(1, 0, 0), (4, 4032, 1008), (50, 150, 3), (1024, 1 << 40, 1 << 30)]:
        assert lib.sdsp_hip_ddc_out_samples(down, S, C.byref(n)) == 0 and n.value == want
    assert lib.sdsp_hip_ddc_out_samples(4, 4030, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_ddc_out_samples(0, 4, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_ddc_out_samples(1025, 1025, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_ddc_out_samples(4, 8, None) == L.ERR_INVALID_ARG


def test_bank_arguments():
    b = sd.ddc_bank(64, 4, [(0, 0.25), (1, -0.25, 0.5), (0, 0x12345678, 7)], channels=2)
    assert b.bands == [(0, 1 << 30, 0), (1, 3 << 30, 1 << 31), (0, 0x12345678, 7)]
    assert b.out_samples(64) == 16 and b.hist == 63 and b.position == 0
    with pytest.raises(sd.SdspHipError):
        b.out_samples(65)
    b.set_antialias_coeff()
    import scipy.signal
    assert np.abs(b.m_coeff - scipy.signal.firwin(64, 1.0 / 4)).max() < 1e-15
    for bad in (-1, 2):
        with pytest.raises(ValueError):
            b.set_variant(bad)
    with pytest.raises(ValueError):
        sd.ddc_bank(64, 4, [(2, 0.1)], channels=2)
    with pytest.raises(ValueError):
        sd.ddc_bank(64, 4, [], channels=2)
    with pytest.raises(ValueError):
        sd.ddc_bank(64, 4, [(0, 0.1)], kind="imaginary")
    with pytest.raises(ValueError):
        sd.ddc_bank(64, 4, [(0, 1 << 32)])


def test_plan_needs_a_device_and_says_so():
    """no CPU fallback: without a usable device, creation fails loudly (with one, it must succeed); the argument errors come first"""
    import torch
    lib = sd.load()
    h = np.ones(64)
    bands = (L.DdcBand * 2)(L.DdcBand(0, 5, 0), L.DdcBand(1, 6, 0))
    bp = C.cast(bands, C.c_void_p)
    p = C.c_void_p()
    create = lambda taps, hp, down, channels, nb, b, kind, prec: lib.sdsp_hip_ddc_plan_create(  # noqa: E731
        C.byref(p), taps, hp, down, channels, nb, b, kind, prec, 0)
    assert create(0, h.ctypes.data, 4, 2, 2, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_SIZE
    assert create(4097, h.ctypes.data, 4, 2, 2, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_SIZE
    assert create(64, h.ctypes.data, 0, 2, 2, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_SIZE
    assert create(64, h.ctypes.data, 1025, 2, 2, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_SIZE
    assert create(64, h.ctypes.data, 4, 0, 2, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_SIZE
    assert create(64, h.ctypes.data, 4, 2, 0, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_SIZE
    assert create(64, h.ctypes.data, 4, 2, 65537, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_SIZE
    assert create(64, None, 4, 2, 2, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_ARG
    assert create(64, h.ctypes.data, 4, 2, 2, None, L.DDC_REAL, L.F32) == L.ERR_INVALID_ARG
    assert create(64, h.ctypes.data, 4, 1, 2, bp, L.DDC_REAL, L.F32) == L.ERR_INVALID_ARG  # src = 1 >= channels
    assert create(64, h.ctypes.data, 4, 2, 2, bp, 2, L.F32) == L.ERR_INVALID_ARG
    assert create(64, h.ctypes.data, 4, 2, 2, bp, L.DDC_REAL, L.F32_F64STATE) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_ddc_plan_create(None, 64, h.ctypes.data, 4, 2, 2, bp, L.DDC_REAL, L.F32, 0) == L.ERR_INVALID_ARG
    rc = create(64, h.ctypes.data, 4, 2, 2, bp, L.DDC_COMPLEX, L.F64)
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_ddc_plan_destroy(p)
    else:
        assert rc == L.ERR_NO_DEVICE
