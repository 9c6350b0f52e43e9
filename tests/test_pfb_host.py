"""CPU checks of the polyphase filter-bank channelizer bank (include/sdsp_hip.h: sdsp_hip_pfb_*): the numpy
reference the GPU tests use against torch.stft(n_fft = L, center=False)[k P] and, for the TIME phase, against the direct sum with
absolute-index phases; block-wise streaming of that reference; the prototype against scipy.signal.firwin; the frame-count rule, state
bytes, plan creation without a device, and the store-hazard scan of pfb.hip."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal
import torch

from conftest import ROOT
from pfb_ref import pfb_ref
from stft_ref import stft_ref

import simpledsp_amd as sd

# (M, P, D): P = 1, D dividing M, D not dividing M, D = 1
SHAPES = [(16, 4, 16), (32, 1, 32), (32, 1, 8), (32, 3, 24), (64, 8, 32), (64, 2, 1), (256, 4, 192), (1024, 4, 1024), (1024, 3, 768)]


def _signal(rng, n, cplx):
    x = rng.standard_normal(n)
    return x + 1j * rng.standard_normal(n) if cplx else x


@pytest.mark.parametrize("m,p,hop", SHAPES)
@pytest.mark.parametrize("cplx", [False, True])
def test_reference_frame_phase_is_every_pth_bin_of_the_long_stft(m, p, hop, cplx):
    rng = np.random.default_rng(m * 131 + p * 7 + hop)
    Lt = m * p
    S = hop * max(3, -(-2 * Lt // hop))
    x = _signal(rng, S, cplx)
    h = rng.standard_normal(Lt)
    hist = _signal(rng, Lt - hop, cplx)
    for hh in (hist, None):
        y, _ = pfb_ref(x, m, p, hop, h, hh, phase="frame")
        full = np.concatenate([(hist if hh is not None else np.zeros_like(hist))[::-1], x])
        want = torch.stft(torch.from_numpy(full), Lt, hop, window=torch.from_numpy(h), center=False, return_complex=True,
                          onesided=not cplx).numpy().T
        want = want[:, ::p][:, :y.shape[1]]
        assert y.shape == want.shape == (S // hop, m if cplx else m // 2 + 1)
        assert np.abs(y - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("m,hop", [(32, 32), (32, 8), (64, 1), (256, 192)])
def test_reference_with_one_tap_per_channel_is_the_stft_reference(m, hop):
    rng = np.random.default_rng(m + hop)
    S = 5 * hop * (m // hop + 1)
    x = rng.standard_normal((2, S))
    h = rng.standard_normal(m)
    hist = rng.standard_normal((2, m - hop))
    y, st = pfb_ref(x, m, 1, hop, h, hist, phase="frame")
    want, want_st = stft_ref(x, m, hop, h, hist)
    assert np.array_equal(y, want) and np.array_equal(st, want_st)


@pytest.mark.parametrize("m,p,hop", [s for s in SHAPES if s[0] <= 256] + [(1024, 2, 768)])
@pytest.mark.parametrize("cplx", [False, True])
def test_reference_time_phase_is_the_direct_sum_with_absolute_phases(m, p, hop, cplx):
    """Y_j[k] = sum_n x[n0 + n] h[n] e^(-2 pi i k (n0 + n) / M), n0 the absolute index of the frame's first sample (the first sample
    of the stream is index 0, so the history sits at negative indices)"""
    rng = np.random.default_rng(m * 17 + p * 5 + hop)
    Lt = m * p
    H = Lt - hop
    F = 5
    S = F * hop
    position = 3 * hop + 7 * m  # an earlier call consumed this much
    x = _signal(rng, S, cplx)
    h = rng.standard_normal(Lt)
    hist = _signal(rng, H, cplx)
    y, _ = pfb_ref(x, m, p, hop, h, hist, phase="time", position=position)
    full = np.concatenate([hist[::-1], x])
    bins = m if cplx else m // 2 + 1
    k = np.arange(bins)[:, None]
    n = np.arange(Lt)[None, :]
    for j in range(F):
        n0 = position - H + j * hop
        ph = np.exp(-2j * np.pi * ((k * (n0 + n)) % m) / m)  # the exact residue keeps the exponentials' arguments small
        want = (ph * (full[j * hop:j * hop + Lt] * h)[None, :]).sum(axis=1)
        assert np.abs(y[j] - want).max() <= 1e-12 * np.abs(want).max(), j
    if hop == m and position % m == 0:
        yf, _ = pfb_ref(x, m, p, hop, h, hist, phase="frame")
        assert np.array_equal(y, yf)


@pytest.mark.parametrize("m,p,hop", [(32, 1, 8), (32, 3, 24), (64, 8, 32), (64, 2, 1), (32, 4, 32)])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("phase", ["frame", "time"])
def test_reference_blockwise_equals_one_call(m, p, hop, cplx, phase):
    rng = np.random.default_rng(m + p + hop)
    Lt = m * p
    blocks = [0, hop, 3 * hop, 0, 7 * hop, hop, 2 * (Lt // hop) * hop + hop]  # blocks shorter and longer than hist, empty ones
    S = sum(blocks)
    x = np.stack([_signal(rng, S, cplx) for _ in range(2)])
    h = rng.standard_normal(Lt)
    want, want_state = pfb_ref(x, m, p, hop, h, None, phase=phase, position=0)
    state, pos, outs = None, 0, []
    for b in blocks:
        y, state = pfb_ref(x[:, pos:pos + b], m, p, hop, h, state, phase=phase, position=pos)
        assert y.shape[1] == b // hop
        outs.append(y)
        pos += b
    assert np.array_equal(np.concatenate(outs, axis=1), want)
    assert np.array_equal(state, want_state)


@pytest.mark.parametrize("window", ["boxcar", "hann", "hamming", "blackman"])
def test_prototype_is_scipy_firwin(window):
    for m in (16, 256, 4096):
        for p in (1, 4, 16):
            h = sd.pfb_prototype(window, m, p)
            want = scipy.signal.firwin(p * m, 1.0 / m, window=window)
            assert h.shape == want.shape
            assert np.abs(h - want).max() <= 1e-13 * np.abs(want).max(), (m, p)
            assert abs(h.sum() - 1.0) < 1e-12
    assert np.array_equal(sd.pfb_prototype("rect", 16, 2), sd.pfb_prototype("boxcar", 16, 2))


def test_prototype_shares_the_fir_design_construction():
    """firwin's Hamming low-pass through both entries: the same numbers where both accept the size"""
    lib = sd.load()
    for m, p in [(16, 4), (256, 16)]:
        a = np.zeros(m * p)
        L = sd.pfb.L
        L.check(lib.sdsp_hip_fir_design(m * p, L.FILTER_LOW_PASS, 1.0 / m, 2.0, 0.0, 1.0, a.ctypes.data))
        assert np.array_equal(a, sd.pfb_prototype("hamming", m, p))
    big = np.zeros(8192)
    assert lib.sdsp_hip_fir_design(8192, sd.pfb.L.FILTER_LOW_PASS, 0.1, 2.0, 0.0, 1.0, big.ctypes.data) == sd.pfb.L.ERR_INVALID_SIZE


def test_prototype_errors():
    lib = sd.load()
    L = sd.pfb.L
    h = np.zeros(1 << 12)
    assert lib.sdsp_hip_pfb_prototype(4, 16, 4, h.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_prototype(-1, 16, 4, h.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_prototype(2, 16, 4, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_prototype(2, 0, 4, h.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_pfb_prototype(2, 16, 0, h.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_pfb_prototype(2, 16, 65, h.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_pfb_prototype(2, 1 << 16, 32, h.ctypes.data) == L.ERR_INVALID_SIZE
    with pytest.raises(ValueError):
        sd.pfb_prototype("kaiser", 16, 4)


def test_frames_rule_and_sizes():
    lib = sd.load()
    L = sd.pfb.L
    n = C.c_uint64(7)
    for hop, S in [(1, 0), (1, 5), (64, 640), (256, 256)]:
        assert lib.sdsp_hip_pfb_frames(hop, S, C.byref(n)) == 0 and n.value == S // hop
    assert lib.sdsp_hip_pfb_frames(64, 65, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_pfb_frames(0, 8, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_pfb_frames(4, 8, None) == L.ERR_INVALID_ARG
    b = sd.pfb_bank(256, 8, 128, streams=3)
    assert b.frames(640) == 5 and b.hist == 8 * 256 - 128 and b.bins == 129 and b.n_taps == 2048 and b.position == 0
    assert np.array_equal(b.taps, sd.pfb_prototype("hamming", 256, 8))
    assert sd.pfb_bank(256, 8, input="complex").bins == 256 and sd.pfb_bank(256, 8).hop == 256
    with pytest.raises(sd.SdspHipError):
        b.frames(100)
    assert lib.sdsp_hip_pfb_state_bytes(None, 1, C.byref(n)) == L.ERR_INVALID_ARG


def test_plan_creation_errors_and_no_device():
    """argument errors come first; without a usable device a valid plan fails loudly (with one, it must succeed and report its
    state bytes)"""
    lib = sd.load()
    L = sd.pfb.L
    h = np.ones(1 << 21)
    p = C.c_void_p()

    def make(m, taps, hop, ptr=h.ctypes.data, kind=L.PFB_REAL, phase=L.PFB_PHASE_TIME, precision=L.F32):
        return lib.sdsp_hip_pfb_plan_create(C.byref(p), m, taps, hop, ptr, kind, phase, precision, 0, 0)

    assert make(1000, 4, 10) == L.ERR_INVALID_SIZE
    assert make(1024, 0, 1024) == L.ERR_INVALID_SIZE
    assert make(1024, 65, 1024) == L.ERR_INVALID_SIZE
    assert make(65536, 32, 65536) == L.ERR_INVALID_SIZE  # L > 2^20
    assert make(1024, 4, 0) == L.ERR_INVALID_SIZE
    assert make(1024, 4, 1025) == L.ERR_INVALID_SIZE
    assert make(1024, 4, 256, ptr=None) == L.ERR_INVALID_ARG
    assert make(1024, 4, 256, precision=7) == L.ERR_INVALID_ARG
    assert make(1024, 4, 256, kind=2) == L.ERR_INVALID_ARG
    assert make(1024, 4, 256, phase=2) == L.ERR_INVALID_ARG
    assert make(16, 4, 4) == L.ERR_UNSUPPORTED  # real input starts at 32
    assert make(8, 4, 4, kind=L.PFB_COMPLEX) == L.ERR_UNSUPPORTED
    assert make(1 << 17, 4, 4) == L.ERR_UNSUPPORTED
    assert make(65536, 4, 4, precision=L.F64) == L.ERR_UNSUPPORTED
    assert make(65536, 4, 4, kind=L.PFB_COMPLEX, precision=L.F64) == L.ERR_UNSUPPORTED
    assert lib.sdsp_hip_pfb_plan_create(None, 1024, 4, 256, h.ctypes.data, 0, 0, 0, 0, 0) == L.ERR_INVALID_ARG
    for kind, esize in ((L.PFB_REAL, 4), (L.PFB_COMPLEX, 8)):
        rc = make(1024, 4, 256, kind=kind)
        if torch.cuda.is_available():
            assert rc == 0
            n = C.c_uint64(0)
            assert lib.sdsp_hip_pfb_state_bytes(p, 5, C.byref(n)) == 0 and n.value == (4096 - 256) * 5 * esize
            lib.sdsp_hip_pfb_plan_destroy(p)
        else:
            assert rc == L.ERR_NO_DEVICE
    assert lib.sdsp_hip_pfb_plan_destroy(None) == 0
    with pytest.raises(ValueError):
        sd.pfb_bank(64, 4, 65)
    with pytest.raises(ValueError):
        sd.pfb_bank(64, 4, taps=np.ones(255))
    with pytest.raises(ValueError):
        sd.pfb_bank(64, 4, input="iq")
    with pytest.raises(ValueError):
        sd.pfb_bank(64, 4, phase="absolute")


def test_no_wide_store_is_followed_by_a_write_to_its_data_registers():
    """the scan of tests/test_capi_host.py (profiles/r03_store_hazard.md) over the fold kernels, built with the flags the library
    ships them with (simpledsp_amd/build.py: -ffp-contract=off keeps every product and sum of the fold a rounding of its own)"""
    from simpledsp_amd import build as B
    flags = B.SOURCES["pfb.hip"]
    assert "-ffp-contract=off" in flags
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_store_hazard.py"), str(ROOT / "simpledsp_amd" / "csrc" / "pfb.hip"),
                        *flags], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unguarded overwrites of store data: 0" in r.stdout
