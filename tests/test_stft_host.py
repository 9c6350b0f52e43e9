"""CPU checks of the STFT bank (include/sdsp_hip.h: sdsp_hip_stft_*): the numpy reference the GPU tests use
against torch.stft(center=False), block-wise streaming of that reference, the periodic windows against scipy.signal.get_window,
the frame-count rule, plan creation without a device, and the store-hazard scan of stft.hip."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal
import torch

from conftest import ROOT
from stft_ref import stft_ref

import simpledsp_amd as sd


@pytest.mark.parametrize("n_fft", [32, 64, 1024])
@pytest.mark.parametrize("hop_div", [0, 4, 2, 1])  # 0: hop = 1
def test_reference_is_torch_stft_over_the_zero_prefixed_stream(n_fft, hop_div):
    hop = 1 if hop_div == 0 else n_fft // hop_div
    rng = np.random.default_rng(n_fft * 31 + hop)
    S = hop * max(3, -(-2 * n_fft // hop))
    x = rng.standard_normal(S)
    w = scipy.signal.get_window("hann", n_fft)
    hist = rng.standard_normal(n_fft - hop)
    y, _ = stft_ref(x, n_fft, hop, w, hist)
    full = np.concatenate([hist[::-1], x])
    want = torch.stft(torch.from_numpy(full), n_fft, hop, window=torch.from_numpy(w), center=False, return_complex=True).numpy().T
    assert y.shape == want.shape == (S // hop, n_fft // 2 + 1)
    assert np.abs(y - want).max() <= 1e-13 * np.abs(want).max()
    y0, _ = stft_ref(x, n_fft, hop, w)  # fresh stream = hist zeros in front
    want0 = torch.stft(torch.from_numpy(np.concatenate([np.zeros(n_fft - hop), x])), n_fft, hop, window=torch.from_numpy(w),
                       center=False, return_complex=True).numpy().T
    assert np.abs(y0 - want0).max() <= 1e-13 * np.abs(want0).max()


@pytest.mark.parametrize("n_fft,hop", [(32, 1), (32, 8), (64, 48), (64, 64), (256, 64)])
@pytest.mark.parametrize("output", ["complex", "power", "magnitude"])
def test_reference_blockwise_equals_one_call(n_fft, hop, output):
    rng = np.random.default_rng(n_fft + hop)
    blocks = [0, hop, 3 * hop, 0, 7 * hop, hop, 2 * n_fft // hop * hop + hop]  # blocks shorter and longer than hist
    x = rng.standard_normal((3, sum(blocks)))
    w = scipy.signal.get_window("hamming", n_fft)
    hist0 = rng.standard_normal((3, n_fft - hop))
    want, want_state = stft_ref(x, n_fft, hop, w, hist0, output)
    got, state, s0 = [], hist0, 0
    for b in blocks:
        y, state = stft_ref(x[:, s0:s0 + b], n_fft, hop, w, state, output)
        got.append(y)
        s0 += b
    assert np.array_equal(np.concatenate(got, axis=1), want)
    assert np.array_equal(state, want_state)


SCIPY_NAMES = {sd.stft.L.WINDOW_RECT: "boxcar", sd.stft.L.WINDOW_HANN: "hann", sd.stft.L.WINDOW_HAMMING: "hamming",
               sd.stft.L.WINDOW_BLACKMAN: "blackman"}


@pytest.mark.parametrize("kind", sorted(SCIPY_NAMES))
def test_windows_are_scipy_periodic(kind):
    lib = sd.load()
    for lg in range(5, 17):
        n = 1 << lg
        w = np.zeros(n)
        assert lib.sdsp_hip_stft_window(kind, n, w.ctypes.data) == 0
        want = scipy.signal.get_window(SCIPY_NAMES[kind], n)
        assert np.abs(w - want).max() <= 1e-15, (SCIPY_NAMES[kind], n)
    assert np.abs(sd.stft_window(SCIPY_NAMES[kind], 64) - scipy.signal.get_window(SCIPY_NAMES[kind], 64)).max() <= 1e-15


def test_window_errors():
    lib = sd.load()
    w = np.zeros(8)
    assert lib.sdsp_hip_stft_window(4, 8, w.ctypes.data) == sd.stft.L.ERR_INVALID_ARG
    assert lib.sdsp_hip_stft_window(-1, 8, w.ctypes.data) == sd.stft.L.ERR_INVALID_ARG
    assert lib.sdsp_hip_stft_window(1, 8, None) == sd.stft.L.ERR_INVALID_ARG
    assert lib.sdsp_hip_stft_window(1, 0, w.ctypes.data) == sd.stft.L.ERR_INVALID_SIZE
    with pytest.raises(ValueError):
        sd.stft_window("kaiser", 8)


def test_frames_rule():
    lib = sd.load()
    n = C.c_uint64(7)
    for hop, S, want in [(1, 0, 0), (1, 5, 5), (256, 1 << 18, 1024), (64, 192, 3), (65536, 65536, 1), (3, 1 << 40, (1 << 40) // 3)]:
        if S % hop:
            continue
        assert lib.sdsp_hip_stft_frames(hop, S, C.byref(n)) == 0
        assert n.value == want
    for hop, S in [(2, 3), (256, 1000), (64, 65)]:
        assert lib.sdsp_hip_stft_frames(hop, S, C.byref(n)) == sd.stft.L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_stft_frames(0, 8, C.byref(n)) == sd.stft.L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_stft_frames(4, 8, None) == sd.stft.L.ERR_INVALID_ARG
    b = sd.stft_bank(256, 64)
    assert b.frames(640) == 10 and b.hist == 192 and b.bins == 129
    with pytest.raises(sd.SdspHipError):
        b.frames(100)


def test_plan_creation_errors_and_no_device():
    """argument errors come first; without a usable device a valid plan fails loudly (with one, it must succeed)"""
    lib = sd.load()
    L = sd.stft.L
    w = np.ones(1 << 17)
    p = C.c_void_p()

    def make(n, hop, win=w.ctypes.data, output=L.STFT_COMPLEX, precision=L.F32):
        return lib.sdsp_hip_stft_plan_create(C.byref(p), n, hop, win, output, precision, 0, 0)

    assert make(1000, 10) == L.ERR_INVALID_SIZE
    assert make(1024, 0) == L.ERR_INVALID_SIZE
    assert make(1024, 1025) == L.ERR_INVALID_SIZE
    assert make(1024, 256, win=None) == L.ERR_INVALID_ARG
    assert make(1024, 256, precision=7) == L.ERR_INVALID_ARG
    assert make(1024, 256, output=3) == L.ERR_INVALID_ARG
    assert make(16, 4) == L.ERR_UNSUPPORTED
    assert make(1 << 17, 4) == L.ERR_UNSUPPORTED
    assert make(65536, 4, precision=L.F64) == L.ERR_UNSUPPORTED
    assert lib.sdsp_hip_stft_plan_create(None, 1024, 256, w.ctypes.data, 0, 0, 0, 0) == L.ERR_INVALID_ARG
    rc = make(1024, 256)
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_stft_plan_destroy(p)
    else:
        assert rc == L.ERR_NO_DEVICE
    assert lib.sdsp_hip_stft_plan_destroy(None) == 0
    with pytest.raises(ValueError):
        sd.stft_bank(64, 65)
    with pytest.raises(ValueError):
        sd.stft_bank(64, 16, window=np.ones(63))
    with pytest.raises(ValueError):
        sd.stft_bank(64, 16, output="phase")


def test_no_wide_store_is_followed_by_a_write_to_its_data_registers():
    """the scan of tests/test_capi_host.py (profiles/r03_store_hazard.md) over the STFT kernels, built with the flags the library
    ships them with (simpledsp_amd/build.py: -ffp-contract=off keeps the power two products and a sum)"""
    from simpledsp_amd import build as B
    flags = B.SOURCES["stft.hip"]
    assert "-ffp-contract=off" in flags
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_store_hazard.py"), str(ROOT / "simpledsp_amd" / "csrc" / "stft.hip"),
                        *flags], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unguarded overwrites of store data: 0" in r.stdout
