"""CPU checks of the inverse STFT bank (include/sdsp_hip.h: sdsp_hip_istft_*): the numpy reference the GPU
tests use against torch.istft(center=False) and as the inverse of tests/stft_ref.py, block-wise streaming of that reference, the
synthesis window and its NOLA check, plan and argument validation without a device, and the store-hazard scan of istft.hip."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal
import torch

from conftest import ROOT
from istft_ref import istft_ref, synthesis_window_ref
from stft_ref import stft_ref

import simpledsp_amd as sd

L = sd.istft.L
WINDOW_KINDS = {L.WINDOW_RECT: "boxcar", L.WINDOW_HANN: "hann", L.WINDOW_HAMMING: "hamming", L.WINDOW_BLACKMAN: "blackman"}


def _spectra(rng, channels, frames, n_fft):
    return rng.standard_normal((channels, frames, n_fft // 2 + 1)) + 1j * rng.standard_normal((channels, frames, n_fft // 2 + 1))


@pytest.mark.parametrize("name", ["hamming", "boxcar"])
@pytest.mark.parametrize("n_fft", [32, 256, 1024])
@pytest.mark.parametrize("hop_div", [4, 2, 1])
def test_reference_is_torch_istft_past_the_first_hist_samples(name, n_fft, hop_div):
    hop = n_fft // hop_div
    H, F = n_fft - hop, 3 * hop_div + 4
    w = scipy.signal.get_window(name, n_fft)
    g = synthesis_window_ref(w, n_fft, hop)
    X = _spectra(np.random.default_rng(n_fft + hop), 1, F, n_fft)[0]
    y, _ = istft_ref(X, n_fft, hop, g)
    want = torch.istft(torch.from_numpy(X.T.copy()), n_fft, hop, window=torch.from_numpy(w), center=False).numpy()
    assert want.shape[0] == (F - 1) * hop + n_fft
    assert np.abs(y[H:] - want[H:F * hop]).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", ["hann", "hamming", "blackman"])
@pytest.mark.parametrize("n_fft,hop", [(32, 1), (64, 16), (256, 64), (256, 128), (1024, 256)])
def test_reference_inverts_the_stft_reference_with_the_hist_delay(name, n_fft, hop):
    H = n_fft - hop
    rng = np.random.default_rng(n_fft * 3 + hop)
    S = hop * (2 * n_fft // hop + 5)
    x = rng.standard_normal((2, S))
    w = scipy.signal.get_window(name, n_fft)
    X, _ = stft_ref(x, n_fft, hop, w)
    y, _ = istft_ref(X, n_fft, hop, synthesis_window_ref(w, n_fft, hop))
    assert y.shape == x.shape
    assert np.abs(y[:, H:] - x[:, :S - H]).max() <= 1e-12
    assert np.abs(y[:, :H]).max() <= 1e-12


@pytest.mark.parametrize("n_fft,hop", [(32, 1), (32, 8), (64, 48), (64, 64), (256, 64)])
def test_reference_blockwise_equals_one_call(n_fft, hop):
    rng = np.random.default_rng(n_fft + hop)
    H = n_fft - hop
    blocks = [0, 1, 3, 0, 7, 1, H // hop + 3]  # blocks with F hop shorter and longer than hist, and empty ones
    X = _spectra(rng, 3, sum(blocks), n_fft)
    g = synthesis_window_ref(scipy.signal.get_window("hamming", n_fft), n_fft, hop)
    p0 = rng.standard_normal((3, H))
    want, want_state = istft_ref(X, n_fft, hop, g, p0)
    got, state, f0 = [], p0, 0
    for b in blocks:
        y, state = istft_ref(X[:, f0:f0 + b], n_fft, hop, g, state)
        got.append(y)
        f0 += b
    assert np.array_equal(np.concatenate(got, axis=1), want)
    assert np.array_equal(state, want_state)


@pytest.mark.parametrize("kind", sorted(WINDOW_KINDS))
def test_synthesis_window_is_w_over_env(kind):
    lib = sd.load()
    for n_fft in (32, 256, 4096):
        w = np.zeros(n_fft)
        assert lib.sdsp_hip_stft_window(kind, n_fft, w.ctypes.data) == 0
        for hop in sorted({1, 3, n_fft // 8, n_fft // 4, n_fft // 2, 3 * n_fft // 4, n_fft}):
            g = np.full(n_fft, 7.0)
            want = synthesis_window_ref(w, n_fft, hop)
            rc = lib.sdsp_hip_istft_synthesis_window(n_fft, hop, w.ctypes.data, L.ISTFT_NORMALIZED, g.ctypes.data)
            if want is None:
                assert rc == L.ERR_INVALID_ARG, (WINDOW_KINDS[kind], n_fft, hop)
            else:
                assert rc == 0, (WINDOW_KINDS[kind], n_fft, hop)
                assert np.abs(g - want).max() <= 1e-15 * np.abs(want).max(), (WINDOW_KINDS[kind], n_fft, hop)
            assert lib.sdsp_hip_istft_synthesis_window(n_fft, hop, w.ctypes.data, L.ISTFT_RAW, g.ctypes.data) == 0
            assert np.array_equal(g, w)
    b = sd.istft_bank(64, 16, window="hamming")
    assert np.abs(b.synthesis_window - synthesis_window_ref(sd.stft_window("hamming", 64), 64, 16)).max() <= 1e-15
    assert np.array_equal(sd.istft_bank(64, 16, window="hamming", normalized=False).synthesis_window, sd.stft_window("hamming", 64))


@pytest.mark.parametrize("name,n_fft,hop,ok", [("hann", 256, 256, False), ("blackman", 256, 256, False), ("hann", 1024, 1024, False),
                                               ("hann", 256, 128, True), ("boxcar", 256, 256, True), ("hann", 64, 1, True)])
def test_nola(name, n_fft, hop, ok):
    lib = sd.load()
    w = scipy.signal.get_window(name, n_fft)
    g = np.zeros(n_fft)
    rc = lib.sdsp_hip_istft_synthesis_window(n_fft, hop, w.ctypes.data, L.ISTFT_NORMALIZED, g.ctypes.data)
    assert rc == (0 if ok else L.ERR_INVALID_ARG)
    if not ok:
        assert "NOLA" in lib.sdsp_hip_last_error_string().decode()
        with pytest.raises(sd.SdspHipError):
            sd.istft_synthesis_window(n_fft, hop, w)
        p = C.c_void_p()
        assert lib.sdsp_hip_istft_plan_create(C.byref(p), n_fft, hop, w.ctypes.data, L.ISTFT_NORMALIZED, L.F32, 0, 0) == L.ERR_INVALID_ARG
        assert "NOLA" in lib.sdsp_hip_last_error_string().decode()
        # RAW takes the window as it is
        assert lib.sdsp_hip_istft_synthesis_window(n_fft, hop, w.ctypes.data, L.ISTFT_RAW, g.ctypes.data) == 0
    else:
        assert np.isfinite(g).all()


def test_synthesis_window_errors():
    lib = sd.load()
    w, g = np.ones(64), np.zeros(64)
    assert lib.sdsp_hip_istft_synthesis_window(48, 16, w.ctypes.data, 0, g.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_istft_synthesis_window(64, 0, w.ctypes.data, 0, g.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_istft_synthesis_window(64, 65, w.ctypes.data, 0, g.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_istft_synthesis_window(64, 16, None, 0, g.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_synthesis_window(64, 16, w.ctypes.data, 0, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_synthesis_window(64, 16, w.ctypes.data, 2, g.ctypes.data) == L.ERR_INVALID_ARG
    z = np.zeros(64)
    assert lib.sdsp_hip_istft_synthesis_window(64, 16, z.ctypes.data, 0, g.ctypes.data) == L.ERR_INVALID_ARG  # all-zero window


def test_plan_creation_errors_and_no_device():
    """argument errors come first; without a usable device a valid plan fails loudly (with one, it must succeed)"""
    lib = sd.load()
    w = np.ones(1 << 17)
    p = C.c_void_p()

    def make(n, hop, win=w.ctypes.data, norm=L.ISTFT_NORMALIZED, precision=L.F32):
        return lib.sdsp_hip_istft_plan_create(C.byref(p), n, hop, win, norm, precision, 0, 0)

    assert make(1000, 10) == L.ERR_INVALID_SIZE
    assert make(1024, 0) == L.ERR_INVALID_SIZE
    assert make(1024, 1025) == L.ERR_INVALID_SIZE
    assert make(1024, 256, win=None) == L.ERR_INVALID_ARG
    assert make(1024, 256, precision=7) == L.ERR_INVALID_ARG
    assert make(1024, 256, norm=2) == L.ERR_INVALID_ARG
    assert make(16, 4) == L.ERR_UNSUPPORTED
    assert make(1 << 17, 4) == L.ERR_UNSUPPORTED
    assert make(65536, 4, precision=L.F64) == L.ERR_UNSUPPORTED
    assert lib.sdsp_hip_istft_plan_create(None, 1024, 256, w.ctypes.data, 0, 0, 0, 0) == L.ERR_INVALID_ARG
    rc = make(1024, 256)
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_istft_plan_destroy(p)
    else:
        assert rc == L.ERR_NO_DEVICE
    assert lib.sdsp_hip_istft_plan_destroy(None) == 0
    nb = C.c_uint64(5)
    assert lib.sdsp_hip_istft_state_bytes(None, 1, C.byref(nb)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_plan_launches(None, 1, 1, C.byref(nb)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_plan_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_process(None, None, 0, None, 0, 1, 1, None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_process_host(None, None, 0, None, 0, 1, 1, None) == L.ERR_INVALID_ARG


def test_python_argument_validation():
    with pytest.raises(ValueError):
        sd.istft_bank(64, 65)
    with pytest.raises(ValueError):
        sd.istft_bank(64, 0)
    with pytest.raises(ValueError):
        sd.istft_bank(64, 16, channels=0)
    with pytest.raises(ValueError):
        sd.istft_bank(64, 16, window=np.ones(63))
    with pytest.raises(ValueError):
        sd.istft_bank(64, 16, window="kaiser")
    b = sd.istft_bank(256, 64, channels=2)
    assert (b.hist, b.bins) == (192, 129)
    with pytest.raises(ValueError):
        b.set_variant(-1)
    # process validates the tensor before touching a device
    cases = [torch.zeros((2, 4, 129), dtype=torch.complex64),                       # host tensor
             torch.zeros((2, 4, 129), dtype=torch.complex128),                      # wrong precision
             torch.zeros((2, 4, 128), dtype=torch.complex64),                       # wrong bin count
             torch.zeros((2, 4 * 129), dtype=torch.complex64),                      # not (channels, frames, bins)
             torch.zeros((2, 4, 129), dtype=torch.float32)]                         # real
    for X in cases:
        with pytest.raises(ValueError):
            b.process(X)


def test_no_wide_store_is_followed_by_a_write_to_its_data_registers():
    """the scan of tests/test_capi_host.py (profiles/r03_store_hazard.md) over the inverse STFT kernels, built with the flags the
    library ships them with (simpledsp_amd/build.py: -ffp-contract=off keeps every overlap-add step a product and a sum)"""
    from simpledsp_amd import build as B
    flags = B.SOURCES["istft.hip"]
    assert "-ffp-contract=off" in flags
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_store_hazard.py"), str(ROOT / "simpledsp_amd" / "csrc" / "istft.hip"),
                        *flags], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unguarded overwrites of store data: 0" in r.stdout
