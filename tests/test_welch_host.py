"""CPU checks of the Welch PSD bank (include/sdsp_hip.h: sdsp_hip_welch_*): the numpy reference the GPU tests
use against scipy.signal.welch, block-wise streaming of that reference, the segment-count rule, plan creation without a device, and
the store-hazard scan of welch.hip."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal
import torch

from conftest import ROOT
from welch_ref import welch_frames, welch_psd, welch_ref

import simpledsp_amd as sd
from simpledsp_amd import _lib as L


@pytest.mark.parametrize("n_fft,hop", [(32, 8), (64, 48), (256, 56), (256, 128), (256, 256), (1024, 256), (1024, 1)])
@pytest.mark.parametrize("detrend", ["constant", "linear", False])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
def test_reference_is_scipy_welch(n_fft, hop, detrend, scaling):
    rng = np.random.default_rng(n_fft * 13 + hop)
    S = 5 * n_fft + 37 if hop > 1 else n_fft + 40
    x = rng.standard_normal((3, S)) + np.linspace(0, 4, S)  # a trend for the detrenders to remove
    w = scipy.signal.get_window("hann", n_fft)
    fs = 48000.0
    acc, F, _ = welch_ref(x, n_fft, hop, w, detrend or "none")
    assert F == (S - n_fft) // hop + 1
    got = welch_psd(acc, F, w, fs, scaling)
    f, want = scipy.signal.welch(x, fs, window=w, nperseg=n_fft, noverlap=n_fft - hop, detrend=detrend, scaling=scaling, axis=-1)
    assert np.array_equal(f, np.fft.rfftfreq(n_fft, 1 / fs))
    assert np.abs(got - want).max(axis=-1).max() <= 1e-13 * np.abs(want).max(axis=-1).min()


@pytest.mark.parametrize("n_fft,hop", [(32, 8), (64, 48), (256, 56), (256, 256), (64, 1)])
@pytest.mark.parametrize("detrend", ["none", "constant", "linear"])
def test_reference_blockwise_counts_the_same_segments(n_fft, hop, detrend):
    rng = np.random.default_rng(n_fft + 7 * hop)
    blocks = [0, 1, n_fft - 2, hop + 1, 0, max(hop - 1, 0), 3, 5 * n_fft + 11, n_fft - 1, hop]
    x = rng.standard_normal((2, sum(blocks)))
    w = scipy.signal.get_window("hamming", n_fft)
    want, want_F, want_state = welch_ref(x, n_fft, hop, w, detrend)
    acc, state, pos, F = None, None, 0, 0
    for b in blocks:
        acc, f, state = welch_ref(x[:, pos:pos + b], n_fft, hop, w, detrend, pos, state, acc)
        assert f == welch_frames(n_fft, hop, pos, b)
        pos += b
        F += f
    assert F == want_F == (sum(blocks) - n_fft) // hop + 1
    assert np.abs(acc - want).max() <= 1e-13 * np.abs(want).max()
    assert np.array_equal(state, want_state)
    assert np.array_equal(state, x[:, ::-1][:, :n_fft - 1])


def test_frames_rule():
    lib = sd.load()
    n = C.c_uint64(7)
    cases = [(256, 64, 0, 0), (256, 64, 0, 255), (256, 64, 0, 256), (256, 64, 0, 1000), (256, 56, 100, 1000), (256, 56, 255, 1),
             (256, 56, 256, 55), (256, 56, 256, 56), (32, 32, 31, 1), (65536, 1, 1 << 20, 1 << 20), (1024, 3, 1 << 40, 12345),
             (64, 48, 5, 0)]
    for N, hop, pos, S in cases:
        assert lib.sdsp_hip_welch_frames(N, hop, pos, S, C.byref(n)) == 0
        want = len([m for m in range(0, (pos + S) // hop + 1) if pos < m * hop + N <= pos + S]) if pos < 1 << 30 else None
        if want is not None:
            assert n.value == want, (N, hop, pos, S)
        assert n.value == welch_frames(N, hop, pos, S)
    assert lib.sdsp_hip_welch_frames(0, 4, 0, 8, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_welch_frames(8, 0, 0, 8, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_welch_frames(8, 4, 0, 8, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_welch_frames(8, 4, 1 << 63, 1 << 63, C.byref(n)) == L.ERR_INVALID_SIZE
    assert sd.welch_bank(256, 56).segments(1000) == (1000 - 256) // 56 + 1


def test_plan_creation_errors_and_no_device():
    """argument errors come first; without a usable device a valid plan fails loudly (with one, it must succeed)"""
    lib = sd.load()
    w = np.ones(1 << 17)
    p = C.c_void_p()

    def make(n, hop, win=w.ctypes.data, detrend=L.DETREND_CONSTANT, scaling=L.SCALING_DENSITY, fs=1.0, precision=L.F32):
        return lib.sdsp_hip_welch_plan_create(C.byref(p), n, hop, win, detrend, scaling, fs, precision, 0, 0)

    assert make(1000, 10) == L.ERR_INVALID_SIZE
    assert make(1024, 0) == L.ERR_INVALID_SIZE
    assert make(1024, 1025) == L.ERR_INVALID_SIZE
    assert make(1024, 256, win=None) == L.ERR_INVALID_ARG
    assert make(1024, 256, precision=7) == L.ERR_INVALID_ARG
    assert make(1024, 256, detrend=3) == L.ERR_INVALID_ARG
    assert make(1024, 256, scaling=2) == L.ERR_INVALID_ARG
    for fs in (0.0, -1.0, float("inf"), float("nan")):
        assert make(1024, 256, fs=fs) == L.ERR_INVALID_ARG
    assert make(16, 4) == L.ERR_UNSUPPORTED
    assert make(1 << 17, 4) == L.ERR_UNSUPPORTED
    assert make(65536, 4, precision=L.F64) == L.ERR_UNSUPPORTED
    assert lib.sdsp_hip_welch_plan_create(None, 1024, 256, w.ctypes.data, 0, 0, 1.0, 0, 0, 0) == L.ERR_INVALID_ARG
    rc = make(1024, 256)
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_welch_plan_destroy(p)
    else:
        assert rc == L.ERR_NO_DEVICE
    assert lib.sdsp_hip_welch_plan_destroy(None) == 0
    with pytest.raises(ValueError):
        sd.welch_bank(64, 65)
    with pytest.raises(ValueError):
        sd.welch_bank(64, 16, window=np.ones(63))
    with pytest.raises(ValueError):
        sd.welch_bank(64, 16, detrend="quadratic")
    with pytest.raises(ValueError):
        sd.welch_bank(64, 16, scaling="power")


def test_one_shot_refuses_what_is_out_of_scope():
    x = torch.zeros(4096)  # a host tensor: refused before any device work
    for kw in [dict(nfft=512), dict(return_onesided=False), dict(average="median"), dict(nperseg=100), dict(noverlap=256),
               dict(detrend=lambda s: s)]:
        with pytest.raises(ValueError):
            sd.welch(x, **kw)
    with pytest.raises(ValueError):
        sd.welch(x)  # not a device tensor


def test_no_wide_store_is_followed_by_a_write_to_its_data_registers():
    """the scan of tests/test_capi_host.py (profiles/r03_store_hazard.md) over the Welch kernels, built with the flags the library
    ships them with (simpledsp_amd/build.py: -ffp-contract=off keeps every product and sum rounded on its own)"""
    from simpledsp_amd import build as B
    flags = B.SOURCES["welch.hip"]
    assert "-ffp-contract=off" in flags
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_store_hazard.py"), str(ROOT / "simpledsp_amd" / "csrc" / "welch.hip"),
                        *flags], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unguarded overwrites of store data: 0" in r.stdout
