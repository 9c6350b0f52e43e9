"""CPU checks of the polyphase resampler (include/sdsp_hip.h: sdsp_hip_resample_*): the numpy reference
the GPU tests use against scipy.signal.upfirdn, block-wise streaming of that reference, the anti-aliasing design against
scipy.signal.firwin, the output-count rule, plan creation without a device, and the store-hazard scan of fir_resample.hip."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal

from conftest import ROOT
from resample_ref import GRID_T, GRID_UD, hist_of, q_of, resample_ref

import simpledsp_amd as sd


def _samples(up, down, at_least=300):
    q = q_of(up, down)
    return q * max(2, -(-at_least // q))


@pytest.mark.parametrize("up,down", GRID_UD)
@pytest.mark.parametrize("taps", GRID_T)
def test_reference_is_causal_upfirdn(up, down, taps):
    rng = np.random.default_rng(taps * 7919 + up * 131 + down)
    S = _samples(up, down)
    h = rng.standard_normal(taps)
    x = rng.standard_normal(S)
    y, state = resample_ref(h, x, up, down)
    want = scipy.signal.upfirdn(h, x, up, down)
    M = S * up // down
    assert y.size == M
    cut = np.zeros(M)
    cut[:min(M, want.size)] = want[:M]
    assert np.abs(y - cut).max() <= 1e-13 * np.abs(cut).max()
    H = hist_of(taps, up)
    assert np.array_equal(state, np.concatenate([x[::-1], np.zeros(H)])[:H])  # S < H: zero history behind the block
    if taps < up:  # phases without taps give exactly 0
        p = (np.arange(M) * down) % up
        assert np.all(y[p >= taps] == 0)


@pytest.mark.parametrize("up,down", GRID_UD)
@pytest.mark.parametrize("taps", [1, 17, 255])
def test_reference_blockwise_equals_one_call(up, down, taps):
    rng = np.random.default_rng(taps + 1000 * up + down)
    q = q_of(up, down)
    blocks = [0, q, 3 * q, 0, 7 * q, q, 11 * q]
    x = rng.standard_normal(sum(blocks))
    h = rng.standard_normal(taps)
    hist0 = rng.standard_normal(hist_of(taps, up))
    want, want_state = resample_ref(h, x, up, down, hist0)
    got, state, s0 = [], hist0, 0
    for b in blocks:
        y, state = resample_ref(h, x[s0:s0 + b], up, down, state)
        got.append(y)
        s0 += b
    assert np.array_equal(np.concatenate(got), want)
    assert np.array_equal(state, want_state)


def test_reference_equals_zero_stuffed_direct_fir():
    rng = np.random.default_rng(5)
    for up, down, taps in [(3, 2, 64), (160, 147, 300), (1, 4, 65), (4, 1, 17)]:
        S = _samples(up, down)
        h, x = rng.standard_normal(taps), rng.standard_normal(S)
        z = np.zeros(S * up)
        z[::up] = x
        direct = np.zeros(S * up)
        for n in range(S * up):  # ascending k, multiply then add, the direct FIR bank's order
            acc = h[0] * z[n]
            for k in range(1, min(taps, n + 1)):
                acc = acc + h[k] * z[n - k]
            direct[n] = acc
        assert np.array_equal(resample_ref(h, x, up, down)[0], direct[::down])


def _design(taps, up, down):
    h = np.zeros(max(taps, 1))
    return sd.load().sdsp_hip_resample_design(taps, up, down, h.ctypes.data), h


@pytest.mark.parametrize("up,down", [(1, 2), (1, 4), (2, 1), (3, 2), (2, 3), (160, 147), (147, 160), (1, 1024), (1024, 1)])
@pytest.mark.parametrize("taps", [1, 2, 31, 64, 255, 1024, 4096])
def test_design_is_scaled_firwin(up, down, taps):
    rc, h = _design(taps, up, down)
    assert rc == 0
    want = up * scipy.signal.firwin(taps, 1.0 / max(up, down))
    # 4096 taps: the window and the normalising sum round differently from scipy's over 4096 terms (measured 4.5e-15)
    tol = 1e-15 if taps <= 1024 else 1e-14
    assert np.abs(h - want).max() <= tol * max(1.0, np.abs(want).max()) * up


def test_design_errors():
    assert _design(64, 1, 1)[0] == -5
    assert _design(0, 1, 2)[0] == -1
    assert _design(4097, 1, 2)[0] == -1
    assert _design(64, 0, 2)[0] == -1
    assert _design(64, 2, 1025)[0] == -1
    assert sd.load().sdsp_hip_resample_design(64, 1, 2, None) == -5


def test_out_samples():
    lib = sd.load()
    n = C.c_uint64(0)
    for up, down, S, want in [(1, 4, 4032, 1008), (2, 1, 10, 20), (3, 2, 4, 6), (160, 147, 147, 160), (147, 160, 320, 294),
                              (2, 4, 6, 3), (1, 1, 0, 0), (5, 7, 0, 0), (1024, 1, 1 << 30, 1 << 40)]:
        assert lib.sdsp_hip_resample_out_samples(up, down, S, C.byref(n)) == 0
        assert n.value == want
    for up, down, S in [(1, 4, 4030), (3, 2, 3), (160, 147, 146), (2, 4, 5)]:
        assert lib.sdsp_hip_resample_out_samples(up, down, S, C.byref(n)) == -1
    assert lib.sdsp_hip_resample_out_samples(0, 1, 4, C.byref(n)) == -1
    assert lib.sdsp_hip_resample_out_samples(1, 1025, 1025, C.byref(n)) == -1
    assert lib.sdsp_hip_resample_out_samples(1, 2, 4, None) == -5
    r = sd.fir_resampler(64, 3, 2)
    assert r.out_samples(4) == 6 and r.hist == 21 and r.q == 2
    with pytest.raises(sd.SdspHipError):
        r.out_samples(5)
    for bad in (-1, 3):  # rejected when set, not at the first process()
        with pytest.raises(ValueError):
            r.set_variant(bad)


def test_plan_needs_a_device_and_says_so():
    """no CPU fallback: without a usable device, creation fails loudly (with one, it must succeed)"""
    import torch
    h = np.ones(64)
    p = C.c_void_p()
    lib = sd.load()
    assert lib.sdsp_hip_resample_plan_create(C.byref(p), 0, h.ctypes.data, 1, 2, sd.F32, 0) == -1
    assert lib.sdsp_hip_resample_plan_create(C.byref(p), 64, h.ctypes.data, 1, 1025, sd.F32, 0) == -1
    assert lib.sdsp_hip_resample_plan_create(C.byref(p), 64, None, 1, 2, sd.F32, 0) == -5
    assert lib.sdsp_hip_resample_plan_create(C.byref(p), 64, h.ctypes.data, 1, 2, 7, 0) == -5
    rc = lib.sdsp_hip_resample_plan_create(C.byref(p), 64, h.ctypes.data, 1, 4, sd.F32, 0)
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_resample_plan_destroy(p)
    else:
        assert rc == -4


def test_no_wide_store_is_followed_by_a_write_to_its_data_registers():
    """the scan of tests/test_capi_host.py (profiles/r03_store_hazard.md) over the resampler's kernels, built with the flags the
    library ships them with (simpledsp_amd/build.py: -ffp-contract=off keeps f64 multiply and add unfused)"""
    from simpledsp_amd import build as B
    flags = B.SOURCES["fir_resample.hip"]
    assert "-ffp-contract=off" in flags
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_store_hazard.py"), str(ROOT / "simpledsp_amd" / "csrc" / "fir_resample.hip"),
                        *flags], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unguarded overwrites of store data: 0" in r.stdout
