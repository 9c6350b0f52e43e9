"""CPU checks of the cross-spectral density bank (include/sdsp_hip.h: sdsp_hip_csd_*): the numpy reference
the GPU tests use against scipy.signal.csd and scipy.signal.coherence, block-wise streaming of that reference, plan creation without
a device, and what the one-shot functions refuse."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal
import torch

from csd_ref import PAIRS, csd_coherence, csd_density, csd_inputs, csd_ref
from welch_ref import welch_frames, welch_ref

import simpledsp_amd as sd
from simpledsp_amd import _lib as L

@pytest.mark.parametrize("n_fft,hop", [(32, 8), (64, 48), (256, 56), (256, 128), (256, 256), (1024, 256)])
@pytest.mark.parametrize("detrend", ["constant", "linear", False])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
def test_reference_is_scipy_csd_and_coherence(n_fft, hop, detrend, scaling):
    S = 6 * n_fft + 37
    x = csd_inputs(n_fft, S, n_fft * 13 + hop)
    w = scipy.signal.get_window("hann", n_fft)
    fs = 48000.0
    xy, au, F, _ = csd_ref(x, PAIRS, n_fft, hop, w, detrend or "none")
    assert F == (S - n_fft) // hop + 1
    got = csd_density(xy, F, w, fs, scaling)
    coh = csd_coherence(xy, au, PAIRS)
    # the auto sums are the Welch reference's
    assert np.array_equal(au, welch_ref(x, n_fft, hop, w, detrend or "none")[0])
    for i, (a, b) in enumerate(PAIRS):
        kw = dict(window=w, nperseg=n_fft, noverlap=n_fft - hop, detrend=detrend)
        f, want = scipy.signal.csd(x[a], x[b], fs, scaling=scaling, **kw)
        assert np.array_equal(f, np.fft.rfftfreq(n_fft, 1 / fs))
        assert np.abs(got[i] - want).max() <= 1e-12 * np.abs(want).max()
        _, cw = scipy.signal.coherence(x[a], x[b], fs, **kw)
        assert np.abs(coh[i] - cw).max() <= 1e-12
        # the f32 coherence bound of the GPU tests stays below 1 only while no auto spectrum falls far below its peak
        assert au[a].min() > 1e-4 * au[a].max() and au[b].min() > 1e-4 * au[b].max()


@pytest.mark.parametrize("n_fft", [32, 256, 1024, 4096, 32768, 65536])
def test_auto_spectra_of_the_gpu_shapes_stay_above_1e_4_of_their_peak(n_fft):
    """what keeps the f32 coherence bound of tests/test_gpu_csd.py below 1: its shapes, seeds and hops, on the f32-rounded samples"""
    big = n_fft >= 32768
    w = scipy.signal.get_window("hann", n_fft).astype(np.float32).astype(np.float64)
    for detrend in (["linear"] if big else ["none", "constant", "linear"]):
        for hop in [n_fft // 2, n_fft // 4, 7 * n_fft // 32 + 1, n_fft][:1 if big else 4]:
            x = csd_inputs(n_fft, 6 * n_fft + 37, n_fft * 7 + hop, np.float32)
            _, au, _, _ = csd_ref(x, PAIRS, n_fft, hop, w, detrend)
            assert (au.min(axis=-1) > 1e-4 * au.max(axis=-1)).all(), (detrend, hop)


@pytest.mark.parametrize("n_fft,hop", [(32, 8), (64, 48), (256, 56), (256, 256), (64, 1)])
@pytest.mark.parametrize("detrend", ["none", "constant", "linear"])
def test_reference_blockwise_counts_the_same_segments(n_fft, hop, detrend):
    blocks = [0, 1, n_fft - 2, hop + 1, 0, max(hop - 1, 0), 3, 5 * n_fft + 11, n_fft - 1, hop]
    x = csd_inputs(n_fft, sum(blocks), n_fft + 7 * hop)
    w = scipy.signal.get_window("hamming", n_fft)
    want_xy, want_au, want_F, want_state = csd_ref(x, PAIRS, n_fft, hop, w, detrend)
    xy, au, state, pos, F = None, None, None, 0, 0
    for b in blocks:
        xy, au, f, state = csd_ref(x[:, pos:pos + b], PAIRS, n_fft, hop, w, detrend, pos, state, xy, au)
        assert f == welch_frames(n_fft, hop, pos, b)
        pos += b
        F += f
    assert F == want_F == (sum(blocks) - n_fft) // hop + 1
    assert np.abs(xy - want_xy).max() <= 1e-13 * np.abs(want_xy).max()
    assert np.abs(au - want_au).max() <= 1e-13 * np.abs(want_au).max()
    assert np.array_equal(state, want_state)
    assert np.array_equal(state, x[:, ::-1][:, :n_fft - 1])


def test_plan_creation_errors_and_no_device():
    """argument errors come first; without a usable device a valid plan fails loudly (with one, it must succeed)"""
    lib = sd.load()
    w = np.ones(1 << 17)
    p = C.c_void_p()
    good = np.array(PAIRS, dtype=np.uint32)

    def make(n=1024, hop=256, win=w.ctypes.data, detrend=L.DETREND_CONSTANT, scaling=L.SCALING_DENSITY, fs=1.0, precision=L.F32,
             channels=4, pairs=good, npairs=None, ws=0):
        return lib.sdsp_hip_csd_plan_create(C.byref(p), n, hop, win, detrend, scaling, fs, precision, channels,
                                            len(pairs) if npairs is None else npairs, pairs.ctypes.data if pairs is not None else None,
                                            ws, 0)

    assert make(n=1000, hop=10) == L.ERR_INVALID_SIZE
    assert make(hop=0) == L.ERR_INVALID_SIZE
    assert make(hop=1025) == L.ERR_INVALID_SIZE
    assert make(win=None) == L.ERR_INVALID_ARG
    assert make(precision=7) == L.ERR_INVALID_ARG
    assert make(detrend=3) == L.ERR_INVALID_ARG
    assert make(scaling=2) == L.ERR_INVALID_ARG
    for fs in (0.0, -1.0, float("inf"), float("nan")):
        assert make(fs=fs) == L.ERR_INVALID_ARG
    assert make(n=16, hop=4) == L.ERR_UNSUPPORTED
    assert make(n=65536, hop=4, precision=L.F64) == L.ERR_UNSUPPORTED
    # the pairs
    assert make(channels=0) == L.ERR_INVALID_SIZE
    assert make(npairs=0) == L.ERR_INVALID_SIZE
    assert make(pairs=None, npairs=2) == L.ERR_INVALID_ARG
    assert make(channels=3) == L.ERR_INVALID_ARG  # the pairs name channel 3
    assert b"pair 1 names channel 3 of 3" in lib.sdsp_hip_last_error_string()
    assert make(pairs=np.array([[0, 1], [4, 0]], dtype=np.uint32)) == L.ERR_INVALID_ARG
    # a workspace below one column: 4 channels x 1024 f32 + (2 x 5 + 4) x 513 doubles
    column = 4 * 1024 * 4 + (2 * 5 + 4) * 513 * 8
    assert make(ws=column - 1) == L.ERR_UNSUPPORTED
    assert str(column).encode() in lib.sdsp_hip_last_error_string()
    assert make(ws=1) == L.ERR_UNSUPPORTED
    assert lib.sdsp_hip_csd_plan_create(None, 1024, 256, w.ctypes.data, 0, 0, 1.0, 0, 4, 5, good.ctypes.data, 0, 0) == L.ERR_INVALID_ARG
    for ws in (0, column):
        rc = make(ws=ws)
        if torch.cuda.is_available():
            assert rc == 0
            lib.sdsp_hip_csd_plan_destroy(p)
        else:
            assert rc == L.ERR_NO_DEVICE
    assert lib.sdsp_hip_csd_plan_destroy(None) == 0
    assert lib.sdsp_hip_csd_state_bytes(None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_csd_plan_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_csd_plan_launches(None, 0, 0, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_csd_process(None, None, 0, 0, 0, None, None, 0, None, 0, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_csd_finalize(None, 0, None, 0, None, 0, 1, None, 0, None) == L.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        sd.csd_bank(64, 65, 2, [(0, 1)])
    with pytest.raises(ValueError):
        sd.csd_bank(64, 16, 2, [(0, 1)], window=np.ones(63))
    with pytest.raises(ValueError):
        sd.csd_bank(64, 16, 2, [(0, 1)], detrend="quadratic")
    with pytest.raises(ValueError):
        sd.csd_bank(64, 16, 2, [(0, 1)], scaling="power")
    with pytest.raises(ValueError):
        sd.csd_bank(64, 16, 2, [(0, 2)])
    with pytest.raises(ValueError):
        sd.csd_bank(64, 16, 2, [])
    with pytest.raises(ValueError):
        sd.csd_bank(64, 16, 0, [(0, 0)])
    assert sd.csd_bank(256, 56, 2, [(0, 1)]).segments(1000) == (1000 - 256) // 56 + 1


def test_one_shot_refuses_what_is_out_of_scope():
    x = torch.zeros(4096)  # host tensors: refused before any device work
    for fn in (sd.csd, sd.coherence):
        for kw in [dict(nfft=512), dict(nperseg=100), dict(noverlap=256), dict(detrend=lambda s: s)]:
            with pytest.raises(ValueError):
                fn(x, x, **kw)
        with pytest.raises(ValueError, match="device tensor"):
            fn(x, x)
    for kw, msg in [(dict(nfft=512), "nfft must equal nperseg"), (dict(nperseg=100), "power of two"),
                    (dict(noverlap=256), r"noverlap must be in \[0, nperseg\)"), (dict(detrend=abs), "detrend must be")]:
        with pytest.raises(ValueError, match=msg):
            sd.csd(x, x, **kw)
        with pytest.raises(ValueError, match=msg):
            sd.welch(x, **kw)  # the same messages
    with pytest.raises(TypeError):
        sd.coherence(x, x, scaling="spectrum")  # as scipy: coherence has no scaling
