"""CPU checks of the FFT-domain FIR plan's size rule (sdsp_hip_fir_fft_size, include/sdsp_hip.h): no GPU needed."""
import ctypes as C

import pytest

import simpledsp_amd as sd


def _size(taps, precision):
    n = C.c_uint32(0)
    rc = sd.load().sdsp_hip_fir_fft_size(taps, precision, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("precision,max_taps,max_n", [(sd.F32, 16384, 32768), (sd.F64, 8192, 16384)])
def test_auto_size_is_a_valid_overlap_save_size(precision, max_taps, max_n):
    for taps in list(range(1, 300)) + [511, 512, 513, 1000, 1024, 2047, 4096, 4097, max_taps - 1, max_taps]:
        rc, n = _size(taps, precision)
        assert rc == 0, taps
        assert n & (n - 1) == 0, (taps, n)
        assert n >= 2 * (taps - 1) and n - taps + 1 >= 1, (taps, n)
        assert 16 <= n <= max_n, (taps, n)
        assert sd.fir_fft_size(taps, precision) == n


def test_auto_size_grows_with_taps():
    sizes = [_size(t, sd.F32)[1] for t in range(1, 16385, 97)]
    assert sizes == sorted(sizes)


@pytest.mark.parametrize("precision,max_taps", [(sd.F32, 16384), (sd.F64, 8192)])
def test_auto_size_errors(precision, max_taps):
    assert _size(0, precision)[0] == -1
    assert _size(max_taps + 1, precision)[0] == -1
    assert _size(1 << 30, precision)[0] == -1
    assert _size(100, 7)[0] == -5
    assert sd.load().sdsp_hip_fir_fft_size(100, precision, None) == -5
    with pytest.raises(sd.SdspHipError):
        sd.fir_fft_size(max_taps + 1, precision)


def test_fft_plan_needs_a_device_and_says_so():
    """no CPU fallback: without a usable device, creation fails loudly (with one, it must succeed)"""
    import numpy as np
    import torch
    h = np.ones(100)
    p = C.c_void_p()
    lib = sd.load()
    rc = lib.sdsp_hip_fir_fft_plan_create(C.byref(p), 100, h.ctypes.data, sd.F32, 0, 0, 0)
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_fir_plan_destroy(p)
    else:
        assert rc == -4
