"""CPU checks of the forward-backward filtering plans (include/sdsp_hip.h: sdsp_hip_filtfilt_*): the double
reference of tests/filtfilt_ref.py against scipy.signal.sosfiltfilt, the library's steady state and default pad length against scipy,
the exported symbols, plan and argument validation without a device, and the store-hazard scan of iir_filtfilt.hip."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal
import torch

from conftest import ROOT
from filtfilt_ref import (BP, GENERIC, HP, LP, PADTYPES, default_padlen_ref, filtfilt_ref, random_stable, sos_of,
                          steady_state_ref)

import simpledsp_amd as sd

L = sd._lib
KINDS = [GENERIC, LP, HP, BP]


def _design(kind, m, rng):
    """a designed cascade of the kind (the library's Butterworth designs), or a random stable GENERIC one"""
    if kind == GENERIC:
        return random_stable(rng, m)
    a, b, g = np.zeros(3 * m), np.zeros(3 * m), C.c_double()
    lib = sd.load()
    if kind == LP:
        assert lib.sdsp_hip_iir_design_lp(m, 3e3, 48e3, 1.0, a.ctypes.data, b.ctypes.data, C.byref(g)) == 0
    elif kind == HP:
        assert lib.sdsp_hip_iir_design_hp(m, 3e3, 48e3, 1.0, a.ctypes.data, b.ctypes.data, C.byref(g)) == 0
    else:
        assert lib.sdsp_hip_iir_design_bp(m, 3e3, 48e3, 2.0, 1.0, a.ctypes.data, b.ctypes.data, C.byref(g)) == 0
    return a, None, g.value


@pytest.mark.parametrize("m", [2, 4, 6, 8, 10, 12, 14, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_is_sosfiltfilt(kind, m):
    rng = np.random.default_rng(10 * m + kind)
    a, b, g = _design(kind, m, rng)
    sos = sos_of(kind, a, b, g)
    P = default_padlen_ref(kind, a, b)
    x = rng.standard_normal((3, max(400, P + 50)))
    for padtype in ["odd", "even", "constant", None]:
        for padlen in [None, 0, 17, x.shape[1] - 1]:
            if padtype is None and padlen is not None:
                continue
            kw = {} if padlen is None else {"padlen": padlen}
            want = scipy.signal.sosfiltfilt(sos, x, padtype=padtype, **kw)
            got = filtfilt_ref(x, kind, a, b, g, PADTYPES[padtype], padlen)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (padtype, padlen)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [2, 4, 8, 16])
def test_steady_state_is_the_constant_input_response(kind, m):
    rng = np.random.default_rng(m + 7 * kind)
    a, b, g = _design(kind, m, rng)
    s = sd.iir_steady_state(m, kind, a, b, g)
    assert np.abs(s - steady_state_ref(kind, a, b, g)).max() <= 1e-15 * np.abs(s).max()
    # scipy: the steady output of sosfilt for a constant input is s_M v, and sosfilt_zi starts it there
    sos = sos_of(kind, a, b, g)
    v = 0.75
    zi = scipy.signal.sosfilt_zi(sos) * v
    y, _ = scipy.signal.sosfilt(sos, np.full(64, v), zi=zi)
    assert np.abs(y - s[-1] * v).max() <= 1e-12 * max(1.0, abs(s[-1] * v))
    assert s[0] == g


def test_default_padlen_is_scipys_edge():
    rng = np.random.default_rng(3)
    for m in (2, 4, 8, 16):
        for kind in KINDS:
            a, b, _ = _design(kind, m, rng)
            assert sd.filtfilt_default_padlen(m, kind, a, b) == 3 * (2 * m + 1) == default_padlen_ref(kind, a, b)
    # designs with zero b2 / a2: scipy subtracts min(#b2 == 0, #a2 == 0) sections
    a, b, g = random_stable(rng, 6)
    a, b = a.reshape(6, 3), b.reshape(6, 3)
    b[[0, 2, 3], 2] = 0.0
    a[[1, 2], 2] = 0.0
    sos = sos_of(GENERIC, a.reshape(-1), b.reshape(-1), g)
    want = 3 * (2 * 6 + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum()))
    assert want == 3 * (13 - 2)
    assert sd.filtfilt_default_padlen(6, GENERIC, a, b) == want == default_padlen_ref(GENERIC, a.reshape(-1), b.reshape(-1))
    b[[1, 4, 5], 2] = 0.0  # all six b2 zero, two a2 zero
    assert sd.filtfilt_default_padlen(6, GENERIC, a, b) == 3 * (13 - 2)
    # scipy's own edge on such a design: the padlen that equals its default
    x = rng.standard_normal(200)
    sos = sos_of(GENERIC, a.reshape(-1), b.reshape(-1), g)
    assert np.array_equal(scipy.signal.sosfiltfilt(sos, x), scipy.signal.sosfiltfilt(sos, x, padlen=3 * 11))


def test_new_symbols_are_exported():
    lib = sd.load()
    for name in ["sdsp_hip_iir_steady_state", "sdsp_hip_filtfilt_default_padlen", "sdsp_hip_filtfilt_plan_create",
                 "sdsp_hip_filtfilt_plan_destroy", "sdsp_hip_filtfilt_process", "sdsp_hip_filtfilt_process_host",
                 "sdsp_hip_filtfilt_plan_set_variant", "sdsp_hip_filtfilt_plan_kernel", "sdsp_hip_filtfilt_plan_launches",
                 "sdsp_hip_filtfilt_plan_get_info"]:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    hdr = (ROOT / "include" / "sdsp_hip.h").read_text()
    for name in ["SDSP_HIP_PAD_NONE 0", "SDSP_HIP_PAD_ODD 1", "SDSP_HIP_PAD_EVEN 2", "SDSP_HIP_PAD_CONSTANT 3"]:
        assert name in hdr
    assert C.sizeof(L.FiltfiltPlanInfo) == 4 * 7 + 4 + 8 + 8 + 64


def test_steady_state_and_padlen_errors():
    lib = sd.load()
    a, b, s, p = np.zeros(48), np.zeros(48), np.zeros(17), C.c_uint32(0)
    a[0::3] = 1.0
    assert lib.sdsp_hip_iir_steady_state(3, GENERIC, a.ctypes.data, b.ctypes.data, 1.0, s.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_iir_steady_state(0, GENERIC, a.ctypes.data, b.ctypes.data, 1.0, s.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_iir_steady_state(18, GENERIC, a.ctypes.data, b.ctypes.data, 1.0, s.ctypes.data) == L.ERR_UNSUPPORTED
    assert lib.sdsp_hip_iir_steady_state(4, 9, a.ctypes.data, b.ctypes.data, 1.0, s.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_iir_steady_state(4, GENERIC, a.ctypes.data, None, 1.0, s.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_iir_steady_state(4, LP, a.ctypes.data, None, 1.0, s.ctypes.data) == 0  # folded kinds need no b
    assert lib.sdsp_hip_iir_steady_state(4, LP, a.ctypes.data, None, 1.0, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_default_padlen(4, GENERIC, None, b.ctypes.data, C.byref(p)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_default_padlen(4, GENERIC, a.ctypes.data, b.ctypes.data, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_default_padlen(5, GENERIC, a.ctypes.data, b.ctypes.data, C.byref(p)) == L.ERR_INVALID_SIZE
    # a pole at z = 1 has no steady state: refused by the host function and at plan creation
    a[3 * 1 + 1], a[3 * 1 + 2] = -1.5, 0.5
    assert lib.sdsp_hip_iir_steady_state(4, GENERIC, a.ctypes.data, b.ctypes.data, 1.0, s.ctypes.data) == L.ERR_INVALID_ARG
    assert "1 + a1 + a2" in lib.sdsp_hip_last_error_string().decode()
    h = C.c_void_p()
    assert lib.sdsp_hip_filtfilt_plan_create(C.byref(h), 4, GENERIC, a.ctypes.data, b.ctypes.data, 1.0, L.F32, L.PAD_ODD, -1, 0,
                                             0) == L.ERR_INVALID_ARG
    with pytest.raises(sd.SdspHipError):
        sd.iir_steady_state(4, GENERIC, a[:12], b[:12], 1.0)


def test_plan_creation_errors_and_no_device():
    """argument errors come first; without a usable device a valid plan fails loudly (with one, it must succeed)"""
    lib = sd.load()
    rng = np.random.default_rng(1)
    a, b, g = random_stable(rng, 4)
    h = C.c_void_p()

    def make(m=4, kind=GENERIC, bb=b.ctypes.data, precision=L.F32, padtype=L.PAD_ODD, padlen=-1):
        return lib.sdsp_hip_filtfilt_plan_create(C.byref(h), m, kind, a.ctypes.data, bb, g, precision, padtype, padlen, 0, 0)

    assert make(m=3) == L.ERR_INVALID_SIZE
    assert make(m=18) == L.ERR_UNSUPPORTED
    assert make(kind=4) == L.ERR_INVALID_ARG
    assert make(bb=None) == L.ERR_INVALID_ARG
    assert make(precision=3) == L.ERR_INVALID_ARG
    assert make(padtype=4) == L.ERR_INVALID_ARG
    assert make(padtype=-1) == L.ERR_INVALID_ARG
    assert make(padlen=1 << 31) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_filtfilt_plan_create(None, 4, GENERIC, a.ctypes.data, b.ctypes.data, g, 0, 1, -1, 0, 0) == L.ERR_INVALID_ARG
    rc = make()
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_filtfilt_plan_destroy(h)
    else:
        assert rc == L.ERR_NO_DEVICE
    assert lib.sdsp_hip_filtfilt_plan_destroy(None) == 0
    n = C.c_uint64(5)
    assert lib.sdsp_hip_filtfilt_plan_launches(None, 1, 100, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_plan_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_plan_kernel(None, None, 1, 100, 100, C.create_string_buffer(64), 64) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_process(None, None, 1, 100, 100, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_process_host(None, None, 1, 100, 100) == L.ERR_INVALID_ARG


def test_python_argument_validation():
    with pytest.raises(ValueError):
        sd.filtfilt_plan(4, GENERIC, np.zeros(12), np.zeros(12), 1.0, padtype="reflect")
    with pytest.raises(ValueError):
        sd.filtfilt_plan(4, GENERIC, np.zeros(12), np.zeros(12), 1.0, padlen=-2)
    with pytest.raises(ValueError):
        sd.filtfilt_plan(4, GENERIC, np.zeros(11), np.zeros(12), 1.0)
    sos = scipy.signal.butter(4, 0.1, output="sos")
    x = torch.zeros((2, 100))
    with pytest.raises(ValueError):
        sd.sosfiltfilt(sos, x)  # host tensor
    with pytest.raises(ValueError):
        sd.sosfiltfilt(sos[:, :5], x)
    bad = sos.copy()
    bad[0, 0] = 0.0
    with pytest.raises(ValueError):
        sd.sosfiltfilt(bad, x)
    with pytest.raises(ValueError):
        sd.sosfiltfilt(np.vstack([sos] * 9), x)  # 18 sections


def test_no_wide_store_is_followed_by_a_write_to_its_data_registers():
    """the scan of tests/test_capi_host.py (profiles/r03_store_hazard.md) over the forward-backward kernels, built with the flags the
    library ships them with (iir.hip's: no FMA contraction, no SLP packing)"""
    from simpledsp_amd import build as B
    flags = B.SOURCES["iir_filtfilt.hip"]
    assert flags == B.SOURCES["iir.hip"]
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_store_hazard.py"),
                        str(ROOT / "simpledsp_amd" / "csrc" / "iir_filtfilt.hip"), *flags], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unguarded overwrites of store data: 0" in r.stdout
