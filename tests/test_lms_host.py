"""CPU checks of the LMS / NLMS adaptive filter bank (include/sdsp_hip.h: sdsp_hip_lms_*): the numpy reference
the GPU tests use (tests/lms_ref.py) against an independent scalar loop and against scipy.signal.lfilter, system identification to
the floor of the arithmetic, and argument checking without a device."""
import ctypes as C

import numpy as np
import pytest

from lms_ref import BLOCKS, lms_ref, lms_ref_stream

import simpledsp_amd as sd
from simpledsp_amd import _lib as L


def _scalar_lms(x, d, T, mu, mode, eps, w, h):
    """one channel, Python floats only (complex values as separate components): the contract read literally"""
    cplx = isinstance(x[0], complex)
    part = (lambda v: (v.real, v.imag)) if cplx else (lambda v: (float(v), 0.0))
    ext = [part(v) for v in list(h)[::-1]] + [part(v) for v in x]
    wr, wi = [part(v)[0] for v in w], [part(v)[1] for v in w]
    ys, es = [], []
    for n in range(len(x)):
        win = [ext[T - 1 + n - t] for t in range(T)]
        yr = yi = 0.0
        for t in range(T):
            vr, vi = win[t]
            if cplx:
                yr = wr[t] * vr + yr
                yr = yr - wi[t] * vi
                yi = wr[t] * vi + yi
                yi = wi[t] * vr + yi
            else:
                yr = wr[t] * vr + yr
        dr, di = part(d[n])
        er, ei = dr - yr, di - yi
        gr, gi = mu * er, mu * ei
        if mode == "nlms":
            p = 0.0
            for vr, vi in win:
                p = vr * vr + p
                if cplx:
                    p = vi * vi + p
            gr, gi = gr / (eps + p), gi / (eps + p)
        for t in range(T):
            vr, vi = win[t]
            if cplx:
                wr[t] = gr * vr + wr[t]
                wr[t] = gi * vi + wr[t]
                wi[t] = gi * vr + wi[t]
                wi[t] = wi[t] - gr * vi
            else:
                wr[t] = gr * vr + wr[t]
        ys.append(complex(yr, yi) if cplx else yr)
        es.append(complex(er, ei) if cplx else er)
    return ys, es, [complex(a, b) if cplx else a for a, b in zip(wr, wi)]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("mode", ["lms", "nlms"])
@pytest.mark.parametrize("cplx", [False, True])
def test_f64_reference_equals_a_scalar_loop_bit_for_bit(cplx, mode):
    rng = np.random.default_rng(3)
    C_, T, S = 3, 5, 60
    mk = lambda *s: rng.standard_normal(s) + (1j * rng.standard_normal(s) if cplx else 0)  # noqa: E731
    x, d, w0, h0 = mk(C_, S), mk(C_, S), 0.1 * mk(C_, T), mk(C_, T - 1)
    mu, eps = (0.5, 1e-3) if mode == "nlms" else (0.2 / T, 0.0)
    y, e, w, h = lms_ref(x, d, T, mu, mode, eps, w0, h0, "f64")
    for c in range(C_):
        conv = (lambda a: [complex(v) for v in a]) if cplx else (lambda a: [float(v) for v in a])
        ys, es, ws = _scalar_lms(conv(x[c]), conv(d[c]), T, mu, mode, eps, conv(w0[c]), conv(h0[c]))
        assert _bits(np.array(ys, dtype=y.dtype)) == _bits(y[c])
        assert _bits(np.array(es, dtype=y.dtype)) == _bits(e[c])
        assert _bits(np.array(ws, dtype=y.dtype)) == _bits(w[c])
    assert _bits(h) == _bits(np.concatenate([h0[:, ::-1], x], axis=1)[:, ::-1][:, :T - 1])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_any_split_of_the_reference_gives_the_same_bits(precision):
    rng = np.random.default_rng(4)
    C_, T = 4, 7
    S = 5 * sum(BLOCKS)
    x, d = rng.standard_normal((C_, S)), rng.standard_normal((C_, S))
    one = lms_ref(x, d, T, 0.5, "nlms", 1e-3, None, None, precision)
    parts = lms_ref_stream(x, d, T, [(5 * v, 0.5) for v in BLOCKS], "nlms", 1e-3, None, None, precision)
    for a, b in zip(one, parts):
        assert a.dtype == b.dtype and _bits(a) == _bits(b)


@pytest.mark.parametrize("cplx", [False, True])
def test_frozen_weights_are_an_fir_filter(cplx):
    """mu = 0: y = lfilter(w, 1, x) to 1e-12 relative, and the weights keep their bits"""
    import scipy.signal
    rng = np.random.default_rng(5)
    C_, T, S = 4, 33, 500
    mk = lambda *s: rng.standard_normal(s) + (1j * rng.standard_normal(s) if cplx else 0)  # noqa: E731
    x, d, w0 = mk(C_, S), mk(C_, S), mk(C_, T)
    for mode, eps in (("lms", 0.0), ("nlms", 1e-3)):
        y, e, w, _ = lms_ref(x, d, T, 0.0, mode, eps, w0, None, "f64")
        for c in range(C_):
            want = scipy.signal.lfilter(w0[c], 1.0, x[c])
            assert np.abs(y[c] - want).max() <= 1e-12 * np.abs(want).max()
        assert _bits(w) == _bits(w0.astype(w.dtype))
        assert _bits(e) == _bits(d - y)


@pytest.mark.parametrize("precision,bound", [("f64", 1e-12), ("f32", 2e-6)])
def test_system_identification_reaches_the_arithmetic_floor(precision, bound):
    """d = h * x, white x, no noise, T = 8, 64 channels: NLMS at mu = 1 and 0.5 in 2000 samples and LMS at mu = 0.2 / T in 4000 end
    with max |w - h| within the bound (measured: 4-7e-16 in f64, 1.2-2.4e-7 in f32; the expected decay (1 - mu (2 - mu) / T)^n is far
    below both)"""
    import scipy.signal
    rng = np.random.default_rng(6)
    C_, T = 64, 8
    h = rng.standard_normal((C_, T))
    for mode, mu, eps, S in (("nlms", 1.0, 1e-6, 2000), ("nlms", 0.5, 1e-6, 2000), ("lms", 0.2 / T, 0.0, 4000)):
        x = rng.standard_normal((C_, S))
        d = np.stack([scipy.signal.lfilter(h[c], 1.0, x[c]) for c in range(C_)])
        _, e, w, _ = lms_ref(x, d, T, mu, mode, eps, None, None, precision)
        err = np.abs(w.astype(np.float64) - h).max()
        print(f"{precision} {mode} mu = {mu:.4g}: max |w - h| = {err:.3e}, last |e| = {np.abs(e[:, -1]).max():.3e}")
        assert err <= bound, (mode, mu)


def test_plan_creation_checks_its_arguments_before_it_needs_a_device():
    import torch
    lib = sd.load()
    p = C.c_void_p()

    def create(channels=4, taps=8, kind=L.LMS_REAL, precision=L.F32, mode=L.LMS_NLMS, eps=1e-3):
        return lib.sdsp_hip_lms_plan_create(C.byref(p), channels, taps, kind, precision, mode, eps, 0)

    assert create(taps=0) == L.ERR_INVALID_SIZE and create(taps=65) == L.ERR_INVALID_SIZE
    assert create(taps=33, kind=L.LMS_COMPLEX, precision=L.F64) == L.ERR_INVALID_SIZE
    assert b"F64 COMPLEX" in lib.sdsp_hip_last_error_string()
    assert create(channels=0) == L.ERR_INVALID_SIZE and create(channels=1 << 31) == L.ERR_INVALID_SIZE
    assert create(kind=2) == L.ERR_INVALID_ARG and create(kind=-1) == L.ERR_INVALID_ARG
    assert create(precision=L.F32_F64STATE) == L.ERR_INVALID_ARG and create(precision=9) == L.ERR_INVALID_ARG
    assert create(mode=2) == L.ERR_INVALID_ARG and create(mode=-1) == L.ERR_INVALID_ARG
    for bad in (0.0, -1e-3, float("nan"), float("inf"), 1e-60):  # 1e-60 rounds to 0 in f32
        assert create(eps=bad) == L.ERR_INVALID_ARG, bad
    assert lib.sdsp_hip_lms_plan_create(None, 4, 8, L.LMS_REAL, L.F32, L.LMS_LMS, 0.0, 0) == L.ERR_INVALID_ARG
    # a null plan
    n = C.c_uint64(0)
    info = L.LmsPlanInfo()
    assert lib.sdsp_hip_lms_process(None, None, 0, None, 0, None, 0, None, 0, 0, 0.1, None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_lms_process_host(None, None, 0, None, 0, None, 0, None, 0, 0, 0.1, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_lms_state_bytes(None, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_lms_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_lms_plan_launches(None, 1, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_lms_plan_get_info(None, C.byref(info)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_lms_plan_destroy(None) == 0
    # what is left needs a device: LMS ignores eps, F64 COMPLEX takes 32 taps
    for kw in (dict(mode=L.LMS_LMS, eps=0.0), dict(taps=32, kind=L.LMS_COMPLEX, precision=L.F64), dict(taps=64)):
        rc = create(**kw)
        if torch.cuda.is_available():
            assert rc == 0
            lib.sdsp_hip_lms_plan_destroy(p)
        else:
            assert rc == L.ERR_NO_DEVICE
    if not torch.cuda.is_available():
        with pytest.raises(sd.SdspHipError):  # no CPU path
            sd.lms_bank(4, 8)
