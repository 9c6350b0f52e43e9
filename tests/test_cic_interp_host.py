"""CPU tests of the CIC interpolator bank (sdsp_hip_cic_interp_*): tests/cic_interp_ref.py, the numpy
reference of the contract, against a serial Hogenauer loop in Python integers and against the big-integer polyphase FIR form; the
identities the kernels rest on; the library's host helpers against Python integers; the register-width rule; every plan-creation
error, then ERR_NO_DEVICE without a device."""
import ctypes as C

import numpy as np
import pytest

from cic_interp_ref import (SHAPES, cic_interp_ref, fir_exact, gain, growth, hogenauer_serial, reg_bits, splits, stream_ref, taps_exact,
                            unity_scale)

import simpledsp_amd as sd
from simpledsp_amd import _lib as L


def _dtype(in_bits):
    return np.int32 if in_bits > 16 else np.int16


def _length(N, M):
    """a few histories"""
    return 3 * N * M + 5


def _rows(rng, N, M, in_bits):
    """three rows of full-range samples: random, the constant minimum (the worst case of the growth bound), the constant maximum"""
    S = _length(N, M)
    lo, hi = -(1 << (in_bits - 1)), (1 << (in_bits - 1)) - 1
    x = np.empty((3, S), dtype=_dtype(in_bits))
    x[0] = rng.integers(lo, hi + 1, S)
    x[1] = lo
    x[2] = hi
    return x


@pytest.mark.parametrize("N,R,M,in_bits", SHAPES)
def test_reference_against_the_serial_form_and_the_exact_fir_form(N, R, M, in_bits):
    """W = in_bits + growth bits exactly are enough: the serial form wrapped to that width, sign-extended, is the unbounded FIR form,
    also on the constant-minimum row, whose outputs reach -2^(in_bits - 1) R^(N-1) M^N and so need every one of those bits; and
    cic_interp_ref in its 32- or 64-bit registers gives the same values"""
    rng = np.random.default_rng(N * 1000 + R)
    x = _rows(rng, N, M, in_bits)
    tight = in_bits + growth(N, R, M)
    W = reg_bits(in_bits, N, R, M)
    assert tight <= W
    y, _ = cic_interp_ref(x, N, R, M, W)
    assert y.shape == (3, R * x.shape[1])
    for c in range(x.shape[0]):
        row = [int(v) for v in x[c]]
        exact = fir_exact(row, N, R, M)
        assert hogenauer_serial(row, N, R, M, tight) == exact
        assert hogenauer_serial(row, N, R, M, W) == exact
        assert [int(v) for v in y[c]] == exact
    steady = -(1 << (in_bits - 1)) * gain(N, R, M)
    assert all(int(v) == steady for v in y[1, -R:])  # every phase settles to the same value
    if growth(N, R, M) == 0:
        assert (N, R, M) == (1, 2, 1) and steady == -(1 << (in_bits - 1))  # a hold: the sample minimum itself
    else:
        # the bound is reached: the value fits tight bits of two's complement and not one fewer
        assert -(1 << (tight - 1)) <= steady < -(1 << (tight - 2))
        assert hogenauer_serial([int(v) for v in x[1]], N, R, M, tight - 1)[-1] != steady


@pytest.mark.parametrize("N,R,M,in_bits", SHAPES)
def test_reference_is_modular_for_inputs_wider_than_in_bits(N, R, M, in_bits):
    """with full-width samples in registers narrower than in_bits + growth the outputs wrap, and cic_interp_ref still equals the
    serial form of that width: the definition is modular"""
    rng = np.random.default_rng(N * 77 + R)
    x = rng.integers(-(1 << 31), 1 << 31, (2, _length(N, M))).astype(np.int32)
    for W in (32, 64):
        y, _ = cic_interp_ref(x, N, R, M, W)
        for c in range(2):
            assert [int(v) for v in y[c]] == hogenauer_serial([int(v) for v in x[c]], N, R, M, W)


@pytest.mark.parametrize("N,R,M,in_bits", SHAPES)
@pytest.mark.parametrize("cplx", [False, True])
def test_reference_streamed_equals_one_call(N, R, M, in_bits, cplx):
    """calls of 0, 1, 2, N M - 1, N M + 1 and the rest with the history carried: outputs and final history of one call"""
    rng = np.random.default_rng(N * 13 + R + cplx)
    S = 2 * N * M + 4 + _length(N, M)
    shape = (2, S, 2) if cplx else (2, S)
    x = rng.integers(-(1 << (in_bits - 1)), 1 << (in_bits - 1), shape).astype(_dtype(in_bits))
    state = rng.integers(-(1 << (in_bits - 1)), 1 << (in_bits - 1), (2, N * M) + shape[2:]).astype(x.dtype)
    W = reg_bits(in_bits, N, R, M)
    for out in ("int", "f32"):
        one, s_one = cic_interp_ref(x, N, R, M, W, state, out)
        many, s_many = stream_ref(x, splits(N, M, S), N, R, M, W, state, out)
        assert one.dtype == many.dtype and one.tobytes() == many.tobytes()
        assert s_one.tobytes() == s_many.tobytes()
        assert np.array_equal(s_one, x[:, ::-1][:, :N * M])  # S >= hist: the block's last samples, newest first
    if cplx:
        for p in range(2):  # the planes are independent real streams
            y, _ = cic_interp_ref(np.ascontiguousarray(x[..., p]), N, R, M, W, np.ascontiguousarray(state[..., p]))
            assert np.array_equal(y, cic_interp_ref(x, N, R, M, W, state)[0][..., p])
    # a history is the inputs in front of the block: one call over both, cut
    full = np.concatenate([state[:, ::-1], x], axis=1)
    assert np.array_equal(cic_interp_ref(full, N, R, M, W)[0][:, N * M * R:], cic_interp_ref(x, N, R, M, W, state)[0])


@pytest.mark.parametrize("N,R,M,in_bits", SHAPES)
def test_phase_sums_of_the_taps(N, R, M, in_bits):
    """every polyphase branch of h = boxcar(R M)^N sums to R^(N-1) M^N and has at most N M taps"""
    h = taps_exact(N, R, M)
    assert len(h) == N * (R * M - 1) + 1
    for p in range(R):
        assert sum(h[p::R]) == gain(N, R, M)
        assert len(h[p::R]) <= N * M
    assert all(v > 0 for v in h)  # so a constant-minimum input reaches the bound


def _warm_up_exact(x, N, R, M, W, m0, warm):
    """does a cascade started from zero registers at input m0 give the stream's outputs from input m0 + warm on?"""
    whole = hogenauer_serial(x, N, R, M, W)
    late = hogenauer_serial(x[m0:], N, R, M, W)
    return late[warm * R:] == whole[(m0 + warm) * R:]


@pytest.mark.parametrize("N,R,M,in_bits", SHAPES)
def test_zero_start_warm_up_identity(N, R, M, in_bits):
    """what lets a workgroup start anywhere: from zero registers N M inputs early, every later output is the stream's"""
    rng = np.random.default_rng(N * 31 + R)
    W = reg_bits(in_bits, N, R, M)
    x = [int(v) for v in rng.integers(-(1 << (in_bits - 1)), 1 << (in_bits - 1), 4 * N * M + 9)]
    for m0 in (1, 3, N * M + 2):
        assert _warm_up_exact(x, N, R, M, W, m0, N * M)
        assert _warm_up_exact(x, N, R, M, W, m0, -(-N * (R * M - 1) // R))  # the taps' own reach is enough as well


@pytest.mark.parametrize("N,R,M", [(8, 2, 1), (3, 3, 2)])
def test_a_warm_up_shorter_than_the_taps_reach_fails(N, R, M):
    rng = np.random.default_rng(N + R)
    x = [int(v) for v in rng.integers(-32768, 32768, 4 * N * M + 9)]
    short = -(-N * (R * M - 1) // R) - 1
    assert 0 < short < N * M
    assert not _warm_up_exact(x, N, R, M, 64, 3, short)


def test_float_output_rule():
    """(float)((double)y * scale): one conversion each way and one product, all to nearest even"""
    x = np.full((1, 12), -32768, dtype=np.int16)
    y, _ = cic_interp_ref(x, 3, 5, 1, 32, out="f32")
    assert y.dtype == np.float32 and y[0, -1] == np.float32(-32768.0 * 25 * (1.0 / 25.0))
    big = np.full((1, 12), 3, dtype=np.int16)
    yi, _ = cic_interp_ref(big, 5, 1024, 1, 64)
    yf, _ = cic_interp_ref(big, 5, 1024, 1, 64, out="f32", scale=3.0)
    assert int(yi[0, -1]) == 3 * 1024 ** 4 and yf[0, -1] == np.float32(float(3 * 1024 ** 4) * 3.0)


# ---------------------------------------------------------------------------------------------------------- the library's helpers

GROWTH_SHAPES = [(N, R, M) for N, R, M, _ in SHAPES] + [(8, 4096, 2), (2, 16384, 2), (8, 16, 1), (5, 256, 1), (5, 255, 1), (1, 16384, 1),
                                                        (1, 2, 2), (8, 8192, 1), (4, 16384, 1)]


def test_growth_and_unity_scale_against_python_integers():
    lib = sd.load()
    for N, R, M in GROWTH_SHAPES:
        assert sd.cic_interp_growth(N, R, M) == growth(N, R, M), (N, R, M)
        assert sd.cic_interp_unity_scale(N, R, M) == unity_scale(N, R, M), (N, R, M)
    assert sd.cic_interp_growth(1, 2, 1) == 0 and sd.cic_interp_unity_scale(1, 2, 1) == 1.0
    b, s = C.c_uint32(7), C.c_double(7.0)
    for bad in ((0, 2, 1), (9, 2, 1), (1, 1, 1), (1, 16385, 1), (1, 2, 0), (1, 2, 3), (8, 8192, 2), (5, 16384, 1)):
        assert lib.sdsp_hip_cic_interp_growth(*bad, C.byref(b)) == L.ERR_INVALID_SIZE, bad
        assert lib.sdsp_hip_cic_interp_unity_scale(*bad, C.byref(s)) == L.ERR_INVALID_SIZE, bad
        assert b.value == 0 and s.value == 0.0
    assert lib.sdsp_hip_cic_interp_growth(3, 5, 1, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cic_interp_unity_scale(3, 5, 1, None) == L.ERR_INVALID_ARG


def test_polyphase_taps_applied_mod_2_64_are_the_reference():
    """variant 1's form: sum_j h[p + j R] x[m - j] mod 2^64 with the library's taps equals cic_interp_ref"""
    from cic_interp_ref import wrap
    N, R, M = 8, 3, 2
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, 60).astype(np.int16)
    h = [int(v) for v in sd.cic_taps(N, R, M)]
    y, _ = cic_interp_ref(x[None], N, R, M, 64)
    for n in range(R * 60):
        m, p = divmod(n, R)
        acc = sum(h[k] * int(x[m - j]) for j, k in enumerate(range(p, len(h), R)) if m - j >= 0)
        assert wrap(acc, 64) == int(y[0, n])


def test_bank_arguments_and_the_width_rule():
    """W = 32 up to in_bits + growth = 32, 64 up to 64; the Python surface refuses what the C API refuses"""
    assert growth(3, 256, 1) == 16 and growth(4, 16, 2) == 16 and growth(6, 64, 1) == 30 and growth(8, 256, 2) == 64
    assert sd.cic_interpolator(3, 256, in_bits=16).reg_bits == 32      # 16 + 16 = 32
    assert sd.cic_interpolator(4, 16, 2).reg_bits == 32
    assert sd.cic_interpolator(6, 64).reg_bits == 64
    assert sd.cic_interpolator(3, 256, in_dtype="i32", in_bits=17).reg_bits == 64  # 33
    b = sd.cic_interpolator(3, 5)
    assert (b.hist, b.growth, b.reg_bits, b.scale) == (3, 5, 32, 1.0 / 25.0)
    assert b.out_samples(14) == 70
    with pytest.raises(ValueError):
        b.out_samples(1 << 31)
    for bad in (dict(kind="iq"), dict(in_dtype="i8"), dict(out="f64")):
        with pytest.raises(ValueError):
            sd.cic_interpolator(3, 5, **bad)
    with pytest.raises(sd.SdspHipError):
        sd.cic_interpolator(9, 5)
    with pytest.raises(ValueError):
        b.set_variant(2)
    with pytest.raises(ValueError):
        b.set_segment(1 << 20)


def test_plan_needs_a_device_and_says_so():
    """no CPU fallback: without a usable device, creation fails loudly (with one, it must succeed); the argument errors come first,
    the width rule at its boundaries 32 / 33 and 64 / 65 bits among them"""
    import torch
    lib = sd.load()
    p = C.c_void_p()
    create = lambda *a: lib.sdsp_hip_cic_interp_plan_create(C.byref(p), *a, 0)  # noqa: E731
    ok = (3, 5, 1, L.CIC_I16, 16, L.CIC_REAL, L.CIC_OUT_INT, 1.0)

    def with_(**kw):
        names = ("order", "up", "delay", "in_type", "in_bits", "kind", "out", "scale")
        a = dict(zip(names, ok))
        a.update(kw)
        return create(*[a[k] for k in names])

    for kw in (dict(order=0), dict(order=9), dict(up=1), dict(up=16385), dict(delay=0), dict(delay=3), dict(order=8, up=8192, delay=2),
               dict(in_bits=1), dict(in_bits=17), dict(in_type=L.CIC_I32, in_bits=33)):
        assert with_(**kw) == L.ERR_INVALID_SIZE, kw
    for kw in (dict(in_type=2), dict(kind=2), dict(out=2), dict(scale=float("nan")), dict(scale=float("inf"))):
        assert with_(**kw) == L.ERR_INVALID_ARG, kw
    assert lib.sdsp_hip_cic_interp_plan_create(None, *ok, 0) == L.ERR_INVALID_ARG
    # growth(8, 256, 2) = 64: one input bit more than the registers hold is refused before any device is asked for
    assert with_(order=8, up=256, delay=2, in_bits=2) == L.ERR_UNSUPPORTED
    msg = lib.sdsp_hip_last_error_string().decode()
    assert "2" in msg and "64" in msg and "66" in msg, msg
    assert growth(7, 1024, 1) == 60
    assert with_(order=7, up=1024, delay=1, in_bits=5) == L.ERR_UNSUPPORTED  # 5 + 60 = 65
    have = torch.cuda.is_available()
    info = L.CicInterpPlanInfo()
    # (in_bits, growth) at 32 | 33 and 64: W as the rule says
    for kw, W in ((dict(order=3, up=256, in_bits=16), 32), (dict(order=3, up=256, in_type=L.CIC_I32, in_bits=17), 64),
                  (dict(order=7, up=1024, in_bits=4), 64), (dict(), 32)):
        rc = with_(**kw)
        if have:
            assert rc == 0
            assert lib.sdsp_hip_cic_interp_plan_get_info(p, C.byref(info)) == 0
            assert info.reg_bits == W and info.in_bits + info.growth <= W and info.hist == info.order * info.delay
            lib.sdsp_hip_cic_interp_plan_destroy(p)
        else:
            assert rc == L.ERR_NO_DEVICE
