"""CPU checks of the arbitrary-ratio polyphase resampler bank (include/sdsp_hip.h: sdsp_hip_arb_*): the host
helpers against Python integers, numpy and scipy.signal.firwin; the numpy reference the GPU tests use (tests/arb_ref.py) against the
textbook form, against resample_ref at rational steps and against itself when streamed; linear against nearest-phase accuracy; and
plan creation without a device."""
import ctypes as C

import numpy as np
import pytest

from arb_ref import ONE, RATIOS, SHAPES, SPLIT, arb_ref, hamming_sinc, out_samples, step_of, tables, textbook
from resample_ref import resample_ref

import simpledsp_amd as sd
from simpledsp_amd import _lib as L

STEPS = [1 << 22, ONE - 1, ONE, ONE + 1, 1 << 42]


def _lib_out(step, time, samples):
    n, t = C.c_uint64(77), C.c_uint64(77)
    rc = sd.load().sdsp_hip_arb_out_samples(step, time, samples, C.byref(n), C.byref(t))
    return rc, n.value, t.value


def test_step_is_the_rounded_scaled_ratio():
    rng = np.random.default_rng(1)
    for r in [1 / 1024, 1024.0, 1.0, 1.0000131, 2.37, 0.7317, 48000 / 44056, 1 + 2.0 ** -33, 1 + 3 * 2.0 ** -33, *rng.uniform(0.001, 1024, 20)]:
        assert sd.arb_step(r) == round(r * 2 ** 32), r  # Python's round: ties to even, on an exact product
    assert sd.arb_step(1 / 1024) == 1 << 22 and sd.arb_step(1024.0) == 1 << 42 and sd.arb_step(1.0) == ONE
    assert sd.arb_step(1 + 2.0 ** -33) == ONE and sd.arb_step(1 + 3 * 2.0 ** -33) == ONE + 2  # ties to even
    lib = sd.load()
    w = C.c_uint64(7)
    for bad in (1 / 1025, 1024.0001, 0.0, -1.0, float("nan"), float("inf")):
        assert lib.sdsp_hip_arb_step(bad, C.byref(w)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_arb_step(1.0, None) == L.ERR_INVALID_ARG
    with pytest.raises(sd.SdspHipError):
        sd.arb_step(2000.0)


@pytest.mark.parametrize("step", STEPS)
def test_out_samples_against_big_integers(step):
    for S in (0, 1, 7, 900, (1 << 31) - 1):
        for time in (0, step - 1, S << 32, (S << 32) + 12345, (1 << 63) - 1):
            n, nxt = out_samples(step, time, S)
            rc, gn, gt = _lib_out(step, time, S)
            if n >= 1 << 31:
                assert rc == L.ERR_INVALID_SIZE, (S, time)
                continue
            assert (rc, gn, gt) == (0, n, nxt), (S, time)
            if n:  # the last output lies inside the block, the next one does not
                assert (time + (n - 1) * step) >> 32 < S <= (time + n * step) >> 32


def test_out_samples_of_a_split_stream_and_the_error_codes():
    step = step_of(0.7317)
    one = out_samples(step, 0, sum(SPLIT))
    time, total = 0, 0
    for S in SPLIT:
        rc, n, time = _lib_out(step, time, S)
        assert rc == 0
        total += n
    assert total == one[0] == 1231 and time == one[1]  # ceil(900 / 0.7317)
    lib = sd.load()
    n, t = C.c_uint64(0), C.c_uint64(0)
    assert lib.sdsp_hip_arb_out_samples(ONE, 0, 8, C.byref(n), None) == 0 and n.value == 8  # next_time is optional
    assert lib.sdsp_hip_arb_out_samples(ONE, 0, 8, None, C.byref(t)) == L.ERR_INVALID_ARG
    assert _lib_out((1 << 22) - 1, 0, 8)[0] == L.ERR_INVALID_SIZE
    assert _lib_out((1 << 42) + 1, 0, 8)[0] == L.ERR_INVALID_SIZE
    assert _lib_out(ONE, 1 << 63, 8)[0] == L.ERR_INVALID_SIZE
    assert _lib_out(ONE, 0, 1 << 31)[0] == L.ERR_INVALID_SIZE
    assert _lib_out(1 << 22, 0, 1 << 21)[0] == L.ERR_INVALID_SIZE  # 2^31 outputs
    assert _lib_out(1 << 22, 1 << 22, 1 << 21) == (0, (1 << 31) - 1, 0)


@pytest.mark.parametrize("L_,T", SHAPES + [(1024, 4), (16, 256)])
def test_tables_against_numpy(L_, T):
    rng = np.random.default_rng(L_ + T)
    h = rng.standard_normal(L_ * T)
    Hd, Dd = np.zeros((L_, T)), np.zeros((L_, T))
    lib = sd.load()
    assert lib.sdsp_hip_arb_tables(L_, T, h.ctypes.data, Hd.ctypes.data, Dd.ctypes.data) == 0
    wantH, wantD = tables(h, L_, T)
    assert np.array_equal(Hd, wantH) and np.array_equal(Dd, wantD)
    # the row after phase L - 1 is phase 0 one tap later; behind the last tap lies zero
    assert np.array_equal(Dd[-1, :-1], Hd[0, 1:] - Hd[-1, :-1])
    assert Dd[-1, -1] == -h[-1]
    assert lib.sdsp_hip_arb_tables(3, T, h.ctypes.data, Hd.ctypes.data, Dd.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_arb_tables(2048, 1, h.ctypes.data, Hd.ctypes.data, Dd.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_arb_tables(L_, 0, h.ctypes.data, Hd.ctypes.data, Dd.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_arb_tables(L_, 4096 // L_ + 1, h.ctypes.data, Hd.ctypes.data, Dd.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_arb_tables(L_, T, None, Hd.ctypes.data, Dd.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_arb_tables(L_, T, h.ctypes.data, None, Dd.ctypes.data) == L.ERR_INVALID_ARG


def test_design_is_the_scaled_firwin():
    import scipy.signal
    lib = sd.load()
    for L_, T, ratio in [(32, 16, 0.7317), (128, 12, 2.37), (4, 5, 37.5), (1, 64, 4.0), (1024, 4, 1.0), (8, 8, 1 / 3.0001)]:
        h = np.zeros(L_ * T)
        assert lib.sdsp_hip_arb_design(L_, T, ratio, h.ctypes.data) == 0
        want = L_ * scipy.signal.firwin(L_ * T, min(1.0, 1.0 / ratio) / L_)
        assert np.abs(h - want).max() <= 1e-14 * L_, (L_, T, ratio)
        assert abs(h.sum() - L_) <= 1e-12 * L_
    h = np.zeros(64)
    assert lib.sdsp_hip_arb_design(1, 64, 1.0, h.ctypes.data) == L.ERR_INVALID_ARG  # no band to protect
    assert lib.sdsp_hip_arb_design(1, 64, 0.5, h.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_arb_design(8, 8, float("nan"), h.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_arb_design(8, 8, 2000.0, h.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_arb_design(8, 8, 2.0, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_arb_design(6, 8, 2.0, h.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_arb_design(8, 513, 2.0, h.ctypes.data) == L.ERR_INVALID_SIZE


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("L_,T", SHAPES)
def test_reference_against_the_textbook_form(L_, T, ratio):
    """f64 within 1e-12 (max over phases of sum|h|) max|x| of the piecewise-linear prototype evaluated at (k + f / 2^32) L, f32
    within 1e-6 normwise (max error over max magnitude); the margins are in DESIGN.md section 5.21"""
    rng = np.random.default_rng(L_ * 131 + T + int(ratio * 1000))
    step = step_of(ratio)
    S = T + int(40 * max(ratio, 1.0))
    time = int(rng.integers(0, step))
    h = rng.standard_normal(L_ * T)
    bound = np.abs(h.reshape(T, L_)).sum(axis=0).max()
    for cplx in (False, True):
        x = rng.standard_normal(S) + (1j * rng.standard_normal(S) if cplx else 0)
        want = textbook(h, L_, T, x, step, time)
        y64, _, _ = arb_ref(h, L_, T, x, step, time, None, "linear", "f64")
        e64 = np.abs(y64[0] - want).max() / (bound * np.abs(x).max())
        x32 = x.astype(np.complex64 if cplx else np.float32)
        want32 = textbook(h, L_, T, x32.astype(np.complex128 if cplx else np.float64), step, time)
        y32, _, _ = arb_ref(h, L_, T, x32, step, time, None, "linear", "f32")
        e32 = np.abs(y32[0] - want32).max() / np.abs(want32).max()
        print(f"L {L_} T {T} ratio {ratio} cplx {cplx}: f64 {e64:.2e} of 1e-12, f32 {e32:.2e} of 1e-6")
        assert e64 <= 1e-12
        assert e32 <= 1e-6


@pytest.mark.parametrize("L_,T,D", [(8, 8, 3), (4, 5, 7), (32, 4, 32)])
def test_nearest_at_a_rational_step_is_the_polyphase_resampler(L_, T, D):
    """step = D 2^32 / L, time 0, f64: the same products in the same order as resample_ref(h, x, L, D), bit for bit"""
    rng = np.random.default_rng(L_ + D)
    q = D // np.gcd(L_, D)
    S = int(q) * 40
    h = rng.standard_normal(L_ * T)
    x = rng.standard_normal((2, S))
    hist = rng.standard_normal((2, T - 1))
    assert (D << 32) % L_ == 0
    y, state, nxt = arb_ref(h, L_, T, x, (D << 32) // L_, 0, hist, "nearest", "f64")
    want, want_state = resample_ref(h, x, L_, D, hist)
    assert y.shape == want.shape and np.array_equal(y, want)
    assert np.array_equal(state, want_state) and nxt == 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("interp", ["nearest", "linear"])
def test_reference_streamed_equals_one_call(precision, interp):
    rng = np.random.default_rng(7)
    for (L_, T), ratio in zip(SHAPES, RATIOS):
        step = step_of(ratio)
        S = sum(SPLIT)
        for cplx in (False, True):
            x = rng.standard_normal((2, S)) + (1j * rng.standard_normal((2, S)) if cplx else 0)
            hist0 = rng.standard_normal((2, T - 1)) + (1j * rng.standard_normal((2, T - 1)) if cplx else 0)
            h = rng.standard_normal(L_ * T)
            time0 = int(rng.integers(0, step))
            want, want_state, want_time = arb_ref(h, L_, T, x, step, time0, hist0, interp, precision)
            got, state, time, s0 = [], hist0, time0, 0
            for b in SPLIT:
                y, state, time = arb_ref(h, L_, T, x[:, s0:s0 + b], step, time, state, interp, precision)
                got.append(y)
                s0 += b
            assert np.array_equal(np.concatenate(got, axis=1), want)
            assert np.array_equal(state, want_state) and time == want_time


@pytest.mark.parametrize("L_,T", [(32, 16), (128, 12)])
def test_linear_is_ten_times_closer_to_the_continuous_kernel_than_nearest(L_, T):
    """white noise through the sdsp_hip_arb_design prototype at ratio 0.7317; the truth is the continuous Hamming-windowed sinc the
    prototype samples"""
    rng = np.random.default_rng(L_)
    ratio = 0.7317
    step = step_of(ratio)
    h = np.zeros(L_ * T)
    assert sd.load().sdsp_hip_arb_design(L_, T, ratio, h.ctypes.data) == 0
    x = rng.standard_normal(400)
    truth = textbook(h, L_, T, x, step, 12345, kernel=hamming_sinc(L_, T, ratio))
    lin = np.abs(arb_ref(h, L_, T, x, step, 12345, None, "linear", "f64")[0][0] - truth).max()
    near = np.abs(arb_ref(h, L_, T, x, step, 12345, None, "nearest", "f64")[0][0] - truth).max()
    print(f"L {L_} T {T}: linear {lin:.2e}, nearest {near:.2e}")
    assert lin <= near / 10


def test_bank_arguments():
    b = sd.arb_resampler(32, 16, 2.37)
    assert b.max_step == step_of(2.37) and b.step == ONE and b.time == 0 and b.hist == 15
    b.step = 0.7317
    assert b.step == step_of(0.7317)
    assert b.out_samples(900) == out_samples(step_of(0.7317), 0, 900) and b.out_samples(900)[0] == 1231
    b.time = 5
    assert b.out_samples(0) == (0, 5)
    b.set_default_coeff()
    import scipy.signal
    assert np.abs(b.m_coeff - 32 * scipy.signal.firwin(512, ONE / b.max_step / 32)).max() < 1e-13  # the ratio the bank holds: max_step / 2^32
    with pytest.raises(ValueError):
        b.step = 2.38  # above max_step
    with pytest.raises(ValueError):
        b.step = 1 << 21
    with pytest.raises(ValueError):
        b.time = 1 << 63
    with pytest.raises(ValueError):
        b.set_coeff(np.ones(5))
    for bad in (-1, 2):
        with pytest.raises(ValueError):
            b.set_variant(bad)
    with pytest.raises(ValueError):
        sd.arb_resampler(32, 16, 2.0, kind="imaginary")
    with pytest.raises(ValueError):
        sd.arb_resampler(32, 16, 2.0, interp="cubic")
    with pytest.raises(sd.SdspHipError):
        sd.arb_resampler(32, 16, 2000.0)
    assert sd.arb_resampler(4, 4, 0.5).step == 1 << 31  # a bank that only interpolates starts at its largest step


def test_plan_needs_a_device_and_says_so():
    """no CPU fallback: without a usable device, creation fails loudly (with one, it must succeed); the argument errors come first"""
    import torch
    lib = sd.load()
    h = np.ones(512)
    p = C.c_void_p()
    create = lambda phases, taps, hp, max_step, kind, interp, prec: lib.sdsp_hip_arb_plan_create(  # noqa: E731
        C.byref(p), phases, taps, hp, max_step, kind, interp, prec, 0)
    ok = (32, 16, h.ctypes.data, ONE, L.ARB_REAL, L.ARB_LINEAR, L.F32)

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return create(*a)

    for phases in (0, 3, 48, 2048):
        assert with_(0, phases) == L.ERR_INVALID_SIZE
    assert with_(1, 0) == L.ERR_INVALID_SIZE
    assert with_(1, 129) == L.ERR_INVALID_SIZE  # 32 x 129 > 4096
    assert with_(3, (1 << 22) - 1) == L.ERR_INVALID_SIZE
    assert with_(3, (1 << 42) + 1) == L.ERR_INVALID_SIZE
    assert with_(2, None) == L.ERR_INVALID_ARG
    assert with_(4, 2) == L.ERR_INVALID_ARG
    assert with_(5, 2) == L.ERR_INVALID_ARG
    assert with_(6, L.F32_F64STATE) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_arb_plan_create(None, *ok, 0) == L.ERR_INVALID_ARG
    rc = create(*ok)
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_arb_plan_destroy(p)
    else:
        assert rc == L.ERR_NO_DEVICE
