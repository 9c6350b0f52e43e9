"""CPU checks of the symbol-timing recovery bank (include/sdsp_hip.h: sdsp_hip_timing_*): the host helpers
(step word, row capacity, gain designer, root-raised-cosine prototype), argument checking without a device, and the numpy reference
the GPU tests use (tests/timing_ref.py): its split invariance, its open loop against the resampler's reference, the row capacity
and that it locks."""
import ctypes as C
import math

import numpy as np
import pytest

from arb_ref import arb_ref
from timing_ref import (BLOCKS, LOCK_ROLLOFF, MODES, design, detector_slope, gains, lock_figures, lock_shape, lock_signal, max_out, rows_of,
                        state_bytes_of, step_of, timing_ref, timing_ref_stream, zero_state)

import simpledsp_amd as sd
from simpledsp_amd import _lib as L


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_timing_step_matches_the_formula_and_the_c_entry():
    lib = sd.load()
    for sps in (2, 2.37, 4, 8, 128, 3.0000001, 2 + 2.0 ** -31, 2 + 3 * 2.0 ** -32):
        w = C.c_uint64(0)
        assert lib.sdsp_hip_timing_step(float(sps), C.byref(w)) == 0
        assert w.value == sd.timing_step(sps) == step_of(sps) == round(sps / 2 * 2 ** 32)
        assert (1 << 32) <= w.value <= (1 << 38)
    assert sd.timing_step(2 + 2.0 ** -32) == 1 << 32 and sd.timing_step(2 + 3 * 2.0 ** -32) == (1 << 32) + 2  # ties to even
    w = C.c_uint64(7)
    for bad in (1.999, 128.001, float("nan"), float("inf"), -4.0):
        assert lib.sdsp_hip_timing_step(bad, C.byref(w)) == L.ERR_INVALID_ARG and w.value == 0
        with pytest.raises(ValueError):
            sd.timing_step(bad)
    assert lib.sdsp_hip_timing_step(4.0, None) == L.ERR_INVALID_ARG


def test_max_out_matches_the_formula_and_the_c_entry():
    lib = sd.load()
    rng = np.random.default_rng(2)
    cases = [(1 << 32, 0), (1 << 32, 1), (1 << 32, 1000), (1 << 38, 5), (1 << 38, (1 << 31) - 1), (1 << 32, (1 << 31) - 1)]
    cases += [(int(rng.integers(1 << 32, 1 << 38)), int(rng.integers(0, 1 << 20))) for _ in range(50)]
    for step0, S in cases:
        n = C.c_uint64(0)
        assert lib.sdsp_hip_timing_max_out_for(step0, S, C.byref(n)) == 0
        least = step0 - (1 << 31)
        strobes = -(-(S << 32) // least)
        assert n.value == sd.timing_max_out(step0, S) == max_out(step0, S) == (strobes + 1) // 2
    n = C.c_uint64(7)
    assert lib.sdsp_hip_timing_max_out_for((1 << 32) - 1, 5, C.byref(n)) == L.ERR_INVALID_SIZE and n.value == 0
    assert lib.sdsp_hip_timing_max_out_for((1 << 38) + 1, 5, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_timing_max_out_for(1 << 33, 1 << 31, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_timing_max_out_for(1 << 33, 5, None) == L.ERR_INVALID_ARG


def test_timing_gains_match_the_formulas_and_the_c_entry():
    lib = sd.load()
    eps = np.finfo(np.float64).eps
    for bn, zeta, kd, sps in ((0.01, math.sqrt(0.5), 1.0, 4.0), (0.005, 1.0, 3.52, 2.0), (0.02, 0.5, 0.3, 2.37)):
        theta = bn / (zeta + 1 / (4 * zeta))
        d = 1 + 2 * zeta * theta + theta ** 2
        want = (4 * zeta * theta / (d * kd) * sps / 2, 4 * theta ** 2 / (d * kd) * sps / 2)
        got = sd.timing_gains(bn, zeta, kd, sps)
        ca, cb = C.c_double(0), C.c_double(0)
        assert lib.sdsp_hip_timing_gains(bn, zeta, kd, sps, C.byref(ca), C.byref(cb)) == 0
        for g, c_, w, r in zip(got, (ca.value, cb.value), want, gains(bn, zeta, kd, sps)):
            assert abs(g - w) <= 4 * eps * w and abs(c_ - g) <= 4 * eps * w and abs(r - w) <= 4 * eps * w
    ca, cb = C.c_double(0), C.c_double(0)
    for bad in ((0.0, 0.7, 1.0, 4.0), (0.01, -1.0, 1.0, 4.0), (0.01, 0.7, 0.0, 4.0), (0.01, 0.7, 1.0, float("nan"))):
        assert lib.sdsp_hip_timing_gains(*bad, C.byref(ca), C.byref(cb)) == L.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            sd.timing_gains(*bad)
    assert lib.sdsp_hip_timing_gains(0.01, 0.7, 1.0, 4.0, None, C.byref(cb)) == L.ERR_INVALID_ARG


def test_timing_design_is_the_root_raised_cosine_and_nyquist_with_itself():
    """the C entry against the formula (timing_ref.design, the same closed form in numpy; both removable singularities are hit), the
    sum convention, the symmetry, and the matched pair: the prototype convolved with itself, at whole symbols from its centre, is zero
    within 3 e(tau_c), where tau_c is half the prototype's length in symbols and e(tau) = (4 b tau + 1) / (pi tau ((4 b tau)^2 - 1))
    bounds the pulse's envelope beyond tau: what the cut removes from each of the two factors"""
    lib = sd.load()
    for Lp, T, sps, ro in ((4, 32, 4, 0.35), (1, 32, 2, 0.35), (8, 64, 4, 0.5), (32, 32, 4, 0.35), (2, 64, 8, 1.0), (4, 48, 3, 0.25),
                           (1, 17, 2, 0.5), (128, 32, 4, 0.35)):
        h = sd.timing_design(Lp, T, sps, ro)
        want = design(Lp, T, sps, ro)
        # 64 eps of the peak: the sine and cosine arguments reach pi tau (1 + b), some tens of radians, and are themselves rounded to
        # about that many eps / 2 before two different libms evaluate them
        assert h.shape == (Lp * T,) and np.abs(h - want).max() <= 64 * np.finfo(np.float64).eps * np.abs(want).max()
        assert abs(h.sum() - Lp) <= 1e-12 * Lp and np.abs(h - h[::-1]).max() <= 1e-14 * np.abs(h).max()
        g = np.convolve(h, h)
        c = Lp * T - 1
        per = sps * Lp
        assert per == int(per)
        at = c + int(per) * np.arange(1, c // int(per) + 1)
        isi = np.abs(g[at]).max() / g[c]
        tau_c = T / sps / 2
        bound = 3 * (4 * ro * tau_c + 1) / (np.pi * tau_c * ((4 * ro * tau_c) ** 2 - 1))
        print(f"L {Lp} T {T} sps {sps} rolloff {ro}: worst |g| at whole symbols {isi:.2e} of the centre (bound {bound:.2e})")
        assert isi <= bound
    # (1, 17, 2, 0.5): tau = 1 / (4 b) = 0.5 symbols is tap 9, the centre tap 8
    h = sd.timing_design(1, 17, 2, 0.5)
    b = 0.5
    lim = b / math.sqrt(2) * ((1 + 2 / math.pi) * math.sin(math.pi / (4 * b)) + (1 - 2 / math.pi) * math.cos(math.pi / (4 * b)))
    assert abs(h[9] / h[8] - lim / (1 - b + 4 * b / math.pi)) <= 1e-14
    buf = np.zeros(16)
    assert lib.sdsp_hip_timing_design(3, 4, 4.0, 0.35, buf.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_timing_design(256, 1, 4.0, 0.35, buf.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_timing_design(1, 65, 4.0, 0.35, buf.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_timing_design(128, 64, 4.0, 0.35, buf.ctypes.data) == L.ERR_INVALID_SIZE  # L T > 4096
    assert lib.sdsp_hip_timing_design(4, 4, 4.0, 0.0, buf.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_design(4, 4, 4.0, 1.5, buf.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_design(4, 4, 0.0, 0.35, buf.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_design(4, 4, 4.0, 0.35, None) == L.ERR_INVALID_ARG


def test_arguments_are_checked_before_a_device_is_needed():
    """plan creation rejects its arguments before it looks for a device.  A plan cannot exist without a device, so without one the
    entry points are tried on a null plan; the checks that need a plan run below where a device is present, and in
    tests/test_gpu_timing.py"""
    import torch
    lib = sd.load()
    p = C.c_void_p()
    h = np.ones(4 * 5)

    def create(channels=4, precision=L.F32, mode=L.TIMING_GARDNER, phases=4, taps=5, h=h, step0=1 << 33, max_dev=0.25):
        return lib.sdsp_hip_timing_plan_create(C.byref(p), channels, precision, mode, phases, taps, None if h is None else h.ctypes.data,
                                               step0, max_dev, 0)

    assert create(channels=0) == L.ERR_INVALID_SIZE and create(channels=1 << 31) == L.ERR_INVALID_SIZE
    for bad in (0.0, -0.1, 0.5000001, float("nan"), float("inf"), 1e-60):  # 1e-60 rounds to 0 in f32
        assert create(max_dev=bad) == L.ERR_INVALID_ARG, bad
    assert b"max_dev" in lib.sdsp_hip_last_error_string()
    assert create(mode=3) == L.ERR_INVALID_ARG and create(mode=-1) == L.ERR_INVALID_ARG
    assert create(precision=L.F32_F64STATE) == L.ERR_INVALID_ARG and create(precision=9) == L.ERR_INVALID_ARG
    assert create(phases=3) == L.ERR_INVALID_SIZE and create(phases=0) == L.ERR_INVALID_SIZE and create(phases=256) == L.ERR_INVALID_SIZE
    assert create(taps=0) == L.ERR_INVALID_SIZE and create(taps=65) == L.ERR_INVALID_SIZE
    assert create(phases=128, taps=33) == L.ERR_INVALID_SIZE  # L T > 4096
    assert create(step0=(1 << 32) - 1) == L.ERR_INVALID_SIZE and create(step0=(1 << 38) + 1) == L.ERR_INVALID_SIZE
    assert b"step0" in lib.sdsp_hip_last_error_string()
    assert create(h=None) == L.ERR_INVALID_ARG
    bad_h = h.copy()
    bad_h[7] = np.nan
    assert create(h=bad_h) == L.ERR_INVALID_ARG
    bad_h[7] = 1e300  # not finite in f32
    assert create(h=bad_h) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_plan_create(None, 4, L.F32, 0, 4, 5, h.ctypes.data, 1 << 33, 0.5, 0) == L.ERR_INVALID_ARG
    # the other entry points on a null plan
    n = C.c_uint64(0)
    info = L.TimingPlanInfo()
    assert lib.sdsp_hip_timing_process(None, None, 8, None, 0, None, 0, None, 0, None, 8, 0.1, 0.01, None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_process_host(None, None, 8, None, 0, None, 0, None, 0, None, 8, 0.1, 0.01, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_state_bytes(None, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_max_out(None, 8, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_plan_launches(None, 1, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_plan_get_info(None, C.byref(info)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_timing_plan_destroy(None) == 0
    # what is left needs a device
    for kw in (dict(max_dev=0.5), dict(step0=1 << 32), dict(precision=L.F64, mode=L.TIMING_ZC_BPSK, step0=1 << 38)):
        rc = create(**kw)
        if torch.cuda.is_available():
            assert rc == 0
            # with a plan: NULL x, y or counts with S > 0
            assert lib.sdsp_hip_timing_process(p, None, 8, None, 0, None, 0, None, 0, None, 8, 0.1, 0.01, None, None) == L.ERR_INVALID_ARG
            lib.sdsp_hip_timing_plan_destroy(p)
        else:
            assert rc == L.ERR_NO_DEVICE
    if not torch.cuda.is_available():
        with pytest.raises(sd.SdspHipError):  # no CPU path
            sd.timing_bank(4, 4.0, h, 4)
    with pytest.raises(ValueError):
        sd.timing_bank(4, 4.0, np.ones(7), 4)
    with pytest.raises(ValueError):
        sd.timing_bank(4, 4.0, h, 4, mode="mm")
    with pytest.raises(ValueError):
        sd.timing_bank(4, 1.5, h, 4)


def _noise(rng, C_, S):
    return (rng.standard_normal((C_, S)) + 1j * rng.standard_normal((C_, S))) / np.sqrt(2.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_any_split_of_the_reference_gives_the_same_bits(precision, mode):
    """BLOCKS (empty and one-sample calls included) in units of 5 samples against one call, from a state that is not zero; the gains
    are strong enough for the loops to move, so the counts differ between channels"""
    rng = np.random.default_rng(4)
    C_, Lp, T = 5, 4, 5
    S = 5 * sum(BLOCKS)
    h = rng.standard_normal(Lp * T) / T
    x = _noise(rng, C_, S)
    step0 = step_of(2.37)
    _, _, _, _, st0, _ = timing_ref(h, Lp, T, _noise(rng, C_, 9), step0, 0.3, 0.05, mode, 0.25, None, precision)
    assert st0["parity"].any() or st0["t"].any()
    y, e, p, cnt, st, _ = timing_ref(h, Lp, T, x, step0, 0.3, 0.05, mode, 0.25, st0, precision)
    ys, es, ps, cnts, sts = timing_ref_stream(h, Lp, T, x, step0, [(5 * v, 0.3, 0.05) for v in BLOCKS], mode, 0.25, st0, precision)
    assert np.array_equal(cnt, cnts) and len(set(cnt.tolist())) > 1
    for one, parts in ((y, ys), (e, es), (p, ps)):
        for a, b in zip(rows_of(one, cnt), parts):
            assert a.dtype == b.dtype and _bits(a) == _bits(b)
    assert state_bytes_of(st) == state_bytes_of(sts)
    assert np.abs(p).max() <= 0.25 and np.abs(p).max() > 0  # the loop moved, inside its clamp


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1), (4, 5), (32, 16)])
def test_zero_gains_equal_the_nearest_phase_resampler_on_every_second_strobe(precision, shape):
    """alpha = beta = 0 free-runs at step0: the strobes are the outputs of arb_ref(..., interp="nearest") at that step, bit for bit, the
    symbol strobes being the odd ones (a fresh loop starts on a mid-symbol strobe); err is the detector on those values, period 0"""
    rng = np.random.default_rng(6)
    Lp, T = shape
    C_, S = 3, 211
    h = rng.standard_normal(Lp * T) / T
    x = _noise(rng, C_, S)
    for sps in (2, 2.37, 8):
        step0 = step_of(sps)
        want, _, next_time = arb_ref(h, Lp, T, x, step0, 0, None, "nearest", precision)
        for mode in MODES:
            y, e, p, cnt, st, _ = timing_ref(h, Lp, T, x, step0, 0.0, 0.0, mode, 0.5, None, precision)
            assert (cnt == want.shape[1] // 2).all()
            assert _bits(y[:, :cnt[0]]) == _bits(want[:, 1::2])
            assert not p.any() and not st["integ"].any() and not st["w"].any()
            assert (st["t"] == np.uint64(next_time)).all() and (st["parity"] == want.shape[1] % 2).all()
        assert np.abs(e).max() > 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_max_out_is_never_exceeded_with_the_advance_pinned_at_its_lowest(precision):
    """every w = -2^31, from a state that starts on a symbol strobe at t = 0 and from a fresh one: the counts stay within max_out, and
    reach it where the call begins on a symbol strobe"""
    rng = np.random.default_rng(8)
    Lp, T, C_ = 4, 5, 2
    h = rng.standard_normal(Lp * T) / T
    for sps in (2, 2.37, 3, 8):
        step0 = step_of(sps)
        for S in (0, 1, 2, 7, 64, 257):
            x = _noise(rng, C_, S)
            st = zero_state(C_, T, precision)
            st["parity"][1] = 1
            y, _, _, cnt, _, _ = timing_ref(h, Lp, T, x, step0, 0.3, 0.05, "gardner", 0.5, st, precision, pin_w=-(1 << 31))
            cap = max_out(step0, S)
            assert y.shape[1] == cap and (cnt <= cap).all() and cnt[1] == cap, (sps, S, cnt, cap)


# Lock bounds.  Measured on the reference over every case below (printed by the test): the mean of period over
# the last 1000 symbols is within 9.3e-6 samples of (true - nominal) / 2, and the tail's symbols lie within 0.054 RMS of the transmitted
# ones (noise of 0.05 per component through the matched filter, plus the cut pulse's self-interference); f32 and f64 agree to the
# digits shown.  The bounds are a little over 3 x those worst values.
LOCK_PERIOD_BOUND, LOCK_RMS_BOUND = 3e-5, 0.17
_KD = {}


def _kd(mode, sps):
    if (mode, sps) not in _KD:
        Lp, T = lock_shape(sps)
        _KD[mode, sps] = detector_slope(mode, sps, Lp, T, design(Lp, T, sps, LOCK_ROLLOFF))
    return _KD[mode, sps]


@pytest.mark.parametrize("bn", [0.005, 0.01])
@pytest.mark.parametrize("delta", [200e-6, -200e-6])
@pytest.mark.parametrize("sps", [2, 4])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_reference_locks(precision, mode, sps, delta, bn):
    Lp, T = lock_shape(sps)
    h = design(Lp, T, sps, LOCK_ROLLOFF)
    x, sym, tau0, period = lock_signal(mode, sps, delta)
    alpha, beta = gains(bn, math.sqrt(0.5), _kd(mode, sps), sps)
    y, e, p, cnt, st, times = timing_ref(h, Lp, T, x, step_of(sps), alpha, beta, mode, 0.5, None, precision)
    f_period, f_rms = lock_figures(y, p, cnt, times, sym, tau0, period, sps, Lp, T)
    print(f"{precision} {mode} sps {sps} delta {delta:+.0e} bn {bn}: kd {_kd(mode, sps):.4f}, |mean(period) - (true - nominal) / 2| = "
          f"{f_period:.2e} samples, rms = {f_rms:.4f}")
    assert f_period <= LOCK_PERIOD_BOUND
    assert f_rms <= LOCK_RMS_BOUND
