"""CPU checks of tests/recur_exact.py, the bit-level checker of the biquad and FIR banks (no device):

* its fused multiply-adds are correctly rounded: against glibc on random and cancelling triples, and against exact rational
  arithmetic on triples CONSTRUCTED to sit next to a rounding midpoint, where the naive float32 emulation (product and sum in
  double, then one narrowing) is shown to double-round;
* its f64 model is the CPU oracle's recurrence bit for bit, every kind, state carried across calls;
* five planted defects pass the rules of tests/test_gpu_iir.py / test_gpu_fir.py (1e-6, or 1.2e-7 in mixed mode, on the rows those
  files pick) and fail R1; the one that is a value error large enough to matter (a channel restarted from zero state) fails R2 too;
* the model itself passes R2 on every case of the GPU tables."""
import ctypes
import ctypes.util
from fractions import Fraction

import numpy as np
import pytest

import recur_exact as rx
import test_gpu_biquad_exact as bq
import test_gpu_fir_exact as fq
from conftest import rel_max_err
from filtfilt_ref import random_stable, steady_state_ref

F32, F64 = np.float32, np.float64


# --------------------------------------------------------------------------------------------------------------------- FMA
@pytest.fixture(scope="module")
def libm():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.fmaf.restype, lib.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    lib.fma.restype, lib.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    return lib


def _triples(rng, n, T, mant_bits):
    """random triples over 40 binades, a third of them with c within a few ulps of -ab (cancellation)"""
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(T)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(T)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(T)
    near = -(a.astype(F64) * b.astype(F64)) * (1 + rng.integers(-4, 5, n) * 2.0 ** -mant_bits)
    return a, b, np.where(rng.random(n) < 1 / 3, near, c).astype(T)


def _same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def test_fmaf_and_fma_against_glibc(libm):
    rng = np.random.default_rng(1)
    n = 100_000
    a, b, c = _triples(rng, n, F32, 23)
    want = np.array([libm.fmaf(*t) for t in zip(a.tolist(), b.tolist(), c.tolist())], dtype=F32)
    assert _same_bits(rx.fmaf(a, b, c), want)
    a, b, c = _triples(rng, n, F64, 52)
    want = np.array([libm.fma(*t) for t in zip(a.tolist(), b.tolist(), c.tolist())], dtype=F64)
    assert _same_bits(rx.fma(a, b, c), want)


def _round_fraction(fr, bits):
    """the exact rational fr rounded to nearest, ties to even, at `bits` significant bits (no exponent limit), as a Fraction"""
    if fr == 0:
        return Fraction(0)
    sign, fr = (-1 if fr < 0 else 1), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1)
    unit = Fraction(2) ** (e - bits + 1)
    q, r = divmod(fr / unit, 1)
    q = int(q)
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and q & 1):
        q += 1
    return sign * q * unit


def _midpoint_triples(rng, n, T, bits):
    """triples whose exact ab + c lies within 2^-30 (relative) of the midpoint of two adjacent results, never on it.
    Two families, in units where c is in [2^bits, 2^(bits+1)) (ulp 2, midpoints at the odd integers):
      far   a = 1 + k eps, b = 1 - k eps: ab = 1 - k^2 eps^2, short of the midpoint by less than a double's own half ulp, so a sum
            formed in double lands ON the midpoint and the narrowing then rounds to even: the double-rounding cases
      near  a = 2 j + 1, b = 1 + i eps with (2 j + 1) i <= 2^(bits - 7): ab = an odd integer + (2 j + 1) i eps, past the midpoint by
            up to 2^-30 relative
    then every operand is scaled by a power of two and given a sign (both exact)."""
    eps = 2.0 ** -(bits - 1)
    out = []
    for fam in ("far", "near"):
        m = n // 2
        # even integers with random mantissas, odd and even, at least 128 inside the binade (c +- ab stays in it)
        c = (2.0 ** bits + 2.0 * rng.integers(64, 2 ** (bits - 1) - 64, m)).astype(T)
        if fam == "far":
            k = rng.integers(1, 300, m)
            a, b = (1 + k * eps).astype(T), (1 - k * eps).astype(T)
        else:
            j = rng.integers(0, 2 ** 5, m)
            i = rng.integers(1, 2 ** (bits - 7) // (2 * j + 1) + 1)
            a, b = (2.0 * j + 1).astype(T), (1 + i * eps).astype(T)
        sa, sc = rng.choice([-1.0, 1.0], m), rng.choice([-1.0, 1.0], m)
        pa, pb = 2.0 ** rng.integers(-10, 11, m), 2.0 ** rng.integers(-10, 11, m)
        out.append(((a * sa * pa).astype(T), (b * pb).astype(T), (c * sc * pa * pb).astype(T)))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(3))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_fma_on_constructed_midpoint_triples(prec):
    T, bits = (F32, 24) if prec == "f32" else (F64, 53)
    rng = np.random.default_rng(2)
    a, b, c = _midpoint_triples(rng, 3000, T, bits)
    want = np.empty(a.size, dtype=T)
    for i, (x, y, z) in enumerate(zip(a.tolist(), b.tolist(), c.tolist())):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        r = _round_fraction(exact, bits)
        # the construction: one more bit of precision would land ON the midpoint's neighbourhood, within 2^-30 relative, not on it
        mid = _round_fraction(exact, bits + 1)
        assert mid != r and 0 < abs(exact - mid) <= abs(exact) / 2 ** 30, (x, y, z)
        want[i] = T(float(r))
        assert Fraction(float(want[i])) == r
    got = rx.fmaf(a, b, c) if prec == "f32" else rx.fma(a, b, c)
    assert _same_bits(got, want), int((got != want).sum())
    if prec == "f32":
        # the naive emulation double-rounds on the "far" family (where c's mantissa is odd): this is why the library rounds to odd
        naive = (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)
        wrong = int((naive != want).sum())
        assert wrong >= 1, "the constructed triples do not exercise double rounding"
        assert wrong >= a.size // 8  # about half of the far family


# ------------------------------------------------------------------------------------------------------ model against the oracle
def _oracle_bank(oracle, m, kind, a, b, g, state, x):
    """the oracle over the rows of x from a device-layout state: (y, final state in the device layout)"""
    channels = x.shape[0]
    y, final = np.empty_like(x), np.empty_like(state)
    for c in range(channels):
        fo = oracle.iir(m)
        fo.set_design(a, b if b is not None else np.zeros(3 * m), g)
        for j in range(m + 1):
            for age in range(3):  # pos = 0: age k (1-based) sits at ring index (0 - k) % 3
                fo._s.mem[3 * j + (-(age + 1)) % 3] = state[3 * j + age, c]
        fo._s.pos = 0
        y[c] = fo.process(x[c], kind)
        mem, pos = fo.mem, fo.pos
        for age in range(3):
            final[age::3, c] = mem[:, (pos - 1 - age) % 3]
    return y, final


@pytest.mark.parametrize("m", [2, 4, 8, 16])
@pytest.mark.parametrize("kind", [rx.GENERIC, rx.LP, rx.HP, rx.BP])
def test_f64_model_is_the_oracle(oracle, m, kind):
    rng = np.random.default_rng(10 * m + kind)
    # (moderate cutoffs: a unit-normal state at every level of 16 low-cutoff sections overflows a float recurrence)
    a, b, g = bq.coefficients(oracle.iir(m), kind, m, {rx.GENERIC: "rand1", rx.LP: "base", rx.HP: "hp10k", rx.BP: "bp"}[kind])
    bb = b if kind == rx.GENERIC else None
    x = rng.standard_normal((5, 301))
    state = rng.standard_normal((3 * (m + 1), 5))
    want, want_state = _oracle_bank(oracle, m, kind, a, bb, g, state, x)
    y, st = rx.biquad_model(x, a, bb, g, kind, "f64", state)
    assert _same_bits(y, want) and _same_bits(st, want_state)
    # two calls, the state carried: the same bits, in the model and in the oracle
    y1, s1 = rx.biquad_model(x[:, :100], a, bb, g, kind, "f64", state)
    y2, s2 = rx.biquad_model(x[:, 100:], a, bb, g, kind, "f64", s1)
    assert _same_bits(np.concatenate([y1, y2], axis=1), want) and _same_bits(s2, want_state)
    w1, ws1 = _oracle_bank(oracle, m, kind, a, bb, g, state, x[:, :100])
    assert _same_bits(y1, w1) and _same_bits(s1, ws1)
    # the baseline of R2 is that recurrence too, and the fused forms carry state across calls the same way
    assert _same_bits(rx.biquad_plain(x, a, bb, g, kind, "f64", state)[0], want)
    for precision in ("f32", "mix"):
        xs, ss = x.astype(rx.SDT[precision]), state.astype(rx.RDT[precision])
        whole = rx.biquad_model(xs, a, bb, g, kind, precision, ss)
        p1 = rx.biquad_model(xs[:, :100], a, bb, g, kind, precision, ss)
        p2 = rx.biquad_model(xs[:, 100:], a, bb, g, kind, precision, p1[1])
        assert _same_bits(np.concatenate([p1[0], p2[0]], axis=1), whole[0]) and _same_bits(p2[1], whole[1])
        assert whole[0].dtype == rx.SDT[precision] and whole[1].dtype == rx.RDT[precision]


@pytest.mark.parametrize("taps", [1, 2, 17, 64])
def test_f64_fir_plain_is_the_oracle(oracle, taps):
    rng = np.random.default_rng(taps)
    h = rng.standard_normal(taps)
    x = rng.standard_normal((3, 50))
    hist = rng.standard_normal((3, max(taps - 1, 1)))
    y, final = rx.fir_plain(x, h, hist, "f64")
    for c in range(3):
        want, mem = oracle.fir_process(h, x[c], hist[c])
        assert _same_bits(y[c], want) and _same_bits(final[c], mem[:taps - 1])
    # short rows keep the older history; blocks give the bits of one call
    y1, h1 = rx.fir_plain(x[:, :7], h, hist, "f64")
    y2, h2 = rx.fir_plain(x[:, 7:], h, h1 if taps > 1 else None, "f64")
    assert _same_bits(np.concatenate([y1, y2], axis=1), y) and _same_bits(h2, final)
    x32, hist32 = x.astype(F32), hist.astype(F32)
    m1, g1 = rx.fir_model_f32(x32[:, :7], h, hist32)
    m2, g2 = rx.fir_model_f32(x32[:, 7:], h, g1 if taps > 1 else None)
    whole = rx.fir_model_f32(x32, h, hist32)
    assert _same_bits(np.concatenate([m1, m2], axis=1), whole[0]) and _same_bits(g2, whole[1])


# ------------------------------------------------------------------------------------------------------------ planted defects
def _old_rule_iir(oracle, got, x, a, b, g, kind, m, rows, tol):
    """tests/test_gpu_iir.py's check: rel_max_err against the double oracle (double coefficients) on the picked rows"""
    for c in rows:
        fo = oracle.iir(m)
        fo.set_design(a, b if b is not None else np.zeros(3 * m), g)
        err = rel_max_err(got[c], fo.process(x[c].astype(F64), kind))
        if not err < tol:
            return False
    return True


def _picks(rng, channels):
    """test_f32_bank_against_oracle's rows: first, last and up to eight drawn ones"""
    return sorted(set([0, channels - 1] + list(rng.choice(channels, min(channels, 8)))))


DEFECT_A_SEED = 104  # filtfilt_ref.random_stable(default_rng(104), 4): test_gpu_filtfilt's "rand" cascade of four sections


def test_defect_a_unfused_f32_generic(oracle):
    """(a) the unfused form in f32 GENERIC on a cascade with arbitrary zeros: a reordering -- R1 fails, R2 holds (it IS the baseline).
    On the Butterworth low-pass (b1 = 2, b2 = 1) the two forms cannot be told apart at all."""
    m = 4
    a, b, g = random_stable(np.random.default_rng(DEFECT_A_SEED), m)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((130, 400)).astype(F32)
    rows = _picks(rng, 130)
    good, _ = rx.biquad_model(x, a, b, g, rx.GENERIC, "f32")
    bad, _ = rx.biquad_plain(x, a, b, g, rx.GENERIC, "f32")
    ld, _ = rx.biquad_ld(x, a, b, g, rx.GENERIC, "f32")
    assert _old_rule_iir(oracle, good, x, a, b, g, rx.GENERIC, m, rows, 1e-6)
    assert _old_rule_iir(oracle, bad, x, a, b, g, rx.GENERIC, m, rows, 1e-6)
    n, first = rx.bit_diff(bad, good)
    assert n > 0.3 * good.size, n  # 84 % of the outputs here
    assert rx.r1(bad, good, "defect a") and not rx.r2(bad, bad, ld, "f32")[0]
    assert "different rounding" in rx.verdict([rx.r1(bad, good, "defect a")], rx.r2(bad, bad, ld, "f32")[0])
    lo = oracle.iir(m)
    lo.set_lp_coeff(10e3, 100e3)
    la, lb, lg = lo.a.reshape(-1), lo.b.reshape(-1), lo.gain
    assert rx.bit_diff(rx.biquad_plain(x, la, lb, lg, rx.GENERIC, "f32")[0], rx.biquad_model(x, la, lb, lg, rx.GENERIC, "f32")[0])[0] == 0


def test_defect_b_gain_in_float_in_mixed_mode(oracle):
    """(b) mixed mode with `gain` applied in float before widening: a value error of a rounded gain and one rounding per input
    sample (e2 2.5 u here, next to the baseline's 0.5 u).  The 1.2e-7 (= 2.0 u, einf) rule on row 33 lets it through and R1 does
    not.  R2 does not see it either: every row carries the same relative error, so what passes 2.0 u on the picked row is under
    3 max(baseline, 1 u) on all of them.  In mixed mode R2 is the looser of the two rules and only adds the unpicked rows."""
    m = 4
    fo = oracle.iir(m)
    fo.set_lp_coeff(500.0, 100e3)
    a, g = fo.a.reshape(-1), fo.gain
    rng = np.random.default_rng(4)
    x = rng.standard_normal((70, 400)).astype(F32)
    good, good_state = rx.biquad_model(x, a, None, g, rx.LP, "mix")
    bad, bad_state = rx.biquad_model(x * F32(g), a, None, 1.0, rx.LP, "mix")
    ld, _ = rx.biquad_ld(x, a, None, g, rx.LP, "mix")
    plain, _ = rx.biquad_plain(x, a, None, g, rx.LP, "mix")
    for got in (good, bad):
        assert _old_rule_iir(oracle, got, x, a, None, g, rx.LP, m, [33], 1.2e-7)
    assert rx.r1(bad, good, "defect b") and rx.r1(bad_state, good_state, "defect b state")
    msg, fig = rx.r2(bad, plain, ld, "mix")
    assert not msg and 2 * fig["base2"] < fig["e2"] <= 3.0, fig


def test_defect_c_y3_plane_is_a_copy_of_y2(oracle):
    """(c) the third age of every level stored as a copy of the second: no output changes (the recurrence reads two ages), so only
    R1 on the final state sees it"""
    m = 4
    fo = oracle.iir(m)
    fo.set_lp_coeff(10e3, 100e3)
    a, b, g = fo.a.reshape(-1), fo.b.reshape(-1), fo.gain
    rng = np.random.default_rng(5)
    x = rng.standard_normal((70, 200)).astype(F32)
    y, state = rx.biquad_model(x, a, b, g, rx.GENERIC, "f32")
    bad_state = state.copy()
    bad_state[2::3] = bad_state[1::3]
    assert _old_rule_iir(oracle, y, x, a, b, g, rx.GENERIC, m, _picks(rng, 70), 1e-6)
    msg = rx.r1(bad_state, state, "defect c state")
    assert msg and not rx.r1(y, y, "defect c output")
    n, first = rx.bit_diff(bad_state, state)
    assert first[0] % 3 == 2 and n > 0.9 * 5 * 70


def test_defect_d_one_unpicked_channel_restarts_from_zero(oracle):
    """(d) channel 37 of 130 loses its state at a call boundary: a value error -- R1 and R2 both fail, the picked rows do not"""
    m = 4
    fo = oracle.iir(m)
    fo.set_lp_coeff(10e3, 100e3)
    a, b, g = fo.a.reshape(-1), fo.b.reshape(-1), fo.gain
    channels, samples = 130, 400
    rng = np.random.default_rng(channels * 7 + samples)
    x = rng.standard_normal((channels, samples)).astype(F32)
    rows = _picks(rng, channels)
    assert 37 not in rows
    good, good_state = rx.biquad_model(x, a, b, g, rx.GENERIC, "f32")
    y1, s1 = rx.biquad_model(x[:, :200], a, b, g, rx.GENERIC, "f32")
    s1 = s1.copy()
    s1[:, 37] = 0
    y2, s2 = rx.biquad_model(x[:, 200:], a, b, g, rx.GENERIC, "f32", s1)
    bad = np.concatenate([y1, y2], axis=1)
    assert _old_rule_iir(oracle, bad, x, a, b, g, rx.GENERIC, m, rows, 1e-6)
    msg = rx.r1(bad, good, "defect d")
    assert msg and "(37, 200)" in msg
    ld, _ = rx.biquad_ld(x, a, b, g, rx.GENERIC, "f32")
    plain, _ = rx.biquad_plain(x, a, b, g, rx.GENERIC, "f32")
    r2, _ = rx.r2(bad, plain, ld, "f32")
    assert "first 37" in r2 and "fails too" in rx.verdict([msg], r2)
    assert not rx.r2(good, plain, ld, "f32")[0]


def test_defect_e_fir_descending_taps(oracle):
    """(e) the f32 FIR sum taken from the last tap down: a reordering -- the 1e-6 rule on three rows passes, R1 fails, R2 holds"""
    taps = 33
    h = oracle.fir_design(taps, 1, 10e3, 100e3)
    rng = np.random.default_rng(6)
    x = rng.standard_normal((70, 300)).astype(F32)
    good, _ = rx.fir_model_f32(x, h)
    h32 = h.astype(F32)
    ext = np.concatenate([np.zeros((70, taps - 1), F32), x], axis=1)
    bad = np.zeros_like(x)
    for k in range(taps - 1, -1, -1):
        bad = rx.fmaf(h32[k], ext[:, taps - 1 - k:taps - 1 - k + 300], bad)
    for got in (good, bad):
        for c in (0, 7, 69):
            assert rel_max_err(got[c], oracle.fir_process(h32.astype(F64), x[c].astype(F64))[0]) < 1e-6
    assert rx.r1(bad, good, "defect e", ignore_zero_sign=True)
    assert not rx.r2(bad, rx.fir_plain(x, h, None, "f32")[0], rx.fir_ld(x, h, None, "f32"), "f32")[0]


def test_zero_signs_count_only_where_the_rule_says():
    a, b = np.array([[0.0, 1.0]], F32), np.array([[-0.0, 1.0]], F32)
    assert rx.bit_diff(a, b) == (1, (0, 0)) and rx.bit_diff(a, b, ignore_zero_sign=True) == (0, None)


# ---------------------------------------------------------------------------------------------- R2 on the model, every table case
@pytest.mark.parametrize("case", bq.CASES + bq.INTERLEAVED_CASES, ids=bq.case_id)
def test_biquad_model_passes_r2_on_the_gpu_table(oracle, case):
    precision, kind, m, name = case[:4]
    a, b, g = bq.coefficients(oracle.iir(m), kind, m, name)
    ref = bq.reference(case, a, b, g)
    msg, fig = rx.r2(ref["y"], ref["plain"], ref["ld"], precision)
    assert not msg, (msg, fig)
    assert np.all(ref["state"] != 0)
    if precision != "f64" and kind != rx.GENERIC:  # the case tells the fused form from the unfused one (in double: now and then)
        assert rx.bit_diff(ref["y"], ref["plain"])[0] > 0 or precision == "mix"


@pytest.mark.parametrize("case", fq.CASES, ids=fq.case_id)
def test_fir_model_passes_r2_on_the_gpu_table(case):
    ref = fq.reference(case, "f32")
    msg, fig = rx.r2(ref["y"], ref["plain"], ref["ld"], "f32")
    assert not msg, (msg, fig)


@pytest.mark.parametrize("case", bq.FILTFILT_CASES, ids=bq.case_id)
def test_filtfilt_model_is_the_composition_of_the_bank_model(oracle, case):
    """the composed model of the forward-backward cases, built here from the bank model call by call with the state buffers a user of
    the library would write (test_gpu_filtfilt._composition), and close to the double reference of tests/filtfilt_ref.py"""
    from filtfilt_ref import PADTYPES, filtfilt_ref
    precision, kind, m, name, padtype, _ = case
    a, b, g = bq.coefficients(oracle.iir(m), kind, m, name)
    bb = b if kind == rx.GENERIC else None
    ss = steady_state_ref(kind, a, bb, g)
    x, P, got = bq.filtfilt_reference(case, a, b, g, ss)
    want = filtfilt_ref(x.astype(F64), kind, a, bb, g, PADTYPES[padtype], P)
    tol = {"f64": 1e-11, "mix": 1e-6, "f32": 1e-4}[precision]  # test_gpu_filtfilt.SCIPY_TOL (f64: a model in another operation order)
    assert np.abs(got - want).max() <= tol * np.abs(want).max()
    assert got.dtype == rx.SDT[precision] and got.shape == x.shape
