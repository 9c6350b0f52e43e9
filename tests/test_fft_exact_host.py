"""The extended-precision checker's own proof (tests/fft_exact.py; no GPU): the longdouble reference against a 50-digit DFT, the
closed forms against the reference, the row set against its seed, the baseline against the pinned oracle, and four planted defects
that the suite's earlier bounds (4 N eps for f64, 1e-6 for f32, Gaussian rows under a max-norm) let through and the rules R1 .. R3
must catch -- each through a numpy stand-in for a kernel: fft_exact.plain_fft with another twiddle function."""
import numpy as np
import pytest

import fft_exact as fx
from conftest import rel_max_err

EPS_LD = float(np.finfo(np.longdouble).eps)
EPS64 = np.finfo(np.float64).eps


def _ld_bound(n):
    """A radix-2 transform in longdouble rounds each point once per addition and about three times per twiddle product in each of
    its log2 N stages, and its twiddles carry a rounding of their own: below 4 eps per stage relative to the largest |X| -- stated
    from the format's eps, not from a run."""
    return 4 * (n.bit_length() - 1) * EPS_LD


def _max_rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("n", [8, 64])
def test_reference_agrees_with_a_50_digit_dft(n):
    import mpmath
    mpmath.mp.dps = 50
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)  # doubles: exact in mpmath and in longdouble
    xs = [mpmath.mpc(float(v.real), float(v.imag)) for v in x]

    def to_ld(v):  # an mpf as the sum of two doubles: 106 bits, more than the 64 of the target
        hi = float(v)
        return np.longdouble(hi) + np.longdouble(float(v - hi))

    for reverse in (False, True):
        sign = 1 if reverse else -1
        want = np.empty(n, dtype=np.clongdouble)
        for k in range(n):
            s = mpmath.fsum(xs[j] * mpmath.expjpi(mpmath.mpf(sign * 2 * ((j * k) % n)) / n) for j in range(n))
            s = s / n if reverse else s
            want[k] = to_ld(s.real) + 1j * to_ld(s.imag)
        for own in (False, True):  # numpy's transform on clongdouble and the own radix-2: both are held, whichever is in use
            got = fx.ref_fft(x, reverse, force_own=own)
            assert got.dtype == np.clongdouble
            err = _max_rel(got, want)
            print(f"N = {n} reverse={reverse} own={own}: {err / EPS_LD:.2f} longdouble eps (bound {_ld_bound(n) / EPS_LD:.0f})")
            assert err <= _ld_bound(n), (n, reverse, own, err)
        # the unit roots themselves: within one longdouble rounding of the 50-digit values
        w = fx.unit_roots(n)
        for j in range(n):
            e = mpmath.expjpi(mpmath.mpf(-2 * j) / n)
            assert abs(w[j] - (to_ld(e.real) + 1j * to_ld(e.imag))) <= 1.5 * EPS_LD, (n, j)


def test_the_reference_is_extended_precision_by_assertion():
    assert np.finfo(np.longdouble).eps < 2e-19
    assert fx.ref_fft(np.ones(16, np.complex64)).dtype == np.clongdouble
    if fx.NUMPY_FFT_IS_EXTENDED:
        assert np.fft.fft(np.ones(16, np.clongdouble)).dtype == np.clongdouble
    # a double-precision transform is 2^11 eps away on a Gaussian row: the check above would see it
    x = fx.row_set(4096, "f64").x[0]
    assert _max_rel(np.fft.fft(x).astype(np.clongdouble), fx.ref_fft(x)) > 100 * EPS_LD


def test_closed_forms_agree_with_the_reference():
    n = 1 << 16
    bound = _ld_bound(n)
    for prec in ("f32", "f64"):
        rows = fx.row_set(n, prec)
        for reverse in (False, True):
            ref = fx.ref_fft(rows.x, reverse)
            scale = n if reverse else 1
            for i, kind in enumerate(rows.kinds):
                if kind == "impulse":
                    closed = fx.impulse_ref(n, rows.impulse_at[i], reverse)
                elif kind == "ones":
                    closed = fx.ones_ref(n, reverse)
                elif kind == "alt":
                    closed = fx.alt_ref(n, reverse)
                else:
                    continue
                # elementwise for the impulses (|X| = 1), against the peak for the two lines
                assert float(np.abs(ref[i] - closed).max() / np.abs(closed).max()) <= bound, (prec, reverse, rows.labels[i])
                assert np.abs(closed).max() * scale == (n if kind in ("ones", "alt") else 1)
    # the packed real layout and the convolution reference
    x = np.random.default_rng(1).standard_normal((2, 256))
    spec = fx.ref_fft(x)
    packed = fx.pack_real(spec)
    want = np.fft.rfft(x, axis=-1)
    assert packed.shape == (2, 128) and np.abs(packed[:, 1:] - want[:, 1:128]).max() < 1e-12
    assert np.abs(packed[:, 0] - (want[:, 0].real + 1j * want[:, 128].real)).max() < 1e-12
    assert _max_rel(fx.unpack_real(packed), spec) <= _ld_bound(256)
    z = fx.row_set(256, "f64").x[:2]
    shift = fx.unit_roots(256)[(5 * np.arange(256)) % 256]  # the exact transform of an impulse delayed by 5
    assert _max_rel(fx.ref_fft(fx.ref_fft(z) * shift, reverse=True), np.roll(z, 5, axis=-1).astype(np.clongdouble)) <= 2 * _ld_bound(256)
    assert _max_rel(fx.conv_ref(z, np.ones(256)), z.astype(np.clongdouble)) <= 2 * _ld_bound(256)


def test_the_row_set_depends_only_on_its_seed():
    for prec in ("f32", "f64"):
        a, b = fx.row_set(1 << 16, prec), fx.row_set(1 << 16, prec)
        assert a.labels == b.labels and np.array_equal(a.x, b.x) and a.x.dtype == fx.CDT[prec]
        assert a.labels == ["gauss0", "gauss1", "impulse@0", "impulse@1", "impulse@N/2-1", "impulse@N/2+1", "impulse@N-1", "impulse@N2-1",
                            "impulse@N2+1", "impulse@odd", "tone@1", "tone@N/2-1", "tone@odd", "ones", "alt"]
        assert a.impulse_at[2:9] == [0, 1, 32767, 32769, 65535, 255, 257] and a.impulse_at[9] % 2 == 1
        small = fx.row_set(1024, prec)
        assert "impulse@N2-1" not in small.labels and len(small) == 13
        assert not np.array_equal(small.x[0], fx.row_set(2048, prec).x[0, :1024])
        big = fx.row_set(1 << 19, prec)
        assert big.labels == ["gauss0"] + a.labels[2:10] + ["tone@odd"] and big.impulse_at[6:8] == [1023, 1025]
        # tones are the longdouble values rounded once; the reference transforms the rounded row
        t = a.x[a.labels.index("tone@1")]
        assert np.array_equal(t, np.conj(fx.unit_roots(1 << 16)).astype(fx.CDT[prec]))
    assert not np.array_equal(fx.row_set(1024, "f32").x[0], fx.row_set(1024, "f64").x[0].astype(np.complex64))


# ---------------------------------------------------------------------------------------------------------------- the baseline
def test_the_baseline_is_tied_to_the_pinned_oracle(oracle):
    """plain_fft in f64 lies within a factor 2 of oracle.fft's error (the reference's own radix-2 algorithm in double) on the Gaussian
    rows, in both metrics: the baseline is "the same operation done plainly", not a transform of another quality."""
    for n in (1024, 4096, 1 << 16):
        for reverse in (False, True):
            case = fx.get_case(n, "f64", reverse)
            for i, kind in enumerate(case.rows.kinds):
                if kind != "gauss":
                    continue
                got = oracle.fft(case.rows.x[i:i + 1].copy(), 2, reverse)[0]
                o2, oinf = fx.errors(got, case.ref(i), "f64")
                p2, pinf = case.base[i]
                print(f"N = {n} reverse={reverse} {case.rows.labels[i]}: plain {p2:.2f} / {pinf:.2f} u, oracle {o2:.2f} / {oinf:.2f} u, "
                      f"factor {p2 / o2:.2f} / {pinf / oinf:.2f}")
                assert 0.5 <= p2 / o2 <= 2.0 and 0.5 <= pinf / oinf <= 2.0, (n, reverse, p2, o2, pinf, oinf)


def test_the_baseline_is_exact_where_r3_asks_for_it():
    for prec in ("f32", "f64"):
        for n in (16, 1024, 1 << 16):
            for reverse in (False, True):
                fails, _ = fx.run_rules(lambda x: fx.plain_fft(x, prec, reverse), n, prec, reverse)
                assert fails == []


# ---------------------------------------------------------------------------------------------------------------- planted defects
def _old_bound_on_gaussian_rows(fn, n, prec):
    """the suite's present check: Gaussian rows, max-norm, 4 N eps (f64) / 1e-6 (f32) against a double-precision reference"""
    case = fx.get_case(n, prec, False)
    g = [i for i, k in enumerate(case.rows.kinds) if k == "gauss"]
    ref = np.stack([case.ref(i)[0] for i in g])  # the reference rounded to double
    return rel_max_err(fn(case.rows.x[g]), ref), (4 * n * EPS64 if prec == "f64" else 1e-6)


def _series_twiddles(n, m, prec, reverse):
    """(a) the leading stage's W_N^j (the N / 2 distinct twiddles: what an inter-pass twiddle is) as W_1024^(j >> FB), correctly
    rounded, times the TWO-term series that csrc/fft_2pass.hip's twiddle_n uses for f32 -- in a double transform"""
    if m != n:
        return fx.rounded_twiddles(n, m, prec, reverse)
    fb = (n.bit_length() - 1) - 10
    j = np.arange(n // 2)
    half = fx.rounded_twiddles(n, 1024, prec, reverse)
    coarse = np.concatenate([half, -half])
    th = (j & ((1 << fb) - 1)).astype(np.float64) * (6.283185307179586476925 / float(n))
    sn = th - th * (th * th) * 0.16666667
    fine = (1.0 - 0.5 * th * th) + 1j * (sn if reverse else -sn)
    return (coarse[j >> fb] * fine).astype(fx.CDT[prec])


def _one_entry_off(index):
    """(b), (d): entry `index` of the leading stage's table times (1 + 2^-40)"""
    def tw(n, m, prec, reverse):
        w = fx.rounded_twiddles(n, m, prec, reverse).copy()
        if m == n:
            w[index] *= 1 + 2.0 ** -40
        return w
    return tw


def _recurrence_table(restart):
    """(c) W_N^j = W_N^(j-1) W_N^1 in float arithmetic, restarted from the correctly rounded value every `restart` entries; every
    stage reads the one table with its stride"""
    tables = {}

    def tw(n, m, prec, reverse):
        if n not in tables:
            exact = fx.rounded_twiddles(n, n, prec, reverse)
            re, im = exact.real.copy(), exact.imag.copy()
            w1r, w1i = re[1], im[1]
            for j in range(len(exact)):
                if j % restart:
                    pr, pi = re[j - 1], im[j - 1]
                    re[j], im[j] = pr * w1r - pi * w1i, pr * w1i + pi * w1r  # np.float32 scalars: one rounding per operation
            tables[n] = (re + 1j * im).astype(fx.CDT[prec])
        return tables[n][:: n // m][: m // 2]
    return tw


DEFECTS = {
    # name: (n, precision, twiddle function, (rule, row kinds) of which at least one must be among the failures)
    "a: two-term series in double": (1 << 16, "f64", _series_twiddles, ("R1", ("gauss", "impulse", "tone"))),
    "b: one entry x (1 + 2^-40)": (1024, "f64", _one_entry_off(341), ("R2", ("matrix",))),
    # R = 16 separates here: the earlier bound passes (5.1e-7) and the rules fail; R = 32 already misses 1e-6 (1.4e-6) with this
    # recurrence (a table of N / 2 entries shared by all stages), R = 8 passes 1e-6 too and fails R1 on two rows only
    "c: float recurrence, restart 16": (4096, "f32", _recurrence_table(16), ("R1", ("gauss", "impulse"))),
    # the entry just past the split N2 = 256: x[N2 + 1] meets it in the leading stage, x[N2 - 1] does not
    "d: 2^-40 on the odd side of the split": (1 << 16, "f64", _one_entry_off(257), ("R1", ("impulse", "tone"))),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_defects_pass_the_old_bound_and_fail_the_new_rules(name):
    n, prec, tw, (rule, kinds) = DEFECTS[name]
    fn = lambda x: fx.plain_fft(x, prec, False, tw)  # noqa: E731
    err, tol = _old_bound_on_gaussian_rows(fn, n, prec)
    assert err < tol, (name, "the earlier bound already catches this", err, tol)
    fails, report = fx.run_rules(fn, n, prec, False)
    print(f"{name}: earlier check {err:.3g} < {tol:.3g}; {len(fails)} failures under the rules")
    for f in fails:
        print("   ", *f)
    caught = [f for f in fails if f[0] == rule and f[1] in kinds]
    assert caught, (name, "not caught under", rule, kinds, fails)
    if name.startswith("d"):  # the side of the split: the impulse past it sees the fault, the one before it is clean
        labels = {f[2] for f in fails}
        assert "impulse@N2+1" in labels and "impulse@N2-1" not in labels and "impulse@1" not in labels
    if name.startswith("b"):  # R2 names the row and the element
        assert caught[0][2] == "impulse@341" and "element (341," in caught[0][3]


@pytest.mark.parametrize("n", [1024, 4096, 1 << 16])
def test_clean_transforms_pass_the_rules(n):
    import scipy.fft
    stand_ins = {
        ("plain", "f64"): lambda x, rev: fx.plain_fft(x, "f64", rev),
        ("plain", "f32"): lambda x, rev: fx.plain_fft(x, "f32", rev),
        ("np.fft.fft", "f64"): lambda x, rev: np.fft.ifft(x, axis=-1) if rev else np.fft.fft(x, axis=-1),
        ("scipy.fft.fft(complex64)", "f32"): lambda x, rev: (scipy.fft.ifft if rev else scipy.fft.fft)(x.astype(np.complex64), axis=-1),
    }
    for (name, prec), fn in stand_ins.items():
        for reverse in (False, True):
            fails, report = fx.run_rules(lambda x: fn(x, reverse), n, prec, reverse)
            worst = fx.worst_by_kind(report)
            print(f"{name} {prec} N = {n} reverse={reverse}: worst ratio to the baseline " +
                  ", ".join(f"{k} {v['ratio']:.2f}" for k, v in worst.items()))
            assert fails == [], (name, prec, n, reverse, fails)
            assert fn(np.ones((1, n), fx.CDT[prec]), reverse).dtype == fx.CDT[prec]


# ---------------------------------------------------------------------------------------------------------------- the in-phase count
def _two_factor_fft(x, prec, passes):
    """numpy model of the kernels' twiddle scheme: a radix-2 DIF whose stage factor W_m^j is applied as a compile-time constant
    W_m^(S (j // S)) times a table value W_m^(j mod S), two rounded products, S = the register stride of the stage's pass; both
    factors correctly rounded, nothing fused"""
    rdt = fx.RDT[prec]
    x = np.asarray(x).astype(fx.CDT[prec])
    n = x.shape[-1]
    strides = []
    left = n
    for k in passes:
        left >>= k
        strides += [left] * k
    re, im = np.ascontiguousarray(x.real, dtype=rdt), np.ascontiguousarray(x.imag, dtype=rdt)
    m = n
    for S in strides:
        j = np.arange(m // 2)
        factors = (fx.unit_roots(m)[(j // S) * S].astype(fx.CDT[prec]), fx.unit_roots(m)[j % S].astype(fx.CDT[prec]))
        vr, vi = re.reshape(re.shape[:-1] + (n // m, m)), im.reshape(im.shape[:-1] + (n // m, m))
        ar, ai, br, bi = vr[..., : m // 2], vi[..., : m // 2], vr[..., m // 2:], vi[..., m // 2:]
        dr, di = ar - br, ai - bi
        ar += br
        ai += bi
        for w in factors:
            wr, wi = w.real.astype(rdt), w.imag.astype(rdt)
            dr, di = dr * wr - di * wi, dr * wi + di * wr
        br[...], bi[...] = dr, di
        m //= 2
    out = np.empty(x.shape, dtype=fx.CDT[prec])
    rev = fx.bit_reverse(n)
    out.real, out.imag = re[..., rev], im[..., rev]
    return out


def test_the_in_phase_count_and_the_model_behind_it():
    """tests/test_gpu_fft_accuracy.py: INPHASE.  The constants' modulus errors are what the count says, in f32 every constant lies
    below 1, and the model of the two-factor scheme -- no kernel, no faulty constant -- is over the common bound on the impulse rows
    of a convolution by one step of the result and within the counted one."""
    w32 = fx.unit_roots(32).astype(np.complex64).astype(np.clongdouble)
    err = (np.abs(w32) - 1) / fx.U["f32"]
    assert (err <= 0).all() and (err[[1, 2, 3, 4]] < -0.1).all()  # W_32^8 k: exact
    assert abs(float(err[15] + err[14] + 2 * err[12]) * 2 + 3.08) < 0.01  # the path to bin N - 1 of the 2^16 two-pass transform
    assert 0.48 < fx.const_modulus_error("f32") < 0.49 and 0.61 < fx.const_modulus_error("f64") < 0.62
    assert fx.constant_stages([5, 3, 5, 3]) == 8 and fx.constant_stages([4, 4, 2]) == 4 and fx.constant_stages([5, 5, 4]) == 8
    n, prec, passes = 1024, "f64", [4, 4, 2]  # csrc/fft_reg64.hip at N = 1024
    case = fx.get_conv_case(n, prec)
    spec = _two_factor_fft(case.rows.x, prec, passes)  # h = ones
    back = (np.conj(_two_factor_fft(np.conj(spec), prec, passes)) / n).astype(fx.CDT[prec])
    fails, _ = case.check("ones", back)
    assert {f[2] for f in fails} == {"impulse@N/2-1", "impulse@N-1"} and all("einf 4.00 u" in f[3] for f in fails), fails
    counted = fx.inphase_transform(passes, prec) + fx.inphase_impulse_forward(passes, prec)
    assert 7.2 < counted < 7.3
    assert case.check("ones", back, inphase_u={"impulse": counted})[0] == []
