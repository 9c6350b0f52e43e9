"""Extended-precision checker of the transform kernels (a helper, not a test file).

Everything here is measured in units of u, the unit roundoff of the working precision (2^-24 for f32, 2^-53 for f64), against a DFT
in x87 extended precision (np.clongdouble, eps 1.08e-19: 2^11 times finer than double), and compared with the error of the SAME
operation done plainly at the SAME precision (`plain_fft`): a textbook radix-2 decimation-in-frequency transform, one rounding per
arithmetic operation, correctly rounded twiddles.  The rules:

  R1  on every row of the row set  e2 <= 3 max(E2_plain(row), 1 u)  and  einf <= 3 max(Einf_plain(row), 1 u)
  R2  N <= 1024: the identity as a batch of N rows, every element of the DFT matrix within 3 max(Einf_plain(batch), 4/3 u)
  R3  the impulse at 0, the all-ones row and the alternating row come out without any rounding: equality

The margin 3 is over the baseline, not a number of its own: a kernel differs from the plain form by fused multiply-adds and radix-4
butterflies (fewer roundings), by twiddles that are products of two or three rounded factors (about 1 to 3 u more, once per
element) on top of a plain total of 2 to 8 u -- at most about twice the plain error -- and the third unit is for the spread of
another rounding sequence on the same row.  It leaves no room for growth with N, a truncated series, a float constant in a double
path or a lost digit.
"""
import functools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not x87 extended precision here: this checker would silently be a double one"

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
CDT = {"f32": np.complex64, "f64": np.complex128}
RDT = {"f32": np.float32, "f64": np.float64}
MARGIN = 3.0
FLOOR_R1 = 1.0        # u
FLOOR_R2 = 4.0 / 3.0  # u: 3 x 4/3 = 4 u, one product by a correctly rounded twiddle can cost about 3 u
SHRINK_AT = 1 << 19   # from here on the row set is one Gaussian row, one tone and the impulses
BASE_N = 1 << 18      # ... and the baseline is the one of the same row at 2^18 times log2 N / 18

# the choice of the reference transform, made once at import: numpy's own FFT where it keeps extended precision, else the
# radix-2 transform below -- never a double one
NUMPY_FFT_IS_EXTENDED = np.fft.fft(np.ones(8, dtype=CLD)).dtype == CLD


def _pi():
    return 4 * np.arctan(LD(1))


@functools.lru_cache(maxsize=3)
def unit_roots(n):
    """W_n^j = exp(-2 pi i j / n), j < n, in longdouble.  Angles are reduced to the first octant in integers, so every sine and
    cosine is taken of an angle <= pi / 4 and the symmetries are exact."""
    if n == 1:
        return np.ones(1, dtype=CLD)
    if n == 2:
        return np.array([1, -1], dtype=CLD)
    j = np.arange(n, dtype=np.int64)
    quad, rem = np.divmod(4 * j, n)          # angle = quad * pi/2 + rem * 2 pi / (4 n)
    swap = rem * 2 > n                       # past pi / 4 within the quadrant: use the complement
    rem = np.where(swap, n - rem, rem)       # in units of 2 pi / (4 n)
    th = rem.astype(LD) * (_pi() / (2 * LD(n)))
    c, s = np.cos(th), np.sin(th)
    c, s = np.where(swap, s, c), np.where(swap, c, s)
    w = np.empty(n, dtype=CLD)               # exp(-i (quad pi/2 + th)) = (-i)^quad (c - i s)
    re = np.choose(quad, [c, -s, -c, s])
    im = np.choose(quad, [-s, -c, s, c])
    w.real, w.imag = re, im
    w.flags.writeable = False
    return w


def _radix2_ld(x):
    """own vectorised radix-2 decimation in frequency in longdouble (the fall-back reference)"""
    x = np.array(x, dtype=CLD)
    n = x.shape[-1]
    w = unit_roots(n)
    m = n
    while m >= 2:
        v = x.reshape(x.shape[:-1] + (n // m, m))
        a, b = v[..., : m // 2].copy(), v[..., m // 2:].copy()
        v[..., : m // 2] = a + b
        v[..., m // 2:] = (a - b) * w[:: n // m][: m // 2]
        m //= 2
    return x[..., bit_reverse(n)]


@functools.lru_cache(maxsize=8)
def bit_reverse(n):
    bits = n.bit_length() - 1
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return r


def ref_fft(x, reverse=False, force_own=False):
    """DFT of the rows of x (any working precision: converted exactly) in np.clongdouble.  forward_fft: X[k] = sum x[n] W^(nk);
    reverse_fft: the conjugate kernel and 1 / N (include/sdsp_hip.h)."""
    xl = np.asarray(x).astype(CLD)
    y = np.fft.fft(xl, axis=-1) if NUMPY_FFT_IS_EXTENDED and not force_own else _radix2_ld(xl)
    assert y.dtype == CLD
    if reverse:  # sum x[n] W^(-nk) = X[-k]; the division by a power of two is exact
        y = np.roll(y[..., ::-1], 1, axis=-1) / LD(xl.shape[-1])
    return y


@functools.lru_cache(maxsize=3)
def _unit_roots_split(n):
    return split(unit_roots(n))


def impulse_ref_split(n, p, reverse=False):
    """impulse_ref as a split() pair, gathered from the split table: conjugation and 1 / N are exact on either part"""
    hi, lo = _unit_roots_split(n)
    idx = (int(p) * np.arange(n, dtype=np.int64)) % n
    hi, lo = hi[idx], lo[idx]
    return (np.conj(hi) / n, np.conj(lo) / n) if reverse else (hi, lo)


def impulse_ref(n, p, reverse=False):
    """closed form: an impulse at p gives W_N^(p k mod N); the product is reduced in integers before the angle is formed"""
    w = unit_roots(n)[(int(p) * np.arange(n, dtype=np.int64)) % n]
    return np.conj(w) / LD(n) if reverse else w


def ones_ref(n, reverse=False):
    y = np.zeros(n, dtype=CLD)
    y[0] = 1 if reverse else n
    return y


def alt_ref(n, reverse=False):
    y = np.zeros(n, dtype=CLD)
    y[n // 2] = 1 if reverse else n
    return y


def pack_real(spec):
    """real-input packed layout: bins 0 .. N/2 - 1 with (X[0], X[N/2]) in the first"""
    half = spec.shape[-1] // 2
    out = spec[..., :half].copy()
    out[..., 0] = spec[..., 0].real + 1j * spec[..., half].real
    return out


def unpack_real(packed):
    """the full Hermitian spectrum of a packed one (any precision: no arithmetic but a sign)"""
    half = packed.shape[-1]
    full = np.empty(packed.shape[:-1] + (2 * half,), dtype=packed.dtype)
    full[..., :half] = packed
    full[..., 0] = packed[..., 0].real
    full[..., half] = packed[..., 0].imag
    full[..., half + 1:] = np.conj(packed[..., 1:][..., ::-1])
    return full


def conv_ref(x, h):
    """circular convolution by the frequency response h: ifft(fft(x) h), in longdouble"""
    return ref_fft(ref_fft(x) * np.asarray(h).astype(CLD), reverse=True)


# ------------------------------------------------------------------------------------------------------------ the baseline
def rounded_twiddles(n, m, prec, reverse):
    """W_m^j, j < m / 2: the longdouble values rounded once to the working precision"""
    w = unit_roots(m)[: m // 2]
    return (np.conj(w) if reverse else w).astype(CDT[prec])


def plain_fft(x, prec, reverse=False, twiddle=rounded_twiddles):
    """Textbook radix-2 decimation in frequency at the working precision: real and imaginary parts are separate arrays of the
    working type, every operation is one numpy call, so each is rounded once and nothing is fused.  twiddle(n, m, prec, reverse)
    gives the stage's W_m^j, j < m / 2 (the planted defects of tests/test_fft_exact_host.py plug in here)."""
    rdt = RDT[prec]
    x = np.asarray(x).astype(CDT[prec])
    n = x.shape[-1]
    re, im = np.ascontiguousarray(x.real, dtype=rdt), np.ascontiguousarray(x.imag, dtype=rdt)
    m = n
    while m >= 2:
        w = twiddle(n, m, prec, reverse)
        wr, wi = np.ascontiguousarray(w.real, dtype=rdt), np.ascontiguousarray(w.imag, dtype=rdt)
        vr, vi = re.reshape(re.shape[:-1] + (n // m, m)), im.reshape(im.shape[:-1] + (n // m, m))
        ar, ai, br, bi = vr[..., : m // 2], vi[..., : m // 2], vr[..., m // 2:], vi[..., m // 2:]
        dr, di = ar - br, ai - bi
        ar += br
        ai += bi
        br[...] = dr * wr - di * wi
        bi[...] = dr * wi + di * wr
        m //= 2
    out = np.empty(x.shape, dtype=CDT[prec])
    rev = bit_reverse(n)
    out.real, out.imag = re[..., rev], im[..., rev]
    if reverse:
        out *= rdt(1.0 / n)  # a power of two: exact
    return out


def plain_conv(x, h, prec):
    """the plain composition fft -> multiply -> ifft at the working precision"""
    rdt = RDT[prec]
    s = plain_fft(x, prec)
    h = np.asarray(h).astype(CDT[prec])
    sr, si, hr, hi = s.real.astype(rdt), s.imag.astype(rdt), h.real.astype(rdt), h.imag.astype(rdt)
    p = np.empty(s.shape, dtype=CDT[prec])
    p.real, p.imag = sr * hr - si * hi, sr * hi + si * hr
    return plain_fft(p, prec, reverse=True)


# ------------------------------------------------------------------------------------------------------------ the metrics
def split(ref):
    """a longdouble array as (hi, lo) doubles, hi + lo = ref to 2^-106: errors() then works in double without losing anything --
    got - hi is exact (the two agree to a few u) and lo is subtracted from a difference that small"""
    dt = np.complex128 if np.iscomplexobj(ref) else np.float64
    hi = ref.astype(dt)
    return hi, (ref - hi).astype(dt)


def errors(got, ref, prec):
    """(e2, einf) of one row in units of u: ||got - ref||_2 / ||ref||_2 and max |got - ref| / max |ref|.  ref: a longdouble array, or
    its split() (large rows: x87 arithmetic on 2^22 points takes a second a pass)"""
    if isinstance(ref, tuple):
        hi, lo = ref
        d = np.abs((np.asarray(got).astype(hi.dtype) - hi) - lo)
        a = np.abs(hi)
    else:
        d = np.abs(np.asarray(got).astype(ref.dtype) - ref)
        a = np.abs(ref)
    e2 = np.sqrt((d * d).sum()) / np.sqrt((a * a).sum())
    return float(e2 / U[prec]), float(d.max() / a.max() / U[prec])


# ------------------------------------------------------------------------------------------------------------ the row set
def _split(n):
    return 1 << -(-(n.bit_length() - 1) // 2)  # N2 = 2^ceil(log2 N / 2)


def _tone(n, q, prec):
    return np.conj(unit_roots(n))[(int(q) * np.arange(n, dtype=np.int64)) % n].astype(CDT[prec])  # exp(+2 pi i q n / N), rounded


def _one_hot(n, p, prec):
    x = np.zeros(n, dtype=CDT[prec])
    x[p] = 1
    return x


class Rows:
    """the rows of one size: x (rows, n) at the working precision, a label and a kind per row"""

    def __init__(self, n, prec, labels, kinds, x, impulse_at):
        self.n, self.prec, self.labels, self.kinds, self.x, self.impulse_at = n, prec, labels, kinds, x, impulse_at

    def __len__(self):
        return len(self.labels)


def row_set(n, prec, full=None):
    """One generator seeded from (N, precision) alone.  Two complex Gaussian rows; impulses at 0, 1, N/2 - 1, N/2 + 1, N - 1, a
    seeded odd position and (N >= 2^16) both sides of the split N2 = 2^ceil(log2 N / 2); tones exp(+2 pi i q n / N) rounded to the
    working precision at q = 1, N/2 - 1 and a seeded odd one; the all-ones row; the alternating row.  From 2^19 on (full=False):
    one Gaussian row, the tone at the seeded odd bin and the impulses."""
    assert n >= 4 and n & (n - 1) == 0
    full = n < SHRINK_AT if full is None else full
    rng = np.random.default_rng([n, 32 if prec == "f32" else 64])
    g = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))).astype(CDT[prec])
    p_odd = int(rng.integers(0, n // 2)) * 2 + 1
    q_odd = int(rng.integers(0, n // 2)) * 2 + 1
    rows = [("gauss0", "gauss", g[0], None)]
    if full:
        rows.append(("gauss1", "gauss", g[1], None))
    imp = [("0", 0), ("1", 1), ("N/2-1", n // 2 - 1), ("N/2+1", n // 2 + 1), ("N-1", n - 1)]
    if n >= 1 << 16:
        imp += [("N2-1", _split(n) - 1), ("N2+1", _split(n) + 1)]
    imp.append(("odd", p_odd))
    rows += [(f"impulse@{name}", "impulse", _one_hot(n, p, prec), p) for name, p in imp]
    tones = [("1", 1), ("N/2-1", n // 2 - 1), ("odd", q_odd)] if full else [("odd", q_odd)]
    rows += [(f"tone@{name}", "tone", _tone(n, q, prec), None) for name, q in tones]
    if full:
        alt = np.ones(n, dtype=CDT[prec])
        alt[1::2] = -1
        rows += [("ones", "ones", np.ones(n, dtype=CDT[prec]), None), ("alt", "alt", alt, None)]
    return Rows(n, prec, [r[0] for r in rows], [r[1] for r in rows], np.stack([r[2] for r in rows]), [r[3] for r in rows])


EXACT_ROWS = ("impulse@0", "ones", "alt")  # R3


def exact_output(rows, i, reverse):
    """what R3 demands of row i, at the working precision, or None"""
    n, label = rows.n, rows.labels[i]
    if label not in EXACT_ROWS:
        return None
    ref = {"impulse@0": impulse_ref(n, 0, reverse), "ones": ones_ref(n, reverse), "alt": alt_ref(n, reverse)}[label]
    return ref.astype(CDT[rows.prec])  # 1, N, 1 / N: exact in either precision


class Case:
    """rows of one (n, precision, direction) with their longdouble references and baseline errors, computed once"""

    def __init__(self, n, prec, reverse, full=None):
        self.rows = rows = row_set(n, prec, full)
        self.n, self.prec, self.reverse = n, prec, reverse
        self._ref = {}
        dense = [i for i, k in enumerate(rows.kinds) if k in ("gauss", "tone")]
        if dense:  # one longdouble transform serves both directions: sum x[n] W^(-nk) = X[-k], and 1 / N is exact
            if (n, prec) not in _FORWARD:
                for k in [k for k in _FORWARD if k[0] >= SHRINK_AT and k[0] != n]:
                    del _FORWARD[k]
                _FORWARD[(n, prec)] = split(ref_fft(rows.x[dense]))
            hi, lo = _FORWARD[(n, prec)]
            if reverse:
                hi, lo = (np.roll(v[..., ::-1], 1, axis=-1) / n for v in (hi, lo))
            self._ref = {i: (hi[j], lo[j]) for j, i in enumerate(dense)}
        full = len(rows) > 0 and "ones" in rows.labels
        if n >= SHRINK_AT and not full:  # the law is at most linear in log2 N: the same rows at 2^18, times log2 N / 18
            small = get_case(BASE_N, prec, reverse)
            idx = [small.rows.labels.index(lb) for lb in rows.labels]
            grow = (n.bit_length() - 1) / 18.0
            self.base = [(small.base[i][0] * grow, small.base[i][1] * grow) for i in idx]
        else:
            plain = plain_fft(rows.x, prec, reverse)
            self.base = [errors(plain[i], self.ref(i), prec) for i in range(len(rows))]

    def ref(self, i):
        """row i's reference as a split() pair"""
        if i in self._ref:
            return self._ref[i]
        n, kind = self.n, self.rows.kinds[i]
        if kind == "impulse":
            return impulse_ref_split(n, self.rows.impulse_at[i], self.reverse)  # not kept: 32 bytes a point
        return split(ones_ref(n, self.reverse) if kind == "ones" else alt_ref(n, self.reverse))


_CASES = {}
_FORWARD = {}  # (n, precision) -> split() forward references of the Gaussian and tone rows


def get_case(n, prec, reverse):
    key = (n, prec, bool(reverse))
    if key not in _CASES:
        if n >= SHRINK_AT:  # one large size at a time: a reference row of 2^22 points is 128 MiB
            for k in [k for k in _CASES if k[0] >= SHRINK_AT and k[0] != n]:
                del _CASES[k]
        _CASES[key] = Case(n, prec, reverse)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------ the rules
def bound(base, floor=FLOOR_R1, margin=MARGIN):
    return margin * max(base, floor)


def check_rows(got, refs, base, labels, kinds, prec, exact=None, margin=MARGIN, exact_margin_u=None, inphase_u=None):
    """R1 (and R3 where exact[i] is not None) on rows.  got: (rows, n) at the working precision; refs: callable i -> longdouble row;
    base: per row (E2_plain, Einf_plain) in u.  exact_margin_u: for a kernel that legitimately rounds on the R3 rows (the step is
    named where this is passed), the bound in u on every element, relative to the row's peak, that replaces equality.  inphase_u:
    {row kind: u} added to the einf bound of rows of that kind (the counted term of inphase_transform / inphase_impulse_forward,
    for a kernel whose exception names the count).  Returns (failures, report): failures are (rule, kind,
    label, text), the report has a line of figures per row."""
    failures, report = [], []
    for i, label in enumerate(labels):
        e2, einf = errors(got[i], refs(i), prec)
        b2, binf = bound(base[i][0], margin=margin), bound(base[i][1], margin=margin) + (inphase_u or {}).get(kinds[i], 0.0)
        report.append(dict(label=label, kind=kinds[i], e2=e2, einf=einf, base2=base[i][0], baseinf=base[i][1], bound2=b2, boundinf=binf))
        if not e2 <= b2:
            failures.append(("R1", kinds[i], label, f"e2 {e2:.2f} u > {b2:.2f} u = {margin:g} max({base[i][0]:.2f}, 1)"))
        if not einf <= binf:
            failures.append(("R1", kinds[i], label, f"einf {einf:.2f} u > {binf:.2f} u = {margin:g} max({base[i][1]:.2f}, 1)"
                             + (f" + {inphase_u[kinds[i]]:.2f}" if inphase_u and kinds[i] in inphase_u else "")))
        want = exact[i] if exact is not None else None
        if want is not None:
            if exact_margin_u is None:
                if not np.array_equal(got[i], want):  # -0 == +0
                    failures.append(("R3", kinds[i], label, f"not exact: einf {einf:.3g} u, {int((got[i] != want).sum())} points differ"))
            elif not einf <= exact_margin_u:  # R3 speaks of every element: so does its relaxation (R1 still holds e2 on the row)
                failures.append(("R3", kinds[i], label, f"einf {einf:.2f} u > {exact_margin_u:g} u"))
    return failures, report


def check_case(case, got, margin=MARGIN, exact_margin_u=None, inphase_u=None):
    rows = case.rows
    exact = [exact_output(rows, i, case.reverse) for i in range(len(rows))]
    return check_rows(got, case.ref, case.base, rows.labels, rows.kinds, case.prec, exact, margin, exact_margin_u, inphase_u)


# ---- R4: the counted term of an output that is an in-phase sum of N terms (a tone's peak, the impulse a convolution gives back).
# Random rounding errors average out over such a sum; a unit factor that is the SAME for every term does not: its modulus error
# |w| - 1 goes into the peak in full.  The kernels multiply by a compile-time constant W_32^e (W_16^e) and by a table value in
# every stage, where the plain transform multiplies by one table value.
def const_modulus_error(prec):
    """the largest | |w| - 1 | in u over the compile-time constants W_32^e rounded to the precision (csrc/fft32.h, fft_passes.h):
    0.48 u in f32 -- where every one of them lies below 1 --, 0.62 u in f64"""
    w = unit_roots(32).astype(CDT[prec]).astype(CLD)
    return float(np.abs(np.abs(w) - 1).max() / U[prec])


TABLE_MODULUS_ERROR = 2 ** 0.5 / 2  # u: components within u / 2 each, | |w| - 1 | <= (|c| + |s|) u / 2 <= u / sqrt 2


def constant_stages(register_passes):
    """stages that can carry a non-trivial constant: in a register pass of k stages the constants of the last two are 1 and -+i"""
    return sum(max(0, k - 2) for k in register_passes)


def inphase_transform(register_passes, prec):
    """a transform's sum into ONE bin: the constants on that bin's path are fixed, at most one per stage that carries one; the table
    values depend on the term's position and average out"""
    return constant_stages(register_passes) * const_modulus_error(prec)


def inphase_impulse_forward(register_passes, prec):
    """the forward transform of an impulse, summed over all bins afterwards: at its one position constant AND table value of every
    stage are fixed, and a bin meets a stage's factor where it lies on the twiddled side: half the bins"""
    stages = sum(register_passes)
    return 0.5 * (constant_stages(register_passes) * const_modulus_error(prec) + stages * TABLE_MODULUS_ERROR)


@functools.lru_cache(maxsize=8)
def matrix_base(n, prec, reverse):
    """Einf_plain of the identity batch in u: the worst element of the plain transform's DFT matrix"""
    plain = plain_fft(np.eye(n, dtype=CDT[prec]), prec, reverse)
    return matrix_error(plain, n, prec, reverse)[0]


def dft_matrix(n, reverse):
    w = unit_roots(n)[np.outer(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)) % n]
    return np.conj(w) / LD(n) if reverse else w


def matrix_error(got, n, prec, reverse):
    """(worst elementwise error in u, its (row, column)) of got = transform(identity) against the exact matrix; every |entry| is 1
    (1 / N in reverse), so this is an elementwise relative error"""
    d = np.abs(np.asarray(got).astype(CLD) - dft_matrix(n, reverse)) * (LD(n) if reverse else LD(1))
    at = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d.max() / U[prec]), tuple(int(v) for v in at)


def check_matrix(got, n, prec, reverse, margin=MARGIN):
    """R2.  Returns (failures, figures)."""
    base = matrix_base(n, prec, reverse)
    err, at = matrix_error(got, n, prec, reverse)
    b = bound(base, FLOOR_R2, margin)
    fails = [] if err <= b else [("R2", "matrix", f"impulse@{at[0]}", f"element {at} off by {err:.2f} u > {b:.2f} u = {margin:g} max({base:.2f}, 4/3)")]
    return fails, dict(label="matrix", kind="matrix", einf=err, baseinf=base, boundinf=b)


def run_rules(fn, n, prec, reverse, margin=MARGIN):
    """every rule on a transform given as a function of a (rows, n) array at the working precision"""
    case = get_case(n, prec, reverse)
    fails, report = check_case(case, fn(case.rows.x.copy()), margin)
    if n <= 1024:
        f2, r2 = check_matrix(fn(np.eye(n, dtype=CDT[prec])), n, prec, reverse, margin)
        fails, report = fails + f2, report + [r2]
    return fails, report


# ------------------------------------------------------------------------------------------------------------ real-input rows
def real_row_set(n, prec):
    """n real samples: two Gaussian rows, impulses at 0, 1, n/2 and n - 1, cosines at bins 1 and n/2 - 1 (rounded), the constant and
    the alternating row"""
    rng = np.random.default_rng([n, 32 if prec == "f32" else 64, 1])
    rdt = RDT[prec]
    g = rng.standard_normal((2, n)).astype(rdt)
    rows = [("gauss0", "gauss", g[0]), ("gauss1", "gauss", g[1])]
    for name, p in (("0", 0), ("1", 1), ("n/2", n // 2), ("n-1", n - 1)):
        rows.append((f"impulse@{name}", "impulse", _one_hot(n, p, prec).real.astype(rdt)))
    for name, q in (("1", 1), ("n/2-1", n // 2 - 1)):
        rows.append((f"cos@{name}", "tone", unit_roots(n)[(q * np.arange(n, dtype=np.int64)) % n].real.astype(rdt)))
    alt = np.ones(n, dtype=rdt)
    alt[1::2] = -1
    rows += [("ones", "ones", np.ones(n, dtype=rdt)), ("alt", "alt", alt)]
    return [r[0] for r in rows], [r[1] for r in rows], np.stack([r[2] for r in rows])


class RealCase:
    """Forward: real rows -> packed spectrum.  Reverse: the packed spectrum of each row, rounded to the working precision, back to
    real samples; the reference inverts the ROUNDED spectrum.  Baselines: plain_fft of the row as a complex one."""

    def __init__(self, n, prec, reverse):
        self.n, self.prec, self.reverse = n, prec, reverse
        self.labels, self.kinds, x = real_row_set(n, prec)
        spec = pack_real(ref_fft(x))
        if not reverse:
            self.x, self.refs = x, spec
            plain = pack_real(plain_fft(x, prec))
            self.exact = [spec[i].astype(CDT[prec]) if lb in EXACT_ROWS else None for i, lb in enumerate(self.labels)]
        else:
            self.x = spec.astype(CDT[prec])  # what the plan is given (as reals: re, im interleaved)
            full = unpack_real(self.x)
            self.refs = ref_fft(full, reverse=True).real
            plain = plain_fft(full, prec, reverse=True).real
            self.exact = [x[i] if lb in EXACT_ROWS else None for i, lb in enumerate(self.labels)]
        self.base = [errors(plain[i], self.refs[i], prec) for i in range(len(self.labels))]

    def check(self, got, margin=MARGIN, exact_margin_u=None):
        return check_rows(got, lambda i: self.refs[i], self.base, self.labels, self.kinds, self.prec, self.exact, margin, exact_margin_u)


_REAL = {}


def get_real_case(n, prec, reverse):
    key = (n, prec, bool(reverse))
    if key not in _REAL:
        _REAL[key] = RealCase(n, prec, reverse)
    return _REAL[key]


# ------------------------------------------------------------------------------------------------------------ convolution
class ConvCase:
    """x: the row set of the size; h: random, the rounded transform of an impulse delayed by a seeded d (a circular shift), all ones
    (the identity).  Reference: conv_ref on the rounded h; baseline: plain_conv."""

    H_KINDS = ("random", "shift", "ones")

    def __init__(self, n, prec):
        self.n, self.prec = n, prec
        self.rows = rows = row_set(n, prec, full=True)
        rng = np.random.default_rng([n, 32 if prec == "f32" else 64, 2])
        d = int(rng.integers(1, n))
        self.h = {"random": (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(CDT[prec]),
                  "shift": unit_roots(n)[(d * np.arange(n, dtype=np.int64)) % n].astype(CDT[prec]),
                  "ones": np.ones(n, dtype=CDT[prec])}
        self.refs = {k: conv_ref(rows.x, h) for k, h in self.h.items()}
        self.base = {}
        for k, h in self.h.items():
            plain = plain_conv(rows.x, h, prec)
            self.base[k] = [errors(plain[i], self.refs[k][i], prec) for i in range(len(rows))]

    def check(self, kind, got, margin=MARGIN, inphase_u=None):
        rows = self.rows
        return check_rows(got, lambda i: self.refs[kind][i], self.base[kind], rows.labels, rows.kinds, self.prec, None, margin, None, inphase_u)


_CONV = {}


def get_conv_case(n, prec):
    if (n, prec) not in _CONV:
        _CONV[(n, prec)] = ConvCase(n, prec)
    return _CONV[(n, prec)]


def worst_by_kind(report):
    """per row kind: the worst e2, einf and ratios to the baseline's bound -- what the accuracy table prints"""
    out = {}
    for r in report:
        k = out.setdefault(r["kind"], dict(e2=0.0, einf=0.0, base2=0.0, baseinf=0.0, bound2=0.0, boundinf=0.0, ratio=0.0))
        for f in ("e2", "einf", "base2", "baseinf", "bound2", "boundinf"):
            k[f] = max(k[f], r.get(f, 0.0))
        ratio = max(r.get("e2", 0.0) / max(r.get("base2", 0.0), FLOOR_R1), r["einf"] / max(r["baseinf"], FLOOR_R1))
        k["ratio"] = max(k["ratio"], ratio)
    return out
