"""Bit-level and extended-precision checker of the time-domain kernels: the cascaded-biquad banks (csrc/iir_step.h, csrc/iir.hip,
csrc/iir_filtfilt.hip) and the direct-form FIR bank (csrc/fir.hip).  A helper, not a test file; numpy only; DESIGN.md section 5.34.

The arithmetic of these kernels is fixed operation by operation in their headers, so two things can be said off the GPU:

  R1  bits      every output element and every element of the final state (all three ages of every level; the whole FIR history)
                has the bits of a plain model of the documented recurrence at the working precision, with correctly rounded
                fused multiply-adds (`biquad_model`, `fir_model_f32`, `fir_plain` in f64).  Compared as integers.  For FIR
                outputs -0 and +0 count as equal: the packed kernel starts odd outputs from h0 * x and even ones from
                fma(h0, x, 0), which differ only in the sign of a zero.
  R2  accuracy  per channel  e2(kernel vs LD) <= MARGIN max(e2(plain vs LD), 1 u),  and over the whole case the worst channel's einf
                against MARGIN max(the worst channel's baseline einf, 1 u).  LD is the same recurrence in x87 extended precision on
                the SAME rounded coefficients (they convert exactly: what is measured is recurrence roundoff, not coefficient
                quantisation); plain is the unfused reference-order recurrence at the working precision.  No fixed bound can serve
                these filters (an f32 recurrence at f0/fs = 0.005 is off by 1e-4), so the error is judged against the baseline
                computed on the same filter and the same input.  Mixed mode is held in units of u = 2^-24 of the stored samples.
                einf is not held per channel: the correct fused model itself reaches 2.7 times the plain einf on single channels.

R1 is to be re-derived, not deleted, when the arithmetic changes on purpose; R2 stays valid through such a change.
"""
import numpy as np

from fft_exact import LD, MARGIN, U as _U

GENERIC, LP, HP, BP = 0, 1, 2, 3
U = {"f32": _U["f32"], "f64": _U["f64"], "mix": _U["f32"]}  # mixed mode: the unit roundoff of the stored samples
SDT = {"f32": np.float32, "f64": np.float64, "mix": np.float32}  # S: the type the samples are stored in
RDT = {"f32": np.float32, "f64": np.float64, "mix": np.float64}  # R: the type the recurrence runs in
FLOOR = 1.0  # u
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------ correctly rounded fused multiply-add
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _round_to_odd_sum(a, b):
    """RO(a + b) in double: the nearest-even sum, moved to its odd neighbour on the side of the error where it is inexact and even"""
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    nudged = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    return np.where((e != 0) & even, nudged, s)


def fmaf(a, b, c):
    """float32 fma(a, b, c), one rounding: the product of two floats is exact in double (48 bits), the sum is rounded to odd at 53
    bits, and a round-to-odd value of 53 >= 24 + 2 bits rounds to float as the exact one does"""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    p = a.astype(F64) * b.astype(F64)
    return np.atleast_1d(_round_to_odd_sum(p, np.broadcast_to(c.astype(F64), p.shape))).astype(F32).reshape(p.shape)


_SPLITTER = F64(2 ** 27 + 1)
_LO, _HI = 2.0 ** -300, 2.0 ** 300


def _in_range(v, what):
    m = np.abs(v[v != 0])
    assert np.all(np.isfinite(v)) and (m.size == 0 or (m.min() > _LO and m.max() < _HI)), \
        f"fma operand {what} outside [2^-300, 2^300]: the error-free product and sum below would over- or underflow"


def _two_prod(a, b):
    p = a * b
    t = _SPLITTER * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLITTER * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """float64 fma(a, b, c) by the Boldo-Melquiond construction: (uh, ul) = TwoProduct(a, b), (th, tl) = TwoSum(c, uh),
    v = RO(tl + ul), result th + v.  Valid without overflow or underflow: the operands' range is asserted, not handled."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=F64) for v in (a, b, c)))
    _in_range(a, "a"), _in_range(b, "b"), _in_range(c, "c")
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    return th + np.atleast_1d(_round_to_odd_sum(tl, ul)).reshape(th.shape)


def fma_t(a, b, c):
    """the kernel's fma_t: the fma of the operands' type"""
    return fmaf(a, b, c) if np.asarray(a).dtype == F32 else fma(a, b, c)


# ------------------------------------------------------------------------------------------------------ the biquad cascade
def _coefficients(a, b, gain, kind, T):
    """(gain, a1, a2, b1, b2) as the kernels hold them: each double cast to T once (make_args); b is read on GENERIC only"""
    a = np.asarray(a, dtype=F64).reshape(-1, 3)
    m = a.shape[0]
    b = np.zeros((m, 3)) if kind != GENERIC else np.asarray(b, dtype=F64).reshape(m, 3)
    return T(gain), [T(v) for v in a[:, 1]], [T(v) for v in a[:, 2]], [T(v) for v in b[:, 1]], [T(v) for v in b[:, 2]]


def _levels(state, m, channels, T):
    """device layout [3 * j + age][channel] -> three lists of m + 1 level vectors (ages 1, 2, 3)"""
    if state is None:
        state = np.zeros((3 * (m + 1), channels), dtype=T)
    state = np.asarray(state)
    assert state.shape == (3 * (m + 1), channels), (state.shape, m, channels)
    return tuple([state[3 * j + age].astype(T) for j in range(m + 1)] for age in range(3))


def _pack(y1, y2, y3, T):
    return np.stack([lv[j] for j in range(len(y1)) for lv in (y1, y2, y3)]).astype(T)


def _unfused_terms(kind, j, y1, y2, nxt1, nxt2, a1, a2, b1, b2):
    """the two increments of section j in the reference's grouping (casc_2o_iir.h; cascade_step's !FUSED branch), one rounding an
    operation in the arrays' type"""
    if kind == GENERIC:
        return y1[j] * b1[j] - nxt1 * a1[j], y2[j] * b2[j] - nxt2 * a2[j]
    if kind == LP:
        return y1[j] + y1[j] - nxt1 * a1[j], y2[j] - nxt2 * a2[j]
    if kind == HP:
        return -y1[j] - y1[j] - nxt1 * a1[j], y2[j] - nxt2 * a2[j]
    return -nxt1 * a1[j], -y2[j] - nxt2 * a2[j]


def _fused_terms(kind, j, y1, y2, nxt1, nxt2, a1, a2, b1, b2):
    """cascade_step's FUSED branch (f32 and mixed mode): every "x b - y a" pair is a multiply and an FMA"""
    if kind == GENERIC:
        return fma_t(y1[j], b1[j], -(nxt1 * a1[j])), fma_t(y2[j], b2[j], -(nxt2 * a2[j]))
    if kind == LP:
        return fma_t(-nxt1, a1[j], y1[j] + y1[j]), fma_t(-nxt2, a2[j], y2[j])
    if kind == HP:
        return fma_t(-nxt1, a1[j], -y1[j] - y1[j]), fma_t(-nxt2, a2[j], y2[j])
    return -nxt1 * a1[j], fma_t(-nxt2, a2[j], -y2[j])


def _run(x, a, b, gain, kind, T, terms, state, out_dtype, coeff_T=None):
    """cascade_step over the rows of x: recurrence type T, coefficients rounded to coeff_T (default T) first"""
    x = np.atleast_2d(np.asarray(x))
    channels, n = x.shape
    g, a1, a2, b1, b2 = _coefficients(a, b, gain, kind, coeff_T or T)
    if coeff_T is not None:
        g, a1, a2, b1, b2 = T(g), [T(v) for v in a1], [T(v) for v in a2], [T(v) for v in b1], [T(v) for v in b2]
    m = len(a1)
    y1, y2, y3 = _levels(state, m, channels, T)
    out = np.empty((channels, n), dtype=out_dtype)
    xr = x.astype(T)  # widened (or kept) once: exact
    for s in range(n):
        cur = [xr[:, s] * g]
        for j in range(m):
            t1, t2 = terms(kind, j, y1, y2, y1[j + 1], y2[j + 1], a1, a2, b1, b2)
            acc = cur[j] + t1  # acc += ...: a rounding of its own each time
            acc = acc + t2
            cur.append(acc)
        y3, y2, y1 = y2, y1, cur
        out[:, s] = cur[m]  # narrowed to the stored type
    return out, _pack(y1, y2, y3, T)


def biquad_model(x, a, b, gain, kind, precision, state=None):
    """iir_step.h's cascade_step restated: x (channels, samples) in the stored type; a, b: 3 m doubles each (b None unless GENERIC);
    state: the device layout [3 * j + age][channel] in R, None = zeros.  The FUSED forms for f32 and mix, the unfused ones for
    f64.  Returns (y in S, final state in R)."""
    terms = _unfused_terms if precision == "f64" else _fused_terms
    assert np.asarray(x).dtype == SDT[precision], (np.asarray(x).dtype, precision)
    return _run(x, a, b, gain, kind, RDT[precision], terms, state, SDT[precision])


def biquad_plain(x, a, b, gain, kind, precision, state=None):
    """the baseline: the unfused reference-order recurrence at R, output narrowed to S"""
    return _run(x, a, b, gain, kind, RDT[precision], _unfused_terms, state, SDT[precision])


def biquad_ld(x, a, b, gain, kind, precision, state=None):
    """the same recurrence in np.longdouble, in the reference's grouping, on the R-rounded coefficients and state (exact
    conversions); the output is not narrowed"""
    return _run(x, a, b, gain, kind, LD, _unfused_terms, state, LD, coeff_T=RDT[precision])


# -------------------------------------------------------------------------------------- forward-backward filtering (filtfilt)
PAD_NONE, PAD_ODD, PAD_EVEN, PAD_CONSTANT = 0, 1, 2, 3


def _extend(x, padtype, P):
    """csrc/iir_filtfilt.hip's extend(), in the stored type: odd = S(2) * edge - mirror (the doubling is exact)"""
    if padtype == PAD_NONE or P == 0:
        return x.copy()
    S = x.dtype.type
    x0, xl = x[:, :1], x[:, -1:]
    lm, rm = x[:, P:0:-1], x[:, -2:-2 - P:-1]
    if padtype == PAD_ODD:
        left, right = S(2) * x0 - lm, S(2) * xl - rm
    elif padtype == PAD_EVEN:
        left, right = lm, rm
    else:
        left, right = np.repeat(x0, P, axis=1), np.repeat(xl, P, axis=1)
    return np.concatenate([left, x, right], axis=1).astype(x.dtype)


def _steady(ss, v, precision):
    """every age of level j = R(s_j) * R(v), one rounding in R"""
    R = RDT[precision]
    lv = np.asarray(ss, dtype=F64).astype(R)[:, None] * v.astype(R)[None, :]
    return np.repeat(lv, 3, axis=0).astype(R)


def filtfilt_model(x, a, b, gain, kind, precision, padtype, padlen, ss):
    """the forward-backward plan as the composition of the bank's model: pad in S, steady-state start, forward, flip, steady-state
    start from the last (stored) forward output, backward, flip, slice.  ss: the m + 1 steady-state levels per unit input in
    double (sdsp_hip_iir_steady_state)."""
    x = np.atleast_2d(np.asarray(x))
    L = x.shape[1]
    P = 0 if padtype == PAD_NONE else padlen
    e = _extend(x, padtype, P)
    u, _ = biquad_model(e, a, b, gain, kind, precision, _steady(ss, e[:, 0], precision))
    u = np.ascontiguousarray(u[:, ::-1])
    w, _ = biquad_model(u, a, b, gain, kind, precision, _steady(ss, u[:, 0], precision))
    return np.ascontiguousarray(w[:, ::-1][:, P:P + L])


# ---------------------------------------------------------------------------------------------------------------- the FIR bank
def _fir_window(x, hist, taps, T):
    """the stream of every row with its history in front: hist (channels, taps - 1), newest input first, None = zeros"""
    x = np.atleast_2d(np.asarray(x))
    channels = x.shape[0]
    if hist is None:
        hist = np.zeros((channels, taps - 1), dtype=x.dtype)
    hist = np.asarray(hist)[:, :taps - 1]
    assert hist.shape == (channels, taps - 1), (hist.shape, channels, taps)
    return np.concatenate([hist[:, ::-1], x], axis=1).astype(T)


def _fir_history(ext, taps, dtype):
    return np.ascontiguousarray(ext[:, ::-1][:, :taps - 1]).astype(dtype)


def fir_model_f32(x, h, hist=None):
    """csrc/fir.hip's f32 kernels: h rounded to float as the plan does, acc = 0, then acc = fmaf(h[k], x[n - k], acc) for ascending
    k.  Returns (y, final history), both float32."""
    assert np.asarray(x).dtype == F32
    h = np.asarray(h, dtype=F64).astype(F32)
    taps, n = h.size, np.atleast_2d(x).shape[1]
    ext = _fir_window(x, hist, taps, F32)
    acc = np.zeros((ext.shape[0], n), dtype=F32)
    for k in range(taps):
        acc = fmaf(h[k], ext[:, taps - 1 - k:taps - 1 - k + n], acc)
    return acc, _fir_history(ext, taps, F32)


def fir_plain(x, h, hist=None, precision="f64"):
    """multiply then add, unfused, ascending taps, acc = h[0] x[n] first: the f64 kernel's (and the oracle's) order; at f32 the
    baseline of R2"""
    T = RDT[precision]
    h = np.asarray(h, dtype=F64).astype(T)
    taps, n = h.size, np.atleast_2d(x).shape[1]
    ext = _fir_window(x, hist, taps, T)
    acc = h[0] * ext[:, taps - 1:taps - 1 + n]
    for k in range(1, taps):
        acc = acc + h[k] * ext[:, taps - 1 - k:taps - 1 - k + n]
    return acc.astype(T), _fir_history(ext, taps, T)


def fir_ld(x, h, hist=None, precision="f32"):
    """the same sum in np.longdouble on the coefficients rounded to the working precision"""
    h = np.asarray(h, dtype=F64).astype(RDT[precision]).astype(LD)
    taps, n = h.size, np.atleast_2d(x).shape[1]
    ext = _fir_window(x, hist, taps, LD)
    acc = np.zeros((ext.shape[0], n), dtype=LD)
    for k in range(taps):
        acc = acc + h[k] * ext[:, taps - 1 - k:taps - 1 - k + n]
    return acc


# ------------------------------------------------------------------------------------------------------------------ the rules
def errors(got, ref, prec):
    """per row (e2, einf) in units of u: ||got - ref||_2 / ||ref||_2 and max |got - ref| / max |ref|, as fft_exact.errors"""
    ref = np.atleast_2d(ref)
    d = np.abs(np.atleast_2d(got).astype(LD) - ref)
    a = np.abs(ref)
    e2 = np.sqrt((d * d).sum(axis=1)) / np.sqrt((a * a).sum(axis=1))
    einf = d.max(axis=1) / a.max(axis=1)
    return (e2 / U[prec]).astype(F64), (einf / U[prec]).astype(F64)


def _as_int(v, zero_sign):
    v = np.ascontiguousarray(v)
    assert v.dtype in (F32, F64), v.dtype
    if zero_sign:  # -0 -> +0
        v = np.where(v == 0, v.dtype.type(0), v)
    return np.ascontiguousarray(v).view(np.int32 if v.dtype == F32 else np.int64)


def bit_diff(got, want, ignore_zero_sign=False):
    """(count, first differing index or None) of two arrays compared as integers"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    ne = _as_int(got, ignore_zero_sign) != _as_int(want, ignore_zero_sign)
    n = int(ne.sum())
    return n, (tuple(int(i) for i in np.argwhere(ne)[0]) if n else None)


def r1(got, want, what, ignore_zero_sign=False):
    """R1 on one array: "" or the failure text with the count and the first differing (channel, sample)"""
    n, first = bit_diff(got, want, ignore_zero_sign)
    if not n:
        return ""
    return (f"{what}: {n} of {np.asarray(got).size} elements differ from the model, first at {first}: "
            f"got {np.asarray(got)[first]!r}, model {np.asarray(want)[first]!r}")


def r2(got, plain, ref, prec):
    """R2 on one case.  Returns (failure text or "", figures): per channel e2, whole-case einf; figures = dict of the worst
    channel's e2 / einf for kernel and baseline and the ratio that is held to MARGIN"""
    e2, einf = errors(got, ref, prec)
    b2, binf = errors(plain, ref, prec)
    bound2 = MARGIN * np.maximum(b2, FLOOR)
    boundinf = MARGIN * max(float(binf.max()), FLOOR)
    ratio = max(float((e2 / np.maximum(b2, FLOOR)).max()), float(einf.max()) / max(float(binf.max()), FLOOR))
    fig = dict(e2=float(e2.max()), einf=float(einf.max()), base2=float(b2.max()), baseinf=float(binf.max()), ratio=ratio)
    bad = np.flatnonzero(~(e2 <= bound2))  # also catches NaN
    msg = []
    if bad.size:
        c = int(bad[0])
        msg.append(f"{bad.size} channels over in e2, first {c}: {e2[c]:.3f} u against {MARGIN} x max({b2[c]:.3f}, {FLOOR}) u")
    if not float(einf.max()) <= boundinf:
        msg.append(f"einf of the worst channel {einf.max():.3f} u against {MARGIN} x max({binf.max():.3f}, {FLOOR}) u")
    return "; ".join(msg), fig


def verdict(r1_msgs, r2_msg):
    """the text of a failed case: when R1 fails it also says whether R2 holds, which tells "wrong" from "different rounding" """
    r1_msgs = [m for m in r1_msgs if m]
    parts = []
    if r1_msgs:
        parts.append("R1 (bits) fails: " + " | ".join(r1_msgs))
        parts.append("R2 (accuracy) holds: the values are as accurate as the plain recurrence, so this is a different rounding "
                     "sequence, not a wrong value" if not r2_msg else "R2 (accuracy) fails too: " + r2_msg)
    elif r2_msg:
        parts.append("R2 (accuracy) fails: " + r2_msg)
    return "\n".join(parts)
