"""numpy reference of the symbol-timing recovery bank (include/sdsp_hip.h: sdsp_hip_timing_*) in exactly the
contract's operation order, vectorised over the channels with per-channel stream times: one pass of the Python loop is one strobe of
every channel that is still inside the call.  Also what the timing tests share: the lock signals and their figures.

The table is made here in double and rounded with astype, as the plan rounds it, so the reference needs neither the library nor a
device.  alpha, beta and max_dev are host doubles rounded here with the precision's type, as the library rounds them.  f64 follows
the order literally (numpy never contracts); in f32 one fmaf is lms_ref._fma32 (exact double product, round-to-odd sum, one rounding
to f32).  Time is exact: uint64 words."""
import numpy as np

from arb_ref import tables
from lms_ref import BLOCKS, _fma32  # noqa: F401  (BLOCKS is re-exported for the tests)

MODES = ("gardner", "zc_qpsk", "zc_bpsk")
ONE = 1 << 32
_U32 = np.uint64(32)


def real_dtype(precision):
    return np.float64 if precision == "f64" else np.float32


def row_dtype(precision):
    return np.complex128 if precision == "f64" else np.complex64


def step_of(sps):
    """round(sps / 2 2^32), ties to even, on an exact product"""
    return round(sps * 2.0 ** 31)


def max_out(step0, samples):
    """the most symbols any loop yields from `samples` inputs: every half step is at least step0 - 2^31, so at most
    n = ceil(samples 2^32 / (step0 - 2^31)) strobes start below `samples`, (n + 1) / 2 of them symbol strobes"""
    least = int(step0) - (1 << 31)
    return (-((-(samples << 32)) // least) + 1) // 2


def gains(bn, zeta, kd, sps):
    theta = bn / (zeta + 1.0 / (4.0 * zeta))
    d = 1.0 + 2.0 * zeta * theta + theta * theta
    return 4.0 * zeta * theta / (d * kd) * sps / 2.0, 4.0 * theta * theta / (d * kd) * sps / 2.0


def _ma(a, b, c):
    """ma(a, b, c) = a b + c: one fmaf in f32, a multiply then an add in f64"""
    if c.dtype == np.float32:
        return _fma32(np.broadcast_to(a, c.shape), np.broadcast_to(b, c.shape), c)
    return a * b + c


def _sign(v):
    """+-1 by the sign bit: -0 counts as negative; a NaN stays a NaN"""
    return np.where(np.isnan(v), v, np.where(np.signbit(v), v.dtype.type(-1), v.dtype.type(1)))


def zero_state(channels, T, precision="f64"):
    dt, rt = real_dtype(precision), row_dtype(precision)
    return dict(t=np.zeros(channels, dtype=np.uint64), ps=np.zeros(channels, dtype=rt), ym=np.zeros(channels, dtype=rt),
                integ=np.zeros(channels, dtype=dt), w=np.zeros(channels, dtype=np.int32), parity=np.zeros(channels, dtype=np.uint32),
                hist=np.zeros((channels, T - 1), dtype=rt))


def state_bytes_of(state):
    """the state as the library lays it out: one array per field, each at the next multiple of 8 bytes, the history last"""
    out = b""
    for name in ("t", "ps", "ym", "integ", "w", "parity", "hist"):
        b = np.ascontiguousarray(state[name]).tobytes()
        out += b + b"\0" * (-len(b) % 8)
    return out


def timing_ref(h, L, T, x, step0, alpha, beta, mode="gardner", max_dev=0.5, state=None, precision="f64", pin_w=None):
    """x: (channels, S) complex; state: a dict as zero_state's, or None for a fresh loop; pin_w: an advance word that replaces every w
    (for the capacity test).  Returns (y, err, period, counts, state, times): y (channels, max_out) complex, err and period alike
    but real, zero behind each row's count; counts (channels,) uint32; the new state; times (channels, max_out) uint64, each symbol
    strobe's t (the integer part counts from this call's first sample), which the lock figures use."""
    assert mode in MODES
    dt, rt = real_dtype(precision), row_dtype(precision)
    x = np.atleast_2d(np.asarray(x)).astype(rt)
    C, S = x.shape
    Hn = T - 1
    lb = L.bit_length() - 1
    assert 1 << lb == L and ONE <= step0 <= (1 << 38)
    st = zero_state(C, T, precision) if state is None else {k: np.array(v) for k, v in state.items()}
    t, ps, ym, integ, w, parity = st["t"], st["ps"], st["ym"], st["integ"], st["w"], st["parity"]
    assert t.dtype == np.uint64 and integ.dtype == dt and ps.dtype == rt and w.dtype == np.int32
    if pin_w is not None:
        w[:] = pin_w
    ext = np.concatenate([st["hist"].reshape(C, Hn)[:, ::-1], x], axis=1)  # ext[:, Hn + n] = x[n]
    ext2 = np.stack([np.ascontiguousarray(ext.real), np.ascontiguousarray(ext.imag)])  # both planes alike
    Ht = tables(h, L, T)[0].astype(dt)
    alpha, beta, dev = dt(alpha), dt(beta), dt(max_dev)
    lo, hi = dt(-2.0 ** 31), dt(2.0 ** 31 - (128 if precision == "f32" else 1))
    cap = max_out(step0, S)
    y = np.zeros((C, cap), dtype=rt)
    err, period = np.zeros((C, cap), dtype=dt), np.zeros((C, cap), dtype=dt)
    times = np.zeros((C, cap), dtype=np.uint64)
    m = np.zeros(C, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            idx = np.nonzero((t >> _U32) < np.uint64(S))[0]
            if idx.size == 0:
                break
            ti = t[idx]
            i = (ti >> _U32).astype(np.int64)
            f = ti & np.uint64(0xffffffff)
            p = (f >> np.uint64(32 - lb)).astype(np.int64) if lb else np.zeros(idx.size, dtype=np.int64)
            z = Ht[p, 0] * ext2[:, idx, Hn + i]  # a plain product
            for k in range(1, T):
                z = _ma(Ht[p, k], ext2[:, idx, Hn + i - k], z)
            assert z.dtype == dt
            zr, zi = z[0], z[1]
            sym = parity[idx] != 0
            mid = idx[~sym]
            ym.real[mid], ym.imag[mid] = zr[~sym], zi[~sym]
            parity[mid] = 1
            if sym.any():
                s = idx[sym]
                zr, zi = zr[sym], zi[sym]
                pr, pi = np.ascontiguousarray(ps.real[s]), np.ascontiguousarray(ps.imag[s])
                mr, mi = np.ascontiguousarray(ym.real[s]), np.ascontiguousarray(ym.imag[s])
                if mode == "gardner":
                    e = _ma(pi - zi, mi, (pr - zr) * mr)
                elif mode == "zc_qpsk":
                    e = _ma(_sign(pi) - _sign(zi), mi, (_sign(pr) - _sign(zr)) * mr)
                else:
                    e = (_sign(pr) - _sign(zr)) * mr
                g = _ma(beta, e, integ[s])
                g = np.where(g < -dev, -dev, np.where(g > dev, dev, g))  # a NaN stays
                v = _ma(alpha, e, g)
                q = v * dt(2.0 ** 32)
                q = np.where(q < lo, lo, np.where(q > hi, hi, q))
                q = np.where(np.isnan(q), dt(0), q)
                assert e.dtype == dt and g.dtype == dt and q.dtype == dt
                integ[s] = g
                w[s] = np.rint(q).astype(np.int64).astype(np.int32) if pin_w is None else pin_w
                y.real[s, m[s]], y.imag[s, m[s]] = zr, zi
                err[s, m[s]], period[s, m[s]] = e, g
                times[s, m[s]] = t[s]
                m[s] += 1
                ps.real[s], ps.imag[s] = zr, zi
                parity[s] = 0
            t[idx] = ti + np.uint64(step0) + w[idx].astype(np.int64).view(np.uint64)  # mod 2^64: a negative w subtracts
    assert (m <= cap).all()
    t -= np.uint64(S << 32)
    new = dict(t=t, ps=ps, ym=ym, integ=integ, w=w, parity=parity, hist=ext[:, ::-1][:, :Hn].copy())
    return y, err, period, m.astype(np.uint32), new, times


def timing_ref_stream(h, L, T, x, step0, calls, mode="gardner", max_dev=0.5, state=None, precision="f64"):
    """the reference fed call by call: calls = [(samples, alpha, beta)].  Returns (y, err, period, counts, state): per channel the
    concatenated symbols of all calls as lists of 1-D arrays, the total counts and the final state."""
    C = np.atleast_2d(x).shape[0]
    ys, es, ps = [[] for _ in range(C)], [[] for _ in range(C)], [[] for _ in range(C)]
    s0 = 0
    for n, alpha, beta in calls:
        y, e, p, cnt, state, _ = timing_ref(h, L, T, x[:, s0:s0 + n], step0, alpha, beta, mode, max_dev, state, precision)
        for c in range(C):
            ys[c].append(y[c, :cnt[c]])
            es[c].append(e[c, :cnt[c]])
            ps[c].append(p[c, :cnt[c]])
        s0 += n
    cat = lambda rows: [np.concatenate(r) for r in rows]  # noqa: E731
    ys, es, ps = cat(ys), cat(es), cat(ps)
    return ys, es, ps, np.array([r.size for r in ys], dtype=np.uint32), state


def rows_of(y, counts):
    """the per-channel rows of one call, as timing_ref_stream returns them"""
    return [y[c, :counts[c]] for c in range(y.shape[0])]


# ---- the root-raised-cosine pulse and prototype
def rrc(tau, rolloff):
    """the unit-energy root-raised-cosine pulse at tau symbols, the two removable singularities at their limits"""
    tau = np.asarray(tau, dtype=np.float64)
    b = rolloff
    u = 4.0 * b * tau
    zero, edge = tau == 0.0, np.abs(np.abs(u) - 1.0) < 1e-9
    safe = np.where(zero | edge, 0.1, tau)  # a harmless value: the edge 1 / (4 b) is at least 0.25
    us = 4.0 * b * safe
    v = (np.sin(np.pi * safe * (1 - b)) + us * np.cos(np.pi * safe * (1 + b))) / (np.pi * safe * (1 - us * us))
    v = np.where(zero, 1.0 - b + 4.0 * b / np.pi, v)
    lim = b / np.sqrt(2.0) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * b)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * b)))
    return np.where(edge, lim, v)


def design(L, T, sps, rolloff):
    """sdsp_hip_timing_design's formula: the pulse at sps L per symbol, centred at (L T - 1) / 2, summing to L"""
    j = np.arange(L * T, dtype=np.float64)
    v = rrc((j - 0.5 * (L * T - 1)) / (sps * L), rolloff)
    return v * (L / v.sum())


# ---- the lock test's signals (tests/test_timing_host.py on the reference, tests/test_gpu_timing.py on the device)
LOCK_CHANNELS, LOCK_SYMBOLS, LOCK_TAIL, LOCK_NOISE, LOCK_ROLLOFF, LOCK_PHASES, LOCK_SPAN = 8, 3000, 1000, 0.05, 0.35, 32, 8


def lock_shape(sps):
    """(L, T) of the lock tests' interpolator: LOCK_PHASES phases, a prototype LOCK_SPAN symbols long"""
    return LOCK_PHASES, int(LOCK_SPAN * sps)


def pulse_train(sym, period, tau0, samples, rolloff=LOCK_ROLLOFF, span=LOCK_SPAN):
    """x[c, n] = sum over k of sym[c, k] rrc((n - tau0[c]) / period[c] - k), the pulse cut at +-span symbols; complex128"""
    C, K = sym.shape
    n = np.arange(samples, dtype=np.float64)
    u = (n[None, :] - np.asarray(tau0, dtype=np.float64)[:, None]) / np.asarray(period, dtype=np.float64)[:, None]
    k0 = np.floor(u).astype(np.int64)
    x = np.zeros((C, samples), dtype=np.complex128)
    rows = np.arange(C)[:, None]
    for j in range(-span, span + 1):
        k = k0 + j
        ok = (k >= 0) & (k < K)
        x += np.where(ok, sym[rows, np.clip(k, 0, K - 1)] * rrc(u - k, rolloff), 0.0)
    return x


def lock_signal(mode, sps, delta, seed=0):
    """(x, sym, tau0, period): LOCK_CHANNELS rows of root-raised-cosine shaped unit-amplitude symbols (BPSK for "zc_bpsk", QPSK
    otherwise) at a period of sps (1 + delta) samples, symbol k centred at tau0 + k period with a random fractional start, plus complex
    Gaussian noise of LOCK_NOISE per component; complex128"""
    rng = np.random.default_rng(1000 * MODES.index(mode) + int(round(sps * 10)) + (7 if delta < 0 else 0) + seed)
    C, K = LOCK_CHANNELS, LOCK_SYMBOLS + 2 * LOCK_SPAN
    period = np.full(C, sps * (1.0 + delta))
    S = int(LOCK_SYMBOLS * sps)
    tau0 = rng.uniform(0.0, 1.0, C) * period
    if mode == "zc_bpsk":
        sym = (2.0 * rng.integers(0, 2, (C, K)) - 1.0).astype(np.complex128)
    else:
        sym = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, (C, K))))
    x = pulse_train(sym, period, tau0, S)
    x = x + LOCK_NOISE * (rng.standard_normal((C, S)) + 1j * rng.standard_normal((C, S)))
    return x, sym, tau0, period


def filter_delay(L, T):
    """samples by which the interpolator's output lags its input: the prototype's centre, (L T - 1) / 2 positions of 1 / L sample"""
    return (L * T - 1) / (2.0 * L)


def lock_figures(y, period, counts, times, sym, tau0, true_period, sps, L, T, tail=LOCK_TAIL):
    """(max over channels of |mean of period over the tail - (true - nominal) / 2|, max over channels of the RMS distance of the
    tail's symbols from the transmitted ones), in double.  A symbol strobe at stream time t shows the input at t - filter_delay, so
    it belongs to transmitted symbol round((t - delay - tau0) / true_period)."""
    worst_p, worst_d = 0.0, 0.0
    for c in range(y.shape[0]):
        n = int(counts[c])
        assert n >= 2 * tail, (c, n)
        sl = slice(n - tail, n)
        worst_p = max(worst_p, abs(period[c, sl].astype(np.float64).mean() - (true_period[c] - sps) / 2.0))
        at = times[c, sl].astype(np.float64) / 2.0 ** 32 - filter_delay(L, T)
        k = np.rint((at - tau0[c]) / true_period[c]).astype(np.int64)
        assert (k >= 0).all() and (k < sym.shape[1]).all() and (np.diff(k) == 1).all(), c  # one strobe per symbol, none slipped
        d = y[c, sl].astype(np.complex128) - sym[c, k]
        worst_d = max(worst_d, float(np.sqrt(np.mean(np.abs(d) ** 2))))
    return worst_p, worst_d


def detector_slope(mode, sps, L, T, h, eps=0.05, symbols=400, seed=5):
    """kd: the open-loop slope of the detector in units of e per symbol of timing offset, read off the reference in double with zero
    gains: noiseless signals whose symbol peaks lie eps symbols after and before the symbol strobes; e < 0 means the strobes are late,
    so kd = (mean e at early strobes - mean e at late strobes) / (2 eps)"""
    rng = np.random.default_rng(seed)
    K = symbols + 2 * LOCK_SPAN
    if mode == "zc_bpsk":
        sym = (2.0 * rng.integers(0, 2, (1, K)) - 1.0).astype(np.complex128)
    else:
        sym = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, (1, K))))
    step0 = step_of(sps)
    half = step0 / 2.0 ** 32
    means = []
    for off in (+eps, -eps):  # peaks after the strobes (strobes early), then before (late)
        # symbol strobes fall at half (2 m + 1); peak k shows at tau0 + delay + k sps in the output
        tau0 = half + off * sps - filter_delay(L, T) + LOCK_SPAN * sps
        x = pulse_train(sym, np.array([float(sps)]), np.array([tau0]), int(symbols * sps))
        _, e, _, cnt, _, _ = timing_ref(h, L, T, x, step0, 0.0, 0.0, mode, 0.5, None, "f64")
        means.append(e[0, 2 * LOCK_SPAN:cnt[0]].mean())
    return (means[0] - means[1]) / (2 * eps)
