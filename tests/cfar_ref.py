"""The contract of the CFAR detector bank (include/sdsp_hip.h: sdsp_hip_cfar_*) in numpy: history then block,
I/Q to power with two rounded products and a rounded sum, sliding windows, a Python loop over the L columns of each side with
correctly rounded additions (numpy adds two arrays of one dtype element by element, each sum rounded once), keys, sort and take k for
OS, one rounded product (a NaN product becomes the canonical quiet NaN), one comparison.  tests/test_cfar_host.py pins it to a scalar
loop; tests/test_gpu_cfar.py holds every kernel to its bits."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from rank_ref import from_key, row_dtype, to_key

MODES = ("ca", "go", "so", "os")
# calls of a stream: empty ones, single samples, ragged ones (the names stand for lengths that depend on the geometry)
BLOCKS = (0, 1, "half", 0, "W-2", "W-1", "W", 3, 0, "rest")


def geometry(train, guard):
    half = train + guard
    return half, 2 * half + 1, train + 2 * guard + 1  # half, W, D


def block_lengths(train, guard, total):
    """BLOCKS as numbers that sum to `total`"""
    half, W, _ = geometry(train, guard)
    names = {"half": half, "W-2": W - 2, "W-1": W - 1, "W": W}
    out = [names.get(b, b) for b in BLOCKS[:-1]]
    rest = total - sum(out)
    assert rest >= 0, "the stream is shorter than the fixed calls"
    return out + [rest]


def in_dtype(precision, kind):
    if kind == "iq":
        return np.complex128 if precision == "f64" else np.complex64
    return row_dtype(precision)


def power(x):
    """POWER rows as they are; IQ (complex) rows: fl(fl(re re) + fl(im im))"""
    x = np.ascontiguousarray(x)
    if np.iscomplexobj(x):
        re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
        return (re * re) + (im * im)
    return x


def scale(mode, train, alpha, dtype):
    """c: a double rounded once to the precision"""
    c = {"ca": alpha / (2.0 * train), "go": alpha / train, "so": alpha / train, "os": alpha}[mode]
    return np.dtype(dtype).type(c)


def side_sums(p, train, guard):
    """p: (C, S + W - 1) powers, oldest first.  Returns (lag, lead), each (C, S): (((+0 + first) + next) + ..) in ascending index"""
    _, W, _ = geometry(train, guard)
    win = sliding_window_view(p, W, axis=1)  # (C, S, W): win[.., n, i] = p[n - W + 1 + i]
    lag = np.zeros(win.shape[:2], dtype=p.dtype)
    lead = np.zeros(win.shape[:2], dtype=p.dtype)
    with np.errstate(all="ignore"):
        for i in range(train):
            lag = lag + win[:, :, i]
            lead = lead + win[:, :, W - train + i]
    return lag, lead


def cfar_ref(x, train, guard, mode, alpha, rank=None, hist=None):
    """x: (channels, S) float32 / float64 power or complex64 / complex128 I/Q; hist: (channels, W - 1) of x's dtype, newest first, or
    None for zeros.  Returns (thr (channels, S), det (channels, S) uint8, new history (channels, W - 1))."""
    assert mode in MODES
    x = np.ascontiguousarray(x)
    C, S = x.shape
    L = train
    half, W, _ = geometry(train, guard)
    if hist is None:
        hist = np.zeros((C, W - 1), dtype=x.dtype)
    assert hist.shape == (C, W - 1) and hist.dtype == x.dtype
    full = np.concatenate([hist[:, ::-1], x], axis=1)  # oldest first
    new_hist = np.ascontiguousarray(full[:, full.shape[1] - (W - 1):][:, ::-1])
    p = power(full)
    rt = p.dtype
    if S == 0:
        return np.zeros((C, 0), dtype=rt), np.zeros((C, 0), dtype=np.uint8), new_hist
    c = scale(mode, L, alpha, rt)
    with np.errstate(all="ignore"):
        if mode == "os":
            assert rank is not None and 0 <= rank < 2 * L
            win = sliding_window_view(to_key(p), W, axis=1)
            cells = np.concatenate([win[:, :, :L], win[:, :, W - L:]], axis=2)  # (C, S, 2 L)
            v = from_key(np.sort(cells, axis=2)[:, :, rank], rt)
            thr = v * c
        else:
            lag, lead = side_sums(p, L, guard)
            if mode == "ca":
                thr = (lag + lead) * c
            elif mode == "go":
                thr = np.where(lag > lead, lag, lead) * c
            else:
                thr = np.where(lag < lead, lag, lead) * c
        thr = np.where(np.isnan(thr), rt.type(np.nan), thr)  # a NaN threshold is the canonical quiet NaN (np.nan's bits)
        cut = p[:, W - 1 - half:W - 1 - half + S]  # p[n - half]
        det = (cut > thr).astype(np.uint8)
    return np.ascontiguousarray(thr.astype(rt)), det, new_hist


def cfar_ref_stream(x, train, guard, mode, alpha, blocks, rank=None, hist=None):
    """the same stream fed in calls of the given lengths"""
    thrs, dets, s0 = [], [], 0
    for n in blocks:
        t, d, hist = cfar_ref(x[:, s0:s0 + n], train, guard, mode, alpha, rank, hist)
        thrs.append(t)
        dets.append(d)
        s0 += n
    assert s0 == x.shape[1]
    return np.concatenate(thrs, axis=1), np.concatenate(dets, axis=1), hist


def cfar_ref_rows(x, train, guard, mode, alpha, rank=None):
    """finite rows (simpledsp_amd.cfar): output n belongs to cell n; the first and last half cells are untested (thr = +inf, det = 0)"""
    x = np.ascontiguousarray(x)
    half, _, _ = geometry(train, guard)
    S = x.shape[1]
    padded = np.concatenate([x, np.zeros((x.shape[0], half), dtype=x.dtype)], axis=1)
    thr, det, _ = cfar_ref(padded, train, guard, mode, alpha, rank)
    thr, det = thr[:, half:].copy(), det[:, half:].copy()
    edge = min(half, S)
    thr[:, :edge] = np.inf
    thr[:, S - edge:] = np.inf
    det[:, :edge] = 0
    det[:, S - edge:] = 0
    return thr, det
