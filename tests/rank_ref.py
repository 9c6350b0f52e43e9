"""The contract of the rank-order filter bank (include/sdsp_hip.h: sdsp_hip_rank_*) in numpy: history then
block, values to totalOrder keys, sliding windows, sort, take rank r, keys back to values.  tests/test_rank_host.py pins it to a
scalar loop and to scipy; tests/test_gpu_rank.py holds both kernels to its bits."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def row_dtype(precision):
    return np.float64 if precision == "f64" else np.float32


def to_key(x):
    """totalOrder keys of a float array: ~u where the sign bit is set, else u | signbit (u = the bits as an unsigned integer)"""
    x = np.ascontiguousarray(x)
    ut = UINT[x.dtype]
    u = x.view(ut)
    sign = ut(1) << ut(8 * u.itemsize - 1)
    return np.where(u & sign != 0, ~u, u | sign).astype(ut)


def from_key(k, dtype):
    ut = UINT[np.dtype(dtype)]
    k = np.ascontiguousarray(k, dtype=ut)
    sign = ut(1) << ut(8 * k.itemsize - 1)
    return np.where(k & sign != 0, k ^ sign, ~k).astype(ut).view(dtype)


def specials(dtype):
    """bit patterns that stress the order: both zeros, denormals, ones, the largest finite values, infinities, and NaNs of both signs
    with several payloads -- among them the all-ones pattern (key 0) and 0x7FFF..F (key all-ones), the two a sentinel's key equals"""
    ut = UINT[np.dtype(dtype)]
    if np.dtype(dtype) == np.float32:
        pos = [0x00000000, 0x00000001, 0x007FFFFF, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7F800001, 0x7FC00000, 0x7FC00123, 0x7FFFFFFF]
        sign = 0x80000000
    else:
        pos = [0x0000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000,
               0x7FF0000000000001, 0x7FF8000000000000, 0x7FF8000000000123, 0x7FFFFFFFFFFFFFFF]
        sign = 0x8000000000000000
    return np.array(pos + [p | sign for p in pos], dtype=ut).view(dtype)


def rank_ref(x, window, rank, hist=None):
    """x: (channels, S) float32 / float64; hist: (channels, window - 1), newest first, or None for zeros.
    Returns (y (channels, S), new history (channels, window - 1))."""
    x = np.ascontiguousarray(x)
    C, S = x.shape
    W = window
    assert 0 <= rank < W
    if hist is None:
        hist = np.zeros((C, W - 1), dtype=x.dtype)
    assert hist.shape == (C, W - 1) and hist.dtype == x.dtype
    full = np.concatenate([hist[:, ::-1], x], axis=1)  # oldest first
    new_hist = np.ascontiguousarray(full[:, full.shape[1] - (W - 1):][:, ::-1])
    if S == 0:
        return np.zeros((C, 0), dtype=x.dtype), new_hist
    keys = to_key(full)
    win = sliding_window_view(keys, W, axis=1)  # (C, S, W)
    picked = np.sort(win, axis=2)[:, :, rank]
    return from_key(picked, x.dtype), new_hist


def rank_ref_stream(x, window, rank, blocks, hist=None):
    """the same stream fed in calls of the given lengths"""
    outs, s0 = [], 0
    for n in blocks:
        y, hist = rank_ref(x[:, s0:s0 + n], window, rank, hist)
        outs.append(y)
        s0 += n
    assert s0 == x.shape[1]
    return np.concatenate(outs, axis=1), hist
