"""The numpy statement of the 2-D CFAR contract (include/sdsp_hip.h: sdsp_hip_cfar2d_*): the sums in the
contract's order at the precision, n(r), the scale tables, both edge modes, the peak rule and the ordered hit list.  Every addition is
one numpy operation on arrays of the precision, so each is rounded once and none is fused."""
from __future__ import annotations

import math

import numpy as np

MARK, CLIP = 0, 1


def cells(R: int, Ld: int, Gd: int, Lr: int, Gr: int) -> np.ndarray:
    """n(r): the training cells of column r that lie inside the map"""
    r = np.arange(R, dtype=np.int64)

    def inside(h):
        return np.minimum(r + h, R - 1) - np.maximum(r - h, 0) + 1

    return (2 * (Ld + Gd) + 1) * inside(Lr + Gr) - (2 * Gd + 1) * inside(Gr)


def alpha_table(R, geom, alpha: float) -> np.ndarray:
    """c(r) = alpha / n(r) in double"""
    with np.errstate(all="ignore"):
        return np.float64(alpha) / cells(R, *geom).astype(np.float64)


def pfa_table(R, geom, pfa: float) -> np.ndarray:
    """c(r) = pfa^(-1 / n(r)) - 1 in double, with the C library's pow; +inf where n(r) = 0"""
    return np.array([math.pow(pfa, -1.0 / n) - 1.0 if n else math.inf for n in cells(R, *geom).tolist()], dtype=np.float64)


def total(p: np.ndarray, geom) -> np.ndarray:
    """T of every cell of p (maps, D, R), in p's dtype"""
    Ld, Gd, Lr, Gr = geom
    Hd, Hr = Ld + Gd, Lr + Gr
    maps, D, R = p.shape
    dt = p.dtype
    with np.errstate(all="ignore"):
        pp = np.zeros((maps, D, R + 2 * Hr), dtype=dt)
        pp[:, :, Hr:Hr + R] = p

        def across(lo, hi):  # sum over j = lo .. hi of p[d][r + j], ascending, from +0
            acc = np.zeros((maps, D, R), dtype=dt)
            for j in range(lo, hi + 1):
                acc = acc + pp[:, :, Hr + j:Hr + j + R]
            return acc

        lag, mid, lead = across(-Hr, -Gr - 1), across(-Gr, Gr), across(Gr + 1, Hr)
        side = lag + lead
        full = (lag + mid) + lead

        def down(a, lo, hi):  # sum over i = lo .. hi of a[(d + i) mod D], ascending, from +0
            acc = np.zeros((maps, D, R), dtype=dt)
            for i in range(lo, hi + 1):
                acc = acc + np.roll(a, -i, axis=1)
            return acc

        top, band, bottom = down(full, -Hd, -Gd - 1), down(side, -Gd, Gd), down(full, Gd + 1, Hd)
        return (top + band) + bottom


def canonical(thr: np.ndarray) -> np.ndarray:
    """every NaN becomes the canonical quiet NaN"""
    u = np.uint32 if thr.dtype == np.float32 else np.uint64
    quiet = u(0x7FC00000) if thr.dtype == np.float32 else u(0x7FF8000000000000)
    out = thr.copy()
    out.view(u)[np.isnan(thr)] = quiet
    return out


def detect(p: np.ndarray, geom, scale: np.ndarray, edge: int = MARK, peak: bool = False):
    """p: (maps, D, R) of the precision; scale: R doubles c(r).  Returns thr (p's dtype), det (uint8) and the list of hit lists: per
    map a structured array (doppler, range, power, thr) in ascending (doppler, range)."""
    Ld, Gd, Lr, Gr = geom
    Hr = Lr + Gr
    maps, D, R = p.shape
    dt = p.dtype
    with np.errstate(all="ignore"):
        c = np.asarray(scale, dtype=np.float64).astype(dt)
        thr = canonical(total(p, geom) * c[None, None, :])
        if edge == MARK:
            r = np.arange(R)
            thr[:, :, (r < Hr) | (r >= R - Hr)] = np.inf
        det = p > thr
        if peak:
            for i in (-1, 0, 1):
                for j in (-1, 0, 1):
                    if i == 0 and j == 0:
                        continue
                    q = np.roll(p, -i, axis=1)  # q[d] = p[(d + i) mod D]
                    qq = np.zeros_like(p)
                    ok = np.zeros((maps, D, R), dtype=bool)  # the neighbour column lies in the map
                    if j == 0:
                        qq, ok[:] = q, True
                    elif j < 0:
                        qq[:, :, 1:], ok[:, :, 1:] = q[:, :, :-1], True
                    else:
                        qq[:, :, :-1], ok[:, :, :-1] = q[:, :, 1:], True
                    before = i < 0 or (i == 0 and j < 0)
                    wins = (p > qq) if before else (p >= qq)
                    det &= wins | ~ok
    lists = []
    for m in range(maps):
        at = np.argwhere(det[m])  # row-major: ascending (d, r)
        h = np.zeros(len(at), dtype=hit_dtype(dt))
        h["doppler"], h["range"] = at[:, 0], at[:, 1]
        h["power"], h["thr"] = p[m][det[m]], thr[m][det[m]]
        lists.append(h)
    return thr, det.astype(np.uint8), lists


def hit_dtype(real) -> np.dtype:
    """sdsp_hip_cfar2d_hit_f32 / _f64"""
    real = np.dtype(real)
    return np.dtype({"names": ["doppler", "range", "power", "thr"], "formats": [np.uint32, np.uint32, real, real],
                     "offsets": [0, 4, 8, 8 + real.itemsize], "itemsize": 8 + 2 * real.itemsize})


def brute(p: np.ndarray, geom, clip_count: bool = True):
    """the training set by its definition, one cell at a time in float64: (sum, count) of every cell of one map p (D, R)"""
    Ld, Gd, Lr, Gr = geom
    Hd, Hr = Ld + Gd, Lr + Gr
    D, R = p.shape
    s, n = np.zeros((D, R)), np.zeros((D, R), dtype=np.int64)
    p64 = p.astype(np.float64)
    for d in range(D):
        for r in range(R):
            for i in range(-Hd, Hd + 1):
                for j in range(-Hr, Hr + 1):
                    if (abs(i) <= Gd and abs(j) <= Gr) or not 0 <= r + j < R:
                        continue
                    s[d, r] += p64[(d + i) % D, r + j]
                    n[d, r] += 1
    return s, n
