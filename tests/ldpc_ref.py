"""The contract of the LDPC decoder banks (include/sdsp_hip.h: sdsp_hip_ldpc_*) in numpy, vectorised over
codewords: layered normalised / offset min-sum on integers over a quasi-cyclic code given as a base matrix of shifts and a lifting
size.  Also the test-code generator (a test utility, not a recommended code), a direct encoder for its staircase codes, and the
quantisers of the two input kinds."""
import numpy as np


class Code:
    """base: mb x nb shifts, -1 for the zero block; entry s is the circulant with a one at (i, (i + s) mod z)"""

    def __init__(self, base, z):
        self.base = np.asarray(base, dtype=np.int64)
        self.mb, self.nb = self.base.shape
        self.z = int(z)
        self.n, self.m = self.nb * self.z, self.mb * self.z
        self.k = self.n - self.m
        i = np.arange(self.z)
        self.cols = [np.flatnonzero(self.base[r] >= 0) for r in range(self.mb)]
        # var[r][j, i]: the variable of entry j (ascending block column) of check i of layer r
        self.var = [np.stack([c * self.z + (i + self.base[r, c]) % self.z for c in self.cols[r]]) for r in range(self.mb)]
        self.degree = [len(c) for c in self.cols]
        self.edges = sum(self.degree) * self.z
        self.column_degree = np.repeat((self.base >= 0).sum(axis=0), self.z)

    def dense(self):
        H = np.zeros((self.m, self.n), dtype=np.uint8)
        for r in range(self.mb):
            for j in range(self.degree[r]):
                H[r * self.z + np.arange(self.z), self.var[r][j]] ^= 1
        return H

    def syndrome(self, hard):
        """hard: (codewords, n) 0 / 1 -> (codewords, m) parities"""
        hard = np.asarray(hard).astype(np.uint8)
        return np.concatenate([np.bitwise_xor.reduce(hard[:, v], axis=1) for v in self.var], axis=1)


def generate(mb, nb, z, seed):
    """the test codes: three random circulants per information column, a staircase of zero shifts over the parity columns"""
    rng = np.random.default_rng(seed)
    kb = nb - mb
    B = -np.ones((mb, nb), dtype=np.int64)
    for c in range(kb):
        rows = rng.choice(mb, size=min(3, mb), replace=False)
        for r in rows:
            B[r, c] = rng.integers(0, z)
    for r in range(mb):
        B[r, kb + r] = 0
        if r + 1 < mb:
            B[r + 1, kb + r] = 0
    for r in range(mb):
        if (B[r] >= 0).sum() < 2:
            c = rng.integers(0, kb)
            B[r, c] = rng.integers(0, z)
    return B.astype(np.int16)


def encode_staircase(code, data):
    """data: (codewords, k) bits -> (codewords, n): parity block r = the information sum of row r xor parity block r - 1"""
    data = np.asarray(data, dtype=np.uint8) & 1
    kb, z = code.nb - code.mb, code.z
    out = np.zeros((data.shape[0], code.n), dtype=np.uint8)
    out[:, :code.k] = data
    prev = np.zeros((data.shape[0], z), dtype=np.uint8)
    for r in range(code.mb):
        info = [j for j, c in enumerate(code.cols[r]) if c < kb]
        prev = prev ^ np.bitwise_xor.reduce(data[:, code.var[r][info]], axis=1)
        out[:, code.k + r * z:code.k + (r + 1) * z] = prev
    return out


def quantise_i8(x):
    return np.maximum(np.asarray(x, dtype=np.int8).astype(np.int32), -127)


def quantise_f32(x, scale):
    """clamp(rint(fl32(x scale)), -127, 127), NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.rint((np.asarray(x, dtype=np.float32) * np.float32(scale)).astype(np.float32))
        y = np.where(np.isnan(y), np.float32(0), np.clip(y, -127, 127))
    return y.astype(np.int32)


def normalise(x, norm, beta):
    return np.maximum(((x * norm + 8) >> 4) - beta, 0)


def pack_bits(bits):
    """(codewords, out_bits) 0 / 1 -> uint32 words, bit v in bit v mod 32 of word v / 32, the top bits zero"""
    bits = np.asarray(bits, dtype=np.uint8)
    cw, nbits = bits.shape
    words = (nbits + 31) // 32
    padded = np.zeros((cw, words * 32), dtype=np.uint64)
    padded[:, :nbits] = bits
    return (padded.reshape(cw, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def decode(code, q, max_iter, norm=12, beta=0, early_stop=True, out_bits=None, last_minimum=False, return_messages=False):
    """q: (codewords, n) quantised soft values.  Returns (bits uint8 (codewords, out_bits), post int16, status int32), and with
    return_messages the sum of the final messages into each variable.  last_minimum: call the last of tied minima "the minimum"."""
    L = np.array(q, dtype=np.int32).reshape(-1, code.n)
    cw = L.shape[0]
    z = code.z
    f1 = [np.zeros((cw, z), dtype=np.int32) for _ in range(code.mb)]
    f2 = [np.zeros((cw, z), dtype=np.int32) for _ in range(code.mb)]
    ix = [np.zeros((cw, z), dtype=np.int64) for _ in range(code.mb)]
    sg = [np.zeros((cw, d, z), dtype=bool) for d in code.degree]

    def messages(r, rows):
        j = np.arange(code.degree[r])[None, :, None]
        mag = np.where(j == ix[r][rows][:, None, :], f2[r][rows][:, None, :], f1[r][rows][:, None, :])
        return np.where(sg[r][rows], -mag, mag)

    def passes(rows):
        return ~code.syndrome(L[rows] < 0).any(axis=1)

    status = np.where(passes(np.arange(cw)), 0, -1).astype(np.int32)
    live = np.arange(cw) if not early_stop else np.flatnonzero(status != 0)
    for it in range(1, max_iter + 1):
        if live.size == 0:
            break
        for r in range(code.mb):
            V = code.var[r]
            T = L[live[:, None, None], V[None]] - messages(r, live)
            a = np.minimum(np.abs(T), 127)
            sig = T < 0
            S = np.bitwise_xor.reduce(sig, axis=1)
            d = code.degree[r]
            first = (d - 1 - np.argmin(a[:, ::-1, :], axis=1)) if last_minimum else np.argmin(a, axis=1)
            m1 = np.take_along_axis(a, first[:, None, :], axis=1)[:, 0, :]
            others = a.copy()
            np.put_along_axis(others, first[:, None, :], 255, axis=1)
            m2 = others.min(axis=1)
            f1[r][live], f2[r][live], ix[r][live] = normalise(m1, norm, beta), normalise(m2, norm, beta), first
            sg[r][live] = S[:, None, :] ^ sig
            L[live[:, None, None], V[None]] = T + messages(r, live)
        if early_stop or it == max_iter:
            ok = passes(live)
            status[live] = np.where(ok, it, -1)
            if early_stop:
                live = live[~ok]
    nbits = code.n if out_bits is None else out_bits
    res = ((L[:, :nbits] < 0).astype(np.uint8), L.astype(np.int16), status)
    if return_messages:
        total = np.zeros((cw, code.n), dtype=np.int32)
        for r in range(code.mb):
            np.add.at(total, (np.arange(cw)[:, None, None], code.var[r][None]), messages(r, np.arange(cw)))
        res += (total,)
    return res
