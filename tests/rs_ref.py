"""numpy reference of the Reed-Solomon decoder banks over GF(256) (include/sdsp_hip.h: sdsp_hip_rs_*), written
from the contract.

Field: GF(2^8) by `field_poly` (9 bits, bit 8 set), alpha = 0x02, which must have order 255.  Code: g(x) = prod_{j < nroots}
(x - alpha^(prim (fcr + j))), 0 <= fcr < 255, gcd(prim, 255) = 1, 2 <= nroots <= 64, nroots < n <= 255, k = n - nroots; symbol i of a
codeword is the coefficient of x^(n-1-i), data first, parity last.  Frame: `interleave` = I codewords, byte s I + j is symbol s of
codeword j.  Erasures: the same layout, non-zero marks an erased symbol.  Result of a received word r with erased set E: a failure if
|E| > nroots; else the one codeword c with 2 |{i not in E: c_i != r_i}| + |E| <= nroots, corrected = |{i: c_i != r_i}|; a failure if
there is none.  A failure leaves the symbols as received, corrected = -1.

The decoder here is errors-and-erasures Berlekamp-Massey, a root search, Forney's values, and then the contract itself as the last
word: the corrected word must have zero syndromes and lie within the bound.  brute_force() is the definition taken literally, for
codes of 65536 codewords.  A helper, not a test file."""
import math

import numpy as np

MAX_NROOTS = 64
MAX_INTERLEAVE = 16


def field_tables(field_poly):
    """(exp, log): exp[i] = alpha^i for i < 510 (twice round, so that a sum of two logs needs no reduction), log[exp[i]] = i.
    None if field_poly is no 9-bit polynomial under which alpha = 2 has order 255."""
    if not (0x100 <= field_poly < 0x200):
        return None
    exp = np.zeros(512, dtype=np.uint8)
    log = np.zeros(256, dtype=np.int64)
    x = 1
    for i in range(255):
        if i and x == 1:
            return None
        exp[i] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= field_poly
    if x != 1:
        return None
    exp[255:510] = exp[:255]
    return exp, log


class Code:
    def __init__(self, field_poly, fcr, prim, nroots, n=255):
        t = field_tables(field_poly)
        if t is None:
            raise ValueError("alpha = 2 does not have order 255 under this polynomial")
        if not (0 <= fcr < 255) or not (1 <= prim < 255) or math.gcd(prim, 255) != 1:
            raise ValueError("fcr must be in [0, 255) and gcd(prim, 255) = 1")
        if not (2 <= nroots <= MAX_NROOTS) or not (nroots < n <= 255):
            raise ValueError("2 <= nroots <= 64 and nroots < n <= 255")
        self.exp, self.log = t
        self.field_poly, self.fcr, self.prim, self.nroots, self.n, self.k = field_poly, fcr, prim, nroots, n, n - nroots
        self.t = nroots // 2
        self.power = np.arange(n - 1, -1, -1, dtype=np.int64)  # symbol i multiplies x^(n-1-i)
        self.xlog = (prim * self.power) % 255                   # log of the locator X_i = alpha^(prim (n-1-i))
        self.roots = [(prim * (fcr + j)) % 255 for j in range(nroots)]

    # ---- field
    def mul(self, a, b):
        a = np.asarray(a, dtype=np.int64)
        b = np.asarray(b, dtype=np.int64)
        return np.where((a != 0) & (b != 0), self.exp[self.log[a] + self.log[b]], 0).astype(np.uint8)

    def _m(self, a, b):
        return int(self.exp[self.log[a] + self.log[b]]) if a and b else 0

    def _inv(self, a):
        return int(self.exp[(255 - self.log[a]) % 255])

    # ---- code
    def generator(self):
        """the nroots + 1 coefficients of g, highest first"""
        g = [1]
        for r in self.roots:
            a = int(self.exp[r])
            g = [x ^ self._m(y, a) for x, y in zip(g + [0], [0] + g)]
        return np.array(g, dtype=np.uint8)

    def encode(self, data):
        """(..., k) data symbols -> (..., n) codewords: data, then the remainder of data(x) x^nroots by g"""
        d = np.asarray(data, dtype=np.uint8)
        assert d.shape[-1] == self.k
        g = self.generator()[1:]
        par = np.zeros(d.shape[:-1] + (self.nroots,), dtype=np.uint8)
        for s in range(self.k):
            fb = d[..., s] ^ par[..., 0]
            par = np.concatenate([par[..., 1:], np.zeros_like(par[..., :1])], axis=-1) ^ self.mul(fb[..., None], g)
        return np.concatenate([d, par], axis=-1)

    def syndromes(self, words):
        """(N, n) words -> (N, nroots): S_j = r(alpha^(prim (fcr + j)))"""
        w = np.asarray(words, dtype=np.int64)
        lg = self.log[w]
        out = np.zeros((w.shape[0], self.nroots), dtype=np.uint8)
        for j, r in enumerate(self.roots):
            term = np.where(w != 0, self.exp[(lg + r * self.power) % 255], 0).astype(np.uint8)
            out[:, j] = np.bitwise_xor.reduce(term, axis=1)
        return out

    def decode_word(self, r, erased, syn=None):
        """one received word (n,) uint8 and its erasure flags (n,) bool -> (word, corrected)"""
        n, nroots = self.n, self.nroots
        r = np.asarray(r, dtype=np.uint8)
        E = [int(i) for i in np.flatnonzero(erased)]
        if len(E) > nroots:
            return r.copy(), -1
        S = [int(v) for v in (self.syndromes(r[None])[0] if syn is None else syn)]
        if not any(S):
            return r.copy(), 0
        # the erasure locator, then Berlekamp-Massey on top of it; lam[c] is the coefficient of x^c
        lam = [1] + [0] * nroots
        for i in E:
            x = int(self.exp[self.xlog[i]])
            lam = [lam[0]] + [lam[c] ^ self._m(x, lam[c - 1]) for c in range(1, nroots + 1)]
        b = list(lam)
        el = ne = len(E)
        for step in range(ne + 1, nroots + 1):
            d = 0
            for c in range(step):
                d ^= self._m(lam[c], S[step - 1 - c])
            xb = [0] + b[:-1]
            if d == 0:
                b = xb
            else:
                t = [lam[c] ^ self._m(d, xb[c]) for c in range(nroots + 1)]
                if 2 * el <= step + ne - 1:
                    el = step + ne - el
                    di = self._inv(d)
                    b = [self._m(v, di) for v in lam]
                else:
                    b = xb
                lam = t
        deg = max(c for c in range(nroots + 1) if lam[c])
        if deg == 0:
            return r.copy(), -1
        # roots among the n positions: lam(X_i^-1) = 0; den = z lam'(z), the odd terms
        zlog = (255 - self.xlog) % 255
        val = np.zeros(n, dtype=np.uint8)
        den = np.zeros(n, dtype=np.uint8)
        for c in range(deg + 1):
            if lam[c]:
                term = self.exp[(int(self.log[lam[c]]) + c * zlog) % 255]
                val ^= term
                if c & 1:
                    den ^= term
        pos = np.flatnonzero(val == 0)
        if len(pos) != deg or np.any(den[pos] == 0):
            return r.copy(), -1
        omega = [0] * nroots
        for m in range(nroots):
            for c in range(min(m, deg) + 1):
                omega[m] ^= self._m(lam[c], S[m - c])
        out = r.copy()
        for i in pos:
            z = int(zlog[i])
            num = 0
            for m in range(nroots):
                if omega[m]:
                    num ^= int(self.exp[(int(self.log[omega[m]]) + m * z) % 255])
            if num:
                # e_i = X_i^(1 - fcr) omega(z) / lam'(z) = X_i^(-fcr) omega(z) / (z lam'(z))
                out[i] ^= self.exp[(int(self.log[num]) + 255 - int(self.log[den[i]]) + int(self.fcr * zlog[i])) % 255]
        # the contract as the last word
        if self.syndromes(out[None]).any():
            return r.copy(), -1
        diff = out != r
        outside = int(np.count_nonzero(diff & ~np.asarray(erased, dtype=bool)))
        if 2 * outside + len(E) > nroots:
            return r.copy(), -1
        return out, int(np.count_nonzero(diff))

    def decode_words(self, words, erased=None):
        """(N, n) words -> ((N, n) out, (N,) corrected int32); clean words cost their syndromes only"""
        w = np.ascontiguousarray(words, dtype=np.uint8)
        e = np.zeros(w.shape, dtype=bool) if erased is None else np.asarray(erased) != 0
        out = w.copy()
        corrected = np.zeros(w.shape[0], dtype=np.int32)
        syn = self.syndromes(w)
        corrected[e.sum(axis=1) > self.nroots] = -1
        for i in np.flatnonzero(syn.any(axis=1) & (corrected == 0)):
            out[i], corrected[i] = self.decode_word(w[i], e[i], syn[i])
        return out, corrected

    def brute_force(self, r, erased):
        """the definition taken literally over every codeword (k = 2 only)"""
        assert self.k == 2
        if not hasattr(self, "_all"):
            a = np.arange(256, dtype=np.uint8)
            self._all = self.encode(np.stack(np.meshgrid(a, a, indexing="ij"), axis=-1).reshape(-1, 2))
        e = np.asarray(erased, dtype=bool)
        if e.sum() > self.nroots:
            return np.array(r, dtype=np.uint8), -1
        diff = self._all != np.asarray(r, dtype=np.uint8)[None]
        ok = np.flatnonzero(2 * (diff & ~e[None]).sum(axis=1) + e.sum() <= self.nroots)
        assert len(ok) <= 1
        if len(ok) == 0:
            return np.array(r, dtype=np.uint8), -1
        return self._all[ok[0]].copy(), int(diff[ok[0]].sum())


# ---- frames
def to_words(frames, n, interleave):
    """(F, I n) frame bytes -> (F I, n) codewords, codeword f I + j"""
    f = np.asarray(frames)
    return np.ascontiguousarray(f.reshape(f.shape[0], n, interleave).transpose(0, 2, 1)).reshape(-1, n)


def to_frames(words, interleave):
    """(F I, n) codewords -> (F, I n) frame bytes"""
    w = np.asarray(words)
    n = w.shape[1]
    return np.ascontiguousarray(w.reshape(-1, interleave, n).transpose(0, 2, 1)).reshape(-1, interleave * n)


def encode_frames(code, data, interleave=1):
    """(F, I k) data bytes -> (F, I n) frames"""
    d = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, interleave * code.k)
    return to_frames(code.encode(to_words(d, code.k, interleave)), interleave)


def decode_frames(code, frames, erasures=None, interleave=1, out_kind="full"):
    """(F, I n) frames (and erasure flags) -> (out, corrected): out (F, I n) or, for "data", (F, I k); corrected (F I,) int32"""
    f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, interleave * code.n)
    e = None if erasures is None else to_words(np.asarray(erasures).reshape(f.shape), code.n, interleave)
    words, corrected = code.decode_words(to_words(f, code.n, interleave), e)
    out = to_frames(words, interleave)
    if out_kind == "data":
        out = np.ascontiguousarray(out[:, :interleave * code.k])
    return out, corrected
