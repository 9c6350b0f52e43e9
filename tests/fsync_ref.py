"""The numpy form of the frame synchroniser banks' contract (include/sdsp_hip.h: sdsp_hip_fsync_*).

A stream of bits per channel, a marker of M bits in front of P payload bytes (period L = M + 8 P), a SEARCH / VERIFY / LOCK machine
with a flywheel, either polarity, and frames out packed most significant bit first, inversion and the pseudo-random sequence removed.
`FrameSync` is streaming: any split of a row into calls gives the same frames, records and state.  The distances of all positions of
a call come from one sliding-window sum; the machine then walks the hit arrays.  tests/test_fsync_host.py holds this file to a
bit-by-bit implementation of the contract's paragraphs."""
import numpy as np

SEARCH, VERIFY, LOCK = 0, 1, 2
NORMAL, EITHER = 0, 1
CCSDS_ASM = 0x1ACFFC1D


def ccsds_pn(n):
    """n bytes of the CCSDS pseudo-randomiser: a[i+8] = a[i] ^ a[i+3] ^ a[i+5] ^ a[i+7] from eight ones, first bit most significant"""
    a = [1] * 8
    while len(a) < 8 * n:
        i = len(a) - 8
        a.append(a[i] ^ a[i + 3] ^ a[i + 5] ^ a[i + 7])
    return np.packbits(np.array(a[:8 * n], dtype=np.uint8)) if n else np.zeros(0, dtype=np.uint8)


def marker_bits(marker, M):
    """the marker as it goes over the line: bit M - 1 first"""
    return np.array([(int(marker) >> (M - 1 - i)) & 1 for i in range(M)], dtype=np.uint8)


def attach(frames, marker, M, pn=None, invert=False):
    """the transmit side: (frames, P) payload bytes -> one row of frames * (M + 8 P) bits (0 / 1 bytes)"""
    frames = np.asarray(frames, dtype=np.uint8)
    frames = frames.reshape(-1, frames.shape[-1])
    body = frames if pn is None else frames ^ np.asarray(pn, dtype=np.uint8)[None, :]
    row = np.concatenate([np.broadcast_to(marker_bits(marker, M), (frames.shape[0], M)), np.unpackbits(body, axis=1)], axis=1).reshape(-1)
    return (row ^ 1) if invert else row.copy()


def max_frames(nbits, M, P):
    return -(-int(nbits) // (M + 8 * P))


def pack_words(bits):
    """rows of 0 / 1 bytes (a multiple of 32 long) -> uint32 words, the oldest bit lowest (viterbi_bank's PACKED)"""
    b = np.asarray(bits, dtype=np.uint8)
    return np.packbits(b.reshape(b.shape[0], -1, 32), axis=2, bitorder="little").view("<u4").reshape(b.shape[0], -1)


class _Row:
    def __init__(self):
        self.bits = np.zeros(0, dtype=np.uint8)
        self.d = np.zeros(0, dtype=np.int64)  # d(p) of every position examined so far
        self.mode, self.p, self.pol, self.count, self.misses = SEARCH, 0, 0, 0, 0
        self.pending = None  # (pos, info) of the frame accepted and not yet complete


class FrameSync:
    def __init__(self, marker, M, P, tol, verify, flywheel, polarity=EITHER, pn=None, channels=1):
        assert 8 <= M <= 64 and 1 <= P <= 8192 and 0 <= tol <= min(15, M // 2 - 1) and 0 <= verify <= 255 and 0 <= flywheel <= 255
        self.M, self.P, self.L, self.tol, self.V, self.F, self.either = M, P, M + 8 * P, tol, verify, flywheel, polarity == EITHER
        self.mbits = marker_bits(marker, M)
        self.pn = None if pn is None else np.asarray(pn, dtype=np.uint8).copy()
        self.rows = [_Row() for _ in range(channels)]
        self.transitions = set()

    def reset(self):
        self.rows = [_Row() for _ in self.rows]

    def state(self):
        """(mode, next position, polarity, count, misses, pending, bits seen) per channel"""
        r = self.rows
        return (np.array([x.mode for x in r], dtype=np.uint32), np.array([x.p for x in r], dtype=np.uint64),
                np.array([x.pol for x in r], dtype=np.uint32), np.array([x.count for x in r], dtype=np.uint32),
                np.array([x.misses for x in r], dtype=np.uint32), np.array([x.pending is not None for x in r], dtype=np.uint32),
                np.array([x.bits.size for x in r], dtype=np.uint64))

    def _hit(self, r, p, pol):
        d = int(r.d[p])
        return (d if pol == 0 else self.M - d) <= self.tol

    def _row(self, r, new):
        M, L, V, F = self.M, self.L, self.V, self.F
        first = r.d.size
        r.bits = np.concatenate([r.bits, (np.asarray(new) != 0).astype(np.uint8)])
        total = r.bits.size
        if total - M + 1 > first:
            w = np.lib.stride_tricks.sliding_window_view(r.bits[first:], M)
            r.d = np.concatenate([r.d, (w ^ self.mbits[None, :]).sum(axis=1, dtype=np.int64)])
        out = []

        def emit(pos, info):
            body = np.packbits(r.bits[pos + M:pos + L])
            if info & 0x100:
                body = body ^ 0xFF
            if self.pn is not None:
                body = body ^ self.pn
            out.append((pos, info, body))

        def accept(pos, fly):
            d = int(r.d[pos])
            info = (d if r.pol == 0 else M - d) | (r.pol << 8) | (int(fly) << 9)
            if pos + L <= total:
                emit(pos, info)
            else:
                r.pending = (pos, info)

        if r.pending is not None and r.pending[0] + L <= total:
            emit(*r.pending)
            r.pending = None
        T = self.transitions
        while r.p + M <= total:
            p = r.p
            if r.mode == SEARCH:
                if self._hit(r, p, 0) or (self.either and self._hit(r, p, 1)):
                    r.pol = 0 if self._hit(r, p, 0) else 1
                    r.count = r.misses = 0
                    if V == 0:
                        r.mode = LOCK
                        accept(p, False)
                        T.add("search-lock")
                    else:
                        r.mode = VERIFY
                        T.add("search-verify")
                    r.p = p + L
                else:
                    r.p = p + 1
            elif r.mode == VERIFY:
                if self._hit(r, p, r.pol):
                    r.count += 1
                    if r.count == V:
                        r.mode = LOCK
                        accept(p, False)
                        T.add("verify-lock")
                    else:
                        T.add("verify-verify")
                    r.p = p + L
                else:
                    r.mode, r.p = SEARCH, p - L + 1
                    T.add("verify-search")
            else:
                if self._hit(r, p, r.pol):
                    r.misses = 0
                    accept(p, False)
                    r.p = p + L
                    T.add("lock-hit")
                else:
                    r.misses += 1
                    if r.misses > F:
                        r.mode = SEARCH
                        T.add("lock-search")
                    else:
                        accept(p, True)
                        r.p = p + L
                        T.add("lock-flywheel")
        return out

    def process(self, bits):
        """bits: (channels, nbits), non-zero counts as 1.  Returns (out, counts, pos, info) shaped as the bank's outputs; slots at and
        beyond counts[c] are zero here and unwritten there."""
        bits = np.asarray(bits)
        ch, nbits = bits.shape
        mf = max_frames(nbits, self.M, self.P)
        out = np.zeros((ch, mf, self.P), dtype=np.uint8)
        counts = np.zeros(ch, dtype=np.uint32)
        pos = np.zeros((ch, mf), dtype=np.uint64)
        info = np.zeros((ch, mf), dtype=np.uint32)
        for c in range(ch):
            got = self._row(self.rows[c], bits[c])
            assert len(got) <= mf
            counts[c] = len(got)
            for k, (q, i, body) in enumerate(got):
                out[c, k], pos[c, k], info[c, k] = body, q, i
        return out, counts, pos, info
