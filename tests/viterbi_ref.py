"""numpy reference of the streaming Viterbi decoder banks (include/sdsp_hip.h: sdsp_hip_viterbi_*), written
from the contract: vectorised over channels and states, a Python loop over steps.  Metrics are int64 and reduced to 32-bit two's
complement where the contract compares or stores them.  A helper, not a test file."""
import numpy as np

START_METRIC = -(1 << 20)


def wrap32(v):
    """int64 values reduced to 32-bit two's complement (still int64)"""
    return ((np.asarray(v, dtype=np.int64) + (1 << 31)) & 0xffffffff) - (1 << 31)


def delay(block, depth):
    return block * -(-depth // block)


def quantise(x, in_kind="i8", scale=1.0):
    """the soft values as the integers the decoder works on"""
    if in_kind == "i8":
        return np.maximum(np.asarray(x, dtype=np.int8).astype(np.int64), -127)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.rint(np.asarray(x, dtype=np.float32) * np.float32(scale))  # one float32 product, ties to even
        y = np.where(np.isnan(y), np.float32(0), np.clip(y, np.float32(-127), np.float32(127)))
    return y.astype(np.int64)


def coded_bits(k, generators, reg):
    """the n coded bits of the register `reg` (the input of i steps ago in bit i): generator bit k - 1 multiplies the newest input"""
    out = []
    for g in generators:
        c = 0
        for i in range(k):
            c ^= ((g >> (k - 1 - i)) & 1) & ((reg >> i) & 1)
        out.append(c)
    return out


def encode(bits, k, generators, terminate=False):
    """the shift-register encoder from state 0: n coded bits per input bit"""
    reg, out = 0, []
    for b in list(bits) + [0] * ((k - 1) if terminate else 0):
        reg = ((reg << 1) | (1 if b else 0)) & ((1 << k) - 1)
        out += coded_bits(k, generators, reg)
    return np.array(out, dtype=np.uint8)


def pack_bits(bits):
    """(channels, steps) 0 / 1 -> (channels, steps / 32) uint32 words, least significant bit first"""
    b = np.asarray(bits, dtype=np.uint64).reshape(bits.shape[0], -1, 32)
    return (b << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


class ViterbiRef:
    def __init__(self, k, generators, block, depth, channels, start_state=-1, in_kind="i8", scale=1.0):
        self.k, self.gens, self.n, self.B, self.D = k, list(generators), len(generators), block, depth
        self.S = 1 << (k - 1)
        self.Dr = delay(block, depth)
        self.channels, self.in_kind, self.scale = channels, in_kind, scale
        s = np.arange(self.S)
        self.p0, self.p1 = s >> 1, (s >> 1) + self.S // 2
        # the signs of the branch metrics: +1 where the coded bit is 0
        self.sg0 = np.array([[1 - 2 * c for c in coded_bits(k, self.gens, (int(p) << 1) | (int(t) & 1))] for t, p in zip(s, self.p0)], dtype=np.int64)
        self.sg1 = np.array([[1 - 2 * c for c in coded_bits(k, self.gens, (int(p) << 1) | (int(t) & 1))] for t, p in zip(s, self.p1)], dtype=np.int64)
        self.reset(start_state)

    def reset(self, start_state=-1):
        self.m = np.zeros((self.channels, self.S), dtype=np.int64)
        if start_state >= 0:
            self.m[:] = START_METRIC
            self.m[:, start_state] = 0
        self.pos = 0  # steps of the stream so far
        self.dec = np.zeros((self.channels, self.Dr, self.S), dtype=np.uint8)  # the decisions of the last Dr steps, oldest first

    def metrics(self):
        return wrap32(self.m).astype(np.int32)

    def set_metrics(self, m):
        self.m = np.asarray(m).astype(np.int64).reshape(self.channels, self.S).copy()

    def process(self, soft):
        """soft: (channels, steps n); returns (channels, steps) uint8: out[t] = the bit of stream step pos + t - Dr"""
        n, B, D, Dr, S = self.n, self.B, self.D, self.Dr, self.S
        q = quantise(soft, self.in_kind, self.scale).reshape(self.channels, -1, n)
        steps = q.shape[1]
        assert steps % B == 0
        out = np.zeros((self.channels, steps), dtype=np.uint8)
        dec = np.concatenate([self.dec, np.zeros((self.channels, steps, S), dtype=np.uint8)], axis=1)  # steps pos - Dr .. pos + steps
        rows = np.arange(self.channels)
        m = self.m
        for t in range(steps):
            g = self.pos + t
            a0 = m[:, self.p0] + q[:, t, :] @ self.sg0.T
            a1 = m[:, self.p1] + q[:, t, :] @ self.sg1.T
            d = wrap32(a1 - a0) > 0
            m = wrap32(np.where(d, a1, a0))
            dec[:, Dr + t] = d
            first = g - D + 1 - B  # the first step of the block that this step decides
            if first >= 0 and first % B == 0:
                s = np.argmax(wrap32(m - m[:, :1]), axis=1)  # the lowest state of the largest difference
                for u in range(g, first - 1, -1):
                    if u < first + B:
                        out[:, u + Dr - self.pos] = s & 1
                    s = (s >> 1) + dec[rows, u - (self.pos - Dr), s].astype(np.int64) * (S // 2)
        self.m = m
        self.pos += steps
        self.dec = dec[:, -Dr:].copy()
        return out
