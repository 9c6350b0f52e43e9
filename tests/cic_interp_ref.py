"""numpy reference of the CIC interpolator bank's contract (include/sdsp_hip.h: sdsp_hip_cic_interp_*).

Streamed, with history in and out: the combs are wrapped differences over the history (N M inputs, itself preceded by zeros: the
cascade started from zero registers N M inputs early) followed by the block, the zero-stuffed sequence goes through N np.cumsum in
uint32 / uint64, which wrap, and the first N M R outputs, the history's, are dropped.  tests/test_cic_interp_host.py pins this to a
serial Hogenauer loop in Python integers and to the big-integer polyphase FIR form.  A plain module, not a conftest."""
import numpy as np

from cic_ref import taps_exact, wrap  # noqa: F401  (wrap is re-exported for the tests)

# (N, R, M, in_bits): the shapes the identities were checked on
SHAPES = [(1, 2, 1, 16), (3, 5, 1, 16), (4, 16, 2, 16), (6, 64, 1, 16), (5, 7, 2, 32), (8, 3, 2, 16), (2, 1024, 1, 16), (8, 2, 1, 16),
          (3, 3, 2, 16)]


def gain(N, R, M):
    """the sum of every polyphase branch of boxcar(R M)^N: the gain at DC"""
    return R ** (N - 1) * M ** N


def growth(N, R, M):
    return (gain(N, R, M) - 1).bit_length()


def reg_bits(in_bits, N, R, M):
    """W: 32 if in_bits + growth <= 32, else 64 (more than 64 is unsupported)"""
    return 32 if in_bits + growth(N, R, M) <= 32 else 64


def unity_scale(N, R, M):
    return 1.0 / float(gain(N, R, M))


def splits(N, M, S):
    """call lengths 0, 1, 2, N M - 1, N M + 1, rest of a stream of S samples"""
    head = [0, 1, 2, N * M - 1, N * M + 1]
    assert sum(head) <= S
    return head + [S - sum(head)]


def cic_interp_ref(x, N, R, M, W, state=None, out="int", scale=None):
    """x: (channels, S) integers, or (channels, S, 2) for interleaved I/Q; state: (channels, N M[, 2]) of x's dtype, newest first, or
    None for zero history.  Returns (y, new_state): y (channels, R S[, 2]) as int32 / int64 by W, or float32 for out="f32"; new_state
    like state."""
    x = np.asarray(x)
    cplx = x.ndim == 3
    hist = N * M
    C, S = x.shape[0], x.shape[1]
    if state is None:
        state = np.zeros((C, hist) + x.shape[2:], dtype=x.dtype)
    state = np.asarray(state, dtype=x.dtype)
    assert state.shape == (C, hist) + x.shape[2:]
    xx = np.concatenate([state[:, ::-1], x], axis=1)  # oldest first: xx[:, hist + m] = x[m]
    new_state = np.ascontiguousarray(xx[:, ::-1][:, :hist])
    rows = np.moveaxis(xx, 2, 1).reshape(2 * C, hist + S) if cplx else xx
    U = np.uint32 if W == 32 else np.uint64
    v = rows.astype(np.int64).astype(U)  # sign-extended, then wrapped to W bits
    for _ in range(N):  # combs from zero registers at the start of the history
        d = v.copy()
        d[:, M:] -= v[:, :-M]
        v = d
    u = np.zeros((v.shape[0], (hist + S) * R), dtype=U)
    u[:, ::R] = v
    for _ in range(N):
        u = np.cumsum(u, axis=1, dtype=U)
    y = np.ascontiguousarray(u[:, hist * R:]).view(np.int32 if W == 32 else np.int64)
    if out == "f32":
        y = np.float32(y.astype(np.float64) * (unity_scale(N, R, M) if scale is None else scale))
    if cplx:
        y = np.ascontiguousarray(np.moveaxis(y.reshape(C, 2, R * S), 1, 2))
    return y, new_state


def stream_ref(x, blocks, N, R, M, W, state=None, out="int", scale=None):
    """x through cic_interp_ref in calls of `blocks` samples with the history carried; (y, final state)"""
    parts, s0 = [], 0
    for b in blocks:
        y, state = cic_interp_ref(x[:, s0:s0 + b], N, R, M, W, state, out, scale)
        parts.append(y)
        s0 += b
    return np.concatenate(parts, axis=1), state


def hogenauer_serial(x, N, R, M, W):
    """the contract's serial form on a list of Python integers from zero registers: every register wrapped to W bits"""
    delays = [[0] * M for _ in range(N)]
    integ = [0] * N
    y = []
    for s in x:
        v = wrap(s, W)
        for k in range(N):
            d = delays[k]
            v, old = wrap(v - d[0], W), v
            d.pop(0)
            d.append(old)
        for p in range(R):
            u = v if p == 0 else 0
            for k in range(N):
                integ[k] = wrap(integ[k] + u, W)
                u = integ[k]
            y.append(u)
    return y


def fir_exact(x, N, R, M):
    """y[m R + p] = sum_j h[p + j R] x[m - j] with h = boxcar(R M)^N, in unbounded Python integers (zeros before the stream)"""
    h = taps_exact(N, R, M)
    y = []
    for m in range(len(x)):
        for p in range(R):
            y.append(sum(h[k] * x[m - j] for j, k in enumerate(range(p, len(h), R)) if m - j >= 0))
    return y
