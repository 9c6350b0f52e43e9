"""numpy reference of the CIC decimator bank's contract (include/sdsp_hip.h: sdsp_hip_cic_*).

Streamed, with history in and out: the integrators are np.cumsum in uint32 / uint64, which wrap, run from zero registers over the
history followed by the block; the combs are wrapped differences of the decimated sequence.  tests/test_cic_host.py pins this to a
serial Hogenauer loop in Python integers and to the big-integer FIR form.  A plain module, not a conftest."""
import numpy as np

# (N, R, M, in_bits): the shapes the identities were checked on
SHAPES = [(1, 2, 1, 16), (3, 5, 1, 16), (4, 16, 2, 16), (6, 64, 1, 16), (5, 7, 2, 32), (8, 3, 2, 16), (6, 1024, 1, 2)]


def growth(N, R, M):
    return ((R * M) ** N - 1).bit_length()


def reg_bits(in_bits, N, R, M):
    """W: 32 if in_bits + growth <= 32, else 64 (more than 64 is unsupported)"""
    return 32 if in_bits + growth(N, R, M) <= 32 else 64


def out_samples(R, position, S):
    return (position + S) // R - position // R


def unity_scale(N, R, M):
    return 1.0 / float((R * M) ** N)


def splits(R, S, extra=()):
    """call lengths 0, 1, R - 1, R + 1, 3, *extra, rest of a stream of S samples"""
    head = [0, 1, R - 1, R + 1, 3, *extra]
    assert sum(head) <= S
    return head + [S - sum(head)]


def cic_ref(x, N, R, M, W, position=0, state=None, out="int", scale=None):
    """x: (channels, S) integers, or (channels, S, 2) for interleaved I/Q; state: (channels, N M R[, 2]) of x's dtype, newest first,
    or None for zero history.  Returns (y, new_state): y (channels, n_out[, 2]) as int32 / int64 by W, or float32 for out="f32";
    new_state like state."""
    x = np.asarray(x)
    cplx = x.ndim == 3
    hist = N * M * R
    C, S = x.shape[0], x.shape[1]
    if state is None:
        state = np.zeros((C, hist) + x.shape[2:], dtype=x.dtype)
    state = np.asarray(state, dtype=x.dtype)
    assert state.shape == (C, hist) + x.shape[2:]
    xx = np.concatenate([state[:, ::-1], x], axis=1)  # oldest first: xx[:, hist + n] = x[n]
    new_state = np.ascontiguousarray(xx[:, ::-1][:, :hist])
    rows = np.moveaxis(xx, 2, 1).reshape(2 * C, hist + S) if cplx else xx
    U = np.uint32 if W == 32 else np.uint64
    v = rows.astype(np.int64).astype(U)  # sign-extended, then wrapped to W bits
    for _ in range(N):
        v = np.cumsum(v, axis=1, dtype=U)
    n = np.arange(-hist, S)
    due = np.nonzero((position % R + n) % R == R - 1)[0]
    z = v[:, due]
    for _ in range(N):
        z = z[:, M:] - z[:, :-M]  # the N M due indices inside the history feed the combs and leave no output
    n_out = out_samples(R, position, S)
    assert z.shape[1] == n_out
    y = np.ascontiguousarray(z).view(np.int32 if W == 32 else np.int64)
    if out == "f32":
        y = np.float32(y.astype(np.float64) * (unity_scale(N, R, M) if scale is None else scale))
    if cplx:
        y = np.ascontiguousarray(np.moveaxis(y.reshape(C, 2, n_out), 1, 2))
    return y, new_state


def stream_ref(x, blocks, N, R, M, W, position=0, state=None, out="int", scale=None):
    """x through cic_ref in calls of `blocks` samples with the history and position carried; (y, final state)"""
    parts, s0 = [], 0
    for b in blocks:
        y, state = cic_ref(x[:, s0:s0 + b], N, R, M, W, position, state, out, scale)
        parts.append(y)
        s0 += b
        position += b
    return np.concatenate(parts, axis=1), state


def wrap(v, W):
    """a Python integer as a W-bit two's complement value"""
    v &= (1 << W) - 1
    return v - (1 << W) if v >> (W - 1) else v


def hogenauer_serial(x, N, R, M, W, position=0):
    """the contract's serial form on a list of Python integers from zero registers: every register wrapped to W bits"""
    integ = [0] * N
    delays = [[0] * M for _ in range(N)]
    y = []
    for i, s in enumerate(x):
        v = wrap(s, W)
        for k in range(N):
            integ[k] = wrap(integ[k] + v, W)
            v = integ[k]
        if (position + i) % R == R - 1:
            for k in range(N):
                d = delays[k]
                v, old = wrap(v - d[0], W), v
                d.pop(0)
                d.append(old)
            y.append(v)
    return y


def fir_exact(x, N, R, M, position=0):
    """boxcar(R M) convolved N times, in unbounded Python integers (zeros before the stream), kept at the due indices"""
    L = R * M
    v = list(x)
    for _ in range(N):
        acc, run = [0], 0
        for s in v:
            run += s
            acc.append(run)
        v = [acc[i + 1] - acc[max(0, i + 1 - L)] for i in range(len(v))]
    return [v[i] for i in range(len(v)) if (position + i) % R == R - 1]


def taps_exact(N, R, M):
    """coefficients of boxcar(R M)^N as Python integers"""
    L = R * M
    h = [1]
    for _ in range(N):
        acc, run = [0], 0
        for s in h + [0] * (L - 1):
            run += s
            acc.append(run)
        h = [acc[i + 1] - acc[max(0, i + 1 - L)] for i in range(len(h) + L - 1)]
    return h
