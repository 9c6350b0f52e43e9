"""Double-precision reference of the forward-backward filtering plans (include/sdsp_hip.h: sdsp_hip_filtfilt_*, DESIGN.md section
5.13), vectorised over channels: the steady state, the edge extension and the two Direct-Form-I passes of the header's five steps.
tests/test_filtfilt_host.py pins it to scipy.signal.sosfiltfilt."""
import numpy as np
import scipy.signal

GENERIC, LP, HP, BP = 0, 1, 2, 3
PAD_NONE, PAD_ODD, PAD_EVEN, PAD_CONSTANT = 0, 1, 2, 3
PADTYPES = {"odd": PAD_ODD, "even": PAD_EVEN, "constant": PAD_CONSTANT, None: PAD_NONE}
FOLDED = {LP: (2.0, 1.0), HP: (-2.0, 1.0), BP: (0.0, -1.0)}


def numerators(kind, a, b):
    """(b1, b2) per section as the kind's process body uses them"""
    m = len(a) // 3
    if kind == GENERIC:
        b = np.asarray(b, dtype=np.float64).reshape(m, 3)
        return b[:, 1].copy(), b[:, 2].copy()
    b1, b2 = FOLDED[kind]
    return np.full(m, b1), np.full(m, b2)


def steady_state_ref(kind, a, b, gain):
    """s_0 = gain, s_{j+1} = s_j (1 + b1 + b2) / (1 + a1 + a2)"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b1, b2 = numerators(kind, a.reshape(-1), b)
    s = [float(gain)]
    for j in range(a.shape[0]):
        s.append(s[-1] * (1.0 + b1[j] + b2[j]) / (1.0 + a[j, 1] + a[j, 2]))
    return np.array(s)


def default_padlen_ref(kind, a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    m = a.shape[0]
    _, b2 = numerators(kind, a.reshape(-1), b)
    return 3 * (2 * m + 1 - min(int((b2 == 0).sum()), int((a[:, 2] == 0).sum())))


def sos_of(kind, a, b, gain):
    """scipy's second-order sections of the cascade: rows [1, b1, b2, 1, a1, a2], gain folded into the first row"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b1, b2 = numerators(kind, a.reshape(-1), b)
    sos = np.zeros((a.shape[0], 6))
    sos[:, 0], sos[:, 1], sos[:, 2] = 1.0, b1, b2
    sos[:, 3], sos[:, 4], sos[:, 5] = 1.0, a[:, 1], a[:, 2]
    sos[0, :3] *= gain
    return sos


def extend(x, padtype, P):
    """the extension e of L + 2P samples per row"""
    if padtype == PAD_NONE or P == 0:
        return x.copy()
    x0, xl = x[:, :1], x[:, -1:]
    left_m = x[:, P:0:-1]           # x[P - i], i < P
    right_m = x[:, -2:-2 - P:-1]    # x[L - 2 - i], i < P
    if padtype == PAD_ODD:
        left, right = 2 * x0 - left_m, 2 * xl - right_m
    elif padtype == PAD_EVEN:
        left, right = left_m, right_m
    else:
        left, right = np.repeat(x0, P, axis=1), np.repeat(xl, P, axis=1)
    return np.concatenate([left, x, right], axis=1)


def cascade(e, kind, a, b, gain, s):
    """Direct-Form-I cascade over the rows of e, every age of level j starting at s_j e[:, 0]"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b1, b2 = numerators(kind, a.reshape(-1), b)
    v = e[:, :1]
    cur = e * gain
    for j in range(a.shape[0]):
        xin, yin = s[j] * v, s[j + 1] * v  # the section's input and output histories
        fir = cur + b1[j] * np.concatenate([xin, cur[:, :-1]], axis=1) + b2[j] * np.concatenate([xin, xin, cur[:, :-2]], axis=1)[:, :cur.shape[1]]
        ar = [1.0, a[j, 1], a[j, 2]]
        zi = np.stack([scipy.signal.lfiltic([1.0], ar, [yin[c, 0], yin[c, 0]]) for c in range(e.shape[0])])
        cur, _ = scipy.signal.lfilter([1.0], ar, fir, axis=1, zi=zi)
    return cur


def filtfilt_ref(x, kind, a, b, gain, padtype=PAD_ODD, padlen=None):
    """the plan's result in double for rows x (channels, L)"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    L = x.shape[1]
    P = 0 if padtype == PAD_NONE else (default_padlen_ref(kind, a, b) if padlen is None else padlen)
    if L <= P:
        raise ValueError("L must exceed padlen")
    s = steady_state_ref(kind, a, b, gain)
    e = extend(x, padtype, P)
    u = cascade(e, kind, a, b, gain, s)
    w = cascade(u[:, ::-1].copy(), kind, a, b, gain, s)[:, ::-1]
    return w[:, P:P + L]


def random_stable(rng, m):
    """a random stable GENERIC cascade: poles inside radius 0.95, arbitrary real zeros, 1 + a1 + a2 != 0"""
    a = np.zeros((m, 3))
    b = np.zeros((m, 3))
    for j in range(m):
        r, th = rng.uniform(0.2, 0.95), rng.uniform(0.05, np.pi - 0.05)
        a[j] = [1.0, -2 * r * np.cos(th), r * r]
        b[j] = [1.0, rng.uniform(-1.5, 1.5), rng.uniform(-0.9, 0.9)]
    return a.reshape(-1), b.reshape(-1), float(rng.uniform(0.5, 2.0))
