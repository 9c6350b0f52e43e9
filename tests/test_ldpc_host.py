"""Host side of the LDPC decoder banks (sdsp_hip_ldpc_*), no device: the numpy reference
(tests/ldpc_ref.py) against a second reading of the contract written edge by edge, against floating-point layered min-sum where the
two must agree exactly, the invariants of the contract, the library's host helpers against the reference, the refusals of plan
creation, whose argument checks come before the device is touched, and what the reference decodes at 4 dB."""
import ctypes as C

import numpy as np
import pytest

import ldpc_ref as R

INVALID_SIZE, UNSUPPORTED, NO_DEVICE, INVALID_ARG = -1, -2, -4, -5
SMALL = [(3, 6, 2, 3), (3, 6, 5, 4), (2, 5, 7, 5)]  # mb, nb, z, seed


def _lib():
    import simpledsp_amd._lib as L
    return L, L.load()


def _inputs(rng, cw, n, amp=40):
    """random int8 soft values with zeros, the rails and -128 among them"""
    q = np.clip(np.rint(rng.standard_normal((cw, n)) * amp), -128, 127).astype(np.int8)
    special = rng.random((cw, n))
    q[special < 0.05] = 0
    q[(special >= 0.05) & (special < 0.08)] = 127
    q[(special >= 0.08) & (special < 0.11)] = -127
    q[(special >= 0.11) & (special < 0.14)] = -128
    return q


def literal_decode(H, z, q, max_iter, norm, beta, early_stop):
    """one codeword, the contract read edge by edge over a dense H: a Python loop per check, one explicit message per edge"""
    m, n = H.shape
    L = [int(x) for x in q]
    rows = [[int(v) for v in np.flatnonzero(H[c])] for c in range(m)]  # ascending variable = ascending block column
    msg = {(c, v): 0 for c in range(m) for v in rows[c]}

    def passes():
        return all(sum(L[v] < 0 for v in rows[c]) % 2 == 0 for c in range(m))

    status = 0 if passes() else -1
    it = 0
    while it < max_iter and not (early_stop and status >= 0):
        it += 1
        for c in range(m):  # the checks of layer c // z, in any order
            T = [L[v] - msg[c, v] for v in rows[c]]
            a = [min(abs(t), 127) for t in T]
            S = sum(t < 0 for t in T) % 2
            for j, v in enumerate(rows[c]):
                least_of_others = min(a[:j] + a[j + 1:])
                mag = max(((least_of_others * norm + 8) >> 4) - beta, 0)
                new = -mag if S ^ (T[j] < 0) else mag
                msg[c, v] = new
                L[v] = T[j] + new
        if early_stop or it == max_iter:
            status = it if passes() else -1
    return np.array([x < 0 for x in L], dtype=np.uint8), np.array(L, dtype=np.int16), status


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("max_iter", [0, 1, 7])
def test_reference_equals_the_contract_read_edge_by_edge(shape, early, max_iter):
    mb, nb, z, seed = shape
    code = R.Code(R.generate(mb, nb, z, seed), z)
    H = code.dense()
    rng = np.random.default_rng(100 * seed + max_iter)
    raw = _inputs(rng, 24, code.n)
    raw[0] = 0
    raw[1, :4] = [-128, 127, -127, 0]
    raw[2] = 90 * (1 - 2 * R.encode_staircase(code, rng.integers(0, 2, (1, code.k)))[0])  # a clean codeword
    q = R.quantise_i8(raw)
    for norm, beta in [(12, 0), (16, 1)]:
        bits, post, status = R.decode(code, q, max_iter, norm, beta, early)
        for c in range(q.shape[0]):
            wb, wp, ws = literal_decode(H, z, q[c], max_iter, norm, beta, early)
            assert ws == status[c] and np.array_equal(wp, post[c]) and np.array_equal(wb, bits[c]), (c, ws, status[c])
        if max_iter == 7 and early:
            assert len(set(status.tolist())) >= 3, status  # immediate passes, late passes and failures were all among the draws


def float_min_sum(H, q, iters):
    """layered min-sum in floating point over a dense H: every quantity is a small integer, so it is exact"""
    m, n = H.shape
    L = q.astype(np.float64)
    msg = np.zeros((m, n))
    for _ in range(iters):
        for c in range(m):
            vs = np.flatnonzero(H[c])
            T = L[vs] - msg[c, vs]
            sgn = np.where(T < 0, -1.0, 1.0)
            for j, v in enumerate(vs):
                others = np.delete(np.arange(len(vs)), j)
                msg[c, v] = np.prod(sgn[others]) * np.abs(T[others]).min()
            L[vs] = T + msg[c, vs]
    return L


@pytest.mark.parametrize("shape", SMALL)
def test_plain_min_sum_equals_floating_point_where_nothing_saturates(shape):
    mb, nb, z, seed = shape
    code = R.Code(R.generate(mb, nb, z, seed), z)
    q = np.random.default_rng(seed).integers(-6, 7, (12, code.n))
    _, post, _ = R.decode(code, q, 4, norm=16, beta=0, early_stop=False)
    assert np.abs(post).max() < 127
    for c in range(q.shape[0]):
        assert np.array_equal(float_min_sum(code.dense(), q[c], 4), post[c].astype(np.float64))


@pytest.mark.parametrize("shape", SMALL + [(4, 24, 21, 6)])
def test_invariants_of_the_contract(shape):
    mb, nb, z, seed = shape
    code = R.Code(R.generate(mb, nb, z, seed), z)
    rng = np.random.default_rng(seed)
    q = R.quantise_i8(_inputs(rng, 40, code.n, amp=90))
    for norm, beta in [(12, 0), (16, 0), (16, 3), (1, 0)]:
        bits, post, status, total = R.decode(code, q, 6, norm, beta, early_stop=False, return_messages=True)
        assert np.array_equal(post.astype(np.int32) - q, total)  # the posterior is the input plus the messages into the variable
        assert (np.abs(post.astype(np.int32)) <= 127 * (1 + code.column_degree)).all()
        other = R.decode(code, q, 6, norm, beta, early_stop=False, last_minimum=True)
        assert all(np.array_equal(x, y) for x, y in zip((bits, post, status), other))  # which tied minimum is "the first"
    words = R.encode_staircase(code, rng.integers(0, 2, (8, code.k)))
    assert not code.syndrome(words).any()
    for amp in (1, 9, 127):
        clean = amp * (1 - 2 * words.astype(np.int32))
        bits, _, status = R.decode(code, clean, 5, early_stop=True)
        assert not status.any() and np.array_equal(bits, words)
        bits, _, status = R.decode(code, clean, 5, early_stop=False)
        assert (status == 5).all() and np.array_equal(bits, words)


def test_quantisers_and_packing():
    x = np.array([0.4, 0.5, 1.5, -0.5, -2.5, 1e9, -1e9, np.inf, -np.inf, np.nan, 15.9], dtype=np.float32)
    assert list(R.quantise_f32(x, 8.0)) == [3, 4, 12, -4, -20, 127, -127, 127, -127, 0, 127]
    assert list(R.quantise_i8(np.array([-128, -127, 0, 127], dtype=np.int8))) == [-127, -127, 0, 127]
    bits = np.zeros((1, 40), dtype=np.uint8)
    bits[0, [0, 31, 32, 39]] = 1
    assert list(R.pack_bits(bits)[0]) == [0x80000001, 0x81]


CODES = [(3, 6, 2, 3), (2, 5, 7, 5), (12, 24, 27, 1), (4, 24, 81, 2)]


@pytest.mark.parametrize("shape", CODES)
def test_library_encoder_and_parity_matrix(shape):
    import simpledsp_amd as sd
    mb, nb, z, seed = shape
    base = R.generate(mb, nb, z, seed)
    code = R.Code(base, z)
    data = np.random.default_rng(seed).integers(0, 2, (5, code.k), dtype=np.uint8)
    words = sd.ldpc_encode(data, base, z)
    assert words.dtype == np.uint8 and words.shape == (5, code.n) and np.array_equal(words[:, :code.k], data)
    assert not code.syndrome(words).any()
    assert np.array_equal(words, R.encode_staircase(code, data))
    P = sd.ldpc_parity_matrix(base, z)
    assert P.shape == (code.m, (code.k + 31) // 32) and P.dtype == np.uint32
    Pbits = ((P[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(code.m, -1)[:, :code.k]
    assert np.array_equal((Pbits.astype(np.int64) @ data.T.astype(np.int64) % 2).T, words[:, code.k:])
    assert sd.ldpc_encode(np.zeros(0, dtype=np.uint8), base, z).shape == (0, code.n)


def test_singular_parity_part_and_helper_refusals_write_nothing():
    L, lib = _lib()
    singular = np.array([[0, 1, 0, 0], [1, 0, 0, 0]], dtype=np.int16)  # the two parity columns are equal
    P = np.full((4, 1), 7, dtype=np.uint32)
    d = np.ones(4, dtype=np.uint8)
    o = np.full(8, 7, dtype=np.uint8)
    assert lib.sdsp_hip_ldpc_parity_matrix(singular.ctypes.data, 2, 4, 2, P.ctypes.data) == UNSUPPORTED
    assert lib.sdsp_hip_ldpc_encode(singular.ctypes.data, 2, 4, 2, d.ctypes.data, 1, o.ctypes.data) == UNSUPPORTED
    good = R.generate(2, 4, 2, 1)
    assert lib.sdsp_hip_ldpc_parity_matrix(good.ctypes.data, 2, 4, 2, None) == INVALID_ARG
    assert lib.sdsp_hip_ldpc_parity_matrix(None, 2, 4, 2, P.ctypes.data) == INVALID_ARG
    assert lib.sdsp_hip_ldpc_parity_matrix(good.ctypes.data, 2, 4, 1, P.ctypes.data) == INVALID_SIZE
    assert lib.sdsp_hip_ldpc_encode(good.ctypes.data, 2, 4, 2, d.ctypes.data, 1, None) == INVALID_ARG
    assert lib.sdsp_hip_ldpc_encode(good.ctypes.data, 2, 4, 2, None, 1, o.ctypes.data) == INVALID_ARG
    assert lib.sdsp_hip_ldpc_encode(good.ctypes.data, 2, 4, 2, d.ctypes.data, 1 << 31, o.ctypes.data) == INVALID_SIZE
    assert lib.sdsp_hip_ldpc_encode(good.ctypes.data, 2, 4, 2, o.ctypes.data, 1, o.ctypes.data + 2) == INVALID_ARG  # overlap
    bad = good.copy()
    bad[0, 0] = 2
    assert lib.sdsp_hip_ldpc_encode(bad.ctypes.data, 2, 4, 2, d.ctypes.data, 1, o.ctypes.data) == INVALID_ARG
    assert (P == 7).all() and (o == 7).all() and lib.sdsp_hip_last_error_string()


def _staircase(mb, nb, fill=0):
    """a valid base of any shape within the limits: the staircase, and one information entry per row and column"""
    B = -np.ones((mb, nb), dtype=np.int16)
    kb = nb - mb
    for r in range(mb):
        B[r, kb + r] = 0
        if r + 1 < mb:
            B[r + 1, kb + r] = 0
    for c in range(kb):
        B[c % mb, c] = fill
    for r in range(mb):
        B[r, r % kb] = fill
    return B


def _create(base, mb, nb, z, norm=12, beta=0, early=1, in_kind=0, scale=1.0, out_kind=0, out_bits=None):
    L, lib = _lib()
    h = C.c_void_p(0x1234)
    ptr = None if base is None else base.ctypes.data
    rc = lib.sdsp_hip_ldpc_plan_create(C.byref(h), ptr, mb, nb, z, norm, beta, early, in_kind, scale, out_kind,
                                       nb * z if out_bits is None else out_bits, 0)
    if rc == 0:
        lib.sdsp_hip_ldpc_plan_destroy(h)
    else:
        assert not h.value and lib.sdsp_hip_last_error_string()
    return rc


def _row(mb, nb, degree):
    B = _staircase(mb, nb)
    B[0] = -1
    B[0, :degree] = 0
    B[1, (B >= 0).sum(axis=0) == 0] = 0  # no column is left empty
    return B


@pytest.mark.parametrize("what,args,code", [
    ("z below", (_staircase(3, 6), 3, 6, 1), INVALID_SIZE),
    ("z above", (_staircase(3, 6), 3, 6, 513), INVALID_SIZE),
    ("mb below", (_staircase(3, 6), 0, 6, 2), INVALID_SIZE),
    ("mb above", (_staircase(65, 66), 65, 66, 2), INVALID_SIZE),
    ("nb equal to mb", (_staircase(3, 6), 3, 3, 2), INVALID_SIZE),
    ("nb above", (_staircase(3, 129), 3, 129, 2), INVALID_SIZE),
    ("n above", (_staircase(3, 33), 3, 33, 497), INVALID_SIZE),
    ("row of one entry", (_row(3, 40, 1), 3, 40, 2), INVALID_ARG),
    ("row of 33 entries", (_row(3, 40, 33), 3, 40, 2), INVALID_ARG),
    ("shift of z", (_staircase(3, 6, fill=2), 3, 6, 2), INVALID_ARG),
    ("shift of -2", (_staircase(3, 6, fill=-2), 3, 6, 2), INVALID_ARG),
])
def test_creation_refuses_codes_outside_the_limits_without_a_device(what, args, code):
    assert _create(*args) == code, what


def test_creation_refuses_an_empty_column_and_bad_parameters():
    B = _staircase(3, 6)
    empty = B.copy()
    empty[:, 1] = -1
    empty[:, 0] = 0  # rows keep two entries
    assert _create(empty, 3, 6, 2) == INVALID_ARG
    assert _create(None, 3, 6, 2) == INVALID_ARG
    for kw in ({"norm": 0}, {"norm": 17}, {"beta": 32}, {"out_bits": 0}, {"out_bits": 13}):
        assert _create(B, 3, 6, 2, **kw) == INVALID_SIZE, kw
    for kw in ({"in_kind": 2}, {"out_kind": 2}, {"in_kind": 1, "scale": 0.0}, {"in_kind": 1, "scale": float("nan")},
               {"in_kind": 1, "scale": float("inf")}, {"in_kind": 1, "scale": -1.0}):
        assert _create(B, 3, 6, 2, **kw) == INVALID_ARG, kw
    L, lib = _lib()
    assert lib.sdsp_hip_ldpc_plan_create(None, B.ctypes.data, 3, 6, 2, 12, 0, 1, 0, 1.0, 0, 12, 0) == INVALID_ARG
    assert lib.sdsp_hip_ldpc_process(None, None, None, None, None, 0, 0, None) == INVALID_ARG
    assert lib.sdsp_hip_ldpc_plan_set_variant(None, 0) == INVALID_ARG
    assert lib.sdsp_hip_ldpc_plan_get_info(None, None) == INVALID_ARG
    assert lib.sdsp_hip_ldpc_plan_destroy(None) == 0


@pytest.mark.parametrize("what,args,kw", [
    ("z = 2, 3 x 6", (_staircase(3, 6), 3, 6, 2), {}),
    ("z = 512", (_staircase(3, 6, fill=511), 3, 6, 512), {}),
    ("mb = 64, nb = 128", (_staircase(64, 128), 64, 128, 128), {}),
    ("mb = 1", (_staircase(1, 2), 1, 2, 2), {}),
    ("n = 16384", (_staircase(3, 32), 3, 32, 512), {}),
    ("row of 32 entries", (_row(3, 40, 32), 3, 40, 2), {}),
    ("row of two entries", (_row(3, 40, 2), 3, 40, 2), {}),
    ("parameters at their ends", (_staircase(3, 6), 3, 6, 2), {"norm": 16, "beta": 31, "out_bits": 1, "in_kind": 1, "scale": 1e-3, "out_kind": 1}),
])
def test_creation_takes_codes_at_the_limits(what, args, kw):
    assert _create(*args, **kw) in (0, NO_DEVICE), what  # past the argument checks: created, or no device to create it on


def test_header_declares_no_stride_for_the_ldpc_entries():
    from conftest import ROOT
    text = (ROOT / "include" / "sdsp_hip.h").read_text()
    start = text.index("int sdsp_hip_ldpc_parity_matrix")
    assert "stride" not in text[start:text.index("sdsp_hip_ldpc_plan_get_info", start)]
    assert "stride" not in text[text.index("LDPC decoder banks"):]


def test_capability_of_the_reference_at_4_db(capsys):
    """(12 x 24, Z = 32) from the generator with seed 1, 1000 codewords, BPSK over AWGN at Eb/N0 = 4 dB, float32 samples with scale 8,
    at most 30 iterations with early stop: at most 10 frame errors of 1000 for each (norm, beta)."""
    base = R.generate(12, 24, 32, 1)
    code = R.Code(base, 32)
    rng = np.random.default_rng(7)
    data = rng.integers(0, 2, (1000, code.k), dtype=np.uint8)
    noise = rng.standard_normal((1000, code.n))
    words = R.encode_staircase(code, data)
    sigma = np.sqrt(1.0 / (2 * 0.5 * 10 ** 0.4))
    y = ((1.0 - 2.0 * words) + sigma * noise).astype(np.float32)
    q = R.quantise_f32(y, 8.0)
    raw = ((q < 0) != words).mean()
    assert 0.05 < raw < 0.065, raw
    for norm, beta in [(12, 0), (13, 0), (16, 0), (16, 1)]:
        bits, _, status = R.decode(code, q, 30, norm, beta, early_stop=True)
        errors = int((bits != words).any(axis=1).sum())
        with capsys.disabled():
            print(f"\nldpc capability: norm {norm} beta {beta}: {errors} frame errors of 1000, {int((status < 0).sum())} undecoded, "
                  f"mean iterations {np.where(status < 0, 30, status).mean():.2f}, raw bit error rate {raw:.4f}")
        assert errors <= 10, (norm, beta, errors)
