"""CPU tests of the rank-order filter bank's contract (sdsp_hip_rank_*): the key transform, tests/rank_ref.py
against a scalar loop and against scipy, split invariance of the reference, and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

from rank_ref import UINT, from_key, rank_ref, rank_ref_stream, specials, to_key

import simpledsp_amd as sd
from simpledsp_amd import _lib as L

DTYPES = [np.float32, np.float64]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _tied(rng, shape, dtype):
    """finite data with heavy ties: small integers, both zeros among them"""
    x = rng.integers(-4, 5, size=shape).astype(dtype)
    x[rng.random(shape) < 0.1] = -0.0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
def test_key_transform_round_trips_every_special_bit_pattern(dtype):
    s = specials(dtype)
    ut = UINT[np.dtype(dtype)]
    assert len(set(s.view(ut).tolist())) == len(s) == 20
    assert _same(from_key(to_key(s), dtype), s)
    k = to_key(s)
    assert len(set(k.tolist())) == len(s)
    assert int(k.min()) == 0 and int(k.max()) == int(np.iinfo(ut).max)  # the two patterns a sentinel's key equals
    rng = np.random.default_rng(1)
    bits = rng.integers(0, np.iinfo(ut).max, size=4096, dtype=ut, endpoint=True)
    assert np.array_equal(from_key(to_key(bits.view(dtype)), dtype).view(ut), bits)


@pytest.mark.parametrize("dtype", DTYPES)
def test_key_transform_orders_as_total_order(dtype):
    ut = UINT[np.dtype(dtype)]
    s = specials(dtype)
    bits = s.view(ut)
    sign = ut(1) << ut(8 * bits.itemsize - 1)
    neg = (bits & sign) != 0
    mag = (bits & ~sign).astype(object)

    def total_order_less(i, j):
        """IEEE 754-2019 5.10 on sign and magnitude: negatives below positives, magnitudes reversed among negatives"""
        if neg[i] != neg[j]:
            return bool(neg[i])
        return mag[i] > mag[j] if neg[i] else mag[i] < mag[j]

    k = to_key(s)
    for i in range(len(s)):
        for j in range(len(s)):
            assert (k[i] < k[j]) == total_order_less(i, j), (i, j)
    order = s[np.argsort(k)]
    fin = ~np.isnan(order)
    assert np.isnan(order[:4]).all() and np.isnan(order[-4:]).all() and fin[4:-4].all()  # -NaNs, then -inf .. +inf, then +NaNs
    assert np.all(np.diff(order[4:-4].astype(np.float64)) >= 0)
    z = np.array([0.0, -0.0], dtype=dtype)
    assert to_key(z)[1] < to_key(z)[0]  # -0 < +0


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_equals_a_scalar_loop_with_sorted_keys(dtype):
    rng = np.random.default_rng(2)
    sp = specials(dtype)
    for W, r in ((1, 0), (2, 1), (5, 2), (8, 0), (16, 15), (17, 3)):
        S = 40
        x = sp[rng.integers(0, len(sp), size=(3, S))]
        h = sp[rng.integers(0, len(sp), size=(3, W - 1))]
        y, nh = rank_ref(x, W, r, h)
        for c in range(3):
            full = list(h[c, ::-1]) + list(x[c])
            keys = [int(v) for v in to_key(np.array(full, dtype=dtype))]
            want = [sorted(keys[n:n + W])[r] for n in range(S)]
            assert [int(v) for v in to_key(y[c])] == want
            assert _same(nh[c], np.array(full[len(full) - (W - 1):][::-1], dtype=dtype).reshape(W - 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_any_split_of_the_reference_gives_the_same_bits(dtype):
    rng = np.random.default_rng(3)
    sp = specials(dtype)
    W, r = 9, 3
    x = sp[rng.integers(0, len(sp), size=(4, 120))]
    h = sp[rng.integers(0, len(sp), size=(4, W - 1))]
    one = rank_ref(x, W, r, h)
    for blocks in ([0, 1, 7, 0, 33, 79], [120], [3] * 40, [119, 1]):
        y, nh = rank_ref_stream(x, W, r, blocks, h)
        assert _same(y, one[0]) and _same(nh, one[1]), blocks


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_equals_scipy_by_value(dtype):
    import scipy.ndimage
    import scipy.signal
    rng = np.random.default_rng(4)
    C_, S = 2, 300
    x = _tied(rng, (C_, S), dtype)
    for W in range(1, 256, 2):
        half = (W - 1) // 2
        # median: zero history and a zero tail, the first half outputs dropped
        padded = np.concatenate([x, np.zeros((C_, half), dtype=dtype)], axis=1)
        y = rank_ref(padded, W, half)[0][:, half:]
        for c in range(C_):
            assert np.array_equal(y[c], scipy.signal.medfilt(x[c], W)), W
        # minimum and maximum: a history of +-inf never wins; origin shifts scipy's centred window to the causal one
        for r, fn, fill in ((0, scipy.ndimage.minimum_filter1d, np.inf), (W - 1, scipy.ndimage.maximum_filter1d, -np.inf)):
            h = np.full((C_, W - 1), fill, dtype=dtype)
            got = rank_ref(x, W, r, h)[0]
            assert np.array_equal(got, fn(x, W, axis=1, mode="constant", cval=fill, origin=(W - 1) // 2)), (W, r)
        # any rank
        r = int(rng.integers(0, W))
        want = scipy.ndimage.rank_filter(x, r, size=(1, W), mode="constant", cval=0.0, origin=(0, (W - 1) // 2))
        assert np.array_equal(rank_ref(x, W, r)[0], want), (W, r)


def test_python_layer_checks_its_arguments_before_it_needs_a_device():
    import torch
    from simpledsp_amd.rank_filter import rank_index
    assert rank_index(5, "median") == 2 and rank_index(5, "min") == 0 and rank_index(6, "max") == 5 and rank_index(6, 4) == 4
    for bad in ((6, "median"), (5, 5), (5, -1), (5, "mean"), (0, 0), (5, 1.0), (5, True)):
        with pytest.raises(ValueError):
            rank_index(*bad)
    with pytest.raises(ValueError):
        sd.rank_filter_bank(4, 256)
    with pytest.raises(ValueError):
        sd.rank_filter_bank(4, 129, precision=sd.F64)
    with pytest.raises(ValueError):
        sd.rank_filter_bank(4, 8, "median")
    with pytest.raises(ValueError):
        sd.rank_filter_bank(0, 5)
    with pytest.raises(ValueError):
        sd.rank_filter_bank(4, 5, precision=sd.F32_F64STATE)
    for bad in (4, 0, -3, 3.0):
        with pytest.raises(ValueError):
            sd.medfilt(torch.zeros(8), bad)
    with pytest.raises(ValueError):
        sd.medfilt(torch.zeros(8, dtype=torch.int32), 3)
    with pytest.raises(ValueError):
        sd.medfilt(torch.zeros(8), 257)
    with pytest.raises(ValueError):
        sd.medfilt(torch.zeros(8), 3)  # a host tensor


def test_plan_creation_checks_its_arguments_before_it_needs_a_device():
    import torch
    lib = sd.load()
    p = C.c_void_p()

    def create(channels=4, window=5, rank=2, precision=L.F32):
        return lib.sdsp_hip_rank_plan_create(C.byref(p), channels, window, rank, precision, 0)

    assert create(window=0) == L.ERR_INVALID_SIZE and create(window=256, rank=0) == L.ERR_INVALID_SIZE
    assert create(window=128, rank=0, precision=L.F64) == L.ERR_INVALID_SIZE
    assert create(channels=0) == L.ERR_INVALID_SIZE and create(channels=1 << 31) == L.ERR_INVALID_SIZE
    assert create(rank=5) == L.ERR_INVALID_ARG
    assert create(precision=L.F32_F64STATE) == L.ERR_INVALID_ARG and create(precision=9) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_plan_create(None, 4, 5, 2, L.F32, 0) == L.ERR_INVALID_ARG
    n = C.c_uint64(0)
    info = L.RankPlanInfo()
    assert lib.sdsp_hip_rank_process(None, None, 0, None, 0, 0, None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_process_host(None, None, 0, None, 0, 0, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_state_bytes(None, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_plan_set_run(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_plan_launches(None, 1, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_plan_get_info(None, C.byref(info)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_plan_destroy(None) == 0
    # what is left needs a device
    for kw in (dict(window=255, rank=254), dict(window=127, rank=0, precision=L.F64), dict(window=1, rank=0)):
        rc = create(**kw)
        if torch.cuda.is_available():
            assert rc == 0
            lib.sdsp_hip_rank_plan_destroy(p)
        else:
            assert rc == L.ERR_NO_DEVICE
    if not torch.cuda.is_available():
        with pytest.raises(sd.SdspHipError):  # no CPU path
            sd.rank_filter_bank(4, 5)
