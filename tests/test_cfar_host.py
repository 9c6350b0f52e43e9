"""CPU tests of the CFAR contract (tests/cfar_ref.py) and of the host designer simpledsp_amd.cfar_alpha: the numpy reference pinned
to a scalar loop, the lag / lead identity the sum kernel is built on, split invariance, the designer formulas, and the reference's
measured false-alarm rate."""
import math

import numpy as np
import pytest

from cfar_ref import block_lengths, cfar_ref, cfar_ref_rows, cfar_ref_stream, geometry, in_dtype, power, scale, side_sums
from rank_ref import row_dtype, specials, to_key
from simpledsp_amd.cfar import cfar_alpha, default_rank


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rows(rng, shape, precision, kind):
    """exponential powers mixed with special bit patterns (POWER), or normal I/Q samples"""
    rt = row_dtype(precision)
    if kind == "iq":
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(in_dtype(precision, kind))
    x = rng.exponential(1.0, shape).astype(rt)
    sp = specials(rt)
    mask = rng.random(shape) < 0.05
    x[mask] = sp[rng.integers(0, len(sp), size=int(mask.sum()))]
    x[rng.random(shape) < 0.05] = rt(-0.0)
    return x


def scalar_cfar(x, train, guard, mode, alpha, rank, hist):
    """the contract, one cell at a time with numpy scalars of the precision"""
    C, S = x.shape
    L = train
    half, W, _ = geometry(train, guard)
    full = np.concatenate([hist[:, ::-1], x], axis=1)
    p = power(full)
    rt = p.dtype.type
    c = scale(mode, L, alpha, p.dtype)
    thr = np.zeros((C, S), dtype=p.dtype)
    det = np.zeros((C, S), dtype=np.uint8)
    with np.errstate(all="ignore"):
        for ch in range(C):
            for n in range(S):
                m = n + W - 1  # index of p[n] in `full`
                lag_cells = [p[ch, m - W + 1 + i] for i in range(L)]
                lead_cells = [p[ch, m - L + 1 + i] for i in range(L)]
                if mode == "os":
                    cells = np.array(lag_cells + lead_cells, dtype=p.dtype)
                    keys = [int(k) for k in to_key(cells)]
                    order = sorted(range(2 * L), key=lambda i: keys[i])
                    t = rt(cells[order[rank]] * c)
                else:
                    lag, lead = rt(0.0), rt(0.0)
                    for v in lag_cells:
                        lag = rt(lag + v)
                    for v in lead_cells:
                        lead = rt(lead + v)
                    if mode == "ca":
                        t = rt(rt(lag + lead) * c)
                    elif mode == "go":
                        t = rt((lag if lag > lead else lead) * c)
                    else:
                        t = rt((lag if lag < lead else lead) * c)
                if t != t:
                    t = rt(np.nan)  # the canonical quiet NaN
                thr[ch, n] = t
                det[ch, n] = 1 if p[ch, m - half] > t else 0
    return thr, det


@pytest.mark.parametrize("kind", ["power", "iq"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["ca", "go", "so", "os"])
def test_reference_equals_scalar_loop(mode, precision, kind):
    rng = np.random.default_rng(11)
    for L, G in ((1, 0), (2, 1), (4, 0), (7, 3)):
        _, W, _ = geometry(L, G)
        x = _rows(rng, (2, 3 * W + 5), precision, kind)
        h = _rows(rng, (2, W - 1), precision, kind)
        for rank in sorted({0, L, 2 * L - 1}) if mode == "os" else (None,):
            want = scalar_cfar(x, L, G, mode, 3.7, rank, h)
            got = cfar_ref(x, L, G, mode, 3.7, rank, h)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (mode, precision, kind, L, G, rank)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_lag_sum_is_the_lead_sum_of_an_earlier_position(precision):
    """both sums run in ascending index, so lag(n) = lead(n - (L + 2 G + 1)) bit for bit"""
    rng = np.random.default_rng(13)
    for L, G in ((1, 0), (3, 2), (16, 2), (33, 40)):
        _, W, D = geometry(L, G)
        p = _rows(rng, (3, 4 * W), precision, "power")
        lag, lead = side_sums(p, L, G)
        assert lag.shape[1] == 4 * W - (W - 1) and D + L == W
        assert _same(lag[:, D:], lead[:, :lag.shape[1] - D])


@pytest.mark.parametrize("kind", ["power", "iq"])
@pytest.mark.parametrize("mode", ["ca", "go", "so", "os"])
def test_reference_is_split_invariant(mode, kind):
    rng = np.random.default_rng(17)
    L, G = 5, 2
    _, W, _ = geometry(L, G)
    blocks = block_lengths(L, G, 6 * W)
    assert 0 in blocks and sum(blocks) == 6 * W
    x = _rows(rng, (3, 6 * W), "f32", kind)
    h = _rows(rng, (3, W - 1), "f32", kind)
    rank = 7 if mode == "os" else None
    one = cfar_ref(x, L, G, mode, 2.5, rank, h)
    many = cfar_ref_stream(x, L, G, mode, 2.5, blocks, rank, h)
    for a, b in zip(one, many):
        assert _same(a, b)


def test_zero_rows_give_zero_threshold_and_no_detection():
    for mode in ("ca", "go", "so", "os"):
        thr, det, _ = cfar_ref(np.zeros((2, 50), dtype=np.float32), 4, 1, mode, 5.0, 3 if mode == "os" else None)
        assert not thr.any() and not det.any()


def test_finite_rows_mark_their_edges():
    rng = np.random.default_rng(19)
    x = rng.exponential(1.0, (2, 60)).astype(np.float64)
    thr, det = cfar_ref_rows(x, 4, 2, "ca", 4.0)
    assert thr.shape == x.shape and np.isinf(thr[:, :6]).all() and np.isinf(thr[:, -6:]).all() and np.isfinite(thr[:, 6:-6]).all()
    assert not det[:, :6].any() and not det[:, -6:].any()
    n = 30  # an interior cell against its own training cells
    cells = np.concatenate([x[0, n - 6:n - 2], x[0, n + 3:n + 7]])
    assert thr[0, n] == pytest.approx(cells.sum() * 4.0 / 8.0, rel=1e-12)


def test_ca_alpha_closed_form():
    for L, pfa in ((1, 1e-2), (8, 1e-3), (16, 1e-4), (128, 1e-6)):
        n = 2 * L
        a = cfar_alpha("ca", L, pfa)
        assert a == n * (pfa ** (-1.0 / n) - 1.0)
        assert (1.0 + a / n) ** (-n) == pytest.approx(pfa, rel=1e-12)


def test_os_alpha_reproduces_pfa():
    assert default_rank(16) == 24
    for L, k, pfa in ((2, 3, 1e-2), (16, 23, 1e-2), (16, None, 1e-4), (64, 96, 1e-6), (127, 0, 1e-3)):
        a = cfar_alpha("os", L, pfa, k)
        kk = default_rank(L) if k is None else k
        prod = math.prod((2 * L - i) / (2 * L - i + a) for i in range(kk + 1))
        assert prod == pytest.approx(pfa, rel=1e-12)


def test_designer_refuses_what_it_cannot_design():
    for mode in ("go", "so"):
        with pytest.raises(ValueError):
            cfar_alpha(mode, 8, 1e-3)
    with pytest.raises(ValueError):
        cfar_alpha("os", 8, 1e-3, 16)
    with pytest.raises(ValueError):
        cfar_alpha("ca", 8, 1.5)
    with pytest.raises(ValueError):
        cfar_alpha("xx", 8, 1e-3)


@pytest.mark.parametrize("mode,rank", [("ca", None), ("os", 23)])
def test_reference_false_alarm_rate(mode, rank):
    """64 x 20000 seeded exponential f64 samples, (L, G) = (16, 2), pfa = 1e-2: the measured rate is within 10 % of the design value
    (neighbouring cells share training cells, hence the width)"""
    rng = np.random.default_rng(2024)
    x = rng.exponential(1.0, (64, 20000))
    pfa = 1e-2
    alpha = cfar_alpha(mode, 16, pfa, rank)
    _, det, _ = cfar_ref(x, 16, 2, mode, alpha, rank)
    W = 2 * 18 + 1
    rate = det[:, W - 1:].mean()  # outputs whose window lies inside the noise
    print(f"{mode}: measured {rate:.6f} = {rate / pfa:.4f} of pfa")
    assert abs(rate / pfa - 1.0) <= 0.10
