"""GPU tests of the CFAR detector bank (sdsp_hip_cfar_*) on a real MI355X.

The checker is tests/cfar_ref.py, the contract in numpy, itself pinned to a scalar loop in tests/test_cfar_host.py.  The contract fixes
the order of every addition and the rounding of every product, so both precisions, both input kinds and both kernel variants are held
to bit-exact agreement with it, through tobytes(): thr, det, the final history and the state buffer.  A threshold that is a NaN is
the canonical quiet NaN in the contract, so it is compared by its bits like every other one.

The bank is causal, so the reference of a long row is the reference of each of its prefixes, and rows are independent, so the reference
of 65 rows holds that of the first one and the first three: one reference per case serves every (channels, S) of it."""
import numpy as np
import pytest

import arena
from cfar_ref import block_lengths, cfar_ref, cfar_ref_rows, geometry, in_dtype, power
from rank_ref import row_dtype, specials

pytestmark = pytest.mark.gpu

CH = 65  # one full wave of runs and one more row
GEOMETRIES = [(1, 0), (2, 1), (4, 0), (7, 3), (16, 2), (33, 40), (64, 255), (128, 0)]
OS_EDGES = [4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127]  # 2 L = 8, 10, 16, 18, 32, 34, 64, 66, 128, 130, 254: both sides of each WP step
OS_EDGES_F64 = [63]  # 2 L = 126: the largest OS window of f64, the whole of its WP = 128 array but two sentinels
ALPHA = 2.75


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def sd():
    import simpledsp_amd
    simpledsp_amd.load(build_if_missing=True)
    return simpledsp_amd


def _rows(rng, shape, precision, kind, special=0.0):
    """exponential powers or normal I/Q samples; `special`: the share of POWER cells replaced by special bit patterns (NaNs and
    infinities of both signs, both zeros, denormals, negative values)"""
    rt = row_dtype(precision)
    if kind == "iq":
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(in_dtype(precision, kind))
    x = rng.exponential(1.0, shape).astype(rt)
    if special:
        sp = specials(rt)
        mask = rng.random(shape) < special
        x[mask] = sp[rng.integers(0, len(sp), size=int(mask.sum()))]
    return x


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _as_tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _bank(sd, channels, L, G, mode, precision, kind="power", variant=0, rank=None, alpha=ALPHA, hist=None):
    b = sd.cfar_bank(channels, L, G, mode, alpha=alpha, rank=rank, input=kind, precision=sd.F64 if precision == "f64" else sd.F32)
    b.set_variant(variant)
    if hist is not None:
        b.set_history(_as_tensor(hist))
    return b


def _hist_after(x, h0):
    """the history a call over x leaves: the newest W - 1 elements of (h0 reversed, x), newest first"""
    full = np.concatenate([h0[:, ::-1], x], axis=1)
    return np.ascontiguousarray(full[:, full.shape[1] - h0.shape[1]:][:, ::-1])


def _check(b, out, want, tag):
    """out: the device (thr, det); want = (thr, det, history)"""
    thr, det = _np(out[0]), _np(out[1])
    assert thr.shape == want[0].shape and det.shape == want[1].shape, (tag, thr.shape, det.shape)
    if not _same(thr, want[0]):
        ut = np.uint64 if thr.dtype == np.float64 else np.uint32
        where = np.argwhere(thr.view(ut) != want[0].view(ut))
        raise AssertionError((tag, "thr", len(where), "first at", where[0].tolist(), float(thr[tuple(where[0])]),
                              float(want[0][tuple(where[0])])))
    assert _same(det, want[1]), (tag, "det", int((det != want[1]).sum()))
    assert _same(_np(b.history()), want[2]), (tag, "history")
    assert _same(_np(b.state), want[2].reshape(-1)), (tag, "state")


def _unit(info, W):
    """the granule of variant 0 whose multiples the lengths straddle: OS, the staging block; sum modes, the segment the automatic run
    gives a small call (four windows or 256 outputs, a multiple of 16, capped at the largest segment)"""
    if info["mode"] == 3:
        return info["block"]
    return min(info["block"], (max(256, 4 * W) + 15) // 16 * 16)


def _lengths(half, W, unit):
    """0, 1, half, W - 2, W - 1, W, and one, two and three granules +- 1"""
    out = {0, 1, half, W - 2, W - 1, W}
    for m in (1, 2, 3):
        out |= {m * unit - 1, m * unit, m * unit + 1}
    return sorted(out)


def _valid(mode, precision, L):
    return mode != "os" or 2 * L <= (127 if precision == "f64" else 255)


def _run_case(sd, torch, mode, precision, kind, L, G, ranks, seed):
    half, W, _ = geometry(L, G)
    rng = np.random.default_rng(seed)
    info = _bank(sd, CH, L, G, mode, precision, kind, rank=ranks[0]).info()
    assert (info["half"], info["window"], info["lag_shift"]) == (half, W, L + 2 * G + 1)
    lengths = _lengths(half, W, _unit(info, W))
    top = max(lengths) + (-max(lengths)) % 4  # rows that start on 16-byte boundaries
    x = _rows(rng, (CH, top), precision, kind, special=0.002)
    h0 = _rows(rng, (CH, W - 1), precision, kind)
    xd = _dev(torch, x)
    for rank in ranks:
        ref = cfar_ref(x, L, G, mode, ALPHA, rank, h0)
        for channels in (1, 3, CH):
            xc = xd[:channels].contiguous()
            for S in lengths:
                want = (ref[0][:channels, :S], ref[1][:channels, :S], _hist_after(x[:channels, :S], h0[:channels]))
                for variant in (0, 1):
                    b = _bank(sd, channels, L, G, mode, precision, kind, variant, rank, hist=h0[:channels])
                    _check(b, b.process(xc, samples=S), want, (mode, precision, kind, L, G, rank, channels, S, variant))


@pytest.mark.parametrize("L,G", GEOMETRIES)
@pytest.mark.parametrize("kind", ["power", "iq"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["ca", "go", "so"])
def test_sum_modes_bit_exact(sd, torch_cuda, mode, precision, kind, L, G):
    """both variants, non-zero history, 1, 3 and 65 rows, every row length at which the staging takes another path"""
    _run_case(sd, torch_cuda, mode, precision, kind, L, G, [None], 1000 * L + G)


def _os_ranks(L, seed):
    rng = np.random.default_rng(seed)
    return sorted({0, L, 2 * L - 1, int(rng.integers(0, 2 * L))})


@pytest.mark.parametrize("precision,L,G", [(p, L, G) for p in ("f32", "f64") for L, G in GEOMETRIES + [(L, 1) for L in OS_EDGES]]
                         + [("f64", L, 1) for L in OS_EDGES_F64])
@pytest.mark.parametrize("kind", ["power", "iq"])
def test_os_mode_bit_exact(sd, torch_cuda, precision, kind, L, G):
    """as above for OS at ranks 0, the middle, 2 L - 1 and a seeded one; the geometries past the register limits are refused"""
    if not _valid("os", precision, L):
        with pytest.raises(ValueError):
            _bank(sd, CH, L, G, "os", precision, kind, rank=0)
        d = sd._lib.CfarDesc(L, G, sd.CFAR_OS, 0, sd.CFAR_POWER, 1.0)
        import ctypes
        h = ctypes.c_void_p()
        rc = sd.load().sdsp_hip_cfar_plan_create(ctypes.byref(h), CH, ctypes.byref(d), sd.F64 if precision == "f64" else sd.F32, 0)
        assert rc == sd._lib.ERR_INVALID_SIZE
        return
    _run_case(sd, torch_cuda, "os", precision, kind, L, G, _os_ranks(L, 77 + L), 2000 * L + G)


def test_os_padded_sizes(sd, torch_cuda):
    assert [_bank(sd, 2, L, 1, "os", "f32", rank=0).info()["padded"] for L in OS_EDGES] == [8, 16, 16, 32, 32, 64, 64, 128, 128, 256, 256]
    assert _bank(sd, 2, 63, 1, "os", "f64", rank=0).info()["padded"] == 128
    assert _bank(sd, 2, 8, 1, "ca", "f32").info()["padded"] == 0
    assert sd.cfar_bank(2, 16, 2, "os", alpha=1.0).rank == 24  # the default rank: (3 * 2 L) // 4


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["ca", "go", "so", "os"])
def test_special_values(sd, torch_cuda, mode, precision):
    """rows drawn from twenty special bit patterns (NaNs and infinities of both signs, both zeros, denormals, negative values, the
    patterns whose keys equal a sentinel's) with long ties, and all-zero rows, where thr = 0 and det = 0"""
    torch = torch_cuda
    L, G = 5, 2
    _, W, _ = geometry(L, G)
    rng = np.random.default_rng(300 + len(mode))
    S = 700
    sp = specials(row_dtype(precision))
    x = sp[rng.integers(0, len(sp), size=(CH, S))]
    x[:, 100:160] = x[:, 100:101]  # sixty equal cells in a row
    h0 = sp[rng.integers(0, len(sp), size=(CH, W - 1))]
    for rank in ([0, 4, 9] if mode == "os" else [None]):
        want = cfar_ref(x, L, G, mode, ALPHA, rank, h0)
        zero = np.zeros((CH, S), dtype=x.dtype)
        for variant in (0, 1):
            b = _bank(sd, CH, L, G, mode, precision, "power", variant, rank, hist=h0)
            _check(b, b.process(_dev(torch, x)), want, (mode, precision, rank, variant))
            z = _bank(sd, CH, L, G, mode, precision, "power", variant, rank)
            thr, det = z.process(_dev(torch, zero))
            assert _same(_np(thr), zero) and not bool(det.any()), (mode, precision, rank, variant, "zero rows")


@pytest.mark.parametrize("mode,precision,kind,L,G", [("ca", "f32", "power", 7, 3), ("go", "f64", "iq", 16, 2), ("so", "f32", "iq", 2, 1),
                                                     ("os", "f32", "power", 9, 2), ("os", "f64", "iq", 16, 0)])
def test_any_split_gives_the_same_bits(sd, torch_cuda, mode, precision, kind, L, G):
    """ragged calls (empty ones, 1, half, W - 2, W - 1, W, the rest) equal one call: outputs and final state"""
    torch = torch_cuda
    half, W, _ = geometry(L, G)
    rng = np.random.default_rng(29 + W)
    S = 5 * W + 301
    blocks = block_lengths(L, G, S)
    assert blocks.count(0) >= 3
    x = _rows(rng, (CH, S), precision, kind, special=0.01)
    h0 = _rows(rng, (CH, W - 1), precision, kind)
    rank = L if mode == "os" else None
    want = cfar_ref(x, L, G, mode, ALPHA, rank, h0)
    starts = np.cumsum([0] + blocks[:-1])
    for variant in (0, 1):
        b = _bank(sd, CH, L, G, mode, precision, kind, variant, rank, hist=h0)
        parts = [b.process(_dev(torch, x[:, s0:s0 + n].copy())) for s0, n in zip(starts, blocks)]
        out = (torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1))
        _check(b, out, want, (variant, "split"))


@pytest.mark.parametrize("mode,precision,kind,L,G", [("ca", "f32", "power", 7, 3), ("so", "f64", "iq", 33, 40), ("os", "f32", "iq", 4, 1),
                                                     ("os", "f64", "power", 20, 3)])
def test_history_reset_and_alpha(sd, torch_cuda, mode, precision, kind, L, G):
    """history() / set_history() move a stream between banks; reset() starts it again; set_alpha() changes later calls only"""
    torch = torch_cuda
    half, W, _ = geometry(L, G)
    rng = np.random.default_rng(51 + W)
    S = 2 * W + 40
    x = _rows(rng, (3, 2 * S), precision, kind)
    rank = L + 1 if mode == "os" else None
    whole = cfar_ref(x, L, G, mode, ALPHA, rank)
    first = cfar_ref(x[:, :S], L, G, mode, ALPHA, rank)
    a = _bank(sd, 3, L, G, mode, precision, kind, 0, rank)
    _check(a, a.process(_dev(torch, x[:, :S].copy())), first, "first half")
    b = _bank(sd, 3, L, G, mode, precision, kind, 0, rank)
    b.set_history(a.history().clone())
    out = b.process(_dev(torch, x[:, S:].copy()))
    _check(b, out, (whole[0][:, S:], whole[1][:, S:], whole[2]), "second half through set_history")
    b.reset()
    assert not bool(torch.view_as_real(b.state).any() if b.state.is_complex() else b.state.any())
    _check(b, b.process(_dev(torch, x[:, :S].copy())), first, "after reset")
    # another alpha for the second half: the state stays, the thresholds follow
    b.set_alpha(0.5)
    assert b.info()["alpha"] == 0.5
    second = cfar_ref(x[:, S:], L, G, mode, 0.5, rank, first[2])
    _check(b, b.process(_dev(torch, x[:, S:].copy())), second, "after set_alpha")


@pytest.mark.parametrize("mode,precision,kind,L,G", [("ca", "f32", "power", 7, 3), ("go", "f64", "iq", 40, 9), ("so", "f32", "power", 1, 0),
                                                     ("os", "f32", "power", 7, 3), ("os", "f64", "iq", 17, 0),
                                                     ("os", "f32", "iq", 65, 1), ("os", "f32", "power", 127, 0),
                                                     ("os", "f64", "power", 63, 1)])
def test_the_run_length_does_not_change_the_bits(sd, torch_cuda, mode, precision, kind, L, G):
    """3 rows of 5000 samples: runs start inside rows, inside the history and at ragged ends; every run gives variant 1's bits.  The
    last three cases are the arrays of 256 and 128 keys (f32 2 L = 130 and 254, f64 2 L = 126) with several runs per row"""
    torch = torch_cuda
    half, W, _ = geometry(L, G)
    S, C_ = 5000, 3
    rng = np.random.default_rng(31 + W)
    x = _rows(rng, (C_, S), precision, kind, special=0.01)
    h0 = _rows(rng, (C_, W - 1), precision, kind)
    xd = _dev(torch, x)
    rank = 2 * L - 2 if mode == "os" else None
    want = cfar_ref(x, L, G, mode, ALPHA, rank, h0)
    plain = _bank(sd, C_, L, G, mode, precision, kind, 1, rank, hist=h0)
    _check(plain, plain.process(xd), want, "plain")
    block = plain.info()["block"]
    for run in (0, 1, W - 1, W, 64, 100, block, block + 1, S):
        b = _bank(sd, C_, L, G, mode, precision, kind, 0, rank, hist=h0)
        b.set_run(run)
        assert b.info()["run"] == run
        _check(b, b.process(xd), want, run)
        took = b.info()["last_run"]
        if mode == "os":
            assert took == run if run else 4 * W <= took <= S
        else:
            assert took == min(run, block) if run else 256 <= took <= block
    b.set_run(0)
    assert b.info()["run"] == 0


def test_either_output_alone(sd, torch_cuda):
    torch = torch_cuda
    L_ = sd._lib
    rng = np.random.default_rng(61)
    for mode, rank in (("ca", None), ("os", 5)):
        x = _rows(rng, (CH, 333), "f32", "power")
        want = cfar_ref(x, 4, 1, mode, ALPHA, rank)
        for variant in (0, 1):
            b = _bank(sd, CH, 4, 1, mode, "f32", "power", variant, rank)
            thr, det = b.process(_dev(torch, x), det=False)
            assert det is None and _same(_np(thr), want[0])
            b.reset()
            thr, det = b.process(_dev(torch, x), thr=None)
            assert thr is None and _same(_np(det), want[1])
            with pytest.raises(ValueError):
                b.process(_dev(torch, x), thr=False, det=False)
            xd = _dev(torch, x)
            rc = sd.load().sdsp_hip_cfar_process(b._plan, xd.data_ptr(), 333, None, 0, None, 0, 333, None, None)
            assert rc == L_.ERR_INVALID_ARG


def _framed_u8(torch, shape, lead, margin, row_stride):
    """arena.framed for bytes: (arena, view), the arena filled with 0xA5"""
    inner = shape[0] * row_stride
    ar = torch.full((2 * margin + lead + inner,), 0xA5, dtype=torch.uint8, device="cuda")
    start = margin + lead
    return ar, ar[start:start + inner].view(shape[0], row_stride)


@pytest.mark.parametrize("kind", ["power", "iq"])
@pytest.mark.parametrize("mode,precision", [("ca", "f32"), ("go", "f64"), ("os", "f32"), ("os", "f64")])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, mode, precision, kind):
    """x, thr, det and state carved 0, 1 or 2 elements past a 512-byte boundary out of filled arenas, row strides of their own above S:
    the interior has the aligned run's bits and nothing outside it is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(35)
    L, G = 4, 2
    _, W, _ = geometry(L, G)
    rank = 5 if mode == "os" else None
    S = 2 * 256 + 9
    assert S % 4 == 1
    x = _rows(rng, (CH, S), precision, kind)
    h0 = _rows(rng, (CH, W - 1), precision, kind)
    ref = _bank(sd, CH, L, G, mode, precision, kind, 0, rank, hist=h0)
    clean = ref.process(_dev(torch, x))
    _check(ref, clean, cfar_ref(x, L, G, mode, ALPHA, rank, h0), "aligned")
    start = _dev(torch, h0).flatten()
    xdt, tdt = start.dtype, clean[0].dtype
    for variant in (0, 1):
        b = _bank(sd, CH, L, G, mode, precision, kind, variant, rank)
        # strides S + 5 and S + 7: rows start anywhere; lead 0 with strides S + 7, S + 3: every row starts on a 16-byte boundary
        for lead, px, pt in ((0, 5, 7), (1, 5, 7), (2, 5, 7), (0, 7, 3)):
            for fx, ft in zip(arena.fills(xdt), arena.fills(tdt)):
                ax, vx = arena.framed(torch, (CH, S), xdt, lead, 64, fx, row_stride=S + px)
                at, vt = arena.framed(torch, (CH, S), tdt, lead, 64, ft, row_stride=S + pt)
                ad, vd = _framed_u8(torch, (CH, S), lead, 64, S + pt)
                ast, vst = arena.framed(torch, (start.numel(),), xdt, lead, 64, fx)
                vx[:, :S].copy_(_dev(torch, x))
                vst.copy_(start)
                before = [arena.bits(a).clone() for a in (ax, at, ast)]
                before_d = ad.clone()
                assert lib.sdsp_hip_cfar_process(b._plan, vx.data_ptr(), S + px, vt.data_ptr(), S + pt, vd.data_ptr(), S + pt, S,
                                                 vst.data_ptr(), None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, px, fx)
                assert arena.same_bits(vt[:, :S], clean[0]), tag
                assert bool(torch.equal(vd[:, :S], clean[1])), tag
                assert arena.same_bits(vst, ref.state), tag
                arena.assert_frame_untouched(before[0], ax, slice(0, 0))  # x is never written
                arena.assert_frame_untouched(before[1], at, arena.interior_mask(torch, at, vt, S))
                arena.assert_frame_untouched(before[2], ast, arena.interior_mask(torch, ast, vst))
                inside = torch.zeros(ad.numel(), dtype=torch.bool, device="cuda")
                inside[64 + lead:64 + lead + CH * (S + pt)].view(CH, S + pt)[:, :S] = True
                assert bool(torch.equal(ad[~inside], before_d[~inside])), (tag, "det frame")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("L,G", [(1, 0), (5, 2), (16, 0)])
def test_a_nan_reaches_exactly_its_training_windows(sd, torch_cuda, L, G, variant):
    """CA: a NaN at cell m of a row makes thr[n] NaN exactly where m is a training cell of n, and changes nothing else"""
    torch = torch_cuda
    half, W, _ = geometry(L, G)
    rng = np.random.default_rng(37)
    S = 1100
    x = _rows(rng, (CH, S), "f32", "power")
    clean = [_np(t) for t in _bank(sd, CH, L, G, "ca", "f32", variant=variant).process(_dev(torch, x))]
    xp = x.copy()
    places = [(63, 11, 0x7FC00000), (64, 300, 0xFFC00001)]
    for c, m, pattern in places:
        xp.view(np.uint32)[c, m] = pattern
    want = cfar_ref(xp, L, G, "ca", ALPHA)
    got = [_np(t) for t in _bank(sd, CH, L, G, "ca", "f32", variant=variant).process(_dev(torch, xp))]
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    nan_at = np.zeros((CH, S), dtype=bool)
    cut_at = np.zeros((CH, S), dtype=bool)
    for c, m, _ in places:
        nan_at[c, m:m + L] = True                  # m is a lead cell of n: n - L + 1 <= m <= n
        nan_at[c, m + W - L:m + W] = True          # m is a lag cell of n: n - W + 1 <= m <= n - W + L
        cut_at[c, m + half] = True                 # m is the cell under test of n
    assert np.array_equal(np.isnan(got[0]), nan_at)
    assert _same(got[0][~nan_at], clean[0][~nan_at])
    assert not got[1][nan_at | cut_at].any()
    assert _same(got[1][~(nan_at | cut_at)], clean[1][~(nan_at | cut_at)])


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["ca", "so", "os"])
def test_iq_equals_power_of_its_squares(sd, torch_cuda, mode, precision):
    """an IQ bank gives the bits of a POWER bank fed with numpy's re re + im im"""
    torch = torch_cuda
    rng = np.random.default_rng(71)
    L, G = 6, 1
    _, W, _ = geometry(L, G)
    z = _rows(rng, (CH, 600), precision, "iq")
    hz = _rows(rng, (CH, W - 1), precision, "iq")
    rank = 8 if mode == "os" else None
    for variant in (0, 1):
        a = _bank(sd, CH, L, G, mode, precision, "iq", variant, rank, hist=hz)
        b = _bank(sd, CH, L, G, mode, precision, "power", variant, rank, hist=power(hz))
        ta, da = a.process(_dev(torch, z))
        tb, db = b.process(_dev(torch, power(z)))
        assert arena.same_bits(ta, tb) and bool(torch.equal(da, db)), (mode, precision, variant)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_finite_rows(sd, torch_cuda, precision):
    """cfar(): output n belongs to cell n and the edges are marked; two 30 dB targets G + 2 cells apart in exponential noise are both
    found by OS (L = 16, k = 24, pfa = 1e-4) at their own indices"""
    torch = torch_cuda
    rng = np.random.default_rng(83)
    L, G, k = 16, 2, 24
    half = L + G
    x = rng.exponential(1.0, (5, 400)).astype(row_dtype(precision))
    t0, t1 = 200, 200 + G + 2
    x[2, t0] = x[2, t1] = 1000.0
    alpha = sd.cfar_alpha("os", L, 1e-4, k)
    thr, det = sd.cfar(_dev(torch, x), L, G, "os", pfa=1e-4, rank=k)
    want = cfar_ref_rows(x, L, G, "os", alpha, k)
    assert _same(_np(thr), want[0]) and _same(_np(det), want[1])
    assert bool(torch.isinf(thr[:, :half]).all()) and bool(torch.isinf(thr[:, -half:]).all())
    assert not bool(det[:, :half].any()) and not bool(det[:, -half:].any())
    assert int(det[2, t0]) == 1 and int(det[2, t1]) == 1
    for mode in ("ca", "go", "so"):
        thr, det = sd.cfar(_dev(torch, x), L, G, mode, alpha=6.0)
        want = cfar_ref_rows(x, L, G, mode, 6.0)
        assert _same(_np(thr), want[0]) and _same(_np(det), want[1]), mode
    t1d, d1d = sd.cfar(_dev(torch, x[2]), L, G, "ca", pfa=1e-3)  # one row, the designer's alpha
    want = cfar_ref_rows(x[2:3], L, G, "ca", sd.cfar_alpha("ca", L, 1e-3))
    assert _same(_np(t1d), want[0][0]) and _same(_np(d1d), want[1][0])
    z = (rng.standard_normal((2, 90)) + 1j * rng.standard_normal((2, 90))).astype(in_dtype(precision, "iq"))
    thr, det = sd.cfar(_dev(torch, z), 3, 1, "go", alpha=4.0)
    want = cfar_ref_rows(z, 3, 1, "go", 4.0)
    assert _same(_np(thr), want[0]) and _same(_np(det), want[1])


@pytest.mark.parametrize("mode", ["ca", "os"])
def test_graph_capture_replays_the_eager_result(sd, torch_cuda, mode):
    """three calls (a long one, a ragged one, a short one) captured into one graph replay to the eager bits"""
    torch = torch_cuda
    rng = np.random.default_rng(39)
    L, G = 6, 2
    rank = 7 if mode == "os" else None
    sizes = [64, 37, 7]
    S = sum(sizes)
    x = _rows(rng, (CH, S), "f32", "power", special=0.02)
    want = cfar_ref(x, L, G, mode, ALPHA, rank)
    xs = [_dev(torch, x[:, s0:s0 + n].copy()) for s0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    ts = [torch.empty((CH, n), dtype=torch.float32, device="cuda") for n in sizes]
    ds = [torch.empty((CH, n), dtype=torch.uint8, device="cuda") for n in sizes]
    b = _bank(sd, CH, L, G, mode, "f32", rank=rank)
    run = lambda: [b.process(xs[i], thr=ts[i], det=ds[i]) for i in range(3)]  # noqa: E731
    run()  # the state exists before capture
    _check(b, (torch.cat(ts, dim=1).clone(), torch.cat(ds, dim=1).clone()), want, "eager")
    b.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    b.reset()
    for t in ts + ds:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    _check(b, (torch.cat(ts, dim=1), torch.cat(ds, dim=1)), want, "replay")


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(43)
    for mode, kind, rank in (("go", "iq", None), ("os", "power", 3)):
        L, G, S = 5, 1, 90
        _, W, _ = geometry(L, G)
        x = _rows(rng, (CH, S), "f64", kind)
        h0 = _rows(rng, (CH, W - 1), "f64", kind)
        b = _bank(sd, CH, L, G, mode, "f64", kind, 0, rank, hist=h0)
        thr, det = b.process(_dev(torch_cuda, x))
        st, ot, od = h0.copy().reshape(-1), np.zeros((CH, S)), np.zeros((CH, S), dtype=np.uint8)
        assert lib.sdsp_hip_cfar_process_host(b._plan, x.ctypes.data, S, ot.ctypes.data, S, od.ctypes.data, S, S, st.ctypes.data) == 0
        assert _same(ot, _np(thr)) and _same(od, _np(det)) and _same(st, _np(b.state))
        ot2 = np.zeros((CH, S))
        assert lib.sdsp_hip_cfar_process_host(b._plan, x.ctypes.data, S, ot2.ctypes.data, S, None, 0, S, None) == 0  # zero history
        assert _same(ot2, cfar_ref(x, L, G, mode, ALPHA, rank)[0])


def test_info_error_codes_and_launch_count(sd, torch_cuda):
    import ctypes
    torch = torch_cuda
    lib = sd.load()
    L_ = sd._lib
    b = _bank(sd, CH, 16, 2, "os", "f32", rank=23)
    info = b.info()
    assert (info["channels"], info["train"], info["guard"], info["half"], info["window"], info["lag_shift"]) == (CH, 16, 2, 18, 37, 21)
    assert (info["rank"], info["padded"], info["mode"], info["input"], info["precision"]) == (23, 32, sd.CFAR_OS, sd.CFAR_POWER, sd.F32)
    assert (info["variant"], info["run"], info["last_run"], info["kernel"]) == (0, 0, 0, "sdsp_cfar_os_kernel")
    assert info["alpha"] == ALPHA and info["scale"] == float(np.float32(ALPHA))
    assert info["lds_bytes"] == 5 * info["block"] * 65 * 4 + 512
    ca = _bank(sd, CH, 16, 2, "ca", "f64", "iq")
    assert ca.info()["kernel"] == "sdsp_cfar_sum_kernel" and ca.info()["scale"] == ALPHA / 32.0 and ca.info()["block"] == 1024
    assert _bank(sd, CH, 16, 2, "go", "f32").info()["scale"] == float(np.float32(ALPHA / 16.0)) and _bank(sd, 1, 1, 0, "so", "f32").info()["block"] == 2048
    assert b.state_bytes() == CH * 36 * 4 and ca.state_bytes() == CH * 36 * 16 and b.history().shape == (CH, 36)
    assert b.launches(100) == 2 and b.launches(0) == 0
    b.set_variant(1)
    assert b.info()["kernel"] == "sdsp_cfar_plain_kernel" and b.info()["variant"] == 1

    def create(channels=2, train=4, guard=1, mode=sd.CFAR_CA, rank=0, kind=sd.CFAR_POWER, precision=sd.F32):
        h = ctypes.c_void_p()
        d = L_.CfarDesc(train, guard, mode, rank, kind, 1.0)
        rc = lib.sdsp_hip_cfar_plan_create(ctypes.byref(h), channels, ctypes.byref(d), precision, 0)
        if rc == 0:
            lib.sdsp_hip_cfar_plan_destroy(h)
        return rc

    assert create() == 0 and create(train=128, guard=255) == 0 and create(train=127, mode=sd.CFAR_OS, rank=253) == 0
    assert create(train=0) == L_.ERR_INVALID_SIZE and create(train=129) == L_.ERR_INVALID_SIZE and create(guard=256) == L_.ERR_INVALID_SIZE
    assert create(channels=0) == L_.ERR_INVALID_SIZE and create(channels=1 << 31) == L_.ERR_INVALID_SIZE
    assert create(train=128, mode=sd.CFAR_OS) == L_.ERR_INVALID_SIZE and create(train=64, mode=sd.CFAR_OS, precision=sd.F64) == L_.ERR_INVALID_SIZE
    assert create(train=4, mode=sd.CFAR_OS, rank=8) == L_.ERR_INVALID_ARG
    assert create(mode=4) == L_.ERR_INVALID_ARG and create(kind=2) == L_.ERR_INVALID_ARG and create(precision=7) == L_.ERR_INVALID_ARG
    h = ctypes.c_void_p()
    assert lib.sdsp_hip_cfar_plan_create(ctypes.byref(h), 2, None, sd.F32, 0) == L_.ERR_INVALID_ARG
    for bad in (dict(train=0), dict(train=129), dict(guard=-1), dict(guard=256), dict(mode="cago"), dict(rank=8, mode="os"), dict(input="x")):
        kw = dict(channels=2, train=4, guard=1, mode="ca", alpha=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            sd.cfar_bank(**kw)
    with pytest.raises(ValueError):
        sd.cfar_bank(2, 4, 1, "go", pfa=1e-3)  # no designer for GO
    with pytest.raises(ValueError):
        sd.cfar_bank(2, 4, 1, "ca")  # neither alpha nor pfa
    assert sd.cfar_bank(2, 4, 1, "ca", pfa=1e-3).alpha == sd.cfar_alpha("ca", 4, 1e-3)

    p = _bank(sd, 2, 4, 1, "ca", "f32")
    x, t = torch.zeros((2, 64), device="cuda"), torch.zeros((2, 64), device="cuda")
    d = torch.zeros((2, 64), dtype=torch.uint8, device="cuda")
    X, T, D = x.data_ptr(), t.data_ptr(), d.data_ptr()

    def run(x=X, xs=64, t=T, ts=64, d=D, ds=64, n=64, state=None):
        return lib.sdsp_hip_cfar_process(p._plan, x, xs, t, ts, d, ds, n, state, None)

    assert run() == 0
    assert run(x=None) == L_.ERR_INVALID_ARG and run(t=None, d=None) == L_.ERR_INVALID_ARG
    assert run(t=None) == 0 and run(d=None) == 0
    assert run(xs=60) == L_.ERR_INVALID_ARG and run(ts=63) == L_.ERR_INVALID_ARG and run(ds=10) == L_.ERR_INVALID_ARG
    assert run(t=X + 8 * 4) == L_.ERR_INVALID_ARG and run(d=X + 3) == L_.ERR_INVALID_ARG and run(d=T + 100) == L_.ERR_INVALID_ARG  # overlaps
    assert run(x=X + 2, n=32) == L_.ERR_INVALID_ARG  # misaligned
    assert run(n=1 << 31) == L_.ERR_INVALID_SIZE
    assert run(n=0) == 0
    assert lib.sdsp_hip_cfar_plan_set_variant(p._plan, 2) == L_.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar_plan_set_run(p._plan, 1 << 31) == L_.ERR_INVALID_SIZE
    # a grid that does not fit one launch: 2^30 rows of 2^20 one-sample segments.  The refusal comes before any launch, so the
    # disjoint address ranges are never touched
    big = _bank(sd, 1 << 30, 4, 1, "ca", "f32")
    big.set_run(1)
    rc = lib.sdsp_hip_cfar_process(big._plan, 1 << 12, 1 << 20, (1 << 12) + (1 << 53), 1 << 20, None, 0, 1 << 20, None, None)
    assert rc == L_.ERR_UNSUPPORTED and b"too large for one launch" in lib.sdsp_hip_last_error_string()
    # a call of S = 0 leaves the state alone
    st = torch.full((2 * 10,), 3.0, device="cuda")
    assert run(n=0, state=st.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((st == 3.0).all())
