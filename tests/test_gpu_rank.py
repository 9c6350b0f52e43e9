"""GPU tests of the rank-order filter bank (sdsp_hip_rank_*) on a real MI355X.

The checker is tests/rank_ref.py, the contract in numpy, itself pinned to a scalar loop and to scipy in tests/test_rank_host.py.  Every
output is one of the inputs, so both precisions and both kernel variants are held to bit-exact agreement with it, through tobytes():
y, the final history and the state buffer."""
import numpy as np
import pytest

import arena
from rank_ref import rank_ref, rank_ref_stream, row_dtype, specials

pytestmark = pytest.mark.gpu

CH = 133  # two full waves and a ragged one
# every size of the ladder of sorted-array sizes (8, 16, 32, 64, 128, 256) with the window below and above each step
WINDOWS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255]


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


def _rand(rng, shape, precision):
    """normal values quantised to eighths: ties in most windows, every value exact in both precisions"""
    return (np.round(8.0 * rng.standard_normal(shape)) / 8.0).astype(row_dtype(precision))


def _special_rows(rng, shape, precision):
    sp = specials(row_dtype(precision))
    return sp[rng.integers(0, len(sp), size=shape)]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _bank(sd, W, rank, precision, variant=0, hist=None, channels=CH):
    b = sd.rank_filter_bank(channels, W, rank, sd.F64 if precision == "f64" else sd.F32)
    b.set_variant(variant)
    if hist is not None and W > 1:
        b.set_history(_as_tensor(hist))
    return b


def _as_tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _check(b, y, want, tag):
    """y: the device result; want = the reference's (y, history)"""
    got_y, got_h = _np(y), _np(b.history())
    assert got_y.shape == want[0].shape and got_h.shape == want[1].shape, (tag, got_y.shape, got_h.shape)
    assert _same(got_y, want[0]), (tag, "y", int((got_y.view(np.uint8) != want[0].view(np.uint8)).sum()))
    assert _same(got_h, want[1]), (tag, "history")
    assert _same(_np(b.state), want[1].reshape(-1)), (tag, "state")


def _lengths(W, block):
    """0, 1, W - 2, and one, two and three staging blocks +- 1"""
    out = {0, 1, max(W - 2, 0)}
    for m in (1, 2, 3):
        out |= {m * block - 1, m * block, m * block + 1}
    return sorted(out)


@pytest.mark.parametrize("window,precision", [(W, p) for W in WINDOWS for p in ("f32", "f64") if p == "f32" or W <= 127])
def test_bit_exact_against_reference(sd, torch_cuda, window, precision):
    """ranks 0, (W - 1) // 2, W - 1 and a seeded interior one; both variants; non-zero history; every row length at which the staging
    takes another path"""
    W = window
    rng = np.random.default_rng(7919 * W + len(precision))
    ranks = sorted({0, (W - 1) // 2, W - 1, int(rng.integers(0, W))})
    block = _bank(sd, W, 0, precision).info()["block"]
    assert block >= 1
    lengths = _lengths(W, block)
    top = max(lengths) + (-max(lengths)) % 4  # rows that start on 16-byte boundaries: the whole-block lengths take the aligned paths
    x = _rand(rng, (CH, top), precision)
    h0 = _rand(rng, (CH, W - 1), precision)
    xd = _dev(torch_cuda, x)
    for r in ranks:
        for S in lengths:
            want = rank_ref(x[:, :S], W, r, h0)
            for variant in (0, 1):
                b = _bank(sd, W, r, precision, variant, h0)
                y = b.process(xd, samples=S)
                _check(b, y, want, (precision, W, r, S, variant))


def test_f64_windows_end_at_127(sd, torch_cuda):
    with pytest.raises(ValueError):
        sd.rank_filter_bank(CH, 128, 0, sd.F64)
    assert sd.rank_filter_bank(CH, 127, "median", sd.F64).info()["padded"] == 128
    assert [sd.rank_filter_bank(2, W, 0).info()["padded"] for W in (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255)] == \
        [8, 8, 16, 16, 32, 32, 64, 64, 128, 128, 256, 256]


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("window", [5, 16, 63])
def test_ties_and_specials(sd, torch_cuda, window, precision):
    """rows drawn from twenty special bit patterns: nearly every window holds duplicates, both zeros, NaNs of both signs and the two
    patterns whose keys equal a sentinel's"""
    W = window
    rng = np.random.default_rng(100 + W)
    block = _bank(sd, W, 0, precision).info()["block"]
    S = 3 * block + 5
    x = _special_rows(rng, (CH, S), precision)
    h0 = _special_rows(rng, (CH, W - 1), precision)
    xd = _dev(torch_cuda, x)
    for r in sorted({0, 1, (W - 1) // 2, W - 2, W - 1}):
        want = rank_ref(x, W, r, h0)
        for variant in (0, 1):
            b = _bank(sd, W, r, precision, variant, h0)
            _check(b, b.process(xd), want, (precision, W, r, variant))


@pytest.mark.parametrize("precision,window,rank", [("f32", 5, 2), ("f32", 33, 0), ("f64", 16, 15), ("f64", 64, 20)])
def test_any_split_gives_the_same_bits(sd, torch_cuda, precision, window, rank):
    """ragged calls (0, 1, W - 2, a block +- 1, the rest) equal one call: outputs and final state"""
    W = window
    rng = np.random.default_rng(29 + W)
    block = _bank(sd, W, rank, precision).info()["block"]
    blocks = [0, 1, max(W - 2, 0), block - 1, 0, block + 1, 2 * block + 3]
    S = sum(blocks)
    x = _special_rows(rng, (CH, S), precision)
    h0 = _special_rows(rng, (CH, W - 1), precision)
    want = rank_ref(x, W, rank, h0)
    assert _same(rank_ref_stream(x, W, rank, blocks, h0)[0], want[0])
    starts = np.cumsum([0] + blocks[:-1])
    for variant in (0, 1):
        b = _bank(sd, W, rank, precision, variant, h0)
        parts = [b.process(_dev(torch_cuda, x[:, s0:s0 + n].copy())) for s0, n in zip(starts, blocks)]
        _check(b, torch_cuda.cat(parts, dim=1), want, (variant, "split"))
        one = _bank(sd, W, rank, precision, variant, h0)
        _check(one, one.process(_dev(torch_cuda, x)), want, (variant, "unsplit"))


@pytest.mark.parametrize("precision,window,rank", [("f32", 7, 3), ("f32", 40, 39), ("f64", 17, 0)])
def test_the_run_length_does_not_change_the_bits(sd, torch_cuda, precision, window, rank):
    """3 rows of 5000 samples: runs start inside rows, inside the history and at ragged ends; every run gives variant 1's bits"""
    W, S, C_ = window, 5000, 3
    rng = np.random.default_rng(31 + W)
    x = _special_rows(rng, (C_, S), precision)
    x[:, ::3] = _rand(rng, (C_, S), precision)[:, ::3]
    h0 = _special_rows(rng, (C_, W - 1), precision)
    xd = _dev(torch_cuda, x)
    plain = _bank(sd, W, rank, precision, 1, h0, channels=C_)
    ref = plain.process(xd)
    want = rank_ref(x, W, rank, h0)
    _check(plain, ref, want, "plain")
    for run in (0, 1, W - 1, W, 64, 100, S):
        b = _bank(sd, W, rank, precision, 0, h0, channels=C_)
        b.set_run(run)
        assert b.info()["run"] == run
        y = b.process(xd)
        assert arena.same_bits(y, ref), run
        _check(b, y, want, run)
        assert b.info()["last_run"] == run if run else 4 * W <= b.info()["last_run"] <= S
    b.set_run(0)
    assert b.info()["run"] == 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, precision):
    """x, y and state carved 0, 1 or 2 elements past a 512-byte boundary out of NaN-filled (and pattern-filled) arenas, row strides of
    their own above S: the interior has the aligned run's bits and nothing outside it is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(35)
    W, rank = 9, 4
    ref = _bank(sd, W, rank, precision)
    S = 2 * ref.info()["block"] + 9
    assert S % 4 == 1
    x = _rand(rng, (CH, S), precision)
    h0 = _rand(rng, (CH, W - 1), precision)
    ref.set_history(_as_tensor(h0))
    cy = ref.process(_dev(torch, x))
    _check(ref, cy, rank_ref(x, W, rank, h0), "aligned")
    start = _dev(torch, h0).flatten()
    for variant in (0, 1):
        b = _bank(sd, W, rank, precision, variant)
        # strides S + 5 and S + 7: rows start anywhere; lead 0 with strides S + 7 and S + 3 (multiples of four elements, S = 4 k + 1):
        # every row starts on a 16-byte boundary, so the blocks inside the rows take the whole-chunk accesses
        for lead, px, py in ((0, 5, 7), (1, 5, 7), (2, 5, 7), (0, 7, 3)):
            for fill in arena.fills(cy.dtype):
                (ax, vx), (ay, vy) = [arena.framed(torch, (CH, S), cy.dtype, lead, 64, fill, row_stride=S + pad) for pad in (px, py)]
                ast, vst = arena.framed(torch, (start.numel(),), cy.dtype, lead, 64, fill)
                vx[:, :S].copy_(_dev(torch, x))
                vst.copy_(start)
                arenas = [ax, ay, ast]
                before = [arena.bits(a).clone() for a in arenas]
                assert lib.sdsp_hip_rank_process(b._plan, vx.data_ptr(), S + px, vy.data_ptr(), S + py, S, vst.data_ptr(), None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, px, fill)
                assert arena.same_bits(vy[:, :S], cy), tag
                assert arena.same_bits(vst, ref.state), tag
                arena.assert_frame_untouched(before[0], ax, slice(0, 0))  # x is never written
                arena.assert_frame_untouched(before[1], ay, arena.interior_mask(torch, ay, vy, S))
                arena.assert_frame_untouched(before[2], ast, arena.interior_mask(torch, ast, vst))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("window,rank", [(5, 2), (16, 0), (33, 32)])
def test_a_nan_reaches_exactly_its_window(sd, torch_cuda, window, rank, variant):
    """a NaN of each sign at (c, n): no output outside row c, n .. n + W - 1 changes"""
    W = window
    rng = np.random.default_rng(37)
    S = 3 * _bank(sd, W, rank, "f32").info()["block"] + 21
    x = _rand(rng, (CH, S), "f32")
    clean = _np(_bank(sd, W, rank, "f32", variant).process(_dev(torch_cuda, x)))
    xp = x.copy()
    places = [(63, 11, 0x7FC00000), (64, 17, 0xFFC00001)]  # a wave's last lane, the next wave's first
    for c, n, pattern in places:
        xp.view(np.uint32)[c, n] = pattern
    want = rank_ref(xp, W, rank)
    b = _bank(sd, W, rank, "f32", variant)
    got = _np(b.process(_dev(torch_cuda, xp)))
    assert _same(got, want[0])
    untouched = np.ones((CH, S), dtype=bool)
    for c, n, _ in places:
        untouched[c, n:n + W] = False
    assert _same(got[untouched], clean[untouched])


@pytest.mark.parametrize("precision,sizes", [("f32", (3, 5, 31, 255)), ("f64", (3, 5, 31, 127))])
def test_scipy_parity(sd, torch_cuda, precision, sizes):
    """medfilt equals scipy.signal.medfilt by value on finite rows; the bank with +-inf history equals minimum_filter1d /
    maximum_filter1d"""
    import scipy.ndimage
    import scipy.signal
    rng = np.random.default_rng(41)
    C_, S = 5, 301
    x = _rand(rng, (C_, S), precision)
    xd = _dev(torch_cuda, x)
    for k in sizes:
        got = _np(sd.medfilt(xd, k))
        assert got.shape == x.shape
        for c in range(C_):
            assert np.array_equal(got[c], scipy.signal.medfilt(x[c], k)), (k, c)
        assert np.array_equal(_np(sd.medfilt(xd[0], k)), scipy.signal.medfilt(x[0], k))
        for rank, fn, fill in (("min", scipy.ndimage.minimum_filter1d, np.inf), ("max", scipy.ndimage.maximum_filter1d, -np.inf)):
            b = _bank(sd, k, rank, precision, 0, np.full((C_, k - 1), fill, dtype=x.dtype), channels=C_)
            want = fn(x, k, axis=1, mode="constant", cval=fill, origin=(k - 1) // 2)
            assert np.array_equal(_np(b.process(xd)), want), (k, rank)


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    """three calls (a block multiple, a ragged one, a short one) captured into one graph replay to the eager bits"""
    torch = torch_cuda
    rng = np.random.default_rng(39)
    W, rank = 15, 7
    sizes = [64, 37, 7]
    S = sum(sizes)
    x = _special_rows(rng, (CH, S), "f32")
    want = rank_ref(x, W, rank)
    xs = [_dev(torch, x[:, s0:s0 + n].copy()) for s0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    ys = [torch.empty((CH, n), dtype=torch.float32, device="cuda") for n in sizes]
    b = _bank(sd, W, rank, "f32")
    run = lambda: [b.process(xs[i], y=ys[i]) for i in range(3)]  # noqa: E731
    run()  # the state exists before capture
    _check(b, torch.cat(ys, dim=1).clone(), want, "eager")
    b.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    b.reset()
    for t in ys:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    _check(b, torch.cat(ys, dim=1), want, "replay")


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(43)
    W, rank, S = 16, 5, 90
    x = _special_rows(rng, (CH, S), "f64")
    h0 = _special_rows(rng, (CH, W - 1), "f64")
    b = _bank(sd, W, rank, "f64", 0, h0)
    y = b.process(_dev(torch_cuda, x))
    st, oy = h0.copy().reshape(-1), np.zeros_like(x)
    assert lib.sdsp_hip_rank_process_host(b._plan, x.ctypes.data, S, oy.ctypes.data, S, S, st.ctypes.data) == 0
    assert _same(oy, _np(y)) and _same(st, _np(b.state))
    oy2 = np.zeros_like(x)
    assert lib.sdsp_hip_rank_process_host(b._plan, x.ctypes.data, S, oy2.ctypes.data, S, S, None) == 0  # no state: zero history
    assert _same(oy2, rank_ref(x, W, rank)[0])


def test_info_error_codes_and_launch_count(sd, torch_cuda):
    torch = torch_cuda
    lib = sd.load()
    L = sd._lib
    b = _bank(sd, 31, "median", "f32")
    info = b.info()
    assert (info["channels"], info["window"], info["rank"], info["padded"], info["out_index"]) == (CH, 31, 15, 32, 15)
    assert (info["precision"], info["variant"], info["run"], info["last_run"], info["kernel"]) == (sd.F32, 0, 0, 0, "sdsp_rank_kernel")
    assert info["block"] == 16 and info["lds_bytes"] == (2 * 16 + 4) * 65 * 4 + 512 and info["departing"] == 0
    i64 = _bank(sd, 31, "median", "f64").info()
    assert i64["block"] == 8 and i64["lds_bytes"] == (2 * 8 + 2) * 65 * 8 + 512
    assert b.state_bytes() == CH * 30 * 4 and b.history().shape == (CH, 30)
    assert b.launches(100) == 2 and b.launches(0) == 0
    assert _bank(sd, 1, 0, "f32").launches(100) == 1  # no history to carry
    b.set_variant(1)
    assert b.info()["kernel"] == "sdsp_rank_plain_kernel" and b.info()["variant"] == 1
    p = _bank(sd, 16, 3, "f32", channels=2)
    x, y = torch.zeros((2, 64), device="cuda"), torch.zeros((2, 64), device="cuda")
    X, Y = x.data_ptr(), y.data_ptr()

    def run(x=X, xs=64, y=Y, ys=64, n=64, state=None):
        return lib.sdsp_hip_rank_process(p._plan, x, xs, y, ys, n, state, None)

    assert run() == 0
    assert run(x=None) == L.ERR_INVALID_ARG and run(y=None) == L.ERR_INVALID_ARG
    assert run(xs=60) == L.ERR_INVALID_ARG and run(ys=63) == L.ERR_INVALID_ARG
    assert run(y=X + 8 * 4) == L.ERR_INVALID_ARG  # overlaps
    assert run(x=X + 2, n=32) == L.ERR_INVALID_ARG  # misaligned
    assert run(n=1 << 31) == L.ERR_INVALID_SIZE
    assert run(n=0) == 0
    assert lib.sdsp_hip_rank_plan_set_variant(p._plan, 2) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_rank_plan_set_run(p._plan, 1 << 31) == L.ERR_INVALID_SIZE
    # a grid that does not fit one launch: 2^30 rows of 2^20 one-sample runs.  The refusal comes before any launch, so the two
    # disjoint address ranges are never touched
    big = _bank(sd, 3, 1, "f32", channels=1 << 30)
    big.set_run(1)
    assert lib.sdsp_hip_rank_process(big._plan, 1 << 12, 1 << 20, (1 << 12) + (1 << 53), 1 << 20, 1 << 20, None, None) == L.ERR_UNSUPPORTED
    assert b"too large for one launch" in lib.sdsp_hip_last_error_string()
    # a call of S = 0 leaves the state alone
    st = torch.full((2 * 15,), 3.0, device="cuda")
    assert run(n=0, state=st.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((st == 3.0).all())
