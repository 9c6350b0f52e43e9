"""GPU tests of the symbol-timing recovery bank (sdsp_hip_timing_*) on a real MI355X.

The checker is tests/timing_ref.py, the contract's operation order in numpy, itself checked in tests/test_timing_host.py.  Both
precisions, the three detectors and both kernel variants are held to bit-exact agreement with it: every channel's count, its symbols,
err and period up to that count, and the final state."""
import ctypes as C

import numpy as np
import pytest

import arena
from timing_ref import (BLOCKS, LOCK_CHANNELS, LOCK_ROLLOFF, MODES, design, detector_slope, gains, lock_shape, lock_signal, max_out,
                        real_dtype, row_dtype, rows_of, state_bytes_of, step_of, timing_ref, timing_ref_stream)

pytestmark = pytest.mark.gpu

CH = 133  # two full waves and a ragged one
SHAPES = [(1, 1), (4, 5), (32, 16), (128, 32), (32, 64)]  # (L, T)
SPS = [2, 2.37, 8]
ALPHA, BETA, MAX_DEV = 0.3, 0.05, 0.25
SENTINEL = -77.0


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


def _rand(rng, shape, precision, scale=1.0):
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    return (scale * x).astype(row_dtype(precision))


def _taps(rng, L, T):
    return rng.standard_normal(L * T) / T


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _bank(sd, torch, h, L, sps, precision, mode, variant=0, state=None, channels=CH, max_dev=MAX_DEV):
    b = sd.timing_bank(channels, sps, h, L, mode, sd.F64 if precision == "f64" else sd.F32, max_dev)
    b.set_variant(variant)
    if state is not None:
        raw = np.frombuffer(state_bytes_of(state), dtype=np.uint8)
        assert raw.size == b.state_bytes()
        b._ensure_state().copy_(torch.from_numpy(raw.copy()))
    return b


def _state(b):
    return _np(b._ensure_state()).tobytes()


def _check(b, got, want, tag, state=True):
    """got = (y, err, period, counts) device tensors (None = left out), want = the reference's (y, err, period, counts, state, ..)"""
    counts = _np(got[3]).view(np.uint32)
    assert _same(counts, want[3]), (tag, "counts", counts[:8], want[3][:8])
    for name, g, w in zip(("y", "err", "period"), got[:3], want[:3]):
        if g is not None:
            h = _np(g)
            assert h.shape[1] >= w.shape[1], (tag, name, h.shape, w.shape)
            for c, (a, r) in enumerate(zip(rows_of(h, counts), rows_of(w, counts))):
                assert _same(a, r), (tag, name, "channel", c, int((a != r).sum()))
    if state:
        assert _state(b) == state_bytes_of(want[4]), (tag, "state")


def _start_state(rng, h, L, T, step0, mode, precision):
    """a state that is not zero: the reference after 9 samples"""
    return timing_ref(h, L, T, _rand(rng, (CH, 9), precision), step0, ALPHA, BETA, mode, MAX_DEV, None, precision)[4]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_bit_exact_against_reference(sd, torch_cuda, precision, mode):
    """both variants, every (L, T) and samples per symbol, from a state that is not zero; rows of five blocks and a ragged tail (the
    block length is the plan's), so the ring of block + T - 1 rows wraps; every fifth channel is scaled by 1e6, which drives w to both
    clamps and integ to +-max_dev on those channels only: the counts differ between the lanes of one wave.  All outputs, y alone,
    and S = 1 and S = 0"""
    rng = np.random.default_rng(7919 + len(mode) + len(precision))
    dt = real_dtype(precision)
    for L, T in SHAPES:
        h = _taps(rng, L, T)
        for sps in SPS:
            step0 = step_of(sps)
            st0 = _start_state(rng, h, L, T, step0, mode, precision)
            block = _bank(sd, torch_cuda, h, L, sps, precision, mode).info()["block"]
            for S in ((5 * block + 37, 1, 0) if (L, T, sps) == (4, 5, 2.37) else (5 * block + 37,)):
                x = _rand(rng, (CH, S + 3), precision)
                x[3::5] *= 1e6
                want = timing_ref(h, L, T, x[:, :S], step0, ALPHA, BETA, mode, MAX_DEV, st0, precision)
                if S > 1:
                    q = (dt(ALPHA) * want[1].astype(np.float64) + want[2].astype(np.float64)) * 2.0 ** 32
                    assert (q[3::5] > 2.0 ** 31).any() and (q[3::5] < -2.0 ** 31).any(), (L, T, sps)
                    assert (want[2][3::5] == dt(MAX_DEV)).any() and (want[2][3::5] == -dt(MAX_DEV)).any()
                    assert len(set(want[3][:64].tolist())) > 1  # counts differ inside the first wave
                for variant in (0, 1):
                    for wants in ((True, True), (False, False)):
                        b = _bank(sd, torch_cuda, h, L, sps, precision, mode, variant, st0)
                        got = b.process(_dev(torch_cuda, x), ALPHA, BETA, samples=S, want_err=wants[0], want_period=wants[1])
                        assert [g is not None for g in got[1:3]] == list(wants)
                        assert got[0].shape == (CH, max_out(step0, S)) == (CH, b.max_out(S))
                        _check(b, got, want, (precision, mode, L, T, sps, variant, S, wants))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_edges_of_the_contract(sd, torch_cuda, precision):
    """a small max_dev clamps the integrator at both signs; rows of signed zeros under the sign detectors (L = T = 1 with a unit tap:
    every strobe is a sample itself, -0 included); the largest and the smallest step word"""
    rng = np.random.default_rng(11)
    dt = real_dtype(precision)
    S = 150
    one = np.ones(1)
    x = _rand(rng, (CH, S), precision)
    n = np.arange(S)
    x.real[7, :] = np.where(n % 3 == 0, -0.0, 0.0)
    x.imag[8, :] = np.where(n % 2 == 0, -0.0, 0.0)
    x.real[9, :], x.imag[9, :] = np.where(n % 2 == 0, -0.0, 0.0), np.where(n % 3 == 0, -0.0, 0.0)  # every pair of signed zeros
    assert np.signbit(x.real[7, 0]) and not np.signbit(x.real[7, 1]) and x[9, 0] == 0
    for mode in MODES:
        for max_dev in (0.25, 1e-4):
            want = timing_ref(one, 1, 1, x, 1 << 32, 0.0, 0.05, mode, max_dev, None, precision)
            if max_dev == 1e-4:
                assert (want[2] == dt(max_dev)).any() and (want[2] == -dt(max_dev)).any(), mode
            for variant in (0, 1):
                b = _bank(sd, torch_cuda, one, 1, 2, precision, mode, variant, max_dev=max_dev)
                _check(b, b.process(_dev(torch_cuda, x), 0.0, 0.05, want_err=True, want_period=True), want, (mode, variant, max_dev))
    h = _taps(rng, 4, 5)
    for sps in (2, 128):
        want = timing_ref(h, 4, 5, x, step_of(sps), ALPHA, BETA, "gardner", MAX_DEV, None, precision)
        for variant in (0, 1):
            b = _bank(sd, torch_cuda, h, 4, sps, precision, "gardner", variant)
            _check(b, b.process(_dev(torch_cuda, x), ALPHA, BETA, want_err=True, want_period=True), want, (sps, variant))


@pytest.mark.parametrize("precision,mode,shape,sps", [("f32", "gardner", (32, 64), 2.37), ("f64", "zc_qpsk", (32, 16), 2),
                                                      ("f32", "zc_bpsk", (4, 5), 8), ("f64", "gardner", (128, 32), 2.37)])
def test_any_split_gives_the_same_bits(sd, torch_cuda, precision, mode, shape, sps):
    """lms_ref.py's BLOCKS pattern in units of the plan's block with ragged ends, empty and one-sample calls included, with gains
    changing from call to call (zero for one of them) against the reference fed the same way; with constant gains also against the
    unsplit run"""
    rng = np.random.default_rng(29)
    L, T = shape
    h = _taps(rng, L, T)
    step0 = step_of(sps)
    block = _bank(sd, torch_cuda, h, L, sps, precision, mode).info()["block"]
    ragged = [0, 0, 5, 0, 0, 1, -3]
    blocks = [v * block + r for v, r in zip(BLOCKS, ragged)]
    blocks[1] = 1  # a call of one sample
    assert blocks[0] == 0 and blocks[3] == 0
    S = sum(blocks)
    x = _rand(rng, (CH, S), precision)
    x[3::5] *= 1e3
    starts = np.cumsum([0] + blocks[:-1])
    for scale in ([1, 1, 0.5, 1, 0, 1, 0.25], [1] * len(blocks)):
        calls = [(n, ALPHA * s, BETA * s) for n, s in zip(blocks, scale)]
        want = timing_ref_stream(h, L, T, x, step0, calls, mode, MAX_DEV, None, precision)
        for variant in (0, 1):
            b = _bank(sd, torch_cuda, h, L, sps, precision, mode, variant)
            rows = [[[] for _ in range(CH)] for _ in range(3)]
            for s0, (n, al, be) in zip(starts, calls):
                got = b.process(_dev(torch_cuda, x[:, s0:s0 + n].copy()), al, be, want_err=True, want_period=True)
                cnt = _np(got[3])
                if n == 0:
                    assert not cnt.any()
                for k in range(3):
                    part = _np(got[k])
                    for c in range(CH):
                        rows[k][c].append(part[c, :cnt[c]])
            for k, name in enumerate(("y", "err", "period")):
                for c in range(CH):
                    assert _same(np.concatenate(rows[k][c]), want[k][c]), (variant, scale[2], name, c)
            assert _state(b) == state_bytes_of(want[4]), (variant, scale[2])
    one = _bank(sd, torch_cuda, h, L, sps, precision, mode)
    got = one.process(_dev(torch_cuda, x), ALPHA, BETA, want_err=True, want_period=True)
    cnt = _np(got[3]).view(np.uint32)
    assert _same(cnt, want[3])
    for k in range(3):
        for c, row in enumerate(rows_of(_np(got[k]), cnt)):
            assert _same(row, want[k][c]), ("unsplit", k, c)
    assert _state(one) == state_bytes_of(want[4])


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_zero_gains_equal_the_nearest_phase_resampler(sd, torch_cuda, precision, variant):
    """alpha = beta = 0 free-runs at step0: the symbol strobes are every second output (the odd ones) of arb_resampler in nearest mode
    with the same table at that step, bit for bit"""
    torch = torch_cuda
    rng = np.random.default_rng(13)
    prec = sd.F64 if precision == "f64" else sd.F32
    S = 211
    for (L, T), sps in zip(SHAPES, (2, 2.37, 8, 2.37, 2)):
        h = _taps(rng, L, T)
        step0 = step_of(sps)
        xd = _dev(torch, _rand(rng, (CH, S), precision))
        arb = sd.arb_resampler(L, T, step0, kind="complex", interp="nearest", precision=prec)
        arb.set_coeff(h)
        arb.step = step0
        open_loop = arb.process(xd)
        for mode in MODES:
            b = _bank(sd, torch, h, L, sps, precision, mode, variant)
            y, _, period, counts = b.process(xd, 0.0, 0.0, want_period=True)
            n = open_loop.shape[1] // 2
            assert bool((counts == n).all())
            assert arena.same_bits(y[:, :n], open_loop[:, 1::2].contiguous()), (L, T, sps, mode)
            assert not bool(period[:, :n].any()) and not bool(b.period().any())
            assert bool((b.time() == arb.time).all())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_null_state_null_outputs_and_rows_past_their_counts(sd, torch_cuda, precision, variant):
    """state NULL = a zero-filled one, nothing kept; err and period NULL are not written; with y_stride exactly max_out(S) and every
    buffer filled with a sentinel, each row holds its count of symbols and the sentinel behind them"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(33)
    L, T, sps = 32, 16, 2.37
    h = _taps(rng, L, T)
    step0 = step_of(sps)
    b = _bank(sd, torch, h, L, sps, precision, "gardner", variant)
    S = 3 * b.info()["block"] + 9
    cap = b.max_out(S)
    x = _rand(rng, (CH, S), precision)
    x[3::5] *= 1e6
    want = timing_ref(h, L, T, x, step0, ALPHA, BETA, "gardner", MAX_DEV, None, precision)
    assert want[3].min() < want[3].max() <= cap
    xd = _dev(torch, x)
    ct, rt = (torch.complex128, torch.float64) if precision == "f64" else (torch.complex64, torch.float32)
    for with_reals in (True, False):
        y = torch.full((CH, cap), complex(SENTINEL, SENTINEL), dtype=ct, device="cuda")
        e, p = torch.full((CH, cap), SENTINEL, dtype=rt, device="cuda"), torch.full((CH, cap), SENTINEL, dtype=rt, device="cuda")
        cnt = torch.full((CH,), -1, dtype=torch.int32, device="cuda")
        assert lib.sdsp_hip_timing_process(b._plan, xd.data_ptr(), S, y.data_ptr(), cap, e.data_ptr() if with_reals else None, cap,
                                           p.data_ptr() if with_reals else None, cap, cnt.data_ptr(), S, ALPHA, BETA, None, None) == 0
        torch.cuda.synchronize()
        _check(b, (y, e if with_reals else None, p if with_reals else None, cnt), want, (variant, with_reals), state=False)
        counts = _np(cnt)
        behind = np.arange(cap)[None, :] >= counts[:, None]
        assert behind.any()
        yn, en, pn = _np(y), _np(e), _np(p)
        assert (yn[behind] == complex(SENTINEL, SENTINEL)).all()
        if with_reals:
            assert (en[behind] == SENTINEL).all() and (pn[behind] == SENTINEL).all()
        else:
            assert (en == SENTINEL).all() and (pn == SENTINEL).all()
    assert b.state() is None  # nothing was kept, and the second call started from zero again
    assert arena.same_bits(xd, _dev(torch, x))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, precision):
    """x, y, err, period, counts and state carved 0, 1 or 2 elements past a 512-byte boundary out of NaN-filled (and pattern-filled)
    arenas (the state: 8-byte steps, its alignment), padded row strides of their own: every row has the aligned run's bits up to its
    count and nothing else is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(35)
    mode, (L, T), sps = "zc_qpsk", (4, 5), 2.37
    h = _taps(rng, L, T)
    step0 = step_of(sps)
    st0 = _start_state(rng, h, L, T, step0, mode, precision)
    ref = _bank(sd, torch, h, L, sps, precision, mode, 0, st0)
    S = ref.info()["block"] + 9
    cap = ref.max_out(S)
    x = _rand(rng, (CH, S), precision)
    x[3::5] *= 1e6
    want = timing_ref(h, L, T, x, step0, ALPHA, BETA, mode, MAX_DEV, st0, precision)
    cy, ce, cp, cc = ref.process(_dev(torch, x), ALPHA, BETA, want_err=True, want_period=True)
    _check(ref, (cy, ce, cp, cc), want, "aligned")
    counts = _np(cc)
    written = torch.from_numpy(np.arange(cap)[None, :] < counts[:, None]).cuda()
    start = np.frombuffer(state_bytes_of(st0), dtype=np.uint8).copy()
    for variant in (0, 1):
        b = _bank(sd, torch, h, L, sps, precision, mode, variant)
        for lead in (0, 1, 2):
            for fill in arena.fills(cy.dtype):
                rfill = fill.real if isinstance(fill, complex) else fill
                (ax, vx), (ay, vy) = [arena.framed(torch, (CH, n), cy.dtype, lead, 64, fill, row_stride=n + pad) for n, pad in ((S, 5), (cap, 7))]
                (ae, ve), (ap, vp) = [arena.framed(torch, (CH, cap), ce.dtype, lead, 64, rfill, row_stride=cap + pad) for pad in (3, 1)]
                ac, vc = arena.framed(torch, (CH,), torch.int32, lead, 64, 7)
                ast, vst = arena.framed(torch, (start.size // 8,), torch.float64, lead, 64, 7.0)
                vst.view(torch.uint8).copy_(torch.from_numpy(start))
                vx[:, :S].copy_(_dev(torch, x))
                arenas = [ax, ay, ae, ap, ac, ast]
                before = [arena.bits(a).clone() for a in arenas]
                assert lib.sdsp_hip_timing_process(b._plan, vx.data_ptr(), S + 5, vy.data_ptr(), cap + 7, ve.data_ptr(), cap + 3, vp.data_ptr(),
                                                   cap + 1, vc.data_ptr(), S, ALPHA, BETA, vst.data_ptr(), None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, fill)
                assert torch.equal(vc, cc), tag
                for v, c in ((vy, cy), (ve, ce), (vp, cp)):
                    assert arena.same_bits(v[:, :cap][written], c[written]), tag
                assert _np(vst.view(torch.uint8)).tobytes() == state_bytes_of(want[4]), tag
                arena.assert_frame_untouched(before[0], ax, slice(0, 0))  # x is never written
                for i, (a, v) in enumerate(((ay, vy), (ae, ve), (ap, vp))):
                    mask = arena.interior_mask(torch, a, v, cap)
                    inner = mask[(v.data_ptr() - a.data_ptr()) // a.element_size():][:v.numel()].view(v.shape)
                    inner[:, :cap] &= written  # behind a row's count nothing is written either
                    arena.assert_frame_untouched(before[1 + i], a, mask)
                arena.assert_frame_untouched(before[4], ac, arena.interior_mask(torch, ac, vc))
                arena.assert_frame_untouched(before[5], ast, arena.interior_mask(torch, ast, vst))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_nan_reaches_exactly_its_channel(sd, torch_cuda, mode, variant):
    """a NaN in x of channel 63 (a wave's last lane) and one in channel 64 (the next wave's first): the strobes whose windows hold it
    and the integrator from the first such symbol on are NaN, exactly where the reference's are; the time goes on at step0, so the
    channel's count is the open loop's; every other channel keeps the clean run's bits"""
    rng = np.random.default_rng(37)
    L, T, sps = 4, 5, 2.37
    h = _taps(rng, L, T)
    step0 = step_of(sps)
    S = _bank(sd, torch_cuda, h, L, sps, "f32", mode).info()["block"] * 3 + 21
    x = _rand(rng, (CH, S), "f32")
    clean_bank = _bank(sd, torch_cuda, h, L, sps, "f32", mode, variant)
    clean = clean_bank.process(_dev(torch_cuda, x), ALPHA, BETA, want_err=True, want_period=True)
    xp = x.copy()
    xp[63, 11] = complex(np.nan, 1.0)
    xp[64, 17] = complex(np.nan, np.nan)  # the real part too: zc_bpsk reads nothing else in its detector
    want = timing_ref(h, L, T, xp, step0, ALPHA, BETA, mode, MAX_DEV, None, "f32")
    for c in (63, 64):
        n = want[3][c]
        bad = np.isnan(want[2][c, :n])
        assert bad.any() and not bad[0] and bad[np.argmax(bad):].all()  # period: from the first poisoned symbol on
        assert np.isnan(want[0][c, :n]).any() and not np.isnan(want[0][c, n - 3:n]).any()  # y: the windows that hold the NaN only
        assert np.isnan(want[4]["integ"][c])
    b = _bank(sd, torch_cuda, h, L, sps, "f32", mode, variant)
    got = b.process(_dev(torch_cuda, xp), ALPHA, BETA, want_err=True, want_period=True)
    counts = _np(got[3]).view(np.uint32)
    assert _same(counts, want[3])
    others = np.ones(CH, dtype=bool)
    others[[63, 64]] = False
    for name, g, w, c in zip(("y", "err", "period"), got[:3], want[:3], clean[:3]):
        hv, cv = _np(g), _np(c)
        for ch in range(CH):
            a, r = hv[ch, :counts[ch]], w[ch, :counts[ch]]
            assert np.array_equal(np.isnan(a), np.isnan(r)), (name, ch)
            assert _same(a[~np.isnan(a)], r[~np.isnan(r)]), (name, ch)
            if others[ch]:
                assert _same(a, cv[ch, :counts[ch]]), (name, ch)
    assert _same(counts[others], _np(clean[3]).view(np.uint32)[others])
    # the state: the time of every channel is the reference's, the poisoned integrators are NaN, the others are the clean run's
    assert _same(_np(b.time()).view(np.uint64), want[4]["t"])
    integ, clean_integ = _np(b.period()), _np(clean_bank.period())
    assert np.isnan(integ[[63, 64]]).all() and _same(integ[others], clean_integ[others])


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    """three calls (a block multiple, a ragged one, a short one) captured into one graph replay to the eager bits"""
    torch = torch_cuda
    rng = np.random.default_rng(39)
    mode, (L, T), sps = "gardner", (32, 16), 2.37
    h = _taps(rng, L, T)
    step0 = step_of(sps)
    sizes = [64, 37, 7]
    S = sum(sizes)
    x = _rand(rng, (CH, S), "f32")
    calls = [(n, ALPHA, BETA) for n in sizes]
    want = timing_ref_stream(h, L, T, x, step0, calls, mode, MAX_DEV, None, "f32")
    b = _bank(sd, torch, h, L, sps, "f32", mode)
    xs = [_dev(torch, x[:, s0:s0 + n].copy()) for s0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    caps = [b.max_out(n) for n in sizes]
    ys = [torch.zeros((CH, n), dtype=torch.complex64, device="cuda") for n in caps]
    es = [torch.zeros((CH, n), dtype=torch.float32, device="cuda") for n in caps]
    ps = [torch.zeros((CH, n), dtype=torch.float32, device="cuda") for n in caps]
    cs = [torch.zeros((CH,), dtype=torch.int32, device="cuda") for _ in caps]
    run = lambda: [b.process(xs[i], ALPHA, BETA, y=ys[i], err=es[i], period=ps[i], counts=cs[i]) for i in range(3)]  # noqa: E731

    def check(tag):
        torch.cuda.synchronize()
        cnt = [_np(c) for c in cs]
        for k, bufs in enumerate((ys, es, ps)):
            parts = [_np(t) for t in bufs]
            for c in range(CH):
                row = np.concatenate([parts[i][c, :cnt[i][c]] for i in range(3)])
                assert _same(row, want[k][c]), (tag, k, c)
        assert _state(b) == state_bytes_of(want[4]), tag

    run()  # the state exists before capture
    check("eager")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    b.reset()
    for t in ys + es + ps + cs:
        t.zero_()
    g.replay()
    check("replay")


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(41)
    S = 90
    for precision, mode, (L, T), sps in (("f64", "zc_qpsk", (4, 5), 2.37), ("f32", "gardner", (32, 16), 2)):
        dt = real_dtype(precision)
        h = _taps(rng, L, T)
        step0 = step_of(sps)
        st0 = _start_state(rng, h, L, T, step0, mode, precision)
        x = _rand(rng, (CH, S), precision)
        b = _bank(sd, torch_cuda, h, L, sps, precision, mode, 0, st0)
        got = b.process(_dev(torch_cuda, x), ALPHA, BETA, want_err=True, want_period=True)
        cap = b.max_out(S)
        counts = _np(got[3])
        st = np.frombuffer(state_bytes_of(st0), dtype=np.uint8).copy()
        oy, oe, op = np.zeros((CH, cap), dtype=x.dtype), np.zeros((CH, cap), dtype=dt), np.zeros((CH, cap), dtype=dt)
        oc = np.zeros(CH, dtype=np.int32)
        assert lib.sdsp_hip_timing_process_host(b._plan, x.ctypes.data, S, oy.ctypes.data, cap, oe.ctypes.data, cap, op.ctypes.data, cap,
                                                oc.ctypes.data, S, ALPHA, BETA, st.ctypes.data) == 0
        assert _same(oc, counts) and st.tobytes() == _state(b)
        for o, g in ((oy, got[0]), (oe, got[1]), (op, got[2])):
            for a, r in zip(rows_of(o, counts), rows_of(_np(g), counts)):
                assert _same(a, r)
        # y alone, without state
        oy2, oc2 = np.zeros((CH, cap), dtype=x.dtype), np.zeros(CH, dtype=np.int32)
        assert lib.sdsp_hip_timing_process_host(b._plan, x.ctypes.data, S, oy2.ctypes.data, cap, None, 0, None, 0, oc2.ctypes.data, S, ALPHA,
                                                BETA, None) == 0
        want = timing_ref(h, L, T, x, step0, ALPHA, BETA, mode, MAX_DEV, None, precision)
        assert _same(oc2.view(np.uint32), want[3])
        for a, r in zip(rows_of(oy2, oc2), rows_of(want[0], oc2)):
            assert _same(a, r)
        # an empty call zeroes the counts
        oc2[:] = 5
        assert lib.sdsp_hip_timing_process_host(b._plan, None, 0, None, 0, None, 0, None, 0, oc2.ctypes.data, 0, ALPHA, BETA, None) == 0
        assert not oc2.any()


def test_info_error_codes_and_launch_count(sd, torch_cuda):
    torch = torch_cuda
    lib = sd.load()
    Lm = sd._lib
    rng = np.random.default_rng(43)
    for precision, rs in (("f32", 4), ("f64", 8)):
        for L, T in SHAPES:
            h = _taps(rng, L, T)
            b = _bank(sd, torch, h, L, 2.37, precision, "zc_bpsk")
            info = b.info()
            assert (info["channels"], info["mode"], info["precision"]) == (CH, sd.TIMING_ZC_BPSK, sd.F64 if precision == "f64" else sd.F32)
            assert (info["phases"], info["taps"], info["step0"]) == (L, T, step_of(2.37)) and b.step0 == sd.timing_step(2.37) == step_of(2.37)
            assert info["kernel"] == "sdsp_timing_kernel" and info["variant"] == 0
            assert info["max_dev"] == float(real_dtype(precision)(MAX_DEV))
            assert info["block"] >= 1 and (info["block"] * 2 * rs) % 16 == 0
            pitch = T | 1 if L > 1 else T
            up16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
            table, ring = up16(L * pitch * rs), up16((info["block"] + T - 1) * 65 * 2 * rs)
            assert 1 <= info["waves"] <= 4 and info["waves"] == min(4, (160 * 1024 - table) // ring)
            assert info["lds_bytes"] == table + info["waves"] * ring <= 160 * 1024
            up8 = lambda v: (v + 7) // 8 * 8  # noqa: E731
            assert b.state_bytes() == (8 * CH + 2 * up8(2 * rs * CH) + up8(rs * CH) + 2 * up8(4 * CH) + up8(2 * rs * CH * (T - 1)))
            assert b.period().shape == (CH,) and b.time().shape == (CH,) and b.time().data_ptr() == b.state().data_ptr()
            assert b.launches(100) == 1 and b.launches(0) == 0
            b.set_variant(1)
            assert b.info()["kernel"] == "sdsp_timing_plain_kernel" and b.info()["variant"] == 1
            b.reset()
            assert not bool(b.state().any())
    assert b.info()["waves"] < 4  # (32, 64) in f64: the rings of four waves do not fit
    h = _taps(rng, 4, 5)
    p = _bank(sd, torch, h, 4, 4, "f32", "gardner", channels=2)
    cap = p.max_out(64)
    assert cap == max_out(step_of(4), 64) == 22
    x, y = torch.zeros((2, 64), dtype=torch.complex64, device="cuda"), torch.zeros((2, 64), dtype=torch.complex64, device="cuda")
    e, f = torch.zeros((2, 64), device="cuda"), torch.zeros((2, 64), device="cuda")
    cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    state = torch.zeros((p.state_bytes(),), dtype=torch.uint8, device="cuda")
    X, Y, E, F, N, ST = (t.data_ptr() for t in (x, y, e, f, cnt, state))

    def run(x=X, xs=64, y=Y, ys=64, e=E, es=64, f=F, fs=64, c=N, n=64, alpha=0.01, beta=0.001, state=None):
        return lib.sdsp_hip_timing_process(p._plan, x, xs, y, ys, e, es, f, fs, c, n, alpha, beta, state, None)

    assert run() == 0 and run(state=ST) == 0
    assert run(x=None) == Lm.ERR_INVALID_ARG and run(y=None) == Lm.ERR_INVALID_ARG and run(c=None) == Lm.ERR_INVALID_ARG
    assert run(e=None) == 0 and run(f=None) == 0 and run(e=None, f=None) == 0
    assert run(ys=cap) == 0 and run(es=cap) == 0 and run(fs=cap) == 0
    assert run(xs=60) == Lm.ERR_INVALID_ARG and run(ys=cap - 1) == Lm.ERR_INVALID_ARG  # short strides
    assert run(es=cap - 1) == Lm.ERR_INVALID_ARG and run(fs=cap - 1) == Lm.ERR_INVALID_ARG
    assert run(y=X) == Lm.ERR_INVALID_ARG and run(y=X + 8 * 100, ys=cap) == Lm.ERR_INVALID_ARG  # y overlaps x
    assert run(e=X) == Lm.ERR_INVALID_ARG and run(f=Y + 4) == Lm.ERR_INVALID_ARG and run(f=E) == Lm.ERR_INVALID_ARG
    assert run(c=E) == Lm.ERR_INVALID_ARG and run(state=Y) == Lm.ERR_INVALID_ARG and run(state=N) == Lm.ERR_INVALID_ARG
    assert run(x=X + 4, n=32) == Lm.ERR_INVALID_ARG and run(e=E + 2, n=32) == Lm.ERR_INVALID_ARG  # misaligned
    assert run(state=ST + 4) == Lm.ERR_INVALID_ARG and run(c=N + 2) == Lm.ERR_INVALID_ARG
    assert run(alpha=float("nan")) == Lm.ERR_INVALID_ARG and run(beta=1e300) == Lm.ERR_INVALID_ARG
    assert run(n=1 << 31) == Lm.ERR_INVALID_SIZE
    assert lib.sdsp_hip_timing_plan_set_variant(p._plan, 2) == Lm.ERR_INVALID_ARG
    # a call of S = 0 zeroes the counts and leaves the state alone
    cnt.fill_(9)
    state.fill_(3)
    assert run(n=0, state=ST) == 0 and run(x=None, y=None, n=0, state=ST) == 0
    torch.cuda.synchronize()
    assert not bool(cnt.any()) and bool((state == 3).all())
    # plan creation: bad L, T, step0 and max_dev
    q = C.c_void_p()
    hp = np.ones(4096)

    def create(phases=4, taps=5, step0=1 << 33, max_dev=0.25):
        return lib.sdsp_hip_timing_plan_create(C.byref(q), 2, Lm.F32, 0, phases, taps, hp.ctypes.data, step0, max_dev, 0)

    assert create(phases=3) == Lm.ERR_INVALID_SIZE and create(phases=256) == Lm.ERR_INVALID_SIZE
    assert create(taps=0) == Lm.ERR_INVALID_SIZE and create(taps=65) == Lm.ERR_INVALID_SIZE and create(phases=128, taps=33) == Lm.ERR_INVALID_SIZE
    assert create(step0=(1 << 32) - 1) == Lm.ERR_INVALID_SIZE and create(step0=(1 << 38) + 1) == Lm.ERR_INVALID_SIZE
    assert create(max_dev=0.0) == Lm.ERR_INVALID_ARG and create(max_dev=0.51) == Lm.ERR_INVALID_ARG
    assert create(phases=128, taps=32, step0=1 << 38, max_dev=0.5) == 0
    assert lib.sdsp_hip_timing_plan_destroy(q) == 0


_KD = {}


@pytest.mark.parametrize("mode", MODES)
def test_the_lock_signals_in_f32_equal_the_reference(sd, torch_cuda, mode):
    """signals of tests/test_timing_host.py's lock test through the device in f32: the same bits as the reference, so what that test
    shows of the reference (period and symbols within its bounds) holds for the GPU without a second tolerance.  The figures
    themselves are asserted on the host only"""
    for sps, delta, bn in ((2, 200e-6, 0.01), (4, -200e-6, 0.005)):
        L, T = lock_shape(sps)
        h = design(L, T, sps, LOCK_ROLLOFF)
        if (mode, sps) not in _KD:
            _KD[mode, sps] = detector_slope(mode, sps, L, T, h)
        x = lock_signal(mode, sps, delta)[0][:, :1500 * sps // 2]  # the first 750 symbols: the acquisition and the start of the tail
        alpha, beta = gains(bn, np.sqrt(0.5), _KD[mode, sps], sps)
        assert (alpha, beta) == sd.timing_gains(bn, np.sqrt(0.5), _KD[mode, sps], sps)
        want = timing_ref(h, L, T, x, step_of(sps), alpha, beta, mode, 0.5, None, "f32")
        for variant in (0, 1):
            b = _bank(sd, torch_cuda, h, L, sps, "f32", mode, variant, channels=LOCK_CHANNELS, max_dev=0.5)
            got = b.process(_dev(torch_cuda, x.astype(np.complex64)), alpha, beta, want_err=True, want_period=True)
            _check(b, got, want, (sps, delta, bn, variant))
