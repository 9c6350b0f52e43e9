"""GPU tests of the carrier-recovery PLL / Costas loop bank (sdsp_hip_pll_*) on a real MI355X.

The checker is tests/pll_ref.py, the contract's operation order in numpy, itself checked in tests/test_pll_host.py.  Both precisions,
the three detectors and both kernel variants are held to bit-exact agreement with it: y, err, freq and the final state."""
import numpy as np
import pytest

import arena
from pll_ref import (BLOCKS, LOCK_CHANNELS, MODES, lock_signal, pll_ref, pll_ref_stream, real_dtype, row_dtype)

pytestmark = pytest.mark.gpu

CH = 133  # two full waves and a ragged one
ALPHA, BETA, MAX_DEV = 0.05, 0.002, 0.25


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


def _words(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _bank(sd, fcw, precision, mode, variant=0, integ=None, theta=None, channels=CH, max_dev=MAX_DEV):
    b = sd.pll_bank(channels, fcw, mode, sd.F64 if precision == "f64" else sd.F32, max_dev)
    b.set_variant(variant)
    if integ is not None:
        b.set_freq(integ)
    if theta is not None:
        b.set_phase(theta)
    return b


def _state(b):
    return _np(b.freq()), _np(b.phase()).view(np.uint32)


def _check(b, got, want, tag):
    """got = (y, err, freq) device tensors (None = left out), want = the reference's (y, err, freq, integ, theta)"""
    for name, g, w in zip(("y", "err", "freq"), got, want):
        if g is not None:
            h = _np(g)
            assert h.shape == w.shape, (tag, name, h.shape, w.shape)
            assert _same(h, w), (tag, name, int((h != w).sum()))
    integ, theta = _state(b)
    assert _same(integ, want[3]), (tag, "integ")
    assert _same(theta, want[4]), (tag, "theta")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_bit_exact_against_reference(sd, torch_cuda, precision, mode):
    """both variants from a non-zero state (random theta, integ within +-max_dev); rows of two blocks and a ragged tail (the block
    length is the plan's), S = 1 and S = 0; all outputs, and each single output alone"""
    rng = np.random.default_rng(7919 + len(mode) + len(precision))
    fcw, th0 = _words(rng, CH), _words(rng, CH)
    i0 = rng.uniform(-MAX_DEV, MAX_DEV, CH).astype(real_dtype(precision))
    block = _bank(sd, fcw, precision, mode).info()["block"]
    assert block >= 1
    for S in (2 * block + 37, 1, 0):
        pad = S + 4 + (-S) % 4
        x = _rand(rng, (CH, pad), precision)
        want = pll_ref(x[:, :S], fcw, ALPHA, BETA, mode, MAX_DEV, i0, th0, precision)
        if S > 1:
            assert np.abs(want[2]).max() > 0 and (want[4] != th0).all()
        for variant in (0, 1):
            for wants in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
                b = _bank(sd, fcw, precision, mode, variant, i0, th0)
                got = b.process(_dev(torch_cuda, x), ALPHA, BETA, samples=S, want_y=wants[0], want_err=wants[1], want_freq=wants[2])
                assert [g is not None for g in got] == list(wants)
                _check(b, got, want, (precision, mode, variant, S, wants))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_edges_of_the_contract(sd, torch_cuda, precision):
    """theta wraps (fcw0 = 0xffffffff and 0x80000000 with negative k); a channel scaled by 1e6 saturates t at both clamps; a small max_dev
    clamps the integrator at both signs; -0 components in QPSK mode"""
    rng = np.random.default_rng(11)
    dt = real_dtype(precision)
    S = 150
    fcw = _words(rng, CH)
    fcw[0::2], fcw[1::4] = 0xffffffff, 0x80000000
    th0 = _words(rng, CH)
    th0[:8] = [0, 1, 0xffffffff, 0x80000000, 0x7fffffff, 5, 0xfffffc00, 0x3ff]
    x = _rand(rng, (CH, S), precision)
    x[3::5] *= 1e6  # v 2^32 far outside int32 on both sides
    n = np.arange(S)
    x.real[7, ::3] = np.where(n[::3] % 2 == 0, -0.0, 0.0)  # (+-0, im)
    x.imag[8, ::2] = np.where(n[::2] % 4 == 0, -0.0, 0.0)  # (re, +-0)
    x.real[9, :], x.imag[9, :] = np.where(n % 2 == 0, -0.0, 0.0), np.where(n % 3 == 0, -0.0, 0.0)  # every pair of signed zeros
    assert np.signbit(x.real[9, 0]) and np.signbit(x.imag[9, 0]) and not np.signbit(x.real[9, 1]) and x[9, 0] == 0
    for mode in MODES:
        for max_dev in (0.25, 1e-4):
            want = pll_ref(x, fcw, 0.3, 0.05, mode, max_dev, None, th0, precision)
            f = want[2]
            if max_dev == 1e-4:  # the integrator sits on both rails somewhere
                assert (f == dt(max_dev)).any() and (f == -dt(max_dev)).any(), mode
            for variant in (0, 1):
                b = _bank(sd, fcw, precision, mode, variant, None, th0, max_dev=max_dev)
                got = b.process(_dev(torch_cuda, x), 0.3, 0.05)
                _check(b, got, want, (precision, mode, variant, max_dev))
    # the reference itself saw both clamps of t on the scaled channels, and negative k
    y, err, freq, _, _ = pll_ref(x, fcw, 0.3, 0.05, "cross", 0.25, None, th0, precision)
    t = (dt(0.3) * err.astype(np.float64) + freq.astype(np.float64)) * 2.0 ** 32
    assert (t[3::5] > 2.0 ** 31).any() and (t[3::5] < -2.0 ** 31).any() and (t < 0).any()


@pytest.mark.parametrize("variant", [0, 1])
def test_zero_gains_leave_the_oscillator_at_its_centre_word(sd, torch_cuda, variant):
    rng = np.random.default_rng(13)
    S = 77
    fcw, th0 = _words(rng, CH), _words(rng, CH)
    x = _rand(rng, (CH, S), "f32")
    for mode in MODES:
        b = _bank(sd, fcw, "f32", mode, variant, None, th0)
        got = b.process(_dev(torch_cuda, x), 0.0, 0.0)
        integ, theta = _state(b)
        assert np.array_equal(theta, ((th0.astype(np.int64) + S * fcw.astype(np.int64)) & 0xffffffff).astype(np.uint32))
        assert not integ.any() and not _np(got[2]).any()
        _check(b, got, pll_ref(x, fcw, 0.0, 0.0, mode, MAX_DEV, None, th0, "f32"), (mode, variant))


@pytest.mark.parametrize("precision,mode", [("f32", "qpsk"), ("f64", "bpsk"), ("f32", "cross")])
def test_any_split_gives_the_same_bits(sd, torch_cuda, precision, mode):
    """lms_ref.py's BLOCKS pattern (empty calls included) in units of 13 samples, with gains changing from call to call (zero for one
    of them) against the reference fed the same way; with constant gains also against the unsplit run"""
    rng = np.random.default_rng(29)
    blocks = [13 * v for v in BLOCKS]
    S = sum(blocks)
    fcw = _words(rng, CH)
    x = _rand(rng, (CH, S), precision)
    starts = np.cumsum([0] + blocks[:-1])
    for scale in ([1, 1, 0.5, 1, 0, 1, 0.25], [1] * len(blocks)):
        calls = [(n, ALPHA * s, BETA * s) for n, s in zip(blocks, scale)]
        want = pll_ref_stream(x, fcw, calls, mode, MAX_DEV, None, None, precision)
        for variant in (0, 1):
            b = _bank(sd, fcw, precision, mode, variant)
            parts = [b.process(_dev(torch_cuda, x[:, s0:s0 + n].copy()), al, be) for s0, (n, al, be) in zip(starts, calls)]
            got = tuple(torch_cuda.cat([p[i] for p in parts], dim=1) for i in range(3))
            _check(b, got, want, (variant, scale[2]))
    one = _bank(sd, fcw, precision, mode)
    _check(one, one.process(_dev(torch_cuda, x), ALPHA, BETA), want, "unsplit")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_in_place_and_null_state(sd, torch_cuda, precision, variant):
    """y = x (the same pointer and stride) gives the out-of-place bits; state NULL = a zero-filled one, nothing kept"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(33)
    fcw = _words(rng, CH)
    ref = _bank(sd, fcw, precision, "qpsk", variant)
    S = 2 * ref.info()["block"] + 9
    x = _rand(rng, (CH, S), precision)
    xd = _dev(torch, x)
    y, err, freq = ref.process(xd, ALPHA, BETA)
    _check(ref, (y, err, freq), pll_ref(x, fcw, ALPHA, BETA, "qpsk", MAX_DEV, None, None, precision), variant)
    assert arena.same_bits(xd, _dev(torch, x))  # x is not written out of place
    b = _bank(sd, fcw, precision, "qpsk", variant)
    buf = xd.clone()
    y2, err2, freq2 = b.process(buf, ALPHA, BETA, y=buf)
    assert y2.data_ptr() == buf.data_ptr()
    assert arena.same_bits(buf, y) and arena.same_bits(err2, err) and arena.same_bits(freq2, freq)
    assert torch.equal(b.state, ref.state)  # bytes
    oy, oe, of = torch.zeros_like(y), torch.zeros_like(err), torch.zeros_like(freq)
    assert lib.sdsp_hip_pll_process(ref._plan, xd.data_ptr(), S, oy.data_ptr(), S, oe.data_ptr(), S, of.data_ptr(), S, S, ALPHA, BETA, None,
                                    None) == 0
    torch.cuda.synchronize()
    assert arena.same_bits(oy, y) and arena.same_bits(oe, err) and arena.same_bits(of, freq)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, precision):
    """x, y, err, freq and state carved 0, 1 or 2 elements past a 512-byte boundary out of NaN-filled (and pattern-filled) arenas, padded
    row strides of their own: the interior has the aligned run's bits and nothing outside it is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(35)
    mode = "bpsk"
    fcw, th0 = _words(rng, CH), _words(rng, CH)
    i0 = rng.uniform(-MAX_DEV, MAX_DEV, CH).astype(real_dtype(precision))
    ref = _bank(sd, fcw, precision, mode, 0, i0, th0)
    S = ref.info()["block"] + 9
    x = _rand(rng, (CH, S), precision)
    cy, ce, cf = ref.process(_dev(torch, x), ALPHA, BETA)
    _check(ref, (cy, ce, cf), pll_ref(x, fcw, ALPHA, BETA, mode, MAX_DEV, i0, th0, precision), "aligned")
    start_bytes = _bank(sd, fcw, precision, mode, 0, i0, th0).state.clone()  # the state the aligned run began with
    rs = 8 if precision == "f64" else 4
    for variant in (0, 1):
        b = _bank(sd, fcw, precision, mode, variant)
        for lead in (0, 1, 2):
            for fill in arena.fills(cy.dtype):
                (ax, vx), (ay, vy) = [arena.framed(torch, (CH, S), cy.dtype, lead, 64, fill, row_stride=S + pad) for pad in (5, 7)]
                (ae, ve), (af, vf) = [arena.framed(torch, (CH, S), ce.dtype, lead, 64, fill.real if isinstance(fill, complex) else fill,
                                                   row_stride=S + pad) for pad in (3, 1)]
                # the state: an arena of reals with the view `lead` reals in; it holds channels reals and channels words
                words = (start_bytes.numel() + rs - 1) // rs
                ast, vst = arena.framed(torch, (words,), ce.dtype, lead, 64, 7.0)
                vst.view(torch.uint8)[:start_bytes.numel()].copy_(start_bytes)
                vx[:, :S].copy_(_dev(torch, x))
                arenas = [ax, ay, ae, af, ast]
                before = [arena.bits(a).clone() for a in arenas]
                state_before = vst.view(torch.uint8).clone()
                assert lib.sdsp_hip_pll_process(b._plan, vx.data_ptr(), S + 5, vy.data_ptr(), S + 7, ve.data_ptr(), S + 3, vf.data_ptr(),
                                                S + 1, S, ALPHA, BETA, vst.data_ptr(), None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, fill)
                assert arena.same_bits(vy[:, :S], cy) and arena.same_bits(ve[:, :S], ce) and arena.same_bits(vf[:, :S], cf), tag
                got_state = vst.view(torch.uint8)
                assert torch.equal(got_state[:start_bytes.numel()], ref.state), tag
                assert torch.equal(got_state[start_bytes.numel():], state_before[start_bytes.numel():]), tag  # the tail past the words
                arena.assert_frame_untouched(before[0], ax, slice(0, 0))  # x is never written
                arena.assert_frame_untouched(before[1], ay, arena.interior_mask(torch, ay, vy, S))
                arena.assert_frame_untouched(before[2], ae, arena.interior_mask(torch, ae, ve, S))
                arena.assert_frame_untouched(before[3], af, arena.interior_mask(torch, af, vf, S))
                arena.assert_frame_untouched(before[4], ast, arena.interior_mask(torch, ast, vst))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_nan_reaches_exactly_its_channel(sd, torch_cuda, mode, variant):
    """a NaN in x of channel 63 (a wave's last lane) and one in channel 64 (the next wave's first): y and err of that sample and the
    integrator from that sample on are NaN, exactly where the reference's are; theta goes on at fcw0, so the later y and err are those
    of the open loop; every other channel keeps the clean run's bits"""
    rng = np.random.default_rng(37)
    fcw = _words(rng, CH)
    S = _bank(sd, fcw, "f32", mode).info()["block"] + 21
    x = _rand(rng, (CH, S), "f32")
    clean_bank = _bank(sd, fcw, "f32", mode, variant)
    clean = clean_bank.process(_dev(torch_cuda, x), ALPHA, BETA)
    xp = x.copy()
    xp[63, 11] = complex(np.nan, 1.0)
    xp[64, 17] = complex(0.5, np.nan)
    want = pll_ref(xp, fcw, ALPHA, BETA, mode, MAX_DEV, None, None, "f32")
    for c, n in ((63, 11), (64, 17)):
        for w in want[:2]:  # y and err: that sample alone
            assert np.isnan(w[c, n]).all() and not np.isnan(np.delete(w[c], n)).any()
        assert not np.isnan(want[2][c, :n]).any() and np.isnan(want[2][c, n:]).all()  # freq: from that sample on
    b = _bank(sd, fcw, "f32", mode, variant)
    got = b.process(_dev(torch_cuda, xp), ALPHA, BETA)
    have = tuple(_np(g) for g in got) + _state(b)
    clean_np = tuple(_np(g) for g in clean) + _state(clean_bank)
    others = np.ones(CH, dtype=bool)
    others[[63, 64]] = False
    for name, h, w, c in zip(("y", "err", "freq", "integ", "theta"), have, want, clean_np):
        if h.dtype.kind != "u":
            assert np.array_equal(np.isnan(h), np.isnan(w)), name
            assert _same(h[~np.isnan(h)], w[~np.isnan(w)]), name
        else:
            assert _same(h, w), name  # theta is an integer: the poisoned channels go on at fcw0
        assert _same(h[others], c[others]), name
    assert np.isnan(have[3][[63, 64]]).all()


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    """three calls (a block multiple, a ragged one, a short one) captured into one graph replay to the eager bits"""
    torch = torch_cuda
    rng = np.random.default_rng(39)
    mode = "qpsk"
    sizes = [64, 37, 7]
    S = sum(sizes)
    fcw = _words(rng, CH)
    x = _rand(rng, (CH, S), "f32")
    want = pll_ref(x, fcw, ALPHA, BETA, mode, MAX_DEV, None, None, "f32")
    xs = [_dev(torch, x[:, s0:s0 + n].copy()) for s0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    ys = [torch.empty((CH, n), dtype=torch.complex64, device="cuda") for n in sizes]
    es = [torch.empty((CH, n), dtype=torch.float32, device="cuda") for n in sizes]
    fs = [torch.empty((CH, n), dtype=torch.float32, device="cuda") for n in sizes]
    b = _bank(sd, fcw, "f32", mode)
    run = lambda: [b.process(xs[i], ALPHA, BETA, y=ys[i], err=es[i], freq=fs[i]) for i in range(3)]  # noqa: E731
    run()  # the state exists before capture
    cat = lambda: tuple(torch.cat(t, dim=1).clone() for t in (ys, es, fs))  # noqa: E731
    _check(b, cat(), want, "eager")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    b.reset()
    for t in ys + es + fs:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    _check(b, cat(), want, "replay")


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(41)
    S = 90
    for precision, mode in (("f64", "qpsk"), ("f32", "cross")):
        dt = real_dtype(precision)
        fcw, th0 = _words(rng, CH), _words(rng, CH)
        i0 = rng.uniform(-MAX_DEV, MAX_DEV, CH).astype(dt)
        x = _rand(rng, (CH, S), precision)
        b = _bank(sd, fcw, precision, mode, 0, i0, th0)
        y, err, freq = b.process(_dev(torch_cuda, x), ALPHA, BETA)
        st = np.concatenate([i0.view(np.uint8), th0.view(np.uint8)])
        oy, oe, of = np.zeros_like(x), np.zeros((CH, S), dtype=dt), np.zeros((CH, S), dtype=dt)
        assert lib.sdsp_hip_pll_process_host(b._plan, x.ctypes.data, S, oy.ctypes.data, S, oe.ctypes.data, S, of.ctypes.data, S, S, ALPHA,
                                             BETA, st.ctypes.data) == 0
        assert _same(oy, _np(y)) and _same(oe, _np(err)) and _same(of, _np(freq)) and _same(st, _np(b.state))
        # y alone, without state
        oy2 = np.zeros_like(x)
        assert lib.sdsp_hip_pll_process_host(b._plan, x.ctypes.data, S, oy2.ctypes.data, S, None, 0, None, 0, S, ALPHA, BETA, None) == 0
        assert _same(oy2, pll_ref(x, fcw, ALPHA, BETA, mode, MAX_DEV, None, None, precision)[0])


def test_info_error_codes_and_launch_count(sd, torch_cuda):
    torch = torch_cuda
    lib = sd.load()
    L = sd._lib
    for precision, rs in (("f32", 4), ("f64", 8)):
        b = _bank(sd, 0x1999999a, precision, "bpsk")  # one shared word
        info = b.info()
        assert (info["channels"], info["mode"], info["precision"]) == (CH, sd.PLL_BPSK, sd.F64 if precision == "f64" else sd.F32)
        assert info["kernel"] == "sdsp_pll_kernel" and info["variant"] == 0
        assert info["max_dev"] == float(real_dtype(precision)(MAX_DEV))
        assert info["block"] >= 1 and (info["block"] * 2 * rs) % 16 == 0 and (info["block"] * rs) % 16 == 0
        assert info["lds_bytes"] == 2 * 2048 * 2 * rs + info["waves"] * info["block"] * 65 * 4 * rs <= 160 * 1024
        assert b.state_bytes() == CH * (rs + 4)
        assert b.freq().shape == (CH,) and b.phase().shape == (CH,)
        assert b.freq().data_ptr() == b.state.data_ptr() and b.phase().data_ptr() == b.state.data_ptr() + CH * rs
        assert b.launches(100) == 1 and b.launches(0) == 0
        b.set_variant(1)
        assert b.info()["kernel"] == "sdsp_pll_plain_kernel" and b.info()["variant"] == 1
        # the shared word serves every channel
        x = _rand(np.random.default_rng(5), (CH, 40), precision)
        _check(b, b.process(_dev(torch, x), ALPHA, BETA), pll_ref(x, np.uint32(0x1999999a), ALPHA, BETA, "bpsk", MAX_DEV, None, None,
                                                                precision), precision)
        b.reset()
        assert not _state(b)[0].any() and not _state(b)[1].any()
    p = _bank(sd, 5, "f32", "cross", channels=2)
    x, y = torch.zeros((2, 64), dtype=torch.complex64, device="cuda"), torch.zeros((2, 64), dtype=torch.complex64, device="cuda")
    e, f = torch.zeros((2, 64), device="cuda"), torch.zeros((2, 64), device="cuda")
    X, Y, E, F = (t.data_ptr() for t in (x, y, e, f))

    def run(x=X, xs=64, y=Y, ys=64, e=E, es=64, f=F, fs=64, n=64, alpha=0.01, beta=0.001, state=None):
        return lib.sdsp_hip_pll_process(p._plan, x, xs, y, ys, e, es, f, fs, n, alpha, beta, state, None)

    assert run() == 0
    assert run(x=None) == L.ERR_INVALID_ARG
    assert run(y=None) == 0 and run(e=None) == 0 and run(f=None) == 0 and run(y=None, e=None, f=None) == 0
    assert run(y=X) == 0  # in place
    assert run(y=X, ys=65) == L.ERR_INVALID_ARG and run(y=X + 8, n=32) == L.ERR_INVALID_ARG  # overlaps that are not in place
    assert run(xs=60) == L.ERR_INVALID_ARG and run(ys=63) == L.ERR_INVALID_ARG
    assert run(es=63) == L.ERR_INVALID_ARG and run(fs=63) == L.ERR_INVALID_ARG
    assert run(e=X) == L.ERR_INVALID_ARG and run(f=Y + 4) == L.ERR_INVALID_ARG and run(f=E) == L.ERR_INVALID_ARG  # overlaps
    assert run(state=E) == L.ERR_INVALID_ARG and run(state=X + 64) == L.ERR_INVALID_ARG and run(state=Y) == L.ERR_INVALID_ARG  # state
    assert run(x=X + 4, n=32) == L.ERR_INVALID_ARG and run(e=E + 2, n=32) == L.ERR_INVALID_ARG  # misaligned
    assert run(alpha=float("nan")) == L.ERR_INVALID_ARG and run(beta=1e300) == L.ERR_INVALID_ARG
    assert run(n=1 << 31) == L.ERR_INVALID_SIZE
    assert run(n=0) == 0 and run(x=None, n=0) == 0
    assert lib.sdsp_hip_pll_plan_set_variant(p._plan, 2) == L.ERR_INVALID_ARG
    # a call of S = 0 leaves the state alone
    st = torch.full((4,), 3.0, device="cuda")
    assert run(n=0, state=st.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((st == 3.0).all())


@pytest.mark.parametrize("mode", MODES)
def test_the_lock_signals_in_f32_equal_the_reference(sd, torch_cuda, mode):
    """the signals of tests/test_pll_host.py's lock test through the device in f32: the same bits as the reference, so what that test
    shows of the reference (frequency and phase within its bounds) holds for the GPU without a second tolerance"""
    for bn in (0.01, 0.02):
        x, _, _ = lock_signal(mode, bn)
        alpha, beta = sd.pll_gains(bn, mode=mode)
        fcw = np.uint32(round(0.1 * 2 ** 32))
        want = pll_ref(x, fcw, alpha, beta, mode, 0.5, None, None, "f32")
        for variant in (0, 1):
            b = _bank(sd, fcw, "f32", mode, variant, channels=LOCK_CHANNELS, max_dev=0.5)
            _check(b, b.process(_dev(torch_cuda, x.astype(np.complex64)), alpha, beta), want, (bn, variant))
