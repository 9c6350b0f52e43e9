"""GPU tests of the FFT-domain (overlap-save) FIR plan -- sdsp_hip_fir_fft_plan_create, DESIGN.md section 5.9.

The checker is the CPU oracle's direct-form FIR in double (oracle.fir_process), run on the x and h the plan actually sees
(rounded to f32 for f32 plans).  The metric is conftest.rel_max_err per channel: f64 <= 1e-12, f32 <= 1e-5 (the fused
convolution measured 2.5e-7 per f32 transform, profiles/r03_accuracy.md; the overlap-save output of a frame pair is one such
transform).  Unlike the direct plan, block-by-block streaming is NOT bit-identical to one long call: the frame grid starts
afresh at every call, so the same output sample comes out of a different frame and rounds differently -- streaming is held
to the same tolerance.  Everything that does not go through the convolution is exact: the history a call leaves behind is
the last T-1 inputs bit for bit, and slicing (the plan's workspace budget) does not change a single bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_max_err

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-12, "f32": 1e-5}


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


def _prec(sd, precision):
    return (sd.F64, np.float64) if precision == "f64" else (sd.F32, np.float32)


def _bank(sd, taps, channels, precision, h, state=None, **kw):
    prec, _ = _prec(sd, precision)
    bank = sd.fft_fir_filter(taps, channels, prec, **kw)
    bank.set_coeff(h)
    if state is not None:
        import torch
        bank._state = torch.from_numpy(np.ascontiguousarray(state)).cuda()
    return bank


def _run(torch, bank, x, **kw):
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    bank.process(d, **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def _seen(h, x, state, precision):
    """h, x and history as the plan holds them, in double"""
    npdt = np.float64 if precision == "f64" else np.float32
    return (h.astype(npdt).astype(np.float64), x.astype(npdt).astype(np.float64), state.astype(npdt).astype(np.float64))


def _check(oracle, h, x, state, got, got_state, precision):
    hs, xs, ss = _seen(h, x, state, precision)
    for c in range(x.shape[0]):
        want, want_state = oracle.fir_process(hs, xs[c], ss[c] if h.size > 1 else None)
        err = rel_max_err(got[c], want)
        assert err <= TOL[precision], (c, err)
        if h.size > 1:
            assert np.array_equal(got_state[c].astype(np.float64), want_state), c  # the last T-1 inputs, exactly


def _pow2_at_least(v):
    n = 16
    while n < v:
        n *= 2
    return n


def _cases():
    out = []
    for precision, taps_list in (("f64", [1, 2, 17, 255, 1000, 4096, 8192]), ("f32", [1, 64, 1000, 4097, 16384])):
        for taps in taps_list:
            for shape in [(1, 100000), (67, 1000), (5, 15), (3, max(1, (taps - 1) // 2))]:
                for fft_n in ("auto", "min"):
                    out.append((precision, taps, shape, fft_n))
    return out


@pytest.mark.parametrize("precision,taps,shape,fft_n", _cases())
def test_accuracy_and_state_against_oracle(sd, torch_cuda, oracle, precision, taps, shape, fft_n):
    """random h, x and starting history; the last shape is samples < T-1 (old history shifts into the new one)"""
    channels, samples = shape
    _, npdt = _prec(sd, precision)
    rng = np.random.default_rng(taps * 7 + channels * 13 + samples)
    h = rng.standard_normal(taps) / np.sqrt(taps)
    x = rng.standard_normal((channels, samples)).astype(npdt)
    state = rng.standard_normal((channels, max(taps - 1, 1))).astype(npdt)
    n = 0 if fft_n == "auto" else _pow2_at_least(2 * (taps - 1))
    bank = _bank(sd, taps, channels, precision, h, state, fft_n=n)
    got = _run(torch_cuda, bank, x)
    info = bank.info()
    assert info["method"] == sd.FIR_FFT and info["taps"] == taps
    assert info["fft_n"] == (n or sd.fir_fft_size(taps, _prec(sd, precision)[0])) and info["hop"] == info["fft_n"] - taps + 1
    _check(oracle, h, x, state, got, bank.state.cpu().numpy(), precision)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("taps,fft_n", [(33, 64), (100, 256), (1000, 2048)])
def test_frame_counts_and_row_offsets(sd, torch_cuda, oracle, precision, taps, fft_n):
    """samples at and around multiples of the hop (even and odd frame counts, partial last frame), and a block inside a
    longer row (stride > samples via offset): everything outside the block stays untouched"""
    _, npdt = _prec(sd, precision)
    hop = fft_n - taps + 1
    rng = np.random.default_rng(taps)
    h = rng.standard_normal(taps) / np.sqrt(taps)
    for samples in (hop, 2 * hop, 3 * hop, 2 * hop + 1, 3 * hop - 1, 4 * hop + 7):
        channels, offset, stride = 6, 5, samples + 13
        row = rng.standard_normal((channels, stride)).astype(npdt)
        state = rng.standard_normal((channels, taps - 1)).astype(npdt)
        bank = _bank(sd, taps, channels, precision, h, state, fft_n=fft_n)
        got = _run(torch_cuda, bank, row, samples=samples, offset=offset)
        assert np.array_equal(got[:, :offset], row[:, :offset])
        assert np.array_equal(got[:, offset + samples:], row[:, offset + samples:])
        _check(oracle, h, row[:, offset:offset + samples], state, got[:, offset:offset + samples], bank.state.cpu().numpy(),
               precision)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_preload_and_direct_fft_direct_stream(sd, torch_cuda, oracle, precision):
    """preload_filter's history is honoured; a stream split direct -> FFT -> direct over three blocks (the same state
    buffer handed on) matches the oracle's one long call"""
    torch = torch_cuda
    prec, npdt = _prec(sd, precision)
    taps, channels = 513, 9
    rng = np.random.default_rng(5)
    h = rng.standard_normal(taps) / np.sqrt(taps)
    x = rng.standard_normal((channels, 7000)).astype(npdt)
    bank = _bank(sd, taps, channels, precision, h)
    bank.preload_filter(0.75)
    got = _run(torch, bank, x)
    hs, xs, _ = _seen(h, x, np.zeros(1), precision)
    for c in (0, channels - 1):
        want = oracle.fir_process(hs, xs[c], np.full(taps - 1, 0.75))[0]
        assert rel_max_err(got[c], want) <= TOL[precision]

    direct = sd.fir_filter(taps, channels, prec)
    direct.set_coeff(h)
    fft = _bank(sd, taps, channels, precision, h)
    d = torch.from_numpy(x.copy()).cuda()
    direct.process(d, samples=1500, offset=0)
    fft._state = direct.state
    fft.process(d, samples=4000, offset=1500)
    direct._state = fft.state
    direct.process(d, samples=1500, offset=5500)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    for c in range(channels):
        want, want_state = oracle.fir_process(hs, xs[c])
        assert rel_max_err(got[c], want) <= TOL[precision], c
        assert np.array_equal(direct.state[c].cpu().numpy().astype(np.float64), want_state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_uneven_block_streaming(sd, torch_cuda, oracle, precision):
    """block-by-block calls of uneven lengths (shorter than T-1, shorter than the hop, longer than several frames) against the
    one-long-call oracle, within the tolerance (see the module docstring for why not bit for bit)"""
    _, npdt = _prec(sd, precision)
    taps, channels = 300, 11
    rng = np.random.default_rng(17)
    h = rng.standard_normal(taps) / np.sqrt(taps)
    blocks = [1, 150, 299, 300, 1, 724, 5000, 3, 2047]
    x = rng.standard_normal((channels, sum(blocks))).astype(npdt)
    bank = _bank(sd, taps, channels, precision, h)
    import torch
    d = torch.from_numpy(x.copy()).cuda()
    pos = 0
    for b in blocks:
        bank.process(d, samples=b, offset=pos)
        pos += b
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    hs, xs, _ = _seen(h, x, np.zeros(1), precision)
    for c in range(channels):
        want, want_state = oracle.fir_process(hs, xs[c])
        assert rel_max_err(got[c], want) <= TOL[precision], c
        assert np.array_equal(bank.state[c].cpu().numpy().astype(np.float64), want_state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("taps,fft_n,channels,samples,units", [
    (129, 512, 200, 37, 1),      # many short channels, one pair per slice: every slice ends a channel
    (129, 512, 200, 1500, 3),    # several pairs per channel, slices straddle channels
    (1000, 2048, 1, 50000, 2),   # one channel far longer than the whole workspace: a carry at every slice boundary
    (1000, 2048, 7, 700, 1),     # samples < T-1 with slicing
])
def test_slicing_is_bit_identical(sd, torch_cuda, precision, taps, fft_n, channels, samples, units):
    """a plan whose workspace holds `units` frame pairs gives the same bits -- output and history -- as a default-budget plan of
    the same fft_n.  This is the test of the in-place hazard: a slice's scatter overwrites the T-1 inputs the next slice's
    first frame still needs."""
    _, npdt = _prec(sd, precision)
    rs = 8 if precision == "f64" else 4
    rng = np.random.default_rng(taps + channels)
    h = rng.standard_normal(taps) / np.sqrt(taps)
    x = rng.standard_normal((channels, samples)).astype(npdt)
    state = rng.standard_normal((channels, taps - 1)).astype(npdt)
    ref = _bank(sd, taps, channels, precision, h, state, fft_n=fft_n)
    want = _run(torch_cuda, ref, x)
    tiny = _bank(sd, taps, channels, precision, h, state, fft_n=fft_n, workspace_bytes=units * (2 * fft_n + taps - 1) * rs)
    got = _run(torch_cuda, tiny, x)
    pairs = -(-(-(-samples // (fft_n - taps + 1))) // 2)
    slices = -(-channels * pairs // units)
    assert tiny.launches(samples) >= 3 * slices and slices >= 5
    assert ref.launches(samples) < tiny.launches(samples)
    assert np.array_equal(got, want)
    assert np.array_equal(tiny.state.cpu().numpy(), ref.state.cpu().numpy())


@pytest.mark.parametrize("precision,taps", [("f32", 1000), ("f32", 16384), ("f64", 4096)])
def test_fused_and_three_launch_variants_agree(sd, torch_cuda, oracle, precision, taps):
    _, npdt = _prec(sd, precision)
    rng = np.random.default_rng(taps + 1)
    h = rng.standard_normal(taps) / np.sqrt(taps)
    x = rng.standard_normal((4, 3 * taps + 5)).astype(npdt)
    state = rng.standard_normal((4, taps - 1)).astype(npdt)
    outs, launches = {}, {}
    for variant in (0, 1):
        bank = _bank(sd, taps, 4, precision, h, state)
        bank.set_variant(variant)
        outs[variant] = _run(torch_cuda, bank, x)
        launches[variant] = bank.launches(x.shape[1])
        _check(oracle, h, x, state, outs[variant], bank.state.cpu().numpy(), precision)
    assert launches[1] >= launches[0] + 2  # forward, multiply, reverse instead of one fused launch
    assert rel_max_err(outs[0], outs[1]) <= 2 * TOL[precision]


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_process_is_stream_capturable(sd, torch_cuda, precision):
    """process only enqueues (everything is allocated at creation / set_variant): captured once with a sliced workspace,
    replayed three times, it equals three eager calls bit for bit -- output and history"""
    torch = torch_cuda
    _, npdt = _prec(sd, precision)
    rs = 8 if precision == "f64" else 4
    taps, fft_n, channels, samples = 200, 1024, 40, 3000
    rng = np.random.default_rng(3)
    h = rng.standard_normal(taps) / np.sqrt(taps)
    x = rng.standard_normal((channels, samples)).astype(npdt)
    kw = dict(fft_n=fft_n, workspace_bytes=7 * (2 * fft_n + taps - 1) * rs)
    eager = _bank(sd, taps, channels, precision, h, **kw)
    want = torch.from_numpy(x.copy()).cuda()
    for _ in range(3):
        eager.process(want)
    cap = _bank(sd, taps, channels, precision, h, **kw)
    y = torch.from_numpy(x.copy()).cuda()
    warm = torch.from_numpy(x.copy()).cuda()
    cap.process(warm)  # first call: the plan and the history buffer exist before capture
    cap.reset()
    cap._state = torch.zeros_like(eager.state)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap.process(y)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), x)  # capturing ran nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    assert torch.equal(cap.state, eager.state)


def test_host_entry_info_and_errors(sd, torch_cuda, oracle):
    lib = sd.load()
    rng = np.random.default_rng(9)
    taps, channels, samples = 700, 3, 5000
    h = rng.standard_normal(taps) / np.sqrt(taps)
    x = rng.standard_normal((channels, samples))
    state = rng.standard_normal((channels, taps - 1))
    plan = C.c_void_p()
    sd._lib.check(lib.sdsp_hip_fir_fft_plan_create(C.byref(plan), taps, h.ctypes.data, sd.F64, 0, 0, 0))
    try:
        nbytes = C.c_uint64(0)
        sd._lib.check(lib.sdsp_hip_fir_state_bytes(plan, channels, C.byref(nbytes)))
        assert nbytes.value == channels * (taps - 1) * 8
        data, st = x.copy(), state.copy()
        sd._lib.check(lib.sdsp_hip_fir_process_host(plan, data.ctypes.data, channels, samples, samples, st.ctypes.data))
        _check(oracle, h, x, state, data, st, "f64")
        info = sd._lib.FirPlanInfo()
        sd._lib.check(lib.sdsp_hip_fir_plan_get_info(plan, C.byref(info)))
        assert (info.method, info.taps, info.precision, info.fft_n, info.hop) == (sd.FIR_FFT, taps, sd.F64, 4096, 4096 - taps + 1)
        assert info.kernel.decode() not in ("", "sdsp_fir_kernel") and info.workspace_bytes > 0
    finally:
        lib.sdsp_hip_fir_plan_destroy(plan)

    direct = sd.fir_filter(taps, channels, sd.F64)
    direct.set_coeff(h)
    di = direct.info()
    assert (di["method"], di["fft_n"], di["hop"], di["kernel"]) == (sd.FIR_DIRECT, 0, 0, "sdsp_fir_kernel")
    assert direct.launches(samples) == 1

    def rc(taps, hp, precision, fft_n, out=True):
        p = C.c_void_p()
        r = lib.sdsp_hip_fir_fft_plan_create(C.byref(p) if out else None, taps, hp, precision, fft_n, 0, 0)
        if r == 0:
            lib.sdsp_hip_fir_plan_destroy(p)
        return r

    hb = np.ones(20000)
    hp = hb.ctypes.data
    assert rc(0, hp, sd.F32, 0) == -1
    assert rc(16385, hp, sd.F32, 0) == -1 and rc(8193, hp, sd.F64, 0) == -1
    assert rc(16384, hp, sd.F32, 0) == 0 and rc(8192, hp, sd.F64, 0) == 0
    assert rc(100, hp, sd.F32, 1000) == -1  # not a power of two
    assert rc(100, hp, sd.F32, 128) == -1   # N < 2(T-1)
    assert rc(100, hp, sd.F32, 256) == 0
    assert rc(2, hp, sd.F32, 8) == -2        # below the fused range
    assert rc(100, hp, sd.F32, 65536) == -2 and rc(100, hp, sd.F64, 32768) == -2
    assert rc(100, hp, sd.F32, 32768) == 0 and rc(100, hp, sd.F64, 16384) == 0
    assert rc(100, hp, 7, 0) == -5 and rc(100, None, sd.F32, 0) == -5 and rc(100, hp, sd.F32, 0, out=False) == -5
    # the direct plan is unchanged: still at most SDSP_HIP_FIR_MAX_TAPS
    p = C.c_void_p()
    assert lib.sdsp_hip_fir_plan_create(C.byref(p), 4097, hp, sd.F32, 0) == -1
