"""GPU tests of the carried-state kernels the streaming banks share (stream_carry.hip) on a real MI355X,
through every bank that routes to them and at every element size: the history update (STFT and Welch banks: 4- and 8-byte reals;
complex channelizer: 8- and 16-byte elements) and the pending-sum seed (inverse STFT bank, complex synthesis bank).

Every shape has hist above 256 and not a multiple of 256, so the in-place shifts walk two chunks with a ragged last one, and the blocks
put S (samples of one call) below hist - 256, between hist - 256 and hist, at hist, above it, and at 0.  The kernels only copy: the
state is compared for equality with what was fed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHANNELS = 3
EPS64 = np.finfo(np.float64).eps


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
    return sd.F64 if precision == "f64" else sd.F32


def _np(precision, cplx):
    if cplx:
        return np.complex128 if precision == "f64" else np.complex64
    return np.float64 if precision == "f64" else np.float32


def _rand(rng, shape, precision, cplx):
    x = rng.standard_normal(shape)
    if cplx:
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(_np(precision, cplx))


def _regimes(blocks, hist, unit):
    """the S-versus-hist cases a list of per-call sample counts reaches"""
    assert hist > 256 and hist % 256 and hist - 256 >= unit
    return {("zero" if s == 0 else "low" if s < hist - 256 else "mid" if s < hist else "hist" if s == hist else "high") for s in blocks}


def _history_after(x, pos, hist):
    """the last hist elements of x[:, :pos], newest first, zeros before the start"""
    full = np.concatenate([np.zeros((x.shape[0], hist), dtype=x.dtype), x[:, :pos]], axis=1)
    return full[:, full.shape[1] - hist:][:, ::-1]


def _feed_history(torch, bank, x, blocks, hist):
    """feeds x in `blocks`, checks the state after every call, returns the per-call results"""
    outs, pos = [], 0
    for n in blocks:
        outs.append(bank.process(torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + n])).cuda()))
        pos += n
        assert np.array_equal(bank.state.cpu().numpy()[:, :hist], _history_after(x, pos, hist)), (n, pos)
    assert pos == x.shape[1]
    return outs


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_history_update_stft(torch_cuda, sd, precision):
    """4- and 8-byte elements: hist = 448 = 256 + 192"""
    torch = torch_cuda
    n_fft, hop = 512, 64
    hist = n_fft - hop
    blocks = [2 * hop, 5 * hop, 7 * hop, 9 * hop, 0, hop, 4 * hop, 2 * hop]
    assert _regimes(blocks, hist, hop) == {"zero", "low", "mid", "hist", "high"}
    x = _rand(np.random.default_rng(1), (CHANNELS, sum(blocks)), precision, False)
    b = sd.stft_bank(n_fft, hop, CHANNELS, precision=_prec(sd, precision))
    outs = _feed_history(torch, b, x, blocks, hist)
    one = sd.stft_bank(n_fft, hop, CHANNELS, precision=_prec(sd, precision))
    assert torch.equal(torch.cat(outs, dim=1), one.process(torch.from_numpy(x).cuda()))
    assert torch.equal(b.state, one.state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_history_update_complex_channelizer(torch_cuda, sd, precision):
    """8- and 16-byte elements: hist = 5 * 64 - 16 = 304 = 256 + 48"""
    torch = torch_cuda
    m, p, hop = 64, 5, 16
    hist = m * p - hop
    blocks = [2 * hop, 10 * hop, 19 * hop, 21 * hop, 0, hop, 17 * hop, 2 * hop]
    assert _regimes(blocks, hist, hop) == {"zero", "low", "mid", "hist", "high"}
    x = _rand(np.random.default_rng(2), (CHANNELS, sum(blocks)), precision, True)
    kw = dict(streams=CHANNELS, taps="hamming", input="complex", precision=_prec(sd, precision))
    b = sd.pfb_bank(m, p, hop, **kw)
    outs = _feed_history(torch, b, x, blocks, hist)
    one = sd.pfb_bank(m, p, hop, **kw)
    assert torch.equal(torch.cat(outs, dim=1), one.process(torch.from_numpy(x).cuda()))
    assert torch.equal(b.state, one.state)


def test_history_update_welch(torch_cuda, sd):
    """4-byte elements through the Welch bank: hist = 511 = 256 + 255, blocks of any length.  The bank's result is its sums: every
    segment's powers are the same bits however the stream is cut (they depend on the samples alone), and a bin's sum adds the same F
    non-negative doubles in another grouping.  Each grouping is within (F - 1) u / (1 - (F - 1) u) of the exact sum, u = eps / 2, so
    two of them differ by less than F eps of the sum."""
    torch = torch_cuda
    n_fft, hop = 512, 128
    hist = n_fft - 1
    blocks = [100, 300, 511, 700, 0, 200, 400, 37]
    assert _regimes(blocks, hist, 1) == {"zero", "low", "mid", "hist", "high"}
    x = _rand(np.random.default_rng(3), (CHANNELS, sum(blocks)), "f32", False)
    b = sd.welch_bank(n_fft, hop, CHANNELS)
    counts = _feed_history(torch, b, x, blocks, hist)
    one = sd.welch_bank(n_fft, hop, CHANNELS)
    F = one.process(torch.from_numpy(x).cuda())
    assert sum(counts) == F == (x.shape[1] - n_fft) // hop + 1
    assert torch.equal(b.state, one.state)
    got, want = b.acc.cpu().numpy(), one.acc.cpu().numpy()
    diff = np.abs(got - want)
    print(f"welch sums, blocks against one call: largest difference {(diff / np.maximum(want, np.finfo(np.float64).tiny)).max():.3e} "
          f"of the sum (bound {F * EPS64:.3e})")
    assert (diff <= F * EPS64 * want).all()


def _feed_seed(torch, bank, X, frames):
    outs, f0 = [], 0
    for n in frames:
        outs.append(bank.process(X[:, f0:f0 + n].contiguous()))
        f0 += n
    assert f0 == X.shape[1]
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_seed_istft(torch_cuda, sd, precision):
    """4- and 8-byte elements: hist = 448; F hop = 128 (below hist - 256), 384 (just below hist), 448, 576, and an empty call"""
    torch = torch_cuda
    n_fft, hop = 512, 64
    hist = n_fft - hop
    frames = [2, 6, 7, 9, 0, 1, 5]
    assert _regimes([f * hop for f in frames], hist, hop) == {"zero", "low", "mid", "hist", "high"}
    assert 6 * hop == hist - hop
    rng = np.random.default_rng(4)
    X = torch.from_numpy(_rand(rng, (CHANNELS, sum(frames), n_fft // 2 + 1), precision, True)).cuda()
    pend = torch.from_numpy(_rand(rng, (CHANNELS, hist), precision, False)).cuda()
    one = sd.istft_bank(n_fft, hop, CHANNELS, precision=_prec(sd, precision))
    one._state = pend.clone()
    want = one.process(X)
    b = sd.istft_bank(n_fft, hop, CHANNELS, precision=_prec(sd, precision))
    b._state = pend.clone()
    assert torch.equal(_feed_seed(torch, b, X, frames), want)
    assert torch.equal(b.state, one.state)


def _synth(sd, precision, taps):
    return sd.pfb_synthesis_bank(64, 5, 16, streams=CHANNELS, taps=taps, output="complex", precision=_prec(sd, precision))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_seed_complex_synthesis(torch_cuda, sd, precision):
    """8- and 16-byte elements: hist = 304; F hop = 32 (below hist - 256), 288 (just below hist), 304, 336, and an empty call"""
    torch = torch_cuda
    m, hop, hist = 64, 16, 304
    frames = [2, 18, 19, 21, 0, 1, 10]
    assert _regimes([f * hop for f in frames], hist, hop) == {"zero", "low", "mid", "hist", "high"}
    assert 18 * hop == hist - hop
    rng = np.random.default_rng(5)
    taps = rng.standard_normal(5 * m)
    X = torch.from_numpy(_rand(rng, (CHANNELS, sum(frames), m), precision, True)).cuda()
    pend = torch.from_numpy(_rand(rng, (CHANNELS, hist), precision, True)).cuda()
    one = _synth(sd, precision, taps)
    assert one.hist == hist
    one._state = pend.clone()
    want = one.process(X)
    b = _synth(sd, precision, taps)
    b._state = pend.clone()
    assert torch.equal(_feed_seed(torch, b, X, frames), want)
    assert torch.equal(b.state, one.state)


def test_seed_null_state_through_the_c_entry(torch_cuda, sd):
    """no state: nothing is seeded, the sums start from zero and the tail is dropped -- the first call of a fresh bank"""
    torch = torch_cuda
    lib = sd.load()
    m, hop, F = 64, 16, 5
    rng = np.random.default_rng(6)
    taps = rng.standard_normal(5 * m)
    X = torch.from_numpy(_rand(rng, (CHANNELS, F, m), "f32", True)).cuda()
    want = _synth(sd, "f32", taps).process(X)
    b = _synth(sd, "f32", taps)
    b._ensure_plan()
    out = torch.full((CHANNELS, F * hop + 3), 7.0 - 1.0j, dtype=torch.complex64, device="cuda")
    sd.pfb_synth.L.check(lib.sdsp_hip_pfb_synth_process(b._plan, X.data_ptr(), F * m, out.data_ptr(), F * hop + 3, CHANNELS, F, 0, None,
                                                        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out[:, :F * hop], want)
    assert torch.equal(out[:, F * hop:], torch.full_like(out[:, F * hop:], 7.0 - 1.0j))
