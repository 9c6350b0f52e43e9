"""GPU tests of the STFT bank (sdsp_hip_stft_*) on a real MI355X.

The checker is tests/stft_ref.py (double), itself pinned to torch.stft(center=False) in tests/test_stft_host.py.  Every case is
also held bit for bit to the composition a user writes with the library alone: unfold x window in the plan precision ->
RfftPlan.exec -> unpack the packed half spectrum (-> re re + im im)."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal

from conftest import rel_max_err
from stft_ref import stft_ref

pytestmark = pytest.mark.gpu

N_F32 = [32, 512, 1024, 4096, 8192, 65536]
N_F64 = [32, 512, 1024, 4096, 8192, 32768]


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


def _np(precision):
    return np.float64 if precision == "f64" else np.float32


def _tol(precision, n_fft, output):
    """f64: 4 N eps per frame; f32: 2e-6 (the real-input transform's 1e-6 plus the window rounding).  The power squares the
    magnitude, so its relative error is twice that of the spectrum."""
    t = 4 * n_fft * np.finfo(np.float64).eps if precision == "f64" else 2e-6
    return 2 * t if output == "power" else t


def _hops(n_fft):
    return ([1] if n_fft <= 512 else []) + [n_fft // 4, n_fft // 2, n_fft]


def _shapes(n_fft, hop):
    """(channels, samples, in_stride): odd in_stride > samples; 130 channels where the frames stay few"""
    S = hop * max(3, -(-2 * n_fft // hop))
    if hop == 1:
        S = 3 * n_fft // 2
    shapes = [(1, S, S), (3, S, S + 3)]
    if n_fft <= 1024 and hop >= n_fft // 4:
        shapes.append((130, S, S + 1 + (S % 2 == 0)))
    return shapes


def _window(n_fft):
    return scipy.signal.get_window("hann", n_fft)


def _compose(torch, sd, xs, hist_rows, n_fft, hop, w, precision, output, variant=0):
    """the library-only STFT: history + block -> unfold -> x window (plan precision) -> RfftPlan.exec -> unpack"""
    dt = torch.float64 if precision == "f64" else torch.float32
    full = torch.cat([hist_rows.flip(-1), xs], dim=1)
    frames = (full.unfold(-1, n_fft, hop) * torch.from_numpy(w.astype(_np(precision))).cuda()).contiguous()
    Cn, F = frames.shape[0], frames.shape[1]
    plan = sd.RfftPlan(n_fft, 2, sd.forward_fft, max_batch=Cn * F, precision=_prec(sd, precision))
    if variant:
        plan.set_variant(variant)
    z = plan.exec(frames)  # (C, F, N/2) packed
    out = torch.empty((Cn, F, n_fft // 2 + 1), dtype=z.dtype, device=z.device)
    out[..., 1:n_fft // 2] = z[..., 1:]
    out[..., 0] = torch.complex(z[..., 0].real, torch.zeros_like(z[..., 0].real))
    out[..., n_fft // 2] = torch.complex(z[..., 0].imag, torch.zeros_like(z[..., 0].imag))
    if output == "power":
        return out.real * out.real + out.imag * out.imag
    assert dt == out.real.dtype
    return out


def _bank(sd, n_fft, hop, channels, precision, output, **kw):
    return sd.stft_bank(n_fft, hop, channels, window=_window(n_fft), output=output, precision=_prec(sd, precision), **kw)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("output", ["complex", "power", "magnitude"])
@pytest.mark.parametrize("n_idx", range(6))
def test_against_reference_and_composition(torch_cuda, sd, precision, output, n_idx):
    torch = torch_cuda
    n_fft = (N_F64 if precision == "f64" else N_F32)[n_idx]
    w = _window(n_fft)
    for hop in _hops(n_fft):
        for channels, S, stride in _shapes(n_fft, hop):
            rng = np.random.default_rng(n_fft * 7 + hop * 3 + channels)
            H = n_fft - hop
            x = rng.standard_normal((channels, stride)).astype(_np(precision))
            hist = rng.standard_normal((channels, max(H, 1))).astype(_np(precision))
            xd = torch.from_numpy(x).cuda()
            b = _bank(sd, n_fft, hop, channels, precision, output)
            b._state = torch.from_numpy(hist.copy()).cuda()
            x_before = xd.clone()
            y = b.process(xd, samples=S)
            assert torch.equal(xd, x_before)  # in is never written
            want, want_state = stft_ref(x[:, :S], n_fft, hop, w, hist[:, :H], output)
            got = y.cpu().numpy()
            assert got.shape == want.shape
            err = rel_max_err(got, want)
            assert err <= _tol(precision, n_fft, output), (hop, channels, err)
            if H:
                assert np.array_equal(b.state.cpu().numpy(), want_state.astype(_np(precision)))
            if output != "magnitude":
                ref = _compose(torch, sd, xd[:, :S], torch.from_numpy(hist[:, :H]).cuda(), n_fft, hop, w, precision, output)
                assert torch.equal(y, ref), (hop, channels)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop", [(32, 1), (32, 8), (512, 384), (1024, 256), (1024, 1024), (4096, 1024), (8192, 4096)])
def test_blockwise_equals_one_call(torch_cuda, sd, precision, n_fft, hop):
    torch = torch_cuda
    H = n_fft - hop
    # blocks shorter than hist (the in-place shift of the state), empty blocks, and longer ones
    blocks = [hop, 0, 3 * hop, hop, (H // hop + 2) * hop, 2 * hop]
    channels = 3
    rng = np.random.default_rng(n_fft + hop)
    x = torch.from_numpy(rng.standard_normal((channels, sum(blocks))).astype(_np(precision))).cuda()
    one = _bank(sd, n_fft, hop, channels, precision, "complex")
    one.preload_filter(0.5)
    want = one.process(x)
    b = _bank(sd, n_fft, hop, channels, precision, "complex")
    b.preload_filter(0.5)
    got, s0 = [], 0
    for blk in blocks:
        got.append(b.process(x[:, s0:s0 + blk].contiguous()))
        s0 += blk
    assert torch.equal(torch.cat(got, dim=1), want)
    if H:
        assert torch.equal(b.state, one.state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop", [(32, 3), (512, 128), (4096, 2048), (8192, 8192)])
def test_small_workspace_slices_equal_default(torch_cuda, sd, precision, n_fft, hop):
    """a workspace of one or a few frames: slices cut through channels"""
    torch = torch_cuda
    rs = 8 if precision == "f64" else 4
    channels = 5
    S = hop * (2 * n_fft // hop + 3)
    rng = np.random.default_rng(n_fft)
    x = torch.from_numpy(rng.standard_normal((channels, S)).astype(_np(precision))).cuda()
    ref = _bank(sd, n_fft, hop, channels, precision, "power")
    want = ref.process(x)
    for frames in (1, 3, 7):
        b = _bank(sd, n_fft, hop, channels, precision, "power", workspace_bytes=frames * n_fft * rs)
        assert b.info()["workspace_bytes"] == frames * n_fft * rs
        got = b.process(x)
        assert torch.equal(got, want), frames
        if hop < n_fft:
            assert torch.equal(b.state, ref.state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_preload_equals_a_stream_preceded_by_the_value(torch_cuda, sd, precision):
    torch = torch_cuda
    n_fft, hop, channels = 1024, 256, 4
    H = n_fft - hop
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((channels, 8 * hop)).astype(_np(precision))).cuda()
    a = _bank(sd, n_fft, hop, channels, precision, "complex")
    a.preload_filter(-0.75)
    got = a.process(x)
    b = _bank(sd, n_fft, hop, channels, precision, "complex")
    b.process(torch.full((channels, H), -0.75, dtype=x.dtype, device=x.device))  # hist samples of the value, H a multiple of hop
    assert torch.equal(b.process(x), got)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_nan_reaches_exactly_the_frames_that_cover_it(torch_cuda, sd, precision):
    torch = torch_cuda
    n_fft, hop, channels, S = 256, 64, 3, 64 * 12
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((channels, S)).astype(_np(precision))).cuda()
    s = 300
    x[1, s] = float("nan")
    y = _bank(sd, n_fft, hop, channels, precision, "complex").process(x)
    bad = torch.isnan(torch.view_as_real(y)).flatten(2).any(-1).cpu().numpy()  # (channels, F)
    p = s + n_fft - hop  # position in history + block
    cover = np.array([j * hop <= p < j * hop + n_fft for j in range(S // hop)])
    assert not bad[0].any() and not bad[2].any()
    assert np.array_equal(bad[1], cover)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("output", ["complex", "power"])
def test_nothing_past_each_row_is_written(torch_cuda, sd, precision, output):
    torch = torch_cuda
    n_fft, hop, channels, S = 512, 128, 7, 128 * 9
    F = S // hop
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((channels, S + 5)).astype(_np(precision))).cuda()
    b = _bank(sd, n_fft, hop, channels, precision, output)
    odt = b._out_dtype()
    out = torch.full((channels, F + 3, n_fft // 2 + 1), 12345.0, dtype=odt, device=x.device)
    got = b.process(x, samples=S, out=out)
    assert got.shape == (channels, F, n_fft // 2 + 1)
    assert torch.all(out[:, F:] == 12345.0)
    c = _bank(sd, n_fft, hop, channels, precision, output)
    assert torch.equal(out[:, :F], c.process(x[:, :S].contiguous()))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_variant_one_agrees(torch_cuda, sd, precision):
    torch = torch_cuda
    checked = 0
    for n_fft in (N_F64 if precision == "f64" else N_F32):
        hop = n_fft // 4
        channels, S = 3, hop * 12
        x = torch.from_numpy(np.random.default_rng(n_fft).standard_normal((channels, S)).astype(_np(precision))).cuda()
        b = _bank(sd, n_fft, hop, channels, precision, "complex")
        try:
            b.set_variant(1)
        except sd.SdspHipError as e:
            assert e.code == sd._lib.ERR_UNSUPPORTED
            continue
        want, _ = stft_ref(x.cpu().numpy(), n_fft, hop, _window(n_fft))
        assert rel_max_err(b.process(x).cpu().numpy(), want) <= _tol(precision, n_fft, "complex")
        ref = _compose(torch, sd, x, torch.zeros((channels, n_fft - hop), dtype=x.dtype, device=x.device), n_fft, hop,
                       _window(n_fft), precision, "complex", variant=1)
        b.reset()
        assert torch.equal(b.process(x), ref)
        checked += 1
    assert checked > 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_graph_capture_replays_the_eager_call(torch_cuda, sd, precision):
    torch = torch_cuda
    n_fft, hop, channels, S = 1024, 256, 9, 256 * 16
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((channels, S)).astype(_np(precision))).cuda()
    eager = _bank(sd, n_fft, hop, channels, precision, "power", workspace_bytes=5 * n_fft * 8)
    want = eager.process(x)
    g_bank = _bank(sd, n_fft, hop, channels, precision, "power", workspace_bytes=5 * n_fft * 8)
    g_bank.preload_filter(0.0)
    g_bank.info()  # plan outside the capture
    out = torch.empty_like(want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_bank.process(x, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(g_bank.state, eager.state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_errors_and_host_path(torch_cuda, sd, precision):
    torch = torch_cuda
    L = sd._lib
    lib = sd.load()
    n_fft, hop, channels, S = 256, 64, 3, 640
    F, bins = S // hop, n_fft // 2 + 1
    b = _bank(sd, n_fft, hop, channels, precision, "complex")
    b.info()
    p = b._plan
    rs = 8 if precision == "f64" else 4
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((channels, S)).astype(_np(precision))).cuda()
    out = torch.zeros((channels, F, bins), dtype=b._out_dtype(), device=x.device)
    st = torch.zeros((channels, n_fft - hop), dtype=x.dtype, device=x.device)

    def run(i=x.data_ptr(), istr=S, o=out.data_ptr(), ostr=F * bins, ch=channels, s=S, state=st.data_ptr()):
        return lib.sdsp_hip_stft_process(p, i, istr, o, ostr, ch, s, state, None)

    assert run(s=S - 1) == L.ERR_INVALID_SIZE
    assert run(i=None) == L.ERR_INVALID_ARG
    assert run(o=None) == L.ERR_INVALID_ARG
    assert run(istr=S - 1) == L.ERR_INVALID_ARG
    assert run(ostr=F * bins - 1) == L.ERR_INVALID_ARG
    assert run(o=x.data_ptr() + 16) == L.ERR_INVALID_ARG  # overlapping in and out
    assert lib.sdsp_hip_stft_process(None, x.data_ptr(), S, out.data_ptr(), F * bins, channels, S, None, None) == L.ERR_INVALID_ARG
    assert run(ch=0) == 0 and run(s=0) == 0 and run(ch=0, i=None, o=None) == 0
    assert torch.all(out == 0) and torch.all(st == 0)
    assert lib.sdsp_hip_stft_plan_set_variant(p, -1) == L.ERR_INVALID_ARG
    nb = C.c_uint64(0)
    assert lib.sdsp_hip_stft_state_bytes(p, channels, C.byref(nb)) == 0 and nb.value == channels * (n_fft - hop) * rs
    assert b.launches(S) >= 4 and b.launches(0) == 0
    info = b.info()
    assert (info["n_fft"], info["hop"], info["bins"], info["hist"]) == (n_fft, hop, bins, n_fft - hop)
    assert info["kernel"]
    # the host entry equals the device entry, state included
    hist = np.random.default_rng(6).standard_normal((channels, n_fft - hop)).astype(_np(precision))
    st.copy_(torch.from_numpy(hist))
    assert run() == 0
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    oh = np.zeros((channels, F, bins, 2), dtype=_np(precision))
    sh = hist.copy()
    assert lib.sdsp_hip_stft_process_host(p, xh.ctypes.data, S, oh.ctypes.data, F * bins, channels, S, sh.ctypes.data) == 0
    assert np.array_equal(oh, torch.view_as_real(out).cpu().numpy())
    assert np.array_equal(sh, st.cpu().numpy())
