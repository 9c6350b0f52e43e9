"""GPU tests of the inverse STFT bank (sdsp_hip_istft_*) on a real MI355X.

The checker is tests/istft_ref.py (double), itself pinned to torch.istft(center=False) and to tests/stft_ref.py in
tests/test_istft_host.py.  Every case is also held bit for bit to the composition a user writes with the library alone: pack the half
spectrum -> RfftPlan reverse -> x g in the plan precision -> overlap-add in ascending frame order, carrying the tail by hand."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal

from conftest import rel_max_err
from istft_ref import istft_ref

pytestmark = pytest.mark.gpu

N_F32 = [1 << k for k in range(5, 17)]  # 32 .. 65536
N_F64 = [1 << k for k in range(5, 16)]  # 32 .. 32768
EPS32, EPS64 = 2.0 ** -24, np.finfo(np.float64).eps


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


def _npc(precision):
    return np.complex128 if precision == "f64" else np.complex64


def _tol(precision, n_fft, hop):
    """per channel: the reverse transform's bound (f32 2e-6 with the window rounding, f64 4 N eps) plus one rounding per overlapping
    frame of the overlap-add"""
    k = -(-n_fft // hop)
    return 4 * n_fft * EPS64 + k * EPS64 if precision == "f64" else 2e-6 + k * EPS32


def _hops(n_fft):
    return ([1] if n_fft <= 512 else []) + [n_fft // 4, n_fft // 2, n_fft]


def _frames(n_fft, hop):
    return 3 * n_fft // 2 if hop == 1 else max(3, -(-2 * n_fft // hop)) + 1


def _shapes(n_fft, hop):
    """(channels, frames, frame rows of X, out columns): spare frame rows and odd out strides; 130 channels where frames stay few"""
    F = _frames(n_fft, hop)
    shapes = [(1, F, F, F * hop), (3, F, F + 1, F * hop + 3)]
    if n_fft <= 1024 and hop >= n_fft // 4:
        shapes.append((130, F, F + 2, F * hop + 1))
    return shapes


def _window(n_fft, name="hann"):
    return scipy.signal.get_window(name, n_fft)


def _spectra(torch, rng, channels, rows, n_fft, precision):
    bins = n_fft // 2 + 1
    X = (rng.standard_normal((channels, rows, bins)) + 1j * rng.standard_normal((channels, rows, bins))).astype(_npc(precision))
    return X, torch.from_numpy(X).cuda()


def _bank(sd, n_fft, hop, channels, precision, window=None, **kw):
    """default window: Hann, or Hamming at hop = N (Hann breaks NOLA there)"""
    w = _window(n_fft, "hann" if hop < n_fft else "hamming") if window is None else window
    return sd.istft_bank(n_fft, hop, channels, window=w, precision=_prec(sd, precision), **kw)


def _compose(torch, sd, Xd, pending, n_fft, hop, g, precision, variant=0):
    """the library-only inverse STFT: pack -> RfftPlan reverse -> x g (plan precision) -> ascending overlap-add; returns (y, tail)"""
    Cn, F = Xd.shape[0], Xd.shape[1]
    H, half = n_fft - hop, n_fft // 2
    packed = torch.empty((Cn, F, half), dtype=Xd.dtype, device=Xd.device)
    packed[..., 1:] = Xd[..., 1:half]
    packed[..., 0] = torch.complex(Xd[..., 0].real, Xd[..., half].real)
    plan = sd.RfftPlan(n_fft, 2, sd.reverse_fft, max_batch=Cn * F, precision=_prec(sd, precision))
    if variant:
        plan.set_variant(variant)
    z = plan.exec(torch.view_as_real(packed).reshape(Cn, F, n_fft).contiguous())
    y = z * torch.from_numpy(g.astype(_np(precision))).cuda()
    a = torch.zeros((Cn, F * hop + H), dtype=y.dtype, device=y.device)
    if pending is not None and H:
        a[:, :H] = pending
    for j in range(F):
        a[:, j * hop:j * hop + n_fft] += y[:, j]
    return a[:, :F * hop], a[:, F * hop:]


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_idx", range(12))
def test_against_reference_and_composition(torch_cuda, sd, precision, n_idx):
    torch = torch_cuda
    ns = N_F64 if precision == "f64" else N_F32
    if n_idx >= len(ns):  # f64 tops out at 32768: its twelfth case runs hops off the vector width
        n_fft, hops = 256, [3, 5]
    else:
        n_fft, hops = ns[n_idx], _hops(ns[n_idx])
    for hop in hops:
        H = n_fft - hop
        for channels, F, rows, ocols in _shapes(n_fft, hop):
            rng = np.random.default_rng(n_fft * 7 + hop * 3 + channels)
            X, Xd = _spectra(torch, rng, channels, rows, n_fft, precision)
            pend = rng.standard_normal((channels, max(H, 1))).astype(_np(precision))
            b = _bank(sd, n_fft, hop, channels, precision)
            b._state = torch.from_numpy(pend.copy()).cuda()
            g = b.synthesis_window
            X_before = Xd.clone()
            out = torch.full((channels, ocols), 777.0, dtype=b._dtype(), device=Xd.device)
            y = b.process(Xd, frames=F, out=out)
            assert torch.equal(Xd, X_before)  # in is never written
            assert torch.all(out[:, F * hop:] == 777.0)  # nothing past each row's F hop outputs
            want, want_state = istft_ref(X[:, :F], n_fft, hop, g, pend[:, :H])
            got = y.cpu().numpy()
            assert got.shape == want.shape
            err = rel_max_err(got, want)
            assert err <= _tol(precision, n_fft, hop), (hop, channels, err)
            ref, tail = _compose(torch, sd, Xd[:, :F], torch.from_numpy(pend[:, :H]).cuda(), n_fft, hop, g, precision)
            assert torch.equal(y, ref), (hop, channels)
            if H:
                assert torch.equal(b.state, tail), (hop, channels)
                assert rel_max_err(b.state.cpu().numpy(), want_state) <= _tol(precision, n_fft, hop) * 4


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_variants_equal_the_composition_bit_for_bit(torch_cuda, sd, precision):
    torch = torch_cuda
    checked = 0
    for n_fft in (N_F64 if precision == "f64" else N_F32):
        hop = n_fft // 4
        channels, F = 3, 12
        rng = np.random.default_rng(n_fft)
        X, Xd = _spectra(torch, rng, channels, F, n_fft, precision)
        for variant in (0, 1):
            b = _bank(sd, n_fft, hop, channels, precision)
            try:
                b.set_variant(variant)
            except sd.SdspHipError as e:
                assert variant and e.code == sd._lib.ERR_UNSUPPORTED
                continue
            y = b.process(Xd)
            ref, tail = _compose(torch, sd, Xd, None, n_fft, hop, b.synthesis_window, precision, variant=variant)
            assert torch.equal(y, ref), (n_fft, variant)
            assert torch.equal(b.state, tail), (n_fft, variant)
            checked += variant
    assert checked > 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop", [(32, 1), (32, 8), (512, 384), (1024, 256), (1024, 1024), (4096, 1024), (8192, 4096), (256, 6)])
def test_blockwise_equals_one_call(torch_cuda, sd, precision, n_fft, hop):
    torch = torch_cuda
    H = n_fft - hop
    # blocks with F hop shorter than hist (the in-place shift of the state), empty blocks, and longer ones
    blocks = [1, 0, 3, 1, H // hop + 2, 2, 0]
    channels = 3
    rng = np.random.default_rng(n_fft + hop)
    _, Xd = _spectra(torch, rng, channels, sum(blocks), n_fft, precision)
    pend = torch.from_numpy(rng.standard_normal((channels, max(H, 1))).astype(_np(precision))).cuda()
    one = _bank(sd, n_fft, hop, channels, precision)
    one._state = pend.clone()
    want = one.process(Xd)
    b = _bank(sd, n_fft, hop, channels, precision)
    b._state = pend.clone()
    got, f0 = [], 0
    for blk in blocks:
        got.append(b.process(Xd[:, f0:f0 + blk].contiguous()))
        f0 += blk
    assert torch.equal(torch.cat(got, dim=1), want)
    if H:
        assert torch.equal(b.state, one.state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop", [(32, 3), (512, 128), (4096, 2048), (8192, 8192), (256, 16)])
def test_small_workspace_slices_equal_default(torch_cuda, sd, precision, n_fft, hop):
    """a workspace of 1 .. 7 frames: slices cut through channels"""
    torch = torch_cuda
    rs = 8 if precision == "f64" else 4
    channels, F = 5, 2 * n_fft // hop + 3
    rng = np.random.default_rng(n_fft)
    _, Xd = _spectra(torch, rng, channels, F, n_fft, precision)
    pend = torch.from_numpy(rng.standard_normal((channels, max(n_fft - hop, 1))).astype(_np(precision))).cuda()
    ref = _bank(sd, n_fft, hop, channels, precision)
    ref._state = pend.clone()
    want = ref.process(Xd)
    for frames in range(1, 8):
        b = _bank(sd, n_fft, hop, channels, precision, workspace_bytes=frames * n_fft * rs)
        assert b.info()["workspace_bytes"] == frames * n_fft * rs
        b._state = pend.clone()
        assert torch.equal(b.process(Xd), want), frames
        if hop < n_fft:
            assert torch.equal(b.state, ref.state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop,name", [(32, 8, "hann"), (256, 64, "hann"), (1024, 256, "hann"), (1024, 512, "hamming"),
                                            (4096, 1024, "blackman"), (512, 512, "boxcar"), (8192, 2048, "hann")])
def test_round_trip_through_stft_bank(torch_cuda, sd, precision, n_fft, hop, name):
    torch = torch_cuda
    H, channels = n_fft - hop, 3
    S = hop * (2 * n_fft // hop + 6)
    x = torch.from_numpy(np.random.default_rng(n_fft + 1).standard_normal((channels, S)).astype(_np(precision))).cuda()
    w = _window(n_fft, name)
    X = sd.stft_bank(n_fft, hop, channels, window=w, output="complex", precision=_prec(sd, precision)).process(x)
    y = _bank(sd, n_fft, hop, channels, precision, window=w).process(X)
    tol = 8 * n_fft * EPS64 if precision == "f64" else 1e-5
    assert y.shape == x.shape
    assert rel_max_err(y[:, H:].cpu().numpy(), x[:, :S - H].cpu().numpy()) <= tol
    assert float(y[:, :H].abs().max()) <= tol if H else True


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_raw_mode_uses_the_window_as_given(torch_cuda, sd, precision):
    torch = torch_cuda
    n_fft, hop, channels, F = 1024, 256, 3, 9
    w = _window(n_fft, "hann") ** 0.5  # a synthesis window the caller made
    rng = np.random.default_rng(8)
    X, Xd = _spectra(torch, rng, channels, F, n_fft, precision)
    b = _bank(sd, n_fft, hop, channels, precision, window=w, normalized=False)
    assert np.array_equal(b.synthesis_window, w)
    assert b.info()["norm"] == sd._lib.ISTFT_RAW
    y = b.process(Xd)
    want, _ = istft_ref(X, n_fft, hop, w)
    assert rel_max_err(y.cpu().numpy(), want) <= _tol(precision, n_fft, hop)
    ref, _ = _compose(torch, sd, Xd, None, n_fft, hop, w, precision)
    assert torch.equal(y, ref)
    # hop = N with a Hann window: refused when normalised, taken as it is in RAW mode
    with pytest.raises(sd.SdspHipError) as e:
        _bank(sd, 256, 256, 1, precision, window=_window(256)).info()
    assert e.value.code == sd._lib.ERR_INVALID_ARG and "NOLA" in e.value.message
    assert _bank(sd, 256, 256, 1, precision, window=_window(256), normalized=False).info()["hist"] == 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_nan_reaches_exactly_the_positions_of_its_frame(torch_cuda, sd, precision):
    torch = torch_cuda
    n_fft, hop, channels, F = 256, 64, 3, 12
    _, Xd = _spectra(torch, np.random.default_rng(1), channels, F, n_fft, precision)
    j = 5
    Xd[1, j, 3] = complex(float("nan"), 0.0)
    b = _bank(sd, n_fft, hop, channels, precision)
    y = b.process(Xd)
    bad = torch.isnan(y).cpu().numpy()
    assert not bad[0].any() and not bad[2].any()
    want = np.zeros(F * hop, dtype=bool)
    want[j * hop:j * hop + n_fft] = True
    assert np.array_equal(bad[1], want)
    assert not torch.isnan(b.state).any()  # frame 5 ends at 5 hop + N = 576 < F hop = 768: nothing pending


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_null_state_starts_from_zero_and_drops_the_tail(torch_cuda, sd, precision):
    torch = torch_cuda
    lib = sd.load()
    n_fft, hop, channels, F = 512, 128, 4, 7
    bins = n_fft // 2 + 1
    X, Xd = _spectra(torch, np.random.default_rng(3), channels, F, n_fft, precision)
    b = _bank(sd, n_fft, hop, channels, precision)
    b.info()
    out = torch.full((channels, F * hop + 8), -5.0, dtype=b._dtype(), device=Xd.device)
    assert lib.sdsp_hip_istft_process(b._plan, Xd.data_ptr(), F * bins, out.data_ptr(), F * hop + 8, channels, F, None, None) == 0
    torch.cuda.synchronize()
    fresh = _bank(sd, n_fft, hop, channels, precision).process(Xd)
    assert torch.equal(out[:, :F * hop], fresh)
    assert torch.all(out[:, F * hop:] == -5.0)


def _kernel_nodes(torch, fn):
    """kernel launches `fn` makes on a captured stream (hipGraph nodes of kernel type; the graph is never launched)"""
    hip = C.CDLL("libamdhip64.so")
    s = torch.cuda.Stream()
    graph = C.c_void_p()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
        try:
            fn()
        finally:
            assert hip.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(graph)) == 0
    try:
        n = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
        nodes = (C.c_void_p * max(n.value, 1))()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
        kinds = []
        for i in range(n.value):
            t = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
            kinds.append(t.value)
        return sum(1 for k in kinds if k == 0)  # hipGraphNodeTypeKernel
    finally:
        hip.hipGraphDestroy(graph)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop,ws_frames", [(1024, 256, 0), (1024, 256, 5), (256, 256, 3), (65536, 16384, 2)])
def test_launches_matches_the_launches_made(torch_cuda, sd, precision, n_fft, hop, ws_frames):
    torch = torch_cuda
    if precision == "f64" and n_fft > 32768:
        n_fft, hop = 32768, 8192
    rs = 8 if precision == "f64" else 4
    channels, F = 3, 11
    _, Xd = _spectra(torch, np.random.default_rng(2), channels, F, n_fft, precision)
    b = _bank(sd, n_fft, hop, channels, precision, window=_window(n_fft, "hamming"), workspace_bytes=ws_frames * n_fft * rs)
    out = torch.empty((channels, F * hop), dtype=b._dtype(), device=Xd.device)
    b.process(Xd, out=out)  # plan and state exist before the capture
    n = _kernel_nodes(torch, lambda: b.process(Xd, out=out))
    assert n == b.launches(F), (n, b.launches(F))
    assert b.launches(0) == 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_graph_capture_replays_the_eager_call(torch_cuda, sd, precision):
    torch = torch_cuda
    n_fft, hop, channels, F = 1024, 256, 9, 16
    _, Xd = _spectra(torch, np.random.default_rng(4), channels, F, n_fft, precision)
    eager = _bank(sd, n_fft, hop, channels, precision, workspace_bytes=5 * n_fft * 8)
    want = eager.process(Xd)
    g_bank = _bank(sd, n_fft, hop, channels, precision, workspace_bytes=5 * n_fft * 8)
    g_bank._state = torch.zeros((channels, n_fft - hop), dtype=want.dtype, device=want.device)
    g_bank.info()  # plan outside the capture
    out = torch.empty_like(want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_bank.process(Xd, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(g_bank.state, eager.state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_errors_and_host_path(torch_cuda, sd, precision):
    torch = torch_cuda
    L = sd._lib
    lib = sd.load()
    n_fft, hop, channels, F = 256, 64, 3, 10
    bins, S, H = n_fft // 2 + 1, F * hop, n_fft - hop
    b = _bank(sd, n_fft, hop, channels, precision)
    b.info()
    p = b._plan
    rs = 8 if precision == "f64" else 4
    X, Xd = _spectra(torch, np.random.default_rng(5), channels, F, n_fft, precision)
    out = torch.zeros((channels, S), dtype=b._dtype(), device=Xd.device)
    st = torch.zeros((channels, H), dtype=b._dtype(), device=Xd.device)

    def run(i=Xd.data_ptr(), istr=F * bins, o=out.data_ptr(), ostr=S, ch=channels, f=F, state=st.data_ptr()):
        return lib.sdsp_hip_istft_process(p, i, istr, o, ostr, ch, f, state, None)

    assert run(i=None) == L.ERR_INVALID_ARG
    assert run(o=None) == L.ERR_INVALID_ARG
    assert run(istr=F * bins - 1) == L.ERR_INVALID_ARG
    assert run(ostr=S - 1) == L.ERR_INVALID_ARG
    assert run(o=Xd.data_ptr() + 64) == L.ERR_INVALID_ARG  # overlapping in and out
    assert run(i=Xd.data_ptr() + rs) == L.ERR_INVALID_ARG  # a complex bin split in two
    assert run(o=out.data_ptr() + 1) == L.ERR_INVALID_ARG
    assert run(state=st.data_ptr() + 1) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_process(None, Xd.data_ptr(), F * bins, out.data_ptr(), S, channels, F, None, None) == L.ERR_INVALID_ARG
    assert run(ch=0) == 0 and run(f=0) == 0 and run(ch=0, i=None, o=None) == 0 and run(f=0, i=None, o=None) == 0
    assert torch.all(out == 0) and torch.all(st == 0)
    assert lib.sdsp_hip_istft_plan_set_variant(p, -1) == L.ERR_INVALID_ARG
    nb = C.c_uint64(0)
    assert lib.sdsp_hip_istft_state_bytes(p, channels, C.byref(nb)) == 0 and nb.value == channels * H * rs
    assert lib.sdsp_hip_istft_state_bytes(p, channels, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_istft_plan_get_info(p, None) == L.ERR_INVALID_ARG
    info = b.info()
    assert (info["n_fft"], info["hop"], info["bins"], info["hist"]) == (n_fft, hop, bins, H)
    assert info["norm"] == L.ISTFT_NORMALIZED and info["precision"] == _prec(sd, precision) and info["kernel"]
    assert info["env_min"] == pytest.approx(1.5) and info["env_max"] == pytest.approx(1.5)  # periodic Hann at hop N / 4
    # the host entry equals the device entry, state included
    pend = np.random.default_rng(6).standard_normal((channels, H)).astype(_np(precision))
    st.copy_(torch.from_numpy(pend))
    assert run() == 0
    torch.cuda.synchronize()
    oh = np.zeros((channels, S), dtype=_np(precision))
    sh = pend.copy()
    assert lib.sdsp_hip_istft_process_host(p, X.ctypes.data, F * bins, oh.ctypes.data, S, channels, F, sh.ctypes.data) == 0
    assert np.array_equal(oh, out.cpu().numpy())
    assert np.array_equal(sh, st.cpu().numpy())
    assert lib.sdsp_hip_istft_process_host(p, None, F * bins, oh.ctypes.data, S, channels, F, None) == L.ERR_INVALID_ARG
