"""GPU tests of the Welch PSD bank (sdsp_hip_welch_*) on a real MI355X.

The checker is tests/welch_ref.py (double), itself pinned to scipy.signal.welch in tests/test_welch_host.py.  With detrend NONE and
one segment per call the sums are held bit for bit to a numpy sequential sum of re re + im im over RfftPlan.exec of the rounded
windowed segments."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal

from welch_ref import welch_frames, welch_psd, welch_ref

pytestmark = pytest.mark.gpu

N_F32 = [32, 256, 1024, 4096, 65536]
N_F64 = [32, 256, 1024, 4096, 32768]


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


def _tol(precision):
    return 1e-12 if precision == "f64" else 2e-5


def _peak_err(got, want):
    """max over channels of max_k |got - want| / max_k |want|"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)).max())


def _rounded_window(w, precision):
    return w.astype(_np(precision)).astype(np.float64)


def _bank(sd, n_fft, hop, channels, precision, **kw):
    kw.setdefault("window", scipy.signal.get_window("hann", n_fft))
    return sd.welch_bank(n_fft, hop, channels, precision=_prec(sd, precision), **kw)


def _hops(n_fft):
    return [n_fft // 2, n_fft // 4, 7 * n_fft // 32 + 1, n_fft]  # 7 N / 32 + 1 does not divide N


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("detrend", ["none", "constant", "linear"])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("n_idx", range(5))
def test_against_reference_and_scipy(torch_cuda, sd, precision, detrend, scaling, n_idx):
    torch = torch_cuda
    n_fft = (N_F64 if precision == "f64" else N_F32)[n_idx]
    w = scipy.signal.get_window("hann", n_fft)
    wr = _rounded_window(w, precision)
    fs = 1000.0
    for hop in _hops(n_fft):
        channels = 3 if n_fft >= 4096 else 5
        S = 4 * n_fft + 37
        rng = np.random.default_rng(n_fft * 7 + hop)
        x = (rng.standard_normal((channels, S + 3)) + np.linspace(-2, 3, S + 3)).astype(_np(precision))
        xd = torch.from_numpy(x).cuda()
        x_before = xd.clone()
        b = _bank(sd, n_fft, hop, channels, precision, window=w, detrend=detrend, scaling=scaling, fs=fs)
        # two calls: the second one reads the history the first one left
        s1 = n_fft + hop // 2
        b.process(xd, samples=s1)
        b.process(xd[:, s1:].contiguous(), samples=S - s1)
        assert torch.equal(xd, x_before)
        F = (S - n_fft) // hop + 1
        assert b.frames == F
        got = b.psd().cpu().numpy()
        acc, F_ref, state = welch_ref(x[:, :S], n_fft, hop, wr, detrend)
        assert F_ref == F
        want = welch_psd(acc, F, wr, fs, scaling)
        err = _peak_err(got, want)
        assert err <= _tol(precision), (hop, err)
        assert np.array_equal(b.state.cpu().numpy(), state.astype(_np(precision)))
        if precision == "f64":
            _, sp = scipy.signal.welch(x[:, :S], fs, window=w, nperseg=n_fft, noverlap=n_fft - hop,
                                       detrend=False if detrend == "none" else detrend, scaling=scaling)
            assert _peak_err(got, sp) <= 1e-12, hop


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("detrend", [False, "constant", "linear"])
def test_one_shot_matches_scipy(torch_cuda, sd, precision, detrend):
    torch = torch_cuda
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((4, 10000)) * 3 + 1).astype(_np(precision))
    for nperseg, noverlap, window in [(256, None, "hann"), (256, 200, "hamming"), (1024, 0, "blackman"), (64, 63, "boxcar")]:
        f, p = sd.welch(torch.from_numpy(x).cuda(), fs=8000.0, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend)
        fw, pw = scipy.signal.welch(x.astype(np.float64), fs=8000.0, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend)
        assert np.array_equal(f, fw)
        assert p.dtype == torch.from_numpy(x).dtype and p.shape == pw.shape
        assert _peak_err(p.cpu().numpy(), pw) <= _tol(precision), (nperseg, noverlap)
    f1, p1 = sd.welch(torch.from_numpy(x[0]).cuda(), nperseg=128, detrend=detrend)
    _, pw1 = scipy.signal.welch(x[0].astype(np.float64), nperseg=128, detrend=detrend)
    assert p1.shape == pw1.shape and _peak_err(p1.cpu().numpy(), pw1) <= _tol(precision)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop", [(256, 64), (1024, 1024), (32, 5)])
def test_one_segment_per_call_is_a_sequential_double_sum(torch_cuda, sd, precision, n_fft, hop):
    torch = torch_cuda
    channels, calls = 3, 9
    w = scipy.signal.get_window("hann", n_fft)
    npdt = _np(precision)
    S = n_fft + (calls - 1) * hop
    x = np.random.default_rng(n_fft + hop).standard_normal((channels, S)).astype(npdt)
    b = _bank(sd, n_fft, hop, channels, precision, window=w, detrend="none")
    plan = sd.RfftPlan(n_fft, 2, sd.forward_fft, max_batch=channels, precision=_prec(sd, precision))
    acc = np.zeros((channels, n_fft // 2 + 1))
    pos = 0
    for m in range(calls):
        end = m * hop + n_fft
        blk = torch.from_numpy(np.ascontiguousarray(x[:, pos:end])).cuda()
        assert b.process(blk) == 1
        pos = end
        frames = x[:, m * hop:m * hop + n_fft] * w.astype(npdt)  # round_p(x w)
        z = plan.exec(torch.from_numpy(np.ascontiguousarray(frames)).cuda()).cpu().numpy()  # (channels, N/2) packed
        re = z.real.astype(np.float64)
        im = z.imag.astype(np.float64)
        p = np.empty_like(acc)
        p[:, 1:n_fft // 2] = re[:, 1:] * re[:, 1:] + im[:, 1:] * im[:, 1:]
        p[:, 0] = re[:, 0] * re[:, 0]
        p[:, n_fft // 2] = im[:, 0] * im[:, 0]
        acc = acc + p
        assert np.array_equal(b.acc.cpu().numpy(), acc), m


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop,detrend", [(256, 56, "linear"), (1024, 256, "constant"), (64, 64, "none"), (4096, 1000, "constant")])
def test_streaming_slicing_and_determinism(torch_cuda, sd, precision, n_fft, hop, detrend):
    torch = torch_cuda
    channels = 4
    blocks = [0, 1, n_fft - 2, hop + 1, hop - 1, 0, 3, 6 * n_fft + 11, n_fft - 1, 2 * hop]
    S = sum(blocks)
    x = np.random.default_rng(n_fft + 3 * hop).standard_normal((channels, S)).astype(_np(precision))
    xd = torch.from_numpy(x).cuda()
    one = _bank(sd, n_fft, hop, channels, precision, detrend=detrend)
    one.process(xd)
    want = one.acc.clone()
    tol = 1e-14 if precision == "f64" else 1e-6
    # arbitrary blocks
    bb = _bank(sd, n_fft, hop, channels, precision, detrend=detrend)
    pos = 0
    for blk in blocks:
        got = bb.process(torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + blk])).cuda())
        assert got == welch_frames(n_fft, hop, pos, blk)
        pos += blk
    assert bb.frames == one.frames == (S - n_fft) // hop + 1
    assert _peak_err(bb.acc.cpu().numpy(), want.cpu().numpy()) <= tol
    assert np.array_equal(bb.state.cpu().numpy(), x[:, ::-1][:, :n_fft - 1])
    assert torch.equal(bb.state, one.state)
    # workspaces of 1 .. 7 segments
    unit = n_fft * (8 if precision == "f64" else 4) + (n_fft // 2 + 1) * 8
    for k in range(1, 8):
        bk = _bank(sd, n_fft, hop, channels, precision, detrend=detrend, workspace_bytes=k * unit)
        assert bk.info()["workspace_bytes"] == k * unit
        bk.process(xd)
        assert _peak_err(bk.acc.cpu().numpy(), want.cpu().numpy()) <= tol, k
    # identical calls on identical plans: identical bits
    again = _bank(sd, n_fft, hop, channels, precision, detrend=detrend)
    again.process(xd)
    assert torch.equal(again.acc, want)
    assert torch.equal(again.psd(), one.psd())


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_few_long_channels(torch_cuda, sd, precision):
    torch = torch_cuda
    channels, S, n_fft, hop = 2, 1 << 22, 1024, 512
    x = np.random.default_rng(21).standard_normal((channels, S)).astype(_np(precision))
    w = scipy.signal.get_window("hann", n_fft)
    b = _bank(sd, n_fft, hop, channels, precision, window=w, detrend="constant")
    b.process(torch.from_numpy(x).cuda())
    got = b.psd().cpu().numpy()
    acc, F, _ = welch_ref(x, n_fft, hop, _rounded_window(w, precision), "constant")
    assert b.frames == F == (S - n_fft) // hop + 1
    assert _peak_err(got, welch_psd(acc, F, _rounded_window(w, precision))) <= _tol(precision)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_nan_stays_in_its_channel_and_rows_end_at_bins(torch_cuda, sd, precision):
    torch = torch_cuda
    lib = sd.load()
    n_fft, hop, channels, S = 256, 64, 4, 2048
    bins = n_fft // 2 + 1
    x = np.random.default_rng(8).standard_normal((channels, S + 5)).astype(_np(precision))
    x[2, 700] = np.nan
    xd = torch.from_numpy(x).cuda()
    x_before = xd.clone()
    b = _bank(sd, n_fft, hop, channels, precision, detrend="constant")
    b.info()
    acc = torch.full((channels, bins + 7), -3.0, dtype=torch.float64, device=xd.device)
    acc[:, :bins] = 0
    st = torch.zeros((channels, n_fft - 1), dtype=xd.dtype, device=xd.device)
    assert lib.sdsp_hip_welch_process(b._plan, xd.data_ptr(), S + 5, channels, S, 0, st.data_ptr(), acc.data_ptr(), bins + 7, None) == 0
    F = welch_frames(n_fft, hop, 0, S)
    out = torch.full((channels, bins + 3), -9.0, dtype=xd.dtype, device=xd.device)
    assert lib.sdsp_hip_welch_finalize(b._plan, acc.data_ptr(), bins + 7, F, out.data_ptr(), bins + 3, channels, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x_before.cpu().numpy(), equal_nan=True)  # in is never written
    assert torch.all(acc[:, bins:] == -3.0) and torch.all(out[:, bins:] == -9.0)
    o = out[:, :bins].cpu().numpy()
    assert np.isnan(o[2]).all()
    keep = [0, 1, 3]
    assert np.isfinite(o[keep]).all()
    acc_ref, _, _ = welch_ref(x[keep, :S], n_fft, hop, _rounded_window(scipy.signal.get_window("hann", n_fft), precision), "constant")
    want = welch_psd(acc_ref, F, _rounded_window(scipy.signal.get_window("hann", n_fft), precision))
    assert _peak_err(o[keep], want) <= _tol(precision)


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
def test_graph_capture_replays_the_eager_call(torch_cuda, sd, precision):
    torch = torch_cuda
    n_fft, hop, channels, S = 1024, 256, 9, 256 * 16 + 100
    unit = n_fft * (8 if precision == "f64" else 4) + (n_fft // 2 + 1) * 8
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((channels, S)).astype(_np(precision))).cuda()
    eager = _bank(sd, n_fft, hop, channels, precision, workspace_bytes=5 * unit)
    eager.process(x)
    want = eager.psd()
    g_bank = _bank(sd, n_fft, hop, channels, precision, workspace_bytes=5 * unit)
    g_bank._ensure_plan()
    g_bank._ensure_buffers()  # plan, history and sums outside the capture
    out = torch.empty_like(want)
    pos0 = g_bank.position
    launches = g_bank.launches(S, finalize=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_bank.process(x)
        g_bank.psd(out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(g_bank.state, eager.state) and torch.equal(g_bank.acc, eager.acc)
    # the kernel nodes of one process + finalize: a fresh bank at the same position
    c_bank = _bank(sd, n_fft, hop, channels, precision, workspace_bytes=5 * unit)
    c_bank._ensure_plan()
    c_bank._ensure_buffers()
    c_bank.frames = 1
    assert c_bank.position == pos0
    n = _kernel_nodes(torch, lambda: (c_bank.process(x), c_bank.psd(out=out)))
    assert n == launches, (n, launches)
    assert c_bank.launches(0) == 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_errors_and_host_paths(torch_cuda, sd, precision):
    torch = torch_cuda
    L = sd._lib
    lib = sd.load()
    n_fft, hop, channels, S = 256, 56, 3, 1000
    bins = n_fft // 2 + 1
    rs = 8 if precision == "f64" else 4
    b = _bank(sd, n_fft, hop, channels, precision, detrend="linear", scaling="spectrum", fs=3.0)
    info = b.info()
    assert (info["n_fft"], info["hop"], info["bins"], info["hist"]) == (n_fft, hop, bins, n_fft - 1)
    assert (info["detrend"], info["scaling"], info["fs"], info["precision"]) == (L.DETREND_LINEAR, L.SCALING_SPECTRUM, 3.0,
                                                                                 _prec(sd, precision))
    assert info["kernel"] and info["workspace_bytes"] > 0
    p = b._plan
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((channels, S)).astype(_np(precision))).cuda()
    acc = torch.zeros((channels, bins), dtype=torch.float64, device=x.device)
    st = torch.zeros((channels, n_fft - 1), dtype=x.dtype, device=x.device)
    out = torch.zeros((channels, bins), dtype=x.dtype, device=x.device)

    def run(i=x.data_ptr(), istr=S, ch=channels, s=S, pos=0, state=st.data_ptr(), a=acc.data_ptr(), astr=bins, plan=p):
        return lib.sdsp_hip_welch_process(plan, i, istr, ch, s, pos, state, a, astr, None)

    def fin(a=acc.data_ptr(), astr=bins, frames=5, o=out.data_ptr(), ostr=bins, ch=channels, plan=p):
        return lib.sdsp_hip_welch_finalize(plan, a, astr, frames, o, ostr, ch, None)

    assert run(plan=None) == L.ERR_INVALID_ARG
    assert run(i=None) == L.ERR_INVALID_ARG
    assert run(a=None) == L.ERR_INVALID_ARG
    assert run(state=None, pos=10) == L.ERR_INVALID_ARG
    assert run(istr=S - 1) == L.ERR_INVALID_ARG
    assert run(astr=bins - 1) == L.ERR_INVALID_ARG
    assert run(state=x.data_ptr() + 64) == L.ERR_INVALID_ARG  # in overlaps state
    assert run(a=x.data_ptr() + 64) == L.ERR_INVALID_ARG  # in overlaps acc
    assert run(i=x.data_ptr() + 1) == L.ERR_INVALID_ARG  # misaligned
    assert run(pos=1 << 63, s=1 << 63) == L.ERR_INVALID_SIZE
    assert run(ch=0) == 0 and run(s=0) == 0 and run(ch=0, i=None, a=None) == 0
    assert fin(plan=None) == L.ERR_INVALID_ARG
    assert fin(frames=0) == L.ERR_INVALID_SIZE
    assert fin(a=None) == L.ERR_INVALID_ARG and fin(o=None) == L.ERR_INVALID_ARG
    assert fin(astr=bins - 1) == L.ERR_INVALID_ARG and fin(ostr=bins - 1) == L.ERR_INVALID_ARG
    assert fin(o=acc.data_ptr() + 8) == L.ERR_INVALID_ARG  # acc overlaps out
    assert fin(ch=0) == 0
    torch.cuda.synchronize()
    assert torch.all(acc == 0) and torch.all(st == 0) and torch.all(out == 0)
    nb = C.c_uint64(0)
    assert lib.sdsp_hip_welch_state_bytes(p, channels, C.byref(nb)) == 0 and nb.value == channels * (n_fft - 1) * rs
    assert lib.sdsp_hip_welch_state_bytes(None, channels, C.byref(nb)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_welch_plan_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_welch_plan_launches(p, channels, S, 0, None) == L.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        b.psd()  # no segment yet
    # the host entries equal the device entries, history included: two calls from position 0
    s1 = 300
    assert run(s=s1) == 0 and run(i=x.data_ptr() + s1 * rs, s=S - s1, pos=s1) == 0
    F = welch_frames(n_fft, hop, 0, S)
    assert fin(frames=F) == 0
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    acc_h = np.zeros((channels, bins))
    st_h = np.zeros((channels, n_fft - 1), dtype=_np(precision))
    assert lib.sdsp_hip_welch_process_host(p, xh.ctypes.data, S, channels, s1, 0, st_h.ctypes.data, acc_h.ctypes.data, bins) == 0
    tail = np.ascontiguousarray(xh[:, s1:])
    assert lib.sdsp_hip_welch_process_host(p, tail.ctypes.data, S - s1, channels, S - s1, s1, st_h.ctypes.data, acc_h.ctypes.data,
                                           bins) == 0
    assert np.array_equal(acc_h, acc.cpu().numpy())
    assert np.array_equal(st_h, st.cpu().numpy())
    out_h = np.zeros((channels, bins), dtype=_np(precision))
    assert lib.sdsp_hip_welch_finalize_host(p, acc_h.ctypes.data, bins, F, out_h.ctypes.data, bins, channels) == 0
    assert np.array_equal(out_h, out.cpu().numpy())
    assert lib.sdsp_hip_welch_finalize_host(p, acc_h.ctypes.data, bins, 0, out_h.ctypes.data, bins, channels) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_welch_process_host(p, xh.ctypes.data, S, channels, S, 5, None, acc_h.ctypes.data, bins) == L.ERR_INVALID_ARG
    wr = _rounded_window(scipy.signal.get_window("hann", n_fft), precision)
    acc_ref, _, _ = welch_ref(xh, n_fft, hop, wr, "linear")
    assert _peak_err(out_h, welch_psd(acc_ref, F, wr, 3.0, "spectrum")) <= _tol(precision)
