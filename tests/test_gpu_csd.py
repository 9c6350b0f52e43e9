"""GPU tests of the cross-spectral density and coherence bank (sdsp_hip_csd_*) on a real MI355X.

The checker is tests/csd_ref.py (double), itself pinned to scipy.signal.csd and scipy.signal.coherence in tests/test_csd_host.py.
With detrend NONE and one segment per call the sums are held bit for bit to a numpy sequential sum of conj(X_a) X_b in the
contract's operation order over the stft_bank's complex frames, and the auto sums to the Welch bank's."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal

from csd_ref import PAIRS, csd_coherence, csd_density, csd_inputs, csd_ref
from welch_ref import welch_frames

pytestmark = pytest.mark.gpu

N_F32 = [32, 256, 1024, 4096, 65536]
N_F64 = [32, 256, 1024, 4096, 32768]
CH = 4


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
    """max over rows of max_k |got - want| / max_k |want|"""
    got, want = np.asarray(got), np.asarray(want)
    return float((np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)).max())


def _rounded_window(w, precision):
    return w.astype(_np(precision)).astype(np.float64)


def _bank(sd, n_fft, hop, precision, pairs=PAIRS, channels=CH, **kw):
    kw.setdefault("window", scipy.signal.get_window("hann", n_fft))
    return sd.csd_bank(n_fft, hop, channels, pairs, precision=_prec(sd, precision), **kw)


def _hops(n_fft):
    return [n_fft // 2, n_fft // 4, 7 * n_fft // 32 + 1, n_fft]  # 7 N / 32 + 1 does not divide N


def _xy(bank):
    """acc_xy as a complex numpy array (npairs, bins)"""
    a = bank.acc_xy.cpu().numpy()
    return a[..., 0] + 1j * a[..., 1]


def _column(n_fft, precision, npairs=len(PAIRS), channels=CH):
    return channels * n_fft * (8 if precision == "f64" else 4) + (2 * npairs + channels) * (n_fft // 2 + 1) * 8


def _coherence_bound_f32(xy, au, pairs):
    """first-order bound on the coherence error from a 2e-5 peak-relative error of Pxy, Pxx and Pyy, per bin:
    2e-5 (2 max|Pxy| / sqrt(Pxx_k Pyy_k) + max Pxx / Pxx_k + max Pyy / Pyy_k), from the double reference"""
    pairs = np.asarray(pairs)
    pa, pb = au[pairs[:, 0]], au[pairs[:, 1]]
    with np.errstate(divide="ignore"):
        return 2e-5 * (2 * np.abs(xy).max(axis=-1, keepdims=True) / np.sqrt(pa * pb) + pa.max(axis=-1, keepdims=True) / pa
                       + pb.max(axis=-1, keepdims=True) / pb)


def _check_coherence(precision, got, xy, au, pairs, x64=None, kw=None):
    want = csd_coherence(xy, au, pairs)
    if precision == "f64":
        assert np.abs(got - want).max() <= 1e-12
        if x64 is not None:
            for i, (a, b) in enumerate(pairs):
                _, cw = scipy.signal.coherence(x64[a], x64[b], **kw)
                assert np.abs(got[i] - cw).max() <= 1e-12, i
    else:
        bound = _coherence_bound_f32(xy, au, pairs)
        assert bound.max() < 1  # every auto spectrum above 1e-4 of its peak (tests/test_csd_host.py): no bin is left out
        assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("detrend", ["none", "constant", "linear"])
@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("n_idx", range(5))
def test_against_reference_and_scipy(torch_cuda, sd, precision, detrend, scaling, n_idx):
    torch = torch_cuda
    n_fft = (N_F64 if precision == "f64" else N_F32)[n_idx]
    if n_idx == 4 and (detrend, scaling) != ("linear", "density"):
        return  # the largest N of each precision once
    w = scipy.signal.get_window("hann", n_fft)
    wr = _rounded_window(w, precision)
    fs = 1000.0
    for hop in _hops(n_fft)[:1 if n_idx == 4 else 4]:
        S = 6 * n_fft + 37
        x = np.concatenate([csd_inputs(n_fft, S, n_fft * 7 + hop), np.ones((CH, 3))], axis=1).astype(_np(precision))
        xd = torch.from_numpy(x).cuda()
        x_before = xd.clone()
        b = _bank(sd, n_fft, hop, precision, window=w, detrend=detrend, scaling=scaling, fs=fs)
        # two calls: the second one starts mid-hop and reads the history the first one left
        s1 = n_fft + hop // 2
        b.process(xd, samples=s1)
        b.process(xd[:, s1:].contiguous(), samples=S - s1)
        assert torch.equal(xd, x_before)
        F = (S - n_fft) // hop + 1
        assert b.frames == F
        got = b.csd().cpu().numpy()
        coh = b.coherence().cpu().numpy()
        x64 = x[:, :S].astype(np.float64)
        xy, au, F_ref, state = csd_ref(x64, PAIRS, n_fft, hop, wr, detrend)
        assert F_ref == F
        err = _peak_err(got, csd_density(xy, F, wr, fs, scaling))
        assert err <= _tol(precision), (hop, err)
        assert np.array_equal(b.state.cpu().numpy(), state.astype(_np(precision)))
        kw = dict(fs=fs, window=w, nperseg=n_fft, noverlap=n_fft - hop, detrend=False if detrend == "none" else detrend)
        if precision == "f64":
            for i, (a, c) in enumerate(PAIRS):
                _, sp = scipy.signal.csd(x64[a], x64[c], scaling=scaling, **kw)
                assert _peak_err(got[i], sp) <= 1e-12, (hop, i)
        _check_coherence(precision, coh, xy, au, PAIRS, x64, kw)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("detrend", [False, "constant", "linear"])
def test_one_shot_matches_scipy(torch_cuda, sd, precision, detrend):
    """The coherence of one bin is not compared: bin 0 of the boxcar window with detrending.  A detrended segment sums to zero
    under that window, so both auto spectra there are rounding residue (1e-31 of their peak in double) and the coherence is a
    ratio of residues: scipy.signal.coherence and tests/csd_ref.py, both in double, differ there by up to 0.13, while they agree
    to 6e-16 on every other bin.  The reference's own error is of order 1 at that bin, so no bound on it means anything; the
    cross-spectral density is compared there like everywhere else."""
    torch = torch_cuda
    x = csd_inputs(256, 10000, 11).astype(_np(precision))
    y = np.ascontiguousarray(x[[1, 3, 1, 3]])  # row by row: (0, 1), (1, 3), (2, 1), (3, 3)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    for nperseg, noverlap, window in [(256, None, "hann"), (256, 200, "hamming"), (1024, 0, "blackman"), (64, 63, "boxcar")]:
        kw = dict(fs=8000.0, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend)
        f, p = sd.csd(xd, yd, **kw)
        fw, pw = scipy.signal.csd(x64, y64, **kw)
        assert np.array_equal(f, fw)
        assert p.dtype == (torch.complex128 if precision == "f64" else torch.complex64) and p.shape == pw.shape
        assert _peak_err(p.cpu().numpy(), pw) <= _tol(precision), (nperseg, noverlap)
        f, c = sd.coherence(xd, yd, **kw)
        fw, cw = scipy.signal.coherence(x64, y64, **kw)
        assert np.array_equal(f, fw)
        assert c.dtype == xd.dtype and c.shape == cw.shape
        wr = _rounded_window(scipy.signal.get_window(window, nperseg), precision)
        hop = nperseg - (nperseg // 2 if noverlap is None else noverlap)
        pairs = [(i, 4 + i) for i in range(4)]
        xy, au, _, _ = csd_ref(np.concatenate([x64, y64]), pairs, nperseg, hop, wr, detrend or "none")
        residue = au <= 1e-20 * au.max(axis=-1, keepdims=True)  # an auto spectrum that is rounding residue (the docstring)
        assert np.array_equal(np.nonzero(residue.any(axis=0))[0], [0] if window == "boxcar" and detrend else [])
        live = ~(residue[:4] | residue[4:])
        err = np.abs(c.cpu().numpy() - cw)
        if precision == "f64":
            assert err[live].max() <= 1e-12
        else:
            bound = _coherence_bound_f32(xy, au, pairs)
            assert bound[live].max() < 1 and np.all(err[live] <= bound[live])
    f1, p1 = sd.csd(xd[0], yd[0], nperseg=128, detrend=detrend)
    _, pw1 = scipy.signal.csd(x64[0], y64[0], nperseg=128, detrend=detrend)
    assert p1.shape == pw1.shape and _peak_err(p1.cpu().numpy(), pw1) <= _tol(precision)
    for fn in (sd.csd, sd.coherence):
        with pytest.raises(ValueError, match="same shape"):
            fn(xd[0], yd[0, :4000])  # scipy zero-pads the shorter one
        with pytest.raises(ValueError, match="fewer samples"):
            fn(xd[0, :100], yd[0, :100])


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop", [(256, 64), (1024, 1024), (32, 5)])
def test_one_segment_per_call_is_a_sequential_double_sum(torch_cuda, sd, precision, n_fft, hop):
    torch = torch_cuda
    calls = 9
    w = scipy.signal.get_window("hann", n_fft)
    npdt = _np(precision)
    half = n_fft // 2
    S = n_fft + (calls - 1) * hop
    x = csd_inputs(n_fft, S, n_fft + hop).astype(npdt)
    b = _bank(sd, n_fft, hop, precision, window=w, detrend="none")
    wb = sd.welch_bank(n_fft, hop, CH, window=w, detrend="none", precision=_prec(sd, precision))
    frames = sd.stft_bank(n_fft, n_fft, CH, window=w, output="complex", precision=_prec(sd, precision))  # hop = N: no history
    acc = np.zeros((len(PAIRS), half + 1), dtype=np.complex128)
    pa, pb = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    pos = 0
    for m in range(calls):
        end = m * hop + n_fft
        blk = torch.from_numpy(np.ascontiguousarray(x[:, pos:end])).cuda()
        assert b.process(blk) == 1 and wb.process(blk) == 1
        pos = end
        # the call's own segment through the STFT bank: the same round_p(x w) and the same transform
        seg = torch.from_numpy(np.ascontiguousarray(x[:, m * hop:m * hop + n_fft])).cuda()
        z = frames.process(seg).cpu().numpy()[:, 0, :]  # (channels, bins)
        re, im = z.real.astype(np.float64), z.imag.astype(np.float64)
        ar, ai, br, bi = re[pa], im[pa], re[pb], im[pb]
        p = (ar * br + ai * bi) + 1j * (ar * bi - ai * br)
        p[:, 0] = ar[:, 0] * br[:, 0]           # bins 0 and N / 2: one product, im = +0
        p[:, half] = ar[:, half] * br[:, half]  # (the packed slot's imaginary part is bin N / 2's real part)
        acc = acc + p
        got = _xy(b)
        assert np.array_equal(got.real, acc.real) and np.array_equal(got.imag, acc.imag), m
        assert torch.equal(b.acc_auto, wb.acc), m


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("slicing", ["default", "one column", "three columns", "blocks"])
def test_conjugate_and_diagonal_identities(torch_cuda, sd, precision, slicing):
    torch = torch_cuda
    n_fft, hop = 256, 56
    S = 40 * n_fft + 5
    x = torch.from_numpy(csd_inputs(n_fft, S, 3).astype(_np(precision))).cuda()
    ws = {"one column": 1, "three columns": 3}.get(slicing, 0) * _column(n_fft, precision)
    b = _bank(sd, n_fft, hop, precision, detrend="linear", workspace_bytes=ws)
    if slicing == "blocks":
        pos = 0
        for blk in [300, 1, 2 * n_fft + 7, 17 * n_fft, S - 300 - 1 - 2 * n_fft - 7 - 17 * n_fft]:
            b.process(x[:, pos:pos + blk].contiguous())
            pos += blk
    else:
        b.process(x)
    xy, au = b.acc_xy.cpu().numpy(), b.acc_auto.cpu().numpy()
    i01, i33, i10 = PAIRS.index((0, 1)), PAIRS.index((3, 3)), PAIRS.index((1, 0))
    assert np.abs(xy[i01, :, 1]).max() > 0
    assert np.array_equal(xy[i10, :, 0].view(np.uint64), xy[i01, :, 0].view(np.uint64))  # equal bits
    assert np.array_equal(xy[i10, :, 1], -xy[i01, :, 1])
    assert np.all(xy[i33, :, 1] == 0)
    assert np.array_equal(xy[i33, :, 0].view(np.uint64), au[3].view(np.uint64))
    coh = b.coherence().cpu().numpy()
    assert np.all(au[3] > 0) and np.all(coh[i33] == 1)
    c = b.csd().cpu().numpy()
    assert np.array_equal(c[i10], np.conj(c[i01])) and np.all(c[i33].imag == 0)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n_fft,hop,detrend,S", [(256, 56, "linear", 0), (1024, 256, "constant", 0), (64, 64, "none", 0),
                                                 (32, 5, "constant", 32 + 5 * 330)])
def test_streaming_slicing_and_determinism(torch_cuda, sd, precision, n_fft, hop, detrend, S):
    torch = torch_cuda
    blocks = [0, 1, n_fft - 2, hop + 1, hop - 1, 0, 3, 6 * n_fft + 11, n_fft - 1, 2 * hop]
    if S:
        blocks.append(S - sum(blocks))  # more than 300 segments: R > 1 and several runs
    S = sum(blocks)
    x = csd_inputs(n_fft, S, n_fft + 3 * hop).astype(_np(precision))
    xd = torch.from_numpy(x).cuda()
    one = _bank(sd, n_fft, hop, precision, detrend=detrend)
    one.process(xd)
    F = (S - n_fft) // hop + 1
    want_xy, want_au = _xy(one), one.acc_auto.cpu().numpy()
    tol = 1e-14 if precision == "f64" else 1e-6
    # against the reference too, so that all of them agreeing on something wrong does not pass
    wr = _rounded_window(scipy.signal.get_window("hann", n_fft), precision)
    xy, au, _, _ = csd_ref(x.astype(np.float64), PAIRS, n_fft, hop, wr, detrend)
    assert _peak_err(want_xy, xy) <= _tol(precision) and _peak_err(want_au, au) <= _tol(precision)
    # ragged blocks
    bb = _bank(sd, n_fft, hop, precision, detrend=detrend)
    pos = 0
    for blk in blocks:
        got = bb.process(torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + blk])).cuda())
        assert got == welch_frames(n_fft, hop, pos, blk)
        pos += blk
    assert bb.frames == one.frames == F
    assert _peak_err(_xy(bb), want_xy) <= tol and _peak_err(bb.acc_auto.cpu().numpy(), want_au) <= tol
    assert np.array_equal(bb.state.cpu().numpy(), x[:, ::-1][:, :n_fft - 1])
    assert torch.equal(bb.state, one.state)
    # workspaces of 1, 2 and 5 segment columns
    column = _column(n_fft, precision)
    assert one.info()["column_bytes"] == column
    for k in (1, 2, 5):
        bk = _bank(sd, n_fft, hop, precision, detrend=detrend, workspace_bytes=k * column)
        assert bk.info()["workspace_bytes"] == k * column and bk.info()["slice_columns"] == k
        bk.process(xd)
        assert _peak_err(_xy(bk), want_xy) <= tol and _peak_err(bk.acc_auto.cpu().numpy(), want_au) <= tol, k
    # identical calls on identical plans: identical bits
    again = _bank(sd, n_fft, hop, precision, detrend=detrend)
    again.process(xd)
    assert torch.equal(again.acc_xy, one.acc_xy) and torch.equal(again.acc_auto, one.acc_auto)
    assert torch.equal(torch.view_as_real(again.csd()), torch.view_as_real(one.csd()))
    assert torch.equal(again.coherence(), one.coherence())


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_nan_stays_with_its_channel_and_rows_end_at_bins(torch_cuda, sd, precision):
    torch = torch_cuda
    L = sd._lib
    lib = sd.load()
    n_fft, hop, S = 256, 64, 2048
    bins = n_fft // 2 + 1
    x = csd_inputs(n_fft, S + 5, 8).astype(_np(precision))
    x[2, 700] = np.nan
    xd = torch.from_numpy(x).cuda()
    x_before = xd.clone()
    b = _bank(sd, n_fft, hop, precision, detrend="constant")
    b.info()
    acc = torch.full((len(PAIRS), 2 * bins + 6), -3.0, dtype=torch.float64, device=xd.device)
    acc[:, :2 * bins] = 0
    au = torch.full((CH, bins + 7), -4.0, dtype=torch.float64, device=xd.device)
    au[:, :bins] = 0
    st = torch.zeros((CH, n_fft - 1), dtype=xd.dtype, device=xd.device)
    assert lib.sdsp_hip_csd_process(b._plan, xd.data_ptr(), S + 5, S, 0, st.data_ptr(), acc.data_ptr(), 2 * bins + 6, au.data_ptr(),
                                    bins + 7, None) == 0
    F = welch_frames(n_fft, hop, 0, S)
    out = torch.full((len(PAIRS), 2 * bins + 4), -9.0, dtype=xd.dtype, device=xd.device)
    coh = torch.full((len(PAIRS), bins + 3), -8.0, dtype=xd.dtype, device=xd.device)
    assert lib.sdsp_hip_csd_finalize(b._plan, L.CSD_CROSS, acc.data_ptr(), 2 * bins + 6, au.data_ptr(), bins + 7, F, out.data_ptr(),
                                     2 * bins + 4, None) == 0
    assert lib.sdsp_hip_csd_finalize(b._plan, L.CSD_COHERENCE, acc.data_ptr(), 2 * bins + 6, au.data_ptr(), bins + 7, F,
                                     coh.data_ptr(), bins + 3, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x_before.cpu().numpy(), equal_nan=True)  # in is never written
    assert torch.all(acc[:, 2 * bins:] == -3.0) and torch.all(au[:, bins:] == -4.0)
    assert torch.all(out[:, 2 * bins:] == -9.0) and torch.all(coh[:, bins:] == -8.0)
    o = out[:, :2 * bins].cpu().numpy()
    o = o[:, 0::2] + 1j * o[:, 1::2]
    c = coh[:, :bins].cpu().numpy()
    a = au[:, :bins].cpu().numpy()
    with2 = [i for i, p in enumerate(PAIRS) if 2 in p]
    keep = [i for i, p in enumerate(PAIRS) if 2 not in p]
    assert with2 and np.isnan(o[with2].real).all() and np.isnan(c[with2]).all() and np.isnan(a[2]).all()
    assert np.isfinite(o[keep]).all() and np.isfinite(c[keep]).all() and np.isfinite(a[[0, 1, 3]]).all()
    wr = _rounded_window(scipy.signal.get_window("hann", n_fft), precision)
    x64 = np.nan_to_num(x[:, :S].astype(np.float64))
    xy, au_ref, _, _ = csd_ref(x64, PAIRS, n_fft, hop, wr, "constant")
    assert _peak_err(o[keep], csd_density(xy, F, wr)[keep]) <= _tol(precision)
    _check_coherence(precision, c[keep], xy[keep], au_ref, [PAIRS[i] for i in keep])


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
    n_fft, hop, S = 1024, 256, 256 * 16 + 100
    ws = 5 * _column(n_fft, precision)
    x = torch.from_numpy(csd_inputs(n_fft, S, 4).astype(_np(precision))).cuda()
    eager = _bank(sd, n_fft, hop, precision, workspace_bytes=ws)
    eager.process(x)
    want, want_coh = eager.csd(), eager.coherence()
    g_bank = _bank(sd, n_fft, hop, precision, workspace_bytes=ws)
    g_bank._ensure_plan()
    g_bank._ensure_buffers()  # plan, history and sums outside the capture
    out, coh = torch.empty_like(want), torch.empty_like(want_coh)
    pos0 = g_bank.position
    launches = g_bank.launches(S, finalize=True) + 1  # two finalize launches
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_bank.process(x)
        g_bank.csd(out=out)
        g_bank.coherence(out=coh)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(want)) and torch.equal(coh, want_coh)
    assert torch.equal(g_bank.state, eager.state)
    assert torch.equal(g_bank.acc_xy, eager.acc_xy) and torch.equal(g_bank.acc_auto, eager.acc_auto)
    # the kernel nodes of one process + two finalize calls: a fresh bank at the same position
    c_bank = _bank(sd, n_fft, hop, precision, workspace_bytes=ws)
    c_bank._ensure_plan()
    c_bank._ensure_buffers()
    c_bank.frames = 1
    assert c_bank.position == pos0
    n = _kernel_nodes(torch, lambda: (c_bank.process(x), c_bank.csd(out=out), c_bank.coherence(out=coh)))
    assert n == launches, (n, launches)
    assert c_bank.launches(0) == 0


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_errors_and_host_paths(torch_cuda, sd, precision):
    torch = torch_cuda
    L = sd._lib
    lib = sd.load()
    n_fft, hop, S = 256, 56, 1000
    bins = n_fft // 2 + 1
    NP = len(PAIRS)
    rs = 8 if precision == "f64" else 4
    b = _bank(sd, n_fft, hop, precision, detrend="linear", scaling="spectrum", fs=3.0)
    info = b.info()
    assert (info["n_fft"], info["hop"], info["bins"], info["hist"]) == (n_fft, hop, bins, n_fft - 1)
    assert (info["detrend"], info["scaling"], info["fs"], info["precision"]) == (L.DETREND_LINEAR, L.SCALING_SPECTRUM, 3.0,
                                                                                 _prec(sd, precision))
    assert (info["channels"], info["npairs"], info["column_bytes"]) == (CH, NP, _column(n_fft, precision))
    assert info["kernel"] and info["workspace_bytes"] == info["slice_columns"] * info["column_bytes"] > 0
    p = b._plan
    x = torch.from_numpy(csd_inputs(n_fft, S, 5).astype(_np(precision))).cuda()
    acc = torch.zeros((NP, 2 * bins), dtype=torch.float64, device=x.device)
    au = torch.zeros((CH, bins), dtype=torch.float64, device=x.device)
    st = torch.zeros((CH, n_fft - 1), dtype=x.dtype, device=x.device)
    out = torch.zeros((NP, 2 * bins), dtype=x.dtype, device=x.device)
    coh = torch.zeros((NP, bins), dtype=x.dtype, device=x.device)

    def run(i=x.data_ptr(), istr=S, s=S, pos=0, state=st.data_ptr(), a=acc.data_ptr(), astr=2 * bins, u=au.data_ptr(), ustr=bins,
            plan=p):
        return lib.sdsp_hip_csd_process(plan, i, istr, s, pos, state, a, astr, u, ustr, None)

    def fin(mode=L.CSD_CROSS, a=acc.data_ptr(), astr=2 * bins, u=au.data_ptr(), ustr=bins, frames=5, o=out.data_ptr(),
            ostr=2 * bins, plan=p):
        return lib.sdsp_hip_csd_finalize(plan, mode, a, astr, u, ustr, frames, o, ostr, None)

    assert run(plan=None) == L.ERR_INVALID_ARG
    assert run(i=None) == L.ERR_INVALID_ARG
    assert run(a=None) == L.ERR_INVALID_ARG
    assert run(state=None, pos=10) == L.ERR_INVALID_ARG
    assert run(istr=S - 1) == L.ERR_INVALID_ARG
    assert run(astr=2 * bins - 1) == L.ERR_INVALID_ARG
    assert run(ustr=bins - 1) == L.ERR_INVALID_ARG
    assert run(state=x.data_ptr() + 64) == L.ERR_INVALID_ARG  # in overlaps state
    assert run(a=x.data_ptr() + 64) == L.ERR_INVALID_ARG  # in overlaps acc_xy
    assert run(u=x.data_ptr() + 64) == L.ERR_INVALID_ARG  # in overlaps acc_auto
    assert run(u=acc.data_ptr() + 64) == L.ERR_INVALID_ARG  # the accumulators overlap
    assert run(i=x.data_ptr() + 1) == L.ERR_INVALID_ARG  # misaligned
    assert run(a=acc.data_ptr() + 4) == L.ERR_INVALID_ARG
    assert run(pos=1 << 63, s=1 << 63) == L.ERR_INVALID_SIZE
    assert run(s=0) == 0 and run(s=0, i=None, a=None) == 0
    assert fin(plan=None) == L.ERR_INVALID_ARG
    assert fin(mode=2) == L.ERR_INVALID_ARG
    assert fin(frames=0) == L.ERR_INVALID_SIZE
    assert fin(a=None) == L.ERR_INVALID_ARG and fin(o=None) == L.ERR_INVALID_ARG
    assert fin(astr=2 * bins - 1) == L.ERR_INVALID_ARG and fin(ostr=2 * bins - 1) == L.ERR_INVALID_ARG
    assert fin(o=acc.data_ptr() + 8) == L.ERR_INVALID_ARG  # acc_xy overlaps out
    assert fin(mode=L.CSD_COHERENCE, u=None, o=coh.data_ptr(), ostr=bins) == L.ERR_INVALID_ARG  # coherence needs acc_auto
    assert fin(mode=L.CSD_COHERENCE, o=coh.data_ptr(), ostr=bins - 1) == L.ERR_INVALID_ARG
    assert fin(mode=L.CSD_COHERENCE, o=coh.data_ptr(), ostr=bins, ustr=bins - 1) == L.ERR_INVALID_ARG
    assert fin(mode=L.CSD_COHERENCE, o=au.data_ptr() + 8, ostr=bins) == L.ERR_INVALID_ARG  # acc_auto overlaps out
    torch.cuda.synchronize()
    assert torch.all(acc == 0) and torch.all(au == 0) and torch.all(st == 0) and torch.all(out == 0) and torch.all(coh == 0)
    nb = C.c_uint64(0)
    assert lib.sdsp_hip_csd_state_bytes(p, C.byref(nb)) == 0 and nb.value == CH * (n_fft - 1) * rs
    assert lib.sdsp_hip_csd_plan_launches(p, S, 0, None) == L.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        b.csd()  # no segment yet
    no_auto = _bank(sd, n_fft, hop, precision, auto=False)
    no_auto.process(x)
    assert no_auto.acc_auto is None
    with pytest.raises(ValueError):
        no_auto.coherence()
    # the host entries equal the device entries, history included: two calls from position 0
    s1 = 300
    assert run(s=s1) == 0 and run(i=x.data_ptr() + s1 * rs, s=S - s1, pos=s1) == 0
    F = welch_frames(n_fft, hop, 0, S)
    assert fin(frames=F) == 0 and fin(mode=L.CSD_COHERENCE, frames=F, o=coh.data_ptr(), ostr=bins) == 0
    torch.cuda.synchronize()
    # without auto spectra the cross sums are the same bits
    with_auto = _bank(sd, n_fft, hop, precision, detrend="linear")
    with_auto.process(x)
    no_auto2 = _bank(sd, n_fft, hop, precision, detrend="linear", auto=False)
    no_auto2.process(x)
    assert torch.equal(with_auto.acc_xy, no_auto2.acc_xy)
    xh = x.cpu().numpy()
    acc_h, au_h = np.zeros((NP, 2 * bins)), np.zeros((CH, bins))
    st_h = np.zeros((CH, n_fft - 1), dtype=_np(precision))
    assert lib.sdsp_hip_csd_process_host(p, xh.ctypes.data, S, s1, 0, st_h.ctypes.data, acc_h.ctypes.data, 2 * bins, au_h.ctypes.data,
                                         bins) == 0
    tail = np.ascontiguousarray(xh[:, s1:])
    assert lib.sdsp_hip_csd_process_host(p, tail.ctypes.data, S - s1, S - s1, s1, st_h.ctypes.data, acc_h.ctypes.data, 2 * bins,
                                         au_h.ctypes.data, bins) == 0
    assert np.array_equal(acc_h, acc.cpu().numpy()) and np.array_equal(au_h, au.cpu().numpy())
    assert np.array_equal(st_h, st.cpu().numpy())
    out_h, coh_h = np.zeros((NP, 2 * bins), dtype=_np(precision)), np.zeros((NP, bins), dtype=_np(precision))
    assert lib.sdsp_hip_csd_finalize_host(p, L.CSD_CROSS, acc_h.ctypes.data, 2 * bins, au_h.ctypes.data, bins, F, out_h.ctypes.data,
                                          2 * bins) == 0
    assert lib.sdsp_hip_csd_finalize_host(p, L.CSD_COHERENCE, acc_h.ctypes.data, 2 * bins, au_h.ctypes.data, bins, F,
                                          coh_h.ctypes.data, bins) == 0
    assert np.array_equal(out_h, out.cpu().numpy()) and np.array_equal(coh_h, coh.cpu().numpy())
    assert lib.sdsp_hip_csd_finalize_host(p, L.CSD_CROSS, acc_h.ctypes.data, 2 * bins, None, 0, 0, out_h.ctypes.data,
                                          2 * bins) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_csd_finalize_host(p, L.CSD_COHERENCE, acc_h.ctypes.data, 2 * bins, None, 0, F, coh_h.ctypes.data,
                                          bins) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_csd_process_host(p, xh.ctypes.data, S, S, 5, None, acc_h.ctypes.data, 2 * bins, None, 0) == L.ERR_INVALID_ARG
    wr = _rounded_window(scipy.signal.get_window("hann", n_fft), precision)
    xy, au_ref, _, _ = csd_ref(xh.astype(np.float64), PAIRS, n_fft, hop, wr, "linear")
    got = out_h[:, 0::2] + 1j * out_h[:, 1::2]
    assert _peak_err(got, csd_density(xy, F, wr, 3.0, "spectrum")) <= _tol(precision)
    _check_coherence(precision, coh_h, xy, au_ref, PAIRS)
