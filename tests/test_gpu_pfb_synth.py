"""GPU tests of the polyphase synthesis banks (sdsp_hip_pfb_synth_*) on a real MI355X.

The checker is tests/pfb_synth_ref.py (double), itself pinned to tests/pfb_ref.py and tests/istft_ref.py in
tests/test_pfb_synth_host.py.  Every case is also held bit for bit to the composition a user writes with the library alone: copy / pack
-> FftPlan(M, RADIX_AUTO) / RfftPlan reverse -> torch.roll per frame (TIME) -> tile P times x g in the plan precision -> the pending
sums, then strided adds in ascending frame order."""
import ctypes as C

import numpy as np
import pytest

from pfb_ref import pfb_shifts
from pfb_synth_ref import pfb_synth_frames_ref, pfb_synth_ref

pytestmark = pytest.mark.gpu

MS = [16, 32, 256, 1024, 4096]
TAPS_PER_CHANNEL = [1, 3, 8]
EPS64 = np.finfo(np.float64).eps
POSITION = 1234567  # not a multiple of 4: TIME rotations that split a 16-byte vector


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


def _bound(precision, m, p, hop, vmax):
    """K (tol(M) + (K + 1) eps) max|v|, K = ceil(L / D) covering frames per output: K transform errors of the project's bound (f32 2e-6,
    f64 4 M eps, relative to max|v|) plus K roundings each of a product and of a sum of at most K + 1 terms no larger than max|v|"""
    K = -(-m * p // hop)
    tol = 4 * m * EPS64 if precision == "f64" else 2e-6
    eps = np.finfo(_np(precision, False)).eps
    return K * (tol + (K + 1) * eps) * vmax


def _hops(m):
    return [m, m // 2, m // 4, 3 * m // 4] + ([1] if m <= 32 else [])


def _frames(m, p, hop):
    return 6 if m == 4096 else p * m // hop + 3


def _streams(m, p, hop):
    return [1, 3] + ([130] if m <= 256 and hop >= m // 4 and p <= 3 else [])


def _spectra(rng, shape, precision):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(_np(precision, True))


def _bank(sd, m, p, hop, streams, precision, cplx, phase, taps, **kw):
    return sd.pfb_synthesis_bank(m, p, hop, streams=streams, taps=taps, output="complex" if cplx else "real", phase=phase,
                                 precision=_prec(sd, precision), **kw)


SENT_IN, SENT_OUT = 3.0 - 5.0j, 7.0


def _call(torch, sd, b, X, position, pending, pad_in=0, pad_out=0, null_state=False):
    """the C entry on rows padded by pad_in bins / pad_out samples of sentinels; returns (out (streams, F D), state tensor or None)"""
    lib = sd.load()
    b._ensure_plan()
    streams, F = X.shape[0], X.shape[1]
    S = F * b.hop
    in_stride, out_stride = F * b.bins + pad_in, S + pad_out
    xin = np.full((streams, in_stride), SENT_IN, dtype=X.dtype)
    xin[:, :F * b.bins] = X.reshape(streams, -1)
    xd = torch.from_numpy(xin).cuda()
    before = xd.clone()
    out = torch.full((streams, out_stride), SENT_OUT, dtype=b._out_dtype(), device="cuda")
    st = None
    if b.hist and not null_state:
        st = torch.from_numpy(np.ascontiguousarray(pending)).cuda()
        assert st.shape == (streams, b.hist) and st.dtype == b._out_dtype()
    sd.pfb_synth.L.check(lib.sdsp_hip_pfb_synth_process(b._plan, xd.data_ptr(), in_stride, out.data_ptr(), out_stride, streams, F,
                                                        position, st.data_ptr() if st is not None else None,
                                                        torch.cuda.current_stream().cuda_stream))
    assert torch.equal(xd, before)  # in is never written
    assert torch.equal(out[:, S:], torch.full_like(out[:, S:], SENT_OUT))  # nothing past each stream's F D outputs
    return out[:, :S], st


def _compose(torch, sd, Xd, pending, m, p, hop, g, precision, cplx, phase, position, variant=0):
    """the library-only synthesis; Xd (streams, F, bins) device tensor; returns (y, tail)"""
    Cn, F = Xd.shape[0], Xd.shape[1]
    Lt, H = m * p, m * p - hop
    rdt = torch.float64 if precision == "f64" else torch.float32
    if cplx:
        plan = sd.FftPlan(m, 0, sd.reverse_fft, _prec(sd, precision), max_batch=max(Cn * F, 1))  # radix 0: SDSP_HIP_RADIX_AUTO
        if variant:
            plan.set_variant(variant)
        v = plan.exec(Xd.clone().contiguous())
    else:
        half = m // 2
        packed = torch.empty((Cn, F, half), dtype=Xd.dtype, device=Xd.device)
        packed[..., 1:] = Xd[..., 1:half]
        packed[..., 0] = torch.complex(Xd[..., 0].real, Xd[..., half].real)
        plan = sd.RfftPlan(m, 2, sd.reverse_fft, max_batch=max(Cn * F, 1), precision=_prec(sd, precision))
        if variant:
            plan.set_variant(variant)
        v = plan.exec(torch.view_as_real(packed).reshape(Cn, F, m).contiguous())
    if phase == "time":
        s = pfb_shifts(m, p, hop, F, position)
        v = torch.stack([torch.roll(v[:, j], -int(s[j]), dims=-1) for j in range(F)], dim=1)  # u[r] = v[(r + s) mod M]
    gt = torch.from_numpy(g).to(rdt).cuda()
    t = v.repeat(1, 1, p)
    y = torch.complex(t.real * gt, t.imag * gt) if cplx else t * gt  # every product rounded in the plan precision
    a = torch.zeros((Cn, F * hop + H), dtype=y.dtype, device=y.device)
    if pending is not None and H:
        a[:, :H] = pending
    for j in range(F):
        a[:, j * hop:j * hop + Lt] += y[:, j]
    return a[:, :F * hop], a[:, F * hop:]


def _pending(rng, streams, hist, precision, cplx, scale):
    x = rng.uniform(-1, 1, (streams, max(hist, 1)))
    if cplx:
        x = x + 1j * rng.uniform(-1, 1, (streams, max(hist, 1)))
        x = x / np.sqrt(2)
    return (x * scale).astype(_np(precision, cplx))[:, :hist]


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m", MS)
def test_against_reference_and_composition(torch_cuda, sd, precision, cplx, m):
    torch = torch_cuda
    if m == 16 and not cplx:
        with pytest.raises(sd.SdspHipError) as e:  # the real-input plans start at 32, as for the analysis bank
            _bank(sd, 16, 1, 16, 1, precision, False, "time", np.ones(16))._ensure_plan()
        assert e.value.code == sd._lib.ERR_UNSUPPORTED
        return
    bins = m if cplx else m // 2 + 1
    worst = 0.0
    for p in TAPS_PER_CHANNEL:
        for hop in _hops(m):
            F = _frames(m, p, hop)
            for streams in _streams(m, p, hop):
                rng = np.random.default_rng(m * 7 + hop * 3 + streams + p)
                Lt, H = m * p, m * p - hop
                g = rng.uniform(-1, 1, Lt)
                g_p = g.astype(_np(precision, False)).astype(np.float64)  # rounded once to the plan precision
                X = _spectra(rng, (streams, F, bins), precision)
                pad = (3, 5) if streams == 3 else (0, 0)  # odd strides
                for phase in ("frame", "time"):
                    vmax = np.abs(pfb_synth_frames_ref(X, m, p, hop, phase, POSITION, cplx)).max()
                    pend = _pending(rng, streams, H, precision, cplx, vmax)
                    want, want_state = pfb_synth_ref(X, m, p, hop, g_p, pend if H else None, phase, POSITION, cplx=cplx)
                    b = _bank(sd, m, p, hop, streams, precision, cplx, phase, g)
                    y, st = _call(torch, sd, b, X, POSITION, pend, *pad)
                    got = y.cpu().numpy()
                    err = np.abs(got - want).max()
                    if H:
                        err = max(err, np.abs(st.cpu().numpy() - want_state).max())
                    bound = _bound(precision, m, p, hop, vmax)
                    worst = max(worst, err / bound)
                    assert err <= bound, (p, hop, streams, phase, err, bound)
                    ref, ref_tail = _compose(torch, sd, torch.from_numpy(X).cuda(), torch.from_numpy(pend).cuda() if H else None, m, p,
                                             hop, g, precision, cplx, phase, POSITION)
                    assert torch.equal(y, ref), (p, hop, streams, phase)
                    if H:
                        assert torch.equal(st, ref_tail), (p, hop, streams, phase)
                    want_form = "sliding" if hop == m else "plain"
                    assert b.info()["unfold"] == want_form
                    if hop == m and streams == 3:  # the plain form gives the sliding form's bits
                        b2 = _bank(sd, m, p, hop, streams, precision, cplx, phase, g)
                        b2._set_unfold_form(1)
                        assert b2.info()["unfold"] == "plain"
                        y2, st2 = _call(torch, sd, b2, X, POSITION, pend, *pad)
                        assert torch.equal(y2, y) and (not H or torch.equal(st2, st))
    print(f"pfb synthesis {precision} {'complex' if cplx else 'real'} M={m}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_the_two_limits(torch_cuda, sd, precision, cplx):
    """P = 1, D = M: the reverse transform times g; P = 1, FRAME, REAL: istft_bank(RAW) with window g, bit for bit"""
    torch = torch_cuda
    m, F, streams = 256, 7, 3
    rng = np.random.default_rng(5)
    bins = m if cplx else m // 2 + 1
    g = rng.uniform(-1, 1, m)
    X = torch.from_numpy(_spectra(rng, (streams, F, bins), precision)).cuda()
    b = _bank(sd, m, 1, m, streams, precision, cplx, "frame", g)
    assert b.hist == 0
    ref, _ = _compose(torch, sd, X, None, m, 1, m, g, precision, cplx, "frame", 0)
    assert torch.equal(b.process(X), ref)
    if not cplx:
        for hop in (64, 96, 7):
            bi = sd.istft_bank(m, hop, channels=streams, window=g, normalized=False, precision=_prec(sd, precision))
            bs = _bank(sd, m, 1, hop, streams, precision, False, "frame", g)
            for n in (2, 5):
                assert torch.equal(bs.process(X[:, :n].contiguous()), bi.process(X[:, :n].contiguous()))
            assert torch.equal(bs.state, bi.state)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m,p,hop", [(32, 3, 8), (256, 8, 128), (256, 3, 192), (1024, 8, 1024), (64, 2, 1)])
def test_blockwise_equals_one_call(torch_cuda, sd, precision, cplx, m, p, hop):
    torch = torch_cuda
    rng = np.random.default_rng(m + hop + p)
    Lt = m * p
    blocks = [1, 3, 0, 7, 1, 2 * (Lt // hop) + 1, 2]  # F D < hist, an empty call, one past the history
    if (Lt - hop) > hop:
        assert blocks[0] * hop < Lt - hop
    F, streams = sum(blocks), 5
    bins = m if cplx else m // 2 + 1
    X = _spectra(rng, (streams, F, bins), precision)
    Xd = torch.from_numpy(X).cuda()
    g = rng.uniform(-1, 1, Lt)
    for phase in ("frame", "time"):
        one = _bank(sd, m, p, hop, streams, precision, cplx, phase, g)
        want = one.process(Xd)
        assert one.position == F * hop
        b = _bank(sd, m, p, hop, streams, precision, cplx, phase, g)
        outs, at = [], 0
        for n in blocks:
            outs.append(b.process(Xd[:, at:at + n].contiguous()))
            at += n
            assert b.position == at * hop
        assert torch.equal(torch.cat(outs, dim=1), want)
        assert torch.equal(b.state, one.state)
        ref, ref_state = pfb_synth_ref(X, m, p, hop, g.astype(_np(precision, False)).astype(np.float64), None, phase, 0, cplx=cplx)
        vmax = np.abs(pfb_synth_frames_ref(X, m, p, hop, phase, 0, cplx)).max()
        assert np.abs(want.cpu().numpy() - ref).max() <= _bound(precision, m, p, hop, vmax)
        assert np.abs(one.state.cpu().numpy()[:, :Lt - hop] - ref_state).max() <= _bound(precision, m, p, hop, vmax)
        b.reset()
        assert b.position == 0 and b.state is None
        assert torch.equal(b.process(Xd), want)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("hop", [256, 128, 192])
def test_small_workspaces_equal_the_default(torch_cuda, sd, precision, cplx, hop):
    torch = torch_cuda
    m, p, streams, F = 256, 3, 5, 9
    rng = np.random.default_rng(hop)
    bins = m if cplx else m // 2 + 1
    Xd = torch.from_numpy(_spectra(rng, (streams, F, bins), precision)).cuda()
    g = rng.uniform(-1, 1, m * p)
    full = _bank(sd, m, p, hop, streams, precision, cplx, "time", g)
    want = full.process(Xd)
    unit = m * np.dtype(_np(precision, cplx)).itemsize
    for frames in range(1, 8):  # slices that start and end inside a stream
        b = _bank(sd, m, p, hop, streams, precision, cplx, "time", g, workspace_bytes=frames * unit)
        assert b.info()["workspace_bytes"] == frames * unit
        assert b.launches(F) >= -(-streams * F // frames) * 3
        assert torch.equal(b.process(Xd), want), frames
        assert torch.equal(b.state, full.state), frames


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("phase", ["frame", "time"])
@pytest.mark.parametrize("m,p,hop,cplx", [(64, 3, 16, False), (64, 3, 16, True), (16, 4, 8, True)])  # real streams start at M = 32
def test_round_trip_through_the_analysis_bank(torch_cuda, sd, precision, cplx, phase, m, p, hop):
    torch = torch_cuda
    rng = np.random.default_rng(m + hop)
    Lt, H, streams = m * p, m * p - hop, 3
    h = sd.pfb_prototype("blackman" if m == 64 else "hamming", m, p)
    g = sd.pfb_dual_prototype(h, m, p, hop)
    S = (3 * Lt // hop + 5) * hop
    x = rng.standard_normal((streams, S))
    if cplx:
        x = x + 1j * rng.standard_normal((streams, S))
    x = x.astype(_np(precision, cplx))
    kind = "complex" if cplx else "real"
    ana = sd.pfb_bank(m, p, hop, streams=streams, taps=h, input=kind, phase=phase, precision=_prec(sd, precision))
    syn = _bank(sd, m, p, hop, streams, precision, cplx, phase, g)
    xd = torch.from_numpy(x).cuda()
    half = (S // hop // 2) * hop
    y = torch.cat([syn.process(ana.process(xd[:, :half].contiguous())), syn.process(ana.process(xd[:, half:].contiguous()))], dim=1)
    want = np.concatenate([np.zeros((streams, H), dtype=x.dtype), x], axis=1)[:, :S]
    err = np.abs(y.cpu().numpy() - want).max() / (np.abs(x).max() * np.abs(g).max())
    print(f"round trip {precision} {kind} {phase} ({m}, {p}, {hop}): err {err:.3e}")
    assert err <= (1e-10 if precision == "f64" else 1e-4)
    # a window name is the dual of that window's prototype
    named = sd.pfb_synthesis_bank(m, p, hop, taps="blackman" if m == 64 else "hamming", output=kind)
    assert np.array_equal(named.taps, g)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m,p,hop", [(64, 4, 64), (64, 4, 16), (64, 3, 48)])
def test_nan_reaches_exactly_the_positions_its_frame_covers(torch_cuda, sd, precision, cplx, m, p, hop):
    torch = torch_cuda
    Lt, F, streams, jn = m * p, 24, 2, 5
    bins = m if cplx else m // 2 + 1
    rng = np.random.default_rng(3)
    X = _spectra(rng, (streams, F, bins), precision)
    X[1, jn, 3] = np.nan
    for phase in ("frame", "time"):
        b = _bank(sd, m, p, hop, streams, precision, cplx, phase, rng.uniform(0.5, 1, Lt))
        y = b.process(torch.from_numpy(X).cuda())
        full = torch.cat([y, b.state[:, :b.hist]], dim=1).cpu().numpy()
        has_nan = np.isnan(full)
        covered = np.zeros(F * hop + Lt - hop, dtype=bool)
        covered[jn * hop:jn * hop + Lt] = True
        assert np.array_equal(has_nan[1], covered)
        assert not has_nan[0].any()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("hop", [64, 256, 37])
def test_sentinels_null_state_launches_graph_and_host_entry(torch_cuda, sd, precision, cplx, hop):
    torch = torch_cuda
    lib = sd.load()
    check = sd.pfb_synth.L.check
    m, p, streams, F = 256, 3, 3, 11
    S, H = F * hop, m * p - hop
    bins = m if cplx else m // 2 + 1
    rng = np.random.default_rng(11)
    X = _spectra(rng, (streams, F, bins), precision)
    g = rng.uniform(-1, 1, m * p)
    pend = _pending(rng, streams, H, precision, cplx, 0.1)
    b = _bank(sd, m, p, hop, streams, precision, cplx, "time", g)
    want, want_state = _call(torch, sd, b, X, POSITION, pend)
    # padded rows (odd strides) keep their sentinels (checked in _call); the state sits between guard elements that stay intact
    guard = 5
    buf = torch.full((guard + streams * H + guard,), -9.0, dtype=b._out_dtype(), device="cuda")
    buf[guard:guard + streams * H] = torch.from_numpy(pend).cuda().reshape(-1)
    in_stride, out_stride = F * bins + 3, S + 5
    xin = np.full((streams, in_stride), SENT_IN, dtype=X.dtype)
    xin[:, :F * bins] = X.reshape(streams, -1)
    xd = torch.from_numpy(xin).cuda()
    out = torch.full((streams, out_stride), SENT_OUT, dtype=b._out_dtype(), device="cuda")
    esz = buf.element_size()
    check(lib.sdsp_hip_pfb_synth_process(b._plan, xd.data_ptr(), in_stride, out.data_ptr(), out_stride, streams, F, POSITION,
                                         buf.data_ptr() + guard * esz, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(out[:, :S], want) and torch.equal(out[:, S:], torch.full_like(out[:, S:], SENT_OUT))
    assert torch.equal(buf[guard:guard + streams * H].view(streams, H), want_state)
    assert torch.equal(buf[:guard], torch.full_like(buf[:guard], -9.0)) and torch.equal(buf[-guard:], torch.full_like(buf[-guard:], -9.0))
    # NULL state: start from zero, drop the tail
    y0, _ = _call(torch, sd, b, X, POSITION, None, 3, 5, null_state=True)
    z0, _ = _call(torch, sd, b, X, POSITION, np.zeros_like(pend))
    assert torch.equal(y0, z0)
    # the launch count is what plan_launches says: kernel nodes of a captured stream; the replay equals the eager call
    Xd = torch.from_numpy(X).cuda()
    g_state = torch.from_numpy(pend).cuda()
    g_out = torch.zeros_like(want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            check(lib.sdsp_hip_pfb_synth_process(b._plan, Xd.data_ptr(), F * bins, g_out.data_ptr(), S, streams, F, POSITION,
                                                 g_state.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    g_state.copy_(torch.from_numpy(pend).cuda())
    g_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, want) and torch.equal(g_state, want_state)
    small = _bank(sd, m, p, hop, streams, precision, cplx, "time", g, workspace_bytes=4 * m * np.dtype(_np(precision, cplx)).itemsize)
    for bank in (b, small):
        bank._ensure_plan()
        st = torch.from_numpy(pend).cuda()
        o = torch.zeros_like(want)
        made = _kernel_nodes(torch, lambda: check(lib.sdsp_hip_pfb_synth_process(
            bank._plan, Xd.data_ptr(), F * bins, o.data_ptr(), S, streams, F, POSITION, st.data_ptr(),
            torch.cuda.current_stream().cuda_stream)))
        assert made == bank.launches(F) and made >= 4
    # the host entry equals the device entry
    h_out = np.zeros((streams, S), dtype=_np(precision, cplx))
    h_state = pend.copy()
    check(lib.sdsp_hip_pfb_synth_process_host(b._plan, np.ascontiguousarray(X).ctypes.data, F * bins, h_out.ctypes.data, S, streams, F,
                                              POSITION, h_state.ctypes.data))
    assert np.array_equal(h_out, want.cpu().numpy()) and np.array_equal(h_state, want_state.cpu().numpy())


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
        kernels = 0
        for i in range(n.value):
            t = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(t)) == 0
            kernels += t.value == 0  # hipGraphNodeTypeKernel
        return kernels
    finally:
        hip.hipGraphDestroy(graph)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_inner_variant_one_agrees_within_the_tolerance(torch_cuda, sd, precision, cplx):
    """the inner reverse transform's alternate kernel where the size has one: within the tolerance of the reference, and bit for bit
    the composition with that variant.  16384 joins the sizes: the real-input plans in double have an alternate only at 8192 / 16384"""
    torch = torch_cuda
    agreed = 0
    for m in (MS + [16384])[0 if cplx else 1:]:
        p, hop, streams, F = 3, m // 2, 3, 12
        rng = np.random.default_rng(m)
        bins = m if cplx else m // 2 + 1
        X = _spectra(rng, (streams, F, bins), precision)
        g = rng.uniform(-1, 1, m * p)
        b = _bank(sd, m, p, hop, streams, precision, cplx, "time", g)
        try:
            b.set_variant(1)
        except sd.SdspHipError as e:
            assert e.code == sd._lib.ERR_UNSUPPORTED
            continue
        y = b.process(torch.from_numpy(X).cuda())
        want, _ = pfb_synth_ref(X, m, p, hop, g.astype(_np(precision, False)).astype(np.float64), None, "time", 0, cplx=cplx)
        vmax = np.abs(pfb_synth_frames_ref(X, m, p, hop, "time", 0, cplx)).max()
        assert np.abs(y.cpu().numpy() - want).max() <= _bound(precision, m, p, hop, vmax), m
        ref, _ = _compose(torch, sd, torch.from_numpy(X).cuda(), None, m, p, hop, g, precision, cplx, "time", 0, variant=1)
        assert torch.equal(y, ref), m
        assert b.info()["kernel"]
        agreed += 1
    assert agreed > 0
    with pytest.raises(ValueError):
        b.set_variant(-1)


def test_process_errors(torch_cuda, sd):
    torch = torch_cuda
    lib = sd.load()
    L = sd.pfb_synth.L
    for cplx in (False, True):
        b = _bank(sd, 64, 4, 32, 2, "f32", cplx, "time", np.ones(256))
        b._ensure_plan()
        odt = torch.complex64 if cplx else torch.float32
        X = torch.zeros((2, 4, b.bins), dtype=torch.complex64, device="cuda")
        out = torch.zeros((2, 128), dtype=odt, device="cuda")
        st = torch.zeros((2, b.hist), dtype=odt, device="cuda")

        def call(in_ptr=X.data_ptr(), in_stride=4 * b.bins, out_ptr=out.data_ptr(), out_stride=128, streams=2, frames=4,
                 state=st.data_ptr(), plan=b._plan):
            return lib.sdsp_hip_pfb_synth_process(plan, in_ptr, in_stride, out_ptr, out_stride, streams, frames, 0, state, None)

        assert call() == 0
        assert call(in_stride=4 * b.bins - 1) == L.ERR_INVALID_ARG
        assert call(out_stride=127) == L.ERR_INVALID_ARG
        assert call(in_ptr=None) == L.ERR_INVALID_ARG
        assert call(out_ptr=None) == L.ERR_INVALID_ARG
        assert call(plan=None) == L.ERR_INVALID_ARG
        assert call(out_ptr=X.data_ptr()) == L.ERR_INVALID_ARG  # overlap
        assert call(in_ptr=X.data_ptr() + 4) == L.ERR_INVALID_ARG  # misaligned
        assert call(out_ptr=out.data_ptr() + 1) == L.ERR_INVALID_ARG
        assert call(state=st.data_ptr() + 2) == L.ERR_INVALID_ARG
        assert call(state=None) == 0  # start from zero, drop the tail
        assert call(streams=0) == 0 and call(frames=0) == 0
        assert call(frames=3, streams=1, in_stride=0, out_stride=0) == 0  # one stream: the strides are not used
        n = C.c_uint64(0)
        assert lib.sdsp_hip_pfb_synth_plan_launches(b._plan, 2, 4, C.byref(n)) == 0 and n.value == 4  # seed, copy / pack, transform, unfold
        assert lib.sdsp_hip_pfb_synth_plan_set_unfold_form(b._plan, 2) == L.ERR_INVALID_ARG
        nb = C.c_uint64(0)
        assert lib.sdsp_hip_pfb_synth_state_bytes(b._plan, 2, C.byref(nb)) == 0 and nb.value == 2 * b.hist * (8 if cplx else 4)
        with pytest.raises(ValueError):
            b.process(X.to(torch.complex128))
        with pytest.raises(ValueError):
            b.process(X[:1])
        with pytest.raises(ValueError):
            b.process(X, frames=5)
        with pytest.raises(ValueError):
            b.process(X, out=torch.zeros((2, 100), dtype=odt, device="cuda"))
        assert b.process(X, frames=0).shape == (2, 0)
    torch.cuda.synchronize()
