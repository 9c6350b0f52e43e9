"""GPU tests of the polyphase filter-bank channelizer bank (sdsp_hip_pfb_*) on a real MI355X.

The checker is tests/pfb_ref.py (double), itself pinned to torch.stft(n_fft = L)[k P] and to the direct sum in tests/test_pfb_host.py.
Every case is also held bit for bit to the composition a user writes with the library alone: history + block -> unfold(L, D) x taps in
the plan precision -> the P polyphase branches added in ascending order -> (TIME: torch.roll per frame) -> RfftPlan.exec + unpack
(real input) or FftPlan(M, RADIX_AUTO).exec (complex input)."""
import ctypes as C

import numpy as np
import pytest

from pfb_ref import pfb_fold_ref, pfb_ref, pfb_shifts

pytestmark = pytest.mark.gpu

M_F32 = [16, 32, 256, 1024, 4096, 16384, 65536]
M_F64 = [16, 32, 256, 1024, 4096, 16384, 32768]
TAPS_PER_CHANNEL = [1, 3, 8]
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


def _tol(precision, n_taps):
    """the STFT bank's rule with N = L, the length of the transform the bank equals: f64 4 L eps; f32 2e-6"""
    return 4 * n_taps * EPS64 if precision == "f64" else 2e-6


def _err(got, want):
    """relative maximum error of one call"""
    return np.abs(got - want).max() / np.abs(want).max()


def _hops(m):
    return [m, m // 2, m // 4, 3 * m // 4] + ([1] if m <= 256 else [])


def _frames(m, p, hop):
    """past the history where that stays small, a few frames otherwise (the history is random, so every frame is a full test)"""
    need = p * m // hop + 3
    return need if m <= 1024 and hop > 1 else (m * p + 40 if hop == 1 and m <= 32 else 6 if hop > 1 else 300)


def _shapes(m, p, hop):
    """(streams, samples, in_stride): odd in_stride > samples; 130 streams where the frames stay few"""
    S = hop * _frames(m, p, hop)
    shapes = [(1, S, S), (3, S, S + 3)]
    if m <= 1024 and hop >= m // 4 and p <= 3:
        shapes.append((130, S, S + 1 + (S % 2 == 0)))
    return shapes


def _rand(rng, shape, precision, cplx):
    x = rng.standard_normal(shape)
    if cplx:
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(_np(precision, cplx))


def _fold_compose(torch, xs, hist_rows, m, p, hop, taps_t):
    """history + block -> unfold(L, D) x taps -> view (C, F, P, M) -> the sum over p in ascending order"""
    full = torch.cat([hist_rows.flip(-1), xs], dim=1)

    def fold(part):
        fr = part.unfold(-1, m * p, hop) * taps_t  # (C, F, L), each product rounded in the plan precision
        fr = fr.view(fr.shape[0], fr.shape[1], p, m)
        u = fr[:, :, 0]
        for q in range(1, p):
            u = u + fr[:, :, q]
        return u

    if full.is_complex():  # real and imaginary parts folded separately with the real tap
        return torch.complex(fold(full.real), fold(full.imag))
    return fold(full)


def _compose(torch, sd, xs, hist_rows, m, p, hop, taps, precision, phase, position, variant=0):
    cplx = xs.is_complex()
    rdt = torch.float64 if precision == "f64" else torch.float32
    u = _fold_compose(torch, xs, hist_rows, m, p, hop, torch.from_numpy(taps).to(rdt).cuda())
    Cn, F = u.shape[0], u.shape[1]
    if phase == "time":
        s = pfb_shifts(m, p, hop, F, position)
        u = torch.stack([torch.roll(u[:, j], int(s[j]), dims=-1) for j in range(F)], dim=1)
    v = u.contiguous()
    if cplx:
        plan = sd.FftPlan(m, 0, sd.forward_fft, _prec(sd, precision), max_batch=Cn * F)  # radix 0: SDSP_HIP_RADIX_AUTO
        if variant:
            plan.set_variant(variant)
        return plan.exec(v)
    plan = sd.RfftPlan(m, 2, sd.forward_fft, max_batch=Cn * F, precision=_prec(sd, precision))
    if variant:
        plan.set_variant(variant)
    z = plan.exec(v)  # (C, F, M/2) packed
    out = torch.empty((Cn, F, m // 2 + 1), dtype=z.dtype, device=z.device)
    out[..., 1:m // 2] = z[..., 1:]
    out[..., 0] = torch.complex(z[..., 0].real, torch.zeros_like(z[..., 0].real))
    out[..., m // 2] = torch.complex(z[..., 0].imag, torch.zeros_like(z[..., 0].imag))
    return out


def _ref_from_fold(u, m, p, hop, phase, position, cplx):
    if phase == "time":
        s = pfb_shifts(m, p, hop, u.shape[1], position)
        u = np.stack([np.roll(u[:, j], int(s[j]), axis=-1) for j in range(u.shape[1])], axis=1)
    return np.fft.fft(u, axis=-1) if cplx else np.fft.rfft(u, axis=-1)


def _bank(sd, m, p, hop, streams, precision, cplx, phase, taps, **kw):
    return sd.pfb_bank(m, p, hop, streams=streams, taps=taps, input="complex" if cplx else "real", phase=phase,
                       precision=_prec(sd, precision), **kw)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m_idx", range(7))
def test_against_reference_and_composition(torch_cuda, sd, precision, cplx, m_idx):
    torch = torch_cuda
    m = (M_F64 if precision == "f64" else M_F32)[m_idx]
    if m == 16 and not cplx:
        with pytest.raises(sd.SdspHipError):  # the real-input plans start at 32
            _bank(sd, 16, 1, 16, 1, precision, False, "time", np.ones(16))._ensure_plan()
        return
    for p in TAPS_PER_CHANNEL:
        for hop in _hops(m):
            for streams, S, stride in _shapes(m, p, hop):
                rng = np.random.default_rng(m * 7 + hop * 3 + streams + p)
                Lt, H = m * p, m * p - hop
                taps = rng.standard_normal(Lt)
                taps_p = taps.astype(_np(precision, False)).astype(np.float64)  # rounded once to the plan precision
                x = _rand(rng, (streams, stride), precision, cplx)
                hist = _rand(rng, (streams, max(H, 1)), precision, cplx)
                xd = torch.from_numpy(x).cuda()
                position = 5 * hop + 3 * m
                u_ref, want_state = pfb_fold_ref(x[:, :S], m, p, hop, taps_p, hist[:, :H])
                for phase in ("frame", "time"):
                    b = _bank(sd, m, p, hop, streams, precision, cplx, phase, taps)
                    b._state = torch.from_numpy(hist.copy()).cuda()
                    b.position = position
                    x_before = xd.clone()
                    y = b.process(xd, samples=S)
                    assert torch.equal(xd, x_before)  # in is never written
                    assert b.position == position + S
                    want = _ref_from_fold(u_ref, m, p, hop, phase, position, cplx)
                    got = y.cpu().numpy()
                    assert got.shape == want.shape
                    err = _err(got, want)
                    print(f"pfb {precision} {'complex' if cplx else 'real'} M={m} P={p} D={hop} streams={streams} {phase}: "
                          f"err {err:.3e} (bound {_tol(precision, Lt):.3e})")
                    assert err <= _tol(precision, Lt), (p, hop, streams, phase, err)
                    if H:
                        assert np.array_equal(b.state.cpu().numpy()[:, :H], want_state.astype(_np(precision, cplx)))
                    ref = _compose(torch, sd, xd[:, :S], torch.from_numpy(hist[:, :H]).cuda(), m, p, hop, taps, precision, phase,
                                   position)
                    assert torch.equal(y, ref), (p, hop, streams, phase)
                    if hop in (m, m // 2) and streams == 3:  # the plain form gives the sliding form's bits
                        b2 = _bank(sd, m, p, hop, streams, precision, cplx, phase, taps)
                        b2._state = torch.from_numpy(hist.copy()).cuda()
                        b2.position = position
                        b2._set_fold_form(1)
                        assert b2.info()["fold"] == "plain" and b.info()["fold"] == "sliding"
                        assert torch.equal(b2.process(xd, samples=S), y)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m,p,hop", [(32, 3, 8), (256, 8, 128), (256, 3, 192), (1024, 8, 1024), (64, 2, 1)])
def test_blockwise_equals_one_call(torch_cuda, sd, precision, cplx, m, p, hop):
    torch = torch_cuda
    rng = np.random.default_rng(m + hop + p)
    Lt = m * p
    blocks = [hop, 3 * hop, 0, 7 * hop, hop, 2 * (Lt // hop) * hop + hop, 2 * hop]  # shorter and longer than hist, an empty one
    S = sum(blocks)
    streams = 5
    x = _rand(rng, (streams, S), precision, cplx)
    xd = torch.from_numpy(x).cuda()
    for phase in ("frame", "time"):
        one = _bank(sd, m, p, hop, streams, precision, cplx, phase, "hamming")
        want = one.process(xd)
        b = _bank(sd, m, p, hop, streams, precision, cplx, phase, "hamming")
        outs, pos = [], 0
        for n in blocks:
            outs.append(b.process(xd[:, pos:pos + n].contiguous()))
            pos += n
            assert b.position == pos
        assert torch.equal(torch.cat(outs, dim=1), want)
        assert torch.equal(b.state, one.state)
        ref, ref_state = pfb_ref(x, m, p, hop, one.taps.astype(_np(precision, False)).astype(np.float64), None, phase, 0)
        assert _err(want.cpu().numpy(), ref) <= _tol(precision, Lt)
        assert np.array_equal(one.state.cpu().numpy()[:, :Lt - hop], ref_state.astype(_np(precision, cplx)))
        b.reset()
        assert b.position == 0 and b.state is None
        assert torch.equal(b.process(xd), want)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("hop", [256, 128, 192])
def test_small_workspaces_equal_the_default(torch_cuda, sd, precision, cplx, hop):
    torch = torch_cuda
    m, p, streams, F = 256, 3, 5, 9
    rng = np.random.default_rng(hop)
    xd = torch.from_numpy(_rand(rng, (streams, F * hop), precision, cplx)).cuda()
    want = _bank(sd, m, p, hop, streams, precision, cplx, "time", "hann").process(xd)
    unit = m * np.dtype(_np(precision, cplx)).itemsize
    for frames in range(1, 8):  # slices that start and end inside a stream
        b = _bank(sd, m, p, hop, streams, precision, cplx, "time", "hann", workspace_bytes=frames * unit)
        assert b.info()["workspace_bytes"] == frames * unit
        assert b.launches(F * hop) >= -(-streams * F // frames) * 2
        assert torch.equal(b.process(xd), want), frames


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m,p,hop", [(64, 4, 64), (64, 4, 16), (64, 3, 48)])
def test_preload_and_nan_reach_exactly_the_frames_that_cover_them(torch_cuda, sd, precision, cplx, m, p, hop):
    torch = torch_cuda
    Lt, H, F, streams = m * p, m * p - hop, 24, 2
    x = np.full((streams, F * hop), 0.5, dtype=_np(precision, cplx))
    at = 5 * hop + 3  # index in the block
    x[1, at] = np.nan
    b = _bank(sd, m, p, hop, streams, precision, cplx, "frame", "hamming")
    b.preload_filter(0.5)
    y = b.process(torch.from_numpy(x).cuda()).cpu().numpy()
    # a steady input of 0.5: every frame is the transform of 0.5 * (the taps folded), the same for all frames
    assert np.array_equal(y[0], np.broadcast_to(y[0, 0], y[0].shape))
    pos = H + at  # index in history + block; frame j covers [j hop, j hop + L)
    covered = np.array([j * hop <= pos < j * hop + Lt for j in range(F)])
    has_nan = np.isnan(y[1]).any(axis=-1)
    assert np.array_equal(has_nan, covered) and covered.any() and not covered.all()
    assert not np.isnan(y[0]).any()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("phase", ["frame", "time"])
def test_sentinels_padded_rows_graph_and_host_entry(torch_cuda, sd, precision, cplx, phase):
    torch = torch_cuda
    m, p, hop, streams, F = 256, 3, 64, 3, 11
    S = F * hop
    rng = np.random.default_rng(11)
    x = _rand(rng, (streams, S + 5), precision, cplx)
    xd = torch.from_numpy(x).cuda()
    b = _bank(sd, m, p, hop, streams, precision, cplx, phase, "blackman")
    want = b.process(xd, samples=S)
    state_after = b.state.clone()
    # out with spare frames per row (out_stride > F bins): the spare part keeps its sentinel
    b.reset()
    out = torch.full((streams, F + 2, b.bins), 7.0 + 3.0j, dtype=want.dtype, device="cuda")
    got = b.process(xd, samples=S, out=out)
    assert torch.equal(got, want) and torch.equal(b.state, state_after)
    assert torch.equal(out[:, F:], torch.full_like(out[:, F:], 7.0 + 3.0j))
    # out rows at an odd stride through the C entry, input sentinel columns untouched
    lib = sd.load()
    b.reset()
    b._ensure_plan()
    stride = F * b.bins + 3
    flat = torch.full((streams * stride,), 1.0 - 2.0j, dtype=want.dtype, device="cuda")
    st = torch.zeros((streams, b.hist), dtype=xd.dtype, device="cuda")
    x_before = xd.clone()
    sd.pfb.L.check(lib.sdsp_hip_pfb_process(b._plan, xd.data_ptr(), S + 5, flat.data_ptr(), stride, streams, S, 0, st.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
    rows = flat.view(streams, stride)
    assert torch.equal(rows[:, :F * b.bins].reshape(streams, F, b.bins), want)
    assert torch.equal(rows[:, F * b.bins:], torch.full_like(rows[:, F * b.bins:], 1.0 - 2.0j))
    assert torch.equal(xd, x_before) and torch.equal(st, state_after)
    # a captured graph replays the eager call bit for bit
    g_state = torch.zeros((streams, b.hist), dtype=xd.dtype, device="cuda")
    g_out = torch.zeros_like(want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            sd.pfb.L.check(lib.sdsp_hip_pfb_process(b._plan, xd.data_ptr(), S + 5, g_out.data_ptr(), F * b.bins, streams, S, 0,
                                                    g_state.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    g_state.zero_()
    g_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, want) and torch.equal(g_state, state_after)
    # the host entry equals the device entry
    h_out = np.zeros((streams, F, b.bins), dtype=_np(precision, True))
    h_state = np.zeros((streams, b.hist), dtype=_np(precision, cplx))
    xh = np.ascontiguousarray(x)
    sd.pfb.L.check(lib.sdsp_hip_pfb_process_host(b._plan, xh.ctypes.data, S + 5, h_out.ctypes.data, F * b.bins, streams, S, 0,
                                                 h_state.ctypes.data))
    assert np.array_equal(h_out, want.cpu().numpy()) and np.array_equal(h_state, state_after.cpu().numpy())


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_inner_variant_one_agrees_within_the_tolerance(torch_cuda, sd, precision, cplx):
    """the inner transform's alternate kernel where the size has one: within the tolerance of the reference, and bit for bit the
    composition with that variant"""
    torch = torch_cuda
    agreed = 0
    for m in (M_F64 if precision == "f64" else M_F32)[0 if cplx else 1:]:
        p, hop, streams = 3, m // 2, 3
        rng = np.random.default_rng(m)
        x = _rand(rng, (streams, 12 * hop), precision, cplx)
        xd = torch.from_numpy(x).cuda()
        b = _bank(sd, m, p, hop, streams, precision, cplx, "time", "hamming")
        try:
            b.set_variant(1)
        except sd.SdspHipError as e:
            assert e.code == sd._lib.ERR_UNSUPPORTED
            continue
        y = b.process(xd)
        want, _ = pfb_ref(x, m, p, hop, b.taps.astype(_np(precision, False)).astype(np.float64), None, "time", 0)
        assert _err(y.cpu().numpy(), want) <= _tol(precision, m * p), m
        ref = _compose(torch, sd, xd, torch.zeros((streams, m * p - hop), dtype=xd.dtype, device="cuda"), m, p, hop, b.taps, precision,
                       "time", 0, variant=1)
        assert torch.equal(y, ref), m
        assert b.info()["kernel"]
        agreed += 1
    assert agreed > 0
    with pytest.raises(ValueError):
        b.set_variant(-1)


def test_process_errors(torch_cuda, sd):
    torch = torch_cuda
    lib = sd.load()
    L = sd.pfb.L
    for cplx in (False, True):
        b = _bank(sd, 64, 4, 32, 2, "f32", cplx, "time", "hamming")
        b._ensure_plan()
        dt = torch.complex64 if cplx else torch.float32
        x = torch.zeros((2, 128), dtype=dt, device="cuda")
        out = torch.zeros((2, 4, b.bins), dtype=torch.complex64, device="cuda")
        st = torch.zeros((2, b.hist), dtype=dt, device="cuda")

        def call(in_ptr=x.data_ptr(), in_stride=128, out_ptr=out.data_ptr(), out_stride=4 * b.bins, streams=2, samples=128,
                 state=st.data_ptr(), plan=b._plan):
            return lib.sdsp_hip_pfb_process(plan, in_ptr, in_stride, out_ptr, out_stride, streams, samples, 0, state, None)

        assert call() == 0
        assert call(samples=100) == L.ERR_INVALID_SIZE  # S % D != 0
        assert call(in_stride=127) == L.ERR_INVALID_ARG
        assert call(out_stride=4 * b.bins - 1) == L.ERR_INVALID_ARG
        assert call(in_ptr=None) == L.ERR_INVALID_ARG
        assert call(out_ptr=None) == L.ERR_INVALID_ARG
        assert call(plan=None) == L.ERR_INVALID_ARG
        assert call(out_ptr=x.data_ptr()) == L.ERR_INVALID_ARG  # overlap
        assert call(in_ptr=x.data_ptr() + 1) == L.ERR_INVALID_ARG  # misaligned
        assert call(state=None) == 0  # zero history, final history dropped
        assert call(streams=0) == 0 and call(samples=0) == 0
        n = C.c_uint64(0)
        assert lib.sdsp_hip_pfb_plan_launches(b._plan, 2, 100, C.byref(n)) == L.ERR_INVALID_SIZE
        assert lib.sdsp_hip_pfb_plan_launches(b._plan, 2, 128, C.byref(n)) == 0 and n.value == (3 if cplx else 4)
        assert lib.sdsp_hip_pfb_plan_set_fold_form(b._plan, 2) == L.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            b.process(x.to(torch.complex128 if cplx else torch.float64))
        with pytest.raises(ValueError):
            b.process(x[:1])
        with pytest.raises(sd.SdspHipError):
            b.process(x, samples=100)
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_tone_at_a_sub_band_centre_is_a_constant_phasor(torch_cuda, sd, precision):
    """what makes it a channelizer and not only an STFT: a complex exponential at the centre of sub-band k0, TIME phase, D = M / 2.
    Once the history has filled, sub-band k0 carries H(f0) -- the same phasor in every frame; every sub-band other than k0 +- 1
    lies below the prototype's stop-band level."""
    torch = torch_cuda
    m, p, k0 = 256, 8, 37
    hop, Lt = m // 2, m * p
    h = sd.pfb_prototype("hamming", m, p)
    hp = h.astype(_np(precision, False)).astype(np.float64)
    F = 2 * Lt // hop + 40
    n = np.arange(F * hop)
    x = np.exp(2j * np.pi * ((k0 * n) % m) / m).astype(_np(precision, True))
    b = _bank(sd, m, p, hop, 1, precision, True, "time", h)
    y = b.process(torch.from_numpy(x[None, :]).cuda()).cpu().numpy()[0].astype(np.complex128)
    full = y[Lt // hop:]  # frames whose taps all lie in the block
    # pass-band gain at the tone: |sum h[n]| (the tone sits at the sub-band centre, where the phases cancel exactly)
    gain = abs(hp.sum())
    tol = _tol(precision, Lt)
    z = full[:, k0]
    # the allowed step: the tolerance on the spectrum (relative to its largest bin, which is bin k0 here) over the gain at the tone
    step = np.abs(np.angle(z[1:] / z[:-1])).max()
    print(f"tone {precision}: |z| {np.abs(z).mean():.6f} gain {gain:.6f} phase step {step:.3e} bound {tol / gain:.3e}")
    assert step <= tol / gain
    assert np.abs(np.abs(z) - gain).max() <= tol * gain
    # stop band: the prototype's response at every multiple of the sub-band spacing from 2 spacings on, from h itself
    Hf = np.abs(np.fft.fft(hp, 64 * Lt))
    spacing = 64 * Lt // m
    stop = Hf[2 * spacing - spacing // 2: 64 * Lt - 2 * spacing + spacing // 2 + 1].max()  # |f| >= 1.5 spacings from the centre
    others = np.delete(np.abs(full), [k0 - 1, k0, k0 + 1], axis=1)
    print(f"tone {precision}: largest other sub-band {others.max():.3e}, stop-band level {stop:.3e}")
    assert others.max() <= stop
    # the FRAME phase of the same bank is the STFT: there the phasor turns by 2 pi k0 D / M = pi per frame for odd k0
    bf = _bank(sd, m, p, hop, 1, precision, True, "frame", h)
    zf = bf.process(torch.from_numpy(x[None, :]).cuda()).cpu().numpy()[0][Lt // hop:, k0]
    assert np.abs(np.abs(np.angle(zf[1:] / zf[:-1])) - np.pi).max() < 1e-3
