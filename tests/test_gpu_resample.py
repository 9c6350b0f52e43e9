"""GPU tests of the polyphase FIR resampler bank (sdsp_hip_resample_*) on a real MI355X.

The checker is tests/resample_ref.py (double, the contract's summation order), itself pinned to scipy.signal.upfirdn in
tests/test_resample_host.py.  f64 is held to bit-exact agreement with it; f32 to bit-exact agreement with the zero-stuff ->
fir_filter -> every D-th sample composition on the GPU, and to 1e-6 normwise of the double reference."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_max_err
from resample_ref import GRID_T, GRID_UD, hist_of, phase_tap_sums, q_of, resample_ref

pytestmark = pytest.mark.gpu


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


def _np(precision):
    return np.float64 if precision == "f64" else np.float32


def _bank(sd, h, up, down, channels, precision, variant=0, state=None):
    import torch
    r = sd.fir_resampler(h.size, up, down, channels, sd.F64 if precision == "f64" else sd.F32)
    r.set_coeff(h)
    r.set_variant(variant)
    if state is not None:
        r._state = torch.from_numpy(np.ascontiguousarray(state.astype(_np(precision)))).cuda()
    return r


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _matches(got, ref, precision):
    """the bank against tests/resample_ref.py fed the taps of the precision: f64 bit for bit, f32 to 1e-6 normwise (the reference sums
    in double)"""
    if precision == "f64":
        return np.array_equal(got, ref)
    return got.shape == ref.shape and (ref.size == 0 or rel_max_err(got, ref) <= 1e-6 or np.abs(ref).max() == 0)


def _samples(up, down, at_least):
    q = q_of(up, down)
    return q * max(1, -(-at_least // q))


def _shapes(up, down, taps):
    """(channels, samples, in_stride): odd strides, in_stride > samples, 1 .. 130 channels"""
    s1 = _samples(up, down, 2 * taps + 5)
    s2 = _samples(up, down, 64)
    return [(1, s1, s1), (3, s2, s2 + 3), (130, s2, s2 + 1 + (s2 % 2 == 0))]


@pytest.mark.parametrize("up,down", GRID_UD)
@pytest.mark.parametrize("taps", GRID_T)
def test_f64_bit_exact_against_reference_all_variants(sd, torch_cuda, up, down, taps):
    rng = np.random.default_rng(taps * 7919 + up * 131 + down)
    h = rng.standard_normal(taps)
    H = hist_of(taps, up)
    for channels, samples, in_stride in _shapes(up, down, taps):
        xs = rng.standard_normal((channels, in_stride))
        hist = rng.standard_normal((channels, max(H, 1)))
        want, want_state = resample_ref(h, xs[:, :samples], up, down, hist[:, :H])
        M = want.shape[1]
        outs = []
        for variant in (0, 1, 2):
            r = _bank(sd, h, up, down, channels, "f64", variant, hist)
            out = r.process(_dev(torch_cuda, xs), samples=samples)
            torch_cuda.cuda.synchronize()
            got = out.cpu().numpy()
            assert got.shape == (channels, M)
            assert _matches(got, want, "f64"), (variant, channels, samples)
            if H:
                assert np.array_equal(r.state.cpu().numpy(), want_state), variant
            outs.append(got)


@pytest.mark.parametrize("up,down", GRID_UD)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_equals_zero_stuff_fir_filter_slice_on_gpu(sd, torch_cuda, up, down, precision):
    rng = np.random.default_rng(up * 1000 + down)
    npdt = _np(precision)
    prec = sd.F64 if precision == "f64" else sd.F32
    for taps in (1, 17, 64, 255):
        h = rng.standard_normal(taps)
        channels, S = 5, _samples(up, down, 400)
        x = rng.standard_normal((channels, S)).astype(npdt)
        r = _bank(sd, h, up, down, channels, precision)
        got = r.process(_dev(torch_cuda, x)).cpu().numpy()
        r2 = _bank(sd, h, up, down, channels, precision, 2)
        assert np.array_equal(r2.process(_dev(torch_cuda, x)).cpu().numpy(), got)
        z = np.zeros((channels, S * up), dtype=npdt)
        z[:, ::up] = x
        f = sd.fir_filter(taps, channels, prec)
        f.set_coeff(h)
        zd = _dev(torch_cuda, z)
        f.process(zd)
        torch_cuda.cuda.synchronize()
        want = zd.cpu().numpy()[:, ::down]
        assert np.array_equal(got, want), (taps, precision)
        if precision == "f32":
            ref, _ = resample_ref(h.astype(np.float32), x, up, down)
            assert _matches(got, ref, "f32")


def test_unit_ratio_equals_fir_filter_output_and_state(sd, torch_cuda):
    rng = np.random.default_rng(11)
    for precision, prec in (("f32", sd.F32), ("f64", sd.F64)):
        for taps in (1, 2, 33, 64, 300):
            x = rng.standard_normal((7, 1000)).astype(_np(precision))
            h = rng.standard_normal(taps)
            r = _bank(sd, h, 1, 1, 7, precision)
            f = sd.fir_filter(taps, 7, prec)
            f.set_coeff(h)
            got = r.process(_dev(torch_cuda, x)).cpu().numpy()
            d = _dev(torch_cuda, x)
            f.process(d)
            torch_cuda.cuda.synchronize()
            assert np.array_equal(got, d.cpu().numpy()), (precision, taps)
            if taps > 1:
                assert np.array_equal(r.state.cpu().numpy(), f.state.cpu().numpy())


@pytest.mark.parametrize("up,down", GRID_UD)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_streaming_equals_one_call(sd, torch_cuda, up, down, precision):
    rng = np.random.default_rng(3 * up + 5 * down)
    q = q_of(up, down)
    npdt = _np(precision)
    for taps in (17, 255, 1024):
        H = hist_of(taps, up)
        blocks = [0] + [q * int(v) for v in rng.integers(0, max(2, 2 * H // q + 3), size=6)] + [q * max(1, (H // 3) // q), 0]
        S = sum(blocks)
        x = rng.standard_normal((4, S)).astype(npdt)
        h = rng.standard_normal(taps)
        one = _bank(sd, h, up, down, 4, precision)
        want = one.process(_dev(torch_cuda, x)).cpu().numpy()
        for variant in (0, 2):
            r = _bank(sd, h, up, down, 4, precision, variant)
            parts, s0 = [], 0
            for b in blocks:
                parts.append(r.process(_dev(torch_cuda, x[:, s0:s0 + b].copy())).cpu().numpy())
                s0 += b
            assert np.array_equal(np.concatenate(parts, axis=1), want), variant
            if H:
                ext = np.concatenate([np.zeros((4, H), dtype=npdt), x], axis=1)
                assert np.array_equal(r.state.cpu().numpy(), ext[:, ::-1][:, :H]), variant


def test_state_none_preload_and_untouched_buffers(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(2)
    for up, down, taps in [(1, 4, 64), (3, 2, 65), (160, 147, 300), (1, 3, 17)]:
        S = _samples(up, down, 600)
        h = rng.standard_normal(taps)
        x = rng.standard_normal((3, S))
        r = _bank(sd, h, up, down, 3, "f64")
        r._ensure_plan()
        xd = _dev(torch_cuda, x)
        M = S * up // down
        out = torch_cuda.full((3, M + 9), float("nan"), dtype=torch_cuda.float64, device="cuda")
        assert lib.sdsp_hip_resample_process(r._plan, xd.data_ptr(), S, out.data_ptr(), M + 9, 3, S, None, None) == 0
        torch_cuda.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :M], resample_ref(h, x, up, down)[0])
        assert np.all(np.isnan(got[:, M:]))  # the tail of every row is not touched
        assert np.array_equal(xd.cpu().numpy(), x)  # in is never written
        # preload: a constant input v gives v times the tap sum of each output's phase
        v = 0.75
        r.preload_filter(v)
        y = r.process(_dev(torch_cuda, np.full((3, S), v))).cpu().numpy()
        want = resample_ref(h, np.full(S, v), up, down, np.full(hist_of(taps, up), v))[0]
        assert np.array_equal(y[1], want)
        assert np.allclose(y[2], v * phase_tap_sums(h, up, down, np.arange(M)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("up,down,taps", [(1, 4, 64), (1, 3, 17), (3, 2, 65), (4, 1, 30), (160, 147, 300)])
def test_nan_reaches_exactly_its_outputs(sd, torch_cuda, up, down, taps):
    rng = np.random.default_rng(taps)
    S = _samples(up, down, 900)
    h = rng.uniform(0.5, 1.5, taps)  # no zero taps
    x = rng.standard_normal((2, S))
    pos = S // 2 + 1
    x[1, pos] = np.nan
    for variant in (0, 1, 2):
        r = _bank(sd, h, up, down, 2, "f32", variant)
        got = r.process(_dev(torch_cuda, x.astype(np.float32))).cpu().numpy()
        m = np.arange(S * up // down)
        n = m * down
        k = n - pos * up  # the tap that reads x[pos] ((n - k) / up = pos; k = n mod up by construction)
        hit = (k >= 0) & (k < taps)
        assert np.array_equal(np.isnan(got[1]), hit), variant
        assert not np.isnan(got[0]).any()


def test_error_codes(sd, torch_cuda):
    lib = sd.load()
    r = _bank(sd, np.ones(16), 3, 2, 2, "f32")
    r._ensure_plan()
    p = r._plan
    x = torch_cuda.zeros((2, 64), device="cuda")
    y = torch_cuda.zeros((2, 96), device="cuda")
    ok = lambda *a: lib.sdsp_hip_resample_process(p, *a, None)  # noqa: E731
    assert ok(x.data_ptr(), 64, y.data_ptr(), 96, 2, 64, None) == 0
    assert ok(x.data_ptr(), 64, y.data_ptr(), 96, 2, 63, None) == -1  # q = 2
    assert ok(None, 64, y.data_ptr(), 96, 2, 64, None) == -5
    assert ok(x.data_ptr(), 64, None, 96, 2, 64, None) == -5
    assert ok(x.data_ptr(), 62, y.data_ptr(), 96, 2, 64, None) == -5  # in_stride < samples
    assert ok(x.data_ptr(), 64, y.data_ptr(), 95, 2, 64, None) == -5  # out_stride < outputs
    assert ok(x.data_ptr(), 64, x.data_ptr() + 4 * 10, 96, 1, 64, None) == -5  # overlap; both ranges lie inside x
    assert ok(y.data_ptr() + 4 * 10, 64, y.data_ptr(), 96, 1, 64, None) == -5
    assert ok(x.data_ptr(), 64, y.data_ptr(), 96, 0, 64, None) == 0
    assert lib.sdsp_hip_resample_process(None, x.data_ptr(), 64, y.data_ptr(), 96, 2, 64, None, None) == -5
    assert lib.sdsp_hip_resample_plan_set_variant(p, 3) == -5
    h = np.ones(8)
    q = C.c_void_p()
    assert lib.sdsp_hip_resample_plan_create(C.byref(q), 4097, np.ones(4097).ctypes.data, 1, 2, sd.F32, 0) == -1
    assert lib.sdsp_hip_resample_plan_create(C.byref(q), 8, h.ctypes.data, 0, 2, sd.F32, 0) == -1
    assert lib.sdsp_hip_resample_plan_create(C.byref(q), 8, h.ctypes.data, 1, 1025, sd.F32, 0) == -1
    assert lib.sdsp_hip_resample_plan_create(C.byref(q), 8, h.ctypes.data, 1, 2, 2, 0) == -5  # F32_F64STATE is IIR only
    assert lib.sdsp_hip_resample_plan_create(None, 8, h.ctypes.data, 1, 2, sd.F32, 0) == -5
    with pytest.raises(sd.SdspHipError):
        r.process(torch_cuda.zeros((2, 63), device="cuda"))


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(9)
    h = rng.standard_normal(64)
    x = rng.standard_normal((33, 4032)).astype(np.float32)
    eager = _bank(sd, h, 1, 4, 33, "f32")
    want = eager.process(_dev(torch, x)).cpu().numpy()
    r = _bank(sd, h, 1, 4, 33, "f32")
    xd = _dev(torch, x)
    out = torch.empty((33, 1008), device="cuda")
    r.process(xd, out=out)  # plan + state exist before capture
    r.reset()
    r._state = torch.zeros((33, 63), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.process(xd, out=out)
    r._state.zero_()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(4)
    for up, down in [(1, 4), (3, 2)]:
        h = rng.standard_normal(65)
        S = _samples(up, down, 500)
        M = S * up // down
        x = rng.standard_normal((6, S))
        hist = rng.standard_normal((6, hist_of(65, up)))
        r = _bank(sd, h, up, down, 6, "f64", state=hist)
        dev = r.process(_dev(torch_cuda, x)).cpu().numpy()
        r._ensure_plan()
        out = np.zeros((6, M))
        st = hist.copy()
        assert lib.sdsp_hip_resample_process_host(r._plan, x.ctypes.data, S, out.ctypes.data, M, 6, S, st.ctypes.data) == 0
        assert np.array_equal(out, dev)
        assert np.array_equal(st, r.state.cpu().numpy())


def test_full_size_64bit_indexing(sd, torch_cuda):
    torch = torch_cuda
    channels, S, taps = 1 << 20, 4096, 64
    h = np.random.default_rng(1).standard_normal(taps) / 8
    r = _bank(sd, h, 1, 4, channels, "f32")
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((channels, S), device="cuda", generator=gen)
    out = r.process(x)
    torch.cuda.synchronize()
    for c in (0, channels // 2, channels - 1):
        xc = x[c].cpu().numpy()
        want = resample_ref(h.astype(np.float32), xc, 1, 4)[0]
        assert rel_max_err(out[c].cpu().numpy(), want) <= 1e-6, c
    del x, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("up,down,taps", [(160, 147, 64), (147, 160, 300), (2, 1, 64), (1, 3, 255), (5, 7, 1024)])
def test_long_rows_cross_several_blocks(sd, torch_cuda, up, down, taps):
    """rows several generic-kernel blocks long (blocks hold up to 256 periods), f64 against the reference in every variant"""
    rng = np.random.default_rng(up + down + taps)
    S = q_of(up, down) * 700
    h = rng.standard_normal(taps)
    x = rng.standard_normal((3, S))
    hist = rng.standard_normal((3, max(hist_of(taps, up), 1)))
    want, want_state = resample_ref(h, x, up, down, hist[:, :hist_of(taps, up)])
    for variant in (0, 1, 2):
        r = _bank(sd, h, up, down, 3, "f64", variant, hist)
        assert np.array_equal(r.process(_dev(torch_cuda, x)).cpu().numpy(), want), variant
        if hist_of(taps, up):
            assert np.array_equal(r.state.cpu().numpy(), want_state), variant
