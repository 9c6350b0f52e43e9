"""GPU tests of the digital down-converter bank (sdsp_hip_ddc_*) on a real MI355X.

The checker is tests/ddc_ref.py, the contract's operation order in numpy, itself pinned to mix -> scipy.signal.upfirdn in
tests/test_ddc_host.py.  Both precisions, both input kinds and both kernel variants are held to bit-exact agreement with it."""
import ctypes as C

import numpy as np
import pytest

import arena
from ddc_ref import BLOCKS, GRID_D, GRID_T, ddc_ref, real_dtype

pytestmark = pytest.mark.gpu

F1, F2, F3 = 0x12345678, (1 << 32) - 0x01000001, 1 << 31
BANDS = [(0, F1, 0x0badcafe), (2, F2, 7), (0, F3, 1 << 30), (2, F2, 7), (0, 0, 0)]  # channel 1 has no band; bands 1 and 3 are one band twice


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


def _in_dtype(precision, cplx):
    if cplx:
        return np.complex128 if precision == "f64" else np.complex64
    return real_dtype(precision)


def _rand(rng, shape, precision, cplx):
    x = rng.standard_normal(shape)
    if cplx:
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(_in_dtype(precision, cplx))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bank(sd, h, down, bands, channels, precision, cplx, variant=0, state=None, position=0):
    import torch
    b = sd.ddc_bank(len(h), down, bands, channels, "complex" if cplx else "real", sd.F64 if precision == "f64" else sd.F32)
    b.set_coeff(h)
    b.set_variant(variant)
    b.position = position
    if state is not None:
        b._state = torch.from_numpy(np.ascontiguousarray(state.astype(_in_dtype(precision, cplx)))).cuda()
    return b


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("down", GRID_D)
@pytest.mark.parametrize("taps", GRID_T)
def test_bit_exact_against_reference(sd, torch_cuda, taps, down):
    """every precision, kind and variant; rows of two LDS blocks and a ragged tail (the block size is the plan's), and one S < H"""
    rng = np.random.default_rng(taps * 7919 + down)
    h = rng.standard_normal(taps)
    H = taps - 1
    for precision in ("f32", "f64"):
        for cplx in (False, True):
            block = _bank(sd, h, down, BANDS, 3, precision, cplx).info()["block_out"]
            for S in ((2 * block + 37) * down, down * max(1, (H // 2) // down)):
                x = _rand(rng, (3, S + 4 + (-S) % 4), precision, cplx)  # rows on 16-byte boundaries (odd strides: the framed test)
                hist = _rand(rng, (3, max(H, 1)), precision, cplx)
                position = int(rng.integers(0, 1 << 34)) * down
                want, want_state = ddc_ref(h, x[:, :S], down, BANDS, position, hist[:, :H], precision)
                for variant in (0, 1):
                    b = _bank(sd, h, down, BANDS, 3, precision, cplx, variant, hist, position)
                    out = torch_cuda.empty((len(BANDS), S // down + 2 + (S // down) % 2), dtype=b._out_dtype(), device="cuda")
                    got = b.process(_dev(torch_cuda, x), out=out, samples=S).cpu().numpy()
                    tag = (precision, cplx, variant, S)
                    assert got.shape == want.shape, tag
                    assert np.array_equal(got, want), (tag, int((got != want).sum()))
                    assert _same(got[1], got[3]), tag  # the duplicated band
                    if H:
                        assert np.array_equal(b.state.cpu().numpy(), want_state), tag
                    assert b.position == position + S


@pytest.mark.parametrize("cplx,down", [(True, 1), (True, 1024), (False, 1024)])
def test_longest_filter_runs_blocks_of_one_or_two_outputs(sd, torch_cuda, cplx, down):
    """T = 4096 in f64: the history alone fills the LDS target, so a workgroup of the fused kernel makes one output per band (complex
    input) or two (real input, D = 1024) from a line of more than 64 KiB; seven outputs are several such blocks with odd first outputs"""
    rng = np.random.default_rng(4096 + down)
    taps, S = 4096, 7 * down
    h = rng.standard_normal(taps)
    x = _rand(rng, (3, S), "f64", cplx)
    hist = _rand(rng, (3, taps - 1), "f64", cplx)
    position = (2 ** 32 - 3) * down
    want, want_state = ddc_ref(h, x, down, BANDS, position, hist, "f64")
    for variant in (0, 1):
        b = _bank(sd, h, down, BANDS, 3, "f64", cplx, variant, hist, position)
        assert b.info()["block_out"] == (1 if cplx else 2)
        got = b.process(_dev(torch_cuda, x)).cpu().numpy()
        assert np.array_equal(got, want), variant
        assert np.array_equal(b.state.cpu().numpy(), want_state), variant


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_zero_frequency_is_the_decimating_resampler(sd, torch_cuda, precision):
    rng = np.random.default_rng(21)
    prec = sd.F64 if precision == "f64" else sd.F32
    for taps, down in [(64, 4), (17, 3), (255, 16), (33, 1), (1, 1)]:
        h = rng.standard_normal(taps)
        x = _rand(rng, (4, 40 * 16 * 3), precision, False)
        b = _bank(sd, h, down, [(c, 0, 0) for c in range(4)], 4, precision, False)
        y = b.process(_dev(torch_cuda, x)).cpu().numpy()
        if down == 1:
            f = sd.fir_filter(taps, 4, prec)
            f.set_coeff(h)
            d = _dev(torch_cuda, x)
            f.process(d)
            want, ref_state = d.cpu().numpy(), f.state
        else:
            r = sd.fir_resampler(taps, 1, down, 4, prec)
            r.set_coeff(h)
            want, ref_state = r.process(_dev(torch_cuda, x)).cpu().numpy(), r.state
        assert np.all(y.real == want), (taps, down)
        assert np.all(y.imag == 0), (taps, down)
        if taps > 1:
            assert np.array_equal(b.state.cpu().numpy(), ref_state.cpu().numpy())


def test_half_rate_band_is_the_sign_alternated_stream(sd, torch_cuda):
    """fcw = 2^31: g[k] = ((-1)^k h[k], +-0) and w = C[32768 (n mod 2)] (x) F[0] = ((-1)^n, +-0) exactly, and sign changes are exact in
    every product and sum, so the real part equals the fcw = 0 run on x (-1)^n and the imaginary part is 0 (== in both: the sign of a
    zero is not part of the claim); position even, so that n and the call's sample index have the same parity"""
    rng = np.random.default_rng(22)
    for precision in ("f32", "f64"):
        for taps, down in [(64, 4), (17, 3), (255, 1)]:
            S = 600 * down
            h = rng.standard_normal(taps)
            x = _rand(rng, (1, S), precision, False)
            sign = np.where(np.arange(S) % 2 == 0, 1, -1).astype(x.dtype)
            a = _bank(sd, h, down, [(0, 1 << 31, 0)], 1, precision, False, position=2 * down).process(_dev(torch_cuda, x)).cpu().numpy()
            b = _bank(sd, h, down, [(0, 0, 0)], 1, precision, False, position=2 * down).process(_dev(torch_cuda, x * sign)).cpu().numpy()
            assert np.all(a.real == b.real) and np.all(a.imag == 0) and np.all(b.imag == 0), (precision, taps, down)
            assert np.array_equal(a, ddc_ref(h, x, down, [(0, 1 << 31, 0)], 2 * down, None, precision)[0])


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_streaming_equals_one_call(sd, torch_cuda, precision, cplx):
    rng = np.random.default_rng(23)
    for taps, down in [(17, 4), (255, 3), (64, 50), (33, 1)]:
        H = taps - 1
        blocks = [v * down for v in BLOCKS]
        S = sum(blocks)
        h = rng.standard_normal(taps)
        x = _rand(rng, (3, S), precision, cplx)
        hist = _rand(rng, (3, H), precision, cplx)
        pos0 = (2 ** 32 - 5 * down)  # the phase index wraps inside the stream
        for start in (hist, None):  # a random history; and a fresh stream, state = NULL, which is zero history
            one = _bank(sd, h, down, BANDS, 3, precision, cplx, 0, start, pos0)
            want = one.process(_dev(torch_cuda, x)).cpu().numpy()
            b = _bank(sd, h, down, BANDS, 3, precision, cplx, 0, start, pos0)
            parts = [b.process(_dev(torch_cuda, x[:, s0:s0 + n].copy())).cpu().numpy()
                     for s0, n in zip(np.cumsum([0] + blocks[:-1]), blocks)]
            assert _same(np.concatenate(parts, axis=1), want), (taps, down)
            assert _same(b.state.cpu().numpy(), one.state.cpu().numpy())
            assert b.position == pos0 + S
        # state = NULL through the C entry: zero history, nothing carried
        lib = sd.load()
        one._ensure_plan()
        xd = _dev(torch_cuda, x)
        out = torch_cuda.zeros((len(BANDS), S // down), dtype=one._out_dtype(), device="cuda")
        assert lib.sdsp_hip_ddc_process(one._plan, xd.data_ptr(), S, out.data_ptr(), S // down, S, pos0, None, None) == 0
        assert _same(out.cpu().numpy(), want)


def test_phase_wrap_and_large_positions(sd, torch_cuda):
    rng = np.random.default_rng(24)
    taps, down = 17, 4
    h = rng.standard_normal(taps)
    x = _rand(rng, (3, 64 * down), "f32", False)
    for position in (2 ** 32 - 3 * down, 2 ** 40 + 5 * down):
        got = _bank(sd, h, down, BANDS, 3, "f32", False, position=position).process(_dev(torch_cuda, x)).cpu().numpy()
        low = _bank(sd, h, down, BANDS, 3, "f32", False, position=position % 2 ** 32).process(_dev(torch_cuda, x)).cpu().numpy()
        assert np.array_equal(got, ddc_ref(h, x, down, BANDS, position, None, "f32")[0])
        assert _same(got, low)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("taps,down", [(64, 4), (17, 3), (255, 16), (5, 50)])
def test_nan_reaches_exactly_its_outputs(sd, torch_cuda, taps, down, variant):
    rng = np.random.default_rng(taps)
    S = 700 * down
    h = rng.uniform(0.5, 1.5, taps)  # no zero taps
    bands = [(0, F1, 0), (2, F2, 0), (0, 0x40000001, 3)]  # frequencies whose cos and sin are never 0 over 255 taps
    x = _rand(rng, (3, S), "f32", False)
    hist = _rand(rng, (3, taps - 1), "f32", False)
    clean_bank = _bank(sd, h, down, bands, 3, "f32", False, variant, hist)
    clean = clean_bank.process(_dev(torch_cuda, x)).cpu().numpy()
    p = S // 2 + 1
    m = np.arange(S // down)
    hit = (m >= -(-p // down)) & (m <= (p + taps - 1) // down)
    for poisoned in (0, 1):  # channel 1: no band names it
        xp = x.copy()
        xp[poisoned, p] = np.nan
        b = _bank(sd, h, down, bands, 3, "f32", False, variant, hist)
        got = b.process(_dev(torch_cuda, xp)).cpu().numpy()
        for i, (src, _, _) in enumerate(bands):
            want_nan = hit if src == poisoned else np.zeros_like(hit)
            assert np.array_equal(np.isnan(got[i].real), want_nan) and np.array_equal(np.isnan(got[i].imag), want_nan), (poisoned, i)
            assert _same(got[i][~want_nan], clean[i][~want_nan]), (poisoned, i)
        assert _same(b.state.cpu().numpy(), clean_bank.state.cpu().numpy())  # p is far from the end: no state row holds it


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, precision, cplx):
    """in, out and state carved 0, 1 or 2 elements past a 512-byte boundary out of NaN-filled (and pattern-filled) arenas, padded
    strides: the interior has the aligned run's bits and nothing outside it is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(25)
    taps, down = 17, 4
    H = taps - 1
    h = rng.standard_normal(taps)
    nb = len(BANDS)
    b = _bank(sd, h, down, BANDS, 3, precision, cplx)
    S = (b.info()["block_out"] + 9) * down
    M = S // down
    x = _rand(rng, (3, S), precision, cplx)
    hist = _rand(rng, (3, H), precision, cplx)
    ref = _bank(sd, h, down, BANDS, 3, precision, cplx, 0, hist, 8 * down)
    clean = ref.process(_dev(torch, x))
    clean_state = ref.state
    for variant in (0, 1):
        b = _bank(sd, h, down, BANDS, 3, precision, cplx, variant)
        b._ensure_plan()
        for lead in (0, 1, 2):
            for fill in arena.fills(clean.dtype):
                fin = arena.fills(_dev(torch, x).dtype)[0 if fill != fill else 1]
                ain, vin = arena.framed(torch, (3, S), _dev(torch, x).dtype, lead, 64, fin, row_stride=S + 5)
                aout, vout = arena.framed(torch, (nb, M), clean.dtype, lead, 64, fill, row_stride=M + 3)
                ast, vst = arena.framed(torch, (3, H), _dev(torch, x).dtype, lead, 64, fin)
                vin[:, :S].copy_(_dev(torch, x))
                vst.copy_(_dev(torch, hist))
                before = [arena.bits(a).clone() for a in (ain, aout, ast)]
                assert lib.sdsp_hip_ddc_process(b._plan, vin.data_ptr(), S + 5, vout.data_ptr(), M + 3, S, 8 * down, vst.data_ptr(),
                                                None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, fill)
                assert arena.same_bits(vout[:, :M], clean), tag
                assert arena.same_bits(vst, clean_state), tag
                arena.assert_frame_untouched(before[0], ain, slice(0, 0))  # in is never written
                arena.assert_frame_untouched(before[1], aout, arena.interior_mask(torch, aout, vout, M))
                arena.assert_frame_untouched(before[2], ast, arena.interior_mask(torch, ast, vst))


def test_row_strides_beyond_32_bits(sd, torch_cuda):
    """two channels 2^32 + 64 f32 elements apart inside one allocation, of which only the two rows are written"""
    torch = torch_cuda
    rng = np.random.default_rng(26)
    taps, down, S = 17, 4, 4096
    stride = (1 << 32) + 64
    h = rng.standard_normal(taps)
    x = _rand(rng, (2, S), "f32", False)
    bands = [(1, F1, 5), (0, F2, 0)]
    big = torch.empty(stride + S, dtype=torch.float32, device="cuda")
    big[:S].copy_(_dev(torch, x[0]))
    big[stride:stride + S].copy_(_dev(torch, x[1]))
    lib = sd.load()
    want = ddc_ref(h, x, down, bands, 0, None, "f32")[0]
    for variant in (0, 1):
        b = _bank(sd, h, down, bands, 2, "f32", False, variant)
        b._ensure_plan()
        out = torch.zeros((2, S // down), dtype=torch.complex64, device="cuda")
        state = torch.zeros((2, taps - 1), dtype=torch.float32, device="cuda")
        assert lib.sdsp_hip_ddc_process(b._plan, big.data_ptr(), stride, out.data_ptr(), S // down, S, 0, state.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), variant
        assert np.array_equal(state.cpu().numpy(), x[:, ::-1][:, :taps - 1]), variant
    del big
    torch.cuda.empty_cache()


def test_error_codes_and_launch_count(sd, torch_cuda):
    torch = torch_cuda
    lib = sd.load()
    b = _bank(sd, np.ones(16), 4, [(0, F1, 0), (1, F2, 0)], 2, "f32", False)
    b._ensure_plan()
    p = b._plan
    x = torch.zeros((2, 64), device="cuda")
    y = torch.zeros((2, 16), dtype=torch.complex64, device="cuda")
    run = lambda *a: lib.sdsp_hip_ddc_process(p, *a, None, None)  # noqa: E731
    assert run(x.data_ptr(), 64, y.data_ptr(), 16, 64, 0) == 0
    assert run(x.data_ptr(), 64, y.data_ptr(), 16, 63, 0) == -1  # not a multiple of D
    assert run(None, 64, y.data_ptr(), 16, 64, 0) == -5
    assert run(x.data_ptr(), 64, None, 16, 64, 0) == -5
    assert run(x.data_ptr(), 60, y.data_ptr(), 16, 64, 0) == -5  # in_stride < samples
    assert run(x.data_ptr(), 64, y.data_ptr(), 15, 64, 0) == -5  # out_stride < outputs
    assert run(x.data_ptr(), 64, x.data_ptr() + 8 * 4, 16, 64, 0) == -5  # overlap
    assert run(x.data_ptr() + 2, 64, y.data_ptr(), 16, 32, 0) == -5  # misaligned
    assert run(x.data_ptr(), 64, y.data_ptr(), 16, 0, 0) == 0
    assert lib.sdsp_hip_ddc_process(None, x.data_ptr(), 64, y.data_ptr(), 16, 64, 0, None, None) == -5
    assert lib.sdsp_hip_ddc_plan_set_variant(p, 2) == -5
    n = C.c_uint64(0)
    assert lib.sdsp_hip_ddc_state_bytes(p, C.byref(n)) == 0 and n.value == 2 * 15 * 4
    # the band kernel, and one launch for the new history when T > 1
    assert b.launches(64) == 2 and b.launches(0) == 0
    assert _bank(sd, np.ones(1), 4, [(0, 0, 0)], 1, "f32", False).launches(64) == 1
    with pytest.raises(sd.SdspHipError):
        b.launches(63)
    info = b.info()
    assert (info["taps"], info["down"], info["channels"], info["bands"], info["hist"]) == (16, 4, 2, 2, 15)
    assert info["kernel"] == "sdsp_ddc_kernel" and info["block_out"] == 512 and info["input_kind"] == sd.DDC_REAL
    b.set_variant(1)
    assert b.info()["kernel"] == "sdsp_ddc_plain_kernel"
    with pytest.raises(sd.SdspHipError):
        b.process(torch.zeros((2, 63), device="cuda"))


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(27)
    taps, down, S = 65, 3, 1500
    for cplx in (False, True):
        h = rng.standard_normal(taps)
        x = _rand(rng, (3, S), "f64", cplx)
        hist = _rand(rng, (3, taps - 1), "f64", cplx)
        b = _bank(sd, h, down, BANDS, 3, "f64", cplx, 0, hist, 77 * down)
        dev = b.process(_dev(torch_cuda, x)).cpu().numpy()
        out = np.zeros((len(BANDS), S // down), dtype=np.complex128)
        st = hist.copy()
        assert lib.sdsp_hip_ddc_process_host(b._plan, x.ctypes.data, S, out.ctypes.data, S // down, S, 77 * down, st.ctypes.data) == 0
        assert _same(out, dev)
        assert _same(st, b.state.cpu().numpy())


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(28)
    taps, down, S = 64, 64, 65536  # a line of about 60 KiB of LDS: the launch needs nothing set up under capture
    h = rng.standard_normal(taps)
    x = _rand(rng, (3, S), "f32", False)
    want = _bank(sd, h, down, BANDS, 3, "f32", False).process(_dev(torch, x)).cpu().numpy()
    b = _bank(sd, h, down, BANDS, 3, "f32", False)
    xd = _dev(torch, x)
    out = torch.empty((len(BANDS), S // down), dtype=torch.complex64, device="cuda")
    b.process(xd, out=out)  # plan + state exist before capture
    b.reset()
    b._state = torch.zeros((3, taps - 1), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.process(xd, out=out)
    b._state.zero_()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), want)
