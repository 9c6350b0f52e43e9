"""GPU tests of the digital up-converter bank (sdsp_hip_duc_*) on a real MI355X.

The checker is tests/duc_ref.py, the contract's operation order in numpy, itself pinned to scipy.signal.upfirdn -> mix -> sum in
tests/test_duc_host.py.  Both precisions, both output kinds and both kernel variants are held to bit-exact agreement with it."""
import ctypes as C

import numpy as np
import pytest

import arena
from duc_ref import BLOCKS, GRID_T, GRID_U, duc_ref, hist_len

pytestmark = pytest.mark.gpu

F1, F2, F3 = 0x12345678, (1 << 32) - 0x01000001, 1 << 31
# channel 0: one band; channel 1: nine (three chunks of a four-band chunking), two of them one band twice; channel 2: none
BANDS = [(1, F1, 0x0badcafe), (1, F2, 7), (0, F3, 1 << 30), (1, F2, 7), (1, 0, 0), (1, 0x40000001, 5), (1, F3, 0), (1, 1, 0xffffffff),
         (1, F1, 1 << 31), (1, 0xdeadbeef, 3)]
NB = len(BANDS)


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


def _cdt(precision):
    return np.complex128 if precision == "f64" else np.complex64


def _rand(rng, shape, precision):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(_cdt(precision))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bank(sd, h, up, bands, channels, precision, kind="complex", variant=0, state=None, position=0):
    import torch
    b = sd.duc_bank(len(h), up, bands, channels, kind, sd.F64 if precision == "f64" else sd.F32)
    b.set_coeff(h)
    b.set_variant(variant)
    b.position = position
    if state is not None:
        st = np.ascontiguousarray(state.astype(_cdt(precision)))
        b._state = torch.from_numpy(st if st.shape[1] else np.zeros((st.shape[0], 1), dtype=st.dtype)).cuda()
    return b


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _stream(torch, b, x, blocks):
    parts, s0 = [], 0
    for n in blocks:
        parts.append(b.process(_dev(torch, x[:, s0:s0 + n].copy())).cpu().numpy())
        s0 += n
    assert s0 == x.shape[1]
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("up", GRID_U)
@pytest.mark.parametrize("taps", GRID_T)
def test_bit_exact_against_reference(sd, torch_cuda, taps, up):
    """every precision, kind and variant, streamed through BLOCKS in a unit chosen from the plan's block size: the longest call spans
    a workgroup boundary and ends in a partial block, the shortest are empty or shorter than H"""
    rng = np.random.default_rng(taps * 7919 + up)
    h = rng.standard_normal(taps)
    H = hist_len(taps, up)
    for precision in ("f32", "f64"):
        unit = _bank(sd, h, up, BANDS, 3, precision).info()["block_in"] // 8 + 1
        blocks = [v * unit for v in BLOCKS]
        S = sum(blocks)
        x = _rand(rng, (NB, S), precision)
        hist = _rand(rng, (NB, H), precision)
        position = int(rng.integers(0, 1 << 34))
        for kind in ("complex", "real"):
            want, want_state = duc_ref(h, x, up, BANDS, 3, kind, position, hist, precision)
            for variant in (0, 1):
                b = _bank(sd, h, up, BANDS, 3, precision, kind, variant, hist, position)
                got = _stream(torch_cuda, b, x, blocks)
                tag = (precision, kind, variant, S)
                assert got.shape == want.shape and got.dtype == want.dtype, tag
                assert np.array_equal(got, want), (tag, int((got != want).sum()))
                assert not got[2].any() and not np.signbit(got[2].real).any(), tag  # the channel without bands: +0
                if H:
                    assert np.array_equal(b.state.cpu().numpy(), want_state), tag
                assert b.position == position + S


@pytest.mark.parametrize("taps,up", [(4096, 1024), (4096, 1), (1, 1024)])
def test_longest_plans_run_and_match_the_plain_kernel(sd, torch_cuda, taps, up):
    """the largest T and U: f64 with T = 4096, U = 1 stages 32 KiB of taps and a line of 4095 + block_in elements, above the 64 KiB
    target; U = 1024 makes blocks of one input position"""
    rng = np.random.default_rng(taps + up)
    h = rng.standard_normal(taps)
    H = hist_len(taps, up)
    bands = [(0, F1, 5), (1, F2, 0), (0, 0x40000001, 9)]
    for precision in ("f32", "f64"):
        block = _bank(sd, h, up, bands, 2, precision).info()["block_in"]
        assert block == max(1, 1024 // up)
        S = 2 * block + max(1, block // 3)
        x = _rand(rng, (3, S), precision)
        hist = _rand(rng, (3, H), precision)
        position = 2 ** 32 - 3
        outs, states = [], []
        for variant in (0, 1):
            b = _bank(sd, h, up, bands, 2, precision, "complex", variant, hist, position)
            outs.append(b.process(_dev(torch_cuda, x)).cpu().numpy())
            states.append(b.state.cpu().numpy())
        assert outs[0].shape == (2, S * up)
        assert _same(outs[0], outs[1]), precision
        assert _same(states[0], states[1]), precision
        if H <= 3:  # few filter steps: the numpy reference is quick
            want, want_state = duc_ref(h, x, up, bands, 2, "complex", position, hist, precision)
            assert np.array_equal(outs[0], want), precision
            if H:
                assert np.array_equal(states[0], want_state), precision


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_zero_frequency_is_the_interpolating_resampler(sd, torch_cuda, precision):
    """fcw = 0, phase0 = 0: w = (1, +0) exactly, so each plane is fir_resampler(U, 1) of that plane, as values (== : the sign of a
    zero is not part of the claim)"""
    rng = np.random.default_rng(21)
    prec = sd.F64 if precision == "f64" else sd.F32
    for taps, up in [(64, 4), (17, 3), (255, 16), (5, 50)]:
        h = rng.standard_normal(taps)
        x = _rand(rng, (4, 300), precision)
        b = _bank(sd, h, up, [(c, 0, 0) for c in range(4)], 4, precision)
        y = b.process(_dev(torch_cuda, x)).cpu().numpy()
        for plane, part in ((x.real, y.real), (x.imag, y.imag)):
            r = sd.fir_resampler(taps, up, 1, 4, prec)
            r.set_coeff(h)
            want = r.process(_dev(torch_cuda, np.ascontiguousarray(plane))).cpu().numpy()
            assert want.shape == part.shape
            assert np.all(part == want), (taps, up)


def test_half_rate_band_is_the_sign_alternated_stream(sd, torch_cuda):
    """fcw = 2^31: w = C[32768 (n mod 2)] (x) F[0] conjugated = ((-1)^n, +-0) exactly, and sign changes are exact in every product and
    sum: the output is the fcw = 0 output with every odd stream index negated (position U even: n and r have one parity)"""
    rng = np.random.default_rng(22)
    for precision in ("f32", "f64"):
        for taps, up in [(64, 4), (17, 3), (255, 1)]:
            h = rng.standard_normal(taps)
            x = _rand(rng, (1, 400), precision)
            a = _bank(sd, h, up, [(0, 1 << 31, 0)], 1, precision, position=2).process(_dev(torch_cuda, x)).cpu().numpy()
            b = _bank(sd, h, up, [(0, 0, 0)], 1, precision, position=2).process(_dev(torch_cuda, x)).cpu().numpy()
            sign = np.where(np.arange(400 * up) % 2 == 0, 1, -1)
            assert np.all(a.real == b.real * sign) and np.all(a.imag == b.imag * sign), (precision, taps, up)


@pytest.mark.parametrize("kind", ["complex", "real"])
def test_superposition_of_two_bands(sd, torch_cuda, kind):
    """bands A and B into one channel: (0 + yA) + yB is the rounded sum of the two single-band outputs"""
    rng = np.random.default_rng(29)
    for precision in ("f32", "f64"):
        for taps, up in [(64, 4), (17, 3), (40, 96)]:
            h = rng.standard_normal(taps)
            x = _rand(rng, (2, 300), precision)
            A, B = (0, F1, 11), (0, F2, 1 << 29)
            both = _bank(sd, h, up, [A, B], 1, precision, kind).process(_dev(torch_cuda, x)).cpu().numpy()
            ya = _bank(sd, h, up, [A], 1, precision, kind).process(_dev(torch_cuda, x[:1])).cpu().numpy()
            yb = _bank(sd, h, up, [B], 1, precision, kind).process(_dev(torch_cuda, x[1:])).cpu().numpy()
            assert np.all(both == ya + yb), (precision, taps, up)


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_streaming_equals_one_call(sd, torch_cuda, precision, kind):
    rng = np.random.default_rng(23)
    for taps, up in [(17, 4), (255, 3), (64, 50), (33, 1)]:  # H = 4, 84, 1, 32: most calls are shorter than H
        H = hist_len(taps, up)
        S = sum(BLOCKS)
        h = rng.standard_normal(taps)
        x = _rand(rng, (NB, S), precision)
        hist = _rand(rng, (NB, H), precision)
        pos0 = (2 ** 32 - 5 * up) // up  # the phase index wraps inside the stream
        for start in (hist, None):  # a random history; and a fresh stream
            one = _bank(sd, h, up, BANDS, 3, precision, kind, 0, start, pos0)
            want = one.process(_dev(torch_cuda, x)).cpu().numpy()
            b = _bank(sd, h, up, BANDS, 3, precision, kind, 0, start, pos0)
            assert _same(_stream(torch_cuda, b, x, BLOCKS), want), (taps, up)
            assert _same(b.state.cpu().numpy(), one.state.cpu().numpy())
            assert b.position == pos0 + S
        # state = NULL through the C entry: zero history, nothing carried
        lib = sd.load()
        one._ensure_plan()
        xd = _dev(torch_cuda, x)
        out = torch_cuda.zeros((3, S * up), dtype=one._out_dtype(), device="cuda")
        assert lib.sdsp_hip_duc_process(one._plan, xd.data_ptr(), S, out.data_ptr(), S * up, S, pos0, None, None) == 0
        assert _same(out.cpu().numpy(), want)


def test_phase_wrap_and_large_positions(sd, torch_cuda):
    rng = np.random.default_rng(24)
    taps, up = 17, 4
    h = rng.standard_normal(taps)
    x = _rand(rng, (NB, 64), "f32")
    for position in (2 ** 32 - 3, 2 ** 40 + 5, 2 ** 30 - 1):  # position U wraps 2^32 in the last one
        got = _bank(sd, h, up, BANDS, 3, "f32", position=position).process(_dev(torch_cuda, x)).cpu().numpy()
        high = _bank(sd, h, up, BANDS, 3, "f32", position=position + 2 ** 32).process(_dev(torch_cuda, x)).cpu().numpy()
        assert np.array_equal(got, duc_ref(h, x, up, BANDS, 3, "complex", position, None, "f32")[0])
        assert _same(got, high)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("taps,up", [(64, 4), (17, 3), (255, 16), (5, 50)])
def test_nan_reaches_exactly_its_outputs(sd, torch_cuda, taps, up, variant):
    """a NaN at input m0 of band i: outputs [m0 U, min(m0 U + T, S U)) of channel dst_i and nothing else, on both sides of a
    workgroup boundary of the fused kernel"""
    rng = np.random.default_rng(taps)
    h = rng.uniform(0.5, 1.5, taps)
    bands = [(0, F1, 0), (2, F2, 0), (0, 0x40000001, 3), (1, F1, 9)]
    H = hist_len(taps, up)
    for kind in ("complex", "real"):
        clean_bank = _bank(sd, h, up, bands, 3, "f32", kind, variant)
        block = clean_bank.info()["block_in"]
        S = 2 * block + 5
        x = _rand(rng, (4, S), "f32")
        hist = _rand(rng, (4, H), "f32")
        clean_bank = _bank(sd, h, up, bands, 3, "f32", kind, variant, hist)
        clean = clean_bank.process(_dev(torch_cuda, x)).cpu().numpy()
        r = np.arange(S * up)
        for m0 in (block - 1, block):
            hit = (r >= m0 * up) & (r < min(m0 * up + taps, S * up))
            for band in (0, 1, 2):
                xp = x.copy()
                xp[band, m0] = np.nan
                b = _bank(sd, h, up, bands, 3, "f32", kind, variant, hist)
                got = b.process(_dev(torch_cuda, xp)).cpu().numpy()
                for c in range(3):
                    want_nan = hit if c == bands[band][0] else np.zeros_like(hit)
                    tag = (kind, m0, band, c)
                    assert np.array_equal(np.isnan(got[c].real), want_nan), tag
                    if kind == "complex":
                        assert np.array_equal(np.isnan(got[c].imag), want_nan), tag
                    assert _same(got[c][~want_nan], clean[c][~want_nan]), tag
                if H:  # m0 is more than H from the end: no state row holds it
                    assert _same(b.state.cpu().numpy(), clean_bank.state.cpu().numpy())


@pytest.mark.parametrize("kind", ["complex", "real"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, precision, kind):
    """in, out and state carved 0, 1 or 2 elements past a 512-byte boundary out of NaN-filled (and pattern-filled) arenas, padded
    strides: the interior has the aligned run's bits and nothing outside it is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(25)
    taps, up = 17, 4
    H = hist_len(taps, up)
    h = rng.standard_normal(taps)
    b = _bank(sd, h, up, BANDS, 3, precision, kind)
    S = b.info()["block_in"] + 9
    R = S * up
    x = _rand(rng, (NB, S), precision)
    hist = _rand(rng, (NB, H), precision)
    ref = _bank(sd, h, up, BANDS, 3, precision, kind, 0, hist, 8)
    clean = ref.process(_dev(torch, x))
    clean_state = ref.state
    cdt = _dev(torch, x).dtype
    for variant in (0, 1):
        b = _bank(sd, h, up, BANDS, 3, precision, kind, variant)
        b._ensure_plan()
        for lead in (0, 1, 2):
            for fill in arena.fills(clean.dtype):
                fin = arena.fills(cdt)[0 if fill != fill else 1]
                ain, vin = arena.framed(torch, (NB, S), cdt, lead, 64, fin, row_stride=S + 5)
                aout, vout = arena.framed(torch, (3, R), clean.dtype, lead, 64, fill, row_stride=R + 3)
                ast, vst = arena.framed(torch, (NB, H), cdt, lead, 64, fin)
                vin[:, :S].copy_(_dev(torch, x))
                vst.copy_(_dev(torch, hist))
                before = [arena.bits(a).clone() for a in (ain, aout, ast)]
                assert lib.sdsp_hip_duc_process(b._plan, vin.data_ptr(), S + 5, vout.data_ptr(), R + 3, S, 8, vst.data_ptr(), None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, fill)
                assert arena.same_bits(vout[:, :R], clean), tag
                assert arena.same_bits(vst, clean_state), tag
                arena.assert_frame_untouched(before[0], ain, slice(0, 0))  # in is never written
                arena.assert_frame_untouched(before[1], aout, arena.interior_mask(torch, aout, vout, R))
                arena.assert_frame_untouched(before[2], ast, arena.interior_mask(torch, ast, vst))


def test_error_codes_and_launch_count(sd, torch_cuda):
    torch = torch_cuda
    lib = sd.load()
    b = _bank(sd, np.ones(16), 4, [(0, F1, 0), (1, F2, 0)], 2, "f32")
    b._ensure_plan()
    p = b._plan
    x = torch.zeros((2, 16), dtype=torch.complex64, device="cuda")
    y = torch.zeros((2, 64), dtype=torch.complex64, device="cuda")
    run = lambda *a: lib.sdsp_hip_duc_process(p, *a, None, None)  # noqa: E731
    assert run(x.data_ptr(), 16, y.data_ptr(), 64, 16, 0) == 0
    assert run(x.data_ptr(), 16, y.data_ptr(), 64, 15, 0) == 0  # any S
    assert run(None, 16, y.data_ptr(), 64, 16, 0) == -5
    assert run(x.data_ptr(), 16, None, 64, 16, 0) == -5
    assert run(x.data_ptr(), 15, y.data_ptr(), 64, 16, 0) == -5  # in_stride < samples
    assert run(x.data_ptr(), 16, y.data_ptr(), 63, 16, 0) == -5  # out_stride < outputs
    assert run(x.data_ptr(), 16, x.data_ptr() + 8 * 8, 64, 16, 0) == -5  # overlap
    assert run(x.data_ptr() + 4, 16, y.data_ptr(), 64, 8, 0) == -5  # misaligned
    assert run(x.data_ptr(), 16, y.data_ptr(), 64, 0, 0) == 0
    assert run(None, 16, None, 64, 0, 0) == 0  # nothing to do
    assert lib.sdsp_hip_duc_process(None, x.data_ptr(), 16, y.data_ptr(), 64, 16, 0, None, None) == -5
    assert lib.sdsp_hip_duc_plan_set_variant(p, 2) == -5
    n = C.c_uint64(0)
    assert lib.sdsp_hip_duc_state_bytes(p, C.byref(n)) == 0 and n.value == 2 * 3 * 8
    # the band kernel, and one launch for the new history when H > 0
    assert b.launches(64) == 2 and b.launches(0) == 0
    assert _bank(sd, np.ones(4), 4, [(0, 0, 0)], 1, "f32").launches(64) == 1  # T <= U: H = 0
    info = b.info()
    assert (info["taps"], info["up"], info["channels"], info["bands"], info["hist"]) == (16, 4, 2, 2, 3)
    assert info["kernel"] == "sdsp_duc_kernel" and info["block_in"] == 256 and info["output_kind"] == sd.DUC_COMPLEX
    b.set_variant(1)
    assert b.info()["kernel"] == "sdsp_duc_plain_kernel"
    with pytest.raises(ValueError):
        b.process(torch.zeros((2, 16), device="cuda"))  # not complex
    with pytest.raises(ValueError):
        b.process(torch.zeros((3, 16), dtype=torch.complex64, device="cuda"))  # three rows for two bands


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(27)
    taps, up, S = 65, 3, 500
    H = hist_len(taps, up)
    for kind, odt in (("complex", np.complex128), ("real", np.float64)):
        h = rng.standard_normal(taps)
        x = _rand(rng, (NB, S), "f64")
        hist = _rand(rng, (NB, H), "f64")
        b = _bank(sd, h, up, BANDS, 3, "f64", kind, 0, hist, 77)
        dev = b.process(_dev(torch_cuda, x)).cpu().numpy()
        out = np.zeros((3, S * up), dtype=odt)
        st = hist.copy()
        assert lib.sdsp_hip_duc_process_host(b._plan, x.ctypes.data, S, out.ctypes.data, S * up, S, 77, st.ctypes.data) == 0
        assert _same(out, dev)
        assert _same(st, b.state.cpu().numpy())


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(28)
    taps, up, S = 64, 16, 4096
    H = hist_len(taps, up)
    h = rng.standard_normal(taps)
    x = _rand(rng, (NB, S), "f32")
    want = _bank(sd, h, up, BANDS, 3, "f32").process(_dev(torch, x)).cpu().numpy()
    b = _bank(sd, h, up, BANDS, 3, "f32")
    xd = _dev(torch, x)
    out = torch.empty((3, S * up), dtype=torch.complex64, device="cuda")
    b.process(xd, out=out)  # plan + state exist before capture
    b.reset()
    b._state = torch.zeros((NB, H), dtype=torch.complex64, device="cuda")
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
