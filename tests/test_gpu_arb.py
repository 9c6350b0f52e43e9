"""GPU tests of the arbitrary-ratio polyphase resampler bank (sdsp_hip_arb_*) on a real MI355X.

The checker is tests/arb_ref.py, the contract's operation order in numpy, itself pinned to the textbook form and to resample_ref in
tests/test_arb_host.py.  Both precisions, both input kinds, both interpolation modes and both kernel variants are held to bit-exact
agreement with it, output, carried history and stream time alike."""
import ctypes as C

import numpy as np
import pytest

import arena
from arb_ref import BLOCKS, ONE, arb_ref, out_samples, real_dtype, step_of

pytestmark = pytest.mark.gpu

GRID_LT = [(1, 1), (1, 5), (4, 5), (32, 16)]
GRID_STEP = [1 << 22, ONE - 1, ONE, ONE + 1, step_of(0.7317), step_of(2.37), step_of(37.5)]


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


def _bank(sd, h, L, T, max_step, precision, cplx, interp, variant=0, state=None, step=None, time=0):
    import torch
    b = sd.arb_resampler(L, T, int(max_step), "complex" if cplx else "real", interp, sd.F64 if precision == "f64" else sd.F32)
    b.set_coeff(h)
    b.set_variant(variant)
    b.step = int(max_step if step is None else step)
    b.time = time
    if state is not None:
        b._state = torch.from_numpy(np.ascontiguousarray(state.astype(_in_dtype(precision, cplx)))).cuda()
    return b


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _unit(block_out, step):
    """input samples that make a little under half a block of outputs: the BLOCKS multiples 3, 7 and 11 then end inside a block
    and span one or more workgroup boundaries"""
    return max(1, -(-(9 * block_out * step) // (20 * ONE)))


LDS_TARGETS = (32 * 1024, 64 * 1024, 144 * 1024)


def _check_block_out(block, L, T, max_step, precision, cplx, linear):
    """the LDS rule of DESIGN.md section 5.21 from first principles, not by its formula: the padded table and the staged span of
    `block` outputs at max_step -- ((block - 1) max_step >> 32) + T + 1 elements -- fit the plan's LDS target, and one output more
    would not (or the block is at its cap of 1024).  The target is the smallest of 32, 64 and 144 KiB whose table bound (8 KiB, 32
    KiB, none) admits the table and that holds the table plus one output's line"""
    rs = 8 if precision == "f64" else 4
    es, ws = rs * (2 if cplx else 1), rs * (2 if linear else 1)
    tb = -(-(L * ((T | 1) if L > 1 else T) * ws) // 16) * 16

    def lds(outs):
        return tb + ((((outs - 1) * max_step) >> 32) + T + 1) * es

    target = next(t for t, bound in zip(LDS_TARGETS, (8 * 1024, 32 * 1024, tb)) if tb <= bound and lds(1) <= t)
    assert 1 <= block <= 1024, block
    assert lds(block) <= target, (block, lds(block), target)
    assert block == 1024 or lds(block + 1) > target, (block, lds(block + 1), target)


def _stream(torch, b, x, blocks):
    """x through the bank in calls of `blocks` samples; returns the concatenated output"""
    parts, s0 = [], 0
    for n in blocks:
        parts.append(b.process(_dev(torch, x[:, s0:s0 + n].copy())).cpu().numpy())
        s0 += n
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("step", GRID_STEP)
@pytest.mark.parametrize("L,T", GRID_LT)
def test_bit_exact_against_reference(sd, torch_cuda, L, T, step):
    """every precision, kind, mode and variant, streamed through calls that are empty, shorter than the history, end inside a block
    and span workgroups; three channels with a random history; a random time, for complex input one beyond the first calls"""
    rng = np.random.default_rng(L * 7919 + T * 31 + step % 1000)
    h = rng.standard_normal(L * T)
    H = T - 1
    for precision in ("f32", "f64"):
        for cplx in (False, True):
            for interp in ("nearest", "linear"):
                info = _bank(sd, h, L, T, step, precision, cplx, interp).info()
                _check_block_out(info["block_out"], L, T, step, precision, cplx, interp == "linear")
                unit = _unit(info["block_out"], step)
                blocks = [v * unit for v in BLOCKS]
                S = sum(blocks)
                x = _rand(rng, (3, S), precision, cplx)
                hist = _rand(rng, (3, max(H, 1)), precision, cplx)
                time0 = int(rng.integers(0, step)) + ((unit << 32) if cplx else 0)  # complex: nothing before the third call's block
                want, want_state, want_time = arb_ref(h, L, T, x, step, time0, hist[:, :H], interp, precision)
                for variant in (0, 1):
                    b = _bank(sd, h, L, T, step, precision, cplx, interp, variant, hist, step, time0)
                    got = _stream(torch_cuda, b, x, blocks)
                    tag = (precision, cplx, interp, variant, S)
                    assert got.shape == want.shape, tag
                    assert np.array_equal(got, want), (tag, int((got != want).sum()))
                    if H:
                        assert np.array_equal(b.state.cpu().numpy(), want_state), tag
                    assert b.time == want_time, tag


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_step_changes_between_calls(sd, torch_cuda, precision, cplx):
    rng = np.random.default_rng(31)
    L, T = 32, 16
    steps = [step_of(0.7317), step_of(1.0000131), step_of(2.37)]
    h = rng.standard_normal(L * T)
    sizes = [1500, 7, 2100]
    x = _rand(rng, (3, sum(sizes)), precision, cplx)
    hist = _rand(rng, (3, T - 1), precision, cplx)
    for variant in (0, 1):
        b = _bank(sd, h, L, T, steps[2], precision, cplx, "linear", variant, hist, steps[0], 99)
        state, time, s0 = hist, 99, 0
        for n, step in zip(sizes, steps):
            b.step = step
            got = b.process(_dev(torch_cuda, x[:, s0:s0 + n].copy())).cpu().numpy()
            want, state, time = arb_ref(h, L, T, x[:, s0:s0 + n], step, time, state, "linear", precision)
            assert np.array_equal(got, want), (variant, step)
            assert np.array_equal(b.state.cpu().numpy(), state) and b.time == time
            s0 += n


@pytest.mark.parametrize("L,T,D", [(8, 8, 3), (32, 4, 32)])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_nearest_at_a_rational_step_is_the_polyphase_resampler(sd, torch_cuda, precision, L, T, D):
    rng = np.random.default_rng(L + D)
    prec = sd.F64 if precision == "f64" else sd.F32
    q = D // int(np.gcd(L, D))
    S = q * 700
    h = rng.standard_normal(L * T)
    x = _rand(rng, (3, S), precision, False)
    r = sd.fir_resampler(L * T, L, D, 3, prec)
    r.set_coeff(h)
    want = r.process(_dev(torch_cuda, x)).cpu().numpy()
    for variant in (0, 1):
        b = _bank(sd, h, L, T, (D << 32) // L, precision, False, "nearest", variant)
        got = b.process(_dev(torch_cuda, x)).cpu().numpy()
        assert _same(got, want), variant
        assert _same(b.state.cpu().numpy(), r.state.cpu().numpy()) and b.time == 0


LARGEST = {  # (L, T, precision, interp) -> block_out at max_step = 2^42, worked out by hand from the rule (complex input)
    (1024, 4, "f64", "linear"): 4,     # 80 KiB of table (row pad), 4096 pairs of line: (4096 - 5) >> 10 = 3 further outputs
    (16, 256, "f64", "linear"): 5,     # 64.25 KiB of table, 5104 pairs: (5104 - 257) >> 10 = 4
    (1, 4096, "f64", "nearest"): 3,    # 32 KiB of table, but one output's line is 64 KiB: the 144 KiB target, 7168 pairs, 3071 >> 10 = 2
    (1, 4096, "f32", "linear"): 10,    # 32 KiB of table + 4097 pairs of 8 bytes = 64 KiB + 8: the 144 KiB target, 14336 pairs, 10239 >> 10 = 9
}


@pytest.mark.parametrize("max_step", [1 << 42, 1 << 22])
@pytest.mark.parametrize("L,T,precision,interp", list(LARGEST))
def test_largest_plans(sd, torch_cuda, L, T, precision, interp, max_step):
    """L T = 4096, complex input: a table of 64 KiB and more next to the line, or (L = 1) a line of 4097 elements that pushes a
    small table to the largest target; at max_step = 2^42 a block is a handful of outputs, each 1024 samples from the last"""
    rng = np.random.default_rng(L + T)
    h = rng.standard_normal(L * T)
    block = 1024 if max_step == 1 << 22 else LARGEST[(L, T, precision, interp)]
    _check_block_out(block, L, T, max_step, precision, True, interp == "linear")
    S = -(-((3 * block + 1) * max_step) // ONE)
    x = _rand(rng, (3, S), precision, True)
    hist = _rand(rng, (3, T - 1), precision, True)
    time0 = max_step // 3
    want, want_state, want_time = arb_ref(h, L, T, x, max_step, time0, hist, interp, precision)
    assert want.shape[1] > 2 * block
    for variant in (0, 1):
        b = _bank(sd, h, L, T, max_step, precision, True, interp, variant, hist, max_step, time0)
        assert b.info()["block_out"] == block
        got = b.process(_dev(torch_cuda, x)).cpu().numpy()
        assert np.array_equal(got, want), variant
        assert np.array_equal(b.state.cpu().numpy(), want_state) and b.time == want_time


@pytest.mark.parametrize("max_step", [1 << 42, ONE, 1 << 22])
def test_block_out_fits_its_target_where_one_line_outgrows_a_small_table(sd, torch_cuda, max_step):
    """L = 1 with thousands of taps: a table of at most 64 KiB whose single output needs a line as long again, on both sides of the
    sizes at which the line stops fitting beside the table; every precision, kind and mode"""
    for T in (2047, 2048, 2730, 2731, 4095, 4096):
        for precision in ("f32", "f64"):
            for cplx in (False, True):
                for interp in ("nearest", "linear"):
                    info = _bank(sd, np.ones(T), 1, T, max_step, precision, cplx, interp).info()
                    _check_block_out(info["block_out"], 1, T, max_step, precision, cplx, interp == "linear")


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_null_state_is_zero_history_and_nothing_is_carried(sd, torch_cuda, precision):
    """state = NULL through the C entry, complex input, both variants: the values of a zero history, bit for bit"""
    lib = sd.load()
    rng = np.random.default_rng(41)
    L, T, step, time0 = 32, 16, step_of(0.7317), 4321
    h = rng.standard_normal(L * T)
    b = _bank(sd, h, L, T, step, precision, True, "linear")
    S = -(-((b.info()["block_out"] + 50) * step) // ONE)
    x = _rand(rng, (3, S), precision, True)
    want, _, _ = arb_ref(h, L, T, x, step, time0, None, "linear", precision)
    M = want.shape[1]
    for variant in (0, 1):
        b.set_variant(variant)
        xd = _dev(torch_cuda, x)
        out = torch_cuda.zeros((3, M), dtype=xd.dtype, device="cuda")
        assert lib.sdsp_hip_arb_process(b._plan, xd.data_ptr(), S, out.data_ptr(), M, 3, S, step, time0, None, None) == 0
        torch_cuda.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), variant


def test_runs_of_several_blocks_per_workgroup(sd, torch_cuda):
    """64 channels of 64 blocks behind a 40 KiB table: a workgroup walks four blocks with one copy of the table.  Variant 0 against
    variant 1 everywhere and against the reference on the first and the last channel"""
    rng = np.random.default_rng(5)
    L, T, step = 1024, 4, step_of(1.0000131)
    S = 64 * 1024
    h = rng.standard_normal(L * T)
    x = _rand(rng, (64, S), "f32", False)
    hist = _rand(rng, (64, T - 1), "f32", False)
    outs = []
    for variant in (0, 1):
        b = _bank(sd, h, L, T, step, "f32", False, "linear", variant, hist, step, 12345)
        assert b.info()["block_out"] == 1024
        outs.append(b.process(_dev(torch_cuda, x)).cpu().numpy())
    assert _same(outs[0], outs[1])
    for c in (0, 63):
        want, _, _ = arb_ref(h, L, T, x[c:c + 1], step, 12345, hist[c:c + 1], "linear", "f32")
        assert np.array_equal(outs[0][c:c + 1], want), c


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, precision, cplx):
    """in, out and state carved 0, 1 or 2 elements past a 512-byte boundary out of NaN-filled (and pattern-filled) arenas, padded
    strides: the interior has the aligned run's bits and nothing outside it -- past n_out, around every row -- is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(25)
    L, T, step = 4, 5, step_of(0.7317)
    H = T - 1
    h = rng.standard_normal(L * T)
    b = _bank(sd, h, L, T, step, precision, cplx, "linear")
    S = -(-((b.info()["block_out"] + 9) * step) // ONE)
    M, _ = out_samples(step, 777, S)
    x = _rand(rng, (3, S), precision, cplx)
    hist = _rand(rng, (3, H), precision, cplx)
    ref = _bank(sd, h, L, T, step, precision, cplx, "linear", 0, hist, step, 777)
    clean = ref.process(_dev(torch, x))
    clean_state = ref.state
    for variant in (0, 1):
        b = _bank(sd, h, L, T, step, precision, cplx, "linear", variant)
        b._ensure_plan()
        for lead in (0, 1, 2):
            for fill in arena.fills(clean.dtype):
                ain, vin = arena.framed(torch, (3, S), clean.dtype, lead, 64, fill, row_stride=S + 5)
                aout, vout = arena.framed(torch, (3, M), clean.dtype, lead, 64, fill, row_stride=M + 3)
                ast, vst = arena.framed(torch, (3, H), clean.dtype, lead, 64, fill)
                vin[:, :S].copy_(_dev(torch, x))
                vst.copy_(_dev(torch, hist))
                before = [arena.bits(a).clone() for a in (ain, aout, ast)]
                assert lib.sdsp_hip_arb_process(b._plan, vin.data_ptr(), S + 5, vout.data_ptr(), M + 3, 3, S, step, 777, vst.data_ptr(),
                                                None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, fill)
                assert arena.same_bits(vout[:, :M], clean), tag
                assert arena.same_bits(vst, clean_state), tag
                arena.assert_frame_untouched(before[0], ain, slice(0, 0))  # in is never written
                arena.assert_frame_untouched(before[1], aout, arena.interior_mask(torch, aout, vout, M))
                arena.assert_frame_untouched(before[2], ast, arena.interior_mask(torch, ast, vst))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("L,T,ratio", [(32, 16, 0.7317), (4, 5, 2.37), (1, 5, 37.5), (1, 1, 1.0000131)])
def test_nan_reaches_exactly_its_outputs(sd, torch_cuda, L, T, ratio, variant):
    """one NaN in x reaches exactly the outputs whose T-tap window covers it (a NaN times any tap is a NaN), in its channel only"""
    rng = np.random.default_rng(T)
    step = step_of(ratio)
    h = rng.standard_normal(L * T)
    for interp in ("nearest", "linear"):
        block = _bank(sd, h, L, T, step, "f32", False, interp).info()["block_out"]
        S = -(-(2 * block * step + step // 2) // ONE) + T
        x = _rand(rng, (3, S), "f32", False)
        hist = _rand(rng, (3, T - 1), "f32", False)
        clean_bank = _bank(sd, h, L, T, step, "f32", False, interp, variant, hist, step, 4242)
        clean = clean_bank.process(_dev(torch_cuda, x)).cpu().numpy()
        p = -(-(block * step) // ONE)  # near the first block boundary
        i = (4242 + np.arange(clean.shape[1], dtype=np.uint64) * np.uint64(step)) >> np.uint64(32)
        hit = (i >= p) & (i <= p + T - 1)
        assert hit.any() or ratio > T
        xp = x.copy()
        xp[1, p] = np.nan
        b = _bank(sd, h, L, T, step, "f32", False, interp, variant, hist, step, 4242)
        got = b.process(_dev(torch_cuda, xp)).cpu().numpy()
        assert np.array_equal(np.isnan(got[1]), hit), interp
        assert _same(got[1][~hit], clean[1][~hit]) and _same(got[[0, 2]], clean[[0, 2]]), interp
        assert _same(b.state.cpu().numpy(), clean_bank.state.cpu().numpy())  # p is far from the end: no state row holds it


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(27)
    L, T, S, step = 32, 16, 1500, step_of(0.7317)
    for cplx in (False, True):
        h = rng.standard_normal(L * T)
        x = _rand(rng, (3, S), "f64", cplx)
        hist = _rand(rng, (3, T - 1), "f64", cplx)
        b = _bank(sd, h, L, T, step, "f64", cplx, "linear", 0, hist, step, 555)
        M, _ = b.out_samples(S)
        dev = b.process(_dev(torch_cuda, x)).cpu().numpy()
        out = np.zeros((3, M), dtype=x.dtype)
        st = hist.copy()
        assert lib.sdsp_hip_arb_process_host(b._plan, x.ctypes.data, S, out.ctypes.data, M, 3, S, step, 555, st.ctypes.data) == 0
        assert _same(out, dev)
        assert _same(st, b.state.cpu().numpy())


def test_error_codes_and_launch_count(sd, torch_cuda):
    torch = torch_cuda
    lib = sd.load()
    b = _bank(sd, np.ones(64), 4, 16, 2 * ONE, "f32", False, "linear", step=ONE)
    b._ensure_plan()
    p = b._plan
    x = torch.zeros((2, 64), device="cuda")
    y = torch.zeros((2, 64), device="cuda")
    run = lambda *a: lib.sdsp_hip_arb_process(p, *a, None, None)  # noqa: E731
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 2, 64, ONE, 0) == 0
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 2, 64, 2 * ONE + 1, 0) == -1  # above the plan's max_step
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 2, 64, (1 << 22) - 1, 0) == -1
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 2, 64, ONE, 1 << 63) == -1
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 2, 1 << 31, ONE, 0) == -1
    assert run(None, 64, y.data_ptr(), 64, 2, 64, ONE, 0) == -5
    assert run(x.data_ptr(), 64, None, 64, 2, 64, ONE, 0) == -5
    assert run(x.data_ptr(), 64, None, 64, 2, 64, ONE, 64 << 32) == 0  # no output: out is not looked at
    assert run(x.data_ptr(), 60, y.data_ptr(), 64, 2, 64, ONE, 0) == -5  # in_stride < samples
    assert run(x.data_ptr(), 64, y.data_ptr(), 63, 2, 64, ONE, 0) == -5  # out_stride < outputs
    assert run(x.data_ptr(), 64, x.data_ptr() + 8 * 4, 64, 2, 64, ONE, 0) == -5  # overlap
    assert run(x.data_ptr() + 2, 64, y.data_ptr(), 64, 1, 32, ONE, 0) == -5  # misaligned
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 2, 0, ONE, 0) == 0
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 0, 64, ONE, 0) == 0
    assert lib.sdsp_hip_arb_process(None, x.data_ptr(), 64, y.data_ptr(), 64, 2, 64, ONE, 0, None, None) == -5
    assert lib.sdsp_hip_arb_plan_set_variant(p, 2) == -5
    n = C.c_uint64(0)
    assert lib.sdsp_hip_arb_state_bytes(p, 2, C.byref(n)) == 0 and n.value == 2 * 15 * 4
    # the resampling kernel, and one launch for the new history when T > 1
    assert b.launches(64) == 2 and b.launches(0) == 0
    b.time = 64 << 32
    assert b.launches(64) == 1  # no output, the history still moves
    assert _bank(sd, np.ones(4), 4, 1, ONE, "f32", False, "linear").launches(64) == 1
    info = b.info()
    assert (info["phases"], info["taps"], info["hist"], info["max_step"]) == (4, 16, 15, 2 * ONE)
    assert info["kernel"] == "sdsp_arb_kernel" and info["block_out"] == 1024
    assert info["input_kind"] == sd.ARB_REAL and info["interp"] == sd.ARB_LINEAR
    b.set_variant(1)
    assert b.info()["kernel"] == "sdsp_arb_plain_kernel"


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    """one call is one straight chain, the resampling kernel and then the history kernel: no parallel branches"""
    torch = torch_cuda
    rng = np.random.default_rng(28)
    L, T, S, step = 32, 16, 40000, step_of(0.7317)
    h = rng.standard_normal(L * T)
    x = _rand(rng, (3, S), "f32", False)
    want = _bank(sd, h, L, T, step, "f32", False, "linear").process(_dev(torch, x)).cpu().numpy()
    b = _bank(sd, h, L, T, step, "f32", False, "linear")
    xd = _dev(torch, x)
    out = torch.empty((3, want.shape[1]), dtype=torch.float32, device="cuda")
    b.process(xd, out=out)  # plan + state exist before capture
    b.reset()
    b._state = torch.zeros((3, T - 1), device="cuda")
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
    assert _same(b._state.cpu().numpy(), x[:, ::-1][:, :T - 1])
