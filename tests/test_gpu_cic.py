"""GPU tests of the CIC decimator bank (sdsp_hip_cic_*) on a real MI355X.

The checker is tests/cic_ref.py, the contract in numpy, itself pinned to the serial Hogenauer form and to the big-integer FIR form
in tests/test_cic_host.py.  Every comparison is bit for bit: both input types, both kinds, both register widths, both output kinds,
both kernel variants and every segment length, output and carried history alike."""
import ctypes as C

import numpy as np
import pytest

import arena
from cic_ref import cic_ref, growth, out_samples, reg_bits, stream_ref

pytestmark = pytest.mark.gpu

CHANNELS = 3
GRID = [(1, 2, 1), (3, 5, 1), (4, 16, 2), (8, 3, 2), (6, 64, 1)]


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


@pytest.fixture(scope="module")
def chunk(sd, torch_cuda):
    return sd.cic_decimator(3, 5).info()["chunk"]


def _np_dtype(in_dtype):
    return np.int32 if in_dtype == "i32" else np.int16


def _rand(rng, shape, bits, in_dtype):
    """samples of `bits` significant bits: noise on a large DC offset, so that the integrators wrap many times"""
    top = 1 << (bits - 1)
    dc = (5 * top) // 8
    noise = rng.integers(-(top // 4), top // 4 + 1, shape)
    return (dc + noise).astype(_np_dtype(in_dtype))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, variant=0, segment=0, state=None, position=0):
    b = sd.cic_decimator(N, R, M, "complex" if cplx else "real", in_dtype, in_bits, out)
    b.set_variant(variant)
    b.set_segment(segment)
    b.position = position
    if state is not None:
        b._state = _dev(torch, state)
    return b


def _in_bits(in_dtype, N, R, M):
    """the widest samples the 64-bit registers hold"""
    return min(32 if in_dtype == "i32" else 16, 64 - growth(N, R, M))


def _check_all_forms(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, x, state, position, sample_bits=None):
    """the fused kernel with automatic segments, with segments of one and of two chunks, and the plain kernel: output and final
    history equal to the reference's, bit for bit"""
    W = reg_bits(in_bits, N, R, M)
    want, want_state = cic_ref(x, N, R, M, W, position, state, out)
    assert want.shape[1] == out_samples(R, position, x.shape[1])
    xd = _dev(torch, x)
    for variant, segment in ((0, 0), (0, 1), (0, 2), (1, 0)):
        b = _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, variant, segment, state, position)
        info = b.info()
        assert (info["reg_bits"], info["hist"], info["growth"]) == (W, N * M * R, growth(N, R, M))
        assert info["kernel"] == ("sdsp_cic_plain_kernel" if variant else "sdsp_cic_kernel") and info["segment"] == segment
        assert b.launches(x.shape[1]) == (2 if want.shape[1] else 1)
        got = b.process(xd).cpu().numpy()
        tag = (N, R, M, cplx, in_dtype, in_bits, out, "variant", variant, "segment", segment)
        assert _same(got, want), (tag, int((got != want).sum()), "of", want.size)
        assert _same(b.state.cpu().numpy(), want_state), tag
        assert b.position == position + x.shape[1]
    return want


def _case(sd, torch, rng, chunk, N, R, M, cplx, in_dtype, in_bits, out, S=None):
    S = 5 * chunk + 37 if S is None else S
    tail = (2,) if cplx else ()
    x = _rand(rng, (CHANNELS, S) + tail, in_bits, in_dtype)
    state = _rand(rng, (CHANNELS, N * M * R) + tail, in_bits, in_dtype)
    return _check_all_forms(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, x, state, position=R + 3)


@pytest.mark.parametrize("N,R,M", GRID)
def test_bit_exact_against_reference(sd, torch_cuda, chunk, N, R, M):
    """rows of 5 chunks + 37 samples, three channels with a random history, a position off the decimation grid: I16 and I32, real
    and complex, integer and float output, at the widest in_bits the registers hold.  With segments of 1 and 2 chunks a row spans
    several workgroups, and every workgroup's warm-up and several passes"""
    rng = np.random.default_rng(N * 7919 + R)
    for in_dtype in ("i16", "i32"):
        for cplx in (False, True):
            for out in ("int", "f32"):
                _case(sd, torch_cuda, rng, chunk, N, R, M, cplx, in_dtype, _in_bits(in_dtype, N, R, M), out)


def test_both_register_widths_from_both_input_types(sd, torch_cuda, chunk):
    """W = 32 from I16 and from I32 rows, and W = 64 one bit above the boundary"""
    rng = np.random.default_rng(3)
    assert reg_bits(16, 3, 5, 1) == 32 and reg_bits(25, 3, 5, 1) == 32 and reg_bits(26, 3, 5, 1) == 64 and reg_bits(16, 4, 16, 2) == 64
    for cplx in (False, True):
        _case(sd, torch_cuda, rng, chunk, 3, 5, 1, cplx, "i16", 16, "int")
        _case(sd, torch_cuda, rng, chunk, 3, 5, 1, cplx, "i32", 25, "f32")
        _case(sd, torch_cuda, rng, chunk, 3, 5, 1, cplx, "i32", 26, "int")
        _case(sd, torch_cuda, rng, chunk, 4, 16, 2, cplx, "i16", 16, "f32")


def test_decimation_longer_than_a_chunk(sd, torch_cuda, chunk):
    """R > chunk: most passes hold no due sample"""
    rng = np.random.default_rng(4)
    R = chunk + 453
    assert 2 * R <= 65536
    for in_dtype, cplx, out in (("i16", False, "int"), ("i32", True, "int"), ("i16", True, "f32")):
        want = _case(sd, torch_cuda, rng, chunk, 2, R, 1, cplx, in_dtype, _in_bits(in_dtype, 2, R, 1), out)
        assert want.shape[1] == (R + 3 + 5 * chunk + 37) // R - 1 >= 3


def test_samples_wider_than_in_bits_wrap_like_the_reference(sd, torch_cuda, chunk):
    """full 32-bit samples declared as 8 bits in 32-bit registers, and full 16-bit samples declared as 4 bits at 4 + 60 = 64: the
    final outputs wrap, and equal the reference all the same"""
    rng = np.random.default_rng(5)
    S = 5 * chunk + 37
    x = rng.integers(-(1 << 31), 1 << 31, (CHANNELS, S)).astype(np.int32)
    st = rng.integers(-(1 << 31), 1 << 31, (CHANNELS, 4 * 2 * 16)).astype(np.int32)
    want = _check_all_forms(sd, torch_cuda, 4, 16, 2, False, "i32", 8, "int", x, st, 9)
    wide = cic_ref(x, 4, 16, 2, 64, 9, st)[0]  # what registers wide enough give: the 32-bit outputs are its low words, wrapped
    assert want.dtype == np.int32 and np.array_equal(wide.astype(np.int32), want) and not np.array_equal(wide, want.astype(np.int64))
    x = rng.integers(-(1 << 15), 1 << 15, (CHANNELS, 20000, 2)).astype(np.int16)
    st = rng.integers(-(1 << 15), 1 << 15, (CHANNELS, 6144, 2)).astype(np.int16)
    _check_all_forms(sd, torch_cuda, 6, 1024, 1, True, "i16", 4, "int", x, st, 1000)


def test_complex_is_two_real_planes(sd, torch_cuda, chunk):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    N, R, M = 4, 16, 2
    x = _rand(rng, (CHANNELS, 3 * chunk + 11, 2), 16, "i16")
    st = _rand(rng, (CHANNELS, N * M * R, 2), 16, "i16")
    y = _bank(sd, torch, N, R, M, True, "i16", 16, "int", state=st, position=5).process(_dev(torch, x)).cpu().numpy()
    for p in range(2):
        b = _bank(sd, torch, N, R, M, False, "i16", 16, "int", state=np.ascontiguousarray(st[..., p]), position=5)
        assert _same(b.process(_dev(torch, x[..., p])).cpu().numpy(), np.ascontiguousarray(y[..., p]))


def _stream(torch, b, x, blocks):
    parts, s0 = [], 0
    for n in blocks:
        parts.append(b.process(_dev(torch, x[:, s0:s0 + n])).cpu().numpy())
        s0 += n
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("N,R,M,cplx,in_dtype", [(3, 5, 1, False, "i16"), (4, 16, 2, True, "i32"), (6, 64, 1, True, "i16")])
def test_any_split_of_a_stream_gives_the_same_bits(sd, torch_cuda, chunk, N, R, M, cplx, in_dtype):
    """calls of 0, 1, R - 1, R + 1, hist - 1, hist, hist + 1 samples and the rest with the state buffer carried: the output and the
    final state of one call, with both kernels"""
    torch = torch_cuda
    rng = np.random.default_rng(7 + N)
    hist = N * M * R
    blocks = [0, 1, R - 1, R + 1, hist - 1, hist, hist + 1]
    blocks.append(2 * chunk + 5)
    S = sum(blocks)
    in_bits = _in_bits(in_dtype, N, R, M)
    tail = (2,) if cplx else ()
    x = _rand(rng, (CHANNELS, S) + tail, in_bits, in_dtype)
    st = _rand(rng, (CHANNELS, hist) + tail, in_bits, in_dtype)
    W = reg_bits(in_bits, N, R, M)
    want, want_state = cic_ref(x, N, R, M, W, 2, st)
    ref_stream, ref_state = stream_ref(x, blocks, N, R, M, W, 2, st)
    assert _same(ref_stream, want) and _same(ref_state, want_state)
    for variant in (0, 1):
        one = _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, "int", variant, state=st, position=2)
        assert _same(one.process(_dev(torch, x)).cpu().numpy(), want)
        many = _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, "int", variant, segment=1, state=st, position=2)
        assert _same(_stream(torch, many, x, blocks), want), variant
        assert _same(many.state.cpu().numpy(), want_state) and _same(one.state.cpu().numpy(), want_state)
        assert many.position == one.position == 2 + S


@pytest.mark.parametrize("in_dtype,cplx", [("i16", False), ("i16", True), ("i32", False), ("i32", True)])
def test_state_after_a_call_is_the_newest_history(sd, torch_cuda, in_dtype, cplx):
    """S below, at and above hist, also with no output: state[c hist + j] = x_c[-1 - j] over the old history and the block; I16
    real rows are the 2-byte carry"""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    N, R, M = 3, 700, 1
    hist = N * M * R
    tail = (2,) if cplx else ()
    for S in (1, 699, hist - 1, hist, hist + 1, 3 * hist + 5):
        x = _rand(rng, (CHANNELS, S) + tail, 16, in_dtype)
        st = _rand(rng, (CHANNELS, hist) + tail, 16, in_dtype)
        b = _bank(sd, torch, N, R, M, cplx, in_dtype, 16, "int", state=st)
        y = b.process(_dev(torch, x))
        assert y.shape[1] == S // R
        full = np.concatenate([st[:, ::-1], x], axis=1)
        assert _same(b.state.cpu().numpy(), full[:, ::-1][:, :hist]), S
        assert _same(y.cpu().numpy(), cic_ref(x, N, R, M, 64, 0, st)[0])


def _raw_call(sd, torch, plan, xd, in_stride, out, out_stride, channels, samples, position, state):
    from simpledsp_amd import _lib as L
    L.check(sd.load().sdsp_hip_cic_process(plan, xd.data_ptr(), in_stride, out.data_ptr(), out_stride, channels, samples, position,
                                           None if state is None else state.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def test_null_state_is_zero_history_and_position_counts_mod_R(sd, torch_cuda, chunk):
    torch = torch_cuda
    rng = np.random.default_rng(9)
    N, R, M = 4, 16, 2
    S = 2 * chunk + 9
    x = _rand(rng, (CHANNELS, S), 16, "i16")
    xd = _dev(torch, x)
    b = _bank(sd, torch, N, R, M, False, "i16", 16, "int")
    b._ensure_plan()
    for position in (0, 7, (1 << 40) + 3):
        want, _ = cic_ref(x, N, R, M, 64, position % R)
        n = want.shape[1]
        assert n == out_samples(R, position, S)
        out = torch.zeros((CHANNELS, n), dtype=torch.int64, device="cuda")
        _raw_call(sd, torch, b._plan, xd, S, out, n, CHANNELS, S, position, None)
        assert _same(out.cpu().numpy(), want), position
        zeros = torch.zeros((CHANNELS, N * M * R), dtype=torch.int16, device="cuda")
        out2 = torch.zeros_like(out)
        _raw_call(sd, torch, b._plan, xd, S, out2, n, CHANNELS, S, position, zeros)
        assert _same(out2.cpu().numpy(), want)
        assert _same(zeros.cpu().numpy(), x[:, ::-1][:, :N * M * R])
    assert _same(xd.cpu().numpy(), x)


@pytest.mark.parametrize("in_dtype,cplx,out", [("i16", False, "int"), ("i32", True, "f32"), ("i16", True, "int")])
def test_padded_strides_and_offset_pointers(sd, torch_cuda, chunk, in_dtype, cplx, out):
    """rows inside larger buffers, pointers 1 and 3 elements off a 512-byte boundary, strides longer than the rows: the same bits,
    `in` and its frame unchanged, the canaries past n_out, between the rows and around the output intact; both kernels"""
    torch = torch_cuda
    rng = np.random.default_rng(10)
    N, R, M = 3, 5, 1
    width = 2 if cplx else 1
    S = 3 * chunk + 37
    in_bits = 16 if in_dtype == "i16" else 24
    W = reg_bits(in_bits, N, R, M)
    tail = (2,) if cplx else ()
    x = _rand(rng, (CHANNELS, S) + tail, in_bits, in_dtype)
    st = _rand(rng, (CHANNELS, N * M * R) + tail, in_bits, in_dtype)
    position = 4
    want, want_state = cic_ref(x, N, R, M, W, position, st, out)
    n = want.shape[1]
    tdt = torch.int32 if in_dtype == "i32" else torch.int16
    odt = {"f32": torch.float32}.get(out, torch.int64 if W == 64 else torch.int32)
    in_stride, out_stride = S + 13, n + 7
    for variant in (0, 1):
        b = _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, variant, segment=1)
        b._ensure_plan()
        for lead in (1, 3):
            for fill_in, fill_out in ((-1, 7), (0x5a5a, -3)):
                # scalars: a complex row is 2 S scalars in a stride of 2 in_stride
                ain, vin = arena.framed(torch, (CHANNELS, S * width), tdt, lead * width, 64, fill_in, in_stride * width)
                vin[:, :S * width].copy_(_dev(torch, x.reshape(CHANNELS, S * width)))
                aout, vout = arena.framed(torch, (CHANNELS, n * width), odt, lead * width, 64, fill_out, out_stride * width)
                in_before, out_before = ain.clone(), arena.bits(aout).clone()
                state = _dev(torch, st)
                _raw_call(sd, torch, b._plan, vin, in_stride, vout, out_stride, CHANNELS, S, position, state)
                tag = (variant, lead, fill_in)
                assert torch.equal(ain, in_before), tag
                arena.assert_frame_untouched(out_before, aout, arena.interior_mask(torch, aout, vout, n * width))
                got = vout[:, :n * width].cpu().numpy().reshape(want.shape)
                assert _same(got, want), tag
                assert _same(state.cpu().numpy(), want_state), tag


def test_graph_capture_replays_the_eager_result(sd, torch_cuda, chunk):
    """one call is one straight chain, the decimating kernel and then the history kernel: no parallel branches"""
    torch = torch_cuda
    rng = np.random.default_rng(11)
    N, R, M = 4, 16, 2
    S = 4 * chunk + 21
    x = _rand(rng, (CHANNELS, S, 2), 16, "i16")
    st = _rand(rng, (CHANNELS, N * M * R, 2), 16, "i16")
    want, want_state = cic_ref(x, N, R, M, 64, 6, st)
    b = _bank(sd, torch, N, R, M, True, "i16", 16, "int", state=st, position=6)
    xd = _dev(torch, x)
    out = torch.empty((CHANNELS, want.shape[1], 2), dtype=torch.int64, device="cuda")
    b.process(xd, out=out)  # plan + state exist before capture
    assert _same(out.cpu().numpy(), want)
    b.position = 6
    b.state.copy_(_dev(torch, st))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.process(xd, out=out)
    b.state.copy_(_dev(torch, st))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), want)
    assert _same(b.state.cpu().numpy(), want_state)


def test_process_argument_errors(sd, torch_cuda):
    """null pointers, short strides and overlapping ranges are refused before anything is launched"""
    torch = torch_cuda
    from simpledsp_amd import _lib as L
    lib = sd.load()
    b = sd.cic_decimator(3, 5)
    b._ensure_plan()
    x = torch.zeros((2, 100), dtype=torch.int16, device="cuda")
    y = torch.zeros((2, 20), dtype=torch.int32, device="cuda")
    call = lambda *a: lib.sdsp_hip_cic_process(*a, None, None)  # noqa: E731
    assert call(None, x.data_ptr(), 100, y.data_ptr(), 20, 2, 100, 0) == L.ERR_INVALID_ARG
    assert call(b._plan, None, 100, y.data_ptr(), 20, 2, 100, 0) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 100, None, 20, 2, 100, 0) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 99, y.data_ptr(), 20, 2, 100, 0) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 100, y.data_ptr(), 19, 2, 100, 0) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 100, x.data_ptr(), 20, 2, 100, 0) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr() + 1, 100, y.data_ptr(), 20, 1, 50, 0) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 100, y.data_ptr() + 2, 20, 1, 50, 0) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 1 << 31, y.data_ptr(), 20, 1, 1 << 31, 0) == L.ERR_INVALID_SIZE
    assert call(b._plan, x.data_ptr(), 100, y.data_ptr(), 20, 0, 100, 0) == 0
    assert call(b._plan, x.data_ptr(), 100, y.data_ptr(), 20, 2, 0, 0) == 0
    n = C.c_uint64(0)
    assert lib.sdsp_hip_cic_state_bytes(b._plan, 3, C.byref(n)) == 0 and n.value == 3 * 15 * 2
    torch.cuda.synchronize()
    assert not bool(y.any())
