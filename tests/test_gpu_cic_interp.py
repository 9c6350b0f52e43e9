"""GPU tests of the CIC interpolator bank (sdsp_hip_cic_interp_*) on a real MI355X.

The checker is tests/cic_interp_ref.py, the contract in numpy, itself pinned to the serial Hogenauer form and to the big-integer
FIR form in tests/test_cic_interp_host.py.  Every comparison is bit for bit: both input types, both kinds, both register widths,
both output kinds, both kernel variants and every segment length, output and carried history alike."""
import ctypes as C

import numpy as np
import pytest

import arena
from cic_interp_ref import cic_interp_ref, gain, growth, reg_bits, stream_ref

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
    return sd.cic_interpolator(3, 5).info()["chunk"]


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


def _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, variant=0, segment=0, state=None):
    b = sd.cic_interpolator(N, R, M, "complex" if cplx else "real", in_dtype, in_bits, out)
    b.set_variant(variant)
    b.set_segment(segment)
    if state is not None:
        b._state = _dev(torch, state)
    return b


def _in_bits(in_dtype, N, R, M):
    """the widest samples the 64-bit registers hold"""
    return min(32 if in_dtype == "i32" else 16, 64 - growth(N, R, M))


def _inputs(chunk, R, chunks=5, extra=37):
    """inputs per row for about `chunks` chunks + `extra` outputs"""
    return -(-(chunks * chunk + extra) // R)


def _check_all_forms(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, x, state):
    """the scan kernel with automatic segments, with segments of one and of two chunks, and the plain kernel: output and final
    history equal to the reference's, bit for bit"""
    W = reg_bits(in_bits, N, R, M)
    want, want_state = cic_interp_ref(x, N, R, M, W, state, out)
    assert want.shape[1] == R * x.shape[1]
    xd = _dev(torch, x)
    for variant, segment in ((0, 0), (0, 1), (0, 2), (1, 0)):
        b = _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, variant, segment, state)
        info = b.info()
        assert (info["reg_bits"], info["hist"], info["growth"], info["up"]) == (W, N * M, growth(N, R, M), R)
        assert info["kernel"] == ("sdsp_cic_interp_plain_kernel" if variant else "sdsp_cic_interp_kernel") and info["segment"] == segment
        assert b.launches(x.shape[1]) == 2 and b.launches(0) == 0
        got = b.process(xd).cpu().numpy()
        tag = (N, R, M, cplx, in_dtype, in_bits, out, "variant", variant, "segment", segment)
        assert _same(got, want), (tag, int((got != want).sum()), "of", want.size)
        assert _same(b.state.cpu().numpy(), want_state), tag
    return want


def _case(sd, torch, rng, chunk, N, R, M, cplx, in_dtype, in_bits, out, S=None, sample_bits=None):
    S = _inputs(chunk, R) if S is None else S
    tail = (2,) if cplx else ()
    bits = in_bits if sample_bits is None else sample_bits
    x = _rand(rng, (CHANNELS, S) + tail, bits, in_dtype)
    state = _rand(rng, (CHANNELS, N * M) + tail, bits, in_dtype)
    return _check_all_forms(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, x, state)


@pytest.mark.parametrize("N,R,M", GRID)
def test_bit_exact_against_reference(sd, torch_cuda, chunk, N, R, M):
    """rows of about 5 chunks + 37 outputs, three channels with a random history: I16 and I32, real and complex, integer and float
    output, at the widest in_bits the registers hold.  With segments of 1 and 2 chunks a row spans several workgroups, and every
    workgroup's warm-up and several passes.  At I16, (4, 16, 2) is exactly W = 32 and (6, 64, 1) is W = 64"""
    rng = np.random.default_rng(N * 7919 + R)
    assert reg_bits(16, 4, 16, 2) == 32 and 16 + growth(4, 16, 2) == 32 and reg_bits(16, 6, 64, 1) == 64
    for in_dtype in ("i16", "i32"):
        for cplx in (False, True):
            for out in ("int", "f32"):
                _case(sd, torch_cuda, rng, chunk, N, R, M, cplx, in_dtype, _in_bits(in_dtype, N, R, M), out)


def test_a_row_shorter_than_one_chunk(sd, torch_cuda, chunk):
    rng = np.random.default_rng(2)
    for N, R, M, S in ((3, 5, 1, 1), (3, 5, 1, 2), (4, 16, 2, 7), (1, 2, 1, 100), (8, 3, 2, chunk // 3 - 1)):
        assert R * S < chunk
        for cplx in (False, True):
            _case(sd, torch_cuda, rng, chunk, N, R, M, cplx, "i16", 16, "int", S=S)
            _case(sd, torch_cuda, rng, chunk, N, R, M, cplx, "i32", _in_bits("i32", N, R, M), "f32", S=S)


def test_up_sampling_longer_than_a_chunk(sd, torch_cuda, chunk):
    """R > chunk: a pass holds one input boundary or none"""
    rng = np.random.default_rng(4)
    assert 4096 > chunk
    for in_dtype, cplx, out in (("i16", False, "int"), ("i32", True, "int"), ("i16", True, "f32")):
        _case(sd, torch_cuda, rng, chunk, 2, 4096, 1, cplx, in_dtype, _in_bits(in_dtype, 2, 4096, 1), out, S=3)
        _case(sd, torch_cuda, rng, chunk, 2, 16384, 2, cplx, in_dtype, _in_bits(in_dtype, 2, 16384, 2), out, S=2)


def test_samples_wider_than_in_bits_wrap_like_the_reference(sd, torch_cuda, chunk):
    """full 32-bit samples declared as 8 bits in 32-bit registers, and full 16-bit samples declared as 4 bits at 4 + 60 = 64: the
    final outputs wrap, and equal the reference all the same"""
    rng = np.random.default_rng(5)
    S = _inputs(chunk, 16)
    x = rng.integers(-(1 << 31), 1 << 31, (CHANNELS, S)).astype(np.int32)
    st = rng.integers(-(1 << 31), 1 << 31, (CHANNELS, 4 * 2)).astype(np.int32)
    want = _check_all_forms(sd, torch_cuda, 4, 16, 2, False, "i32", 8, "int", x, st)
    wide = cic_interp_ref(x, 4, 16, 2, 64, st)[0]  # what registers wide enough give: the 32-bit outputs are its low words, wrapped
    assert want.dtype == np.int32 and np.array_equal(wide.astype(np.int32), want) and not np.array_equal(wide, want.astype(np.int64))
    assert growth(7, 1024, 1) == 60
    x = rng.integers(-(1 << 15), 1 << 15, (CHANNELS, 11, 2)).astype(np.int16)
    st = rng.integers(-(1 << 15), 1 << 15, (CHANNELS, 7, 2)).astype(np.int16)
    _check_all_forms(sd, torch_cuda, 7, 1024, 1, True, "i16", 4, "int", x, st)


def test_complex_is_two_real_planes(sd, torch_cuda, chunk):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    N, R, M = 4, 16, 2
    x = _rand(rng, (CHANNELS, _inputs(chunk, R, 3, 11), 2), 16, "i16")
    st = _rand(rng, (CHANNELS, N * M, 2), 16, "i16")
    y = _bank(sd, torch, N, R, M, True, "i16", 16, "int", state=st).process(_dev(torch, x)).cpu().numpy()
    for p in range(2):
        b = _bank(sd, torch, N, R, M, False, "i16", 16, "int", state=np.ascontiguousarray(st[..., p]))
        assert _same(b.process(_dev(torch, x[..., p])).cpu().numpy(), np.ascontiguousarray(y[..., p]))


@pytest.mark.parametrize("N,R,M,in_dtype", [(1, 2, 1, "i16"), (3, 5, 1, "i16"), (4, 16, 2, "i16"), (6, 64, 1, "i32"), (2, 4096, 1, "i32")])
def test_a_constant_input_settles_to_the_dc_gain(sd, torch_cuda, chunk, N, R, M, in_dtype):
    """c in, c R^(N-1) M^N out at every phase once the N M inputs of history are c, and at once with a history of c"""
    torch = torch_cuda
    in_bits = _in_bits(in_dtype, N, R, M)
    c = -(1 << (in_bits - 1))  # the constant minimum reaches the growth bound
    S = max(_inputs(chunk, R, 2, 5), N * M + 2)
    x = np.full((CHANNELS, S), c, dtype=_np_dtype(in_dtype))
    for variant in (0, 1):
        y = _bank(sd, torch, N, R, M, False, in_dtype, in_bits, "int", variant, segment=1).process(_dev(torch, x)).cpu().numpy()
        assert (y[:, N * M * R:] == c * gain(N, R, M)).all()
        b = _bank(sd, torch, N, R, M, False, in_dtype, in_bits, "f32", variant, state=x[:, :N * M])
        f = b.process(_dev(torch, x)).cpu().numpy()
        assert f.dtype == np.float32 and (f == np.float32(c)).all()  # unity scale: a power of two or exact all the same here


def _stream(torch, b, x, blocks):
    parts, s0 = [], 0
    for n in blocks:
        parts.append(b.process(_dev(torch, x[:, s0:s0 + n])).cpu().numpy())
        s0 += n
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("N,R,M,cplx,in_dtype", [(3, 5, 1, False, "i16"), (4, 16, 2, True, "i32"), (6, 64, 1, True, "i16")])
def test_any_split_of_a_stream_gives_the_same_bits(sd, torch_cuda, chunk, N, R, M, cplx, in_dtype):
    """calls of 0, 1, 2, hist - 1, hist, hist + 1 samples and the rest with the state buffer carried: the output and the final
    state of one call, with both kernels"""
    torch = torch_cuda
    rng = np.random.default_rng(7 + N)
    hist = N * M
    blocks = [0, 1, 2, hist - 1, hist, hist + 1, 1, 0]
    blocks.append(_inputs(chunk, R, 2, 5))
    S = sum(blocks)
    in_bits = _in_bits(in_dtype, N, R, M)
    tail = (2,) if cplx else ()
    x = _rand(rng, (CHANNELS, S) + tail, in_bits, in_dtype)
    st = _rand(rng, (CHANNELS, hist) + tail, in_bits, in_dtype)
    W = reg_bits(in_bits, N, R, M)
    want, want_state = cic_interp_ref(x, N, R, M, W, st)
    ref_stream, ref_state = stream_ref(x, blocks, N, R, M, W, st)
    assert _same(ref_stream, want) and _same(ref_state, want_state)
    for variant in (0, 1):
        one = _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, "int", variant, state=st)
        assert _same(one.process(_dev(torch, x)).cpu().numpy(), want)
        many = _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, "int", variant, segment=1, state=st)
        assert _same(_stream(torch, many, x, blocks), want), variant
        assert _same(many.state.cpu().numpy(), want_state) and _same(one.state.cpu().numpy(), want_state)


@pytest.mark.parametrize("in_dtype,cplx", [("i16", False), ("i16", True), ("i32", False), ("i32", True)])
def test_state_after_a_call_is_the_newest_history(sd, torch_cuda, in_dtype, cplx):
    """S below, at and above hist: state[c hist + j] = x_c[-1 - j] over the old history and the block; I16 real rows are the 2-byte
    carry"""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    N, R, M = 8, 3, 2
    hist = N * M
    tail = (2,) if cplx else ()
    for S in (1, 2, hist - 1, hist, hist + 1, 3 * hist + 5):
        x = _rand(rng, (CHANNELS, S) + tail, 16, in_dtype)
        st = _rand(rng, (CHANNELS, hist) + tail, 16, in_dtype)
        b = _bank(sd, torch, N, R, M, cplx, in_dtype, 16, "int", state=st)
        y = b.process(_dev(torch, x))
        assert y.shape[1] == S * R
        full = np.concatenate([st[:, ::-1], x], axis=1)
        assert _same(b.state.cpu().numpy(), full[:, ::-1][:, :hist]), S
        assert _same(y.cpu().numpy(), cic_interp_ref(x, N, R, M, 64, st)[0])


def _raw_call(sd, torch, plan, xd, in_stride, out, out_stride, channels, samples, state):
    from simpledsp_amd import _lib as L
    L.check(sd.load().sdsp_hip_cic_interp_process(plan, xd.data_ptr(), in_stride, out.data_ptr(), out_stride, channels, samples,
                                                  None if state is None else state.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def test_null_state_is_zero_history(sd, torch_cuda, chunk):
    torch = torch_cuda
    rng = np.random.default_rng(9)
    N, R, M = 4, 16, 2
    S = _inputs(chunk, R, 2, 9)
    x = _rand(rng, (CHANNELS, S), 16, "i16")
    xd = _dev(torch, x)
    want, _ = cic_interp_ref(x, N, R, M, 32)
    n = want.shape[1]
    for variant in (0, 1):
        b = _bank(sd, torch, N, R, M, False, "i16", 16, "int", variant)
        b._ensure_plan()
        out = torch.zeros((CHANNELS, n), dtype=torch.int32, device="cuda")
        _raw_call(sd, torch, b._plan, xd, S, out, n, CHANNELS, S, None)
        assert _same(out.cpu().numpy(), want), variant
        zeros = torch.zeros((CHANNELS, N * M), dtype=torch.int16, device="cuda")
        out2 = torch.zeros_like(out)
        _raw_call(sd, torch, b._plan, xd, S, out2, n, CHANNELS, S, zeros)
        assert _same(out2.cpu().numpy(), want)
        assert _same(zeros.cpu().numpy(), x[:, ::-1][:, :N * M])
    assert _same(xd.cpu().numpy(), x)


@pytest.mark.parametrize("in_dtype,cplx,out,N,R,M", [("i16", False, "int", 3, 5, 1), ("i32", True, "f32", 3, 5, 1), ("i16", True, "int", 3, 5, 1),
                                                     ("i16", False, "int", 6, 64, 1), ("i32", True, "int", 4, 16, 2),
                                                     ("i16", False, "f32", 1, 2, 1)])
def test_padded_strides_and_offset_pointers(sd, torch_cuda, chunk, in_dtype, cplx, out, N, R, M):
    """rows inside larger buffers, pointers 1 and 3 elements off a 512-byte boundary, an odd out_stride longer than the rows, so
    that the 16-byte alignment of the stores differs from row to row: the same bits, `in` and its frame unchanged, the canaries
    past the outputs, between the rows and around the output intact; both kernels"""
    torch = torch_cuda
    rng = np.random.default_rng(10)
    width = 2 if cplx else 1
    S = _inputs(chunk, R, 3, 37)
    in_bits = min(16 if in_dtype == "i16" else 24, 64 - growth(N, R, M))
    W = reg_bits(in_bits, N, R, M)
    tail = (2,) if cplx else ()
    x = _rand(rng, (CHANNELS, S) + tail, in_bits, in_dtype)
    st = _rand(rng, (CHANNELS, N * M) + tail, in_bits, in_dtype)
    want, want_state = cic_interp_ref(x, N, R, M, W, st, out)
    n = want.shape[1]
    tdt = torch.int32 if in_dtype == "i32" else torch.int16
    odt = {"f32": torch.float32}.get(out, torch.int64 if W == 64 else torch.int32)
    in_stride, out_stride = S + 13, (n + 7) | 1
    for variant, segment in ((0, 1), (0, 0), (1, 0)):
        b = _bank(sd, torch, N, R, M, cplx, in_dtype, in_bits, out, variant, segment)
        b._ensure_plan()
        for lead in (1, 3):
            for fill_in, fill_out in ((-1, 7), (0x5a5a, -3)):
                # scalars: a complex row is 2 S scalars in a stride of 2 in_stride
                ain, vin = arena.framed(torch, (CHANNELS, S * width), tdt, lead * width, 64, fill_in, in_stride * width)
                vin[:, :S * width].copy_(_dev(torch, x.reshape(CHANNELS, S * width)))
                aout, vout = arena.framed(torch, (CHANNELS, n * width), odt, lead * width, 64, fill_out, out_stride * width)
                in_before, out_before = ain.clone(), arena.bits(aout).clone()
                state = _dev(torch, st)
                _raw_call(sd, torch, b._plan, vin, in_stride, vout, out_stride, CHANNELS, S, state)
                tag = (variant, segment, lead, fill_in)
                assert torch.equal(ain, in_before), tag
                arena.assert_frame_untouched(out_before, aout, arena.interior_mask(torch, aout, vout, n * width))
                got = vout[:, :n * width].cpu().numpy().reshape(want.shape)
                assert _same(got, want), tag
                assert _same(state.cpu().numpy(), want_state), tag


def test_graph_capture_replays_the_eager_result(sd, torch_cuda, chunk):
    """one call is one straight chain, the interpolating kernel and then the history kernel: no parallel branches"""
    torch = torch_cuda
    rng = np.random.default_rng(11)
    N, R, M = 6, 64, 1
    S = _inputs(chunk, R, 4, 21)
    x = _rand(rng, (CHANNELS, S, 2), 16, "i16")
    st = _rand(rng, (CHANNELS, N * M, 2), 16, "i16")
    want, want_state = cic_interp_ref(x, N, R, M, 64, st)
    b = _bank(sd, torch, N, R, M, True, "i16", 16, "int", state=st)
    xd = _dev(torch, x)
    out = torch.empty((CHANNELS, want.shape[1], 2), dtype=torch.int64, device="cuda")
    b.process(xd, out=out)  # plan + state exist before capture
    assert _same(out.cpu().numpy(), want)
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
    b = sd.cic_interpolator(3, 5)
    b._ensure_plan()
    x = torch.zeros((2, 20), dtype=torch.int16, device="cuda")
    y = torch.zeros((2, 100), dtype=torch.int32, device="cuda")
    call = lambda *a: lib.sdsp_hip_cic_interp_process(*a, None, None)  # noqa: E731
    assert call(None, x.data_ptr(), 20, y.data_ptr(), 100, 2, 20) == L.ERR_INVALID_ARG
    assert call(b._plan, None, 20, y.data_ptr(), 100, 2, 20) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 20, None, 100, 2, 20) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 19, y.data_ptr(), 100, 2, 20) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 20, y.data_ptr(), 99, 2, 20) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 20, x.data_ptr(), 100, 2, 20) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr() + 1, 20, y.data_ptr(), 100, 1, 10) == L.ERR_INVALID_ARG
    assert call(b._plan, x.data_ptr(), 20, y.data_ptr() + 2, 100, 1, 10) == L.ERR_INVALID_ARG
    big = -(-(1 << 31) // 5)
    assert call(b._plan, x.data_ptr(), big, y.data_ptr(), 100, 1, big) == L.ERR_INVALID_SIZE  # 5 S >= 2^31
    assert call(b._plan, x.data_ptr(), 1 << 31, y.data_ptr(), 100, 1, 1 << 31) == L.ERR_INVALID_SIZE
    assert call(b._plan, x.data_ptr(), 20, y.data_ptr(), 100, 0, 20) == 0
    assert call(b._plan, x.data_ptr(), 20, y.data_ptr(), 100, 2, 0) == 0
    n = C.c_uint64(0)
    assert lib.sdsp_hip_cic_interp_state_bytes(b._plan, 3, C.byref(n)) == 0 and n.value == 3 * 3 * 2
    assert lib.sdsp_hip_cic_interp_plan_launches(b._plan, big, C.byref(n)) == L.ERR_INVALID_SIZE
    torch.cuda.synchronize()
    assert not bool(y.any())
