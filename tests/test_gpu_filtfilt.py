"""GPU tests of the forward-backward filtering plans (sdsp_hip_filtfilt_*) on a real MI355X.

Every case is held bit for bit to the composition a user writes with the library alone: pad in torch in the sample type, a state
buffer of R(s_j) R(e[0]) in sdsp_hip_iir_process's layout, process, flip, a second state from the last forward output, process,
flip, slice.  The values are also held to scipy.signal.sosfiltfilt, whose agreement with the double reference of
tests/filtfilt_ref.py is checked on the CPU in tests/test_filtfilt_host.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.signal

from filtfilt_ref import BP, GENERIC, HP, LP, default_padlen_ref, random_stable, sos_of

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


PRECISIONS = {"f32": 0, "f64": 1, "mix": 2}


def _dtypes(torch, precision):
    """(sample dtype, recurrence dtype)"""
    return (torch.float64 if precision == "f64" else torch.float32, torch.float32 if precision == "f32" else torch.float64)


def _design(sd, design, m, seed=0):
    """(kind, a, b, gain): the library's Butterworth designs, a band-stop and a random stable cascade on GENERIC plans"""
    lib = sd.load()
    a, b, g = np.zeros(3 * m), np.zeros(3 * m), C.c_double()
    if design == "lp":
        assert lib.sdsp_hip_iir_design_lp(m, 2e3, 48e3, 1.0, a.ctypes.data, b.ctypes.data, C.byref(g)) == 0
        return LP, a, None, g.value
    if design == "hp":
        assert lib.sdsp_hip_iir_design_hp(m, 2e3, 48e3, 1.0, a.ctypes.data, b.ctypes.data, C.byref(g)) == 0
        return HP, a, None, g.value
    if design == "bp":
        assert lib.sdsp_hip_iir_design_bp(m, 4e3, 48e3, 2.0, 1.0, a.ctypes.data, b.ctypes.data, C.byref(g)) == 0
        return BP, a, None, g.value
    if design == "bs":
        assert lib.sdsp_hip_iir_design_bs(m, 4e3, 48e3, 1.5, 1.0, a.ctypes.data, b.ctypes.data, C.byref(g)) == 0
        return GENERIC, a, b, g.value
    a, b, g = random_stable(np.random.default_rng(100 + m + seed), m)
    return GENERIC, a, b, g


def _composition(torch, sd, x, kind, a, b, gain, precision, padtype, padlen):
    """the result with the library's IIR bank alone (x: (channels, L) device tensor of the sample dtype; not modified)"""
    lib = sd.load()
    S, R = _dtypes(torch, precision)
    m = len(a) // 3
    Lx = x.shape[1]
    P = 0 if padtype is None else (default_padlen_ref(kind, a, b) if padlen is None else padlen)
    if P:
        x0, xl = x[:, :1], x[:, -1:]
        lm, rm = x[:, 1:P + 1].flip(1), x[:, Lx - 1 - P:Lx - 1].flip(1)
        if padtype == "odd":
            left, right = 2 * x0 - lm, 2 * xl - rm
        elif padtype == "even":
            left, right = lm, rm
        else:
            left, right = x0.expand(-1, P), xl.expand(-1, P)
        e = torch.cat([left, x, right], dim=1).contiguous()
    else:
        e = x.clone().contiguous()
    s = torch.from_numpy(sd.iir_steady_state(m, kind, a, b, gain)).to(device=x.device, dtype=R)
    plan = C.c_void_p()
    assert lib.sdsp_hip_iir_plan_create(C.byref(plan), m, kind, a.ctypes.data, None if b is None else b.ctypes.data, gain,
                                        PRECISIONS[precision], 0) == 0
    try:
        C_, N = e.shape
        st = (s[:, None] * e[:, 0].to(R)[None, :]).repeat_interleave(3, dim=0).contiguous()
        assert lib.sdsp_hip_iir_process(plan, e.data_ptr(), C_, N, N, st.data_ptr(), None) == 0
        u = e.flip(1).contiguous()
        st = (s[:, None] * u[:, 0].to(R)[None, :]).repeat_interleave(3, dim=0).contiguous()
        assert lib.sdsp_hip_iir_process(plan, u.data_ptr(), C_, N, N, st.data_ptr(), None) == 0
        torch.cuda.synchronize()
    finally:
        lib.sdsp_hip_iir_plan_destroy(plan)
    return u.flip(1)[:, P:P + Lx].contiguous()


def _plan(sd, kind, a, b, g, precision, padtype="odd", padlen=None, workspace_bytes=0):
    return sd.filtfilt_plan(len(a) // 3, kind, a, b, g, PRECISIONS[precision], padtype, padlen, 0, workspace_bytes)


FUSED, DIRECT = "sdsp_filtfilt_fused_kernel", "sdsp_filtfilt_direct_kernel"
SCIPY_TOL = {"f64": 1e-12, "mix": 1e-6, "f32": 1e-4}  # against scipy.signal.sosfiltfilt in double, relative to the largest value


def _scipy_err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def _expected_kernel(m, x, samples=None):
    """variant 0's choice: the fused kernel for up to 8 sections on 16-byte aligned rows (pointer and stride)"""
    aligned = x.data_ptr() % 16 == 0 and (x.shape[0] == 1 or x.shape[1] * x.element_size() % 16 == 0)
    return FUSED if m <= 8 and aligned else DIRECT


def _signal(torch, precision, channels, samples, seed=0, stride=None):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((channels, stride or samples)), axis=1) * 0.1 + rng.standard_normal((channels, 1))
    return torch.from_numpy(x).to(device="cuda", dtype=_dtypes(torch, precision)[0])


@pytest.mark.parametrize("precision", ["f32", "f64", "mix"])
@pytest.mark.parametrize("design", ["lp", "hp", "bp", "bs", "rand"])
@pytest.mark.parametrize("m", [2, 4, 8, 16])
@pytest.mark.parametrize("padtype", ["odd", "even", "constant", None])
@pytest.mark.parametrize("samples", [4100, 4097])  # 16-byte aligned rows (fused kernel up to 8 sections) and not (direct kernel)
def test_bit_exact_to_the_composition(torch_cuda, sd, precision, design, m, padtype, samples):
    torch = torch_cuda
    kind, a, b, g = _design(sd, design, m)
    x = _signal(torch, precision, 65, samples, seed=m)
    want = _composition(torch, sd, x, kind, a, b, g, precision, padtype, None)
    plan = _plan(sd, kind, a, b, g, precision, padtype)
    y = x.clone()
    assert plan.kernel_name(y) == _expected_kernel(m, y) == (FUSED if m <= 8 and samples == 4100 else DIRECT)
    got = plan.process(y)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("precision", ["f32", "f64", "mix"])
@pytest.mark.parametrize("shape", [(64, 4096), (65, 4097), (100, 1000), (1, 777), (1, 4096)])
@pytest.mark.parametrize("design,m", [("lp", 4), ("rand", 6), ("bs", 8), ("rand", 10)])
@pytest.mark.parametrize("padtype", ["odd", "even", "constant", None])
def test_shapes_bit_exact(torch_cuda, sd, precision, shape, design, m, padtype):
    torch = torch_cuda
    kind, a, b, g = _design(sd, design, m)
    x = _signal(torch, precision, *shape, seed=shape[1])
    want = _composition(torch, sd, x, kind, a, b, g, precision, padtype, None)
    plan = _plan(sd, kind, a, b, g, precision, padtype)
    y = x.clone()
    assert plan.kernel_name(y) == _expected_kernel(m, y)
    got = plan.process(y)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("precision", ["f32", "f64", "mix"])
@pytest.mark.parametrize("stride", [136, 131])  # 16-byte aligned rows (fused kernel) and not (direct kernel)
@pytest.mark.parametrize("L_", [130, 129])  # the last 16-byte vector of a row straddles L: f32 both, f64 129
def test_stride_rows_and_untouched_tail(torch_cuda, sd, precision, stride, L_):
    torch = torch_cuda
    kind, a, b, g = _design(sd, "lp", 4)
    x = _signal(torch, precision, 3, L_, seed=5, stride=stride)
    x[:, L_:] = -7.25
    want = _composition(torch, sd, x[:, :L_].contiguous(), kind, a, b, g, precision, "odd", None)
    plan = _plan(sd, kind, a, b, g, precision)
    assert plan.kernel_name(x, L_) == (FUSED if stride == 136 else DIRECT)
    plan.process(x, samples=L_)
    torch.cuda.synchronize()
    assert torch.equal(x[:, :L_], want)
    assert torch.all(x[:, L_:] == -7.25)


@pytest.mark.parametrize("precision", ["f32", "f64", "mix"])
@pytest.mark.parametrize("design", ["lp", "hp", "bp", "bs", "rand"])
def test_against_scipy(torch_cuda, sd, precision, design):
    torch = torch_cuda
    tol = SCIPY_TOL[precision]
    for m in (2, 4, 8, 16):
        kind, a, b, g = _design(sd, design, m)
        x = _signal(torch, precision, 8, 3000, seed=m)
        sos = sos_of(kind, a, b, g)
        for padtype in ["odd", "even", "constant", None]:
            want = scipy.signal.sosfiltfilt(sos, x.double().cpu().numpy(), padtype=padtype)
            got = _plan(sd, kind, a, b, g, precision, padtype).process(x.clone()).double().cpu().numpy()
            err = _scipy_err(got, want)
            assert err <= tol, (m, padtype, err)


@pytest.mark.parametrize("precision", ["f32", "f64", "mix"])
@pytest.mark.parametrize("m", [2, 8, 12])
def test_variants_and_misaligned_pointer_are_bit_identical(torch_cuda, sd, precision, m):
    torch = torch_cuda
    kind, a, b, g = _design(sd, "rand", m)
    C_, N = 130, 2052  # 16-byte aligned rows in both sample types, 2052 not a multiple of the 512-byte super-tile
    x = _signal(torch, precision, C_, N, seed=3)
    plan = _plan(sd, kind, a, b, g, precision)
    y0 = x.clone()
    assert plan.kernel_name(y0) == (FUSED if m <= 8 else DIRECT)
    v0 = plan.process(y0)
    plan.set_variant(1)
    y1 = x.clone()
    assert plan.kernel_name(y1) == DIRECT
    v1 = plan.process(y1)
    plan.set_variant(0)
    # the same rows one element off 16 bytes: variant 0 hands them to the direct kernel
    buf = torch.zeros((C_ * N + 1,), dtype=x.dtype, device=x.device)
    buf[1:] = x.reshape(-1)
    lib = sd.load()
    name = C.create_string_buffer(64)
    ptr = buf.data_ptr() + buf.element_size()
    assert lib.sdsp_hip_filtfilt_plan_kernel(plan._plan, ptr, C_, N, N, name, 64) == 0 and name.value.decode() == DIRECT
    assert lib.sdsp_hip_filtfilt_process(plan._plan, ptr, C_, N, N, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(v0, v1)
    assert torch.equal(buf[1:].reshape(C_, N), v0)
    with pytest.raises(sd.SdspHipError):
        plan.set_variant(2)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("padlen", [0, 1, 300, 1000, 1999])
def test_pad_lengths(torch_cuda, sd, precision, padlen):
    torch = torch_cuda
    kind, a, b, g = _design(sd, "lp", 4)
    x = _signal(torch, precision, 70, 2000, seed=padlen)
    for padtype in ["odd", "even", "constant"]:
        want = _composition(torch, sd, x, kind, a, b, g, precision, padtype, padlen)
        plan = _plan(sd, kind, a, b, g, precision, padtype, padlen)
        assert plan.padlen == padlen
        got = plan.process(x.clone())
        torch.cuda.synchronize()
        assert torch.equal(got, want), padtype
        if precision == "f64":
            ref = scipy.signal.sosfiltfilt(sos_of(kind, a, b, g), x.cpu().numpy(), padtype=padtype, padlen=padlen)
            assert np.abs(got.cpu().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


def test_length_not_above_padlen_is_refused(torch_cuda, sd):
    torch = torch_cuda
    kind, a, b, g = _design(sd, "lp", 4)
    plan = _plan(sd, kind, a, b, g, "f32", "odd", 100)
    x = _signal(torch, "f32", 2, 100)
    with pytest.raises(ValueError):
        plan.process(x)
    lib = sd.load()
    assert lib.sdsp_hip_filtfilt_process(plan._plan, x.data_ptr(), 2, 100, 100, None) == sd._lib.ERR_INVALID_SIZE
    n = C.c_uint64(9)
    assert lib.sdsp_hip_filtfilt_plan_launches(plan._plan, 2, 100, C.byref(n)) == sd._lib.ERR_INVALID_SIZE
    assert lib.sdsp_hip_filtfilt_process(plan._plan, x.data_ptr(), 2, 101, 100, None) == sd._lib.ERR_INVALID_ARG  # stride < samples
    assert lib.sdsp_hip_filtfilt_process(plan._plan, x.data_ptr() + 1, 1, 101, 101, None) == sd._lib.ERR_INVALID_ARG
    assert lib.sdsp_hip_filtfilt_process(plan._plan, x.data_ptr(), 0, 101, 101, None) == 0
    with pytest.raises(ValueError):  # scipy refuses the same
        scipy.signal.sosfiltfilt(sos_of(kind, a, b, g), np.zeros(100), padlen=100)
    # the default edge: L = P refused, L = P + 1 accepted
    d = _plan(sd, kind, a, b, g, "f32")
    assert d.padlen == 27
    with pytest.raises(ValueError):
        d.process(_signal(torch, "f32", 3, 27))
    d.process(_signal(torch, "f32", 3, 28))


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


@pytest.mark.parametrize("precision", ["f32", "f64", "mix"])
@pytest.mark.parametrize("variant", [0, 1])
def test_slices_give_the_same_bits_and_launches_match(torch_cuda, sd, precision, variant):
    torch = torch_cuda
    kind, a, b, g = _design(sd, "rand", 4)
    x = _signal(torch, precision, 1000, 1500, seed=9)
    whole = _plan(sd, kind, a, b, g, precision)
    rs = 8 if precision == "f64" else 4
    tiny = _plan(sd, kind, a, b, g, precision, workspace_bytes=64 * 27 * rs)
    tiny.set_variant(variant)
    info = tiny.info()
    assert info["slice_channels"] == 64 and info["workspace_bytes"] == 64 * 27 * rs
    assert whole.launches(1000, 1500) == 1 and tiny.launches(1000, 1500) == 16 and tiny.launches(0, 1500) == 0
    want = whole.process(x.clone())
    y = x.clone()
    got = tiny.process(y)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    y.copy_(x)
    n = _kernel_nodes(torch, lambda: tiny.process(y))
    assert n == tiny.launches(1000, 1500)
    nopad = _plan(sd, kind, a, b, g, precision, None)
    assert nopad.info()["workspace_bytes"] == 0 and nopad.launches(1000, 1500) == 1


@pytest.mark.parametrize("precision", ["f32", "f64", "mix"])
def test_graph_capture_replays_the_eager_call(torch_cuda, sd, precision):
    torch = torch_cuda
    kind, a, b, g = _design(sd, "bs", 4)
    x = _signal(torch, precision, 300, 2500, seed=11)
    plan = _plan(sd, kind, a, b, g, precision, workspace_bytes=128 * 27 * 8)
    want = plan.process(x.clone())
    y = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.process(y)
    y.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)


@pytest.mark.parametrize("precision", ["f32", "f64", "mix"])
def test_bank_filtfilt_leaves_the_stream_alone(torch_cuda, sd, precision):
    torch = torch_cuda
    p = PRECISIONS[precision]
    bank = sd.casc_2o_iir_lp(4, 6, p)
    bank.set_lp_coeff(1e3, 48e3)
    x = _signal(torch, precision, 6, 1024, seed=2)
    bank.process(x.clone())  # a stream in progress
    state = bank.state.clone()
    y = x.clone()
    bank.filtfilt(y)
    torch.cuda.synchronize()
    assert torch.equal(bank.state, state)
    want = _composition(torch, sd, x, LP, bank.m_a_coeff.reshape(-1), None, bank.m_gain, precision, "odd", None)
    assert torch.equal(y, want)
    # padtype / padlen select cached plans; a new design replaces them
    y2 = x.clone()
    bank.filtfilt(y2, padtype="even", padlen=50)
    assert torch.equal(y2, _composition(torch, sd, x, LP, bank.m_a_coeff.reshape(-1), None, bank.m_gain, precision, "even", 50))
    assert len(bank._filtfilt_plans) == 2
    info = bank._filtfilt_plans[(1, None)].info()  # six rows: one 64-channel group of the default edge
    assert (info["padlen"], info["workspace_bytes"], info["slice_channels"]) == (27, 64 * 27 * x.element_size(), 64)
    bank.set_lp_coeff(3e3, 48e3)
    assert len(bank._filtfilt_plans) == 0
    # samples < row length: the tail is untouched
    z = x.clone()
    bank.filtfilt(z, samples=1000)
    torch.cuda.synchronize()
    assert torch.equal(z[:, 1000:], x[:, 1000:])
    assert torch.equal(bank.state, state)


def test_sosfiltfilt_helper_matches_scipy(torch_cuda, sd):
    torch = torch_cuda
    rng = np.random.default_rng(21)
    x = rng.standard_normal((5, 3000)).cumsum(axis=1)
    xd = torch.from_numpy(x).cuda()
    for order, wn, btype in [(5, 0.1, "lowpass"), (5, 0.2, "highpass"), (3, [0.1, 0.3], "bandpass"), (7, 0.05, "lowpass")]:
        sos = scipy.signal.butter(order, wn, btype, output="sos")
        for padtype, padlen in [("odd", None), ("even", None), ("constant", 100), (None, None)]:
            want = scipy.signal.sosfiltfilt(sos, x, padtype=padtype, padlen=padlen)
            got = sd.sosfiltfilt(sos, xd, padtype, padlen)
            assert got.data_ptr() != xd.data_ptr()
            assert np.abs(got.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max(), (order, btype, padtype)
    # an un-normalised a0 and b0 != 1
    sos = scipy.signal.butter(4, 0.15, output="sos") * np.array([[3.0, 3.0, 3.0, 2.0, 2.0, 2.0]])
    want = scipy.signal.sosfiltfilt(sos / sos[:, 3:4], x)  # scipy itself wants a0 = 1
    assert np.abs(sd.sosfiltfilt(sos, xd).cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # float32 tensors: the f32 plan, and the mixed plan by request
    xf = xd.float()
    sos = scipy.signal.butter(5, 0.1, output="sos")
    want = scipy.signal.sosfiltfilt(sos, xf.double().cpu().numpy())
    got = sd.sosfiltfilt(sos, xf)
    assert got.dtype == torch.float32
    assert np.abs(got.double().cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()
    got = sd.sosfiltfilt(sos, xf, precision=sd.F32_F64STATE)
    assert np.abs(got.double().cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max()


def test_process_host_matches_device(torch_cuda, sd):
    torch = torch_cuda
    kind, a, b, g = _design(sd, "rand", 6)
    x = _signal(torch, "f64", 9, 700, seed=4)
    plan = _plan(sd, kind, a, b, g, "f64")
    want = plan.process(x.clone()).cpu().numpy()
    h = np.ascontiguousarray(x.cpu().numpy())
    assert sd.load().sdsp_hip_filtfilt_process_host(plan._plan, h.ctypes.data, 9, 700, 700) == 0
    assert np.array_equal(h, want)


def test_default_workspace_is_bounded(torch_cuda, sd):
    kind, a, b, g = _design(sd, "lp", 4)
    short = _plan(sd, kind, a, b, g, "f32").info()
    assert short["workspace_bytes"] <= 256 << 20 and short["slice_channels"] >= 1 << 17
    long_ = _plan(sd, kind, a, b, g, "f64", "odd", 1999).info()  # 2^17 channels of this edge would take 2 GiB
    assert long_["workspace_bytes"] <= 1 << 30 and long_["slice_channels"] % 64 == 0
    huge = _plan(sd, kind, a, b, g, "f64", "odd", 1 << 22).info()  # one 64-channel group needs more than the cap
    assert huge["slice_channels"] == 64 and huge["workspace_bytes"] == 64 * (1 << 22) * 8
    nopad = _plan(sd, kind, a, b, g, "f64", None).info()
    assert nopad["workspace_bytes"] == 0
