"""GPU parity tests for the FIR filter bank -- through the C ABI on a real MI355X.

The reference has no FIR filter (README.md:16 TODO), so parity with the reference is UNPINNED for
this row; the checker is the CPU oracle's FIR (pinned to scipy.signal.firwin / lfilter in
tests/test_oracle_fir.py).  The f64 kernel keeps the oracle's operation order (ascending taps, one
multiply and one add each) and is held to BIT-EXACT agreement; the f32 kernel (FMA) to the normwise
1e-6 of SURVEY 8(d).  Block-by-block streaming must equal one long call bit for bit
(testIIR.cpp:61-75 semantics)."""
import numpy as np
import pytest

from conftest import rel_max_err
from recur_exact import fir_plain

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


def _run(torch, bank, x, **kw):
    dt = torch.float64 if bank.precision == 1 else torch.float32
    d = torch.from_numpy(np.ascontiguousarray(x)).to(dt).cuda()
    bank.process(d, **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("taps", [1, 2, 15, 16, 17, 31, 32, 33, 48, 100, 257])
@pytest.mark.parametrize("channels,samples", [(1, 4096), (3, 1), (5, 15), (67, 100), (130, 1000), (9, 5000), (2, 9000)])
def test_f64_bit_exact_against_oracle(sd, torch_cuda, oracle, taps, channels, samples):
    rng = np.random.default_rng(taps * 1000 + channels + samples)
    h = rng.standard_normal(taps)
    x = rng.standard_normal((channels, samples))
    outs = {}
    for variant in (0, 1):
        bank = sd.fir_filter(taps, channels, sd.F64)
        bank.set_coeff(h)
        bank.set_variant(variant)
        outs[variant] = _run(torch_cuda, bank, x)
        if taps > 1:
            want_state = np.zeros((channels, taps - 1))
            k = min(samples, taps - 1)
            want_state[:, :k] = x[:, ::-1][:, :k]
            assert np.array_equal(bank.state.cpu().numpy(), want_state)
    for c in sorted({0, channels - 1, channels // 2}):
        assert np.array_equal(outs[0][c], oracle.fir_process(h, x[c])[0]), (taps, c)
    # every row: the oracle's operation order vectorised over the channels (tests/recur_exact.py, equal to the oracle bit for bit on the CPU)
    assert np.array_equal(outs[0], fir_plain(x, h, None, "f64")[0]), taps
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("taps,precision", [(1000, "f64"), (4096, "f64"), (4096, "f32")])
def test_long_filters(sd, torch_cuda, oracle, taps, precision):
    """SDSP_HIP_FIR_MAX_TAPS and the > 64 KiB LDS line (f64, 4096 taps: 72 KiB)."""
    rng = np.random.default_rng(taps)
    h = rng.standard_normal(taps) / np.sqrt(taps)
    f64 = precision == "f64"
    x = rng.standard_normal((3, 9000)).astype(np.float64 if f64 else np.float32)
    bank = sd.fir_filter(taps, 3, sd.F64 if f64 else sd.F32)
    bank.set_coeff(h)
    got = _run(torch_cuda, bank, x)
    if f64:
        assert np.array_equal(got[1], oracle.fir_process(h, x[1])[0])
    else:
        h32 = h.astype(np.float32).astype(np.float64)
        # a sequential f32 sum of T terms carries ~sqrt(T) eps: 64 * 1.19e-7 = 7.6e-6 at T = 4096 (the 1e-6 of
        # SURVEY 8(d) is stated for the short filters of the other tests)
        assert rel_max_err(got[1], oracle.fir_process(h32, x[1].astype(np.float64))[0]) < np.sqrt(taps) * 1.19e-7
    with pytest.raises(sd.SdspHipError):
        too_long = sd.fir_filter(4097, 1, sd.F32)
        too_long.set_coeff(np.ones(4097))
        too_long.process(torch_cuda.zeros((1, 16), device="cuda"))


@pytest.mark.parametrize("taps,ftype", [(31, 1), (32, 1), (33, 2), (64, 3), (65, 4)])
def test_designed_filters_f32_and_lfilter(sd, torch_cuda, oracle, taps, ftype):
    import scipy.signal
    rng = np.random.default_rng(taps)
    channels, samples = 300, 4096
    x = rng.standard_normal((channels, samples)).astype(np.float32)
    bank = sd.fir_filter(taps, channels, sd.F32)
    {1: bank.set_lp_coeff, 2: bank.set_hp_coeff}.get(ftype, lambda *a: None)(10e3, 100e3)
    if ftype == 3:
        bank.set_bp_coeff(10e3, 100e3, 1.1)
    if ftype == 4:
        bank.set_bs_coeff(10e3, 100e3, 1.1)
    got = _run(torch_cuda, bank, x)
    for variant in (1, 2, 3):  # default-policy, packed-FMA and one-FMA-per-tap kernels: same values
        bank.reset()
        bank.set_variant(variant)
        assert np.array_equal(_run(torch_cuda, bank, x), got), variant
    h32 = bank.m_coeff.astype(np.float32).astype(np.float64)
    for c in (0, 7, 299):
        want = oracle.fir_process(h32, x[c].astype(np.float64))[0]
        assert rel_max_err(got[c], want) < 1e-6
        assert rel_max_err(got[c], scipy.signal.lfilter(bank.m_coeff, 1.0, x[c].astype(np.float64))) < 1e-6


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_streaming_blocks_unaligned_rows_and_preload(sd, torch_cuda, oracle, precision):
    prec = sd.F64 if precision == "f64" else sd.F32
    npdt = np.float64 if precision == "f64" else np.float32
    rng = np.random.default_rng(11)
    taps, channels, samples = 45, 70, 1003  # odd stride: rows are not 16-byte aligned -> element path
    x = rng.standard_normal((channels, samples)).astype(npdt)
    whole_bank = sd.fir_filter(taps, channels, prec)
    whole_bank.set_lp_coeff(10e3, 100e3)
    whole = _run(torch_cuda, whole_bank, x)
    bank = sd.fir_filter(taps, channels, prec)
    bank.set_lp_coeff(10e3, 100e3)
    dt = torch_cuda.float64 if precision == "f64" else torch_cuda.float32
    d = torch_cuda.from_numpy(x.copy()).to(dt).cuda()
    for a, b in ((0, 1), (1, 8), (8, 40), (40, 600), (600, 1003)):  # blocks shorter and longer than the history
        bank.process(d, samples=b - a, offset=a)
    torch_cuda.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), whole)
    if precision == "f64":
        assert np.array_equal(whole[3], oracle.fir_process(whole_bank.m_coeff, x[3])[0])
    # a steady input through a preloaded unit-DC-gain low-pass is steady from the first sample
    pre = sd.fir_filter(taps, 5, prec)
    pre.set_lp_coeff(10e3, 100e3)
    pre.preload_filter(10.0)
    out = _run(torch_cuda, pre, np.full((5, 300), 10.0, dtype=npdt))
    assert np.abs(out - 10.0).max() < (1e-12 if precision == "f64" else 1e-5)


def test_host_entry_and_errors(sd, torch_cuda, oracle):
    import ctypes as C
    from simpledsp_amd import _lib as L
    lib = sd.load()
    rng = np.random.default_rng(3)
    h = rng.standard_normal(20)
    x = rng.standard_normal((4, 333))
    plan = C.c_void_p()
    L.check(lib.sdsp_hip_fir_plan_create(C.byref(plan), 20, h.ctypes.data, L.F64, 0))
    nbytes = C.c_uint64()
    L.check(lib.sdsp_hip_fir_state_bytes(plan, 4, C.byref(nbytes)))
    assert nbytes.value == 4 * 19 * 8
    y = x.copy()
    state = np.zeros((4, 19))
    L.check(lib.sdsp_hip_fir_process_host(plan, y.ctypes.data, 4, 200, 333, state.ctypes.data))
    L.check(lib.sdsp_hip_fir_process_host(plan, y[:, 200:].ctypes.data, 4, 133, 333, state.ctypes.data))
    for c in range(4):
        want, mem = oracle.fir_process(h, x[c])
        assert np.array_equal(y[c], want) and np.array_equal(state[c], mem)
    assert lib.sdsp_hip_fir_process(plan, None, 4, 10, 10, None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_fir_process(plan, y.ctypes.data, 4, 10, 5, None, None) == L.ERR_INVALID_ARG  # stride < samples
    assert lib.sdsp_hip_fir_process(plan, None, 0, 10, 10, None, None) == 0  # nothing to do
    lib.sdsp_hip_fir_plan_destroy(plan)


def test_full_size_properties(sd, torch_cuda, oracle):
    """BASELINE config-4 shape (1M channels x 4096 samples, f32) through a 32-tap low-pass: spot channels
    against the oracle, and linearity of the whole batch (size-independent property)."""
    torch = torch_cuda
    channels, samples, taps = 1 << 20, 4096, 32
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((channels, samples), generator=g, device="cuda", dtype=torch.float32)
    keep = {c: x[c].cpu().numpy().astype(np.float64) for c in (0, 12345, channels - 1)}
    bank = sd.fir_filter(taps, channels, sd.F32)
    bank.set_lp_coeff(10e3, 100e3)
    h32 = bank.m_coeff.astype(np.float32).astype(np.float64)
    y = x.clone()
    bank.process(y)
    torch.cuda.synchronize()
    for c, xin in keep.items():
        assert rel_max_err(y[c].cpu().numpy(), oracle.fir_process(h32, xin)[0]) < 1e-6
    # linearity: F(2x) == 2 F(x) exactly (power-of-two scaling commutes with every rounding)
    x.mul_(2.0)
    bank.reset()
    bank.process(x)
    torch.cuda.synchronize()
    assert torch.equal(x, y * 2.0)
