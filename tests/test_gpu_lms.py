"""GPU tests of the LMS / NLMS adaptive filter bank (sdsp_hip_lms_*) on a real MI355X.

The checker is tests/lms_ref.py, the contract's operation order in numpy, itself pinned to a scalar loop and to scipy.signal.lfilter in
tests/test_lms_host.py.  Both precisions, both kinds, both modes and both kernel variants are held to bit-exact agreement with it: y, e,
the final weights and the final history."""
import ctypes as C

import numpy as np
import pytest

import arena
from lms_ref import BLOCKS, lms_ref, lms_ref_stream, row_dtype

pytestmark = pytest.mark.gpu

CH = 133  # two full waves and a ragged one


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


def _rand(rng, shape, precision, cplx, scale=1.0):
    x = rng.standard_normal(shape)
    if cplx:
        x = (x + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)  # unit variance
    return (scale * x).astype(row_dtype(precision, cplx))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _step(mode, T):
    """(mu, eps) that keep everything finite on unit-variance data"""
    return (0.5, 1e-3) if mode == "nlms" else (0.2 / T, 0.0)


def _bank(sd, T, precision, cplx, mode, variant=0, weights=None, hist=None, channels=CH):
    b = sd.lms_bank(channels, T, "complex" if cplx else "real", sd.F64 if precision == "f64" else sd.F32, mode, _step(mode, T)[1])
    b.set_variant(variant)
    if weights is not None:
        b.set_weights(weights)
    if hist is not None and T > 1:
        b.set_history(hist)
    return b


def _np(t):
    return t.cpu().numpy()


def _check(b, got, want, tag):
    """got = (y, e) device tensors, want = the reference's (y, e, weights, history)"""
    names = ("y", "e", "weights", "history")
    have = (_np(got[0]), _np(got[1]), _np(b.weights()), _np(b.history()))
    for name, h, w in zip(names, have, want):
        assert h.shape == w.shape, (tag, name, h.shape, w.shape)
        assert _same(h, w), (tag, name, int((h != w).sum()))


@pytest.mark.parametrize("mode", ["lms", "nlms"])
# every path of the tap loop: T = TP (the form without tests) at 8, 16, 32, 64; the tested form under every bound with 1, 2 and 3
# taps left over after the groups of four (5, 7 | 14 | 27 | 33, 46), and T = 1
@pytest.mark.parametrize("n_taps", [1, 5, 7, 8, 14, 16, 27, 32, 33, 46, 64])
def test_bit_exact_against_reference(sd, torch_cuda, n_taps, mode):
    """every precision, kind and variant from a non-zero state; rows of two blocks and a ragged tail (the block length is the plan's),
    one S shorter than the history, S = 0"""
    rng = np.random.default_rng(n_taps * 7919 + len(mode))
    for precision in ("f32", "f64"):
        for cplx in (False, True):
            T = min(n_taps, 32) if (precision == "f64" and cplx) else n_taps  # F64 COMPLEX up to its limit
            mu, eps = _step(mode, T)
            block = _bank(sd, T, precision, cplx, mode).info()["block"]
            assert block >= 1
            for S in (2 * block + 37, (T - 1) // 2, 0):
                pad = S + 4 + (-S) % 4
                x, d = _rand(rng, (CH, pad), precision, cplx), _rand(rng, (CH, pad), precision, cplx)
                w0, h0 = _rand(rng, (CH, T), precision, cplx, 0.1), _rand(rng, (CH, T - 1), precision, cplx)
                want = lms_ref(x[:, :S], d[:, :S], T, mu, mode, eps, w0, h0, precision)
                for variant in (0, 1):
                    b = _bank(sd, T, precision, cplx, mode, variant, w0, h0)
                    got = b.process(_dev(torch_cuda, x), _dev(torch_cuda, d), mu, samples=S)
                    _check(b, got, want, (precision, cplx, variant, T, S))


@pytest.mark.parametrize("mode", ["lms", "nlms"])
@pytest.mark.parametrize("precision,cplx,n_taps", [("f32", False, 16), ("f32", True, 5), ("f64", False, 33), ("f64", True, 16)])
def test_any_split_gives_the_same_bits(sd, torch_cuda, precision, cplx, n_taps, mode):
    """beam_ref.py's BLOCKS pattern (empty calls included) in units of 29 samples: with mu changing from call to call (0 for one of
    them) against the reference fed the same way; with a constant mu also against the unsplit run"""
    rng = np.random.default_rng(29 + n_taps)
    T = n_taps
    mu, eps = _step(mode, T)
    blocks = [29 * v for v in BLOCKS]
    S = sum(blocks)
    x, d = _rand(rng, (CH, S), precision, cplx), _rand(rng, (CH, S), precision, cplx)
    starts = np.cumsum([0] + blocks[:-1])
    for mus in ([mu, mu, 0.5 * mu, mu, 0.0, mu, 0.25 * mu], [mu] * len(blocks)):
        want = lms_ref_stream(x, d, T, list(zip(blocks, mus)), mode, eps, None, None, precision)
        for variant in (0, 1):
            b = _bank(sd, T, precision, cplx, mode, variant)
            parts = [b.process(_dev(torch_cuda, x[:, s0:s0 + n].copy()), _dev(torch_cuda, d[:, s0:s0 + n].copy()), m)
                     for s0, n, m in zip(starts, blocks, mus)]
            got = tuple(torch_cuda.cat([p[i] for p in parts], dim=1) for i in (0, 1))
            _check(b, got, want, (variant, mus[2]))
    # the last round had a constant mu: the unsplit run gives its bits
    one = _bank(sd, T, precision, cplx, mode)
    _check(one, one.process(_dev(torch_cuda, x), _dev(torch_cuda, d), mu), want, "unsplit")


@pytest.mark.parametrize("precision,cplx,mode", [("f32", False, "nlms"), ("f64", True, "lms")])
def test_a_stream_continues_from_set_weights_and_a_carried_history(sd, torch_cuda, precision, cplx, mode):
    rng = np.random.default_rng(31)
    T, S1, S2 = 16, 45, 70
    mu, eps = _step(mode, T)
    x, d = _rand(rng, (CH, S1 + S2), precision, cplx), _rand(rng, (CH, S1 + S2), precision, cplx)
    want = lms_ref(x, d, T, mu, mode, eps, None, None, precision)
    a = _bank(sd, T, precision, cplx, mode)
    a.process(_dev(torch_cuda, x[:, :S1].copy()), _dev(torch_cuda, d[:, :S1].copy()), mu)
    for variant in (0, 1):
        b = _bank(sd, T, precision, cplx, mode, variant, _np(a.weights()), _np(a.history()))
        y, e = b.process(_dev(torch_cuda, x[:, S1:].copy()), _dev(torch_cuda, d[:, S1:].copy()), mu)
        assert _same(_np(y), want[0][:, S1:]) and _same(_np(e), want[1][:, S1:]), variant
        assert _same(_np(b.weights()), want[2]) and _same(_np(b.history()), want[3]), variant


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("precision,cplx,mode", [("f32", True, "nlms"), ("f64", False, "lms")])
def test_null_outputs_and_null_state(sd, torch_cuda, precision, cplx, mode, variant):
    """y, e or both NULL: the same weights and the same other output; state NULL = a zero-filled one, nothing kept"""
    rng = np.random.default_rng(33)
    T = 5
    mu, eps = _step(mode, T)
    full_bank = _bank(sd, T, precision, cplx, mode, variant)
    S = full_bank.info()["block"] + 9
    x, d = _rand(rng, (CH, S), precision, cplx), _rand(rng, (CH, S), precision, cplx)
    xd, dd = _dev(torch_cuda, x), _dev(torch_cuda, d)
    y, e = full_bank.process(xd, dd, mu)
    _check(full_bank, (y, e), lms_ref(x, d, T, mu, mode, eps, None, None, precision), variant)
    for want_y, want_e in ((True, False), (False, True), (False, False)):
        b = _bank(sd, T, precision, cplx, mode, variant)
        gy, ge = b.process(xd, dd, mu, want_y=want_y, want_e=want_e)
        assert (gy is None) == (not want_y) and (ge is None) == (not want_e)
        assert gy is None or arena.same_bits(gy, y)
        assert ge is None or arena.same_bits(ge, e)
        assert arena.same_bits(b.state, full_bank.state), (want_y, want_e)
    lib = sd.load()
    oy, oe = torch_cuda.zeros_like(y), torch_cuda.zeros_like(e)
    assert lib.sdsp_hip_lms_process(full_bank._plan, xd.data_ptr(), S, dd.data_ptr(), S, oy.data_ptr(), S, oe.data_ptr(), S, S, mu, None,
                                    None) == 0
    torch_cuda.cuda.synchronize()
    assert arena.same_bits(oy, y) and arena.same_bits(oe, e)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, precision, cplx):
    """x, d, y, e and state carved 0, 1 or 2 elements past a 512-byte boundary out of NaN-filled (and pattern-filled) arenas, padded row
    strides of their own: the interior has the aligned run's bits and nothing outside it is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(35)
    T, mode = 5, "nlms"
    mu, eps = _step(mode, T)
    ref = _bank(sd, T, precision, cplx, mode)
    S = ref.info()["block"] + 9
    x, d = _rand(rng, (CH, S), precision, cplx), _rand(rng, (CH, S), precision, cplx)
    w0, h0 = _rand(rng, (CH, T), precision, cplx, 0.1), _rand(rng, (CH, T - 1), precision, cplx)
    ref.set_weights(w0)
    ref.set_history(h0)
    cy, ce = ref.process(_dev(torch, x), _dev(torch, d), mu)
    _check(ref, (cy, ce), lms_ref(x, d, T, mu, mode, eps, w0, h0, precision), "aligned")
    start = torch.cat([_dev(torch, w0).flatten(), _dev(torch, h0).flatten()])
    for variant in (0, 1):
        b = _bank(sd, T, precision, cplx, mode, variant)
        for lead in (0, 1, 2):
            for fill in arena.fills(cy.dtype):
                frames = [arena.framed(torch, (CH, S), cy.dtype, lead, 64, fill, row_stride=S + pad) for pad in (5, 3, 7, 1)]
                ast, vst = arena.framed(torch, (start.numel(),), cy.dtype, lead, 64, fill)
                (ax, vx), (ad, vd), (ay, vy), (ae, ve) = frames
                vx[:, :S].copy_(_dev(torch, x))
                vd[:, :S].copy_(_dev(torch, d))
                vst.copy_(start)
                arenas = [ax, ad, ay, ae, ast]
                before = [arena.bits(a).clone() for a in arenas]
                assert lib.sdsp_hip_lms_process(b._plan, vx.data_ptr(), S + 5, vd.data_ptr(), S + 3, vy.data_ptr(), S + 7, ve.data_ptr(),
                                                S + 1, S, mu, vst.data_ptr(), None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, fill)
                assert arena.same_bits(vy[:, :S], cy) and arena.same_bits(ve[:, :S], ce), tag
                assert arena.same_bits(vst, ref.state), tag
                arena.assert_frame_untouched(before[0], ax, slice(0, 0))  # x and d are never written
                arena.assert_frame_untouched(before[1], ad, slice(0, 0))
                arena.assert_frame_untouched(before[2], ay, arena.interior_mask(torch, ay, vy, S))
                arena.assert_frame_untouched(before[3], ae, arena.interior_mask(torch, ae, ve, S))
                arena.assert_frame_untouched(before[4], ast, arena.interior_mask(torch, ast, vst))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mode", ["lms", "nlms"])
def test_nan_reaches_exactly_its_channel(sd, torch_cuda, mode, variant):
    """a NaN in d of channel 63 (a wave's last lane) and one in x of channel 64 (the next wave's first): those channels' later outputs
    and weights are NaN exactly where the reference's are, every other channel keeps the clean run's bits"""
    rng = np.random.default_rng(37)
    T = 5
    mu, eps = _step(mode, T)
    S = _bank(sd, T, "f32", False, mode).info()["block"] + 21
    x, d = _rand(rng, (CH, S), "f32", False), _rand(rng, (CH, S), "f32", False)
    clean_bank = _bank(sd, T, "f32", False, mode, variant)
    clean = clean_bank.process(_dev(torch_cuda, x), _dev(torch_cuda, d), mu)
    xp, dp = x.copy(), d.copy()
    dp[63, 11] = np.nan
    xp[64, 17] = np.nan
    want = lms_ref(xp, dp, T, mu, mode, eps, None, None, "f32")
    assert not np.isnan(want[0][63, :12]).any() and np.isnan(want[0][63, 12:]).all()  # y is a-priori: NaN from the next sample on
    assert not np.isnan(want[1][63, :11]).any() and np.isnan(want[1][63, 11:]).all()
    assert not np.isnan(want[0][64, :17]).any() and np.isnan(want[0][64, 17:]).all()
    b = _bank(sd, T, "f32", False, mode, variant)
    got = b.process(_dev(torch_cuda, xp), _dev(torch_cuda, dp), mu)
    have = (_np(got[0]), _np(got[1]), _np(b.weights()), _np(b.history()))
    clean_np = (_np(clean[0]), _np(clean[1]), _np(clean_bank.weights()), _np(clean_bank.history()))
    others = np.ones(CH, dtype=bool)
    others[[63, 64]] = False
    for name, h, w, c in zip(("y", "e", "weights", "history"), have, want, clean_np):
        assert np.array_equal(np.isnan(h), np.isnan(w)), name
        assert _same(h[~np.isnan(h)], w[~np.isnan(w)]), name
        assert _same(h[others], c[others]), name
    assert np.isnan(have[2][[63, 64]]).all()


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    """three calls (a block multiple, a ragged one, a short one) captured into one graph replay to the eager bits"""
    torch = torch_cuda
    rng = np.random.default_rng(39)
    T, mode = 16, "nlms"
    mu, eps = _step(mode, T)
    sizes = [64, 37, 7]
    S = sum(sizes)
    x, d = _rand(rng, (CH, S), "f32", False), _rand(rng, (CH, S), "f32", False)
    want = lms_ref(x, d, T, mu, mode, eps, None, None, "f32")
    xs = [_dev(torch, x[:, s0:s0 + n].copy()) for s0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    ds = [_dev(torch, d[:, s0:s0 + n].copy()) for s0, n in zip(np.cumsum([0] + sizes[:-1]), sizes)]
    ys = [torch.empty((CH, n), dtype=torch.float32, device="cuda") for n in sizes]
    es = [torch.empty((CH, n), dtype=torch.float32, device="cuda") for n in sizes]
    b = _bank(sd, T, "f32", False, mode)
    run = lambda: [b.process(xs[i], ds[i], mu, y=ys[i], e=es[i]) for i in range(3)]  # noqa: E731
    run()  # the state exists before capture
    eager = (torch.cat(ys, dim=1).clone(), torch.cat(es, dim=1).clone())
    _check(b, eager, want, "eager")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    b.state.zero_()
    for t in ys + es:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    _check(b, (torch.cat(ys, dim=1), torch.cat(es, dim=1)), want, "replay")


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(41)
    T, S, mode = 16, 90, "nlms"
    mu, eps = _step(mode, T)
    for cplx in (False, True):
        x, d = _rand(rng, (CH, S), "f64", cplx), _rand(rng, (CH, S), "f64", cplx)
        w0, h0 = _rand(rng, (CH, T), "f64", cplx, 0.1), _rand(rng, (CH, T - 1), "f64", cplx)
        b = _bank(sd, T, "f64", cplx, mode, 0, w0, h0)
        st = np.concatenate([w0.flatten(), h0.flatten()])
        y, e = b.process(_dev(torch_cuda, x), _dev(torch_cuda, d), mu)
        oy, oe = np.zeros_like(x), np.zeros_like(x)
        assert lib.sdsp_hip_lms_process_host(b._plan, x.ctypes.data, S, d.ctypes.data, S, oy.ctypes.data, S, oe.ctypes.data, S, S, mu,
                                             st.ctypes.data) == 0
        assert _same(oy, _np(y)) and _same(oe, _np(e)) and _same(st, _np(b.state))
        # without e and without state
        oy2 = np.zeros_like(x)
        assert lib.sdsp_hip_lms_process_host(b._plan, x.ctypes.data, S, d.ctypes.data, S, oy2.ctypes.data, S, None, 0, S, mu, None) == 0
        assert _same(oy2, lms_ref(x, d, T, mu, mode, eps, None, None, "f64")[0])


def test_weights_info_error_codes_and_launch_count(sd, torch_cuda):
    torch = torch_cuda
    lib = sd.load()
    L = sd._lib
    b = _bank(sd, 16, "f32", True, "nlms")
    info = b.info()
    assert (info["channels"], info["taps"], info["kind"], info["precision"], info["mode"]) == (CH, 16, sd.LMS_COMPLEX, sd.F32, sd.LMS_NLMS)
    assert info["kernel"] == "sdsp_lms_kernel" and info["variant"] == 0 and info["eps"] == float(np.float32(1e-3))
    assert info["lds_bytes"] == (16 + 2 * info["block"]) * 65 * 8 and 4 * info["lds_bytes"] <= 160 * 1024
    assert b.state_bytes() == CH * (2 * 16 - 1) * 8
    assert b.weights().shape == (CH, 16) and b.history().shape == (CH, 15)
    assert b.weights().data_ptr() == b.state.data_ptr() and b.history().data_ptr() == b.state.data_ptr() + CH * 16 * 8
    assert b.launches(100) == 2 and b.launches(0) == 0
    assert _bank(sd, 1, "f32", False, "lms").launches(100) == 1  # no history to carry
    b.set_variant(1)
    assert b.info()["kernel"] == "sdsp_lms_plain_kernel" and b.info()["variant"] == 1
    for precision, cplx in (("f32", False), ("f32", True), ("f64", False), ("f64", True)):
        for T in (1, 8, 9, 32) + (() if (precision == "f64" and cplx) else (33, 64)):
            i = _bank(sd, T, precision, cplx, "lms").info()
            es = (8 if precision == "f64" else 4) * (2 if cplx else 1)
            assert i["block"] >= 1 and (i["block"] * es) % 16 == 0 and 4 * i["lds_bytes"] <= 160 * 1024, (precision, cplx, T)
    p = _bank(sd, 16, "f32", False, "lms", channels=2)
    x, d = torch.zeros((2, 64), device="cuda"), torch.zeros((2, 64), device="cuda")
    y, e = torch.zeros((2, 64), device="cuda"), torch.zeros((2, 64), device="cuda")
    X, D, Y, E = (t.data_ptr() for t in (x, d, y, e))

    def run(x=X, xs=64, d=D, ds=64, y=Y, ys=64, e=E, es=64, n=64, mu=0.01, state=None):
        return lib.sdsp_hip_lms_process(p._plan, x, xs, d, ds, y, ys, e, es, n, mu, state, None)

    assert run() == 0
    assert run(x=None) == L.ERR_INVALID_ARG and run(d=None) == L.ERR_INVALID_ARG
    assert run(y=None) == 0 and run(e=None) == 0 and run(y=None, e=None) == 0
    assert run(xs=60) == L.ERR_INVALID_ARG and run(ds=60) == L.ERR_INVALID_ARG
    assert run(ys=63) == L.ERR_INVALID_ARG and run(es=63) == L.ERR_INVALID_ARG
    assert run(y=X + 8 * 4) == L.ERR_INVALID_ARG and run(e=D) == L.ERR_INVALID_ARG and run(e=Y + 4) == L.ERR_INVALID_ARG  # overlaps
    assert run(x=X + 2, n=32) == L.ERR_INVALID_ARG  # misaligned
    assert run(mu=float("nan")) == L.ERR_INVALID_ARG and run(mu=1e300) == L.ERR_INVALID_ARG
    assert run(n=1 << 31) == L.ERR_INVALID_SIZE
    assert run(n=0) == 0
    assert lib.sdsp_hip_lms_plan_set_variant(p._plan, 2) == L.ERR_INVALID_ARG
    # a call of S = 0 leaves the state alone
    st = torch.full((2 * 31,), 3.0, device="cuda")
    assert run(n=0, state=st.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((st == 3.0).all())
