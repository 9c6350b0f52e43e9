"""GPU tests of the time-delay beamformer bank (sdsp_hip_beam_*) on a real MI355X.

The checker is tests/beam_ref.py, the contract's operation order in numpy, itself pinned to scipy.signal.lfilter in
tests/test_beam_host.py.  Both precisions, both kinds and both kernel variants are held to bit-exact agreement with it."""
import ctypes as C

import numpy as np
import pytest

import arena
from beam_ref import BLOCKS, beam_ref, hist_len, row_dtype

pytestmark = pytest.mark.gpu

DMAX = 300  # the plan's largest delay in the grid cases: more than one LDS window apart from delay 0 is the spread test's job


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


def _rand(rng, shape, precision, cplx):
    x = rng.standard_normal(shape)
    if cplx:
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(row_dtype(precision, cplx))


def _taps(rng, n, cplx):
    g = rng.standard_normal(n)
    return g + 1j * rng.standard_normal(n) if cplx else g


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    """bit patterns: exact and NaN-safe"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _entries(rng, beams, n_taps, cplx):
    """sensors = 3, sensor 1 unused.  Beam 1 has a single entry, beam 2 none, beams 3 and 4 are one beam listed twice; delays 0, 1, 7 and
    the plan's maximum; further beams get random delays"""
    twice = [(0, DMAX, _taps(rng, n_taps, cplx)), (2, 0, _taps(rng, n_taps, cplx))]
    e = [(0, 0, 0, _taps(rng, n_taps, cplx)), (0, 2, 7, _taps(rng, n_taps, cplx)), (1, 2, 1, _taps(rng, n_taps, cplx))]
    e += [(3, c, d, g) for c, d, g in twice] + [(4, c, d, g) for c, d, g in twice]
    for b in range(5, beams):
        for c in (0, 2):
            if rng.integers(0, 4):
                e.append((b, c, int(rng.integers(0, 41)), _taps(rng, n_taps, cplx)))
    return e


def _bank(sd, entries, sensors, beams, n_taps, groups, precision, cplx, variant=0, state=None):
    import torch
    b = sd.beamformer_bank(sensors, beams, n_taps, groups, "complex" if cplx else "real", sd.F64 if precision == "f64" else sd.F32)
    b.set_entries(entries)
    b.set_variant(variant)
    if state is not None:
        b._state = torch.from_numpy(np.ascontiguousarray(state.astype(row_dtype(precision, cplx)))).cuda()
    return b


@pytest.mark.parametrize("beams", [5, 9])
@pytest.mark.parametrize("n_taps", [1, 5, 16, 33])
def test_bit_exact_against_reference(sd, torch_cuda, n_taps, beams):
    """every precision, kind and variant; rows of two blocks and a ragged tail (the block size is the plan's), one S < hist, S = 0"""
    rng = np.random.default_rng(n_taps * 7919 + beams)
    groups, sensors = 2, 3
    for precision in ("f32", "f64"):
        for cplx in (False, True):
            ent = _entries(rng, beams, n_taps, cplx)
            H = hist_len(ent, n_taps)
            assert H == DMAX + n_taps - 1
            info = _bank(sd, ent, sensors, beams, n_taps, groups, precision, cplx).info()
            assert info["hist"] == H and info["max_delay"] == DMAX and info["chunks"] == -(-beams // 4)
            for S in (2 * info["block_out"] + 37, H // 2, 0):
                x = _rand(rng, (groups * sensors, S + 4 + (-S) % 4), precision, cplx)
                hist = _rand(rng, (groups * sensors, H), precision, cplx)
                want, want_state = beam_ref(ent, x[:, :S], sensors, beams, n_taps, groups, hist, precision)
                got = {}
                for variant in (0, 1):
                    b = _bank(sd, ent, sensors, beams, n_taps, groups, precision, cplx, variant, hist)
                    out = torch_cuda.empty((groups * beams, S + 4 + (-S) % 4), dtype=b._row_dtype(), device="cuda")
                    got[variant] = b.process(_dev(torch_cuda, x), out=out, samples=S).cpu().numpy()
                    tag = (precision, cplx, variant, S)
                    assert got[variant].shape == want.shape, tag
                    assert _same(got[variant], want), (tag, int((got[variant] != want).sum()))
                    assert _same(b.state.cpu().numpy(), want_state), tag
                    for grp in range(groups):
                        r = got[variant][grp * beams:(grp + 1) * beams]
                        assert _same(r[3], r[4]), tag                  # the beam listed twice
                        assert _same(r[2], np.zeros_like(r[2])), tag   # no entry: +0
                assert _same(got[0], got[1]), (precision, cplx, S)


@pytest.mark.parametrize("precision,cplx", [("f32", False), ("f64", True)])
def test_a_wide_delay_spread_splits_the_chunk(sd, torch_cuda, precision, cplx):
    """delays 0 and 40000 on one sensor in adjacent beams: their windows cannot share an LDS line, so the chunk table has one more chunk;
    the bits are the reference's"""
    rng = np.random.default_rng(31)
    n_taps, sensors, beams, groups = 16, 2, 3, 2
    ent = lambda far: [(0, 0, 0, _taps(rng, n_taps, cplx)), (0, 1, 3, _taps(rng, n_taps, cplx)),  # noqa: E731
                       (1, 0, far, _taps(rng, n_taps, cplx)), (2, 1, 9, _taps(rng, n_taps, cplx))]
    near, wide = ent(5), ent(40000)
    narrow_info = _bank(sd, near, sensors, beams, n_taps, groups, precision, cplx).info()
    info = _bank(sd, wide, sensors, beams, n_taps, groups, precision, cplx).info()
    assert narrow_info["chunks"] == 1 and info["chunks"] == 2 and info["max_spread"] < 40000
    assert info["hist"] == 40000 + n_taps - 1 and 2 * info["lds_line_bytes"] <= 64 * 1024
    H = info["hist"]
    S = info["block_out"] + 77
    x = _rand(rng, (groups * sensors, S), precision, cplx)
    hist = _rand(rng, (groups * sensors, H), precision, cplx)
    want, want_state = beam_ref(wide, x, sensors, beams, n_taps, groups, hist, precision)
    for variant in (0, 1):
        b = _bank(sd, wide, sensors, beams, n_taps, groups, precision, cplx, variant, hist)
        assert _same(b.process(_dev(torch_cuda, x)).cpu().numpy(), want), variant
        assert _same(b.state.cpu().numpy(), want_state), variant


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_streaming_equals_one_call(sd, torch_cuda, precision, cplx):
    rng = np.random.default_rng(23)
    groups, sensors, beams = 2, 3, 5
    lib = sd.load()
    for n_taps, unit in [(16, 97), (5, 400), (33, 1)]:
        ent = _entries(rng, beams, n_taps, cplx)
        H = hist_len(ent, n_taps)
        blocks = [v * unit for v in BLOCKS]
        S = sum(blocks)
        x = _rand(rng, (groups * sensors, S), precision, cplx)
        hist = _rand(rng, (groups * sensors, H), precision, cplx)
        for start in (hist, None):  # a random history; and a fresh stream, which is zero history
            want_ref, state_ref = beam_ref(ent, x, sensors, beams, n_taps, groups, start, precision)
            one = _bank(sd, ent, sensors, beams, n_taps, groups, precision, cplx, 0, start)
            want = one.process(_dev(torch_cuda, x)).cpu().numpy()
            assert _same(want, want_ref)
            b = _bank(sd, ent, sensors, beams, n_taps, groups, precision, cplx, 0, start)
            parts = [b.process(_dev(torch_cuda, x[:, s0:s0 + n].copy())).cpu().numpy()
                     for s0, n in zip(np.cumsum([0] + blocks[:-1]), blocks)]
            assert _same(np.concatenate(parts, axis=1), want), (n_taps, unit)
            assert _same(b.state.cpu().numpy(), one.state.cpu().numpy())
            assert _same(b.state.cpu().numpy(), state_ref)
        # state = NULL through the C entry: zero history, nothing carried
        one._ensure_plan()
        xd = _dev(torch_cuda, x)
        out = torch_cuda.zeros((groups * beams, S), dtype=one._row_dtype(), device="cuda")
        assert lib.sdsp_hip_beam_process(one._plan, xd.data_ptr(), S, out.data_ptr(), S, S, None, None) == 0
        assert _same(out.cpu().numpy(), want)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, precision, cplx):
    """in, out and state carved 0, 1 or 2 elements past a 512-byte boundary out of NaN-filled (and pattern-filled) arenas, odd padded
    strides: the interior has the aligned run's bits and nothing outside it is written"""
    torch = torch_cuda
    lib = sd.load()
    rng = np.random.default_rng(25)
    n_taps, groups, sensors, beams = 5, 2, 3, 5
    ent = _entries(rng, beams, n_taps, cplx)
    H = hist_len(ent, n_taps)
    S = _bank(sd, ent, sensors, beams, n_taps, groups, precision, cplx).info()["block_out"] + 9
    x = _rand(rng, (groups * sensors, S), precision, cplx)
    hist = _rand(rng, (groups * sensors, H), precision, cplx)
    ref = _bank(sd, ent, sensors, beams, n_taps, groups, precision, cplx, 0, hist)
    clean = ref.process(_dev(torch, x))
    clean_state = ref.state
    assert _same(clean.cpu().numpy(), beam_ref(ent, x, sensors, beams, n_taps, groups, hist, precision)[0])
    for variant in (0, 1):
        b = _bank(sd, ent, sensors, beams, n_taps, groups, precision, cplx, variant)
        b._ensure_plan()
        for lead in (0, 1, 2):
            for fill in arena.fills(clean.dtype):
                ain, vin = arena.framed(torch, (groups * sensors, S), clean.dtype, lead, 64, fill, row_stride=S + 5)
                aout, vout = arena.framed(torch, (groups * beams, S), clean.dtype, lead, 64, fill, row_stride=S + 3)
                ast, vst = arena.framed(torch, (groups * sensors, H), clean.dtype, lead, 64, fill)
                vin[:, :S].copy_(_dev(torch, x))
                vst.copy_(_dev(torch, hist))
                before = [arena.bits(a).clone() for a in (ain, aout, ast)]
                assert lib.sdsp_hip_beam_process(b._plan, vin.data_ptr(), S + 5, vout.data_ptr(), S + 3, S, vst.data_ptr(), None) == 0
                torch.cuda.synchronize()
                tag = (variant, lead, fill)
                assert arena.same_bits(vout[:, :S], clean), tag
                assert arena.same_bits(vst, clean_state), tag
                arena.assert_frame_untouched(before[0], ain, slice(0, 0))  # in is never written
                arena.assert_frame_untouched(before[1], aout, arena.interior_mask(torch, aout, vout, S))
                arena.assert_frame_untouched(before[2], ast, arena.interior_mask(torch, ast, vst))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n_taps", [1, 5, 16, 33])
def test_nan_reaches_exactly_its_outputs(sd, torch_cuda, n_taps, variant):
    rng = np.random.default_rng(n_taps)
    groups, sensors, beams = 2, 3, 5
    ent = [(b, c, d, rng.uniform(0.5, 1.5, n_taps)) for b, c, d, _ in _entries(rng, beams, n_taps, False)]  # no zero taps
    H = hist_len(ent, n_taps)
    S = 1500
    x = _rand(rng, (groups * sensors, S), "f32", False)
    hist = _rand(rng, (groups * sensors, H), "f32", False)
    clean_bank = _bank(sd, ent, sensors, beams, n_taps, groups, "f32", False, variant, hist)
    clean = clean_bank.process(_dev(torch_cuda, x)).cpu().numpy()
    p = 1021  # its outputs straddle the first block's end
    n = np.arange(S)
    for poisoned in (0, 1, sensors + 2):  # sensor 1: no beam names it; the last: group 1
        xp = x.copy()
        xp[poisoned, p] = np.nan
        want = beam_ref(ent, xp, sensors, beams, n_taps, groups, hist, "f32")[0]
        got = _bank(sd, ent, sensors, beams, n_taps, groups, "f32", False, variant, hist).process(_dev(torch_cuda, xp)).cpu().numpy()
        grp, sensor = divmod(poisoned, sensors)
        for row in range(groups * beams):
            hit = np.zeros(S, dtype=bool)
            for b, c, d, _ in ent:
                if row == grp * beams + b and c == sensor:
                    hit |= (n >= p + d) & (n <= p + d + n_taps - 1)
            assert np.array_equal(np.isnan(want[row]), hit), (poisoned, row)  # the reference says so ...
            assert np.array_equal(np.isnan(got[row]), hit), (poisoned, row)   # ... and the kernel does it
            assert _same(got[row][~hit], clean[row][~hit]), (poisoned, row)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_unit_tap_is_the_delayed_row(sd, torch_cuda, precision, cplx):
    """T = 1, tap 1.0, delay d: fma(1, x, +0) = x, so the beam is the sensor's row delayed by d, bit for bit"""
    rng = np.random.default_rng(41)
    delays = [0, 1, 7, 1500]
    ent = [(b, 0, d, [1.0]) for b, d in enumerate(delays)]
    S = 2600
    x = _rand(rng, (1, S), precision, cplx)
    hist = _rand(rng, (1, 1500), precision, cplx)
    ext = np.concatenate([hist[:, ::-1], x], axis=1)[0]
    for variant in (0, 1):
        got = _bank(sd, ent, 1, len(delays), 1, 1, precision, cplx, variant, hist).process(_dev(torch_cuda, x)).cpu().numpy()
        for b, d in enumerate(delays):
            assert _same(got[b], ext[1500 - d:1500 - d + S]), (variant, d)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_single_entry_beam_is_the_fir_filter(sd, torch_cuda, precision):
    """one entry with delay 0 per beam = fir_filter of that sensor with the same taps, as values: fir.hip starts from the first product
    and not from +0, so only the sign of a zero may differ"""
    rng = np.random.default_rng(42)
    prec = sd.F64 if precision == "f64" else sd.F32
    for n_taps in (16, 33, 1):
        h = rng.standard_normal(n_taps)
        x = _rand(rng, (4, 3000), precision, False)
        b = _bank(sd, [(c, c, 0, h) for c in range(4)], 4, 4, n_taps, 1, precision, False)
        y = b.process(_dev(torch_cuda, x)).cpu().numpy()
        f = sd.fir_filter(n_taps, 4, prec)
        f.set_coeff(h)
        d = _dev(torch_cuda, x)
        f.process(d)
        assert np.array_equal(y, d.cpu().numpy()), n_taps
        if n_taps > 1:
            assert np.array_equal(b.state.cpu().numpy(), f.state.cpu().numpy())


def test_steering_helpers_fill_a_dense_plan(sd, torch_cuda):
    """set_steering = plane_wave_delays -> beam_delay_taps -> set_dense; complex weights turn the real delay taps"""
    rng = np.random.default_rng(43)
    pos = np.arange(6)[:, None] * np.array([[0.5, 0.0]])
    ang = np.deg2rad([40.0, 100.0, 75.0])
    tau = sd.plane_wave_delays(pos, np.stack([np.cos(ang), np.sin(ang)], axis=1), 1.0, 3.3)
    w = rng.standard_normal((3, 6)) + 1j * rng.standard_normal((3, 6))
    b = sd.beamformer_bank(6, 3, 16, 1, "complex", sd.F32)
    b.set_steering(tau, w, 8.0)
    delays, taps = sd.beam_delay_taps(tau, np.ones((3, 6)), 16, 8.0)
    ent = [(i, c, int(delays[i, c]), taps[i, c] * w[i, c]) for i in range(3) for c in range(6)]
    x = _rand(rng, (6, 1300), "f32", True)
    assert _same(b.process(_dev(torch_cuda, x)).cpu().numpy(), beam_ref(ent, x, 6, 3, 16, 1, None, "f32")[0])
    assert b.info()["entries"] == 18


def test_error_codes_and_launch_count(sd, torch_cuda):
    torch = torch_cuda
    lib = sd.load()
    L = sd._lib
    g = np.ones(3 * 16)
    ent = (L.BeamEntry * 3)(L.BeamEntry(0, 0, 0), L.BeamEntry(0, 1, 5), L.BeamEntry(1, 1, 9))
    p = C.c_void_p()

    def create(sensors=2, beams=2, groups=1, taps=16, n=3, e=ent, taps_ptr=g.ctypes.data, kind=L.BEAM_REAL, precision=L.F32):
        return lib.sdsp_hip_beam_plan_create(C.byref(p), sensors, beams, groups, taps, n, e, taps_ptr, kind, precision, 0)

    assert create(sensors=0) == -1 and create(sensors=4097) == -1 and create(beams=0) == -1 and create(beams=4097) == -1
    assert create(groups=0) == -1 and create(groups=1 << 31) == -1
    assert create(taps=0) == -1 and create(taps=257) == -1
    assert create(n=(1 << 20) + 1) == -1
    assert create(e=None) == -5 and create(taps_ptr=None) == -5
    assert create(kind=2) == -5 and create(precision=L.F32_F64STATE) == -5
    assert create(sensors=1) == -5 and create(beams=1) == -5  # an entry names sensor 1 / beam 1
    assert create(e=(L.BeamEntry * 3)(L.BeamEntry(0, 0, 0), L.BeamEntry(0, 1, 65536), L.BeamEntry(1, 1, 9))) == -1
    assert create(e=(L.BeamEntry * 3)(L.BeamEntry(0, 1, 0), L.BeamEntry(0, 0, 5), L.BeamEntry(1, 1, 9))) == -5  # sensors descend
    assert create(e=(L.BeamEntry * 3)(L.BeamEntry(0, 1, 0), L.BeamEntry(0, 1, 5), L.BeamEntry(1, 1, 9))) == -5  # a pair twice
    assert create(e=(L.BeamEntry * 3)(L.BeamEntry(1, 0, 0), L.BeamEntry(0, 1, 5), L.BeamEntry(1, 1, 9))) == -5  # beams not grouped
    assert b"sorted by beam" in lib.sdsp_hip_last_error_string()
    assert lib.sdsp_hip_beam_plan_create(None, 2, 2, 1, 16, 3, ent, g.ctypes.data, L.BEAM_REAL, L.F32, 0) == -5
    assert create() == 0
    x = torch.zeros((2, 64), device="cuda")
    y = torch.zeros((2, 64), device="cuda")
    run = lambda *a: lib.sdsp_hip_beam_process(p, *a, None, None)  # noqa: E731
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 64) == 0
    assert run(None, 64, y.data_ptr(), 64, 64) == -5
    assert run(x.data_ptr(), 64, None, 64, 64) == -5
    assert run(x.data_ptr(), 60, y.data_ptr(), 64, 64) == -5  # in_stride < samples
    assert run(x.data_ptr(), 64, y.data_ptr(), 63, 64) == -5  # out_stride < samples
    assert run(x.data_ptr(), 64, x.data_ptr() + 8 * 4, 64, 64) == -5  # overlap
    assert run(x.data_ptr() + 2, 64, y.data_ptr(), 64, 32) == -5  # misaligned
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 1 << 31) == -1
    assert run(x.data_ptr(), 64, y.data_ptr(), 64, 0) == 0
    assert lib.sdsp_hip_beam_process(None, x.data_ptr(), 64, y.data_ptr(), 64, 64, None, None) == -5
    assert lib.sdsp_hip_beam_plan_set_variant(p, 2) == -5
    n = C.c_uint64(0)
    assert lib.sdsp_hip_beam_state_bytes(p, C.byref(n)) == 0 and n.value == 2 * (9 + 15) * 4
    assert lib.sdsp_hip_beam_plan_launches(p, 64, C.byref(n)) == 0 and n.value == 2  # the beam kernel and the new history
    assert lib.sdsp_hip_beam_plan_launches(p, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.sdsp_hip_beam_plan_destroy(p) == 0
    one = _bank(sd, [(0, 0, 0, [2.0])], 1, 1, 1, 1, "f32", False)
    assert one.launches(64) == 1  # hist = 0: nothing to carry
    empty = _bank(sd, [], 2, 3, 4, 1, "f32", False)  # a plan without entries: every beam +0
    out = empty.process(torch.ones((2, 70), device="cuda")).cpu().numpy()
    assert _same(out, np.zeros((3, 70), dtype=np.float32))
    b = _bank(sd, [(0, 0, 0, np.ones(16)), (1, 1, 9, np.ones(16))], 2, 2, 16, 3, "f64", True)
    info = b.info()
    assert (info["sensors"], info["beams"], info["groups"], info["taps"], info["entries"]) == (2, 2, 3, 16, 2)
    assert (info["max_delay"], info["hist"], info["chunks"], info["variant"]) == (9, 24, 1, 0)
    assert info["kernel"] == "sdsp_beam_kernel" and info["block_out"] == 1024 and info["kind"] == sd.BEAM_COMPLEX
    assert info["lds_line_bytes"] % 16 == 0 and 2 * info["lds_line_bytes"] <= 64 * 1024
    b.set_variant(1)
    assert b.info()["kernel"] == "sdsp_beam_plain_kernel" and b.info()["variant"] == 1


def test_host_entry_equals_device_path(sd, torch_cuda):
    lib = sd.load()
    rng = np.random.default_rng(27)
    groups, sensors, beams, n_taps, S = 2, 3, 5, 16, 1500
    for cplx in (False, True):
        ent = _entries(rng, beams, n_taps, cplx)
        H = hist_len(ent, n_taps)
        x = _rand(rng, (groups * sensors, S), "f64", cplx)
        hist = _rand(rng, (groups * sensors, H), "f64", cplx)
        b = _bank(sd, ent, sensors, beams, n_taps, groups, "f64", cplx, 0, hist)
        dev = b.process(_dev(torch_cuda, x)).cpu().numpy()
        out = np.zeros((groups * beams, S), dtype=x.dtype)
        st = hist.copy()
        assert lib.sdsp_hip_beam_process_host(b._plan, x.ctypes.data, S, out.ctypes.data, S, S, st.ctypes.data) == 0
        assert _same(out, dev)
        assert _same(st, b.state.cpu().numpy())


def test_graph_capture_replays_the_eager_result(sd, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(28)
    groups, sensors, beams, n_taps, S = 2, 3, 5, 16, 5000
    ent = _entries(rng, beams, n_taps, False)
    x = _rand(rng, (groups * sensors, S), "f32", False)
    want = _bank(sd, ent, sensors, beams, n_taps, groups, "f32", False).process(_dev(torch, x)).cpu().numpy()
    b = _bank(sd, ent, sensors, beams, n_taps, groups, "f32", False)
    xd = _dev(torch, x)
    out = torch.empty((groups * beams, S), dtype=torch.float32, device="cuda")
    b.process(xd, out=out)  # plan + state exist before capture
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
