"""GPU tests of the 2-D CFAR plans (sdsp_hip_cfar2d_*) on a real MI355X.

The checker is tests/cfar2d_ref.py, the contract in numpy, itself pinned to the training set's definition in tests/test_cfar2d_host.py.
The contract fixes the order of every addition, so both precisions, both edge modes and both kernel variants are held to bit-exact
agreement with it: thr, det, counts and every written record.  The maps are small on purpose: every path of the kernels (wrapped rows,
clipped columns, partial strips and row blocks, the chunked staging of the widest window) is reached at these sizes."""
import ctypes as C

import numpy as np
import pytest

import arena
import cfar2d_ref as ref
from rank_ref import specials

pytestmark = pytest.mark.gpu

GEOMS = [(0, 0, 1, 0), (1, 0, 0, 0), (1, 1, 1, 1), (4, 1, 8, 2), (2, 3, 16, 0), (32, 16, 64, 64)]  # (Ld, Gd, Lr, Gr)
DTYPES = [np.float32, np.float64]
EDGES = ["mark", "clip"]
ALPHA = 2.75  # about 6 % of exponential noise above the threshold
STRIP = 64


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


def _prec(sd, dtype):
    return sd.F64 if np.dtype(dtype) == np.float64 else sd.F32


def _plan(sd, D, R, geom, dtype, edge="mark", peak=False, alpha=ALPHA, scale=None, max_maps=3, variant=0):
    Ld, Gd, Lr, Gr = geom
    plan = sd.cfar2d_plan(D, R, (Ld, Lr), (Gd, Gr), alpha=None if scale is not None else alpha, scale=scale, edge=edge, peak=peak,
                          max_maps=max_maps, precision=_prec(sd, dtype))
    plan.set_variant(variant)
    return plan


def _maps(seed, maps, D, R, dtype):
    return np.random.default_rng(seed).standard_exponential((maps, D, R)).astype(dtype)


def _edge(edge):
    return ref.CLIP if edge == "clip" else ref.MARK


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_result(res, want, cap, tag):
    """res: a Cfar2dResult on the device; want: (thr, det, lists) of the reference"""
    thr, det, lists = want
    if res.thr is not None:
        assert _same(res.thr.cpu().numpy(), thr), (tag, "thr")
    if res.det is not None:
        assert _same(res.det.cpu().numpy(), det), (tag, "det")
    if res.hits is not None:
        counts = res.counts.cpu().numpy().view(np.uint32)
        assert counts.tolist() == [len(h) for h in lists], (tag, "counts")
        for m, h in enumerate(lists):
            got = res.hits.numpy(m)
            assert got.tobytes() == h[:cap].tobytes(), (tag, "records of map", m)


def _run_both(sd, torch, p, geom, edge, tag, peak=False, alpha=ALPHA, scale=None, extra_cap=3):
    """p (maps, D, R) through both variants with every output, against the reference; returns the reference"""
    maps, D, R = p.shape
    c = scale if scale is not None else ref.alpha_table(R, geom, alpha)
    want = ref.detect(p, geom, c, _edge(edge), peak)
    cap = max(len(h) for h in want[2]) + extra_cap
    dev = torch.from_numpy(p).cuda()
    for variant in (0, 1):
        plan = _plan(sd, D, R, geom, p.dtype, edge, peak, alpha, scale, max_maps=maps, variant=variant)
        res = plan.process(dev, hits=cap)
        torch.cuda.synchronize()
        _check_result(res, want, cap, (tag, "variant", variant))
        plan.close()
    return want


def _shapes(sd, geom, dtype):
    Ld, Gd, Lr, Gr = geom
    Hd, Hr = Ld + Gd, Lr + Gr
    low = 2 * Hd + 1
    tile = _plan(sd, max(low, 64), 600, geom, dtype).info()["tile_rows"]
    k = -(-(low + 1) // tile)  # the first multiple of the row block with D = k tile - 1 still allowed
    D0 = max(low, 5)
    shapes = [(low, 33), (k * tile + 1, 33), (k * tile - 1, 33), (D0, 1), (D0, 2 * Hr + 1), (D0, STRIP), (D0, STRIP - 1), (D0, STRIP + 1),
              (D0, 2 * STRIP + 3)]
    if Hr:
        shapes.append((D0, 2 * Hr))
    return shapes, tile


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", GEOMS)
def test_both_variants_equal_the_reference_bit_for_bit(sd, torch_cuda, geom, dtype, edge):
    shapes, tile = _shapes(sd, geom, dtype)
    for i, (D, R) in enumerate(shapes):
        plan = _plan(sd, D, R, geom, dtype)
        assert plan.info()["tile_rows"] == tile or D <= tile // 2  # the row block the shapes were made for
        _run_both(sd, torch_cuda, _maps(100 + i, 3, D, R, dtype), geom, edge, (geom, D, R))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_ordinary_map(sd, torch_cuda, dtype):
    for edge in EDGES:
        _run_both(sd, torch_cuda, _maps(9, 3, 64, 600, dtype), (4, 1, 8, 2), edge, ("64 x 600", edge))
    _run_both(sd, torch_cuda, _maps(9, 3, 64, 600, dtype), (4, 1, 8, 2), "clip", "64 x 600 peak", peak=True)
    table = ref.pfa_table(600, (4, 1, 8, 2), 1e-2)
    _run_both(sd, torch_cuda, _maps(9, 3, 64, 600, dtype), (4, 1, 8, 2), "clip", "64 x 600 table", scale=table)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", [(1, 1, 1, 1), (4, 1, 8, 2)])
def test_special_values(sd, torch_cuda, geom, dtype):
    """+-0, +-inf, subnormals, the largest finite values and NaNs of several payloads and both signs among the powers: the same bits as
    the reference, every NaN threshold the canonical quiet NaN, and no detection where either side is a NaN"""
    rng = np.random.default_rng(31)
    p = _maps(32, 3, 23, 131, dtype)
    sp = specials(dtype)
    mask = rng.random(p.shape) < 0.02
    p[mask] = sp[rng.integers(0, len(sp), size=int(mask.sum()))]
    p[1, 5] = sp[rng.integers(0, len(sp), size=131)]  # a whole row of them
    for edge in EDGES:
        for peak in (False, True):
            thr, det, _ = _run_both(sd, torch_cuda, p, geom, edge, ("specials", edge, peak), peak=peak)
            nan = np.isnan(thr)
            assert nan.any() and (~nan).any()
            u = np.uint32 if dtype == np.float32 else np.uint64
            quiet = 0x7FC00000 if dtype == np.float32 else 0x7FF8000000000000
            assert np.all(thr.view(u)[nan] == quiet)
            assert not det[nan | np.isnan(p)].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_nan_reaches_exactly_its_training_cells(sd, torch_cuda, dtype):
    torch = torch_cuda
    geom = (2, 1, 3, 1)
    Hd, Hr, Gd, Gr = 3, 4, 1, 1
    D, R = 40, 131
    tile = _plan(sd, D, R, geom, dtype).info()["tile_rows"]
    assert tile < D
    p = _maps(41, 3, D, R, dtype)
    c = ref.alpha_table(R, geom, ALPHA)
    clean = ref.detect(p, geom, c, ref.CLIP)[0]
    dd, rr = np.meshgrid(np.arange(D), np.arange(R), indexing="ij")
    for d0, r0 in ((0, 70), (D - 1, 5), (20, 0), (20, R - 1), (tile - 1, STRIP - 1), (tile, STRIP), (tile - 1, STRIP)):
        q = p.copy()
        q[1, d0, r0] = np.nan
        di = np.minimum((dd - d0) % D, (d0 - dd) % D)
        rj = np.abs(rr - r0)
        reached = (di <= Hd) & (rj <= Hr) & ~((di <= Gd) & (rj <= Gr))
        assert not reached[d0, r0]
        dev = torch.from_numpy(q).cuda()
        for variant in (0, 1):
            plan = _plan(sd, D, R, geom, dtype, "clip", variant=variant)
            thr = plan.process(dev, det=False).thr.cpu().numpy()
            assert np.array_equal(np.isnan(thr[1]), reached), (d0, r0, variant)
            assert _same(thr[1][~reached], clean[1][~reached]), (d0, r0, variant)
            assert _same(thr[0], clean[0]) and _same(thr[2], clean[2]), (d0, r0, variant)


def _framed_call(torch, plan, p, want, cap, lead, fill_index):
    """every buffer of one call framed `lead` elements past a 512-byte boundary; the frames, the records past min(count, cap) and the
    interiors are checked against `want`"""
    thr_w, det_w, lists = want
    maps, D, R = p.shape
    real = torch.from_numpy(p).dtype
    word = torch.int32 if p.dtype == np.float32 else torch.int64  # one element of a record's alignment
    words = 4 if p.dtype == np.float32 else 3
    margin = 256
    fr, fi = arena.fills(real)[fill_index], arena.fills(word)[fill_index]
    a_thr, thr = arena.framed(torch, (maps, D, R), real, lead, margin, fr)
    a_det, det = arena.framed(torch, (maps, D, R), torch.uint8, lead, margin, fi)
    a_hit, hit = arena.framed(torch, (maps, max(cap, 1), words), word, lead, margin, fi)
    a_cnt, cnt = arena.framed(torch, (maps,), torch.int32, lead, margin, fi)
    before = {k: (arena.bits(a).clone() if a.is_floating_point() else a.clone()) for k, a in (("thr", a_thr), ("det", a_det), ("hit", a_hit), ("cnt", a_cnt))}

    def run(view):
        plan.process_ptr(view.data_ptr(), thr.data_ptr(), det.data_ptr(), hit.data_ptr(), cnt.data_ptr(), cap, maps,
                         torch.cuda.current_stream().cuda_stream)

    # the input: its frame and its interior keep their bits (check_framed's "in place" result is the input itself)
    arena.check_framed(torch, torch.from_numpy(p).cuda(), torch.from_numpy(p).cuda(), run, [lead], margin, what="p")
    torch.cuda.synchronize()
    arena.assert_frame_untouched(before["thr"], a_thr, arena.interior_mask(torch, a_thr, thr))
    assert _same(thr.cpu().numpy(), thr_w)
    for key, a, view, inner in (("det", a_det, det, det_w), ("cnt", a_cnt, cnt, np.array([len(h) for h in lists], dtype=np.uint32))):
        assert bool(torch.equal(a[~arena.interior_mask(torch, a, view)], before[key][~arena.interior_mask(torch, a, view)])), key
        assert view.cpu().numpy().tobytes() == inner.tobytes(), key
    # the records: the first min(count, cap) of every map are the reference's, every other word of the arena keeps its fill
    expect = before["hit"].cpu().numpy().copy()
    start = (hit.data_ptr() - a_hit.data_ptr()) // a_hit.element_size()
    inner = expect[start:start + hit.numel()].reshape(maps, max(cap, 1), words)
    for m, h in enumerate(lists):
        n = min(len(h), cap)
        inner[m, :n] = np.frombuffer(h[:n].tobytes(), dtype=expect.dtype).reshape(n, words)
    assert a_hit.cpu().numpy().tobytes() == expect.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", (0, 1))
def test_framed_buffers_at_every_element_offset(sd, torch_cuda, dtype, variant):
    geom, D, R = (4, 1, 8, 2), 13, 33
    p = _maps(51, 3, D, R, dtype)
    for edge in EDGES:
        want = ref.detect(p, geom, ref.alpha_table(R, geom, ALPHA), _edge(edge))
        counts = [len(h) for h in want[2]]
        assert min(counts) < max(counts)
        cap = max(counts) - 1  # one map overflows, the others leave records unwritten
        plan = _plan(sd, D, R, geom, dtype, edge, variant=variant)
        for lead in range(4):
            for fill_index in (0, 1):
                _framed_call(torch_cuda, plan, p, want, cap, lead, fill_index)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("edge", EDGES)
def test_hit_list_caps_and_extreme_maps(sd, torch_cuda, dtype, edge):
    """alpha = 0 makes the threshold +0: a positive map hits in every cell (MARK: of the interior), a zero map in none; two ordinary
    maps with zeros sprinkled in stand around them.  cap = 0, 1, a count, a count - 1, and more than every count."""
    torch = torch_cuda
    geom, D, R = (1, 1, 2, 1), 9, 70
    rng = np.random.default_rng(61)
    p = _maps(62, 4, D, R, dtype)
    for m in (0, 3):
        p[m][rng.random((D, R)) < 0.7] = 0.0
    p[1] = 0.0
    want = ref.detect(p, geom, ref.alpha_table(R, geom, 0.0), _edge(edge))
    counts = [len(h) for h in want[2]]
    assert counts[1] == 0 and counts[2] == (D * R if edge == "clip" else D * (R - 6)) and 0 < counts[0] < counts[2]
    dev = torch.from_numpy(p).cuda()
    for variant in (0, 1):
        plan = _plan(sd, D, R, geom, dtype, edge, alpha=0.0, max_maps=4, variant=variant)
        for cap in (0, 1, counts[0], counts[0] - 1, counts[2], counts[2] - 1, counts[2] + 5):
            res = plan.process(dev, hits=cap)
            torch.cuda.synchronize()
            _check_result(res, want, cap, (edge, variant, cap))
            if cap:  # nothing at or past min(count, cap) was written: process() hands out zeroed records
                raw = res.hits.raw.cpu().numpy()
                for m in range(4):
                    assert not raw[m, min(counts[m], cap):].any(), (edge, variant, cap, m)


@pytest.mark.parametrize("dtype", DTYPES)
def test_each_output_alone_has_the_bits_of_the_full_call(sd, torch_cuda, dtype):
    torch = torch_cuda
    geom, D, R = (4, 1, 8, 2), 35, 131
    p = _maps(71, 3, D, R, dtype)
    want = ref.detect(p, geom, ref.alpha_table(R, geom, ALPHA), ref.CLIP, True)
    cap = max(len(h) for h in want[2])
    dev = torch.from_numpy(p).cuda()
    for variant in (0, 1):
        plan = _plan(sd, D, R, geom, dtype, "clip", peak=True, variant=variant)
        for thr, det, hits in ((True, False, None), (False, True, None), (False, False, cap), (True, False, cap), (False, True, cap)):
            res = plan.process(dev, thr=thr, det=det, hits=hits)
            torch.cuda.synchronize()
            assert (res.thr is not None, res.det is not None, res.hits is not None) == (thr, det, hits is not None)
            _check_result(res, want, cap, (variant, thr, det, hits))


@pytest.mark.parametrize("dtype", DTYPES)
def test_maps_below_max_maps_and_refused_calls(sd, torch_cuda, dtype):
    torch = torch_cuda
    geom, D, R = (1, 1, 2, 1), 9, 70
    p = _maps(81, 3, D, R, dtype)
    want = ref.detect(p, geom, ref.alpha_table(R, geom, ALPHA), ref.MARK)
    cap = 16
    for variant in (0, 1):
        plan = _plan(sd, D, R, geom, dtype, max_maps=3, variant=variant)
        for maps in (1, 2, 3):
            res = plan.process(torch.from_numpy(p[:maps]).cuda(), hits=cap)
            torch.cuda.synchronize()
            _check_result(res, (want[0][:maps], want[1][:maps], want[2][:maps]), cap, (variant, maps))
        # refused calls return their code and write nothing
        real = torch.from_numpy(p).dtype
        x = torch.from_numpy(np.concatenate([p, p[:1]])).cuda()
        thr = torch.full((4, D, R), 7.0, dtype=real, device="cuda")
        det = torch.full((4, D, R), 7, dtype=torch.uint8, device="cuda")
        hits = torch.full((4, cap, 6), 7, dtype=torch.int32, device="cuda")
        counts = torch.full((4,), 7, dtype=torch.int32, device="cuda")
        es = x.element_size()
        lib, h, L = plan._lib, plan._h, sd._lib
        P = lambda t: t.data_ptr()
        cases = [
            (L.ERR_INVALID_SIZE, (P(x), P(thr), P(det), P(hits), P(counts), cap, 4)),          # maps > max_maps
            (L.ERR_INVALID_SIZE, (P(x), P(thr), P(det), P(hits), P(counts), 1 << 31, 3)),      # cap
            (L.ERR_INVALID_ARG, (None, P(thr), P(det), P(hits), P(counts), cap, 3)),           # no input
            (L.ERR_INVALID_ARG, (P(x), None, None, None, None, cap, 3)),                       # no output
            (L.ERR_INVALID_ARG, (P(x), P(thr), P(det), P(hits), None, cap, 3)),                # hits without counts
            (L.ERR_INVALID_ARG, (P(x), P(thr), P(det), None, P(counts), cap, 3)),              # counts without hits
            (L.ERR_INVALID_ARG, (P(x) + 2, P(thr), P(det), P(hits), P(counts), cap, 3)),       # misaligned
            (L.ERR_INVALID_ARG, (P(x), P(thr) + 1, P(det), P(hits), P(counts), cap, 3)),
            (L.ERR_INVALID_ARG, (P(x), P(thr), P(det), P(hits) + es // 2, P(counts), cap, 3)),
            (L.ERR_INVALID_ARG, (P(x), P(thr), P(det), P(hits), P(counts) + 2, cap, 3)),
            (L.ERR_INVALID_ARG, (P(x), P(x) + es * D * R, P(det), P(hits), P(counts), cap, 3)),  # thr inside p
            (L.ERR_INVALID_ARG, (P(x), P(thr), P(det), P(thr) + es * 8, P(counts), cap, 3)),      # hits inside thr
            (L.ERR_INVALID_ARG, (P(x), P(thr), P(det), P(hits), P(hits) + 16, cap, 3)),           # counts inside hits
        ]
        for code, args in cases:
            assert lib.sdsp_hip_cfar2d_process(h, *args, None) == code, args
        torch.cuda.synchronize()
        assert bool((thr == 7.0).all()) and bool((det == 7).all()) and bool((hits == 7).all()) and bool((counts == 7).all())
        assert lib.sdsp_hip_cfar2d_process(h, P(x), P(thr), P(det), P(hits), P(counts), cap, 0, None) == L.OK  # maps == 0: nothing
        torch.cuda.synchronize()
        assert bool((thr == 7.0).all()) and bool((counts == 7).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_peak_rule(sd, torch_cuda, dtype):
    torch = torch_cuda
    geom = (1, 1, 1, 1)  # the guard box is the 3 x 3 neighbourhood
    p = np.ones((3, 6, 70), dtype=dtype)
    p[0, 2, 2:5] = 50.0     # a plateau along range: its first cell
    p[0, 0, 6] = p[0, 5, 6] = 40.0  # across the Doppler wrap: the row-5 cell, which has row 0 behind it
    p[0, 1:4, 30] = 45.0    # along Doppler: its first cell
    p[0, 3, 63:66] = 60.0   # across a strip boundary
    p[1] = p[0]
    p[1, 1, 3] = np.nan     # a NaN neighbour suppresses (2, 2), whose threshold does not see it
    p[2] = _maps(91, 1, 6, 70, dtype)[0]
    want = _run_both(sd, torch, p, geom, "clip", "peak", peak=True, alpha=1.6)
    cells = lambda m: [(int(h["doppler"]), int(h["range"])) for h in want[2][m]]
    assert cells(0) == [(1, 30), (2, 2), (3, 63), (5, 6)]
    assert cells(1) == [(1, 30), (3, 63), (5, 6)]
    for D in (1, 2, 3):  # the wrapped neighbours as they fall
        _run_both(sd, torch, _maps(92, 3, D, 70, dtype), (0, 0, 2, 1), "clip", ("peak D", D), peak=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_set_alpha_equals_a_fresh_plan(sd, torch_cuda, dtype):
    torch = torch_cuda
    geom, D, R = (4, 1, 8, 2), 13, 131
    p = _maps(95, 3, D, R, dtype)
    dev = torch.from_numpy(p).cuda()
    for edge in EDGES:
        want = ref.detect(p, geom, ref.alpha_table(R, geom, ALPHA), _edge(edge))
        for variant in (0, 1):
            plan = _plan(sd, D, R, geom, dtype, edge, alpha=1.0, variant=variant)
            plan.set_alpha(ALPHA)
            assert plan.info()["alpha"] == ALPHA
            res = plan.process(dev, hits=64)
            torch.cuda.synchronize()
            _check_result(res, want, 64, (edge, variant))
    tabled = _plan(sd, D, R, geom, dtype, scale=np.ones(R))
    with pytest.raises(sd.SdspHipError) as e:
        tabled.set_alpha(2.0)
    assert e.value.code == sd._lib.ERR_INVALID_ARG


@pytest.mark.parametrize("variant", (0, 1))
def test_graph_capture_replays_the_eager_result(sd, torch_cuda, variant):
    torch = torch_cuda
    geom, D, R, cap = (4, 1, 8, 2), 35, 131, 400
    p = _maps(97, 3, D, R, np.float32)
    want = ref.detect(p, geom, ref.alpha_table(R, geom, ALPHA), ref.MARK)
    plan = _plan(sd, D, R, geom, np.float32, variant=variant)
    x = torch.from_numpy(p).cuda()
    thr = torch.zeros_like(x)
    det = torch.zeros((3, D, R), dtype=torch.uint8, device="cuda")
    raw = torch.zeros((3, cap, 4), dtype=torch.int32, device="cuda")
    counts = torch.zeros((3,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.process_ptr(x.data_ptr(), thr.data_ptr(), det.data_ptr(), raw.data_ptr(), counts.data_ptr(), cap, 3,
                         torch.cuda.current_stream().cuda_stream)
    for t in (thr, det, raw, counts):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    res = sd.Cfar2dResult(thr, det, sd.Cfar2dHits(raw, counts, cap, torch.float32), counts)
    _check_result(res, want, cap, "replay")
    x.mul_(0.5)
    x[1, 7, 60] = 1000.0
    g.replay()
    torch.cuda.synchronize()
    _check_result(res, ref.detect(x.cpu().numpy(), geom, ref.alpha_table(R, geom, ALPHA), ref.MARK), cap, "replay on new input")


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entry_equals_the_device_path(sd, torch_cuda, dtype):
    geom, D, R = (4, 1, 8, 2), 16, 33
    p = _maps(99, 3, D, R, dtype)
    want = ref.detect(p, geom, ref.alpha_table(R, geom, ALPHA), ref.CLIP)
    for variant in (0, 1):
        plan = _plan(sd, D, R, geom, dtype, "clip", variant=variant)
        for cap in (0, 5, 200):
            thr, det, lists, counts = plan.process_host(p, hits=cap)
            assert _same(thr, want[0]) and _same(det, want[1])
            assert counts.tolist() == [len(h) for h in want[2]]
            for m in range(3):
                assert lists[m].tobytes() == want[2][m][:cap].tobytes()
        thr, det, lists, counts = plan.process_host(p, det=False)
        assert _same(thr, want[0]) and det is None and lists is None


def test_launches_and_info(sd, torch_cuda):
    for dtype in DTYPES:
        es = np.dtype(dtype).itemsize
        for geom in GEOMS:
            Ld, Gd, Lr, Gr = geom
            Hd, Hr = Ld + Gd, Lr + Gr
            D = max(2 * Hd + 1, 64)
            plan = _plan(sd, D, 600, geom, dtype, "clip", peak=True, max_maps=5)
            i = plan.info()
            assert (i["D"], i["R"], i["max_maps"]) == (D, 600, 5)
            assert (i["train_d"], i["guard_d"], i["train_r"], i["guard_r"]) == geom
            assert i["cells"] == (2 * Hd + 1) * (2 * Hr + 1) - (2 * Gd + 1) * (2 * Gr + 1) == int(ref.cells(600, *geom)[300])
            assert (i["edge"], i["peak"], i["tabled"], i["variant"], i["alpha"]) == (1, 1, 0, 0, ALPHA)
            assert i["kernel"] == "sdsp_cfar2d_kernel" and i["tile_cols"] == STRIP and i["tile_rows"] in (8, 16, 32)
            assert i["threads"] == 8 * i["tile_rows"] <= 256
            rows = i["tile_rows"] + 2 * Hd
            pitch = (STRIP + 2 * Hr) | 1
            chunk = min(rows, max(8, 24 * 1024 // (pitch * es)))
            assert i["lds_bytes"] == (2 * rows * (STRIP + 1) + i["tile_rows"] * STRIP + chunk * pitch) * es <= 160 * 1024
            assert i["workspace_bytes"] == 5 * D * 10 * 12
            assert (plan.launches(True, False), plan.launches(False, True), plan.launches(True, True)) == (1, 3, 3)
            plan.set_variant(1)
            i = plan.info()
            assert i["kernel"] == "sdsp_cfar2d_plain_kernel" and i["variant"] == 1 and i["lds_bytes"] == 0
            assert (plan.launches(True, False), plan.launches(False, True), plan.launches(True, True)) == (1, 3, 4)
    assert _plan(sd, 64, 600, (4, 1, 8, 2), np.float32).info()["tile_rows"] == 32


def test_chain_from_the_column_plan(sd, torch_cuda):
    """FftColsPlan(n = 16, POWER, shift) on a 2 x 16 x 40 cube, then a cfar2d_plan on its output buffer: the reference applied to that
    buffer's bits; range_doppler_detect returns the same list"""
    torch = torch_cuda
    rng = np.random.default_rng(20)
    cube = (rng.standard_normal((2, 16, 40)) + 1j * rng.standard_normal((2, 16, 40))).astype(np.complex64)
    cube[0, :, 17] += 6.0 * np.exp(2j * np.pi * 3 * np.arange(16) / 16)
    cube[1, :, 30] += 5.0 * np.exp(-2j * np.pi * 5 * np.arange(16) / 16)
    window = np.hanning(16)
    train, guard, pfa, cap = (2, 4), (1, 1), 1e-3, 64
    cols = sd.FftColsPlan(16, 40, sd.forward_fft, sd.F32, output="power", shift=True, window=window)
    power = cols.exec(torch.from_numpy(cube).cuda())
    det = sd.cfar2d_plan(16, 40, train, guard, pfa=pfa, peak=True, max_maps=2)
    res = det.process(power, hits=cap)
    torch.cuda.synchronize()
    geom = (train[0], guard[0], train[1], guard[1])
    want = ref.detect(power.cpu().numpy(), geom, ref.pfa_table(40, geom, pfa), ref.MARK, True)
    _check_result(res, want, cap, "chain")
    assert (8 + 3, 17) in [(int(h["doppler"]), int(h["range"])) for h in want[2][0]]
    assert (8 - 5, 30) in [(int(h["doppler"]), int(h["range"])) for h in want[2][1]]
    power2, hits = sd.range_doppler_detect(torch.from_numpy(cube).cuda(), window, train, guard, pfa, cap=cap)
    torch.cuda.synchronize()
    assert arena.same_bits(power2, power)
    for m in range(2):
        assert hits.numpy(m).tobytes() == want[2][m].tobytes()
    one = sd.cfar2d(power, train, guard, pfa=pfa, peak=True, hits=cap)
    _check_result(one, want, cap, "one-off")
