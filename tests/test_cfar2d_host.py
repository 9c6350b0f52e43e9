"""CPU-side checks of the 2-D CFAR plans: the numpy contract (tests/cfar2d_ref.py) against the training set taken by its definition,
the host designer sdsp_hip_cfar2d_scale against the Python table bit for bit, the false-alarm rate the designer delivers, and every
argument error of sdsp_hip_cfar2d_plan_create -- all of which come back before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

import cfar2d_ref as ref

import simpledsp_amd as sd
from simpledsp_amd import _lib as L

GEOMS = ((0, 0, 1, 0), (1, 0, 0, 0), (1, 1, 1, 1), (2, 1, 3, 2), (2, 3, 4, 0))


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_reference_equals_the_training_set_by_definition(geom, dtype):
    Ld, Gd, Lr, Gr = geom
    Hd, Hr = Ld + Gd, Lr + Gr
    rng = np.random.default_rng(7)
    eps = np.finfo(dtype).eps
    for D, R in ((2 * Hd + 1, 2 * Hr + 3), (2 * Hd + 1, max(1, 2 * Hr)), (2 * Hd + 4, max(1, Hr)), (2 * Hd + 2, 1), (2 * Hd + 3, 19)):
        p = rng.standard_exponential((2, D, R)).astype(dtype)
        T = ref.total(p, geom)
        n_ref = ref.cells(R, *geom)
        for m in range(2):
            s, n = ref.brute(p[m], geom)
            assert np.array_equal(n, np.broadcast_to(n_ref, (D, R))), (D, R)
            # positive terms: the error of a sum of n terms in any order is below n eps times the sum
            assert np.all(np.abs(T[m].astype(np.float64) - s) <= np.maximum(n, 1) * eps * s), (D, R)
        # MARK and CLIP differ on the edge columns only, where MARK is +inf and never detects
        c = ref.alpha_table(R, geom, 3.0)
        tm, dm, _ = ref.detect(p, geom, c, ref.MARK)
        tc, dc, lists = ref.detect(p, geom, c, ref.CLIP)
        r = np.arange(R)
        edge = (r < Hr) | (r >= R - Hr)
        assert np.all(np.isinf(tm[:, :, edge])) and not dm[:, :, edge].any()
        assert np.array_equal(tm[:, :, ~edge], tc[:, :, ~edge]) and np.array_equal(dm[:, :, ~edge], dc[:, :, ~edge])
        with np.errstate(all="ignore"):
            want = (T * c.astype(dtype)[None, None, :])
        assert np.array_equal(tc[~np.isnan(want)], want[~np.isnan(want)])
        for m in range(2):
            assert len(lists[m]) == int(dc[m].sum())
            order = lists[m]["doppler"].astype(np.int64) * R + lists[m]["range"]
            assert np.all(np.diff(order) > 0)


def test_peak_rule_of_the_reference():
    geom = (1, 1, 1, 1)  # the guard box is the 3 x 3 neighbourhood: a NaN there leaves the threshold alone
    p = np.ones((1, 6, 9), dtype=np.float32)
    p[0, 2, 2:5] = 50.0  # a plateau along range: its first cell wins (p > q for the neighbour in front, p >= q for the one behind)
    p[0, 0, 6] = p[0, 5, 6] = 40.0  # a plateau across the Doppler wrap: the row-5 cell has row 0 behind it (i = +1) and wins
    c = ref.alpha_table(9, geom, 1.6)
    _, det, lists = ref.detect(p, geom, c, ref.CLIP, peak=False)
    assert det[0, 2, 2:5].all() and det[0, 0, 6] and det[0, 5, 6]
    _, det, lists = ref.detect(p, geom, c, ref.CLIP, peak=True)
    assert [(int(h["doppler"]), int(h["range"])) for h in lists[0]] == [(2, 2), (5, 6)]
    q = p.copy()
    q[0, 1, 3] = np.nan  # a NaN neighbour suppresses (2, 2), whose threshold does not see it
    thr, _, lists = ref.detect(q, geom, c, ref.CLIP, peak=True)
    assert not np.isnan(thr[0, 2, 2])
    assert [(int(h["doppler"]), int(h["range"])) for h in lists[0]] == [(5, 6)]


def _desc(geom, edge=L.CFAR2D_EDGE_MARK, peak=0, alpha=1.0):
    Ld, Gd, Lr, Gr = geom
    return L.Cfar2dDesc(Ld, Gd, Lr, Gr, edge, peak, alpha)


@pytest.mark.parametrize("geom", GEOMS + ((4, 1, 8, 2), (32, 16, 64, 64)))
def test_designer_equals_the_python_table_bit_for_bit(geom):
    lib = sd.load()
    Hd, Hr = geom[0] + geom[1], geom[2] + geom[3]
    for R in (1, max(1, 2 * Hr), 2 * Hr + 1, 2 * Hr + 40):
        for pfa in (1e-2, 1e-6, 0.5):
            out = np.full(R, -1.0)
            d = _desc(geom)
            assert lib.sdsp_hip_cfar2d_scale(2 * Hd + 1, R, C.byref(d), pfa, out.ctypes.data) == L.OK
            want = ref.pfa_table(R, geom, pfa)
            assert np.array_equal(out.view(np.uint64), want.view(np.uint64)), (R, pfa)
            assert np.array_equal(sd.cfar2d_scale(2 * Hd + 1, R, (geom[0], geom[2]), (geom[1], geom[3]), pfa), want)
    # on the interior the table is the CA constant alpha_n / n
    n = int(ref.cells(2 * Hr + 40, *geom)[Hr + 5])
    assert n == (2 * Hd + 1) * (2 * Hr + 1) - (2 * geom[1] + 1) * (2 * geom[3] + 1)
    assert ref.pfa_table(2 * Hr + 40, geom, 1e-3)[Hr + 5] == 1e-3 ** (-1.0 / n) - 1.0


def test_designer_delivers_its_false_alarm_rate():
    """40 maps of 32 x 128 exponential noise, window (4, 1, 4, 1), pfa = 1e-2: the interior cells' false alarms lie within five binomial
    sigma of pfa cells, and in CLIP mode with the constant-pfa table the edge columns do too.  Conditions on the reference: the GPU
    inherits them by bit equality."""
    geom, pfa = (4, 1, 4, 1), 1e-2
    Hr = 5
    p = np.random.default_rng(20261020).standard_exponential((40, 32, 128)).astype(np.float32)
    c = ref.pfa_table(128, geom, pfa)
    _, det, _ = ref.detect(p, geom, c, ref.MARK)
    cells = 40 * 32 * (128 - 2 * Hr)
    sigma = np.sqrt(cells * pfa * (1 - pfa))
    alarms = int(det.sum())
    print(f"interior: {alarms} of {cells}, expected {pfa * cells:.0f} +- {sigma:.1f}")
    assert abs(alarms - pfa * cells) <= 5 * sigma
    _, det, _ = ref.detect(p, geom, c, ref.CLIP)
    edge_cells = 40 * 32 * 2 * Hr
    sigma = np.sqrt(edge_cells * pfa * (1 - pfa))
    alarms = int(det[:, :, :Hr].sum() + det[:, :, -Hr:].sum())
    print(f"edge columns: {alarms} of {edge_cells}, expected {pfa * edge_cells:.0f} +- {sigma:.1f}")
    assert abs(alarms - pfa * edge_cells) <= 5 * sigma


def _create(D, R, geom=(4, 1, 8, 2), max_maps=1, precision=L.F32, edge=L.CFAR2D_EDGE_MARK, scale=None, out=True, desc=True):
    lib = sd.load()
    h = C.c_void_p()
    d = _desc(geom, edge)
    s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    rc = lib.sdsp_hip_cfar2d_plan_create(C.byref(h) if out else None, D, R, max_maps, C.byref(d) if desc else None,
                                         None if s is None else s.ctypes.data, precision, 0)
    assert h.value is None or rc == L.OK
    if h.value:
        lib.sdsp_hip_cfar2d_plan_destroy(h)
    return rc


def test_argument_errors_come_before_the_device():
    ok = (L.OK, L.ERR_NO_DEVICE)  # whatever machine this runs on, an argument error is never one of these
    assert _create(64, 600) in ok
    assert _create(64, 600, out=False) == L.ERR_INVALID_ARG
    assert _create(64, 600, desc=False) == L.ERR_INVALID_ARG
    for geom in ((4, 1, 65, 2), (4, 1, 8, 65), (33, 1, 8, 2), (4, 17, 8, 2), (0, 1, 0, 2)):
        assert _create(200, 600, geom) == L.ERR_INVALID_SIZE, geom
    assert _create(200, 600, (32, 16, 64, 64)) in ok
    assert _create(200, 600, (0, 0, 1, 0)) in ok and _create(200, 600, (1, 0, 0, 0)) in ok
    assert _create(10, 600) == L.ERR_INVALID_SIZE  # D < 2 Hd + 1 = 11
    assert _create(11, 600) in ok
    assert _create((1 << 20) + 1, 8) == L.ERR_INVALID_SIZE
    assert _create(1 << 20, 8) in ok
    assert _create(64, 0) == L.ERR_INVALID_SIZE
    assert _create(64, 1 << 31) == L.ERR_INVALID_SIZE
    assert _create(64, 600, max_maps=0) == L.ERR_INVALID_SIZE
    assert _create(64, 1 << 20, max_maps=1 << 14) == L.ERR_INVALID_SIZE  # maps D R = 2^40
    assert _create(64, 1 << 20, max_maps=1 << 60) == L.ERR_INVALID_SIZE
    for edge in (-1, 2):
        assert _create(64, 600, edge=edge) == L.ERR_INVALID_ARG
    for precision in (-1, L.F32_F64STATE, 3):
        assert _create(64, 600, precision=precision) == L.ERR_INVALID_ARG
    table = np.ones(600)
    assert _create(64, 600, scale=table) in ok
    for bad in (np.nan, np.inf, -np.inf):
        t = table.copy()
        t[17] = bad
        for precision in (L.F32, L.F64):
            assert _create(64, 600, precision=precision, scale=t) == L.ERR_INVALID_ARG
    t = table.copy()
    t[5] = 1e300  # finite in double, infinite once rounded to float
    assert _create(64, 600, precision=L.F32, scale=t) == L.ERR_INVALID_ARG
    assert _create(64, 600, precision=L.F64, scale=t) in ok
    # the designer
    lib = sd.load()
    out = np.zeros(600)
    d = _desc((4, 1, 8, 2))
    for pfa in (0.0, 1.0, -0.1, 2.0, np.nan):
        assert lib.sdsp_hip_cfar2d_scale(64, 600, C.byref(d), pfa, out.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar2d_scale(64, 600, C.byref(d), 1e-3, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar2d_scale(64, 600, None, 1e-3, out.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar2d_scale(10, 600, C.byref(d), 1e-3, out.ctypes.data) == L.ERR_INVALID_SIZE
    # the null-plan forms of the other entries
    n = C.c_uint64(0)
    assert lib.sdsp_hip_cfar2d_plan_destroy(None) == L.OK
    assert lib.sdsp_hip_cfar2d_process(None, None, None, None, None, None, 0, 1, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar2d_process_host(None, None, None, None, None, None, 0, 1) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar2d_plan_set_alpha(None, 1.0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar2d_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar2d_plan_launches(None, 1, 1, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cfar2d_plan_get_info(None, None) == L.ERR_INVALID_ARG


def test_python_layer_validates_and_needs_a_device():
    count = C.c_int(0)
    have = sd.load().sdsp_hip_device_count(C.byref(count)) == L.OK and count.value > 0
    if not have:
        with pytest.raises(sd.SdspHipError) as e:
            sd.cfar2d_plan(64, 600, (4, 8), (1, 2), alpha=3.0)
        assert e.value.code == L.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        sd.cfar2d_plan(64, 600, (4, 8), (1, 2))  # neither alpha nor pfa nor scale
    with pytest.raises(ValueError):
        sd.cfar2d_plan(64, 600, (4, 8), (1, 2), alpha=1.0, pfa=1e-3)
    with pytest.raises(ValueError):
        sd.cfar2d_plan(64, 600, (4, 8), (1, 2), alpha=1.0, edge="wrap")
    with pytest.raises(ValueError):
        sd.cfar2d_plan(64, 600, 4, (1, 2), alpha=1.0)
    with pytest.raises(ValueError):
        sd.cfar2d_plan(64, 600, (4, 8), (1, 2), scale=np.ones(599))
