"""Host tests of the polyphase synthesis banks (sdsp_hip_pfb_synth_*): the dual-prototype helper, the double
reference tests/pfb_synth_ref.py against the analysis reference tests/pfb_ref.py and the inverse STFT reference, and every argument
error that is detectable without a device.  The tests of the two limits and of the block split pin the reference itself (numpy
against tests/istft_ref.py and against itself), not the library: they are what lets the GPU tests trust it."""
import ctypes as C

import numpy as np
import pytest

import simpledsp_amd as sd
from istft_ref import istft_ref
from pfb_ref import pfb_ref
from pfb_synth_ref import dual_systems, pfb_synth_ref

L = sd._lib

SHAPES = [(16, 4, 8, "hamming"), (16, 4, 5, "hamming"), (16, 4, 1, "hamming"), (64, 3, 16, "blackman"), (32, 8, 16, "hamming"),
          (16, 1, 16, "hamming"), (16, 1, 4, "hann")]
REFUSED = [(16, 4, 12), (16, 4, 16), (32, 8, 24)]


def _signal(rng, n, cplx):
    x = rng.standard_normal(n)
    return x + 1j * rng.standard_normal(n) if cplx else x


@pytest.mark.parametrize("m,p,hop,window", SHAPES)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("phase", ["frame", "time"])
def test_round_trip_is_the_delayed_signal(m, p, hop, window, cplx, phase):
    rng = np.random.default_rng(m + p + hop)
    Lt, H = m * p, m * p - hop
    h = sd.pfb_prototype(window, m, p)
    g = sd.pfb_dual_prototype(h, m, p, hop)
    F = 3 * Lt // hop + 7
    x = _signal(rng, (2, F * hop), cplx)
    Y, _ = pfb_ref(x, m, p, hop, h, None, phase, 0)
    y, _ = pfb_synth_ref(Y, m, p, hop, g, None, phase, 0, cplx=cplx)
    want = np.concatenate([np.zeros((2, H), dtype=x.dtype), x], axis=1)[:, :F * hop]
    err = np.abs(y - want).max() / np.abs(x).max()
    print(f"round trip M={m} P={p} D={hop} {window} {'complex' if cplx else 'real'} {phase}: err {err:.3e}")
    assert err <= 1e-11
    if not cplx:
        assert not np.iscomplexobj(y)


@pytest.mark.parametrize("m,p,hop,window", SHAPES)
def test_helper_equals_lstsq_per_residue(m, p, hop, window):
    h = sd.pfb_prototype(window, m, p)
    g = sd.pfb_dual_prototype(h, m, p, hop)
    want = np.zeros(m * p)
    worst_cond = 0.0
    for idx, A, b in dual_systems(h, m, p, hop):
        want[idx] = np.linalg.lstsq(A, b, rcond=None)[0]
        assert np.abs(A @ g[idx] - b).max() <= 1e-9
        worst_cond = max(worst_cond, np.linalg.cond(A))
    assert worst_cond <= 2e5
    assert np.abs(g - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("m,p,hop", REFUSED)
def test_helper_refuses_a_prototype_without_a_dual(m, p, hop):
    h = sd.pfb_prototype("hamming", m, p)
    with pytest.raises(sd.SdspHipError) as e:
        sd.pfb_dual_prototype(h, m, p, hop)
    assert e.value.code == L.ERR_INVALID_ARG
    resid = max(np.abs(A @ np.linalg.lstsq(A, b, rcond=None)[0] - b).max() for _, A, b in dual_systems(h, m, p, hop))
    assert resid >= 5e-4  # far from the 1e-9 line: the refusal does not hang on rounding


def test_the_badly_conditioned_oversampled_hamming_prototype():
    """(256, 8, 128): condition number 1.2e8 -- normal equations would lose all sixteen digits; the helper's residual stays tiny"""
    m, p, hop = 256, 8, 128
    h = sd.pfb_prototype("hamming", m, p)
    g = sd.pfb_dual_prototype(h, m, p, hop)
    assert max(np.abs(A @ g[idx] - b).max() for idx, A, b in dual_systems(h, m, p, hop)) <= 1e-9


@pytest.mark.parametrize("hop", [32, 16, 24, 5])
def test_one_tap_per_channel_frame_real_is_the_raw_inverse_stft(hop):
    m, F = 32, 9
    rng = np.random.default_rng(hop)
    g = rng.uniform(-1, 1, m)
    X = rng.standard_normal((3, F, m // 2 + 1)) + 1j * rng.standard_normal((3, F, m // 2 + 1))
    pend = rng.standard_normal((3, m - hop))
    y, st = pfb_synth_ref(X, m, 1, hop, g, pend, "frame", 0)
    y2, st2 = istft_ref(X, m, hop, g, pend)
    assert np.array_equal(y, y2) and np.array_equal(st, st2)


def test_one_tap_per_channel_at_the_critical_hop_is_the_reverse_transform_times_g():
    m, F = 16, 5
    rng = np.random.default_rng(1)
    g = rng.uniform(-1, 1, m)
    X = rng.standard_normal((2, F, m)) + 1j * rng.standard_normal((2, F, m))
    y, st = pfb_synth_ref(X, m, 1, m, g, None, "frame", 0)
    assert st.shape == (2, 0)
    assert np.array_equal(y, (np.fft.ifft(X, axis=-1) * g).reshape(2, F * m))


@pytest.mark.parametrize("m,p,hop", [(16, 4, 8), (16, 4, 5), (16, 2, 16), (32, 3, 1)])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("phase", ["frame", "time"])
def test_reference_is_block_split_invariant(m, p, hop, cplx, phase):
    rng = np.random.default_rng(m * p + hop)
    bins = m if cplx else m // 2 + 1
    blocks = [1, 3, 0, 2, 2 * (m * p // hop) + 1, 1]  # F D < hist, an empty one, past the history
    F = sum(blocks)
    X = rng.standard_normal((2, F, bins)) + 1j * rng.standard_normal((2, F, bins))
    g = rng.uniform(-1, 1, m * p)
    pend0 = rng.standard_normal((2, m * p - hop)) * (1 + 1j if cplx else 1)
    want, want_state = pfb_synth_ref(X, m, p, hop, g, pend0, phase, 7, cplx=cplx)
    outs, pend, at, pos = [], pend0, 0, 7
    for n in blocks:
        y, pend = pfb_synth_ref(X[:, at:at + n], m, p, hop, g, pend, phase, pos, cplx=cplx)
        outs.append(y)
        at += n
        pos += n * hop
    assert np.array_equal(np.concatenate(outs, axis=1), want) and np.array_equal(pend, want_state)


def test_helper_argument_errors():
    lib = sd.load()
    h = np.ones(64)
    g = np.zeros(64)

    def call(m=16, p=4, hop=8, hp=h.ctypes.data, gp=g.ctypes.data):
        return lib.sdsp_hip_pfb_dual_prototype(m, p, hop, hp, gp)

    assert call(hp=None) == L.ERR_INVALID_ARG
    assert call(gp=None) == L.ERR_INVALID_ARG
    assert call(m=1, p=4) == L.ERR_INVALID_SIZE
    assert call(p=0) == L.ERR_INVALID_SIZE
    assert call(p=L.PFB_MAX_TAPS_PER_CHANNEL + 1) == L.ERR_INVALID_SIZE
    assert call(m=1 << 19, p=4) == L.ERR_INVALID_SIZE  # p m > SDSP_HIP_PFB_MAX_TAPS
    assert call(hop=0) == L.ERR_INVALID_SIZE
    assert call(hop=17) == L.ERR_INVALID_SIZE
    assert call(hop=16) == L.ERR_INVALID_ARG  # all-ones prototype, critically sampled with P = 4: no dual
    assert b"dual" in lib.sdsp_hip_last_error_string()
    assert call(m=16, p=1, hop=16) == 0 and np.array_equal(g[:16], np.ones(16))
    with pytest.raises(ValueError):
        sd.pfb_dual_prototype(np.ones(63), 16, 4, 8)


def test_plan_create_argument_errors():
    lib = sd.load()
    taps = np.ones(64 * 4)
    plan = C.c_void_p()

    def create(m=64, p=4, hop=32, tp=taps.ctypes.data, kind=L.PFB_REAL, phase=L.PFB_PHASE_TIME, precision=L.F32, out=C.byref(plan)):
        return lib.sdsp_hip_pfb_synth_plan_create(out, m, p, hop, tp, kind, phase, precision, 0, 0)

    assert create(out=None) == L.ERR_INVALID_ARG
    assert create(m=48) == L.ERR_INVALID_SIZE
    assert create(m=0) == L.ERR_INVALID_SIZE
    assert create(p=0) == L.ERR_INVALID_SIZE
    assert create(p=L.PFB_MAX_TAPS_PER_CHANNEL + 1) == L.ERR_INVALID_SIZE
    assert create(m=1 << 16, p=32) == L.ERR_INVALID_SIZE  # p m > SDSP_HIP_PFB_MAX_TAPS
    assert create(hop=0) == L.ERR_INVALID_SIZE
    assert create(hop=65) == L.ERR_INVALID_SIZE
    assert create(tp=None) == L.ERR_INVALID_ARG
    assert create(precision=7) == L.ERR_INVALID_ARG
    assert create(precision=L.F32_F64STATE) == L.ERR_INVALID_ARG
    assert create(kind=2) == L.ERR_INVALID_ARG
    assert create(phase=2) == L.ERR_INVALID_ARG
    assert create(m=16, hop=8) == L.ERR_UNSUPPORTED  # the real-input plans start at 32
    assert create(m=8, hop=8, kind=L.PFB_COMPLEX) == L.ERR_UNSUPPORTED
    assert create(m=1 << 16, p=1, hop=1 << 16, precision=L.F64) == L.ERR_UNSUPPORTED
    assert create(m=1 << 17, p=1, hop=1 << 17) == L.ERR_UNSUPPORTED
    assert plan.value is None
    n = C.c_uint64(0)
    assert lib.sdsp_hip_pfb_synth_state_bytes(None, 1, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_synth_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_synth_plan_set_unfold_form(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_synth_plan_launches(None, 1, 1, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_synth_plan_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_synth_plan_destroy(None) == 0
    assert lib.sdsp_hip_pfb_synth_process(None, None, 0, None, 0, 1, 1, 0, None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_pfb_synth_process_host(None, None, 0, None, 0, 1, 1, 0, None) == L.ERR_INVALID_ARG


def test_python_argument_errors():
    with pytest.raises(ValueError):
        sd.pfb_synthesis_bank(64, 4, 32, output="imaginary")
    with pytest.raises(ValueError):
        sd.pfb_synthesis_bank(64, 4, 32, phase="sample")
    with pytest.raises(ValueError):
        sd.pfb_synthesis_bank(64, 4, 65)
    with pytest.raises(ValueError):
        sd.pfb_synthesis_bank(64, 4, 32, streams=0)
    with pytest.raises(ValueError):
        sd.pfb_synthesis_bank(64, 4, 32, taps=np.ones(255))
    with pytest.raises(sd.SdspHipError):
        sd.pfb_synthesis_bank(16, 4, 12, taps="hamming", output="complex")  # a window name without a dual at this hop
    b = sd.pfb_synthesis_bank(64, 3, 16, taps="blackman")
    assert b.hist == 176 and b.bins == 33 and b.taps.shape == (192,) and b.position == 0 and b.state is None
