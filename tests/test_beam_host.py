"""CPU checks of the time-delay beamformer bank (include/sdsp_hip.h: sdsp_hip_beam_*): the numpy reference the
GPU tests use (tests/beam_ref.py) against scipy.signal.lfilter, the host tap designer against the contract's formula in numpy, the
quality of the designed fractional delays, a steered line array against its analytic response, and argument checking without a
device."""
import ctypes as C

import numpy as np
import pytest

from beam_ref import BLOCKS, beam_ref, delay_taps_formula, hist_len, response

import simpledsp_amd as sd
from simpledsp_amd import _lib as L

# worst |H(f) - e^(-2 pi i f (mu + c0))| of the contract's formula over mu = k / 64 and 301 frequencies in [0, fmax], measured with numpy:
#   (T, beta) = (16, 8), f <= 0.3: 4.62e-4 (2.65e-4 at f = 0.2);   (32, 8), f <= 0.4: 2.33e-4
DESIGN_ERROR = {(16, 8.0, 0.3): 4.7e-4, (32, 8.0, 0.4): 2.4e-4}


def _formula_error(n_taps, beta, fmax, taps_of):
    f = np.linspace(0.0, fmax, 301)
    c0 = (n_taps - 1) // 2
    worst = 0.0
    for mu in np.arange(64) / 64.0:
        worst = max(worst, np.abs(response(taps_of(mu), f) - np.exp(-2j * np.pi * f * (mu + c0))).max())
    return worst


@pytest.mark.parametrize("cplx", [False, True])
def test_reference_is_a_sum_of_delayed_lfilters(cplx):
    """beam_ref in f64 against sum over entries of scipy.signal.lfilter(taps, 1, delayed x): rounding only, a few hundred terms"""
    import scipy.signal
    rng = np.random.default_rng(5)
    groups, sensors, beams, n_taps, S = 2, 8, 3, 33, 800
    ent = []
    for b in range(beams):
        for c in range(sensors):
            g = rng.standard_normal(n_taps) + (1j * rng.standard_normal(n_taps) if cplx else 0)
            ent.append((b, c, int(rng.integers(0, 60)), g))
    H = hist_len(ent, n_taps)
    x = rng.standard_normal((groups * sensors, S)) + (1j * rng.standard_normal((groups * sensors, S)) if cplx else 0)
    hist = rng.standard_normal((groups * sensors, H)) + (1j * rng.standard_normal((groups * sensors, H)) if cplx else 0)
    got, state = beam_ref(ent, x, sensors, beams, n_taps, groups, hist, "f64")
    ext = np.concatenate([hist[:, ::-1], x], axis=1)
    want = np.zeros_like(got)
    for grp in range(groups):
        for b, c, d, g in ent:
            full = scipy.signal.lfilter(g, 1.0, ext[grp * sensors + c])  # the stream from its history on
            want[grp * beams + b] += full[H - d:H - d + S]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(state, ext[:, ::-1][:, :H])
    # any split into calls gives the same bits and the same final state
    st, parts = hist, []
    for s0, n in zip(np.cumsum([0] + [31 * v for v in BLOCKS[:-1]]), [31 * v for v in BLOCKS]):
        y, st = beam_ref(ent, x[:, s0:s0 + n], sensors, beams, n_taps, groups, st, "f64")
        parts.append(y)
    total = 31 * sum(BLOCKS)
    assert np.concatenate(parts, axis=1).tobytes() == np.ascontiguousarray(got[:, :total]).tobytes()
    assert st.tobytes() == beam_ref(ent, x[:, :total], sensors, beams, n_taps, groups, hist, "f64")[1].tobytes()


def test_designer_matches_the_formula():
    rng = np.random.default_rng(6)
    for n_taps, beta in [(2, 0.0), (5, 3.0), (16, 8.0), (32, 8.0), (33, 12.5), (256, 8.0)]:
        for tau in [0.0, 0.5, 7.25, 65534.999, *rng.uniform(0, 300, 6)]:
            for weight in (1.0, -0.37):
                d, g = delay_taps_formula(tau, weight, n_taps, beta)
                delays, taps = sd.beam_delay_taps(np.array([tau]), weight, n_taps, beta)
                assert delays[0] == d
                assert np.abs(taps[0] - g).max() <= 1e-12 * np.abs(g).max(), (n_taps, beta, tau)
                assert abs(taps[0].sum() - weight) <= 1e-12
    # one tap: the nearest whole sample and the bare weight
    for tau, d in [(0.0, 0), (0.49, 0), (0.5, 1), (7.5, 8), (7.25, 7)]:
        delays, taps = sd.beam_delay_taps(np.array([tau]), 0.75, 1, 8.0)
        assert delays[0] == d and taps[0, 0] == 0.75
    # arrays keep their shape
    delays, taps = sd.beam_delay_taps(rng.uniform(0, 9, (3, 4)), rng.standard_normal((3, 4)), 16, 8.0)
    assert delays.shape == (3, 4) and taps.shape == (3, 4, 16)


@pytest.mark.parametrize("n_taps,beta,fmax", sorted(DESIGN_ERROR))
def test_designed_delays_are_as_good_as_the_formula(n_taps, beta, fmax):
    """the library's taps stay within 2 x the error of the formula evaluated with numpy (the factor covers only I0-series and rounding
    differences), and that error is the one written down above"""
    formula = _formula_error(n_taps, beta, fmax, lambda mu: delay_taps_formula(mu, 1.0, n_taps, beta)[1])
    library = _formula_error(n_taps, beta, fmax, lambda mu: sd.beam_delay_taps(np.array([mu]), 1.0, n_taps, beta)[1][0])
    print(f"T = {n_taps}, beta = {beta}, f <= {fmax}: formula {formula:.3e}, library {library:.3e}")
    assert formula <= DESIGN_ERROR[(n_taps, beta, fmax)]
    assert library <= 2 * formula


def test_steered_line_array_matches_its_analytic_response():
    """8 sensors on a line, a tone at 0.2 cycles per sample arriving as a plane wave with a fractional delay from sensor to sensor; one
    beam on the source and one off it.  Past the history the output is sum w_c e^(2 pi i f (n - c0 - a_c - tau_bc)) to within
    sum |w_c| x (the design error) + 1e-12"""
    n_taps, beta, f, sensors = 16, 8.0, 0.2, 8
    c0 = (n_taps - 1) // 2
    pos = np.arange(sensors)[:, None] * np.array([[0.5, 0.0]])
    speed, fs = 1.0, 3.3  # 1.65 samples from sensor to sensor along the line
    ang = np.deg2rad([40.0, 100.0])
    u = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    tau = sd.plane_wave_delays(pos, u, speed, fs)
    assert tau.shape == (2, sensors) and tau.min() == 0.0
    assert np.allclose(tau[0] - tau[0, 0], -np.arange(sensors) * 0.5 * np.cos(ang[0]) * fs)
    assert np.any(np.abs(tau - np.round(tau)) > 0.1)
    arrive = (pos @ u[0]) / speed * fs  # the source lies against u[0]: beam 0 is on it
    w = np.hamming(sensors) / np.hamming(sensors).sum() * np.ones((2, 1))
    delays, taps = sd.beam_delay_taps(tau, w, n_taps, beta)
    ent = [(b, c, int(delays[b, c]), taps[b, c]) for b in range(2) for c in range(sensors)]
    H = hist_len(ent, n_taps)
    S = H + 400
    n = np.arange(S)
    x = np.exp(2j * np.pi * f * (n[None, :] - arrive[:, None]))
    y, _ = beam_ref(ent, x, sensors, 2, n_taps, 1, None, "f64")
    bound = np.abs(w[0]).sum() * DESIGN_ERROR[(16, 8.0, 0.3)] + 1e-12
    for b in range(2):
        ideal = (w[b][:, None] * np.exp(2j * np.pi * f * (n[None, :] - c0 - arrive[:, None] - tau[b][:, None]))).sum(axis=0)
        assert np.abs(y[b, H:] - ideal[H:]).max() <= bound, b
    on, off = np.abs(y[0, H:]).mean(), np.abs(y[1, H:]).mean()
    assert abs(on - 1.0) <= bound and off < 0.25  # the beam on the source adds coherently (sum w = 1), the other does not


def test_argument_checking_of_the_designer_and_the_delays():
    lib = sd.load()
    g = np.zeros(256)
    d = C.c_uint32(0)
    design = lambda tau, w, n, beta: lib.sdsp_hip_beam_delay_taps(tau, w, n, beta, C.byref(d), g.ctypes.data)  # noqa: E731
    assert design(1.5, 1.0, 16, 8.0) == 0 and d.value == 1
    assert design(65534.5, 1.0, 16, 8.0) == 0 and d.value == 65534
    for bad in (-0.001, 65535.0, 1e9, float("nan"), float("inf")):
        assert design(bad, 1.0, 16, 8.0) == L.ERR_INVALID_ARG, bad
    assert design(1.5, float("nan"), 16, 8.0) == L.ERR_INVALID_ARG and design(1.5, float("inf"), 16, 8.0) == L.ERR_INVALID_ARG
    assert design(1.5, 1.0, 16, float("nan")) == L.ERR_INVALID_ARG and design(1.5, 1.0, 16, -1.0) == L.ERR_INVALID_ARG
    assert design(1.5, 1.0, 0, 8.0) == L.ERR_INVALID_SIZE and design(1.5, 1.0, 257, 8.0) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_beam_delay_taps(1.5, 1.0, 16, 8.0, None, g.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_beam_delay_taps(1.5, 1.0, 16, 8.0, C.byref(d), None) == L.ERR_INVALID_ARG
    with pytest.raises(sd.SdspHipError):
        sd.beam_delay_taps(np.array([-1.0]), 1.0, 16, 8.0)
    pos = np.zeros((4, 2))
    with pytest.raises(ValueError):
        sd.plane_wave_delays(pos, np.ones((2, 3)), 1.0, 1.0)  # dims differ
    with pytest.raises(ValueError):
        sd.plane_wave_delays(pos, np.ones((2, 2)), 0.0, 1.0)
    with pytest.raises(ValueError):
        sd.plane_wave_delays(pos, np.ones((2, 2)), 1.0, float("nan"))
    with pytest.raises(ValueError):
        sd.plane_wave_delays(np.full((4, 2), np.inf), np.ones((2, 2)), 1.0, 1.0)
    with pytest.raises(ValueError):
        sd.plane_wave_delays(np.zeros((0, 2)), np.ones((2, 2)), 1.0, 1.0)
    assert sd.plane_wave_delays(np.arange(4.0), np.array([1.0, -1.0]), 2.0, 4.0).tolist() == [[6.0, 4.0, 2.0, 0.0], [6.0, 8.0, 10.0, 12.0]]


def test_plan_creation_checks_its_arguments_before_it_needs_a_device():
    import torch
    lib = sd.load()
    g = np.ones(3 * 16 * 2)
    ent = (L.BeamEntry * 3)(L.BeamEntry(0, 0, 0), L.BeamEntry(0, 1, 5), L.BeamEntry(1, 1, 9))
    p = C.c_void_p()

    def create(sensors=2, beams=2, groups=1, taps=16, n=3, e=ent, taps_ptr=g.ctypes.data, kind=L.BEAM_COMPLEX, precision=L.F64):
        return lib.sdsp_hip_beam_plan_create(C.byref(p), sensors, beams, groups, taps, n, e, taps_ptr, kind, precision, 0)

    assert create(sensors=0) == L.ERR_INVALID_SIZE and create(beams=4097) == L.ERR_INVALID_SIZE
    assert create(groups=0) == L.ERR_INVALID_SIZE and create(taps=257) == L.ERR_INVALID_SIZE and create(taps=0) == L.ERR_INVALID_SIZE
    assert create(n=(1 << 20) + 1) == L.ERR_INVALID_SIZE
    assert create(e=None) == L.ERR_INVALID_ARG and create(taps_ptr=None) == L.ERR_INVALID_ARG
    assert create(kind=7) == L.ERR_INVALID_ARG and create(precision=L.F32_F64STATE) == L.ERR_INVALID_ARG
    assert create(sensors=1) == L.ERR_INVALID_ARG and create(beams=1) == L.ERR_INVALID_ARG
    assert create(e=(L.BeamEntry * 3)(L.BeamEntry(0, 0, 65536), L.BeamEntry(0, 1, 5), L.BeamEntry(1, 1, 9))) == L.ERR_INVALID_SIZE
    assert create(e=(L.BeamEntry * 3)(L.BeamEntry(0, 1, 0), L.BeamEntry(0, 1, 5), L.BeamEntry(1, 1, 9))) == L.ERR_INVALID_ARG
    assert create(e=(L.BeamEntry * 3)(L.BeamEntry(1, 0, 0), L.BeamEntry(0, 1, 5), L.BeamEntry(1, 1, 9))) == L.ERR_INVALID_ARG
    rc = create()
    if torch.cuda.is_available():
        assert rc == 0
        lib.sdsp_hip_beam_plan_destroy(p)
    else:
        assert rc == L.ERR_NO_DEVICE
        with pytest.raises(sd.SdspHipError):  # no CPU path
            b = sd.beamformer_bank(2, 2, 16)
            b.set_dense(np.zeros((2, 2), dtype=int), np.ones((2, 2, 16)))
            b.info()
