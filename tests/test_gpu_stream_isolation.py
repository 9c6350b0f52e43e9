"""Framed buffers, offset pointers and slice-edge NaNs for the six streaming banks that frame -> transform -> emit / overlap-add
(stft, istft, welch, csd, pfb, pfb_synth) and the carried-state kernels they share (stream_carry.hip), on a real MI355X.

Every bank goes through the C entries with data_ptr()s, so that every buffer of a call can be a view into an arena of its own
(tests/arena.py: Buffers, check_framed_bank, check_poisoned_bank; tests/test_arena_host.py shows with planted defects that those
checks fail when they should).  Per bank, precision and kind:
  1. the clean result, in ordinary exactly-sized tensors, is held to the bank's numpy reference within the tolerance of the bank's own
     GPU test file (imported from there); everything after that is bit equality with, or a NaN mask over, that clean result;
  2. in, out, state and the accumulators framed at once, under LAYOUTS: leads of 0, 1, 2 elements past a 512-byte base, exact / odd /
     16-byte-keeping row strides, and three layouts with a single pointer off.  test_every_alignment_switch_is_taken_both_ways computes
     from the launchers' own conditions which layout sends which kernel down its vector path and which down its element path;
  3. the stream as two calls against the same framed state -- the first short (the in-place shift / seed of stream_carry.hip, two
     chunks at hist = 448 or 511), the second of at least hist (the flat path) -- and once with state = NULL;
  4. one NaN input element next to every kind of slice edge: in the last frame of a slice and the first of the next inside one
     channel, in the last frame of a channel and the first of the next inside one slice, in the first and the last sample.

Shapes: n_fft / m in {32, 512}, 3 to 5 channels, 9 to 11 frames per call; a hop off the vector width (3) where the bank takes one."""
import numpy as np
import pytest
import scipy.signal
import torch

import arena
from conftest import rel_max_err
from csd_ref import PAIRS, csd_density, csd_ref
from istft_ref import istft_ref
from pfb_ref import pfb_ref
from pfb_synth_ref import pfb_synth_frames_ref, pfb_synth_ref
from stft_ref import stft_ref
from test_gpu_csd import _peak_err as csd_err, _tol as csd_tol
from test_gpu_istft import _tol as istft_tol
from test_gpu_pfb import _err as pfb_err, _tol as pfb_tol
from test_gpu_pfb_synth import _bound as synth_bound
from test_gpu_stft import _tol as stft_tol
from test_gpu_welch import _peak_err as welch_err, _tol as welch_tol
from welch_ref import welch_frames, welch_psd, welch_ref

pytestmark = pytest.mark.gpu

EPS64 = np.finfo(np.float64).eps
SMALL = 7  # units per slice of the small workspaces: with 9, 10 or 11 frames per channel a slice starts inside channel 0 (unit 7) and
#            channel 1 starts inside the slice [7, 14)
CSD_COLS = 3  # the CSD bank slices by segment columns of all channels: [0, 3) [3, 6) [6, 9) [9, ..)


@pytest.fixture(scope="module")
def sd():
    import simpledsp_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    simpledsp_amd.load(build_if_missing=True)
    return simpledsp_amd


def _rdt(prec):
    return torch.float64 if prec == "f64" else torch.float32


def _cdt(prec):
    return torch.complex128 if prec == "f64" else torch.complex64


def _rs(prec):
    return 8 if prec == "f64" else 4


def _rand(rng, shape, dtype):
    x = rng.standard_normal(shape)
    if dtype.is_complex:
        x = x + 1j * rng.standard_normal(shape)
    return torch.from_numpy(x).to(dtype)


# ------------------------------------------------------------------ the cases

# (n_fft or m, hop, channels, frames, first call of the two): hop 3 is off every vector width and puts the history / block seam (hist =
# 29 or 93) inside a 16-byte lane group; 512 / 64 has hist = 448 (511 for welch and csd), above 256 and no multiple of it, so the
# in-place shift and seed walk two chunks, and its first call (2 frames = 128 samples; 200 samples) is below hist - 256
SHAPES = {"n32h3": (32, 3, 5, 11, 2), "n32h8": (32, 8, 3, 9, 2), "n512h64": (512, 64, 3, 10, 2)}
# taps per channel and phase of the two polyphase banks per shape; pfb_synth adds hop = m, the only hop its sliding form takes
PFB = {"n32h3": (3, "time"), "n32h8": (1, "frame"), "n512h64": (1, "time"), "n32h32": (2, "time")}
SYNTH_SHAPES = dict(SHAPES, n32h32=(32, 32, 3, 9, 2))
VARIANTS = {"stft": ("complex", "power"), "istft": ("real",), "welch": ("real",), "csd": ("real",), "pfb": ("real", "complex"),
            "pfb_synth": ("real", "complex")}


def _frames(kind, shape):
    """welch and csd have hist = 511 at n = 512: twelve segments, so that the second of the two calls still has hist samples"""
    return 12 if kind in ("welch", "csd") and shape == "n512h64" else SYNTH_SHAPES[shape][3]


def _cases():
    """every bank takes every shape: no hop is refused (welch, csd and the polyphase banks take any 1 <= hop <= n) and no pointer that
    is a whole number of elements past its buffer's natural alignment is (the C entries refuse only pointers that are not a multiple
    of the element size, which test_errors_* of each bank asserts already)"""
    out = []
    for kind, variants in VARIANTS.items():
        for shape in (SYNTH_SHAPES if kind == "pfb_synth" else SHAPES):
            for var in variants:
                for prec in ("f32", "f64"):
                    out.append(pytest.param(kind, shape, var, prec, id=f"{kind}-{shape}-{var}-{prec}"))
    return out


class _Bank:
    """the bank protocol of arena.check_framed_bank over one C entry"""

    def __init__(self, sd, kind, shape, var, prec, ws="one"):
        self.sd, self.lib, self.kind, self.var, self.prec = sd, sd.load(), kind, var, prec
        self.n, self.hop, self.C, _, self.first = SYNTH_SHAPES[shape]
        self.F = _frames(kind, shape)
        self.shape = shape
        self.rng = np.random.default_rng(sum(map(ord, f"{kind}{shape}{var}{prec}")))
        self.rdt, self.cdt, self.rs = _rdt(prec), _cdt(prec), _rs(prec)
        self.setup()
        # ws: "default" (0: the plan's own budget), units per slice, or "one": a workspace of exactly the call's units -- the single
        # slice the default budget gives for these shapes, without its 256 MiB allocation
        self.bank = self.make(0 if ws == "default" else (self.units() if ws == "one" else ws) * self.unit_bytes)
        self.bank._ensure_plan()
        self.plan = self.bank._plan
        self.per_slice = self.bank.info()["workspace_bytes"] // self.unit_bytes

    def bank_prec(self):
        return self.sd.F64 if self.prec == "f64" else self.sd.F32

    def units(self):
        return self.C * self.F

    def spec(self, init=None, shape=None, dtype=None, **kw):
        return dict(shape=tuple(init.shape) if init is not None else shape, dtype=init.dtype if init is not None else dtype, init=init, **kw)

    def poisons(self):
        """(label, row, col) of in: next to the slice and channel edges of a call in slices of SMALL units, first and last sample"""
        edges = arena.edge_units(self.C, self.F, SMALL)
        cols = self.specs()["in"]["shape"][1]
        return [(label, c, self.element_of(j)) for label, c, j in edges] + [("channel 0, sample 0", 0, 0),
                                                                            ("last channel, last sample", self.C - 1, cols - 1)]

    def frames_mask(self, row, covered, rows, per_frame):
        """(rows, F per_frame) mask: the frames of `row` for which covered(j)"""
        m = torch.zeros((rows, self.F, per_frame), dtype=torch.bool)
        for j in range(self.F):
            m[row, j] = bool(covered(j))
        return m.reshape(rows, -1)

    def history_mask(self, row, col, samples, hist):
        """newest first: state[row, k] = in[row, samples - 1 - k]"""
        m = torch.zeros((self.C, hist), dtype=torch.bool)
        if samples - 1 - col < hist:
            m[row, samples - 1 - col] = True
        return m

    def span_masks(self, row, t0, length, samples, hist):
        """overlap-add: positions [t0, t0 + length) of `row`, the first `samples` in out and the rest in the pending sums"""
        t = torch.arange(samples + hist)
        hit = (t >= t0) & (t < t0 + length)
        out = torch.zeros((self.C, samples), dtype=torch.bool)
        state = torch.zeros((self.C, hist), dtype=torch.bool)
        out[row], state[row] = hit[:samples], hit[samples:]
        return {"out": out, "state": state}


class Stft(_Bank):
    def setup(self):
        self.bins, self.H, self.ticks = self.n // 2 + 1, self.n - self.hop, self.F
        self.unit_bytes = self.n * self.rs
        self.w = scipy.signal.get_window("hann", self.n)
        self.x = _rand(self.rng, (self.C, self.F * self.hop), self.rdt)
        self.hist0 = _rand(self.rng, (self.C, self.H), self.rdt)
        self.odt = self.cdt if self.var == "complex" else self.rdt

    def make(self, workspace):
        return self.sd.stft_bank(self.n, self.hop, self.C, window=self.w, output=self.var, precision=self.bank_prec(), workspace_bytes=workspace)

    def specs(self, null_state=False):
        s = {"in": self.spec(self.x, read_only=True), "out": self.spec(shape=(self.C, self.F * self.bins), dtype=self.odt)}
        if not null_state:
            s["state"] = self.spec(self.hist0, strided=False)
        return s

    def run(self, b, t0, t1):
        rc = self.lib.sdsp_hip_stft_process(self.plan, b.ptr("in", t0 * self.hop), b.stride("in"), b.ptr("out", t0 * self.bins), b.stride("out"),
                                            self.C, (t1 - t0) * self.hop, b.ptr("state"), None)
        assert rc == 0, rc

    def launches(self):
        return self.bank.launches(self.F * self.hop)

    def reference(self, clean, null_state=False):
        hist = None if null_state else self.hist0.numpy()
        want, state = stft_ref(self.x.numpy(), self.n, self.hop, self.w, hist, self.var)
        got = clean["out"].cpu().numpy().reshape(want.shape)
        if not null_state:
            assert np.array_equal(clean["state"].cpu().numpy(), state.astype(self.x.numpy().dtype))
        return rel_max_err(got, want), stft_tol(self.prec, self.n, self.var)

    def element_of(self, j):
        return j * self.hop + self.hop - 1  # the newest sample of frame j

    def masks(self, row, col):
        p = col + self.H
        return {"out": self.frames_mask(row, lambda j: j * self.hop <= p < j * self.hop + self.n, self.C, self.bins),
                "state": self.history_mask(row, col, self.F * self.hop, self.H)}


class Istft(_Bank):
    def setup(self):
        self.bins, self.H, self.ticks = self.n // 2 + 1, self.n - self.hop, self.F
        self.unit_bytes = self.n * self.rs
        self.w = scipy.signal.get_window("hann", self.n)
        self.X = _rand(self.rng, (self.C, self.F * self.bins), self.cdt)
        self.pend = _rand(self.rng, (self.C, self.H), self.rdt)

    def make(self, workspace):
        return self.sd.istft_bank(self.n, self.hop, self.C, window=self.w, precision=self.bank_prec(), workspace_bytes=workspace)

    def specs(self, null_state=False):
        s = {"in": self.spec(self.X, read_only=True), "out": self.spec(shape=(self.C, self.F * self.hop), dtype=self.rdt)}
        if not null_state:
            s["state"] = self.spec(self.pend, strided=False)
        return s

    def run(self, b, t0, t1):
        rc = self.lib.sdsp_hip_istft_process(self.plan, b.ptr("in", t0 * self.bins), b.stride("in"), b.ptr("out", t0 * self.hop), b.stride("out"),
                                             self.C, t1 - t0, b.ptr("state"), None)
        assert rc == 0, rc

    def launches(self):
        return self.bank.launches(self.F)

    def reference(self, clean, null_state=False):
        X3 = self.X.numpy().reshape(self.C, self.F, self.bins)
        want, state = istft_ref(X3, self.n, self.hop, self.bank.synthesis_window, None if null_state else self.pend.numpy())
        tol = istft_tol(self.prec, self.n, self.hop)
        err = rel_max_err(clean["out"].cpu().numpy(), want)
        if not null_state:  # test_gpu_istft.py holds the pending sums to four times the output's tolerance
            err = max(err, rel_max_err(clean["state"].cpu().numpy(), state) / 4)
        return err, tol

    def element_of(self, j):
        return j * self.bins + 1  # bin 1 of frame j

    def masks(self, row, col):
        return self.span_masks(row, (col // self.bins) * self.hop, self.n, self.F * self.hop, self.H)


class Welch(_Bank):
    """ticks are samples: a call may end anywhere.  The stream starts at position n + 5 with a random history, so that the first
    segments read the state; with state = NULL it starts at position 0, the only place the contract allows that."""

    def setup(self):
        self.bins, self.H = self.n // 2 + 1, self.n - 1
        self.pos0 = self.n + 5
        self.S = self.ticks = self.samples_for(self.F)
        self.first = {32: 7, 512: 200}[self.n]
        self.unit_bytes = self.n * self.rs + self.bins * 8
        self.w = scipy.signal.get_window("hann", self.n)
        self.x = _rand(self.rng, (self.C, self.S), self.rdt)
        self.hist0 = _rand(self.rng, (self.C, self.H), self.rdt)
        self.acc0 = torch.from_numpy(self.rng.uniform(0, self.n, (self.C, self.bins)))

    def samples_for(self, F):
        S = 1
        while welch_frames(self.n, self.hop, self.pos0, S) < F:
            S += 1
        return S + self.hop // 2  # the call ends between two segment ends

    def make(self, workspace):
        return self.sd.welch_bank(self.n, self.hop, self.C, window=self.w, precision=self.bank_prec(), workspace_bytes=workspace)

    def specs(self, null_state=False):
        s = {"in": self.spec(self.x, read_only=True), "acc": self.spec(self.acc0), "out": self.spec(shape=(self.C, self.bins), dtype=self.rdt)}
        if not null_state:
            s["state"] = self.spec(self.hist0, strided=False)
        return s

    def run(self, b, t0, t1):
        pos0 = self.pos0 if b.has("state") else 0
        rc = self.lib.sdsp_hip_welch_process(self.plan, b.ptr("in", t0), b.stride("in"), self.C, t1 - t0, pos0 + t0, b.ptr("state"), b.ptr("acc"),
                                             b.stride("acc"), None)
        assert rc == 0, rc
        if t1 == self.ticks:
            total = welch_frames(self.n, self.hop, pos0, self.S)
            rc = self.lib.sdsp_hip_welch_finalize(self.plan, b.ptr("acc"), b.stride("acc"), total, b.ptr("out"), b.stride("out"), self.C, None)
            assert rc == 0, rc

    def launches(self):
        return self.bank.launches(self.S, self.pos0)

    def reference(self, clean, null_state=False):
        wr = self.w.astype(self.x.numpy().dtype).astype(np.float64)
        acc, F, state = welch_ref(self.x.numpy(), self.n, self.hop, wr, "constant", 0 if null_state else self.pos0,
                                  None if null_state else self.hist0.numpy(), self.acc0.numpy())
        assert F == (welch_frames(self.n, self.hop, 0, self.S) if null_state else self.F)
        if not null_state:
            assert np.array_equal(clean["state"].cpu().numpy(), state.astype(self.x.numpy().dtype))
        err = max(welch_err(clean["out"].cpu().numpy(), welch_psd(acc, F, wr)), welch_err(clean["acc"].cpu().numpy(), acc))
        return err, welch_tol(self.prec)

    def starts(self):
        """first block sample of every segment the one call counts (negative: it starts in the history)"""
        first = (self.pos0 - self.n) // self.hop + 1
        return [first * self.hop - self.pos0 + m * self.hop for m in range(self.F)]

    def element_of(self, j):
        return self.starts()[j] + self.n - 1  # the newest sample of segment j

    def covered(self, col):
        return any(s <= col < s + self.n for s in self.starts())

    def masks(self, row, col):
        rows = torch.zeros((self.C, self.bins), dtype=torch.bool)
        rows[row] = self.covered(col)
        return {"acc": rows, "out": rows.clone(), "state": self.history_mask(row, col, self.S, self.H)}

    def loose(self, clean):
        """two calls against one: every segment's powers are the same bits however the stream is cut, and a bin's sum adds the same F
        non-negative doubles and the initial value in another grouping -- test_gpu_stream_carry.py::test_history_update_welch's bound
        with F + 1 terms.  The estimate is a rounding of the sum and is compared in the one-call layouts."""
        def acc(got, want):
            assert bool(((got - want).abs() <= (self.F + 1) * EPS64 * want).all()), float(((got - want).abs() / want).max())
        return {"acc": acc, "out": lambda got, want: None}


class Csd(Welch):
    """the Welch bank's stream with the four channels and five pairs of tests/csd_ref.py; accumulators and the CROSS estimate are rows of
    reals (re, im interleaved), the unit in which their strides count"""

    def setup(self):
        self.C = 4
        Welch.setup(self)
        self.np_ = len(PAIRS)
        self.unit_bytes = self.C * self.n * self.rs + (2 * self.np_ + self.C) * self.bins * 8  # one segment column
        self.xy0 = torch.from_numpy(self.rng.standard_normal((self.np_, 2 * self.bins)) * self.n)
        self.xy0[:, 1] = 0  # the imaginary parts of bins 0 and n / 2 stay +0.0
        self.xy0[:, -1] = 0

    def units(self):
        return self.F

    def make(self, workspace):
        return self.sd.csd_bank(self.n, self.hop, self.C, PAIRS, window=self.w, precision=self.bank_prec(), workspace_bytes=workspace)

    def specs(self, null_state=False):
        s = {"in": self.spec(self.x, read_only=True), "acc_xy": self.spec(self.xy0), "acc_auto": self.spec(self.acc0),
             "out": self.spec(shape=(self.np_, 2 * self.bins), dtype=self.rdt)}
        if not null_state:
            s["state"] = self.spec(self.hist0, strided=False)
        return s

    def run(self, b, t0, t1):
        pos0 = self.pos0 if b.has("state") else 0
        rc = self.lib.sdsp_hip_csd_process(self.plan, b.ptr("in", t0), b.stride("in"), t1 - t0, pos0 + t0, b.ptr("state"), b.ptr("acc_xy"),
                                           b.stride("acc_xy"), b.ptr("acc_auto"), b.stride("acc_auto"), None)
        assert rc == 0, rc
        if t1 == self.ticks:
            total = welch_frames(self.n, self.hop, pos0, self.S)
            rc = self.lib.sdsp_hip_csd_finalize(self.plan, 0, b.ptr("acc_xy"), b.stride("acc_xy"), b.ptr("acc_auto"), b.stride("acc_auto"),
                                                total, b.ptr("out"), b.stride("out"), None)
            assert rc == 0, rc

    def reference(self, clean, null_state=False):
        wr = self.w.astype(self.x.numpy().dtype).astype(np.float64)
        xy0 = self.xy0.numpy()[:, 0::2] + 1j * self.xy0.numpy()[:, 1::2]
        xy, au, F, state = csd_ref(self.x.numpy().astype(np.float64), PAIRS, self.n, self.hop, wr, "constant", 0 if null_state else self.pos0,
                                   None if null_state else self.hist0.numpy(), xy0, self.acc0.numpy())
        if not null_state:
            assert np.array_equal(clean["state"].cpu().numpy(), state.astype(self.x.numpy().dtype))
        cplx = lambda t: t.cpu().numpy().astype(np.float64)[:, 0::2] + 1j * t.cpu().numpy().astype(np.float64)[:, 1::2]  # noqa: E731
        err = max(csd_err(cplx(clean["out"]), csd_density(xy, F, wr)), csd_err(cplx(clean["acc_xy"]), xy),
                  csd_err(clean["acc_auto"].cpu().numpy(), au))
        return err, csd_tol(self.prec)

    def launches(self):
        return self.bank.launches(self.S, self.pos0)

    def poisons(self):
        """a slice is the segment columns [ja, jb) of all channels, its units channel-major: next to a slice edge inside channel 1
        (columns 2 and 3), next to the channel edge inside the slice [3, 6) (column 5 of channel 1, column 3 of channel 2)"""
        maps = arena.slice_map(self.F, CSD_COLS)
        assert maps[:2] == [(0, 3), (3, 6)]
        units = [("last column of a slice", 1, 2), ("first column of the next slice", 1, 3),
                 ("last unit of channel 1 in the slice [3, 6)", 1, 5), ("first unit of channel 2 in that slice", 2, 3)]
        return [(label, c, self.element_of(j)) for label, c, j in units] + [("channel 0, sample 0", 0, 0),
                                                                            ("last channel, last sample", self.C - 1, self.S - 1)]

    def masks(self, row, col):
        hit = self.covered(col)
        auto = torch.zeros((self.C, self.bins), dtype=torch.bool)
        auto[row] = hit
        xy = torch.zeros((self.np_, 2 * self.bins), dtype=torch.bool)
        for i, pair in enumerate(PAIRS):  # the pairs that name the channel, and only those
            xy[i] = hit and row in pair
        xy[:, 1] = False  # the contract's +0.0 imaginary parts of bins 0 and n / 2: not computed from the spectra
        xy[:, -1] = False
        return {"acc_xy": xy, "acc_auto": auto, "out": xy.clone(), "state": self.history_mask(row, col, self.S, self.H)}

    def loose(self, clean):
        """as Welch.loose for the auto sums.  A cross sum adds F signed products and the initial value, each product at most |X_a| |X_b|
        in size, so two groupings differ by less than (F + 1) eps (|initial| + sum |X_a| |X_b|), and by Cauchy-Schwarz the sum is at
        most sqrt(sum |X_a|^2 sum |X_b|^2), which the auto sums give."""
        seg = (clean["acc_auto"] - self.acc0.to(clean["acc_auto"].device)).clamp(min=0)
        a, c = [torch.tensor([p[i] for p in PAIRS], device=seg.device) for i in (0, 1)]
        size = (seg[a] * seg[c]).sqrt().repeat_interleave(2, dim=1) + self.xy0.to(seg.device).abs()

        def acc_xy(got, want):
            assert bool(((got - want).abs() <= (self.F + 1) * EPS64 * size).all())
        return {"acc_xy": acc_xy, "acc_auto": Welch.loose(self, clean)["acc"], "out": lambda got, want: None}


class Pfb(_Bank):
    def setup(self):
        self.m, self.cplx = self.n, self.var == "complex"
        self.p, self.phase = PFB[self.shape]
        self.L, self.H, self.ticks = self.m * self.p, self.m * self.p - self.hop, self.F
        self.bins = self.m if self.cplx else self.m // 2 + 1
        self.unit_bytes = self.m * self.rs * (2 if self.cplx else 1)
        self.pos0 = 7 * self.hop  # frames are rotated by (position - hist) mod m in phase TIME
        self.taps = self.rng.standard_normal(self.L)
        self.edt = self.cdt if self.cplx else self.rdt
        self.x = _rand(self.rng, (self.C, self.F * self.hop), self.edt)
        self.hist0 = _rand(self.rng, (self.C, self.H), self.edt)

    def make(self, workspace):
        return self.sd.pfb_bank(self.m, self.p, self.hop, streams=self.C, taps=self.taps, input=self.var, phase=self.phase,
                                precision=self.bank_prec(), workspace_bytes=workspace)

    def specs(self, null_state=False):
        s = {"in": self.spec(self.x, read_only=True), "out": self.spec(shape=(self.C, self.F * self.bins), dtype=self.cdt)}
        if not null_state:
            s["state"] = self.spec(self.hist0, strided=False)
        return s

    def run(self, b, t0, t1):
        rc = self.lib.sdsp_hip_pfb_process(self.plan, b.ptr("in", t0 * self.hop), b.stride("in"), b.ptr("out", t0 * self.bins), b.stride("out"),
                                           self.C, (t1 - t0) * self.hop, self.pos0 + t0 * self.hop, b.ptr("state"), None)
        assert rc == 0, rc

    def launches(self):
        return self.bank.launches(self.F * self.hop)

    def reference(self, clean, null_state=False):
        taps_p = self.taps.astype(np.float64 if self.prec == "f64" else np.float32).astype(np.float64)
        want, state = pfb_ref(self.x.numpy(), self.m, self.p, self.hop, taps_p, None if null_state else self.hist0.numpy(), self.phase, self.pos0)
        if not null_state:
            assert np.array_equal(clean["state"].cpu().numpy(), state.astype(self.x.numpy().dtype))
        return pfb_err(clean["out"].cpu().numpy().reshape(want.shape), want), pfb_tol(self.prec, self.L)

    def element_of(self, j):
        return j * self.hop + self.hop - 1

    def masks(self, row, col):
        q = col + self.H
        return {"out": self.frames_mask(row, lambda j: j * self.hop <= q < j * self.hop + self.L, self.C, self.bins),
                "state": self.history_mask(row, col, self.F * self.hop, self.H)}


class PfbSynth(_Bank):
    def setup(self):
        self.m, self.cplx = self.n, self.var == "complex"
        self.p, self.phase = PFB[self.shape]
        self.L, self.H, self.ticks = self.m * self.p, self.m * self.p - self.hop, self.F
        self.bins = self.m if self.cplx else self.m // 2 + 1
        self.unit_bytes = self.m * self.rs * (2 if self.cplx else 1)
        self.pos0 = 7 * self.hop
        self.g = self.rng.uniform(-1, 1, self.L)
        self.edt = self.cdt if self.cplx else self.rdt
        self.X = _rand(self.rng, (self.C, self.F * self.bins), self.cdt)
        X3 = self.X.numpy().reshape(self.C, self.F, self.bins)
        self.vmax = float(np.abs(pfb_synth_frames_ref(X3, self.m, self.p, self.hop, self.phase, self.pos0, self.cplx)).max())
        pend = self.rng.uniform(-1, 1, (self.C, self.H))  # pending sums no larger than max |v|, as test_gpu_pfb_synth.py's bound assumes
        if self.cplx:
            pend = (pend + 1j * self.rng.uniform(-1, 1, (self.C, self.H))) / np.sqrt(2)
        self.pend = torch.from_numpy(pend * self.vmax).to(self.edt)

    def make(self, workspace):
        return self.sd.pfb_synthesis_bank(self.m, self.p, self.hop, streams=self.C, taps=self.g, output=self.var, phase=self.phase,
                                          precision=self.bank_prec(), workspace_bytes=workspace)

    def specs(self, null_state=False):
        s = {"in": self.spec(self.X, read_only=True), "out": self.spec(shape=(self.C, self.F * self.hop), dtype=self.edt)}
        if not null_state:
            s["state"] = self.spec(self.pend, strided=False)
        return s

    def run(self, b, t0, t1):
        rc = self.lib.sdsp_hip_pfb_synth_process(self.plan, b.ptr("in", t0 * self.bins), b.stride("in"), b.ptr("out", t0 * self.hop),
                                                 b.stride("out"), self.C, t1 - t0, self.pos0 + t0 * self.hop, b.ptr("state"), None)
        assert rc == 0, rc

    def launches(self):
        return self.bank.launches(self.F)

    def reference(self, clean, null_state=False):
        g_p = self.g.astype(np.float64 if self.prec == "f64" else np.float32).astype(np.float64)
        X3 = self.X.numpy().reshape(self.C, self.F, self.bins)
        want, state = pfb_synth_ref(X3, self.m, self.p, self.hop, g_p, None if null_state else self.pend.numpy(), self.phase, self.pos0,
                                    cplx=self.cplx)
        err = np.abs(clean["out"].cpu().numpy() - want).max()
        if not null_state:
            err = max(err, np.abs(clean["state"].cpu().numpy() - state).max())
        return float(err), synth_bound(self.prec, self.m, self.p, self.hop, self.vmax)

    def element_of(self, j):
        return j * self.bins + 1

    def masks(self, row, col):
        return self.span_masks(row, (col // self.bins) * self.hop, self.L, self.F * self.hop, self.H)


KINDS = {"stft": Stft, "istft": Istft, "welch": Welch, "csd": Csd, "pfb": Pfb, "pfb_synth": PfbSynth}

_made = {}


def _bank_and_clean(sd, kind, shape, var, prec):
    """the case's bank (a one-slice workspace) and its clean result, computed once, held to the reference once, and shared"""
    key = (kind, shape, var, prec)
    if key not in _made:
        bank = KINDS[kind](sd, kind, shape, var, prec)
        clean = arena.clean_bank(torch, bank)
        err, tol = bank.reference(clean)
        print(f"{'-'.join(key)}: clean result against the reference {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (key, err, tol)
        _made[key] = (bank, clean)
    return _made[key]


# ------------------------------------------------------------------ layouts and the switches they throw

NAMES = ("in", "out", "state", "acc", "acc_xy", "acc_auto")
OUTS = ("out", "acc", "acc_xy", "acc_auto")


def _layout(default, **off):
    return {name: off.get(name, default) for name in NAMES}


LAYOUTS = {f"lead{lead}-{stride}": _layout((lead, stride)) for lead in (0, 1, 2) for stride in arena.STRIDES}
# one pointer off, everything else on 16 bytes with strides that keep them (an exact stride may be off by itself: 11 frames of 17 bins)
LAYOUTS["state1"] = _layout((0, "vec"), state=(1, "exact"))                   # istft.hip:150, pfb_synth.hip:289: only `state` fails
LAYOUTS["out1"] = _layout((0, "vec"), **{name: (1, "vec") for name in OUTS})  # only `out` (the accumulators) fails, `in` aligned
LAYOUTS["in1"] = _layout((0, "vec"), **{"in": (1, "vec")})                    # only `in` fails
ODD = LAYOUTS["lead1-odd"]


def _switches(kind, shape, var, prec, layout):
    """the launchers' alignment conditions for this case under this layout, computed as they compute them: an arena's base and margin
    are multiples of 512 bytes, so a pointer's offset from 16 bytes is its lead, and a stride is arena.stride_for's"""
    n, hop = SYNTH_SHAPES[shape][:2]
    F = _frames(kind, shape)
    rs = _rs(prec)
    vec = 16 // rs
    cplx = var == "complex"
    bins = n if kind in ("pfb", "pfb_synth") and cplx else n // 2 + 1
    es = {"stft": (rs, 2 * rs if cplx else rs), "istft": (2 * rs, rs), "pfb": (2 * rs if cplx else rs, 2 * rs),
          "pfb_synth": (2 * rs, 2 * rs if cplx else rs), "welch": (rs, rs), "csd": (rs, rs)}[kind]  # element bytes of in and out
    cols ={"stft": (F * hop, F * bins), "istft": (F * bins, F * hop), "pfb": (F * hop, F * bins), "pfb_synth": (F * bins, F * hop)}.get(kind)

    def aligned(name, esize, ncols=None):
        lead, stride = layout[name]
        ok = (lead * esize) % 16 == 0
        if ncols is not None:
            ok = ok and (arena.stride_for(ncols, esize, stride) * esize) % 16 == 0
        return ok

    if kind == "stft":
        return {"stft.hip:129 vec_ok": aligned("in", es[0], cols[0])}
    if kind in ("welch", "csd"):
        S = _welch_samples(n, hop, F)
        return {"welch.hip:355 vec_ok" + (" (csd)" if kind == "csd" else ""): aligned("in", es[0], S)}
    if kind == "istft":
        return {"istft.hip:149 vec (ola<R, VEC>)": hop % vec == 0 and aligned("out", es[1], cols[1]) and aligned("state", es[1])}
    if kind == "pfb":
        sw = {"pfb.hip:182 in_vec_ok": aligned("in", es[0], cols[0])}
        if cplx:  # real input folds into the plan's workspace: dst, dst_cstride = F m and dst_sub = g0 m are always multiples of 16 bytes
            sw["pfb.hip:183 dst_vec_ok (complex)"] = aligned("out", es[1], cols[1])
        return sw
    place = aligned("out", es[1], cols[1]) and aligned("state", es[1])
    ept = 16 // es[1]
    sw = {"pfb_synth.hip:288 place_vec_ok": place}
    if ept > 1:  # f64 complex output has one element per 16 bytes: no wide form
        sw["pfb_synth.hip:293 wide"] = hop != n and hop % ept == 0 and place
    if prec == "f32":  # an f64 bin is 16 bytes: one copy kernel
        sw["pfb_synth.hip:324 wide copy"] = aligned("in", es[0], cols[0])
    return sw


def _welch_samples(n, hop, F):
    S = 1
    while welch_frames(n, hop, n + 5, S) < F:
        S += 1
    return S + hop // 2


def test_every_alignment_switch_is_taken_both_ways():
    """no GPU work: which (case, layout) pairs make each launcher condition true and which false.  Every switch has both; the table
    is printed for the record (pytest -s)."""
    seen = {}
    for param in _cases():
        kind, shape, var, prec = param.values
        for lname, layout in LAYOUTS.items():
            for sw, value in _switches(kind, shape, var, prec, layout).items():
                seen.setdefault(sw, {True: [], False: []})[bool(value)].append(f"{param.id}/{lname}")
    for sw, by in sorted(seen.items()):
        print(f"{sw}: true in {len(by[True])} (e.g. {by[True][:2]}), false in {len(by[False])} (e.g. {by[False][:2]})")
        assert by[True] and by[False], sw
    assert len(seen) == 9


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("kind,shape,var,prec", _cases())
def test_framed_buffers_and_offset_pointers(sd, kind, shape, var, prec):
    """items 1 and 2: every buffer of the call framed, under every layout and both fills"""
    bank, clean = _bank_and_clean(sd, kind, shape, var, prec)
    if kind in ("welch", "csd"):
        assert _welch_samples(bank.n, bank.hop, bank.F) == bank.S  # what _switches takes the stride of `in` from
    for name, layout in LAYOUTS.items():
        arena.check_framed_bank(torch, bank, clean, layout, tag=name)


@pytest.mark.parametrize("kind,shape,var,prec", _cases())
def test_two_calls_and_null_state(sd, kind, shape, var, prec):
    """item 3: the carry kernels on a framed state, at lead 0 and lead 1 of `state`; state = NULL once"""
    bank, clean = _bank_and_clean(sd, kind, shape, var, prec)
    hist = bank.specs()["state"]["shape"][1]
    samples = bank.first * (1 if kind in ("welch", "csd") else bank.hop)
    if bank.n == 512:  # the two-chunk in-place path, then the flat path
        assert samples < hist - 256 and hist > 256 and hist % 256
        assert (bank.ticks - bank.first) * (1 if kind in ("welch", "csd") else bank.hop) >= hist
    loose = bank.loose(clean) if kind in ("welch", "csd") else None
    for name in ("lead0-vec", "state1", "lead1-odd"):
        arena.check_framed_bank(torch, bank, clean, LAYOUTS[name], splits=(bank.first,), loose=loose, tag=f"two calls {name}")
    null = arena.clean_bank(torch, bank, null_state=True)
    err, tol = bank.reference(null, null_state=True)
    assert err <= tol, (err, tol)
    for name in ("lead0-exact", "lead1-odd"):
        arena.check_framed_bank(torch, bank, null, LAYOUTS[name], null_state=True, tag=f"state = NULL {name}")


@pytest.mark.parametrize("kind,shape,var,prec", _cases())
def test_nan_at_slice_and_channel_edges(sd, kind, shape, var, prec):
    """item 4: at the default workspace (one slice) and at a small one whose slices cut through channels"""
    one, clean = _bank_and_clean(sd, kind, shape, var, prec)
    poisons = one.poisons()
    for ws in ("default", CSD_COLS if kind == "csd" else SMALL):
        bank = KINDS[kind](sd, kind, shape, var, prec, ws=ws)
        if ws == "default":
            assert bank.per_slice >= bank.units() and bank.launches() == one.launches()
        else:  # the call really is sliced
            assert bank.per_slice == ws and bank.launches() > one.launches()
            print(f"{kind}-{shape}-{var}-{prec}: slices {arena.slice_map(bank.units(), ws)} of {bank.units()} units, {bank.F} per channel; NaNs at "
                  f"{[(label, row, col) for label, row, col in poisons]}")
        want = clean
        if kind in ("welch", "csd") and ws != "default":
            # a sum's grouping follows the slices (sdsp_hip.h: runs per slice, then one addition into the accumulator), so a sliced call
            # has this workspace's own clean sums: within the regrouping bound of the one-slice ones, the same history
            want = arena.clean_bank(torch, bank)
            for name, close in one.loose(clean).items():
                close(want[name], clean[name])
            assert arena.same_bits(want["state"], clean["state"])
        for name in ("lead0-vec", "lead1-odd"):
            arena.check_poisoned_bank(torch, bank, want, poisons, LAYOUTS[name], tag=f"{ws} {name}")
