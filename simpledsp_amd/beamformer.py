"""Host mirror of the time-delay beamformer bank (include/sdsp_hip.h: sdsp_hip_beam_*).

`groups` sensor arrays of `sensors` rows each are steered into `beams` rows each: a beam is the sum over its entries of the entry's sensor
delayed by whole samples and filtered with the entry's own n_taps taps (a fractional-delay filter carrying the weight).  Same
conventions as ddc_bank (channel-major rows, per-row device history carried across calls); a call of S samples returns a
(groups * beams, S) device tensor.  There is no stream position: the operation is time-invariant."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

KINDS = {"real": L.BEAM_REAL, "complex": L.BEAM_COMPLEX}


def beam_delay_taps(tau, weights, n_taps: int, beta: float):
    """Kaiser-windowed-sinc fractional-delay taps (sdsp_hip_beam_delay_taps) for every element of tau (samples, >= 0) and the weight of
    the same position: returns (delays, taps), an integer array of tau's shape and a float64 array of shape tau.shape + (n_taps,).  An
    entry with these taps delays by tau + (n_taps - 1) // 2 samples."""
    tau = np.asarray(tau, dtype=np.float64)
    weights = np.broadcast_to(np.asarray(weights, dtype=np.float64), tau.shape)
    lib = L.load()
    delays = np.zeros(tau.shape, dtype=np.int64)
    taps = np.zeros(tau.shape + (int(n_taps),), dtype=np.float64)
    row = np.zeros(max(int(n_taps), 1), dtype=np.float64)
    d = C.c_uint32(0)
    for idx in np.ndindex(*tau.shape):
        L.check(lib.sdsp_hip_beam_delay_taps(float(tau[idx]), float(weights[idx]), int(n_taps), float(beta), C.byref(d), row.ctypes.data))
        delays[idx] = d.value
        taps[idx] = row[:int(n_taps)]
    return delays, taps


def plane_wave_delays(positions, directions, speed: float, fs: float):
    """Steering delays in samples for plane waves: positions (C, D) sensor coordinates, directions (B, D) unit vectors along which each
    beam's wave travels (from its source towards the array: the wave reaches sensor c at (p_c . u_b) / speed), speed in the positions'
    unit per second, fs in Hz.  tau[b, c] = -(p_c . u_b) / speed * fs, minus the global minimum (so every delay is >= 0 and the
    relative timing between beams is kept).  numpy only."""
    p = np.asarray(positions, dtype=np.float64)
    u = np.asarray(directions, dtype=np.float64)
    if p.ndim == 1:
        p = p[:, None]
    if u.ndim == 1:
        u = u[:, None]
    if p.ndim != 2 or u.ndim != 2 or p.shape[1] != u.shape[1] or p.shape[0] == 0 or u.shape[0] == 0:
        raise ValueError("positions must be (sensors, dims) and directions (beams, dims) with the same dims")
    if not (np.isfinite(speed) and speed > 0 and np.isfinite(fs) and fs > 0):
        raise ValueError("speed and fs must be positive and finite")
    if not (np.all(np.isfinite(p)) and np.all(np.isfinite(u))):
        raise ValueError("positions and directions must be finite")
    tau = -(u @ p.T) / float(speed) * float(fs)
    return tau - tau.min()


class beamformer_bank:
    """A filter-and-sum beamformer: entries (beam, sensor, delay, taps) fixed by set_entries / set_dense / set_steering; process()
    streams blocks through it."""

    def __init__(self, sensors: int, beams: int, n_taps: int, groups: int = 1, kind: str = "real", precision: int = L.F32,
                 device: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}")
        if sensors <= 0 or beams <= 0 or n_taps <= 0 or groups <= 0:
            raise ValueError("sensors, beams, n_taps and groups must be positive")
        self._lib = L.load()
        self.sensors, self.beams, self.n_taps, self.groups = sensors, beams, n_taps, groups
        self.kind, self.precision, self.device = kind, precision, device
        self._entries = np.zeros((0, 3), dtype=np.uint32)
        self._taps = np.zeros((0, n_taps), dtype=np.complex128 if kind == "complex" else np.float64)
        self._plan = None
        self._state = None  # torch tensor (groups * sensors, max(hist, 1)) of the row dtype, newest sample first
        self._variant = 0

    # ---- entries
    def set_entries(self, entries):
        """entries: [(beam, sensor, delay, taps)], sorted by beam and, within a beam, by strictly ascending sensor; taps: n_taps values
        (complex for kind="complex").  Drops the plan and the history."""
        ent = np.zeros((len(entries), 3), dtype=np.uint32)
        taps = np.zeros((len(entries), self.n_taps), dtype=self._taps.dtype)
        for i, (b, c, d, g) in enumerate(entries):
            if not (0 <= int(b) < self.beams and 0 <= int(c) < self.sensors):
                raise ValueError("an entry names a beam or a sensor the bank does not have")
            if not 0 <= int(d) <= L.BEAM_MAX_DELAY:
                raise ValueError("a delay must be in [0, 65535]")
            g = np.asarray(g)
            if self.kind == "real" and np.iscomplexobj(g):
                raise ValueError("a real bank takes real taps")
            g = g.astype(taps.dtype).reshape(-1)
            if g.size != self.n_taps:
                raise ValueError("tap count differs from n_taps")
            ent[i] = (int(b), int(c), int(d))
            taps[i] = g
        self._entries, self._taps = ent, taps
        self._drop_plan()
        self._state = None

    def set_dense(self, delays, taps):
        """every beam uses every sensor: delays (beams, sensors) integers, taps (beams, sensors, n_taps)"""
        delays = np.asarray(delays)
        taps = np.asarray(taps)
        if delays.shape != (self.beams, self.sensors) or taps.shape != (self.beams, self.sensors, self.n_taps):
            raise ValueError("delays must be (beams, sensors) and taps (beams, sensors, n_taps)")
        self.set_entries([(b, c, int(delays[b, c]), taps[b, c]) for b in range(self.beams) for c in range(self.sensors)])

    def set_steering(self, tau, weights, beta: float):
        """dense fractional-delay steering: tau (beams, sensors) delays in samples (plane_wave_delays), weights (beams, sensors) (the
        shading; complex weights for kind="complex" turn the real delay taps), Kaiser beta"""
        tau = np.asarray(tau, dtype=np.float64)
        weights = np.asarray(weights)
        if tau.shape != (self.beams, self.sensors) or weights.shape != tau.shape:
            raise ValueError("tau and weights must be (beams, sensors)")
        if np.iscomplexobj(weights):
            if self.kind != "complex":
                raise ValueError("a real bank takes real weights")
            delays, taps = beam_delay_taps(tau, np.ones(tau.shape), self.n_taps, beta)
            taps = taps * weights[:, :, None]
        else:
            delays, taps = beam_delay_taps(tau, weights, self.n_taps, beta)
        self.set_dense(delays, taps)

    # ---- stream
    def _row_dtype(self):
        import torch
        if self.kind == "complex":
            return torch.complex128 if self.precision == L.F64 else torch.complex64
        return torch.float64 if self.precision == L.F64 else torch.float32

    @property
    def hist(self) -> int:
        d = int(self._entries[:, 2].max()) if len(self._entries) else 0
        return d + self.n_taps - 1

    def reset(self):
        """forget the history"""
        self._state = None

    @property
    def state(self):
        return self._state

    def set_variant(self, v: int):
        """0 = the fused kernel, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        self._variant = v
        if self._plan:
            L.check(self._lib.sdsp_hip_beam_plan_set_variant(self._plan, v))

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_beam_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            ent = np.ascontiguousarray(self._entries, dtype=np.uint32)
            g = np.ascontiguousarray(self._taps)
            g = g.view(np.float64) if self.kind == "complex" else g.astype(np.float64)
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_beam_plan_create(C.byref(h), self.sensors, self.beams, self.groups, self.n_taps, len(ent),
                                                        ent.ctypes.data if len(ent) else None, g.ctypes.data if len(ent) else None,
                                                        KINDS[self.kind], self.precision, self.device))
            self._plan = h
            L.check(self._lib.sdsp_hip_beam_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_beam_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.BeamPlanInfo()
        L.check(self._lib.sdsp_hip_beam_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per row"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_beam_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    def process(self, x, out=None, samples: int | None = None):
        """x: contiguous device tensor (groups * sensors, in_stride) of the bank's row dtype; steers x[:, :samples] of every row
        (default: the whole row), continuing from the bank's history.  Returns a (groups * beams, samples) device tensor; out, when
        given, is a contiguous (groups * beams, >= samples) tensor of that dtype, of which the first `samples` columns are written."""
        import torch
        dt = self._row_dtype()
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
            raise ValueError("process needs a contiguous (groups * sensors, samples) device tensor of the bank's row dtype")
        if x.shape[0] != self.groups * self.sensors:
            raise ValueError("row count differs from groups * sensors")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        in_stride = x.shape[1]
        samples = in_stride if samples is None else samples
        if samples < 0 or samples > in_stride:
            raise ValueError("block exceeds the row")
        rows = self.groups * self.beams
        if out is None:
            out = torch.empty((rows, samples), dtype=dt, device=x.device)
        if (out.dtype != dt or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.device != x.device
                or out.shape[0] != rows or out.shape[1] < samples):
            raise ValueError("out must be a contiguous (groups * beams, >= samples) device tensor of the bank's row dtype")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((self.groups * self.sensors, max(self.hist, 1)), dtype=dt, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_beam_process(self._plan, x.data_ptr(), in_stride, out.data_ptr(), out.shape[1], samples,
                                                self._state.data_ptr(), stream))
        return out if out.shape[1] == samples else out[:, :samples]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
