"""Host mirror of the arbitrary-ratio polyphase resampler bank (include/sdsp_hip.h: sdsp_hip_arb_*).

Every channel is resampled by any ratio in [1 / 1024, 1024] (input samples per output sample, Q32.32) through a prototype low-pass of
phases * taps_per_phase taps, taking the nearest of `phases` polyphase rows or interpolating linearly between two.  The ratio may
change from call to call, calls may have any length, and the bank carries the per-channel history and the stream time, so any split
of a stream into calls gives the same samples.  Same conventions as ddc_bank (channel-major rows, device history carried across
calls, set_coeff / set_default_coeff); the channel count is that of the tensor given to process."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

KINDS = {"real": L.ARB_REAL, "complex": L.ARB_COMPLEX}
INTERPS = {"nearest": L.ARB_NEAREST, "linear": L.ARB_LINEAR}


def arb_step(ratio: float) -> int:
    """round(ratio * 2^32), ties to even, for ratio = input samples per output sample in [1 / 1024, 1024]: sdsp_hip_arb_step"""
    w = C.c_uint64(0)
    L.check(L.load().sdsp_hip_arb_step(float(ratio), C.byref(w)))
    return w.value


def _step(v) -> int:
    """an integer is a Q32.32 step as it is; a float is a ratio and is converted"""
    if isinstance(v, (int, np.integer)):
        return int(v)
    return arb_step(v)


class arb_resampler:
    """A bank of arbitrary-ratio resamplers.  max_ratio (a float ratio or an integer Q32.32 step) is the largest step a call may
    use; it sizes the kernel's blocks.  `step` (settable between calls, float ratio or integer) starts at min(1, max_ratio);
    `time` is the Q32.32 instant of the next call's first output relative to its first input sample."""

    def __init__(self, phases: int, taps_per_phase: int, max_ratio, kind: str = "real", interp: str = "linear", precision: int = L.F32,
                 device: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}")
        if interp not in INTERPS:
            raise ValueError(f"interp must be one of {sorted(INTERPS)}")
        if phases <= 0 or taps_per_phase <= 0:
            raise ValueError("phases and taps_per_phase must be positive")
        self._lib = L.load()
        self.phases, self.taps_per_phase = phases, taps_per_phase
        self.kind, self.interp, self.precision, self.device = kind, interp, precision, device
        self.max_step = _step(max_ratio)
        if not L.ARB_MIN_STEP <= self.max_step <= L.ARB_MAX_STEP:
            raise ValueError("max_ratio must be in [1 / 1024, 1024]")
        self.hist = taps_per_phase - 1
        self.m_coeff = np.zeros(phases * taps_per_phase)
        self._plan = None
        self._state = None  # torch tensor (channels, max(hist, 1)) of the input dtype, newest sample first
        self._step = min(1 << 32, self.max_step)
        self._time = 0
        self._variant = 0

    def set_coeff(self, h):
        """the prototype: phases * taps_per_phase values, phase p, tap k = h[k * phases + p] (the upfirdn layout)"""
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if h.size != self.phases * self.taps_per_phase:
            raise ValueError("coefficient count differs from phases * taps_per_phase")
        self.m_coeff = h.copy()
        self._drop_plan()

    def set_default_coeff(self, max_ratio=None):
        """Hamming low-pass for ratios up to max_ratio (default: the bank's): phases * scipy.signal.firwin(phases * taps_per_phase,
        min(1, 1 / max_ratio) / phases), from sdsp_hip_arb_design"""
        r = self.max_step / 2.0 ** 32 if max_ratio is None else float(max_ratio)
        h = np.zeros(self.phases * self.taps_per_phase)
        L.check(self._lib.sdsp_hip_arb_design(self.phases, self.taps_per_phase, r, h.ctypes.data))
        self.set_coeff(h)

    def _real_dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _dtype(self):
        import torch
        if self.kind == "complex":
            return torch.complex128 if self.precision == L.F64 else torch.complex64
        return self._real_dtype()

    def reset(self):
        """forget the history and the stream time"""
        self._state = None
        self._time = 0

    @property
    def state(self):
        return self._state

    @property
    def step(self) -> int:
        """input samples per output sample, Q32.32"""
        return self._step

    @step.setter
    def step(self, value):
        s = _step(value)
        if not L.ARB_MIN_STEP <= s <= self.max_step:
            raise ValueError("step must be in [2^22, max_step]")
        self._step = s

    @property
    def time(self) -> int:
        """the instant of the next call's first output relative to its first input sample, Q32.32"""
        return self._time

    @time.setter
    def time(self, value: int):
        if not 0 <= value < 1 << 63:
            raise ValueError("time must be in [0, 2^63)")
        self._time = int(value)

    def out_samples(self, samples: int):
        """(n_out, next_time) of a call of `samples` per channel at the bank's step and time"""
        n, t = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.sdsp_hip_arb_out_samples(self._step, self._time, samples, C.byref(n), C.byref(t)))
        return n.value, t.value

    def set_variant(self, v: int):
        """0 = the fused kernel, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        self._variant = v
        if self._plan:
            L.check(self._lib.sdsp_hip_arb_plan_set_variant(self._plan, v))

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_arb_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_arb_plan_create(C.byref(h), self.phases, self.taps_per_phase, self.m_coeff.ctypes.data,
                                                       self.max_step, KINDS[self.kind], INTERPS[self.interp], self.precision,
                                                       self.device))
            self._plan = h
            L.check(self._lib.sdsp_hip_arb_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_arb_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.ArbPlanInfo()
        L.check(self._lib.sdsp_hip_arb_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per channel at the bank's step and time"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_arb_plan_launches(self._plan, self._step, self._time, samples, C.byref(n)))
        return n.value

    def process(self, x, out=None, samples: int | None = None):
        """x: contiguous device tensor (channels, in_stride) of the bank's dtype (real, or complex for kind="complex"); resamples
        x[:, :samples] of every channel (default: the whole row), continuing from the bank's history and time.  Returns a
        (channels, n_out) device tensor; out, when given, is a contiguous (channels, >= n_out) tensor of that dtype, of which the
        first n_out columns are written."""
        import torch
        dt = self._dtype()
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
            raise ValueError("process needs a contiguous (channels, samples) device tensor of the bank's dtype")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        channels, in_stride = x.shape
        if self._state is not None and self._state.shape[0] != channels:
            raise ValueError("channel count differs from the carried history's (reset() starts a new stream)")
        samples = in_stride if samples is None else samples
        if samples > in_stride:
            raise ValueError("block exceeds the row")
        outs, next_time = self.out_samples(samples)
        if out is None:
            out = torch.empty((channels, outs), dtype=dt, device=x.device)
        if (out.dtype != dt or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.device != x.device
                or out.shape[0] != channels or out.shape[1] < outs):
            raise ValueError("out must be a contiguous (channels, >= n_out) device tensor of the bank's dtype")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((channels, max(self.hist, 1)), dtype=dt, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_arb_process(self._plan, x.data_ptr(), in_stride, out.data_ptr(), out.shape[1], channels, samples,
                                               self._step, self._time, self._state.data_ptr(), stream))
        self._time = next_time
        return out if out.shape[1] == outs else out[:, :outs]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
