"""Host mirror of the polyphase FIR resampler bank (include/sdsp_hip.h: sdsp_hip_resample_*).

Up by `up`, filter with n_taps coefficients, down by `down`, for `channels` streams at once, out of place.  Same conventions as
fir_filter (channel-major rows, per-channel device history carried across calls, set_coeff / copy_coeff_from / preload_filter);
the outputs of a call of S samples are out[:, :S*up/down], S a multiple of down / gcd(up, down)."""
from __future__ import annotations

import ctypes as C
from math import gcd

import numpy as np

from . import _lib as L


class fir_resampler:
    """A bank of `channels` identical rate changers by up / down with an n_taps-tap filter and per-channel history."""

    def __init__(self, n_taps: int, up: int, down: int, channels: int = 1, precision: int = L.F32, device: int = 0):
        if n_taps <= 0 or up <= 0 or down <= 0:
            raise ValueError("n_taps, up and down must be positive")
        self._lib = L.load()
        self.n_taps, self.up, self.down = n_taps, up, down
        self.channels, self.precision, self.device = channels, precision, device
        self.q = down // gcd(up, down)
        self.hist = (n_taps - 1) // up
        self.m_coeff = np.zeros(n_taps)
        self._plan = None
        self._state = None  # torch tensor (channels, max(hist, 1)), newest input first
        self._variant = 0

    def set_coeff(self, h):
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if h.size != self.n_taps:
            raise ValueError("coefficient count differs from n_taps")
        self.m_coeff = h.copy()
        self._drop_plan()

    def set_antialias_coeff(self):
        """Hamming low-pass at 1 / (2 max(up, down)) of the intermediate rate, gain up (sdsp_hip_resample_design)"""
        h = np.zeros(self.n_taps)
        L.check(self._lib.sdsp_hip_resample_design(self.n_taps, self.up, self.down, h.ctypes.data))
        self.set_coeff(h)

    def copy_coeff_from(self, other: "fir_resampler"):  # design, not history
        self.set_coeff(other.m_coeff)

    def _dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def preload_filter(self, value: float):  # history of a steady input
        import torch
        self._state = torch.full((self.channels, max(self.hist, 1)), value, dtype=self._dtype(), device=f"cuda:{self.device}")

    def reset(self):
        self._state = None

    @property
    def state(self):
        return self._state

    def set_variant(self, v: int):
        """0 = default, 1 = plain cross-check kernel, 2 = the generic polyphase kernel for every ratio (same bits)"""
        if v not in (0, 1, 2):
            raise ValueError("variant must be 0, 1 or 2")
        self._variant = v
        if self._plan:
            L.check(self._lib.sdsp_hip_resample_plan_set_variant(self._plan, v))

    def out_samples(self, samples: int) -> int:
        """outputs one call of `samples` inputs per channel yields (raises unless samples is a multiple of q)"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_resample_out_samples(self.up, self.down, samples, C.byref(n)))
        return n.value

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_resample_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_resample_plan_create(C.byref(h), self.n_taps, self.m_coeff.ctypes.data, self.up, self.down,
                                                            self.precision, self.device))
            self._plan = h
            L.check(self._lib.sdsp_hip_resample_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_resample_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.ResamplePlanInfo()
        L.check(self._lib.sdsp_hip_resample_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def process(self, x, out=None, samples: int | None = None):
        """x: contiguous device tensor (channels, in_stride); resamples x[:, :samples] of every channel (default: the whole row),
        continuing from the bank's history.  out: contiguous device tensor (channels, >= samples*up/down), allocated when None;
        only out[:, :samples*up/down] is written.  Returns out."""
        import torch
        dt = self._dtype()
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
            raise ValueError("process needs a contiguous (channels, samples) device tensor of the bank dtype")
        if x.shape[0] != self.channels:
            raise ValueError("channel count differs from the bank's")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        in_stride = x.shape[1]
        samples = in_stride if samples is None else samples
        if samples > in_stride:
            raise ValueError("block exceeds the row")
        outs = self.out_samples(samples)
        if out is None:
            out = torch.empty((self.channels, outs), dtype=dt, device=x.device)
        if out.dtype != dt or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.device != x.device:
            raise ValueError("out must be a contiguous (channels, n) device tensor of the bank dtype on the input's device")
        if out.shape[0] != self.channels or out.shape[1] < outs:
            raise ValueError("out is too small for samples*up/down outputs per channel")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((self.channels, max(self.hist, 1)), dtype=dt, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_resample_process(self._plan, x.data_ptr(), in_stride, out.data_ptr(), out.shape[1], self.channels,
                                                    samples, self._state.data_ptr(), stream))
        return out

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
