"""Host mirror of the polyphase filter-bank channelizer bank (include/sdsp_hip.h: sdsp_hip_pfb_*).

Splits each of `streams` real or complex streams into n_channels equally spaced sub-bands with a prototype low-pass of
taps_per_channel * n_channels taps: per frame one fold of the taps_per_channel polyphase branches and one n_channels-point transform of
the library.  Same conventions as stft_bank (stream-major rows, per-stream device history carried across calls, preload_filter / reset);
a call of S samples (a multiple of hop) returns S / hop frames per stream as a (streams, frames, bins) complex device tensor, bins =
n_channels / 2 + 1 for real input and n_channels for complex input.

The taps multiply the samples in window (correlation) order, u[r] = sum_p x[p M + r] h[p M + r], as the STFT window does: pass
h[::-1] when the prototype is meant in convolution order.  A symmetric prototype is the same either way."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .stft import WINDOWS

INPUTS = {"real": L.PFB_REAL, "complex": L.PFB_COMPLEX}
PHASES = {"frame": L.PFB_PHASE_FRAME, "time": L.PFB_PHASE_TIME}


def pfb_prototype(window: str, n_channels: int, taps_per_channel: int) -> np.ndarray:
    """windowed-sinc prototype with cutoff at half the sub-band spacing and unit DC gain:
    scipy.signal.firwin(taps_per_channel * n_channels, 1.0 / n_channels, window=window), from sdsp_hip_pfb_prototype"""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {sorted(WINDOWS)}")
    h = np.zeros(max(n_channels * taps_per_channel, 1))
    L.check(L.load().sdsp_hip_pfb_prototype(WINDOWS[window], n_channels, taps_per_channel, h.ctypes.data))
    return h


class pfb_bank:
    """A bank of `streams` streaming polyphase filter banks of n_channels sub-bands every `hop` samples with per-stream history.

    phase="time": every sub-band is a down-converted baseband signal, phase-continuous from frame to frame for any hop (the frames are
    rotated by the absolute index of their first sample, which the bank counts in `position`); phase="frame": the phase refers to each
    frame's first sample, which makes the output bins k * taps_per_channel of the STFT with the prototype as its window."""

    def __init__(self, n_channels: int, taps_per_channel: int, hop: int | None = None, streams: int = 1, taps="hamming",
                 input: str = "real", phase: str = "time", precision: int = L.F32, device: int = 0, workspace_bytes: int = 0):
        if input not in INPUTS:
            raise ValueError(f"input must be one of {sorted(INPUTS)}")
        if phase not in PHASES:
            raise ValueError(f"phase must be one of {sorted(PHASES)}")
        hop = n_channels if hop is None else hop
        if n_channels <= 0 or taps_per_channel <= 0 or hop <= 0 or hop > n_channels:
            raise ValueError("need n_channels >= 1, taps_per_channel >= 1 and 1 <= hop <= n_channels")
        self._lib = L.load()
        self.n_channels, self.taps_per_channel, self.hop, self.streams = n_channels, taps_per_channel, hop, streams
        self.input, self.phase, self.precision, self.device, self.workspace_bytes = input, phase, precision, device, workspace_bytes
        self.n_taps = n_channels * taps_per_channel
        self.bins = n_channels if input == "complex" else n_channels // 2 + 1
        self.hist = self.n_taps - hop
        if isinstance(taps, str):
            self.taps = pfb_prototype(taps, n_channels, taps_per_channel)
        else:
            self.taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))
            if self.taps.size != self.n_taps:
                raise ValueError("taps length differs from taps_per_channel * n_channels")
        self._plan = None
        self._state = None  # torch tensor (streams, max(hist, 1)) of the input dtype, newest sample first
        self._position = 0
        self._variant = 0

    def _real_dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _out_dtype(self):
        import torch
        return torch.complex128 if self.precision == L.F64 else torch.complex64

    def _in_dtype(self):
        return self._out_dtype() if self.input == "complex" else self._real_dtype()

    def preload_filter(self, value):  # history of a steady input
        import torch
        self._state = torch.full((self.streams, max(self.hist, 1)), value, dtype=self._in_dtype(), device=f"cuda:{self.device}")

    def reset(self):
        """forget the history and the stream position"""
        self._state = None
        self._position = 0

    @property
    def state(self):
        return self._state

    @property
    def position(self) -> int:
        """samples per stream consumed so far (the phase reference of phase="time")"""
        return self._position

    @position.setter
    def position(self, value: int):
        if value < 0:
            raise ValueError("position must be >= 0")
        self._position = int(value)

    def frames(self, samples: int) -> int:
        """frames one call of `samples` per stream writes (raises unless samples is a multiple of hop)"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_pfb_frames(self.hop, samples, C.byref(n)))
        return n.value

    def set_variant(self, v: int):
        """the inner transform's kernel variant (sdsp_hip_fft_plan_set_variant)"""
        if v < 0:
            raise ValueError("variant must be >= 0")
        self._ensure_plan()
        L.check(self._lib.sdsp_hip_pfb_plan_set_variant(self._plan, v))
        self._variant = v

    def _set_fold_form(self, form: int):
        """measurement and cross-check hook: 1 runs the plain per-frame fold whatever the hop, 0 the form the sizes select"""
        self._ensure_plan()
        L.check(self._lib.sdsp_hip_pfb_plan_set_fold_form(self._plan, form))

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_pfb_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_pfb_plan_create(C.byref(h), self.n_channels, self.taps_per_channel, self.hop, self.taps.ctypes.data,
                                                       INPUTS[self.input], PHASES[self.phase], self.precision, self.workspace_bytes,
                                                       self.device))
            self._plan = h
            if self._variant:
                L.check(self._lib.sdsp_hip_pfb_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_pfb_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.PfbPlanInfo()
        L.check(self._lib.sdsp_hip_pfb_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        d["fold"] = i.fold.decode()
        return d

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per stream"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_pfb_plan_launches(self._plan, self.streams, samples, C.byref(n)))
        return n.value

    def process(self, x, samples: int | None = None, out=None):
        """x: contiguous device tensor (streams, in_stride) of the input dtype (real, or complex for input="complex"); channelizes
        x[:, :samples] of every stream (default: the whole row), continuing from the bank's history and position.  Returns a
        (streams, frames, bins) complex device tensor; out, when given, is a contiguous (streams, >= frames, bins) tensor of that
        dtype, of which the first frames are written."""
        import torch
        dt = self._in_dtype()
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
            raise ValueError("process needs a contiguous (streams, samples) device tensor of the bank's input dtype")
        if x.shape[0] != self.streams:
            raise ValueError("stream count differs from the bank's")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        in_stride = x.shape[1]
        samples = in_stride if samples is None else samples
        if samples > in_stride:
            raise ValueError("block exceeds the row")
        F = self.frames(samples)
        if out is None:
            out = torch.empty((self.streams, F, self.bins), dtype=self._out_dtype(), device=x.device)
        if (out.dtype != self._out_dtype() or not out.is_cuda or not out.is_contiguous() or out.dim() != 3 or out.device != x.device
                or out.shape[0] != self.streams or out.shape[1] < F or out.shape[2] != self.bins):
            raise ValueError("out must be a contiguous (streams, >= frames, bins) complex device tensor of the bank precision")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((self.streams, max(self.hist, 1)), dtype=dt, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_pfb_process(self._plan, x.data_ptr(), in_stride, out.data_ptr(), out.shape[1] * self.bins,
                                               self.streams, samples, self._position, self._state.data_ptr(), stream))
        self._position += samples
        return out if out.shape[1] == F else out[:, :F]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
