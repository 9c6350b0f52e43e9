"""Host mirror of the polyphase synthesis filter bank (include/sdsp_hip.h: sdsp_hip_pfb_synth_*).

The inverse of pfb_bank: rebuilds each of `streams` real or complex streams from frames of n_channels sub-bands (pfb_bank's output
layout).  Per frame one reverse n_channels-point transform of the library, then every output sample gathers its taps_per_channel *
n_channels / hop covering frames times the synthesis prototype.  The pending sums of the last taps_per_channel * n_channels - hop
positions are carried per stream on the device across calls; a call of F frames returns (streams, F * hop) samples.

With the dual of the analysis prototype (pfb_dual_prototype, or a window name here), pfb_synthesis_bank(pfb_bank(x)) is x delayed by
taps_per_channel * n_channels - hop samples."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .pfb import INPUTS, PHASES, pfb_prototype


def pfb_dual_prototype(taps, n_channels: int, taps_per_channel: int, hop: int) -> np.ndarray:
    """the minimum-norm synthesis prototype that reconstructs through the analysis prototype `taps` at this hop
    (sdsp_hip_pfb_dual_prototype); raises SdspHipError where no dual of the prototype's support exists"""
    h = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))
    if n_channels > 0 and taps_per_channel > 0 and h.size != n_channels * taps_per_channel:
        raise ValueError("taps length differs from taps_per_channel * n_channels")
    g = np.zeros(max(h.size, 1))
    L.check(L.load().sdsp_hip_pfb_dual_prototype(n_channels, taps_per_channel, hop, h.ctypes.data, g.ctypes.data))
    return g


class pfb_synthesis_bank:
    """A bank of `streams` streaming polyphase synthesis filter banks of n_channels sub-bands, `hop` samples per frame, with
    per-stream pending sums.

    taps: the synthesis prototype itself (an array of taps_per_channel * n_channels values), or a window name: the dual of
    pfb_prototype(window, ...) at this hop (raises where none exists).  phase must be the analysis bank's."""

    def __init__(self, n_channels: int, taps_per_channel: int, hop: int | None = None, streams: int = 1, taps="hamming",
                 output: str = "real", phase: str = "time", precision: int = L.F32, device: int = 0, workspace_bytes: int = 0):
        if output not in INPUTS:
            raise ValueError(f"output must be one of {sorted(INPUTS)}")
        if phase not in PHASES:
            raise ValueError(f"phase must be one of {sorted(PHASES)}")
        hop = n_channels if hop is None else hop
        if n_channels <= 0 or taps_per_channel <= 0 or hop <= 0 or hop > n_channels:
            raise ValueError("need n_channels >= 1, taps_per_channel >= 1 and 1 <= hop <= n_channels")
        if streams <= 0:
            raise ValueError("need streams >= 1")
        self._lib = L.load()
        self.n_channels, self.taps_per_channel, self.hop, self.streams = n_channels, taps_per_channel, hop, streams
        self.output, self.phase, self.precision, self.device, self.workspace_bytes = output, phase, precision, device, workspace_bytes
        self.n_taps = n_channels * taps_per_channel
        self.bins = n_channels if output == "complex" else n_channels // 2 + 1
        self.hist = self.n_taps - hop
        if isinstance(taps, str):
            self.taps = pfb_dual_prototype(pfb_prototype(taps, n_channels, taps_per_channel), n_channels, taps_per_channel, hop)
        else:
            self.taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))
            if self.taps.size != self.n_taps:
                raise ValueError("taps length differs from taps_per_channel * n_channels")
        self._plan = None
        self._state = None  # torch tensor (streams, max(hist, 1)) of the output dtype: pending sums of the next call, time order
        self._position = 0
        self._variant = 0

    def _real_dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _in_dtype(self):
        import torch
        return torch.complex128 if self.precision == L.F64 else torch.complex64

    def _out_dtype(self):
        return self._in_dtype() if self.output == "complex" else self._real_dtype()

    def reset(self):
        """forget the pending sums and the stream position"""
        self._state = None
        self._position = 0

    @property
    def state(self):
        return self._state

    @property
    def position(self) -> int:
        """samples per stream produced so far (the phase reference of phase="time")"""
        return self._position

    @position.setter
    def position(self, value: int):
        if value < 0:
            raise ValueError("position must be >= 0")
        self._position = int(value)

    def set_variant(self, v: int):
        """the inner reverse transform's kernel variant (sdsp_hip_fft_plan_set_variant)"""
        if v < 0:
            raise ValueError("variant must be >= 0")
        self._ensure_plan()
        L.check(self._lib.sdsp_hip_pfb_synth_plan_set_variant(self._plan, v))
        self._variant = v

    def _set_unfold_form(self, form: int):
        """measurement and cross-check hook: 1 runs the plain per-position unfold whatever the hop, 0 the form the sizes select"""
        self._ensure_plan()
        L.check(self._lib.sdsp_hip_pfb_synth_plan_set_unfold_form(self._plan, form))

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_pfb_synth_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_pfb_synth_plan_create(C.byref(h), self.n_channels, self.taps_per_channel, self.hop,
                                                             self.taps.ctypes.data, INPUTS[self.output], PHASES[self.phase],
                                                             self.precision, self.workspace_bytes, self.device))
            self._plan = h
            if self._variant:
                L.check(self._lib.sdsp_hip_pfb_synth_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_pfb_synth_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.PfbSynthPlanInfo()
        L.check(self._lib.sdsp_hip_pfb_synth_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        d["unfold"] = i.unfold.decode()
        return d

    def launches(self, frames: int) -> int:
        """kernel launches of one process call of `frames` per stream"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_pfb_synth_plan_launches(self._plan, self.streams, frames, C.byref(n)))
        return n.value

    def process(self, X, frames: int | None = None, out=None):
        """X: contiguous complex device tensor (streams, >= frames, bins); synthesises X[:, :frames] of every stream (default: every
        frame), continuing from the bank's pending sums and position.  Returns a (streams, frames * hop) device tensor of the output
        dtype; out, when given, is a contiguous (streams, >= frames * hop) tensor of that dtype, of which the first frames * hop
        columns are written."""
        import torch
        if (X.dtype != self._in_dtype() or not X.is_cuda or not X.is_contiguous() or X.dim() != 3 or X.shape[2] != self.bins):
            raise ValueError("process needs a contiguous (streams, frames, bins) complex device tensor of the bank precision")
        if X.shape[0] != self.streams:
            raise ValueError("stream count differs from the bank's")
        if X.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        F = X.shape[1] if frames is None else frames
        if F < 0 or F > X.shape[1]:
            raise ValueError("frames must be in [0, X.shape[1]]")
        S = F * self.hop
        dt = self._out_dtype()
        if out is None:
            out = torch.empty((self.streams, S), dtype=dt, device=X.device)
        if (out.dtype != dt or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.device != X.device
                or out.shape[0] != self.streams or out.shape[1] < S):
            raise ValueError("out must be a contiguous (streams, >= frames * hop) device tensor of the bank's output dtype")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((self.streams, max(self.hist, 1)), dtype=dt, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(X.device).cuda_stream
        L.check(self._lib.sdsp_hip_pfb_synth_process(self._plan, X.data_ptr(), X.shape[1] * self.bins, out.data_ptr(), out.shape[1],
                                                     self.streams, F, self._position, self._state.data_ptr(), stream))
        self._position += S
        return out if out.shape[1] == S else out[:, :S]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
