"""Host mirror of the inverse STFT bank (include/sdsp_hip.h: sdsp_hip_istft_*).

Overlap-add synthesis of `channels` real streams at once from frames of n_fft / 2 + 1 complex bins (stft_bank(output="complex")'s
layout): every frame is transformed back with the library's reverse real-input FFT, multiplied by the synthesis window and added
into the output at `hop` samples per frame.  The pending sums of the last n_fft - hop positions are carried per channel on the
device across calls; a call of F frames returns (channels, F hop) real samples.  normalized=True divides the window by its
squared overlap-add (torch.istft / scipy.signal.istft), so that istft_bank(stft_bank(x)) is x delayed by n_fft - hop samples."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .stft import stft_window


def synthesis_window(n_fft: int, hop: int, window, normalized: bool = True) -> np.ndarray:
    """the synthesis window (double) an istft_bank of these arguments uses (sdsp_hip_istft_synthesis_window)"""
    w = _window(window, n_fft)
    g = np.zeros(n_fft)
    L.check(L.load().sdsp_hip_istft_synthesis_window(n_fft, hop, w.ctypes.data, _norm(normalized), g.ctypes.data))
    return g


def _window(window, n_fft):
    if isinstance(window, str):
        return stft_window(window, n_fft)
    w = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
    if w.size != n_fft:
        raise ValueError("window length differs from n_fft")
    return w


def _norm(normalized):
    return L.ISTFT_NORMALIZED if normalized else L.ISTFT_RAW


class istft_bank:
    """A bank of `channels` streaming inverse STFTs (overlap-add) of n_fft points every `hop` samples with per-channel pending sums."""

    def __init__(self, n_fft: int, hop: int, channels: int = 1, window="hann", normalized: bool = True, precision: int = L.F32,
                 device: int = 0, workspace_bytes: int = 0):
        if n_fft <= 0 or hop <= 0 or hop > n_fft:
            raise ValueError("need 1 <= hop <= n_fft")
        if channels <= 0:
            raise ValueError("need channels >= 1")
        self._lib = L.load()
        self.n_fft, self.hop, self.channels = n_fft, hop, channels
        self.normalized, self.precision, self.device, self.workspace_bytes = bool(normalized), precision, device, workspace_bytes
        self.bins = n_fft // 2 + 1
        self.hist = n_fft - hop
        self.window = _window(window, n_fft)
        self._plan = None
        self._state = None  # torch tensor (channels, max(hist, 1)): pending sums of the next call's first hist outputs, time order
        self._variant = 0

    def _dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _in_dtype(self):
        import torch
        return torch.complex128 if self.precision == L.F64 else torch.complex64

    def reset(self):
        self._state = None

    @property
    def state(self):
        return self._state

    @property
    def synthesis_window(self) -> np.ndarray:
        """the synthesis window in double (the plan rounds it once to its precision)"""
        return synthesis_window(self.n_fft, self.hop, self.window, self.normalized)

    def set_variant(self, v: int):
        """the inner reverse real-input transform's kernel variant (sdsp_hip_fft_plan_set_variant)"""
        if v < 0:
            raise ValueError("variant must be >= 0")
        self._ensure_plan()
        L.check(self._lib.sdsp_hip_istft_plan_set_variant(self._plan, v))
        self._variant = v

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_istft_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_istft_plan_create(C.byref(h), self.n_fft, self.hop, self.window.ctypes.data, _norm(self.normalized),
                                                         self.precision, self.workspace_bytes, self.device))
            self._plan = h
            if self._variant:
                L.check(self._lib.sdsp_hip_istft_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_istft_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.IstftPlanInfo()
        L.check(self._lib.sdsp_hip_istft_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, frames: int) -> int:
        """kernel launches of one process call of `frames` per channel"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_istft_plan_launches(self._plan, self.channels, frames, C.byref(n)))
        return n.value

    def process(self, X, frames: int | None = None, out=None):
        """X: contiguous complex device tensor (channels, >= frames, bins); synthesises X[:, :frames] of every channel (default: every
        frame), continuing from the bank's pending sums.  Returns a (channels, frames hop) device tensor of the bank's real dtype; out,
        when given, is a contiguous (channels, >= frames hop) tensor of that dtype, of which the first frames hop columns are written."""
        import torch
        if (X.dtype != self._in_dtype() or not X.is_cuda or not X.is_contiguous() or X.dim() != 3 or X.shape[2] != self.bins):
            raise ValueError("process needs a contiguous (channels, frames, n_fft // 2 + 1) complex device tensor of the bank precision")
        if X.shape[0] != self.channels:
            raise ValueError("channel count differs from the bank's")
        if X.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        F = X.shape[1] if frames is None else frames
        if F < 0 or F > X.shape[1]:
            raise ValueError("frames must be in [0, X.shape[1]]")
        S = F * self.hop
        if out is None:
            out = torch.empty((self.channels, S), dtype=self._dtype(), device=X.device)
        if (out.dtype != self._dtype() or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.device != X.device
                or out.shape[0] != self.channels or out.shape[1] < S):
            raise ValueError("out must be a contiguous (channels, >= frames * hop) device tensor of the bank dtype")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((self.channels, max(self.hist, 1)), dtype=self._dtype(), device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(X.device).cuda_stream
        L.check(self._lib.sdsp_hip_istft_process(self._plan, X.data_ptr(), X.shape[1] * self.bins, out.data_ptr(), out.shape[1],
                                                 self.channels, F, self._state.data_ptr(), stream))
        return out if out.shape[1] == S else out[:, :S]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
