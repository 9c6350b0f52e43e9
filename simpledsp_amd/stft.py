"""Host mirror of the STFT bank (include/sdsp_hip.h: sdsp_hip_stft_*).

Short-time Fourier transform of `channels` real streams at once: frames of n_fft samples every `hop` samples, multiplied by a
window, transformed with the library's real-input FFT.  Same conventions as fir_resampler (channel-major rows, per-channel device
history carried across calls, preload_filter / reset); a call of S samples (a multiple of hop) returns S / hop frames per channel
as a (channels, frames, n_fft / 2 + 1) device tensor: complex, power (|X|^2) or magnitude (|X|)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

WINDOWS = {"rect": L.WINDOW_RECT, "boxcar": L.WINDOW_RECT, "hann": L.WINDOW_HANN, "hamming": L.WINDOW_HAMMING,
           "blackman": L.WINDOW_BLACKMAN}
OUTPUTS = {"complex": L.STFT_COMPLEX, "power": L.STFT_POWER, "magnitude": L.STFT_MAGNITUDE}


def stft_window(name: str, n: int) -> np.ndarray:
    """periodic window of n points (scipy.signal.get_window(name, n)) from sdsp_hip_stft_window"""
    if name not in WINDOWS:
        raise ValueError(f"window must be one of {sorted(WINDOWS)} or an array")
    w = np.zeros(max(n, 1))
    L.check(L.load().sdsp_hip_stft_window(WINDOWS[name], n, w.ctypes.data))
    return w[:n]


class stft_bank:
    """A bank of `channels` streaming STFTs of n_fft points every `hop` samples with per-channel history."""

    def __init__(self, n_fft: int, hop: int, channels: int = 1, window="hann", output: str = "complex", precision: int = L.F32,
                 device: int = 0, workspace_bytes: int = 0):
        if output not in OUTPUTS:
            raise ValueError(f"output must be one of {sorted(OUTPUTS)}")
        if n_fft <= 0 or hop <= 0 or hop > n_fft:
            raise ValueError("need 1 <= hop <= n_fft")
        self._lib = L.load()
        self.n_fft, self.hop, self.channels = n_fft, hop, channels
        self.output, self.precision, self.device, self.workspace_bytes = output, precision, device, workspace_bytes
        self.bins = n_fft // 2 + 1
        self.hist = n_fft - hop
        if isinstance(window, str):
            self.window = stft_window(window, n_fft)
        else:
            self.window = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
            if self.window.size != n_fft:
                raise ValueError("window length differs from n_fft")
        self._plan = None
        self._state = None  # torch tensor (channels, max(hist, 1)), newest sample first
        self._variant = 0

    def _dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _out_dtype(self):
        import torch
        if self.output == "complex":
            return torch.complex128 if self.precision == L.F64 else torch.complex64
        return self._dtype()

    def preload_filter(self, value: float):  # history of a steady input
        import torch
        self._state = torch.full((self.channels, max(self.hist, 1)), value, dtype=self._dtype(), device=f"cuda:{self.device}")

    def reset(self):
        self._state = None

    @property
    def state(self):
        return self._state

    def frames(self, samples: int) -> int:
        """frames one call of `samples` per channel writes (raises unless samples is a multiple of hop)"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_stft_frames(self.hop, samples, C.byref(n)))
        return n.value

    def set_variant(self, v: int):
        """the inner real-input transform's kernel variant (sdsp_hip_fft_plan_set_variant)"""
        if v < 0:
            raise ValueError("variant must be >= 0")
        self._ensure_plan()
        L.check(self._lib.sdsp_hip_stft_plan_set_variant(self._plan, v))
        self._variant = v

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_stft_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_stft_plan_create(C.byref(h), self.n_fft, self.hop, self.window.ctypes.data, OUTPUTS[self.output],
                                                        self.precision, self.workspace_bytes, self.device))
            self._plan = h
            if self._variant:
                L.check(self._lib.sdsp_hip_stft_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_stft_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.StftPlanInfo()
        L.check(self._lib.sdsp_hip_stft_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per channel"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_stft_plan_launches(self._plan, self.channels, samples, C.byref(n)))
        return n.value

    def process(self, x, samples: int | None = None, out=None):
        """x: contiguous device tensor (channels, in_stride); transforms x[:, :samples] of every channel (default: the whole row),
        continuing from the bank's history.  Returns a (channels, frames, bins) device tensor (complex for output="complex");
        out, when given, is a contiguous (channels, >= frames, bins) tensor of that dtype, of which the first frames are written."""
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
        F = self.frames(samples)
        if out is None:
            out = torch.empty((self.channels, F, self.bins), dtype=self._out_dtype(), device=x.device)
        if (out.dtype != self._out_dtype() or not out.is_cuda or not out.is_contiguous() or out.dim() != 3 or out.device != x.device
                or out.shape[0] != self.channels or out.shape[1] < F or out.shape[2] != self.bins):
            raise ValueError("out must be a contiguous (channels, >= frames, bins) device tensor of the output dtype")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((self.channels, max(self.hist, 1)), dtype=dt, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_stft_process(self._plan, x.data_ptr(), in_stride, out.data_ptr(), out.shape[1] * self.bins,
                                                self.channels, samples, self._state.data_ptr(), stream))
        return out if out.shape[1] == F else out[:, :F]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
