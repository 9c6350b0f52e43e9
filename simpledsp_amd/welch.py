"""Host mirror of the Welch PSD bank (include/sdsp_hip.h: sdsp_hip_welch_*).

Welch power spectral density of `channels` real streams at once, accumulated across calls: scipy's segments of n_fft samples every
`hop` samples, detrended, windowed and transformed with the library's real-input FFT; their powers are summed in double on the
device.  welch_bank carries the per-channel history and sums, the stream position and the segment count (the same conventions as
stft_bank: channel-major rows, device tensors); welch() is the one-shot form of scipy.signal.welch(x, axis=-1)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .stft import stft_window

DETRENDS = {"none": L.DETREND_NONE, "constant": L.DETREND_CONSTANT, "linear": L.DETREND_LINEAR}
SCALINGS = {"density": L.SCALING_DENSITY, "spectrum": L.SCALING_SPECTRUM}


def welch_frames(n_fft: int, hop: int, position: int, samples: int) -> int:
    """segments a call of `samples` per channel at stream position `position` counts (sdsp_hip_welch_frames)"""
    n = C.c_uint64(0)
    L.check(L.load().sdsp_hip_welch_frames(n_fft, hop, position, samples, C.byref(n)))
    return n.value


class welch_bank:
    """A bank of `channels` streaming Welch estimators of n_fft-point segments every `hop` samples."""

    def __init__(self, n_fft: int, hop: int, channels: int = 1, window="hann", detrend="constant", scaling: str = "density",
                 fs: float = 1.0, precision: int = L.F32, device: int = 0, workspace_bytes: int = 0):
        if detrend is False or detrend is None:
            detrend = "none"
        if detrend not in DETRENDS:
            raise ValueError(f"detrend must be one of {sorted(DETRENDS)} or False")
        if scaling not in SCALINGS:
            raise ValueError(f"scaling must be one of {sorted(SCALINGS)}")
        if n_fft <= 0 or hop <= 0 or hop > n_fft:
            raise ValueError("need 1 <= hop <= n_fft")
        self._lib = L.load()
        self.n_fft, self.hop, self.channels = n_fft, hop, channels
        self.detrend, self.scaling, self.fs = detrend, scaling, float(fs)
        self.precision, self.device, self.workspace_bytes = precision, device, workspace_bytes
        self.bins = n_fft // 2 + 1
        self.hist = n_fft - 1
        if isinstance(window, str):
            self.window = stft_window(window, n_fft)
        else:
            self.window = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
            if self.window.size != n_fft:
                raise ValueError("window length differs from n_fft")
        self._plan = None
        self._state = None  # torch tensor (channels, n_fft - 1), newest sample first
        self._acc = None    # torch float64 tensor (channels, bins)
        self.position = 0   # samples per channel processed since reset
        self.frames = 0     # segments summed into acc

    def _dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def reset(self):
        """start a new stream: position, segment count, history and sums back to zero"""
        self.position = 0
        self.frames = 0
        self._state = None
        self._acc = None

    @property
    def state(self):
        return self._state

    @property
    def acc(self):
        return self._acc

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_welch_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_welch_plan_create(C.byref(h), self.n_fft, self.hop, self.window.ctypes.data,
                                                         DETRENDS[self.detrend], SCALINGS[self.scaling], self.fs, self.precision,
                                                         self.workspace_bytes, self.device))
            self._plan = h

    def _ensure_buffers(self):
        import torch
        dev = f"cuda:{self.device}"
        if self._state is None:
            self._state = torch.zeros((self.channels, self.hist), dtype=self._dtype(), device=dev)
        if self._acc is None:
            self._acc = torch.zeros((self.channels, self.bins), dtype=torch.float64, device=dev)

    def info(self) -> dict:
        """the plan's sdsp_hip_welch_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.WelchPlanInfo()
        L.check(self._lib.sdsp_hip_welch_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def segments(self, samples: int, position: int | None = None) -> int:
        """segments a call of `samples` per channel counts at `position` (default: the bank's)"""
        return welch_frames(self.n_fft, self.hop, self.position if position is None else position, samples)

    def launches(self, samples: int, position: int | None = None, finalize: bool = False) -> int:
        """kernel launches of one process call of `samples` per channel at `position` (default: the bank's), plus the finalize
        launch when `finalize`"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_welch_plan_launches(self._plan, self.channels, samples,
                                                       self.position if position is None else position, C.byref(n)))
        return n.value + (1 if finalize else 0)

    def process(self, x, samples: int | None = None):
        """x: contiguous device tensor (channels, in_stride); adds the segments that end inside x[:, :samples] of every channel
        (default: the whole row) to the bank's sums, continuing from its history.  Returns the segments counted."""
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
        if samples < 0 or samples > in_stride:
            raise ValueError("block exceeds the row")
        F = self.segments(samples)
        self._ensure_plan()
        self._ensure_buffers()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_welch_process(self._plan, x.data_ptr(), in_stride, self.channels, samples, self.position,
                                                 self._state.data_ptr(), self._acc.data_ptr(), self.bins, stream))
        self.position += samples
        self.frames += F
        return F

    def psd(self, out=None):
        """the Welch estimate of every channel from the segments so far: a (channels, bins) device tensor of the bank dtype
        (into `out` when given, a contiguous tensor of that shape and dtype)"""
        import torch
        if self.frames == 0:
            raise ValueError("no complete segment yet")
        self._ensure_plan()
        self._ensure_buffers()
        if out is None:
            out = torch.empty((self.channels, self.bins), dtype=self._dtype(), device=self._acc.device)
        if (out.dtype != self._dtype() or not out.is_cuda or not out.is_contiguous() or out.shape != (self.channels, self.bins)
                or out.device != self._acc.device):
            raise ValueError("out must be a contiguous (channels, bins) device tensor of the bank dtype")
        stream = torch.cuda.current_stream(out.device).cuda_stream
        L.check(self._lib.sdsp_hip_welch_finalize(self._plan, self._acc.data_ptr(), self.bins, self.frames, out.data_ptr(), self.bins,
                                                  self.channels, stream))
        return out

    def freqs(self) -> np.ndarray:
        """the bin frequencies, np.fft.rfftfreq(n_fft, 1 / fs)"""
        return np.fft.rfftfreq(self.n_fft, 1.0 / self.fs)

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass


def welch(x, fs: float = 1.0, window="hann", nperseg: int = 256, noverlap: int | None = None, nfft: int | None = None,
          detrend="constant", return_onesided: bool = True, scaling: str = "density", average: str = "mean", workspace_bytes: int = 0):
    """scipy.signal.welch(x, fs, window, nperseg, noverlap, nfft, detrend, return_onesided, scaling, axis=-1, average) for a
    (channels, samples) or (samples,) float32 / float64 device tensor: returns (f as a numpy array, Pxx as a device tensor of x's
    dtype and leading shape).  Out of scope (ValueError): nfft != nperseg, two-sided spectra, average other than "mean", a
    non-power-of-two nperseg, fewer samples than nperseg, and detrend functions."""
    import torch
    if nfft is not None and nfft != nperseg:
        raise ValueError("nfft must equal nperseg (no zero padding)")
    if not return_onesided:
        raise ValueError("only one-sided spectra")
    if average != "mean":
        raise ValueError('only average="mean"')
    if callable(detrend):
        raise ValueError('detrend must be "constant", "linear" or False')
    if nperseg < 1 or nperseg & (nperseg - 1):
        raise ValueError("nperseg must be a power of two")
    noverlap = nperseg // 2 if noverlap is None else noverlap
    if not 0 <= noverlap < nperseg:
        raise ValueError("noverlap must be in [0, nperseg)")
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in (torch.float32, torch.float64) or x.dim() not in (1, 2):
        raise ValueError("x must be a (channels, samples) or (samples,) float32 / float64 device tensor")
    if x.shape[-1] < nperseg:
        raise ValueError("fewer samples than nperseg")
    if not isinstance(window, str):
        window = np.asarray(window, dtype=np.float64)
        if window.shape != (nperseg,):
            raise ValueError("window length differs from nperseg")
    x2 = (x[None, :] if x.dim() == 1 else x).contiguous()
    b = welch_bank(nperseg, nperseg - noverlap, x2.shape[0], window=window, detrend=detrend, scaling=scaling, fs=fs,
                   precision=L.F64 if x.dtype == torch.float64 else L.F32, device=x.device.index or 0,
                   workspace_bytes=workspace_bytes)
    # the one-shot call never reads history: no state buffer
    b._ensure_plan()
    acc = torch.zeros((x2.shape[0], b.bins), dtype=torch.float64, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    L.check(b._lib.sdsp_hip_welch_process(b._plan, x2.data_ptr(), x2.shape[1], x2.shape[0], x2.shape[1], 0, None, acc.data_ptr(),
                                          b.bins, stream))
    b._acc, b.frames = acc, b.segments(x2.shape[1])
    b._state = None
    pxx = torch.empty((x2.shape[0], b.bins), dtype=x.dtype, device=x.device)
    L.check(b._lib.sdsp_hip_welch_finalize(b._plan, acc.data_ptr(), b.bins, b.frames, pxx.data_ptr(), b.bins, x2.shape[0], stream))
    return b.freqs(), (pxx[0] if x.dim() == 1 else pxx)
