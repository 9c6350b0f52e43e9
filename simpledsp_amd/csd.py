"""Host mirror of the cross-spectral density and coherence bank (include/sdsp_hip.h: sdsp_hip_csd_*).

Welch cross-spectral density conj(X_a) X_b and magnitude-squared coherence of a list of channel pairs of `channels` real streams,
accumulated across calls: the Welch bank's segments, detrending, window and real-input FFT; the cross powers of the pairs and the
auto spectra of the channels are summed in double on the device.  csd_bank carries the per-channel history, the sums, the stream
position and the segment count (the conventions of welch_bank); csd() and coherence() are the one-shot forms of scipy.signal.csd and
scipy.signal.coherence with axis=-1."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .stft import stft_window
from .welch import DETRENDS, SCALINGS, welch_frames


class csd_bank:
    """A bank of streaming cross-spectrum estimators over `pairs` (a list of (a, b) channel indices) of `channels` streams, with
    n_fft-point segments every `hop` samples.  auto=False drops the auto spectra (and with them coherence)."""

    def __init__(self, n_fft: int, hop: int, channels: int, pairs, window="hann", detrend="constant", scaling: str = "density",
                 fs: float = 1.0, precision: int = L.F32, workspace_bytes: int = 0, device: int = 0, auto: bool = True):
        if detrend is False or detrend is None:
            detrend = "none"
        if detrend not in DETRENDS:
            raise ValueError(f"detrend must be one of {sorted(DETRENDS)} or False")
        if scaling not in SCALINGS:
            raise ValueError(f"scaling must be one of {sorted(SCALINGS)}")
        if n_fft <= 0 or hop <= 0 or hop > n_fft:
            raise ValueError("need 1 <= hop <= n_fft")
        self.pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        if channels < 1 or self.pairs.shape[0] < 1:
            raise ValueError("need at least one channel and one pair")
        if self.pairs.min() < 0 or self.pairs.max() >= channels:
            raise ValueError("a pair names a channel outside [0, channels)")
        self._pairs32 = np.ascontiguousarray(self.pairs.astype(np.uint32))
        self.npairs = self.pairs.shape[0]
        self._lib = L.load()
        self.n_fft, self.hop, self.channels = n_fft, hop, channels
        self.detrend, self.scaling, self.fs = detrend, scaling, float(fs)
        self.precision, self.device, self.workspace_bytes, self.auto = precision, device, workspace_bytes, auto
        self.bins = n_fft // 2 + 1
        self.hist = n_fft - 1
        if isinstance(window, str):
            self.window = stft_window(window, n_fft)
        else:
            self.window = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1))
            if self.window.size != n_fft:
                raise ValueError("window length differs from n_fft")
        self._plan = None
        self._state = None     # torch tensor (channels, n_fft - 1), newest sample first
        self._acc_xy = None    # torch float64 tensor (npairs, bins, 2): re, im
        self._acc_auto = None  # torch float64 tensor (channels, bins)
        self.position = 0      # samples per channel processed since reset
        self.frames = 0        # segments summed into the accumulators

    def _dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _cdtype(self):
        import torch
        return torch.complex128 if self.precision == L.F64 else torch.complex64

    def reset(self):
        """start a new stream: position, segment count, history and sums back to zero"""
        self.position = 0
        self.frames = 0
        self._state = None
        self._acc_xy = None
        self._acc_auto = None

    @property
    def state(self):
        return self._state

    @property
    def acc_xy(self):
        """the cross sums: a (npairs, bins, 2) float64 device tensor of re, im"""
        return self._acc_xy

    @property
    def acc_auto(self):
        """the auto sums: a (channels, bins) float64 device tensor (None with auto=False)"""
        return self._acc_auto

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_csd_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_csd_plan_create(C.byref(h), self.n_fft, self.hop, self.window.ctypes.data,
                                                       DETRENDS[self.detrend], SCALINGS[self.scaling], self.fs, self.precision,
                                                       self.channels, self.npairs, self._pairs32.ctypes.data, self.workspace_bytes,
                                                       self.device))
            self._plan = h

    def _ensure_buffers(self, state: bool = True):
        import torch
        dev = f"cuda:{self.device}"
        if self._state is None and state:
            self._state = torch.zeros((self.channels, self.hist), dtype=self._dtype(), device=dev)
        if self._acc_xy is None:
            self._acc_xy = torch.zeros((self.npairs, self.bins, 2), dtype=torch.float64, device=dev)
        if self._acc_auto is None and self.auto:
            self._acc_auto = torch.zeros((self.channels, self.bins), dtype=torch.float64, device=dev)

    def info(self) -> dict:
        """the plan's sdsp_hip_csd_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.CsdPlanInfo()
        L.check(self._lib.sdsp_hip_csd_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def segments(self, samples: int, position: int | None = None) -> int:
        """segments a call of `samples` per channel counts at `position` (default: the bank's)"""
        return welch_frames(self.n_fft, self.hop, self.position if position is None else position, samples)

    def launches(self, samples: int, position: int | None = None, finalize: bool = False) -> int:
        """kernel launches of one process call of `samples` per channel at `position` (default: the bank's), plus one finalize
        launch when `finalize`"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_csd_plan_launches(self._plan, samples, self.position if position is None else position,
                                                     C.byref(n)))
        return n.value + (1 if finalize else 0)

    def _run(self, x, samples: int, with_state: bool):
        import torch
        self._ensure_plan()
        self._ensure_buffers(with_state)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_csd_process(self._plan, x.data_ptr(), x.shape[1], samples, self.position,
                                               self._state.data_ptr() if with_state else None, self._acc_xy.data_ptr(),
                                               2 * self.bins, self._acc_auto.data_ptr() if self.auto else None, self.bins, stream))

    def process(self, x, samples: int | None = None):
        """x: contiguous device tensor (channels, in_stride); adds the segments that end inside x[:, :samples] of every channel
        (default: the whole row) to the bank's sums, continuing from its history.  Returns the segments counted."""
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
        self._run(x, samples, True)
        self.position += samples
        self.frames += F
        return F

    def _finalize(self, mode: int, out, shape, dtype, what: str):
        import torch
        if self.frames == 0:
            raise ValueError("no complete segment yet")
        self._ensure_plan()
        self._ensure_buffers()
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self._acc_xy.device)
        if (out.dtype != dtype or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != shape
                or out.device != self._acc_xy.device):
            raise ValueError(f"out must be a contiguous (npairs, bins) {what} device tensor of the bank precision")
        stream = torch.cuda.current_stream(out.device).cuda_stream
        row = 2 * self.bins if mode == L.CSD_CROSS else self.bins
        L.check(self._lib.sdsp_hip_csd_finalize(self._plan, mode, self._acc_xy.data_ptr(), 2 * self.bins,
                                                self._acc_auto.data_ptr() if self.auto else None, self.bins, self.frames,
                                                out.data_ptr(), row, stream))
        return out

    def csd(self, out=None):
        """the cross-spectral density of every pair from the segments so far: a (npairs, bins) complex device tensor (into `out`
        when given, a contiguous tensor of that shape and dtype)"""
        return self._finalize(L.CSD_CROSS, out, (self.npairs, self.bins), self._cdtype(), "complex")

    def coherence(self, out=None):
        """the magnitude-squared coherence |Pab|^2 / (Paa Pbb) of every pair from the segments so far: a (npairs, bins) real device
        tensor"""
        if not self.auto:
            raise ValueError("coherence needs the auto spectra (auto=True)")
        return self._finalize(L.CSD_COHERENCE, out, (self.npairs, self.bins), self._dtype(), "real")

    def freqs(self) -> np.ndarray:
        """the bin frequencies, np.fft.rfftfreq(n_fft, 1 / fs)"""
        return np.fft.rfftfreq(self.n_fft, 1.0 / self.fs)

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass


def _one_shot(x, y, fs, window, nperseg, noverlap, nfft, detrend, scaling, auto):
    """the bank of a one-shot call after its single process call: x's rows are channels [0, R), y's [R, 2 R), pair i = (i, R + i)"""
    import torch
    if nfft is not None and nfft != nperseg:
        raise ValueError("nfft must equal nperseg (no zero padding)")
    if callable(detrend):
        raise ValueError('detrend must be "constant", "linear" or False')
    if nperseg < 1 or nperseg & (nperseg - 1):
        raise ValueError("nperseg must be a power of two")
    noverlap = nperseg // 2 if noverlap is None else noverlap
    if not 0 <= noverlap < nperseg:
        raise ValueError("noverlap must be in [0, nperseg)")
    for t in (x, y):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.float32, torch.float64) or t.dim() not in (1, 2):
            raise ValueError("x must be a (channels, samples) or (samples,) float32 / float64 device tensor")
    if x.shape != y.shape or x.dtype != y.dtype or x.device != y.device:
        raise ValueError("x and y must have the same shape, dtype and device (no zero padding of the shorter one)")
    if x.shape[-1] < nperseg:
        raise ValueError("fewer samples than nperseg")
    if not isinstance(window, str):
        window = np.asarray(window, dtype=np.float64)
        if window.shape != (nperseg,):
            raise ValueError("window length differs from nperseg")
    xy = torch.cat([x.reshape(-1, x.shape[-1]), y.reshape(-1, y.shape[-1])], dim=0).contiguous()
    rows = xy.shape[0] // 2
    b = csd_bank(nperseg, nperseg - noverlap, 2 * rows, [(i, rows + i) for i in range(rows)], window=window, detrend=detrend,
                 scaling=scaling, fs=fs, precision=L.F64 if x.dtype == torch.float64 else L.F32, device=x.device.index or 0, auto=auto)
    # the one-shot call never reads history: no state buffer
    b._run(xy, xy.shape[1], False)
    b.frames = b.segments(xy.shape[1])
    return b


def csd(x, y, fs: float = 1.0, window="hann", nperseg: int = 256, noverlap: int | None = None, nfft: int | None = None,
        detrend="constant", scaling: str = "density"):
    """scipy.signal.csd(x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided=True, scaling, axis=-1) for two
    (channels, samples) or (samples,) float32 / float64 device tensors of equal shape, paired row by row: returns (f as a numpy
    array, Pxy as a complex device tensor of x's precision and leading shape).  Refused (ValueError): what simpledsp_amd.welch
    refuses, and x and y of different lengths."""
    b = _one_shot(x, y, fs, window, nperseg, noverlap, nfft, detrend, scaling, False)
    p = b.csd()
    return b.freqs(), (p[0] if x.dim() == 1 else p)


def coherence(x, y, fs: float = 1.0, window="hann", nperseg: int = 256, noverlap: int | None = None, nfft: int | None = None,
              detrend="constant"):
    """scipy.signal.coherence(x, y, fs, window, nperseg, noverlap, nfft, detrend, axis=-1) in the form of csd() above: returns
    (f, Cxy as a real device tensor)."""
    b = _one_shot(x, y, fs, window, nperseg, noverlap, nfft, detrend, "density", True)
    c = b.coherence()
    return b.freqs(), (c[0] if x.dim() == 1 else c)
