"""Host mirror of the digital down-converter bank (include/sdsp_hip.h: sdsp_hip_ddc_*).

From `channels` input streams the bank takes a list of bands (source channel, centre frequency, phase), shifts each to baseband,
filters it with one real n_taps-tap low-pass and keeps every `down`-th sample, with the oscillator phase continuous across calls.  Same
conventions as fir_resampler (channel-major rows, per-channel device history carried across calls, set_coeff / set_antialias_coeff);
a call of S samples (a multiple of down) returns a (bands, S / down) complex device tensor."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

KINDS = {"real": L.DDC_REAL, "complex": L.DDC_COMPLEX}


def ddc_phase_word(cycles: float) -> int:
    """round(cycles * 2^32) mod 2^32 for cycles in [-0.5, 0.5] (a frequency in cycles per sample, or a phase in cycles):
    sdsp_hip_ddc_phase_word"""
    w = C.c_uint32(0)
    L.check(L.load().sdsp_hip_ddc_phase_word(float(cycles), C.byref(w)))
    return w.value


def _word(v) -> int:
    """an integer is a phase word as it is; a float is converted"""
    if isinstance(v, (int, np.integer)):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError("an integer phase word must be in [0, 2^32)")
        return int(v)
    return ddc_phase_word(v)


class ddc_bank:
    """A bank of down-converters: bands = [(src, freq), (src, freq, phase), ..], freq in cycles per sample and phase in cycles (floats in
    [-0.5, 0.5]) or 32-bit phase words (ints).  All bands share the n_taps-tap low-pass and the decimation factor `down`."""

    def __init__(self, n_taps: int, down: int, bands, channels: int = 1, kind: str = "real", precision: int = L.F32, device: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}")
        if n_taps <= 0 or down <= 0 or channels <= 0:
            raise ValueError("n_taps, down and channels must be positive")
        bands = [tuple(b) for b in bands]
        if not bands or any(len(b) not in (2, 3) for b in bands):
            raise ValueError("bands must be a non-empty list of (src, freq) or (src, freq, phase)")
        self._lib = L.load()
        self.n_taps, self.down, self.channels = n_taps, down, channels
        self.kind, self.precision, self.device = kind, precision, device
        self.bands = [(int(b[0]), _word(b[1]), _word(b[2]) if len(b) == 3 else 0) for b in bands]
        if any(not 0 <= b[0] < channels for b in self.bands):
            raise ValueError("a band names an input channel the bank does not have")
        self.hist = n_taps - 1
        self.m_coeff = np.zeros(n_taps)
        self._plan = None
        self._state = None  # torch tensor (channels, max(hist, 1)) of the input dtype, newest sample first
        self._position = 0
        self._variant = 0

    def set_coeff(self, h):
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if h.size != self.n_taps:
            raise ValueError("coefficient count differs from n_taps")
        self.m_coeff = h.copy()
        self._drop_plan()

    def set_antialias_coeff(self):
        """Hamming low-pass at 1 / (2 down) of the input rate with unit gain: scipy.signal.firwin(n_taps, 1 / down), from
        sdsp_hip_resample_design(n_taps, 1, down); needs down >= 2"""
        h = np.zeros(self.n_taps)
        L.check(self._lib.sdsp_hip_resample_design(self.n_taps, 1, self.down, h.ctypes.data))
        self.set_coeff(h)

    def _real_dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _out_dtype(self):
        import torch
        return torch.complex128 if self.precision == L.F64 else torch.complex64

    def _in_dtype(self):
        return self._out_dtype() if self.kind == "complex" else self._real_dtype()

    def reset(self):
        """forget the history and the stream position"""
        self._state = None
        self._position = 0

    @property
    def state(self):
        return self._state

    @property
    def position(self) -> int:
        """samples per channel consumed so far (the oscillator's phase reference)"""
        return self._position

    @position.setter
    def position(self, value: int):
        if value < 0:
            raise ValueError("position must be >= 0")
        self._position = int(value)

    def out_samples(self, samples: int) -> int:
        """outputs per band of one call of `samples` per channel (raises unless samples is a multiple of down)"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_ddc_out_samples(self.down, samples, C.byref(n)))
        return n.value

    def set_variant(self, v: int):
        """0 = the fused kernel, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        self._variant = v
        if self._plan:
            L.check(self._lib.sdsp_hip_ddc_plan_set_variant(self._plan, v))

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_ddc_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            arr = (L.DdcBand * len(self.bands))(*[L.DdcBand(*b) for b in self.bands])
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_ddc_plan_create(C.byref(h), self.n_taps, self.m_coeff.ctypes.data, self.down, self.channels,
                                                       len(self.bands), C.cast(arr, C.c_void_p), KINDS[self.kind], self.precision,
                                                       self.device))
            self._plan = h
            L.check(self._lib.sdsp_hip_ddc_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_ddc_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.DdcPlanInfo()
        L.check(self._lib.sdsp_hip_ddc_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per channel"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_ddc_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    def process(self, x, out=None, samples: int | None = None):
        """x: contiguous device tensor (channels, in_stride) of the input dtype (real, or complex for kind="complex"); converts
        x[:, :samples] of every channel (default: the whole row), continuing from the bank's history and position.  Returns a
        (bands, samples / down) complex device tensor; out, when given, is a contiguous (bands, >= samples / down) tensor of that
        dtype, of which the first samples / down columns are written."""
        import torch
        dt = self._in_dtype()
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
            raise ValueError("process needs a contiguous (channels, samples) device tensor of the bank's input dtype")
        if x.shape[0] != self.channels:
            raise ValueError("channel count differs from the bank's")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        in_stride = x.shape[1]
        samples = in_stride if samples is None else samples
        if samples > in_stride:
            raise ValueError("block exceeds the row")
        outs = self.out_samples(samples)
        nb = len(self.bands)
        if out is None:
            out = torch.empty((nb, outs), dtype=self._out_dtype(), device=x.device)
        if (out.dtype != self._out_dtype() or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.device != x.device
                or out.shape[0] != nb or out.shape[1] < outs):
            raise ValueError("out must be a contiguous (bands, >= samples / down) complex device tensor of the bank precision")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((self.channels, max(self.hist, 1)), dtype=dt, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_ddc_process(self._plan, x.data_ptr(), in_stride, out.data_ptr(), out.shape[1], samples,
                                               self._position, self._state.data_ptr(), stream))
        self._position += samples
        return out if out.shape[1] == outs else out[:, :outs]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
