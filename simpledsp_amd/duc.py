"""Host mirror of the digital up-converter bank (include/sdsp_hip.h: sdsp_hip_duc_*).

The bank takes a list of bands (output channel, centre frequency, phase), one baseband complex stream per band, all at the same low
rate.  It interpolates each by `up` through one real n_taps-tap low-pass, shifts it up to its centre frequency and sums the bands of
each output channel, with the oscillator phase continuous across calls.  Same conventions as ddc_bank (band-major rows, per-band device
history carried across calls, set_coeff / set_antiimage_coeff); a call of S samples per band returns a (channels, S * up) device
tensor, complex or real."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ddc import _word

KINDS = {"real": L.DUC_REAL, "complex": L.DUC_COMPLEX}


class duc_bank:
    """A bank of up-converters: bands = [(dst, freq), (dst, freq, phase), ..], freq in cycles per OUTPUT sample and phase in cycles
    (floats in [-0.5, 0.5]) or 32-bit phase words (ints).  All bands share the n_taps-tap low-pass and the interpolation factor `up`;
    row i of the input is band i."""

    def __init__(self, n_taps: int, up: int, bands, channels: int = 1, kind: str = "complex", precision: int = L.F32, device: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}")
        if n_taps <= 0 or up <= 0 or channels <= 0:
            raise ValueError("n_taps, up and channels must be positive")
        bands = [tuple(b) for b in bands]
        if not bands or any(len(b) not in (2, 3) for b in bands):
            raise ValueError("bands must be a non-empty list of (dst, freq) or (dst, freq, phase)")
        self._lib = L.load()
        self.n_taps, self.up, self.channels = n_taps, up, channels
        self.kind, self.precision, self.device = kind, precision, device
        self.bands = [(int(b[0]), _word(b[1]), _word(b[2]) if len(b) == 3 else 0) for b in bands]
        if any(not 0 <= b[0] < channels for b in self.bands):
            raise ValueError("a band names an output channel the bank does not have")
        self.hist = (n_taps - 1) // up
        self.m_coeff = np.zeros(n_taps)
        self._plan = None
        self._state = None  # torch tensor (bands, max(hist, 1)) complex, newest sample first
        self._position = 0
        self._variant = 0

    def set_coeff(self, h):
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if h.size != self.n_taps:
            raise ValueError("coefficient count differs from n_taps")
        self.m_coeff = h.copy()
        self._drop_plan()

    def set_antiimage_coeff(self):
        """Hamming low-pass at 1 / (2 up) of the output rate with gain up: up * scipy.signal.firwin(n_taps, 1 / up), from
        sdsp_hip_resample_design(n_taps, up, 1); needs up >= 2"""
        h = np.zeros(self.n_taps)
        L.check(self._lib.sdsp_hip_resample_design(self.n_taps, self.up, 1, h.ctypes.data))
        self.set_coeff(h)

    def _real_dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _in_dtype(self):
        import torch
        return torch.complex128 if self.precision == L.F64 else torch.complex64

    def _out_dtype(self):
        return self._in_dtype() if self.kind == "complex" else self._real_dtype()

    def reset(self):
        """forget the history and the stream position"""
        self._state = None
        self._position = 0

    @property
    def state(self):
        return self._state

    @property
    def position(self) -> int:
        """input samples per band consumed so far (the oscillator's phase reference is position * up)"""
        return self._position

    @position.setter
    def position(self, value: int):
        if value < 0:
            raise ValueError("position must be >= 0")
        self._position = int(value)

    def out_samples(self, samples: int) -> int:
        """outputs per channel of one call of `samples` per band"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_duc_out_samples(self.up, samples, C.byref(n)))
        return n.value

    def set_variant(self, v: int):
        """0 = the fused kernel, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        self._variant = v
        if self._plan:
            L.check(self._lib.sdsp_hip_duc_plan_set_variant(self._plan, v))

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_duc_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            arr = (L.DucBand * len(self.bands))(*[L.DucBand(*b) for b in self.bands])
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_duc_plan_create(C.byref(h), self.n_taps, self.m_coeff.ctypes.data, self.up, self.channels,
                                                       len(self.bands), C.cast(arr, C.c_void_p), KINDS[self.kind], self.precision,
                                                       self.device))
            self._plan = h
            L.check(self._lib.sdsp_hip_duc_plan_set_variant(h, self._variant))

    def info(self) -> dict:
        """the plan's sdsp_hip_duc_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.DucPlanInfo()
        L.check(self._lib.sdsp_hip_duc_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per band"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_duc_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    def process(self, x, out=None, samples: int | None = None):
        """x: contiguous complex device tensor (bands, in_stride) of the bank precision; converts x[:, :samples] of every band
        (default: the whole row), continuing from the bank's history and position.  Returns a (channels, samples * up) device tensor
        of the output kind; out, when given, is a contiguous (channels, >= samples * up) tensor of that dtype, of which the first
        samples * up columns are written."""
        import torch
        dt = self._in_dtype()
        nb = len(self.bands)
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
            raise ValueError("process needs a contiguous (bands, samples) complex device tensor of the bank precision")
        if x.shape[0] != nb:
            raise ValueError("row count differs from the bank's band count")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        in_stride = x.shape[1]
        samples = in_stride if samples is None else samples
        if samples < 0 or samples > in_stride:
            raise ValueError("block exceeds the row")
        outs = self.out_samples(samples)
        if out is None:
            out = torch.empty((self.channels, outs), dtype=self._out_dtype(), device=x.device)
        if (out.dtype != self._out_dtype() or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or out.device != x.device
                or out.shape[0] != self.channels or out.shape[1] < outs):
            raise ValueError("out must be a contiguous (channels, >= samples * up) device tensor of the bank's output dtype")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((nb, max(self.hist, 1)), dtype=dt, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_duc_process(self._plan, x.data_ptr(), in_stride, out.data_ptr(), out.shape[1], samples,
                                               self._position, self._state.data_ptr(), stream))
        self._position += samples
        return out if out.shape[1] == outs else out[:, :outs]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
