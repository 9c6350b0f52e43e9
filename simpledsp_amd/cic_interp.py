"""Host mirror of the CIC interpolator bank (include/sdsp_hip.h: sdsp_hip_cic_interp_*).

Every channel, a stream of 16- or 32-bit integer samples (real, or interleaved I/Q), goes through `order` combs of differential
delay `delay` at the input rate, is zero-stuffed by `up`, and goes through `order` integrators at the output rate: Hogenauer's
interpolator, no multiplies and no coefficients, exact in modular integer arithmetic.  A call of S samples per channel gives up * S
outputs; the bank carries the per-channel input history (order * delay samples), so any split of a stream into calls gives the
same bits.  There is no stream position: every call starts on an input boundary.  Same conventions as cic_decimator."""
from __future__ import annotations

import ctypes as C

from . import _lib as L
from .cic import IN_DTYPES, KINDS, OUTS


def cic_interp_growth(order: int, up: int, delay: int = 1) -> int:
    """bit_length(up ** (order - 1) * delay ** order - 1), the bits the registers need above the input's: sdsp_hip_cic_interp_growth"""
    b = C.c_uint32(0)
    L.check(L.load().sdsp_hip_cic_interp_growth(order, up, delay, C.byref(b)))
    return b.value


def cic_interp_unity_scale(order: int, up: int, delay: int = 1) -> float:
    """1.0 / float(up ** (order - 1) * delay ** order), the scale of unity gain at DC: sdsp_hip_cic_interp_unity_scale"""
    s = C.c_double(0.0)
    L.check(L.load().sdsp_hip_cic_interp_unity_scale(order, up, delay, C.byref(s)))
    return s.value


class cic_interpolator:
    """A bank of CIC interpolators.  in_bits (default: the dtype's width) is the number of significant bits of a sample; with the
    growth it decides the register width, 32 or 64 bits.  out="int" gives int32 / int64 by that width, out="f32" gives
    float32((double)y * scale), scale=None meaning unity gain at DC."""

    def __init__(self, order: int, up: int, delay: int = 1, kind: str = "real", in_dtype: str = "i16", in_bits: int | None = None,
                 out: str = "int", scale: float | None = None, device: int | None = None):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}")
        if in_dtype not in IN_DTYPES:
            raise ValueError(f"in_dtype must be one of {sorted(IN_DTYPES)}")
        if out not in OUTS:
            raise ValueError(f"out must be one of {sorted(OUTS)}")
        self._lib = L.load()
        self.order, self.up, self.delay = order, up, delay
        self.kind, self.in_dtype, self.out = kind, in_dtype, out
        self.in_bits = (32 if in_dtype == "i32" else 16) if in_bits is None else in_bits
        self.growth = cic_interp_growth(order, up, delay)
        self.scale = cic_interp_unity_scale(order, up, delay) if scale is None else float(scale)
        self.device = 0 if device is None else device
        self.hist = order * delay
        self.reg_bits = 32 if self.in_bits + self.growth <= 32 else 64
        self._plan = None
        self._state = None  # torch tensor (channels, hist[, 2]) of the input dtype, newest sample first
        self._variant = 0
        self._segment = 0

    def _in_torch(self):
        import torch
        return torch.int32 if self.in_dtype == "i32" else torch.int16

    def _out_torch(self):
        import torch
        if self.out == "f32":
            return torch.float32
        return torch.int64 if self.reg_bits == 64 else torch.int32

    def reset(self):
        """forget the history"""
        self._state = None

    @property
    def state(self):
        return self._state

    def out_samples(self, samples: int) -> int:
        """outputs per channel of a call of `samples` per channel"""
        if not 0 <= samples * self.up < 1 << 31:
            raise ValueError("up * samples must be in [0, 2^31)")
        return samples * self.up

    def set_variant(self, v: int):
        """0 = the scan kernel, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        self._variant = v
        if self._plan:
            L.check(self._lib.sdsp_hip_cic_interp_plan_set_variant(self._plan, v))

    def set_segment(self, chunks: int):
        """chunks of output per workgroup of the scan kernel, 0 = automatic (same bits)"""
        if not 0 <= chunks < 1 << 20:
            raise ValueError("chunks must be in [0, 2^20)")
        self._segment = chunks
        if self._plan:
            L.check(self._lib.sdsp_hip_cic_interp_plan_set_segment(self._plan, chunks))

    def _drop_plan(self):
        if self._plan:
            self._lib.sdsp_hip_cic_interp_plan_destroy(self._plan)
            self._plan = None

    def _ensure_plan(self):
        if self._plan is None:
            h = C.c_void_p()
            L.check(self._lib.sdsp_hip_cic_interp_plan_create(C.byref(h), self.order, self.up, self.delay, IN_DTYPES[self.in_dtype],
                                                              self.in_bits, KINDS[self.kind], OUTS[self.out], self.scale, self.device))
            self._plan = h
            L.check(self._lib.sdsp_hip_cic_interp_plan_set_variant(h, self._variant))
            L.check(self._lib.sdsp_hip_cic_interp_plan_set_segment(h, self._segment))

    def info(self) -> dict:
        """the plan's sdsp_hip_cic_interp_plan_info as a dict (creates the plan)"""
        self._ensure_plan()
        i = L.CicInterpPlanInfo()
        L.check(self._lib.sdsp_hip_cic_interp_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per channel"""
        self._ensure_plan()
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_cic_interp_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    def process(self, x, out=None, samples: int | None = None):
        """x: contiguous device tensor of the bank's integer dtype, (channels, in_stride) for kind="real" and (channels, in_stride, 2)
        for kind="complex"; interpolates x[:, :samples] of every channel (default: the whole row), continuing from the bank's
        history.  Returns a (channels, up * samples[, 2]) device tensor of int32 / int64 / float32; out, when given, is a contiguous
        (channels, >= up * samples[, 2]) tensor of that dtype, of which the first up * samples columns are written."""
        import torch
        cplx = self.kind == "complex"
        dims = 3 if cplx else 2
        if (x.dtype != self._in_torch() or not x.is_cuda or not x.is_contiguous() or x.dim() != dims or (cplx and x.shape[2] != 2)):
            raise ValueError("process needs a contiguous (channels, samples[, 2]) device tensor of the bank's integer dtype")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        channels, in_stride = x.shape[0], x.shape[1]
        if self._state is not None and self._state.shape[0] != channels:
            raise ValueError("channel count differs from the carried history's (reset() starts a new stream)")
        samples = in_stride if samples is None else samples
        if samples > in_stride:
            raise ValueError("block exceeds the row")
        outs = self.out_samples(samples)
        odt = self._out_torch()
        tail = (2,) if cplx else ()
        if out is None:
            out = torch.empty((channels, outs) + tail, dtype=odt, device=x.device)
        if (out.dtype != odt or not out.is_cuda or not out.is_contiguous() or out.dim() != dims or out.device != x.device
                or out.shape[0] != channels or out.shape[1] < outs or (cplx and out.shape[2] != 2)):
            raise ValueError("out must be a contiguous (channels, >= up * samples[, 2]) device tensor of the bank's output dtype")
        self._ensure_plan()
        if self._state is None:
            self._state = torch.zeros((channels, self.hist) + tail, dtype=x.dtype, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_cic_interp_process(self._plan, x.data_ptr(), in_stride, out.data_ptr(), out.shape[1], channels, samples,
                                                      self._state.data_ptr(), stream))
        return out if out.shape[1] == outs else out[:, :outs]

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass
