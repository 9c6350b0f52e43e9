"""Host mirror of the symbol-timing recovery bank (include/sdsp_hip.h: sdsp_hip_timing_*).

`channels` independent second-order timing loops on interleaved I/Q rows: process(x, alpha, beta) interpolates every row with the
bank's polyphase table at two strobes per symbol, measures the timing error on the symbol strobes with the bank's detector (Gardner or
zero-crossing) and steers the step through a proportional-plus-integral loop filter whose gains are arguments of the call.  It returns
the symbol strobes y, optionally the detector output err and the tracked period offset, and counts: how many symbols each channel
yielded in this call -- the number depends on the data and differs from channel to channel.  Same conventions as the other banks
(channel-major rows, per-channel device state carried across calls).  The state is one device buffer (layout in the header);
period() and time() are views of it."""
from __future__ import annotations

import ctypes as C
import math

from . import _lib as L

MODES = {"gardner": L.TIMING_GARDNER, "zc_qpsk": L.TIMING_ZC_QPSK, "zc_bpsk": L.TIMING_ZC_BPSK}


def timing_step(sps: float) -> int:
    """the half-symbol step word of sps samples per symbol: round(sps / 2 2^32), ties to even (sdsp_hip_timing_step)"""
    if not (2.0 <= sps <= 128.0):
        raise ValueError("samples per symbol must be in [2, 128]")
    return round(sps * 2.0 ** 31)  # the scaling is exact


def timing_max_out(step0: int, samples: int) -> int:
    """the capacity a row needs for `samples` inputs (sdsp_hip_timing_max_out_for): every half step is at least step0 - 2^31"""
    if not (1 << 32) <= step0 <= (1 << 38):
        raise ValueError("step0 must be in [2^32, 2^38]")
    if not 0 <= samples < (1 << 31):
        raise ValueError("samples must be in [0, 2^31)")
    least = step0 - (1 << 31)
    return (((samples << 32) + least - 1) // least + 1) // 2


def timing_gains(bn: float, zeta: float = math.sqrt(0.5), kd: float = 1.0, sps: float = 2.0):
    """(alpha, beta) of a loop of noise bandwidth bn (cycles per symbol) and damping zeta for a detector of slope kd (units of e per
    symbol of timing offset) at sps samples per symbol: theta = bn / (zeta + 1 / (4 zeta)), d = 1 + 2 zeta theta + theta^2,
    alpha = 4 zeta theta / (d kd) sps / 2, beta = 4 theta^2 / (d kd) sps / 2.  Pure host arithmetic (sdsp_hip_timing_gains is the C
    entry point of the same name)."""
    if not all(math.isfinite(v) and v > 0 for v in (bn, zeta, kd, sps)):
        raise ValueError("bn, zeta, kd and sps must be finite and > 0")
    theta = bn / (zeta + 1.0 / (4.0 * zeta))
    d = 1.0 + 2.0 * zeta * theta + theta * theta
    return 4.0 * zeta * theta / (d * kd) * sps / 2.0, 4.0 * theta * theta / (d * kd) * sps / 2.0


def timing_design(phases: int, taps: int, sps: float, rolloff: float = 0.35):
    """the root-raised-cosine matched prototype of phases x taps doubles for sps samples per symbol (sdsp_hip_timing_design): sampled at
    sps phases per symbol, centred, scaled so that the values sum to `phases`"""
    import numpy as np
    h = np.zeros(max(phases * taps, 1), dtype=np.float64)
    L.check(L.load().sdsp_hip_timing_design(phases, taps, float(sps), float(rolloff), h.ctypes.data))
    return h


class timing_bank:
    """A bank of second-order symbol-timing loops: mode "gardner", "zc_qpsk" or "zc_bpsk"."""

    def __init__(self, channels: int, sps: float, h, phases: int, mode: str = "gardner", precision: int = L.F32, max_dev: float = 0.5,
                 device: int = 0):
        """sps: nominal samples per symbol in [2, 128]; h: the phases x taps prototype (timing_design, or any interpolating filter in
        the arb_resampler convention); max_dev in (0, 0.5] samples per half symbol bounds the integrator"""
        import numpy as np
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        if channels <= 0:
            raise ValueError("channels must be positive")
        taps_all = np.ascontiguousarray(np.asarray(h, dtype=np.float64).reshape(-1))
        if phases <= 0 or taps_all.size == 0 or taps_all.size % phases:
            raise ValueError("h must hold phases x taps values")
        self._lib = L.load()
        self.channels, self.sps, self.phases, self.taps = channels, sps, phases, taps_all.size // phases
        self.mode, self.precision, self.max_dev, self.device = mode, precision, max_dev, device
        self.step0 = timing_step(sps)
        p = C.c_void_p()
        L.check(self._lib.sdsp_hip_timing_plan_create(C.byref(p), channels, precision, MODES[mode], phases, self.taps, taps_all.ctypes.data,
                                                      self.step0, float(max_dev), device))
        self._plan = p
        self._state = None  # flat torch byte tensor, the header's layout

    def _row_dtype(self):
        import torch
        return torch.complex128 if self.precision == L.F64 else torch.complex64

    def _real_dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    # ---- state
    def _ensure_state(self):
        import torch
        if self._state is None:
            self._state = torch.zeros(self.state_bytes(), dtype=torch.uint8, device=f"cuda:{self.device}")
        return self._state

    def state(self):
        """the whole state buffer (bytes), or None before the first call"""
        return self._state

    def _offsets(self):
        """byte offsets of the state's arrays: t, ps, ym, integ, w, parity, history; each at the next multiple of 8"""
        ch, rs = self.channels, 8 if self.precision == L.F64 else 4
        sizes = [8 * ch, 2 * rs * ch, 2 * rs * ch, rs * ch, 4 * ch, 4 * ch, 2 * rs * ch * (self.taps - 1)]
        offs, o = [], 0
        for s in sizes:
            offs.append(o)
            o = (o + s + 7) // 8 * 8
        return offs, sizes

    def time(self):
        """(channels,) int64 view of the Q32.32 stream times inside the state buffer"""
        import torch
        offs, sizes = self._offsets()
        return self._ensure_state()[offs[0]:offs[0] + sizes[0]].view(torch.int64)

    def period(self):
        """(channels,) view of the integrators inside the state buffer: the tracked offset of the half-symbol period, in samples"""
        offs, sizes = self._offsets()
        return self._ensure_state()[offs[3]:offs[3] + sizes[3]].view(self._real_dtype())

    def reset(self):
        """a fresh loop at t = 0 preceded by zeros, in place: views from period() / time() stay valid and nothing is allocated"""
        if self._state is not None:
            self._state.zero_()

    # ---- plan
    def set_variant(self, v: int):
        """0 = the register-resident kernel with the table and the rows in LDS, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_timing_plan_set_variant(self._plan, v))

    def info(self) -> dict:
        """the plan's sdsp_hip_timing_plan_info as a dict"""
        i = L.TimingPlanInfo()
        L.check(self._lib.sdsp_hip_timing_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def state_bytes(self) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_timing_state_bytes(self._plan, C.byref(n)))
        return n.value

    def max_out(self, samples: int) -> int:
        """the capacity a row of y, err or period needs for `samples` inputs"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_timing_max_out(self._plan, samples, C.byref(n)))
        return n.value

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per row"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_timing_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    # ---- stream
    def process(self, x, alpha: float, beta: float, samples: int | None = None, y=None, err=None, period=None, want_err: bool = False,
                want_period: bool = False, counts=None):
        """x: a contiguous complex device tensor (channels, stride) of the bank's precision; runs the loops over [:, :samples] of every
        row (default: the whole of x's rows), continuing from the bank's state.  Returns (y, err, period, counts): y (channels,
        max_out(samples)) complex, err and period alike but real (None unless wanted or given), counts (channels,) int32: row c holds
        counts[c] symbols, what lies behind them is not written.  y, err and period, when given, are contiguous (channels, >=
        max_out(samples)) tensors to write into; counts a contiguous (channels,) int32 tensor."""
        import torch
        ct, rt = self._row_dtype(), self._real_dtype()
        if x.dtype != ct or not x.is_cuda or not x.is_contiguous() or x.dim() != 2 or x.shape[0] != self.channels:
            raise ValueError("process needs a contiguous (channels, samples) complex device tensor of the bank's precision")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        samples = x.shape[1] if samples is None else samples
        if samples < 0 or samples > x.shape[1]:
            raise ValueError("block exceeds the row")
        cap = self.max_out(samples)

        def out_for(t, want, dt):
            if t is None:
                return torch.empty((self.channels, cap), dtype=dt, device=x.device) if want else None
            if (t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.device != x.device
                    or t.shape[0] != self.channels or t.shape[1] < cap):
                raise ValueError("y, err and period must be contiguous (channels, >= max_out(samples)) device tensors of the bank's precision")
            return t

        y, err, period = out_for(y, True, ct), out_for(err, want_err, rt), out_for(period, want_period, rt)
        if counts is None:
            counts = torch.empty((self.channels,), dtype=torch.int32, device=x.device)
        elif counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous() or tuple(counts.shape) != (self.channels,):
            raise ValueError("counts must be a contiguous (channels,) int32 device tensor")
        st = self._ensure_state()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        stride = lambda t: t.shape[1] if t is not None else 0  # noqa: E731
        L.check(self._lib.sdsp_hip_timing_process(self._plan, x.data_ptr(), x.shape[1], ptr(y), stride(y), ptr(err), stride(err),
                                                  ptr(period), stride(period), counts.data_ptr(), samples, float(alpha), float(beta),
                                                  st.data_ptr(), stream))
        trim = lambda t: t if t is None or t.shape[1] == cap else t[:, :cap]  # noqa: E731
        return trim(y), trim(err), trim(period), counts

    def __del__(self):
        try:
            if self._plan:
                self._lib.sdsp_hip_timing_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass
