"""Host mirror of the carrier-recovery PLL / Costas loop bank (include/sdsp_hip.h: sdsp_hip_pll_*).

`channels` independent second-order loops on interleaved I/Q rows: process(x, alpha, beta) de-rotates every row with its own numerically
controlled oscillator, measures the phase error with the bank's detector and steers the oscillator through a proportional-plus-integral
loop filter whose gains are arguments of the call.  It returns the de-rotated rows y, the detector output err and the tracked frequency
offset freq (cycles per sample).  Same conventions as the other banks (channel-major rows, per-channel device state carried across
calls).  The state is one device buffer: the integrators (channels reals), then the phase words (channels uint32); freq() and phase()
are views of it."""
from __future__ import annotations

import ctypes as C
import math

from . import _lib as L

MODES = {"cross": L.PLL_CROSS, "bpsk": L.PLL_BPSK, "qpsk": L.PLL_QPSK}


def pll_gains(bn: float, zeta: float = math.sqrt(0.5), amplitude: float = 1.0, mode: str = "cross"):
    """(alpha, beta) of a loop of noise bandwidth bn (cycles per sample) and damping zeta for a signal of the given amplitude:
    theta = bn / (zeta + 1 / (4 zeta)), d = 1 + 2 zeta theta + theta^2, alpha = 4 zeta theta / (d Kd 2 pi), beta = 4 theta^2 / (d Kd 2 pi),
    with the detector gain per radian Kd = A (cross), A^2 (bpsk), A sqrt(2) (qpsk).  Pure host arithmetic (sdsp_hip_pll_gains is the C
    entry point of the same name)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}")
    if not (math.isfinite(bn) and bn > 0 and math.isfinite(zeta) and zeta > 0 and math.isfinite(amplitude) and amplitude > 0):
        raise ValueError("bn, zeta and amplitude must be finite and > 0")
    theta = bn / (zeta + 1.0 / (4.0 * zeta))
    d = 1.0 + 2.0 * zeta * theta + theta * theta
    kd = {"cross": amplitude, "bpsk": amplitude * amplitude, "qpsk": amplitude * math.sqrt(2.0)}[mode]
    return 4.0 * zeta * theta / (d * kd * (2.0 * math.pi)), 4.0 * theta * theta / (d * kd * (2.0 * math.pi))


class pll_bank:
    """A bank of second-order carrier-recovery loops: mode "cross" (a tone or pilot), "bpsk" or "qpsk" (Costas detectors)."""

    def __init__(self, channels: int, fcw0, mode: str = "cross", precision: int = L.F32, max_dev: float = 0.5, device: int = 0):
        """fcw0: the uint32 centre-frequency words of ddc_phase_word, one per channel or one shared word; max_dev in (0, 0.5] cycles
        per sample bounds the integrator"""
        import numpy as np
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        if channels <= 0:
            raise ValueError("channels must be positive")
        words = np.ascontiguousarray(np.asarray(fcw0, dtype=np.uint32).reshape(-1))
        if words.size not in (1, channels):
            raise ValueError("fcw0 must hold one word or one word per channel")
        self._lib = L.load()
        self.channels, self.mode, self.precision, self.max_dev, self.device = channels, mode, precision, max_dev, device
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_pll_plan_create(C.byref(h), channels, precision, MODES[mode], words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                   words.size, float(max_dev), device))
        self._plan = h
        self._state = None  # flat torch byte tensor: channels reals, then channels uint32

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

    @property
    def state(self):
        """the whole state buffer (bytes), or None before the first call"""
        return self._state

    def _real_bytes(self):
        return self.channels * (8 if self.precision == L.F64 else 4)

    def freq(self):
        """(channels,) view of the integrators inside the state buffer: the tracked frequency offsets in cycles per sample"""
        return self._ensure_state()[:self._real_bytes()].view(self._real_dtype())

    def phase(self):
        """(channels,) int32 view of the phase words inside the state buffer (the bits of the uint32 accumulators)"""
        import torch
        return self._ensure_state()[self._real_bytes():].view(torch.int32)

    def set_freq(self, f):
        """copy f (channels,) into the integrators; the phases stay"""
        import torch
        f = torch.as_tensor(f)
        if tuple(f.shape) != (self.channels,):
            raise ValueError("freq must be (channels,)")
        self.freq().copy_(f.to(self._real_dtype()))

    def set_phase(self, theta):
        """copy the uint32 phase words theta (channels,) into the state buffer; the integrators stay"""
        import numpy as np
        import torch
        if isinstance(theta, torch.Tensor):
            theta = theta.cpu().numpy()
        words = np.ascontiguousarray(np.asarray(theta).astype(np.uint32).reshape(-1))
        if words.size != self.channels:
            raise ValueError("phase must be (channels,)")
        self.phase().copy_(torch.from_numpy(words.view(np.int32)))

    def reset(self):
        """zero integrators, phase 0, in place: views from freq() / phase() stay valid and nothing is allocated"""
        if self._state is not None:
            self._state.zero_()

    # ---- plan
    def set_variant(self, v: int):
        """0 = the register-resident kernel with the tables in LDS, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_pll_plan_set_variant(self._plan, v))

    def info(self) -> dict:
        """the plan's sdsp_hip_pll_plan_info as a dict"""
        i = L.PllPlanInfo()
        L.check(self._lib.sdsp_hip_pll_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def state_bytes(self) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_pll_state_bytes(self._plan, C.byref(n)))
        return n.value

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per row"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_pll_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    # ---- stream
    def process(self, x, alpha: float, beta: float, samples: int | None = None, y=None, err=None, freq=None, want_y: bool = True,
                want_err: bool = True, want_freq: bool = True):
        """x: a contiguous complex device tensor (channels, stride) of the bank's precision; runs the loops over [:, :samples] of every
        row (default: the whole of x's rows), continuing from the bank's state.  Returns (y, err, freq), each (channels, samples); y,
        err and freq, when given, are contiguous (channels, >= samples) tensors to write into (y may be x itself: in place);
        want_* = False skips that output (None is returned)."""
        import torch
        ct, rt = self._row_dtype(), self._real_dtype()
        if x.dtype != ct or not x.is_cuda or not x.is_contiguous() or x.dim() != 2 or x.shape[0] != self.channels:
            raise ValueError("process needs a contiguous (channels, samples) complex device tensor of the bank's precision")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        samples = x.shape[1] if samples is None else samples
        if samples < 0 or samples > x.shape[1]:
            raise ValueError("block exceeds the row")

        def out_for(t, want, dt):
            if not want:
                return None
            if t is None:
                return torch.empty((self.channels, samples), dtype=dt, device=x.device)
            if (t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.device != x.device
                    or t.shape[0] != self.channels or t.shape[1] < samples):
                raise ValueError("y, err and freq must be contiguous (channels, >= samples) device tensors of the bank's precision")
            return t

        y, err, freq = out_for(y, want_y, ct), out_for(err, want_err, rt), out_for(freq, want_freq, rt)
        st = self._ensure_state()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        stride = lambda t: t.shape[1] if t is not None else 0  # noqa: E731
        L.check(self._lib.sdsp_hip_pll_process(self._plan, x.data_ptr(), x.shape[1], ptr(y), stride(y), ptr(err), stride(err), ptr(freq),
                                               stride(freq), samples, float(alpha), float(beta), st.data_ptr(), stream))
        trim = lambda t: t if t is None or t.shape[1] == samples else t[:, :samples]  # noqa: E731
        return trim(y), trim(err), trim(freq)

    def __del__(self):
        try:
            if self._plan:
                self._lib.sdsp_hip_pll_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass
