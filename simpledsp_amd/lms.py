"""Host mirror of the LMS / NLMS adaptive filter bank (include/sdsp_hip.h: sdsp_hip_lms_*).

`channels` independent adaptive FIR filters of n_taps weights each: process(x, d, mu) filters the reference rows x with the current
weights, compares with the desired rows d and moves the weights with every sample; it returns the a-priori output y and error e.  Same
conventions as the other banks (channel-major rows, per-channel device state carried across calls).  The state is one device buffer:
the weights (channels, n_taps), then the x history (channels, n_taps - 1), newest first; weights() and set_weights() read and write its
first part."""
from __future__ import annotations

import ctypes as C

from . import _lib as L

KINDS = {"real": L.LMS_REAL, "complex": L.LMS_COMPLEX}
MODES = {"lms": L.LMS_LMS, "nlms": L.LMS_NLMS}


class lms_bank:
    """An LMS (mode="lms") or normalised LMS (mode="nlms", step mu / (eps + window energy)) filter bank."""

    def __init__(self, channels: int, n_taps: int, kind: str = "real", precision: int = L.F32, mode: str = "lms", eps: float = 0.0,
                 device: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        if channels <= 0 or n_taps <= 0:
            raise ValueError("channels and n_taps must be positive")
        self._lib = L.load()
        self.channels, self.n_taps, self.kind, self.precision, self.mode, self.eps = channels, n_taps, kind, precision, mode, eps
        self.device = device
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_lms_plan_create(C.byref(h), channels, n_taps, KINDS[kind], precision, MODES[mode], float(eps), device))
        self._plan = h
        self._state = None  # flat torch tensor of channels * (2 n_taps - 1) elements of the row dtype

    def _row_dtype(self):
        import torch
        if self.kind == "complex":
            return torch.complex128 if self.precision == L.F64 else torch.complex64
        return torch.float64 if self.precision == L.F64 else torch.float32

    # ---- state
    def _ensure_state(self):
        import torch
        if self._state is None:
            self._state = torch.zeros(self.channels * (2 * self.n_taps - 1), dtype=self._row_dtype(), device=f"cuda:{self.device}")
        return self._state

    @property
    def state(self):
        """the whole state buffer (flat), or None before the first call"""
        return self._state

    def weights(self):
        """(channels, n_taps) view of the weights inside the state buffer: w[c, t] multiplies x[n - t]"""
        return self._ensure_state()[:self.channels * self.n_taps].view(self.channels, self.n_taps)

    def history(self):
        """(channels, n_taps - 1) view of the x history inside the state buffer, newest first"""
        return self._ensure_state()[self.channels * self.n_taps:].view(self.channels, self.n_taps - 1)

    def set_weights(self, w):
        """copy w (channels, n_taps; a tensor or an array) into the state buffer; the history stays"""
        import torch
        w = torch.as_tensor(w)
        if tuple(w.shape) != (self.channels, self.n_taps):
            raise ValueError("weights must be (channels, n_taps)")
        if w.is_complex() and self.kind != "complex":
            raise ValueError("a real bank takes real weights")
        self.weights().copy_(w.to(self._row_dtype()))

    def set_history(self, h):
        """copy h (channels, n_taps - 1), newest first, into the state buffer; the weights stay"""
        import torch
        h = torch.as_tensor(h)
        if tuple(h.shape) != (self.channels, self.n_taps - 1):
            raise ValueError("history must be (channels, n_taps - 1)")
        self.history().copy_(h.to(self._row_dtype()))

    def reset(self):
        """zero weights, zero history, in place: views from weights() / history() stay valid and nothing is allocated"""
        if self._state is not None:
            self._state.zero_()

    # ---- plan
    def set_variant(self, v: int):
        """0 = the register-resident kernel, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_lms_plan_set_variant(self._plan, v))

    def info(self) -> dict:
        """the plan's sdsp_hip_lms_plan_info as a dict"""
        i = L.LmsPlanInfo()
        L.check(self._lib.sdsp_hip_lms_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def state_bytes(self) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_lms_state_bytes(self._plan, C.byref(n)))
        return n.value

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per row"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_lms_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    # ---- stream
    def process(self, x, d, mu: float, samples: int | None = None, y=None, e=None, want_y: bool = True, want_e: bool = True):
        """x, d: contiguous device tensors (channels, stride) of the bank's row dtype; adapts over [:, :samples] of every row (default:
        the whole of x's rows), continuing from the bank's state.  Returns (y, e), each (channels, samples); y / e, when given, are
        contiguous (channels, >= samples) tensors to write into; want_y / want_e = False skips that output (None is returned)."""
        import torch
        dt = self._row_dtype()
        for t in (x, d):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[0] != self.channels:
                raise ValueError("process needs contiguous (channels, samples) device tensors of the bank's row dtype")
            if t.device.index != self.device:
                raise ValueError("tensor lives on a different device than the bank")
        samples = x.shape[1] if samples is None else samples
        if samples < 0 or samples > x.shape[1] or samples > d.shape[1]:
            raise ValueError("block exceeds the row")

        def out_for(t, want):
            if not want:
                return None
            if t is None:
                return torch.empty((self.channels, samples), dtype=dt, device=x.device)
            if (t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.device != x.device
                    or t.shape[0] != self.channels or t.shape[1] < samples):
                raise ValueError("y and e must be contiguous (channels, >= samples) device tensors of the bank's row dtype")
            return t

        y, e = out_for(y, want_y), out_for(e, want_e)
        st = self._ensure_state()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_lms_process(self._plan, x.data_ptr(), x.shape[1], d.data_ptr(), d.shape[1],
                                               y.data_ptr() if y is not None else None, y.shape[1] if y is not None else 0,
                                               e.data_ptr() if e is not None else None, e.shape[1] if e is not None else 0,
                                               samples, float(mu), st.data_ptr(), stream))
        trim = lambda t: t if t is None or t.shape[1] == samples else t[:, :samples]  # noqa: E731
        return trim(y), trim(e)

    def __del__(self):
        try:
            if self._plan:
                self._lib.sdsp_hip_lms_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass
