"""Host mirror of zero-phase forward-backward filtering for biquad cascades (include/sdsp_hip.h: sdsp_hip_filtfilt_*, DESIGN.md
section 5.13).

scipy.signal.sosfiltfilt on the device for many whole records at once: every row is extended at both ends (odd / even / constant),
filtered forward from the cascade's steady state, then backward, and its middle written back in place, in one kernel launch per
workspace slice.  filtfilt_plan takes a cascade in the library's form (sections, kind, a, b, gain); casc_2o_iir.filtfilt uses a
bank's designed coefficients; sosfiltfilt takes scipy's second-order-sections array."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

_PADTYPES = {None: L.PAD_NONE, "none": L.PAD_NONE, "odd": L.PAD_ODD, "even": L.PAD_EVEN, "constant": L.PAD_CONSTANT}


def _padtype(padtype) -> int:
    try:
        return _PADTYPES[padtype]
    except (KeyError, TypeError):
        raise ValueError("padtype must be 'odd', 'even', 'constant' or None") from None


def _coeffs(sections, a, b):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if a.size != 3 * sections:
        raise ValueError("a needs 3 * sections values")
    if b is not None:
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))
        if b.size != 3 * sections:
            raise ValueError("b needs 3 * sections values")
    return a, b


def steady_state(sections: int, kind: int, a, b, gain: float) -> np.ndarray:
    """s[0 .. sections] (sdsp_hip_iir_steady_state): level j of the cascade at s_j v holds its output at s_M v for a constant v"""
    a, b = _coeffs(sections, a, b)
    s = np.zeros(sections + 1)
    L.check(L.load().sdsp_hip_iir_steady_state(sections, kind, a.ctypes.data, None if b is None else b.ctypes.data, gain,
                                               s.ctypes.data))
    return s


def default_padlen(sections: int, kind: int, a, b) -> int:
    """scipy.signal.sosfiltfilt's default edge for this cascade (sdsp_hip_filtfilt_default_padlen)"""
    a, b = _coeffs(sections, a, b)
    p = C.c_uint32(0)
    L.check(L.load().sdsp_hip_filtfilt_default_padlen(sections, kind, a.ctypes.data, None if b is None else b.ctypes.data,
                                                      C.byref(p)))
    return p.value


class filtfilt_plan:
    """Forward-backward filtering with one cascade (shared coefficients) over (channels, samples) device tensors, in place.

    precision: F32, F64 or F32_F64STATE (float samples, double recurrence).  padlen None = scipy's default for the cascade."""

    def __init__(self, sections: int, kind: int, a, b, gain: float, precision: int = L.F32, padtype="odd", padlen=None,
                 device: int = 0, workspace_bytes: int = 0):
        if padlen is not None and padlen < 0:
            raise ValueError("padlen must be >= 0")
        self._lib = L.load()
        self.sections, self.kind, self.gain = sections, kind, float(gain)
        self.a, self.b = _coeffs(sections, a, b)
        self.precision, self.device = precision, device
        self.padtype = _padtype(padtype)
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_filtfilt_plan_create(
            C.byref(h), sections, kind, self.a.ctypes.data, None if self.b is None else self.b.ctypes.data, self.gain, precision,
            self.padtype, -1 if padlen is None else int(padlen), workspace_bytes, device))
        self._plan = h
        self.padlen = self.info()["padlen"]

    def _dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def set_variant(self, v: int):
        """0 = the fused kernel (default), 1 = the direct kernel (bit-identical)"""
        L.check(self._lib.sdsp_hip_filtfilt_plan_set_variant(self._plan, v))

    def info(self) -> dict:
        i = L.FiltfiltPlanInfo()
        L.check(self._lib.sdsp_hip_filtfilt_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def kernel_name(self, data, samples: int | None = None) -> str:
        """the kernel process(data, samples) would launch (the library's own selection function)"""
        buf = C.create_string_buffer(64)
        stride = data.shape[1]
        L.check(self._lib.sdsp_hip_filtfilt_plan_kernel(self._plan, data.data_ptr(), data.shape[0],
                                                        stride if samples is None else samples, stride, buf, 64))
        return buf.value.decode()

    def launches(self, channels: int, samples: int) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_filtfilt_plan_launches(self._plan, channels, samples, C.byref(n)))
        return n.value

    def process(self, data, samples: int | None = None):
        """data: contiguous (channels, stride) device tensor of the plan's sample dtype; filters data[:, :samples] of every row
        in place (default: the whole row) and returns data"""
        import torch
        if data.dtype != self._dtype() or not data.is_cuda or not data.is_contiguous() or data.dim() != 2:
            raise ValueError("filtfilt needs a contiguous (channels, samples) device tensor of the plan dtype")
        if data.device.index != self.device:
            raise ValueError("tensor lives on a different device than the plan")
        stride = data.shape[1]
        samples = stride if samples is None else samples
        if samples > stride or samples < 0:
            raise ValueError("samples must be in [0, data.shape[1]]")
        if samples <= self.padlen:
            raise ValueError(f"the rows need more than padlen = {self.padlen} samples")
        stream = torch.cuda.current_stream(data.device).cuda_stream
        L.check(self._lib.sdsp_hip_filtfilt_process(self._plan, data.data_ptr(), data.shape[0], samples, stride, stream))
        return data

    def __del__(self):
        try:
            if self._plan:
                self._lib.sdsp_hip_filtfilt_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass


_DEFAULT_BUDGET = 256 << 20  # sdsp_hip_filtfilt_plan_create's default slice budget for short edges


def _workspace_for(rows: int, padlen: int, precision: int) -> int:
    """a slice budget that holds `rows` channels in one launch, or 0 (the library's default) where that would exceed it"""
    need = -(-max(rows, 1) // 64) * 64 * padlen * (8 if precision == L.F64 else 4)
    return need if 0 < need <= _DEFAULT_BUDGET else 0


def bank_filtfilt(bank, data, samples=None, padtype="odd", padlen=None):
    """casc_2o_iir.filtfilt: the bank's designed coefficients, kind and precision; the bank's streaming state is not used"""
    key = (_padtype(padtype), padlen)
    plans = bank._filtfilt_plans
    if key not in plans:
        b = None if bank.kind != L.IIR_GENERIC else bank.m_b_coeff
        P = 0 if key[0] == L.PAD_NONE else (default_padlen(bank.m_t, bank.kind, bank.m_a_coeff, b) if padlen is None else padlen)
        plans[key] = filtfilt_plan(bank.m_t, bank.kind, bank.m_a_coeff, b, bank.m_gain, bank.precision, padtype, padlen,
                                   bank.device, _workspace_for(data.shape[0], P, bank.precision))
    return plans[key].process(data, samples)


def sosfiltfilt(sos, x, padtype="odd", padlen=None, precision=None):
    """scipy.signal.sosfiltfilt(sos, x, axis=-1, padtype, padlen) for a 2-D device tensor x (rows = channels); returns a new tensor.

    Each row of sos is normalised by a0 and its b0 is folded into the gain (b0 == 0 is refused).  An odd section count is padded
    with the identity section [1, 0, 0, 1, 0, 0]; the default padlen is computed from the sos given.  precision: default F64 for
    float64 tensors and F32 for float32; F32_F64STATE runs float32 tensors with a double recurrence."""
    import torch
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or sos.shape[0] < 1:
        raise ValueError("sos must have shape (n_sections, 6)")
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.float64)):
        raise ValueError("x must be a 2-D float32 / float64 device tensor (channels, samples)")
    n = sos.shape[0]
    if n > L.MAX_SECTIONS:
        raise ValueError(f"at most {L.MAX_SECTIONS} sections")
    if np.any(sos[:, 3] == 0):
        raise ValueError("a0 must be nonzero")
    if np.any(sos[:, 0] == 0):
        raise ValueError("b0 == 0 cannot be folded into the gain")
    if padlen is None:  # scipy's rule on the caller's sections (the identity section would change its count)
        padlen = 3 * (2 * n + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))
    if padtype is None:
        padlen = 0
    sec = sos / sos[:, 3:4]
    gain = float(np.prod(sec[:, 0]))
    b = np.zeros((n, 3))
    a = np.zeros((n, 3))
    b[:, 0] = 1.0
    b[:, 1:] = sec[:, 1:3] / sec[:, 0:1]
    a[:, 0] = 1.0
    a[:, 1:] = sec[:, 4:6]
    if n % 2:
        b = np.vstack([b, [1.0, 0.0, 0.0]])
        a = np.vstack([a, [1.0, 0.0, 0.0]])
    m = b.shape[0]
    if precision is None:
        precision = L.F64 if x.dtype == torch.float64 else L.F32
    plan = filtfilt_plan(m, L.IIR_GENERIC, a, b, gain, precision, padtype, padlen, x.device.index or 0,
                         _workspace_for(x.shape[0], padlen, precision))
    y = x.to(plan._dtype()).contiguous().clone()
    return plan.process(y)
