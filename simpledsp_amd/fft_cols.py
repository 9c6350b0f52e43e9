"""Host mirror of the column FFT plans (include/sdsp_hip.h: sdsp_hip_fft_cols_*).

Where FftPlan transforms the contiguous rows of (batch, n), FftColsPlan transforms every COLUMN of `batch` compact row-major cubes
(batch, n, width): X[b, k, r] = sum_p w[p] x[b, p, r] W_n^(p k).  That is the Doppler step of a pulse-Doppler chain -- cubes
[cube][pulse][range bin], a window over the pulses, one transform per range bin, optionally the power and zero Doppler in the middle
(shift), in the channel-major layout cfar_bank takes -- and the second axis of a 2-D transform: fft2 / ifft2 run the row kernels of
FftPlan and a column plan, in place, with no transpose and no workspace.  torch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .fft import FftPlan, forward_fft, reverse_fft, _torch_dtypes

OUTPUTS = {"complex": L.FFT_COLS_COMPLEX, "power": L.FFT_COLS_POWER}


class FftColsPlan:
    """A batched transform down the columns of (batch, n, width) cubes: n a power of two in [8, 1024], any width >= 1."""

    def __init__(self, n: int, width: int, T=forward_fft, precision: int = L.F32, output="complex", shift: bool = False, window=None,
                 device: int = 0):
        if output not in OUTPUTS:
            raise ValueError('output must be "complex" or "power"')
        for name, v in (("n", n), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError(f"{name} must be a non-negative int")
        self._h = None
        self._lib = L.load()
        w = None
        if window is not None:
            w = np.ascontiguousarray(window, dtype=np.float64)
            if w.shape != (n,):
                raise ValueError("window must hold n values")
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_fft_cols_plan_create(C.byref(h), int(n), int(width), T.direction, precision, OUTPUTS[output],
                                                         1 if shift else 0, w.ctypes.data if w is not None else None, device))
        self._h = h
        self.n, self.width, self.direction, self.precision = int(n), int(width), T.direction, precision
        self.output, self.shift, self.windowed, self.device = output, bool(shift), w is not None, device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdsp_hip_fft_cols_plan_destroy(self._h)
            self._h = None

    __del__ = close

    def set_variant(self, v: int):
        """0 = sdsp_fft_cols_kernel (registers / one LDS exchange), 1 = sdsp_fft_cols_plain_kernel (the plain sum in double: the
        cross-check)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_fft_cols_plan_set_variant(self._h, v))

    def launches(self, batch: int) -> int:
        """kernel launches of one exec of `batch` cubes"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_fft_cols_plan_launches(self._h, batch, C.byref(n)))
        return int(n.value)

    def info(self) -> dict:
        """the plan's sdsp_hip_fft_cols_plan_info as a dict"""
        i = L.FftColsPlanInfo()
        L.check(self._lib.sdsp_hip_fft_cols_plan_get_info(self._h, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    # ---- dtypes
    def _np_dtypes(self):
        cplx = np.complex128 if self.precision == L.F64 else np.complex64
        real = np.float64 if self.precision == L.F64 else np.float32
        return cplx, (real if self.output == "power" else cplx)

    def _out_torch_dtype(self, x):
        import torch
        if self.output == "power":
            return torch.float64 if self.precision == L.F64 else torch.float32
        return x.dtype

    def exec_ptr(self, in_ptr: int, out_ptr: int, batch: int, stream: int = 0):
        L.check(self._lib.sdsp_hip_fft_cols_exec(self._h, in_ptr, out_ptr, batch, stream))

    def exec(self, x, out=None):
        """x: a contiguous device tensor (batch, n, width) (or (n, width)) of the plan's complex dtype.  out: a contiguous device tensor
        of the same shape -- the complex dtype, or the real dtype for output="power" --, or None: complex output is then written in
        place into x, power into a new tensor.  Runs on torch's current stream; returns the output tensor."""
        import torch
        if (_torch_dtypes().get(x.dtype) != self.precision or not x.is_cuda or not x.is_contiguous() or x.dim() not in (2, 3)
                or tuple(x.shape[-2:]) != (self.n, self.width)):
            raise ValueError("exec needs a contiguous device tensor (batch, n, width) of the plan's complex dtype")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the plan")
        if out is None:
            out = x if self.output == "complex" else torch.empty(x.shape, dtype=self._out_torch_dtype(x), device=x.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != self._out_torch_dtype(x) or not out.is_cuda or not out.is_contiguous()
              or out.shape != x.shape or out.device != x.device):
            raise ValueError("out must be a contiguous device tensor of x's shape and of the plan's output dtype")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        self.exec_ptr(x.data_ptr(), out.data_ptr(), x.numel() // (self.n * self.width), stream)
        return out

    def exec_host(self, a: np.ndarray, out: np.ndarray | None = None) -> np.ndarray:
        """the same on C-contiguous numpy arrays (H2D, transform, D2H); out = None: in place for complex output, a new array for power"""
        cplx, odt = self._np_dtypes()
        if a.dtype != cplx or not a.flags.c_contiguous or a.ndim not in (2, 3) or tuple(a.shape[-2:]) != (self.n, self.width):
            raise ValueError("exec_host needs a C-contiguous (batch, n, width) array of the plan's complex dtype")
        if out is None:
            out = a if self.output == "complex" else np.empty(a.shape, dtype=odt)
        elif out.dtype != odt or not out.flags.c_contiguous or out.shape != a.shape:
            raise ValueError("out must be a C-contiguous array of a's shape and of the plan's output dtype")
        L.check(self._lib.sdsp_hip_fft_cols_exec_host(self._h, a.ctypes.data, out.ctypes.data, a.size // (self.n * self.width)))
        return out


_row_cache: dict = {}
_col_cache: dict = {}


def _fft2(x, T):
    import torch
    prec = _torch_dtypes().get(getattr(x, "dtype", None))
    if prec is None or not isinstance(x, torch.Tensor) or not x.is_cuda or not x.is_contiguous() or x.dim() not in (2, 3):
        raise ValueError("fft2 needs a contiguous complex64 / complex128 device tensor (batch, n, m) or (n, m)")
    n, m = int(x.shape[-2]), int(x.shape[-1])
    dev = x.device.index or 0
    rk, ck = (m, T.direction, prec, dev), (n, m, T.direction, prec, dev)
    if rk not in _row_cache:
        _row_cache[rk] = FftPlan(m, 0, T, prec, max_batch=1, device=dev)
    if ck not in _col_cache:
        _col_cache[ck] = FftColsPlan(n, m, T, prec, device=dev)
    _row_cache[rk].exec(x)
    _col_cache[ck].exec(x)
    return x


def fft2(x):
    """2-D transform of every (n, m) image of a contiguous complex device tensor (batch, n, m), in place: the rows through a cached
    AUTO FftPlan, the columns through a cached FftColsPlan (n a power of two in [8, 1024], m a power of two).  Values: numpy.fft.fft2."""
    return _fft2(x, forward_fft)


def ifft2(x):
    """the inverse of fft2 (REVERSE plans: conjugate twiddles and the 1/n, 1/m scales), in place.  Values: numpy.fft.ifft2."""
    return _fft2(x, reverse_fft)
