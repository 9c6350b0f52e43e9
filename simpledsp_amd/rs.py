"""Host mirror of the Reed-Solomon decoder banks over GF(256) (include/sdsp_hip.h: sdsp_hip_rs_*).

A decoder takes frames of `interleave` symbol-interleaved codewords of the code (field_poly, fcr, prim, nroots, n), optionally with
erasure flags, and returns the corrected frames ("full") or their data symbols ("data") and a count of corrected symbols per
codeword, -1 where a codeword is beyond the code.  The arithmetic is on integers, so the bytes are those of tests/rs_ref.py in
either kernel variant.  rs_encode is the matching systematic encoder and rs_generator its polynomial, both on the host.  torch is
used for device memory and streams only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

OUT_KINDS = {"full": L.RS_FULL, "data": L.RS_DATA}


def rs_generator(field_poly: int, fcr: int, prim: int, nroots: int) -> np.ndarray:
    """the nroots + 1 coefficients of g(x) = prod (x - alpha^(prim (fcr + j))), the highest first (sdsp_hip_rs_generator)"""
    g = np.zeros(max(int(nroots), 0) + 1, dtype=np.uint8)
    L.check(L.load().sdsp_hip_rs_generator(int(field_poly), int(fcr), int(prim), int(nroots), g.ctypes.data))
    return g


def rs_encode(data, field_poly: int, fcr: int, prim: int, nroots: int, n: int = 255, interleave: int = 1) -> np.ndarray:
    """frames of interleave * (n - nroots) data bytes -> frames of interleave * n bytes: the data symbols, then the parity symbols,
    byte s * interleave + j being symbol s of codeword j (sdsp_hip_rs_encode; on the host)"""
    k = int(n) - int(nroots)
    d = np.ascontiguousarray(data, dtype=np.uint8)
    row = int(interleave) * k
    if row <= 0 or d.size % row != 0:
        raise ValueError("data must hold whole frames of interleave * (n - nroots) bytes")
    frames = d.size // row
    out = np.zeros((frames, int(interleave) * int(n)), dtype=np.uint8)
    L.check(L.load().sdsp_hip_rs_encode(int(field_poly), int(fcr), int(prim), int(nroots), int(n), int(interleave),
                                        d.ctypes.data if d.size else None, frames, out.ctypes.data if out.size else None))
    return out


class rs_decoder:
    """A Reed-Solomon errors-and-erasures decoder for frames of `interleave` codewords; out_kind "full" or "data"."""

    def __init__(self, field_poly: int, fcr: int, prim: int, nroots: int, n: int = 255, interleave: int = 1, out_kind: str = "full",
                 device: int = 0):
        if out_kind not in OUT_KINDS:
            raise ValueError('out_kind must be "full" or "data"')
        self._plan = None
        self._lib = L.load()
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_rs_plan_create(C.byref(h), int(field_poly), int(fcr), int(prim), int(nroots), int(n), int(interleave),
                                                   OUT_KINDS[out_kind], device))
        self._plan = h
        self.field_poly, self.fcr, self.prim, self.nroots, self.n = int(field_poly), int(fcr), int(prim), int(nroots), int(n)
        self.interleave, self.out_kind, self.device = int(interleave), out_kind, device
        self.k, self.t = self.n - self.nroots, self.nroots // 2
        self.frame_bytes = self.interleave * self.n
        self.out_bytes = self.interleave * (self.k if out_kind == "data" else self.n)

    # ---- plan
    @property
    def variant(self) -> int:
        return self.info()["variant"]

    def set_variant(self, v: int):
        """0 = sdsp_rs_wave_kernel, 1 = sdsp_rs_plain_kernel; same bytes"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_rs_plan_set_variant(self._plan, v))

    def info(self) -> dict:
        """the plan's sdsp_hip_rs_plan_info as a dict"""
        i = L.RsPlanInfo()
        L.check(self._lib.sdsp_hip_rs_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, frames: int) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_rs_plan_launches(self._plan, frames, C.byref(n)))
        return n.value

    # ---- frames
    def process_ptr(self, src: int, erasures: int | None, dst: int, corrected: int | None, frames: int, stream: int = 0):
        L.check(self._lib.sdsp_hip_rs_process(self._plan, src, erasures, dst, corrected, frames, stream))

    def _bytes(self, t, frames, row, what):
        import torch
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous()
                or t.numel() != frames * row):
            raise ValueError(f"{what} must be a contiguous uint8 device tensor of {frames} x {row} bytes")
        if t.device.index != self.device:
            raise ValueError("tensor lives on a different device than the decoder")

    def process(self, frames, erasures=None, out=None, corrected=None, stream=None):
        """frames: a contiguous uint8 device tensor of whole frames, (frames, interleave * n) or flat; erasures: the same shape, non-zero
        marks an erased symbol.  out: where the result goes ("full": may be `frames` itself, the in-place form); corrected: an int32
        device tensor of frames * interleave counts, or False for none.  Returns (out, corrected).  Runs on `stream` (a torch stream)
        or torch's current one."""
        import torch
        if not isinstance(frames, torch.Tensor) or frames.numel() % self.frame_bytes != 0:
            raise ValueError("frames must hold whole frames of interleave * n bytes")
        nf = frames.numel() // self.frame_bytes
        self._bytes(frames, nf, self.frame_bytes, "frames")
        if erasures is not None:
            self._bytes(erasures, nf, self.frame_bytes, "erasures")
        if out is None:
            out = torch.empty((nf, self.out_bytes), dtype=torch.uint8, device=frames.device)
        else:
            self._bytes(out, nf, self.out_bytes, "out")
        if corrected is None:
            corrected = torch.empty(nf * self.interleave, dtype=torch.int32, device=frames.device)
        elif corrected is False:
            corrected = None
        elif (not isinstance(corrected, torch.Tensor) or corrected.dtype != torch.int32 or not corrected.is_cuda
              or not corrected.is_contiguous() or corrected.numel() != nf * self.interleave or corrected.device != frames.device):
            raise ValueError("corrected must be a contiguous int32 device tensor of frames * interleave counts")
        s = torch.cuda.current_stream(frames.device) if stream is None else stream
        self.process_ptr(frames.data_ptr() if nf else None, erasures.data_ptr() if erasures is not None and nf else None,
                         out.data_ptr() if nf else None, corrected.data_ptr() if corrected is not None and nf else None, nf, s.cuda_stream)
        return out, corrected

    def process_host(self, frames: np.ndarray, erasures: np.ndarray | None = None):
        """the same on C-contiguous uint8 numpy arrays (H2D, decode, D2H): returns (out, corrected)"""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        if f.size % self.frame_bytes != 0:
            raise ValueError("frames must hold whole frames of interleave * n bytes")
        nf = f.size // self.frame_bytes
        e = None
        if erasures is not None:
            e = np.ascontiguousarray(erasures, dtype=np.uint8)
            if e.size != f.size:
                raise ValueError("erasures must have the frames' size")
        out = np.zeros((nf, self.out_bytes), dtype=np.uint8)
        corrected = np.zeros(nf * self.interleave, dtype=np.int32)
        L.check(self._lib.sdsp_hip_rs_process_host(self._plan, f.ctypes.data if nf else None, e.ctypes.data if e is not None and nf else None,
                                                    out.ctypes.data if nf else None, corrected.ctypes.data if nf else None, nf))
        return out, corrected

    def close(self):
        if getattr(self, "_plan", None):
            self._lib.sdsp_hip_rs_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rs_decode(frames, field_poly: int, fcr: int, prim: int, nroots: int, n: int = 255, interleave: int = 1, erasures=None,
              out_kind: str = "full"):
    """One-shot decoding: frames is a uint8 device tensor or a numpy array of whole frames; returns (out, corrected) of the same kind."""
    is_np = isinstance(frames, np.ndarray)
    device = 0 if is_np else (frames.device.index or 0)
    dec = rs_decoder(field_poly, fcr, prim, nroots, n, interleave, out_kind, device)
    try:
        if is_np:
            return dec.process_host(frames, erasures)
        import torch
        res = dec.process(frames, erasures)
        torch.cuda.current_stream(frames.device).synchronize()
        return res
    finally:
        dec.close()
