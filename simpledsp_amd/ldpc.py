"""Host mirror of the LDPC decoder banks for quasi-cyclic codes (include/sdsp_hip.h: sdsp_hip_ldpc_*).

A decoder takes codewords of n = nb * z soft values (int8, or float32 quantised with `scale`; positive favours bit 0, 0 is an
erasure) of the code given by a base matrix of shifts (-1: no block) and the lifting size z, runs at most max_iter iterations of
layered normalised / offset min-sum on integers, and returns hard bits (bytes or packed words), int16 posteriors and a status per
codeword: the iterations run, -1 where the syndrome test still fails.  The arithmetic is on integers, so the results are those of
tests/ldpc_ref.py in either kernel variant.  ldpc_encode is the matching [data | parity] encoder and ldpc_parity_matrix its matrix,
both on the host.  The code is an argument: an 802.11n or 5G NR table is passed as its base matrix, punctured columns fed as zeros.
torch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

IN_KINDS = {"i8": L.LDPC_I8, "f32": L.LDPC_F32}
OUT_KINDS = {"bytes": L.LDPC_BYTES, "packed": L.LDPC_PACKED}


def _base(base):
    b = np.ascontiguousarray(base, dtype=np.int16)
    if b.ndim != 2:
        raise ValueError("base must be a 2-D matrix of shifts, -1 for no block")
    return b


def ldpc_parity_matrix(base, z: int) -> np.ndarray:
    """the m x ceil(k / 32) uint32 words of P with parity = P data over GF(2) for codewords [data | parity], k = n - m
    (sdsp_hip_ldpc_parity_matrix; on the host)"""
    b = _base(base)
    mb, nb = b.shape
    m, k = mb * int(z), max(nb - mb, 0) * int(z)
    P = np.zeros((max(m, 0), (k + 31) // 32), dtype=np.uint32)
    L.check(L.load().sdsp_hip_ldpc_parity_matrix(b.ctypes.data, mb, nb, int(z), P.ctypes.data if P.size else None))
    return P


def ldpc_encode(data, base, z: int) -> np.ndarray:
    """rows of k = (nb - mb) * z data bits (0 / 1 bytes) -> rows of n bits: the data, then the parity (sdsp_hip_ldpc_encode; host)"""
    b = _base(base)
    mb, nb = b.shape
    k, n = (nb - mb) * int(z), nb * int(z)
    d = np.ascontiguousarray(data, dtype=np.uint8)
    if k <= 0 or d.size % k != 0:
        raise ValueError("data must hold whole rows of (nb - mb) * z bits")
    rows = d.size // k
    out = np.zeros((rows, n), dtype=np.uint8)
    L.check(L.load().sdsp_hip_ldpc_encode(b.ctypes.data, mb, nb, int(z), d.ctypes.data if rows else None, rows,
                                          out.ctypes.data if rows else None))
    return out


class ldpc_decoder:
    """A layered min-sum decoder for the quasi-cyclic code (base, z); in_kind "i8" or "f32", out_kind "bytes" or "packed"."""

    def __init__(self, base, z: int, norm: int = 12, beta: int = 0, early_stop: bool = True, in_kind: str = "i8", scale: float = 1.0,
                 out_kind: str = "bytes", out_bits: int | None = None, device: int = 0):
        if in_kind not in IN_KINDS:
            raise ValueError('in_kind must be "i8" or "f32"')
        if out_kind not in OUT_KINDS:
            raise ValueError('out_kind must be "bytes" or "packed"')
        self._plan = None
        self._lib = L.load()
        b = _base(base)
        self.mb, self.nb = b.shape
        self.z = int(z)
        self.n, self.m = self.nb * self.z, self.mb * self.z
        self.k = self.n - self.m
        self.out_bits = self.n if out_bits is None else int(out_bits)
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_ldpc_plan_create(C.byref(h), b.ctypes.data, self.mb, self.nb, self.z, int(norm), int(beta),
                                                     1 if early_stop else 0, IN_KINDS[in_kind], float(scale), OUT_KINDS[out_kind],
                                                     self.out_bits, device))
        self._plan = h
        self.base = b
        self.norm, self.beta, self.early_stop, self.scale = int(norm), int(beta), bool(early_stop), float(scale)
        self.in_kind, self.out_kind, self.device = in_kind, out_kind, device
        self.bits_row = (self.out_bits + 31) // 32 if out_kind == "packed" else self.out_bits  # elements of `bits` per codeword

    # ---- plan
    @property
    def variant(self) -> int:
        return self.info()["variant"]

    def set_variant(self, v: int):
        """0 = sdsp_ldpc_wave_kernel, 1 = sdsp_ldpc_plain_kernel (allocates its workspace); same results"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_ldpc_plan_set_variant(self._plan, v))

    def info(self) -> dict:
        """the plan's sdsp_hip_ldpc_plan_info as a dict"""
        i = L.LdpcPlanInfo()
        L.check(self._lib.sdsp_hip_ldpc_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def launches(self, codewords: int) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_ldpc_plan_launches(self._plan, codewords, C.byref(n)))
        return n.value

    # ---- codewords
    def process_ptr(self, llr: int, bits: int | None, post: int | None, status: int | None, codewords: int, max_iter: int, stream: int = 0):
        L.check(self._lib.sdsp_hip_ldpc_process(self._plan, llr, bits, post, status, codewords, max_iter, stream))

    def _dtypes(self):
        import torch
        return (torch.float32 if self.in_kind == "f32" else torch.int8), (torch.int32 if self.out_kind == "packed" else torch.uint8)

    def _out(self, t, dtype, count, what, like):
        import torch
        if t is None:
            return torch.empty(count, dtype=dtype, device=like.device)
        if t is False:
            return None
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.numel() != count
                or t.device != like.device):
            raise ValueError(f"{what} must be a contiguous {dtype} device tensor of {count} elements")
        return t

    def process(self, llr, max_iter: int = 20, bits=None, post=None, status=None, stream=None):
        """llr: a contiguous device tensor of whole codewords, (codewords, n) or flat: int8, or float32 for an "f32" decoder.  bits
        (uint8, or int32 words for "packed"), post (int16) and status (int32) are made where None and left out where False; at least
        one must remain.  Returns (bits, post, status).  Runs on `stream` (a torch stream) or torch's current one."""
        import torch
        tin, tbits = self._dtypes()
        if (not isinstance(llr, torch.Tensor) or llr.dtype != tin or not llr.is_cuda or not llr.is_contiguous()
                or llr.numel() % self.n != 0):
            raise ValueError(f"llr must be a contiguous {tin} device tensor of whole codewords of {self.n} values")
        if llr.device.index != self.device:
            raise ValueError("tensor lives on a different device than the decoder")
        cw = llr.numel() // self.n
        bits = self._out(bits, tbits, cw * self.bits_row, "bits", llr)
        post = self._out(post, torch.int16, cw * self.n, "post", llr)
        status = self._out(status, torch.int32, cw, "status", llr)
        s = torch.cuda.current_stream(llr.device) if stream is None else stream
        ptr = lambda t: t.data_ptr() if t is not None and cw else None
        self.process_ptr(ptr(llr), ptr(bits), ptr(post), ptr(status), cw, int(max_iter), s.cuda_stream)
        if bits is not None:
            bits = bits.view(cw, self.bits_row)
        if post is not None:
            post = post.view(cw, self.n)
        return bits, post, status

    def process_host(self, llr: np.ndarray, max_iter: int = 20):
        """the same on C-contiguous numpy arrays (H2D, decode, D2H): returns (bits, post, status); packed bits are uint32 words"""
        x = np.ascontiguousarray(llr, dtype=np.float32 if self.in_kind == "f32" else np.int8)
        if x.size % self.n != 0:
            raise ValueError(f"llr must hold whole codewords of {self.n} values")
        cw = x.size // self.n
        bits = np.zeros((cw, self.bits_row), dtype=np.uint32 if self.out_kind == "packed" else np.uint8)
        post = np.zeros((cw, self.n), dtype=np.int16)
        status = np.zeros(cw, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if cw else None
        L.check(self._lib.sdsp_hip_ldpc_process_host(self._plan, ptr(x), ptr(bits), ptr(post), ptr(status), cw, int(max_iter)))
        return bits, post, status

    def close(self):
        if getattr(self, "_plan", None):
            self._lib.sdsp_hip_ldpc_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ldpc_decode(llr, base, z: int, max_iter: int = 20, norm: int = 12, beta: int = 0, early_stop: bool = True, scale: float = 1.0,
                out_kind: str = "bytes", out_bits: int | None = None):
    """One-shot decoding: llr is a device tensor or a numpy array of whole codewords, int8 or float32 (quantised with `scale`);
    returns (bits, post, status) of the same kind."""
    is_np = isinstance(llr, np.ndarray)
    if is_np:
        f32 = llr.dtype.kind == "f"
    else:
        import torch
        f32 = llr.dtype == torch.float32
    device = 0 if is_np else (llr.device.index or 0)
    dec = ldpc_decoder(base, z, norm, beta, early_stop, "f32" if f32 else "i8", scale, out_kind, out_bits, device)
    try:
        if is_np:
            return dec.process_host(llr, max_iter)
        res = dec.process(llr, max_iter)
        torch.cuda.current_stream(llr.device).synchronize()
        return res
    finally:
        dec.close()
