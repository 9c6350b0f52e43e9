"""Host mirror of the streaming Viterbi decoder banks (include/sdsp_hip.h: sdsp_hip_viterbi_*).

A bank decodes one rate-1/n convolutional code (K = 3 .. 9, n = 2 or 3) in many channels at once: rows of steps * n soft values in
(int8, or float32 quantised by the plan's scale), `steps` decoded bits per row out, Dr = block * ceil(depth / block) steps behind the
input.  Every operation is on integers, so the bits are those of tests/viterbi_ref.py in either kernel variant.  conv_encode is the
matching encoder and viterbi_decode a one-shot for whole frames.  torch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

IN_KINDS = {"i8": L.VITERBI_I8, "f32": L.VITERBI_F32}
OUT_KINDS = {"bytes": L.VITERBI_BYTES, "packed": L.VITERBI_PACKED}


def _generators(generators):
    g = [int(v) for v in generators]
    if len(g) not in (2, 3):
        raise ValueError("a code needs 2 or 3 generators")
    return (C.c_uint32 * len(g))(*g)


def viterbi_delay(block: int, depth: int) -> int:
    """Dr = block * ceil(depth / block): the steps between a row's input and its output (sdsp_hip_viterbi_delay)"""
    d = C.c_uint32(0)
    L.check(L.load().sdsp_hip_viterbi_delay(int(block), int(depth), C.byref(d)))
    return int(d.value)


def conv_encode(bits, k: int, generators, terminate: bool = False) -> np.ndarray:
    """the coded bits (0 / 1, uint8) of the rate-1/n code from state 0: n per input bit, generator 0 first; with `terminate`, k - 1
    zero bits follow the input.  Generators are k-bit integers whose most significant bit multiplies the newest input bit."""
    b = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
    g = _generators(generators)
    out = np.empty((b.size + (int(k) - 1 if terminate else 0)) * len(g), dtype=np.uint8)
    L.check(L.load().sdsp_hip_conv_encode(int(k), len(g), g, b.ctypes.data if b.size else None, b.size, int(bool(terminate)),
                                          out.ctypes.data if out.size else None))
    return out


class viterbi_bank:
    """A bank of streaming Viterbi decoders: `max_channels` channels of the code (k, generators), traceback block `block` and depth
    `depth`, input kind "i8" or "f32" (quantised as clamp(rint(x * scale), -127, 127)), output kind "bytes" or "packed"."""

    def __init__(self, k: int, generators, block: int = 32, depth: int | None = None, in_kind: str = "i8", out_kind: str = "bytes",
                 scale: float = 1.0, max_channels: int = 1, device: int = 0):
        if in_kind not in IN_KINDS or out_kind not in OUT_KINDS:
            raise ValueError('in_kind must be "i8" or "f32", out_kind "bytes" or "packed"')
        self._plan = None
        self._lib = L.load()
        g = _generators(generators)
        if depth is None:
            depth = -(-5 * int(k) // int(block)) * int(block)
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_viterbi_plan_create(C.byref(h), int(k), len(g), g, int(block), int(depth), IN_KINDS[in_kind],
                                                        OUT_KINDS[out_kind], float(scale), int(max_channels), device))
        self._plan = h
        self.k, self.n, self.generators, self.block, self.depth = int(k), len(g), tuple(g), int(block), int(depth)
        self.in_kind, self.out_kind, self.scale, self.max_channels, self.device = in_kind, out_kind, float(scale), int(max_channels), device
        self.states = 1 << (self.k - 1)
        self.delay = viterbi_delay(self.block, self.depth)

    # ---- plan
    @property
    def variant(self) -> int:
        """the kernel variant in use: 0 = a wave per channel (K = 7), 1 = the plain kernel"""
        return self.info()["variant"]

    def set_variant(self, v: int):
        """0 = sdsp_viterbi_wave_kernel (K = 7 only), 1 = sdsp_viterbi_plain_kernel; same bits, same state"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_viterbi_plan_set_variant(self._plan, v))

    def info(self) -> dict:
        """the plan's sdsp_hip_viterbi_plan_info as a dict"""
        i = L.ViterbiPlanInfo()
        L.check(self._lib.sdsp_hip_viterbi_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["generators"] = tuple(i.generators)[:i.n]
        d["kernel"] = i.kernel.decode()
        return d

    def state_bytes(self) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_viterbi_plan_state_bytes(self._plan, C.byref(n)))
        return n.value

    def launches(self, channels: int, steps: int) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_viterbi_plan_launches(self._plan, channels, steps, C.byref(n)))
        return n.value

    # ---- state
    def reset(self, start_state: int = -1):
        """a fresh stream in every channel; start_state >= 0 is the encoder's known start state"""
        L.check(self._lib.sdsp_hip_viterbi_plan_reset(self._plan, int(start_state)))

    def metrics(self, channels: int | None = None) -> np.ndarray:
        """the path metrics (channels, states) int32 of the first `channels` channels (default: all), on the host"""
        c = self.max_channels if channels is None else int(channels)
        m = np.empty((c, self.states), dtype=np.int32)
        L.check(self._lib.sdsp_hip_viterbi_plan_get_metrics(self._plan, m.ctypes.data, c))
        return m

    def set_metrics(self, metrics):
        """write (channels, states) int32 metrics into the first channels; the decisions held stay"""
        m = np.ascontiguousarray(metrics, dtype=np.int32)
        if m.ndim != 2 or m.shape[1] != self.states:
            raise ValueError("metrics must be (channels, states)")
        L.check(self._lib.sdsp_hip_viterbi_plan_set_metrics(self._plan, m.ctypes.data, m.shape[0]))

    # ---- stream
    def _in_dtype(self):
        import torch
        return torch.float32 if self.in_kind == "f32" else torch.int8

    def process_ptr(self, src: int, dst: int, channels: int, steps: int, stream: int = 0):
        L.check(self._lib.sdsp_hip_viterbi_process(self._plan, src, dst, channels, steps, stream))

    def process(self, soft, out=None):
        """soft: a contiguous device tensor (channels, steps * n) of int8 or float32, channels <= max_channels, steps a multiple of the
        block.  Returns the decoded bits of the steps Dr earlier: (channels, steps) uint8, or (channels, steps / 32) int32 words for
        "packed" (bit 0 of a word is its oldest step).  Runs on torch's current stream."""
        import torch
        if (not isinstance(soft, torch.Tensor) or soft.dtype != self._in_dtype() or not soft.is_cuda or not soft.is_contiguous()
                or soft.dim() != 2 or soft.shape[1] % self.n != 0):
            raise ValueError("process needs a contiguous (channels, steps * n) device tensor of the bank's input dtype")
        if soft.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        channels, steps = int(soft.shape[0]), int(soft.shape[1]) // self.n
        if steps % self.block != 0:
            raise ValueError("steps must be a multiple of the block")
        shape = (channels, steps // 32) if self.out_kind == "packed" else (channels, steps)
        dt = torch.int32 if self.out_kind == "packed" else torch.uint8
        if out is None:
            out = torch.empty(shape, dtype=dt, device=soft.device)
        elif out.dtype != dt or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != shape or out.device != soft.device:
            raise ValueError("out must be a contiguous device tensor of the output's shape and dtype")
        self.process_ptr(soft.data_ptr(), out.data_ptr(), channels, steps, torch.cuda.current_stream(soft.device).cuda_stream)
        return out

    def process_host(self, soft: np.ndarray) -> np.ndarray:
        """the same on a C-contiguous numpy array (H2D, decode, D2H)"""
        dt = np.float32 if self.in_kind == "f32" else np.int8
        if soft.dtype != dt or not soft.flags.c_contiguous or soft.ndim != 2 or soft.shape[1] % self.n != 0:
            raise ValueError("process_host needs a C-contiguous (channels, steps * n) array of the bank's input dtype")
        channels, steps = soft.shape[0], soft.shape[1] // self.n
        if steps % self.block != 0:
            raise ValueError("steps must be a multiple of the block")
        out = np.zeros((channels, steps // 32), dtype=np.uint32) if self.out_kind == "packed" else np.zeros((channels, steps), dtype=np.uint8)
        L.check(self._lib.sdsp_hip_viterbi_process_host(self._plan, soft.ctypes.data if soft.size else None,
                                                         out.ctypes.data if out.size else None, channels, steps))
        return out

    def close(self):
        if getattr(self, "_plan", None):
            self._lib.sdsp_hip_viterbi_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def viterbi_decode(soft, k: int, generators, block: int = 32, depth: int | None = None, scale: float = 1.0, start_state: int = -1):
    """One-shot decoding of whole frames: soft is a device tensor (channels, T * n) or (T * n,) of int8 or float32 (quantised with
    `scale`).  A fresh bank is reset, the rows are followed by zero soft values (erasures) up to a multiple of `block` plus Dr further
    steps, and the first T bits come back as (channels, T) uint8.  After k - 1 erasure steps every state holds the maximum metric and
    the tie rule picks state 0, so the result is the traceback from a best end state.  depth defaults to the smallest multiple of
    `block` that is >= 5 k.  start_state >= 0 tells the decoder the encoder's start state (0 for conv_encode); without it the first
    bits of a frame rest on the coded symbols alone, and a frame shorter than k - 1 steps cannot be told from its siblings."""
    import torch
    if not isinstance(soft, torch.Tensor) or soft.dtype not in (torch.int8, torch.float32) or soft.dim() not in (1, 2) or not soft.is_cuda:
        raise ValueError("viterbi_decode needs an int8 or float32 device tensor (channels, T * n) or (T * n,)")
    n = len(list(generators))
    rows = soft.reshape(1, -1) if soft.dim() == 1 else soft
    if n not in (2, 3) or rows.shape[1] % n != 0:
        raise ValueError("a row must hold n soft values per step")
    channels, T = int(rows.shape[0]), int(rows.shape[1]) // n
    if channels == 0 or T == 0:
        return torch.zeros((channels, T) if soft.dim() == 2 else (T,), dtype=torch.uint8, device=soft.device)
    bank = viterbi_bank(k, generators, block, depth, "f32" if soft.dtype == torch.float32 else "i8", "bytes", scale, channels,
                        soft.device.index or 0)
    try:
        if start_state >= 0:
            bank.reset(start_state)
        total = -(-T // bank.block) * bank.block + bank.delay
        padded = torch.zeros((channels, total * n), dtype=rows.dtype, device=rows.device)
        padded[:, :T * n] = rows
        bits = bank.process(padded)[:, bank.delay:bank.delay + T].contiguous()
    finally:
        torch.cuda.current_stream(soft.device).synchronize()
        bank.close()
    return bits if soft.dim() == 2 else bits.reshape(-1)
