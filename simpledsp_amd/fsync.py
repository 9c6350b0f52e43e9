"""Host mirror of the streaming frame synchroniser banks (include/sdsp_hip.h: sdsp_hip_fsync_*).

A bank finds the attached sync marker in many rows of bits at once, at any bit offset and in either polarity, follows it with a
SEARCH / VERIFY / LOCK machine per channel and writes the payloads behind accepted markers as compact frames of bytes: the first bit
of a byte the most significant, the inversion and the pseudo-random sequence removed -- what rs_decoder takes as it lies.  The input
is viterbi_bank's output, "bytes" or "packed".  Every operation is on integers, so the frames, records and state are those of
tests/fsync_ref.py in either kernel variant and for any split of a stream into calls.  torch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

CCSDS_ASM = L.FSYNC_CCSDS_ASM
IN_KINDS = {"bytes": L.FSYNC_BYTES, "packed": L.FSYNC_PACKED}
POLARITIES = {"normal": L.FSYNC_NORMAL, "either": L.FSYNC_EITHER}
MODES = ("search", "verify", "lock")


def ccsds_pn(n: int) -> np.ndarray:
    """n bytes of the CCSDS pseudo-randomiser (FF 48 0E C0 ..; sdsp_hip_fsync_ccsds_pn)"""
    out = np.zeros(int(n), dtype=np.uint8)
    L.check(L.load().sdsp_hip_fsync_ccsds_pn(out.ctypes.data if out.size else None, out.size))
    return out


def fsync_max_frames(marker_bits: int, payload_bytes: int, nbits: int) -> int:
    """ceil(nbits / L): the frames one call of nbits can emit per row (sdsp_hip_fsync_max_frames)"""
    n = C.c_uint64(0)
    L.check(L.load().sdsp_hip_fsync_max_frames(int(marker_bits), int(payload_bytes), int(nbits), C.byref(n)))
    return int(n.value)


def attach_sync(frames, marker: int = CCSDS_ASM, marker_bits: int = 32, pn=None, invert: bool = False) -> np.ndarray:
    """the transmit side: (frames, P) payload bytes -> one row of frames * (marker_bits + 8 P) bits (0 / 1, uint8): the marker, then the
    payload XOR pn, all of it inverted with `invert`"""
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    if f.ndim == 1:
        f = f.reshape(1, -1)
    if f.ndim != 2 or f.shape[1] == 0:
        raise ValueError("frames must be (frames, P) bytes")
    q = None
    if pn is not None:
        q = np.ascontiguousarray(pn, dtype=np.uint8)
        if q.shape != (f.shape[1],):
            raise ValueError("pn must hold P bytes")
    bits = np.empty(f.shape[0] * (int(marker_bits) + 8 * f.shape[1]), dtype=np.uint8)
    L.check(L.load().sdsp_hip_fsync_attach(int(marker), int(marker_bits), f.shape[1], None if q is None else q.ctypes.data,
                                           f.ctypes.data if f.size else None, f.shape[0], int(bool(invert)),
                                           bits.ctypes.data if bits.size else None))
    return bits


class frame_sync_bank:
    """A bank of streaming frame synchronisers: `max_channels` channels, a marker of `marker_bits` bits (bit marker_bits - 1 first on the
    line) in front of `payload_bytes` bytes, `tol` marker errors accepted, `verify` further markers before lock, `flywheel` misses
    ridden out in lock, polarity "normal" or "either", an optional pn sequence of payload_bytes bytes, input "bytes" or "packed", at
    most `max_bits` bits per row and call."""

    def __init__(self, marker: int = CCSDS_ASM, marker_bits: int = 32, payload_bytes: int = 1275, tol: int = 0, verify: int = 1,
                 flywheel: int = 1, polarity: str = "either", pn=None, in_kind: str = "bytes", max_channels: int = 1,
                 max_bits: int = 1 << 16, device: int = 0):
        if in_kind not in IN_KINDS or polarity not in POLARITIES:
            raise ValueError('in_kind must be "bytes" or "packed", polarity "normal" or "either"')
        self._plan = None
        self._lib = L.load()
        q = None
        if pn is not None:
            q = np.ascontiguousarray(pn, dtype=np.uint8)
            if q.shape != (int(payload_bytes),):
                raise ValueError("pn must hold payload_bytes bytes")
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_fsync_plan_create(C.byref(h), int(marker), int(marker_bits), int(payload_bytes), int(tol), int(verify),
                                                      int(flywheel), POLARITIES[polarity], None if q is None else q.ctypes.data,
                                                      IN_KINDS[in_kind], int(max_channels), int(max_bits), device))
        self._plan = h
        self.marker, self.marker_bits, self.payload_bytes = int(marker), int(marker_bits), int(payload_bytes)
        self.period = self.marker_bits + 8 * self.payload_bytes
        self.tol, self.verify, self.flywheel, self.polarity, self.in_kind = int(tol), int(verify), int(flywheel), polarity, in_kind
        self.max_channels, self.max_bits, self.device = int(max_channels), int(max_bits), device

    # ---- plan
    @property
    def info(self) -> dict:
        """the plan's sdsp_hip_fsync_plan_info as a dict"""
        i = L.FsyncPlanInfo()
        L.check(self._lib.sdsp_hip_fsync_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    @property
    def variant(self) -> int:
        return self.info["variant"]

    def set_variant(self, v: int):
        """0 = the staged kernels over a packed working row, 1 = sdsp_fsync_plain_kernel; same bits, same state"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_fsync_plan_set_variant(self._plan, v))

    def state_bytes(self) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_fsync_plan_state_bytes(self._plan, C.byref(n)))
        return n.value

    def launches(self, channels: int, nbits: int) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_fsync_plan_launches(self._plan, channels, nbits, C.byref(n)))
        return n.value

    def max_frames(self, nbits: int) -> int:
        return -(-int(nbits) // self.period)

    # ---- state
    def reset(self):
        """a fresh stream in every channel"""
        L.check(self._lib.sdsp_hip_fsync_plan_reset(self._plan))

    def state(self, channels: int | None = None) -> dict:
        """the machine of the first `channels` channels (default: all), on the host: mode (0 search, 1 verify, 2 lock), next, polarity,
        count, misses, pending, seen"""
        c = self.max_channels if channels is None else int(channels)
        u32 = lambda: np.zeros(c, dtype=np.uint32)  # noqa: E731
        u64 = lambda: np.zeros(c, dtype=np.uint64)  # noqa: E731
        s = {"mode": u32(), "next": u64(), "polarity": u32(), "count": u32(), "misses": u32(), "pending": u32(), "seen": u64()}
        L.check(self._lib.sdsp_hip_fsync_plan_get_state(self._plan, *[v.ctypes.data for v in s.values()], c))
        return s

    # ---- stream
    def _nbits(self, cols: int) -> int:
        return cols * 32 if self.in_kind == "packed" else cols

    def process_ptr(self, src: int, out: int, counts: int, pos: int, info: int, channels: int, nbits: int, stream: int = 0):
        L.check(self._lib.sdsp_hip_fsync_process(self._plan, src, out, counts, pos, info, channels, nbits, stream))

    def process(self, bits, records: bool = False):
        """bits: a contiguous device tensor (channels, nbits) of uint8, or (channels, nbits / 32) of int32 for "packed".  Returns
        (frames, counts): frames (channels, max_frames(nbits), payload_bytes) uint8, of which the first counts[c] of row c are
        written; with `records` also pos (int64, the marker's first bit) and info (int32: bits 0-7 the marker distance, bit 8
        inverted, bit 9 flywheel).  Runs on torch's current stream."""
        import torch
        dt = torch.int32 if self.in_kind == "packed" else torch.uint8
        if not isinstance(bits, torch.Tensor) or bits.dtype != dt or not bits.is_cuda or not bits.is_contiguous() or bits.dim() != 2:
            raise ValueError("process needs a contiguous (channels, bits) device tensor of the bank's input dtype")
        if bits.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        channels, nbits = int(bits.shape[0]), self._nbits(int(bits.shape[1]))
        mf = self.max_frames(nbits)
        frames = torch.zeros((channels, mf, self.payload_bytes), dtype=torch.uint8, device=bits.device)
        counts = torch.zeros((channels,), dtype=torch.int32, device=bits.device)
        pos = torch.zeros((channels, mf), dtype=torch.int64, device=bits.device) if records else None
        info = torch.zeros((channels, mf), dtype=torch.int32, device=bits.device) if records else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        self.process_ptr(ptr(bits), ptr(frames), counts.data_ptr() if channels else None, ptr(pos), ptr(info), channels, nbits,
                         torch.cuda.current_stream(bits.device).cuda_stream)
        return (frames, counts, pos, info) if records else (frames, counts)

    def process_host(self, bits: np.ndarray, records: bool = False):
        """the same on a C-contiguous numpy array (uint8, or uint32 words for "packed"): H2D, run, D2H"""
        dt = np.uint32 if self.in_kind == "packed" else np.uint8
        if bits.dtype != dt or not bits.flags.c_contiguous or bits.ndim != 2:
            raise ValueError("process_host needs a C-contiguous (channels, bits) array of the bank's input dtype")
        channels, nbits = bits.shape[0], self._nbits(bits.shape[1])
        mf = self.max_frames(nbits)
        frames = np.zeros((channels, mf, self.payload_bytes), dtype=np.uint8)
        counts = np.zeros(channels, dtype=np.uint32)
        pos = np.zeros((channels, mf), dtype=np.uint64) if records else None
        info = np.zeros((channels, mf), dtype=np.uint32) if records else None
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        L.check(self._lib.sdsp_hip_fsync_process_host(self._plan, ptr(bits), ptr(frames), ptr(counts), ptr(pos), ptr(info), channels, nbits))
        return (frames, counts, pos, info) if records else (frames, counts)

    def close(self):
        if getattr(self, "_plan", None):
            self._lib.sdsp_hip_fsync_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
