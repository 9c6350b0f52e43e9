"""Host mirror of the 2-D CFAR plans (include/sdsp_hip.h: sdsp_hip_cfar2d_*).

A cell-averaging detector over compact range-Doppler maps (maps, D, R): D rows of Doppler, which wrap, by R columns of range, which
have edges -- the POWER output of FftColsPlan(n = D, width = R).  The training cells of (d, r) are the rectangle |i| <= Ld + Gd,
|j| <= Lr + Gr around it without the guard box |i| <= Gd, |j| <= Gr; thr = T c(r) with T their sum and c(r) = alpha / n(r) (or a
constant-false-alarm table made from pfa), det = p > thr, optionally only where p is the maximum of its 3 x 3 neighbourhood.  Beside
the dense maps a plan writes the detections of every map as an ordered list.  The bits are the contract's (tests/cfar2d_ref.py), in
either kernel variant.  torch is used for device memory and streams only."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib as L

EDGES = {"mark": L.CFAR2D_EDGE_MARK, "clip": L.CFAR2D_EDGE_CLIP}

Cfar2dResult = collections.namedtuple("Cfar2dResult", "thr det hits counts")


def _pair(name, v):
    if (not isinstance(v, (tuple, list)) or len(v) != 2
            or any(isinstance(e, bool) or not isinstance(e, (int, np.integer)) or e < 0 for e in v)):
        raise ValueError(f"{name} must be a pair of non-negative ints (doppler, range)")
    return int(v[0]), int(v[1])


def _desc(train, guard, edge, peak, alpha):
    (Ld, Lr), (Gd, Gr) = _pair("train", train), _pair("guard", guard)
    if edge not in EDGES:
        raise ValueError('edge must be "mark" or "clip"')
    return L.Cfar2dDesc(Ld, Gd, Lr, Gr, EDGES[edge], 1 if peak else 0, float(alpha))


def cfar2d_scale(D: int, R: int, train, guard, pfa: float) -> np.ndarray:
    """the constant-false-alarm table c(r) = pfa^(-1 / n(r)) - 1 of R doubles: the CA scale alpha_n / n for the n(r) training cells
    that column r keeps inside the map (sdsp_hip_cfar2d_scale); for edge="clip" plans, and equal to a constant on the interior"""
    out = np.empty(int(R), dtype=np.float64)
    d = _desc(train, guard, "clip", False, 0.0)
    L.check(L.load().sdsp_hip_cfar2d_scale(int(D), int(R), C.byref(d), float(pfa), out.ctypes.data))
    return out


class Cfar2dHits:
    """The hit lists of one call: `raw` is the (maps, cap, 4 | 6) int32 device tensor of the records; doppler, range, power and thr are
    views of it (maps, cap); counts is the (maps,) int32 device tensor of totals, which may exceed cap.  Records at or past
    min(counts[m], cap) were not written."""

    def __init__(self, raw, counts, cap, real):
        self.raw, self.counts, self.cap = raw[:, :cap], counts, cap
        self.doppler, self.range = self.raw[..., 0], self.raw[..., 1]
        values = self.raw[..., 2:].view(real)
        self.power, self.thr = values[..., 0], values[..., 1]

    def numpy(self, m: int) -> np.ndarray:
        """the written records of map m as a structured host array (doppler, range, power, thr)"""
        n = min(int(self.counts[m].item()) & 0xffffffff, self.cap)
        real = np.float32 if self.raw.shape[-1] == 4 else np.float64
        dt = np.dtype([("doppler", np.uint32), ("range", np.uint32), ("power", real), ("thr", real)])
        return np.ascontiguousarray(self.raw[m, :n].cpu().numpy()).view(dt).reshape(n)


class cfar2d_plan:
    """A 2-D CA-CFAR plan for maps of D x R cells: train = (Ld, Lr), guard = (Gd, Gr), exactly one of alpha, pfa and scale (a table of
    R doubles); pfa designs the table of cfar2d_scale."""

    def __init__(self, D: int, R: int, train, guard=(0, 0), alpha: float | None = None, pfa: float | None = None, scale=None,
                 edge: str = "mark", peak: bool = False, max_maps: int = 1, precision: int = L.F32, device: int = 0):
        if sum(v is not None for v in (alpha, pfa, scale)) != 1:
            raise ValueError("give exactly one of alpha, pfa and scale")
        self._h = None
        self._lib = L.load()
        d = _desc(train, guard, edge, peak, alpha if alpha is not None else 0.0)
        table = None
        if pfa is not None:
            table = cfar2d_scale(D, R, train, guard, pfa)
        elif scale is not None:
            table = np.ascontiguousarray(scale, dtype=np.float64)
            if table.shape != (R,):
                raise ValueError("scale must hold R values")
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_cfar2d_plan_create(C.byref(h), int(D), int(R), int(max_maps), C.byref(d),
                                                       table.ctypes.data if table is not None else None, precision, device))
        self._h = h
        self.D, self.R, self.max_maps, self.precision, self.device = int(D), int(R), int(max_maps), precision, device
        self.train, self.guard, self.edge, self.peak = tuple(train), tuple(guard), edge, bool(peak)
        self.scale = table

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdsp_hip_cfar2d_plan_destroy(self._h)
            self._h = None

    __del__ = close

    def set_alpha(self, alpha: float):
        """c(r) = alpha / n(r) from now on (plans made with alpha only)"""
        L.check(self._lib.sdsp_hip_cfar2d_plan_set_alpha(self._h, float(alpha)))

    def set_variant(self, v: int):
        """0 = sdsp_cfar2d_kernel (tiles through LDS), 1 = sdsp_cfar2d_plain_kernel (plain loops from global memory: the cross-check)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_cfar2d_plan_set_variant(self._h, v))

    def launches(self, thr_or_det: bool = True, hits: bool = False) -> int:
        """kernel launches of one process with these outputs"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_cfar2d_plan_launches(self._h, int(bool(thr_or_det)), int(bool(hits)), C.byref(n)))
        return int(n.value)

    def info(self) -> dict:
        """the plan's sdsp_hip_cfar2d_plan_info as a dict"""
        i = L.Cfar2dPlanInfo()
        L.check(self._lib.sdsp_hip_cfar2d_plan_get_info(self._h, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def _real(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def process_ptr(self, p: int, thr: int, det: int, hits: int, counts: int, cap: int, maps: int, stream: int = 0):
        L.check(self._lib.sdsp_hip_cfar2d_process(self._h, p, thr, det, hits, counts, cap, maps, stream))

    def process(self, p, thr: bool = True, det: bool = True, hits: int | None = None) -> Cfar2dResult:
        """p: a contiguous device tensor (maps, D, R) (or (D, R)) of the plan's real dtype, maps <= max_maps.  thr, det: whether to
        write the threshold map and the byte map; hits: the capacity of the list of every map, or None for no list.  Runs on torch's
        current stream; returns Cfar2dResult(thr, det, hits, counts) with None for what was not asked; hits is a Cfar2dHits."""
        import torch
        if (not isinstance(p, torch.Tensor) or p.dtype != self._real() or not p.is_cuda or not p.is_contiguous() or p.dim() not in (2, 3)
                or tuple(p.shape[-2:]) != (self.D, self.R)):
            raise ValueError("process needs a contiguous device tensor (maps, D, R) of the plan's real dtype")
        if p.device.index != self.device:
            raise ValueError("tensor lives on a different device than the plan")
        if hits is not None and (isinstance(hits, bool) or not isinstance(hits, (int, np.integer)) or hits < 0):
            raise ValueError("hits must be a capacity >= 0 or None")
        maps = p.numel() // (self.D * self.R)
        t = torch.empty(p.shape, dtype=p.dtype, device=p.device) if thr else None
        b = torch.empty(p.shape, dtype=torch.uint8, device=p.device) if det else None
        raw = counts = None
        if hits is not None:
            words = 6 if self.precision == L.F64 else 4
            raw = torch.zeros((maps, max(int(hits), 1), words), dtype=torch.int32, device=p.device)  # cap 0: still a pointer
            counts = torch.zeros((maps,), dtype=torch.int32, device=p.device)
        stream = torch.cuda.current_stream(p.device).cuda_stream
        self.process_ptr(p.data_ptr(), t.data_ptr() if thr else 0, b.data_ptr() if det else 0, raw.data_ptr() if raw is not None else 0,
                         counts.data_ptr() if counts is not None else 0, int(hits or 0), maps, stream)
        return Cfar2dResult(t, b, Cfar2dHits(raw, counts, int(hits), self._real()) if raw is not None else None, counts)

    def process_host(self, p: np.ndarray, thr: bool = True, det: bool = True, hits: int | None = None):
        """the same on a C-contiguous numpy array (H2D, detect, D2H): (thr, det, list of structured arrays, counts)"""
        real = np.float64 if self.precision == L.F64 else np.float32
        if p.dtype != real or not p.flags.c_contiguous or p.ndim not in (2, 3) or tuple(p.shape[-2:]) != (self.D, self.R):
            raise ValueError("process_host needs a C-contiguous (maps, D, R) array of the plan's real dtype")
        maps = p.size // (self.D * self.R)
        t = np.empty(p.shape, dtype=real) if thr else None
        b = np.empty(p.shape, dtype=np.uint8) if det else None
        rec = np.dtype([("doppler", np.uint32), ("range", np.uint32), ("power", real), ("thr", real)])
        raw = np.zeros((maps, max(int(hits), 1)), dtype=rec) if hits is not None else None
        counts = np.zeros(maps, dtype=np.uint32) if hits is not None else None
        L.check(self._lib.sdsp_hip_cfar2d_process_host(self._h, p.ctypes.data, t.ctypes.data if thr else None, b.ctypes.data if det else None,
                                                        raw.ctypes.data if raw is not None else None,
                                                        counts.ctypes.data if counts is not None else None, int(hits or 0), maps))
        lists = [raw[m, :min(int(counts[m]), int(hits))] for m in range(maps)] if hits is not None else None
        return t, b, lists, counts


def cfar2d(p, train, guard=(0, 0), alpha=None, pfa=None, scale=None, edge="mark", peak=False, thr=True, det=True, hits=None):
    """one-off detection on a device tensor (maps, D, R) or (D, R): a plan for its shape, one process, the plan dropped"""
    import torch
    if not isinstance(p, torch.Tensor) or p.dtype not in (torch.float32, torch.float64) or p.dim() not in (2, 3):
        raise ValueError("cfar2d needs a float32 / float64 device tensor (maps, D, R) or (D, R)")
    D, R = int(p.shape[-2]), int(p.shape[-1])
    plan = cfar2d_plan(D, R, train, guard, alpha=alpha, pfa=pfa, scale=scale, edge=edge, peak=peak,
                       max_maps=max(1, p.numel() // (D * R)), precision=L.F64 if p.dtype == torch.float64 else L.F32,
                       device=p.device.index or 0)
    try:
        return plan.process(p, thr=thr, det=det, hits=hits)
    finally:
        torch.cuda.current_stream(p.device).synchronize()
        plan.close()


_chain_cache: dict = {}


def range_doppler_detect(cube, window=None, train=(4, 8), guard=(1, 2), pfa: float = 1e-4, cap: int = 1024, edge: str = "mark",
                         peak: bool = True, shift: bool = True):
    """The end of a pulse-Doppler chain: cube is a contiguous complex device tensor (maps, pulses, range bins).  A cached
    FftColsPlan(POWER, shift) turns it into range-Doppler power maps and a cached cfar2d_plan reads that same buffer and lists the
    detections.  Returns (power, Cfar2dHits)."""
    import torch
    from .fft import _torch_dtypes, forward_fft
    from .fft_cols import FftColsPlan
    prec = _torch_dtypes().get(getattr(cube, "dtype", None))
    if prec is None or not isinstance(cube, torch.Tensor) or not cube.is_cuda or not cube.is_contiguous() or cube.dim() != 3:
        raise ValueError("range_doppler_detect needs a contiguous complex64 / complex128 device tensor (maps, pulses, range bins)")
    maps, n, width = (int(v) for v in cube.shape)
    dev = cube.device.index or 0
    w = None if window is None else np.ascontiguousarray(window, dtype=np.float64)
    key = (maps, n, width, prec, dev, None if w is None else w.tobytes(), tuple(train), tuple(guard), float(pfa), edge, bool(peak), bool(shift))
    if key not in _chain_cache:
        _chain_cache[key] = (FftColsPlan(n, width, forward_fft, prec, output="power", shift=shift, window=w, device=dev),
                             cfar2d_plan(n, width, train, guard, pfa=pfa, edge=edge, peak=peak, max_maps=maps, precision=prec, device=dev))
    cols, det = _chain_cache[key]
    power = cols.exec(cube)
    return power, det.process(power, thr=False, det=False, hits=cap).hits
