"""Host mirror of the CFAR detector bank (include/sdsp_hip.h: sdsp_hip_cfar_*).

`channels` independent rows of power (or of complex I/Q samples, which become power re re + im im on the way in).  With train = L,
guard = G, half = L + G and W = 2 half + 1, process(x) returns for every input sample n a threshold made from the 2 L training cells
around the cell under test p[n - half] (L on each side, G guard cells apart from it) and the decision p[n - half] > thr as one byte:
the bank is causal with a delay of half samples.  Modes: "ca" (the mean of all 2 L cells), "go" / "so" (the greater / smaller of the
two side means), "os" (the element of rank k of the 2 L cells), each times alpha.  Same conventions as the other banks (channel-major
rows, per-channel device state carried across calls).  The state is one device buffer: the x history (channels, W - 1), newest first.
cfar() serves finite rows such as range profiles; cfar_alpha() designs alpha for a false-alarm probability."""
from __future__ import annotations

import ctypes as C

from . import _lib as L

MODES = {"ca": L.CFAR_CA, "go": L.CFAR_GO, "so": L.CFAR_SO, "os": L.CFAR_OS}
INPUTS = {"power": L.CFAR_POWER, "iq": L.CFAR_IQ}


def _mode(mode) -> int:
    if isinstance(mode, str) and mode.lower() in MODES:
        return MODES[mode.lower()]
    if not isinstance(mode, (bool, str)) and mode in MODES.values():
        return int(mode)
    raise ValueError('mode must be "ca", "go", "so" or "os"')


def default_rank(train: int) -> int:
    """the OS rank used when none is given: three quarters of the way up the 2 L training cells"""
    return (3 * 2 * train) // 4


def cfar_alpha(mode, train: int, pfa: float, rank: int | None = None) -> float:
    """alpha for a false-alarm probability pfa in square-law detected exponential noise (independent cells).
    CA: alpha = N (pfa^(-1/N) - 1) with N = 2 train.  OS: alpha solves prod_{i=0..k} (N - i) / (N - i + alpha) = pfa (bisection), k the
    rank (default (3 N) // 4).  GO and SO have no designer: give alpha yourself."""
    m = _mode(mode)
    if isinstance(train, bool) or not isinstance(train, int) or train < 1:
        raise ValueError("train must be a positive int")
    if not 0.0 < pfa < 1.0:
        raise ValueError("pfa must be in (0, 1)")
    n = 2 * train
    if m == L.CFAR_CA:
        return n * (pfa ** (-1.0 / n) - 1.0)
    if m != L.CFAR_OS:
        raise ValueError("no designer for GO and SO: give alpha")
    k = default_rank(train) if rank is None else rank
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < n:
        raise ValueError("rank must be in [0, 2 train)")

    def prob(a):
        p = 1.0
        for i in range(k + 1):
            p *= (n - i) / (n - i + a)
        return p

    lo, hi = 0.0, 1.0
    while prob(hi) > pfa:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if prob(mid) > pfa:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _resolve_alpha(mode, train, alpha, pfa, rank):
    if (alpha is None) == (pfa is None):
        raise ValueError("give exactly one of alpha and pfa")
    return float(alpha) if alpha is not None else cfar_alpha(mode, train, pfa, rank)


class cfar_bank:
    """A streaming CFAR detector over every row: thresholds and one-byte decisions, delayed by train + guard samples."""

    def __init__(self, channels: int, train: int, guard: int, mode="ca", alpha: float | None = None, pfa: float | None = None,
                 rank: int | None = None, input="power", precision: int = L.F32, device: int = 0):
        self.mode = _mode(mode)
        if input not in INPUTS:
            raise ValueError('input must be "power" or "iq"')
        if precision not in (L.F32, L.F64):
            raise ValueError("precision must be F32 or F64")
        for name, v in (("channels", channels), ("train", train), ("guard", guard)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an int")
        if channels <= 0:
            raise ValueError("channels must be positive")
        if not 1 <= train <= L.CFAR_MAX_TRAIN:
            raise ValueError(f"train must be in [1, {L.CFAR_MAX_TRAIN}]")
        if not 0 <= guard <= L.CFAR_MAX_GUARD:
            raise ValueError(f"guard must be in [0, {L.CFAR_MAX_GUARD}]")
        if self.mode == L.CFAR_OS:
            limit = L.RANK_MAX_WINDOW_F64 if precision == L.F64 else L.RANK_MAX_WINDOW
            if 2 * train > limit:
                raise ValueError(f"OS mode: 2 train must be at most {limit} for this precision")
            rank = default_rank(train) if rank is None else rank
            if isinstance(rank, bool) or not isinstance(rank, int) or not 0 <= rank < 2 * train:
                raise ValueError("rank must be in [0, 2 train)")
        else:
            rank = 0
        self.alpha = _resolve_alpha(self.mode, train, alpha, pfa, rank if self.mode == L.CFAR_OS else None)
        self._plan = None
        self._lib = L.load()
        self.channels, self.train, self.guard, self.rank = channels, train, guard, rank
        self.half, self.window = train + guard, 2 * (train + guard) + 1
        self.input, self.precision, self.device = input, precision, device
        d = L.CfarDesc(train, guard, self.mode, rank, INPUTS[input], self.alpha)
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_cfar_plan_create(C.byref(h), channels, C.byref(d), precision, device))
        self._plan = h
        self._state = None  # flat torch tensor of channels * (window - 1) elements of the input dtype

    def _row_dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    def _in_dtype(self):
        import torch
        if self.input == "iq":
            return torch.complex128 if self.precision == L.F64 else torch.complex64
        return self._row_dtype()

    # ---- state
    def _ensure_state(self):
        import torch
        if self._state is None:
            self._state = torch.zeros(self.channels * (self.window - 1), dtype=self._in_dtype(), device=f"cuda:{self.device}")
        return self._state

    @property
    def state(self):
        """the whole state buffer (flat), or None before the first call"""
        return self._state

    def history(self):
        """(channels, window - 1) view of the state buffer: the x history, newest first"""
        return self._ensure_state().view(self.channels, self.window - 1)

    def set_history(self, h):
        """copy h (channels, window - 1), newest first, into the state buffer; a tensor of the input dtype keeps its bits"""
        import torch
        h = torch.as_tensor(h)
        if tuple(h.shape) != (self.channels, self.window - 1):
            raise ValueError("history must be (channels, window - 1)")
        self.history().copy_(h.to(self._in_dtype()))

    def reset(self):
        """zero history, in place: views from history() stay valid and nothing is allocated"""
        if self._state is not None:
            self._state.zero_()

    # ---- plan
    def set_alpha(self, alpha: float):
        """the factor for later calls; the history stays"""
        L.check(self._lib.sdsp_hip_cfar_plan_set_alpha(self._plan, float(alpha)))
        self.alpha = float(alpha)

    def set_variant(self, v: int):
        """0 = the LDS boxcar kernel (CA, GO, SO) or the register-resident sorted-array kernel (OS), 1 = the plain cross-check kernel
        (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_cfar_plan_set_variant(self._plan, v))

    def set_run(self, run: int):
        """outputs per workgroup (CA, GO, SO) or per lane (OS) of variant 0; 0 = chosen per call.  The bits do not depend on it (tests
        and benchmarks only)"""
        if run < 0:
            raise ValueError("run must be >= 0")
        L.check(self._lib.sdsp_hip_cfar_plan_set_run(self._plan, run))

    def info(self) -> dict:
        """the plan's sdsp_hip_cfar_plan_info as a dict"""
        i = L.CfarPlanInfo()
        L.check(self._lib.sdsp_hip_cfar_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def state_bytes(self) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_cfar_state_bytes(self._plan, C.byref(n)))
        return n.value

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per row"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_cfar_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    # ---- stream
    def process(self, x, thr=True, det=True, samples: int | None = None):
        """x: a contiguous device tensor (channels, stride) of the bank's input dtype (the row dtype, or its complex dtype for
        input="iq"); takes [:, :samples] of every row (default: the whole of x's rows), continuing from the bank's history.  thr and
        det: True (a new tensor), False / None (not computed), or a contiguous (channels, >= samples) device tensor to write into (the
        row dtype, uint8).  Returns (thr, det), each (channels, samples) or None."""
        import torch
        dt = self._in_dtype()
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 2 or x.shape[0] != self.channels:
            raise ValueError("process needs a contiguous (channels, samples) device tensor of the bank's input dtype")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        samples = x.shape[1] if samples is None else samples
        if samples < 0 or samples > x.shape[1]:
            raise ValueError("block exceeds the row")

        def out(arg, dtype, name):
            if arg is None or arg is False:
                return None
            if arg is True:
                return torch.empty((self.channels, samples), dtype=dtype, device=x.device)
            if (not isinstance(arg, torch.Tensor) or arg.dtype != dtype or not arg.is_cuda or not arg.is_contiguous() or arg.dim() != 2
                    or arg.device != x.device or arg.shape[0] != self.channels or arg.shape[1] < samples):
                raise ValueError(f"{name} must be a contiguous (channels, >= samples) device tensor of dtype {dtype}")
            return arg

        t, d = out(thr, self._row_dtype(), "thr"), out(det, torch.uint8, "det")
        if t is None and d is None:
            raise ValueError("thr and det cannot both be left out")
        st = self._ensure_state()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_cfar_process(self._plan, x.data_ptr(), x.shape[1], t.data_ptr() if t is not None else None,
                                                t.shape[1] if t is not None else 0, d.data_ptr() if d is not None else None,
                                                d.shape[1] if d is not None else 0, samples, st.data_ptr(), stream))
        cut = lambda y: y if y is None or y.shape[1] == samples else y[:, :samples]  # noqa: E731
        return cut(t), cut(d)

    def __del__(self):
        try:
            if self._plan:
                self._lib.sdsp_hip_cfar_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass


def cfar(x, train: int, guard: int, mode="ca", alpha: float | None = None, pfa: float | None = None, rank: int | None = None):
    """CFAR over finite rows such as range profiles: x is a device tensor (channels, samples) or (samples,), float32 / float64 power or
    complex64 / complex128 I/Q.  Returns (thr, det) of x's shape where output n belongs to cell n: every row goes through a fresh
    cfar_bank followed by train + guard zeros, and the first train + guard outputs are dropped.  The first and last train + guard cells
    of a row have no full set of training cells inside it and are marked untested: thr = +inf, det = 0."""
    import torch
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or x.dtype not in (torch.float32, torch.float64, torch.complex64,
                                                                                  torch.complex128):
        raise ValueError("cfar needs a float32, float64, complex64 or complex128 tensor of one or two dimensions")
    if not x.is_cuda:
        raise ValueError("cfar needs a device tensor")
    precision = L.F64 if x.dtype in (torch.float64, torch.complex128) else L.F32
    rows = x.reshape(1, -1) if x.dim() == 1 else x
    half = train + guard
    C_, S = rows.shape
    real = torch.float64 if precision == L.F64 else torch.float32
    if C_ == 0 or S == 0:
        return torch.empty(x.shape, dtype=real, device=x.device), torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    bank = cfar_bank(C_, train, guard, mode, alpha, pfa, rank, "iq" if x.is_complex() else "power", precision, x.device.index)
    padded = torch.cat([rows, rows.new_zeros((C_, half))], dim=1).contiguous()
    t, d = bank.process(padded)
    t, d = t[:, half:].contiguous(), d[:, half:].contiguous()
    edge = min(half, S)
    t[:, :edge] = float("inf")
    t[:, S - edge:] = float("inf")
    d[:, :edge] = 0
    d[:, S - edge:] = 0
    return t.reshape(x.shape), d.reshape(x.shape)
