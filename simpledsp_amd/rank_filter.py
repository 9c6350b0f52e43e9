"""Host mirror of the rank-order filter bank (include/sdsp_hip.h: sdsp_hip_rank_*).

`channels` independent real rows: process(x) returns, for every sample, the element of rank r of the last `window` samples of its row
(r = 0 the running minimum, window - 1 the running maximum, (window - 1) / 2 the running median), continuing from the bank's history.
The order is IEEE 754 totalOrder and every output is one of the inputs, bit for bit.  Same conventions as the other banks
(channel-major rows, per-channel device state carried across calls).  The state is one device buffer: the x history
(channels, window - 1), newest first.  medfilt() is scipy.signal.medfilt for the rows of a device tensor."""
from __future__ import annotations

import ctypes as C

from . import _lib as L


def rank_index(window: int, rank) -> int:
    """the rank as an index 0 .. window - 1: an int, or "min", "max", "median" (odd windows only)"""
    if isinstance(window, bool) or not isinstance(window, int) or window <= 0:
        raise ValueError("window must be a positive int")
    if rank == "min":
        return 0
    if rank == "max":
        return window - 1
    if rank == "median":
        if window % 2 == 0:
            raise ValueError('rank="median" needs an odd window')
        return (window - 1) // 2
    if isinstance(rank, bool) or not isinstance(rank, int):
        raise ValueError('rank must be an int or one of "median", "min", "max"')
    if not 0 <= rank < window:
        raise ValueError("rank must be in [0, window)")
    return rank


def check_window(window: int, precision: int) -> None:
    limit = L.RANK_MAX_WINDOW_F64 if precision == L.F64 else L.RANK_MAX_WINDOW
    if precision not in (L.F32, L.F64):
        raise ValueError("precision must be F32 or F64")
    if window > limit:
        raise ValueError(f"window must be at most {limit} for this precision")


class rank_filter_bank:
    """A running rank-order filter (median, minimum, maximum or any rank) over the last `window` samples of every row."""

    def __init__(self, channels: int, window: int, rank="median", precision: int = L.F32, device: int = 0):
        self.rank = rank_index(window, rank)
        check_window(window, precision)
        if channels <= 0:
            raise ValueError("channels must be positive")
        self._plan = None
        self._lib = L.load()
        self.channels, self.window, self.precision, self.device = channels, window, precision, device
        h = C.c_void_p()
        L.check(self._lib.sdsp_hip_rank_plan_create(C.byref(h), channels, window, self.rank, precision, device))
        self._plan = h
        self._state = None  # flat torch tensor of channels * (window - 1) elements of the row dtype

    def _row_dtype(self):
        import torch
        return torch.float64 if self.precision == L.F64 else torch.float32

    # ---- state
    def _ensure_state(self):
        import torch
        if self._state is None:
            self._state = torch.zeros(self.channels * (self.window - 1), dtype=self._row_dtype(), device=f"cuda:{self.device}")
        return self._state

    @property
    def state(self):
        """the whole state buffer (flat), or None before the first call"""
        return self._state

    def history(self):
        """(channels, window - 1) view of the state buffer: the x history, newest first"""
        return self._ensure_state().view(self.channels, self.window - 1)

    def set_history(self, h):
        """copy h (channels, window - 1), newest first, into the state buffer; a tensor of the row dtype keeps its bits"""
        import torch
        h = torch.as_tensor(h)
        if tuple(h.shape) != (self.channels, self.window - 1):
            raise ValueError("history must be (channels, window - 1)")
        self.history().copy_(h.to(self._row_dtype()))

    def reset(self):
        """zero history, in place: views from history() stay valid and nothing is allocated"""
        if self._state is not None:
            self._state.zero_()

    # ---- plan
    def set_variant(self, v: int):
        """0 = the register-resident kernel, 1 = the plain cross-check kernel (same bits)"""
        if v not in (0, 1):
            raise ValueError("variant must be 0 or 1")
        L.check(self._lib.sdsp_hip_rank_plan_set_variant(self._plan, v))

    def set_run(self, run: int):
        """outputs per lane of variant 0; 0 = chosen per call.  The bits do not depend on it (tests and benchmarks only)"""
        if run < 0:
            raise ValueError("run must be >= 0")
        L.check(self._lib.sdsp_hip_rank_plan_set_run(self._plan, run))

    def info(self) -> dict:
        """the plan's sdsp_hip_rank_plan_info as a dict"""
        i = L.RankPlanInfo()
        L.check(self._lib.sdsp_hip_rank_plan_get_info(self._plan, C.byref(i)))
        d = {name: getattr(i, name) for name, _ in i._fields_}
        d["kernel"] = i.kernel.decode()
        return d

    def state_bytes(self) -> int:
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_rank_state_bytes(self._plan, C.byref(n)))
        return n.value

    def launches(self, samples: int) -> int:
        """kernel launches of one process call of `samples` per row"""
        n = C.c_uint64(0)
        L.check(self._lib.sdsp_hip_rank_plan_launches(self._plan, samples, C.byref(n)))
        return n.value

    # ---- stream
    def process(self, x, y=None, samples: int | None = None):
        """x: a contiguous device tensor (channels, stride) of the bank's row dtype; filters [:, :samples] of every row (default: the
        whole of x's rows), continuing from the bank's history.  Returns y (channels, samples); y, when given, is a contiguous
        (channels, >= samples) tensor to write into."""
        import torch
        dt = self._row_dtype()
        if x.dtype != dt or not x.is_cuda or not x.is_contiguous() or x.dim() != 2 or x.shape[0] != self.channels:
            raise ValueError("process needs a contiguous (channels, samples) device tensor of the bank's row dtype")
        if x.device.index != self.device:
            raise ValueError("tensor lives on a different device than the bank")
        samples = x.shape[1] if samples is None else samples
        if samples < 0 or samples > x.shape[1]:
            raise ValueError("block exceeds the row")
        if y is None:
            y = torch.empty((self.channels, samples), dtype=dt, device=x.device)
        elif (y.dtype != dt or not y.is_cuda or not y.is_contiguous() or y.dim() != 2 or y.device != x.device
              or y.shape[0] != self.channels or y.shape[1] < samples):
            raise ValueError("y must be a contiguous (channels, >= samples) device tensor of the bank's row dtype")
        st = self._ensure_state()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(self._lib.sdsp_hip_rank_process(self._plan, x.data_ptr(), x.shape[1], y.data_ptr(), y.shape[1], samples, st.data_ptr(),
                                                stream))
        return y if y.shape[1] == samples else y[:, :samples]

    def __del__(self):
        try:
            if self._plan:
                self._lib.sdsp_hip_rank_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass


def medfilt(x, kernel_size: int = 3):
    """scipy.signal.medfilt for the rows of a device tensor x (channels, samples) or (samples,), float32 or float64: the centred median
    of kernel_size (odd) samples with zeros past both ends, equal to scipy's in value.  Every row is followed by (kernel_size - 1) / 2
    zeros and goes through a fresh rank_filter_bank with zero history, whose first (kernel_size - 1) / 2 outputs are dropped."""
    import torch
    if isinstance(kernel_size, bool) or not isinstance(kernel_size, int) or kernel_size <= 0 or kernel_size % 2 == 0:
        raise ValueError("kernel_size must be a positive odd int")
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("medfilt needs a float32 or float64 tensor of one or two dimensions")
    precision = L.F64 if x.dtype == torch.float64 else L.F32
    check_window(kernel_size, precision)
    if not x.is_cuda:
        raise ValueError("medfilt needs a device tensor")
    rows = x.reshape(1, -1) if x.dim() == 1 else x
    half = (kernel_size - 1) // 2
    if rows.shape[0] == 0 or rows.shape[1] == 0:
        return x.clone()
    padded = torch.nn.functional.pad(rows, (0, half)).contiguous()
    bank = rank_filter_bank(rows.shape[0], kernel_size, "median", precision, x.device.index)
    y = bank.process(padded)[:, half:].contiguous()
    return y.reshape(x.shape)
