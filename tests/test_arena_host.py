"""The framed-buffer checks of tests/arena.py fail when they should -- shown on CPU tensors, with planted defects.

The "kernels" here are numpy functions working in place on the view they are given (and, where the defect is an out-of-range
access, on the arena memory around it).  The operation is y = 2 x per row.  A clean function passes every check; each planted
defect -- a one-element write just before / just after the interior, a write into row padding, a read one element past the
interior, a 1e-9 leak from the neighbouring row -- is reported.  The last two are far below any rounding tolerance on Gaussian
data: they are caught because the checks compare bits under two fills and track NaNs, which is what tests/test_gpu_isolation.py
relies on for the HIP kernels.

The second half does the same for the streaming-bank harness (arena.Buffers, check_framed_bank, check_poisoned_bank) that
tests/test_gpu_stream_isolation.py runs the HIP banks through: numpy stand-ins of an STFT and an inverse STFT bank pass it, and
each of seven planted defects is reported by the assertion meant for it.

The third part does it for the wide-row harness (arena.WideRows, run_placed, check_wide) of tests/test_gpu_wide_strides.py, at a wrap of
2^16 in place of 2^32: a stand-in that narrows the row offset of `in` or of `out` to 16 bits -- in elements or in bytes -- fails the
bit comparison, the narrowed write leaves row 1 at its fill, and a refusal that changed a buffer is reported."""
import numpy as np
import pytest
import torch

import arena

ROWS, COLS, MARGIN = 6, 40, 64


def _around(view, before=1, after=1):
    """numpy array over the view's elements plus `before` / `after` elements of the arena around it (shared memory)"""
    flat = torch.as_strided(view, (before + view.numel() + after,), (1,), view.storage_offset() - before)
    return flat.numpy()


def clean(view):
    v = view.numpy()
    v *= 2


def writes_before(view):
    clean(view)
    _around(view)[0] = 1.0


def writes_after(view):
    clean(view)
    _around(view)[-1] = 1.0


def reads_past_the_end(view):
    a = _around(view)
    past = a[-1].copy()
    clean(view)
    a[-2] += 1e-9 * past  # the last output picks up what lies behind the buffer


def leaks_from_the_next_row(view):
    v = view.numpy()
    x = v.copy()
    v *= 2
    v[:-1] += 1e-9 * x[1:]


def _input(dtype=torch.float64):
    g = torch.Generator().manual_seed(3)
    x = torch.randn((ROWS, COLS), generator=g, dtype=torch.float64)
    return x.to(dtype) if not dtype.is_complex else torch.complex(x, x.flip(0)).to(dtype)


def _clean_of(x, fn=clean):
    y = x.clone()
    fn(y)
    return y


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.complex64, torch.complex128])
def test_clean_function_passes(dtype):
    x = _input(dtype)
    arena.check_framed(torch, x, _clean_of(x), clean, (0, 1, 2), MARGIN, device="cpu")
    arena.check_framed(torch, x, _clean_of(x), lambda v: clean(v[:, 3:3 + COLS]), (0, 1), MARGIN, row_stride=COLS + 5,
                       col_offset=3, device="cpu")


@pytest.mark.parametrize("fn,where", [(writes_before, "-1 from the interior's start"), (writes_after, "+1 from its end")])
def test_one_element_write_outside_is_reported(fn, where):
    x = _input()
    with pytest.raises(AssertionError, match="outside the interior") as e:
        arena.check_framed(torch, x, _clean_of(x), fn, (0,), MARGIN, device="cpu")
    assert where in str(e.value)


def test_write_into_row_padding_is_reported():
    x = _input()

    def pads(view):  # filters columns 3 .. 3 + COLS of every row, and one padding column of row 2
        clean(view[:, 3:3 + COLS])
        view[2, 3 + COLS] = 0.5
    with pytest.raises(AssertionError, match="outside the interior"):
        arena.check_framed(torch, x, _clean_of(x), pads, (0,), MARGIN, row_stride=COLS + 5, col_offset=3, device="cpu")

    def pads_in_front(view):
        clean(view[:, 3:3 + COLS])
        view[0, 2] = 0.5
    with pytest.raises(AssertionError, match="outside the interior"):
        arena.check_framed(torch, x, _clean_of(x), pads_in_front, (0,), MARGIN, row_stride=COLS + 5, col_offset=3, device="cpu")


def test_read_past_the_interior_is_reported():
    x = _input()
    want = _clean_of(x)
    with pytest.raises(AssertionError, match="differs from the clean result"):
        arena.check_framed(torch, x, want, reads_past_the_end, (0,), MARGIN, device="cpu")
    # the defect is invisible to a rounding tolerance under the finite fill: 7e-9 on values of order one
    a, view = arena.framed(torch, tuple(x.shape), x.dtype, 0, MARGIN, 7.0, device="cpu")
    view.copy_(x)
    reads_past_the_end(view)
    assert not arena.same_bits(view, want) and float((view - want).abs().max()) < 1e-8


def test_leak_from_the_neighbouring_row_is_reported():
    x = _input()
    want = _clean_of(x)
    poisoned = [0, 3, ROWS - 1]
    xp = x.clone()
    masks = {}
    for i, r in enumerate(poisoned):  # y = 2 x is elementwise: the NaN stays where it was put
        col = (0, COLS // 2, COLS - 1)[i]
        xp[r, col] = float("nan")
        masks[r] = torch.zeros(COLS, dtype=torch.bool)
        masks[r][col] = True
    good = _clean_of(xp)
    arena.assert_rows_isolated(good, want, poisoned, nan_from=masks)
    bad = _clean_of(xp, leaks_from_the_next_row)
    with pytest.raises(AssertionError, match="clean rows"):
        arena.assert_rows_isolated(bad, want, poisoned, nan_from=masks)
    # without a NaN the leak is 1e-9 of a neighbour: no tolerance test sees it
    assert float((_clean_of(x, leaks_from_the_next_row) - want).abs().max()) < 1e-8


def test_nan_masks_of_poisoned_rows():
    x = _input()
    want = torch.cumsum(x, dim=1)  # a causal operation: a NaN at column s reaches columns s .. end
    xp = x.clone()
    xp[2, 7] = float("nan")
    got = torch.cumsum(xp, dim=1)
    mask = torch.zeros(COLS, dtype=torch.bool)
    mask[7:] = True
    arena.assert_rows_isolated(got, want, [2], nan_from={2: mask})
    early = mask.clone()
    early[6] = True
    with pytest.raises(AssertionError, match="NaN mask differs"):
        arena.assert_rows_isolated(got, want, [2], nan_from={2: early})
    with pytest.raises(AssertionError, match="are not NaN"):
        arena.assert_rows_isolated(got, want, [2])
    got[2, 3] += 1e-12  # a poisoned row must keep the clean bits before its NaN
    with pytest.raises(AssertionError, match="outside the NaN mask"):
        arena.assert_rows_isolated(got, want, [2], nan_from={2: mask})


# ------------------------------------------------------------------ the streaming-bank harness (tests/test_gpu_stream_isolation.py)
#
# The stand-in "banks" are the numpy references of the STFT and inverse STFT contracts behind the bank protocol of
# arena.check_framed_bank, working in slices of UNITS (channel, frame) units like the HIP banks.  `fault` plants one defect.

N_FFT, HOP, CH, FRAMES, UNITS = 16, 4, 3, 7, 5  # hist = 12; slices [0,5) [5,10) [10,15) [15,20) [20,21) of 21 units
BINS, HIST = N_FFT // 2 + 1, N_FFT - HOP
WINDOW = 0.5 + 0.25 * np.cos(np.arange(N_FFT))  # no zeros: a NaN sample reaches every bin of its frames


class StftStandIn:
    ticks = FRAMES

    def __init__(self, fault=None):
        from stft_ref import stft_ref
        self.ref, self.fault = stft_ref, fault
        rng = np.random.default_rng(11)
        self.x = torch.from_numpy(rng.standard_normal((CH, FRAMES * HOP)))
        self.hist = torch.from_numpy(rng.standard_normal((CH, HIST)))

    def specs(self, null_state=False):
        s = {"in": dict(shape=(CH, FRAMES * HOP), dtype=torch.float64, init=self.x, read_only=True),
             "out": dict(shape=(CH, FRAMES * BINS), dtype=torch.complex128, init=None)}
        if not null_state:
            s["state"] = dict(shape=(CH, HIST), dtype=torch.float64, init=self.hist, strided=False)
        return s

    def run(self, b, t0, t1):
        F, S = t1 - t0, (t1 - t0) * HOP
        x = b.t["in"][:, t0 * HOP:t1 * HOP].numpy().copy()
        if self.fault == "reads_before_in":  # sample 0 of channel 0 picks up 1e-9 of the element in front of the buffer
            x[0, 0] += 1e-9 * _around(b.t["in"])[0]
        hist = b.inner("state").numpy().copy() if b.has("state") else None
        y, state = self.ref(x, N_FFT, HOP, WINDOW, hist)
        for g0, g1 in arena.slice_map(CH * F, UNITS):
            for g in range(g0, g1):
                c, j = divmod(g, F)
                src = c
                if self.fault == "frame_from_the_previous_channel" and j == 0 and g > g0:  # a channel that starts inside a slice
                    src = c - 1
                b.t["out"][c, (t0 + j) * BINS:(t0 + j + 1) * BINS] = torch.from_numpy(y[src, j])
        if self.fault == "writes_past_last_row":
            _around(b.t["out"])[-1] = 1.0
        if self.fault == "writes_before_first_row":
            _around(b.t["out"])[0] = 1.0
        if self.fault == "writes_row_padding" and b.stride("out") > FRAMES * BINS:
            b.t["out"][1, FRAMES * BINS] = 1.0
        if self.fault == "writes_in":
            b.t["in"][1, 2] = 0.0
        if b.has("state"):
            if self.fault == "state_shifted_by_one" and S < HIST:  # the in-place shift of a short block
                state = np.roll(state, 1, axis=1)
            b.inner("state").copy_(torch.from_numpy(state))

    def masks(self, row, col):
        out = torch.zeros((CH, FRAMES, BINS), dtype=torch.bool)
        p = col + HIST
        for j in range(FRAMES):
            out[row, j] = j * HOP <= p < j * HOP + N_FFT
        state = torch.zeros((CH, HIST), dtype=torch.bool)
        if FRAMES * HOP - 1 - col < HIST:
            state[row, FRAMES * HOP - 1 - col] = True
        return {"out": out.reshape(CH, -1), "state": state}


class IstftStandIn:
    ticks = FRAMES

    def __init__(self, fault=None):
        from istft_ref import istft_ref
        self.ref, self.fault = istft_ref, fault
        rng = np.random.default_rng(12)
        X = rng.standard_normal((CH, FRAMES, BINS)) + 1j * rng.standard_normal((CH, FRAMES, BINS))
        self.X = torch.from_numpy(X.reshape(CH, -1))
        self.pending = torch.from_numpy(rng.standard_normal((CH, HIST)))

    def specs(self, null_state=False):
        s = {"in": dict(shape=(CH, FRAMES * BINS), dtype=torch.complex128, init=self.X, read_only=True),
             "out": dict(shape=(CH, FRAMES * HOP), dtype=torch.float64, init=None)}
        if not null_state:
            s["state"] = dict(shape=(CH, HIST), dtype=torch.float64, init=self.pending, strided=False)
        return s

    def run(self, b, t0, t1):
        X = b.t["in"][:, t0 * BINS:t1 * BINS].numpy().reshape(CH, t1 - t0, BINS)
        y, state = self.ref(X, N_FFT, HOP, WINDOW, b.inner("state").numpy().copy() if b.has("state") else None)
        b.t["out"][:, t0 * HOP:t1 * HOP].copy_(torch.from_numpy(y))
        if self.fault == "writes_before_first_row":
            _around(b.t["out"])[0] = 1.0
        if b.has("state"):
            b.inner("state").copy_(torch.from_numpy(state))

    def masks(self, row, col):
        j = col // BINS
        t = torch.arange(FRAMES * HOP + HIST)
        hit = (t >= j * HOP) & (t < j * HOP + N_FFT)
        out = torch.zeros((CH, FRAMES * HOP), dtype=torch.bool)
        state = torch.zeros((CH, HIST), dtype=torch.bool)
        out[row], state[row] = hit[:FRAMES * HOP], hit[FRAMES * HOP:]
        return {"out": out, "state": state}


ODD = {"in": (1, "odd"), "out": (1, "odd"), "state": (1, "exact")}
LAYOUTS = [{}, ODD, {"in": (2, "vec"), "out": (2, "vec"), "state": (2, "exact")}, {"state": (1, "exact")}]


def _stft_poisons():
    edges = arena.edge_units(CH, FRAMES, UNITS)
    assert [(c, j) for _, c, j in edges] == [(0, 4), (0, 5), (0, 6), (1, 0)]  # slices [0, 5) [5, 10): 5 is inside channel 0, 7 in [5, 10)
    return [(label, c, j * HOP + HOP - 1) for label, c, j in edges] + [("first", 0, 0), ("last", CH - 1, FRAMES * HOP - 1)]


def _drive(bank, clean=None, poison_bank=None):
    """what tests/test_gpu_stream_isolation.py does with a HIP bank: layouts, two calls, state = NULL, poisons"""
    clean = arena.clean_bank(torch, bank, "cpu") if clean is None else clean
    for layout in LAYOUTS:
        arena.check_framed_bank(torch, bank, clean, layout, device="cpu", tag="one call")
    arena.check_framed_bank(torch, bank, arena.clean_bank(torch, bank, "cpu", null_state=True), ODD, device="cpu", null_state=True)
    poisons = _stft_poisons() if isinstance(bank, StftStandIn) else [("a bin of frame 3", 1, 3 * BINS + 2), ("last", CH - 1, FRAMES * BINS - 2)]
    for layout in ({}, ODD):
        arena.check_poisoned_bank(torch, bank, clean, poisons, layout, device="cpu", tag="poison")
    for layout in LAYOUTS:
        arena.check_framed_bank(torch, bank, clean, layout, splits=(2,), device="cpu", tag="two calls")


def test_stream_harness_passes_the_clean_stand_ins():
    for bank in (StftStandIn(), IstftStandIn()):
        _drive(bank)
    # the stand-ins are the references themselves: their clean result is the reference's, to the bit
    from stft_ref import stft_ref
    b = StftStandIn()
    want, state = stft_ref(b.x.numpy(), N_FFT, HOP, WINDOW, b.hist.numpy())
    clean = arena.clean_bank(torch, b, "cpu")
    assert np.array_equal(clean["out"].numpy().reshape(want.shape), want) and np.array_equal(clean["state"].numpy(), state)


@pytest.mark.parametrize("fault,match", [
    ("writes_past_last_row", r"buffer 'out': 1 element\(s\) outside the interior.*\+1 from its end"),
    ("writes_before_first_row", r"buffer 'out': 1 element\(s\) outside the interior.*-1 from the interior's start"),
    ("writes_row_padding", r"buffer 'out': 1 element\(s\) outside the interior"),
    ("reads_before_in", r"the interior of 'out' differs from the clean result"),
    ("frame_from_the_previous_channel", r"first frame of channel 1\) buffer 'out': NaN mask differs"),
    ("state_shifted_by_one", r"two calls.*differs from the clean result"),  # the second call reads the shifted history
    ("writes_in", r"read-only buffer 'in' was written"),
])
def test_stream_harness_reports_each_planted_fault(fault, match):
    """the clean result comes from the faulted bank itself where the fault would be in a HIP bank's clean run too (a slice-edge mix-up,
    a wrong in-place shift): only the NaN masks and the two-call comparison can see those"""
    bank = StftStandIn(fault)
    own = fault in ("frame_from_the_previous_channel", "state_shifted_by_one")
    clean = arena.clean_bank(torch, bank if own else StftStandIn(), "cpu")
    with pytest.raises(AssertionError, match=match):
        _drive(bank, clean)
    if fault == "reads_before_in":  # far below any tolerance under the finite fill: it is the bit comparison that sees it
        b = arena.Buffers(torch, bank.specs(), {}, 1, "cpu")
        bank.run(b, 0, FRAMES)
        assert float((b.inner("out") - clean["out"]).abs().max()) < 1e-6 and not arena.same_bits(b.inner("out"), clean["out"])


def test_stream_harness_reports_a_write_in_front_of_an_overlap_add_output():
    with pytest.raises(AssertionError, match=r"buffer 'out': 1 element\(s\) outside the interior.*-1 from the interior's start"):
        _drive(IstftStandIn("writes_before_first_row"), arena.clean_bank(torch, IstftStandIn(), "cpu"))


def test_edge_units_and_strides():
    assert arena.slice_map(21, 5) == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 21)]
    with pytest.raises(AssertionError, match="no slice starts inside a channel"):
        arena.edge_units(3, 7, 7)  # slices of whole channels
    with pytest.raises(AssertionError, match="no slice starts inside a channel"):
        arena.edge_units(3, 7, 1000)  # one slice
    assert [arena.stride_for(10, 4, k) for k in arena.STRIDES] == [10, 11, 12]
    assert [arena.stride_for(11, 4, k) for k in arena.STRIDES] == [11, 13, 12]
    assert [arena.stride_for(8, 16, k) for k in arena.STRIDES] == [8, 9, 9]
    assert arena.stride_for(12, 8, "vec") == 14


def test_bits_are_exact_and_nan_safe():
    a = torch.tensor([float("nan"), 0.0, -0.0, 1.0])
    assert arena.same_bits(a, a.clone())
    assert not arena.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert arena.bits(torch.zeros(3, dtype=torch.complex64)).shape == (3, 2)
    assert arena.bits(torch.zeros(3, dtype=torch.complex128)).dtype == torch.int64


# ------------------------------------------------------------------ one buffer with its rows more than `wrap` bytes apart

WRAP = 1 << 16  # the stand-ins' "2^32": tests/test_gpu_wide_strides.py runs the same functions with the real one
WIDE_COLS = 200


class WideStandIn:
    """out[c] = 2 in[c] + history[c] for two rows, with the row offsets formed the way a kernel forms them: c * stride in elements,
    or that times the element size in bytes.  `fault` = (buffer, unit) truncates that buffer's offset in that unit to 16 bits;
    refuse = (status, writes) returns the status without computing, after writing one element of out when `writes`."""

    def __init__(self, dtype, fault=None, refuse=None):
        self.dtype, self.fault, self.refuse = dtype, fault, refuse
        g = torch.Generator().manual_seed(11)
        self.x = torch.randn((2, WIDE_COLS), generator=g, dtype=torch.float64).to(dtype)
        self.h = torch.randn((2, 1), generator=g, dtype=torch.float64).to(dtype)

    def specs(self):
        return {"in": dict(shape=(2, WIDE_COLS), dtype=self.dtype, init=self.x, read_only=True),
                "out": dict(shape=(2, WIDE_COLS), dtype=self.dtype, init=None),
                "state": dict(shape=(2, 1), dtype=self.dtype, init=self.h)}

    def offset(self, name, p, c):
        off = c * p.stride
        if self.fault == (name, "elements"):
            off %= WRAP
        es = p.base.element_size()
        if self.fault == (name, "bytes"):
            off = (off * es % WRAP) // es
        return p.offset + off

    def call(self, p):
        if self.refuse:
            if self.refuse[1]:
                p["out"].base[p["out"].offset] = 0
            return self.refuse[0]
        for c in range(2):
            i, o = self.offset("in", p["in"], c), self.offset("out", p["out"], c)
            x = p["in"].base[i:i + WIDE_COLS].clone()
            p["out"].base[o:o + WIDE_COLS] = 2 * x + p["state"].row(c)
            p["state"].row(c).copy_(x[-1:])
        return 0


def _wide_flat():
    return torch.empty(arena.wide_distance(4, WRAP) + (1 << 14), dtype=torch.uint8)


def _wide_drive(bank, wide, flat=None):
    flat = _wide_flat() if flat is None else flat
    ok = WideStandIn(bank.dtype)
    clean = [arena.run_placed(torch, ok.specs(), ok.call, fill, device="cpu")[1] for fill in (0, 1)]
    assert bool(torch.equal(clean[0]["out"], 2 * ok.x + ok.h)) and arena.same_bits(clean[0]["out"], clean[1]["out"])
    return arena.check_wide(torch, bank.specs(), bank.call, clean, wide, flat, WRAP, "cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.complex64, torch.int32])
@pytest.mark.parametrize("wide", ["in", "out"])
def test_wide_rows_correct_stand_in_passes(dtype, wide):
    assert _wide_drive(WideStandIn(dtype), wide) == 0


def test_wide_rows_geometry():
    """4-byte elements pass the wrap in elements and in bytes, 8-byte ones in bytes only; either way the truncated offset is 256 bytes"""
    assert arena.wide_distance(4) == (1 << 34) + 256 and arena.wide_distance(1) == (1 << 32) + 64
    for dtype, elems in ((torch.float32, (1 << 32) + 64), (torch.complex64, (1 << 31) + 32), (torch.complex128, (1 << 30) + 16)):
        es = torch.empty((), dtype=dtype).element_size()
        assert arena.wide_distance(es) // es == elems and arena.wide_distance(es) % (1 << 32) == 256
    w = arena.WideRows(torch, _wide_flat(), torch.float32, WIDE_COLS, 7.0, WRAP)
    assert w.stride == WRAP + 64 and w.stride % WRAP == 64 and w.ptr == w.base.data_ptr() + arena.WIDE_GUARD
    assert arena.WideRows(torch, _wide_flat(), torch.float64, WIDE_COLS, 7.0, WRAP).stride == WRAP // 2 + 32  # below the wrap in elements
    with pytest.raises(AssertionError, match="inside row 0"):
        arena.WideRows(torch, _wide_flat(), torch.float32, 64, 7.0, WRAP)


@pytest.mark.parametrize("dtype,unit", [(torch.float32, "elements"), (torch.float32, "bytes"), (torch.float64, "bytes")])
def test_wide_rows_truncated_read_is_reported(dtype, unit):
    """row 1 of out is then row 0 of in, shifted: finite, plausible values that only the comparison with the compact call sees"""
    with pytest.raises(AssertionError, match="'in' wide, fill 0: 'out' differs from the compact call in 200 element.*row 1, column 0"):
        _wide_drive(WideStandIn(dtype, ("in", unit)), "in")
    assert _wide_drive(WideStandIn(dtype, ("in", unit)), "out") == 0  # the fault needs the buffer it sits in to be the wide one


@pytest.mark.parametrize("dtype,unit", [(torch.float32, "elements"), (torch.float32, "bytes"), (torch.float64, "bytes")])
def test_wide_rows_truncated_write_is_reported_and_leaves_row_1_at_its_fill(dtype, unit):
    flat = _wide_flat()
    with pytest.raises(AssertionError, match="'out' wide, fill 0: 'out' differs from the compact call.*row 0"):
        _wide_drive(WideStandIn(dtype, ("out", unit)), "out", flat)
    es = torch.empty((), dtype=dtype).element_size()
    row1 = flat[arena.wide_distance(es, WRAP) + arena.WIDE_GUARD:][:WIDE_COLS * es].view(dtype)
    assert bool(torch.isnan(row1).all())  # fill 0: nothing was ever written there
    row0 = flat[arena.WIDE_GUARD:][:WIDE_COLS * es].view(dtype)
    assert not bool(torch.isnan(row0[256 // es:]).any())  # row 1's result landed 256 bytes into row 0


def test_wide_rows_element_truncation_is_invisible_to_eight_byte_types():
    """what the device module's docstring says: the stride of an 8-byte type stays below the wrap in elements"""
    assert _wide_drive(WideStandIn(torch.float64, ("in", "elements")), "in") == 0


def test_wide_rows_write_into_a_guard_band_is_reported():
    class Past(WideStandIn):
        def call(self, p):
            WideStandIn.call(self, p)
            o = p["out"]
            o.base[o.offset + o.stride + WIDE_COLS] = 1.0  # one element past wide row 1
            return 0
    with pytest.raises(AssertionError, match="guard band after wide row 1 was written, first at byte 2 of the band"):  # 1.0f and the NaN fill share their low bytes
        _wide_drive(Past(torch.float32), "out")


def test_wide_rows_refusal_must_change_nothing():
    assert _wide_drive(WideStandIn(torch.float32, refuse=(22, False)), "in") == 22
    with pytest.raises(AssertionError, match="refused with 22, but 'out' changed"):
        _wide_drive(WideStandIn(torch.float32, refuse=(22, True)), "in")
    with pytest.raises(AssertionError, match="'out' wide, fill 0.*refused with 22, but 'out' changed"):
        _wide_drive(WideStandIn(torch.float32, refuse=(22, True)), "out")
