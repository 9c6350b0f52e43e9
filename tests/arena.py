"""Framed device buffers for tests that must fail on an out-of-range or cross-channel access by construction.

A kernel under test gets a view INTO one larger tensor (the arena) instead of a tensor of its own: whatever it writes outside
the view lands in the arena and is seen (`assert_frame_untouched`), on both sides and in row padding.  Whatever it reads
outside the view is the arena's fill; every case runs under two fills (all-NaN and a finite pattern) and the interior must
come out with the same bits under both, so a read from outside that reaches an output fails whatever it read.  NaN poisoning
(`assert_rows_isolated`) shows that rows which share a workgroup, a wave or a ring slot do not leak into each other: a NaN is
not hidden by any tolerance.  All comparisons are on bit patterns (`bits`), so they are exact and NaN-safe.

tests/test_arena_host.py shows on CPU tensors that each check fails when it should; tests/test_gpu_isolation.py uses them.
A plain module, not a conftest: it changes nothing about how the suite runs.

The second half (`Buffers` and the `check_*_bank` functions) frames EVERY buffer of a streaming bank's call at once -- in, out, state,
accumulators -- and drives a "bank": any object with the few members listed at `check_framed_bank`.  The HIP banks of
tests/test_gpu_stream_isolation.py and the numpy stand-ins of tests/test_arena_host.py (with planted defects) go through the same
functions, on "cuda" and on "cpu".

The third part (`WideRows`, `run_placed`, `check_wide`) puts ONE buffer of a call at a row distance past `wrap` bytes (2^32 on the
device, 2^16 for the stand-ins of tests/test_arena_host.py), so that an offset truncated to log2(wrap) bits lands in row 0's data.
"""
import math

NAN = float("nan")


def fills(dtype):
    """the two fills every framed case runs under: all-NaN and a finite pattern (7 + 3j / 7.0); integer types have no NaN and take
    0x55 in its place"""
    if dtype.is_complex:
        return (complex(NAN, NAN), complex(7.0, 3.0))
    if not dtype.is_floating_point:
        return (0x55, 7)
    return (NAN, 7.0)


def bits(t):
    """t reinterpreted as int32 / int64 (complex: a trailing axis of two): equality on it is exact and NaN-safe"""
    import torch
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def framed(torch, shape, dtype, lead_elems, margin_elems, fill, row_stride=None, device="cuda"):
    """ONE tensor of margin + lead + interior + margin elements, all of it `fill`; returns (arena, view).  `view` is the
    contiguous view of `shape` that starts margin + lead elements in.  With `row_stride` (2-D shapes) the view is
    (rows, row_stride): rows of shape[1] samples then have row_stride - shape[1] padding columns, which belong to the frame
    (see `interior_mask`).  The arena's base is 512-byte aligned, so lead_elems = 1 gives an element-aligned-only pointer."""
    if row_stride is not None:
        assert len(shape) == 2 and row_stride >= shape[1]
        shape = (shape[0], row_stride)
    inner = math.prod(shape)
    arena = torch.full((2 * margin_elems + lead_elems + inner,), fill, dtype=dtype, device=device)
    if arena.is_cuda:  # host arenas (tests/test_arena_host.py) only exercise the bookkeeping
        assert arena.data_ptr() % 512 == 0, "the arena's base must be 512-byte aligned for `lead_elems` to mean what it says"
    start = margin_elems + lead_elems
    view = arena[start:start + inner].view(shape)
    assert view.is_contiguous() and view.data_ptr() == arena.data_ptr() + start * arena.element_size()
    return arena, view


def interior_mask(torch, arena, view, samples=None, col_offset=0):
    """flat boolean mask over the arena: True where the kernel may write -- the whole view, or columns
    col_offset .. col_offset + samples of every row of a (rows, row_stride) view"""
    mask = torch.zeros(arena.numel(), dtype=torch.bool, device=arena.device)
    start = (view.data_ptr() - arena.data_ptr()) // arena.element_size()
    inner = mask[start:start + view.numel()].view(view.shape)
    if samples is None:
        inner[...] = True
    else:
        assert view.dim() == 2 and col_offset + samples <= view.shape[1]
        inner[:, col_offset:col_offset + samples] = True
    return mask


def assert_frame_untouched(arena_before_bits, arena_after, interior):
    """every element outside the interior (a slice of the flat arena, or a flat boolean mask) still has its original bits"""
    import torch
    after = bits(arena_after)
    assert after.shape == arena_before_bits.shape
    if isinstance(interior, slice):
        mask = torch.zeros(arena_after.numel(), dtype=torch.bool, device=arena_after.device)
        mask[interior] = True
        interior = mask
    changed = after != arena_before_bits
    if changed.dim() == 2:  # complex: either half
        changed = changed.any(dim=1)
    changed &= ~interior
    if bool(changed.any()):
        where = torch.nonzero(changed).flatten()
        inside = torch.nonzero(interior).flatten()
        first, last = int(inside[0]), int(inside[-1])
        raise AssertionError(f"{where.numel()} element(s) outside the interior [{first}, {last}] were written, the first at flat "
                             f"index {int(where[0])} ({int(where[0]) - first:+d} from the interior's start, "
                             f"{int(where[0]) - last:+d} from its end)")


def check_framed(torch, x, clean, run, leads, margin_elems, row_stride=None, col_offset=0, device="cuda", what=""):
    """x: the input, shaped like the interior; clean: the result of the same operation in an ordinary, exactly-sized tensor.
    For every lead and both fills: put x into a framed buffer, call run(view) (in place; for row_stride views run filters
    columns col_offset .. col_offset + x.shape[1]), then the interior must have clean's bits and the frame must be untouched."""
    for lead in leads:
        for fill in fills(x.dtype):
            arena, view = framed(torch, tuple(x.shape), x.dtype, lead, margin_elems, fill, row_stride, device)
            samples = x.shape[1] if row_stride is not None else None
            target = view if row_stride is None else view[:, col_offset:col_offset + samples]
            target.copy_(x)
            before = bits(arena).clone()
            run(view)
            if arena.is_cuda:
                torch.cuda.synchronize()
            tag = (what, "lead", lead, "fill", fill)
            assert_frame_untouched(before, arena, interior_mask(torch, arena, view, samples, col_offset))
            assert same_bits(target, clean), (tag, "the interior differs from the clean result",
                                              int((bits(target) != bits(clean)).sum()))


def assert_rows_isolated(out, clean, poisoned, nan_from=None):
    """out, clean: (rows, ...) results of the poisoned and of the clean input.  Every row outside `poisoned` has clean's bits.
    A poisoned row is NaN in every element (complex: in both halves); with nan_from = {row: mask}, a boolean mask per poisoned
    row, it is NaN exactly where the mask says and has clean's bits everywhere else."""
    import torch
    assert out.shape == clean.shape
    rows = out.shape[0]
    poisoned = sorted(set(poisoned))
    keep = torch.ones(rows, dtype=torch.bool, device=out.device)
    keep[poisoned] = False
    diff = (bits(out[keep]) != bits(clean[keep]))
    if bool(diff.any()):
        bad = torch.nonzero(diff.reshape(diff.shape[0], -1).any(dim=1)).flatten()
        idx = torch.nonzero(keep).flatten()[bad]
        raise AssertionError(f"clean rows {idx[:8].tolist()} (of {bad.numel()}) changed when rows {poisoned} were poisoned")
    for r in poisoned:
        row = torch.view_as_real(out[r]) if out.is_complex() else out[r]
        isnan = torch.isnan(row)
        if nan_from is None:
            if not bool(isnan.all()):
                raise AssertionError(f"poisoned row {r}: {int((~isnan).sum())} of {isnan.numel()} values are not NaN")
        else:
            want = nan_from[r].to(isnan.device)
            if not bool(torch.equal(isnan, want)):
                miss = torch.nonzero(isnan != want).flatten()
                raise AssertionError(f"poisoned row {r}: NaN mask differs from the expected one at {miss[:8].tolist()} "
                                     f"({miss.numel()} places)")
            if not bool(torch.equal(bits(out[r])[~want], bits(clean[r])[~want])):
                raise AssertionError(f"poisoned row {r}: values outside the NaN mask differ from the clean result")


# ------------------------------------------------------------------ every buffer of a streaming bank's call, framed at once

STRIDES = ("exact", "odd", "vec")


def stride_for(cols, element_size, kind):
    """row stride in elements: "exact" = cols; "odd" = the next odd number above cols (rows alternate between 16-byte aligned and
    not); "vec" = the next multiple of 16 bytes above cols (every row keeps the alignment of the first)"""
    if kind == "exact":
        return cols
    if kind == "odd":
        return cols + 1 + cols % 2
    assert kind == "vec", kind
    per = max(1, 16 // element_size)
    return (cols // per + 1) * per


def assert_nan_exactly(out, clean, mask, tag=""):
    """out is NaN (complex: in either half) exactly where the boolean `mask` says and has clean's bits everywhere else"""
    import torch
    assert out.shape == clean.shape == mask.shape, (tag, out.shape, clean.shape, mask.shape)
    isnan = torch.isnan(torch.view_as_real(out)).any(dim=-1) if out.is_complex() else torch.isnan(out)
    mask = mask.to(isnan.device)
    if not bool(torch.equal(isnan, mask)):
        extra, missing = torch.nonzero(isnan & ~mask), torch.nonzero(~isnan & mask)
        raise AssertionError(f"{tag}: NaN mask differs from the expected one: {extra.shape[0]} unexpected NaN(s), the first at "
                             f"{extra[:1].tolist()}; {missing.shape[0]} missing, the first at {missing[:1].tolist()}")
    if not bool(torch.equal(bits(out)[~mask], bits(clean)[~mask])):
        diff = (bits(out) != bits(clean))
        diff = (diff.any(dim=-1) if out.is_complex() else diff) & ~mask
        raise AssertionError(f"{tag}: {int(diff.sum())} value(s) outside the NaN mask differ from the clean result, the first at "
                             f"{torch.nonzero(diff)[:1].tolist()}")


class Buffers:
    """The named 2-D buffers of a bank's call.  specs: {name: dict(shape = (rows, cols), dtype, init = tensor (rows, cols) or None,
    read_only = bool, strided = bool)}.  layout = None: ordinary, exactly-sized tensors (the clean run).  Otherwise every buffer is a
    view into an arena of its own (`framed`), a margin of at least one whole row on each side; layout[name] = (lead elements past the
    arena's 512-byte base, one of STRIDES), (0, "exact") where a name is missing; a buffer with strided = False (a state: its rows
    are contiguous by contract) takes the lead only.  The arenas are `fills(dtype)[fill]` everywhere except where `init` goes."""

    def __init__(self, torch, specs, layout=None, fill=0, device="cuda"):
        self.torch, self.specs, self.device = torch, specs, device
        self.t, self.arena, self.before, self.cols = {}, {}, {}, {}
        for name, s in specs.items():
            rows, cols = s["shape"]
            self.cols[name] = cols
            if layout is None:
                self.t[name] = torch.zeros((rows, cols), dtype=s["dtype"], device=device)
            else:
                lead, kind = layout.get(name, (0, "exact"))
                esize = torch.empty((), dtype=s["dtype"]).element_size()
                stride = stride_for(cols, esize, kind if s.get("strided", True) else "exact")
                margin = -(-max(stride, 1) // 128) * 128  # whole rows, and a multiple of 512 bytes: the lead stays what it says
                self.arena[name], self.t[name] = framed(torch, (rows, cols), s["dtype"], lead, margin, fills(s["dtype"])[fill], stride,
                                                        device)
            if s.get("init") is not None:
                self.inner(name).copy_(s["init"])
            if layout is not None:
                self.before[name] = bits(self.arena[name]).clone()

    def has(self, name):
        return name in self.t

    def inner(self, name):
        """the (rows, cols) part of the buffer that belongs to the call"""
        return self.t[name][:, :self.cols[name]]

    def stride(self, name):
        return self.t[name].shape[1]

    def ptr(self, name, col=0):
        """address of element (0, col); None for a buffer the call does not have (state = NULL)"""
        if name not in self.t:
            return None
        return self.t[name].data_ptr() + col * self.t[name].element_size()

    def sync(self):
        if self.device != "cpu":
            self.torch.cuda.synchronize()

    def writable(self):
        return [n for n, s in self.specs.items() if not s.get("read_only")]

    def check_frames(self, tag=""):
        """a read-only buffer's arena is unchanged everywhere; of the others, everything outside the (rows, cols) interiors is: the
        margins on both sides, the lead and the row padding"""
        torch = self.torch
        self.sync()
        for name, arena in self.arena.items():
            if self.specs[name].get("read_only"):
                changed = bits(arena) != self.before[name]
                if bool(changed.any()):
                    at = int(torch.nonzero(changed.reshape(arena.numel(), -1).any(dim=1))[0])
                    start = (self.t[name].data_ptr() - arena.data_ptr()) // arena.element_size()
                    raise AssertionError(f"{tag}: read-only buffer '{name}' was written, first at flat index {at} ({at - start:+d} "
                                         f"from its first element)")
                continue
            try:
                assert_frame_untouched(self.before[name], arena, interior_mask(torch, arena, self.t[name], self.cols[name]))
            except AssertionError as e:
                raise AssertionError(f"{tag}: buffer '{name}': {e}") from None


def clean_bank(torch, bank, device="cuda", null_state=False):
    """the bank's whole stream in one call on ordinary, exactly-sized tensors: {name: result} of every writable buffer"""
    b = Buffers(torch, bank.specs(null_state), device=device)
    bank.run(b, 0, bank.ticks)
    b.sync()
    return {n: b.inner(n).clone() for n in b.writable()}


def check_framed_bank(torch, bank, clean, layout, splits=(), device="cuda", null_state=False, loose=None, tag=""):
    """A bank is any object with
        ticks                    frames (or samples, where a call may end anywhere) of its whole stream
        specs(null_state)        the Buffers specs of one stream: "in" read-only, every other buffer writable; no "state" when null_state
        run(b, t0, t1)           one call on the Buffers b: ticks [t0, t1) of the stream (b.has("state") says whether it gets a state)
        masks(row, col)          {name: boolean (rows, cols) tensor}: where every writable buffer is NaN after ONE call of the whole
                                 stream with in[row, col] = NaN (check_poisoned_bank)
    Under both fills: frames every buffer by `layout`, feeds the stream as the calls `splits` cuts it into (none: one call) against
    the same buffers, checks after every call that nothing outside the interiors changed (and nothing at all in "in"), and at the end
    that every writable interior has clean's bits -- or passes loose[name](got, want) where the contract promises less than bits."""
    edges = [0, *splits, bank.ticks]
    for fill in (0, 1):
        b = Buffers(torch, bank.specs(null_state), layout, fill, device)
        for t0, t1 in zip(edges, edges[1:]):
            bank.run(b, t0, t1)
            b.check_frames(f"{tag} fill {fill} ticks [{t0}, {t1})")
        for name, want in clean.items():
            got = b.inner(name)
            if loose and name in loose:
                loose[name](got, want)
            elif not same_bits(got, want):
                diff = bits(got) != bits(want)
                raise AssertionError(f"{tag} fill {fill}: the interior of '{name}' differs from the clean result in {int(diff.sum())} "
                                     f"place(s), the first at {torch.nonzero(diff)[:1].tolist()}")


def check_poisoned_bank(torch, bank, clean, poisons, layout, device="cuda", tag=""):
    """poisons: (label, row, col) elements of "in".  One at a time and under both fills: the framed call with that element NaN leaves
    every writable buffer NaN exactly where bank.masks(row, col) says, with clean's bits everywhere else, and the frames untouched."""
    for fill in (0, 1):
        for label, row, col in poisons:
            specs = dict(bank.specs())
            x = specs["in"]["init"].clone()
            x[row, col] = complex(NAN, NAN) if x.is_complex() else NAN
            specs["in"] = dict(specs["in"], init=x)
            b = Buffers(torch, specs, layout, fill, device)
            bank.run(b, 0, bank.ticks)
            where = f"{tag} fill {fill} NaN at in[{row}, {col}] ({label})"
            b.check_frames(where)
            masks = bank.masks(row, col)
            for name, want in clean.items():
                assert_nan_exactly(b.inner(name), want, masks[name], f"{where} buffer '{name}'")


def slice_map(units, per_slice):
    """[g0, g1) of every workspace slice of a call of `units` units"""
    return [(g, min(g + per_slice, units)) for g in range(0, units, per_slice)]


def edge_units(channels, frames, per_slice):
    """(label, channel, frame) of the units next to the edges of a call whose units g = channel frames + frame run in slices of
    `per_slice`: the last frame of a slice and the first of the next INSIDE one channel, and the last frame of a channel and the first
    of the next INSIDE one slice.  Raises where the shape has no such edge: the caller chose the wrong workspace."""
    out = []
    cut = [g for g, _ in slice_map(channels * frames, per_slice)[1:] if g % frames]
    assert cut, ("no slice starts inside a channel", channels, frames, per_slice)
    g = cut[0]
    assert (g - 1) // frames == g // frames
    out += [("last frame of a slice", (g - 1) // frames, (g - 1) % frames), ("first frame of the next slice", g // frames, g % frames)]
    seam = [c * frames for c in range(1, channels) if (c * frames) % per_slice]
    assert seam, ("no channel starts inside a slice", channels, frames, per_slice)
    c = seam[0] // frames
    out += [(f"last frame of channel {c - 1}, in the slice of the next", c - 1, frames - 1), (f"first frame of channel {c}", c, 0)]
    return out


# ------------------------------------------------------------------ one buffer of a call with its two rows more than `wrap` apart

WIDE_GUARD = 4096  # bytes on either side of each wide row that are filled, and must keep their bits


def wide_distance(element_size, wrap=1 << 32):
    """bytes from row 0 to row 1.  4-byte elements and wider: 4 wrap + 256, so that the stride in 4-byte units is wrap + 64 and both the
    element index (4-byte types) and the byte offset (every type) pass `wrap`; narrower elements: wrap + 64.  Truncated to log2(wrap)
    bits the offset is 256 (64) bytes: inside row 0, whose rows are at least 160 elements long."""
    return 4 * wrap + 256 if element_size >= 4 else wrap + 64


def raw(t):
    """t's bytes, flat: equality on them is exact, NaN-safe and works for every dtype"""
    import torch
    return t.contiguous().reshape(-1).view(torch.uint8)


class Placed:
    """Where a (rows, cols) buffer of a call lies: `base` is a flat typed tensor, element (r, c) is base[offset + r stride + c].  A device
    entry gets `ptr` and `stride`; a numpy stand-in indexes `base` itself, with whatever arithmetic it wants to get wrong."""

    def __init__(self, base, offset, stride, rows, cols):
        self.base, self.offset, self.stride, self.rows, self.cols = base, offset, stride, rows, cols

    @property
    def ptr(self):
        return self.base.data_ptr() + self.offset * self.base.element_size()

    def row(self, r):
        return self.base[self.offset + r * self.stride:self.offset + r * self.stride + self.cols]

    def get(self):
        import torch
        return torch.stack([self.row(r) for r in range(self.rows)]).clone()

    def put(self, t):
        for r in range(self.rows):
            self.row(r).copy_(t.reshape(self.rows, self.cols)[r])


class WideRows(Placed):
    """Two rows of `cols` elements of `dtype` inside the flat byte tensor `flat`, `wide_distance` apart, row 0 one guard band in.  The
    rows and WIDE_GUARD bytes on either side of each are `fill`; nothing else of `flat` is touched or looked at."""

    def __init__(self, torch, flat, dtype, cols, fill, wrap=1 << 32):
        assert flat.dtype == torch.uint8 and flat.dim() == 1 and flat.is_contiguous()
        es = torch.empty((), dtype=dtype).element_size()
        self.distance = wide_distance(es, wrap)
        assert self.distance % es == 0 and WIDE_GUARD % es == 0
        assert cols * es > self.distance % wrap, "the truncated offset must fall inside row 0"
        assert cols * es + 2 * WIDE_GUARD < wrap, "a row and its bands stay below the wrap"
        assert 2 * WIDE_GUARD + self.distance + cols * es <= flat.numel(), "the flat buffer is too small"
        Placed.__init__(self, flat.view(dtype), WIDE_GUARD // es, self.distance // es, 2, cols)
        self.windows = [flat[r * self.distance:r * self.distance + 2 * WIDE_GUARD + cols * es] for r in (0, 1)]
        for w in self.windows:
            w.view(dtype).fill_(fill)
        self.before = None

    def mark(self):
        self.before = [w.clone() for w in self.windows]

    def assert_guards(self, tag=""):
        import torch
        for r, (w, b) in enumerate(zip(self.windows, self.before)):
            for side, sl in (("before", slice(0, WIDE_GUARD)), ("after", slice(w.numel() - WIDE_GUARD, w.numel()))):
                if not bool(torch.equal(w[sl], b[sl])):
                    at = int(torch.nonzero(w[sl] != b[sl])[0])
                    raise AssertionError(f"{tag}: the guard band {side} wide row {r} was written, first at byte {at} of the band")

    def unchanged(self):
        import torch
        return all(bool(torch.equal(w, b)) for w, b in zip(self.windows, self.before))


def run_placed(torch, specs, call, fill, wide=None, flat=None, wrap=1 << 32, device="cuda", tag="", guards=None):
    """One call with every buffer placed.  specs: {name: dict(shape = (rows, cols), dtype, init = tensor or None, read_only = bool)};
    every buffer is an ordinary, exactly-sized tensor except `wide`, whose two rows go into `flat` (WideRows).  All of them are
    fills(dtype)[fill] except where `init` goes.  call(placed) -> status, placed = {name: Placed}.
    Status 0: returns (0, {name: contents after the call}), after checking that read-only buffers kept their bits and the wide rows'
    guard bands theirs (with a list for `guards`, the WideRows is appended to it and its bands are left to the caller).  Any other
    status is a refusal: nothing at all may have changed, and (status, None) is returned."""
    placed, before = {}, {}
    for name, s in specs.items():
        rows, cols = s["shape"]
        f = fills(s["dtype"])[fill]
        if name == wide:
            assert rows == 2, (tag, name, "the wide buffer has two rows", rows)
            placed[name] = WideRows(torch, flat, s["dtype"], cols, f, wrap)
        else:
            placed[name] = Placed(torch.full((rows * cols,), f, dtype=s["dtype"], device=device), 0, cols, rows, cols)
        if s.get("init") is not None:
            placed[name].put(s["init"].to(device))
        before[name] = placed[name].get()
    if wide is not None:
        placed[wide].mark()
    status = call(placed)
    if device != "cpu":
        torch.cuda.synchronize()
    after = {name: p.get() for name, p in placed.items()}
    if status != 0:
        for name in specs:
            assert bool(torch.equal(raw(after[name]), raw(before[name]))), (tag, f"refused with {status}, but '{name}' changed")
        assert wide is None or placed[wide].unchanged(), (tag, f"refused with {status}, but the wide rows or their bands changed")
        return status, None
    for name, s in specs.items():
        if s.get("read_only") and not bool(torch.equal(raw(after[name]), raw(before[name]))):
            raise AssertionError(f"{tag}: read-only buffer '{name}' was written")
    if wide is not None and guards is None:
        placed[wide].assert_guards(tag)
    elif wide is not None:
        guards.append(placed[wide])
    return 0, after


def check_wide(torch, specs, call, clean, wide, flat, wrap=1 << 32, device="cuda", tag=""):
    """clean = [results under fill 0, results under fill 1] of run_placed with every buffer compact.  The same call with `wide` in
    `flat` gives, under each fill, clean's bits in every buffer -- or is refused under both, and the status is returned."""
    codes = []
    for fill in (0, 1):
        where = f"{tag} '{wide}' wide, fill {fill}"
        held = []  # the contents first, then the bands: a truncated write shows as what it is
        status, got = run_placed(torch, specs, call, fill, wide, flat, wrap, device, where, held)
        codes.append(status)
        if status != 0:
            continue
        for name, want in clean[fill].items():
            a, b = raw(got[name]), raw(want)
            if a.shape != b.shape or not bool(torch.equal(a, b)):
                es = want.element_size()
                at = torch.nonzero(a != b).flatten() // es
                cols = specs[name]["shape"][1]
                raise AssertionError(f"{where}: '{name}' differs from the compact call in {int(at.unique().numel())} element(s), the first "
                                     f"at row {int(at[0]) // cols}, column {int(at[0]) % cols}")
        held[0].assert_guards(where)
    assert codes[0] == codes[1], (tag, wide, codes)
    return codes[0]
