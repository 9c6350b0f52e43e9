"""Framed device buffers for tests that must fail on an out-of-range or cross-channel access by construction.

A kernel under test gets a view INTO one larger tensor (the arena) instead of a tensor of its own: whatever it writes outside
the view lands in the arena and is seen (`assert_frame_untouched`), on both sides and in row padding.  Whatever it reads
outside the view is the arena's fill; every case runs under two fills (all-NaN and a finite pattern) and the interior must
come out with the same bits under both, so a read from outside that reaches an output fails whatever it read.  NaN poisoning
(`assert_rows_isolated`) shows that rows which share a workgroup, a wave or a ring slot do not leak into each other: a NaN is
not hidden by any tolerance.  All comparisons are on bit patterns (`bits`), so they are exact and NaN-safe.

tests/test_arena_host.py shows on CPU tensors that each check fails when it should; tests/test_gpu_isolation.py uses them.
A plain module, not a conftest: it changes nothing about how the suite runs.
"""
import math

NAN = float("nan")


def fills(dtype):
    """the two fills every framed case runs under: all-NaN and a finite pattern (7 + 3j / 7.0)"""
    if dtype.is_complex:
        return (complex(NAN, NAN), complex(7.0, 3.0))
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
