"""The framed-buffer checks of tests/arena.py fail when they should -- shown on CPU tensors, with planted defects.

The "kernels" here are numpy functions working in place on the view they are given (and, where the defect is an out-of-range
access, on the arena memory around it).  The operation is y = 2 x per row.  A clean function passes every check; each planted
defect -- a one-element write just before / just after the interior, a write into row padding, a read one element past the
interior, a 1e-9 leak from the neighbouring row -- is reported.  The last two are far below any rounding tolerance on Gaussian
data: they are caught because the checks compare bits under two fills and track NaNs, which is what tests/test_gpu_isolation.py
relies on for the HIP kernels."""
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


def test_bits_are_exact_and_nan_safe():
    a = torch.tensor([float("nan"), 0.0, -0.0, 1.0])
    assert arena.same_bits(a, a.clone())
    assert not arena.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert arena.bits(torch.zeros(3, dtype=torch.complex64)).shape == (3, 2)
    assert arena.bits(torch.zeros(3, dtype=torch.complex128)).dtype == torch.int64
