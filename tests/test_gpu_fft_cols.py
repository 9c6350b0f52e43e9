"""GPU tests of the column FFT plans (sdsp_hip_fft_cols_*, simpledsp_amd.FftColsPlan, fft2 / ifft2) against
the numpy contract of tests/fft_cols_ref.py: parity of both kernel variants, exact structure, the independence of a column from
everything around it (bit for bit), round trips, framed buffers at every element offset, NaN isolation, the other entry points and the
2-D transforms.  Shapes are small: every n of {8 .. 1024} is an instantiation of its own and 32 / 64 is the boundary between the
lane-per-column form and the LDS form; widths straddle the tile (16) and the wave (64) and 130 = 8 x 16 + 2 ends in a ragged tile."""

import numpy as np
import pytest

import arena
import fft_cols_ref as ref

pytestmark = pytest.mark.gpu

NS = (8, 16, 32, 64, 128, 256, 512, 1024)
WIDTHS = (1, 15, 16, 17, 63, 64, 65, 130)
PRECISIONS = ("f32", "f64")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def sd():
    import simpledsp_amd
    simpledsp_amd.load(build_if_missing=True)
    return simpledsp_amd


def _cube(seed, batch, n, width, f64):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((batch, n, width)) + 1j * rng.standard_normal((batch, n, width))
    return x.astype(ref.dtypes(f64)[0])


def _plan(sd, n, width, f64, reverse=False, window=None, shift=False, power=False, variant=0):
    p = sd.FftColsPlan(n, width, sd.reverse_fft if reverse else sd.forward_fft, sd.F64 if f64 else sd.F32,
                       "power" if power else "complex", shift, window)
    p.set_variant(variant)
    return p


# what a plan can be asked for: (reverse, windowed, shift, power)
CONFIGS = {
    "forward": (False, False, False, False),
    "reverse": (True, False, False, False),
    "hann": (False, True, False, False),
    "shift": (False, False, True, False),
    "reverse-shift": (True, False, True, False),
    "power": (False, False, False, True),
    "doppler": (False, True, True, True),  # window, shift and power together
}


def _out_like(torch, x, power):
    return torch.empty(x.shape, dtype=x.real.dtype if power else x.dtype, device=x.device)


def _check(got, want, n, f64, power, tag):
    if power:
        wmax = np.sqrt(want.max(axis=-2, keepdims=True))
        ex = ref.power_excess(got, want, wmax, n, f64)
        assert ex <= 1.0, (tag, "power error in units of its bound", ex)
        return ex * ref.tol(n, f64)
    err = ref.col_err(got, want, f64)
    assert err < ref.tol(n, f64), (tag, err, ref.tol(n, f64))
    return err


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", NS)
def test_parity_with_the_reference(sd, torch_cuda, n, precision):
    torch = torch_cuda
    f64 = precision == "f64"
    w = ref.hann(n)
    worst = {}
    for wi, width in enumerate(WIDTHS):
        xs = {batch: _cube(1000 * n + wi + batch, batch, n, width, f64) for batch in (1, 3)}
        for name, (reverse, windowed, shift, power) in CONFIGS.items():
            wants = {b: ref.fft_cols(x, f64, reverse, w if windowed else None, shift, power) for b, x in xs.items()}
            plan = _plan(sd, n, width, f64, reverse, w if windowed else None, shift, power)
            for variant in (0, 1):
                plan.set_variant(variant)
                for batch, x in xs.items():
                    got = plan.exec(torch.from_numpy(x).cuda()).cpu().numpy()
                    e = _check(got, wants[batch], n, f64, power, (n, precision, width, batch, name, variant))
                    worst[(variant, name)] = max(worst.get((variant, name), 0.0), e)
            plan.close()
    print(f"n {n} {precision}: worst error per (variant, config), tolerance {ref.tol(n, f64):.3g}: "
          + ", ".join(f"{k[0]}/{k[1]} {v:.3g}" for k, v in sorted(worst.items())))


# ---------------------------------------------------------------------------------------------------------------- 2. exact structure
def _structure_bound(n, f64):
    """An impulse at pulse p leaves X[k] = W_n^(p k).  Variant 1 forms it as 1 x table value plus zeros: the table's bits.  Variant 0
    reaches it as a product of at most 2 log2 n rounded unit factors (a thread twiddle and a W_32 constant per stage), each factor
    within eps / 2 of its exact value and each complex product within sqrt(5) eps / 2 of its own (one rounded product and one fused
    multiply-add per component): below 2 eps per factor, 4 log2 n eps in all."""
    eps = np.finfo(np.float64 if f64 else np.float32).eps
    return 4 * int(np.log2(n)) * eps


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", NS)
def test_impulse_gives_the_twiddle_row_and_ones_give_a_line(sd, torch_cuda, n, precision):
    torch = torch_cuda
    f64 = precision == "f64"
    cplx = ref.dtypes(f64)[0]
    width, col = 21, 17  # a ragged second tile; the column sits in it
    for reverse in (False, True):
        table = sd.calc_twiddles(n, sd.reverse_fft if reverse else sd.forward_fft).astype(cplx)  # rounded once to the precision
        scale = 1.0 / n if reverse else 1.0
        for p in (1, n // 2 + 3, n - 1):
            x = np.zeros((2, n, width), dtype=cplx)
            x[1, p, col] = 1.0
            want = (table[(p * np.arange(n)) % n] * cplx(scale)).astype(cplx)  # the scale is a power of two: exact
            for variant in (0, 1):
                plan = _plan(sd, n, width, f64, reverse, variant=variant)
                got = plan.exec(torch.from_numpy(x).cuda()).cpu().numpy()
                plan.close()
                tag = (n, precision, reverse, p, variant)
                line = got[1, :, col]
                d = float(np.abs(line.astype(np.complex128) - want.astype(np.complex128)).max()) / scale
                print(f"impulse {tag}: max |X - W| = {d:.3g}")
                if variant == 1:
                    assert np.array_equal(line, want), (tag, d)
                else:
                    assert d <= _structure_bound(n, f64), (tag, d, _structure_bound(n, f64))
                got[1, :, col] = 0
                flat = got.view(ref.dtypes(f64)[1])
                assert not flat.any() and not np.signbit(flat).any(), (tag, "another column is not +0")
        # a column of ones: n at k = 0 (1 after reverse), zeros elsewhere
        x = np.zeros((2, n, width), dtype=cplx)
        x[0, :, 3] = 1.0
        want = np.zeros((2, n, width), dtype=np.complex128)
        want[0, 0, 3] = 1.0 if reverse else n
        for variant in (0, 1):
            plan = _plan(sd, n, width, f64, reverse, variant=variant)
            got = plan.exec(torch.from_numpy(x).cuda()).cpu().numpy()
            plan.close()
            assert np.abs(got - want).max() <= ref.tol(n, f64) * want[0, 0, 3].real, (n, precision, reverse, variant)


# ---------------------------------------------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", NS)
def test_a_column_has_the_same_bits_alone_and_anywhere(sd, torch_cuda, n, precision):
    """every column of cube 2 of a 3 x n x 130 call, transformed alone (width = 1, batch = 1), has the bits it got in the matrix: first
    and last lane, both sides of every tile edge, the ragged tile; in place and out of place; each variant by itself"""
    torch = torch_cuda
    f64 = precision == "f64"
    width = 130
    x = torch.from_numpy(_cube(7 * n + 1, 3, n, width, f64)).cuda()
    alone_in = x[2].transpose(0, 1).contiguous().view(width, n, 1)  # 130 cubes of n x 1
    w = ref.hann(n) + 0.25
    for name in ("hann", "reverse-shift", "doppler"):
        reverse, windowed, shift, power = CONFIGS[name]
        for variant in (0, 1):
            big = _plan(sd, n, width, f64, reverse, w if windowed else None, shift, power, variant)
            one = _plan(sd, n, 1, f64, reverse, w if windowed else None, shift, power, variant)
            out = big.exec(x, _out_like(torch, x, power))
            alone = _out_like(torch, alone_in, power)
            for r in range(width):
                one.exec_ptr(alone_in[r].data_ptr(), alone[r].data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            tag = (n, precision, name, variant)
            assert arena.same_bits(alone.view(width, n).transpose(0, 1).contiguous(), out[2].contiguous()), (tag, "out of place")
            if not power:
                inplace = big.exec(x.clone())
                assert arena.same_bits(inplace, out), (tag, "in place differs from out of place")
                alone2 = alone_in.clone()
                for r in range(width):
                    one.exec_ptr(alone2[r].data_ptr(), alone2[r].data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert arena.same_bits(alone2, alone), (tag, "a single column in place")
            # batch and cube index: cube 2 alone
            solo = big.exec(x[2:3].contiguous(), _out_like(torch, x[2:3], power))
            assert arena.same_bits(solo[0], out[2]), (tag, "batch 1 against cube 2 of 3")
            big.close()
            one.close()


# ---------------------------------------------------------------------------------------------------------------- 4. round trip
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", NS)
def test_reverse_undoes_forward(sd, torch_cuda, n, precision):
    torch = torch_cuda
    f64 = precision == "f64"
    for width in (17, 130):
        x = _cube(n + width, 3, n, width, f64)
        for shift in (False, True):
            for variant in (0, 1):
                fwd = _plan(sd, n, width, f64, False, shift=shift, variant=variant)
                rev = _plan(sd, n, width, f64, True, shift=shift, variant=variant)
                d = torch.from_numpy(x).cuda()
                rev.exec(fwd.exec(d))
                err = ref.col_err(d.cpu().numpy(), x.astype(np.complex128), f64)
                assert err < 2 * ref.tol(n, f64), (n, precision, width, shift, variant, err)
                fwd.close()
                rev.close()


# ---------------------------------------------------------------------------------------------------------------- 5. framed buffers
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", (8, 64, 1024))
def test_framed_buffers_and_offset_pointers(sd, torch_cuda, n, precision):
    """in and out inside sentinel frames, each starting 0 .. 3 elements past a 16-byte boundary: the bits of the allocator-aligned
    call, no frame byte changed, in unchanged out of place"""
    torch = torch_cuda
    f64 = precision == "f64"
    margin = 64  # elements: a multiple of 16 bytes for every element type here
    w = ref.hann(n) + 0.5
    for width in (17, 65):
        x = torch.from_numpy(_cube(3 * n + width, 2, n, width, f64)).cuda()
        for name in ("forward", "reverse-shift", "doppler"):
            reverse, windowed, shift, power = CONFIGS[name]
            for variant in (0, 1):
                plan = _plan(sd, n, width, f64, reverse, w if windowed else None, shift, power, variant)
                out_dtype = x.real.dtype if power else x.dtype
                clean = plan.exec(x, torch.empty(x.shape, dtype=out_dtype, device="cuda"))
                torch.cuda.synchronize()
                tag = (n, precision, width, name, variant)
                for li in range(4):
                    for lo in range(4):
                        for fi, fo in zip(arena.fills(x.dtype), arena.fills(out_dtype)):
                            a_in, v_in = arena.framed(torch, tuple(x.shape), x.dtype, li, margin, fi)
                            a_out, v_out = arena.framed(torch, tuple(x.shape), out_dtype, lo, margin, fo)
                            v_in.copy_(x)
                            before_in, before_out = arena.bits(a_in).clone(), arena.bits(a_out).clone()
                            plan.exec(v_in, v_out)
                            torch.cuda.synchronize()
                            arena.assert_frame_untouched(before_out, a_out, arena.interior_mask(torch, a_out, v_out))
                            assert torch.equal(arena.bits(a_in), before_in), (tag, li, lo, "the input or its frame was written")
                            assert arena.same_bits(v_out, clean), (tag, li, lo, "differs from the aligned call")
                    if not power:  # in place
                        for fill in arena.fills(x.dtype):
                            a, v = arena.framed(torch, tuple(x.shape), x.dtype, li, margin, fill)
                            v.copy_(x)
                            before = arena.bits(a).clone()
                            plan.exec(v)
                            torch.cuda.synchronize()
                            arena.assert_frame_untouched(before, a, arena.interior_mask(torch, a, v))
                            assert arena.same_bits(v, clean), (tag, li, "in place differs from the aligned call")
                plan.close()


# ---------------------------------------------------------------------------------------------------------------- 6. NaN isolation
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", NS)
def test_a_nan_stays_in_its_column(sd, torch_cuda, n, precision):
    torch = torch_cuda
    f64 = precision == "f64"
    width = 130
    x = torch.from_numpy(_cube(11 * n, 3, n, width, f64)).cuda()
    # first and last column, both sides of a tile edge (15 | 16) and of the wave edge of the short form (63 | 64), the ragged tile;
    # first and last row
    poisons = [(0, 0, 0), (0, n - 1, 129), (1, 0, 15), (1, n - 1, 16), (2, 0, 63), (2, n - 1, 64), (2, n // 2, 128)]
    bad = x.clone()
    mask = torch.zeros(x.shape, dtype=torch.bool, device="cuda")
    for b, p, r in poisons:
        bad[b, p, r] = complex(float("nan"), float("nan"))
        mask[b, :, r] = True
    w = ref.hann(n)  # w[0] = 0: the NaN of row 0 meets a zero weight and must still poison its column
    assert w[0] == 0.0
    for name in ("forward", "hann", "reverse-shift", "doppler"):
        reverse, windowed, shift, power = CONFIGS[name]
        for variant in (0, 1):
            plan = _plan(sd, n, width, f64, reverse, w if windowed else None, shift, power, variant)
            new = lambda: _out_like(torch, x, power)  # noqa: E731
            clean, out = plan.exec(x, new()), plan.exec(bad, new())
            torch.cuda.synchronize()
            arena.assert_nan_exactly(out, clean, mask, tag=str((n, precision, name, variant)))
            if not power:
                arena.assert_nan_exactly(plan.exec(bad.clone()), clean, mask, tag=str((n, precision, name, variant, "in place")))
            plan.close()


# ---------------------------------------------------------------------------------------------------------------- 7. other entry points
@pytest.mark.parametrize("n", (16, 256))
def test_graph_capture_and_replay(sd, torch_cuda, n):
    torch = torch_cuda
    x = torch.from_numpy(_cube(n, 3, n, 65, False)).cuda()
    plan = _plan(sd, n, 65, False, window=ref.hann(n), shift=True, power=True)
    want = plan.exec(x)
    out = torch.zeros_like(want)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.exec(x, out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert arena.same_bits(out, want)
    x.mul_(2.0)
    g.replay()
    torch.cuda.synchronize()
    assert arena.same_bits(out, plan.exec(x))  # the replay read the new input


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exec_host_batch_zero_launches_and_info(sd, torch_cuda, precision):
    torch = torch_cuda
    f64 = precision == "f64"
    n, width = 128, 33
    x = _cube(5, 3, n, width, f64)
    w = ref.hann(n)
    for variant in (0, 1):
        plan = _plan(sd, n, width, f64, variant=variant)
        dev = plan.exec(torch.from_numpy(x).cuda()).cpu().numpy()
        host = x.copy()
        assert plan.exec_host(host) is host and np.array_equal(host.view(np.uint8), dev.view(np.uint8))  # in place
        apart = np.full_like(x, 7)
        keep = x.copy()
        plan.exec_host(keep, apart)
        assert np.array_equal(apart.view(np.uint8), dev.view(np.uint8)) and np.array_equal(keep, x)
        dop = _plan(sd, n, width, f64, window=w, shift=True, power=True, variant=variant)
        pw = dop.exec_host(x)
        assert pw.dtype == ref.dtypes(f64)[1] and pw.shape == x.shape
        assert np.array_equal(pw, dop.exec(torch.from_numpy(x).cuda()).cpu().numpy())
        # batch == 0 does nothing, and needs no valid data behind the pointers' first byte
        d = torch.from_numpy(x).cuda()
        plan.exec_ptr(d.data_ptr(), d.data_ptr(), 0)
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), x)
        assert plan.launches(0) == 0 and plan.launches(1) == 1 and plan.launches(3) == 1 and plan.launches(1 << 20) == 1
        i, j = plan.info(), dop.info()
        es = 16 if f64 else 8
        assert (i["n"], i["width"], i["direction"], i["precision"]) == (n, width, sd.FORWARD, sd.F64 if f64 else sd.F32)
        assert (i["output"], i["shift"], i["windowed"], i["device"], i["variant"]) == (sd.FFT_COLS_COMPLEX, 0, 0, 0, variant)
        assert (j["output"], j["shift"], j["windowed"]) == (sd.FFT_COLS_POWER, 1, 1)
        assert i["algorithmic_bytes"] == n * width * 2 * es and j["algorithmic_bytes"] == n * width * (es + es // 2)
        if variant == 0:
            assert i["kernel"] == "sdsp_fft_cols_kernel" and (i["tile_columns"], i["threads"]) == (16, 64)
            assert i["lds_bytes"] == n * 16 * (es // 2)
        else:
            assert i["kernel"] == "sdsp_fft_cols_plain_kernel" and i["lds_bytes"] == 0 and i["threads"] == i["tile_columns"] * n
        plan.close()
        dop.close()
    short = _plan(sd, 32, 5, f64).info()
    assert (short["tile_columns"], short["threads"], short["lds_bytes"]) == (64, 64, 0)
    big = _plan(sd, 1024, 5, f64).info()
    assert (big["tile_columns"], big["threads"], big["lds_bytes"]) == (16, 512, 1024 * 16 * (8 if f64 else 4))
    # a grid that does not fit one launch is issued over whole cubes: 2^31 - 1 workgroups at most
    wide = _plan(sd, 8, 64 * 1000, f64)
    per = (2 ** 31 - 1) // 1000
    assert wide.launches(per) == 1 and wide.launches(per + 1) == 2 and wide.launches(3 * per + 1) == 4


def test_overlap_and_alignment_rules(sd, torch_cuda):
    torch = torch_cuda
    L = sd._lib
    n, width, batch = 64, 17, 2
    elems = batch * n * width
    for f64 in (False, True):
        es = 16 if f64 else 8
        buf = torch.zeros(4 * elems + 8, dtype=torch.complex128 if f64 else torch.complex64, device="cuda")
        base = buf.data_ptr()
        cx = _plan(sd, n, width, f64)
        pw = _plan(sd, n, width, f64, power=True)
        rc = lambda plan, i, o, b=batch: plan._lib.sdsp_hip_fft_cols_exec(plan._h, i, o, b, None)  # noqa: E731
        assert rc(cx, base, base) == L.OK                                   # in place
        assert rc(cx, base, base + elems * es) == L.OK                      # touching, disjoint
        assert rc(cx, base + elems * es, base) == L.OK
        for off in (es, (elems - 1) * es, -es):                             # any partial overlap
            assert rc(cx, base + elems * es, base + elems * es + off) == L.ERR_INVALID_ARG, off
        assert rc(pw, base, base) == L.ERR_INVALID_ARG                      # POWER runs out of place
        assert rc(pw, base, base + elems * es) == L.OK
        assert rc(pw, base + elems * es // 2, base) == L.OK                 # the real output is half as long
        assert rc(pw, base + elems * es // 2 - es, base) == L.ERR_INVALID_ARG
        assert rc(pw, base, base + elems * es - es // 2) == L.ERR_INVALID_ARG
        # alignment: one element of the pointer's own type
        assert rc(cx, base + es // 2, base + 2 * elems * es) == L.ERR_INVALID_ARG
        assert rc(cx, base, base + 2 * elems * es + es // 2) == L.ERR_INVALID_ARG
        assert rc(pw, base, base + 2 * elems * es + es // 2) == L.OK         # a real element
        assert rc(pw, base, base + 2 * elems * es + es // 4) == L.ERR_INVALID_ARG
        assert rc(cx, None, base) == L.ERR_INVALID_ARG and rc(cx, base, None) == L.ERR_INVALID_ARG
        assert rc(cx, base, base, (1 << 40) // (n * width) + 1) == L.ERR_INVALID_SIZE
        assert rc(cx, None, None, 0) == L.ERR_INVALID_ARG                   # null pointers are refused before batch is looked at
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            cx.exec(buf[:elems].view(batch, n, width).real)
        with pytest.raises(ValueError):
            cx.exec(buf[:elems].view(batch, width, n))
        with pytest.raises(ValueError):
            cx.set_variant(2)


# ---------------------------------------------------------------------------------------------------------------- 8. fft2
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,m,used", [(8, 16, 16), (64, 64, 48), (1024, 32, 32), (32, 4096, 4096)])
def test_fft2_and_ifft2_equal_numpy(sd, torch_cuda, n, m, used, precision):
    """(3, n, m) images; the (64, 64) case holds 48 columns of data zero-padded to 64.  Bounds: two transforms in a row, so the sums
    of the per-transform bounds: f32 2e-6 normwise over the image, f64 4 (n + m) eps of the image's largest |X|"""
    torch = torch_cuda
    f64 = precision == "f64"
    x = _cube(n + m, 3, n, m, f64)
    x[:, :, used:] = 0
    for inverse in (False, True):
        want = (np.fft.ifft2 if inverse else np.fft.fft2)(x.astype(np.complex128))
        d = torch.from_numpy(x).cuda()
        got = (sd.ifft2 if inverse else sd.fft2)(d)
        assert got is d  # in place
        g = d.cpu().numpy().astype(np.complex128)
        diff = np.abs(g - want)
        if f64:
            err = float((diff.max(axis=(-2, -1)) / np.abs(want).max(axis=(-2, -1))).max())
            bound = 4 * (n + m) * ref.EPS64
        else:
            err = float((np.sqrt((diff ** 2).sum(axis=(-2, -1))) / np.sqrt((np.abs(want) ** 2).sum(axis=(-2, -1)))).max())
            bound = 2e-6
        print(f"fft2 ({n}, {m}) {precision} inverse={inverse}: err {err:.3g}, bound {bound:.3g}")
        assert err < bound, (n, m, precision, inverse, err, bound)
