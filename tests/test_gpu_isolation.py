"""Framed buffers, offset pointers and NaN isolation for the core kernels -- FFT exec / convolve / real-input plans, biquad
banks, FIR banks, FFT-domain FIR banks -- on a real MI355X, through the Python wrappers the other GPU tests use.

Every case computes a CLEAN result in an ordinary, aligned, exactly-sized tensor and holds it to the independent reference at
the tolerance the family's own test file uses (the CPU oracle, numpy.fft in double above 2^20; f64 filters bit for bit).  Every
other assertion is a bit-equality or a NaN mask against that clean result (tests/arena.py):

* frame and alignment: the same input inside ONE larger tensor, starting 0 / 1 / 2 elements (rows: 0 / pad columns) past a
  512-byte boundary, under an all-NaN fill and a finite fill -- the interior has the clean bits both times and no element of
  the frame or of the row padding changes.  A write outside the addressed range, a read outside it that reaches an output, or
  a kernel that cannot take an element-aligned pointer fails here.
* isolation: one NaN in each of a few transforms / channels chosen on both sides of a workgroup tile boundary -- the poisoned
  ones are NaN where the operation says, every other transform / channel (output and state) has the clean bits.

tests/test_arena_host.py shows on the CPU that these checks report a one-element overrun, a read past the end and a 1e-9 leak
between neighbours."""
import functools

import numpy as np
import pytest

import arena
from conftest import rel_max_err
from test_gpu_fft import EPS64, SIZE_TABLE, TOL32

pytestmark = pytest.mark.gpu

NAN = float("nan")


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


def _cdt(torch, f64):
    return torch.complex128 if f64 else torch.complex64


def _rdt(torch, f64):
    return torch.float64 if f64 else torch.float32


def _randc(torch, shape, f64, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.view_as_complex(torch.randn(tuple(shape) + (2,), generator=g, device="cuda", dtype=_rdt(torch, f64)))


# ------------------------------------------------------------------------------------------------ FFT exec
FFT_CASES = [(n, radix, prec) for n, radix, prec, _, _, _ in SIZE_TABLE] + \
            [(1 << 21, 2, "f32"), (1 << 22, 2, "f32"), (1 << 23, 2, "f32"), (1 << 20, 2, "f64")]
FFT_VARIANTS = [0, 1, 2, 3, 8, 99]


def _ragged_batch(n, f64):
    """larger than, and not a multiple of, the transforms per workgroup / wave / ticket unit / ring of every kernel of the size:
    the ragged batches of tests/test_gpu_fft.py"""
    if f64:
        return {64: 1031, 1024: 257, 4096: 67, 8192: 37, 16384: 19, 1 << 15: 515, 1 << 20: 17}[n]
    if n <= 64:
        return 1031
    return {256: 4099, 512: 1031, 1024: 129, 2048: 130, 4096: 255, 8192: 300, 16384: 300, 32768: 67, 1 << 16: 531, 1 << 18: 131,
            1 << 19: 67, 1 << 20: 37, 1 << 21: 19, 1 << 22: 9, 1 << 23: 3}[n]


def _tiles(kernel, n, f64):
    """transforms that share a workgroup tile / a wave / a ticket unit in the kernel the plan reports (csrc/fft_reg.hip,
    fft_reg64.hip, fft_wave.hip, fft_2pass.hip: fft_2pass_fused_shape); one transform per workgroup everywhere else"""
    if kernel == "sdsp_fft_reg_kernel":
        return {max(1, (2048 if n <= 2048 else 4096) // n)}
    if kernel == "sdsp_fft_reg_f64_kernel":
        return {max(1, (1024 if n <= 1024 else 2048) // n)}
    if kernel == "sdsp_fft_wave_f32":
        per_wave = max(1, 1024 // n)
        return {per_wave, 4 * per_wave}
    if kernel == "sdsp_fft1024_wave":
        return {2 if f64 else 4}
    if kernel.startswith("sdsp_fft2p"):
        return {max(1, (8 << 20) // (n * (16 if f64 else 8)))}
    return {1}


def _poison_set(batch, tiles):
    p = {0, batch - 1}
    for g in tiles:
        p |= {g - 1, g}
    return sorted(r for r in p if 0 <= r < batch)


def _poison_rows(x, rows, value):
    """one NaN in each row of `rows`, at a different index in each: first point, last point, one in the middle"""
    xp = x.clone()
    n = x.shape[-1]
    for i, r in enumerate(rows):
        xp[r, (0, n - 1, n // 2 + 1)[i % 3] % n] = value
    return xp


def _picks(batch):
    return sorted({0, batch // 2, batch - 1})


@functools.lru_cache(maxsize=2)
def _fft_reference(oracle, torch, n, radix, f64, batch):
    """(x on the device, {reverse: reference of the picked transforms}): the oracle's algorithm of the plan's radix in double on
    the input as the plan sees it; numpy.fft in double above 2^20, where the oracle takes seconds per transform"""
    x = _randc(torch, (batch, n), f64, n % 1009 + 7 * radix + batch)
    xs = x[_picks(batch)].cpu().numpy().astype(np.complex128)
    ref_radix = radix or 2
    if radix == 4 and n.bit_length() % 2 == 0:  # not a power of 4 (never listed): the plan would not exist
        ref_radix = 2
    want = {}
    for rev in (False, True):
        if n <= (1 << 20):
            want[rev] = oracle.fft(xs, ref_radix, rev)
        else:
            want[rev] = np.fft.ifft(xs, axis=-1) if rev else np.fft.fft(xs, axis=-1)
    return x, want


def _fft_id(case):
    n, radix, prec = case
    return f"n{n}-r{radix}-{prec}"


@pytest.mark.parametrize("variant", FFT_VARIANTS)  # varies fastest: the size's reference is computed once
@pytest.mark.parametrize("case", FFT_CASES, ids=_fft_id)
def test_fft_exec_frame_alignment_and_isolation(sd, torch_cuda, oracle, case, variant):
    """every row of test_gpu_fft.SIZE_TABLE plus f32 2^21 .. 2^23 and f64 2^20, both directions, every variant number (numbers a
    size does not have fall back to its default and still run); batch 1, a ragged batch, and -- for the sizes that own a
    workspace -- the ragged batch through a plan of max_batch 2 (sliced exec).  The persistent kernels' ragged batches are longer
    than their ring of intermediates, so a poisoned slot is re-used by a clean transform within the call."""
    torch = torch_cuda
    n, radix, precision = case
    f64 = precision == "f64"
    prec = sd.F64 if f64 else sd.F32
    batch = _ragged_batch(n, f64)
    x, want = _fft_reference(oracle, torch, n, radix, f64, batch)
    picks = _picks(batch)
    tol = 4 * n * EPS64 if f64 else TOL32
    margin = max(n, 8192)
    workspace = n >= ((1 << 15) if f64 else (1 << 16))
    configs = [(1, 1), (batch, batch)] + ([(batch, 2)] if workspace else [])
    for T, rev in ((sd.forward_fft, False), (sd.reverse_fft, True)):
        for b, max_batch in configs:
            plan = sd.FftPlan(n, radix, T, prec, max_batch=max_batch)
            plan.set_variant(variant)
            kernel = plan.info.kernel.decode()
            tag = (n, radix, precision, variant, "rev" if rev else "fwd", b, max_batch, kernel)
            xb = x[:b]
            clean = xb.clone()
            plan.exec(clean)
            plan.status()
            pk = [0] if b == 1 else picks
            err = rel_max_err(clean[pk].cpu().numpy(), want[rev][[picks.index(p) for p in pk]])
            assert err < tol, (tag, err)
            # 1. frame and alignment
            arena.check_framed(torch, xb, clean, plan.exec, (0, 1, 2), margin, what=tag)
            plan.status()
            # 2. isolation
            rows = _poison_set(b, _tiles(kernel, n, f64))
            xp = _poison_rows(xb, rows, complex(NAN, NAN))
            plan.exec(xp)
            plan.status()
            try:
                arena.assert_rows_isolated(xp, clean, rows)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None
            plan.close()


# ------------------------------------------------------------------------------------------------ fused convolution
# the fused and the two-pass sizes of test_gpu_fft.test_fast_convolution_matches_reference_composition, with its batches where
# they are ragged against the size's tile (larger ones cut to the ragged batch of the exec test: minutes, not tens of minutes)
CONV_CASES = [(4096, 4, "f32", 67), (4096, 2, "f32", 5), (256, 4, "f32", 33), (1024, 2, "f64", 4), (1 << 15, 2, "f32", 2),
              (16, 2, "f32", 300), (64, 4, "f32", 70), (1024, 2, "f32", 9), (1024, 4, "f32", 1030), (256, 2, "f32", 1027),
              (256, 4, "f32", 1026), (512, 2, "f32", 77), (2048, 2, "f32", 35), (16384, 4, "f32", 7), (8192, 2, "f32", 37),
              (16384, 2, "f32", 5), (1 << 15, 2, "f32", 9), (64, 4, "f64", 70), (4096, 4, "f64", 3), (8192, 2, "f64", 37),
              (16384, 2, "f64", 19), (4096, 2, "f64", 5),
              (1 << 16, 2, "f32", 3), (1 << 16, 4, "f32", 2), (1 << 17, 2, "f64", 2), (1 << 21, 2, "f32", 2), (1 << 20, 2, "f32", 2),
              (1 << 16, 2, "f32", 600), (1 << 20, 2, "f32", 33), (1 << 18, 2, "f64", 70), (1 << 22, 2, "f32", 9)]


def _conv_variants(n, radix, f64):
    """the variants test_fast_convolution_matches_reference_composition runs for the size"""
    fused = n <= (8192 if f64 else 16384) or (radix == 2 and n == (16384 if f64 else 1 << 15))
    two_fused = (not f64 and (n in (256, 1024, 16384) or (radix == 2 and n in (512, 2048, 4096, 8192)))) or \
                (f64 and radix == 2 and n in (4096, 8192))
    return (0, 1, 2) if two_fused else (0, 1) if fused else (0,)


@pytest.mark.parametrize("n,radix,precision,batch", CONV_CASES)
def test_fused_convolution_frame_alignment_and_isolation(sd, torch_cuda, oracle, n, radix, precision, batch):
    torch = torch_cuda
    f64 = precision == "f64"
    prec = sd.F64 if f64 else sd.F32
    x = _randc(torch, (batch, n), f64, n % 1013 + batch)
    h = _randc(torch, (n,), f64, n % 1013 + batch + 1)
    picks = _picks(batch)
    xs, hs = x[picks].cpu().numpy().astype(np.complex128), h.cpu().numpy().astype(np.complex128)
    if n <= (1 << 16):
        want = oracle.fft(oracle.fft(xs, radix) * hs, radix, True)
    else:
        want = np.fft.ifft(np.fft.fft(xs, axis=-1) * hs, axis=-1)
    tol = 2e-6 if not f64 else 8 * n * EPS64  # two transforms and a product (test_gpu_fft.py)
    margin = max(n, 8192)
    for variant in _conv_variants(n, radix, f64):
        plan = sd.FftPlan(n, radix, sd.forward_fft, prec, max_batch=batch)
        plan.set_variant(variant)
        tag = (n, radix, precision, batch, variant)
        clean = x.clone()
        plan.convolve(clean, h)
        plan.status()
        err = rel_max_err(clean[picks].cpu().numpy(), want)
        assert err < tol, (tag, err)
        # frame and lead on x (h aligned), then lead 0 / 1 on h (x framed, lead 1)
        arena.check_framed(torch, x, clean, lambda v: plan.convolve(v, h), (0, 1, 2), margin, what=tag + ("x",))
        for lead_h in (0, 1):
            for fill in arena.fills(h.dtype):
                h_arena, h_view = arena.framed(torch, (n,), h.dtype, lead_h, margin, fill)
                h_view.copy_(h)
                h_before = arena.bits(h_arena).clone()
                arena.check_framed(torch, x, clean, lambda v: plan.convolve(v, h_view), (1,), margin, what=tag + ("h", lead_h, fill))
                assert torch.equal(arena.bits(h_arena), h_before), (tag, "h or its frame was written")
        plan.status()
        rows = _poison_set(batch, _tiles(plan.info.kernel.decode(), n, f64) | {max(1, 2048 // n)})
        xp = _poison_rows(x, rows, complex(NAN, NAN))
        plan.convolve(xp, h)
        plan.status()
        try:
            arena.assert_rows_isolated(xp, clean, rows)
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from None
        plan.close()


# ------------------------------------------------------------------------------------------------ real-input plans
# the n_real / radix / precision rows of test_gpu_fft.test_real_input_packing, one ragged batch each (its larger one)
RFFT_CASES = [(32, 2, 5, "f32"), (32, 4, 130, "f32"), (128, 4, 33, "f32"), (1024, 2, 130, "f32"), (512, 2, 1027, "f32"),
              (512, 4, 1029, "f32"), (2048, 2, 1030, "f32"), (4096, 2, 9, "f32"), (2048, 4, 5, "f32"), (8192, 2, 300, "f32"),
              (8192, 4, 9, "f32"), (32768, 2, 67, "f32"), (16384, 2, 131, "f32"), (32768, 4, 41, "f32"), (65536, 2, 19, "f32"),
              (32, 2, 70, "f64"), (128, 4, 33, "f64"), (2048, 4, 5, "f64"), (16384, 2, 19, "f64"), (8192, 2, 33, "f64"),
              (8192, 4, 3, "f64"), (32768, 2, 9, "f64")]


def _rfft_has_variant_1(n_real, radix, f64):
    half = n_real // 2
    wave = not f64 and radix == 2 and half == 512
    big = not f64 and ((radix == 2 and half in (2048, 4096, 8192, 16384)) or (radix == 4 and half in (4096, 16384)))
    big64 = f64 and radix == 2 and half in (4096, 8192)
    return wave or big or big64


@pytest.mark.parametrize("n_real,radix,batch,precision", RFFT_CASES)
def test_real_input_plans_frame_alignment_and_isolation(sd, torch_cuda, oracle, n_real, radix, batch, precision):
    """sdsp_hip_fft_exec asks every plan, real-input ones included, for a pointer aligned to one COMPLEX element (csrc/capi.hip),
    so `lead` counts pairs of real samples here; a pointer that is only aligned to one real sample is refused with
    SDSP_HIP_ERR_INVALID_ARG, which is asserted too."""
    torch = torch_cuda
    f64 = precision == "f64"
    prec = sd.F64 if f64 else sd.F32
    half = n_real // 2
    tol = 4 * n_real * EPS64 if f64 else TOL32
    g = torch.Generator(device="cuda").manual_seed(n_real + batch)
    x = torch.randn((batch, n_real), generator=g, device="cuda", dtype=_rdt(torch, f64))
    full = oracle.fft(x.cpu().numpy().astype(np.complex128), 2)
    want = full[:, :half].copy()
    want[:, 0] = full[:, 0].real + 1j * full[:, half].real
    packed = torch.view_as_real(torch.from_numpy(want).to(_cdt(torch, f64)).cuda()).reshape(batch, n_real).contiguous()
    margin = max(n_real, 8192)
    for variant in ((0, 1) if _rfft_has_variant_1(n_real, radix, f64) else (0,)):
        for T, src in ((sd.forward_fft, x), (sd.reverse_fft, packed)):
            fwd = T is sd.forward_fft
            plan = sd.RfftPlan(n_real, radix, T, max_batch=batch, precision=prec)
            plan.set_variant(variant)
            kernel = plan.info.kernel.decode()
            tag = (n_real, radix, precision, batch, variant, "fwd" if fwd else "rev", kernel)
            clean = src.clone()
            plan.exec(clean)
            torch.cuda.synchronize()
            if fwd:
                got = torch.view_as_complex(clean.view(batch, half, 2)).cpu().numpy()
                assert rel_max_err(got, want) < tol, (tag, rel_max_err(got, want))
            else:
                assert rel_max_err(clean.cpu().numpy(), x.cpu().numpy()) < tol, tag
            arena.check_framed(torch, src, clean, plan.exec, (0, 2, 4), margin, what=tag)
            # a float-aligned pointer is not a complex-aligned one: refused, nothing runs
            a, view = arena.framed(torch, (batch, n_real), src.dtype, 1, margin, 7.0)
            before = arena.bits(a).clone()
            with pytest.raises(sd.SdspHipError):
                plan.exec(view)
            torch.cuda.synchronize()
            assert torch.equal(arena.bits(a), before)
            # isolation: one real sample (forward) / one packed bin, both halves (reverse) per poisoned transform
            tiles = _tiles(kernel, half, f64) | {max(1, 2048 // half)}
            rows = _poison_set(batch, tiles)
            xp = src.clone()
            for i, r in enumerate(rows):
                if fwd:
                    xp[r, (0, n_real - 1, half + 1)[i % 3]] = NAN
                else:
                    k = (0, half - 1, half // 2 + 1)[i % 3] % half
                    xp[r, 2 * k:2 * k + 2] = NAN
            plan.exec(xp)
            torch.cuda.synchronize()
            try:
                if fwd:  # a packed bin is NaN if either half is; bin 0 = (X[0], X[N/2]) in both
                    out, ref = xp.view(batch, half, 2), clean.view(batch, half, 2)
                    arena.assert_rows_isolated(out[:, 0], ref[:, 0], rows)
                    assert bool(torch.isnan(out[rows]).any(dim=-1).all()), "a bin of a poisoned transform is not NaN"
                    keep = torch.ones(batch, dtype=torch.bool, device="cuda")
                    keep[rows] = False
                    assert arena.same_bits(out[keep], ref[keep]), "clean transforms changed"
                else:
                    arena.assert_rows_isolated(xp, clean, rows)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None
            plan.close()


# ------------------------------------------------------------------------------------------------ biquad banks
IIR_PRECISIONS = ["f32", "f64", "mixed"]
IIR_SHAPES = [(192, 2048), (130, 2048), (257, 36), (65, 98)]
ROW_FRAMES = [(0, 0), (3, 0), (3, 3), (16, 0), (16, 16)]  # (pad, offset): stride = samples + pad, the block starts at `offset`


def _iir_prec(sd, torch, precision):
    return {"f32": (sd.F32, torch.float32, 1e-6), "f64": (sd.F64, torch.float64, 0.0),
            "mixed": (sd.F32_F64STATE, torch.float32, 1.2e-7)}[precision]


def _iir_f32_tol(precision, m, tol):
    """f32 recurrences: the 1e-6 of the four-section BASELINE filter; every further cascaded section adds its own rounding noise,
    so deeper cascades get that bound scaled by m / 4, x 2 -- the rule test_gpu_iir.test_more_than_eight_sections states for
    m_t = 10 .. 16, applied from m_t = 6 on (measured at m_t = 8 on this filter: 1.1e-6 .. 2.1e-6 against 4e-6; at m_t = 4:
    7.2e-7).  The mixed mode rounds once to float whatever the depth: its bound does not move."""
    return 2e-6 * m / 4 if precision == "f32" and m > 4 else tol


def _iir_expected_kernel(precision, m, variant, ptr, channels, samples, stride):
    """csrc/iir.hip's table: which kernel serves (precision, sections, shape, variant)"""
    ss = 8 if precision == "f64" else 4
    aligned = ptr % 16 == 0 and (stride * ss) % 16 == 0 and (samples * ss) % 16 == 0
    if m > 8 or variant == 2 or not aligned:
        return "sdsp_iir_direct_kernel"
    tiles = channels % 64 == 0 and (samples * ss) % 512 == 0
    if variant == 0:
        return "sdsp_iir_landing_kernel" if precision == "f32" and m <= 4 and tiles else "sdsp_iir_supertile_kernel"
    if variant == 1:
        return "sdsp_iir_wide_kernel" if tiles else "sdsp_iir_supertile_kernel"
    return "sdsp_iir_supertile_kernel"


def _cuts(samples):
    """two calls per row: one cut on a tile boundary where the row has one (both calls reach the vector kernels), one at an
    unaligned sample (both calls run the direct kernel and hand the state over)"""
    return [samples // 2, samples // 2 - 3] if samples >= 64 else [16, 17]


def _iir_poison(channels, samples, cut):
    """(channel, sample) -> earliest poisoned sample per channel"""
    where = {}
    for c, s in ((0, 0), (63, samples // 4 + 5), (64, cut - 1), (channels - 1, cut)):
        if c < channels:
            where[c] = min(s, where.get(c, samples))
    return where


def _make_bank(sd, m, channels, prec, kind, variant):
    bank = sd.casc_2o_iir(m, channels, prec, kind)
    bank.set_lp_coeff(10e3, 100e3)  # the BASELINE config-4 filter
    bank.set_variant(variant)
    return bank


def _check_iir_poisoned(torch, out, clean, state, clean_state, where, tag):
    """out / clean: (channels, samples); a poisoned channel has the clean bits before its sample and is NaN from it to the end;
    its state is NaN in every level that the recurrence feeds (levels 1 .. m_t) and holds the clean (finite) scaled inputs in
    level 0; clean channels are bit-identical in output and state"""
    samples = out.shape[1]
    masks = {c: torch.arange(samples, device=out.device) >= s for c, s in where.items()}
    try:
        arena.assert_rows_isolated(out, clean, list(where), nan_from=masks)
        st, cst = state.t(), clean_state.t()  # (channels, 3 * (m_t + 1))
        smask = torch.arange(st.shape[1], device=out.device) >= 3
        arena.assert_rows_isolated(st, cst, list(where), nan_from={c: smask for c in where})
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from None


@pytest.mark.parametrize("precision", IIR_PRECISIONS)
@pytest.mark.parametrize("m", [2, 4, 8, 12])
@pytest.mark.parametrize("shape", IIR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_biquad_bank_frame_and_isolation(sd, torch_cuda, oracle, precision, m, shape, variant):
    torch = torch_cuda
    prec, dt, tol = _iir_prec(sd, torch, precision)
    channels, samples = shape
    g = torch.Generator(device="cuda").manual_seed(channels * 7 + samples + m)
    x = torch.randn((channels, samples), generator=g, device="cuda", dtype=dt)
    tol = _iir_f32_tol(precision, m, tol)
    margin = 64 * (samples + 16)  # one whole [64 channels x row] tile on each side
    kernels = set()
    for kind in (sd.IIR_GENERIC, sd.IIR_LP):
        for cut in _cuts(samples):
            tag = (precision, m, shape, variant, kind, cut)
            bank = _make_bank(sd, m, channels, prec, kind, variant)
            clean = x.clone()
            for k, (s0, cnt) in enumerate(((0, cut), (cut, samples - cut))):
                name = bank.kernel_name(clean, samples=cnt, offset=s0)
                assert name == _iir_expected_kernel(precision, m, variant, clean.data_ptr() + s0 * clean.element_size(), channels,
                                                    cnt, samples), (tag, k, name)
                kernels.add(name)
                bank.process(clean, samples=cnt, offset=s0)
            torch.cuda.synchronize()
            clean_state = bank.state.clone()
            for c in sorted({0, 63, 64, channels - 1} & set(range(channels))):
                fo = oracle.iir(m)
                fo.set_lp_coeff(10e3, 100e3)
                ref = fo.process(x[c].cpu().numpy().astype(np.float64), kind)
                got = clean[c].cpu().numpy()
                if precision == "f64":
                    assert np.array_equal(got, ref), (tag, c)
                else:
                    assert rel_max_err(got, ref) < tol, (tag, c, rel_max_err(got, ref))
            # frame, row padding, both fills: output and state bit-identical to the clean call sequence
            for pad, offset in ROW_FRAMES:
                def run(view):
                    b = _make_bank(sd, m, channels, prec, kind, variant)
                    b.process(view, samples=cut, offset=offset)
                    b.process(view, samples=samples - cut, offset=offset + cut)
                    torch.cuda.synchronize()
                    assert arena.same_bits(b.state, clean_state), (tag, pad, offset, "state differs from the clean result")
                arena.check_framed(torch, x, clean, run, (0,), margin, row_stride=samples + pad, col_offset=offset,
                                   what=tag + (pad, offset))
            # isolation, in an exactly-sized tensor and in a padded, offset one
            where = _iir_poison(channels, samples, cut)
            xp = x.clone()
            for c, s in where.items():
                xp[c, s] = NAN
            for pad, offset in ((0, 0), (3, 3)):
                a, view = arena.framed(torch, shape, dt, 0, margin, 7.0, row_stride=samples + pad)
                block = view[:, offset:offset + samples]
                block.copy_(xp)
                before = arena.bits(a).clone()
                b = _make_bank(sd, m, channels, prec, kind, variant)
                b.process(view, samples=cut, offset=offset)
                b.process(view, samples=samples - cut, offset=offset + cut)
                torch.cuda.synchronize()
                arena.assert_frame_untouched(before, a, arena.interior_mask(torch, a, view, samples, offset))
                _check_iir_poisoned(torch, block, clean, b.state, clean_state, where, tag + (pad, offset))
    # the shapes reach the kernels they are listed for (variant 2 and m_t > 8 are the direct kernel by definition)
    if m <= 8 and variant != 2 and shape == (192, 2048):
        assert ("sdsp_iir_landing_kernel" if precision == "f32" and m <= 4 and variant == 0 else
                "sdsp_iir_wide_kernel" if variant == 1 else "sdsp_iir_supertile_kernel") in kernels, kernels
    if m <= 8 and variant != 2 and shape == (130, 2048):
        assert "sdsp_iir_supertile_kernel" in kernels, kernels
    assert "sdsp_iir_direct_kernel" in kernels, kernels  # the unaligned cut of every shape


@pytest.mark.parametrize("precision,shape", [("f32", (260, 333)), ("f64", (260, 333)), ("mixed", (260, 333)), ("f32", (7, 40))],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("m", [2, 4, 8, 12])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_interleaved_biquad_bank_frame_and_isolation(sd, torch_cuda, oracle, precision, shape, m, variant):
    """the sample-major layout: neighbouring channels are neighbouring lanes (16- / 8- / 4-byte lanes: variants 0 / 1 / 2).  The
    layout has no row padding (the row stride is the channel count); the buffer is framed with 0 / 1 / 2 leading elements and
    `offset` rows of the frame's fill in front of and behind the block."""
    torch = torch_cuda
    prec, dt, tol = _iir_prec(sd, torch, precision)
    channels, samples = shape
    tol = _iir_f32_tol(precision, m, tol)
    g = torch.Generator(device="cuda").manual_seed(channels * 5 + samples + m)
    x = torch.randn((samples, channels), generator=g, device="cuda", dtype=dt)
    cut = samples // 2 - 3
    margin = 8192
    for kind in (sd.IIR_GENERIC, sd.IIR_LP):
        tag = (precision, shape, m, variant, kind)
        bank = _make_bank(sd, m, channels, prec, kind, variant)
        clean = x.clone()
        bank.process_interleaved(clean, samples=cut, offset=0)
        bank.process_interleaved(clean, samples=samples - cut, offset=cut)
        torch.cuda.synchronize()
        clean_state = bank.state.clone()
        for c in sorted({0, 63, 64, channels - 1} & set(range(channels))):
            fo = oracle.iir(m)
            fo.set_lp_coeff(10e3, 100e3)
            ref = fo.process(x[:, c].cpu().numpy().astype(np.float64), kind)
            got = clean[:, c].cpu().numpy()
            if precision == "f64":
                assert np.array_equal(got, ref), (tag, c)
            else:
                assert rel_max_err(got, ref) < tol, (tag, c, rel_max_err(got, ref))
        where = _iir_poison(channels, samples, cut)
        xp = x.clone()
        for c, s in where.items():
            xp[s, c] = NAN
        for lead in (0, 1, 2):
            for rows_off in (0, 3):
                for fill in arena.fills(dt):
                    for src in (x, xp):
                        a, view = arena.framed(torch, (samples + 2 * rows_off, channels), dt, lead, margin, fill)
                        block = view[rows_off:rows_off + samples]
                        block.copy_(src)
                        before = arena.bits(a).clone()
                        b = _make_bank(sd, m, channels, prec, kind, variant)
                        b.process_interleaved(view, samples=cut, offset=rows_off)
                        b.process_interleaved(view, samples=samples - cut, offset=rows_off + cut)
                        torch.cuda.synchronize()
                        start = (block.data_ptr() - a.data_ptr()) // a.element_size()
                        arena.assert_frame_untouched(before, a, slice(start, start + block.numel()))
                        t2 = tag + (lead, rows_off, fill)
                        if src is x:
                            assert arena.same_bits(block, clean), (t2, "output differs from the clean result")
                            assert arena.same_bits(b.state, clean_state), (t2, "state differs from the clean result")
                        else:
                            _check_iir_poisoned(torch, block.t(), clean.t(), b.state, clean_state, where, t2)


# ------------------------------------------------------------------------------------------------ FIR banks
def _fir_taps(taps, f64, seed):
    h = np.random.default_rng(seed).standard_normal(taps)
    assert np.all(h.astype(np.float64 if f64 else np.float32) != 0), "a tap rounds to zero: the NaN mask would have a hole"
    return h


def _nan_span(samples, s, taps):
    """outputs that depend on input s: an indicator sequence through an all-ones filter of `taps` taps"""
    ind = np.zeros(samples)
    ind[s] = 1.0
    return np.convolve(ind, np.ones(taps))[:samples] > 0


def _fir_state(xrow, taps):
    """the history a call sequence leaves: the last taps - 1 inputs, newest first, zeros before the first sample"""
    hist = np.concatenate([np.zeros(taps - 1, xrow.dtype), xrow])[-(taps - 1):]
    return hist[::-1]


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("taps", [1, 16, 33, 257])
@pytest.mark.parametrize("shape", [(67, 100), (130, 1000), (9, 5000)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_fir_bank_frame_and_isolation(sd, torch_cuda, oracle, precision, taps, shape, variant):
    torch = torch_cuda
    f64 = precision == "f64"
    prec, dt, npdt = (sd.F64, torch.float64, np.float64) if f64 else (sd.F32, torch.float32, np.float32)
    channels, samples = shape
    h = _fir_taps(taps, f64, taps * 1000 + channels)
    g = torch.Generator(device="cuda").manual_seed(taps + channels + samples)
    x = torch.randn((channels, samples), generator=g, device="cuda", dtype=dt)
    cut = samples // 2 - 3
    tag = (precision, taps, shape, variant)
    margin = 64 * (samples + 16)

    def make():
        b = sd.fir_filter(taps, channels, prec)
        b.set_coeff(h)
        b.set_variant(variant)
        return b

    def two_calls(b, view, offset=0):
        b.process(view, samples=cut, offset=offset)
        b.process(view, samples=samples - cut, offset=offset + cut)
        torch.cuda.synchronize()

    bank = make()
    clean = x.clone()
    two_calls(bank, clean)
    clean_state = bank.state.clone()
    xh = x.cpu().numpy()
    # a sequential f32 sum of T terms carries ~sqrt(T) eps (test_gpu_fir.test_long_filters); 1e-6 for the short filters
    tol = max(1e-6, np.sqrt(taps) * 1.19e-7)
    for c in sorted({0, channels // 2, channels - 1}):
        ref = oracle.fir_process(h.astype(npdt).astype(np.float64), xh[c].astype(np.float64))[0]
        if f64:
            assert np.array_equal(clean[c].cpu().numpy(), ref), (tag, c)
        else:
            assert rel_max_err(clean[c].cpu().numpy(), ref) < tol, (tag, c)
    if taps > 1:
        want_state = np.stack([_fir_state(xh[c], taps) for c in range(channels)])
        assert np.array_equal(clean_state.cpu().numpy(), want_state), tag
    for pad, offset in ROW_FRAMES:
        def run(view):
            b = make()
            two_calls(b, view, offset)
            assert arena.same_bits(b.state, clean_state), (tag, pad, offset, "state differs from the clean result")
        arena.check_framed(torch, x, clean, run, (0,), margin, row_stride=samples + pad, col_offset=offset, what=tag + (pad, offset))
    where = _iir_poison(channels, samples, cut)
    xp = x.clone()
    for c, s in where.items():
        xp[c, s] = NAN
    masks = {c: torch.from_numpy(_nan_span(samples, s, taps)).cuda() for c, s in where.items()}
    xph = xp.cpu().numpy()
    for pad, offset in ((0, 0), (3, 3)):
        a, view = arena.framed(torch, shape, dt, 0, margin, 7.0, row_stride=samples + pad)
        block = view[:, offset:offset + samples]
        block.copy_(xp)
        before = arena.bits(a).clone()
        b = make()
        two_calls(b, view, offset)
        arena.assert_frame_untouched(before, a, arena.interior_mask(torch, a, view, samples, offset))
        try:
            arena.assert_rows_isolated(block, clean, list(where), nan_from=masks)
        except AssertionError as e:
            raise AssertionError(f"{tag + (pad, offset)}: {e}") from None
        if taps > 1:  # the history is the last taps - 1 inputs themselves, a NaN among them included
            want_state = torch.from_numpy(np.stack([_fir_state(xph[c], taps) for c in range(channels)])).cuda()
            assert arena.same_bits(b.state, want_state), (tag, pad, offset, "state")
        else:
            assert arena.same_bits(b.state, clean_state), (tag, pad, offset, "state")


# ------------------------------------------------------------------------------------------------ FFT-domain FIR banks
FIR_FFT_CASES = [("f32", 33, 64), ("f64", 33, 64), ("f32", 1000, 2048), ("f64", 1000, 2048), ("f64", 4096, 0), ("f32", 16384, 0)]


def _fft_fir_input(torch, precision, taps, channels, samples):
    f64 = precision == "f64"
    h = _fir_taps(taps, f64, taps + 1) / np.sqrt(taps)
    assert np.all(h.astype(np.float64 if f64 else np.float32) != 0)
    g = torch.Generator(device="cuda").manual_seed(taps + 3)
    x = torch.randn((channels, samples), generator=g, device="cuda", dtype=_rdt(torch, f64))
    state0 = torch.randn((channels, taps - 1), generator=g, device="cuda", dtype=_rdt(torch, f64))
    return h, x, state0


@functools.lru_cache(maxsize=4)
def _fft_fir_reference(oracle, torch, precision, taps, samples, c):
    """the oracle's direct-form FIR in double on the h, x and history the plan sees (seconds per channel at 16384 taps: once)"""
    npdt = np.float64 if precision == "f64" else np.float32
    h, x, state0 = _fft_fir_input(torch, precision, taps, 5, samples)
    return oracle.fir_process(h.astype(npdt).astype(np.float64), x[c].cpu().numpy().astype(np.float64),
                              state0[c].cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("sliced", [False, True], ids=["default-workspace", "sliced"])
@pytest.mark.parametrize("precision,taps,fft_n", FIR_FFT_CASES)
def test_fft_fir_bank_frame_and_isolation(sd, torch_cuda, oracle, precision, taps, fft_n, variant, sliced):
    """Overlap-save packs frames 2p and 2p + 1 of one channel into one complex transform (csrc/fir_fft.hip), so a NaN input
    reaches every output of the frame PAIRS whose frames read it -- and nothing else: outputs
    s .. s + taps - 1 must be NaN, outputs outside those pairs, other channels and every history must have the clean bits."""
    torch = torch_cuda
    f64 = precision == "f64"
    prec, dt, npdt = (sd.F64, torch.float64, np.float64) if f64 else (sd.F32, torch.float32, np.float32)
    tol = 1e-12 if f64 else 1e-5  # tests/test_gpu_fir_fft.py: TOL
    n = fft_n or sd.fir_fft_size(taps, prec)
    L = n - taps + 1
    channels, samples = 5, 7 * L + 3  # eight frames = four pairs per channel, the last frame partial
    rs = 8 if f64 else 4
    ws = 3 * (2 * n + taps - 1) * rs if sliced else 0  # three frame pairs per slice: slices straddle channels
    h, x, state0 = _fft_fir_input(torch, precision, taps, channels, samples)
    tag = (precision, taps, n, variant, sliced)
    margin = max(8192, 2 * n)

    def make():
        b = sd.fft_fir_filter(taps, channels, prec, fft_n=fft_n, workspace_bytes=ws)
        b.set_coeff(h)
        b.set_variant(variant)
        b._state = state0.clone()
        return b

    bank = make()
    clean = x.clone()
    bank.process(clean)
    torch.cuda.synchronize()
    assert bank.info()["fft_n"] == n and bank.info()["hop"] == L
    if sliced:
        assert bank.launches(samples) > make_default_launches(sd, taps, channels, prec, fft_n, h, variant, samples)
    clean_state = bank.state.clone()
    for c in (0, channels - 1):
        ref, ref_state = _fft_fir_reference(oracle, torch, precision, taps, samples, c)
        err = rel_max_err(clean[c].cpu().numpy(), ref)
        assert err <= tol, (tag, c, err)
        assert np.array_equal(clean_state[c].cpu().numpy().astype(np.float64), ref_state), (tag, c)
    for pad, offset in ((0, 0), (3, 3), (16, 16)):
        def run(view):
            b = make()
            b.process(view, samples=samples, offset=offset)
            torch.cuda.synchronize()
            assert arena.same_bits(b.state, clean_state), (tag, pad, offset, "state differs from the clean result")
        arena.check_framed(torch, x, clean, run, (0,), margin, row_stride=samples + pad, col_offset=offset, what=tag + (pad, offset))
    # one NaN per poisoned channel: first sample, the last sample of an even frame, somewhere inside an odd frame
    where = {0: 0, 2: 2 * L + L - 1, channels - 1: 5 * L + L // 2}
    xp = x.clone()
    for c, s in where.items():
        xp[c, s] = NAN
    b = make()
    b.process(xp)
    torch.cuda.synchronize()
    keep = torch.ones(channels, dtype=torch.bool, device="cuda")
    keep[list(where)] = False
    assert arena.same_bits(xp[keep], clean[keep]), (tag, "clean channels changed")
    xph = x.cpu().numpy().copy()
    for c, s in where.items():
        xph[c, s] = np.nan
        isnan = torch.isnan(xp[c]).cpu().numpy()
        required = _nan_span(samples, s, taps)
        # frame f reads inputs f L - (taps - 1) .. (f + 1) L - 1 and writes outputs f L .. (f + 1) L - 1
        frames = [f for f in range(-(-samples // L)) if f * L - (taps - 1) <= s < (f + 1) * L]
        allowed = np.zeros(samples, bool)
        for p in {f // 2 for f in frames}:
            allowed[2 * p * L:(2 * p + 2) * L] = True
        assert np.all(allowed[required])
        assert np.all(isnan[required]), (tag, c, "an output that depends on the NaN input is finite")
        assert not np.any(isnan & ~allowed), (tag, c, "a NaN outside the frame pairs that read the poisoned input")
        same = torch.from_numpy(~allowed).cuda()
        assert torch.equal(arena.bits(xp[c])[same], arena.bits(clean[c])[same]), (tag, c, "outputs outside the pairs changed")
    assert samples >= taps - 1  # the history is the call's own last taps - 1 inputs
    want_state = torch.from_numpy(np.stack([_fir_state(xph[c], taps) for c in range(channels)])).cuda()
    assert arena.same_bits(b.state, want_state), (tag, "history")


def make_default_launches(sd, taps, channels, prec, fft_n, h, variant, samples):
    b = sd.fft_fir_filter(taps, channels, prec, fft_n=fft_n)
    b.set_coeff(h)
    b.set_variant(variant)
    return b.launches(samples)
