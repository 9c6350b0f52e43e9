"""Every FFT kernel held to unit-roundoff error in extended precision, on a real MI355X.

The checker is tests/fft_exact.py: a DFT in np.clongdouble as the reference, a plain radix-2 transform at the working precision as
the baseline, and three rules in units of u = 2^-24 (f32) / 2^-53 (f64):

  R1  on every row of the row set  e2 <= 3 max(E2_plain(row), 1 u)  and  einf <= 3 max(Einf_plain(row), 1 u)
  R2  N <= 1024: batch = N, input = the identity; every element of the DFT matrix within 3 max(Einf_plain(batch), 4/3 u)
  R3  the impulse at 0, the all-ones row and the alternating row come out exactly

One explicit table, (n, radix, precision, variant, form) -> kernel name, taken from select_kernel / select_conv (csrc/capi.hip) and
the variant lists of tests/test_gpu_fft.py; every case asserts the kernel the plan reports before it runs anything, and the last test
holds the table against the list of names written out below.  Plans, variants and workspaces are the ones the suite already runs;
only the inputs and the checker are new.  Batches are the row set (13 to 15 rows, 10 from 2^19 on) plus one row where that makes the
count odd: an odd batch is ragged against every power-of-two tile.

Two defects found by these rules are fixed with them: the double W_64 constants of the radix-4 layers
(csrc/fft32_r4.h, up to 5.5 u off) and the double plans' thread-twiddle tables (built from a row whose angles were formed in double,
up to 1.85 u off).  Two counted exceptions (R4) stand next to their counts below: the plain-sum column kernel in double
(EXCEPTIONS) and the in-phase rows of three kernels (INPHASE).
"""
import numpy as np
import pytest

import fft_exact as fx

pytestmark = pytest.mark.gpu

REG, REG64 = "sdsp_fft_reg_kernel", "sdsp_fft_reg_f64_kernel"
WAVE, WAVE1024 = "sdsp_fft_wave_f32", "sdsp_fft1024_wave"
R4_4096, R2_4096, CONV_4096 = "sdsp_fft4096_r4_f32", "sdsp_fft4096_r2_f32", "sdsp_fft4096_conv_f32"
MIX, BIG, BIG64, BIG64_REAL = "sdsp_fft_mix_f32", "sdsp_fft_big_kernel", "sdsp_fft_big_f64_kernel", "sdsp_fft_big_f64_real_kernel"
TILE = "sdsp_fft_tile_kernel"
TWO_PASS, TWO_PASS_FUSED = "sdsp_fft2p_cols+sdsp_fft2p_rows", "sdsp_fft2p_fused"
FFT1M, FFT1M_FUSED = "sdsp_fft1m_cols+sdsp_fft1m_rows", "sdsp_fft1m_fused"
MID = "sdsp_fft_col16_kernel+rows+sdsp_fft_untwist16"

# every name select_kernel / select_conv can return for a plan that runs ("none" is the no-op of n = 1 and the unsupported case),
# with the precisions it exists in
ALL_KERNELS = {
    REG: {"f32"}, REG64: {"f64"}, WAVE: {"f32"}, WAVE1024: {"f32", "f64"}, R4_4096: {"f32"}, R2_4096: {"f32"}, CONV_4096: {"f32"},
    MIX: {"f32"}, BIG: {"f32"}, BIG64: {"f64"}, BIG64_REAL: {"f64"}, TILE: {"f32", "f64"}, TWO_PASS: {"f32", "f64"},
    TWO_PASS_FUSED: {"f32", "f64"}, FFT1M: {"f32"}, FFT1M_FUSED: {"f32"}, MID: {"f32", "f64"},
}

RING = "ring"  # max_batch of a plan whose workspace holds the persistent two-pass schedule's ring: 256 MiB of intermediates


def _ring(n, prec):
    return max(16, (1 << 28) // (n * (16 if prec == "f64" else 8)))  # as tests/test_gpu_fft.py: _two_pass_variants


# ---- complex plans: (n, radix, precision, variant, max_batch or None = the batch, kernel)
COMPLEX_CASES = [
    # f32 register-pass family: streaming and default cache policy; its sizes' one-wave kernels (variant 2)
    (16, 2, "f32", 0, None, REG), (16, 2, "f32", 1, None, REG), (64, 4, "f32", 0, None, REG), (64, 4, "f32", 1, None, REG),
    (512, 2, "f32", 0, None, REG), (512, 2, "f32", 1, None, REG), (2048, 2, "f32", 0, None, REG), (2048, 2, "f32", 1, None, REG),
    (256, 2, "f32", 0, None, REG), (256, 2, "f32", 2, None, WAVE), (256, 4, "f32", 2, None, WAVE),
    (1024, 2, "f32", 0, None, REG), (1024, 2, "f32", 2, None, WAVE1024), (1024, 4, "f32", 0, None, REG), (1024, 4, "f32", 2, None, WAVE1024),
    (2048, 2, "f32", 2, None, WAVE),
    # the tuned N = 4096 kernels; the coverage kernel in one pass (variant 99)
    (4096, 4, "f32", 0, None, R4_4096), (4096, 2, "f32", 0, None, R2_4096), (4096, 4, "f32", 99, None, TILE), (512, 2, "f32", 99, None, TILE),
    # registers-resident kernel (radix-2 stages, and the radix-4 form of (16384, 4)) and the mixed-radix kernel
    (8192, 0, "f32", 0, None, BIG), (8192, 0, "f32", 1, None, MIX), (8192, 2, "f32", 0, None, BIG),
    (16384, 2, "f32", 0, None, BIG), (16384, 4, "f32", 0, None, BIG), (16384, 4, "f32", 1, None, MIX), (32768, 2, "f32", 0, None, BIG),
    # two passes: the persistent launch, the two launches per chunk (variant 3), the three streaming passes (variant 1), the general
    # four-step through the coverage kernel (variant 2; variant 8 of a radix-4 plan: radix-4 stages)
    (1 << 16, 2, "f32", 0, RING, TWO_PASS_FUSED), (1 << 16, 2, "f32", 3, RING, TWO_PASS), (1 << 16, 2, "f32", 1, 2, MID),
    (1 << 16, 2, "f32", 2, 2, TILE), (1 << 16, 4, "f32", 8, 32, TILE),
    (1 << 19, 2, "f32", 0, RING, TWO_PASS_FUSED), (1 << 19, 2, "f32", 3, RING, TWO_PASS), (1 << 19, 2, "f32", 1, 2, MID),
    # N = 2^20: the persistent kernel, its chunked schedule, the generic persistent kernel; 2^21 and 2^22
    (1 << 20, 2, "f32", 0, 37, FFT1M_FUSED), (1 << 20, 2, "f32", 1, 37, FFT1M), (1 << 20, 2, "f32", 2, 37, TWO_PASS_FUSED),
    (1 << 21, 2, "f32", 0, 2, TWO_PASS), (1 << 22, 2, "f32", 0, 2, TWO_PASS),
    # double: register-pass family and its one-wave variant; registers-resident kernel with what served the size before (variant 1)
    (64, 4, "f64", 0, None, REG64), (1024, 2, "f64", 0, None, REG64), (1024, 2, "f64", 1, None, WAVE1024),
    (4096, 2, "f64", 0, None, BIG64), (4096, 2, "f64", 1, None, REG64), (4096, 4, "f64", 0, None, BIG64), (4096, 4, "f64", 1, None, REG64),
    (8192, 2, "f64", 0, None, BIG64), (8192, 2, "f64", 1, None, REG64),
    (16384, 2, "f64", 0, None, BIG64), (16384, 2, "f64", 1, 2, MID), (16384, 4, "f64", 0, None, BIG64), (16384, 4, "f64", 1, 2, MID),
    # double, two passes: persistent and two-launch; the three-pass variant; the four-step through the coverage kernel
    (1 << 15, 2, "f64", 0, RING, TWO_PASS_FUSED), (1 << 15, 2, "f64", 3, RING, TWO_PASS), (1 << 15, 2, "f64", 1, 2, MID),
    (1 << 15, 2, "f64", 2, 2, TILE),
    (1 << 16, 2, "f64", 0, RING, TWO_PASS_FUSED), (1 << 16, 2, "f64", 3, RING, TWO_PASS), (1 << 16, 2, "f64", 1, 2, MID),
    (1 << 20, 2, "f64", 0, RING, TWO_PASS_FUSED), (1 << 20, 2, "f64", 3, RING, TWO_PASS),
]

# ---- real-input plans: (n_real, radix, precision, variant, kernel); variant 1 where it selects another kernel
REAL_CASES = [
    (32, 2, "f32", 0, REG), (512, 2, "f32", 0, REG), (1024, 2, "f32", 0, WAVE), (1024, 2, "f32", 1, REG), (2048, 2, "f32", 0, REG),
    (8192, 2, "f32", 0, BIG), (8192, 2, "f32", 1, REG), (32768, 2, "f32", 0, BIG), (32768, 2, "f32", 1, REG), (65536, 2, "f32", 0, BIG),
    (32, 2, "f64", 0, REG64), (2048, 2, "f64", 0, REG64), (8192, 2, "f64", 0, BIG64_REAL), (8192, 2, "f64", 1, REG64),
    (32768, 2, "f64", 0, BIG64_REAL),
]

# ---- fused convolution: (n, radix, precision, variant, the plan's transform kernel, the kernel select_conv runs)
CONV_CASES = [
    (256, 2, "f32", 0, REG, WAVE), (1024, 2, "f32", 0, REG, WAVE1024), (1024, 2, "f32", 2, WAVE1024, REG), (2048, 2, "f32", 0, REG, BIG),
    (4096, 4, "f32", 0, R4_4096, CONV_4096), (16384, 2, "f32", 0, BIG, BIG),
    (1024, 2, "f64", 0, REG64, REG64), (4096, 2, "f64", 0, BIG64, BIG64),
    (1 << 16, 2, "f32", 0, TWO_PASS, TWO_PASS),  # three launches: forward (the multiply rides on its pass 2), reverse
]

# ---- column plans: n, both variants, both precisions at width 17
COLS_NS = (8, 32, 64, 1024)
COLS_WIDTH = 17

# R3 / R4 exceptions: (form, kernel, precision) -> (n -> margin over the baseline, bound in u on the R3 rows or None = exact, reason).
# Every other kernel is held to the common rules.
EXCEPTIONS = {
    # sdsp_fft_cols_plain_kernel is the plain sum X[k] = sum_p v[p] W^(p k), accumulated in double: the cross-check of the column plans,
    # not a butterfly network.  In double its running sum is rounded once per term, n times, where the baseline's path to an output
    # is rounded once per stage, log2 n times; errors of independent roundings add in squares, so the counted figure is
    # sqrt(n / log2 n) times the baseline (1.6 at n = 8, 10.1 at n = 1024) under the common factor 3.  R3: the all-ones and the
    # alternating row ask it for sum_p W^(p k) = 0 from n table values, each rounded to double, through that running sum -- the
    # rounding step is the table's and the accumulator's; held to 1 u of the peak n on those rows.  (In f32 the double accumulator
    # is rounded once at the end: the common rules hold there.)
    ("cols", "sdsp_fft_cols_plain_kernel", "f64"): (lambda n: fx.MARGIN * (n / (n.bit_length() - 1)) ** 0.5, 1.0,
                                                    "plain sum: n roundings of the running sum against log2 n"),
}


# R4, the in-phase rows of three kernels.  A tone's peak and the impulse a convolution gives back are sums of N terms in phase:
# rounding errors that differ from term to term average out, a unit factor that every term meets does not -- its modulus error goes
# into the peak in full.  These kernels multiply in every stage by a compile-time constant W_32^e (W_16^e in the register-pass
# family) and by a table value, where the plain transform multiplies by one table value; rounded to f32 ALL fifteen constants have
# a modulus below 1 (by 0.13 to 0.48 u: fx.const_modulus_error), so their errors add up along a path instead of cancelling: the
# bin N - 1 of the 2^16 two-pass transform meets W_32^15, W_32^14, W_32^12 and W_32^12 in each pass, 2 (0.48 + 0.48 + 0.29 + 0.29)
# = 3.08 u below 1 from the constants alone, which is the 4.00 u measured there (a result just under 1 steps by 1 u).  A numpy model
# of the scheme (constant x table value per stage, correctly rounded tables, no fused multiply-add) gives the f64 convolution's
# 4.00 u exactly.  The counted term, added to the einf bound of those rows only, one constant per stage that can carry one (the
# last two stages of a register pass have 1 and -+i) at the largest modulus error of the table of constants:
#   a transform's sum into one bin       constant_stages x const_modulus_error              (table values vary with the term)
#   forward transform of an impulse      (constant_stages x const_modulus_error + stages x u / sqrt 2) / 2
#                                        (one position: constant and table value of every stage are fixed; half the bins meet them)
# (form, kernel, precision) -> (n -> register passes of one transform, row kinds, which of the two counts apply)
def _two_pass_passes(n):  # csrc/fft_2pass.hip: N = N1 x N2, a factor of 32 T points = five stages + log2 T stages
    bits = n.bit_length() - 1
    out = []
    for f in ((bits + 1) // 2, bits // 2):
        out += [5, f - 5] if f <= 10 else [f]
    return out


def _big_passes(n):  # csrc/fft_big.hip: passes A and B of five stages, pass C the rest
    bits = n.bit_length() - 1
    return [5] * (bits // 5) + ([bits % 5] if bits % 5 else [])


def _reg64_passes(n):  # csrc/fft_reg64.hip: P = ceil(log2 N / 4) passes of four stages, the last one the rest
    bits = n.bit_length() - 1
    p = (bits + 3) // 4
    return [4] * (p - 1) + [bits - 4 * (p - 1)]


INPHASE = {
    # reverse tone at bin 1 of N = 2^16: 8 constant stages x 0.48 u = 3.87 u (measured 4.00 u against 3.00 u without the term)
    ("complex", TWO_PASS, "f32"): (_two_pass_passes, ("tone",)),
    ("complex", TWO_PASS_FUSED, "f32"): (_two_pass_passes, ("tone",)),
    # convolution = forward transform of the impulse + the reverse transform's sum into one bin.  N = 16384 f32: (8 x 0.48 + 14 x 0.71)
    # / 2 + 8 x 0.48 = 10.7 u (measured 3.98 against 3.00); N = 1024 f64: (4 x 0.62 + 10 x 0.71) / 2 + 4 x 0.62 = 7.3 u (4.02 against
    # 3.00); N = 2^16 f32: (8 x 0.48 + 16 x 0.71) / 2 + 8 x 0.48 = 11.4 u (4.08 / 6.02 / 4.00 against 3.08 / 6.00 / 3.00).  Worst case:
    # every factor's error at its largest and of one sign
    ("conv", BIG, "f32"): (_big_passes, ("impulse",)),
    ("conv", REG64, "f64"): (_reg64_passes, ("impulse",)),
    ("conv", TWO_PASS, "f32"): (_two_pass_passes, ("impulse",)),
}


def _inphase(form, kernel, prec, n):
    if (form, kernel, prec) not in INPHASE:
        return None
    passes, kinds = INPHASE[(form, kernel, prec)]
    u = fx.inphase_transform(passes(n), prec)
    if form == "conv":
        u += fx.inphase_impulse_forward(passes(n), prec)
    return {k: u for k in kinds}


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


def _id(case):
    return "-".join(str(c) for c in case)


def _prec(sd, prec):
    return sd.F64 if prec == "f64" else sd.F32


def _ragged(x):
    """the rows plus a copy of the first one where the count is even: an odd batch is ragged against every power-of-two tile"""
    return x if len(x) % 2 else np.concatenate([x, x[:1]])


def _margins(form, kernel, prec, n):
    margin, exact_u, _ = EXCEPTIONS.get((form, kernel, prec), (lambda n: fx.MARGIN, None, ""))
    return margin(n), exact_u


def _summary(tag, report):
    worst = fx.worst_by_kind(report)
    print(f"{tag}: " + "; ".join(f"{k} e2 {v['e2']:.2f} (plain {v['base2']:.2f}) einf {v['einf']:.2f} (plain {v['baseinf']:.2f}) "
                                 f"ratio {v['ratio']:.2f}" for k, v in worst.items()))
    return worst


def run_complex(sd, torch, case, reverse):
    """(failures, report) of one row of COMPLEX_CASES in one direction; asserts the kernel first"""
    n, radix, prec, variant, max_batch, kernel = case
    acc = fx.get_case(n, prec, reverse)
    x = _ragged(acc.rows.x)
    batch = max(len(x), n if n <= 1024 else 0)
    mb = _ring(n, prec) if max_batch == RING else (max_batch or batch)
    plan = sd.FftPlan(n, radix, sd.reverse_fft if reverse else sd.forward_fft, _prec(sd, prec), max_batch=mb)
    plan.set_variant(variant)
    assert plan.info.kernel.decode() == kernel, (case, plan.info.kernel.decode())
    d = torch.from_numpy(x).cuda()
    plan.exec(d)
    plan.status()
    got = d.cpu().numpy()
    assert np.array_equal(got[len(acc.rows):].view(fx.RDT[prec]), got[:len(x) - len(acc.rows)].view(fx.RDT[prec]))  # the copy's bits
    margin, exact_u = _margins("complex", kernel, prec, n)
    fails, report = fx.check_case(acc, got, margin, exact_u, _inphase("complex", kernel, prec, n))
    if n <= 1024:  # R2: the whole DFT matrix, every twiddle path to every bin, every position of a ragged last tile
        d = torch.from_numpy(np.eye(n, dtype=fx.CDT[prec])).cuda()
        plan.exec(d)
        plan.status()
        f2, r2 = fx.check_matrix(d.cpu().numpy(), n, prec, reverse, margin)
        fails, report = fails + f2, report + [r2]
    plan.close()
    return fails, report


def run_real(sd, torch, case, reverse):
    n_real, radix, prec, variant, kernel = case
    acc = fx.get_real_case(n_real, prec, reverse)
    x = _ragged(acc.x)
    plan = sd.RfftPlan(n_real, radix, sd.reverse_fft if reverse else sd.forward_fft, max_batch=len(x), precision=_prec(sd, prec))
    plan.set_variant(variant)
    assert plan.info.kernel.decode() == kernel, (case, plan.info.kernel.decode())
    if reverse:  # the packed spectrum viewed as n_real reals
        d = torch.view_as_real(torch.from_numpy(x).cuda()).reshape(len(x), n_real).contiguous()
    else:
        d = torch.from_numpy(x).cuda()
    got = plan.exec(d)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    plan.close()
    margin, exact_u = _margins("real", kernel, prec, n_real)
    return acc.check(got, margin, exact_u)


def run_conv(sd, torch, case):
    n, radix, prec, variant, kernel, _conv_kernel = case
    acc = fx.get_conv_case(n, prec)
    x = _ragged(acc.rows.x)
    plan = sd.FftPlan(n, radix, sd.forward_fft, _prec(sd, prec), max_batch=len(x))
    plan.set_variant(variant)
    assert plan.info.kernel.decode() == kernel, (case, plan.info.kernel.decode())
    fails, report = [], []
    margin, _ = _margins("conv", _conv_kernel, prec, n)
    for kind in acc.H_KINDS:
        d, h = torch.from_numpy(x).cuda(), torch.from_numpy(acc.h[kind]).cuda()
        plan.convolve(d, h)
        plan.status()
        f, r = acc.check(kind, d.cpu().numpy(), margin, _inphase("conv", _conv_kernel, prec, n))
        fails += [(rule, f"h={kind}/{k}", label, text) for rule, k, label, text in f]
        report += [dict(row, kind=f"h={kind}") for row in r]
    plan.close()
    return fails, report


def run_cols(sd, torch, n, prec, variant, reverse):
    acc = fx.get_case(n, prec, reverse)
    rows = acc.rows
    assert len(rows) <= COLS_WIDTH
    plan = sd.FftColsPlan(n, COLS_WIDTH, sd.reverse_fft if reverse else sd.forward_fft, _prec(sd, prec))
    plan.set_variant(variant)
    kernel = plan.info()["kernel"]
    assert kernel == ("sdsp_fft_cols_plain_kernel" if variant else "sdsp_fft_cols_kernel")
    cube = np.zeros((1, n, COLS_WIDTH), dtype=fx.CDT[prec])  # row i of the set down column i; the other columns stay zero
    cube[0, :, :len(rows)] = rows.x.T
    got = plan.exec(torch.from_numpy(cube).cuda()).cpu().numpy()
    assert not got[0, :, len(rows):].any()
    margin, exact_u = _margins("cols", kernel, prec, n)
    fails, report = fx.check_case(acc, np.ascontiguousarray(got[0, :, :len(rows)].T), margin, exact_u)
    # R2: the identity, 17 columns a cube
    cubes = -(-n // COLS_WIDTH)
    eye = np.zeros((cubes * COLS_WIDTH, n), dtype=fx.CDT[prec])
    eye[:n] = np.eye(n, dtype=fx.CDT[prec])
    x = np.ascontiguousarray(eye.reshape(cubes, COLS_WIDTH, n).transpose(0, 2, 1))
    out = plan.exec(torch.from_numpy(x).cuda()).cpu().numpy().transpose(0, 2, 1).reshape(cubes * COLS_WIDTH, n)
    f2, r2 = fx.check_matrix(out[:n], n, prec, reverse, margin)
    plan.close()
    return fails + f2, report + [r2]


def _show(fails):
    return "\n".join(" ".join(str(v) for v in f) for f in fails)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("case", COMPLEX_CASES, ids=_id)
def test_complex_plans(sd, torch_cuda, case, reverse):
    fails, report = run_complex(sd, torch_cuda, case, reverse)
    _summary(f"complex {_id(case)} reverse={reverse}", report)
    assert not fails, _show(fails)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("case", REAL_CASES, ids=_id)
def test_real_input_plans(sd, torch_cuda, case, reverse):
    fails, report = run_real(sd, torch_cuda, case, reverse)
    _summary(f"real {_id(case)} reverse={reverse}", report)
    assert not fails, _show(fails)


@pytest.mark.parametrize("case", CONV_CASES, ids=_id)
def test_fused_convolution(sd, torch_cuda, case):
    fails, report = run_conv(sd, torch_cuda, case)
    _summary(f"conv {_id(case)}", report)
    assert not fails, _show(fails)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n", COLS_NS)
def test_column_plans(sd, torch_cuda, n, precision, variant, reverse):
    fails, report = run_cols(sd, torch_cuda, n, precision, variant, reverse)
    _summary(f"cols {n}-{precision}-{variant} reverse={reverse}", report)
    assert not fails, _show(fails)


def test_the_table_reaches_every_kernel_name():
    """every name select_kernel / select_conv can return, at both precisions where it exists (no GPU call: the cases above assert
    the names against the plans)"""
    hit = {}
    for n, radix, prec, variant, mb, kernel in COMPLEX_CASES:
        hit.setdefault(kernel, set()).add(prec)
    for n, radix, prec, variant, kernel in REAL_CASES:
        hit.setdefault(kernel, set()).add(prec)
    for n, radix, prec, variant, kernel, conv in CONV_CASES:
        hit.setdefault(conv, set()).add(prec)
    assert hit == ALL_KERNELS, {k: (hit.get(k), v) for k, v in ALL_KERNELS.items() if hit.get(k) != v}
    # the fused convolutions: one case per kernel select_conv runs in one launch
    assert {c[5] for c in CONV_CASES} >= {WAVE, WAVE1024, REG, BIG, CONV_4096, REG64, BIG64}
