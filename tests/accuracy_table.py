#!/usr/bin/env python3
"""(Test infrastructure: uses the oracle, hence it lives under tests/.)  Measured parity margins: normwise error max|got-ref|/max|ref| (SURVEY 8d metric) of every f32 kernel against
the double-precision oracle on seeded random input, next to the 1e-6 bound the tests enforce."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
import simpledsp_amd as sd
from oracle import Oracle

o = Oracle()
rng = np.random.default_rng(2024)


# ---- the transform family in units of u against the extended-precision reference (tests/fft_exact.py): per case
# of tests/test_gpu_fft_accuracy.py's table and per row kind the worst e2 / einf next to the plain baseline's and the bound
import fft_exact as fx
import test_gpu_fft_accuracy as acc


def units_of_u_section():
    print("\n## Transform kernels in units of u (2^-24 f32, 2^-53 f64) against the longdouble DFT\n")
    print("Per row kind: worst e2 / einf (plain baseline's e2 / einf; bound e2 / einf); `ratio` = the case's worst error over max(baseline, 1 u), bound 3.\n")
    print("| form | case | kernel | direction | " + " | ".join(("gauss", "impulse", "tone", "exact rows", "matrix")) + " | ratio |\n|---|---|---|---|---|---|---|---|---|---|")

    def _cells(report):
        w = fx.worst_by_kind(report)
        for k in ("ones", "alt"):  # the R3 rows in one column
            if k in w:
                e = w.setdefault("exact", dict(e2=0.0, einf=0.0, base2=0.0, baseinf=0.0, bound2=0.0, boundinf=0.0, ratio=0.0))
                for f in e:
                    e[f] = max(e[f], w[k][f])
        cells = []
        for k in ("gauss", "impulse", "tone", "exact", "matrix"):
            v = w.get(k)
            cells.append("-" if v is None else f"{v['einf']:.2f} ({v['baseinf']:.2f}; {v['boundinf']:.2f})" if k == "matrix" else
                         f"{v['e2']:.2f} / {v['einf']:.2f} ({v['base2']:.2f} / {v['baseinf']:.2f}; {v['bound2']:.2f} / {v['boundinf']:.2f})")
        return cells, max(v["ratio"] for v in w.values())

    def _row(form, case, kernel, direction, report, fails):
        cells, ratio = _cells(report)
        print(f"| {form} | {case} | `{kernel}` | {direction} | " + " | ".join(cells) + f" | {ratio:.2f}{' **over**' if fails else ''} |")

    for case in acc.COMPLEX_CASES:
        for reverse in (False, True):
            fails, report = acc.run_complex(sd, torch, case, reverse)
            _row("complex", f"N = {case[0]}, radix {case[1]}, {case[2]}, variant {case[3]}", case[5], "rev" if reverse else "fwd", report, fails)
    for case in acc.REAL_CASES:
        for reverse in (False, True):
            fails, report = acc.run_real(sd, torch, case, reverse)
            _row("real", f"n_real = {case[0]}, radix {case[1]}, {case[2]}, variant {case[3]}", case[4], "rev" if reverse else "fwd", report, fails)
    for case in acc.CONV_CASES:
        fails, report = acc.run_conv(sd, torch, case)
        by_h = {}
        for r in report:
            by_h.setdefault(r["kind"], []).append(r)
        for h, rows in by_h.items():
            w = fx.worst_by_kind(rows)[h]
            print(f"| conv | N = {case[0]}, radix {case[1]}, {case[2]}, variant {case[3]}, {h} | `{case[5]}` | - | all rows: {w['e2']:.2f} / {w['einf']:.2f} "
                  f"({w['base2']:.2f} / {w['baseinf']:.2f}; {w['bound2']:.2f} / {w['boundinf']:.2f}) | - | - | - | - | "
                  f"{w['ratio']:.2f}{' **over**' if any(f[1].startswith(h) for f in fails) else ''} |")
    for n in acc.COLS_NS:
        for prec in ("f32", "f64"):
            for variant in (0, 1):
                for reverse in (False, True):
                    fails, report = acc.run_cols(sd, torch, n, prec, variant, reverse)
                    _row("cols", f"n = {n}, width {acc.COLS_WIDTH}, {prec}, variant {variant}", "sdsp_fft_cols_plain_kernel" if variant else "sdsp_fft_cols_kernel",
                         "rev" if reverse else "fwd", report, fails)


if "--units-of-u" in sys.argv:  # that section alone (profiles/fft_accuracy_u.md)
    units_of_u_section()
    sys.exit(0)


# ---- the time-domain kernels against their bit-level models and in units of u (tests/recur_exact.py): per case of
# tests/test_gpu_biquad_exact.py's and tests/test_gpu_fir_exact.py's tables the worst channel's e2 / einf for kernel, model and plain baseline
import recur_exact as rx
import test_gpu_biquad_exact as bq
import test_gpu_fir_exact as fq


def recur_section():
    kinds = {0: "GENERIC", 1: "LP", 2: "HP", 3: "BP"}

    def _row(family, case, kernel, got, ref, prec, differing):
        _, k = rx.r2(got, ref["plain"], ref["ld"], prec)
        _, mo = rx.r2(ref["y"], ref["plain"], ref["ld"], prec)
        print(f"| {family} | {case} | `{kernel}` | {k['e2']:.2f} / {k['einf']:.2f} | {mo['e2']:.2f} / {mo['einf']:.2f} | {k['base2']:.2f} / {k['baseinf']:.2f} | "
              f"{k['ratio']:.2f}{' **over**' if k['ratio'] > rx.MARGIN else ''} | {differing} |")

    print("\n## Biquad and FIR banks against their models, in units of u (2^-24 f32 and mixed mode, 2^-53 f64) against the longdouble recurrence\n")
    print("Worst channel's e2 / einf of the kernel (variant 0, one call), of the model and of the plain unfused baseline; `ratio` = the larger of the worst "
          "per-channel e2 over max(baseline, 1 u) and the case's einf over max(baseline einf, 1 u), bound 3; `bits` = elements of output and final state "
          "that differ from the model (R1: 0).\n")
    print("| family | case | kernel | kernel e2 / einf | model e2 / einf | plain e2 / einf | ratio | bits |\n|---|---|---|---|---|---|---|---|")
    for case in bq.CASES:
        precision, kind, m, name, shape = case
        ref, got, _, state, names = bq.run_channel_major(sd, torch, case, 0, False)
        diff = rx.bit_diff(got, ref["y"])[0] + rx.bit_diff(state, ref["final"])[0]
        c, n = bq.SHAPES[shape][:2]
        _row("biquad", f"{precision}, {kinds[kind]}, {m} sections, {name}, {c} x {n}", names[0], got, ref, precision, diff)
    for case in fq.CASES:
        got, hist = fq.run(sd, torch, case, "f32", 0, False)
        ref = fq.reference(case, "f32")
        diff = rx.bit_diff(got, ref["y"], True)[0] + rx.bit_diff(hist, ref["final"])[0]
        _row("FIR", f"f32, {case[0]} taps, {case[1]} x {case[2]}", "sdsp_fir_kernel", got, ref, "f32", diff)


if "--recur" in sys.argv:  # that section alone (profiles/recur_accuracy.md)
    recur_section()
    sys.exit(0)


def rel(got, ref):
    got = np.asarray(got, dtype=np.complex128 if np.iscomplexobj(ref) else np.float64)
    return float((np.abs(got - ref).max(axis=-1) / np.abs(ref).max(axis=-1)).max())


print("| kernel | case | max normwise error | bound |\n|---|---|---|---|")
for n in (16, 64, 256, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 1 << 20, 1 << 21, 1 << 22):
    for radix in (2, 4, 0):
        if radix == 4 and not sd.isPowerOf4(n):
            continue
        if radix == 0 and n != 8192:
            continue  # AUTO: only at 8192 a kernel of its own (mixed radix)
        batch = max(2, min(64, (1 << 16) // n))
        x = (rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))).astype(np.complex64)
        errs = []
        for T, rev in ((sd.forward_fft, False), (sd.reverse_fft, True)):
            # two-pass sizes: a workspace large enough for their default schedule, the persistent launch (a 256 MiB ring of intermediates)
            plan = sd.FftPlan(n, radix, T, sd.F32, max_batch=max(batch, (1 << 28) // (8 * n)))
            d = torch.from_numpy(x).cuda()
            plan.exec(d)
            torch.cuda.synchronize()
            x128 = x.astype(np.complex128)
            ref = o.fft(x128, radix or 2, rev) if n <= (1 << 20) else (np.fft.ifft(x128, axis=-1) if rev else np.fft.fft(x128, axis=-1))
            errs.append(rel(d.cpu().numpy(), ref))
        print(f"| `{plan.info.kernel.decode()}` | N = {n}, radix {radix}, fwd / rev | {errs[0]:.2e} / {errs[1]:.2e} | 1e-6 |")

# double precision (round 3): against the oracle in units of the reference's own bound 4 N eps (testFFT.cpp:37)
for n in (64, 1024, 4096, 8192, 16384, 1 << 15, 1 << 16, 1 << 18, 1 << 20):
    for radix in (2, 4):
        if radix == 4 and not sd.isPowerOf4(n):
            continue
        batch = max(2, min(16, (1 << 16) // n))
        x = rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))
        errs = []
        for T, rev in ((sd.forward_fft, False), (sd.reverse_fft, True)):
            plan = sd.FftPlan(n, radix, T, sd.F64, max_batch=max(batch, (1 << 28) // (16 * n)))
            d = torch.from_numpy(x).cuda()
            plan.exec(d)
            torch.cuda.synchronize()
            errs.append(rel(d.cpu().numpy(), o.fft(x, radix, rev)))
        tol = 4 * n * np.finfo(np.float64).eps
        print(f"| `{plan.info.kernel.decode()}` (f64) | N = {n}, radix {radix}, fwd / rev | {errs[0]:.2e} / {errs[1]:.2e} (= {errs[0] / tol:.3f} / {errs[1] / tol:.3f} of the bound) | 4 N eps = {tol:.1e} |")

# cascaded biquads, BASELINE config-4 filter, f32
x = rng.standard_normal((64, 4096)).astype(np.float32)
bank = sd.casc_2o_iir(4, 64, sd.F32, sd.IIR_GENERIC)
bank.set_lp_coeff(10e3, 100e3)
d = torch.from_numpy(x).cuda()
bank.process(d)
torch.cuda.synchronize()
fo = o.iir(4)
want = []
for c in range(64):
    f = o.iir(4)
    f.set_lp_coeff(10e3, 100e3)
    want.append(f.process(x[c].astype(np.float64)))
print(f"| `{bank.kernel_name(d)}` | 4-section LP, 4096 samples, f32 | {rel(d.cpu().numpy(), np.array(want)):.2e} | 1e-6 (f64: bit-exact) |")

# the same filter and a low cutoff (f0/fs = 0.005) in pure f32 and in the mixed mode (float samples, double recurrence)
for f0 in (10e3, 500.0):
    for prec, name in ((sd.F32, "f32"), (sd.F32_F64STATE, "float samples + double recurrence")):
        bank = sd.casc_2o_iir(4, 64, prec, sd.IIR_GENERIC)
        bank.set_lp_coeff(f0, 100e3)
        d = torch.from_numpy(x).cuda()
        bank.process(d)
        torch.cuda.synchronize()
        want = []
        for c in range(64):
            f = o.iir(4)
            f.set_lp_coeff(f0, 100e3)
            want.append(f.process(x[c].astype(np.float64)))
        print(f"| `{bank.kernel_name(d)}` | 4-section LP f0/fs = {f0 / 100e3:g}, 4096 samples, {name} | {rel(d.cpu().numpy(), np.array(want)):.2e} | "
              f"{'1e-6 (BASELINE filter only)' if prec == sd.F32 else '1.2e-7'} |")

# FIR, f32
for taps in (16, 32, 64):
    fb = sd.fir_filter(taps, 64, sd.F32)
    fb.set_lp_coeff(10e3, 100e3)
    d = torch.from_numpy(x).cuda()
    fb.process(d)
    torch.cuda.synchronize()
    h32 = fb.m_coeff.astype(np.float32).astype(np.float64)
    want = np.array([o.fir_process(h32, x[c].astype(np.float64))[0] for c in range(64)])
    print(f"| `sdsp_fir_kernel` | {taps}-tap LP, 4096 samples, f32 | {rel(d.cpu().numpy(), want):.2e} | 1e-6 (f64: bit-exact) |")

# fused convolution
for n, radix in ((4096, 4), (1024, 2)):
    xb = (rng.standard_normal((8, n)) + 1j * rng.standard_normal((8, n))).astype(np.complex64)
    hh = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    plan = sd.FftPlan(n, radix, sd.forward_fft, sd.F32, max_batch=8)
    d = torch.from_numpy(xb).cuda()
    plan.convolve(d, torch.from_numpy(hh).cuda())
    torch.cuda.synchronize()
    ref = o.fft(o.fft(xb.astype(np.complex128), radix) * hh.astype(np.complex128), radix, True)
    print(f"| fused convolution | N = {n}, radix {radix} | {rel(d.cpu().numpy(), ref):.2e} | 2e-6 (two transforms) |")

units_of_u_section()
recur_section()
