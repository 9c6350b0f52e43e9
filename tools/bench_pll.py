#!/usr/bin/env python3
"""Carrier-recovery PLL / Costas loop bank against what a user has without it, in one process, alternating:
(a) variant 1, the plain one-thread-per-channel kernel with tables and state in global memory.  It is slow, so it runs on the first
    `--plain-samples` samples of at most `--plain-channels` channels and its time is scaled to the whole shape;
(b) the per-sample loop in torch (table gather, two complex products, detector, loop filter, phase advance: about twenty launches per
    sample; double-precision angle instead of the tables) on the first `--torch-samples` samples, scaled to the whole row;
(c) ddc_bank with T = 1, D = 1 and one band per channel at the same frequency, on at most 65536 channels (its band limit), scaled:
    what the open-loop mix costs, that is, the price of feedback.
Shapes: f32 and f64 on `--channels` x 4032 samples and the underfilled 4096 x 2^16; every mode, with all outputs and with y only.
Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min).

Model bytes per sample: x in and y out (16 B in f32, 32 B in f64), plus one real (4 B / 8 B) per real output row, as a share of 8 TB/s.
A line where variant 0 is slower than a baseline is marked LOSES.

  python tools/bench_pll.py [--channels 262144,65536] [--precisions f32,f64] [--modes cross,bpsk,qpsk] [--no-under]
                            [--warmup 2] [--steps 5] [--repeats 3] [--out profiles/pll_bench.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK_BYTES = 8e12
F0, BN = 0.1, 0.01


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def rounds(a, fns):
    """median and spread of every function over alternating rounds"""
    t = [[] for _ in fns]
    for _ in range(a.repeats):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, a.warmup, a.steps))
    return [(statistics.median(v), max(v) / min(v)) for v in t]


def torch_form(x, fcw, alpha, beta, mode, ns):
    """baseline (b): the recursion sample by sample on whole-bank tensors, over the first ns samples"""
    C = x.shape[0]
    rt = torch.float64 if x.dtype == torch.complex128 else torch.float32
    y = torch.empty((C, ns), device=x.device, dtype=x.dtype)
    theta = torch.zeros(C, device=x.device, dtype=torch.int64)
    integ = torch.zeros(C, device=x.device, dtype=rt)
    step = torch.full((C,), int(fcw), device=x.device, dtype=torch.int64)

    def fn():
        theta.zero_()
        integ.zero_()
        for n in range(ns):
            ang = (theta >> 10).to(torch.float64) * (-2 * np.pi / 2 ** 22)
            w = torch.polar(torch.ones_like(ang), ang).to(x.dtype)
            v = x[:, n] * w
            y[:, n] = v
            if mode == "cross":
                e = v.imag
            elif mode == "bpsk":
                e = v.real * v.imag
            else:
                e = torch.sign(v.real) * v.imag - torch.sign(v.imag) * v.real
            integ.add_(beta * e).clamp_(-0.5, 0.5)
            k = ((alpha * e + integ) * 2.0 ** 32).clamp_(-2.0 ** 31, 2.0 ** 31 - 128).round_().to(torch.int64)
            theta.add_(step + k).bitwise_and_(0xffffffff)
        return y
    return fn


def shape(a, C, S, precision, mode, full, log):
    f64 = precision == "f64"
    ct, rt = (torch.complex128, torch.float64) if f64 else (torch.complex64, torch.float32)
    prec = sd.F64 if f64 else sd.F32
    alpha, beta = sd.pll_gains(BN, mode=mode)
    fcw = sd.ddc_phase_word(F0)
    # a tone a little off the centre word with some noise: the loops lock and stay locked
    n = torch.arange(S, device="cuda", dtype=torch.float64)
    df = (torch.rand(C, device="cuda", dtype=torch.float64) - 0.5) * 0.8 * BN
    x = torch.polar(torch.ones((C, S), device="cuda", dtype=torch.float64), 2 * np.pi * (F0 + df)[:, None] * n[None, :]).to(ct)
    x += 0.05 * torch.randn((C, S), device="cuda", dtype=ct)
    del n
    y = torch.empty_like(x)
    err = torch.empty((C, S), device="cuda", dtype=rt) if full else None
    freq = torch.empty((C, S), device="cuda", dtype=rt) if full else None
    bank = sd.pll_bank(C, fcw, mode, prec)
    pc, ps = min(C, a.plain_channels), min(S, a.plain_samples)
    plain = sd.pll_bank(pc, fcw, mode, prec)
    plain.set_variant(1)
    xs = x[:pc, :ps].contiguous()
    ys = torch.empty_like(xs)
    es = torch.empty((pc, ps), device="cuda", dtype=rt) if full else None
    fs = torch.empty((pc, ps), device="cuda", dtype=rt) if full else None
    ns = min(S, a.torch_samples)
    dc = min(C, 65536)
    ddc = sd.ddc_bank(1, 1, [(c, int(fcw)) for c in range(dc)], channels=dc, kind="complex", precision=prec)
    ddc.set_coeff([1.0])
    xd = x[:dc].contiguous() if dc < C else x
    yd = torch.empty_like(xd)

    def run0():
        bank.reset()  # every call starts the same loops (one memset of the state, timed with the call)
        return bank.process(x, alpha, beta, y=y, err=err, freq=freq, want_err=full, want_freq=full)

    def run1():
        plain.reset()
        return plain.process(xs, alpha, beta, y=ys, err=es, freq=fs, want_err=full, want_freq=full)

    def run_ddc():
        ddc.reset()
        return ddc.process(xd, out=yd)

    res = rounds(a, [run0, run1, torch_form(x, fcw, alpha, beta, mode, ns), run_ddc])
    ms, s0 = res[0]
    mp, s1 = res[1][0] * (C * S) / (pc * ps), res[1][1]
    mt, s2 = res[2][0] * S / ns, res[2][1]
    md, s3 = res[3][0] * C / dc, res[3][1]
    rs = 8 if f64 else 4
    model = C * S * (4 * rs + (2 * rs if full else 0))
    info = bank.info()
    lost = [name for name, t in (("(a)", mp), ("(b)", mt), ("(c)", md)) if t < ms]
    line = (f"  {C:7d} x {S:6d}  {precision} {mode:5s} {'y err freq' if full else 'y only    '} block {info['block']} waves {info['waves']} lds "
            f"{info['lds_bytes']:6d} B: {ms:9.3f} ms (spread {s0:.3f})  {C * S / (ms * 1e-3) / 1e9:7.2f} G samples/s  model "
            f"{model / 1e9:6.3f} GB -> {100 * model / (ms * 1e-3) / PEAK_BYTES:5.1f} % of 8 TB/s  |  (a) plain on {pc} x {ps}, scaled "
            f"{mp:11.3f} ms (spread {s1:.3f}) -> {mp / ms:7.2f}x  |  (b) torch loop on {ns} samples, scaled {mt:12.3f} ms (spread {s2:.3f}) -> "
            f"{mt / ms:9.2f}x  |  (c) ddc_bank T = 1 on {dc} channels, scaled {md:9.3f} ms (spread {s3:.3f}) -> {md / ms:6.2f}x")
    if lost:
        line += "  LOSES to " + ", ".join(lost)
    print(line, flush=True)
    log.append(line)
    del x, y, err, freq, xs, ys, es, fs, xd, yd, bank, plain, ddc
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="262144,65536")
    ap.add_argument("--samples", type=int, default=4032)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--modes", default="cross,bpsk,qpsk")
    ap.add_argument("--no-under", action="store_true")
    ap.add_argument("--plain-channels", type=int, default=65536)
    ap.add_argument("--plain-samples", type=int, default=252)
    ap.add_argument("--torch-samples", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "pll_bench.txt"))
    a = ap.parse_args()
    log = ["# tools/bench_pll.py " + " ".join(sys.argv[1:])]
    cases = [(int(c), a.samples) for c in a.channels.split(",") if c]
    if not a.no_under:
        cases.append((4096, 1 << 16))
    for C, S in cases:
        head = f"== {C} channels x {S} samples" + ("  (underfilled: 64 waves for 1024 SIMDs)" if C == 4096 else "")
        print(head, flush=True)
        log.append(head)
        for precision in a.precisions.split(","):
            for mode in a.modes.split(","):
                for full in (True, False):
                    shape(a, C, S, precision, mode, full, log)
                    Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured


if __name__ == "__main__":
    main()
