#!/usr/bin/env python3
"""LMS / NLMS adaptive filter bank against what a user has without it, in one process, alternating:
(a) variant 1, the plain one-thread-per-channel kernel with its weights in global memory.  It is slow, so it runs on the first
    `--plain-samples` samples of at most `--plain-channels` channels and its time is scaled to the whole shape;
(b) the per-sample loop in torch (window view x weights, sum, error, update: six launches per sample) on the first `--torch-samples`
    samples, scaled to the whole row;
(c) with mu = 0 (frozen weights), fir_filter at the same T on the same rows (real rows only: fir_filter has no complex rows): the
    price of carrying adaptable weights in registers instead of SGPRs.
Shapes, all f32: `--channels` x 4032 samples at T in {8, 12, 16, 24, 32, 48, 64} (12, 24 and 48 run the form of the kernel with
per-group tests, the others the form without), real and complex, LMS and NLMS; and 4096 x 2^16, the underfilled
case (64 waves on 1024 SIMDs).  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and
spread (max / min).

Model: real LMS 2 T multiply-adds per sample (NLMS 3 T), complex 8 T (NLMS 10 T), against four elements moved (x, d in; y, e out).
The multiply-add rate is given as a share of 39.3e12 / s, the f32 rate of one scalar v_fma per lane and clock (256 CUs x 64 x 2.4 GHz),
the bytes as a share of 8 TB/s.  A line where variant 0 is slower than a baseline is marked LOSES.

  python tools/bench_lms.py [--channels 262144,65536] [--taps 8,12,16,24,32,48,64] [--kinds real,complex] [--modes lms,nlms] [--no-under]
                            [--warmup 2] [--steps 5] [--repeats 3] [--out profiles/lms_bench.txt]
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
PEAK_FMA = 256 * 64 * 2.4e9


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


def torch_form(x, d, T, mu, eps, nlms, ns):
    """baseline (b): the recursion sample by sample on whole-bank tensors, over the first ns samples"""
    C = x.shape[0]
    xp = torch.nn.functional.pad(x[:, :ns], (T - 1, 0)).contiguous()
    win = xp.unfold(1, T, 1).flip(2)  # win[:, n, t] = x[n - t], a view
    w = torch.zeros((C, T), device=x.device, dtype=x.dtype)
    y = torch.empty((C, ns), device=x.device, dtype=x.dtype)
    e = torch.empty((C, ns), device=x.device, dtype=x.dtype)

    def fn():
        w.zero_()
        for n in range(ns):
            v = win[:, n]
            y[:, n] = (w * v).sum(1)
            e[:, n] = d[:, n] - y[:, n]
            g = mu * e[:, n]
            if nlms:
                g = g / (eps + (v * v.conj()).real.sum(1))
            w.add_(g[:, None] * v.conj())
        return y
    return fn


def shape(a, C, S, T, kind, mode, log):
    cplx, nlms = kind == "complex", mode == "nlms"
    dt = torch.complex64 if cplx else torch.float32
    mu, eps = (0.5, 1e-3) if nlms else (0.2 / T, 0.0)
    x = torch.randn((C, S), device="cuda", dtype=dt)
    d = torch.randn((C, S), device="cuda", dtype=dt)
    y, e = torch.empty_like(x), torch.empty_like(x)
    bank = sd.lms_bank(C, T, kind, sd.F32, mode, eps)
    pc, ps = min(C, a.plain_channels), min(S, a.plain_samples)
    plain = sd.lms_bank(pc, T, kind, sd.F32, mode, eps)
    plain.set_variant(1)
    xs, ds = x[:pc, :ps].contiguous(), d[:pc, :ps].contiguous()
    ys, es = torch.empty_like(xs), torch.empty_like(xs)
    ns = min(S, a.torch_samples)

    def run0():
        bank.reset()  # every call starts the same stream (one memset of the state, timed with the call): the weights stay bounded
        return bank.process(x, d, mu, y=y, e=e)

    def run1():
        plain.reset()
        return plain.process(xs, ds, mu, y=ys, e=es)

    fns = [run0, run1, torch_form(x, d, T, mu, eps, nlms, ns)]
    fir = None
    if not cplx:
        frozen = sd.lms_bank(C, T, kind, sd.F32, mode, eps)
        h = np.random.default_rng(T).standard_normal(T) / T
        frozen.set_weights(torch.from_numpy(np.tile(h, (C, 1))).to(torch.float32))
        fir = sd.fir_filter(T, C, sd.F32)
        fir.set_coeff(h)
        buf = torch.empty_like(x)

        def run_fir():
            buf.copy_(x)  # fir_filter works in place: the copy is timed on its own and taken off
            fir.process(buf)

        fns += [lambda: frozen.process(x, d, 0.0, y=y, e=e), run_fir, lambda: buf.copy_(x)]
    res = rounds(a, fns)
    ms, s0 = res[0]
    mp, s1 = res[1][0] * (C * S) / (pc * ps), res[1][1]
    mt, s2 = res[2][0] * S / ns, res[2][1]
    es_ = 8 if cplx else 4
    model = 4 * C * S * es_
    fma = C * S * T * ((10 if nlms else 8) if cplx else (3 if nlms else 2))
    info = bank.info()
    lost = []
    line = (f"  {C:7d} x {S:6d}  f32 {kind:7s} {mode:4s} T {T:2d} block {info['block']:2d} lds {info['lds_bytes']:6d} B: {ms:9.3f} ms "
            f"(spread {s0:.3f})  {fma / (ms * 1e-3) / 1e12:6.2f} T multiply-adds/s = {100 * fma / (ms * 1e-3) / PEAK_FMA:5.1f} % of the "
            f"scalar f32 FMA rate  model {model / 1e9:6.3f} GB -> {100 * model / (ms * 1e-3) / PEAK_BYTES:5.1f} % of 8 TB/s  |  (a) plain on "
            f"{pc} x {ps}, scaled {mp:11.3f} ms (spread {s1:.3f}) -> {mp / ms:7.2f}x  |  (b) torch loop on {ns} samples, scaled "
            f"{mt:12.3f} ms (spread {s2:.3f}) -> {mt / ms:9.2f}x")
    lost += ["(a)"] if mp < ms else []
    lost += ["(b)"] if mt < ms else []
    if fir:
        (mz, s3), (mf, s4), (mc, _) = res[3], res[4], res[5]
        mf = mf - mc
        line += f"  |  (c) mu = 0: {mz:9.3f} ms (spread {s3:.3f}) against fir_filter {mf:9.3f} ms (spread {s4:.3f}) -> {mf / mz:6.2f}x"
        lost += ["(c)"] if mf < mz else []
    else:
        line += "  |  (c) fir_filter n/a"
    if lost:
        line += "  LOSES to " + ", ".join(lost)
    print(line, flush=True)
    log.append(line)
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="262144,65536")
    ap.add_argument("--samples", type=int, default=4032)
    ap.add_argument("--taps", default="8,12,16,24,32,48,64")
    ap.add_argument("--kinds", default="real,complex")
    ap.add_argument("--modes", default="lms,nlms")
    ap.add_argument("--no-under", action="store_true")
    ap.add_argument("--plain-channels", type=int, default=65536)
    ap.add_argument("--plain-samples", type=int, default=252)
    ap.add_argument("--torch-samples", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "lms_bench.txt"))
    a = ap.parse_args()
    log = ["# tools/bench_lms.py " + " ".join(sys.argv[1:])]
    cases = [(int(c), a.samples, [int(t) for t in a.taps.split(",")]) for c in a.channels.split(",") if c]
    if not a.no_under:
        cases.append((4096, 1 << 16, [16, 48, 64]))
    for C, S, taps in cases:
        head = f"== {C} channels x {S} samples" + ("  (underfilled: 64 waves for 1024 SIMDs)" if C == 4096 else "")
        print(head, flush=True)
        log.append(head)
        for kind in a.kinds.split(","):
            for mode in a.modes.split(","):
                for T in taps:
                    shape(a, C, S, T, kind, mode, log)
                    Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured


if __name__ == "__main__":
    main()
