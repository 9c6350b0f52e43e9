#!/usr/bin/env python3
"""Symbol-timing recovery bank against what a user has without it, in one process, alternating:
(a) variant 1, the plain one-thread-per-channel kernel with table and state in global memory.  It is slow, so it runs on the first
    `--plain-samples` samples of at most `--plain-channels` channels and its time is scaled to the whole shape;
(b) arb_resampler in nearest mode with the same table at step0: the open loop, that is, the price of feedback.  It yields both
    strobes of every symbol, twice the outputs of the bank;
(c) the per-strobe loop in torch (window gather, tap products, detector, loop filter, time advance: about forty launches per strobe)
    on the first `--torch-strobes` strobes, scaled to the 2 S / sps strobes of the whole row.
Shapes: f32 and f64 on `--channels` x 4032 samples and the underfilled 4096 x 2^16; (sps, L, T) from (2, 32, 8) to (8, 32, 64), Gardner
with all outputs and with y only, the other detectors at (4, 32, 32).  The rows are QPSK symbols held for sps samples plus noise, so
the loops lock.  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min).

Model bytes per input sample: x in (8 B in f32, 16 B in f64) plus, per symbol (1 / sps of the samples), y out and one real per real
output row, as a share of 8 TB/s.  A line where variant 0 is slower than a baseline is marked LOSES.

  python tools/bench_timing.py [--channels 262144] [--precisions f32,f64] [--no-under] [--warmup 2] [--steps 5] [--repeats 3]
                               [--out profiles/timing_bench.txt]
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
BN, KD, NOISE = 0.01, 1.0, 0.05
CONFIGS = [(2, 32, 8), (4, 32, 32), (8, 32, 64)]  # (sps, L, T)


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


def torch_form(x, h, L, T, step0, alpha, beta, mode, strobes):
    """baseline (c): the recursion strobe by strobe on whole-bank tensors, over the first `strobes` strobes of every channel"""
    C = x.shape[0]
    rt = torch.float64 if x.dtype == torch.complex128 else torch.float32
    H = torch.from_numpy(np.asarray(h).reshape(T, L).T.copy()).to("cuda", rt)
    lb = L.bit_length() - 1
    taps = torch.arange(T, device="cuda")
    t = torch.zeros(C, device="cuda", dtype=torch.int64)
    w = torch.zeros(C, device="cuda", dtype=torch.int64)
    integ = torch.zeros(C, device="cuda", dtype=rt)
    ps, ym = torch.zeros(C, device="cuda", dtype=x.dtype), torch.zeros(C, device="cuda", dtype=x.dtype)
    y = torch.empty((C, strobes // 2 + 1), device="cuda", dtype=x.dtype)

    def fn():
        t.zero_()
        w.zero_()
        integ.zero_()
        for n in range(strobes):
            i = t >> 32
            p = (t & 0xffffffff) >> (32 - lb)
            idx = (i[:, None] - taps[None, :]).clamp_(min=0)
            z = (torch.gather(x, 1, idx) * H[p]).sum(dim=1)
            if n % 2 == 0:
                ym.copy_(z)
            else:
                if mode == "gardner":
                    d = ps - z
                    e = d.real * ym.real + d.imag * ym.imag
                elif mode == "zc_qpsk":
                    e = (torch.sign(ps.real) - torch.sign(z.real)) * ym.real + (torch.sign(ps.imag) - torch.sign(z.imag)) * ym.imag
                else:
                    e = (torch.sign(ps.real) - torch.sign(z.real)) * ym.real
                integ.add_(beta * e).clamp_(-0.5, 0.5)
                w.copy_(((alpha * e + integ) * 2.0 ** 32).clamp_(-2.0 ** 31, 2.0 ** 31 - 128).round_().to(torch.int64))
                y[:, n // 2] = z
                ps.copy_(z)
            t.add_(step0 + w)
        return y
    return fn


def shape(a, C, S, precision, cfg, mode, full, log):
    sps, L, T = cfg
    f64 = precision == "f64"
    ct, rt = (torch.complex128, torch.float64) if f64 else (torch.complex64, torch.float32)
    prec = sd.F64 if f64 else sd.F32
    h = sd.timing_design(L, T, sps, 0.35)
    alpha, beta = sd.timing_gains(BN, kd=KD, sps=sps)
    step0 = sd.timing_step(sps)
    # QPSK symbols held for sps samples, a random start per channel, some noise: the loops lock and stay locked
    sym = (torch.randint(0, 2, (C, S // sps + 2), device="cuda") * 2 - 1).to(rt) * (0.5 ** 0.5)
    x = torch.complex(sym.repeat_interleave(sps, dim=1)[:, :S], sym.flip(0).repeat_interleave(sps, dim=1)[:, :S]).to(ct)
    x += NOISE * torch.randn((C, S), device="cuda", dtype=ct)
    del sym
    bank = sd.timing_bank(C, sps, h, L, mode, prec)
    cap = bank.max_out(S)
    y = torch.empty((C, cap), device="cuda", dtype=ct)
    err = torch.empty((C, cap), device="cuda", dtype=rt) if full else None
    per = torch.empty((C, cap), device="cuda", dtype=rt) if full else None
    cnt = torch.empty((C,), device="cuda", dtype=torch.int32)
    pc, ps_ = min(C, a.plain_channels), min(S, a.plain_samples)
    plain = sd.timing_bank(pc, sps, h, L, mode, prec)
    plain.set_variant(1)
    xs = x[:pc, :ps_].contiguous()
    pcap = plain.max_out(ps_)
    ys = torch.empty((pc, pcap), device="cuda", dtype=ct)
    es = torch.empty((pc, pcap), device="cuda", dtype=rt) if full else None
    fs = torch.empty((pc, pcap), device="cuda", dtype=rt) if full else None
    cs = torch.empty((pc,), device="cuda", dtype=torch.int32)
    arb = sd.arb_resampler(L, T, step0, kind="complex", interp="nearest", precision=prec)
    arb.set_coeff(h)
    arb.step = step0
    ya = torch.empty((C, arb.out_samples(S)[0]), device="cuda", dtype=ct)
    strobes = min(2 * S // sps, a.torch_strobes)

    def run0():
        bank.reset()  # every call starts the same loops (one memset of the state, timed with the call)
        return bank.process(x, alpha, beta, y=y, err=err, period=per, counts=cnt)

    def run1():
        plain.reset()
        return plain.process(xs, alpha, beta, y=ys, err=es, period=fs, counts=cs)

    def run_arb():
        arb.time = 0
        return arb.process(x, out=ya)

    res = rounds(a, [run0, run1, run_arb, torch_form(x, h, L, T, step0, alpha, beta, mode, strobes)])
    ms, s0 = res[0]
    mp, s1 = res[1][0] * (C * S) / (pc * ps_), res[1][1]
    ma, s2 = res[2]
    mt, s3 = res[3][0] * (2 * S / sps) / strobes, res[3][1]
    rs = 8 if f64 else 4
    model = C * S * 2 * rs + C * (S // sps) * (2 * rs + (2 * rs if full else 0))
    info = bank.info()
    counts = cnt.to(torch.float64)
    lost = [name for name, tm in (("(a)", mp), ("(b)", ma), ("(c)", mt)) if tm < ms]
    line = (f"  {C:7d} x {S:6d}  {precision} {mode:8s} sps {sps} L {L} T {T:2d} {'y err period' if full else 'y only      '} block {info['block']} "
            f"waves {info['waves']} lds {info['lds_bytes']:6d} B: {ms:9.3f} ms (spread {s0:.3f})  {C * S / (ms * 1e-3) / 1e9:7.2f} G samples/s  "
            f"symbols per row {counts.mean().item():.1f}  model {model / 1e9:6.3f} GB -> {100 * model / (ms * 1e-3) / PEAK_BYTES:5.1f} % of 8 TB/s  |  "
            f"(a) plain on {pc} x {ps_}, scaled {mp:11.3f} ms (spread {s1:.3f}) -> {mp / ms:7.2f}x  |  (b) arb_resampler nearest at step0 "
            f"{ma:9.3f} ms (spread {s2:.3f}) -> {ma / ms:6.2f}x  |  (c) torch loop on {strobes} strobes, scaled {mt:12.3f} ms (spread {s3:.3f}) "
            f"-> {mt / ms:9.2f}x")
    if lost:
        line += "  LOSES to " + ", ".join(lost)
    print(line, flush=True)
    log.append(line)
    del x, y, err, per, cnt, xs, ys, es, fs, cs, ya, bank, plain, arb
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="262144")
    ap.add_argument("--samples", type=int, default=4032)
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--no-under", action="store_true")
    ap.add_argument("--plain-channels", type=int, default=65536)
    ap.add_argument("--plain-samples", type=int, default=252)
    ap.add_argument("--torch-strobes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "timing_bench.txt"))
    a = ap.parse_args()
    log = ["# tools/bench_timing.py " + " ".join(sys.argv[1:])]
    cases = [(int(c), a.samples) for c in a.channels.split(",") if c]
    if not a.no_under:
        cases.append((4096, 1 << 16))
    for C, S in cases:
        head = f"== {C} channels x {S} samples" + ("  (underfilled: 64 waves for 1024 SIMDs)" if C == 4096 else "")
        print(head, flush=True)
        log.append(head)
        for precision in a.precisions.split(","):
            for cfg in CONFIGS:
                for mode, full in [("gardner", True), ("gardner", False)] + ([("zc_qpsk", True), ("zc_bpsk", True)] if cfg[2] == 32 else []):
                    shape(a, C, S, precision, cfg, mode, full, log)
                    Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured


if __name__ == "__main__":
    main()
