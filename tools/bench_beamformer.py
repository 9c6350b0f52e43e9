#!/usr/bin/env python3
"""Time-delay beamformer bank against what a user has without it, in one process, alternating:
(a) variant 1, the plain one-output-per-thread kernel;
(b) torch.nn.functional.conv1d with the dense zero-filled kernel of length max delay + T (complex rows as two real planes, a kernel of
    twice the rows and columns).  The dense kernel costs B C (max delay + T) multiply-adds per sample whatever the entries hold, so it
    runs on the first `--conv-samples` samples (stream case) or the first `--conv-groups` groups (bank case) and its time is scaled to
    the whole shape; shapes whose kernel passes `--conv-kernel-limit` elements are skipped (n/a);
(c) fir_filter per entry on a delayed copy of the entry's sensor rows, then a sum into the beam: three launches per entry (real rows
    only: fir_filter has no complex rows).
Two cases: 1 group x 16 sensors x 2^22 samples with (B, T) in {(16, 16), (64, 16), (16, 64)} plus (64, 1) for complex rows, and
`--bank-groups` x 8 sensors x 4032 samples with (8, 16); f32 real and complex; dense plans with random delays in [0, spread] for a small
and a large spread (the large one splits the beam chunks: the line prints how many there are).  Device events around `--steps` calls
after `--warmup`; `--repeats` alternating rounds, median and spread (max / min).

Model: entries x T multiply-adds per group and sample (x 4 for complex rows) against (C + B) elements moved.  The multiply-add rate is
given as a share of 39.3e12 / s, the f32 rate of one scalar v_fma per lane and clock (256 CUs x 64 x 2.4 GHz; the packed form doubles
it), the bytes as a share of 8 TB/s.

  python tools/bench_beamformer.py [--cases stream,bank] [--kinds real,complex] [--spreads 32,20000] [--bank-groups 4096]
                                   [--warmup 2] [--steps 5] [--repeats 3] [--no-conv] [--no-fir] [--out profiles/beamformer_bench.txt]
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


def conv_form(a, case, delays, taps, x, groups, C, B, cplx):
    """(fn, share) of baseline (b), or None when the dense kernel is too large"""
    T = taps.shape[-1]
    length = int(delays.max()) + T
    planes = 2 if cplx else 1
    if B * C * length * planes * planes > a.conv_kernel_limit:
        return None
    dense = np.zeros((B, C, length), dtype=taps.dtype)
    for b in range(B):
        for c in range(C):
            dense[b, c, delays[b, c]:delays[b, c] + T] = taps[b, c]
    if cplx:  # [yr; yi] = [[gr, -gi], [gi, gr]] [xr; xi]
        dense = np.concatenate([np.concatenate([dense.real, -dense.imag], axis=1),
                                np.concatenate([dense.imag, dense.real], axis=1)], axis=0)
    w = torch.from_numpy(np.ascontiguousarray(dense[:, :, ::-1])).to(torch.float32).cuda()
    S = x.shape[1]
    ng, ns = (groups, min(S, a.conv_samples)) if case == "stream" else (min(groups, a.conv_groups), S)
    xs = x[:ng * C, :ns]
    xs = torch.view_as_real(xs).permute(2, 0, 1) if cplx else xs[None]                # planes, rows, samples
    xs = xs.reshape(planes, ng, C, ns).permute(1, 0, 2, 3).reshape(ng, planes * C, ns)  # groups, planes x sensors, samples
    xs = torch.nn.functional.pad(xs, (length - 1, 0)).contiguous()
    return (lambda: torch.nn.functional.conv1d(xs, w)), ng * ns / (groups * S)


def fir_form(delays, taps, x, groups, C, B):
    """baseline (c): per entry a delayed copy, fir_filter in place, and a sum into the beam"""
    S = x.shape[1]
    T = taps.shape[-1]
    filters = {}
    for b in range(B):
        for c in range(C):
            f = sd.fir_filter(T, groups, sd.F32)
            f.set_coeff(taps[b, c])
            filters[b, c] = f
    xg = x.view(groups, C, S)
    buf = torch.empty((groups, S), device="cuda", dtype=x.dtype)
    out = torch.empty((groups, B, S), device="cuda", dtype=x.dtype)

    def fn():
        out.zero_()
        for (b, c), f in filters.items():
            d = min(int(delays[b, c]), S)  # a delay beyond the block: the whole block comes from the (zero) history
            buf[:, :d] = 0
            buf[:, d:] = xg[:, c, :S - d]
            f.reset()
            f.process(buf)
            out[:, b] += buf
        return out
    return fn


def shape(a, case, groups, C, S, B, T, spread, kind, log):
    cplx = kind == "complex"
    rng = np.random.default_rng(B * 1000 + T)
    dt = torch.complex64 if cplx else torch.float32
    delays = rng.integers(0, spread + 1, (B, C))
    taps = rng.standard_normal((B, C, T)) / np.sqrt(C * T)
    if cplx:
        taps = taps + 1j * rng.standard_normal((B, C, T)) / np.sqrt(C * T)
    x = torch.randn((groups * C, S), device="cuda", dtype=dt)
    out = torch.empty((groups * B, S), device="cuda", dtype=dt)
    banks = []
    for variant in (0, 1):
        b = sd.beamformer_bank(C, B, T, groups, kind, sd.F32)
        b.set_dense(delays, taps)
        b.set_variant(variant)
        banks.append(b)
    fused, plain = banks
    fns = [lambda: fused.process(x, out=out), lambda: plain.process(x, out=out)]
    conv = None if a.no_conv else conv_form(a, case, delays, taps, x, groups, C, B, cplx)
    if conv:
        fns.append(conv[0])
    fir = None if (a.no_fir or cplx) else fir_form(delays, taps, x, groups, C, B)
    if fir:
        fns.append(fir)
    res = rounds(a, fns)
    (ms, s0), (mp, s1) = res[0], res[1]
    es = 8 if cplx else 4
    model = groups * (C + B) * S * es
    fma = groups * S * B * C * T * (4 if cplx else 1)
    info = fused.info()
    line = (f"  {case:6s} {groups:5d} x {C:2d} sensors x {S:8d}  f32 {kind:7s} B {B:3d} T {T:3d} spread {spread:6d} chunks {info['chunks']:3d} "
            f"line {info['lds_line_bytes']:6d} B: {ms:9.3f} ms (spread {s0:.3f})  {fma / (ms * 1e-3) / 1e12:6.2f} T multiply-adds/s = "
            f"{100 * fma / (ms * 1e-3) / PEAK_FMA:5.1f} % of the scalar f32 FMA rate  model {model / 1e9:6.3f} GB -> "
            f"{100 * model / (ms * 1e-3) / PEAK_BYTES:5.1f} % of 8 TB/s  |  (a) plain {mp:9.3f} ms (spread {s1:.3f}) -> {mp / ms:6.2f}x")
    i = 2
    if conv:
        mc, s2 = res[i]
        i += 1
        line += f"  |  (b) conv1d on {100 * conv[1]:.3g} % of the shape, scaled {mc / conv[1]:11.3f} ms (spread {s2:.3f}) -> {mc / conv[1] / ms:8.2f}x"
    else:
        line += "  |  (b) conv1d n/a"
    if fir:
        mf, s3 = res[i]
        line += f"  |  (c) fir_filter per entry {mf:10.3f} ms (spread {s3:.3f}) -> {mf / ms:7.2f}x"
    else:
        line += "  |  (c) fir_filter per entry n/a"
    print(line, flush=True)
    log.append(line)
    del fused, plain, banks, fns, conv, fir, x, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="stream,bank")
    ap.add_argument("--kinds", default="real,complex")
    ap.add_argument("--spreads", default="32,20000")
    ap.add_argument("--bank-groups", type=int, default=4096)
    ap.add_argument("--conv-samples", type=int, default=1 << 16)
    ap.add_argument("--conv-groups", type=int, default=64)
    ap.add_argument("--conv-kernel-limit", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-conv", action="store_true")
    ap.add_argument("--no-fir", action="store_true")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "beamformer_bench.txt"))
    a = ap.parse_args()
    log = ["# tools/bench_beamformer.py " + " ".join(sys.argv[1:])]
    for case in a.cases.split(","):
        groups, C, S = (1, 16, 1 << 22) if case == "stream" else (a.bank_groups, 8, 4032)
        head = f"== {case}: {groups} group(s) x {C} sensors x {S} samples"
        print(head, flush=True)
        log.append(head)
        for kind in a.kinds.split(","):
            bts = [(16, 16), (64, 16), (16, 64)] + ([(64, 1)] if kind == "complex" else []) if case == "stream" else [(8, 16)]
            for B, T in bts:
                for spread in map(int, a.spreads.split(",")):
                    shape(a, case, groups, C, S, B, T, spread, kind, log)
                    Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured


if __name__ == "__main__":
    main()
