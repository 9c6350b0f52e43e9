#!/usr/bin/env python3
"""Arbitrary-ratio resampler bank against what a user has without it, in one process, alternating:
(a) variant 1, the plain one-output-per-thread kernel;
(b) fir_resampler(U = L, D) at the rational steps D / L both can express (8 / 32, 24 / 32 and 76 / 32 of L = 32, scaled for other L):
    the bank runs at that step in both modes; on complex input the resampler runs on the two planes with a re-interleave;
(c) a torch composition: the integer index of every output and tap (built outside the timed region, as are phase and fraction), then
    gather, weights H[p] + mu Dt[p], product and sum.  It needs outputs x T elements twice over, so it runs on the first outputs of
    the first rows only (as many as keep that at 2^27 elements) and its time is scaled to the whole shape; the line says which share
    of the outputs it ran on.
Two cases: 16 streams x 2^23 samples (single-stream-heavy) and `--bank-rows` x 4032 (bank-heavy; 1M rows as in tools/bench_resample.py
unless told otherwise -- but at 1M rows the complex shape at ratio 0.25 holds 34 GB of input and 135 GB of output, and baseline (b)
as much again for its planes, which is more than the 288 GB of one MI355X: the recorded run uses 262144 rows), (L, T) in {(32, 8), (32, 16), (128, 32)}, ratios 1.0000131, 0.7317, 2.37 and 0.25, real and complex f32 and
one f64 row (on half the rows; every line prints its own row count).  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min).

Model bytes of the bank: (S + n_out) element size per row (= 4 step / 2^32 + 4 bytes per output for real f32); share = model bytes /
time / 8 TB/s.  Multiply-adds: 2 T per output and plane in linear mode (both sums), T in nearest mode.

  python tools/bench_arb_resample.py [--cases stream,bank] [--shapes 32x8,32x16,128x32] [--ratios ...] [--kinds real,complex]
                                     [--bank-rows N] [--warmup 2] [--steps 5] [--repeats 3] [--no-f64] [--no-rational]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK = 8e12


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


def types(precision, cplx):
    f64 = precision == "f64"
    prec, rdt, cdt, rs = (sd.F64, torch.float64, torch.complex128, 8) if f64 else (sd.F32, torch.float32, torch.complex64, 4)
    return prec, rdt, cdt if cplx else rdt, rs * (2 if cplx else 1)


def bank_of(L, T, step, kind, interp, prec, h, variant=0):
    b = sd.arb_resampler(L, T, int(step), kind, interp, prec)
    b.set_coeff(h)
    b.set_variant(variant)
    b.step = int(step)
    return b


def call(bank, x, out):
    def fn():
        bank.time = 0
        bank.process(x, out=out)
    return fn


def torch_form(L, T, step, h, x, rdt):
    """(fn, share): composition (c) on the first outputs of the first rows of x, `share` of the whole problem"""
    S = x.shape[1]
    n = -(-(S << 32) // step)
    nc = min(n, max(1, (1 << 27) // T))
    rows = max(1, min(x.shape[0], (1 << 27) // (nc * T)))
    t = torch.arange(nc, device="cuda", dtype=torch.int64) * step  # below 2^63: nc < 2^27, step < 2^35 in this tool
    lb = L.bit_length() - 1
    i, f = t >> 32, t & 0xffffffff
    p = f >> (32 - lb)
    mu = ((f & ((1 << (32 - lb)) - 1)).to(torch.float64) * 2.0 ** -(32 - lb)).to(rdt)
    gi = i[:, None] - torch.arange(T, device="cuda")[None, :] + (T - 1)  # into x with T - 1 zeros in front
    hext = np.concatenate([h, [0.0]])
    Ht = torch.from_numpy(h.reshape(T, L).T.copy()).to(rdt).cuda()
    Dt = torch.from_numpy((hext[1:] - h).reshape(T, L).T.copy()).to(rdt).cuda()
    xp = torch.cat([torch.zeros((rows, T - 1), device="cuda", dtype=x.dtype), x[:rows, :int(i[-1]) + 1]], dim=1)

    def fn():
        w = Ht[p] + mu[:, None] * Dt[p]
        return (xp[:, gi] * w).sum(-1)
    return fn, rows * nc / (x.shape[0] * n)


def shape(a, case, rows, S, L, T, ratio, precision, kind):
    cplx = kind == "complex"
    prec, rdt, dt, es = types(precision, cplx)
    step = sd.arb_step(ratio)
    h = np.zeros(L * T)
    sd.load().sdsp_hip_arb_design(L, T, max(ratio, 1.0000131), h.ctypes.data)
    x = torch.randn((rows, S), device="cuda", dtype=dt)
    n = -(-(S << 32) // step)
    out = torch.empty((rows, n), device="cuda", dtype=dt)
    fused, plain = bank_of(L, T, step, kind, "linear", prec, h), bank_of(L, T, step, kind, "linear", prec, h, 1)
    comp, share = torch_form(L, T, step, h, x, rdt)
    (ms, s0), (mp, s1), (mc, s2) = rounds(a, [call(fused, x, out), call(plain, x, out), comp])
    mc /= share
    model = rows * (S + n) * es
    fma = rows * n * T * 2 * (2 if cplx else 1)
    print(f"  {case:6s} {rows:7d} rows {precision} {kind:7s} L {L:3d} T {T:2d} ratio {ratio:<9g}: {ms:8.3f} ms (spread {s0:.3f})  model {model / 1e9:6.3f} GB -> "
          f"{100 * model / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s  {fma / (ms * 1e-3) / 1e12:6.2f} T multiply-adds/s  block {fused.info()['block_out']}"
          f"  |  (a) plain {mp:8.3f} ms (spread {s1:.3f}) -> {mp / ms:5.2f}x  |  (c) torch on {100 * share:.3g} % of the outputs, scaled {mc:9.3f} ms "
          f"(spread {s2:.3f}) -> {mc / ms:6.2f}x", flush=True)
    del fused, plain, comp, x, out
    torch.cuda.empty_cache()


def rational(a, case, rows, S, L, T, d32, precision, kind):
    """(b): the bank at step D / L in both modes against fir_resampler(L T taps, L, D)"""
    cplx = kind == "complex"
    prec, rdt, dt, es = types(precision, cplx)
    D = d32 * L // 32
    q = D // int(np.gcd(L, D))
    S = S // q * q
    step = (D << 32) // L
    n = S * L // D
    h = np.zeros(L * T)
    sd.load().sdsp_hip_arb_design(L, T, max(D / L, 1.0000131), h.ctypes.data)
    x = torch.randn((rows, S), device="cuda", dtype=dt)
    out = torch.empty((rows, n), device="cuda", dtype=dt)
    lin, near = bank_of(L, T, step, kind, "linear", prec, h), bank_of(L, T, step, kind, "nearest", prec, h)
    planes = 2 if cplx else 1
    r = sd.fir_resampler(L * T, L, D, planes * rows, prec)
    r.set_coeff(h)
    pout = torch.empty((planes * rows, n), device="cuda", dtype=rdt)

    def resample():
        if not cplx:
            return r.process(x, out=pout)
        r.process(torch.view_as_real(x).permute(2, 0, 1).reshape(2 * rows, S).contiguous(), out=pout)
        return torch.complex(pout[:rows], pout[rows:])

    (ml, s0), (mn, s1), (mb, s2) = rounds(a, [call(lin, x, out), call(near, x, out), resample])
    print(f"  {case:6s} {rows:7d} rows {precision} {kind:7s} L {L:3d} T {T:2d} D / L {D}/{L}: linear {ml:8.3f} ms (spread {s0:.3f})  nearest {mn:8.3f} ms "
          f"(spread {s1:.3f})  |  (b) fir_resampler({L * T}, {L}, {D}) {mb:8.3f} ms (spread {s2:.3f}) -> {mb / ml:5.2f}x of linear, "
          f"{mb / mn:5.2f}x of nearest", flush=True)
    del lin, near, r, x, out, pout
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="stream,bank")
    ap.add_argument("--shapes", default="32x8,32x16,128x32")
    ap.add_argument("--ratios", default="1.0000131,0.7317,2.37,0.25")
    ap.add_argument("--kinds", default="real,complex")
    ap.add_argument("--bank-rows", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-f64", action="store_true")
    ap.add_argument("--no-rational", action="store_true")
    a = ap.parse_args()
    sizes = {"stream": (16, 1 << 23), "bank": (a.bank_rows, 4032)}
    lts = [tuple(map(int, s.split("x"))) for s in a.shapes.split(",")]
    for case in a.cases.split(","):
        rows, S = sizes[case]
        print(f"== {case}: {rows} rows x {S} samples", flush=True)
        for kind in a.kinds.split(","):
            for L, T in lts:
                for ratio in map(float, a.ratios.split(",")):
                    shape(a, case, rows, S, L, T, ratio, "f32", kind)
        if not a.no_f64:
            shape(a, case, rows // 2, S, 32, 16, 0.7317, "f64", "real")
        if not a.no_rational:
            for kind in a.kinds.split(","):
                for L, T in lts:
                    for d32 in (8, 24, 76):
                        rational(a, case, rows, S, L, T, d32, "f32", kind)


if __name__ == "__main__":
    main()
