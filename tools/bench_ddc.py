#!/usr/bin/env python3
"""Digital down-converter bank against the two compositions a user has without it, in one process, alternating:
(a) per band index: x times a complex oscillator in torch (the oscillators are made once, outside the timed region: a user who wants
    the phase continuous from call to call would have to remake them per call) -> the real and imaginary planes as rows of one
    fir_resampler(1, D) -> re-interleave;
(b) pfb_bank with hop D on the same streams, which serves bands whose centres lie on its grid of M = max(2 D, the kind's minimum)
    sub-bands with a prototype of the same length where that is a multiple of M (it computes every sub-band, whatever the band count).
16 streams x 2^23 samples, real and complex f32 (and one f64 shape), D in {4, 16, 64}, T = 8 D, 1 / 4 / 16 bands per stream.  Device
events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min) reported.

Model bytes of the bank: S size per named channel + 8 or 16 S / D per band + 2 H size per channel; share = model bytes / time / 8 TB/s.
Multiply-adds: 2 T per output for real input, 4 T for complex input.

  python tools/bench_ddc.py [--kinds real,complex] [--downs 4,16,64] [--bands 1,4,16] [--warmup 2] [--steps 5] [--repeats 3] [--no-f64]
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
STREAMS, SAMPLES = 16, 1 << 23


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


def shape(a, precision, kind, down, nbc):
    f64 = precision == "f64"
    prec, rdt, cdt, rs = (sd.F64, torch.float64, torch.complex128, 8) if f64 else (sd.F32, torch.float32, torch.complex64, 4)
    cplx = kind == "complex"
    taps = 8 * down
    es = rs * (2 if cplx else 1)
    x = torch.randn((STREAMS, SAMPLES), device="cuda", dtype=cdt if cplx else rdt)
    outs = SAMPLES // down
    # band b of every stream sits on the grid of M sub-bands (k / M cycles per sample), so that (b) serves it too
    m = max(2 * down, 16 if cplx else 32)
    ks = [(3 + 5 * b) % (m // 2) for b in range(nbc)]
    bands = [(c, k / m) for c in range(STREAMS) for k in ks]
    bank = sd.ddc_bank(taps, down, bands, STREAMS, kind, prec)
    bank.set_antialias_coeff()
    out = torch.empty((len(bands), outs), device="cuda", dtype=cdt)

    def ddc():
        bank.process(x, out=out)

    n = torch.arange(SAMPLES, device="cuda", dtype=torch.float64)
    osc = [torch.exp(-2j * np.pi * ((k / m * n) % 1.0)).to(cdt) for k in ks]
    rs_bank = sd.fir_resampler(taps, 1, down, 2 * STREAMS, prec)
    rs_bank.set_coeff(bank.m_coeff)
    planes = torch.empty((2 * STREAMS, outs), device="cuda", dtype=rdt)

    def compose():
        ys = []
        for o in osc:
            mixed = torch.view_as_real(x * o)                                      # the full-rate complex stream, written ...
            rows = mixed.permute(2, 0, 1).reshape(2 * STREAMS, SAMPLES).contiguous()  # ... and re-read into planes
            rs_bank.process(rows, out=planes)
            ys.append(torch.complex(planes[:STREAMS], planes[STREAMS:]))
        return ys

    p = max(1, taps // m)
    pfb = sd.pfb_bank(m, p, down, STREAMS, "hamming", kind, "time", prec)

    pfb_out = torch.empty((STREAMS, outs, pfb.bins), device="cuda", dtype=cdt)

    def channelize():
        return pfb.process(x, out=pfb_out)

    t_d, t_a, t_b = [], [], []
    for _ in range(a.repeats):
        t_d.append(timed(ddc, a.warmup, a.steps))
        t_a.append(timed(compose, a.warmup, a.steps))
        t_b.append(timed(channelize, a.warmup, a.steps))
    ms, ma, mb = statistics.median(t_d), statistics.median(t_a), statistics.median(t_b)
    model = STREAMS * SAMPLES * es + len(bands) * outs * 2 * rs + 2 * STREAMS * (taps - 1) * es
    fma = len(bands) * outs * taps * (4 if cplx else 2)
    print(f"  {precision} {kind:7s} D {down:3d} T {taps:4d} bands/stream {nbc:2d}: {ms:8.3f} ms (spread {max(t_d) / min(t_d):.3f})  "
          f"model {model / 1e9:6.3f} GB -> {100 * model / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s  {fma / (ms * 1e-3) / 1e12:6.2f} T multiply-adds/s  "
          f"block {bank.info()['block_out']}  |  (a) mix+resample {ma:8.3f} ms (spread {max(t_a) / min(t_a):.3f}) -> {ma / ms:5.2f}x  |  "
          f"(b) pfb M={m} P={p} {mb:8.3f} ms (spread {max(t_b) / min(t_b):.3f}) -> {mb / ms:5.2f}x", flush=True)
    del bank, rs_bank, pfb, pfb_out, x, out, osc, planes
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="real,complex")
    ap.add_argument("--downs", default="4,16,64")
    ap.add_argument("--bands", default="1,4,16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-f64", action="store_true")
    a = ap.parse_args()
    print(f"== {STREAMS} streams x {SAMPLES} samples, T = 8 D", flush=True)
    for kind in a.kinds.split(","):
        for down in map(int, a.downs.split(",")):
            for nbc in map(int, a.bands.split(",")):
                shape(a, "f32", kind, down, nbc)
    if not a.no_f64:
        shape(a, "f64", "real", 16, 4)


if __name__ == "__main__":
    main()
