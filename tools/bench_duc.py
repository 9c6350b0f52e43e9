#!/usr/bin/env python3
"""Digital up-converter bank, both kernel variants, against the two compositions a user has without it, in
one process, alternating:
(a) per band index: the real and imaginary planes of that band of every stream as rows of one fir_resampler(U, 1) -> times a complex
    oscillator in torch (the oscillators are made once, outside the timed region: a user who wants the phase continuous from call to
    call would have to remake them per call) -> added to the stream's sum;
(b) pfb_synthesis_bank with hop U on M = max(2 U, 32) sub-bands, which places bands on its grid only, with the dual of a Hamming
    prototype of the same length where that is a multiple of M and a dual exists (it synthesises from every sub-band, whatever the
    band count).
16 output streams x 2^23 output samples, complex and real f32 output (and one f64 shape), U in {4, 16, 64}, T = 8 U, 1 / 4 / 16
bands per stream.  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread
(max / min) reported.

Model bytes of the bank: one complex element (8 or 16 bytes) x S / U in per band + 4 or 8 bytes (f32; twice that in f64) x S out
per stream + 2 H elements per band; share = model bytes / time / 8 TB/s.  Multiply-adds: 2 T / U per output and band (the filter
sum; the oscillator's two complex products per output and band are not counted).

  python tools/bench_duc.py [--kinds complex,real] [--ups 4,16,64] [--bands 1,4,16] [--warmup 2] [--steps 5] [--repeats 3] [--no-f64]
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


def shape(a, precision, kind, up, nbc):
    f64 = precision == "f64"
    prec, rdt, cdt, rs = (sd.F64, torch.float64, torch.complex128, 8) if f64 else (sd.F32, torch.float32, torch.complex64, 4)
    cplx = kind == "complex"
    taps = 8 * up
    ins = SAMPLES // up
    # band b of every stream sits on the grid of M sub-bands (k / M cycles per output sample), so that (b) could place it too;
    # row c nbc + b of the input is band b of stream c
    m = max(2 * up, 32)
    ks = [(3 + 5 * b) % (m // 2) for b in range(nbc)]
    bands = [(c, k / m) for c in range(STREAMS) for k in ks]
    nb = len(bands)
    x = torch.randn((nb, ins), device="cuda", dtype=cdt)
    out = torch.empty((STREAMS, SAMPLES), device="cuda", dtype=cdt if cplx else rdt)
    banks = []
    for variant in (0, 1):
        bank = sd.duc_bank(taps, up, bands, STREAMS, kind, prec)
        bank.set_antiimage_coeff()
        bank.set_variant(variant)
        banks.append(bank)

    def fused():
        banks[0].process(x, out=out)

    def plain():
        banks[1].process(x, out=out)

    n = torch.arange(SAMPLES, device="cuda", dtype=torch.float64)
    osc = [torch.exp(2j * np.pi * ((k / m * n) % 1.0)).to(cdt) for k in ks]
    del n
    rs_bank = sd.fir_resampler(taps, up, 1, 2 * STREAMS, prec)
    rs_bank.set_coeff(banks[0].m_coeff)
    planes = torch.empty((2 * STREAMS, SAMPLES), device="cuda", dtype=rdt)
    xb = x.view(STREAMS, nbc, ins)

    def compose():
        acc = None
        for b, o in enumerate(osc):
            rows = torch.view_as_real(xb[:, b]).permute(2, 0, 1).reshape(2 * STREAMS, ins).contiguous()
            rs_bank.process(rows, out=planes)  # the full-rate planes, written ...
            if cplx:
                y = torch.complex(planes[:STREAMS], planes[STREAMS:]) * o  # ... and re-read
            else:
                y = planes[:STREAMS] * o.real - planes[STREAMS:] * o.imag
            acc = y if acc is None else acc.add_(y)
        return acc

    p = max(1, taps // m)
    pfb, mb_note = None, ""
    try:
        pfb = sd.pfb_synthesis_bank(m, p, up, STREAMS, "hamming", kind, "time", prec)
        spec = torch.randn((STREAMS, ins, pfb.bins), device="cuda", dtype=cdt)
        pfb_out = torch.empty((STREAMS, SAMPLES), device="cuda", dtype=cdt if cplx else rdt)
    except sd.SdspHipError:
        pfb, mb_note = None, "no dual prototype: not measured"

    def synthesise():
        return pfb.process(spec, out=pfb_out)

    t0, t1, t_a, t_b = [], [], [], []
    for _ in range(a.repeats):
        t0.append(timed(fused, a.warmup, a.steps))
        t1.append(timed(plain, a.warmup, a.steps))
        t_a.append(timed(compose, a.warmup, a.steps))
        if pfb is not None:
            t_b.append(timed(synthesise, a.warmup, a.steps))
    m0, m1, ma = statistics.median(t0), statistics.median(t1), statistics.median(t_a)
    hist = (taps - 1) // up
    model = nb * ins * 2 * rs + STREAMS * SAMPLES * rs * (2 if cplx else 1) + 2 * nb * hist * 2 * rs
    fma = nb * SAMPLES * 2 * (taps // up)
    best = min(m0, m1)
    line = (f"  {precision} {kind:7s} U {up:3d} T {taps:4d} bands/stream {nbc:2d}: fused {m0:8.3f} ms (spread {max(t0) / min(t0):.3f})  "
            f"plain {m1:8.3f} ms (spread {max(t1) / min(t1):.3f}) -> plain / fused {m1 / m0:5.2f}x  model {model / 1e9:6.3f} GB -> "
            f"{100 * model / (m0 * 1e-3) / PEAK:5.1f} % of 8 TB/s  {fma / (m0 * 1e-3) / 1e12:6.2f} T multiply-adds/s  "
            f"block_in {banks[0].info()['block_in']}  |  (a) resample+mix+sum {ma:8.3f} ms (spread {max(t_a) / min(t_a):.3f}) -> "
            f"{ma / m0:5.2f}x of fused, {ma / best:5.2f}x of the faster variant  |  ")
    if pfb is not None:
        mb = statistics.median(t_b)
        line += f"(b) pfb_synth M={m} P={p} {mb:8.3f} ms (spread {max(t_b) / min(t_b):.3f}) -> {mb / m0:5.2f}x of fused"
    else:
        line += f"(b) pfb_synth M={m} P={p}: {mb_note}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="complex,real")
    ap.add_argument("--ups", default="4,16,64")
    ap.add_argument("--bands", default="1,4,16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-f64", action="store_true")
    a = ap.parse_args()
    print(f"== {STREAMS} output streams x {SAMPLES} output samples, T = 8 U", flush=True)
    for kind in a.kinds.split(","):
        for up in map(int, a.ups.split(",")):
            for nbc in map(int, a.bands.split(",")):
                shape(a, "f32", kind, up, nbc)
                torch.cuda.empty_cache()
    if not a.no_f64:
        shape(a, "f64", "complex", 16, 4)


if __name__ == "__main__":
    main()
