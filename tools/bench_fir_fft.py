#!/usr/bin/env python3
"""FFT-domain (overlap-save) FIR plan against the direct-form plan on the config-4 shape: 1M channels x
4096 samples f32, 512K x 4096 f64, in place, one call per step, device events around `--steps` calls after `--warmup`.

Byte model (rs = bytes per sample), counted per channel of S samples with F = ceil(S / L) frames in P = ceil(F / 2) pairs:
direct 2 S rs (one read, one write); FFT (S + F (T-1)) rs for the frame gather's reads (the T-1 overlap re-read included; zero
padding is not read), 2 N P rs for its writes (N complex per pair), 4 N P rs for the fused convolution (one read, one write),
2 S rs for the scatter (the valid points of each pair read, written in place); both plus 2 (T-1) rs of history.  For long rows
this is 4 rs N/L + 2 rs per output sample (f32: 16 N/L + 8 B); on short rows (S < 2L) the padded transform dominates.
Share of peak = model bytes / time / 8 TB/s.

  python tools/bench_fir_fft.py [--precision f32,f64] [--warmup 2] [--steps 5] [--quick]
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK = 8e12
MIB = 1 << 20


def model_bytes(rs, fft_n, taps, samples):
    """bytes per output sample (see the module docstring)"""
    hist = 2 * (taps - 1) * rs
    if not fft_n:
        return (2 * samples * rs + hist) / samples
    frames = -(-samples // (fft_n - taps + 1))
    pairs = (frames + 1) // 2
    return ((samples + frames * (taps - 1)) * rs + 6 * fft_n * pairs * rs + 2 * samples * rs + hist) / samples


def timed(bank, x, warmup, steps):
    for _ in range(warmup):
        bank.process(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        bank.process(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def case(label, bank, x, rs, warmup, steps):
    channels, samples = x.shape
    ms = timed(bank, x, warmup, steps)
    info = bank.info()
    b = model_bytes(rs, info["fft_n"], info["taps"], samples)
    gbs = channels * samples * b / ms / 1e6
    print(f"{label:>6} taps {info['taps']:5d} fft_n {info['fft_n']:5d} ws {info['workspace_bytes'] / MIB:7.1f} MiB: {ms:9.3f} ms  "
          f"{channels * samples / ms / 1e9:7.3f} T samples/s  model {b:5.1f} B/sample -> {gbs:6.0f} GB/s = {100 * gbs * 1e9 / PEAK:5.1f} % of "
          f"8 TB/s  launches {bank.launches(samples)}  [{info['kernel']}]", flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f32,f64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="no fft_n / workspace sweeps")
    a = ap.parse_args()
    for precision in a.precision.split(","):
        f64 = precision == "f64"
        prec, rs = (sd.F64, 8) if f64 else (sd.F32, 4)
        channels, samples = (1 << 19) if f64 else (1 << 20), 4096
        x = torch.randn((channels, samples), device="cuda", dtype=torch.float64 if f64 else torch.float32)
        print(f"== {precision}: {channels} channels x {samples} samples", flush=True)

        def bank(taps, fft=True, **kw):
            b = sd.fft_fir_filter(taps, channels, prec, **kw) if fft else sd.fir_filter(taps, channels, prec)
            if taps <= 4096:  # unit DC gain: repeated filtering stays bounded
                b.set_lp_coeff(10e3, 100e3)
            else:  # beyond the designer's range: a moving average, also unit DC gain
                b.set_coeff(np.full(taps, 1.0 / taps))
            return b

        max_taps = 8192 if f64 else 16384
        for taps in (64, 128, 256, 512, 1024, 4096):
            d = case("direct", bank(taps, False), x, rs, a.warmup, a.steps)
            f = case("fft", bank(taps), x, rs, a.warmup, a.steps)
            print(f"       taps {taps}: FFT / direct speed-up {d / f:.2f}x", flush=True)
        for taps in (8192, 16384):
            if taps <= max_taps:
                case("fft", bank(taps), x, rs, a.warmup, a.steps)
        if a.quick:
            continue
        max_n = 16384 if f64 else 32768
        for taps in (1024, 4096):
            n = 16
            while n < 2 * (taps - 1):
                n *= 2
            while n <= max_n:
                case("fft_n", bank(taps, fft_n=n), x, rs, a.warmup, a.steps)
                n *= 2
            for mib in (16, 32, 64, 128, 256, 512):
                case(f"{mib}M", bank(taps, workspace_bytes=mib * MIB), x, rs, a.warmup, a.steps)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
