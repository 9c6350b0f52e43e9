#!/usr/bin/env python3
"""Welch PSD bank against the two ways to get the same estimate without it, in one process, alternating:
  (a) stft     what a user writes with the library: stft_bank(output="power") over the block -> drop the warm-up frames (those
               that reach into the zero history, so that the frames left are scipy's segments; hop divides N here) ->
               torch.sum(dim=1, dtype=float64) -> x c_k
  (b) torch    torch.stft(block, N, hop, window, center=False) -> re re + im im -> mean over frames -> x c_k
Neither composition detrends: with detrend "constant" they do less work than the bank, so their times are lower bounds.
Shapes (1 GiB of input each): f32 1024 x 2^18 and 4 x 2^26, f64 512 x 2^18 and 2 x 2^26.  Device events around `--steps` calls
after `--warmup`; `--repeats` alternating rounds, median and spread (max / min) reported.  Each bank call is a fresh estimate
(reset, one process call, psd).

Byte model of the bank: the compulsory bytes are the input (S rs per channel); the workspace round trips (segments written, read and
written by the transform, read by the run stage: ~4 F N rs per channel) stay on the chip only in part.  Share of peak = input bytes
/ time / 8 TB/s.  The composition (a) writes and reads the power spectrogram (F bins rs per channel) on top of the same transform.

  python tools/bench_welch.py [--shapes f32:1024:18,f32:4:26,f64:512:18,f64:2:26] [--n 256,1024,4096] [--hops 2,4]
                              [--detrend none,constant] [--warmup 2] [--steps 5] [--repeats 3] [--no-alternatives]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="f32:1024:18,f32:4:26,f64:512:18,f64:2:26", help="precision:channels:log2(samples)")
    ap.add_argument("--n", default="256,1024,4096")
    ap.add_argument("--hops", default="2,4", help="hop = N / value")
    ap.add_argument("--detrend", default="none,constant")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-alternatives", action="store_true")
    a = ap.parse_args()
    best = {}
    for shape in a.shapes.split(","):
        precision, channels, lg = shape.split(":")
        channels, S = int(channels), 1 << int(lg)
        f64 = precision == "f64"
        prec, rs, dt = (sd.F64, 8, torch.float64) if f64 else (sd.F32, 4, torch.float32)
        x = torch.randn((channels, S), device="cuda", dtype=dt)
        print(f"== {precision} {channels} x 2^{lg} ({channels * S * rs / 2**30:.2f} GiB in)", flush=True)
        for n in map(int, a.n.split(",")):
            w = sd.stft_window("hann", n)
            wt = torch.from_numpy(w).to(device="cuda", dtype=dt)
            for div in map(int, a.hops.split(",")):
                hop = n // div
                F = (S - n) // hop + 1
                skip = (n - hop) // hop  # the STFT bank's warm-up frames over its zero history
                for detrend in a.detrend.split(","):
                    b = sd.welch_bank(n, hop, channels, window=w, detrend=detrend, precision=prec)
                    out = torch.empty((channels, n // 2 + 1), dtype=dt, device="cuda")

                    def bank():
                        b.reset()
                        b.process(x)
                        return b.psd(out=out)

                    fns = {"bank": bank}
                    if not a.no_alternatives:
                        ck = torch.full((n // 2 + 1,), 2.0, dtype=torch.float64, device="cuda")
                        ck[0] = ck[-1] = 1.0
                        ck *= 1.0 / (w * w).sum() / F
                        sb = sd.stft_bank(n, hop, channels, window=w, output="power", precision=prec)
                        spec = torch.empty((channels, S // hop, n // 2 + 1), dtype=dt, device="cuda")

                        def comp_stft():
                            sb.reset()
                            sb.process(x, out=spec)
                            return (torch.sum(spec[:, skip:], dim=1, dtype=torch.float64) * ck).to(dt)

                        def comp_torch():
                            z = torch.stft(x, n, hop, window=wt, center=False, return_complex=True)
                            p = z.real * z.real + z.imag * z.imag  # (channels, bins, F)
                            return (p.mean(dim=-1).to(torch.float64) * (ck * F)).to(dt)

                        fns["(a) stft"] = comp_stft
                        fns["(b) torch"] = comp_torch
                    times = {k: [] for k in fns}
                    for _ in range(a.repeats):
                        for k, fn in fns.items():
                            times[k].append(timed(fn, a.warmup, a.steps))
                    parts = []
                    base = statistics.median(times["bank"])
                    best[(precision, channels, n, hop, detrend)] = base
                    for k, t in times.items():
                        ms = statistics.median(t)
                        s = f"{k} {ms:8.3f} ms (spread {max(t) / min(t):.3f}"
                        if k == "bank":
                            s += f", {100 * channels * S * rs / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s on the input"
                        else:
                            s += f", bank {ms / base:.2f}x faster"
                        parts.append(s + ")")
                    print(f"  N {n:5d} hop {hop:5d} {detrend:8s} F {F:8d} {b.launches(S)} launches | " + " | ".join(parts), flush=True)
                    del fns, b
                    if not a.no_alternatives:
                        del sb, spec
                    torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()
    # few long channels against many short ones of the same bytes
    pairs = {"f32": (1024, 4), "f64": (512, 2)}
    for (precision, channels, n, hop, detrend), t in best.items():
        many, few = pairs.get(precision, (None, None))
        if channels == few and (precision, many, n, hop, detrend) in best:
            tm = best[(precision, many, n, hop, detrend)]
            print(f"few/many {precision} N {n:5d} hop {hop:5d} {detrend:8s}: {few} ch {t:8.3f} ms / {many} ch {tm:8.3f} ms = "
                  f"{t / tm:.2f}", flush=True)


if __name__ == "__main__":
    main()
