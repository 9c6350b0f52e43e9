#!/usr/bin/env python3
"""Polyphase FIR resampler against the composition a user writes without it, in one process, alternating:
decimation = fir_filter over the whole row + [:, ::D].contiguous(); interpolation / rational = zero-stuff to S U samples +
fir_filter + [:, ::D].contiguous().  fir_filter runs in place, so a decimating user who keeps the input copies it first:
"composition" includes that copy, "in place" filters a scratch row that is not restored (the input consumed).  1M channels x 4032 samples f32, 512K x 4032 f64 (4032 = 2^6 3^2 7 divides every q below;
160/147 runs on 4116 = 28 x 147 samples).  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds,
median and spread (max / min) reported.

Byte model of the resampler (rs = bytes per sample): S rs read + S U / D rs written + 2 H rs of history per channel.
Share of peak = model bytes / time / 8 TB/s.

  python tools/bench_resample.py [--precision f32,f64] [--taps 32,64,128,256] [--ratios 1/2,1/4] [--warmup 2] [--steps 5] [--repeats 3]
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
RATIOS = ["1/2", "1/3", "1/4", "1/8", "2/1", "4/1", "2/3", "3/2", "160/147"]


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
    ap.add_argument("--precision", default="f32,f64")
    ap.add_argument("--taps", default="32,64,128,256")
    ap.add_argument("--ratios", default=",".join(RATIOS))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-composition", action="store_true")
    a = ap.parse_args()
    for precision in a.precision.split(","):
        f64 = precision == "f64"
        prec, rs, dt = (sd.F64, 8, torch.float64) if f64 else (sd.F32, 4, torch.float32)
        channels = (1 << 19) if f64 else (1 << 20)
        for ratio in a.ratios.split(","):
            up, down = map(int, ratio.split("/"))
            samples = 4116 if ratio == "160/147" else 4032
            x = torch.randn((channels, samples), device="cuda", dtype=dt)
            outs = samples * up // down
            out = torch.empty((channels, outs), device="cuda", dtype=dt)
            print(f"== {precision} {channels} x {samples}, up {up} down {down} -> {outs} outputs", flush=True)
            for taps in map(int, a.taps.split(",")):
                r = sd.fir_resampler(taps, up, down, channels, prec)
                r.set_antialias_coeff()
                f = sd.fir_filter(taps, channels, prec)
                f.set_coeff(r.m_coeff)
                stuffed = None
                compose_ok = not a.no_composition
                if compose_ok and up > 1:
                    need = channels * samples * up * rs
                    if need > torch.cuda.mem_get_info()[0] // 2:  # 160/147: 2.5 TB zero-stuffed -- the composition cannot run
                        print(f"  composition not feasible: the zero-stuffed rows need {need / 1e9:.0f} GB", flush=True)
                        compose_ok = False
                    else:
                        stuffed = torch.zeros((channels, samples * up), device="cuda", dtype=dt)

                def resample():
                    r.process(x, out=out)

                scratch = x.clone() if compose_ok and up == 1 else None

                def compose_inplace():
                    f.process(scratch)
                    return scratch[:, ::down].contiguous() if down > 1 else scratch

                def compose():
                    if stuffed is None:
                        y = x.clone()  # fir_filter runs in place
                        f.process(y)
                    else:
                        stuffed[:, ::up] = x
                        f.process(stuffed)
                        y = stuffed
                    return y[:, ::down].contiguous() if down > 1 else y

                t_r, t_c, t_i = [], [], []
                for _ in range(a.repeats):
                    t_r.append(timed(resample, a.warmup, a.steps))
                    if compose_ok:
                        t_c.append(timed(compose, a.warmup, a.steps))
                    if scratch is not None:
                        t_i.append(timed(compose_inplace, a.warmup, a.steps))
                ms = statistics.median(t_r)
                H = (taps - 1) // up
                model = channels * (samples + outs + 2 * H) * rs
                line = (f"  taps {taps:4d} T/D {taps / down:6.1f}: {ms:8.3f} ms (spread {max(t_r) / min(t_r):.3f})  "
                        f"{channels * samples / ms / 1e6:8.2f} G in-samples/s  model {model / 1e9:6.2f} GB -> "
                        f"{100 * model / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s  [{r.info()['kernel']}]")
                if t_c:
                    mc = statistics.median(t_c)
                    line += f"  composition {mc:8.3f} ms (spread {max(t_c) / min(t_c):.3f}) -> speed-up {mc / ms:.2f}x"
                if t_i:
                    mi = statistics.median(t_i)
                    line += f"  in place {mi:8.3f} ms -> {mi / ms:.2f}x"
                print(line, flush=True)
                del r, f, stuffed, scratch
                torch.cuda.empty_cache()
            del x, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
