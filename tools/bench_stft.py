#!/usr/bin/env python3
"""STFT bank against the two ways to get the same frames without it, in one process, alternating:
  composition  what a user writes with the library alone: history + block (torch.cat) -> unfold x window -> .contiguous() ->
               RfftPlan.exec -> unpack the packed half spectrum into N/2 + 1 bins (-> re re + im im), carrying the history by hand
  torch.stft   torch.stft(block, N, hop, window, center=False, return_complex=True) (-> re re + im im): the off-the-shelf
               alternative (rocFFT, bin-major layout, no history: S / hop - hist / hop frames)
1024 channels x 2^18 samples f32, 512 x 2^18 f64 (1 GiB of input).  Device events around `--steps` calls after `--warmup`;
`--repeats` alternating rounds, median and spread (max / min) reported.  `--workspace` (MiB, comma list; 0 = the plan default)
sweeps the bank's slice budget.

Byte model of the bank (rs = bytes per sample, os = bytes per output bin): S rs read + F bins os written + 2 hist rs of history
per channel, the compulsory bytes.  Share of peak = model bytes / time / 8 TB/s.

  python tools/bench_stft.py [--precision f32,f64] [--n 256,1024,4096] [--hops 4,2,1] [--outputs complex,power]
                             [--workspace 0] [--no-alternatives] [--samples 262144] [--warmup 2] [--steps 5] [--repeats 3]
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
    ap.add_argument("--precision", default="f32,f64")
    ap.add_argument("--n", default="256,1024,4096")
    ap.add_argument("--hops", default="4,2,1", help="hop = N / value")
    ap.add_argument("--outputs", default="complex,power")
    ap.add_argument("--workspace", default="0", help="bank slice budgets in MiB (0 = default)")
    ap.add_argument("--samples", type=int, default=1 << 18)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-alternatives", action="store_true")
    a = ap.parse_args()
    S = a.samples
    for precision in a.precision.split(","):
        f64 = precision == "f64"
        prec, rs, dt = (sd.F64, 8, torch.float64) if f64 else (sd.F32, 4, torch.float32)
        channels = 512 if f64 else 1024
        x = torch.randn((channels, S), device="cuda", dtype=dt)
        print(f"== {precision} {channels} x {S} ({channels * S * rs / 2**30:.2f} GiB in)", flush=True)
        for n in map(int, a.n.split(",")):
            w = sd.stft_window("hann", n)
            wt = torch.from_numpy(w).to(device="cuda", dtype=dt)
            for div in map(int, a.hops.split(",")):
                hop = n // div
                H, F, bins = n - hop, S // hop, n // 2 + 1
                for output in a.outputs.split(","):
                    os_ = 2 * rs if output == "complex" else rs
                    model = channels * (S * rs + F * bins * os_ + 2 * H * rs)
                    banks = {}
                    for ws in map(int, a.workspace.split(",")):
                        b = sd.stft_bank(n, hop, channels, window=w, output=output, precision=prec, workspace_bytes=ws << 20)
                        out = torch.empty((channels, F, bins), dtype=b._out_dtype(), device="cuda")
                        b.preload_filter(0.0)
                        banks[ws] = (b, out)
                    fns = {}
                    for ws, (b, out) in banks.items():
                        fns[f"bank {ws or 'default'}"] = (lambda b=b, out=out: b.process(x, out=out))
                    if not a.no_alternatives:
                        plan = sd.RfftPlan(n, 2, sd.forward_fft, max_batch=channels * F, precision=prec)
                        state = {"h": torch.zeros((channels, H), device="cuda", dtype=dt)}

                        def compose():
                            full = torch.cat([state["h"].flip(-1), x], dim=1)
                            state["h"] = full[:, full.shape[1] - H:].flip(-1)
                            z = plan.exec((full.unfold(-1, n, hop) * wt).contiguous())
                            y = torch.empty((channels, F, bins), dtype=z.dtype, device="cuda")
                            y[..., 1:n // 2] = z[..., 1:]
                            y[..., 0] = torch.complex(z[..., 0].real, torch.zeros_like(z[..., 0].real))
                            y[..., n // 2] = torch.complex(z[..., 0].imag, torch.zeros_like(z[..., 0].imag))
                            return y.real * y.real + y.imag * y.imag if output == "power" else y

                        def tstft():
                            z = torch.stft(x, n, hop, window=wt, center=False, return_complex=True)
                            return z.real * z.real + z.imag * z.imag if output == "power" else z

                        fns["composition"] = compose
                        fns["torch.stft"] = tstft
                    times = {k: [] for k in fns}
                    for _ in range(a.repeats):
                        for k, fn in fns.items():
                            times[k].append(timed(fn, a.warmup, a.steps))
                    b0 = banks[next(iter(banks))][0]
                    info = b0.info()
                    parts = []
                    base = None
                    for k, t in times.items():
                        ms = statistics.median(t)
                        base = base or ms
                        s = f"{k} {ms:8.3f} ms (spread {max(t) / min(t):.3f}"
                        if k.startswith("bank"):
                            s += f", {100 * model / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s"
                        else:
                            s += f", bank {ms / base:.2f}x faster"
                        parts.append(s + ")")
                    print(f"  N {n:5d} hop {hop:5d} {output:8s} model {model / 1e9:6.2f} GB, {b0.launches(S)} launches, "
                          f"inner {info['kernel']}, ws {info['workspace_bytes'] >> 20} MiB | " + " | ".join(parts), flush=True)
                    del banks, fns
                    torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
