#!/usr/bin/env python3
"""Inverse STFT bank against the two ways to get the same samples without it, in one process, alternating:
  composition  what a user writes with the library alone: pack the half spectrum (torch) -> RfftPlan reverse -> x g -> overlap-add as
               N / hop strided adds in ascending frame order, carrying the pending sums by hand (bit-identical to the bank)
  torch.istft  torch.istft(X, N, hop, window) (rocFFT, bin-major layout, no streaming state): center=False where torch accepts the
               window, center=True otherwise (torch refuses center=False when the window's overlap-add is zero at the first sample,
               e.g. Hann); the line says which
1024 channels x 2^18 output samples f32, 512 x 2^18 f64.  Hann for hop < N; hop = N uses the rect window (Hann breaks NOLA there and
every implementation refuses it).  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and
spread (max / min) reported.  `--workspace` (MiB, comma list; 0 = the plan default) sweeps the bank's slice budget.

Byte model of the bank (rs = bytes per real): F bins 2 rs read + F hop rs written + 2 hist rs of pending sums per channel, the
compulsory bytes.  Share of peak = model bytes / time / 8 TB/s.

  python tools/bench_istft.py [--precision f32,f64] [--n 256,1024,4096] [--hops 4,2,1] [--workspace 0] [--no-alternatives]
                              [--samples 262144] [--warmup 2] [--steps 5] [--repeats 3]
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
    ap.add_argument("--workspace", default="0", help="bank slice budgets in MiB (0 = default)")
    ap.add_argument("--samples", type=int, default=1 << 18, help="output samples per channel")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-alternatives", action="store_true")
    a = ap.parse_args()
    S = a.samples
    for precision in a.precision.split(","):
        f64 = precision == "f64"
        prec, rs, dt, cdt = (sd.F64, 8, torch.float64, torch.complex128) if f64 else (sd.F32, 4, torch.float32, torch.complex64)
        channels = 512 if f64 else 1024
        print(f"== {precision} {channels} x {S} out ({channels * S * rs / 2**30:.2f} GiB out)", flush=True)
        for n in map(int, a.n.split(",")):
            for div in map(int, a.hops.split(",")):
                hop = n // div
                H, F, bins, K = n - hop, S // hop, n // 2 + 1, n // hop
                wname = "hann" if hop < n else "rect"
                w = sd.stft_window(wname, n)
                X = torch.randn((channels, F, bins), device="cuda", dtype=cdt)
                model = channels * (F * bins * 2 * rs + F * hop * rs + 2 * H * rs)
                banks = {}
                for ws in map(int, a.workspace.split(",")):
                    b = sd.istft_bank(n, hop, channels, window=w, precision=prec, workspace_bytes=ws << 20)
                    out = torch.empty((channels, S), dtype=dt, device="cuda")
                    b.process(X[:, :1].contiguous())  # plan and state before timing
                    banks[ws] = (b, out)
                fns = {}
                for ws, (b, out) in banks.items():
                    fns[f"bank {ws or 'default'}"] = (lambda b=b, out=out: b.process(X, out=out))
                center = None
                if not a.no_alternatives:
                    g = torch.from_numpy(next(iter(banks.values()))[0].synthesis_window).to(device="cuda", dtype=dt)
                    wt = torch.from_numpy(w).to(device="cuda", dtype=dt)
                    plan = sd.RfftPlan(n, 2, sd.reverse_fft, max_batch=channels * F, precision=prec)
                    state = {"p": torch.zeros((channels, H), device="cuda", dtype=dt)}

                    def compose():
                        packed = torch.empty((channels, F, n // 2), dtype=cdt, device="cuda")
                        packed[..., 1:] = X[..., 1:n // 2]
                        packed[..., 0] = torch.complex(X[..., 0].real, X[..., n // 2].real)
                        z = plan.exec(torch.view_as_real(packed).reshape(channels, F, n))
                        y = (z * g).view(channels, F, K, hop)
                        acc = torch.zeros((channels, F + K - 1, hop), dtype=dt, device="cuda")
                        acc[:, :K - 1] = state["p"].view(channels, K - 1, hop)
                        for r in reversed(range(K)):  # every block gets its frames in ascending order
                            acc[:, r:r + F] += y[:, :, r]
                        state["p"] = acc[:, F:].reshape(channels, H)
                        return acc[:, :F].reshape(channels, F * hop)

                    Xt = X.transpose(1, 2)  # torch.istft wants (..., bins, frames)
                    center = False
                    try:
                        torch.istft(Xt[:1, :, :4], n, hop, window=wt, center=False)
                    except RuntimeError:
                        center = True

                    def tistft():
                        return torch.istft(Xt, n, hop, window=wt, center=center)

                    fns["composition"] = compose
                    fns[f"torch.istft(center={center})"] = tistft
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
                print(f"  N {n:5d} hop {hop:5d} {wname:4s} model {model / 1e9:6.2f} GB, {b0.launches(F)} launches, inner {info['kernel']}, "
                      f"ws {info['workspace_bytes'] >> 20} MiB | " + " | ".join(parts), flush=True)
                del banks, fns, X
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
