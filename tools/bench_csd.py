#!/usr/bin/env python3
"""Cross-spectral density bank against the ways to get the same estimate without it, in one process,
alternating:
  (a) stft     what a user writes with the library: stft_bank(output="complex") over the block -> drop the warm-up frames (those
               that reach into the zero history, so that the frames left are scipy's segments; hop divides N here) ->
               torch.conj(X[a]) * X[b] -> sum over frames in complex128 -> x c_k, `--pair-chunk` pairs at a time
  (b) torch    torch.stft(block, N, hop, window, center=False) -> the same
  (c) welch    welch_bank on the same input: what the auto spectra alone cost (no cross spectrum comes out of it)
Neither (a) nor (b) detrends: with detrend "constant" they do less work than the bank, so their times are lower bounds.
Pair sets: (i) disjoint pairs, channel 2 i with 2 i + 1; (ii) all pairs of the first min(16, channels) channels (120 for 16), the
remaining channels unpaired.  Shapes (1 GiB of input each): f32 1024 x 2^18 and 4 x 2^26, f64 512 x 2^18 and 2 x 2^26.  Device events
around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min) reported.  Each bank call is a
fresh estimate (reset, one process call, csd and coherence).

Byte model of the bank: the compulsory bytes are the input (S rs per channel), the history (read and written, (N - 1) rs per channel)
and the accumulators (read and written, 16 (N / 2 + 1) per pair and 8 (N / 2 + 1) per channel, once per slice).  Share of peak =
input bytes / time / 8 TB/s.  The run stage reads two spectra of N rs bytes per (entry, segment), entries = pairs + channels: its
re-read factor over the workspace volume (channels N rs per segment column) is 2 entries / channels, and "run reads" below is that
volume over the whole call's time -- a lower bound of the rate the stage itself sustains from the caches.

  python tools/bench_csd.py [--shapes f32:1024:18,f32:4:26,f64:512:18,f64:2:26] [--n 1024,256] [--hops 2] [--detrend constant]
                            [--sets disjoint,dense] [--warmup 1] [--steps 3] [--repeats 3] [--pair-chunk 8] [--no-alternatives]
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


def pair_set(kind, channels):
    if kind == "disjoint":
        return [(2 * i, 2 * i + 1) for i in range(channels // 2)]
    k = min(16, channels)
    return [(a, b) for a in range(k) for b in range(a + 1, k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="f32:1024:18,f32:4:26,f64:512:18,f64:2:26", help="precision:channels:log2(samples)")
    ap.add_argument("--n", default="1024,256")
    ap.add_argument("--hops", default="2", help="hop = N / value")
    ap.add_argument("--detrend", default="constant")
    ap.add_argument("--sets", default="disjoint,dense")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pair-chunk", type=int, default=8)
    ap.add_argument("--no-alternatives", action="store_true")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        precision, channels, lg = shape.split(":")
        channels, S = int(channels), 1 << int(lg)
        f64 = precision == "f64"
        prec, rs, dt = (sd.F64, 8, torch.float64) if f64 else (sd.F32, 4, torch.float32)
        x = torch.randn((channels, S), device="cuda", dtype=dt)
        print(f"== {precision} {channels} x 2^{lg} ({channels * S * rs / 2**30:.2f} GiB in)", flush=True)
        for n in map(int, a.n.split(",")):
            bins = n // 2 + 1
            w = sd.stft_window("hann", n)
            wt = torch.from_numpy(w).to(device="cuda", dtype=dt)
            for div in map(int, a.hops.split(",")):
                hop = n // div
                F = (S - n) // hop + 1
                skip = (n - hop) // hop  # the STFT bank's warm-up frames over its zero history
                ck = torch.full((bins,), 2.0, dtype=torch.float64, device="cuda")
                ck[0] = ck[-1] = 1.0
                ck *= 1.0 / (w * w).sum() / F
                for detrend in a.detrend.split(","):
                    for kind in a.sets.split(","):
                        pairs = pair_set(kind, channels)
                        pa = torch.tensor([p[0] for p in pairs], device="cuda")
                        pb = torch.tensor([p[1] for p in pairs], device="cuda")
                        b = sd.csd_bank(n, hop, channels, pairs, window=w, detrend=detrend, precision=prec)
                        out = torch.empty((len(pairs), bins), dtype=torch.complex128 if f64 else torch.complex64, device="cuda")
                        coh = torch.empty((len(pairs), bins), dtype=dt, device="cuda")

                        def bank():
                            b.reset()
                            b.process(x)
                            b.csd(out=out)
                            return b.coherence(out=coh)

                        fns = {"bank": bank}
                        if not a.no_alternatives:
                            def cross(X, frame_dim):
                                """X: complex, frames along `frame_dim` of (channels, ., .): sum of conj(X[a]) X[b], chunked"""
                                res = []
                                for i in range(0, len(pairs), a.pair_chunk):
                                    p = torch.conj(X[pa[i:i + a.pair_chunk]]) * X[pb[i:i + a.pair_chunk]]
                                    res.append(torch.sum(p, dim=frame_dim, dtype=torch.complex128))
                                return (torch.cat(res) * ck).to(out.dtype)

                            sb = sd.stft_bank(n, hop, channels, window=w, output="complex", precision=prec)
                            spec = torch.empty((channels, S // hop, bins), dtype=out.dtype, device="cuda")
                            wb = sd.welch_bank(n, hop, channels, window=w, detrend=detrend, precision=prec)
                            psd = torch.empty((channels, bins), dtype=dt, device="cuda")

                            def comp_stft():
                                sb.reset()
                                sb.process(x, out=spec)
                                return cross(spec[:, skip:], 1)

                            def comp_torch():
                                return cross(torch.stft(x, n, hop, window=wt, center=False, return_complex=True), 2)

                            def welch():
                                wb.reset()
                                wb.process(x)
                                return wb.psd(out=psd)

                            fns["(a) stft"] = comp_stft
                            fns["(b) torch"] = comp_torch
                            fns["(c) welch"] = welch
                        times = {k: [] for k in fns}
                        for _ in range(a.repeats):
                            for k, fn in fns.items():
                                times[k].append(timed(fn, a.warmup, a.steps))
                        base = statistics.median(times["bank"])
                        entries = len(pairs) + channels
                        parts = []
                        for k, t in times.items():
                            ms = statistics.median(t)
                            s = f"{k} {ms:8.3f} ms (spread {max(t) / min(t):.3f}"
                            if k == "bank":
                                s += (f", {100 * channels * S * rs / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s on the input, run reads "
                                      f"{2 * entries * F * n * rs / (ms * 1e-3) / 1e12:6.2f} TB/s, re-read {2 * entries / channels:.2f}x")
                            else:
                                s += f", bank {ms / base:.2f}x faster"
                            parts.append(s + ")")
                        info = b.info()
                        print(f"  N {n:5d} hop {hop:5d} {detrend:8s} {kind:8s} {len(pairs):4d} pairs F {F:8d} "
                              f"{info['slice_columns']} columns/slice {b.launches(S)} launches | " + " | ".join(parts), flush=True)
                        del fns, b
                        if not a.no_alternatives:
                            del sb, spec, wb
                        torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
