#!/usr/bin/env python3
"""Polyphase synthesis bank against the two ways to get the same samples without it, in one process,
alternating:
  composition  what a user writes with the library alone: copy / pack -> FftPlan(M, RADIX_AUTO) / RfftPlan reverse -> tile P times x g
               -> the pending sums, then ceil(L / D) strided adds over the frames in ascending order, carrying the tail by hand
  torch.istft  FRAME / REAL only: torch.istft(n_fft = L, hop = D, window = g) on spectra zero-stuffed to L / 2 + 1 bins (bin k P = frame
               bin k): rocFFT at P times the transform length, its own window normalisation on top, no tail
All with the FRAME phase reference (the TIME rotation of the bank is timed as a column of its own, and so is the plain unfold form where
the sizes select the sliding one).  Complex f32 16 streams x 2^23 output samples, real f32 32 x 2^23, f64 at half the streams: 1 GiB of
output.  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min) reported.

Byte model of the bank (es = bytes per output element, 2 rs per input bin): F bins 2 rs read + S es written + 2 hist es of pending
sums per stream, the compulsory bytes.  Share of peak = model bytes / time / 8 TB/s.

  python tools/bench_pfb_synth.py [--precision f32,f64] [--outputs complex,real] [--shapes 256:16:256,1024:8:1024,...]
                                  [--no-alternatives] [--samples 8388608] [--warmup 1] [--steps 3] [--repeats 3]
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
SHAPES = "256:16:256,1024:8:1024,4096:8:4096,4096:8:2048,1024:4:768"


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
    ap.add_argument("--outputs", default="complex,real")
    ap.add_argument("--shapes", default=SHAPES, help="M:P:D, comma list")
    ap.add_argument("--samples", type=int, default=1 << 23)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-alternatives", action="store_true")
    a = ap.parse_args()
    for precision in a.precision.split(","):
        f64 = precision == "f64"
        prec, rs, rdt, cdt = (sd.F64, 8, torch.float64, torch.complex128) if f64 else (sd.F32, 4, torch.float32, torch.complex64)
        for kind in a.outputs.split(","):
            cplx = kind == "complex"
            streams = (16 if cplx else 32) // (2 if f64 else 1)
            es = rs * (2 if cplx else 1)
            for shape in a.shapes.split(","):
                m, p, hop = map(int, shape.split(":"))
                F = a.samples // hop
                S = F * hop
                Lt, H = m * p, m * p - hop
                bins = m if cplx else m // 2 + 1
                X = torch.randn((streams, F, bins), device="cuda", dtype=cdt)
                model = streams * (F * bins * 2 * rs + S * es + 2 * H * es)
                g = np.random.default_rng(1).uniform(-1, 1, Lt)  # the cost does not depend on the taps' values
                gt = torch.from_numpy(g).to(device="cuda", dtype=rdt)
                out = torch.empty((streams, S), dtype=cdt if cplx else rdt, device="cuda")

                def bank(phase, form=0):
                    b = sd.pfb_synthesis_bank(m, p, hop, streams=streams, taps=g, output=kind, phase=phase, precision=prec)
                    if form:
                        b._set_unfold_form(form)
                    return b

                b0 = bank("frame")
                banks = {"bank": b0, "bank time-phase": bank("time")}
                if b0.info()["unfold"] == "sliding":
                    banks["bank plain-form"] = bank("frame", 1)
                fns = {k: (lambda b=b: b.process(X, out=out)) for k, b in banks.items()}
                if not a.no_alternatives:
                    plan = (sd.FftPlan(m, 0, sd.reverse_fft, prec, max_batch=streams * F) if cplx else
                            sd.RfftPlan(m, 2, sd.reverse_fft, max_batch=streams * F, precision=prec))
                    state = {"tail": torch.zeros((streams, H), device="cuda", dtype=out.dtype)}

                    def compose():
                        if cplx:
                            v = plan.exec(X.clone())
                        else:
                            half = m // 2
                            packed = torch.empty((streams, F, half), dtype=cdt, device="cuda")
                            packed[..., 1:] = X[..., 1:half]
                            packed[..., 0] = torch.complex(X[..., 0].real, X[..., half].real)
                            v = plan.exec(torch.view_as_real(packed).reshape(streams, F, m))
                        y = v.repeat(1, 1, p)
                        y = torch.complex(y.real * gt, y.imag * gt) if cplx else y * gt
                        acc = torch.zeros((streams, S + H), device="cuda", dtype=out.dtype)
                        acc[:, :H] = state["tail"]
                        # frame j lands at j D: the frames k, k + q, k + 2 q .. (q = ceil(L / D)) do not overlap, so each of the q
                        # passes is one strided add; ascending k keeps every position's additions in ascending frame order
                        q = -(-Lt // hop)
                        for k in range(min(q, F)):
                            n = (F - k + q - 1) // q
                            view = acc.as_strided((streams, n, Lt), (acc.stride(0), q * hop, 1), acc.storage_offset() + k * hop)
                            view += y[:, k::q]
                        state["tail"] = acc[:, S:]
                        return acc[:, :S]

                    fns["composition"] = compose
                    if not cplx:
                        def tistft():
                            Z = torch.zeros((streams, Lt // 2 + 1, F), dtype=cdt, device="cuda")
                            Z[:, ::p] = X.transpose(1, 2)
                            # |g| + 1: a window torch's own NOLA check accepts (random taps need not); the cost is the same
                            return torch.istft(Z, Lt, hop, window=gt.abs() + 1, center=False, length=None)

                        fns["torch.istft"] = tistft
                times = {k: [] for k in fns}
                for _ in range(a.repeats):
                    for k, fn in fns.items():
                        times[k].append(timed(fn, a.warmup, a.steps))
                info = b0.info()
                parts, base = [], None
                for k, t in times.items():
                    ms = statistics.median(t)
                    base = base or ms
                    s = f"{k} {ms:8.3f} ms (spread {max(t) / min(t):.3f}"
                    if k == "bank":
                        s += f", {100 * model / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s"
                    else:
                        s += f", bank {ms / base:.2f}x faster"
                    parts.append(s + ")")
                print(f"{precision} {kind:7s} {streams:2d} x {S} M {m:5d} P {p:2d} D {hop:5d} {info['unfold']:7s} model {model / 1e9:5.2f} GB, "
                      f"{b0.launches(F)} launches, inner {info['kernel']} | " + " | ".join(parts), flush=True)
                del banks, fns, X, out, b0
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
