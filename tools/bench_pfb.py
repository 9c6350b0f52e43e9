#!/usr/bin/env python3
"""Polyphase filter-bank channelizer bank against the two ways to get the same sub-bands without it, in one
process, alternating:
  composition  what a user writes with the library alone: history + block (torch.cat) -> unfold(L, D) x taps -> view (C, F, P, M) ->
               the P branches added in ascending order -> .contiguous() -> RfftPlan.exec + unpack (real input) or
               FftPlan(M, RADIX_AUTO).exec (complex input), carrying the history by hand
  torch.stft   torch.stft(block, n_fft = L, hop = D, window = taps, center=False)[k P] (onesided=False for complex input): the
               L-point STFT with every P-th bin kept (rocFFT, bin-major layout, no history)
All three with the FRAME phase reference (the TIME rotation of the bank is timed as a column of its own, and so is the plain fold form
where the sizes select the sliding one).  Complex f32 16 streams x 2^23, real f32 32 x 2^23, f64 at half the streams: 1 GiB of input.
Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min) reported.

Byte model of the bank (es = bytes per input element, 2 rs per output bin): S es read + F bins 2 rs written + 2 hist es of history per
stream, the compulsory bytes.  Share of peak = model bytes / time / 8 TB/s.

  python tools/bench_pfb.py [--precision f32,f64] [--inputs complex,real] [--shapes 256:16:256,1024:8:1024,...]
                            [--no-alternatives] [--samples 8388608] [--warmup 1] [--steps 3] [--repeats 3]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
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
    ap.add_argument("--inputs", default="complex,real")
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
        for kind in a.inputs.split(","):
            cplx = kind == "complex"
            streams = (16 if cplx else 32) // (2 if f64 else 1)
            es = rs * (2 if cplx else 1)
            for shape in a.shapes.split(","):
                m, p, hop = map(int, shape.split(":"))
                S = a.samples // hop * hop
                x = torch.randn((streams, S), device="cuda", dtype=cdt if cplx else rdt)
                Lt, H, F = m * p, m * p - hop, S // hop
                bins = m if cplx else m // 2 + 1
                model = streams * (S * es + F * bins * 2 * rs + 2 * H * es)
                h = sd.pfb_prototype("hamming", m, p)
                ht = torch.from_numpy(h).to(device="cuda", dtype=rdt)
                out = torch.empty((streams, F, bins), dtype=cdt, device="cuda")

                def bank(phase, form=0):
                    b = sd.pfb_bank(m, p, hop, streams=streams, taps=h, input=kind, phase=phase, precision=prec)
                    b.preload_filter(0.0)
                    if form:
                        b._set_fold_form(form)
                    return b

                b0 = bank("frame")
                banks = {"bank": b0, "bank time-phase": bank("time")}
                if b0.info()["fold"] == "sliding":
                    banks["bank plain-form"] = bank("frame", 1)
                fns = {k: (lambda b=b: b.process(x, out=out)) for k, b in banks.items()}
                if not a.no_alternatives:
                    plan = (sd.FftPlan(m, 0, sd.forward_fft, prec, max_batch=streams * F) if cplx else
                            sd.RfftPlan(m, 2, sd.forward_fft, max_batch=streams * F, precision=prec))
                    state = {"h": torch.zeros((streams, H), device="cuda", dtype=x.dtype)}

                    def compose():
                        full = torch.cat([state["h"].flip(-1), x], dim=1)
                        state["h"] = full[:, full.shape[1] - H:].flip(-1)
                        fr = (full.unfold(-1, Lt, hop) * ht).view(streams, F, p, m)
                        u = fr[:, :, 0]
                        for q in range(1, p):
                            u = u + fr[:, :, q]
                        z = plan.exec(u.contiguous())
                        if cplx:
                            return z
                        y = torch.empty((streams, F, bins), dtype=z.dtype, device="cuda")
                        y[..., 1:m // 2] = z[..., 1:]
                        y[..., 0] = torch.complex(z[..., 0].real, torch.zeros_like(z[..., 0].real))
                        y[..., m // 2] = torch.complex(z[..., 0].imag, torch.zeros_like(z[..., 0].imag))
                        return y

                    def tstft():
                        z = torch.stft(x, Lt, hop, window=ht, center=False, return_complex=True, onesided=not cplx)
                        return z[:, ::p].contiguous()

                    fns["composition"] = compose
                    fns["torch.stft"] = tstft
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
                print(f"{precision} {kind:7s} {streams:2d} x {S} M {m:5d} P {p:2d} D {hop:5d} {info['fold']:7s} model {model / 1e9:5.2f} GB, "
                      f"{b0.launches(S)} launches, inner {info['kernel']} | " + " | ".join(parts), flush=True)
                del banks, fns, x, out, b0
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
