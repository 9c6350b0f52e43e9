#!/usr/bin/env python3
"""Forward-backward filtering plans against the composition a user writes with the library alone, in one process,
alternating:
  variant 0    the fused kernel (one wave per 64 channels, super-tile transport), the default
  variant 1    the direct kernel (one lane per channel, plain accesses), bit-identical
  composition  torch.cat (odd edge extension) -> steady-state buffer -> sdsp_hip_iir_process -> flip -> second state -> process ->
               flip -> slice (bit-identical to the plan).  Its rows are L + 2P samples; where that is not a multiple of 16 bytes the
               IIR bank serves them with its direct kernel
  composition P=P'  the same with the smallest P' >= P that makes L + 2P' a multiple of 16 bytes, so that the IIR bank runs its tuned
               kernels: the same work at a slightly different edge (not the plan's bits), the composition's best case
Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min) reported.

Byte model of the plan: every sample read and written once in each direction, 4 L rs per channel (f32 16 B, f64 32 B per sample), plus
4 P rs of right-edge workspace (written, read and written, read).  Share of peak = model bytes / time / 8 TB/s.

  python tools/bench_filtfilt.py [--shapes big4,big8,f64,ragged,long,sweep] [--warmup 2] [--steps 5] [--repeats 3]
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK = 8e12
# name -> (precision, channels, samples, sections, slice budgets in MiB to sweep (0 = default))
SHAPES = {
    "big4": ("f32", 262144, 4096, 4, [0]),
    "big8": ("f32", 262144, 4096, 8, [0]),
    "f64": ("f64", 131072, 4096, 4, [0]),
    "ragged": ("f32", 65536, 10000, 4, [0]),
    "long": ("f32", 4096, 1 << 18, 4, [0]),
    "sweep": ("f32", 262144, 4096, 4, [4, 16, 64, 256, 1024]),
}


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
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-composition", action="store_true")
    a = ap.parse_args()
    lib = sd.load()
    for name in a.shapes.split(","):
        precision, channels, L, m, budgets = SHAPES[name]
        f64 = precision == "f64"
        prec, rs, dt = (sd.F64, 8, torch.float64) if f64 else (sd.F32, 4, torch.float32)
        a_c, b_c, g = np.zeros(3 * m), np.zeros(3 * m), C.c_double()
        sd._lib.check(lib.sdsp_hip_iir_design_lp(m, 2e3, 48e3, 1.0, a_c.ctypes.data, b_c.ctypes.data, C.byref(g)))
        gain = g.value
        x = torch.randn((channels, L), device="cuda", dtype=dt).cumsum_(1)
        plans = {}
        for ws in budgets:
            for v in ((0, 1) if len(budgets) == 1 else (0,)):
                p = sd.filtfilt_plan(m, sd.IIR_LP, a_c, None, gain, prec, "odd", None, 0, ws << 20)
                p.set_variant(v)
                plans[f"v{v} ws {ws or 'default'}"] = p
        P = next(iter(plans.values())).padlen
        model = channels * (4 * L * rs + 4 * P * rs)
        fns = {k: (lambda p=p: p.process(x)) for k, p in plans.items()}
        if not a.no_composition:
            s = torch.from_numpy(sd.iir_steady_state(m, sd.IIR_LP, a_c, None, gain)).to(device="cuda", dtype=dt)
            iir = C.c_void_p()
            sd._lib.check(lib.sdsp_hip_iir_plan_create(C.byref(iir), m, sd.IIR_LP, a_c.ctypes.data, None, gain, prec, 0))

            def make_compose(Pc):
                def compose():
                    x0, xl = x[:, :1], x[:, -1:]
                    e = torch.cat([2 * x0 - x[:, 1:Pc + 1].flip(1), x, 2 * xl - x[:, L - 1 - Pc:L - 1].flip(1)], dim=1)
                    N = L + 2 * Pc
                    st = (s[:, None] * e[:, 0][None, :]).repeat_interleave(3, dim=0)
                    stream = torch.cuda.current_stream().cuda_stream
                    sd._lib.check(lib.sdsp_hip_iir_process(iir, e.data_ptr(), channels, N, N, st.data_ptr(), stream))
                    u = e.flip(1)
                    st = (s[:, None] * u[:, 0][None, :]).repeat_interleave(3, dim=0)
                    sd._lib.check(lib.sdsp_hip_iir_process(iir, u.data_ptr(), channels, N, N, st.data_ptr(), stream))
                    x.copy_(u.flip(1)[:, Pc:Pc + L])
                return compose

            fns["composition"] = make_compose(P)
            Pa = P
            while (L + 2 * Pa) * rs % 16:
                Pa += 1
            if Pa != P:
                fns[f"composition P={Pa}"] = make_compose(Pa)
        times = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k, fn in fns.items():
                times[k].append(timed(fn, a.warmup, a.steps))
        parts = []
        base = None
        for k, t in times.items():
            ms = statistics.median(t)
            base = base or ms
            s_ = f"{k} {ms:8.3f} ms (spread {max(t) / min(t):.3f}, {100 * model / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s"
            if k in plans:
                s_ += f", {plans[k].launches(channels, L)} launches, {plans[k].info()['kernel']}"
            if k not in plans or k.startswith("v1"):
                s_ += f", v0 {ms / base:.2f}x faster"
            parts.append(s_ + ")")
        print(f"== {name}: {precision} {channels} x {L}, M {m}, P {P}, model {model / 1e9:.2f} GB | " + " | ".join(parts), flush=True)
        del plans, fns, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
