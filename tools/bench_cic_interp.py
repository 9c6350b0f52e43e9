#!/usr/bin/env python3
"""CIC interpolator bank against what a user has without it, in one process, alternating:
(a) variant 1, the plain kernel: one output per thread as the direct polyphase sum over at most N M taps of boxcar(R M)^N;
(b) the torch composition a user writes today: the samples widened to int64, N x subtraction of the sequence shifted by M,
    zero-stuffing by R, N x torch.cumsum.  It holds several int64 copies of the output, so it runs on the first rows only (as many
    as keep one copy at 2^28 values) and its time is scaled to the whole shape; the line says which share of the rows it ran on;
(c) the float path: convert to f32, then duc_bank at zero frequency (complex rows; at most 65536 rows, scaled likewise) or
    fir_resampler(R, 1) (real rows) with the boxcar(R M)^N taps scaled to unity gain -- where those fit: at most 4096 taps and
    R <= 1024.  The conversion is inside the timed region: it is what the integer input costs a user of the float banks.
Two cases, both for I16 complex rows and I32 real rows of 24 significant bits: 16 streams x 2^23 outputs at (N, R, M) = (3, 16, 1),
(5, 64, 1), (5, 1024, 1), (3, 4096, 2), and `--bank-rows` x 4032 outputs at (3, 8, 1).  Device events around `--steps` calls after
`--warmup`; `--repeats` alternating rounds, median and spread (max / min).

Model bytes of the bank: in bytes + out bytes = (S element size + R S output element size) per row; share = model bytes / time /
8 TB/s.  Adds: 2 (N - 1) per output and plane (a lane-local running sum and the offset, per scan stage; the first integrator is a
hold and costs none).

  python tools/bench_cic_interp.py [--cases stream,bank] [--bank-rows N] [--out int|f32] [--warmup 2] [--steps 5] [--repeats 3] [--no-plain]
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
STREAM_SHAPES = [(3, 16, 1), (5, 64, 1), (5, 1024, 1), (3, 4096, 2)]
BANK_SHAPES = [(3, 8, 1)]
KINDS = [("i16", "complex", 16), ("i32", "real", 24)]


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


def rounds(a, fns):
    """median and spread of every function over alternating rounds; None stays None"""
    t = [[] for _ in fns]
    for _ in range(a.repeats):
        for i, fn in enumerate(fns):
            if fn is not None:
                t[i].append(timed(fn, a.warmup, a.steps))
    return [(statistics.median(v), max(v) / min(v)) if v else None for v in t]


def call(bank, x, out):
    def fn():
        bank.process(x, out=out)
    return fn


def torch_form(N, R, M, x):
    """(fn, share): composition (b) on the first rows of x"""
    S = x.shape[1]
    per_row = x[0].numel() * R
    rows = max(1, min(x.shape[0], (1 << 28) // per_row))
    xs = x[:rows]

    def fn():
        v = xs.to(torch.int64)
        for _ in range(N):
            v = torch.cat([v[:, :M], v[:, M:] - v[:, :-M]], dim=1)
        u = torch.zeros((rows, S, R) + tuple(x.shape[2:]), device=x.device, dtype=torch.int64)
        u[:, :, 0] = v
        u = u.reshape((rows, S * R) + tuple(x.shape[2:]))
        for _ in range(N):
            u = torch.cumsum(u, dim=1)
        return u
    return fn, rows / x.shape[0]


def float_form(N, R, M, x, cplx):
    """(fn, share) of baseline (c), or None where its taps or its factor do not fit"""
    taps = N * (R * M - 1) + 1
    if taps > 4096 or R > 1024:
        return None
    h = sd.cic_taps(N, R, M).astype(np.float64) * sd.cic_interp_unity_scale(N, R, M)
    if cplx:
        rows = min(x.shape[0], 65536)
        bank = sd.duc_bank(taps, R, [(c, 0.0) for c in range(rows)], rows, "complex")
        bank.set_coeff(h)
        out = torch.empty((rows, x.shape[1] * R), device="cuda", dtype=torch.complex64)
        xs = x[:rows]

        def fn():
            return bank.process(torch.view_as_complex(xs.to(torch.float32)), out=out)
        return fn, rows / x.shape[0]
    bank = sd.fir_resampler(taps, R, 1, x.shape[0])
    bank.set_coeff(h)
    out = torch.empty((x.shape[0], x.shape[1] * R), device="cuda", dtype=torch.float32)

    def fn():
        return bank.process(x.to(torch.float32), out=out)
    return fn, 1.0


def shape(a, case, rows, outs, N, R, M, in_dtype, kind, bits):
    cplx = kind == "complex"
    tdt = torch.int32 if in_dtype == "i32" else torch.int16
    S = outs // R
    top = 1 << (bits - 1)
    x = torch.randint(-top, top, (rows, S, 2) if cplx else (rows, S), device="cuda", dtype=torch.int64).to(tdt)
    scan = sd.cic_interpolator(N, R, M, kind, in_dtype, bits, a.out)
    plain = sd.cic_interpolator(N, R, M, kind, in_dtype, bits, a.out)
    plain.set_variant(1)
    n = scan.out_samples(S)
    out = torch.empty((rows, n, 2) if cplx else (rows, n), device="cuda", dtype=scan._out_torch())
    comp, share_b = torch_form(N, R, M, x)
    try:
        flt = float_form(N, R, M, x, cplx)
        note_c = "does not fit (taps > 4096 or R > 1024)"
    except (sd.SdspHipError, ValueError) as e:
        flt, note_c = None, f"not measured: {e}"
    res = rounds(a, [call(scan, x, out), None if a.no_plain else call(plain, x, out), comp, flt[0] if flt else None])
    (ms, s0) = res[0]
    info = scan.info()
    planes = 2 if cplx else 1
    model = rows * (S * x.element_size() + n * out.element_size()) * planes
    adds = rows * n * planes * 2 * (N - 1)
    line = (f"  {case:6s} {rows:7d} rows {in_dtype} {kind:7s} N {N} R {R:4d} M {M} W {info['reg_bits']}: {ms:8.3f} ms (spread {s0:.3f})  model "
            f"{model / 1e9:6.3f} GB -> {100 * model / (ms * 1e-3) / PEAK:5.1f} % of 8 TB/s  {adds / (ms * 1e-3) / 1e12:6.2f} T adds/s")
    if res[1]:
        line += f"  |  (a) plain {res[1][0]:9.3f} ms (spread {res[1][1]:.3f}) -> {res[1][0] / ms:7.2f}x"
    mb = res[2][0] / share_b
    line += f"  |  (b) torch on {100 * share_b:.3g} % of the rows, scaled {mb:9.3f} ms (spread {res[2][1]:.3f}) -> {mb / ms:6.2f}x"
    if res[3]:
        mc = res[3][0] / flt[1]
        line += (f"  |  (c) f32 + {'duc_bank' if cplx else 'fir_resampler'} on {100 * flt[1]:.3g} % of the rows, scaled {mc:9.3f} ms "
                 f"(spread {res[3][1]:.3f}) -> {mc / ms:6.2f}x")
    else:
        line += f"  |  (c) {note_c}"
    print(line, flush=True)
    del scan, plain, comp, flt, x, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="stream,bank")
    ap.add_argument("--bank-rows", type=int, default=262144)
    ap.add_argument("--out", default="int", choices=["int", "f32"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-plain", action="store_true")
    a = ap.parse_args()
    sizes = {"stream": (16, 1 << 23, STREAM_SHAPES), "bank": (a.bank_rows, 4032, BANK_SHAPES)}
    for case in a.cases.split(","):
        rows, outs, shapes = sizes[case]
        print(f"== {case}: {rows} rows x {outs} outputs, out {a.out}", flush=True)
        for in_dtype, kind, bits in KINDS:
            for N, R, M in shapes:
                shape(a, case, rows, outs, N, R, M, in_dtype, kind, bits)


if __name__ == "__main__":
    main()
