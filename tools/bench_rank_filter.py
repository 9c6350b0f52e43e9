#!/usr/bin/env python3
"""Rank-order filter bank against what a user has without it, in one process, alternating:
(a) variant 1, the plain one-thread-per-output kernel that selects by counting in O(W^2).  It is slow, so it runs on a slice of at
    most `--slice-elems` / W outputs and its time is scaled to the whole shape;
(b) `x.unfold(-1, W, 1).kthvalue(r + 1, -1)` in torch on a slice of at most `--slice-elems` / W outputs (the unfolded view is
    materialised by kthvalue: W times the slice), scaled;
(c) for the running minimum, `-max_pool1d(-x, W, 1)` in torch on a slice of at most `--pool-elems` samples, scaled.
Shapes: `--channels` x 4032 samples (very many short rows) and 16 x 2^23 (a few very long ones), f32 and f64; the median of
W in {3, 5, 9, 31, 63, 255 (f64: 127)} and the minimum at W = 31.  Device events around `--steps` calls after `--warmup`;
`--repeats` alternating rounds, median and spread (max / min).  The baselines (b) and (c) have no history: they produce S - W + 1
outputs per row and are scaled by outputs.

Model: one element read and one written per output (8 bytes in f32, 16 in f64), as a share of 8 TB/s; the pass of variant 0 as
`--ops32` (3: compare, select, median of three) vector instructions per array element and output with 32-bit keys and `--ops64` (8) with 64-bit keys, WP elements per
output, as a share of 1.23e12 wave instructions per second.  A line where variant 0 is slower than a baseline
is marked LOSES.

  python tools/bench_rank_filter.py [--channels 262144] [--windows 3,5,9,31,63,255] [--precisions f32,f64] [--no-long]
                                    [--warmup 2] [--steps 5] [--repeats 3] [--out profiles/rank_filter_bench.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK_BYTES = 8e12
PEAK_WAVE_INSTR = 1.23e12


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
    """median and spread of every function over alternating rounds"""
    t = [[] for _ in fns]
    for _ in range(a.repeats):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, a.warmup, a.steps))
    return [(statistics.median(v), max(v) / min(v)) for v in t]


def usable(fn):
    """whether a torch baseline runs at all for this dtype and shape (it is left out, and said so, where it does not)"""
    try:
        fn()
        torch.cuda.synchronize()
        return True
    except (RuntimeError, NotImplementedError):
        return False


def slice_shape(C, S, elems):
    """(rows, samples) of a slice of about `elems` elements: whole rows while they fit, else the head of one row"""
    ps = min(S, max(elems, 1))
    pc = max(1, min(C, elems // ps))
    return pc, ps


def shape(a, C, S, W, rank, precision, x, y, log):
    f64 = precision == "f64"
    r = {"median": (W - 1) // 2, "min": 0}[rank]
    bank = sd.rank_filter_bank(C, W, r, sd.F64 if f64 else sd.F32)
    pc, ps = slice_shape(C, S, a.slice_elems // W)
    plain = sd.rank_filter_bank(pc, W, r, sd.F64 if f64 else sd.F32)
    plain.set_variant(1)
    xs = x[:pc, :ps].contiguous()
    ys = torch.empty_like(xs)
    fns = [lambda: bank.process(x, y=y), lambda: plain.process(xs, y=ys)]
    tc, ts = pc, ps
    kth = lambda: xs.unfold(-1, W, 1).kthvalue(r + 1, -1).values  # noqa: E731
    have_kth = ps >= W and usable(kth)
    if have_kth:
        fns.append(kth)
    qc, qs = slice_shape(C, S, a.pool_elems)
    if rank == "min" and qs >= W:
        xq = x[:qc, :qs].contiguous()
        pool = lambda: -torch.nn.functional.max_pool1d(-xq, W, 1)  # noqa: E731
        if usable(pool):
            fns.append(pool)
    res = rounds(a, fns)
    ms, s0 = res[0]
    outputs = C * S
    mp, s1 = res[1][0] * outputs / (pc * ps), res[1][1]
    info = bank.info()
    es = 8 if f64 else 4
    model = 2 * outputs * es
    instr = outputs * info["padded"] * (a.ops64 if f64 else a.ops32) / 64
    lost = ["(a)"] if mp < ms else []
    line = (f"  {C:7d} x {S:8d}  {precision} {rank:6s} W {W:3d} WP {info['padded']:3d} run {info['last_run']:5d}: {ms:9.3f} ms "
            f"(spread {s0:.3f})  {outputs / (ms * 1e-3) / 1e12:6.3f} T outputs/s  model {model / 1e9:6.3f} GB -> "
            f"{100 * model / (ms * 1e-3) / PEAK_BYTES:5.1f} % of 8 TB/s  pass -> {100 * instr / (ms * 1e-3) / PEAK_WAVE_INSTR:5.1f} % of the "
            f"VALU issue rate  |  (a) plain on {pc} x {ps}, scaled {mp:11.3f} ms (spread {s1:.3f}) -> {mp / ms:8.2f}x")
    k = 2
    if have_kth:
        mt, s2 = res[k][0] * outputs / (tc * (ts - W + 1)), res[k][1]
        line += f"  |  (b) unfold.kthvalue on {tc} x {ts}, scaled {mt:11.3f} ms (spread {s2:.3f}) -> {mt / ms:8.2f}x"
        lost += ["(b)"] if mt < ms else []
        k += 1
    else:
        line += "  |  (b) n/a"
    if k < len(res):
        mq, s3 = res[k][0] * outputs / (qc * (qs - W + 1)), res[k][1]
        line += f"  |  (c) -max_pool1d(-x) on {qc} x {qs}, scaled {mq:9.3f} ms (spread {s3:.3f}) -> {mq / ms:6.2f}x"
        lost += ["(c)"] if mq < ms else []
    if lost:
        line += "  LOSES to " + ", ".join(lost)
    print(line, flush=True)
    log.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=262144)
    ap.add_argument("--samples", type=int, default=4032)
    ap.add_argument("--windows", default="3,5,9,31,63,255")
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--no-long", action="store_true")
    ap.add_argument("--slice-elems", type=int, default=1 << 26)
    ap.add_argument("--pool-elems", type=int, default=1 << 26)
    ap.add_argument("--ops32", type=float, default=3.0)
    ap.add_argument("--ops64", type=float, default=8.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "rank_filter_bench.txt"))
    a = ap.parse_args()
    log = ["# tools/bench_rank_filter.py " + " ".join(sys.argv[1:])]
    cases = [(a.channels, a.samples)] + ([] if a.no_long else [(16, 1 << 23)])
    for precision in a.precisions.split(","):
        f64 = precision == "f64"
        for C, S in cases:
            head = f"== {C} rows x {S} samples, {precision}"
            print(head, flush=True)
            log.append(head)
            x = torch.randn((C, S), device="cuda", dtype=torch.float64 if f64 else torch.float32)
            y = torch.empty_like(x)
            todo = [(min(int(w), 127 if f64 else 255), "median") for w in a.windows.split(",")] + [(31, "min")]
            for W, rank in todo:
                shape(a, C, S, W, rank, precision, x, y, log)
                Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
