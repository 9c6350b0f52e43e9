#!/usr/bin/env python3
"""CFAR detector bank against what a user has without it, in one process, alternating:
(a) variant 1, the plain one-thread-per-output kernel (2 L global reads per output; OS: selection by counting in O(L^2)).  It runs on
    a slice of at most `--slice-elems` / (2 L) outputs and its time is scaled to the whole shape;
(b) CA and GO in torch: `avg_pool1d(p, L, 1) * L` as the side sums, shifted slices for lag, lead and the cell under test, the
    combination, the product and the comparison, on a slice of at most `--pool-elems` samples, scaled;
(c) OS in torch: `p.unfold(-1, W, 1)`, the 2 L training columns gathered by slicing, `kthvalue(k + 1, -1)`, the product and the
    comparison, on a slice of at most `--slice-elems` / (2 L) outputs (kthvalue materialises the gathered view), scaled.
The other form a user reaches for, differences of a shifted `cumsum`, is left out: on rows of 2^23 f32 samples the prefix sums reach
10^7, where an f32 step is 1, so the difference of two of them is off by about one on a sum of eight powers of mean one: it does not
compute the same detector;
`avg_pool1d` sums each window on its own, as the bank does.
I/Q shapes give the baselines the complex rows, so (b) and (c) include `re re + im im`.  Two rank_filter_bank passes plus a torch merge
are not a comparison here: the element of rank k of the union of two windows is not a function of one order statistic of each side,
except for k = 0 and k = 2 L - 1, which are not the ranks a detector uses.
Shapes: `--channels` x 4032 samples (very many short rows) and 16 x 2^23 (a few very long ones), f32 and f64, POWER and IQ, at
(L, G) in {(8, 2), (16, 2), (32, 4), (128, 8)}, for CA, GO and OS at the default rank (OS where 2 L fits the register limits).  Device
events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min).  The torch baselines
have no history: they produce S - W + 1 outputs per row and are scaled by outputs.

Model: per output the input element, one threshold and one decision byte (f32 POWER: 4 + 4 + 1 bytes), as a share of 8 TB/s; the
additions of variant 0 (L per output) or its passes (2 passes of `--ops32` (3) vector instructions per array element with 32-bit keys,
`--ops64` (8) with 64-bit keys, WP elements) as a share of 1.23e12 wave instructions per second.  A line where
variant 0 is slower than a comparison is marked LOSES.

  python tools/bench_cfar.py [--channels 262144] [--geometries 8:2,16:2,32:4,128:8] [--modes ca,go,os] [--precisions f32,f64]
                             [--inputs power,iq] [--no-long] [--warmup 2] [--steps 5] [--repeats 3] [--out profiles/cfar_bench.txt]
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
ALPHA = 5.0


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


def power(x):
    return x.real * x.real + x.imag * x.imag if x.is_complex() else x


def torch_sums(x, L, G, mode):
    """(b): CA or GO over rows without history; S - W + 1 outputs per row"""
    W, D, half = 2 * (L + G) + 1, L + 2 * G + 1, L + G
    p = power(x)
    box = torch.nn.functional.avg_pool1d(p.unsqueeze(1), L, 1).squeeze(1) * L  # box[j] = p[j .. j + L - 1]
    n_out = p.shape[1] - W + 1
    lag, lead = box[:, :n_out], box[:, D:D + n_out]
    v = lag + lead if mode == "ca" else torch.maximum(lag, lead)
    thr = v * (ALPHA / (2 * L) if mode == "ca" else ALPHA / L)
    return thr, (p[:, half:half + n_out] > thr).to(torch.uint8)


def torch_os(x, L, G, k):
    """(c): OS over rows without history; S - W + 1 outputs per row"""
    W, half = 2 * (L + G) + 1, L + G
    p = power(x)
    win = p.unfold(-1, W, 1)
    cells = torch.cat([win[..., :L], win[..., W - L:]], dim=-1)
    thr = cells.kthvalue(k + 1, -1).values * ALPHA
    return thr, (p[:, half:half + thr.shape[1]] > thr).to(torch.uint8)


def shape(a, C, S, L, G, mode, precision, kind, x, thr, det, log):
    f64 = precision == "f64"
    W = 2 * (L + G) + 1
    prec = sd.F64 if f64 else sd.F32
    if mode == "os" and 2 * L > (127 if f64 else 255):
        line = f"  {C:7d} x {S:8d}  {precision} {kind:5s} {mode} L {L:3d} G {G:2d}: n/a (2 L = {2 * L} is past the register limit of OS)"
        print(line, flush=True)
        log.append(line)
        return
    bank = sd.cfar_bank(C, L, G, mode, alpha=ALPHA, input=kind, precision=prec)
    k = bank.rank
    pc, ps = slice_shape(C, S, a.slice_elems // (2 * L))
    plain = sd.cfar_bank(pc, L, G, mode, alpha=ALPHA, input=kind, precision=prec)
    plain.set_variant(1)
    xs = x[:pc, :ps].contiguous()
    ts, ds = thr[:pc, :ps].contiguous(), det[:pc, :ps].contiguous()
    fns = [lambda: bank.process(x, thr=thr, det=det), lambda: plain.process(xs, thr=ts, det=ds)]
    if mode == "os":
        tc, tl = pc, ps
        xt = xs
        base = lambda: torch_os(xt, L, G, k)  # noqa: E731
        name = "(c) unfold.kthvalue"
    else:
        tc, tl = slice_shape(C, S, a.pool_elems)
        xt = x[:tc, :tl].contiguous()
        base = lambda: torch_sums(xt, L, G, mode)  # noqa: E731
        name = "(b) avg_pool1d sums"
    have_base = tl >= W and usable(base)
    if have_base:
        fns.append(base)
    res = rounds(a, fns)
    ms, s0 = res[0]
    outputs = C * S
    mp, s1 = res[1][0] * outputs / (pc * ps), res[1][1]
    info = bank.info()
    es = 8 if f64 else 4
    model = outputs * (es * (2 if kind == "iq" else 1) + es + 1)
    if mode == "os":
        instr = outputs * 2 * info["padded"] * (a.ops64 if f64 else a.ops32) / 64
        what = f"WP {info['padded']:3d} passes"
    else:
        instr = outputs * L / 64
        what = "additions"
    lost = ["(a)"] if mp < ms else []
    line = (f"  {C:7d} x {S:8d}  {precision} {kind:5s} {mode} L {L:3d} G {G:2d} run {info['last_run']:5d}: {ms:9.3f} ms (spread {s0:.3f})  "
            f"{outputs / (ms * 1e-3) / 1e12:6.3f} T outputs/s  model {model / 1e9:6.3f} GB -> "
            f"{100 * model / (ms * 1e-3) / PEAK_BYTES:5.1f} % of 8 TB/s  {what} -> "
            f"{100 * instr / (ms * 1e-3) / PEAK_WAVE_INSTR:5.1f} % of the VALU issue rate  |  (a) plain on {pc} x {ps}, scaled "
            f"{mp:11.3f} ms (spread {s1:.3f}) -> {mp / ms:8.2f}x")
    if have_base:
        mt, s2 = res[2][0] * outputs / (tc * (tl - W + 1)), res[2][1]
        line += f"  |  {name} on {tc} x {tl}, scaled {mt:11.3f} ms (spread {s2:.3f}) -> {mt / ms:8.2f}x"
        lost += [name[:3]] if mt < ms else []
    else:
        line += f"  |  {name[:3]} n/a"
    if lost:
        line += "  LOSES to " + ", ".join(lost)
    print(line, flush=True)
    log.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=262144)
    ap.add_argument("--samples", type=int, default=4032)
    ap.add_argument("--geometries", default="8:2,16:2,32:4,128:8")
    ap.add_argument("--modes", default="ca,go,os")
    ap.add_argument("--precisions", default="f32,f64")
    ap.add_argument("--inputs", default="power,iq")
    ap.add_argument("--no-long", action="store_true")
    ap.add_argument("--slice-elems", type=int, default=1 << 26)
    ap.add_argument("--pool-elems", type=int, default=1 << 26)
    ap.add_argument("--ops32", type=float, default=3.0)
    ap.add_argument("--ops64", type=float, default=8.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "cfar_bench.txt"))
    a = ap.parse_args()
    log = ["# tools/bench_cfar.py " + " ".join(sys.argv[1:])]
    cases = [(a.channels, a.samples)] + ([] if a.no_long else [(16, 1 << 23)])
    geometries = [tuple(int(v) for v in g.split(":")) for g in a.geometries.split(",")]
    for precision in a.precisions.split(","):
        f64 = precision == "f64"
        real = torch.float64 if f64 else torch.float32
        for kind in a.inputs.split(","):
            for C, S in cases:
                head = f"== {C} rows x {S} samples, {precision}, {kind}"
                print(head, flush=True)
                log.append(head)
                if kind == "iq":
                    x = torch.view_as_complex(torch.randn((C, S, 2), device="cuda", dtype=real))
                else:
                    x = torch.empty((C, S), device="cuda", dtype=real).exponential_()
                thr = torch.empty((C, S), device="cuda", dtype=real)
                det = torch.empty((C, S), device="cuda", dtype=torch.uint8)
                for L, G in geometries:
                    for mode in a.modes.split(","):
                        shape(a, C, S, L, G, mode, precision, kind, x, thr, det, log)
                        Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured
                del x, thr, det
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
