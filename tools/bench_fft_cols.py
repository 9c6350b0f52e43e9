#!/usr/bin/env python3
"""Column FFT plans against what a user has without them, in one process, alternating:
variant 0 COMPLEX in place; variant 0 POWER with a Hann window (out of place); variant 1, the plain sum in double, on `--plain-cubes`
cubes and scaled to the shape;
(a) torch transpose -> FftPlan.exec on the contiguous rows -> transpose back (three reads and three writes of the cube), and for the
    POWER case the window product in front and abs() ** 2 behind as passes of their own;
(b) torch.fft.fft(x, dim=-2), and for the POWER case torch.fft.fft(x * w, dim=-2).abs() ** 2.
Shapes (f32, and f64 at the first): 64 cubes x n x 8192 for n in {16, 64, 256, 1024}; 4096 cubes x 64 x 256; 64 x 256 x 8200 beside
64 x 256 x 8192, to show what a power-of-two row pitch costs down a column.  Device events around `--steps` calls after `--warmup`;
`--repeats` alternating rounds, median and spread (max / min).  Shares are of 8 TB/s on the plan's algorithmic_bytes (the cube read
once and the output written once).  Ratios are other / variant 0 of the same output kind; a ratio below 1 -- variant 0 loses -- is
set in bold (**..**).  No target is asserted.

  python tools/bench_fft_cols.py [--warmup 2] [--steps 5] [--repeats 3] [--plain-cubes 2] [--out profiles/fft_cols_bench.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK_BYTES = 8e12
SHAPES = [("f64", 64, 16, 8192), ("f32", 64, 16, 8192), ("f32", 64, 64, 8192), ("f32", 64, 256, 8192), ("f32", 64, 1024, 8192),
          ("f32", 4096, 64, 256), ("f32", 64, 256, 8200)]


def timed(fn, warmup, steps, reset):
    reset()  # the in-place calls grow the data by sqrt(n) each: start every measurement from the same finite random cube
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


def rounds(a, fns, reset):
    """median and spread of every function over alternating rounds"""
    t = [[] for _ in fns]
    for _ in range(a.repeats):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, a.warmup, a.steps, reset))
    return [(statistics.median(v), max(v) / min(v)) for v in t]


def ratio(other, own):
    r = other / own
    return f"{r:6.2f}x" if r >= 1.0 else f"**{r:.2f}x**"


def shape(a, precision, batch, n, width, log):
    f64 = precision == "f64"
    prec = sd.F64 if f64 else sd.F32
    real = torch.float64 if f64 else torch.float32
    x = torch.view_as_complex(torch.randn((batch, n, width, 2), device="cuda", dtype=real))
    x0 = x.clone()
    pw = torch.empty((batch, n, width), device="cuda", dtype=real)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    wd = torch.from_numpy(w).to(real).cuda()[:, None]
    cx = sd.FftColsPlan(n, width, precision=prec)
    dop = sd.FftColsPlan(n, width, precision=prec, output="power", window=w)
    pb = min(batch, a.plain_cubes)
    plain = sd.FftColsPlan(n, width, precision=prec)
    plain.set_variant(1)
    xp = x[:pb].clone()

    def reset():
        x.copy_(x0)
        xp.copy_(x0[:pb])
    rows = sd.FftPlan(n, 0, sd.forward_fft, prec, max_batch=batch * width)

    def transposed():
        t = x.transpose(-1, -2).contiguous()
        rows.exec(t)
        x.copy_(t.transpose(-1, -2))

    def transposed_power():
        t = (x * wd).transpose(-1, -2).contiguous()
        rows.exec(t)
        pw.copy_((t.abs() ** 2).transpose(-1, -2))

    fns = [lambda: cx.exec(x), lambda: dop.exec(x, pw), lambda: plain.exec(xp), transposed, transposed_power,
           lambda: torch.fft.fft(x, dim=-2), lambda: (torch.fft.fft(x * wd, dim=-2).abs() ** 2)]
    res = rounds(a, fns, reset)
    (m0, s0), (m1, s1), (mp, sp), (ma, sa), (map_, sap), (mb, sb), (mbp, sbp) = res
    mp *= batch / pb
    i0, i1 = cx.info(), dop.info()
    share = lambda info, ms: 100 * batch * info["algorithmic_bytes"] / (ms * 1e-3) / PEAK_BYTES  # noqa: E731
    head = f"  {precision} {batch:5d} x {n:5d} x {width:5d} ({batch * i0['algorithmic_bytes'] / 2 / 2 ** 30:5.2f} GiB, tile {i0['tile_columns']}, {i0['threads']} threads, lds {i0['lds_bytes']})"
    lines = [
        f"{head}: complex in place {m0:8.3f} ms (spread {s0:.3f}) {share(i0, m0):5.1f} % of 8 TB/s  |  variant 1 on {pb} cubes, scaled "
        f"{mp:10.3f} ms (spread {sp:.3f}) {ratio(mp, m0)}  |  (a) transpose, rows, transpose {ma:8.3f} ms (spread {sa:.3f}) {ratio(ma, m0)}"
        f"  |  (b) torch.fft.fft(dim=-2) {mb:8.3f} ms (spread {sb:.3f}) {ratio(mb, m0)}",
        f"{' ' * len(head)}: window + power   {m1:8.3f} ms (spread {s1:.3f}) {share(i1, m1):5.1f} % of 8 TB/s  |  (a) with window and "
        f"abs() ** 2 passes {map_:8.3f} ms (spread {sap:.3f}) {ratio(map_, m1)}  |  (b) fft(x * w).abs() ** 2 {mbp:8.3f} ms "
        f"(spread {sbp:.3f}) {ratio(mbp, m1)}",
    ]
    for line in lines:
        print(line, flush=True)
        log.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plain-cubes", type=int, default=2)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "fft_cols_bench.txt"))
    a = ap.parse_args()
    log = ["# tools/bench_fft_cols.py " + " ".join(sys.argv[1:]),
           "# ratios: other / variant 0 of the same output kind; bold = variant 0 loses"]
    for precision, batch, n, width in SHAPES:
        shape(a, precision, batch, n, width, log)
        Path(a.out).write_text("\n".join(log) + "\n")  # after every shape: a cut-short run keeps what it measured
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
