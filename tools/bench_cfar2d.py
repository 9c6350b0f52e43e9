#!/usr/bin/env python3
"""2-D CFAR plans against what a user has without them, in one process, alternating:
(a) variant 1, the plain one-thread-per-cell kernel (every training cell read from global memory), on a slice of whole maps of at most
    `--slice-reads` / (window cells) cells, its time scaled to the whole shape;
(b) torch: the map padded circularly in Doppler and with zeros in range, the outer and the guard box sums by `avg_pool2d` times their
    areas, outer minus guard, the product with c(r), the comparison, and `nonzero` for the list; on a slice of whole maps of at most
    `--pool-cells` cells, scaled.  It subtracts where the plan adds, so its bits are not the plan's: it is timed, not compared;
(c) the 1-D `cfar_bank` (CA, train_r, guard_r) over the same maps x D rows with thr and det: the same bytes moved with a 1-D window,
    which is the floor for the thr+det form.
Shapes, f32: 64 maps x D x 8192 for D = 16, 64, 256, 1024 (the column plan bench's) and 4096 x 64 x 256.  Windows (Ld, Gd, Lr, Gr):
(4,1,8,2), (8,2,16,4), (2,1,32,4).  Outputs: thr+det, det only, and the list only, all at the table of pfa = 1e-4 on exponential noise.
Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min).

Model: one read of the map plus the outputs written (thr: one element per cell; det: one byte; list: the records and counts), as a
share of 8 TB/s.  A line where variant 0 is slower than a comparison is marked LOSES.

  python tools/bench_cfar2d.py [--shapes 64:16:8192,...] [--windows 4:1:8:2,...] [--warmup 2] [--steps 5] [--repeats 3]
                               [--out profiles/cfar2d_bench.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK_BYTES = 8e12
PFA = 1e-4
CAP = 1 << 16


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


def torch_cfar2d(p, win, c, kind):
    Ld, Gd, Lr, Gr = win
    Hd, Hr = Ld + Gd, Lr + Gr
    D, R = p.shape[-2:]
    F = torch.nn.functional
    q = torch.cat([p[:, D - Hd:], p, p[:, :Hd]], 1) if Hd else p
    q = F.pad(q, (Hr, Hr)).unsqueeze(1)
    outer = F.avg_pool2d(q, (2 * Hd + 1, 2 * Hr + 1), 1) * ((2 * Hd + 1) * (2 * Hr + 1))
    guard = F.avg_pool2d(q[:, :, Ld:Ld + D + 2 * Gd, Lr:Lr + R + 2 * Gr], (2 * Gd + 1, 2 * Gr + 1), 1) * ((2 * Gd + 1) * (2 * Gr + 1))
    thr = (outer - guard).squeeze(1) * c
    det = p > thr
    if kind == "list":
        return det.nonzero()
    return (thr, det.to(torch.uint8)) if kind == "thr+det" else det.to(torch.uint8)


def whole_maps(maps, cells_per_map, budget):
    return max(1, min(maps, budget // cells_per_map))


def shape(a, maps, D, R, win, p, log):
    Ld, Gd, Lr, Gr = win
    cells = maps * D * R
    if D < 2 * (Ld + Gd) + 1:
        line = f"  {maps:5d} x {D:4d} x {R:5d}  ({Ld},{Gd},{Lr},{Gr}): n/a (the window needs D >= {2 * (Ld + Gd) + 1})"
        print(line, flush=True)
        log.append(line)
        return
    wcells = (2 * (Ld + Gd) + 1) * (2 * (Lr + Gr) + 1) - (2 * Gd + 1) * (2 * Gr + 1)
    plan = sd.cfar2d_plan(D, R, (Ld, Lr), (Gd, Gr), pfa=PFA, edge="clip", max_maps=maps)
    pm = whole_maps(maps, D * R, a.slice_reads // wcells)
    plain = sd.cfar2d_plan(D, R, (Ld, Lr), (Gd, Gr), pfa=PFA, edge="clip", max_maps=pm)
    plain.set_variant(1)
    tm = whole_maps(maps, D * R, a.pool_cells)
    c = torch.from_numpy(plan.scale).to(device="cuda", dtype=p.dtype)
    bank = sd.cfar_bank(maps * D, Lr, Gr, "ca", alpha=5.0) if Lr else None
    rows = p.view(maps * D, R)
    thr, det = torch.empty_like(p), torch.empty(p.shape, dtype=torch.uint8, device="cuda")
    raw = torch.zeros((maps, CAP, 4), dtype=torch.int32, device="cuda")
    counts = torch.zeros((maps,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    info = plan.info()
    for kind in ("thr+det", "det", "list"):
        t_ptr = thr.data_ptr() if kind == "thr+det" else 0
        d_ptr = det.data_ptr() if kind != "list" else 0
        h_ptr, c_ptr = (raw.data_ptr(), counts.data_ptr()) if kind == "list" else (0, 0)
        fns = [lambda: plan.process_ptr(p.data_ptr(), t_ptr, d_ptr, h_ptr, c_ptr, CAP, maps, stream),
               lambda: plain.process_ptr(p.data_ptr(), t_ptr, d_ptr, h_ptr, c_ptr, CAP, pm, stream),
               lambda: torch_cfar2d(p[:tm], win, c, kind)]
        if kind == "thr+det" and bank is not None:
            fns.append(lambda: bank.process(rows, thr=thr.view(maps * D, R), det=det.view(maps * D, R)))
        res = rounds(a, fns)
        ms, s0 = res[0]
        mp, s1 = res[1][0] * maps / pm, res[1][1]
        mt, s2 = res[2][0] * maps / tm, res[2][1]
        hits = int(counts.to(torch.int64).sum().item()) if kind == "list" else 0
        model = cells * 4 + (cells * 4 if kind == "thr+det" else 0) + (cells if kind != "list" else hits * 16 + maps * 4)
        lost = (["(a)"] if mp < ms else []) + (["(b)"] if mt < ms else [])
        line = (f"  {maps:5d} x {D:4d} x {R:5d}  ({Ld},{Gd},{Lr},{Gr}) {kind:7s} tile {info['tile_rows']:2d} x {info['tile_cols']} lds {info['lds_bytes']:6d}: "
                f"{ms:8.3f} ms (spread {s0:.3f})  model {model / 1e9:6.3f} GB -> {100 * model / (ms * 1e-3) / PEAK_BYTES:5.1f} % of 8 TB/s"
                + (f"  {hits} hits" if kind == "list" else "")
                + f"  |  (a) plain on {pm} maps, scaled {mp:10.3f} ms (spread {s1:.3f}) -> {mp / ms:7.2f}x"
                f"  |  (b) torch on {tm} maps, scaled {mt:10.3f} ms (spread {s2:.3f}) -> {mt / ms:7.2f}x")
        if len(res) > 3:
            m1, s3 = res[3]
            line += f"  |  (c) 1-D cfar_bank {m1:8.3f} ms (spread {s3:.3f}) -> {m1 / ms:5.2f}x"
            lost += ["(c)"] if m1 < ms else []
        if lost:
            line += "  LOSES to " + ", ".join(lost)
        print(line, flush=True)
        log.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64:16:8192,64:64:8192,64:256:8192,64:1024:8192,4096:64:256")
    ap.add_argument("--windows", default="4:1:8:2,8:2:16:4,2:1:32:4")
    ap.add_argument("--slice-reads", type=int, default=1 << 32)
    ap.add_argument("--pool-cells", type=int, default=1 << 25)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "cfar2d_bench.txt"))
    a = ap.parse_args()
    log = [f"# tools/bench_cfar2d.py --shapes {a.shapes} --windows {a.windows} --warmup {a.warmup} --steps {a.steps} --repeats {a.repeats}"]
    for s in a.shapes.split(","):
        maps, D, R = (int(v) for v in s.split(":"))
        head = f"== {maps} maps x {D} x {R}, f32, exponential noise, table of pfa = {PFA}, edge = clip"
        print(head, flush=True)
        log.append(head)
        p = torch.empty((maps, D, R), device="cuda", dtype=torch.float32).exponential_()
        for w in a.windows.split(","):
            shape(a, maps, D, R, tuple(int(v) for v in w.split(":")), p, log)
            Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured
        del p
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
