#!/usr/bin/env python3
"""Viterbi decoder banks against what a user has without them, in one process, alternating:
(a) variant 1, the plain kernel: a workgroup of 64 threads per channel, the metrics in LDS with a barrier per step;
(b) torch: per step a gather of the two predecessor metrics over [channels, 64], the branch metrics by a small matrix product, add,
    compare and select, the decisions stacked; then a gathered traceback from the best end state.  About eight launches per step, so it
    is timed on a slice of at most `--torch-channels` channels by `--torch-steps` steps and scaled to the whole shape.  It is timed, not
    compared: its traceback is one walk over the slice, not the bank's blocks.
Shapes: 4096 channels x 65536 steps and 262144 x 4032, K = 7 (171, 133) and (171, 133, 165), int8 and float32 soft values, (B, D) =
(32, 64) and (128, 128), bytes out; a row is cut to whole blocks (4032 steps: 3968 at B = 128).  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and
spread (max / min).

Model: the soft values read and the bits written once, as a share of 8 TB/s.  The decoder is not a memory-bound kernel: the second
figure is its share of the chip's issue rate (1024 SIMDs x 1.2 G wave-instructions/s) at the counted
instructions per step of the wave kernel's inner loop (`--instr`, from the device assembly: DESIGN.md section 5.33).  A line where
variant 0 is slower than a comparison is marked LOSES.

  python tools/bench_viterbi.py [--shapes 4096:65536,262144:4032] [--warmup 1] [--steps 3] [--repeats 3] [--out profiles/viterbi_bench.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK_BYTES = 8e12
ISSUE = 1024 * 1.2e9
GENS = {2: (0o171, 0o133), 3: (0o171, 0o133, 0o165)}
SCALE = 32.0


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


def branch_signs(gens):
    """(64, n) float32 signs of the branches into state s from s >> 1 and from (s >> 1) + 32: +1 where the coded bit is 0"""
    out = []
    for add in (0, 32):
        rows = []
        for s in range(64):
            reg = (((s >> 1) + add) << 1) | (s & 1)
            rows.append([1.0 - 2.0 * (bin(reg & int(f"{g:07b}"[::-1], 2)).count("1") & 1) for g in gens])
        out.append(torch.tensor(rows, dtype=torch.float32, device="cuda"))
    return out


def torch_viterbi(q, sg0, sg1, p0, p1):
    """q: (channels, steps, n) float32 of quantised soft values (exact integers)"""
    channels, steps, _ = q.shape
    m = torch.zeros((channels, 64), dtype=torch.float32, device=q.device)
    dec = torch.empty((steps, channels, 64), dtype=torch.bool, device=q.device)
    for t in range(steps):
        qt = q[:, t, :]
        a0 = m[:, p0] + qt @ sg0.T
        a1 = m[:, p1] + qt @ sg1.T
        d = a1 > a0
        m = torch.where(d, a1, a0)
        dec[t] = d
    s = torch.argmax(m, dim=1)
    bits = torch.empty((steps, channels), dtype=torch.uint8, device=q.device)
    for t in range(steps - 1, -1, -1):
        bits[t] = (s & 1).to(torch.uint8)
        s = (s >> 1) + dec[t].gather(1, s[:, None]).squeeze(1).to(torch.int64) * 32
    return bits


def shape(a, channels, steps, n, in_kind, B, D, x, log):
    gens = GENS[n]
    banks = []
    for variant in (0, 1):
        b = sd.viterbi_bank(7, gens, B, D, in_kind, "bytes", scale=SCALE, max_channels=channels)
        b.set_variant(variant)
        banks.append(b)
    out = torch.empty((channels, steps), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    tc, ts = min(channels, a.torch_channels), min(steps, a.torch_steps)
    xs = x.view(channels, steps, n)[:tc, :ts, :]
    q = (torch.clamp(torch.round(xs.to(torch.float32) * (SCALE if in_kind == "f32" else 1.0)), -127, 127)).contiguous()
    sg0, sg1 = branch_signs(gens)
    p0 = torch.arange(64, device="cuda") >> 1
    p1 = p0 + 32
    fns = [lambda: banks[0].process_ptr(x.data_ptr(), out.data_ptr(), channels, steps, stream),
           lambda: banks[1].process_ptr(x.data_ptr(), out.data_ptr(), channels, steps, stream),
           lambda: torch_viterbi(q, sg0, sg1, p0, p1)]
    res = rounds(a, fns)
    ms, s0 = res[0]
    mp, s1 = res[1]
    mt, s2 = res[2][0] * (channels / tc) * (steps / ts), res[2][1]
    info = banks[0].info()
    bits = channels * steps
    model = bits * n * (4 if in_kind == "f32" else 1) + bits
    lost = (["(a)"] if mp < ms else []) + (["(b)"] if mt < ms else [])
    instr = a.instr3 if n == 3 else a.instr
    line = (f"  {channels:6d} x {steps:5d}  n = {n} {in_kind:3s} (B, D) = ({B:3d}, {D:3d}) chunk {info['chunk']:4d} waves {info['waves']} lds {info['lds_bytes']:6d}: "
            f"{ms:9.3f} ms (spread {s0:.3f}) = {bits / (ms * 1e-3) / 1e9:7.2f} Gbit/s decoded, {model / 1e9:6.3f} GB -> "
            f"{100 * model / (ms * 1e-3) / PEAK_BYTES:5.2f} % of 8 TB/s, {100 * bits * instr / (ms * 1e-3) / ISSUE:5.1f} % of issue at {instr:g} instr/step"
            f"  |  (a) plain {mp:9.3f} ms (spread {s1:.3f}) -> {mp / ms:6.2f}x"
            f"  |  (b) torch on {tc} x {ts}, scaled {mt:12.1f} ms (spread {s2:.3f}) -> {mt / ms:9.1f}x")
    if lost:
        line += "  LOSES to " + ", ".join(lost)
    print(line, flush=True)
    log.append(line)
    for b in banks:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096:65536,262144:4032")
    ap.add_argument("--tracebacks", default="32:64,128:128")
    ap.add_argument("--torch-channels", type=int, default=16384)
    ap.add_argument("--torch-steps", type=int, default=128)
    ap.add_argument("--instr", type=float, default=16.0, help="wave-instructions per step of the wave kernel's inner loop, n = 2")
    ap.add_argument("--instr3", type=float, default=18.6, help="the same for n = 3")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "viterbi_bench.txt"))
    a = ap.parse_args()
    log = [f"# tools/bench_viterbi.py --shapes {a.shapes} --tracebacks {a.tracebacks} --torch-channels {a.torch_channels} --torch-steps {a.torch_steps} "
           f"--warmup {a.warmup} --steps {a.steps} --repeats {a.repeats}"]
    for s in a.shapes.split(","):
        channels, steps = (int(v) for v in s.split(":"))
        for n in (2, 3):
            for in_kind in ("i8", "f32"):
                head = f"== {channels} channels x {steps} steps, K = 7, n = {n}, {in_kind}: a coded stream of random bits at +-40 with noise of sigma 30"
                print(head, flush=True)
                log.append(head)
                # a noisy coded stream (the decisions of pure noise are the same work, but this is what the bank is for): one row of
                # coded bits repeated over the channels, noise of its own per channel
                bits = torch.randint(0, 2, (steps,), dtype=torch.uint8).numpy()
                coded = torch.from_numpy(sd.conv_encode(bits, 7, GENS[n]).astype("float32")).cuda()
                x = torch.empty((channels, steps * n), dtype=torch.float32 if in_kind == "f32" else torch.int8, device="cuda")
                rows = max(1, (1 << 28) // (steps * n))
                for c0 in range(0, channels, rows):
                    c1 = min(channels, c0 + rows)
                    v = (1 - 2 * coded)[None, :] * 40 + 30 * torch.randn((c1 - c0, steps * n), device="cuda")
                    x[c0:c1] = (v / SCALE).to(torch.float32) if in_kind == "f32" else torch.clamp(torch.round(v), -127, 127).to(torch.int8)
                    del v
                for tb in a.tracebacks.split(","):
                    B, D = (int(v) for v in tb.split(":"))
                    whole = steps // B * B  # a call takes whole blocks: 4032 steps are 3968 at B = 128
                    xs = x if whole == steps else x[:, :whole * n].contiguous()
                    shape(a, channels, whole, n, in_kind, B, D, xs, log)
                    del xs
                    Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured
                del x
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
