#!/usr/bin/env python3
"""Reed-Solomon decoder banks: variant 0, the wave kernel, against variant 1, the plain kernel (a thread per
codeword, serial loops), in one process, alternating.

Codes: RS(255, 223) = (0x187, 112, 11, 32, 255) at I = 1 and I = 5, and the shortened RS(204, 188) = (0x11D, 0, 1, 16, 204) at I = 1.
Sizes: 2^20 codewords, and 4096, which underfills the chip.  Loads: every codeword clean; a symbol error rate of 10^-3 in bursts of
four consecutive bytes of the frame; every codeword with t errors; every codeword with t + 2 errors (uncorrectable).  The frames are a
pool of `--pool` encoded frames repeated, the errors of every codeword its own.  Full frames out of place, no erasure input, the counts
written.  Device events around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min).

Model: the frame read once and written once, as a share of 8 TB/s.  The decoder is not a memory-bound kernel: the second figure is the
share of the chip's issue rate (1.23 T wave-instructions/s) that the syndrome phase alone accounts for, at
the counted instructions per codeword of the wave kernel's syndrome loop (`--instr-per-4`, per four syndromes, from the device
assembly: profiles/rs_kernel_regs.txt).  Gbit/s counts decoded data bits (8 k per codeword), the figure to hold against the Viterbi
bank's 25.7 - 34.8 Gbit/s (profiles/viterbi_bench.txt).  A line where variant 0 is slower than variant 1 is marked LOSES.

  python tools/bench_rs.py [--sizes 1048576,4096] [--warmup 1] [--steps 3] [--repeats 3] [--out profiles/rs_bench.txt]
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
ISSUE = 1.23e12
CODES = [("RS(255,223) I=1", (0x187, 112, 11, 32, 255), 1), ("RS(255,223) I=5", (0x187, 112, 11, 32, 255), 5),
         ("RS(204,188) I=1", (0x11D, 0, 1, 16, 204), 1)]
LOADS = ["clean", "ser 1e-3 bursts", "t errors", "t + 2 errors"]


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


def clean_frames(a, params, interleave, frames):
    """(frames, I n) uint8 on the device: a pool of encoded frames, repeated"""
    n, k = params[4], params[4] - params[3]
    pool = min(a.pool, frames)
    data = np.random.default_rng(1).integers(0, 256, (pool, interleave * k), dtype=np.uint8)
    enc = torch.from_numpy(sd.rs_encode(data, *params, interleave=interleave)).cuda()
    return enc.repeat((frames + pool - 1) // pool, 1)[:frames].contiguous().view(frames, interleave * n)


def load(x, params, interleave, kind, gen):
    """the frames x (frames, I n) with the errors of a load"""
    n, t = params[4], params[3] // 2
    frames = x.shape[0]
    y = x.clone()
    if kind == "clean":
        return y
    if kind == "ser 1e-3 bursts":
        flat = y.view(-1)
        start = torch.rand(flat.numel(), device="cuda", generator=gen) < 2.5e-4
        hit = start.clone()
        for s in range(1, 4):
            hit[s:] |= start[:-s]
        flat ^= hit.to(torch.uint8) * torch.randint(1, 256, (flat.numel(),), device="cuda", generator=gen, dtype=torch.uint8)
        return y
    errors = t if kind == "t errors" else t + 2
    # positions base + 7 i mod n: distinct, since 7 is coprime to 255 and to 204
    v = y.view(frames, n, interleave)
    base = torch.randint(0, n, (frames, 1, interleave), device="cuda", generator=gen)
    pos = (base + 7 * torch.arange(errors, device="cuda").view(1, errors, 1)) % n
    val = torch.randint(1, 256, (frames, errors, interleave), device="cuda", generator=gen, dtype=torch.uint8)
    v.scatter_(1, pos, v.gather(1, pos) ^ val)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,4096", help="codewords per call")
    ap.add_argument("--pool", type=int, default=1024, help="encoded frames in the pool that a call's frames repeat")
    ap.add_argument("--instr-per-4", type=float, default=167.0, help="wave-instructions of the syndrome loop per four syndromes")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "rs_bench.txt"))
    a = ap.parse_args()
    log = [f"# tools/bench_rs.py --sizes {a.sizes} --pool {a.pool} --instr-per-4 {a.instr_per_4:g} --warmup {a.warmup} --steps {a.steps} "
           f"--repeats {a.repeats}"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261021)
    stream = torch.cuda.current_stream().cuda_stream
    for size in (int(v) for v in a.sizes.split(",")):
        for name, params, interleave in CODES:
            n, nroots = params[4], params[3]
            k = n - nroots
            frames = size // interleave
            words = frames * interleave
            head = f"== {name}: {words} codewords in {frames} frames of {interleave * n} bytes, full frames out of place, counts written"
            print(head, flush=True)
            log.append(head)
            x0 = clean_frames(a, params, interleave, frames)
            decs = []
            for variant in (0, 1):
                d = sd.rs_decoder(*params, interleave=interleave)
                d.set_variant(variant)
                decs.append(d)
            out = torch.empty_like(x0)
            cnt = torch.empty(words, dtype=torch.int32, device="cuda")
            for kind in LOADS:
                x = load(x0, params, interleave, kind, gen)
                fns = [lambda d=d: d.process_ptr(x.data_ptr(), None, out.data_ptr(), cnt.data_ptr(), frames, stream) for d in decs]
                res = rounds(a, fns)
                torch.cuda.synchronize()
                failed = int((cnt < 0).sum())
                fixed = int((cnt > 0).sum())
                (m0, s0), (m1, s1) = res
                model = 2 * words * n
                instr = a.instr_per_4 * ((nroots + 3) // 4)
                line = (f"  {words:8d} {kind:16s}: {m0:9.4f} ms (spread {s0:.3f}) = {words * k * 8 / (m0 * 1e-3) / 1e9:8.2f} Gbit/s decoded, "
                        f"{model / 1e6:7.2f} MB -> {100 * model / (m0 * 1e-3) / PEAK_BYTES:5.2f} % of 8 TB/s, syndromes {100 * words * instr / (m0 * 1e-3) / ISSUE:5.1f} % "
                        f"of issue at {instr:g} instr/codeword  |  plain {m1:9.4f} ms (spread {s1:.3f}) -> {m1 / m0:6.2f}x"
                        f"  |  {fixed} corrected, {failed} beyond the code")
                if m1 < m0:
                    line += "  LOSES to plain"
                print(line, flush=True)
                log.append(line)
                Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured
                del x
            for d in decs:
                d.close()
            del x0, out, cnt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
