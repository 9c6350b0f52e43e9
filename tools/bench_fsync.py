#!/usr/bin/env python3
"""Frame synchroniser banks: variant 0, the staged kernels over a packed working row, against variant 1, the
plain kernel (a thread per channel, bit by bit), and against the torch composition a user has without the bank, in one process,
alternating.

Frame: the CCSDS one, a 32-bit marker 0x1ACFFC1D in front of 1275 bytes (RS(255, 223) at I = 5), L = 10232 bits; tol 2, verify 1,
flywheel 1, either polarity, the CCSDS pseudo-randomiser removed.  Shapes: 4096 rows x 2^20 bits and 262144 rows x 32768 bits.  Loads:
"locked": clean frames from a random offset per row, random payloads; "search": random bits without a marker, so the machine stays in
SEARCH for the whole row.  Inputs: "packed" words and "bytes".  Every call starts from a reset state; the reset is outside the timed window.
Device events around each of `--steps` calls after `--warmup` (`--plain-steps` for variant 1 and for torch, whose calls take long on
the long rows); `--repeats` alternating rounds, median and spread (max / min).

The torch composition, on the bytes input in pieces of `--torch-rows` rows: a +-1 conv1d with the marker gives the correlation at every
position, a comparison the hits; for "locked" the payload bits are then gathered at the known offsets (which the bank has to find),
multiplied by the bit weights, summed to bytes and XORed with pn.  It has no machine, no polarity and no split invariance.

Model: the input read once and the frames written once, as a share of 8 TB/s; positions/s counts the bit positions examined (rows x
bits).  A line where variant 0 is slower than what it is compared with is marked LOSES.

  python tools/bench_fsync.py [--shapes 4096x1048576,262144x32768] [--warmup 1] [--steps 3] [--plain-steps 1] [--repeats 3]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import simpledsp_amd as sd  # noqa: E402

PEAK_BYTES = 8e12
M, P, TOL, V, F = 32, 1275, 2, 1, 1
L = M + 8 * P


def timed(fn, warmup, steps, before=None):
    """mean time of one call in ms: device events around every call, `before` (the bank's reset, synchronous) outside them"""
    total = 0.0
    for i in range(warmup + steps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            total += e0.elapsed_time(e1)
    return total / steps


def rounds(a, fns, steps, befores):
    """median and spread of every function over alternating rounds"""
    t = [[] for _ in fns]
    for _ in range(a.repeats):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, a.warmup, steps[i], befores[i]))
    return [(statistics.median(v), max(v) / min(v)) for v in t]


def make_rows(rows, nbits, locked, gen):
    """(rows, nbits) uint8 0 / 1 on the device, and the offset of the first marker of every row"""
    bits = torch.randint(0, 2, (rows, nbits), device="cuda", generator=gen, dtype=torch.uint8)
    offs = torch.randint(0, L, (rows,), device="cuda", generator=gen)
    if locked:
        marker = torch.tensor([(sd.CCSDS_ASM >> (M - 1 - i)) & 1 for i in range(M)], device="cuda", dtype=torch.uint8)
        frames = (nbits + L - 1) // L
        pos = offs[:, None, None] + L * torch.arange(frames, device="cuda")[None, :, None] + torch.arange(M, device="cuda")[None, None, :]
        ok = pos < nbits
        r = torch.arange(rows, device="cuda")[:, None, None].expand_as(pos)
        bits[r[ok], pos[ok]] = marker[None, None, :].expand_as(pos)[ok]
    return bits, offs


def pack(bits, piece=256):
    """(rows, nbits) 0 / 1 bytes -> (rows, nbits / 32) int32 words, the oldest bit lowest"""
    w = (1 << torch.arange(32, device="cuda", dtype=torch.int64))
    out = torch.empty((bits.shape[0], bits.shape[1] // 32), dtype=torch.int32, device="cuda")
    for r in range(0, bits.shape[0], piece):
        v = (bits[r:r + piece].view(-1, bits.shape[1] // 32, 32).to(torch.int64) * w).sum(dim=2)
        out[r:r + piece] = v.to(torch.int32)  # wraps to the low 32 bits
    return out


def torch_composition(a, bits, offs, locked, pn):
    """the conv1d correlation and, for locked rows, the pack at the known offsets; returns the function to time"""
    rows, nbits = bits.shape
    kernel = torch.tensor([1.0 - 2.0 * ((sd.CCSDS_ASM >> (M - 1 - i)) & 1) for i in range(M)], device="cuda").view(1, 1, M)
    frames = (nbits - L) // L  # whole frames behind every offset
    weights = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], device="cuda", dtype=torch.int32)
    body = M + torch.arange(8 * P, device="cuda")
    sink = {}

    def run():
        for r in range(0, rows, a.torch_rows):
            x = bits[r:r + a.torch_rows]
            corr = torch.nn.functional.conv1d((1.0 - 2.0 * x.to(torch.float32)).unsqueeze(1), kernel).squeeze(1)
            sink["hits"] = (corr >= M - 2 * TOL) | (corr <= -(M - 2 * TOL))
            if locked and frames > 0:
                idx = offs[r:r + a.torch_rows, None, None] + L * torch.arange(frames, device="cuda")[None, :, None] + body[None, None, :]
                got = torch.gather(x, 1, idx.view(x.shape[0], -1)).view(x.shape[0], frames, P, 8)
                sink["out"] = (got.to(torch.int32) * weights).sum(dim=3).to(torch.uint8) ^ pn
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x1048576,262144x32768", help="rows x bits, comma separated")
    ap.add_argument("--torch-rows", type=int, default=256, help="rows per piece of the torch composition at 2^20 bits (scaled to the row length)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--plain-steps", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "fsync_bench.txt"))
    a = ap.parse_args()
    log = [f"# tools/bench_fsync.py --shapes {a.shapes} --torch-rows {a.torch_rows} --warmup {a.warmup} --steps {a.steps} "
           f"--plain-steps {a.plain_steps} --repeats {a.repeats}"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261021)
    stream = torch.cuda.current_stream().cuda_stream
    pn_host = sd.ccsds_pn(P)
    pn = torch.from_numpy(pn_host).cuda()
    per_piece = a.torch_rows
    for shape in a.shapes.split(","):
        rows, nbits = (int(v) for v in shape.split("x"))
        a.torch_rows = max(1, per_piece * (1 << 20) // nbits)
        mf = sd.fsync_max_frames(M, P, nbits)
        head = f"== {rows} rows x {nbits} bits, marker {M} bits, {P} bytes (L = {L}), tol {TOL}, verify {V}, flywheel {F}, either polarity, pn"
        print(head, flush=True)
        log.append(head)
        out = torch.empty((rows, mf, P), dtype=torch.uint8, device="cuda")
        counts = torch.empty(rows, dtype=torch.int32, device="cuda")
        for load in ("locked", "search"):
            bits, offs = make_rows(rows, nbits, load == "locked", gen)
            words = pack(bits)
            for kind, src in (("packed", words), ("bytes", bits)):
                banks = []
                for variant in (0, 1):
                    b = sd.frame_sync_bank(sd.CCSDS_ASM, M, P, TOL, V, F, "either", pn_host, kind, max_channels=rows, max_bits=nbits)
                    b.set_variant(variant)
                    banks.append(b)
                state_bytes = banks[0].state_bytes()

                fns = [lambda b=b: b.process_ptr(src.data_ptr(), out.data_ptr(), counts.data_ptr(), None, None, rows, nbits, stream) for b in banks]
                befores = [b.reset for b in banks]
                steps = [a.steps, a.plain_steps]
                if kind == "bytes" and not a.no_torch:
                    fns.append(torch_composition(a, bits, offs, load == "locked", pn))
                    steps.append(a.plain_steps)
                    befores.append(None)
                try:
                    res = rounds(a, fns, steps, befores)
                except RuntimeError as ex:  # the composition ran out of memory or found no convolution: the bank's figures stay
                    note = f"  torch composition failed: {str(ex).splitlines()[0][:160]}"
                    print(note, flush=True)
                    log.append(note)
                    res = rounds(a, fns[:2], steps[:2], befores[:2])
                torch.cuda.synchronize()
                emitted = int(counts.sum())
                (m0, s0), (m1, s1) = res[:2]
                model = rows * (nbits // 8 if kind == "packed" else nbits) + emitted * P
                line = (f"  {load:6s} {kind:6s}: {m0:10.4f} ms (spread {s0:.3f}), {model / 1e6:9.2f} MB -> {100 * model / (m0 * 1e-3) / PEAK_BYTES:5.2f} % of "
                        f"8 TB/s, {rows * nbits / (m0 * 1e-3) / 1e9:8.2f} G positions/s, {emitted} frames, state {state_bytes / 1e6:.2f} MB  |  plain "
                        f"{m1:10.4f} ms (spread {s1:.3f}) -> {m1 / m0:7.2f}x")
                if m1 < m0:
                    line += "  LOSES to plain"
                if len(res) > 2:
                    m2, s2 = res[2]
                    line += f"  |  torch {m2:10.4f} ms (spread {s2:.3f}) -> {m2 / m0:7.2f}x"
                    if m2 < m0:
                        line += "  LOSES to torch"
                print(line, flush=True)
                log.append(line)
                Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured
                for b in banks:
                    b.close()
            del bits, words, offs
            torch.cuda.empty_cache()
        del out, counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
