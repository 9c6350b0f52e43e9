#!/usr/bin/env python3
"""LDPC decoder banks: variant 0, the wave kernel, against variant 1, the plain kernel (a thread per
codeword, messages in global memory), and against the same integer algorithm in torch (a gather per layer, vectorised over
codewords), in one process, alternating.

Codes, staircase codes from the test generator (tests/ldpc_ref.py, seed 1): (12 x 24, Z = 81), the 802.11n shape n = 1944 at rate
1/2; (4 x 24, Z = 81), rate 5/6; (12 x 24, Z = 27); (12 x 24, Z = 512), a large lift.  Sizes: 2^16 and 2^12 codewords.  Operating
points: clean input (every status 0); BPSK over AWGN at the Eb/N0 of `POINTS`, where early stop averages about 3 iterations; the same
noise with early stop off at 20 iterations.  int8 soft values in (scale 8), the k information bits as bytes and the status out,
norm 12, beta 0.  The codewords are a pool of `--pool` encoded words repeated, the noise of every codeword its own.  Device events
around `--steps` calls after `--warmup`; `--repeats` alternating rounds, median and spread (max / min).  The torch form iterates the
whole batch until every codeword passes (or 20 times), with the syndrome test of the contract; its results are compared with
variant 0's before it is timed.

Figures: decoded information bits per second; iterations x edges per second (the iterations each codeword ran, from its status);
the share of the chip's issue rate (1.23 T wave-instructions/s) that the layer loop accounts for, at the
counted instructions of its two passes per entry and wave piece (`--instr-per-entry`, from the device assembly:
profiles/ldpc_kernel_regs.txt) and with every codeword of a wave charged its own iterations, so a lower bound where codewords share
a wave; the model bytes (n in, k + 4 out) as a share of 8 TB/s.  A line where variant 0 is slower than variant 1 is marked LOSES.

  python tools/bench_ldpc.py [--sizes 65536,4096] [--warmup 1] [--steps 2] [--repeats 3] [--out profiles/ldpc_bench.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ldpc_ref as R  # noqa: E402
import simpledsp_amd as sd  # noqa: E402

PEAK_BYTES = 8e12
ISSUE = 1.23e12
SCALE, NORM, BETA, MAX_ITER = 8.0, 12, 0, 20
POINTS = [("12x24 Z=81", 12, 24, 81, 4.0), ("4x24 Z=81", 4, 24, 81, 4.0), ("12x24 Z=27", 12, 24, 27, 3.5), ("12x24 Z=512", 12, 24, 512, 4.7)]


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


class TorchDecoder:
    """the contract on torch tensors: one gather, a handful of elementwise kernels and one scatter per layer, all codewords at once"""

    def __init__(self, code):
        self.code = code
        self.var = [torch.from_numpy(v).cuda() for v in code.var]
        self.j = [torch.arange(d, device="cuda").view(1, d, 1) for d in code.degree]

    def passes(self, L):
        hard = L < 0
        bad = torch.zeros(L.shape[0], dtype=torch.bool, device="cuda")
        for v in self.var:
            bad |= (hard[:, v].sum(dim=1) & 1).any(dim=1)
        return ~bad

    def decode(self, q, early, max_iter):
        code = self.code
        L = q.to(torch.int32)
        cw = L.shape[0]
        msg = [torch.zeros((cw, d, code.z), dtype=torch.int32, device="cuda") for d in code.degree]
        ok = self.passes(L)
        status = torch.where(ok, 0, -1).to(torch.int32)
        for it in range(1, max_iter + 1):
            if early and bool(ok.all()):
                break
            live = ~ok if early else torch.ones_like(ok)
            for r, v in enumerate(self.var):
                T = L[:, v] - msg[r]
                a = T.abs().clamp_(max=127)
                sig = T < 0
                S = (sig.sum(dim=1) & 1).bool()
                m1, ix = a.min(dim=1)
                m2 = a.scatter(1, ix.unsqueeze(1), 255).min(dim=1).values
                f1 = (((m1 * NORM + 8) >> 4) - BETA).clamp_(min=0)
                f2 = (((m2 * NORM + 8) >> 4) - BETA).clamp_(min=0)
                mag = torch.where(self.j[r] == ix.unsqueeze(1), f2.unsqueeze(1), f1.unsqueeze(1))
                new = torch.where(sig ^ S.unsqueeze(1), -mag, mag)
                keep = live.view(-1, 1, 1)
                msg[r] = torch.where(keep, new, msg[r])
                L[:, v] = torch.where(keep, T + new, L[:, v])
            if early or it == max_iter:
                now = self.passes(L)
                status = torch.where(live, torch.where(now, it, -1).to(torch.int32), status)
                ok = ok | now if early else now
        return (L[:, :code.k] < 0).to(torch.uint8), status


def soft_values(a, code, base, z, cw, ebn0, gen):
    """(cw, n) int8 on the device, and the information bits sent"""
    pool = min(a.pool, cw)
    data = np.random.default_rng(1).integers(0, 2, (pool, code.k), dtype=np.uint8)
    words = torch.from_numpy(sd.ldpc_encode(data, base, z)).cuda()
    words = words.repeat((cw + pool - 1) // pool, 1)[:cw]
    x = 1.0 - 2.0 * words.to(torch.float32)
    if ebn0 is not None:
        sigma = float(np.sqrt(1.0 / (2 * code.k / code.n * 10 ** (ebn0 / 10))))
        x += sigma * torch.randn(x.shape, device="cuda", generator=gen)
    return torch.round(x * SCALE).clamp_(-127, 127).to(torch.int8).contiguous(), words[:, :code.k].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,4096", help="codewords per call")
    ap.add_argument("--pool", type=int, default=256, help="encoded codewords in the pool that a call's codewords repeat")
    ap.add_argument("--instr-per-entry", type=float, default=72.0, help="wave-instructions of the layer loop per entry and piece of a layer")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ldpc_bench.txt"))
    a = ap.parse_args()
    log = [f"# tools/bench_ldpc.py --sizes {a.sizes} --pool {a.pool} --instr-per-entry {a.instr_per_entry:g} --warmup {a.warmup} "
           f"--steps {a.steps} --repeats {a.repeats}"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261021)
    stream = torch.cuda.current_stream().cuda_stream
    for size in (int(v) for v in a.sizes.split(",")):
        for name, mb, nb, z, ebn0 in POINTS:
            base = R.generate(mb, nb, z, 1)
            code = R.Code(base, z)
            ref = TorchDecoder(code)
            decs = {}
            for early in (True, False):
                for variant in (0, 1):
                    d = sd.ldpc_decoder(base, z, NORM, BETA, early, "i8", 1.0, "bytes", code.k)
                    d.set_variant(variant)
                    decs[early, variant] = d
            i0, i1 = decs[True, 0].info(), decs[True, 1].info()
            pieces = 1 if z <= 64 else (z + 63) // 64
            head = (f"== {name}: n = {code.n}, k = {code.k}, {code.edges} edges, {size} codewords; variant 0: {i0['group']} codewords per wave, "
                    f"{i0['threads']} threads, {i0['lds_bytes']} B of LDS per workgroup, {i0['codewords_per_cu']} codewords per CU; variant 1: "
                    f"{decs[True, 1].launches(size)} launches of {i1['piece']} codewords, workspace {i1['workspace_bytes'] / 2 ** 20:.0f} MiB")
            print(head, flush=True)
            log.append(head)
            bits = torch.empty((size, code.k), dtype=torch.uint8, device="cuda")
            status = torch.empty(size, dtype=torch.int32, device="cuda")
            for point, noise, early in (("clean", None, True), (f"{ebn0:g} dB early stop", ebn0, True), (f"{ebn0:g} dB 20 iterations", ebn0, False)):
                x, sent = soft_values(a, code, base, z, size, noise, gen)
                fns = [lambda d=decs[early, v]: d.process_ptr(x.data_ptr(), bits.data_ptr(), None, status.data_ptr(), size, MAX_ITER, stream)
                       for v in (0, 1)]
                fns.append(lambda: ref.decode(x, early, MAX_ITER))
                outs = []
                for fn in fns[:2]:
                    fn()
                    torch.cuda.synchronize()
                    outs.append((bits.clone(), status.clone()))
                outs.append(fns[2]())
                same = all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])
                st = outs[0][1]
                iters = torch.where(st < 0, MAX_ITER, st).to(torch.float64) if early else torch.full_like(st, MAX_ITER, dtype=torch.float64)
                total_iters = float(iters.sum())
                wrong = int((outs[0][0] != sent).any(dim=1).sum())
                (m0, s0), (m1, s1), (mt, s_t) = rounds(a, fns)
                model = size * (code.n + code.k + 4)
                instr = a.instr_per_entry * (code.edges // z) * pieces * total_iters / i0["group"]
                line = (f"  {size:6d} {point:22s}: {m0:9.4f} ms (spread {s0:.3f}) = {size * code.k / (m0 * 1e-3) / 1e9:8.2f} Gbit/s decoded, "
                        f"{total_iters / size:5.2f} iterations -> {total_iters * code.edges / (m0 * 1e-3) / 1e9:8.1f} G edge-iterations/s, layer loop "
                        f">= {100 * instr / (m0 * 1e-3) / ISSUE:5.1f} % of issue, {model / 1e6:7.2f} MB -> {100 * model / (m0 * 1e-3) / PEAK_BYTES:5.2f} % of 8 TB/s"
                        f"  |  plain {m1:10.4f} ms (spread {s1:.3f}) -> {m1 / m0:7.2f}x  |  torch {mt:10.4f} ms (spread {s_t:.3f}) -> {mt / m0:7.2f}x"
                        f"  |  {int((st < 0).sum())} undecoded, {wrong} frame errors, results {'equal' if same else 'DIFFER'}")
                if m1 < m0:
                    line += "  LOSES to plain"
                if mt < m0:
                    line += "  LOSES to torch"
                print(line, flush=True)
                log.append(line)
                Path(a.out).write_text("\n".join(log) + "\n")  # after every line: a cut-short run keeps what it measured
                del x, sent, outs
            for d in decs.values():
                d.close()
            del bits, status, ref
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
