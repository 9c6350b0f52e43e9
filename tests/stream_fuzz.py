"""Seeded random cross-check of the streaming banks: the driver, as a library and as a command line.

    python tests/stream_fuzz.py --seed S --cases N [--family F ...] [--case I]

Each plan family's own GPU test file visits a small grid of parameters, one channel count, one split into calls and one start state.
This driver draws the cross product instead.  A family is an adapter (the `Family` classes below) with four parts:

  draw       a case from a numpy Generator: a plain dict of ints, floats and strings that prints on one line -- the plan parameters,
             the data seed, the call lengths of two independent splits, the start state, the subset of optional outputs, the kernel
             variant and the row padding of every buffer;
  data       the inputs and the random start state of a case, made with the `_rand` helpers of the family's GPU test file;
  step       the family's numpy reference (tests/*_ref.py) over ticks [t0, t1) of the stream from a given state;
  open       a session on the HIP bank (built with the `_bank` helper of the family's GPU test file) that takes the stream call by
             call through the C entry, so that NULL outputs, a NULL state and padded rows are all reachable.

The generator of a case is seeded from (seed, family name, case index) alone (`case_rng`), so a case does not change when families or
counts change and any single case can be rebuilt by itself.  A tick is the unit the entry accepts a call in: a sample for most banks.

Checks per case (`check_case`), each reported under its letter:
  (a) one call against the reference: every output and the final state (the stream position among it), under the rule of the
      family's own GPU test file, imported from there (`Family.same`): bit equality for the banks whose contract fixes every
      rounding, the file's tolerance for the banks around a transform (stft, istft, pfb, pfb_synth, welch, csd, fir_fft), for
      filtfilt and for the f32 resampler, whose references work in double;
  (b) the drawn split against (a): bit equality of the outputs and of the final state, whatever the rule of (a) is -- except the
      buffers a family lists in `split_tol`, where the header promises a split's agreement with one call "to rounding" (the
      accumulators of welch and csd) or "within that tolerance, not bit for bit" (the rows of the FFT-domain FIR bank): those are
      held to the family's tolerance against the one call;
  (c) a second, independently drawn split against (a): the same;
  (d) every other kernel variant (for pfb and pfb_synth: the other fold form) against variant 0, where the header says "identical
      values, bit for bit": bit equality.  The variants come from the VARIANTS table of tests/test_gpu_wide_strides.py
      (`_variants_from_the_table`); the inner transform's variant of stft, istft, pfb and pfb_synth is a knob of the case, and what
      the plan APPLIED (a transform without the variant refuses it) is noted in VARIANT_APPLIED for the coverage;
  (e) the padding of every input, output and accumulator row keeps its sentinel bits, and inputs are unchanged unless in place;
  (f) with a subset of the optional outputs, each output produced and the final state have the bits of the full call.
A case the library refuses is a failure (check letter of the run that was refused), never a skip.

All twenty families are adapted: fir_fft, resample, filtfilt, stft, istft, welch, csd, pfb, pfb_synth, ddc, duc, arb, cic,
cic_interp, beam, lms, rank, cfar, pll, timing.  filtfilt is a one-shot operation on whole rows (`stream = False`): one call, no
state, and the stream axes of the draw do not apply to it.

A failing check prints one line: family, seed, index, the check letter, the case dict, the buffer, and the count of differing
elements with the first differing index.  After a HIP runtime error (SDSP_HIP_ERR_HIP from an entry, or an error from the
synchronisation that follows every case) the driver prints that case's line, sets `GPU_STOPPED` and starts nothing more on the GPU
in the process.

tests/test_stream_fuzz_host.py runs the same check functions over numpy stand-ins (`StandIn`: a family's reference wrapped in the
session protocol) with planted defects; tests/test_gpu_stream_fuzz.py runs the committed seeds on the device."""
import argparse
import itertools
import sys
import time
import zlib
from pathlib import Path

import numpy as np

for _p in (str(Path(__file__).resolve().parent), str(Path(__file__).resolve().parents[1])):  # the command line: tests/ and the package
    if _p not in sys.path:
        sys.path.insert(0, _p)

SEEDS = (20261, 20262, 20263)  # the committed seeds of tests/test_gpu_stream_fuzz.py and tests/test_stream_fuzz_host.py
CASES = 12                     # cases per (family, seed)
PADS = (0, 1, 3, 4, 16)        # elements of sentinel past `samples` in every row
CHANNEL_EDGES = (1, 2, 63, 64, 65, 127, 128, 129)
ERR_HIP = -3                   # SDSP_HIP_ERR_HIP: the launch-class status of include/sdsp_hip.h

VARIANT_APPLIED = {}  # family -> {(precision, requested inner-transform variant, applied variant)}, noted by the sessions
GPU_STOPPED = []  # the line of the case a HIP error came back from; once non-empty nothing more is started on the GPU


class GpuStop(Exception):
    """a HIP runtime error came back: the process starts nothing more on the GPU"""


class Refused(Exception):
    """the library refused a call of a drawn case"""


def case_rng(seed, family, index):
    return np.random.default_rng([int(seed), zlib.crc32(family.encode()), int(index)])


# ------------------------------------------------------------------ draws shared by the families

def pick(rng, values, weights=None):
    values = list(values)
    p = None if weights is None else np.asarray(weights, dtype=float) / float(sum(weights))
    v = values[int(rng.choice(len(values), p=p))]
    return v.item() if isinstance(v, np.generic) else v


def draw_channels(rng, top=200, edges=CHANNEL_EDGES, tile=None):
    """1, both sides of 64 and 128 (and of a workgroup tile), or anything up to `top`: three draws in four land on an edge"""
    edges = sorted({e for e in (*edges, *((tile - 1, tile, tile + 1) if tile else ())) if 1 <= e <= top})
    if rng.random() < 0.75:
        return int(pick(rng, edges))
    return int(rng.integers(1, top + 1))


def draw_total(rng, unit, cap, floor=0):
    """ticks of the whole stream relative to the plan's unit (a staging block, a chunk, ..): less than one unit, exactly k units, k
    units +- 1; never more than `cap`"""
    unit = max(int(unit), 1)
    kmax = max(1, min(3, cap // unit))
    k = int(rng.integers(1, kmax + 1))
    kind = pick(rng, ("below", "at", "minus", "plus"), (3, 3, 2, 3))
    if kind == "below":
        total = int(rng.integers(1, unit)) if unit > 1 else 0
    elif kind == "at":
        total = k * unit
    elif kind == "minus":
        total = max(k, 2) * unit - 1 if max(k, 2) * unit - 1 <= cap else k * unit - 1
    else:
        total = k * unit + 1
    return max(floor, min(total, cap))


def draw_calls(rng, total, hist, null_state=False):
    """the stream of `total` ticks as 1 to 8 calls with random cut points; forced with a fixed probability each: an empty call at the
    start, in the middle and at the end, a call of one tick, a call shorter than the history and one of exactly the history (`hist`
    in ticks).  A case with a NULL state is a single call: nothing is carried."""
    if null_state:
        return [int(total)]
    forced = []
    if rng.random() < 0.4 and total >= 1:
        forced.append(1)
    if hist >= 2 and rng.random() < 0.5 and total - sum(forced) >= 1:
        forced.append(int(rng.integers(1, min(hist, total - sum(forced) + 1))))
    if hist >= 1 and rng.random() < 0.5 and total - sum(forced) >= hist:
        forced.append(int(hist))
    rest = total - sum(forced)
    pieces = int(rng.integers(1, max(2, 9 - len(forced))))
    cuts = sorted(int(c) for c in rng.integers(0, rest + 1, pieces - 1)) if rest > 0 else []
    calls = [b - a for a, b in zip([0, *cuts], [*cuts, rest])] if rest > 0 or not forced else []
    for f in forced:
        calls.insert(int(rng.integers(0, len(calls) + 1)), f)
    if rng.random() < 0.35:
        calls.insert(int(rng.integers(1, len(calls))) if len(calls) > 1 else len(calls), 0)
    if rng.random() < 0.35:
        calls.insert(0, 0)
    if rng.random() < 0.35:
        calls.append(0)
    assert sum(calls) == total and all(c >= 0 for c in calls), (calls, total)
    return [int(c) for c in calls]


def draw_position(rng, span=0, unit=1):
    """0, random below 2^34, or within one call (`span` ticks of `unit` samples) of a multiple of 2^32 -- always a multiple of `unit`"""
    kind = pick(rng, ("zero", "random", "edge"), (2, 3, 4))
    if kind == "zero":
        return 0
    if kind == "random":
        return int(rng.integers(1, (1 << 34) // unit)) * unit
    edge = int(rng.integers(1, 4)) << 32
    return max(0, (edge // unit - int(rng.integers(0, max(span, 1) + 1)))) * unit


def draw_pads(rng, names):
    return {n: int(pick(rng, PADS)) for n in names}


def draw_subset(rng, optional, allow_none=True):
    """a subset of the optional outputs as a '+'-joined string ('' = none), never the full set: that one is the base run"""
    subsets = [s for k in range(0 if allow_none else 1, len(optional)) for s in itertools.combinations(optional, k)]
    return "+".join(pick(rng, subsets)) if subsets else "+".join(optional)


def common_draw(rng, fam, case, hist, unit, cap, null_ok=True, floor=0):
    """the part of a case every family draws the same way, appended to the family's plan parameters"""
    start = pick(rng, ("zero", "random", "null") if null_ok else ("zero", "random"), (3, 5, 2) if null_ok else (3, 5))
    total = draw_total(rng, unit, cap, floor)
    case.update(hist=int(hist), unit=int(unit), total=int(total), start=start,
                calls=draw_calls(rng, total, hist, start == "null"), calls2=draw_calls(rng, total, hist, start == "null"),
                variant=int(pick(rng, fam.variants)), subset=draw_subset(rng, fam.optional, fam.none_legal),
                pads=draw_pads(rng, fam.buffers), data_seed=int(rng.integers(0, 1 << 31)))
    return case


# ------------------------------------------------------------------ padded buffers with sentinels

def sentinel(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return dtype.type(complex(-7777.25, 3333.5))
    if dtype.kind == "f":
        return dtype.type(-7777.25)
    return dtype.type(0x5A)


class Buf:
    """a (rows, n + pad) buffer of a call inside a flat tensor that is four elements longer, so that its pointer is never null"""

    def __init__(self, flat, rows, n, width, dtype):
        self.flat, self.rows, self.n, self.width, self.dtype = flat, rows, n, width, np.dtype(dtype)
        self.t = flat[:rows * width].view(rows, width)
        self.valid = None  # per-row counts of the elements the call may write, where they are fewer than n (data-dependent counts)

    @property
    def ptr(self):
        return self.flat.data_ptr()

    @property
    def stride(self):
        return self.width

    def np(self):
        return self.t.cpu().numpy()

    def host(self):
        """the buffer as a writable numpy array (stand-ins on the CPU only)"""
        return self.t.numpy()


class Io:
    """the buffers of ONE call.  inp(): an input row block with `pad` sentinel columns; out(): a sentinel-filled output; done(): what
    check (e) reports for the call"""

    def __init__(self, env, pads):
        self.env, self.pads, self.bufs = env, pads, []

    def _make(self, name, rows, n, dtype, content=None):
        torch = self.env.torch
        width = n + self.pads.get(name, 0)
        a = np.full(rows * width + 4, sentinel(dtype), dtype=dtype)
        if content is not None and n:
            a[:rows * width].reshape(rows, width)[:, :n] = content
        flat = torch.from_numpy(a).to(self.env.device)
        b = Buf(flat, rows, n, width, dtype)
        self.bufs.append([name, b, a.copy(), content is not None, False])  # a copy: on the CPU `flat` shares a's memory
        return b

    def inp(self, name, content):
        content = np.ascontiguousarray(content)
        return self._make(name, content.shape[0], content.shape[1], content.dtype, content)

    def out(self, name, rows, n, dtype):
        return self._make(name, rows, n, dtype)

    def in_place(self, buf):
        """the input `buf` is also an output of this call"""
        for rec in self.bufs:
            if rec[1] is buf:
                rec[4] = True
        return buf

    def sync(self):
        if self.env.device != "cpu":
            try:
                self.env.torch.cuda.synchronize()
            except RuntimeError as e:
                raise GpuStop(f"synchronize: {e}") from None

    def done(self):
        self.sync()
        bad = []
        for name, b, before, is_input, in_place in self.bufs:
            after = b.flat.cpu().numpy()
            body = np.zeros(after.size, dtype=bool)
            body[:b.rows * b.width].reshape(b.rows, b.width)[:, :b.n] = True
            if b.valid is not None:
                body[:b.rows * b.width].reshape(b.rows, b.width)[np.arange(b.width)[None, :] >= np.asarray(b.valid)[:, None]] = False
            count, first = bit_diff(after[~body], before[~body])
            if count:
                bad.append((f"padding of '{name}'", count, first))
            if is_input and not in_place:
                count, first = bit_diff(after[body], before[body])
                if count:
                    bad.append((f"input '{name}' was written", count, first))
        return bad


STATS = {"compared": 0, "runs": 0}  # elements that went through bit_diff and sessions opened, per process: printed with every family


def bit_diff(a, b):
    """(number of elements whose bits differ, index of the first) -- exact and NaN-safe; a shape or dtype mismatch counts as -1"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    STATS["compared"] += a.size
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1, (a.shape, str(a.dtype), b.shape, str(b.dtype))
    if a.size == 0:
        return 0, None
    d = (a.reshape(-1, 1).view(np.uint8) != b.reshape(-1, 1).view(np.uint8)).any(axis=1)
    if not d.any():
        return 0, None
    return int(d.sum()), tuple(int(i) for i in np.unravel_index(int(np.argmax(d)), a.shape))


# ------------------------------------------------------------------ the adapter protocol

class Family:
    """What the driver needs of a plan family.  Subclasses set the class attributes and the methods marked below."""
    name = ""
    variants = (0, 1)     # every value *_plan_set_variant takes
    cross_variants = None  # the variants the header calls identical bit for bit (check (d)); None: all of `variants`
    optional = ()         # outputs the entry takes NULL for
    none_legal = True     # whether all optional outputs may be left out at once
    buffers = ()          # the strided buffers of a call: inputs and outputs
    axes = {}             # case key -> every value the plan takes (test_coverage holds the draws to it)
    crosses = ()          # tuples of axes whose every combination must be seen
    split_tol = ()        # outputs and "state:<name>" buffers whose split agrees with one call "to rounding" only: held to same(), not to bits
    has_history = True
    null_state = True     # the C entry takes state = NULL
    stream = True         # False: a one-shot operation on whole rows, no state, one call (filtfilt)

    def module(self):
        """the family's GPU test file, for its _bank / _rand helpers and its comparison rule"""
        return __import__("test_gpu_" + self.name)

    # -- to implement
    def draw(self, rng, info_of):
        raise NotImplementedError

    def host_info(self, case):
        """a stand-in for the plan's info() where there is no device: the fields draw() reads"""
        raise NotImplementedError

    def plan_info(self, env, case):
        raise NotImplementedError

    def validate(self, case):
        """asserts the limits of include/sdsp_hip.h on a drawn case (no device)"""
        raise NotImplementedError

    def data(self, case):
        """{"in": {name: (rows, ticks-long) array}, "start": {name: array}}: the stream and the random start state"""
        raise NotImplementedError

    def step(self, case, data, state, t0, t1):
        """the reference over ticks [t0, t1) from `state` ({name: array}): ({output: array}, new state)"""
        raise NotImplementedError

    def open(self, env, case, data, variant, start):
        raise NotImplementedError

    def same(self, name, got, want, case, data=None):
        """the comparison rule of the family's GPU test file for one buffer against the reference"""
        return self.module()._same(got, want)

    # -- shared
    def zero_state(self, data):
        return {k: np.zeros_like(v) for k, v in data["start"].items()}

    def start_state(self, data, start):
        return {k: v.copy() for k, v in data["start"].items()} if start == "random" else self.zero_state(data)

    def join(self, parts):
        names = parts[0].keys() if parts else ()
        return {n: np.concatenate([p[n] for p in parts], axis=1) for n in names}

    def step_cached(self, case, data, state, t0, t1):
        """step(), remembered per (ticks, start state) in `data`: the runs of a case repeat the one-call stream several times"""
        key = (t0, t1, tuple(v.tobytes() for v in state.values()))
        memo = data.setdefault("memo", {})
        if key not in memo:
            memo[key] = self.step(case, data, state, t0, t1)
        outs, new = memo[key]
        return {k: v.copy() for k, v in outs.items()}, {k: v.copy() for k, v in new.items()}

    def wants(self, subset):
        return tuple(n for n in subset.split("+") if n)


class Env:
    def __init__(self, torch, device, sd=None):
        self.torch, self.device, self.sd = torch, device, sd
        self.lib = sd.load() if sd is not None else None


def gpu_env():
    import torch
    import simpledsp_amd
    assert torch.cuda.is_available(), "the streaming fuzz needs the MI355X"
    simpledsp_amd.load(build_if_missing=True)
    return Env(torch, "cuda", simpledsp_amd)


def cpu_env():
    import torch
    return Env(torch, "cpu")


def rc_check(rc, what):
    """a status of a C entry: 0 passes, SDSP_HIP_ERR_HIP stops the process's GPU work, anything else is a refusal"""
    if rc == 0:
        return
    if rc == ERR_HIP:
        raise GpuStop(f"{what}: SDSP_HIP_ERR_HIP")
    raise Refused(f"{what}: status {rc}")


def guarded(fn, what):
    """a call into the Python wrappers: their SdspHipError becomes GpuStop or Refused like a bare status"""
    try:
        return fn()
    except ValueError as e:
        raise Refused(f"{what}: {e}") from None
    except RuntimeError as e:
        code = getattr(e, "code", None)
        if code is None or code == ERR_HIP:
            raise GpuStop(f"{what}: {e}") from None
        raise Refused(f"{what}: {e}") from None


def set_inner_variant(fam, case, setter, plan, variant, what):
    """the inner transform's variant of a bank around a transform plan: SDSP_HIP_ERR_UNSUPPORTED ("no such kernel variant") is the
    documented answer of a transform that has none, and the plan stays at variant 0.  What was applied is noted for the coverage"""
    applied = 0
    if variant:
        rc = setter(plan, variant)
        if rc != -2:  # SDSP_HIP_ERR_UNSUPPORTED
            rc_check(rc, what)
            applied = variant
    VARIANT_APPLIED.setdefault(fam.name, set()).add((case["precision"], variant, applied))


def slice_frames(info, frame_bytes):
    """frames (units) one workspace slice of a plan holds: the unit the totals of the banks around a transform are drawn against"""
    return max(1, int(info["workspace_bytes"]) // frame_bytes)


DEFAULT_WORKSPACE = 256 << 20  # what the host stand-ins of info() report for workspace_bytes = 0: the default slice budget


def ptr(b):
    return b.ptr if b is not None else None


def stride(b):
    return b.stride if b is not None else 0


# ------------------------------------------------------------------ a run, and the checks

class Run:
    def __init__(self, outs, state, pad_faults):
        self.outs, self.state, self.pad_faults = outs, state, pad_faults


def run_stream(fam, env, case, data, calls, wants, variant, start, opener=None):
    """the stream of the case through one session, cut into `calls`: every output joined over the calls, the final state
    ({} for a NULL state), and what check (e) found"""
    sess = (opener or fam.open)(env, case, data, variant, start)
    STATS["runs"] += 1
    parts, faults, t = [], [], 0
    for n in calls:
        io = Io(env, case["pads"])
        parts.append(sess.call(t, t + n, wants, io))
        faults += io.done()
        t += n
    assert t == case["total"], (t, case["total"])
    state = sess.state()
    return Run(fam.join(parts), state, faults + list(getattr(sess, "faults", ())))


def _line(fam, seed, index, letter, case, what, count, first):
    return f"FAIL family={fam.name} seed={seed} index={index} check={letter} case={case} buffer={what} differing={count} first={first}"


def _bits(failures, line, what, got, want):
    count, first = bit_diff(got, want)
    if count:
        failures.append(line(what, count, first))


def check_case(fam, env, case, seed, index, opener=None):
    """checks (a) to (f) of the module docstring for one case: the list of failure lines (empty: the case passed).  GpuStop passes
    through; a refusal is a failure of the run it happened in"""
    failures = []
    data = fam.data(case)
    full = fam.optional
    total, variant, start = case["total"], case["variant"], case["start"]
    ref_start = fam.start_state(data, start)
    want_outs, want_state = fam.step_cached(case, data, ref_start, 0, total)

    def attempt(letter, calls, wants, v, st):
        try:
            run = run_stream(fam, env, case, data, calls, wants, v, st, opener)
        except Refused as e:
            failures.append(_line(fam, seed, index, letter, case, f"refused: {e}", -1, None))
            return None
        for what, count, first in run.pad_faults:
            failures.append(_line(fam, seed, index, "e", case, f"{what} (run of check {letter})", count, first))
        return run

    def line(letter):
        return lambda what, count, first: _line(fam, seed, index, letter, case, what, count, first)

    # (a) one call against the reference
    a = attempt("a", [total], full, variant, start)
    if a is None:
        return failures
    for name, w in want_outs.items():
        count, first = bit_diff(a.outs[name], w)
        if not fam.same(name, a.outs[name], w, case, data):
            failures.append(_line(fam, seed, index, "a", case, name, count, first))
    for name in a.state:
        w = want_state[name]
        count, first = bit_diff(a.state[name], w)
        if not fam.same("state:" + name, a.state[name], w, case, data):
            failures.append(_line(fam, seed, index, "a", case, "state:" + name, count, first))
    # (b), (c) the two splits against (a): bits, except the buffers the family's header promises "to rounding" only (Family.split_tol),
    # which are held to the family's tolerance.  A NULL state carries nothing, so there the splits start from a zero-filled one, which
    # the header makes the same stream, and what (a) did not keep is held to the reference's
    split_start = "zero" if start == "null" else start
    for letter, calls in (("b", case["calls"]), ("c", case["calls2"])):
        r = attempt(letter, calls, full, variant, split_start)
        if r is None:
            continue
        for name in a.outs:
            if name in fam.split_tol:
                if not fam.same(name, r.outs[name], a.outs[name], case, data):
                    failures.append(line(letter)(name, *bit_diff(r.outs[name], a.outs[name])))
            else:
                _bits(failures, line(letter), name, r.outs[name], a.outs[name])
        for name, w in a.state.items():
            if "state:" + name in fam.split_tol:
                if not fam.same("state:" + name, r.state[name], w, case, data):
                    failures.append(line(letter)("state:" + name, *bit_diff(r.state[name], w)))
            else:
                _bits(failures, line(letter), "state:" + name, r.state[name], w)
        for name, w in want_state.items():
            if name not in a.state and not fam.same("state:" + name, r.state[name], w, case, data):
                failures.append(line(letter)("state:" + name, *bit_diff(r.state[name], w)))
    # (d) every variant against variant 0, where the header promises identical bits
    cross = fam.variants if fam.cross_variants is None else fam.cross_variants
    runs = {variant: a}
    for v in cross:
        if v not in runs:
            runs[v] = attempt("d", [total], full, v, start)
    base = runs.get(cross[0])
    for v in cross[1:]:
        if base is None or runs[v] is None:
            continue
        for name in base.outs:
            _bits(failures, line("d"), f"{name} (variant {v})", runs[v].outs[name], base.outs[name])
        for name in base.state:
            _bits(failures, line("d"), f"state:{name} (variant {v})", runs[v].state[name], base.state[name])
    # (f) a subset of the optional outputs
    wants = fam.wants(case["subset"])
    if fam.optional and set(wants) != set(full):
        f = attempt("f", [total], wants, variant, start)
        if f is not None:
            if set(f.outs) != set(wants) | (set(a.outs) - set(full)):
                failures.append(_line(fam, seed, index, "f", case, f"outputs {sorted(f.outs)} for the subset {sorted(wants)}", -1, None))
            for name in f.outs:
                _bits(failures, line("f"), name, f.outs[name], a.outs[name])
            for name in a.state:
                _bits(failures, line("f"), "state:" + name, f.state[name], a.state[name])
    return failures


# ------------------------------------------------------------------ numpy stand-ins: a family's reference in the session protocol

class StandIn:
    """The family's reference behind the session protocol, on CPU tensors: what tests/test_stream_fuzz_host.py runs the checks over.
    `defect` names one planted defect (DEFECTS); None is the undamaged bank."""

    def __init__(self, fam, env, case, data, variant, start, defect=None):
        self.fam, self.case, self.data, self.variant, self.defect = fam, case, data, variant, defect
        self.null = start == "null"
        self.st = fam.start_state(data, "zero" if self.null else start)
        if defect == "row64_from_row0" and start == "random":
            for v in self.st.values():
                if v.ndim >= 1 and v.shape[0] > 64:
                    v[64] = v[0]

    def call(self, t0, t1, wants, io):
        fam, n = self.fam, t1 - t0
        ins = {name: io.inp(name, fam.columns(self.case, name, a, t0, t1)) for name, a in self.data["in"].items()}
        outs, new = fam.step_cached(self.case, self.data, self.st, t0, t1)
        if self.defect == "count_off_by_one" and "counts" in outs and outs["counts"].size:
            outs["counts"] = outs["counts"].copy()
            outs["counts"].reshape(-1)[-1] += 1
        if self.defect == "short_call_history" and 0 < n < self.case["hist"]:
            new = dict(new, hist=new["hist"].copy())
            new["hist"][:, n:] = 0
        if self.defect == "zero_call_clears" and n == 0:
            new = {k: np.zeros_like(v) for k, v in new.items()}
        if self.defect == "position_stuck" and n > 0 and t1 % self.case["unit"] == 0 and "position" in new:
            new = dict(new, position=self.st["position"].copy())
        if not self.null:
            self.st = new
        got = {}
        produced = [name for name in outs if name not in fam.optional or name in wants]
        for name in produced:
            v = outs[name]
            if self.defect == "variant1_ulp" and self.variant == 1 and v.size and name == produced[0]:
                v = v.copy()
                raw = v.reshape(-1).view(np.uint8)
                raw[0] ^= 1
            b = io.out(name, v.shape[0], v.shape[1], v.dtype)
            b.host()[:, :v.shape[1]] = v
            if self.defect == "pad_write" and b.width > b.n and name == produced[0]:
                b.host()[0, b.n] = v.dtype.type(1)
            got[name] = b
        if self.defect == "subset_moves" and len(produced) < len(outs):
            pairs = [(m, p) for m in outs if m not in produced for p in produced
                     if outs[p].dtype == outs[m].dtype and outs[p].shape == outs[m].shape]
            if pairs:
                got[pairs[0][1]].host()[:, :outs[pairs[0][0]].shape[1]] = outs[pairs[0][0]]
        del ins
        return {name: b.np()[:, :b.n].copy() for name, b in got.items()}

    def state(self):
        return {} if self.null else {k: v.copy() for k, v in self.st.items()}


DEFECTS = ("short_call_history", "zero_call_clears", "position_stuck", "row64_from_row0", "variant1_ulp", "pad_write", "subset_moves",
           "count_off_by_one")


def stand_in_opener(defect=None):
    return lambda env, case, data, variant, start: StandIn(FAMILIES[case["family"]], env, case, data, variant, start, defect)


# ------------------------------------------------------------------ the families

def _prec(sd, precision):
    return sd.F64 if precision == "f64" else sd.F32


class SampleFamily(Family):
    """banks whose tick is one sample of every row, in and out"""

    def columns(self, case, name, a, t0, t1):
        return a[:, t0:t1]


class _Session:
    """what the HIP sessions share: the bank, the C library, the state tensor or NULL"""

    def __init__(self, fam, env, case, data, variant, start):
        self.fam, self.env, self.case, self.data, self.variant = fam, env, case, data, variant
        self.null = start == "null"
        self.lib = env.lib
        self.bank = None

    def state_ptr(self):
        return None if self.null else (self.bank._ensure_state().data_ptr() or None)

    def collect(self, got):
        return {name: b.np()[:, :b.n].copy() for name, b in got.items()}


class Lms(SampleFamily):
    name = "lms"
    optional = ("y", "e")
    buffers = ("x", "d", "y", "e")
    axes = {"precision": ("f32", "f64"), "kind": ("real", "complex"), "mode": ("lms", "nlms"), "variant": (0, 1), "bound": (8, 16, 32, 64),
            "on_bound": (True, False)}
    crosses = (("bound", "on_bound"),)  # the kernel's 64 forms: every bound both ways

    @staticmethod
    def bound(taps):
        return 8 if taps <= 8 else 16 if taps <= 16 else 32 if taps <= 32 else 64  # lms.hip: tap_bound()

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), kind=pick(rng, ("real", "complex")),
                    mode=pick(rng, ("lms", "nlms")), channels=draw_channels(rng))
        top = 32 if (case["precision"], case["kind"]) == ("f64", "complex") else 64  # SDSP_HIP_LMS_MAX_TAPS_F64_COMPLEX
        # every bound of lms.hip's tap_bound(), with the tap count on it (the form without tests) or below it
        pairs = [(b, on) for b in (8, 16, 32, 64) if b <= top for on in (True, False)]
        bound, on = pick(rng, pairs, [2 if b == 64 else 1 for b, _ in pairs])  # 64 is out of F64 COMPLEX's reach: twice the weight elsewhere
        if on:
            taps = bound
        else:  # below the bound: one, two and three taps past a group of four, and the first tap count of the bound
            low = bound // 2 + 1 if bound > 8 else 1
            taps = int(pick(rng, sorted({low, low + 1, bound - 3, bound - 2, bound - 1, int(rng.integers(low, bound))} - {0, bound})))
        case.update(taps=taps, bound=bound, on_bound=taps == bound)
        info = info_of(case)
        # the reference loops over samples and taps in Python: long filters get a block and a sample, short ones up to three blocks
        cap = 3 * info["block"] + 1 if taps <= 16 else info["block"] + 1
        return common_draw(rng, self, case, taps - 1, info["block"], cap)

    def host_info(self, case):
        es = (8 if case["precision"] == "f64" else 4) * (2 if case["kind"] == "complex" else 1)
        el = 1 if es >= 16 else 16 // es
        rows = 160 * 1024 // 4 // (65 * es)  # lms.hip: block_for()
        return {"block": min(8 * el, (rows - self.bound(case["taps"])) // 2 // el * el)}

    def plan_info(self, env, case):
        t = self.module()
        return t._bank(env.sd, case["taps"], case["precision"], case["kind"] == "complex", case["mode"], channels=case["channels"]).info()

    def validate(self, case):
        top = 32 if (case["precision"], case["kind"]) == ("f64", "complex") else 64
        assert 1 <= case["taps"] <= top and 1 <= case["channels"] < 1 << 31 and case["total"] < 1 << 31, case
        assert self.bound(case["taps"]) == case["bound"] and case["on_bound"] == (case["taps"] == case["bound"]), case

    def data(self, case):
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C, T, p, cplx = case["channels"], case["taps"], case["precision"], case["kind"] == "complex"
        x, d = t._rand(rng, (C, case["total"]), p, cplx), t._rand(rng, (C, case["total"]), p, cplx)
        return {"in": {"x": x, "d": d}, "start": {"weights": t._rand(rng, (C, T), p, cplx, 0.1), "hist": t._rand(rng, (C, T - 1), p, cplx)}}

    def step(self, case, data, state, t0, t1):
        from lms_ref import lms_ref
        mu, eps = self.module()._step(case["mode"], case["taps"])
        y, e, w, h = lms_ref(data["in"]["x"][:, t0:t1], data["in"]["d"][:, t0:t1], case["taps"], mu, case["mode"], eps, state["weights"],
                             state["hist"], case["precision"])
        return {"y": y, "e": e}, {"weights": w, "hist": h}

    def open(self, env, case, data, variant, start):
        return _LmsSession(self, env, case, data, variant, start)


class _LmsSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        t = fam.module()
        st = data["start"] if start == "random" else {"weights": None, "hist": None}
        self.bank = guarded(lambda: t._bank(env.sd, case["taps"], case["precision"], case["kind"] == "complex", case["mode"], variant,
                                            st["weights"], st["hist"], channels=case["channels"]), "lms plan")
        self.mu = t._step(case["mode"], case["taps"])[0]

    def call(self, t0, t1, wants, io):
        n, C = t1 - t0, self.case["channels"]
        x, d = io.inp("x", self.data["in"]["x"][:, t0:t1]), io.inp("d", self.data["in"]["d"][:, t0:t1])
        got = {name: io.out(name, C, n, x.dtype) for name in ("y", "e") if name in wants}
        y, e = got.get("y"), got.get("e")
        rc_check(self.lib.sdsp_hip_lms_process(self.bank._plan, x.ptr, x.stride, d.ptr, d.stride, ptr(y), stride(y), ptr(e), stride(e), n,
                                               self.mu, self.state_ptr(), None), "lms_process")
        io.sync()
        return self.collect(got)

    def state(self):
        if self.null:
            return {}
        return {"weights": self.bank.weights().cpu().numpy().copy(), "hist": self.bank.history().cpu().numpy().copy()}


class Rank(SampleFamily):
    name = "rank"
    buffers = ("x", "y")
    axes = {"precision": ("f32", "f64"), "variant": (0, 1)}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), channels=draw_channels(rng))
        top = 127 if case["precision"] == "f64" else 255  # SDSP_HIP_RANK_MAX_WINDOW_F64, SDSP_HIP_RANK_MAX_WINDOW
        edges = [w for p in (8, 16, 32, 64, 128) for w in (p - 1, p, p + 1) if w <= top]  # the ladder of sorted-array sizes
        W = int(pick(rng, [1, 2, 3, 5, top, *edges])) if rng.random() < 0.8 else int(rng.integers(1, top + 1))
        r = int(pick(rng, sorted({0, (W - 1) // 2, W - 1, int(rng.integers(0, W))})))
        case.update(window=W, rank=r)
        info = info_of(case)
        return common_draw(rng, self, case, W - 1, info["block"], 4096)

    def host_info(self, case):
        return {"block": 256}

    def plan_info(self, env, case):
        return self.module()._bank(env.sd, case["window"], case["rank"], case["precision"], channels=case["channels"]).info()

    def validate(self, case):
        from simpledsp_amd import rank_filter
        from simpledsp_amd._lib import F32, F64
        rank_filter.check_window(case["window"], F64 if case["precision"] == "f64" else F32)
        assert rank_filter.rank_index(case["window"], case["rank"]) == case["rank"] and 1 <= case["channels"] < 1 << 31, case

    def data(self, case):
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C, W, p = case["channels"], case["window"], case["precision"]
        return {"in": {"x": t._rand(rng, (C, case["total"]), p)}, "start": {"hist": t._rand(rng, (C, W - 1), p)}}

    def step(self, case, data, state, t0, t1):
        from rank_ref import rank_ref
        y, h = rank_ref(data["in"]["x"][:, t0:t1], case["window"], case["rank"], state["hist"])
        return {"y": y}, {"hist": h}

    def open(self, env, case, data, variant, start):
        return _RankSession(self, env, case, data, variant, start)


class _RankSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else None
        self.bank = guarded(lambda: fam.module()._bank(env.sd, case["window"], case["rank"], case["precision"], variant, hist,
                                                       channels=case["channels"]), "rank plan")

    def call(self, t0, t1, wants, io):
        n = t1 - t0
        x = io.inp("x", self.data["in"]["x"][:, t0:t1])
        y = io.out("y", x.rows, n, x.dtype)
        rc_check(self.lib.sdsp_hip_rank_process(self.bank._plan, x.ptr, x.stride, y.ptr, y.stride, n, self.state_ptr(), None),
                 "rank_process")
        io.sync()
        return self.collect({"y": y})

    def state(self):
        return {} if self.null else {"hist": self.bank.history().cpu().numpy().copy()}


class Cfar(SampleFamily):
    name = "cfar"
    optional = ("thr", "det")
    none_legal = False  # thr and det cannot both be left out
    buffers = ("x", "thr", "det")
    axes = {"precision": ("f32", "f64"), "kind": ("power", "iq"), "mode": ("ca", "go", "so", "os"), "variant": (0, 1)}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), kind=pick(rng, ("power", "iq")),
                    mode=pick(rng, ("ca", "go", "so", "os"), (2, 2, 2, 3)), channels=draw_channels(rng))
        if case["mode"] == "os":  # 2 L on both sides of every step of the sorted array's size, up to the precision's limit
            top = 63 if case["precision"] == "f64" else 127
            L = int(pick(rng, [v for v in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127) if v <= top]))
            rank = int(pick(rng, sorted({0, L, (3 * L) // 2, 2 * L - 1, int(rng.integers(0, 2 * L))})))
        else:
            L = int(pick(rng, (1, 2, 4, 7, 16, 33, 64, 128))) if rng.random() < 0.7 else int(rng.integers(1, 129))
            rank = -1
        G = int(pick(rng, (0, 1, 2, 3, 40, 255))) if rng.random() < 0.8 else int(rng.integers(0, 256))
        case.update(train=L, guard=G, rank=rank)
        info = info_of(case)
        W = 2 * (L + G) + 1
        return common_draw(rng, self, case, W - 1, self.module()._unit(info, W), 6000)

    def _rank(self, case):
        return case["rank"] if case["mode"] == "os" else None

    def host_info(self, case):
        return {"mode": ("ca", "go", "so", "os").index(case["mode"]), "block": 512}

    def plan_info(self, env, case):
        return self.module()._bank(env.sd, case["channels"], case["train"], case["guard"], case["mode"], case["precision"], case["kind"],
                                   rank=self._rank(case)).info()

    def validate(self, case):
        from simpledsp_amd import _lib as L
        assert 1 <= case["train"] <= L.CFAR_MAX_TRAIN and 0 <= case["guard"] <= L.CFAR_MAX_GUARD and 1 <= case["channels"] < 1 << 31, case
        if case["mode"] == "os":
            assert 2 * case["train"] <= (L.RANK_MAX_WINDOW_F64 if case["precision"] == "f64" else L.RANK_MAX_WINDOW), case
            assert 0 <= case["rank"] < 2 * case["train"], case
        assert self.module()._valid(case["mode"], case["precision"], case["train"])
        assert case["subset"] in ("thr", "det"), case

    def data(self, case):
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C, W = case["channels"], 2 * (case["train"] + case["guard"]) + 1
        return {"in": {"x": t._rows(rng, (C, case["total"]), case["precision"], case["kind"])},
                "start": {"hist": t._rows(rng, (C, W - 1), case["precision"], case["kind"])}}

    def step(self, case, data, state, t0, t1):
        from cfar_ref import cfar_ref
        thr, det, h = cfar_ref(data["in"]["x"][:, t0:t1], case["train"], case["guard"], case["mode"], self.module().ALPHA, self._rank(case),
                               state["hist"])
        return {"thr": thr, "det": det}, {"hist": h}

    def open(self, env, case, data, variant, start):
        return _CfarSession(self, env, case, data, variant, start)


class _CfarSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else None
        self.bank = guarded(lambda: fam.module()._bank(env.sd, case["channels"], case["train"], case["guard"], case["mode"], case["precision"],
                                                       case["kind"], variant, fam._rank(case), hist=hist), "cfar plan")

    def call(self, t0, t1, wants, io):
        from rank_ref import row_dtype
        n = t1 - t0
        x = io.inp("x", self.data["in"]["x"][:, t0:t1])
        got = {}
        if "thr" in wants:
            got["thr"] = io.out("thr", x.rows, n, row_dtype(self.case["precision"]))
        if "det" in wants:
            got["det"] = io.out("det", x.rows, n, np.uint8)
        thr, det = got.get("thr"), got.get("det")
        rc_check(self.lib.sdsp_hip_cfar_process(self.bank._plan, x.ptr, x.stride, ptr(thr), stride(thr), ptr(det), stride(det), n,
                                                self.state_ptr(), None), "cfar_process")
        io.sync()
        return self.collect(got)

    def state(self):
        return {} if self.null else {"hist": self.bank.history().cpu().numpy().copy()}


class Pll(SampleFamily):
    name = "pll"
    optional = ("y", "err", "freq")
    buffers = ("x", "y", "err", "freq")
    has_history = False
    axes = {"precision": ("f32", "f64"), "mode": ("cross", "bpsk", "qpsk"), "variant": (0, 1), "in_place": (0, 1), "shared_word": (0, 1)}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), mode=pick(rng, ("cross", "bpsk", "qpsk")),
                    channels=draw_channels(rng), in_place=int(rng.random() < 0.4), shared_word=int(rng.random() < 0.3),
                    word_seed=int(rng.integers(0, 1 << 31)))
        info = info_of(case)
        case = common_draw(rng, self, case, 0, info["block"], 1500)
        if case["in_place"]:  # y is x: one buffer, one padding
            case["pads"]["y"] = case["pads"]["x"]
        return case

    def host_info(self, case):
        return {"block": 256}

    def _words(self, case):
        t = self.module()
        rng = np.random.default_rng(case["word_seed"])
        return t._words(rng, 1 if case["shared_word"] else case["channels"])

    def plan_info(self, env, case):
        return self.module()._bank(env.sd, self._words(case), case["precision"], case["mode"], channels=case["channels"]).info()

    def validate(self, case):
        t = self.module()
        assert 1 <= case["channels"] < 1 << 31 and 0 < t.MAX_DEV <= 0.5 and case["mode"] in ("cross", "bpsk", "qpsk"), case
        assert self._words(case).size in (1, case["channels"])

    def data(self, case):
        from pll_ref import real_dtype
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C = case["channels"]
        return {"in": {"x": t._rand(rng, (C, case["total"]), case["precision"])},
                "start": {"integ": rng.uniform(-t.MAX_DEV, t.MAX_DEV, C).astype(real_dtype(case["precision"])), "theta": t._words(rng, C)}}

    def step(self, case, data, state, t0, t1):
        from pll_ref import pll_ref
        t = self.module()
        y, err, freq, integ, theta = pll_ref(data["in"]["x"][:, t0:t1], self._words(case), t.ALPHA, t.BETA, case["mode"], t.MAX_DEV,
                                             state["integ"], state["theta"], case["precision"])
        return {"y": y, "err": err, "freq": freq}, {"integ": integ, "theta": theta}

    def open(self, env, case, data, variant, start):
        return _PllSession(self, env, case, data, variant, start)


class _PllSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        st = data["start"] if start == "random" else {"integ": None, "theta": None}
        self.bank = guarded(lambda: fam.module()._bank(env.sd, fam._words(case), case["precision"], case["mode"], variant, st["integ"],
                                                       st["theta"], channels=case["channels"]), "pll plan")

    def call(self, t0, t1, wants, io):
        from pll_ref import real_dtype
        t = self.fam.module()
        n = t1 - t0
        x = io.inp("x", self.data["in"]["x"][:, t0:t1])
        got = {}
        if "y" in wants:
            got["y"] = io.in_place(x) if self.case["in_place"] else io.out("y", x.rows, n, x.dtype)
        for name in ("err", "freq"):
            if name in wants:
                got[name] = io.out(name, x.rows, n, real_dtype(self.case["precision"]))
        y, err, freq = got.get("y"), got.get("err"), got.get("freq")
        rc_check(self.lib.sdsp_hip_pll_process(self.bank._plan, x.ptr, x.stride, ptr(y), stride(y), ptr(err), stride(err), ptr(freq),
                                               stride(freq), n, t.ALPHA, t.BETA, self.state_ptr(), None), "pll_process")
        io.sync()
        return self.collect(got)

    def state(self):
        if self.null:
            return {}
        return {"integ": self.bank.freq().cpu().numpy().copy(), "theta": self.bank.phase().cpu().numpy().view(np.uint32).copy()}


class Timing(SampleFamily):
    """the number of symbols a row yields depends on its data: every output row of a call has room for max_out(samples) elements, of
    which counts[c] are written; the joined outputs are per-channel concatenations, zero behind each row's total"""
    name = "timing"
    optional = ("err", "period")
    buffers = ("x", "y", "err", "period")
    axes = {"precision": ("f32", "f64"), "mode": ("gardner", "zc_qpsk", "zc_bpsk"), "variant": (0, 1)}
    FIELDS = ("t", "ps", "ym", "integ", "w", "parity", "hist")

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), mode=pick(rng, ("gardner", "zc_qpsk", "zc_bpsk")))
        L = int(pick(rng, (1, 2, 4, 32, 128)))
        T = int(pick(rng, [t for t in (1, 2, 5, 16, 31, 32, 64) if L * t <= 4096]))  # SDSP_HIP_TIMING_MAX_TABLE
        case.update(phases=L, taps=T, sps=float(pick(rng, (2.0, 2.37, 3.0, 8.0, 128.0), (3, 3, 2, 2, 1))), tap_seed=int(rng.integers(0, 1 << 31)))
        case["channels"] = 1
        info = info_of(case)
        case["channels"] = draw_channels(rng, tile=64 * info.get("waves", 1))  # the workgroup holds `waves` tiles of 64 channels
        # one pass of the reference's loop is one strobe of T multiply-adds: at most a sample each
        cap = max(info["block"] + 1, min(3 * info["block"] + 1, 6000 // T))
        return common_draw(rng, self, case, T - 1, info["block"], cap)

    def host_info(self, case):
        return {"block": 64 if case["precision"] == "f64" else 128, "waves": 1}

    def _h(self, case):
        return self.module()._taps(np.random.default_rng(case["tap_seed"]), case["phases"], case["taps"])

    def plan_info(self, env, case):
        t = self.module()
        return t._bank(env.sd, env.torch, self._h(case), case["phases"], case["sps"], case["precision"], case["mode"],
                       channels=case["channels"]).info()

    def validate(self, case):
        from simpledsp_amd import _lib as L
        from timing_ref import max_out, step_of
        P, T = case["phases"], case["taps"]
        assert P & (P - 1) == 0 and 1 <= P <= L.TIMING_MAX_PHASES and 1 <= T <= L.TIMING_MAX_TAPS and P * T <= L.TIMING_MAX_TABLE, case
        assert (1 << 32) <= step_of(case["sps"]) <= (1 << 38) and 0 < self.module().MAX_DEV <= 0.5 and 1 <= case["channels"] < 1 << 31, case
        assert max_out(step_of(case["sps"]), case["total"]) <= case["total"] + 1

    def data(self, case):
        from timing_ref import step_of, timing_ref
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C, p = case["channels"], case["precision"]
        x = t._rand(rng, (C, case["total"]), p)
        x[3::5] *= 1e6  # drives the advance word to both clamps on those channels: the counts differ between the lanes of a wave
        start = timing_ref(self._h(case), case["phases"], case["taps"], t._rand(rng, (C, 9), p), step_of(case["sps"]), t.ALPHA, t.BETA,
                           case["mode"], t.MAX_DEV, None, p)[4]  # a state that is not zero: the reference after 9 samples
        return {"in": {"x": x}, "start": {k: np.ascontiguousarray(start[k]) for k in self.FIELDS}}

    def step(self, case, data, state, t0, t1):
        from timing_ref import step_of, timing_ref
        t = self.module()
        y, err, period, counts, new, _ = timing_ref(self._h(case), case["phases"], case["taps"], data["in"]["x"][:, t0:t1],
                                                    step_of(case["sps"]), t.ALPHA, t.BETA, case["mode"], t.MAX_DEV, state, case["precision"])
        top = int(counts.max()) if counts.size else 0
        return ({"y": y[:, :top], "err": err[:, :top], "period": period[:, :top], "counts": counts.reshape(-1, 1).astype(np.uint32)},
                {k: np.ascontiguousarray(new[k]) for k in self.FIELDS})

    def join(self, parts):
        counts = sum(p["counts"].astype(np.int64) for p in parts).reshape(-1)
        top = int(counts.max()) if counts.size else 0
        out = {"counts": counts.astype(np.uint32).reshape(-1, 1)}
        for name in parts[0]:
            if name == "counts":
                continue
            joined = np.zeros((counts.size, top), dtype=parts[0][name].dtype)
            for c in range(counts.size):
                row = np.concatenate([p[name][c, :int(p["counts"][c, 0])] for p in parts])
                joined[c, :row.size] = row[:top]
            out[name] = joined
        return out

    def open(self, env, case, data, variant, start):
        return _TimingSession(self, env, case, data, variant, start)


class _TimingSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        t = fam.module()
        st = data["start"] if start == "random" else None
        self.bank = guarded(lambda: t._bank(env.sd, env.torch, fam._h(case), case["phases"], case["sps"], case["precision"], case["mode"],
                                            variant, st, channels=case["channels"]), "timing plan")

    def call(self, t0, t1, wants, io):
        from timing_ref import max_out, real_dtype, step_of
        t = self.fam.module()
        n, C = t1 - t0, self.case["channels"]
        cap = max_out(step_of(self.case["sps"]), n)
        x = io.inp("x", self.data["in"]["x"][:, t0:t1])
        got = {"y": io.out("y", C, cap, x.dtype)}
        for name in ("err", "period"):
            if name in wants:
                got[name] = io.out(name, C, cap, real_dtype(self.case["precision"]))
        counts = io.out("counts", 1, C, np.uint32)
        err, period = got.get("err"), got.get("period")
        rc_check(self.lib.sdsp_hip_timing_process(self.bank._plan, x.ptr, x.stride, got["y"].ptr, got["y"].stride, ptr(err), stride(err),
                                                  ptr(period), stride(period), counts.ptr, n, t.ALPHA, t.BETA, self.state_ptr(), None),
                 "timing_process")
        io.sync()
        cnt = counts.np()[0, :C].astype(np.int64)
        if (cnt > cap).any():
            raise Refused(f"timing_process: a count of {int(cnt.max())} past the capacity {cap}")
        top = int(cnt.max()) if C else 0
        outs = {"counts": cnt.astype(np.uint32).reshape(-1, 1)}
        for name, b in got.items():
            b.valid = cnt
            a = b.np()[:, :top].copy()
            a[np.arange(top)[None, :] >= cnt[:, None]] = 0
            outs[name] = a
        return outs

    def state(self):
        if self.null:
            return {}
        from timing_ref import real_dtype, row_dtype
        raw = self.bank._ensure_state().cpu().numpy()
        offs, sizes = self.bank._offsets()
        C, T, p = self.case["channels"], self.case["taps"], self.case["precision"]
        kinds = (np.uint64, row_dtype(p), row_dtype(p), real_dtype(p), np.int32, np.uint32, row_dtype(p))
        out = {k: raw[o:o + n].view(dt).copy() for k, o, n, dt in zip(self.fam.FIELDS, offs, sizes, kinds)}
        out["hist"] = out["hist"].reshape(C, T - 1)
        return out


class Ddc(Family):
    """a tick is D input samples of every channel and one output of every band; the stream position is the caller's to carry"""
    name = "ddc"
    buffers = ("in", "out")
    axes = {"precision": ("f32", "f64"), "kind": ("real", "complex"), "variant": (0, 1)}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), kind=pick(rng, ("real", "complex")),
                    channels=draw_channels(rng, top=130))
        D = int(pick(rng, (1, 2, 3, 5, 7, 50), (3, 2, 2, 2, 1, 1)))
        T = int(pick(rng, (1, 2, 17, 64, 255, D + 1, 2 * D + 1, 3 * D + 1))) if rng.random() < 0.8 else int(rng.integers(1, 256))
        # bands: more of them than channels or fewer, one listed twice, and (with more than one channel) a channel that has none;
        # the reference loops over bands and taps, so long filters get few bands
        nb = int(pick(rng, (1, 2, 3, case["channels"] + 1, 63, 64, 65, 129)))
        nb = max(1, min(nb, 1500 // T))
        case.update(down=D, taps=T, n_bands=nb, band_seed=int(rng.integers(0, 1 << 31)), tap_seed=int(rng.integers(0, 1 << 31)))
        info = info_of(case)
        hist = -(-(T - 1) // D)  # ticks: a call of fewer ticks is shorter than the history
        case = common_draw(rng, self, case, hist, info["block_out"], max(4096 // D, 8))
        case["position"] = draw_position(rng, case["total"] * D)
        return case

    def bands(self, case):
        rng = np.random.default_rng(case["band_seed"])
        C, nb = case["channels"], case["n_bands"]
        live = [c for c in range(C) if c != C // 2] if C > 1 else [0]  # channel C / 2 has no band
        words = [0, 1 << 31, 0x12345678, (1 << 32) - 0x01000001]
        out = [(int(pick(rng, live)), int(pick(rng, words)) if rng.random() < 0.3 else int(rng.integers(0, 1 << 32)),
                int(rng.integers(0, 1 << 32))) for _ in range(nb)]
        if nb > 1:
            out[-1] = out[0]  # a band listed twice
        return out

    def _h(self, case):
        return np.random.default_rng(case["tap_seed"]).standard_normal(case["taps"])

    def host_info(self, case):
        es = (8 if case["precision"] == "f64" else 4) * (2 if case["kind"] == "complex" else 1)
        o = max(0, (32768 // es * 16 // 17 - (case["taps"] - 1)) // case["down"])
        return {"block_out": min(o, 1024) & ~3 if o >= 4 else (2 if o >= 2 else 1)}

    def plan_info(self, env, case):
        return self.module()._bank(env.sd, self._h(case), case["down"], self.bands(case), case["channels"], case["precision"],
                                   case["kind"] == "complex").info()

    def validate(self, case):
        import ctypes as C
        import simpledsp_amd as sd
        from simpledsp_amd import _lib as L
        assert 1 <= case["taps"] <= 4096 and 1 <= case["down"] <= L.RESAMPLE_MAX_FACTOR and 1 <= case["n_bands"] <= 65536, case
        bands = self.bands(case)
        assert len(bands) == case["n_bands"] and all(0 <= b[0] < case["channels"] and 0 <= b[1] < 1 << 32 and 0 <= b[2] < 1 << 32 for b in bands)
        n = C.c_uint64(0)
        for ticks in (case["total"], *case["calls"], *case["calls2"]):
            assert sd.load().sdsp_hip_ddc_out_samples(case["down"], ticks * case["down"], C.byref(n)) == 0 and n.value == ticks, case
        assert 0 <= case["position"] < 1 << 35, case

    def columns(self, case, name, a, t0, t1):
        return a[:, t0 * case["down"]:t1 * case["down"]]

    def data(self, case):
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C, cplx = case["channels"], case["kind"] == "complex"
        return {"in": {"in": t._rand(rng, (C, case["total"] * case["down"]), case["precision"], cplx)},
                "start": {"hist": t._rand(rng, (C, case["taps"] - 1), case["precision"], cplx)}, "position": case["position"]}

    def start_state(self, data, start):
        st = Family.start_state(self, data, start)
        st["position"] = np.array([data["position"]], dtype=np.int64)
        return st

    def step(self, case, data, state, t0, t1):
        from ddc_ref import ddc_ref
        D = case["down"]
        pos = int(state["position"][0])
        y, hist = ddc_ref(self._h(case), data["in"]["in"][:, t0 * D:t1 * D], D, self.bands(case), pos, state["hist"], case["precision"])
        return {"out": y}, {"hist": hist, "position": np.array([pos + (t1 - t0) * D], dtype=np.int64)}

    def open(self, env, case, data, variant, start):
        return _DdcSession(self, env, case, data, variant, start)


class _DdcSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam.module()._bank(env.sd, fam._h(case), case["down"], fam.bands(case), case["channels"],
                                                       case["precision"], case["kind"] == "complex", variant), "ddc plan")
        guarded(self.bank._ensure_plan, "ddc plan")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)
        self.position = case["position"]

    def call(self, t0, t1, wants, io):
        D = self.case["down"]
        n = (t1 - t0) * D
        x = io.inp("in", self.data["in"]["in"][:, t0 * D:t1 * D])
        out = io.out("out", self.case["n_bands"], t1 - t0, np.complex128 if self.case["precision"] == "f64" else np.complex64)
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_ddc_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, n, self.position, state, None),
                 "ddc_process")
        io.sync()
        self.position += n
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy(), "position": np.array([self.position], dtype=np.int64)}



class Duc(Family):
    """a tick is one input sample of every band and U outputs of every channel; `channels` are the output rows"""
    name = "duc"
    buffers = ("in", "out")
    axes = {"precision": ("f32", "f64"), "kind": ("real", "complex"), "variant": (0, 1)}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), kind=pick(rng, ("real", "complex")),
                    channels=draw_channels(rng, top=130))
        U = int(pick(rng, (1, 2, 3, 5, 7, 96), (3, 2, 2, 2, 1, 1)))
        T = int(pick(rng, (1, 2, 17, 64, 255, U, U + 1, 3 * U + 1))) if rng.random() < 0.8 else int(rng.integers(1, 256))
        H = (T - 1) // U
        nb = int(pick(rng, (1, 2, 3, case["channels"] + 1, 63, 64, 65, 129)))
        nb = max(1, min(nb, 600 // (H + 1)))  # the reference loops over bands and over the H + 1 taps of a phase
        case.update(up=U, taps=T, n_bands=nb, band_seed=int(rng.integers(0, 1 << 31)), tap_seed=int(rng.integers(0, 1 << 31)))
        info = info_of(case)
        case = common_draw(rng, self, case, H, info["block_in"], max(4096 // U, 8))
        case["position"] = draw_position(rng, case["total"])
        return case

    bands = Ddc.bands
    _h = Ddc._h

    def host_info(self, case):
        return {"block_in": 64}

    def plan_info(self, env, case):
        return self.module()._bank(env.sd, self._h(case), case["up"], self.bands(case), case["channels"], case["precision"],
                                   case["kind"]).info()

    def validate(self, case):
        import ctypes as C
        import simpledsp_amd as sd
        from simpledsp_amd import _lib as L
        assert 1 <= case["taps"] <= 4096 and 1 <= case["up"] <= L.RESAMPLE_MAX_FACTOR and 1 <= case["n_bands"] <= 65536, case
        bands = self.bands(case)
        assert len(bands) == case["n_bands"] and all(0 <= b[0] < case["channels"] and 0 <= b[1] < 1 << 32 and 0 <= b[2] < 1 << 32 for b in bands)
        n = C.c_uint64(0)
        assert sd.load().sdsp_hip_duc_out_samples(case["up"], case["total"], C.byref(n)) == 0 and n.value == case["total"] * case["up"]
        assert 0 <= case["position"] < 1 << 35, case

    def columns(self, case, name, a, t0, t1):
        return a[:, t0:t1]

    def data(self, case):
        from duc_ref import hist_len
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        nb = case["n_bands"]
        return {"in": {"in": t._rand(rng, (nb, case["total"]), case["precision"])},
                "start": {"hist": t._rand(rng, (nb, hist_len(case["taps"], case["up"])), case["precision"])}, "position": case["position"]}

    start_state = Ddc.start_state

    def step(self, case, data, state, t0, t1):
        from duc_ref import duc_ref
        pos = int(state["position"][0])
        y, hist = duc_ref(self._h(case), data["in"]["in"][:, t0:t1], case["up"], self.bands(case), case["channels"], case["kind"], pos,
                          state["hist"], case["precision"])
        return {"out": y}, {"hist": hist, "position": np.array([pos + (t1 - t0)], dtype=np.int64)}

    def open(self, env, case, data, variant, start):
        return _DucSession(self, env, case, data, variant, start)


class _DucSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam.module()._bank(env.sd, fam._h(case), case["up"], fam.bands(case), case["channels"],
                                                       case["precision"], case["kind"], variant), "duc plan")
        guarded(self.bank._ensure_plan, "duc plan")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)
        self.position = case["position"]

    def call(self, t0, t1, wants, io):
        from ddc_ref import real_dtype
        n, p = t1 - t0, self.case["precision"]
        x = io.inp("in", self.data["in"]["in"][:, t0:t1])
        odt = (np.complex128 if p == "f64" else np.complex64) if self.case["kind"] == "complex" else real_dtype(p)
        out = io.out("out", self.case["channels"], n * self.case["up"], odt)
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_duc_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, n, self.position, state, None),
                 "duc_process")
        io.sync()
        self.position += n
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy(), "position": np.array([self.position], dtype=np.int64)}


class Arb(Family):
    """a tick is one input sample; the outputs of a call follow from the step and the Q32.32 time, which the caller carries"""
    name = "arb"
    buffers = ("in", "out")
    axes = {"precision": ("f32", "f64"), "kind": ("real", "complex"), "interp": ("nearest", "linear"), "variant": (0, 1)}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), kind=pick(rng, ("real", "complex")),
                    interp=pick(rng, ("nearest", "linear")), channels=draw_channels(rng, top=130))
        L = int(pick(rng, (1, 4, 32, 128, 1024)))
        T = int(pick(rng, [t for t in (1, 2, 5, 12, 16, 32) if L * t <= 4096 and t * case["channels"] <= 2200]))  # SDSP_HIP_FIR_MAX_TAPS
        one = 1 << 32
        step = int(pick(rng, (1 << 22, one - 1, one, one + 1, round(0.7317 * one), round(2.37 * one), round(37.5 * one), one // 3 + 12345),
                        (1, 2, 2, 2, 3, 3, 1, 2)))
        max_step = int(pick(rng, (step, 2 * step, 1 << 42))) if step >= one else int(pick(rng, (step, one, 1 << 42)))
        case.update(phases=L, taps=T, step=step, max_step=max_step, tap_seed=int(rng.integers(0, 1 << 31)))
        info = info_of(case)
        unit = max(1, (info["block_out"] * step) >> 32)  # input samples one block of outputs spans
        cap = max(8, min(4096, (6000 << 32) // step))    # at most about 6000 outputs a row
        case = common_draw(rng, self, case, T - 1, unit, cap)
        case["time"] = int(pick(rng, (0, int(rng.integers(0, step)), step - 1, (3 << 32) + 5)))  # the last: no output in the first samples
        return case

    def _h(self, case):
        return np.random.default_rng(case["tap_seed"]).standard_normal(case["phases"] * case["taps"])

    def host_info(self, case):
        return {"block_out": 256}

    def plan_info(self, env, case):
        return self.module()._bank(env.sd, self._h(case), case["phases"], case["taps"], case["max_step"], case["precision"],
                                   case["kind"] == "complex", case["interp"]).info()

    def validate(self, case):
        import ctypes as C
        import simpledsp_amd as sd
        from arb_ref import out_samples
        from simpledsp_amd import _lib as L
        P, T = case["phases"], case["taps"]
        assert P & (P - 1) == 0 and 1 <= P <= L.ARB_MAX_PHASES and T >= 1 and P * T <= 4096, case
        assert L.ARB_MIN_STEP <= case["step"] <= case["max_step"] <= L.ARB_MAX_STEP and 0 <= case["time"] < 1 << 63, case
        n, nt = C.c_uint64(0), C.c_uint64(0)
        assert sd.load().sdsp_hip_arb_out_samples(case["step"], case["time"], case["total"], C.byref(n), C.byref(nt)) == 0, case
        assert (n.value, nt.value) == out_samples(case["step"], case["time"], case["total"]) and n.value < 8000, case

    def columns(self, case, name, a, t0, t1):
        return a[:, t0:t1]

    def data(self, case):
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C, cplx = case["channels"], case["kind"] == "complex"
        return {"in": {"in": t._rand(rng, (C, case["total"]), case["precision"], cplx)},
                "start": {"hist": t._rand(rng, (C, case["taps"] - 1), case["precision"], cplx)}, "position": case["time"]}

    start_state = Ddc.start_state  # "position" is the Q32.32 time here

    def step(self, case, data, state, t0, t1):
        from arb_ref import arb_ref
        y, hist, nxt = arb_ref(self._h(case), case["phases"], case["taps"], data["in"]["in"][:, t0:t1], case["step"],
                               int(state["position"][0]), state["hist"], case["interp"], case["precision"])
        return {"out": y}, {"hist": hist, "position": np.array([nxt], dtype=np.int64)}

    def open(self, env, case, data, variant, start):
        return _ArbSession(self, env, case, data, variant, start)


class _ArbSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam.module()._bank(env.sd, fam._h(case), case["phases"], case["taps"], case["max_step"],
                                                       case["precision"], case["kind"] == "complex", case["interp"], variant,
                                                       step=case["step"]), "arb plan")
        guarded(self.bank._ensure_plan, "arb plan")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)
        self.time = case["time"]

    def call(self, t0, t1, wants, io):
        from arb_ref import out_samples
        n = t1 - t0
        n_out, nxt = out_samples(self.case["step"], self.time, n)
        x = io.inp("in", self.data["in"]["in"][:, t0:t1])
        out = io.out("out", x.rows, n_out, x.dtype)
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_arb_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, x.rows, n, self.case["step"],
                                               self.time, state, None), "arb_process")
        io.sync()
        self.time = nxt
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy(), "position": np.array([self.time], dtype=np.int64)}



_PAIR = {np.dtype(np.int16): np.int32, np.dtype(np.int32): np.int64, np.dtype(np.int64): np.complex128, np.dtype(np.float32): np.complex64}


def _pack(a):
    """(rows, n, 2) interleaved pairs as (rows, n) elements of twice the width, (rows, n) arrays as they are: the strides of the
    integer banks count pairs, and every comparison here is on bits"""
    a = np.ascontiguousarray(a)
    return a if a.ndim == 2 else a.view(_PAIR[a.dtype]).reshape(a.shape[0], a.shape[1])


def _unpack(a, base, cplx):
    a = np.ascontiguousarray(a)
    return a.view(base).reshape(a.shape[0], a.shape[1], 2) if cplx else a


class _CicBase(Family):
    """the two integer banks: a tick is one input sample; rows of interleaved I/Q travel packed (_pack)"""
    buffers = ("in", "out")
    axes = {"kind": ("real", "complex"), "in_dtype": ("i16", "i32"), "out": ("int", "f32"), "variant": (0, 1), "segment": (0, 1, 2),
            "reg_bits": (32, 64)}
    ref = None        # the reference module's name
    max_hist = 2000   # input samples of history at most: a call of exactly the history stays small

    def geometry(self, rng):
        raise NotImplementedError

    def draw(self, rng, info_of):
        ref = __import__(self.ref)
        case = dict(family=self.name, kind=pick(rng, ("real", "complex")), in_dtype=pick(rng, ("i16", "i32")), out=pick(rng, ("int", "f32")),
                    channels=draw_channels(rng), segment=int(pick(rng, (0, 1, 2))))
        N, R, M = self.geometry(rng)
        g = ref.growth(N, R, M)
        width = 32 if case["in_dtype"] == "i32" else 16
        # the widest samples the registers hold, and both sides of the step from 32-bit to 64-bit registers
        bits = sorted({b for b in (min(width, 64 - g), 32 - g, 33 - g, 2) if 2 <= b <= min(width, 64 - g)})
        case.update(order=N, rate=R, delay=M, in_bits=int(pick(rng, bits)))
        case["reg_bits"] = ref.reg_bits(case["in_bits"], N, R, M)
        info = info_of(case)
        return self.finish(rng, case, info)

    def host_info(self, case):
        return {"chunk": 1024}

    def _np_in(self, case):
        return np.int32 if case["in_dtype"] == "i32" else np.int16

    def _bank(self, env, case, variant=0, state=None, position=0):
        raise NotImplementedError

    def plan_info(self, env, case):
        return self._bank(env, case).info()

    def columns(self, case, name, a, t0, t1):
        return a[:, t0:t1]

    def data(self, case):
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        tail = (2,) if case["kind"] == "complex" else ()
        C = case["channels"]
        return {"in": {"in": _pack(t._rand(rng, (C, case["total"]) + tail, case["in_bits"], case["in_dtype"]))},
                "start": {"hist": _pack(t._rand(rng, (C, case["hist"]) + tail, case["in_bits"], case["in_dtype"]))},
                "position": case.get("position", 0)}

    start_state = Ddc.start_state


class Cic(_CicBase):
    name = "cic"
    ref = "cic_ref"

    def geometry(self, rng):
        N, M = int(rng.integers(1, 9)), int(pick(rng, (1, 2)))
        R = int(pick(rng, [r for r in (2, 3, 5, 7, 16, 64, 1024) if N * M * r <= self.max_hist and (r * M) ** N < 1 << 62]))
        return N, R, M

    def finish(self, rng, case, info):
        case = common_draw(rng, self, case, case["order"] * case["delay"] * case["rate"], info["chunk"], 6000)
        case["position"] = draw_position(rng, case["total"])
        return case

    def _bank(self, env, case, variant=0, state=None, position=0):
        return self.module()._bank(env.sd, env.torch, case["order"], case["rate"], case["delay"], case["kind"] == "complex", case["in_dtype"],
                                   case["in_bits"], case["out"], variant, case["segment"], state, position)

    def validate(self, case):
        import ctypes as C
        import simpledsp_amd as sd
        from cic_ref import growth, out_samples
        from simpledsp_amd import _lib as L
        N, R, M = case["order"], case["rate"], case["delay"]
        assert 1 <= N <= L.CIC_MAX_ORDER and 2 <= R <= L.CIC_MAX_DOWN and M in (1, 2) and N * M * R <= L.CIC_MAX_HISTORY, case
        assert 2 <= case["in_bits"] <= (32 if case["in_dtype"] == "i32" else 16) and case["in_bits"] + growth(N, R, M) <= 64, case
        g, n = C.c_uint32(0), C.c_uint64(0)
        assert sd.load().sdsp_hip_cic_growth(N, R, M, C.byref(g)) == 0 and g.value == growth(N, R, M), case
        assert sd.load().sdsp_hip_cic_out_samples(R, case["position"], case["total"], C.byref(n)) == 0, case
        assert n.value == out_samples(R, case["position"], case["total"]) and case["hist"] == N * M * R, case

    def step(self, case, data, state, t0, t1):
        from cic_ref import cic_ref
        cplx, base = case["kind"] == "complex", self._np_in(case)
        pos = int(state["position"][0])
        y, hist = cic_ref(_unpack(data["in"]["in"][:, t0:t1], base, cplx), case["order"], case["rate"], case["delay"], case["reg_bits"], pos,
                          _unpack(state["hist"], base, cplx), case["out"])
        return {"out": _pack(y)}, {"hist": _pack(hist), "position": np.array([pos + t1 - t0], dtype=np.int64)}

    def open(self, env, case, data, variant, start):
        return _CicSession(self, env, case, data, variant, start)


class CicInterp(_CicBase):
    name = "cic_interp"
    ref = "cic_interp_ref"

    def geometry(self, rng):
        N, M = int(rng.integers(1, 9)), int(pick(rng, (1, 2)))
        R = int(pick(rng, [r for r in (2, 3, 5, 7, 16, 64, 1024) if r ** (N - 1) * M ** N < 1 << 62 and N * M * r <= 65536]))
        return N, R, M

    def finish(self, rng, case, info):
        R = case["rate"]
        return common_draw(rng, self, case, case["order"] * case["delay"], max(1, info["chunk"] // R), max(8, 6000 // R))

    def _bank(self, env, case, variant=0, state=None, position=0):
        return self.module()._bank(env.sd, env.torch, case["order"], case["rate"], case["delay"], case["kind"] == "complex", case["in_dtype"],
                                   case["in_bits"], case["out"], variant, case["segment"], state)

    def validate(self, case):
        from cic_interp_ref import growth
        from simpledsp_amd import _lib as L
        N, R, M = case["order"], case["rate"], case["delay"]
        assert 1 <= N <= L.CIC_MAX_ORDER and 2 <= R <= L.CIC_MAX_DOWN and M in (1, 2) and N * M * R <= L.CIC_MAX_HISTORY, case
        assert 2 <= case["in_bits"] <= (32 if case["in_dtype"] == "i32" else 16) and case["in_bits"] + growth(N, R, M) <= 64, case
        assert case["total"] * R < 1 << 31 and case["hist"] == N * M, case

    def step(self, case, data, state, t0, t1):
        from cic_interp_ref import cic_interp_ref
        cplx, base = case["kind"] == "complex", self._np_in(case)
        y, hist = cic_interp_ref(_unpack(data["in"]["in"][:, t0:t1], base, cplx), case["order"], case["rate"], case["delay"],
                                 case["reg_bits"], _unpack(state["hist"], base, cplx), case["out"])
        return {"out": _pack(y)}, {"hist": _pack(hist), "position": state["position"]}

    def open(self, env, case, data, variant, start):
        return _CicSession(self, env, case, data, variant, start)


class _CicSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam._bank(env, case, variant), "cic plan")
        guarded(self.bank._ensure_plan, "cic plan")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)
        self.position = case.get("position", 0)
        self.decimates = fam.name == "cic"
        base = np.float32 if case["out"] == "f32" else (np.int32 if case["reg_bits"] == 32 else np.int64)
        self.out_dtype = _PAIR[np.dtype(base)] if case["kind"] == "complex" else base

    def call(self, t0, t1, wants, io):
        n, R = t1 - t0, self.case["rate"]
        x = io.inp("in", self.data["in"]["in"][:, t0:t1])
        n_out = ((self.position + n) // R - self.position // R) if self.decimates else n * R
        out = io.out("out", x.rows, n_out, self.out_dtype)
        state = None if self.null else self.st.data_ptr()
        if self.decimates:
            rc_check(self.lib.sdsp_hip_cic_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, x.rows, n, self.position, state,
                                                   None), "cic_process")
            self.position += n
        else:
            rc_check(self.lib.sdsp_hip_cic_interp_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, x.rows, n, state, None),
                     "cic_interp_process")
        io.sync()
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy(), "position": np.array([self.position], dtype=np.int64)}



class Beam(SampleFamily):
    """`channels` are the output rows, groups x beams; the input rows are groups x sensors"""
    name = "beam"
    buffers = ("in", "out")
    axes = {"precision": ("f32", "f64"), "kind": ("real", "complex"), "variant": (0, 1), "spread": ("small", "large"),
            "many_beams": (0, 1)}
    FAR = 9000  # a delay spread no LDS line of the fused kernel holds (32 KiB: 8192 floats): the chunk table splits there

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), kind=pick(rng, ("real", "complex")))
        sensors, beams = int(pick(rng, (1, 2, 3, 5, 16))), int(pick(rng, (1, 2, 4, 5, 9, 33)))  # chunks of four beams: one and several
        spread = pick(rng, ("small", "large"), (3, 1))
        T = int(pick(rng, (1, 2, 5, 16, 33)))
        rows = draw_channels(rng)
        groups = max(1, -(-rows // beams))
        # the reference loops over groups, entries and taps: many rows get short filters and few sensors per beam
        per_beam = max(1, min(sensors, 1200 // (groups * beams * T)))
        if groups * beams * T > 1200:
            T = max(1, 1200 // (groups * beams))
        case.update(sensors=sensors, beams=beams, groups=groups, channels=groups * beams, taps=T, spread=spread, many_beams=int(beams > 4),
                    per_beam=per_beam, entry_seed=int(rng.integers(0, 1 << 31)))
        info = info_of(case)
        H = self.hist_of(case)
        return common_draw(rng, self, case, H, info["block_out"], 3000)

    def entries(self, case):
        t = self.module()
        rng = np.random.default_rng(case["entry_seed"])
        cplx = case["kind"] == "complex"
        out = []
        for b in range(case["beams"]):
            if case["beams"] > 2 and b == 1:
                continue  # a beam without an entry: its outputs are +0
            use = sorted(rng.choice(case["sensors"], size=min(case["per_beam"], case["sensors"]), replace=False).tolist())
            for c in use:
                out.append((b, int(c), int(rng.integers(0, 8)), t._taps(rng, case["taps"], cplx)))
        if case["spread"] == "large":  # the first and the last entry far apart on the delay axis
            b, c, _, g = out[-1]
            out[-1] = (b, c, self.FAR, g)
        return out

    def hist_of(self, case):
        from beam_ref import hist_len
        return hist_len(self.entries(case), case["taps"])

    def host_info(self, case):
        return {"block_out": 256}

    def _make(self, env, case, variant=0, state=None):
        return self.module()._bank(env.sd, self.entries(case), case["sensors"], case["beams"], case["taps"], case["groups"], case["precision"],
                                   case["kind"] == "complex", variant, state)

    def plan_info(self, env, case):
        return self._make(env, case).info()

    def validate(self, case):
        from simpledsp_amd import _lib as L
        ent = self.entries(case)
        assert 1 <= case["taps"] <= L.BEAM_MAX_TAPS and 1 <= case["sensors"] <= L.BEAM_MAX_ROWS and 1 <= case["beams"] <= L.BEAM_MAX_ROWS, case
        assert case["groups"] >= 1 and 1 <= len(ent) <= L.BEAM_MAX_ENTRIES and all(0 <= e[2] <= L.BEAM_MAX_DELAY for e in ent), case
        keys = [(e[0], e[1]) for e in ent]
        assert keys == sorted(set(keys)) and all(b < case["beams"] and c < case["sensors"] for b, c in keys), case
        assert case["hist"] == max(e[2] for e in ent) + case["taps"] - 1, case

    def data(self, case):
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        rows, cplx = case["groups"] * case["sensors"], case["kind"] == "complex"
        return {"in": {"in": t._rand(rng, (rows, case["total"]), case["precision"], cplx)},
                "start": {"hist": t._rand(rng, (rows, case["hist"]), case["precision"], cplx)}}

    def step(self, case, data, state, t0, t1):
        from beam_ref import beam_ref
        y, hist = beam_ref(self.entries(case), data["in"]["in"][:, t0:t1], case["sensors"], case["beams"], case["taps"], case["groups"],
                           state["hist"], case["precision"])
        return {"out": y}, {"hist": hist}

    def open(self, env, case, data, variant, start):
        return _BeamSession(self, env, case, data, variant, start)


class _BeamSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam._make(env, case, variant), "beam plan")
        guarded(self.bank._ensure_plan, "beam plan")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)

    def call(self, t0, t1, wants, io):
        n = t1 - t0
        x = io.inp("in", self.data["in"]["in"][:, t0:t1])
        out = io.out("out", self.case["channels"], n, x.dtype)
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_beam_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, n, state, None), "beam_process")
        io.sync()
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy()}



class Resample(Family):
    """a tick is q = D / gcd(U, D) input samples, the unit the entry takes calls in, and q U / D outputs.  The reference sums in
    double: f64 is held to its bits, f32 to the 1e-6 of tests/test_gpu_resample.py (`_matches`); the splits and variants to bits"""
    name = "resample"
    variants = (0, 1, 2)
    buffers = ("in", "out")
    axes = {"precision": ("f32", "f64"), "variant": (0, 1, 2), "dec_kernel": (0, 1)}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), channels=draw_channels(rng))
        # U = 1 with D in {1, 2, 4, 8, 16} takes the decimating kernel, every other ratio the polyphase one
        U, D = pick(rng, ((1, 1), (1, 2), (1, 4), (1, 16), (1, 3), (2, 1), (3, 1), (2, 3), (3, 2), (5, 7), (160, 147), (147, 160)))
        T = int(pick(rng, (1, 2, 16, 17, 64, 65, 255, U, U + 1, 2 * U + 1))) if rng.random() < 0.8 else int(rng.integers(1, 256))
        q = D // np.gcd(U, D).item()
        case.update(up=int(U), down=int(D), taps=T, q=int(q), dec_kernel=int(U == 1 and D in (1, 2, 4, 8, 16)),
                    tap_seed=int(rng.integers(0, 1 << 31)))
        info_of(case)
        H = (T - 1) // U
        # the plan's info() names no block: the unit is nominal, 256 input samples
        return common_draw(rng, self, case, -(-H // q), max(1, 256 // q), max(4, 3000 // max(q, (q * U) // D)))

    def _h(self, case):
        return np.random.default_rng(case["tap_seed"]).standard_normal(case["taps"])

    def host_info(self, case):
        return {}

    def plan_info(self, env, case):
        return self.module()._bank(env.sd, self._h(case), case["up"], case["down"], case["channels"], case["precision"]).info()

    def validate(self, case):
        import ctypes as C
        import simpledsp_amd as sd
        from resample_ref import q_of
        from simpledsp_amd import _lib as L
        assert 1 <= case["taps"] <= 4096 and 1 <= case["up"] <= L.RESAMPLE_MAX_FACTOR and 1 <= case["down"] <= L.RESAMPLE_MAX_FACTOR, case
        assert case["q"] == q_of(case["up"], case["down"]), case
        n = C.c_uint64(0)
        for ticks in (case["total"], *case["calls"], *case["calls2"]):
            assert sd.load().sdsp_hip_resample_out_samples(case["up"], case["down"], ticks * case["q"], C.byref(n)) == 0, case
            assert n.value == ticks * case["q"] * case["up"] // case["down"], case

    def columns(self, case, name, a, t0, t1):
        return a[:, t0 * case["q"]:t1 * case["q"]]

    def _dt(self, case):
        return np.float64 if case["precision"] == "f64" else np.float32

    def data(self, case):
        rng = np.random.default_rng(case["data_seed"])
        C, H = case["channels"], (case["taps"] - 1) // case["up"]
        return {"in": {"in": rng.standard_normal((C, case["total"] * case["q"])).astype(self._dt(case))},
                "start": {"hist": rng.standard_normal((C, H)).astype(self._dt(case))}}

    def step(self, case, data, state, t0, t1):
        from resample_ref import resample_ref
        q = case["q"]
        h = self._h(case).astype(self._dt(case))  # the taps as the plan rounds them
        y, hist = resample_ref(h, data["in"]["in"][:, t0 * q:t1 * q], case["up"], case["down"], state["hist"])
        return {"out": y}, {"hist": hist.astype(self._dt(case))}  # the history is a copy of inputs: exact in the precision

    def same(self, name, got, want, case, data=None):
        if name.startswith("state:"):
            return self.module()._matches(got, want, "f64")
        return self.module()._matches(got, want, case["precision"])

    def open(self, env, case, data, variant, start):
        return _ResampleSession(self, env, case, data, variant, start)


class _ResampleSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam.module()._bank(env.sd, fam._h(case), case["up"], case["down"], case["channels"], case["precision"],
                                                       variant), "resample plan")
        guarded(self.bank._ensure_plan, "resample plan")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)

    def call(self, t0, t1, wants, io):
        q = self.case["q"]
        n = (t1 - t0) * q
        x = io.inp("in", self.data["in"]["in"][:, t0 * q:t1 * q])
        out = io.out("out", x.rows, n * self.case["up"] // self.case["down"], x.dtype)
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_resample_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, x.rows, n, state, None),
                 "resample_process")
        io.sync()
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy()}



class Stft(Family):
    """a tick is one hop of samples and one frame of bins.  Against the double reference the spectrum is held to the tolerance of
    tests/test_gpu_stft.py (`_tol`), the history to its bits; the splits to bits, as the header promises.  The variants are the inner
    transform's: the header does not call them bit-identical, and a transform without the variant refuses it (UNSUPPORTED), which the
    session takes as documented and stays at variant 0"""
    name = "stft"
    cross_variants = (0,)
    buffers = ("in", "out")
    axes = {"precision": ("f32", "f64"), "output": ("complex", "power", "magnitude"), "variant": (0, 1), "slices": ("one", "several")}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), output=pick(rng, ("complex", "power", "magnitude")),
                    channels=draw_channels(rng))
        N = int(pick(rng, (32, 64, 256, 1024, 8192), (3, 3, 2, 1, 2)))  # 8192: the first f64 real-input size with a variant 1
        if N == 8192:
            case["channels"] = min(case["channels"], 65)  # rows of 8192: a wave and one more
        hop = int(pick(rng, sorted({N, N // 2, N // 4, 3, N - 1, 1 + N // 3})))
        per_slice = int(pick(rng, (0, 1, 3, 7)))  # frames a workspace slice holds; 0: the default workspace, one slice
        case.update(n_fft=N, hop=hop, per_slice=per_slice, slices="several" if per_slice else "one")
        info = info_of(case)
        hist = -(-(N - hop) // hop)
        cap = max(4, min(200000 // (case["channels"] * N), 3000 // hop))  # frames: the reference transforms channels x frames rows
        return common_draw(rng, self, case, hist, slice_frames(info, N * (8 if case["precision"] == "f64" else 4)), cap)

    def host_info(self, case):
        return {"workspace_bytes": case["per_slice"] * case["n_fft"] * (8 if case["precision"] == "f64" else 4) or DEFAULT_WORKSPACE}

    def _window(self, case):
        import scipy.signal
        return scipy.signal.get_window("hann", case["n_fft"])

    def _make(self, env, case):
        rs = 8 if case["precision"] == "f64" else 4
        return env.sd.stft_bank(case["n_fft"], case["hop"], case["channels"], window=self._window(case), output=case["output"],
                                precision=_prec(env.sd, case["precision"]), workspace_bytes=case["per_slice"] * case["n_fft"] * rs)

    def plan_info(self, env, case):
        return self._make(env, case).info()

    def validate(self, case):
        import ctypes as C
        import simpledsp_amd as sd
        N, hop = case["n_fft"], case["hop"]
        assert N & (N - 1) == 0 and 32 <= N <= 32768 and 1 <= hop <= N, case
        n = C.c_uint64(0)
        for ticks in (case["total"], *case["calls"], *case["calls2"]):
            assert sd.load().sdsp_hip_stft_frames(hop, ticks * hop, C.byref(n)) == 0 and n.value == ticks, case

    def columns(self, case, name, a, t0, t1):
        return a[:, t0 * case["hop"]:t1 * case["hop"]]

    def _dt(self, case):
        return np.float64 if case["precision"] == "f64" else np.float32

    def data(self, case):
        rng = np.random.default_rng(case["data_seed"])
        C = case["channels"]
        return {"in": {"in": rng.standard_normal((C, case["total"] * case["hop"])).astype(self._dt(case))},
                "start": {"hist": rng.standard_normal((C, case["n_fft"] - case["hop"])).astype(self._dt(case))}}

    def step(self, case, data, state, t0, t1):
        from stft_ref import stft_ref
        hop = case["hop"]
        w = self._window(case).astype(self._dt(case)).astype(np.float64)  # the window as the plan rounds it
        y, hist = stft_ref(data["in"]["in"][:, t0 * hop:t1 * hop], case["n_fft"], hop, w, state["hist"], case["output"])
        return {"out": y.reshape(y.shape[0], -1)}, {"hist": hist.astype(self._dt(case))}

    def same(self, name, got, want, case, data=None):
        from conftest import rel_max_err
        if name.startswith("state:"):
            return np.array_equal(got, want)
        if got.shape != want.shape:
            return False
        bins = case["n_fft"] // 2 + 1
        shape = (got.shape[0], -1, bins)
        return want.size == 0 or rel_max_err(got.reshape(shape), want.reshape(shape)) <= self.module()._tol(case["precision"], case["n_fft"],
                                                                                                         case["output"])

    def open(self, env, case, data, variant, start):
        return _StftSession(self, env, case, data, variant, start)


class _StftSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam._make(env, case), "stft plan")
        guarded(self.bank._ensure_plan, "stft plan")
        set_inner_variant(fam, case, self.lib.sdsp_hip_stft_plan_set_variant, self.bank._plan, variant, "stft_plan_set_variant")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)

    def call(self, t0, t1, wants, io):
        hop, bins, p = self.case["hop"], self.case["n_fft"] // 2 + 1, self.case["precision"]
        F = t1 - t0
        x = io.inp("in", self.data["in"]["in"][:, t0 * hop:t1 * hop])
        odt = (np.complex128 if p == "f64" else np.complex64) if self.case["output"] == "complex" else x.dtype
        out = io.out("out", x.rows, F * bins, odt)
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_stft_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, x.rows, F * hop, state, None),
                 "stft_process")
        io.sync()
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy()}



class Pfb(Family):
    """a tick is one hop of samples and one frame of sub-bands.  `variant` is the fold form (sdsp_hip_pfb_plan_set_fold_form: "both
    forms give the same bits"), which check (d) compares; `fft_variant` is the inner transform's, refused with UNSUPPORTED where the
    transform has none.  Against the double reference: `_err` <= `_tol` of tests/test_gpu_pfb.py; history, splits and forms: bits"""
    name = "pfb"
    buffers = ("in", "out")
    axes = {"precision": ("f32", "f64"), "kind": ("real", "complex"), "phase": ("time", "frame"), "variant": (0, 1), "fft_variant": (0, 1),
            "slices": ("one", "several")}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), kind=pick(rng, ("real", "complex")),
                    phase=pick(rng, ("time", "frame")), channels=draw_channels(rng), fft_variant=int(pick(rng, (0, 1))))
        m = int(pick(rng, (16, 32, 64, 256) if case["kind"] == "complex" else (32, 64, 256)))
        P = int(pick(rng, (1, 2, 3, 8)))
        hop = int(pick(rng, sorted({m, m // 2, m // 4, 3 * m // 4, 3, 1})))  # the sliding fold where hop divides m, else the plain one
        per_slice = int(pick(rng, (0, 1, 3, 7)))
        case.update(m=m, taps_per_channel=P, hop=hop, per_slice=per_slice, slices="several" if per_slice else "one",
                    tap_seed=int(rng.integers(0, 1 << 31)))
        info = info_of(case)
        hist = -(-(m * P - hop) // hop)
        cap = max(4, min(1000000 // (case["channels"] * m * P), 3000 // hop))
        case = common_draw(rng, self, case, hist, slice_frames(info, self.frame_bytes(case)), cap)
        case["position"] = draw_position(rng, case["total"] * hop)
        return case

    def host_info(self, case):
        return {"workspace_bytes": case["per_slice"] * self.frame_bytes(case) or DEFAULT_WORKSPACE}

    def frame_bytes(self, case):
        return case["m"] * np.dtype(self._in_dtype(case)).itemsize

    def _taps(self, case):
        return np.random.default_rng(case["tap_seed"]).standard_normal(case["m"] * case["taps_per_channel"])

    def _in_dtype(self, case):
        if case["kind"] == "complex":
            return np.complex128 if case["precision"] == "f64" else np.complex64
        return np.float64 if case["precision"] == "f64" else np.float32

    def _make(self, env, case):
        return self.module()._bank(env.sd, case["m"], case["taps_per_channel"], case["hop"], case["channels"], case["precision"],
                                   case["kind"] == "complex", case["phase"], self._taps(case),
                                   workspace_bytes=case["per_slice"] * self.frame_bytes(case))

    def plan_info(self, env, case):
        return self._make(env, case).info()

    def validate(self, case):
        import ctypes as C
        import simpledsp_amd as sd
        m, P, hop = case["m"], case["taps_per_channel"], case["hop"]
        assert m & (m - 1) == 0 and (16 if case["kind"] == "complex" else 32) <= m <= 32768 and 1 <= P <= 64 and 1 <= hop <= m, case
        n = C.c_uint64(0)
        for ticks in (case["total"], *case["calls"], *case["calls2"]):
            assert sd.load().sdsp_hip_pfb_frames(hop, ticks * hop, C.byref(n)) == 0 and n.value == ticks, case
        assert 0 <= case["position"] < 1 << 35, case

    def columns(self, case, name, a, t0, t1):
        return a[:, t0 * case["hop"]:t1 * case["hop"]]

    def data(self, case):
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C, cplx = case["channels"], case["kind"] == "complex"
        return {"in": {"in": t._rand(rng, (C, case["total"] * case["hop"]), case["precision"], cplx)},
                "start": {"hist": t._rand(rng, (C, case["m"] * case["taps_per_channel"] - case["hop"]), case["precision"], cplx)},
                "position": case["position"]}

    start_state = Ddc.start_state

    def step(self, case, data, state, t0, t1):
        from pfb_ref import pfb_ref
        hop = case["hop"]
        rdt = np.float64 if case["precision"] == "f64" else np.float32
        pos = int(state["position"][0])
        y, hist = pfb_ref(data["in"]["in"][:, t0 * hop:t1 * hop], case["m"], case["taps_per_channel"], hop,
                          self._taps(case).astype(rdt).astype(np.float64), state["hist"], case["phase"], pos)
        return ({"out": y.reshape(y.shape[0], -1)},
                {"hist": hist.astype(self._in_dtype(case)), "position": np.array([pos + (t1 - t0) * hop], dtype=np.int64)})

    def same(self, name, got, want, case, data=None):
        t = self.module()
        if name.startswith("state:"):
            return np.array_equal(got, want)
        if got.shape != want.shape:
            return False
        return want.size == 0 or t._err(got, want) <= t._tol(case["precision"], case["m"] * case["taps_per_channel"])

    def open(self, env, case, data, variant, start):
        return _PfbSession(self, env, case, data, variant, start)


class _PfbSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam._make(env, case), "pfb plan")
        guarded(self.bank._ensure_plan, "pfb plan")
        rc_check(self.lib.sdsp_hip_pfb_plan_set_fold_form(self.bank._plan, variant), "pfb_plan_set_fold_form")
        set_inner_variant(fam, case, self.lib.sdsp_hip_pfb_plan_set_variant, self.bank._plan, case["fft_variant"], "pfb_plan_set_variant")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)
        self.position = case["position"]

    def call(self, t0, t1, wants, io):
        case = self.case
        hop, F = case["hop"], t1 - t0
        bins = case["m"] if case["kind"] == "complex" else case["m"] // 2 + 1
        x = io.inp("in", self.data["in"]["in"][:, t0 * hop:t1 * hop])
        out = io.out("out", x.rows, F * bins, np.complex128 if case["precision"] == "f64" else np.complex64)
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_pfb_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, x.rows, F * hop, self.position, state,
                                               None), "pfb_process")
        io.sync()
        self.position += F * hop
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy(), "position": np.array([self.position], dtype=np.int64)}



class Istft(Family):
    """a tick is one frame of bins in and one hop of samples out; the state is the pending overlap-add sums.  Against the double
    reference: `_tol` of tests/test_gpu_istft.py for the samples, four times that for the pending sums (as tests/test_gpu_wide_strides.py
    holds them); the splits: bits, as the header promises"""
    name = "istft"
    cross_variants = (0,)
    buffers = ("in", "out")
    axes = {"precision": ("f32", "f64"), "variant": (0, 1), "slices": ("one", "several")}

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), channels=draw_channels(rng))
        N = int(pick(rng, (32, 64, 256, 1024, 8192), (3, 3, 2, 1, 2)))  # 8192: the first f64 real-input size with a variant 1
        if N == 8192:
            case["channels"] = min(case["channels"], 65)  # rows of 8192: a wave and one more
        hop = int(pick(rng, sorted({N, N // 2, N // 4, 1 if N <= 64 else N // 8})))  # Hamming at hop = N, Hann below (NOLA)
        per_slice = int(pick(rng, (0, 1, 3, 7)))
        case.update(n_fft=N, hop=hop, per_slice=per_slice, slices="several" if per_slice else "one")
        info = info_of(case)
        hist = -(-(N - hop) // hop)
        cap = max(4, min(200000 // (case["channels"] * N), 3000 // hop))
        return common_draw(rng, self, case, hist, slice_frames(info, N * (8 if case["precision"] == "f64" else 4)), cap)

    def host_info(self, case):
        return {"workspace_bytes": case["per_slice"] * case["n_fft"] * (8 if case["precision"] == "f64" else 4) or DEFAULT_WORKSPACE}

    def _window(self, case):
        import scipy.signal
        return scipy.signal.get_window("hann" if case["hop"] < case["n_fft"] else "hamming", case["n_fft"])

    def _make(self, env, case):
        rs = 8 if case["precision"] == "f64" else 4
        return self.module()._bank(env.sd, case["n_fft"], case["hop"], case["channels"], case["precision"],
                                   workspace_bytes=case["per_slice"] * case["n_fft"] * rs)

    def plan_info(self, env, case):
        return self._make(env, case).info()

    def validate(self, case):
        from istft_ref import synthesis_window_ref
        N, hop = case["n_fft"], case["hop"]
        assert N & (N - 1) == 0 and 32 <= N <= 32768 and 1 <= hop <= N, case
        assert synthesis_window_ref(self._window(case), N, hop) is not None, (case, "the window breaks NOLA")

    def columns(self, case, name, a, t0, t1):
        bins = case["n_fft"] // 2 + 1
        return a[:, t0 * bins:t1 * bins]

    def _dt(self, case):
        return np.float64 if case["precision"] == "f64" else np.float32

    def data(self, case):
        rng = np.random.default_rng(case["data_seed"])
        C, bins = case["channels"], case["n_fft"] // 2 + 1
        X = rng.standard_normal((C, case["total"] * bins)) + 1j * rng.standard_normal((C, case["total"] * bins))
        return {"in": {"in": X.astype(np.complex128 if case["precision"] == "f64" else np.complex64)},
                "start": {"pend": rng.standard_normal((C, case["n_fft"] - case["hop"])).astype(self._dt(case))}}

    def step(self, case, data, state, t0, t1):
        from istft_ref import istft_ref, synthesis_window_ref
        N, hop, bins = case["n_fft"], case["hop"], case["n_fft"] // 2 + 1
        X = data["in"]["in"][:, t0 * bins:t1 * bins].reshape(case["channels"], t1 - t0, bins)
        y, pend = istft_ref(X, N, hop, synthesis_window_ref(self._window(case), N, hop), state["pend"])
        return {"out": y}, {"pend": pend}

    def same(self, name, got, want, case, data=None):
        from conftest import rel_max_err
        if got.shape != want.shape:
            return False
        tol = self.module()._tol(case["precision"], case["n_fft"], case["hop"])
        return want.size == 0 or rel_max_err(got, want) <= (4 * tol if name.startswith("state:") else tol)

    def open(self, env, case, data, variant, start):
        return _IstftSession(self, env, case, data, variant, start)


class _IstftSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        pend = data["start"]["pend"] if start == "random" else np.zeros_like(data["start"]["pend"])
        self.bank = guarded(lambda: fam._make(env, case), "istft plan")
        guarded(self.bank._ensure_plan, "istft plan")
        set_inner_variant(fam, case, self.lib.sdsp_hip_istft_plan_set_variant, self.bank._plan, variant, "istft_plan_set_variant")
        self.st = env.torch.from_numpy(np.ascontiguousarray(pend)).to(env.device)

    def call(self, t0, t1, wants, io):
        hop, bins, F = self.case["hop"], self.case["n_fft"] // 2 + 1, t1 - t0
        x = io.inp("in", self.data["in"]["in"][:, t0 * bins:t1 * bins])
        out = io.out("out", x.rows, F * hop, self.fam._dt(self.case))
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_istft_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, x.rows, F, state, None),
                 "istft_process")
        io.sync()
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"pend": self.st.cpu().numpy().copy()}



class PfbSynth(Family):
    """the inverse channelizer: a tick is one frame of sub-bands in and one hop of samples out; the state is the pending sums.
    `variant` is the unfold form ("both forms give the same bits"), `fft_variant` the inner transform's.  Against the double reference
    the samples and the pending sums are held to the absolute `_bound` of tests/test_gpu_pfb_synth.py; splits and forms: bits"""
    name = "pfb_synth"
    buffers = ("in", "out")
    axes = Pfb.axes

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), kind=pick(rng, ("real", "complex")),
                    phase=pick(rng, ("time", "frame")), channels=draw_channels(rng), fft_variant=int(pick(rng, (0, 1))))
        m = int(pick(rng, (16, 32, 64, 256) if case["kind"] == "complex" else (32, 64, 256)))
        P = int(pick(rng, (1, 2, 3, 8)))
        hop = int(pick(rng, sorted({m, m // 2, m // 4, 3 * m // 4, 3, 1})))  # the sliding unfold at hop = m, else the plain one
        per_slice = int(pick(rng, (0, 1, 3, 7)))
        case.update(m=m, taps_per_channel=P, hop=hop, per_slice=per_slice, slices="several" if per_slice else "one",
                    tap_seed=int(rng.integers(0, 1 << 31)))
        info = info_of(case)
        hist = -(-(m * P - hop) // hop)
        cap = max(4, min(1000000 // (case["channels"] * m * P), 3000 // hop))
        case = common_draw(rng, self, case, hist, slice_frames(info, self.frame_bytes(case)), cap)
        case["position"] = draw_position(rng, case["total"] * hop)
        return case

    def host_info(self, case):
        return {"workspace_bytes": case["per_slice"] * self.frame_bytes(case) or DEFAULT_WORKSPACE}

    def frame_bytes(self, case):
        return case["m"] * np.dtype(self._out_dtype(case)).itemsize

    def _g(self, case):
        return np.random.default_rng(case["tap_seed"]).uniform(-1, 1, case["m"] * case["taps_per_channel"])

    def _out_dtype(self, case):
        if case["kind"] == "complex":
            return np.complex128 if case["precision"] == "f64" else np.complex64
        return np.float64 if case["precision"] == "f64" else np.float32

    def _bins(self, case):
        return case["m"] if case["kind"] == "complex" else case["m"] // 2 + 1

    def _make(self, env, case):
        return self.module()._bank(env.sd, case["m"], case["taps_per_channel"], case["hop"], case["channels"], case["precision"],
                                   case["kind"] == "complex", case["phase"], self._g(case),
                                   workspace_bytes=case["per_slice"] * self.frame_bytes(case))

    def plan_info(self, env, case):
        return self._make(env, case).info()

    def validate(self, case):
        m, P, hop = case["m"], case["taps_per_channel"], case["hop"]
        assert m & (m - 1) == 0 and (16 if case["kind"] == "complex" else 32) <= m <= 32768 and 1 <= P <= 64 and 1 <= hop <= m, case
        assert 0 <= case["position"] < 1 << 35 and case["total"] * hop < 1 << 31, case

    def columns(self, case, name, a, t0, t1):
        return a[:, t0 * self._bins(case):t1 * self._bins(case)]

    def data(self, case):
        from pfb_synth_ref import pfb_synth_frames_ref
        t = self.module()
        rng = np.random.default_rng(case["data_seed"])
        C, bins, cplx = case["channels"], self._bins(case), case["kind"] == "complex"
        X = t._spectra(rng, (C, case["total"], bins), case["precision"])
        frames = pfb_synth_frames_ref(X, case["m"], case["taps_per_channel"], case["hop"], case["phase"], case["position"], cplx)
        vmax = float(np.abs(frames).max()) if frames.size else 1.0
        pend = rng.uniform(-1, 1, (C, case["m"] * case["taps_per_channel"] - case["hop"]))
        if cplx:
            pend = (pend + 1j * rng.uniform(-1, 1, pend.shape)) / np.sqrt(2)
        return {"in": {"in": X.reshape(C, -1)}, "start": {"pend": (pend * vmax).astype(self._out_dtype(case))}, "vmax": vmax,
                "position": case["position"]}

    start_state = Ddc.start_state

    def step(self, case, data, state, t0, t1):
        from pfb_synth_ref import pfb_synth_ref
        bins, hop = self._bins(case), case["hop"]
        rdt = np.float64 if case["precision"] == "f64" else np.float32
        pos = int(state["position"][0])
        X = data["in"]["in"][:, t0 * bins:t1 * bins].reshape(case["channels"], t1 - t0, bins)
        y, pend = pfb_synth_ref(X, case["m"], case["taps_per_channel"], hop, self._g(case).astype(rdt).astype(np.float64), state["pend"],
                                case["phase"], pos, cplx=case["kind"] == "complex")
        return {"out": y}, {"pend": pend, "position": np.array([pos + (t1 - t0) * hop], dtype=np.int64)}

    def same(self, name, got, want, case, data=None):
        if name == "state:position":
            return np.array_equal(got, want)
        if got.shape != want.shape:
            return False
        bound = self.module()._bound(case["precision"], case["m"], case["taps_per_channel"], case["hop"], data["vmax"])
        return want.size == 0 or float(np.abs(got - want).max()) <= bound

    def open(self, env, case, data, variant, start):
        return _PfbSynthSession(self, env, case, data, variant, start)


class _PfbSynthSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        pend = data["start"]["pend"] if start == "random" else np.zeros_like(data["start"]["pend"])
        self.bank = guarded(lambda: fam._make(env, case), "pfb_synth plan")
        guarded(self.bank._ensure_plan, "pfb_synth plan")
        rc_check(self.lib.sdsp_hip_pfb_synth_plan_set_unfold_form(self.bank._plan, variant), "pfb_synth_plan_set_unfold_form")
        set_inner_variant(fam, case, self.lib.sdsp_hip_pfb_synth_plan_set_variant, self.bank._plan, case["fft_variant"],
                          "pfb_synth_plan_set_variant")
        self.st = env.torch.from_numpy(np.ascontiguousarray(pend)).to(env.device)
        self.position = case["position"]

    def call(self, t0, t1, wants, io):
        fam, case = self.fam, self.case
        bins, hop, F = fam._bins(case), case["hop"], t1 - t0
        x = io.inp("in", self.data["in"]["in"][:, t0 * bins:t1 * bins])
        out = io.out("out", x.rows, F * hop, fam._out_dtype(case))
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_pfb_synth_process(self.bank._plan, x.ptr, x.stride, out.ptr, out.stride, x.rows, F, self.position, state,
                                                     None), "pfb_synth_process")
        io.sync()
        self.position += F * hop
        return self.collect({"out": out})

    def state(self):
        return {} if self.null else {"pend": self.st.cpu().numpy().copy(), "position": np.array([self.position], dtype=np.int64)}



class _Padded:
    """a (rows, cols) in-out buffer of a session with `pad` sentinel columns, kept across the calls of a stream (accumulators)"""

    def __init__(self, env, name, content, pad):
        content = np.ascontiguousarray(content)
        self.name, self.rows, self.cols, self.width = name, content.shape[0], content.shape[1], content.shape[1] + pad
        a = np.full(self.rows * self.width + 4, sentinel(content.dtype), dtype=content.dtype)
        a[:self.rows * self.width].reshape(self.rows, self.width)[:, :self.cols] = content
        self.before = a.copy()
        self.flat = env.torch.from_numpy(a.copy()).to(env.device)

    @property
    def ptr(self):
        return self.flat.data_ptr()

    def get(self):
        return self.flat.cpu().numpy()[:self.rows * self.width].reshape(self.rows, self.width)[:, :self.cols].copy()

    def faults(self):
        after = self.flat.cpu().numpy()
        body = np.zeros(after.size, dtype=bool)
        body[:self.rows * self.width].reshape(self.rows, self.width)[:, :self.cols] = True
        count, first = bit_diff(after[~body], self.before[~body])
        return [(f"padding of '{self.name}'", count, first)] if count else []


class Welch(SampleFamily):
    """no output rows: a call adds its segments' powers into the caller's accumulator, which is part of the state here (with the
    history, the position and the segment count).  The header promises a split's agreement with one call "to rounding" only, so the
    accumulator of a split is held to `_peak_err` <= `_tol` of tests/test_gpu_welch.py, like the one call against the reference;
    history, position and count to bits.  One kernel variant: check (d) is empty.  NULL state is legal at position 0 only"""
    name = "welch"
    variants = (0,)
    buffers = ("in", "acc")
    split_tol = ("state:acc",)
    axes = {"precision": ("f32", "f64"), "detrend": ("none", "constant", "linear"), "slices": ("one", "several")}
    acc_names = ("acc",)

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), detrend=pick(rng, ("none", "constant", "linear")),
                    channels=draw_channels(rng))
        N = int(pick(rng, (32, 64, 256), (3, 3, 2)))
        hop = int(pick(rng, sorted({N, N // 2, N // 4, 7 * N // 32 + 1, 1})))
        per_slice = int(pick(rng, (0, 1, 3, 7)))  # segments a workspace slice holds; 0: the default workspace, one slice
        case.update(n_fft=N, hop=hop, per_slice=per_slice, slices="several" if per_slice else "one")
        self.more(rng, case)
        info_of(case)
        cap = max(N + 1, min(3000, hop * (200000 // (case["channels"] * N))))  # the reference transforms channels x segments rows
        case = common_draw(rng, self, case, N - 1, N, cap)  # the unit: one segment
        case["position"] = 0 if case["start"] == "null" else draw_position(rng, case["total"])
        return case

    def more(self, rng, case):
        pass

    def host_info(self, case):
        return {}

    def _window(self, case):
        import scipy.signal
        return scipy.signal.get_window("hann", case["n_fft"])

    def _kw(self, case):
        unit = case["n_fft"] * (8 if case["precision"] == "f64" else 4) + (case["n_fft"] // 2 + 1) * 8
        return dict(detrend=case["detrend"], workspace_bytes=case["per_slice"] * unit)

    def _make(self, env, case):
        return self.module()._bank(env.sd, case["n_fft"], case["hop"], case["channels"], case["precision"], **self._kw(case))

    def plan_info(self, env, case):
        return self._make(env, case).info()

    def validate(self, case):
        import ctypes as C
        import simpledsp_amd as sd
        from welch_ref import welch_frames
        N, hop = case["n_fft"], case["hop"]
        assert N & (N - 1) == 0 and 32 <= N <= 32768 and 1 <= hop <= N and 0 <= case["position"] < 1 << 35, case
        assert case["start"] != "null" or case["position"] == 0, case
        n = C.c_uint64(0)
        assert sd.load().sdsp_hip_welch_frames(N, hop, case["position"], case["total"], C.byref(n)) == 0, case
        assert n.value == welch_frames(N, hop, case["position"], case["total"]), case

    def _dt(self, case):
        return np.float64 if case["precision"] == "f64" else np.float32

    def _start_acc(self, case, rng):
        return {"acc": rng.uniform(0, 4 * case["n_fft"], (case["channels"], case["n_fft"] // 2 + 1))}

    def data(self, case):
        rng = np.random.default_rng(case["data_seed"])
        C = case["channels"]
        x = rng.standard_normal((C, case["total"])).astype(self._dt(case))
        start = {"hist": rng.standard_normal((C, case["n_fft"] - 1)).astype(self._dt(case)), **self._start_acc(case, rng),
                 "frames": np.array([5], dtype=np.int64)}
        return {"in": {"in": x}, "start": start, "position": case["position"]}

    start_state = Ddc.start_state

    def _w(self, case):
        return self._window(case).astype(self._dt(case)).astype(np.float64)  # the window as the plan rounds it

    def step(self, case, data, state, t0, t1):
        from welch_ref import welch_ref
        pos = int(state["position"][0])
        acc, F, hist = welch_ref(data["in"]["in"][:, t0:t1], case["n_fft"], case["hop"], self._w(case), case["detrend"], pos,
                                 state["hist"], state["acc"])
        return {}, {"hist": hist.astype(self._dt(case)), "acc": acc, "frames": state["frames"] + F,
                    "position": np.array([pos + t1 - t0], dtype=np.int64)}

    def same(self, name, got, want, case, data=None):
        t = self.module()
        if name[len("state:"):] not in self.acc_names:
            return np.array_equal(got, want)
        got, want = self.as_complex(got), self.as_complex(want)
        if got.shape != want.shape:
            return False
        if not np.abs(want).max(axis=-1).all():  # a row of zeros: no segment ended in the stream
            return np.array_equal(got, want)
        return t._peak_err(got, want) <= t._tol(case["precision"])

    @staticmethod
    def as_complex(a):
        return a

    def open(self, env, case, data, variant, start):
        return _WelchSession(self, env, case, data, variant, start)


class _WelchSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        st = fam.start_state(data, "zero" if start == "null" else start)
        self.bank = guarded(lambda: fam._make(env, case), "welch plan")
        guarded(self.bank._ensure_plan, "welch plan")
        self.hist = env.torch.from_numpy(np.ascontiguousarray(st["hist"])).to(env.device)
        self.acc = {n: _Padded(env, n, fam.as_reals(st[n]), case["pads"][n]) for n in fam.acc_names}
        self.position, self.frames = case["position"], int(st["frames"][0])

    def call(self, t0, t1, wants, io):
        from welch_ref import welch_frames
        n = t1 - t0
        x = io.inp("in", self.data["in"]["in"][:, t0:t1])
        self.launch(x, n, None if self.null else self.hist.data_ptr())
        io.sync()
        self.frames += welch_frames(self.case["n_fft"], self.case["hop"], self.position, n)
        self.position += n
        return {}

    def launch(self, x, n, state):
        acc = self.acc["acc"]
        rc_check(self.lib.sdsp_hip_welch_process(self.bank._plan, x.ptr, x.stride, x.rows, n, self.position, state, acc.ptr, acc.width, None),
                 "welch_process")

    def state(self):
        self.faults = [f for a in self.acc.values() for f in a.faults()]
        out = {n: self.fam.from_reals(a.get()) for n, a in self.acc.items()}
        out["frames"] = np.array([self.frames], dtype=np.int64)
        out["position"] = np.array([self.position], dtype=np.int64)
        if not self.null:
            out["hist"] = self.hist.cpu().numpy().copy()
        return out


Welch.as_reals = staticmethod(lambda a: a)
Welch.from_reals = staticmethod(lambda a: a)


class Csd(Welch):
    """the Welch bank's protocol with two accumulators: the cross sums of the pairs (complex, re and im interleaved) and the
    channels' own powers.  Tolerances: `_peak_err` <= `_tol` of tests/test_gpu_csd.py"""
    name = "csd"
    buffers = ("in", "acc_xy", "acc_auto")
    split_tol = ("state:acc_xy", "state:acc_auto")
    acc_names = ("acc_xy", "acc_auto")

    def more(self, rng, case):
        case["n_pairs"] = int(pick(rng, (1, 2, 5, case["channels"] + 1)))
        case["pair_seed"] = int(rng.integers(0, 1 << 31))

    def pairs(self, case):
        rng = np.random.default_rng(case["pair_seed"])
        C = case["channels"]
        out = [(int(rng.integers(0, C)), int(rng.integers(0, C))) for _ in range(case["n_pairs"])]
        out[0] = (C - 1, C - 1)  # a channel against itself
        return out

    def _kw(self, case):  # a slice holds whole segment columns: one segment of every channel and pair
        column = self.module()._column(case["n_fft"], case["precision"], case["n_pairs"], case["channels"])
        return dict(detrend=case["detrend"], workspace_bytes=case["per_slice"] * column)

    def _make(self, env, case):
        return self.module()._bank(env.sd, case["n_fft"], case["hop"], case["precision"], self.pairs(case), case["channels"], **self._kw(case))

    def validate(self, case):
        Welch.validate(self, case)
        assert all(0 <= a < case["channels"] and 0 <= b < case["channels"] for a, b in self.pairs(case)), case

    def _start_acc(self, case, rng):
        bins = case["n_fft"] // 2 + 1
        xy = rng.standard_normal((case["n_pairs"], bins)) + 1j * rng.standard_normal((case["n_pairs"], bins))
        return {"acc_xy": 4 * case["n_fft"] * xy, "acc_auto": rng.uniform(0, 4 * case["n_fft"], (case["channels"], bins))}

    def step(self, case, data, state, t0, t1):
        from csd_ref import csd_ref
        pos = int(state["position"][0])
        xy, au, F, hist = csd_ref(data["in"]["in"][:, t0:t1].astype(np.float64), self.pairs(case), case["n_fft"], case["hop"], self._w(case),
                                  case["detrend"], pos, state["hist"], state["acc_xy"], state["acc_auto"])
        return {}, {"hist": hist.astype(self._dt(case)), "acc_xy": xy, "acc_auto": au, "frames": state["frames"] + F,
                    "position": np.array([pos + t1 - t0], dtype=np.int64)}

    @staticmethod
    def as_reals(a):
        a = np.ascontiguousarray(a)
        return a.view(np.float64).reshape(a.shape[0], -1) if np.iscomplexobj(a) else a

    def open(self, env, case, data, variant, start):
        return _CsdSession(self, env, case, data, variant, start)


class _CsdSession(_WelchSession):
    def launch(self, x, n, state):
        xy, au = self.acc["acc_xy"], self.acc["acc_auto"]
        rc_check(self.lib.sdsp_hip_csd_process(self.bank._plan, x.ptr, x.stride, n, self.position, state, xy.ptr, xy.width, au.ptr, au.width,
                                               None), "csd_process")

    def state(self):
        out = _WelchSession.state(self)
        out["acc_xy"] = np.ascontiguousarray(out["acc_xy"]).view(np.complex128)
        return out



class FirFft(SampleFamily):
    """the FFT-domain (overlap-save) FIR bank, in place on its rows.  Its rounding differs from the direct form's, and the header
    says block-by-block calls match one long call "within that tolerance, not bit for bit": the one call against the oracle's
    direct FIR in double and the splits against the one call are both held to TOL of tests/test_gpu_fir_fft.py (normwise per row);
    the history, a copy of inputs, to bits.  Variant 1 is the three-launch composition, "within the same tolerance": no check (d)"""
    name = "fir_fft"
    cross_variants = (0,)
    buffers = ("data",)
    split_tol = ("data",)
    axes = {"precision": ("f32", "f64"), "variant": (0, 1), "fft": ("auto", "min"), "slices": ("one", "several")}

    def module(self):
        return __import__("test_gpu_fir_fft")

    def draw(self, rng, info_of):
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64")), channels=draw_channels(rng))
        T = int(pick(rng, (1, 2, 9, 17, 64, 255, 300))) if rng.random() < 0.8 else int(rng.integers(1, 400))
        fft = pick(rng, ("auto", "min"))
        n = 16
        while n < 2 * (T - 1):
            n *= 2
        per_slice = int(pick(rng, (0, 1, 3)))  # transforms a workspace slice holds; 0: the default budget, one slice
        case.update(taps=T, fft=fft, fft_n=n if fft == "min" else 0, per_slice=per_slice, slices="several" if per_slice else "one",
                    tap_seed=int(rng.integers(0, 1 << 31)))
        info = info_of(case)
        case["n"] = int(info["fft_n"])  # the transform size of the plan, chosen or automatic
        return common_draw(rng, self, case, T - 1, info["hop"], 3000)

    def _h(self, case):
        return np.random.default_rng(case["tap_seed"]).standard_normal(case["taps"])

    def host_info(self, case):
        from simpledsp_amd import _lib as L
        from simpledsp_amd.fir import fir_fft_size
        n = case["fft_n"] or fir_fft_size(case["taps"], L.F64 if case["precision"] == "f64" else L.F32)  # a host helper: no device
        return {"hop": n - case["taps"] + 1, "fft_n": n}

    def _make(self, env, case, state=None):
        one = case.get("n", 0) * (16 if case["precision"] == "f64" else 8)  # one complex transform of the plan's size
        return self.module()._bank(env.sd, case["taps"], case["channels"], case["precision"], self._h(case), state, fft_n=case["fft_n"],
                                   workspace_bytes=case["per_slice"] * one)

    def plan_info(self, env, case):
        return self._make(env, case).info()

    def validate(self, case):
        T, n = case["taps"], case["fft_n"]
        assert 1 <= T <= 8192 and (n == 0 or (n & (n - 1) == 0 and 16 <= n <= 16384 and n >= 2 * (T - 1))), case
        assert self.host_info(case)["hop"] >= 1, case

    def _dt(self, case):
        return np.float64 if case["precision"] == "f64" else np.float32

    def data(self, case):
        rng = np.random.default_rng(case["data_seed"])
        C = case["channels"]
        return {"in": {"data": rng.standard_normal((C, case["total"])).astype(self._dt(case))},
                "start": {"hist": rng.standard_normal((C, case["taps"] - 1)).astype(self._dt(case))}}

    def step(self, case, data, state, t0, t1):
        from oracle import Oracle
        t = self.module()
        x = data["in"]["data"][:, t0:t1]
        hs, xs, ss = t._seen(self._h(case), x, state["hist"], case["precision"])
        o = Oracle()
        y, hist = np.zeros(xs.shape), np.zeros(ss.shape)
        for c in range(xs.shape[0]):
            y[c], hist[c] = o.fir_process(hs, xs[c], ss[c] if case["taps"] > 1 else None)
        return {"data": y}, {"hist": hist.astype(self._dt(case))}

    def same(self, name, got, want, case, data=None):
        from conftest import rel_max_err
        if name.startswith("state:"):
            return np.array_equal(got, want)
        if got.shape != want.shape:
            return False
        return want.size == 0 or rel_max_err(got, want) <= self.module().TOL[case["precision"]]

    def open(self, env, case, data, variant, start):
        return _FirFftSession(self, env, case, data, variant, start)


class _FirFftSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        hist = data["start"]["hist"] if start == "random" else np.zeros_like(data["start"]["hist"])
        self.bank = guarded(lambda: fam._make(env, case), "fir plan")
        guarded(self.bank._ensure_plan, "fir plan")
        rc_check(self.lib.sdsp_hip_fir_plan_set_variant(self.bank._plan, variant), "fir_plan_set_variant")
        self.st = env.torch.from_numpy(np.ascontiguousarray(hist)).to(env.device)

    def call(self, t0, t1, wants, io):
        n = t1 - t0
        x = io.in_place(io.inp("data", self.data["in"]["data"][:, t0:t1]))
        state = None if self.null or self.st.numel() == 0 else self.st.data_ptr()
        rc_check(self.lib.sdsp_hip_fir_process(self.bank._plan, x.ptr, x.rows, n, x.stride, state, None), "fir_process")
        io.sync()
        return self.collect({"data": x})

    def state(self):
        return {} if self.null else {"hist": self.st.cpu().numpy().copy()}



class Filtfilt(SampleFamily):
    """zero-phase filtering of whole rows in place: one call, no state, so checks (b) and (c) repeat the one call (identical calls,
    identical bits) and the stream axes of the draw do not apply.  Against scipy.signal.sosfiltfilt in double under SCIPY_TOL of
    tests/test_gpu_filtfilt.py; variant 1 (the direct kernel) against variant 0: bits"""
    name = "filtfilt"
    stream = False
    has_history = False
    null_state = False
    buffers = ("data",)
    axes = {"precision": ("f32", "f64", "mix"), "design": ("lp", "hp", "bp", "bs", "rand"), "padtype": ("odd", "even", "constant", "none"),
            "variant": (0, 1), "fused": (0, 1), "slices": ("one", "several")}

    def draw(self, rng, info_of):
        from filtfilt_ref import default_padlen_ref
        case = dict(family=self.name, precision=pick(rng, ("f32", "f64", "mix")), design=pick(rng, ("lp", "hp", "bp", "bs", "rand")),
                    padtype=pick(rng, ("odd", "even", "constant", "none")), channels=draw_channels(rng))
        m = int(pick(rng, (2, 4, 8, 12, 16)))  # the fused kernel takes up to 8 sections
        case.update(sections=m, fused=int(m <= 8), slices=pick(rng, ("one", "several")))
        kind, a, b, g = self.design(case)
        P = 0 if case["padtype"] == "none" else int(default_padlen_ref(kind, a, b))
        case["padlen"] = P
        info_of(case)
        total = int(pick(rng, (P + 1, P + 2, 128 * int(rng.integers(1, 20)) + int(pick(rng, (-1, 0, 1))), int(rng.integers(P + 1, P + 3000)))))
        total = max(total, P + 1)
        case.update(hist=0, unit=128, total=total, start="zero", calls=[total], calls2=[total], variant=int(pick(rng, self.variants)),
                    subset="", pads=draw_pads(rng, self.buffers), data_seed=int(rng.integers(0, 1 << 31)))
        return case

    def design(self, case):
        import simpledsp_amd as sd
        return self.module()._design(sd, case["design"], case["sections"])

    def host_info(self, case):
        return {}

    def _make(self, env, case):
        t = self.module()
        kind, a, b, g = self.design(case)
        rs = 8 if case["precision"] == "f64" else 4
        ws = 64 * case["padlen"] * rs if case["slices"] == "several" else 0  # 64 channels a slice, the smallest
        return t._plan(env.sd, kind, a, b, g, case["precision"], None if case["padtype"] == "none" else case["padtype"], None, ws)

    def plan_info(self, env, case):
        return self._make(env, case).info()

    def validate(self, case):
        assert 2 <= case["sections"] <= 16 and case["total"] > case["padlen"] >= 0 and case["calls"] == [case["total"]], case

    def _dt(self, case):
        return np.float64 if case["precision"] == "f64" else np.float32

    def data(self, case):
        rng = np.random.default_rng(case["data_seed"])
        C = case["channels"]
        x = np.cumsum(rng.standard_normal((C, case["total"])), axis=1) * 0.1 + rng.standard_normal((C, 1))  # _signal's random walk
        return {"in": {"data": x.astype(self._dt(case))}, "start": {}}

    def step(self, case, data, state, t0, t1):
        import scipy.signal
        from filtfilt_ref import sos_of
        assert (t0, t1) == (0, case["total"])
        kind, a, b, g = self.design(case)
        want = scipy.signal.sosfiltfilt(sos_of(kind, a, b, g), data["in"]["data"].astype(np.float64),
                                        padtype=None if case["padtype"] == "none" else case["padtype"])
        return {"data": want}, {}

    def same(self, name, got, want, case, data=None):
        t = self.module()
        return got.shape == want.shape and t._scipy_err(got.astype(np.float64), want) <= t.SCIPY_TOL[case["precision"]]

    def open(self, env, case, data, variant, start):
        return _FiltfiltSession(self, env, case, data, variant, start)


class _FiltfiltSession(_Session):
    def __init__(self, fam, env, case, data, variant, start):
        super().__init__(fam, env, case, data, variant, start)
        self.bank = guarded(lambda: fam._make(env, case), "filtfilt plan")
        guarded(lambda: self.bank.set_variant(variant), "filtfilt_plan_set_variant")

    def call(self, t0, t1, wants, io):
        x = io.in_place(io.inp("data", self.data["in"]["data"][:, t0:t1]))
        rc_check(self.lib.sdsp_hip_filtfilt_process(self.bank._plan, x.ptr, x.rows, t1 - t0, x.stride, None), "filtfilt_process")
        io.sync()
        return self.collect({"data": x})

    def state(self):
        return {}


def _variants_from_the_table():
    """the values *_plan_set_variant takes come from the VARIANTS table of tests/test_gpu_wide_strides.py ((0, 1) where an entry is
    not named there).  Left as the classes state them: the banks around a transform plan, whose variants are that plan's (None in the
    table), pfb and pfb_synth, whose `variant` is the fold form, and the FFT-domain FIR plan, whose two variants are the inner
    convolution's while the table's row is the direct plan's"""
    from test_gpu_wide_strides import VARIANTS
    for fam in FAMILIES.values():
        takes = VARIANTS.get(fam.name + "_process", ((0, 1), ()))[0]
        if takes is not None and fam.name not in ("pfb", "pfb_synth", "fir_fft"):
            fam.variants = tuple(takes)
            if "variant" in fam.axes:
                fam.axes = dict(fam.axes, variant=tuple(takes))


FAMILIES = {f.name: f for f in (Lms(), Rank(), Cfar(), Pll(), Timing(), Ddc(), Duc(), Arb(), Cic(), CicInterp(), Beam(), Resample(),
                                    Stft(), Pfb(), Istft(), PfbSynth(), Welch(), Csd(), FirFft(), Filtfilt())}
_variants_from_the_table()


# ------------------------------------------------------------------ drawing and running cases

def draw_case(seed, family, index, info_of=None):
    """the case of (seed, family, index); info_of(case) gives the plan's info() for the parameters drawn so far (default: the family's
    host stand-in)"""
    fam = FAMILIES[family]
    return fam.draw(case_rng(seed, family, index), info_of or fam.host_info)


def run_cases(env, seed, cases, families=None, only=None, log=print, opener=None, host=False, seen=None):
    """runs cases 0 .. cases - 1 (or the one case `only`) of every family named; returns (cases run, failure lines) and appends the
    cases that ran to their end to seen[family].  Stops at the first HIP error: its case line goes to GPU_STOPPED and nothing more
    is started"""
    failures, ran = [], 0
    for name in families or FAMILIES:
        fam = FAMILIES[name]
        t0 = time.perf_counter()
        for index in ([only] if only is not None else range(cases)):
            if GPU_STOPPED:
                return ran, failures
            case = None
            try:
                case = fam.draw(case_rng(seed, name, index), fam.host_info if host else (lambda c: guarded(lambda: fam.plan_info(env, c), "plan")))
                found = check_case(fam, env, case, seed, index, opener)
                if env.device != "cpu":
                    env.torch.cuda.synchronize()
            except Refused as e:  # the plan of the draw
                found = [f"FAIL family={name} seed={seed} index={index} check=draw case={case} buffer=refused: {e} differing=-1 first=None"]
            except (GpuStop, RuntimeError) as e:  # a HIP error from the draw's plan, an entry, or the synchronisation after the case
                line = f"FAIL family={name} seed={seed} index={index} check=gpu-error case={case} {e}"
                GPU_STOPPED.append(line)
                failures.append(line)
                log(line)
                return ran + 1, failures
            ran += 1
            for f in found:
                log(f)
            failures += found
            if only is not None:
                log(f"case family={name} seed={seed} index={index} case={case}: {'FAILED' if found else 'passed'}")
            if seen is not None and case is not None:
                seen.setdefault(name, []).append(case)
        log(f"{name}: seed {seed}: {time.perf_counter() - t0:.2f} s ({STATS['runs']} runs and {STATS['compared']} compared elements so far)")
    return ran, failures


# ------------------------------------------------------------------ coverage of a set of drawn cases

def call_kinds(case):
    """which of the forced kinds of call the two splits of a case hold"""
    calls = [*case["calls"], *case["calls2"]]
    h = case["hist"]
    return {"empty": 0 in calls, "one": 1 in calls, "short": any(0 < c < h for c in calls), "exact": h > 0 and h in calls}


def coverage_gaps(family, cases):
    """what the issue's coverage list misses over `cases` of one family: a list of strings, empty when every axis value was seen"""
    fam, gaps = FAMILIES[family], []
    for key, values in fam.axes.items():
        missing = set(values) - {c[key] for c in cases}
        if missing:
            gaps.append(f"{family}: {key} never {sorted(missing, key=str)}")
    for keys in fam.crosses:
        missing = set(itertools.product(*(fam.axes[k] for k in keys))) - {tuple(c[k] for k in keys) for c in cases}
        if missing:
            gaps.append(f"{family}: {keys} never {sorted(missing)}")
    kinds = [call_kinds(c) for c in cases]
    for k in (("empty", "one") + (("short", "exact") if fam.has_history else ())) if fam.stream else ():
        if not any(d[k] for d in kinds):
            gaps.append(f"{family}: no call of kind '{k}'")
    if not any(c["channels"] < 64 for c in cases) or not any(c["channels"] > 64 for c in cases):
        gaps.append(f"{family}: channel counts on one side of 64 only")
    starts = ({"zero", "random"} | ({"null"} if fam.null_state else set())) if fam.stream else set()
    if starts - {c["start"] for c in cases}:
        gaps.append(f"{family}: start states {sorted(starts - {c['start'] for c in cases})} never drawn")
    rel = {("below" if c["total"] < c["unit"] else "at" if c["total"] == c["unit"] else "above") for c in cases}
    if fam.stream and {"below", "at", "above"} - rel:
        gaps.append(f"{family}: totals {sorted({'below', 'at', 'above'} - rel)} one unit never drawn")
    if fam.optional:
        every = {"+".join(c) for k in range(0 if fam.none_legal else 1, len(fam.optional)) for c in itertools.combinations(fam.optional, k)}
        missing = every - {c["subset"] for c in cases}
        if missing:
            gaps.append(f"{family}: subsets of the optional outputs never drawn: {sorted(missing)}")
    return gaps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=SEEDS[0])
    ap.add_argument("--cases", type=int, default=CASES)
    ap.add_argument("--family", action="append", choices=sorted(FAMILIES))
    ap.add_argument("--case", type=int, default=None, help="run this one case index only")
    ap.add_argument("--stand-in", action="store_true", help="run the numpy stand-ins on the CPU instead of the HIP banks")
    ap.add_argument("--defect", choices=DEFECTS, default=None, help="with --stand-in: plant this defect")
    args = ap.parse_args(argv)
    if args.stand_in:
        env, opener = cpu_env(), stand_in_opener(args.defect)
    else:
        env, opener = gpu_env(), None
    ran, failures = run_cases(env, args.seed, args.cases, args.family, args.case, opener=opener, host=args.stand_in)
    print(f"{ran} case(s), {len(failures)} failing check(s)" + (", stopped on a GPU error" if GPU_STOPPED else ""))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
