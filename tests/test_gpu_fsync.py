"""GPU tests of the frame synchroniser banks (sdsp_hip_fsync_*) on a real MI355X.

The checker is tests/fsync_ref.py, the contract in numpy, itself held to a bit-by-bit implementation in tests/test_fsync_host.py.
Everything is on integers, so both kernel variants are held to the reference bit for bit: `out` up to `counts`, `counts`, `pos`,
`info` and the machine's state, for any split of a stream into calls.  The reference of a stream is worked once and shared by the
variants and input kinds that run it."""
import numpy as np
import pytest

import arena
import fsync_ref as R

pytestmark = pytest.mark.gpu

INVALID_SIZE, INVALID_ARG = -1, -5
MARKERS = {8: 0x47, 16: 0xEB90, 32: 0x1ACFFC1D, 33: 0x1ACFFC1D5, 64: 0x034776C7272895B0}
STATE_KEYS = ("mode", "next", "polarity", "count", "misses", "pending", "seen")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def sd():
    import simpledsp_amd
    simpledsp_amd.load(build_if_missing=True)
    return simpledsp_amd


def _reference(p, rows, edges):
    """the reference's outputs of every call and its final state: p = (marker, M, P, tol, V, F, polarity, pn)"""
    marker, M, P, tol, V, F, pol, pn = p
    fs = R.FrameSync(marker, M, P, tol, V, F, R.EITHER if pol == "either" else R.NORMAL, pn, rows.shape[0])
    calls = [fs.process(rows[:, a:b]) for a, b in zip(edges, edges[1:])]
    return calls, fs.state(), fs


def _device_input(torch, bits, kind, values=None):
    if kind == "packed":
        return torch.from_numpy(R.pack_words(bits).view(np.int32).copy()).cuda().reshape(bits.shape[0], -1)
    b = bits if values is None else bits * values
    return torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint8)).cuda()


def _check_call(got, want, tag):
    frames, counts, pos, info = (t.cpu().numpy() for t in got)
    wout, wcounts, wpos, winfo = want
    assert np.array_equal(counts.astype(np.uint32), wcounts), (tag, "counts", counts, wcounts)
    for c, n in enumerate(wcounts):
        assert np.array_equal(pos[c, :n].astype(np.uint64), wpos[c, :n]), (tag, "pos", c, pos[c, :n], wpos[c, :n])
        assert np.array_equal(info[c, :n].astype(np.uint32), winfo[c, :n]), (tag, "info", c, info[c, :n], winfo[c, :n])
        assert np.array_equal(frames[c, :n], wout[c, :n]), (tag, "out", c)
        # slots at and beyond counts keep process()'s zeros
        assert not frames[c, n:].any() and not pos[c, n:].any() and not info[c, n:].any(), (tag, "a slot beyond counts was written", c)


def _check_state(bank, want, channels, tag):
    got = bank.state(channels)
    for key, w in zip(STATE_KEYS, want):
        assert np.array_equal(got[key], w), (tag, key, got[key], w)


def run_bank(sd, torch, p, rows, kind, edges=None, variants=(0,), ref=None, values=None, tag=""):
    """one bank over the calls `edges` cuts the rows into, variant variants[i % len] in call i, against the reference"""
    marker, M, P, tol, V, F, pol, pn = p
    edges = [0, rows.shape[1]] if edges is None else edges
    calls, state, _ = ref if ref is not None else _reference(p, rows, edges)
    bank = sd.frame_sync_bank(marker, M, P, tol, V, F, pol, pn, kind, max_channels=rows.shape[0] + 1,
                              max_bits=max(1, max(b - a for a, b in zip(edges, edges[1:]))))
    try:
        for i, (a, b) in enumerate(zip(edges, edges[1:])):
            bank.set_variant(variants[i % len(variants)])
            got = bank.process(_device_input(torch, rows[:, a:b], kind, None if values is None else values[:, a:b]), records=True)
            _check_call(got, calls[i], (tag, kind, "variants", variants, "call", i, (a, b)))
        _check_state(bank, state, rows.shape[0], (tag, kind, variants))
    finally:
        torch.cuda.synchronize()
        bank.close()


def framed_rows(rng, marker, M, P, channels, frames, pn=None, prefix=None, invert_from=None, tail=16):
    """`channels` rows of equal length, a multiple of 32: row c has a junk prefix of prefix(c) bits (default c % 64), `frames` frames
    (inverted from frame invert_from on) and junk behind; returns (rows, payloads)"""
    L = M + 8 * P
    total = -(-(63 + frames * L + tail) // 32) * 32
    rows = rng.integers(0, 2, (channels, total), dtype=np.uint8)
    payloads = rng.integers(0, 256, (channels, frames, P), dtype=np.uint8)
    for c in range(channels):
        q = c % 64 if prefix is None else prefix(c)
        for k in range(frames):
            inv = invert_from is not None and k >= invert_from
            rows[c, q + k * L:q + (k + 1) * L] = R.attach(payloads[c, k], marker, M, pn, inv)
    return rows, payloads


MACHINES = [(0, 0, 0, "either"), (1, 1, 1, "normal"), (3, 3, 2, "either")]  # (tol, V, F, polarity)


@pytest.mark.parametrize("P", [1, 4, 37])
@pytest.mark.parametrize("M", [8, 16, 32, 33, 64])
def test_marker_sizes_and_every_alignment(sd, torch_cuda, M, P):
    """every marker size and payload size of the contract; 67 rows whose junk prefix runs through 0 .. 63 bits, so the marker meets every
    alignment against 32- and 64-bit words; 1, 3 and 67 channels, both input kinds, both variants, three machines"""
    rng = np.random.default_rng(100 * M + P)
    marker = MARKERS[M]
    pn = rng.integers(0, 256, P, dtype=np.uint8)
    for i, (tol, V, F, pol) in enumerate(MACHINES):
        rows, _ = framed_rows(rng, marker, M, P, 67, 7, pn, invert_from=4 if i != 1 else None)
        rows[5, 5 + 2 * (M + 8 * P)] ^= 1  # one marker error in the third frame of row 5
        p = (marker, M, P, tol, V, F, pol, pn)
        for channels in (1, 3, 67):
            sub = rows[64:65] if channels == 1 else rows[:channels]  # the single row has the prefix 0
            ref = _reference(p, sub, [0, sub.shape[1]])
            if channels == 67 and (M >= 16 or tol == 0):  # (at M = 8 a tolerance of 1 or 3 hits noise at every few positions)
                assert (ref[0][0][1] >= 2).all(), "every row must emit frames in the reference"
            for kind in ("bytes", "packed"):
                for variant in (0, 1):
                    run_bank(sd, torch_cuda, p, sub, kind, variants=(variant,), ref=ref, tag=("sizes", M, P, tol, V, F, pol, channels))


@pytest.mark.parametrize("kind", ["bytes", "packed"])
def test_splits_with_alternating_variants_equal_one_call(sd, torch_cuda, kind):
    """one stream of about 40 frames as one call and as random splits with an empty call, calls shorter than M and calls shorter than L
    (a frame spans three calls); the variant alternates between the calls"""
    rng = np.random.default_rng(4040 + (kind == "packed"))
    M, P = 32, 9
    L = M + 8 * P  # 104
    pn = R.ccsds_pn(P)
    p = (MARKERS[M], M, P, 1, 1, 1, "either", pn)
    rows, _ = framed_rows(rng, MARKERS[M], M, P, 5, 40, pn, prefix=lambda c: (0, 1, 31, 33, 63)[c], invert_from=25)
    rows[2, 31 + 10 * L:31 + 10 * L + 2] ^= 1  # a damaged marker: a flywheel frame
    N = rows.shape[1]
    run_bank(sd, torch_cuda, p, rows, kind, variants=(0,), tag="one call, variant 0")
    run_bank(sd, torch_cuda, p, rows, kind, variants=(1,), tag="one call, variant 1")
    step = 32 if kind == "packed" else 1
    for trial in range(3):
        cuts = {0, N}
        at = 0
        while at < N:
            r = rng.random()
            n = 0 if r < 0.1 else int(rng.integers(1, M)) if r < 0.4 else int(rng.integers(M, L)) if r < 0.8 else int(rng.integers(L, 6 * L))
            at = min(N, at + -(-n // step) * step)
            cuts.add(at)
        edges = sorted(cuts)
        k = len(edges) // 2
        edges = edges[:k] + [edges[k]] + edges[k:]  # an empty call in the middle
        if kind == "bytes":
            lens = np.diff(edges)
            assert (lens == 0).any() and ((lens > 0) & (lens < M)).any() and (lens < L).sum() > 5
        for variants in ((0, 1), (1, 0)):
            run_bank(sd, torch_cuda, p, rows, kind, edges, variants, tag=("splits", trial))


def test_three_calls_to_one_frame(sd, torch_cuda):
    rng = np.random.default_rng(9)
    M, P = 16, 4
    p = (MARKERS[M], M, P, 0, 0, 0, "normal", None)
    rows, _ = framed_rows(rng, MARKERS[M], M, P, 2, 6, prefix=lambda c: 3 + c)
    edges = list(range(0, rows.shape[1], 20)) + [rows.shape[1]]  # L = 48: every frame spans three calls
    for variants in ((0,), (1,), (0, 1)):
        run_bank(sd, torch_cuda, p, rows, "bytes", edges, variants, tag="20-bit calls")
    edges = list(range(0, rows.shape[1], 32)) + [rows.shape[1]]
    run_bank(sd, torch_cuda, p, rows, "packed", edges, (0, 1), tag="32-bit calls")


def _events():
    """(label, parameters, rows): the contract's events, each planted in a stream of its own"""
    rng = np.random.default_rng(31337)
    M, P, marker = 32, 5, MARKERS[32]
    L = M + 8 * P
    out = []

    def base(frames=12, prefix=11, **kw):
        return framed_rows(rng, marker, M, P, 1, frames, prefix=lambda c: prefix, **kw)[0]

    for tol in (0, 2):
        for extra in (0, 1):
            rows = base()
            rows[0, 11 + 5 * L + 3:11 + 5 * L + 3 + tol + extra] ^= 1
            out.append((f"marker errors: tol {tol} + {extra}", (marker, M, P, tol, 1, 1, "either", None), rows))
    out.append(("inverted stretches", (marker, M, P, 1, 1, 1, "either", None), base(invert_from=5)))
    out.append(("inverted stretch, polarity normal", (marker, M, P, 1, 1, 1, "normal", None), base(invert_from=5)))
    for F in (0, 2):
        for run in (F, F + 1):
            rows = base(frames=14)
            for k in range(4, 4 + run):
                rows[0, 11 + k * L:11 + k * L + 8] ^= 1
            out.append((f"flywheel {F}, {run} damaged markers", (marker, M, P, 1, 1, F, "either", None), rows))
    rows = base()
    out.append(("slip forward", (marker, M, P, 0, 1, 1, "either", None), np.delete(rows, 11 + 6 * L - 1, axis=1)[:, :-31]))
    out.append(("slip backward", (marker, M, P, 0, 1, 1, "either", None),
                np.insert(rows, 11 + 6 * L, 1, axis=1)[:, :-1]))
    # a false candidate directly in front of a true marker: a copy of the marker 16 bits before the first frame; L behind it lies payload
    rows = base(prefix=50)
    rows[0, :50] = 0
    rows[0, 2:2 + M] = R.marker_bits(marker, M)
    out.append(("false candidate, then the rescan", (marker, M, P, 0, 2, 1, "either", None), rows))
    out.append(("no marker at all", (0xFFFFFFFF, 32, P, 0, 1, 1, "normal", None), np.zeros((2, 32 * 81), dtype=np.uint8)))
    out.append(("no marker, longer than a search round", (0xFFFFFFFF, 32, P, 0, 1, 1, "normal", None),
                np.concatenate([np.zeros((1, 32 * 200), dtype=np.uint8), R.attach(np.arange(3 * P).reshape(3, P), 0xFFFFFFFF, 32)[None, :],
                                np.zeros((1, 40), dtype=np.uint8)], axis=1)))
    out.append(("all zeros with marker 0", (0, 16, 3, 0, 1, 1, "either", None), np.zeros((2, 32 * 20), dtype=np.uint8)))
    return out


EVENTS = _events()


@pytest.mark.parametrize("label,p,rows", EVENTS, ids=[e[0] for e in EVENTS])
def test_events(sd, torch_cuda, label, p, rows):
    assert rows.shape[1] % 32 == 0, label
    ref = _reference(p, rows, [0, rows.shape[1]])
    _, _, fs = ref
    counts = ref[0][0][1]
    if label.startswith("false candidate"):
        assert "verify-search" in fs.transitions and int(ref[0][0][2][0, 0]) == 50 + (p[1] + 8 * p[2]) * 2
    if label.startswith("flywheel"):
        F, run = p[5], int(label.split(", ")[1].split()[0])
        flagged = int(((ref[0][0][3][0, :counts[0]] >> 9) & 1).sum())
        assert flagged == (run if run <= F else F), (label, flagged)
    if label.startswith("no marker at all"):
        assert not counts.any() and int(ref[1][1][0]) == rows.shape[1] - 31
    if label.startswith("all zeros"):
        assert counts[0] == rows.shape[1] // 40 - 1  # V = 1: the first frame verifies, every later whole frame comes out
    for kind in ("bytes", "packed"):
        for variant in (0, 1):
            run_bank(sd, torch_cuda, p, rows, kind, variants=(variant,), ref=ref, tag=label)
    mid = rows.shape[1] // 2 // 32 * 32 + 32
    run_bank(sd, torch_cuda, p, rows, "packed", [0, 32, mid, rows.shape[1]], (0, 1), tag=label)


def test_bytes_rows_count_any_non_zero_value_as_one(sd, torch_cuda):
    rng = np.random.default_rng(255)
    M, P = 16, 4
    p = (MARKERS[M], M, P, 1, 1, 1, "either", None)
    rows, _ = framed_rows(rng, MARKERS[M], M, P, 3, 8)
    values = rng.choice(np.array([1, 2, 255], dtype=np.uint8), rows.shape)
    ref = _reference(p, rows, [0, rows.shape[1]])
    assert set(np.unique(rows * values)) == {0, 1, 2, 255}
    for variant in (0, 1):
        run_bank(sd, torch_cuda, p, rows, "bytes", variants=(variant,), ref=ref, values=values, tag="values")


@pytest.mark.parametrize("kind", ["bytes", "packed"])
@pytest.mark.parametrize("variant", [0, 1])
def test_framed_buffers_at_every_offset(sd, torch_cuda, variant, kind):
    """in, out, counts, pos and info as views into larger tensors at every element offset: nothing outside the addressed ranges is
    written, slots at and beyond counts stay untouched, and the results are the reference's under both fills"""
    torch = torch_cuda
    rng = np.random.default_rng(808 + variant)
    M, P = 33, 5  # L = 73: frames of 5 bytes, so `out` frames start at every alignment
    marker = MARKERS[M]
    pn = rng.integers(0, 256, P, dtype=np.uint8)
    rows, _ = framed_rows(rng, marker, M, P, 3, 6, pn, prefix=lambda c: (0, 7, 40)[c])
    rows[1, 7 + 3 * 73:] = 0  # row 1 loses its marker: fewer frames than the others
    p = (marker, M, P, 0, 0, 1, "either", pn)
    calls, wstate, _ = _reference(p, rows, [0, rows.shape[1]])
    wout, wcounts, wpos, winfo = calls[0]
    assert wcounts.min() < wcounts.max() < R.max_frames(rows.shape[1], M, P)
    ch, nbits = rows.shape
    mf = R.max_frames(nbits, M, P)
    src = _device_input(torch, rows, kind)
    specs = {"in": (tuple(src.shape), src.dtype), "out": ((ch, mf * P), torch.uint8), "counts": ((ch, 1), torch.int32),
             "pos": ((ch, mf), torch.int64), "info": ((ch, mf), torch.int32)}
    leads = {"in": range(16) if kind == "bytes" else range(4), "out": range(16), "counts": range(4), "pos": range(2), "info": range(4)}
    bank = sd.frame_sync_bank(marker, M, P, 0, 0, 1, "either", pn, kind, max_channels=ch, max_bits=nbits)
    bank.set_variant(variant)
    try:
        for lead in range(16):
            for fill in (0, 1):
                ar, view, before = {}, {}, {}
                for name, (shape, dt) in specs.items():
                    ld = list(leads[name])[lead % len(leads[name])]
                    ar[name], view[name] = arena.framed(torch, shape, dt, ld, 256, arena.fills(dt)[fill])
                view["in"].copy_(src)
                for name in specs:
                    before[name] = ar[name].clone()
                bank.reset()
                bank.process_ptr(view["in"].data_ptr(), view["out"].data_ptr(), view["counts"].data_ptr(), view["pos"].data_ptr(),
                                 view["info"].data_ptr(), ch, nbits, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                tag = ("framed", kind, variant, lead, fill)
                assert torch.equal(ar["in"], before["in"]), (tag, "in was written")
                assert np.array_equal(view["counts"].cpu().numpy().reshape(-1).astype(np.uint32), wcounts), tag
                # what may change: the first counts[c] slots of every row
                for name, width in (("out", P), ("pos", 1), ("info", 1), ("counts", None)):
                    allowed = torch.zeros(view[name].shape, dtype=torch.bool, device="cuda")
                    for c in range(ch):
                        allowed[c, :(1 if width is None else int(wcounts[c]) * width)] = True
                    mask = torch.zeros(ar[name].numel(), dtype=torch.bool, device="cuda")
                    start = (view[name].data_ptr() - ar[name].data_ptr()) // ar[name].element_size()
                    mask[start:start + view[name].numel()] = allowed.reshape(-1)
                    changed = (ar[name] != before[name]) & ~mask
                    assert not bool(changed.any()), (tag, name, "written outside the addressed slots", torch.nonzero(changed)[:4].tolist())
                for c in range(ch):
                    n = int(wcounts[c])
                    assert np.array_equal(view["out"][c].cpu().numpy()[:n * P].reshape(n, P), wout[c, :n]), (tag, "out", c)
                    assert np.array_equal(view["pos"][c].cpu().numpy()[:n].astype(np.uint64), wpos[c, :n]), (tag, "pos", c)
                    assert np.array_equal(view["info"][c].cpu().numpy()[:n].astype(np.uint32), winfo[c, :n]), (tag, "info", c)
                _check_state(bank, wstate, ch, tag)
    finally:
        torch.cuda.synchronize()
        bank.close()


def test_seeded_random_cross_check(sd, torch_cuda):
    """100 cases over all parameters: marker and payload sizes, tolerance, machine, polarity, pn, channels, input kind, splits and the
    variant of every call"""
    rng = np.random.default_rng(20261021)
    for case in range(100):
        M = int(rng.choice([8, 9, 16, 24, 31, 32, 33, 40, 63, 64]))
        P = int(rng.choice([1, 2, 3, 4, 5, 8, 13, 37]))
        marker = int(rng.integers(0, 1 << 62)) & ((1 << M) - 1) if rng.random() < 0.7 else MARKERS.get(M, (1 << M) - 1)
        tol = int(rng.integers(0, min(15, M // 2 - 1) + 1)) if rng.random() < 0.5 else min(1, M // 2 - 1)
        V, F = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        pol = "either" if rng.random() < 0.6 else "normal"
        pn = rng.integers(0, 256, P, dtype=np.uint8) if rng.random() < 0.5 else None
        channels = int(rng.choice([1, 2, 3, 5, 9]))
        kind = "packed" if rng.random() < 0.5 else "bytes"
        frames = int(rng.integers(3, 12))
        rows, _ = framed_rows(rng, marker, M, P, channels, frames, pn, prefix=lambda c: int(rng.integers(0, 64)),
                              invert_from=int(rng.integers(0, frames + 3)))
        rows ^= (rng.random(rows.shape) < rng.choice([0, 0.002, 0.02])).astype(np.uint8)
        N = rows.shape[1]
        step = 32 if kind == "packed" else 1
        cuts = sorted({0, N, *(int(v) // step * step for v in rng.integers(0, N + 1, int(rng.integers(0, 6))))})
        variants = tuple(int(v) for v in rng.integers(0, 2, 3))
        run_bank(sd, torch_cuda, (marker, M, P, tol, V, F, pol, pn), rows, kind, cuts, variants, tag=("fuzz", case))


def test_refusals_and_empty_calls_on_the_device(sd, torch_cuda):
    torch = torch_cuda
    import simpledsp_amd._lib as L
    bank = sd.frame_sync_bank(0xEB90, 16, 4, 1, 1, 1, "either", None, "packed", max_channels=2, max_bits=256)
    lib = bank._lib
    src = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    out = torch.full((2, 6, 4), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    call = lambda i, o, c, ch, n: lib.sdsp_hip_fsync_process(bank._plan, i, o, c, None, None, ch, n, None)  # noqa: E731
    assert call(src.data_ptr(), out.data_ptr(), counts.data_ptr(), 3, 256) == INVALID_SIZE
    assert call(src.data_ptr(), out.data_ptr(), counts.data_ptr(), 2, 288) == INVALID_SIZE
    assert call(src.data_ptr(), out.data_ptr(), counts.data_ptr(), 2, 100) == INVALID_SIZE
    assert call(None, out.data_ptr(), counts.data_ptr(), 2, 256) == INVALID_ARG
    assert call(src.data_ptr(), out.data_ptr(), None, 2, 256) == INVALID_ARG
    assert call(src.data_ptr() + 1, out.data_ptr(), counts.data_ptr(), 2, 256) == INVALID_ARG
    assert call(src.data_ptr(), out.data_ptr(), counts.data_ptr() + 2, 2, 256) == INVALID_ARG
    assert call(src.data_ptr(), src.data_ptr(), counts.data_ptr(), 2, 256) == INVALID_ARG
    assert call(src.data_ptr(), out.data_ptr(), out.data_ptr() + 4, 2, 256) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_set_variant(bank._plan, 2) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_get_state(bank._plan, None, None, None, None, None, None, None, 3) == INVALID_SIZE
    torch.cuda.synchronize()
    assert (out == 9).all() and (counts == 9).all() and not bank.state()["seen"].any()
    assert call(None, None, None, 0, 256) == 0  # channels == 0: nothing is touched
    assert call(None, out.data_ptr(), counts.data_ptr(), 2, 0) == 0  # nbits == 0: counts alone
    torch.cuda.synchronize()
    assert (out == 9).all() and (counts == 0).all() and not bank.state()["seen"].any()
    assert bank.launches(2, 256) == 5 and bank.launches(2, 0) == 0 and bank.launches(0, 256) == 0
    bank.set_variant(1)
    assert bank.launches(2, 256) == 1 and bank.info["kernel"] == "sdsp_fsync_plain_kernel"
    assert bank.state_bytes() == 2 * (16 + bank.info["ring_words"]) * 4 and bank.info["ring_words"] == (48 + 16 + 31) // 32 + 1
    assert L.FSYNC_PACKED == 1
    bank.close()


def test_process_is_captured_into_a_graph(sd, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(5)
    M, P = 32, 4
    p = (MARKERS[M], M, P, 0, 0, 0, "either", None)
    rows, _ = framed_rows(rng, MARKERS[M], M, P, 3, 5)
    (wout, wcounts, wpos, winfo) = _reference(p, rows, [0, rows.shape[1]])[0][0]
    mf = R.max_frames(rows.shape[1], M, P)
    bank = sd.frame_sync_bank(MARKERS[M], M, P, 0, 0, 0, "either", None, "bytes", max_channels=3, max_bits=rows.shape[1])
    src = _device_input(torch, rows, "bytes")
    out = torch.zeros((3, mf, P), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((3,), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            bank.process_ptr(src.data_ptr(), out.data_ptr(), counts.data_ptr(), None, None, 3, rows.shape[1], s.cuda_stream)
    assert not counts.any()  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), wcounts)
    for c in range(3):
        assert np.array_equal(out[c, :int(wcounts[c])].cpu().numpy(), wout[c, :wcounts[c]])
    bank.close()


CHAIN = dict(frames=5, rows=3, K=7, gens=(0o171, 0o133), B=32, D=64, seed=515, flips=40)
CCSDS_RS = (0x187, 112, 11, 32, 255)


@pytest.mark.parametrize("inverted", [False, True])
def test_viterbi_frame_sync_reed_solomon_chain(sd, torch_cuda, inverted):
    """payloads -> RS(255, 223) -> marker and pn -> K = 7 code -> hard +-40 soft values with sign errors -> viterbi_bank (packed) ->
    frame_sync_bank (packed) -> rs_decoder, all on the device.  Every frame the reference synchroniser emits on the Viterbi bank's
    bits comes back as the payload sent, and the reference emits at least frames - 2 per row: all but the verify frame and the frame
    the decoder's delay cuts."""
    torch = torch_cuda
    c = CHAIN
    rng = np.random.default_rng(c["seed"])
    P, M = 255, 32
    L = M + 8 * P
    pn = sd.ccsds_pn(P)
    data = rng.integers(0, 256, (c["rows"], c["frames"], 223), dtype=np.uint8)
    soft = []
    for r in range(c["rows"]):
        line = sd.attach_sync(sd.rs_encode(data[r], *CCSDS_RS), sd.CCSDS_ASM, M, pn)
        line = np.concatenate([rng.integers(0, 2, 13 + 7 * r, dtype=np.uint8), line])  # the transmitter's start
        padded = np.zeros(-(-(c["frames"] * L + 27) // c["B"]) * c["B"], dtype=np.uint8)
        padded[:line.size] = line
        coded = sd.conv_encode(padded, c["K"], c["gens"])
        s = (40 * (1 - 2 * coded.astype(np.int16))).astype(np.int8)
        s[rng.permutation(s.size)[:c["flips"]]] *= -1
        soft.append(-s if inverted else s)
    soft = np.stack(soft)
    vit = sd.viterbi_bank(c["K"], c["gens"], c["B"], c["D"], "i8", "packed", max_channels=c["rows"])
    words = vit.process(torch.from_numpy(soft).cuda())
    nbits = words.shape[1] * 32
    bits = np.unpackbits(words.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
    assert bits.shape == (c["rows"], nbits)
    ref = R.FrameSync(sd.CCSDS_ASM, M, P, 2, 1, 1, R.EITHER, pn, c["rows"])
    wout, wcounts, wpos, winfo = ref.process(bits)
    assert (wcounts >= c["frames"] - 2).all(), wcounts
    assert (((winfo >> 8) & 1)[:, 0] == int(inverted)).all()
    dec = sd.rs_decoder(*CCSDS_RS, interleave=1, out_kind="data")
    for variant in (0, 1):
        bank = sd.frame_sync_bank(sd.CCSDS_ASM, M, P, 2, 1, 1, "either", pn, "packed", max_channels=c["rows"], max_bits=nbits)
        bank.set_variant(variant)
        frames, counts, pos, info = bank.process(words, records=True)
        _check_call((frames, counts, pos, info), (wout, wcounts, wpos, winfo), ("chain", variant))
        for r in range(c["rows"]):
            n = int(wcounts[r])
            out, cnt = dec.process(frames[r, :n].contiguous())
            first = (int(wpos[r, 0]) - vit.delay - (13 + 7 * r)) // L  # which of the frames sent the first one emitted is
            assert (cnt.cpu().numpy() >= 0).all()
            assert np.array_equal(out.cpu().numpy().reshape(n, 223), data[r, first:first + n]), ("chain", variant, r)
        torch.cuda.synchronize()
        bank.close()
    dec.close()
    vit.close()
