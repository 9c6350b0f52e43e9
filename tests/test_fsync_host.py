"""Host side of the frame synchroniser banks (sdsp_hip_fsync_*), no device: the numpy reference
(tests/fsync_ref.py) against the contract's paragraphs taken literally, bit by bit, on streams where every transition of the machine
occurs; the anchor stream of the contract; the pseudo-randomiser, the transmit helper and the refusals that come before the device is
touched."""
import ctypes as C

import numpy as np
import pytest

import fsync_ref as R

INVALID_SIZE, INVALID_ARG = -1, -5  # SDSP_HIP_ERR_INVALID_SIZE, SDSP_HIP_ERR_INVALID_ARG


def _lib():
    import simpledsp_amd._lib as L
    return L, L.load()


def literal(bits, marker, M, P, tol, V, F, either, pn=None):
    """the contract's paragraphs, one bit at a time, on a whole stream: [(pos, info, payload bytes)], the final machine and the
    transitions taken; a frame accepted whose last bit never arrives stays pending"""
    bits = [1 if b else 0 for b in bits]
    L, n = M + 8 * P, len(bits)
    mk = [(marker >> (M - 1 - i)) & 1 for i in range(M)]

    def d(p):
        return sum(bits[p + i] ^ mk[i] for i in range(M))

    mode, p, pol, count, misses = "search", 0, 0, 0, 0
    frames, pending, taken = [], 0, set()

    def accept(p, fly):
        nonlocal pending
        if p + L > n:
            pending = 1
            return
        dist = d(p) if pol == 0 else M - d(p)
        body = []
        for i in range(P):
            v = 0
            for b in range(8):
                v = 2 * v + bits[p + M + 8 * i + b]
            if pol:
                v ^= 0xFF
            if pn is not None:
                v ^= int(pn[i])
            body.append(v)
        frames.append((p, dist | (pol << 8) | (fly << 9), bytes(body)))

    while p + M <= n:
        if mode == "search":
            normal, inverted = d(p) <= tol, either and M - d(p) <= tol
            if normal or inverted:
                pol, count, misses = (0 if normal else 1), 0, 0
                if V == 0:
                    mode = "lock"
                    accept(p, 0)
                    taken.add("search-lock")
                else:
                    mode = "verify"
                    taken.add("search-verify")
                p += L
            else:
                p += 1
        elif mode == "verify":
            if (d(p) if pol == 0 else M - d(p)) <= tol:
                count += 1
                if count == V:
                    mode = "lock"
                    accept(p, 0)
                    taken.add("verify-lock")
                else:
                    taken.add("verify-verify")
                p += L
            else:
                mode, p = "search", p - L + 1
                taken.add("verify-search")
        else:
            if (d(p) if pol == 0 else M - d(p)) <= tol:
                misses = 0
                accept(p, 0)
                p += L
                taken.add("lock-hit")
            else:
                misses += 1
                if misses > F:
                    mode = "search"
                    taken.add("lock-search")
                else:
                    accept(p, 1)
                    p += L
                    taken.add("lock-flywheel")
    state = (["search", "verify", "lock"].index(mode), p, pol, count, misses, pending, n)
    return frames, state, taken


def _ref_frames(fs, rows, splits=()):
    """the reference over the calls `splits` cuts the rows into: per row [(pos, info, bytes)]"""
    edges = [0, *splits, rows.shape[1]]
    got = [[] for _ in rows]
    for a, b in zip(edges, edges[1:]):
        out, counts, pos, info = fs.process(rows[:, a:b])
        for c in range(rows.shape[0]):
            got[c] += [(int(pos[c, k]), int(info[c, k]), out[c, k].tobytes()) for k in range(counts[c])]
    return got


@pytest.mark.parametrize("V,F,either", [(0, 0, True), (1, 1, True), (2, 1, False), (3, 2, True), (1, 0, False)])
def test_reference_equals_the_contract_bit_by_bit(V, F, either):
    rng = np.random.default_rng(1000 + 16 * V + 2 * F + either)
    M, P, tol, marker = 8, 2, 1, 0xB8
    pn = rng.integers(0, 256, P, dtype=np.uint8)
    taken = set()
    for trial in range(12):
        # stretches of framed data (some inverted, some with marker errors) between stretches of noise: false hits are frequent at M = 8
        parts = []
        for _ in range(6):
            parts.append(rng.integers(0, 2, int(rng.integers(0, 40)), dtype=np.uint8))
            body = R.attach(rng.integers(0, 256, (int(rng.integers(1, 9)), P), dtype=np.uint8), marker, M, pn, bool(rng.integers(0, 2)))
            flips = rng.random(body.size) < 0.03
            parts.append(body ^ flips.astype(np.uint8))
        row = np.concatenate(parts)
        want, wstate, t = literal(row, marker, M, P, tol, V, F, either, pn)
        taken |= t
        for splits in ((), sorted(rng.integers(0, row.size + 1, 7).tolist())):
            fs = R.FrameSync(marker, M, P, tol, V, F, R.EITHER if either else R.NORMAL, pn)
            got = _ref_frames(fs, row[None, :], splits)[0]
            assert got == want, (trial, splits)
            assert tuple(int(v[0]) for v in fs.state()) == wstate, (trial, splits)
    need = {"search-lock", "lock-hit", "lock-search"} if V == 0 else {"search-verify", "verify-lock", "verify-search", "lock-hit", "lock-search"}
    if V > 1:
        need.add("verify-verify")
    if F > 0:
        need.add("lock-flywheel")
    assert need <= taken, need - taken


def test_every_transition_of_the_machine_is_taken_by_the_reference_itself():
    rng = np.random.default_rng(77)
    M, P, marker = 8, 2, 0xB8
    fs = R.FrameSync(marker, M, P, 1, 2, 1, R.EITHER)
    row = np.concatenate([rng.integers(0, 2, 30, dtype=np.uint8), R.attach(rng.integers(0, 256, (8, P), dtype=np.uint8), marker, M),
                          rng.integers(0, 2, 400, dtype=np.uint8), R.attach(rng.integers(0, 256, (6, P), dtype=np.uint8), marker, M, None, True),
                          rng.integers(0, 2, 300, dtype=np.uint8)])
    fs.process(row[None, :])
    # the six transitions of the contract's machine: SEARCH -> VERIFY, VERIFY -> LOCK, VERIFY -> SEARCH, LOCK hit, LOCK flywheel, LOCK -> SEARCH
    assert {"search-verify", "verify-lock", "verify-search", "lock-hit", "lock-flywheel", "lock-search"} <= fs.transitions, fs.transitions


def anchor_stream(payloads, rng):
    """7 arbitrary bits, three clean frames, one with its first 3 marker bits flipped, one clean, a slip of one bit, four clean, three
    inverted, 20 arbitrary bits; M = 16, marker 0xEB90, P = 4"""
    f = [R.attach(payloads[i], 0xEB90, 16) for i in range(9)] + [R.attach(payloads[i], 0xEB90, 16, None, True) for i in range(9, 12)]
    f[3] = f[3].copy()
    f[3][:3] ^= 1
    return np.concatenate([rng.integers(0, 2, 7, dtype=np.uint8), *f[:5], rng.integers(0, 2, 1, dtype=np.uint8), *f[5:],
                           rng.integers(0, 2, 20, dtype=np.uint8)])


def test_anchor_stream():
    rng = np.random.default_rng(20261021)
    payloads = rng.integers(0, 256, (12, 4), dtype=np.uint8)
    row = anchor_stream(payloads, rng)
    assert row.size == 7 + 12 * 48 + 1 + 20
    # (V, F) = (0, 0): every clean frame, the damaged one at 151 dropped, the slip followed, the inverted run taken
    fs = R.FrameSync(0xEB90, 16, 4, 1, 0, 0, R.EITHER)
    got = _ref_frames(fs, row[None, :])[0]
    want, wstate, _ = literal(row, 0xEB90, 16, 4, 1, 0, 0, True)
    assert got == want and tuple(int(v[0]) for v in fs.state()) == wstate
    pos = [g[0] for g in got]
    assert pos[:4] == [7, 55, 103, 199] and 151 not in pos
    assert [q for q in pos if q >= 248 and (q - 248) % 48 == 0] == [248, 296, 344, 392, 440, 488, 536]
    assert pos == [7, 55, 103, 199, 248, 296, 344, 392, 440, 488, 536], pos  # these payloads bring no false hit in between
    by_pos = {g[0]: g for g in got}
    assert [by_pos[q][1] >> 8 for q in (392, 440, 488, 536)] == [0, 1, 1, 1]
    sent = {7 + 48 * i: payloads[i].tobytes() for i in range(5)}
    sent.update({248 + 48 * i: payloads[5 + i].tobytes() for i in range(7)})
    assert all(by_pos[q][2] == sent[q] for q in pos)
    # (V, F) = (1, 1): the first frame verifies, the damaged one rides the flywheel with distance 3, the slip costs one flywheel frame
    # and a new search, which locks again at 344
    fs = R.FrameSync(0xEB90, 16, 4, 1, 1, 1, R.EITHER)
    got = _ref_frames(fs, row[None, :], (5, 100, 101, 130, 400))[0]
    want, wstate, _ = literal(row, 0xEB90, 16, 4, 1, 1, 1, True)
    assert got == want and tuple(int(v[0]) for v in fs.state()) == wstate
    assert [g[0] for g in got[:5]] == [55, 103, 151, 199, 247]
    assert got[2][1] == (3 | 0x200) and got[4][1] & 0x200 and not got[3][1] & 0x200
    assert [g[0] for g in got[5:]][0] == 344, [g[0] for g in got]


def test_ccsds_pn_first_bytes_and_period():
    import simpledsp_amd as sd
    pn = sd.ccsds_pn(1275)
    assert pn.dtype == np.uint8 and list(pn[:8]) == [0xFF, 0x48, 0x0E, 0xC0, 0x9A, 0x0D, 0x70, 0xBC]
    assert np.array_equal(pn, R.ccsds_pn(1275))
    b = np.unpackbits(pn)
    assert np.array_equal(b[255:], b[:-255])
    assert all(not np.array_equal(b[k:], b[:-k]) for k in range(1, 255))
    assert sd.ccsds_pn(0).size == 0 and sd.CCSDS_ASM == 0x1ACFFC1D == R.CCSDS_ASM


@pytest.mark.parametrize("M,marker,P,invert,use_pn", [(32, 0x1ACFFC1D, 9, False, True), (8, 0x47, 3, True, False), (64, 0x034776C7272895B0, 5, True, True),
                                                      (33, 0x1ACFFC1D5, 1, False, False)])
def test_attach_then_reference_returns_the_payloads(M, marker, P, invert, use_pn):
    import simpledsp_amd as sd
    rng = np.random.default_rng(M + P)
    pn = sd.ccsds_pn(P) if use_pn else None
    payloads = rng.integers(0, 256, (6, P), dtype=np.uint8)
    row = sd.attach_sync(payloads, marker, M, pn, invert)
    assert row.dtype == np.uint8 and np.array_equal(row, R.attach(payloads, marker, M, pn, invert))
    fs = R.FrameSync(marker, M, P, 0, 0, 0, R.EITHER, pn)
    got = _ref_frames(fs, np.concatenate([np.zeros(5, dtype=np.uint8), row])[None, :])[0]
    assert [g[0] for g in got] == [5 + k * (M + 8 * P) for k in range(6)]
    assert all(g[2] == payloads[k].tobytes() and g[1] == (0x100 if invert else 0) for k, g in enumerate(got))
    assert sd.fsync_max_frames(M, P, 5 + row.size) == 7 == R.max_frames(5 + row.size, M, P)


GOOD = dict(marker=0x1ACFFC1D, M=32, P=255, tol=2, V=1, F=1, pol=1, kind=0, ch=4, bits=4096)


@pytest.mark.parametrize("change,code", [
    (dict(M=7), INVALID_SIZE), (dict(M=65), INVALID_SIZE), (dict(P=0), INVALID_SIZE), (dict(P=8193), INVALID_SIZE),
    (dict(V=256), INVALID_SIZE), (dict(F=256), INVALID_SIZE), (dict(ch=0), INVALID_SIZE), (dict(ch=1 << 31), INVALID_SIZE),
    (dict(bits=0), INVALID_SIZE), (dict(bits=1 << 31), INVALID_SIZE),
    (dict(tol=16), INVALID_ARG), (dict(M=8, marker=0x47, tol=4), INVALID_ARG), (dict(M=16, marker=0x1EB90), INVALID_ARG),
    (dict(pol=2), INVALID_ARG), (dict(kind=2), INVALID_ARG), (dict(kind=-1), INVALID_ARG),
])
def test_creation_refusals_need_no_device(change, code):
    L, lib = _lib()
    a = dict(GOOD, **change)
    h = C.c_void_p(0x1234)
    assert lib.sdsp_hip_fsync_plan_create(C.byref(h), a["marker"], a["M"], a["P"], a["tol"], a["V"], a["F"], a["pol"], None, a["kind"],
                                          a["ch"], a["bits"], 0) == code
    assert not h.value and lib.sdsp_hip_last_error_string()


def test_null_pointers_and_helper_refusals():
    L, lib = _lib()
    assert lib.sdsp_hip_fsync_plan_create(None, 0x1ACFFC1D, 32, 255, 0, 1, 1, 1, None, 0, 1, 64, 0) == INVALID_ARG
    assert lib.sdsp_hip_fsync_process(None, None, None, None, None, None, 0, 0, None) == INVALID_ARG
    assert lib.sdsp_hip_fsync_process_host(None, None, None, None, None, None, 0, 0) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_reset(None) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_get_state(None, None, None, None, None, None, None, None, 0) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_state_bytes(None, None) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_set_variant(None, 0) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_launches(None, 1, 1, None) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_get_info(None, None) == INVALID_ARG
    assert lib.sdsp_hip_fsync_plan_destroy(None) == 0
    assert lib.sdsp_hip_fsync_ccsds_pn(None, 4) == INVALID_ARG and lib.sdsp_hip_fsync_ccsds_pn(None, 0) == 0
    n = C.c_uint64(7)
    assert lib.sdsp_hip_fsync_max_frames(7, 4, 100, C.byref(n)) == INVALID_SIZE
    assert lib.sdsp_hip_fsync_max_frames(16, 0, 100, C.byref(n)) == INVALID_SIZE
    assert lib.sdsp_hip_fsync_max_frames(16, 4, 100, None) == INVALID_ARG and n.value == 7
    assert lib.sdsp_hip_fsync_max_frames(16, 4, 96, C.byref(n)) == 0 and n.value == 2
    assert lib.sdsp_hip_fsync_max_frames(16, 4, 97, C.byref(n)) == 0 and n.value == 3
    f = np.zeros(4, dtype=np.uint8)
    o = np.full(48, 7, dtype=np.uint8)
    assert lib.sdsp_hip_fsync_attach(0xEB90, 16, 4, None, f.ctypes.data, 1, 0, None) == INVALID_ARG
    assert lib.sdsp_hip_fsync_attach(0xEB90, 16, 4, None, None, 1, 0, o.ctypes.data) == INVALID_ARG
    assert lib.sdsp_hip_fsync_attach(0x1EB90, 16, 4, None, f.ctypes.data, 1, 0, o.ctypes.data) == INVALID_ARG
    assert lib.sdsp_hip_fsync_attach(0xEB90, 65, 4, None, f.ctypes.data, 1, 0, o.ctypes.data) == INVALID_SIZE
    assert (o == 7).all()


def test_header_declares_no_stride_for_the_fsync_entries():
    from conftest import ROOT
    text = (ROOT / "include" / "sdsp_hip.h").read_text()
    start = text.index("int sdsp_hip_fsync_ccsds_pn")
    assert "stride" not in text[start:text.index("sdsp_hip_fsync_plan_get_info", start)]
