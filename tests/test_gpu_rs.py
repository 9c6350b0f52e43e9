"""GPU tests of the Reed-Solomon decoder banks (sdsp_hip_rs_*) on a real MI355X.

The checker is tests/rs_ref.py, the contract in numpy, itself held to brute force in tests/test_rs_host.py.  Everything is on
integers, so both kernel variants are held to the reference bit for bit: the output, the counts, and every byte of a codeword that
failed.  The reference is worked once per code, on a pool of planted codewords (the cases of `_pool`); a call's frames are put
together from the pool and from clean codewords, which cost the reference their syndromes."""
import functools

import numpy as np
import pytest

import arena
import rs_ref as R

pytestmark = pytest.mark.gpu

CCSDS = (0x187, 112, 11, 32, 255)
CODES = [(CCSDS, 1), (CCSDS, 5), ((0x187, 112, 11, 16, 255), 8), ((0x11D, 0, 1, 16, 204), 1), ((0x11D, 1, 1, 64, 255), 16),
         ((0x11D, 1, 1, 2, 3), 1), ((0x11D, 1, 1, 3, 63), 1), ((0x11D, 1, 1, 3, 64), 1), ((0x11D, 1, 1, 3, 65), 1), ((0x11D, 1, 1, 3, 129), 1)]
FRAMES = (1, 3, 67)
INVALID_SIZE, INVALID_ARG = -1, -5


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


@functools.lru_cache(maxsize=None)
def _code(params):
    return R.Code(*params)


def _hit(rng, word, positions):
    """another value at every one of `positions`"""
    p = np.asarray(positions, dtype=np.int64)
    word[p] ^= rng.integers(1, 256, len(p), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _pool(params, seed=0):
    """the planted codewords of a code, the issue's list: (sent, received, flags, reference output, reference counts, labels)"""
    code = _code(params)
    n, k, nroots, t = code.n, code.k, code.nroots, code.t
    rng = np.random.default_rng(1000 * nroots + n + seed)
    cases = []

    def add(label, errors=(), erased=(), hit_erased=True, word=None):
        sent = code.encode(rng.integers(0, 256, (1, k), dtype=np.uint8))[0]
        r = sent.copy() if word is None else word
        errors = [p for p in dict.fromkeys(int(p) for p in errors) if 0 <= p < n]
        erased = [int(p) for p in erased]
        if word is None:
            _hit(rng, r, errors)
            if hit_erased and erased:
                _hit(rng, r, [p for p in erased if p not in errors])
        flags = np.zeros(n, dtype=np.uint8)
        flags[erased] = rng.integers(1, 256, len(erased), dtype=np.uint8)  # any non-zero byte marks
        cases.append((label, sent, r, flags))

    def pick(count, among=None):
        among = np.arange(n) if among is None else np.asarray(among)
        return rng.permutation(among)[:min(count, len(among))]

    for e in (0, 1, t, t + 1, t + 2):
        add(f"{e} errors", pick(e))
    for p in (0, n - 1, 63, 64, k - 1, k):
        add(f"error at {p}", [p])
    add("burst over the edge", range(k - t // 2, k - t // 2 + t))
    add("parity only", pick(t, np.arange(k, n)))
    for ne in (1, nroots, nroots + 1):
        add(f"{ne} erasures", (), pick(ne))
    e = max(1, t // 2)
    for total in (nroots, nroots + 1):
        if total - 2 * e >= 0:
            pos = pick(e + total - 2 * e)
            add(f"2e + E = {total}", pos[:e], pos[e:])
    add("flags on correct symbols", (), pick(min(3, nroots)), hit_erased=False)
    pos = pick(nroots + 1)
    add("E = nroots, an error outside", pos[:1], pos[1:])
    add("all zero", word=np.zeros(n, dtype=np.uint8))
    add("random word", word=rng.integers(0, 256, n, dtype=np.uint8))
    labels = [c[0] for c in cases]
    sent = np.stack([c[1] for c in cases])
    recv = np.stack([c[2] for c in cases])
    flags = np.stack([c[3] for c in cases])
    out, cnt = code.decode_words(recv, flags)
    return sent, recv, flags, out, cnt, labels


def _outcomes(sent, out, cnt):
    ok = (cnt > 0) & (out == sent).all(axis=1)
    return int(ok.sum()), int((cnt < 0).sum()), int(((cnt >= 0) & (out != sent).any(axis=1)).sum())


def _frames(params, interleave, frames, seed=0, with_flags=True):
    """`frames` frames put together from the pool (every case once where there is room, a rotation of them where not) and clean
    codewords: (received, flags, expected out, expected counts), frames as (frames, I n)"""
    code = _code(params)
    sent, recv, flags, out, cnt, _ = _pool(params)
    if not with_flags:  # only the cases without flags keep their reference result
        keep = ~flags.any(axis=1)
        recv, flags, out, cnt = recv[keep], flags[keep], out[keep], cnt[keep]
    N, C = frames * interleave, len(recv)
    rng = np.random.default_rng(seed + 31 * frames + interleave)
    w = code.encode(rng.integers(0, 256, (N, code.k), dtype=np.uint8))
    f = np.zeros((N, code.n), dtype=np.uint8)
    want, wcnt = w.copy(), np.zeros(N, dtype=np.int32)
    where = rng.permutation(N)[:C] if N >= C else np.arange(N)
    which = np.arange(C) if N >= C else (np.arange(N) + seed + frames) % C
    w[where], f[where], want[where], wcnt[where] = recv[which], flags[which], out[which], cnt[which]
    return R.to_frames(w, interleave), R.to_frames(f, interleave), R.to_frames(want, interleave), wcnt


def _run(sd, torch, params, interleave, variant, recv, flags=None, out_kind="full", inplace=False, corrected=None):
    dec = sd.rs_decoder(*params, interleave=interleave, out_kind=out_kind)
    dec.set_variant(variant)
    assert dec.info()["kernel"] == ("sdsp_rs_wave_kernel", "sdsp_rs_plain_kernel")[variant] and dec.launches(len(recv)) == 1
    x = torch.from_numpy(recv).cuda()
    e = None if flags is None else torch.from_numpy(flags).cuda()
    out, cnt = dec.process(x, e, out=x if inplace else None, corrected=corrected)
    torch.cuda.synchronize()
    dec.close()
    return out.cpu().numpy(), None if cnt is None else cnt.cpu().numpy(), x.cpu().numpy()


@pytest.mark.parametrize("params,interleave", CODES)
def test_both_variants_equal_the_reference_bit_for_bit(sd, torch_cuda, params, interleave):
    sent, _, _, out, cnt, labels = _pool(params)
    good, failed, other = _outcomes(sent, out, cnt)
    print(params, interleave, dict(zip(labels, cnt.tolist())))
    assert good > 0 and failed > 0 and other > 0, (good, failed, other)  # on the reference, before the GPU is looked at
    for frames in FRAMES:
        recv, flags, want, wcnt = _frames(params, interleave, frames)
        if frames == 67 or frames * interleave >= len(labels):
            assert (wcnt > 0).any() and (wcnt < 0).any()
        for variant in (0, 1):
            got, gcnt, x = _run(sd, torch_cuda, params, interleave, variant, recv, flags)
            assert np.array_equal(gcnt, wcnt), (params, interleave, frames, variant, np.flatnonzero(gcnt != wcnt)[:8], gcnt[gcnt != wcnt][:8],
                                                wcnt[gcnt != wcnt][:8])
            assert np.array_equal(got, want), (params, interleave, frames, variant)
            assert np.array_equal(x, recv)  # out of place: the input stays


@pytest.mark.parametrize("params,interleave", [(CCSDS, 5), ((0x11D, 0, 1, 16, 204), 1), ((0x11D, 1, 1, 3, 65), 1)])
def test_forms_of_a_call(sd, torch_cuda, params, interleave):
    """in place against out of place, DATA against the prefix of FULL, `corrected` left out, no erasure input"""
    torch = torch_cuda
    code = _code(params)
    recv, flags, want, wcnt = _frames(params, interleave, 9, seed=3)
    recv0, _, want0, wcnt0 = _frames(params, interleave, 9, seed=4, with_flags=False)
    for variant in (0, 1):
        got, gcnt, x = _run(sd, torch, params, interleave, variant, recv, flags, inplace=True)
        assert np.array_equal(x, want) and np.array_equal(got, want) and np.array_equal(gcnt, wcnt)
        got, gcnt, x = _run(sd, torch, params, interleave, variant, recv, flags, out_kind="data")
        assert got.shape == (9, interleave * code.k) and np.array_equal(got, want[:, :interleave * code.k])
        assert np.array_equal(gcnt, wcnt) and np.array_equal(x, recv)
        got, gcnt, _ = _run(sd, torch, params, interleave, variant, recv, flags, corrected=False)
        assert gcnt is None and np.array_equal(got, want)
        got, gcnt, x = _run(sd, torch, params, interleave, variant, recv, flags, inplace=True, corrected=False)
        assert np.array_equal(x, want)
        got, gcnt, _ = _run(sd, torch, params, interleave, variant, recv0)
        assert np.array_equal(got, want0) and np.array_equal(gcnt, wcnt0)
        assert (wcnt0 < 0).any() and (wcnt0 > 0).any()


def test_a_garbage_codeword_changes_only_its_own_symbols(sd, torch_cuda):
    code = _code(CCSDS)
    I = 5
    rng = np.random.default_rng(8)
    clean = R.encode_frames(code, rng.integers(0, 256, (3, I * code.k), dtype=np.uint8), I)
    recv = clean.copy()
    recv.reshape(3, code.n, I)[1, :, 2] = rng.integers(0, 256, code.n, dtype=np.uint8)
    want, wcnt = R.decode_frames(code, recv, None, I)
    assert wcnt[1 * I + 2] == -1 and np.count_nonzero(wcnt) == 1 and np.array_equal(want, recv)
    for variant in (0, 1):
        for inplace in (False, True):
            got, gcnt, _ = _run(sd, torch_cuda, CCSDS, I, variant, recv, inplace=inplace)
            assert np.array_equal(got, recv) and np.array_equal(gcnt, wcnt)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("out_kind", ["full", "data"])
def test_framed_buffers_at_every_byte_offset(sd, torch_cuda, variant, out_kind):
    """every buffer at every offset 0 .. 15 within 16 bytes (the counts: every multiple of 4); nothing outside a buffer is written and
    the inputs stay"""
    torch = torch_cuda
    params, I, frames = (0x11D, 1, 1, 6, 37), 3, 5  # frames of 111 bytes: every frame of a call lies differently within 16 bytes
    code = _code(params)
    recv, flags, want, wcnt = _frames(params, I, frames, seed=5)
    assert (wcnt > 0).any() and (wcnt < 0).any()
    if out_kind == "data":
        want = np.ascontiguousarray(want[:, :I * code.k])
    dec = sd.rs_decoder(*params, interleave=I, out_kind=out_kind)
    dec.set_variant(variant)
    margin = 64
    for lead in range(16):
        leads = {"in": lead, "flags": (lead * 7 + 3) % 16, "out": (lead * 5 + 1) % 16, "cnt": (lead % 4)}
        a_in, v_in = arena.framed(torch, recv.shape, torch.uint8, leads["in"], margin, 0x55)
        a_fl, v_fl = arena.framed(torch, flags.shape, torch.uint8, leads["flags"], margin, 0x55)
        a_out, v_out = arena.framed(torch, want.shape, torch.uint8, leads["out"], margin, 0x55)
        a_cnt, v_cnt = arena.framed(torch, wcnt.shape, torch.int32, leads["cnt"], margin, 0x55)
        v_in.copy_(torch.from_numpy(recv))
        v_fl.copy_(torch.from_numpy(flags))
        before = [a.clone() for a in (a_in, a_fl, a_out, a_cnt)]
        dec.process(v_in, v_fl, out=v_out, corrected=v_cnt)
        torch.cuda.synchronize()
        assert torch.equal(a_in, before[0]) and torch.equal(a_fl, before[1]), lead
        assert np.array_equal(v_out.cpu().numpy(), want) and np.array_equal(v_cnt.cpu().numpy(), wcnt), lead
        for a, v, b in ((a_out, v_out, before[2]), (a_cnt, v_cnt, before[3])):
            start = (v.data_ptr() - a.data_ptr()) // a.element_size()
            assert torch.equal(a[:start], b[:start]) and torch.equal(a[start + v.numel():], b[start + v.numel():]), lead
        if out_kind == "full":  # in place at the same offsets
            a_in, v_in = arena.framed(torch, recv.shape, torch.uint8, leads["in"], margin, 0x55)
            v_in.copy_(torch.from_numpy(recv))
            b = a_in.clone()
            dec.process(v_in, v_fl, out=v_in, corrected=False)
            torch.cuda.synchronize()
            start = margin + leads["in"]
            assert np.array_equal(v_in.cpu().numpy(), want), lead
            assert torch.equal(a_in[:start], b[:start]) and torch.equal(a_in[start + v_in.numel():], b[start + v_in.numel():]), lead
    dec.close()


def test_refusals_write_nothing(sd, torch_cuda):
    torch = torch_cuda
    I, frames = 2, 3
    dec = sd.rs_decoder(*CCSDS, interleave=I)
    data = sd.rs_decoder(*CCSDS, interleave=I, out_kind="data")
    fb = I * 255
    buf = torch.full((8 * frames * fb,), 0x55, dtype=torch.uint8, device="cuda")
    cnt = torch.full((64,), 0x55, dtype=torch.int32, device="cuda")
    p, c = buf.data_ptr(), cnt.data_ptr()
    far = p + 4 * frames * fb
    lib = sd.load()

    def call(d, src, era, dst, cor, nf):
        return lib.sdsp_hip_rs_process(d._plan, src, era, dst, cor, nf, None)

    assert call(dec, None, None, far, c, frames) == INVALID_ARG
    assert call(dec, p, None, None, c, frames) == INVALID_ARG
    assert call(dec, p, None, far, c, 1 << 31) == INVALID_SIZE
    assert call(dec, p, None, p + 1, c, frames) == INVALID_ARG            # a shifted overlap
    assert call(dec, p, None, p + frames * fb - 1, c, frames) == INVALID_ARG
    assert call(data, p, None, p, c, frames) == INVALID_ARG               # DATA has no in-place form
    assert call(dec, p, p, far, c, frames) == INVALID_ARG                 # erasures over in
    assert call(dec, p, far + 5, far, c, frames) == INVALID_ARG           # erasures over out
    assert call(dec, p, None, far, p + 8, frames) == INVALID_ARG          # corrected over in
    assert call(dec, p, None, far, far + 8, frames) == INVALID_ARG        # corrected over out
    assert call(dec, p, far + 2 * frames * fb, far, far + 2 * frames * fb + 4, frames) == INVALID_ARG  # corrected over erasures
    assert call(dec, p, None, far, c + 2, frames) == INVALID_ARG          # misaligned counts
    assert lib.sdsp_hip_rs_plan_set_variant(dec._plan, 2) == INVALID_ARG
    assert call(dec, None, None, None, None, 0) == 0                       # nothing to do, nothing touched
    torch.cuda.synchronize()
    assert bool((buf == 0x55).all()) and bool((cnt == 0x55).all())
    assert dec.launches(0) == 0 and dec.launches(5) == 1
    i = dec.info()
    assert (i["field_poly"], i["fcr"], i["prim"], i["nroots"], i["n"], i["interleave"], i["k"], i["t"]) == (0x187, 112, 11, 32, 255, I, 223, 16)
    assert i["variant"] == 0 and i["threads"] == 64 * i["waves"] and i["lds_bytes"] >= 768 + i["waves"] * fb and dec.k == 223 and dec.t == 16
    out, cor = dec.process(torch.empty((0, fb), dtype=torch.uint8, device="cuda"))
    assert out.shape == (0, fb) and cor.numel() == 0
    dec.close()
    data.close()


def test_process_host_and_one_shot(sd, torch_cuda):
    params, I = (0x187, 112, 11, 16, 255), 8
    recv, flags, want, wcnt = _frames(params, I, 4, seed=6)
    for variant in (0, 1):
        dec = sd.rs_decoder(*params, interleave=I)
        dec.set_variant(variant)
        out, cnt = dec.process_host(recv, flags)
        assert np.array_equal(out, want) and np.array_equal(cnt, wcnt)
        # the in-place form of the C entry
        x, c = recv.copy(), np.zeros(len(wcnt), dtype=np.int32)
        assert sd.load().sdsp_hip_rs_process_host(dec._plan, x.ctypes.data, flags.ctypes.data, x.ctypes.data, c.ctypes.data, len(x)) == 0
        assert np.array_equal(x, want) and np.array_equal(c, wcnt)
        dec.close()
    out, cnt = sd.rs_decode(recv, *params, interleave=I, erasures=flags, out_kind="data")
    assert np.array_equal(out, want[:, :I * 239]) and np.array_equal(cnt, wcnt)
    t = torch_cuda.from_numpy(recv).cuda()
    out, cnt = sd.rs_decode(t, *params, interleave=I, erasures=torch_cuda.from_numpy(flags).cuda())
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(cnt.cpu().numpy(), wcnt)


def test_sixteen_random_cases_over_all_parameters(sd, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(20261021)
    prims = [p for p in range(1, 255) if np.gcd(p, 255) == 1]
    seen = [0, 0, 0]
    for case in range(16):
        poly = int(rng.choice([0x11D, 0x187, 0x12B, 0x169]))
        fcr, prim = int(rng.integers(0, 255)), int(rng.choice(prims))
        nroots = int(rng.integers(2, 65)) if case % 4 else int(rng.choice([2, 3, 63, 64]))
        n = int(rng.integers(nroots + 1, 256)) if case % 3 else 255
        I = int(rng.integers(1, 17))
        frames = int(rng.integers(1, 12))
        code = R.Code(poly, fcr, prim, nroots, n)
        N = frames * I
        sent = code.encode(rng.integers(0, 256, (N, code.k), dtype=np.uint8))
        recv, flags = sent.copy(), np.zeros((N, n), dtype=np.uint8)
        for m in range(N):
            kind = rng.integers(0, 4)
            if kind == 0:
                continue
            e = int(rng.integers(0, nroots // 2 + (2 if kind == 3 else 1)))
            ne = int(rng.integers(0, max(1, nroots - 2 * e + (2 if kind == 3 else 1)))) if kind >= 2 else 0
            pos = rng.permutation(n)[:min(n, e + ne)]
            _hit(rng, recv[m], pos)
            flags[m, pos[e:]] = 1
        use_flags = bool(flags.any()) and case % 5 != 4
        want, wcnt = code.decode_words(recv, flags if use_flags else None)
        a, b, c = _outcomes(sent, want, wcnt)
        seen = [seen[0] + a, seen[1] + b, seen[2] + c]
        out_kind = ("full", "data")[case % 2]
        want_f = R.to_frames(want, I)[:, :I * (code.k if out_kind == "data" else n)]
        for variant in (0, 1):
            got, gcnt, _ = _run(sd, torch, (poly, fcr, prim, nroots, n), I, variant, R.to_frames(recv, I),
                                R.to_frames(flags, I) if use_flags else None, out_kind=out_kind)
            assert np.array_equal(gcnt, wcnt) and np.array_equal(got, want_f), (case, poly, fcr, prim, nroots, n, I, frames, variant)
    assert seen[0] > 0 and seen[1] > 0, seen


def test_variant_switch_between_two_calls(sd, torch_cuda):
    torch = torch_cuda
    recv, flags, want, wcnt = _frames(CCSDS, 5, 3, seed=7)
    dec = sd.rs_decoder(*CCSDS, interleave=5)
    x, e = torch.from_numpy(recv).cuda(), torch.from_numpy(flags).cuda()
    for variant in (0, 1, 0):
        dec.set_variant(variant)
        assert dec.variant == variant
        out, cnt = dec.process(x, e)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(cnt.cpu().numpy(), wcnt)
    dec.close()


def test_wave_kernel_takes_several_frames_per_wave(sd, torch_cuda):
    """above 8192 frames a wave takes a second frame, and the last workgroup is partial"""
    torch = torch_cuda
    params, I, frames = (0x11D, 1, 1, 4, 20), 1, 3 * 8192 + 5
    code = _code(params)
    rng = np.random.default_rng(9)
    sent = code.encode(rng.integers(0, 256, (frames, code.k), dtype=np.uint8))
    recv = sent.copy()
    hit = rng.random(frames) < 0.01
    recv[hit, rng.integers(0, code.n)] ^= 0x5a
    recv[-1, 3] ^= 1
    want, wcnt = code.decode_words(recv)
    assert np.array_equal(want, sent) and wcnt[-1] == 1
    for variant in (0, 1):
        got, gcnt, _ = _run(sd, torch, params, I, variant, recv)
        assert np.array_equal(got, want) and np.array_equal(gcnt, wcnt)


# Es / N0 = -1 dB is Eb / N0 = 2 dB at rate 1/2: the K = 7 decoder leaves about 4 bit errors in a thousand, in bursts
CHAIN = dict(I=5, frames=2, K=7, gens=(0o171, 0o133), B=32, D=64, seed=2027, es_n0_db=-1.0)


def _chain():
    """the chain's stream and what the references make of it: the soft values, the Viterbi reference's bytes, the data sent and the
    Reed-Solomon reference's counts.  Asserts that the inner decoder alone leaves bit errors and that the outer one removes them all."""
    import viterbi_ref as V
    c = CHAIN
    I, frames, K, gens, B, D = c["I"], c["frames"], c["K"], c["gens"], c["B"], c["D"]
    code = _code(CCSDS)
    rng = np.random.default_rng(c["seed"])
    data = rng.integers(0, 256, (frames, I * code.k), dtype=np.uint8)
    bits = np.unpackbits(R.encode_frames(code, data, I).reshape(-1))  # most significant bit first
    Dr = V.delay(B, D)
    padded = np.zeros(-(-len(bits) // B) * B + Dr, dtype=np.uint8)
    padded[:len(bits)] = bits
    coded = V.encode(padded, K, gens).astype(np.float64)
    sigma = np.sqrt(0.5 / 10 ** (c["es_n0_db"] / 10))  # Es / N0 of a coded symbol
    soft = np.clip(np.rint(((1 - 2 * coded) + sigma * rng.standard_normal(coded.shape)) * 32), -127, 127).astype(np.int8).reshape(1, -1)
    ref_bits = V.ViterbiRef(K, gens, B, D, 1).process(soft)[0, Dr:Dr + len(bits)]
    wrong = int(np.count_nonzero(ref_bits != bits))
    assert 0 < wrong < len(bits) // 100, wrong
    ref_recv = np.packbits(ref_bits).reshape(frames, I * code.n)
    ref_out, ref_cnt = R.decode_frames(code, ref_recv, None, I, "data")
    assert np.array_equal(ref_out, data) and (ref_cnt >= 0).all() and (ref_cnt > 0).any(), ref_cnt
    return soft, len(bits), Dr, data, ref_recv, ref_cnt, wrong


def test_viterbi_then_reed_solomon_chain(sd, torch_cuda):
    """a noisy K = 7 stream through viterbi_bank (bytes), the bits packed in torch, RS(255, 223) at I = 5: the inner decoder alone
    leaves bit errors, the outer one removes them all -- asserted on the references before the GPU is looked at"""
    torch = torch_cuda
    c = CHAIN
    soft, nbits, Dr, data, ref_recv, ref_cnt, _ = _chain()
    bank = sd.viterbi_bank(c["K"], c["gens"], c["B"], c["D"], "i8", "bytes", max_channels=1)
    got_bits = bank.process(torch.from_numpy(soft).cuda())[0, Dr:Dr + nbits]
    weights = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.int32, device="cuda")
    recv = (got_bits.reshape(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8).reshape(ref_recv.shape).contiguous()
    assert np.array_equal(recv.cpu().numpy(), ref_recv)
    for variant in (0, 1):
        dec = sd.rs_decoder(*CCSDS, interleave=c["I"], out_kind="data")
        dec.set_variant(variant)
        out, cnt = dec.process(recv)
        assert np.array_equal(out.cpu().numpy(), data) and np.array_equal(cnt.cpu().numpy(), ref_cnt)
        dec.close()
    bank.close()
