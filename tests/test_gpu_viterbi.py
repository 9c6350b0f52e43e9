"""GPU tests of the streaming Viterbi decoder banks (sdsp_hip_viterbi_*) on a real MI355X.

The checker is tests/viterbi_ref.py, the contract in numpy, itself held to brute force in tests/test_viterbi_host.py.  Everything is
on integers, so every kernel variant a plan has is held to the reference bit for bit: the decoded bits, the path metrics and, by
continuing the stream, the decisions the state holds.  The shapes are small on purpose; the cases beyond the issue's table are the
ones at which the kernels take another path: a call longer than a chunk (with a ragged last chunk), and the K = 9 traceback that does
not fit LDS."""

import numpy as np
import pytest

import arena
import viterbi_ref as ref

pytestmark = pytest.mark.gpu

GENS = {(3, 2): (0o7, 0o5), (5, 2): (0o23, 0o35), (7, 2): (0o171, 0o133), (9, 2): (0o561, 0o753),
        (3, 3): (0o7, 0o5, 0o3), (5, 3): (0o25, 0o33, 0o37), (7, 3): (0o171, 0o133, 0o165), (9, 3): (0o557, 0o663, 0o711)}
SCALE = 8.0  # a power of two: (j + 0.5) / 8 is exact, so the F32 rows hold true ties of the rounding
IN_KINDS = ["i8", "f32"]
OUT_KINDS = ["bytes", "packed"]


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


def _variants(k):
    return (0, 1) if k == 7 else (1,)


def _soft(sd, rng, k, gens, channels, steps, in_kind):
    """rows of a noisy coded stream with erasures, -128 and 127 sprinkled in; F32 rows carry exact ties of the quantiser"""
    n = len(gens)
    bits = rng.integers(0, 2, (channels, steps)).astype(np.uint8)
    coded = np.stack([sd.conv_encode(b, k, gens) for b in bits]).astype(np.float64)
    v = np.clip(np.rint((1 - 2 * coded) * 40 + 35 * rng.standard_normal(coded.shape)), -128, 127)
    u = rng.random(coded.shape)
    v[u < 0.02] = 0
    v[(u >= 0.02) & (u < 0.03)] = -128
    v[(u >= 0.03) & (u < 0.04)] = 127
    if in_kind == "i8":
        return v.astype(np.int8).reshape(channels, steps * n)
    frac = rng.choice(np.array([0.0, 0.5, -0.5, 0.25, 0.3], dtype=np.float64), coded.shape)
    return ((v + frac) / SCALE).astype(np.float32).reshape(channels, steps * n)


def _bank(sd, k, gens, B, D, in_kind, out_kind, channels, variant, start=-1):
    bank = sd.viterbi_bank(k, gens, B, D, in_kind, out_kind, scale=SCALE, max_channels=channels)
    bank.set_variant(variant)
    if start >= 0:
        bank.reset(start)
    return bank


def _out(t, out_kind):
    a = t.cpu().numpy()
    return a.view(np.uint32) if out_kind == "packed" else a


def _want(bits, out_kind):
    return ref.pack_bits(bits) if out_kind == "packed" else bits


def _run(sd, torch, k, gens, B, D, in_kind, out_kind, channels, variants, calls, start=-1):
    """the calls through one bank, call i in variant variants[i % len]: ([outputs], final metrics)"""
    bank = _bank(sd, k, gens, B, D, in_kind, out_kind, channels, variants[0], start)
    outs = []
    for i, x in enumerate(calls):
        bank.set_variant(variants[i % len(variants)])
        outs.append(_out(bank.process(torch.from_numpy(x).cuda()), out_kind))
    torch.cuda.synchronize()
    m = bank.metrics()
    bank.close()
    return outs, m


def _ref_run(k, gens, B, D, in_kind, channels, calls, start=-1):
    dec = ref.ViterbiRef(k, gens, B, D, channels, start_state=start, in_kind=in_kind, scale=SCALE)
    outs = [dec.process(x) for x in calls]
    return outs, dec.metrics()


def _split(x, n, B, blocks):
    t, parts = 0, []
    for b in blocks:
        parts.append(np.ascontiguousarray(x[:, t * n:(t + b * B) * n]))
        t += b * B
    assert t * n == x.shape[1]
    return parts


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_every_variant_equals_the_reference_bit_for_bit(sd, torch_cuda, k, n):
    """the issue's table: both input kinds x both output kinds x every variant x five (B, D) x channels 1, 3, 67, steps = 5 B; then
    Dr + B further steps, whose bits come out of the decisions that the first call left in the state"""
    gens = GENS[k, n]
    rng = np.random.default_rng(100 * k + n)
    for B, D in [(32, k - 1), (32, 35), (32, 64), (64, 100), (128, 128)]:
        Dr = ref.delay(B, D)
        for channels in (1, 3, 67):
            for in_kind in IN_KINDS:
                x = _soft(sd, rng, k, gens, channels, 6 * B + Dr, in_kind)
                calls = [np.ascontiguousarray(x[:, :5 * B * n]), np.ascontiguousarray(x[:, 5 * B * n:])]
                want, want_m = _ref_run(k, gens, B, D, in_kind, channels, calls)
                assert not want[0][:, :min(Dr, 5 * B)].any() and (Dr >= 5 * B or want[0].any())
                for out_kind in OUT_KINDS:
                    for variant in _variants(k):
                        tag = (k, n, B, D, channels, in_kind, out_kind, variant)
                        bank = _bank(sd, k, gens, B, D, in_kind, out_kind, channels, variant)
                        assert bank.variant == variant and bank.delay == Dr and bank.states == 1 << (k - 1)
                        got0 = _out(bank.process(torch_cuda.from_numpy(calls[0]).cuda()), out_kind)
                        m0 = bank.metrics()
                        got1 = _out(bank.process(torch_cuda.from_numpy(calls[1]).cuda()), out_kind)
                        assert np.array_equal(got0, _want(want[0], out_kind)), (tag, "bits of the first call")
                        first = ref.ViterbiRef(k, gens, B, D, channels, in_kind=in_kind, scale=SCALE)
                        first.process(calls[0])
                        assert np.array_equal(m0, first.metrics()), (tag, "metrics after the first call")
                        assert np.array_equal(got1, _want(want[1], out_kind)), (tag, "bits out of the carried state")
                        assert np.array_equal(bank.metrics(), want_m), (tag, "final metrics")
                        bank.close()


def test_default_variant_and_info(sd, torch_cuda):
    for (k, n), gens in GENS.items():
        bank = sd.viterbi_bank(k, gens, 32, 64, max_channels=5)
        i = bank.info()
        assert i["variant"] == (0 if k == 7 else 1) and i["states"] == 1 << (k - 1) and i["delay"] == 64 and i["generators"] == gens
        assert i["kernel"] == ("sdsp_viterbi_wave_kernel" if k == 7 else "sdsp_viterbi_plain_kernel")
        assert i["chunk"] % 32 == 0 and i["chunk"] >= 32 and i["lds_bytes"] <= 160 * 1024 and i["ring_in_lds"] == 1
        W = max(1, (1 << (k - 1)) // 64)
        assert i["state_bytes"] == bank.state_bytes() == (5 * (1 << (k - 1)) * 4 + 5 * 4 + 7) // 8 * 8 + 5 * 64 * W * 8
        assert bank.launches(5, 64) == 1 and bank.launches(0, 64) == 0 and bank.launches(5, 0) == 0
        if k != 7:
            with pytest.raises(sd.SdspHipError) as e:
                bank.set_variant(0)
            assert e.value.code == sd._lib.ERR_UNSUPPORTED
        bank.close()


@pytest.mark.parametrize("k,n", [(7, 2), (7, 3), (5, 2), (9, 3)])
@pytest.mark.parametrize("in_kind", IN_KINDS)
def test_splits_and_variant_changes_between_calls(sd, torch_cuda, k, n, in_kind):
    gens = GENS[k, n]
    rng = np.random.default_rng(7 * k + n)
    for B, D in [(32, 35), (64, 100)]:
        x = _soft(sd, rng, k, gens, 5, 12 * B, in_kind)
        want, want_m = _ref_run(k, gens, B, D, in_kind, 5, [x])
        orders = [(v,) for v in _variants(k)] + ([(0, 1), (1, 0)] if k == 7 else [])
        for out_kind in OUT_KINDS:
            for blocks in [(12,), (1, 4, 7), (3, 9)]:
                for variants in orders:
                    outs, m = _run(sd, torch_cuda, k, gens, B, D, in_kind, out_kind, 5, variants, _split(x, n, B, blocks))
                    assert np.array_equal(np.concatenate(outs, axis=1), _want(want[0], out_kind)), (k, n, B, D, out_kind, blocks, variants)
                    assert np.array_equal(m, want_m), (k, n, B, D, out_kind, blocks, variants, "metrics")


@pytest.mark.parametrize("k,n,B,D,steps", [(7, 2, 32, 64, 1280 + 96), (7, 3, 32, 6, 1600), (7, 2, 128, 128, 1024), (7, 2, 1024, 4096, 6 * 1024),
                                           (5, 2, 32, 64, 2400), (9, 2, 32, 64, 352), (9, 2, 1024, 4096, 6 * 1024), (8, 3, 96, 200, 960)])
def test_calls_longer_than_a_chunk_and_the_ring_outside_lds(sd, torch_cuda, k, n, B, D, steps):
    """several chunks in one call with a shorter last one, the longest traceback, and K = 9 with it: the plain kernel's ring then lies
    in global memory"""
    gens = GENS.get((k, n), (0o371, 0o247, 0o225))
    rng = np.random.default_rng(k * B + D)
    x = _soft(sd, rng, k, gens, 3, steps, "i8")
    want, want_m = _ref_run(k, gens, B, D, "i8", 3, [x])
    assert want[0].any()
    for variant in _variants(k):
        bank = _bank(sd, k, gens, B, D, "i8", "bytes", 3, variant)
        i = bank.info()
        assert i["ring_in_lds"] == (0 if (k, D) == (9, 4096) else 1)
        assert steps > i["chunk"] or B == 1024
        got = _out(bank.process(torch_cuda.from_numpy(x).cuda()), "bytes")
        assert np.array_equal(got, want[0]), (k, n, B, D, variant, i)
        assert np.array_equal(bank.metrics(), want_m)
        bank.close()


@pytest.mark.parametrize("k,n", [(7, 2), (7, 3), (5, 3)])
def test_metrics_wrap_without_a_trace(sd, torch_cuda, k, n):
    """the metrics of a running stream plus 2^31 - 100, planted with set_metrics; strong symbols then carry them past the wrap: the
    bits are those of the unshifted stream and the metrics differ by the offset modulo 2^32"""
    gens, B, D, channels = GENS[k, n], 32, 35, 4
    rng = np.random.default_rng(k + n)
    head = _soft(sd, rng, k, gens, channels, 4 * B, "i8")
    bits = rng.integers(0, 2, (channels, 4 * B)).astype(np.uint8)
    strong = np.stack([np.where(sd.conv_encode(b, k, gens) == 1, -127, 127) for b in bits]).astype(np.int8)
    want, want_m = _ref_run(k, gens, B, D, "i8", channels, [head, strong])
    offset = (1 << 31) - 100
    for variant in _variants(k):
        plain = _bank(sd, k, gens, B, D, "i8", "bytes", channels, variant)
        moved = _bank(sd, k, gens, B, D, "i8", "bytes", channels, variant)
        for bank in (plain, moved):
            bank.process(torch_cuda.from_numpy(head).cuda())
        m = plain.metrics().astype(np.int64)
        moved.set_metrics(ref.wrap32(m + offset).astype(np.int32))
        assert np.array_equal(moved.metrics(), ref.wrap32(m + offset).astype(np.int32))
        a = _out(plain.process(torch_cuda.from_numpy(strong).cuda()), "bytes")
        b = _out(moved.process(torch_cuda.from_numpy(strong).cuda()), "bytes")
        ma, mb = plain.metrics().astype(np.int64), moved.metrics().astype(np.int64)
        assert np.array_equal(a, want[1]) and np.array_equal(ma, want_m)
        assert np.array_equal(b, a), (k, n, variant, "bits across the wrap")
        assert np.array_equal(ref.wrap32(mb - ma), np.full_like(ma, ref.wrap32(offset))), (k, n, variant)
        assert (ma.max(axis=1) > 100).all() and (mb.min(axis=1) < 0).all()  # the planted stream did pass 2^31
        plain.close()
        moved.close()


@pytest.mark.parametrize("k,n", [(7, 2), (7, 3), (3, 2), (9, 2)])
def test_special_rows(sd, torch_cuda, k, n):
    gens, B, D = GENS[k, n], 32, 35
    steps = 6 * B
    rng = np.random.default_rng(3)
    S = 1 << (k - 1)
    for variant in _variants(k):
        for out_kind in OUT_KINDS:
            # rows of one value each: erasures, both rails and -128, which is read as -127
            rows = np.stack([np.full(steps * n, v, dtype=np.int8) for v in (0, 127, -127, -128)])
            (got,), m = _run(sd, torch_cuda, k, gens, B, D, "i8", out_kind, 4, (variant,), [rows])
            (want,), want_m = _ref_run(k, gens, B, D, "i8", 4, [rows])
            assert np.array_equal(got, _want(want, out_kind)) and np.array_equal(m, want_m)
            assert not got[0].any() and not m[0].any()
            assert np.array_equal(got[2], got[3]) and np.array_equal(m[2], m[3])
            # F32: NaN is an erasure, the infinities are the rails, huge values clamp
            f = _soft(sd, rng, k, gens, 5, steps, "f32")
            f[0, :] = np.nan
            f[1, ::3] = np.inf
            f[2, 1::4] = -np.inf
            f[3, ::5] = np.nan
            f[4, ::2] = 3e38
            f[4, 1::2] = -3e38
            (got,), m = _run(sd, torch_cuda, k, gens, B, D, "f32", out_kind, 5, (variant,), [f])
            (want,), want_m = _ref_run(k, gens, B, D, "f32", 5, [f])
            assert np.array_equal(got, _want(want, out_kind)) and np.array_equal(m, want_m)
            assert not got[0].any() and not m[0].any()
        # a known start state: the encoder starts in state 0; with the first steps erased only the start metrics tell the decoder so
        bits = rng.integers(0, 2, (3, steps)).astype(np.uint8)
        x = np.stack([np.where(sd.conv_encode(b, k, gens) == 1, -60, 60) for b in bits]).astype(np.int8)
        x[:, :(k - 1) * n] = 0
        for start in (0, S - 1, -1):
            (got,), m = _run(sd, torch_cuda, k, gens, B, D, "i8", "bytes", 3, (variant,), [x], start=start)
            (want,), want_m = _ref_run(k, gens, B, D, "i8", 3, [x], start=start)
            assert np.array_equal(got, want) and np.array_equal(m, want_m), (k, n, variant, start)
            if start == 0:
                Dr = ref.delay(B, D)
                assert np.array_equal(got[:, Dr:], bits[:, :steps - Dr])


def _framed_call(sd, torch, bank, x, in_lead, out_lead, fill):
    """one call with the input and the output inside framed buffers; returns the output's interior after checking the frames"""
    channels = x.shape[0]
    steps = x.shape[1] // bank.n
    tin = torch.from_numpy(x)
    out_shape = (channels, steps // 32) if bank.out_kind == "packed" else (channels, steps)
    out_dtype = torch.int32 if bank.out_kind == "packed" else torch.uint8
    a_in, v_in = arena.framed(torch, tuple(tin.shape), tin.dtype, in_lead, 4096, arena.fills(tin.dtype)[fill])
    a_out, v_out = arena.framed(torch, out_shape, out_dtype, out_lead, 4096, arena.fills(out_dtype)[fill])
    v_in.copy_(tin)
    before_in, before_out = arena.raw(a_in).clone(), arena.raw(a_out).clone()
    bank.process_ptr(v_in.data_ptr(), v_out.data_ptr(), channels, steps, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.equal(arena.raw(a_in), before_in)), "the input was written"
    # the rows are compact, so the interior is one range of bytes (arena.bits takes no one-byte types: the bytes are compared here)
    start = v_out.data_ptr() - a_out.data_ptr()
    stop = start + v_out.numel() * v_out.element_size()
    after = arena.raw(a_out)
    changed = torch.nonzero(after != before_out).flatten()
    outside = changed[(changed < start) | (changed >= stop)]
    assert outside.numel() == 0, f"{outside.numel()} byte(s) outside the output were written, the first {int(outside[0]) - start:+d} from its start"
    return _out(v_out, bank.out_kind)


@pytest.mark.parametrize("k,n", [(7, 2), (7, 3), (5, 2)])
def test_framed_buffers_at_every_offset(sd, torch_cuda, k, n):
    """I8 rows and BYTES outputs at every byte offset 0 .. 15, F32 rows and PACKED outputs at every word offset 0 .. 3, the frames
    filled with NaN or a pattern: the interior is the clean result and nothing outside the addressed ranges is written"""
    gens, B, D, channels = GENS[k, n], 32, 35, 3
    rng = np.random.default_rng(11 + k + n)
    steps = 4 * B + (32 if n == 2 else 0)  # rows of 320 / 384 bytes: row starts at several alignments
    for in_kind in IN_KINDS:
        x = _soft(sd, rng, k, gens, channels, steps, in_kind)
        (want,), _ = _ref_run(k, gens, B, D, in_kind, channels, [x])
        for out_kind in OUT_KINDS:
            in_leads = range(16) if in_kind == "i8" else range(4)
            out_leads = range(16) if out_kind == "bytes" else range(4)
            pairs = [(a, 0) for a in in_leads] + [(0, b) for b in out_leads] + [(max(in_leads), max(out_leads))]
            for variant in _variants(k):
                bank = _bank(sd, k, gens, B, D, in_kind, out_kind, channels, variant)
                for fill in (0, 1):
                    for in_lead, out_lead in pairs:
                        bank.reset()
                        got = _framed_call(sd, torch_cuda, bank, x, in_lead, out_lead, fill)
                        assert np.array_equal(got, _want(want, out_kind)), (k, n, in_kind, out_kind, variant, in_lead, out_lead)
                bank.close()


@pytest.mark.parametrize("k,n", [(7, 2), (9, 3)])
def test_a_garbage_channel_leaves_its_neighbours_alone(sd, torch_cuda, k, n):
    gens, B, D, channels = GENS[k, n], 32, 64, 6
    rng = np.random.default_rng(21)
    for in_kind in IN_KINDS:
        x = _soft(sd, rng, k, gens, channels, 5 * B, in_kind)
        (clean,), clean_m = _ref_run(k, gens, B, D, in_kind, channels, [x])
        for bad in (0, 2, 5):
            y = x.copy()
            y[bad] = np.nan if in_kind == "f32" else rng.integers(-128, 128, y.shape[1])
            if in_kind == "f32":
                y[bad, ::2] = rng.standard_normal(y[bad, ::2].shape) * 1e30
            others = [c for c in range(channels) if c != bad]
            for variant in _variants(k):
                (got,), m = _run(sd, torch_cuda, k, gens, B, D, in_kind, "bytes", channels, (variant,), [y])
                assert np.array_equal(got[others], clean[others]) and np.array_equal(m[others], clean_m[others]), (k, n, in_kind, bad, variant)


def test_nothing_to_do_and_refusals_write_nothing(sd, torch_cuda):
    torch, L = torch_cuda, sd._lib
    lib = sd.load()
    for k, n in [(7, 2), (5, 3)]:
        gens = GENS[k, n]
        for variant in _variants(k):
            bank = _bank(sd, k, gens, 64, 100, "i8", "bytes", 4, variant)
            x = torch.from_numpy(_soft(sd, np.random.default_rng(1), k, gens, 4, 128, "i8")).cuda()
            out = torch.full((4, 128), 0x55, dtype=torch.uint8, device="cuda")
            before_m = bank.metrics()
            args = (bank._plan, x.data_ptr(), out.data_ptr())
            assert lib.sdsp_hip_viterbi_process(*args, 0, 128, None) == L.OK
            assert lib.sdsp_hip_viterbi_process(*args, 4, 0, None) == L.OK
            assert lib.sdsp_hip_viterbi_process(bank._plan, None, None, 0, 0, None) == L.OK
            for steps in (1, 32, 63, 96, 127):
                assert lib.sdsp_hip_viterbi_process(*args, 4, steps, None) == L.ERR_INVALID_SIZE
            assert lib.sdsp_hip_viterbi_process(*args, 5, 128, None) == L.ERR_INVALID_SIZE
            assert lib.sdsp_hip_viterbi_process(*args, 4, 1 << 31, None) == L.ERR_INVALID_SIZE
            assert lib.sdsp_hip_viterbi_process(bank._plan, None, out.data_ptr(), 4, 128, None) == L.ERR_INVALID_ARG
            assert lib.sdsp_hip_viterbi_process(bank._plan, x.data_ptr(), None, 4, 128, None) == L.ERR_INVALID_ARG
            assert lib.sdsp_hip_viterbi_process(bank._plan, x.data_ptr(), x.data_ptr() + 64, 4, 128, None) == L.ERR_INVALID_ARG
            assert lib.sdsp_hip_viterbi_plan_reset(bank._plan, 1 << (k - 1)) == L.ERR_INVALID_ARG
            assert lib.sdsp_hip_viterbi_plan_reset(bank._plan, -2) == L.ERR_INVALID_ARG
            assert lib.sdsp_hip_viterbi_plan_set_variant(bank._plan, 2) == L.ERR_INVALID_ARG
            torch.cuda.synchronize()
            assert bool((out == 0x55).all()) and np.array_equal(bank.metrics(), before_m)
            # and the stream is where it was: the next call gives the bits of a fresh one
            got = bank.process(x).cpu().numpy()
            (want,), _ = _ref_run(k, gens, 64, 100, "i8", 4, [x.cpu().numpy()])
            assert np.array_equal(got, want)
            bank.close()
    # misaligned pointers of the wide kinds
    bank = sd.viterbi_bank(7, GENS[7, 2], 32, 64, "f32", "packed", scale=SCALE, max_channels=2)
    x = torch.zeros(2 * 64 + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.sdsp_hip_viterbi_process(bank._plan, x.data_ptr() + 2, out.data_ptr(), 2, 32, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_process(bank._plan, x.data_ptr(), out.data_ptr() + 1, 2, 32, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_process(bank._plan, x.data_ptr() + 4, out.data_ptr() + 4, 2, 32, None) == L.OK
    torch.cuda.synchronize()
    bank.close()


@pytest.mark.parametrize("k,n", [(7, 2), (9, 3)])
def test_process_host_equals_process(sd, torch_cuda, k, n):
    gens, B, D = GENS[k, n], 32, 35
    rng = np.random.default_rng(31)
    for in_kind in IN_KINDS:
        x = _soft(sd, rng, k, gens, 3, 8 * B, in_kind)
        for out_kind in OUT_KINDS:
            for variant in _variants(k):
                dev = _bank(sd, k, gens, B, D, in_kind, out_kind, 3, variant)
                host = _bank(sd, k, gens, B, D, in_kind, out_kind, 3, variant)
                for part in _split(x, n, B, (3, 5)):
                    a = _out(dev.process(torch_cuda.from_numpy(part).cuda()), out_kind)
                    b = host.process_host(part)
                    assert a.dtype == b.dtype and np.array_equal(a, b), (k, n, in_kind, out_kind, variant)
                assert np.array_equal(dev.metrics(), host.metrics())
                dev.close()
                host.close()


def test_viterbi_decode_one_shot(sd, torch_cuda):
    """whole frames: the bits of a clean and of a noisy frame, and the documented padding (tests/viterbi_ref.py does the same by hand)"""
    rng = np.random.default_rng(41)
    for (k, n), T in [((7, 2), 100), ((7, 3), 33), ((5, 2), 1), ((9, 2), 257)]:
        gens = GENS[k, n]
        bits = rng.integers(0, 2, (4, T)).astype(np.uint8)
        coded = np.stack([sd.conv_encode(b, k, gens) for b in bits]).astype(np.float64)
        soft = np.clip(np.rint((1 - 2 * coded) * 50 + 20 * rng.standard_normal(coded.shape)), -127, 127).astype(np.int8)
        B = 32
        D = -(-5 * k // B) * B
        Dr = ref.delay(B, D)
        total = -(-T // B) * B + Dr
        padded = np.zeros((4, total * n), dtype=np.int8)
        padded[:, :T * n] = soft
        for start in (-1, 0):
            got = sd.viterbi_decode(torch_cuda.from_numpy(soft).cuda(), k, gens, start_state=start).cpu().numpy()
            want = ref.ViterbiRef(k, gens, B, D, 4, start_state=start).process(padded)[:, Dr:Dr + T]
            assert got.shape == (4, T) and np.array_equal(got, want), (k, n, T, start)
            if start == 0 or T >= 33:  # 8 dB of margin: these frames decode clean (a frame of one step only from a known start)
                assert np.array_equal(got, bits), (k, n, T, start)
        one = sd.viterbi_decode(torch_cuda.from_numpy(soft[0]).cuda(), k, gens).cpu().numpy()
        assert one.shape == (T,) and np.array_equal(one, ref.ViterbiRef(k, gens, B, D, 1).process(padded[:1])[0, Dr:Dr + T])


def test_seeded_random_cases(sd, torch_cuda):
    """drawn codes, tracebacks, shapes, kinds, start states and splits, every variant against the reference"""
    rng = np.random.default_rng(20261)
    for case in range(16):
        k = int(rng.integers(3, 10))
        n = int(rng.integers(2, 4))
        gens = tuple(int(g) for g in rng.integers(1, 1 << k, n))
        B = 32 * int(rng.integers(1, 5))
        D = int(rng.integers(k - 1, 200))
        channels = int(rng.integers(1, 9))
        in_kind, out_kind = IN_KINDS[int(rng.integers(2))], OUT_KINDS[int(rng.integers(2))]
        start = int(rng.integers(-1, 1 << (k - 1)))
        blocks = [int(b) for b in rng.integers(1, 6, int(rng.integers(1, 4)))]
        x = _soft(sd, rng, k, gens, channels, sum(blocks) * B, in_kind)
        calls = _split(x, n, B, blocks)
        want, want_m = _ref_run(k, gens, B, D, in_kind, channels, calls, start=start)
        orders = [(v,) for v in _variants(k)] + ([(0, 1)] if k == 7 else [])
        for variants in orders:
            outs, m = _run(sd, torch_cuda, k, gens, B, D, in_kind, out_kind, channels, variants, calls, start=start)
            tag = (case, k, gens, B, D, channels, in_kind, out_kind, start, blocks, variants)
            for got, w in zip(outs, want):
                assert np.array_equal(got, _want(w, out_kind)), tag
            assert np.array_equal(m, want_m), tag
