"""GPU tests of the LDPC decoder banks (sdsp_hip_ldpc_*) on a real MI355X.

The checker is tests/ldpc_ref.py, the contract in numpy, itself held to a second reading of the contract in
tests/test_ldpc_host.py.  Everything is on integers, so both kernel variants are held to the reference bit for bit: the hard bits in
both layouts, the posteriors and the status, with no tolerance anywhere.  Codewords are independent, so the reference of a call of
67 codewords is also that of its first one and its first three."""
import functools

import numpy as np
import pytest

import arena
import ldpc_ref as R

pytestmark = pytest.mark.gpu

INVALID_SIZE, INVALID_ARG = -1, -5
CODEWORDS = (1, 3, 67)
ITERS = (0, 1, 2, 20)
SCALE = 8.0


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


def degree32_base():
    """2 x 34: a row of 32 entries over a row of three"""
    B = -np.ones((2, 34), dtype=np.int16)
    B[0, :32] = np.arange(32) % 5
    B[1, 31:] = [1, 0, 0]
    B[0, 32] = -1
    B[1, 0] = 2
    return B


@functools.lru_cache(maxsize=None)
def _code(shape, z):
    """shape: (mb, nb) from the generator, or "d32"; returns (base, reference code)"""
    base = degree32_base() % z if shape == "d32" else R.generate(shape[0], shape[1], z, 7 * z + shape[0])
    if shape == "d32":
        base[degree32_base() < 0] = -1
    return base, R.Code(base, z)


def _sent(code, rng, cw):
    """codewords of any code: of the staircase codes by their encoder, of the others the all-zero word"""
    try:
        words = R.encode_staircase(code, rng.integers(0, 2, (cw, code.k)))
        if not code.syndrome(words).any():
            return words
    except Exception:
        pass
    return np.zeros((cw, code.n), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _received(shape, z, cw=67, seed=0):
    """float32 samples of `cw` codewords at a mix of noise levels: clean ones, decodable ones and hopeless ones"""
    _, code = _code(shape, z)
    rng = np.random.default_rng(1000 * z + seed)
    words = _sent(code, rng, cw)
    sigma = np.array([0.0, 0.55, 0.75, 1.0, 3.0])[rng.integers(0, 5, cw)]
    sigma[:3] = [0.75, 0.0, 3.0]
    y = (1.0 - 2.0 * words) + sigma[:, None] * rng.standard_normal((cw, code.n))
    return y.astype(np.float32)


def _inputs(shape, z, kind, cw=67, seed=0):
    """(what the decoder is given, what the reference is given)"""
    y = _received(shape, z, cw, seed)
    if kind == "f32":
        return y, R.quantise_f32(y, SCALE)
    raw = np.clip(np.rint(y * SCALE), -128, 127).astype(np.int8)  # -128 stays among them: the decoder reads it as -127
    return raw, R.quantise_i8(raw)


@functools.lru_cache(maxsize=None)
def _want(shape, z, kind, early, max_iter, norm=12, beta=0, cw=67, seed=0):
    _, code = _code(shape, z)
    return R.decode(code, _inputs(shape, z, kind, cw, seed)[1], max_iter, norm, beta, early)


def _device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bits_of(out_kind, bits, out_bits):
    """the expected `bits` output in the decoder's layout"""
    b = bits[:, :out_bits]
    return R.pack_bits(b).view(np.int32) if out_kind == "packed" else b


def _run(torch, dec, x, cw, max_iter):
    bits, post, status = dec.process(_device(torch, x[:cw]), max_iter)
    torch.cuda.synchronize()
    return bits.cpu().numpy(), post.cpu().numpy(), status.cpu().numpy()


def _assert_equal(got, want, out_kind, out_bits, tag):
    bits, post, status = got
    wb, wp, ws = want
    cw = len(status)
    assert np.array_equal(status, ws[:cw]), (tag, status[:8], ws[:8])
    assert np.array_equal(post, wp[:cw]), tag
    assert np.array_equal(bits, _bits_of(out_kind, wb[:cw], out_bits)), tag


GRID = ([((3, 6), z) for z in (2, 5, 21, 27, 32, 33, 64, 65, 81, 130, 512)] + [((4, 24), z) for z in (5, 27, 81)] +
        [((12, 24), z) for z in (2, 21, 32, 33, 65, 130)] + [("d32", 5), ("d32", 64)])


@pytest.mark.parametrize("shape,z", GRID)
def test_both_variants_equal_the_reference(torch_cuda, sd, shape, z):
    torch = torch_cuda
    base, code = _code(shape, z)
    if shape == (4, 24):
        assert max(code.degree) >= 18  # 20 information columns of three entries over four rows, and the staircase
    if shape == "d32":
        assert max(code.degree) == 32
    turn = 0
    seen = set()
    for kind in ("i8", "f32"):
        x, _ = _inputs(shape, z, kind)
        for early in (True, False):
            decs = {}
            for out_kind in ("bytes", "packed"):
                out_bits = code.n if out_kind == "bytes" else max(1, code.n - 3)
                decs[out_kind] = (sd.ldpc_decoder(base, z, 12, 0, early, kind, SCALE, out_kind, out_bits), out_bits)
            for max_iter in ITERS:
                want = _want(shape, z, kind, early, max_iter)
                seen.update(np.sign(want[2]).tolist() if early and max_iter == 20 else [])
                for cw in CODEWORDS:
                    out_kind = ("bytes", "packed")[turn % 2]
                    turn += 1
                    dec, out_bits = decs[out_kind]
                    for variant in (0, 1):
                        dec.set_variant(variant)
                        assert dec.launches(cw) == 1
                        _assert_equal(_run(torch, dec, x, cw, max_iter), want, out_kind, out_bits,
                                      (shape, z, kind, early, max_iter, cw, out_kind, variant))
            for dec, _ in decs.values():
                dec.close()
    if code.n >= 100 and shape != "d32":
        assert seen == {-1, 0, 1}, seen  # passes at once, passes after some iterations and failures within one call


def test_plan_info_reports_the_packing(sd):
    for z, group in ((2, 32), (5, 12), (21, 3), (27, 2), (32, 2), (33, 1), (64, 1), (65, 1), (512, 1)):
        base, code = _code((3, 6), z)
        dec = sd.ldpc_decoder(base, z)
        i = dec.info()
        assert (i["group"], i["n"], i["m"], i["edges"], i["max_row_degree"]) == (group, code.n, code.m, code.edges, max(code.degree))
        assert i["kernel"] == "sdsp_ldpc_wave_kernel" and i["variant"] == 0 and i["threads"] % 64 == 0
        assert i["lds_bytes"] >= (i["threads"] // 64) * group * (2 * code.n + 8 * code.m) and i["lds_bytes"] <= 160 * 1024
        assert i["codewords_per_cu"] >= group
        dec.set_variant(1)
        i = dec.info()
        assert i["kernel"] == "sdsp_ldpc_plain_kernel" and i["workspace_bytes"] <= 256 << 20 and i["piece"] >= 64
        assert i["workspace_bytes"] == i["piece"] * (2 * code.n + code.edges)
        dec.close()


@pytest.mark.parametrize("shape,z", [((12, 24), 27), ((3, 6), 65)])
def test_special_values(torch_cuda, sd, shape, z):
    torch = torch_cuda
    base, code = _code(shape, z)
    rng = np.random.default_rng(z)
    words = _sent(code, rng, 8)
    y = ((1.0 - 2.0 * words) + 0.6 * rng.standard_normal(words.shape)).astype(np.float32)
    y[0] = 0.0                                   # an all-zero input
    y[1, :2 * z] = 0.0                           # two erased block columns, as punctured columns are fed
    y[2, code.k:code.k + z] = 0.0                # an erased parity column
    y[3] = np.where(words[3] > 0, -1e3, 1e3)     # the rails
    y[4, ::7] = 1e3
    y[4, 3::11] = -1e3
    f = y.copy()
    f[5, ::5] = np.nan
    f[6, 1::9] = np.inf
    f[6, 2::9] = -np.inf
    f[7, :] = np.nan
    i8 = np.clip(np.rint(y * SCALE), -128, 127).astype(np.int8)
    i8[5, ::5] = -128
    i8[6] = -128
    for kind, x, q in (("f32", f, R.quantise_f32(f, SCALE)), ("i8", i8, R.quantise_i8(i8))):
        assert (q[1, :2 * z] == 0).all() and abs(q).max() == 127
        for early in (True, False):
            want = R.decode(code, q, 10, 12, 0, early)
            dec = sd.ldpc_decoder(base, z, 12, 0, early, kind, SCALE)
            for variant in (0, 1):
                dec.set_variant(variant)
                _assert_equal(_run(torch, dec, x, 8, 10), want, "bytes", code.n, (kind, early, variant))
            dec.close()


@pytest.mark.parametrize("z,where", [(5, 5), (27, 1), (27, 0)])
def test_a_garbage_codeword_changes_only_its_own_outputs(torch_cuda, sd, z, where):
    torch = torch_cuda
    base, code = _code((12, 24), z)
    rng = np.random.default_rng(z + where)
    cw = 2 * (64 // z) + 1
    words = _sent(code, rng, cw)
    clean = np.clip(np.rint(SCALE * ((1.0 - 2.0 * words) + 0.5 * rng.standard_normal(words.shape))), -127, 127).astype(np.int8)
    dirty = clean.copy()
    dirty[where] = rng.integers(-127, 128, code.n)
    wc, wd = (R.decode(code, R.quantise_i8(a), 12, 12, 0, True) for a in (clean, dirty))
    assert wd[2][where] == -1 and (np.delete(wc[2], where) >= 0).all()  # it never converges; its neighbours do
    dec = sd.ldpc_decoder(base, z, 12, 0, True)
    for variant in (0, 1):
        dec.set_variant(variant)
        gc, gd = _run(torch, dec, clean, cw, 12), _run(torch, dec, dirty, cw, 12)
        _assert_equal(gc, wc, "bytes", code.n, ("clean", variant))
        _assert_equal(gd, wd, "bytes", code.n, ("dirty", variant))
        for a, b in zip(gc, gd):
            assert np.array_equal(np.delete(a, where, axis=0), np.delete(b, where, axis=0))
    dec.close()


@pytest.mark.parametrize("kind,out_kind", [("i8", "bytes"), ("f32", "packed")])
def test_framed_buffers_at_every_offset(torch_cuda, sd, kind, out_kind):
    torch = torch_cuda
    shape, z, cw = (3, 6), 27, 3  # two codewords per wave: a full wave and a ragged one
    base, code = _code(shape, z)
    out_bits = code.n - 5
    x, _ = _inputs(shape, z, kind)
    want = _want(shape, z, kind, True, 20)
    dec = sd.ldpc_decoder(base, z, 12, 0, True, kind, SCALE, out_kind, out_bits)
    tin, tbits = (torch.float32 if kind == "f32" else torch.int8), (torch.int32 if out_kind == "packed" else torch.uint8)
    margin = 256
    for variant in (0, 1):
        dec.set_variant(variant)
        for lead in range(16):
            leads = (lead % (4 if kind == "f32" else 16), (lead * 5 + 1) % (4 if out_kind == "packed" else 16), (lead * 3 + 1) % 8, lead % 4)
            a_in, v_in = arena.framed(torch, (cw, code.n), tin, leads[0], margin, 0x55 if kind == "i8" else 7.0)
            a_bits, v_bits = arena.framed(torch, (cw, dec.bits_row), tbits, leads[1], margin, 0x55)
            a_post, v_post = arena.framed(torch, (cw, code.n), torch.int16, leads[2], margin, 0x55)
            a_st, v_st = arena.framed(torch, (cw,), torch.int32, leads[3], margin, 0x55)
            v_in.copy_(_device(torch, x[:cw]))
            arenas, views = (a_in, a_bits, a_post, a_st), (v_in, v_bits, v_post, v_st)
            before = [a.clone() for a in arenas]
            dec.process(v_in, 20, bits=v_bits.view(-1), post=v_post.view(-1), status=v_st)
            torch.cuda.synchronize()
            _assert_equal((v_bits.cpu().numpy(), v_post.cpu().numpy(), v_st.cpu().numpy()), want, out_kind, out_bits, (variant, lead))
            assert torch.equal(a_in, before[0]), (variant, lead)
            for a, b, v in zip(arenas[1:], before[1:], views[1:]):
                start = (v.data_ptr() - a.data_ptr()) // a.element_size()
                assert torch.equal(a[:start], b[:start]) and torch.equal(a[start + v.numel():], b[start + v.numel():]), (variant, lead)
    dec.close()


def test_every_subset_of_the_outputs_and_every_out_bits(torch_cuda, sd):
    torch = torch_cuda
    shape, z, cw = (3, 6), 21, 7
    base, code = _code(shape, z)
    x, _ = _inputs(shape, z, "i8")
    want = _want(shape, z, "i8", True, 20)
    src = _device(torch, x[:cw])
    for out_kind in ("bytes", "packed"):
        for out_bits in (1, code.k, code.n, 45):
            dec = sd.ldpc_decoder(base, z, 12, 0, True, "i8", 1.0, out_kind, out_bits)
            for variant in (0, 1):
                dec.set_variant(variant)
                for mask in range(1, 8):
                    keep = [None if mask >> b & 1 else False for b in range(3)]
                    bits, post, status = dec.process(src, 20, bits=keep[0], post=keep[1], status=keep[2])
                    torch.cuda.synchronize()
                    assert [t is None for t in (bits, post, status)] == [k is False for k in keep]
                    if bits is not None:
                        assert np.array_equal(bits.cpu().numpy(), _bits_of(out_kind, want[0][:cw], out_bits)), (out_kind, out_bits, variant, mask)
                    if post is not None:
                        assert np.array_equal(post.cpu().numpy(), want[1][:cw])
                    if status is not None:
                        assert np.array_equal(status.cpu().numpy(), want[2][:cw])
            dec.close()


def test_host_calls_one_shot_stream_and_variant_switch(torch_cuda, sd):
    torch = torch_cuda
    shape, z, cw = (12, 24), 33, 9
    base, code = _code(shape, z)
    for kind in ("i8", "f32"):
        x, _ = _inputs(shape, z, kind)
        want = _want(shape, z, kind, True, 20)
        dec = sd.ldpc_decoder(base, z, 12, 0, True, kind, SCALE, "packed", code.k)
        got = dec.process_host(x[:cw], 20)
        assert got[0].dtype == np.uint32
        _assert_equal((got[0].view(np.int32), got[1], got[2]), want, "packed", code.k, "process_host")
        dec.set_variant(1)  # between two calls
        got = dec.process_host(x[:cw], 20)
        _assert_equal((got[0].view(np.int32), got[1], got[2]), want, "packed", code.k, "process_host, variant 1")
        dec.set_variant(0)
        src = _device(torch, x[:cw])
        bits = torch.zeros((cw, dec.bits_row), dtype=torch.int32, device="cuda")
        post = torch.zeros((cw, code.n), dtype=torch.int16, device="cuda")
        status = torch.zeros(cw, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        dec.process_ptr(src.data_ptr(), bits.data_ptr(), post.data_ptr(), status.data_ptr(), cw, 20, s.cuda_stream)
        s.synchronize()
        _assert_equal((bits.cpu().numpy(), post.cpu().numpy(), status.cpu().numpy()), want, "packed", code.k, "process_ptr")
        dec.close()
        got = sd.ldpc_decode(x[:cw], base, z, 20, scale=SCALE)
        _assert_equal(got, want, "bytes", code.n, "ldpc_decode, numpy")
        got = sd.ldpc_decode(src, base, z, 20, scale=SCALE)
        _assert_equal(tuple(t.cpu().numpy() for t in got), want, "bytes", code.n, "ldpc_decode, tensor")
    empty = sd.ldpc_decoder(base, z)
    bits, post, status = empty.process(torch.zeros((0, code.n), dtype=torch.int8, device="cuda"), 5)
    assert bits.numel() == 0 and post.numel() == 0 and status.numel() == 0 and empty.launches(0) == 0
    empty.close()


def test_a_call_of_several_pieces_in_variant_1(torch_cuda, sd):
    torch = torch_cuda
    shape, z = (3, 6), 2
    base, code = _code(shape, z)
    dec = sd.ldpc_decoder(base, z, 12, 0, True)
    dec.set_variant(1)
    piece = dec.info()["piece"]
    cw = piece + 70
    assert dec.launches(cw) == 2 and dec.launches(piece) == 1
    rng = np.random.default_rng(2)
    x = np.clip(np.rint(SCALE * (1.0 + 0.9 * rng.standard_normal((cw, code.n)))), -128, 127).astype(np.int8)
    want = R.decode(code, R.quantise_i8(x), 3, 12, 0, True)
    got1 = _run(torch, dec, x, cw, 3)
    _assert_equal(got1, want, "bytes", code.n, "two pieces")
    dec.set_variant(0)
    _assert_equal(_run(torch, dec, x, cw, 3), want, "bytes", code.n, "one launch")
    dec.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_stream_capture_and_one_replay(torch_cuda, sd, variant):
    torch = torch_cuda
    shape, z, cw = (12, 24), 27, 5
    base, code = _code(shape, z)
    x, _ = _inputs(shape, z, "i8")
    want = _want(shape, z, "i8", True, 20)
    dec = sd.ldpc_decoder(base, z, 12, 0, True)
    dec.set_variant(variant)
    src = _device(torch, x[:cw])
    bits = torch.zeros((cw, code.n), dtype=torch.uint8, device="cuda")
    post = torch.zeros((cw, code.n), dtype=torch.int16, device="cuda")
    status = torch.full((cw,), 77, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.process_ptr(src.data_ptr(), bits.data_ptr(), post.data_ptr(), status.data_ptr(), cw, 20, s.cuda_stream)
    assert (status == 77).all()  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    _assert_equal((bits.cpu().numpy(), post.cpu().numpy(), status.cpu().numpy()), want, "bytes", code.n, "replay")
    direct = _run(torch, dec, x, cw, 20)
    _assert_equal(direct, want, "bytes", code.n, "direct")
    dec.close()


def test_refusals_write_nothing(torch_cuda, sd):
    torch = torch_cuda
    shape, z, cw = (3, 6), 5, 4
    base, code = _code(shape, z)
    n = code.n
    for kind, out_kind in (("i8", "bytes"), ("f32", "packed")):
        dec = sd.ldpc_decoder(base, z, 12, 0, True, kind, SCALE, out_kind)
        esz = 4 if kind == "f32" else 1
        buf = torch.full((4096,), 0x55, dtype=torch.uint8, device="cuda")
        before = buf.clone()
        p = buf.data_ptr()
        llr, bits, post, status = p, p + 1024, p + 2048, p + 3072
        in_bytes, bits_bytes = cw * n * esz, cw * dec.bits_row * (4 if out_kind == "packed" else 1)

        def rc(*args):
            try:
                dec.process_ptr(*args)
            except sd.SdspHipError as e:
                return e.code
            return 0

        assert rc(llr, bits, post, status, cw, 256) == INVALID_SIZE
        assert rc(llr, bits, post, status, 1 << 31, 5) == INVALID_SIZE
        assert rc(llr, None, None, None, cw, 5) == INVALID_ARG          # no output at all
        assert rc(None, bits, post, status, cw, 5) == INVALID_ARG
        assert rc(llr, bits, post + 1, status, cw, 5) == INVALID_ARG      # misaligned
        assert rc(llr, bits, post, status + 2, cw, 5) == INVALID_ARG
        if kind == "f32":
            assert rc(llr + 2, bits, post, status, cw, 5) == INVALID_ARG
            assert rc(llr, bits + 2, post, status, cw, 5) == INVALID_ARG
        assert rc(llr, llr + in_bytes - 4, None, None, cw, 5) == INVALID_ARG  # bits in the input's last bytes
        assert rc(llr, None, llr + in_bytes - 2, None, cw, 5) == INVALID_ARG
        assert rc(llr, None, None, llr, cw, 5) == INVALID_ARG
        assert rc(llr, bits, bits + bits_bytes - 4, None, cw, 5) == INVALID_ARG
        assert rc(llr, bits, None, bits, cw, 5) == INVALID_ARG
        assert rc(llr, None, post, post + 2 * cw * n - 4, cw, 5) == INVALID_ARG
        assert rc(None, None, None, None, 0, 5) == 0                     # nothing to do
        torch.cuda.synchronize()
        assert torch.equal(buf, before)
        with pytest.raises(ValueError):
            dec.set_variant(2)
        dec.close()


def _random_case(seed):
    rng = np.random.default_rng(seed)
    while True:
        z = int(rng.choice([2, 3, 7, 16, 31, 32, 33, 48, 63, 64, 65, 96, 128, 129, 200]))
        mb = int(rng.integers(1, 9))
        nb = mb + int(rng.integers(1, 4 * mb + 2))
        base = R.generate(mb, nb, z, seed)
        if nb * z <= 16384 and ((base >= 0).sum(axis=1) <= 32).all() and ((base >= 0).sum(axis=1) >= 2).all():
            break
    code = R.Code(base, z)
    p = dict(norm=int(rng.integers(1, 17)), beta=int(rng.integers(0, 4)), early=bool(rng.integers(0, 2)),
             kind=("i8", "f32")[int(rng.integers(0, 2))], out_kind=("bytes", "packed")[int(rng.integers(0, 2))],
             out_bits=int(rng.integers(1, code.n + 1)), cw=int(rng.integers(1, 80)), max_iter=int(rng.integers(0, 12)),
             scale=float(rng.choice([1.0, 4.0, 8.0, 11.5])))
    words = _sent(code, rng, p["cw"])
    sigma = rng.choice([0.0, 0.5, 0.8, 2.0], p["cw"])
    y = ((1.0 - 2.0 * words) + sigma[:, None] * rng.standard_normal(words.shape)).astype(np.float32)
    if p["kind"] == "f32":
        return base, code, p, y, R.quantise_f32(y, p["scale"])
    x = np.clip(np.rint(y * 16), -128, 127).astype(np.int8)
    return base, code, p, x, R.quantise_i8(x)


@pytest.mark.parametrize("seed", range(16))
def test_seeded_random_cases(torch_cuda, sd, seed):
    torch = torch_cuda
    base, code, p, x, q = _random_case(seed)
    want = R.decode(code, q, p["max_iter"], p["norm"], p["beta"], p["early"])
    dec = sd.ldpc_decoder(base, code.z, p["norm"], p["beta"], p["early"], p["kind"], p["scale"], p["out_kind"], p["out_bits"])
    for variant in (0, 1):
        dec.set_variant(variant)
        _assert_equal(_run(torch, dec, x, p["cw"], p["max_iter"]), want, p["out_kind"], p["out_bits"], (seed, p, variant))
    dec.close()


def test_the_chain_from_encoder_to_decoder_at_4_db(torch_cuda, sd):
    torch = torch_cuda
    z = 32
    base = R.generate(12, 24, z, 1)
    code = R.Code(base, z)
    rng = np.random.default_rng(4)
    data = rng.integers(0, 2, (200, code.k), dtype=np.uint8)
    words = sd.ldpc_encode(data, base, z)
    assert not code.syndrome(words).any()
    sigma = np.sqrt(1.0 / (2 * 0.5 * 10 ** 0.4))
    y = ((1.0 - 2.0 * words) + sigma * rng.standard_normal(words.shape)).astype(np.float32)
    q = R.quantise_f32(y, SCALE)
    fdec = sd.ldpc_decoder(base, z, 13, 0, True, "f32", SCALE, "bytes", code.k)
    idec = sd.ldpc_decoder(base, z, 13, 0, True, "i8", 1.0, "bytes", code.k)
    want = R.decode(code, q, 30, 13, 0, True)
    for variant in (0, 1):
        fdec.set_variant(variant)
        idec.set_variant(variant)
        gf = _run(torch, fdec, y, 200, 30)
        gi = _run(torch, idec, q.astype(np.int8), 200, 30)
        assert all(np.array_equal(a, b) for a, b in zip(gf, gi))
        _assert_equal(gf, want, "bytes", code.k, variant)
        assert (gf[0] == data).all(axis=1).sum() >= 198
    fdec.close()
    idec.close()
