"""Host side of the Reed-Solomon decoder banks (sdsp_hip_rs_*), no device: the numpy reference
(tests/rs_ref.py) against the contract taken literally over all 65 536 codewords of four small codes, the generator and parity
anchors of the DVB and CCSDS codes, the library's host helpers against the reference, and the refusals of plan creation, whose
argument checks come before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import rs_ref as R

SMALL = [(0x187, 112, 11, 4, 6), (0x11D, 0, 1, 4, 6), (0x11D, 1, 1, 3, 5), (0x187, 112, 11, 2, 4)]
DVB_G = [1, 59, 13, 104, 189, 68, 209, 30, 8, 163, 65, 41, 229, 98, 50, 36, 59]
INVALID_SIZE, INVALID_ARG = -1, -5  # SDSP_HIP_ERR_INVALID_SIZE, SDSP_HIP_ERR_INVALID_ARG


def _lib():
    import simpledsp_amd._lib as L
    return L, L.load()


@pytest.mark.parametrize("params", SMALL)
def test_reference_equals_the_definition_by_brute_force(params):
    code = R.Code(*params)
    assert code.k == 2
    rng = np.random.default_rng(20261021 + params[3] * 16 + params[4])
    n = code.n
    seen = {"ok": 0, "fail": 0, "other": 0}
    for _ in range(1000):
        cw = code.encode(rng.integers(0, 256, (1, 2), dtype=np.uint8))[0]
        r = cw.copy()
        ne = int(rng.integers(0, n + 1))
        p = rng.permutation(n)[:ne]
        r[p] ^= rng.integers(1, 256, ne, dtype=np.uint8)
        erased = np.zeros(n, dtype=bool)
        erased[rng.permutation(n)[:int(rng.integers(0, 6))]] = True
        got, cnt = code.decode_word(r, erased)
        want, wcnt = code.brute_force(r, erased)
        assert cnt == wcnt and np.array_equal(got, want), (r, erased, got, cnt, want, wcnt)
        seen["fail" if cnt < 0 else "ok" if np.array_equal(got, cw) else "other"] += 1
    assert min(seen.values()) > 0, seen  # successes, refusals and miscorrections were all among the draws


@pytest.mark.parametrize("params,interleave", [((0x187, 112, 11, 32, 255), 5), ((0x11D, 0, 1, 16, 204), 1), ((0x11D, 1, 1, 3, 65), 2),
                                               ((0x11D, 1, 1, 64, 255), 16)])
def test_reference_encoder_gives_zero_syndromes(params, interleave):
    code = R.Code(*params)
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, (3, interleave * code.k), dtype=np.uint8)
    frames = R.encode_frames(code, data, interleave)
    assert frames.shape == (3, interleave * code.n)
    assert np.array_equal(frames[:, :interleave * code.k], data)  # systematic, in the frame's own order
    assert not R.Code.syndromes(code, R.to_words(frames, code.n, interleave)).any()
    out, cnt = R.decode_frames(code, frames, None, interleave)
    assert np.array_equal(out, frames) and not cnt.any()


def test_generator_anchors():
    assert list(R.Code(0x11D, 0, 1, 16, 204).generator()) == DVB_G
    g = R.Code(0x187, 112, 11, 32).generator()
    assert list(g[:8]) == [1, 91, 127, 86, 16, 30, 13, 235]
    assert np.array_equal(g, g[::-1]) and len(g) == 33


def test_dvb_parity_anchor():
    code = R.Code(0x11D, 0, 1, 16, 204)
    w = code.encode(np.arange(1, 189, dtype=np.uint8)[None])[0]
    assert list(w[188:192]) == [195, 231, 90, 194] and list(w[-4:]) == [1, 82, 33, 222]


def test_field_refusals_of_the_reference():
    assert R.field_tables(0x11B) is None and R.field_tables(0x11D) is not None and R.field_tables(0x187) is not None
    with pytest.raises(ValueError):
        R.Code(0x11B, 0, 1, 16)
    with pytest.raises(ValueError):
        R.Code(0x11D, 0, 3, 16)


@pytest.mark.parametrize("params", [(0x11D, 0, 1, 16), (0x187, 112, 11, 32), (0x187, 112, 11, 16), (0x11D, 1, 1, 64), (0x11D, 1, 7, 3),
                                    (0x11D, 254, 2, 2)])
def test_library_generator_equals_reference(params):
    import simpledsp_amd as sd
    assert np.array_equal(sd.rs_generator(*params), R.Code(*params, 255).generator())


@pytest.mark.parametrize("params,interleave,frames", [((0x187, 112, 11, 32, 255), 5, 3), ((0x11D, 0, 1, 16, 204), 1, 2),
                                                      ((0x11D, 1, 1, 64, 255), 16, 2), ((0x11D, 1, 1, 2, 3), 1, 4),
                                                      ((0x11D, 1, 1, 3, 65), 3, 2), ((0x187, 112, 11, 16, 255), 8, 1)])
def test_library_encoder_equals_reference(params, interleave, frames):
    import simpledsp_amd as sd
    code = R.Code(*params)
    data = np.random.default_rng(11).integers(0, 256, (frames, interleave * code.k), dtype=np.uint8)
    got = sd.rs_encode(data, *params, interleave=interleave)
    assert got.dtype == np.uint8 and np.array_equal(got, R.encode_frames(code, data, interleave))


def test_library_encoder_dvb_anchor_and_empty_call():
    import simpledsp_amd as sd
    w = sd.rs_encode(np.arange(1, 189, dtype=np.uint8), 0x11D, 0, 1, 16, 204)[0]
    assert list(w[188:192]) == [195, 231, 90, 194] and list(w[-4:]) == [1, 82, 33, 222]
    assert sd.rs_encode(np.zeros(0, dtype=np.uint8), 0x11D, 0, 1, 16, 204).shape == (0, 204)


@pytest.mark.parametrize("args,code", [
    ((0x11B, 0, 1, 16, 255, 1), INVALID_ARG),   # alpha has order 51
    ((0x1D, 0, 1, 16, 255, 1), INVALID_ARG),    # bit 8 missing
    ((0x11D, 0, 3, 16, 255, 1), INVALID_ARG),   # gcd(3, 255) = 3
    ((0x11D, 0, 1, 1, 255, 1), INVALID_SIZE),
    ((0x11D, 0, 1, 65, 255, 1), INVALID_SIZE),
    ((0x11D, 0, 1, 16, 16, 1), INVALID_SIZE),   # n = nroots
    ((0x11D, 0, 1, 16, 256, 1), INVALID_SIZE),
    ((0x11D, 255, 1, 16, 255, 1), INVALID_SIZE),
    ((0x11D, 0, 1, 16, 255, 0), INVALID_SIZE),
    ((0x11D, 0, 1, 16, 255, 17), INVALID_SIZE),
])
def test_creation_refusals_need_no_device(args, code):
    L, lib = _lib()
    h = C.c_void_p(0x1234)
    assert lib.sdsp_hip_rs_plan_create(C.byref(h), *args, L.RS_FULL, 0) == code
    assert not h.value and lib.sdsp_hip_last_error_string()


def test_unknown_kind_and_null_pointers_are_refused():
    L, lib = _lib()
    h = C.c_void_p()
    assert lib.sdsp_hip_rs_plan_create(C.byref(h), 0x11D, 0, 1, 16, 255, 1, 2, 0) == INVALID_ARG
    assert lib.sdsp_hip_rs_plan_create(None, 0x11D, 0, 1, 16, 255, 1, 0, 0) == INVALID_ARG
    assert lib.sdsp_hip_rs_generator(0x11D, 0, 1, 16, None) == INVALID_ARG
    assert lib.sdsp_hip_rs_generator(0x11B, 0, 1, 16, None) == INVALID_ARG
    d = np.zeros(223, dtype=np.uint8)
    o = np.full(255, 7, dtype=np.uint8)
    assert lib.sdsp_hip_rs_encode(0x187, 112, 11, 32, 255, 1, d.ctypes.data, 1, None) == INVALID_ARG
    assert lib.sdsp_hip_rs_encode(0x187, 112, 11, 32, 255, 17, d.ctypes.data, 1, o.ctypes.data) == INVALID_SIZE
    assert lib.sdsp_hip_rs_encode(0x187, 112, 11, 32, 255, 1, d.ctypes.data, 1 << 31, o.ctypes.data) == INVALID_SIZE
    assert (o == 7).all()
    assert lib.sdsp_hip_rs_process(None, None, None, None, None, 0, None) == INVALID_ARG
    assert lib.sdsp_hip_rs_plan_set_variant(None, 0) == INVALID_ARG
    assert lib.sdsp_hip_rs_plan_destroy(None) == 0


def test_header_declares_no_stride_for_the_rs_entries():
    from conftest import ROOT
    text = (ROOT / "include" / "sdsp_hip.h").read_text()
    start = text.index("int sdsp_hip_rs_generator")
    assert "stride" not in text[start:text.index("sdsp_hip_rs_plan_get_info", start)]
