"""CPU checks of the Viterbi decoder banks (include/sdsp_hip.h: sdsp_hip_viterbi_*): the library's encoder
against a shift-register loop, the numpy reference the GPU tests use (tests/viterbi_ref.py) against brute force over every input
sequence of a small code, its split invariance, the delay formula, the error codes that need no device, and the bit error rate of the
contract (8-bit soft values, block-aligned traceback) on the K = 7 code in Gaussian noise."""
import ctypes as C
import itertools

import numpy as np
import pytest

import simpledsp_amd as sd
from simpledsp_amd import _lib as L

import viterbi_ref as ref

CODES = [(3, (0o7, 0o5)), (5, (0o23, 0o35)), (7, (0o171, 0o133)), (9, (0o561, 0o753)), (3, (0o7, 0o5, 0o3)), (7, (0o171, 0o133, 0o165)),
         (9, (0o557, 0o663, 0o711))]


@pytest.mark.parametrize("k,gens", CODES)
def test_conv_encode_equals_a_shift_register(k, gens):
    rng = np.random.default_rng(k * 10 + len(gens))
    for nbits in (0, 1, k - 1, 97):
        bits = rng.integers(0, 2, nbits).astype(np.uint8)
        for term in (False, True):
            got = sd.conv_encode(bits, k, gens, terminate=term)
            assert got.dtype == np.uint8 and got.tolist() == ref.encode(bits, k, gens, term).tolist(), (k, gens, nbits, term)
    # the octal convention on the code everyone knows: an impulse reads the generators out, most significant bit first
    imp = sd.conv_encode([1] + [0] * (k - 1), k, gens).reshape(k, len(gens))
    for j, g in enumerate(gens):
        assert imp[:, j].tolist() == [(g >> (k - 1 - i)) & 1 for i in range(k)]
    assert sd.conv_encode([2, 0, 255], k, gens).tolist() == sd.conv_encode([1, 0, 1], k, gens).tolist()  # non-zero counts as 1


def _correlation(x, q, k, gens):
    """the path metric of input sequence x from state 0 on the soft values q (steps, n)"""
    c = ref.encode(x, k, gens).reshape(-1, len(gens)).astype(np.int64)
    return int(np.where(c == 1, -q[:len(x)], q[:len(x)]).sum())


@pytest.mark.parametrize("gens", [(0o7, 0o5), (0o7, 0o5, 0o3), (0o6, 0o3)])
@pytest.mark.parametrize("T", [1, 2, 5, 12])
def test_reference_reaches_the_brute_force_maximum(gens, T):
    """K = 3, a known start state 0, every one of the 2^T input sequences: the decoded sequence has the largest correlation there is
    (metrics are compared, not sequences: small soft values tie often).  depth = 32 >= T and the frame is followed by erasures."""
    k, n, B, D = 3, len(gens), 32, 32
    rng = np.random.default_rng(1000 * T + n + gens[0])
    for trial in range(6):
        lim = (2, 5, 127)[trial % 3]
        q = rng.integers(-lim, lim + 1, (T, n)).astype(np.int8)
        if trial == 4:
            q[rng.integers(0, T)] = 0  # an erased step
        soft = np.zeros((1, (B + ref.delay(B, D)) * n), dtype=np.int8)
        soft[0, :T * n] = q.reshape(-1)
        dec = ref.ViterbiRef(k, gens, B, D, 1, start_state=0)
        bits = dec.process(soft)[0, ref.delay(B, D):][:T]
        best = max(_correlation(x, q.astype(np.int64), k, gens) for x in itertools.product((0, 1), repeat=T))
        assert _correlation(bits.tolist(), q.astype(np.int64), k, gens) == best, (gens, T, trial)
        # the largest metric at the end is that maximum too
        assert int(dec.metrics().max()) == best


def test_reference_decodes_a_clean_frame_and_pads_with_zeros():
    k, gens, B, D = 7, (0o171, 0o133), 32, 64
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, (3, 160)).astype(np.uint8)
    soft = np.stack([np.where(ref.encode(b, k, gens) == 1, -90, 90) for b in bits]).astype(np.int8)
    soft = np.concatenate([soft, np.zeros((3, ref.delay(B, D) * 2), dtype=np.int8)], axis=1)
    out = ref.ViterbiRef(k, gens, B, D, 3).process(soft)
    assert not out[:, :64].any()  # the first Dr outputs of a stream
    assert np.array_equal(out[:, 64:64 + 160], bits)


@pytest.mark.parametrize("k,gens", CODES)
def test_reference_split_invariance(k, gens):
    n, B, D = len(gens), 32, 40
    rng = np.random.default_rng(k + n)
    soft = rng.integers(-128, 128, (4, 12 * B * n)).astype(np.int8)
    whole = ref.ViterbiRef(k, gens, B, D, 4)
    want = whole.process(soft)
    for split in ((1, 4, 7), (3, 9), (1,) * 12):
        dec = ref.ViterbiRef(k, gens, B, D, 4)
        t, parts = 0, []
        for blocks in split:
            parts.append(dec.process(soft[:, t * n:(t + blocks * B) * n]))
            t += blocks * B
        assert np.array_equal(np.concatenate(parts, axis=1), want), split
        assert np.array_equal(dec.metrics(), whole.metrics()) and np.array_equal(dec.dec, whole.dec)


def test_reference_quantiser():
    x = np.array([0.0, 0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 3.49], dtype=np.float32)
    assert ref.quantise(x, "f32", 1.0).tolist() == [0, 0, 2, 2, 0, -2, 126, 127, 127, -127, 127, -127, 0, 3]
    assert ref.quantise(np.array([-128, -127, 127, 0], dtype=np.int8)).tolist() == [-127, -127, 127, 0]
    assert ref.quantise(np.array([1.0], dtype=np.float32), "f32", 32.0).tolist() == [32]


def test_delay_formula():
    for block in (32, 64, 96, 1024):
        for depth in (1, 6, block - 1, block, block + 1, 100, 4096):
            want = block * -(-depth // block)
            assert sd.viterbi_delay(block, depth) == want == ref.delay(block, depth)
            assert depth <= want < depth + block and want % block == 0
    lib, d = sd.load(), C.c_uint32(7)
    for block, depth in ((0, 8), (16, 8), (48, 8), (1056, 8), (33, 8), (32, 0), (32, 4097)):
        assert lib.sdsp_hip_viterbi_delay(block, depth, C.byref(d)) == L.ERR_INVALID_SIZE, (block, depth)
    assert lib.sdsp_hip_viterbi_delay(32, 8, None) == L.ERR_INVALID_ARG
    assert d.value == 7


def _create(k=7, gens=(0o171, 0o133), block=32, depth=64, in_kind=L.VITERBI_I8, out_kind=L.VITERBI_BYTES, scale=1.0, max_channels=4,
            out=True, null_gens=False):
    h = C.c_void_p()
    g = (C.c_uint32 * len(gens))(*gens)
    rc = sd.load().sdsp_hip_viterbi_plan_create(C.byref(h) if out else None, k, len(gens), None if null_gens else g, block, depth, in_kind,
                                                out_kind, scale, max_channels, 0)
    if rc == L.OK:
        sd.load().sdsp_hip_viterbi_plan_destroy(h)
    return rc


def test_error_codes_without_a_device():
    ok = (L.OK, L.ERR_NO_DEVICE)  # whatever machine this runs on, an argument error is never one of these
    assert _create() in ok
    assert _create(out=False) == L.ERR_INVALID_ARG
    assert _create(null_gens=True) == L.ERR_INVALID_ARG
    for k in (0, 2, 10):
        assert _create(k=k, gens=(1, 1)) == L.ERR_INVALID_SIZE
    for gens in ((0o171,), (1, 1, 1, 1)):
        assert _create(gens=gens) == L.ERR_INVALID_SIZE
    for gens in ((0, 0o133), (0o171, 128), (0o171, 0o133, 1 << 20)):
        assert _create(gens=gens) == L.ERR_INVALID_ARG
    for block in (0, 16, 33, 48, 1056):
        assert _create(block=block) == L.ERR_INVALID_SIZE
    for depth in (0, 5, 4097):
        assert _create(depth=depth) == L.ERR_INVALID_SIZE
    assert _create(depth=6) in ok
    for mc in (0, 1 << 31):
        assert _create(max_channels=mc) == L.ERR_INVALID_SIZE
    for kind in (-1, 2):
        assert _create(in_kind=kind) == L.ERR_INVALID_ARG
        assert _create(out_kind=kind) == L.ERR_INVALID_ARG
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert _create(in_kind=L.VITERBI_F32, scale=scale) == L.ERR_INVALID_ARG
        assert _create(in_kind=L.VITERBI_I8, scale=scale) in ok  # I8 plans do not read it
    lib = sd.load()
    assert lib.sdsp_hip_viterbi_process(None, None, None, 1, 32, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_process_host(None, None, None, 1, 32) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_plan_reset(None, -1) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_plan_set_variant(None, 0) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_plan_get_info(None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_plan_state_bytes(None, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_plan_get_metrics(None, None, 1) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_plan_set_metrics(None, None, 1) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_plan_launches(None, 1, 32, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_viterbi_plan_destroy(None) == L.OK
    g = (C.c_uint32 * 2)(0o7, 0o5)
    out = np.zeros(8, dtype=np.uint8)
    assert lib.sdsp_hip_conv_encode(3, 2, g, None, 2, 0, out.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_conv_encode(3, 2, g, out.ctypes.data, 2, 0, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_conv_encode(3, 2, None, out.ctypes.data, 2, 0, out.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_conv_encode(2, 2, g, out.ctypes.data, 2, 0, out.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_conv_encode(3, 4, g, out.ctypes.data, 2, 0, out.ctypes.data) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_conv_encode(3, 2, (C.c_uint32 * 2)(8, 5), out.ctypes.data, 2, 0, out.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_conv_encode(3, 2, g, None, 0, 0, None) == L.OK


def test_python_surface_checks_its_arguments():
    with pytest.raises(ValueError):
        sd.viterbi_bank(7, (0o171, 0o133), in_kind="i16")
    with pytest.raises(ValueError):
        sd.viterbi_bank(7, (0o171,))
    with pytest.raises(ValueError):
        sd.conv_encode([1, 0], 7, (1, 2, 3, 4))
    with pytest.raises(sd.SdspHipError) as e:
        sd.conv_encode([1, 0], 7, (0, 0o133))
    assert e.value.code == L.ERR_INVALID_ARG


def test_bit_error_rate_of_the_contract_at_4_db():
    """K = 7 (171, 133), BPSK in Gaussian noise at Eb/N0 = 4 dB, quantiser scale 32, (B, D) = (32, 64), 48 channels x 4096 steps on the
    reference.  A numpy prototype of the contract gave 1 to 8 errors in about 1.97e5 bits here (and none at 5 dB); the cap of 2e-4 is
    about five times the worst count seen."""
    k, gens, B, D, channels, steps = 7, (0o171, 0o133), 32, 64, 48, 4096
    rng = np.random.default_rng(20260)
    bits = rng.integers(0, 2, (channels, steps)).astype(np.uint8)
    coded = np.stack([ref.encode(b, k, gens) for b in bits]).astype(np.float64)
    ebn0 = 10.0 ** (4.0 / 10.0)
    sigma = np.sqrt(1.0 / (2.0 * 0.5 * ebn0))  # unit symbol energy at rate 1/2: Es / N0 = Eb / N0 / 2
    x = ((1.0 - 2.0 * coded) + sigma * rng.standard_normal(coded.shape)).astype(np.float32)
    out = ref.ViterbiRef(k, gens, B, D, channels, in_kind="f32", scale=32.0).process(x)
    Dr = ref.delay(B, D)
    compared = channels * (steps - Dr)
    errors = int((out[:, Dr:] != bits[:, :steps - Dr]).sum())
    print(f"viterbi reference BER at 4 dB: {errors} errors in {compared} bits = {errors / compared:.3e} (cap 2e-4)")
    assert compared > 1.9e5
    assert errors / compared <= 2e-4
