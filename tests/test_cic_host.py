"""CPU tests of the CIC decimator bank (sdsp_hip_cic_*): tests/cic_ref.py, the numpy reference of the
contract, against a serial Hogenauer loop in Python integers and against the big-integer FIR form; the library's host helpers
against Python integers; the register-width rule; every plan-creation error, then ERR_NO_DEVICE without a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from cic_ref import (SHAPES, cic_ref, fir_exact, growth, hogenauer_serial, out_samples, reg_bits, splits, stream_ref, taps_exact,
                     unity_scale, wrap)
from conftest import ROOT

import simpledsp_amd as sd
from simpledsp_amd import _lib as L


def _dtype(in_bits):
    return np.int32 if in_bits > 16 else np.int16


def _length(N, R, M):
    """a few histories, and never a multiple of R"""
    return 3 * N * M * R + R + 1


def _rows(rng, N, R, M, in_bits):
    """three rows of full-range samples: random, the constant minimum (the worst case of the growth bound), the constant maximum"""
    S = _length(N, R, M)
    lo, hi = -(1 << (in_bits - 1)), (1 << (in_bits - 1)) - 1
    x = np.empty((3, S), dtype=_dtype(in_bits))
    x[0] = rng.integers(lo, hi + 1, S)
    x[1] = lo
    x[2] = hi
    return x


@pytest.mark.parametrize("N,R,M,in_bits", SHAPES)
def test_reference_against_the_serial_form_and_the_exact_fir_form(N, R, M, in_bits):
    """W = in_bits + growth bits exactly are enough: the serial form wrapped to that width, sign-extended, is the unbounded FIR form,
    also on the constant-minimum row, whose outputs reach -2^(in_bits - 1) (R M)^N and so need every one of those bits; and cic_ref
    in its 32- or 64-bit registers gives the same values"""
    rng = np.random.default_rng(N * 1000 + R)
    x = _rows(rng, N, R, M, in_bits)
    tight = in_bits + growth(N, R, M)
    W = reg_bits(in_bits, N, R, M)
    assert tight <= W
    for position in (0, R - 1, 3 * R + 1):
        y, _ = cic_ref(x, N, R, M, W, position)
        for c in range(x.shape[0]):
            row = [int(v) for v in x[c]]
            exact = fir_exact(row, N, R, M, position)
            assert hogenauer_serial(row, N, R, M, tight, position) == exact
            assert hogenauer_serial(row, N, R, M, W, position) == exact
            assert [int(v) for v in y[c]] == exact
    steady = -(1 << (in_bits - 1)) * (R * M) ** N
    # the bound is reached: the value fits tight bits of two's complement and not one fewer
    assert int(y[1, -1]) == steady and -(1 << (tight - 1)) <= steady < -(1 << (tight - 2))
    assert hogenauer_serial([int(v) for v in x[1]], N, R, M, tight - 1)[-1] != steady


@pytest.mark.parametrize("N,R,M,in_bits", SHAPES)
def test_reference_is_modular_for_inputs_wider_than_in_bits(N, R, M, in_bits):
    """with full-width samples in registers narrower than in_bits + growth the outputs wrap, and cic_ref still equals the serial
    form of that width: the definition is modular"""
    rng = np.random.default_rng(N * 77 + R)
    S = _length(N, R, M)
    x = rng.integers(-(1 << 31), 1 << 31, (2, S)).astype(np.int32)
    for W in (32, 64):
        y, _ = cic_ref(x, N, R, M, W, 5)
        for c in range(2):
            assert [int(v) for v in y[c]] == hogenauer_serial([int(v) for v in x[c]], N, R, M, W, 5)


@pytest.mark.parametrize("N,R,M,in_bits", SHAPES)
@pytest.mark.parametrize("cplx", [False, True])
def test_reference_streamed_equals_one_call(N, R, M, in_bits, cplx):
    """calls of 0, 1, R - 1, R + 1, 3 and the rest with history and position carried: outputs and final history of one call"""
    rng = np.random.default_rng(N * 13 + R + cplx)
    S = _length(N, R, M) + 2 * R + 4
    shape = (2, S, 2) if cplx else (2, S)
    x = rng.integers(-(1 << (in_bits - 1)), 1 << (in_bits - 1), shape).astype(_dtype(in_bits))
    state = rng.integers(-(1 << (in_bits - 1)), 1 << (in_bits - 1), (2, N * M * R) + shape[2:]).astype(x.dtype)
    W = reg_bits(in_bits, N, R, M)
    for out in ("int", "f32"):
        one, s_one = cic_ref(x, N, R, M, W, 7, state, out)
        many, s_many = stream_ref(x, splits(R, S), N, R, M, W, 7, state, out)
        assert one.dtype == many.dtype and one.tobytes() == many.tobytes()
        assert s_one.tobytes() == s_many.tobytes()
        assert np.array_equal(s_one, x[:, ::-1][:, :N * M * R])  # S >= hist: the block's last samples, newest first
    if cplx:
        for p in range(2):  # the planes are independent real streams
            y, _ = cic_ref(np.ascontiguousarray(x[..., p]), N, R, M, W, 7, np.ascontiguousarray(state[..., p]))
            assert np.array_equal(y, cic_ref(x, N, R, M, W, 7, state)[0][..., p])


def test_float_output_rule():
    """(float)((double)y * scale): one conversion each way and one product, all to nearest even"""
    x = np.full((1, 40), -32768, dtype=np.int16)
    y, _ = cic_ref(x, 3, 5, 1, 32, out="f32")
    assert y.dtype == np.float32 and y[0, -1] == np.float32(-32768.0 * 125 * (1.0 / 125.0))
    big = np.full((1, 6 * 1024 * 3 + 1024), 1, dtype=np.int16)
    yi, _ = cic_ref(big, 6, 1024, 1, 64)
    yf, _ = cic_ref(big, 6, 1024, 1, 64, out="f32", scale=3.0)
    assert int(yi[0, -1]) == 1024 ** 6 and yf[0, -1] == np.float32(float(1024 ** 6) * 3.0)


# ---------------------------------------------------------------------------------------------------------- the library's helpers

GROWTH_SHAPES = [(N, R, M) for N, R, M, _ in SHAPES] + [(8, 4096, 2), (2, 16384, 2), (8, 16, 1), (4, 256, 1), (4, 255, 1), (1, 16384, 1)]


def test_growth_and_unity_scale_against_python_integers():
    lib = sd.load()
    for N, R, M in GROWTH_SHAPES:
        assert sd.cic_growth(N, R, M) == growth(N, R, M), (N, R, M)
        assert sd.cic_unity_scale(N, R, M) == unity_scale(N, R, M), (N, R, M)
    b, s = C.c_uint32(7), C.c_double(7.0)
    for bad in ((0, 2, 1), (9, 2, 1), (1, 1, 1), (1, 16385, 1), (1, 2, 0), (1, 2, 3), (8, 8192, 2), (5, 16384, 1)):
        assert lib.sdsp_hip_cic_growth(*bad, C.byref(b)) == L.ERR_INVALID_SIZE, bad
        assert lib.sdsp_hip_cic_unity_scale(*bad, C.byref(s)) == L.ERR_INVALID_SIZE, bad
        assert b.value == 0 and s.value == 0.0
    assert lib.sdsp_hip_cic_growth(3, 5, 1, None) == L.ERR_INVALID_ARG
    assert lib.sdsp_hip_cic_unity_scale(3, 5, 1, None) == L.ERR_INVALID_ARG


def test_out_samples_against_python_integers():
    lib = sd.load()
    n = C.c_uint64(0)
    for R in (2, 5, 64, 1024, 16384):
        for position in (0, 1, R - 1, R, (1 << 40) + 3, (1 << 64) - 1, (1 << 64) - R, (1 << 64) - (1 << 31)):
            for S in (0, 1, R - 1, R, R + 1, 12345, (1 << 31) - 1):
                assert lib.sdsp_hip_cic_out_samples(R, position, S, C.byref(n)) == 0
                assert n.value == out_samples(R, position, S), (R, position, S)
        total, position = 0, 11  # a split stream produces what one call does
        for S in splits(R, 10 * R + 9):
            lib.sdsp_hip_cic_out_samples(R, position, S, C.byref(n))
            total, position = total + n.value, position + S
        assert total == out_samples(R, 11, 10 * R + 9)
    assert lib.sdsp_hip_cic_out_samples(1, 0, 8, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_cic_out_samples(16385, 0, 8, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_cic_out_samples(2, 0, 1 << 31, C.byref(n)) == L.ERR_INVALID_SIZE
    assert lib.sdsp_hip_cic_out_samples(2, 0, 8, None) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("N,R,M", [(N, R, M) for N, R, M, _ in SHAPES] + [(8, 64, 2)])
def test_taps_against_python_integers(N, R, M):
    h = sd.cic_taps(N, R, M)
    want = taps_exact(N, R, M)
    assert h.dtype == np.uint64 and len(h) == N * (R * M - 1) + 1 == len(want)
    assert [int(v) for v in h] == [v % (1 << 64) for v in want]
    assert sum(want) == (R * M) ** N
    assert sd.load().sdsp_hip_cic_taps(N, R, M, None) == L.ERR_INVALID_ARG
    assert sd.load().sdsp_hip_cic_taps(N, 1, M, h.ctypes.data) == L.ERR_INVALID_SIZE


def test_taps_applied_mod_2_64_are_the_reference():
    """variant 1's form: sum h[k] x[n - k] mod 2^W at the due indices equals cic_ref"""
    N, R, M = 8, 3, 2
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, 400).astype(np.int16)
    h = [int(v) for v in sd.cic_taps(N, R, M)]
    y, _ = cic_ref(x[None], N, R, M, 64)
    for m, n in enumerate(range(R - 1, 400, R)):
        acc = sum(h[k] * int(x[n - k]) for k in range(min(len(h), n + 1)))
        assert wrap(acc, 64) == int(y[0, m])


def test_bank_arguments_and_the_width_rule():
    """W = 32 up to in_bits + growth = 32, 64 up to 64; the Python surface refuses what the C API refuses"""
    assert growth(4, 256, 1) == 32 and growth(4, 255, 1) == 32 and growth(2, 256, 1) == 16 and growth(8, 128, 2) == 64
    assert sd.cic_decimator(2, 256, in_bits=16).reg_bits == 32      # 16 + 16 = 32
    assert sd.cic_decimator(2, 256, in_dtype="i32", in_bits=17).reg_bits == 64  # 33
    b = sd.cic_decimator(3, 5)
    assert (b.hist, b.growth, b.reg_bits, b.position, b.scale) == (15, 7, 32, 0, 1.0 / 125.0)
    assert b.out_samples(14) == 2
    b.position = (1 << 40) + 3
    assert b.out_samples(1) == out_samples(5, (1 << 40) + 3, 1)
    for bad in (dict(kind="iq"), dict(in_dtype="i8"), dict(out="f64")):
        with pytest.raises(ValueError):
            sd.cic_decimator(3, 5, **bad)
    with pytest.raises(sd.SdspHipError):
        sd.cic_decimator(9, 5)
    with pytest.raises(ValueError):
        b.set_variant(2)
    with pytest.raises(ValueError):
        b.set_segment(1 << 20)


def test_plan_needs_a_device_and_says_so():
    """no CPU fallback: without a usable device, creation fails loudly (with one, it must succeed); the argument errors come first,
    the width rule at its boundaries 32 / 33 and 64 / 65 bits among them"""
    import torch
    lib = sd.load()
    p = C.c_void_p()
    create = lambda *a: lib.sdsp_hip_cic_plan_create(C.byref(p), *a, 0)  # noqa: E731
    ok = (3, 5, 1, L.CIC_I16, 16, L.CIC_REAL, L.CIC_OUT_INT, 1.0)

    def with_(**kw):
        names = ("order", "down", "delay", "in_type", "in_bits", "kind", "out", "scale")
        a = dict(zip(names, ok))
        a.update(kw)
        return create(*[a[k] for k in names])

    for kw in (dict(order=0), dict(order=9), dict(down=1), dict(down=16385), dict(delay=0), dict(delay=3), dict(order=8, down=8192, delay=2),
               dict(in_bits=1), dict(in_bits=17), dict(in_type=L.CIC_I32, in_bits=33)):
        assert with_(**kw) == L.ERR_INVALID_SIZE, kw
    for kw in (dict(in_type=2), dict(kind=2), dict(out=2), dict(scale=float("nan")), dict(scale=float("inf"))):
        assert with_(**kw) == L.ERR_INVALID_ARG, kw
    assert lib.sdsp_hip_cic_plan_create(None, *ok, 0) == L.ERR_INVALID_ARG
    # growth(8, 128, 2) = 64: one input bit more than the registers hold is refused before any device is asked for
    assert with_(order=8, down=128, delay=2, in_bits=2) == L.ERR_UNSUPPORTED
    msg = lib.sdsp_hip_last_error_string().decode()
    assert "2" in msg and "64" in msg and "66" in msg, msg
    assert with_(order=6, down=1024, delay=1, in_bits=5) == L.ERR_UNSUPPORTED  # 5 + 60 = 65
    have = torch.cuda.is_available()
    info = L.CicPlanInfo()
    # (in_bits, growth) at 32 | 33 and 64 | 64: W as the rule says
    for kw, W in ((dict(order=2, down=256, in_bits=16), 32), (dict(order=2, down=256, in_type=L.CIC_I32, in_bits=17), 64),
                  (dict(order=6, down=1024, in_bits=4), 64), (dict(), 32)):
        rc = with_(**kw)
        if have:
            assert rc == 0
            assert lib.sdsp_hip_cic_plan_get_info(p, C.byref(info)) == 0
            assert info.reg_bits == W and info.in_bits + info.growth <= W and info.hist == info.order * info.down * info.delay
            lib.sdsp_hip_cic_plan_destroy(p)
        else:
            assert rc == L.ERR_NO_DEVICE


def test_host_helpers_under_the_sanitizers(tmp_path):
    """the four host-only helpers in a program of their own with host_math.cpp, both built with -fsanitize=address,undefined: the tap
    buffer is exactly as long as documented.  Nothing loaded into Python runs under a sanitizer."""
    exe = tmp_path / "cic_host_helpers"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
           f"-I{ROOT / 'simpledsp_amd' / 'csrc'}", '-DSDSP_HIP_SOURCE_HASH="none"', str(ROOT / "tests" / "cpp" / "cic_host_helpers.cpp"),
           str(ROOT / "simpledsp_amd" / "csrc" / "host_math.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
