"""The direct-form FIR bank held to bits on every row (tests/recur_exact.py) on a real MI355X.

csrc/fir.hip fixes the order: ascending taps; one FMA per tap in f32 (packed two outputs per instruction or not), one multiply
and one add in f64.  So every output element and the whole final history have the bits of a plain numpy model (R1), for every
variant, from a random history, in one call and in blocks shorter and longer than the history; the f32 values are also held to
R2: e2 <= 3 max(e2 of the unfused f32 sum, 1 u) per row against the longdouble sum."""
import functools

import numpy as np
import pytest

import recur_exact as rx

pytestmark = pytest.mark.gpu

TAPS = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 257)  # the edges of the 16-tap chunks and of the packed pairs
# (channels, samples, row stride): one row; ragged rows; more than one workgroup with an odd stride (rows off 16 bytes: the
# element path); rows shorter than the history
SHAPES = ((1, 300, 300), (67, 100, 100), (130, 1003, 1003), (5, 15, 15))
CASES = [(t,) + s for t in TAPS for s in SHAPES] + [(1000, 67, 100, 100)]
BLOCK_EDGES = (1, 8, 40, 600)  # the five-block split of test_gpu_fir.test_streaming_blocks_unaligned_rows_and_preload


def case_id(case):
    return f"taps{case[0]}-{case[1]}x{case[2]}"


def blocks(samples):
    edges = [0] + [e for e in BLOCK_EDGES if e < samples] + [samples]
    return list(zip(edges[:-1], edges[1:]))


@functools.lru_cache(maxsize=2)
def reference(case, precision):
    """input, random history, model, and for f32 the plain baseline and the longdouble sum; computed once, left unchanged"""
    taps, channels, samples, stride = case
    rng = np.random.default_rng(7919 * taps + 31 * channels + samples)
    T = rx.RDT[precision]
    h = rng.standard_normal(taps) / np.sqrt(taps)
    x = rng.standard_normal((channels, stride)).astype(T)
    hist = rng.standard_normal((channels, max(taps - 1, 1))).astype(T)
    ref = dict(h=h, x=x, hist=hist)
    if precision == "f32":
        ref["y"], ref["final"] = rx.fir_model_f32(x[:, :samples], h, hist)
        ref["plain"], _ = rx.fir_plain(x[:, :samples], h, hist, "f32")
        ref["ld"] = rx.fir_ld(x[:, :samples], h, hist, "f32")
    else:
        ref["y"], ref["final"] = rx.fir_plain(x[:, :samples], h, hist, "f64")
    for v in ref.values():
        v.flags.writeable = False
    return ref


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


def run(sd, torch, case, precision, variant, split):
    """(output, final history) of one run of a case"""
    taps, channels, samples, stride = case
    ref = reference(case, precision)
    bank = sd.fir_filter(taps, channels, sd.F64 if precision == "f64" else sd.F32)
    bank.set_coeff(ref["h"])
    bank.set_variant(variant)
    bank._state = torch.from_numpy(ref["hist"].copy()).cuda()
    d = torch.from_numpy(ref["x"].copy()).cuda()
    for lo, hi in (blocks(samples) if split else [(0, samples)]):
        bank.process(d, samples=hi - lo, offset=lo)
    torch.cuda.synchronize()
    return d.cpu().numpy()[:, :samples], bank.state.cpu().numpy()[:, :taps - 1]


def check(case, precision, got, hist, what):
    ref = reference(case, precision)
    # -0 and +0 are one value here: the packed kernel starts odd outputs from h0 * x and even ones from fma(h0, x, 0)
    r1 = [rx.r1(got, ref["y"], what + " output", ignore_zero_sign=True), rx.r1(hist, ref["final"], what + " final history")]
    r2, fig = rx.r2(got, ref["plain"], ref["ld"], "f32") if precision == "f32" else ("", None)
    return rx.verdict(r1, r2), fig


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_f32_bits_and_accuracy(sd, torch_cuda, case):
    for variant in (0, 1, 2, 3):  # the default choice, default cache policy, packed FMAs, one FMA per tap
        for split in (False, True):
            got, hist = run(sd, torch_cuda, case, "f32", variant, split)
            msg, fig = check(case, "f32", got, hist, f"{case_id(case)} f32 variant {variant} {'blocks ' + str(blocks(case[2])) if split else 'one call'}")
            print(case_id(case), variant, split, fig)
            assert not msg, msg


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_f64_bits_on_every_row(sd, torch_cuda, case):
    for variant in (0, 1):
        for split in (False, True):
            got, hist = run(sd, torch_cuda, case, "f64", variant, split)
            msg, _ = check(case, "f64", got, hist, f"{case_id(case)} f64 variant {variant} {'blocks' if split else 'one call'}")
            assert not msg, msg
