"""Every strided buffer of every device entry with its two rows 2^34 + 256 bytes apart, and stream positions past 2^32, on a real MI355X.

include/sdsp_hip.h takes every row stride as a uint64_t and promises rows "anywhere inside a larger buffer"; the kernels form row
pointers as c * stride, several keep 32-bit offsets behind a host-side check, and the launchers' vector switches are computed from
stride * element size.  A stride or a product narrowed to 32 bits does not fault: it reads or writes another row.  So:

  * ONE arena of 2^34 + 2^20 bytes (`wide_arena`: torch.empty, never filled, freed at teardown) serves the whole module.
  * Each case puts exactly ONE strided buffer of ONE entry into it (the entries refuse overlapping ranges, so two buffers of a call
    cannot share it); every other buffer of the call is an ordinary, exactly-sized tensor.  The wide buffer has two rows: row 0 one guard
    band (4 KiB) past the arena's start, row 1 arena.wide_distance() later -- 2^34 + 256 bytes, that is 2^32 + 64 elements for 4-byte
    reals and int32, 2^31 + 32 for complex64 / 8-byte reals / int64 (2^32 + 64 in reals, the unit the kernels compute in), 2^30 + 16 for
    complex128; a row of bytes (the detector's det) has a stride of 2^32 + 64 bytes.  4-byte types therefore test the truncation of the
    element index AND of the byte offset, 8-byte and wider types that of the byte offset only (tests/test_arena_host.py shows both on
    stand-ins); the arena is not grown for them.
  * + 64: an offset truncated to 32 bits lands 256 bytes into row 0, inside its initialised data (arena.WideRows asserts that the row
    is longer than that), so a truncating read returns row 0's values shifted and a truncating write damages row 0 and leaves row 1
    at its fill: both fail on defined data.  Each row and 4 KiB on either side are filled with the two fills of arena.fills in turn,
    and the bands must keep their bits; the 16 GiB in between are not looked at.

Per entry, precision, kind and kernel variant (every value *_plan_set_variant takes for the shape):
  1. the call with all buffers compact is held to the bank's reference, with the comparison and tolerance of the bank's own GPU test
     file (bit equality for the bit-exact banks);
  2. for every strided buffer in turn, the same call with that buffer wide gives the compact call's bits in every writable buffer and in
     the state, leaves every read-only buffer and the guard bands alone (arena.check_wide);
  3. or the entry refuses the stride before any launch: then nothing changed, the status is the documented one and the header states
     the limit at that entry (REFUSALS).

How a case is made: the bank's Python class builds the plan and makes one call, which a recording proxy of the library sees; the
entry's parameter names come from the header, the tensors behind its pointers from the bank and the case, and the call is then
repeated through the C entry with data_ptr()s (`_discover`).  This leans on private members of the Python bank classes: `_lib` (the
library handle, swapped for the proxy during that one call), `_plan`, the device tensors among a bank's attributes (`_state`, `_acc`,
`_acc_xy`, `_acc_auto`: found by their data_ptr()s), and in the builders `_state`, `_position`, `_ensure_plan`, `_ensure_buffers`
and `_ensure_state`, as the banks' own GPU test files use them; a rename there shows here as a failed assertion of `_discover`, not
as a wrong result.  test_every_stride_parameter_is_covered reads the header and holds the
case table to it, without a GPU.

Known remainder: the kernel-choice thresholds of the biquad launcher (iir.hip: stride * size * 8 < 2^32 for the tiled kernels) at
their exact boundary need 64 rows just under 2^29 bytes apart, a 32 GiB reservation; here the stride is far past them.  Rows of 2^32
samples and channel counts whose product with a small stride passes 2^32 need the memory written and are out of scope.

The second part runs pfb_process, pfb_synth_process, welch_process and csd_process at stream positions that cross 2^32 inside a
call and inside a two-call split, and at 2^40 + 7, against the numpy references (which take Python integers)."""
import ctypes as C
import re
import time
from pathlib import Path

import numpy as np
import pytest
import scipy.signal

import arena
from conftest import design, rel_max_err

gpu = pytest.mark.gpu  # every test that touches the device; the two that only read the header and the references run without one

HEADER = Path(__file__).resolve().parents[1] / "include" / "sdsp_hip.h"


# ------------------------------------------------------------------ the header: entries, their parameters, their stride parameters

def _header_entries():
    """{entry: [(C type, parameter name), ..]} of every `int sdsp_hip_*(..)` declaration"""
    src = HEADER.read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for m in re.finditer(r"\bint\s+(sdsp_hip_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = []
        for p in " ".join(m.group(2).split()).split(","):
            pm = re.match(r"^(.*?)(\w+)$", p.strip())
            if pm and pm.group(1).strip():
                params.append((pm.group(1).strip(), pm.group(2)))
        out[m.group(1)] = params
    return out


ENTRIES = _header_entries()


def _stride_parameters():
    """[(entry, stride parameter)] of every uint64_t *stride parameter the header declares"""
    return [(e, n) for e, params in ENTRIES.items() for t, n in params if t == "uint64_t" and n.endswith("stride")]


def _buffer_of(entry, stride_name):
    """the pointer parameter a stride parameter belongs to"""
    names = [n for _, n in ENTRIES[entry]]
    stem = "data" if stride_name == "stride" else stride_name[:-len("_stride")]
    for cand in (stem, "host_" + stem):
        if cand in names:
            return cand
    raise AssertionError((entry, stride_name, "no pointer parameter goes with it"))


def _stride_of(entry, buffer):
    names = [n for _, n in ENTRIES[entry]]
    for cand in (buffer + "_stride", "stride" if buffer == "data" else None):
        if cand in names:
            return cand
    return None


def _header_text_at(entry):
    """the header from the end of the declaration before `entry` to the end of its own: its comment and its prototype"""
    raw = HEADER.read_text()
    at = re.search(r"\bint\s+" + entry + r"\s*\(", raw).start()
    start = raw.rfind(");", 0, at)
    return " ".join(raw[start:raw.index(");", at)].split())


# ------------------------------------------------------------------ fixtures

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


@pytest.fixture(scope="module")
def wide_arena(torch_cuda):
    """the one 16 GiB reservation of the module, in a list so that teardown drops the last reference to it"""
    t0 = time.perf_counter()
    holder = [torch_cuda.empty((1 << 34) + (1 << 20), dtype=torch_cuda.uint8, device="cuda")]
    print(f"wide arena: {holder[0].numel()} bytes reserved in {time.perf_counter() - t0:.3f} s")
    yield holder
    holder.clear()
    torch_cuda.cuda.empty_cache()


# ------------------------------------------------------------------ one recorded call, repeated through the C entry

class _Recorder:
    """stands in for a bank's library handle and notes the arguments of every process / finalize call"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith(("_process", "_process_interleaved", "_finalize")):
            return fn

        def recorded(*args):
            self.calls.append((name, list(args)))
            return fn(*args)
        return recorded


def _tensors_of(obj):
    import torch
    for v in vars(obj).values():
        for t in (v if isinstance(v, (list, tuple)) else v.values() if isinstance(v, dict) else [v]):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                yield t


def _flat(outs):
    import torch
    if isinstance(outs, torch.Tensor):
        return [outs]
    return [t for t in outs if isinstance(t, torch.Tensor)] if isinstance(outs, (list, tuple)) else []


def _discover(torch, bank, thunk, inputs, entry):
    """Runs thunk() -- one call of `entry` through the bank's Python class -- and returns (specs, call) for arena.run_placed: the specs
    of every buffer the entry got a pointer to, named as the header names the parameter, and call(placed), which repeats the entry
    with those buffers wherever `placed` puts them.  A buffer's contents before the call are those it had before thunk(): the case's
    inputs and the bank's tensors as they were, zeros for what the bank made during the call (its state and sums start at zero),
    the fill for what the call returned (outputs)."""
    before = [(t, t.clone()) for t in [*inputs, *_tensors_of(bank)]]
    rec = _Recorder(bank._lib)
    bank._lib = rec
    try:
        outs = _flat(thunk())
    finally:
        bank._lib = rec._lib
    torch.cuda.synchronize()
    calls = [args for name, args in rec.calls if name == entry]
    assert len(calls) == 1, (entry, [name for name, _ in rec.calls])
    args, params = calls[0], ENTRIES[entry]
    assert len(args) == len(params), (entry, len(args), len(params))
    pool = [(t, None) for t in outs if not any(t is b for b, _ in before)] + before
    pool += [(t, torch.zeros_like(t)) for t in _tensors_of(bank) if not any(t is b for b, _ in pool)]
    index = {n: i for i, (_, n) in enumerate(params)}
    specs, units = {}, {}
    for i, (ctype, name) in enumerate(params):
        value = getattr(args[i], "value", args[i])
        if "*" not in ctype or name in ("plan", "stream") or not value:
            continue
        found = [(t, init) for t, init in pool if t.data_ptr() == value]
        assert found, (entry, name, "no tensor of the case or the bank lies at this pointer")
        t, init = found[0]
        assert t.is_contiguous(), (entry, name)
        rows = t.shape[0] if t.dim() >= 2 else 1
        cols = t.numel() // rows
        specs[name] = dict(shape=(rows, cols), dtype=t.dtype, init=init, read_only="const" in ctype)
        sname = _stride_of(entry, name)
        if sname is not None:
            stride = int(getattr(args[index[sname]], "value", args[index[sname]]))
            assert (cols * t.element_size()) % stride == 0, (entry, name, "the recorded call has compact rows", cols, stride)
            units[name] = cols * t.element_size() // stride  # bytes per stride unit: a complex sample, a real, a byte
    fn = getattr(rec._lib, entry)

    def call(placed):
        a = list(args)
        for name, p in placed.items():
            a[index[name]] = p.ptr
            if isinstance(p, arena.WideRows):
                a[index[_stride_of(entry, name)]] = p.distance // units[name]
                assert a[index[_stride_of(entry, name)]] * units[name] == p.distance > 1 << 32
        return fn(*a)
    return specs, call


# (entry, parameter) -> (status, words of include/sdsp_hip.h at that entry that state the limit): the strides an entry refuses by contract
REFUSALS = {}

RESULTS = {}  # (entry, buffer) -> set of statuses seen, for the summary test_summary prints


def _drive(torch, wide_arena, entry, built, tag):
    """items 1 to 3 of the module docstring for one built case: built = (bank, thunk, inputs, check, wide buffers)"""
    bank, thunk, inputs, check, wide = built
    specs, call = _discover(torch, bank, thunk, inputs, entry)
    clean = []
    for fill in (0, 1):
        status, got = arena.run_placed(torch, specs, call, fill, tag=f"{tag} compact, fill {fill}")
        assert status == 0, (tag, "the compact call failed", status)
        clean.append(got)
    check(clean[0])
    for name in wide:
        assert name in specs, (tag, name, sorted(specs))
        assert _stride_of(entry, name), (tag, name)
        assert specs[name]["shape"][0] == 2 and specs[name]["shape"][1] >= 160, (tag, name, specs[name]["shape"])
        status = arena.check_wide(torch, specs, call, clean, name, wide_arena[0], tag=tag)
        RESULTS.setdefault((entry, name), set()).add(status)
        if status != 0:
            key = (entry, _stride_of(entry, name))
            assert key in REFUSALS, (tag, f"'{name}' wide is refused with {status}: include/sdsp_hip.h names no such limit")
            code, words = REFUSALS[key]
            assert status == code, (tag, name, status, code)
            assert words in _header_text_at(entry), (tag, name, "the header does not state the limit at the entry")


# ------------------------------------------------------------------ the cases

CH = 2
F1, F2 = 0x1234567, 0x9abcdef0


def _prec(sd, precision):
    return sd.F64 if precision == "f64" else sd.F32


def _rdt(torch, precision):
    return torch.float64 if precision == "f64" else torch.float32


def _npr(precision):
    return np.float64 if precision == "f64" else np.float32


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _set_variant(bank, variant):
    """for the banks around an inner transform plan, whose variants are that plan's: False where it has no such variant -- the one
    refusal sdsp_hip_*_plan_set_variant documents for them (UNSUPPORTED, "no such kernel variant"); anything else is an error"""
    from simpledsp_amd._lib import ERR_UNSUPPORTED, SdspHipError
    try:
        bank.set_variant(variant)
        return True
    except SdspHipError as e:
        assert e.code == ERR_UNSUPPORTED and "no such kernel variant" in e.message, (variant, e)
        return False


def _rng(*key):
    return np.random.default_rng(sum(map(ord, "".join(map(str, key)))))


def build_iir(env, precision, kind, variant):
    sd, torch = env.sd, env.torch
    S, m = 2176, 4  # 17 x 512 bytes of f32: 16-byte aligned rows, so variants 0, 1 and 3 take the super-tile kernel and 2 the direct one
    x = _rng("iir", precision).standard_normal((CH, S)).astype(_npr(precision))
    bank = sd.casc_2o_iir(m, CH, _prec(sd, precision), sd.IIR_GENERIC)
    design(bank, 1, 10e3, 100e3, 1.1)
    bank.set_variant(variant)
    data = _dev(torch, x)

    def check(clean):
        got = _np(clean["data"])
        for c in range(CH):
            fo2 = env.oracle.iir(m)
            design(fo2, 1, 10e3, 100e3, 1.1)
            want = fo2.process(x[c].astype(np.float64), sd.IIR_GENERIC)
            if precision == "f64":
                assert np.array_equal(got[c], want), (c, variant)
            else:
                assert rel_max_err(got[c], want) < 1e-6, (c, variant)
        # sdsp_hip_iir_plan_kernel takes the same stride: the library's own choice for compact and for wide rows, for the two rows of
        # this case and for a whole tile of 64, where compact rows go to the kernels that keep 32-bit lane offsets (iir.hip: `tiles`)
        names = {}
        for channels in (CH, 64):
            for stride in (S, arena.wide_distance(data.element_size()) // data.element_size()):
                buf = C.create_string_buffer(64)
                assert env.lib.sdsp_hip_iir_plan_kernel(bank._plan, data.data_ptr(), channels, S, stride, buf, 64) == 0
                names[channels, stride == S] = buf.value.decode()
        print(f"iir {precision} variant {variant}: kernels {names}")
        narrow = ("sdsp_iir_landing_kernel", "sdsp_iir_wide_kernel")
        assert names[64, False] not in narrow and names[CH, False] not in narrow, names
        assert names[64, False] == names[CH, False], names  # the kernel this case ran wide is the one a whole tile gets at that stride
        if variant == 1 or (variant == 0 and precision == "f32"):
            assert names[64, True] in narrow, names  # so the host-side check did flip the choice
    return bank, lambda: bank.process(data), [data], check, ("data",)


def build_iir_interleaved(env, precision, kind, variant):
    """two sample rows of 256 channels, after a compact first call of 64 rows; the reference is the channel-major entry on the
    transposed stream, which the contract makes bit-identical, and for f64 the oracle's recurrence"""
    sd, torch = env.sd, env.torch
    channels, first, m = 256, 64, 4
    x = _rng("iiril", precision).standard_normal((first + 2, channels)).astype(_npr(precision))
    bank = sd.casc_2o_iir(m, channels, _prec(sd, precision), sd.IIR_GENERIC)
    design(bank, 1, 10e3, 100e3, 1.1)
    bank.set_variant(variant)
    try:
        bank.process_interleaved(_dev(torch, x[:first]))
    except sd._lib.SdspHipError as e:  # the interleaved entry has 0, 1 and 2
        assert variant > 2 and e.code == sd._lib.ERR_INVALID_ARG and "unknown IIR kernel variant" in e.message, (variant, e)
        return None
    assert bool((bank.state != 0).any())
    data = _dev(torch, x[first:])

    def check(clean):
        other = sd.casc_2o_iir(m, channels, _prec(sd, precision), sd.IIR_GENERIC)
        design(other, 1, 10e3, 100e3, 1.1)
        t = _dev(torch, x.T)
        other.process(t)
        assert arena.same_bits(clean["data"], t[:, first:].t().contiguous()), variant
        assert arena.same_bits(clean["state"].reshape(other.state.shape), other.state), variant
        if precision == "f64":
            fo = env.oracle.iir(m)
            design(fo, 1, 10e3, 100e3, 1.1)
            assert np.array_equal(_np(clean["data"])[:, 5], fo.process(x[:, 5], sd.IIR_GENERIC)[first:])
    return bank, lambda: bank.process_interleaved(data), [data], check, ("data",)


def build_fir(env, precision, kind, variant):
    sd, torch = env.sd, env.torch
    rng = _rng("fir", precision, kind)
    if kind == "direct":
        taps, S = 33, 2085
        bank = sd.fir_filter(taps, CH, _prec(sd, precision))
    else:
        taps, S = 300, 9000  # three frames of the smallest transform and a ragged one
        bank = sd.fft_fir_filter(taps, CH, _prec(sd, precision))
    h = rng.standard_normal(taps)
    bank.set_coeff(h)
    x = rng.standard_normal((CH, S)).astype(_npr(precision))
    hist = rng.standard_normal((CH, taps - 1)).astype(_npr(precision))
    bank._state = _dev(torch, hist)
    data = _dev(torch, x)

    bank.set_variant(variant)  # applied when the plan is made; an FFT plan falls back where its transform has no such fused kernel

    def check(clean):
        import test_gpu_fir_fft as t
        got = _np(clean["data"])
        if kind == "fft":
            assert bank.info()["method"] == sd.FIR_FFT
            t._check(env.oracle, h, x, hist, got, _np(clean["state"]), precision)
            return
        hs, xs, ss = t._seen(h, x, hist, precision)
        for c in range(CH):
            want, want_state = env.oracle.fir_process(hs, xs[c], ss[c])
            if precision == "f64":
                assert np.array_equal(got[c], want), (c, variant)
            else:
                assert rel_max_err(got[c], want) < 1e-6, (c, variant)
            assert np.array_equal(_np(clean["state"])[c].astype(np.float64), want_state), c
    return bank, lambda: bank.process(data), [data], check, ("data",)


def build_filtfilt(env, precision, kind, variant):
    import test_gpu_filtfilt as t
    sd, torch = env.sd, env.torch
    m, S = 4, 2100
    fk, a, b, g = t._design(sd, "bp", m)
    plan = t._plan(sd, fk, a, b, g, precision, "odd")
    plan.set_variant(variant)
    x = t._signal(torch, precision, CH, S, seed=3)
    data = x.clone()

    def check(clean):
        assert torch.equal(clean["data"], t._composition(torch, sd, x, fk, a, b, g, precision, "odd", None)), variant
        names = []
        for stride in (S, arena.wide_distance(data.element_size()) // data.element_size()):
            buf = C.create_string_buffer(64)
            assert env.lib.sdsp_hip_filtfilt_plan_kernel(plan._plan, data.data_ptr(), CH, S, stride, buf, 64) == 0
            names.append(buf.value.decode())
        assert all(names), names
        print(f"filtfilt {precision} variant {variant}: kernel {names[0]} for compact rows, {names[1]} for wide rows")
    return plan, lambda: plan.process(data), [data], check, ("data",)


def build_resample(env, precision, kind, variant):
    import test_gpu_resample as t
    from resample_ref import hist_of, q_of, resample_ref
    sd, torch = env.sd, env.torch
    up, down, taps = 3, 2, 37
    rng = _rng("resample", precision)
    h = rng.standard_normal(taps)
    S = q_of(up, down) * 700
    x = rng.standard_normal((CH, S)).astype(_npr(precision))
    hist = rng.standard_normal((CH, max(hist_of(taps, up), 1))).astype(_npr(precision))
    if variant > 2:
        with pytest.raises(ValueError, match="variant must be 0, 1 or 2"):
            t._bank(sd, h, up, down, CH, precision, variant, hist)
        return None
    bank = t._bank(sd, h, up, down, CH, precision, variant, hist)
    xd = _dev(torch, x)

    def check(clean):
        hh = h if precision == "f64" else h.astype(np.float32)
        want, want_state = resample_ref(hh, x, up, down, hist[:, :hist_of(taps, up)])
        got = _np(clean["out"])
        if precision == "f64":
            assert np.array_equal(got, want) and np.array_equal(_np(clean["state"]), want_state), variant
        else:
            assert rel_max_err(got, want) <= 1e-6, variant
    return bank, lambda: bank.process(xd), [xd], check, ("in", "out")


STREAM_SHAPES = {"n32h3": (32, 3, 60), "n512h64": (512, 64, 10)}  # n_fft or m, hop, frames: rows of at least 160 elements


def _cplx(rng, shape, cplx):
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def build_stft(env, precision, kind, variant):
    from stft_ref import stft_ref
    from test_gpu_stft import _tol
    sd, torch = env.sd, env.torch
    shape, output = kind.split("-")
    n, hop, F = STREAM_SHAPES[shape]
    w = scipy.signal.get_window("hann", n)
    bank = sd.stft_bank(n, hop, CH, window=w, output=output, precision=_prec(sd, precision))
    if not _set_variant(bank, variant):
        return None
    rng = _rng("stft", kind, precision)
    x = rng.standard_normal((CH, F * hop)).astype(_npr(precision))
    hist = rng.standard_normal((CH, n - hop)).astype(_npr(precision))
    bank._state = _dev(torch, hist)
    xd = _dev(torch, x)

    def check(clean):
        want, state = stft_ref(x, n, hop, w, hist, output)
        err = rel_max_err(_np(clean["out"]).reshape(want.shape), want)
        assert err <= _tol(precision, n, output), (err, variant)
        assert np.array_equal(_np(clean["state"]), state.astype(x.dtype))
    return bank, lambda: bank.process(xd), [xd], check, ("in", "out")


def build_istft(env, precision, kind, variant):
    from istft_ref import istft_ref
    from test_gpu_istft import _tol
    sd, torch = env.sd, env.torch
    n, hop, F = STREAM_SHAPES[kind]
    bins = n // 2 + 1
    w = scipy.signal.get_window("hann", n)
    bank = sd.istft_bank(n, hop, CH, window=w, precision=_prec(sd, precision))
    if not _set_variant(bank, variant):
        return None
    rng = _rng("istft", kind, precision)
    X = _cplx(rng, (CH, F, bins), True).astype(np.complex128 if precision == "f64" else np.complex64)
    pend = rng.standard_normal((CH, n - hop)).astype(_npr(precision))
    bank._state = _dev(torch, pend)
    Xd = _dev(torch, X)

    def check(clean):
        want, state = istft_ref(X, n, hop, bank.synthesis_window, pend)
        tol = _tol(precision, n, hop)
        assert rel_max_err(_np(clean["out"]), want) <= tol, variant
        assert rel_max_err(_np(clean["state"]), state) <= 4 * tol, variant
    return bank, lambda: bank.process(Xd), [Xd], check, ("in", "out")


def _welch_like(env, precision, which, finalize):
    """welch and csd at n = 512 (257 bins: an accumulator row is longer than the 256 bytes a truncated offset lands at), position 0"""
    from csd_ref import csd_density, csd_ref
    from test_gpu_csd import _peak_err as csd_err, _tol as csd_tol
    from test_gpu_welch import _peak_err as welch_err, _tol as welch_tol
    from welch_ref import welch_psd, welch_ref
    sd, torch = env.sd, env.torch
    n, hop, S = 512, 64, 512 + 9 * 64 + 30
    w = scipy.signal.get_window("hann", n)
    rng = _rng(which, precision)
    x = rng.standard_normal((CH, S)).astype(_npr(precision))
    wr = w.astype(x.dtype).astype(np.float64)
    xd = _dev(torch, x)
    pairs = [(0, 1), (1, 0)]
    if which == "welch":
        bank = sd.welch_bank(n, hop, CH, window=w, precision=_prec(sd, precision))
    else:
        bank = sd.csd_bank(n, hop, CH, pairs, window=w, precision=_prec(sd, precision))
    cplx = lambda t: _np(t).astype(np.float64)[:, 0::2] + 1j * _np(t).astype(np.float64)[:, 1::2]  # noqa: E731

    def check(clean):
        if which == "welch":
            acc, F, state = welch_ref(x, n, hop, wr, "constant", 0, None, None)
            assert F == 10
            if finalize:
                assert welch_err(_np(clean["out"]), welch_psd(acc, F, wr)) <= welch_tol(precision)
            else:
                assert welch_err(_np(clean["acc"]), acc) <= welch_tol(precision)
                assert np.array_equal(_np(clean["state"]), state.astype(x.dtype))
            return
        xy, au, F, state = csd_ref(x.astype(np.float64), pairs, n, hop, wr, "constant", 0, None, None, None)
        assert F == 10
        if finalize:
            assert csd_err(cplx(clean["out"].view(_rdt(torch, precision))), csd_density(xy, F, wr)) <= csd_tol(precision)
        else:
            assert csd_err(cplx(clean["acc_xy"]), xy) <= csd_tol(precision)
            assert csd_err(_np(clean["acc_auto"]), au) <= csd_tol(precision)
            assert np.array_equal(_np(clean["state"]), state.astype(x.dtype))
    if not finalize:
        return bank, lambda: bank.process(xd), [xd], check, ("in", "acc") if which == "welch" else ("in", "acc_xy", "acc_auto")
    bank.process(xd)
    if which == "welch":
        return bank, lambda: bank.psd(), [], check, ("acc", "out")
    return bank, lambda: bank.csd(), [], check, ("acc_xy", "acc_auto", "out")


def build_welch(env, precision, kind, variant):
    return _welch_like(env, precision, "welch", False) if variant == 0 else None


def build_welch_finalize(env, precision, kind, variant):
    return _welch_like(env, precision, "welch", True) if variant == 0 else None


def build_csd(env, precision, kind, variant):
    return _welch_like(env, precision, "csd", False) if variant == 0 else None


def build_csd_finalize(env, precision, kind, variant):
    return _welch_like(env, precision, "csd", True) if variant == 0 else None


PFB_TAPS = {"n32h3": (3, "time"), "n512h64": (1, "time")}


class _Pfb:
    """a polyphase analysis bank and its stream at a start position, shared by the stride cases and the position tests"""

    def __init__(self, env, precision, shape, cplx, phase, position, frames=None, seed="pfb"):
        sd = env.sd
        self.m, self.hop, F = STREAM_SHAPES[shape]
        self.F = frames or F
        self.p = PFB_TAPS[shape][0]
        self.phase, self.cplx, self.precision, self.position = phase, cplx, precision, position
        rng = _rng(seed, shape, cplx, precision)
        self.taps = rng.standard_normal(self.m * self.p)
        edt = (np.complex128 if precision == "f64" else np.complex64) if cplx else _npr(precision)
        self.x = _cplx(rng, (CH, self.F * self.hop), cplx).astype(edt)
        self.hist = _cplx(rng, (CH, self.m * self.p - self.hop), cplx).astype(edt)
        self.bank = sd.pfb_bank(self.m, self.p, self.hop, streams=CH, taps=self.taps, input="complex" if cplx else "real", phase=phase,
                                precision=_prec(sd, precision))
        self.start(env.torch, position)

    def start(self, torch, position):
        self.bank._state = _dev(torch, self.hist)
        self.bank._position = position

    def want(self, position=None):
        from pfb_ref import pfb_ref
        taps_p = self.taps.astype(_npr(self.precision)).astype(np.float64)
        return pfb_ref(self.x, self.m, self.p, self.hop, taps_p, self.hist, self.phase, self.position if position is None else position)

    def check(self, out, state, position=None):
        from test_gpu_pfb import _err, _tol
        want, want_state = self.want(position)
        err = _err(out.reshape(want.shape), want)
        assert err <= _tol(self.precision, self.m * self.p), (err, _tol(self.precision, self.m * self.p))
        assert np.array_equal(state.reshape(want_state.shape), want_state.astype(self.x.dtype))


def build_pfb(env, precision, kind, variant):
    shape, var = kind.split("-")
    s = _Pfb(env, precision, shape, var == "complex", PFB_TAPS[shape][1], 7 * STREAM_SHAPES[shape][1])
    if not _set_variant(s.bank, variant):
        return None
    xd = _dev(env.torch, s.x)
    return s.bank, lambda: s.bank.process(xd), [xd], lambda clean: s.check(_np(clean["out"]), _np(clean["state"])), ("in", "out")


class _PfbSynth:
    def __init__(self, env, precision, shape, cplx, phase, position, frames=None, seed="synth"):
        from pfb_synth_ref import pfb_synth_frames_ref
        sd = env.sd
        self.m, self.hop, F = STREAM_SHAPES[shape]
        self.F = frames or F
        self.p = PFB_TAPS[shape][0]
        self.phase, self.cplx, self.precision, self.position = phase, cplx, precision, position
        self.bins = self.m if cplx else self.m // 2 + 1
        rng = _rng(seed, shape, cplx, precision)
        self.g = rng.uniform(-1, 1, self.m * self.p)
        cdt = np.complex128 if precision == "f64" else np.complex64
        self.X = _cplx(rng, (CH, self.F, self.bins), True).astype(cdt)
        self.vmax = float(np.abs(pfb_synth_frames_ref(self.X, self.m, self.p, self.hop, phase, position, cplx)).max())
        pend = rng.uniform(-1, 1, (CH, self.m * self.p - self.hop))
        if cplx:
            pend = (pend + 1j * rng.uniform(-1, 1, pend.shape)) / np.sqrt(2)
        self.pend = (pend * self.vmax).astype(cdt if cplx else _npr(precision))
        self.bank = sd.pfb_synthesis_bank(self.m, self.p, self.hop, streams=CH, taps=self.g, output="complex" if cplx else "real", phase=phase,
                                          precision=_prec(sd, precision))
        self.start(env.torch, position)

    def start(self, torch, position):
        self.bank._state = _dev(torch, self.pend)
        self.bank._position = position

    def check(self, out, state, position=None):
        from pfb_synth_ref import pfb_synth_ref
        from test_gpu_pfb_synth import _bound
        g_p = self.g.astype(_npr(self.precision)).astype(np.float64)
        want, want_state = pfb_synth_ref(self.X, self.m, self.p, self.hop, g_p, self.pend, self.phase,
                                         self.position if position is None else position, cplx=self.cplx)
        err = max(np.abs(out - want).max(), np.abs(state.reshape(want_state.shape) - want_state).max())
        bound = _bound(self.precision, self.m, self.p, self.hop, self.vmax)
        assert err <= bound, (err, bound)


def build_pfb_synth(env, precision, kind, variant):
    shape, var = kind.split("-")
    s = _PfbSynth(env, precision, shape, var == "complex", PFB_TAPS[shape][1], 7 * STREAM_SHAPES[shape][1])
    if not _set_variant(s.bank, variant):
        return None
    Xd = _dev(env.torch, s.X)
    return s.bank, lambda: s.bank.process(Xd), [Xd], lambda clean: s.check(_np(clean["out"]), _np(clean["state"])), ("in", "out")


def build_ddc(env, precision, kind, variant):
    import test_gpu_ddc as t
    from ddc_ref import ddc_ref
    cplx = kind == "complex"
    taps, down = 17, 4
    rng = _rng("ddc", precision, kind)
    h = rng.standard_normal(taps)
    bands = [(1, F1, 5), (0, F2, 0)]
    position = ((1 << 33) + 12345) * down
    block = t._bank(env.sd, h, down, bands, CH, precision, cplx).info()["block_out"]
    S = (2 * block + 197) * down
    x = t._rand(rng, (CH, S), precision, cplx)
    hist = t._rand(rng, (CH, taps - 1), precision, cplx)
    bank = t._bank(env.sd, h, down, bands, CH, precision, cplx, variant, hist, position)
    xd = _dev(env.torch, x)

    def check(clean):
        want, want_state = ddc_ref(h, x, down, bands, position, hist, precision)
        assert np.array_equal(_np(clean["out"]), want) and np.array_equal(_np(clean["state"]), want_state), variant
    return bank, lambda: bank.process(xd), [xd], check, ("in", "out")


def build_duc(env, precision, kind, variant):
    import test_gpu_duc as t
    from duc_ref import duc_ref, hist_len
    taps, up = 17, 4
    rng = _rng("duc", precision, kind)
    h = rng.standard_normal(taps)
    bands = [(1, F1, 5), (0, F2, 0)]
    position = (1 << 33) + 12345
    block = t._bank(env.sd, h, up, bands, CH, precision, kind).info()["block_in"]
    S = 2 * block + 197
    x = t._rand(rng, (len(bands), S), precision)
    hist = t._rand(rng, (len(bands), max(hist_len(taps, up), 1)), precision)
    bank = t._bank(env.sd, h, up, bands, CH, precision, kind, variant, hist, position)
    xd = _dev(env.torch, x)

    def check(clean):
        want, want_state = duc_ref(h, x, up, bands, CH, kind, position, hist[:, :hist_len(taps, up)], precision)
        got = _np(clean["out"])
        assert got.dtype == want.dtype and np.array_equal(got, want), variant
        assert np.array_equal(_np(clean["state"]), want_state), variant
    return bank, lambda: bank.process(xd), [xd], check, ("in", "out")


def build_arb(env, precision, kind, variant):
    import test_gpu_arb as t
    from arb_ref import arb_ref, step_of
    cplx = kind == "complex"
    L, T, step = 4, 5, step_of(0.7317)
    rng = _rng("arb", precision, kind)
    h = rng.standard_normal(L * T)
    block = t._bank(env.sd, h, L, T, step, precision, cplx, "linear").info()["block_out"]
    S = int((2 * block + 197) * step >> 32) + 1
    x = t._rand(rng, (CH, S), precision, cplx)
    hist = t._rand(rng, (CH, T - 1), precision, cplx)
    time0 = 12345
    bank = t._bank(env.sd, h, L, T, step, precision, cplx, "linear", variant, hist, step, time0)
    xd = _dev(env.torch, x)

    def check(clean):
        want, want_state, _ = arb_ref(h, L, T, x, step, time0, hist, "linear", precision)
        assert want.shape[1] >= 160
        assert np.array_equal(_np(clean["out"]), want) and np.array_equal(_np(clean["state"]), want_state), variant
    return bank, lambda: bank.process(xd), [xd], check, ("in", "out")


def _cic_geometry(kind):
    """int32 samples; 16 significant bits keep the registers at 32 (int32 out), 32 bits need 64 (int64 out)"""
    N, R, M = 3, 5, 1
    return N, R, M, {"i32-i32": 16, "i32-i64": 32}[kind]


def build_cic(env, precision, kind, variant):
    import test_gpu_cic as t
    from cic_ref import cic_ref, reg_bits
    sd, torch = env.sd, env.torch
    N, R, M, in_bits = _cic_geometry(kind)
    W = reg_bits(in_bits, N, R, M)
    assert W == (32 if kind == "i32-i32" else 64)
    rng = _rng("cic", kind)
    chunk = sd.cic_decimator(N, R, M).info()["chunk"]
    S, position = 5 * chunk + 37 + 160 * R, (1 << 33) + R + 3
    x = t._rand(rng, (CH, S), in_bits, "i32")
    state = t._rand(rng, (CH, N * M * R), in_bits, "i32")
    bank = t._bank(sd, torch, N, R, M, False, "i32", in_bits, "int", variant, 1, state, position)
    xd = _dev(torch, x)

    def check(clean):
        want, want_state = cic_ref(x, N, R, M, W, position, state, "int")
        assert want.shape[1] >= 160 and want.dtype == (np.int32 if W == 32 else np.int64)
        assert _same(_np(clean["out"]), want) and _same(_np(clean["state"]), want_state), variant
    return bank, lambda: bank.process(xd), [xd], check, ("in", "out")


def build_cic_interp(env, precision, kind, variant):
    import test_gpu_cic_interp as t
    from cic_interp_ref import cic_interp_ref, reg_bits
    sd, torch = env.sd, env.torch
    N, R, M, in_bits = _cic_geometry(kind)
    W = reg_bits(in_bits, N, R, M)
    assert W == (32 if kind == "i32-i32" else 64), W
    rng = _rng("cici", kind)
    chunk = sd.cic_interpolator(N, R, M).info()["chunk"]
    S = t._inputs(chunk, R) + 160
    x = t._rand(rng, (CH, S), in_bits, "i32")
    state = t._rand(rng, (CH, N * M), in_bits, "i32")
    bank = t._bank(sd, torch, N, R, M, False, "i32", in_bits, "int", variant, 1, state)
    xd = _dev(torch, x)

    def check(clean):
        want, want_state = cic_interp_ref(x, N, R, M, W, state, "int")
        assert _same(_np(clean["out"]), want) and _same(_np(clean["state"]), want_state), variant
    return bank, lambda: bank.process(xd), [xd], check, ("in", "out")


def build_beam(env, precision, kind, variant):
    """one group of two sensors, two beams: `in` and `out` both have two rows"""
    import test_gpu_beam as t
    from beam_ref import beam_ref, hist_len
    cplx = kind == "complex"
    n_taps, sensors, beams, groups = 5, 2, 2, 1
    rng = _rng("beam", precision, kind)
    ent = [(0, 0, 0, t._taps(rng, n_taps, cplx)), (0, 1, 7, t._taps(rng, n_taps, cplx)), (1, 0, 3, t._taps(rng, n_taps, cplx)),
           (1, 1, 1, t._taps(rng, n_taps, cplx))]
    H = hist_len(ent, n_taps)
    S = 2 * t._bank(env.sd, ent, sensors, beams, n_taps, groups, precision, cplx).info()["block_out"] + 197
    x = t._rand(rng, (sensors, S), precision, cplx)
    hist = t._rand(rng, (sensors, H), precision, cplx)
    bank = t._bank(env.sd, ent, sensors, beams, n_taps, groups, precision, cplx, variant, hist)
    xd = _dev(env.torch, x)

    def check(clean):
        want, want_state = beam_ref(ent, x, sensors, beams, n_taps, groups, hist, precision)
        assert _same(_np(clean["out"]), want) and _same(_np(clean["state"]), want_state), variant
    return bank, lambda: bank.process(xd), [xd], check, ("in", "out")


def build_lms(env, precision, kind, variant):
    import test_gpu_lms as t
    from lms_ref import lms_ref
    cplx = kind == "complex"
    T, mode = 7, "nlms"
    mu, eps = t._step(mode, T)
    rng = _rng("lms", precision, kind)
    S = 2 * t._bank(env.sd, T, precision, cplx, mode, channels=CH).info()["block"] + 197
    x, d = t._rand(rng, (CH, S), precision, cplx), t._rand(rng, (CH, S), precision, cplx)
    w0, h0 = t._rand(rng, (CH, T), precision, cplx, 0.1), t._rand(rng, (CH, T - 1), precision, cplx)
    bank = t._bank(env.sd, T, precision, cplx, mode, variant, w0, h0, channels=CH)
    xd, dd = _dev(env.torch, x), _dev(env.torch, d)

    def check(clean):
        want = lms_ref(x, d, T, mu, mode, eps, w0, h0, precision)
        assert _same(_np(clean["y"]), want[0]) and _same(_np(clean["e"]), want[1]), variant
        state = _np(clean["state"]).reshape(-1)
        assert _same(state[:CH * T].reshape(CH, T), want[2]) and _same(state[CH * T:].reshape(CH, T - 1), want[3]), variant
    return bank, lambda: bank.process(xd, dd, mu), [xd, dd], check, ("x", "d", "y", "e")


def build_rank(env, precision, kind, variant):
    import test_gpu_rank as t
    from rank_ref import rank_ref
    W, r = 9, 4
    rng = _rng("rank", precision)
    S = 3 * t._bank(env.sd, W, r, precision, channels=CH).info()["block"] + 165
    x, h0 = t._rand(rng, (CH, S), precision), t._rand(rng, (CH, W - 1), precision)
    bank = t._bank(env.sd, W, r, precision, variant, h0, channels=CH)
    xd = _dev(env.torch, x)

    def check(clean):
        want = rank_ref(x, W, r, h0)
        assert _same(_np(clean["y"]), want[0]) and _same(_np(clean["state"]).reshape(want[1].shape), want[1]), variant
    return bank, lambda: bank.process(xd), [xd], check, ("x", "y")


def build_cfar(env, precision, kind, variant):
    import test_gpu_cfar as t
    from cfar_ref import cfar_ref, geometry
    mode, iq = kind.split("-")
    L, G = 7, 3
    _, W, _ = geometry(L, G)
    rng = _rng("cfar", precision, kind)
    rank = 5 if mode == "os" else None
    info = t._bank(env.sd, CH, L, G, mode, precision, iq, rank=rank).info()
    S = 2 * t._unit(info, W) + 197
    x, h0 = t._rows(rng, (CH, S), precision, iq), t._rows(rng, (CH, W - 1), precision, iq)
    bank = t._bank(env.sd, CH, L, G, mode, precision, iq, variant, rank, hist=h0)
    xd = _dev(env.torch, x)

    def check(clean):
        want = cfar_ref(x, L, G, mode, t.ALPHA, rank, h0)
        assert _same(_np(clean["thr"]), want[0]) and _same(_np(clean["det"]), want[1]), variant
        assert _same(_np(clean["state"]).reshape(h0.shape), t._hist_after(x, h0)), variant
    return bank, lambda: bank.process(xd), [xd], check, ("x", "thr", "det")


def build_pll(env, precision, kind, variant):
    import test_gpu_pll as t
    from pll_ref import pll_ref, real_dtype
    rng = _rng("pll", precision, kind)
    fcw, th0 = t._words(rng, CH), t._words(rng, CH)
    i0 = rng.uniform(-t.MAX_DEV, t.MAX_DEV, CH).astype(real_dtype(precision))
    S = 2 * t._bank(env.sd, fcw, precision, kind, channels=CH).info()["block"] + 197
    x = t._rand(rng, (CH, S), precision)
    bank = t._bank(env.sd, fcw, precision, kind, variant, i0, th0, channels=CH)
    bank._ensure_state()
    xd = _dev(env.torch, x)

    def check(clean):
        want = pll_ref(x, fcw, t.ALPHA, t.BETA, kind, t.MAX_DEV, i0, th0, precision)
        for name, w in zip(("y", "err", "freq"), want):
            assert _same(_np(clean[name]), w), (name, variant)
        rb = CH * np.dtype(real_dtype(precision)).itemsize
        raw = _np(clean["state"]).reshape(-1)
        assert _same(raw[:rb].view(real_dtype(precision)), want[3]) and _same(raw[rb:rb + 4 * CH].view(np.uint32), want[4]), variant
    return bank, lambda: bank.process(xd, t.ALPHA, t.BETA, want_err=True, want_freq=True), [xd], check, ("x", "y", "err", "freq")


def build_timing(env, precision, kind, variant):
    import test_gpu_timing as t
    from timing_ref import state_bytes_of, step_of, timing_ref
    L, T, sps = 4, 5, 2.37
    rng = _rng("timing", precision, kind)
    h = t._taps(rng, L, T)
    step0 = step_of(sps)
    st0 = timing_ref(h, L, T, t._rand(rng, (CH, 9), precision), step0, t.ALPHA, t.BETA, kind, t.MAX_DEV, None, precision)[4]
    S = 5 * t._bank(env.sd, env.torch, h, L, sps, precision, kind, channels=CH).info()["block"] + 37 + 480  # at least 160 strobes per row
    x = t._rand(rng, (CH, S), precision)
    bank = t._bank(env.sd, env.torch, h, L, sps, precision, kind, variant, st0, channels=CH)
    xd = _dev(env.torch, x)

    def check(clean):
        want = timing_ref(h, L, T, x, step0, t.ALPHA, t.BETA, kind, t.MAX_DEV, st0, precision)
        assert int(want[3].min()) >= 160
        t._check(bank, (clean["y"], clean["err"], clean["period"], clean["counts"].reshape(-1)), want, (precision, kind, variant), state=False)
        assert _np(clean["state"]).tobytes() == state_bytes_of(want[4]), variant
    return (bank, lambda: bank.process(xd, t.ALPHA, t.BETA, want_err=True, want_period=True), [xd], check,
            ("x", "y", "err", "period"))


BOTH = ("f32", "f64")
STREAM_KINDS = tuple(f"{s}-{v}" for s in STREAM_SHAPES for v in ("real", "complex"))
# entry (without the sdsp_hip_ prefix) -> (builder, precisions, kinds, the strided buffers that go wide)
CASES = {
    "iir_process": (build_iir, BOTH, ("",), ("data",)),
    "iir_process_interleaved": (build_iir_interleaved, BOTH, ("",), ("data",)),
    "fir_process": (build_fir, BOTH, ("direct", "fft"), ("data",)),
    "filtfilt_process": (build_filtfilt, BOTH, ("",), ("data",)),
    "resample_process": (build_resample, BOTH, ("",), ("in", "out")),
    "stft_process": (build_stft, BOTH, tuple(f"{s}-{o}" for s in STREAM_SHAPES for o in ("complex", "power")), ("in", "out")),
    "istft_process": (build_istft, BOTH, tuple(STREAM_SHAPES), ("in", "out")),
    "welch_process": (build_welch, BOTH, ("",), ("in", "acc")),
    "welch_finalize": (build_welch_finalize, BOTH, ("",), ("acc", "out")),
    "csd_process": (build_csd, BOTH, ("",), ("in", "acc_xy", "acc_auto")),
    "csd_finalize": (build_csd_finalize, BOTH, ("",), ("acc_xy", "acc_auto", "out")),
    "pfb_process": (build_pfb, BOTH, STREAM_KINDS, ("in", "out")),
    "pfb_synth_process": (build_pfb_synth, BOTH, STREAM_KINDS, ("in", "out")),
    "ddc_process": (build_ddc, BOTH, ("real", "complex"), ("in", "out")),
    "duc_process": (build_duc, BOTH, ("complex", "real"), ("in", "out")),
    "arb_process": (build_arb, BOTH, ("real", "complex"), ("in", "out")),
    "cic_process": (build_cic, ("int",), ("i32-i32", "i32-i64"), ("in", "out")),
    "cic_interp_process": (build_cic_interp, ("int",), ("i32-i32", "i32-i64"), ("in", "out")),
    "beam_process": (build_beam, BOTH, ("real", "complex"), ("in", "out")),
    "lms_process": (build_lms, BOTH, ("real", "complex"), ("x", "d", "y", "e")),
    "rank_process": (build_rank, BOTH, ("",), ("x", "y")),
    "cfar_process": (build_cfar, BOTH, ("ca-power", "go-iq", "os-power"), ("x", "thr", "det")),
    "pll_process": (build_pll, BOTH, ("cross", "qpsk"), ("x", "y", "err", "freq")),
    "timing_process": (build_timing, BOTH, ("gardner", "zc_qpsk"), ("x", "y", "err", "period")),
}
# stride parameters that are exercised inside another entry's case (its check calls them with the compact and with the wide stride)
ALSO_COVERED = {("sdsp_hip_iir_plan_kernel", "stride"): "iir_process", ("sdsp_hip_filtfilt_plan_kernel", "stride"): "filtfilt_process"}
STAGED = "stages the whole span of its rows through host memory: a wide stride means a 16 GiB copy"
EXCLUDED = {f"sdsp_hip_{name}_host": STAGED for name in (
    "iir_process", "fir_process", "resample_process", "stft_process", "istft_process", "filtfilt_process", "welch_process", "welch_finalize",
    "csd_process", "csd_finalize", "pfb_process", "pfb_synth_process", "ddc_process", "duc_process", "arb_process", "cic_process",
    "cic_interp_process", "beam_process", "lms_process", "rank_process", "cfar_process", "pll_process", "timing_process")}


def test_every_stride_parameter_is_covered():
    """no GPU work: every uint64_t *stride parameter of include/sdsp_hip.h is in the case table or in
    the exclusion table, and the exclusion table holds host-staged entries only"""
    found = _stride_parameters()
    assert len(found) >= 64
    table = []
    for entry, sname in found:
        short = entry[len("sdsp_hip_"):]
        if entry in EXCLUDED:
            assert entry.endswith(("_host", "_sharded")), entry
            table.append((entry, sname, "excluded: " + EXCLUDED[entry]))
        elif (entry, sname) in ALSO_COVERED:
            assert ALSO_COVERED[entry, sname] in CASES
            table.append((entry, sname, "called with the wide stride in the case of " + ALSO_COVERED[entry, sname]))
        else:
            assert short in CASES, (entry, sname, "neither a case nor an exclusion")
            assert _buffer_of(entry, sname) in CASES[short][3], (entry, sname, "no case puts this buffer wide")
            table.append((entry, sname, f"case: '{_buffer_of(entry, sname)}' goes wide"))
    for entry, sname, how in table:
        print(f"{entry}({sname}): {how}")
    for short, (_, _, _, wide) in CASES.items():  # and nothing in the tables that the header does not have
        for name in wide:
            assert ("sdsp_hip_" + short, _stride_of("sdsp_hip_" + short, name)) in found, (short, name)
    assert set(EXCLUDED) <= {e for e, _ in found}


class _Env:
    pass


@pytest.fixture(scope="module")
def env(sd, torch_cuda, request):
    e = _Env()
    e.sd, e.torch, e.lib = sd, torch_cuda, sd.load()
    e.request = request
    return e


def _all_cases():
    return [pytest.param(short, prec, kind, id="-".join(filter(None, (short, kind, prec))))
            for short, (_, precs, kinds, _) in CASES.items() for prec in precs for kind in kinds]


@gpu
@pytest.mark.parametrize("short,precision,kind", _all_cases())
def test_wide_strides(env, wide_arena, oracle, short, precision, kind):
    """items 1 to 3 of the module docstring, for every kernel variant the plan takes"""
    env.oracle = oracle
    build, _, _, wide = CASES[short]
    takes, refused = VARIANTS.get(short, ((0, 1), ()))
    ran = []
    for variant in (range(4) if takes is None else (*takes, *refused)):
        built = build(env, precision, kind, variant)
        if built is None:  # the builder has checked how the variant was refused
            assert takes is None or variant in refused, (short, variant, "a variant the entry documents did not build")
            continue
        assert variant not in refused, (short, variant)
        assert built[4] == wide, (built[4], wide)
        _drive(env.torch, wide_arena, "sdsp_hip_" + short, built, f"{short} {kind} {precision} variant {variant}")
        ran.append(variant)
    print(f"{short} {kind} {precision}: variants {ran}")
    assert (ran == list(takes)) if takes is not None else (ran[:1] == [0]), (short, ran)
    DRIVEN.add((short, precision, kind))


DRIVEN = set()  # the cases of test_wide_strides that ran to their end in this session
# entry -> (the variants its *_plan_set_variant takes, values just past them whose refusal the builder checks); (0, 1) where not named.
# None: the bank's variants are its inner transform plan's -- 0 always, the others where that plan has such a kernel (_set_variant)
VARIANTS = {"iir_process": ((0, 1, 2, 3), ()), "iir_process_interleaved": ((0, 1, 2), (3,)), "fir_process": ((0, 1, 2, 3), ()),
            "resample_process": ((0, 1, 2), (3,)), "welch_process": ((0,), ()), "welch_finalize": ((0,), ()), "csd_process": ((0,), ()),
            "csd_finalize": ((0,), ()), "stft_process": (None, ()), "istft_process": (None, ()), "pfb_process": (None, ()),
            "pfb_synth_process": (None, ())}


@gpu
def test_summary():
    """prints, per entry and buffer, what the cases above saw (pytest -s).  When every case of test_wide_strides ran before it, every
    (entry, buffer) of the case table must have been seen; after a selection of them (-k) it reports that selection only"""
    for (entry, name), seen in sorted(RESULTS.items()):
        what = "computes at wide strides" if seen == {0} else f"refuses: {sorted(seen)}"
        print(f"{entry} '{name}': {what}")
    assert all(seen == {0} or (entry, _stride_of(entry, name)) in REFUSALS for (entry, name), seen in RESULTS.items())
    if len(DRIVEN) == len(_all_cases()):
        assert set(RESULTS) == {("sdsp_hip_" + short, name) for short, (_, _, _, wide) in CASES.items() for name in wide}
    else:
        print(f"only {len(DRIVEN)} of {len(_all_cases())} cases ran in this session: the table above is partial")


# ------------------------------------------------------------------ stream positions past 2^32

POS_SHAPES = ("n32h3", "n512h64")


def _positions(hop):
    """start positions of the polyphase banks, which take any position (samples of the stream before the call): five hops before 2^32
    (the position crosses 2^32 inside the call and inside a two-call split), 2^40 + 7 (a frame rotation that is no multiple of the
    hop), and 2^40 + 7 hop"""
    return [(1 << 32) - 5 * hop, (1 << 40) + 7, (1 << 40) + 7 * hop]


def _welch_alias_differs(n, hop, position, samples):
    """whether a position truncated to 32 bits would move the segments of a call of `samples` samples: another count or another
    first-segment offset (computed with the reference's own rule alone)"""
    from welch_ref import welch_frames

    def framing(p):
        first = 0 if p < n else (p - n) // hop + 1  # index of the first segment that ends after position p
        return welch_frames(n, hop, p, samples), first * hop - p  # the count, and where that segment starts relative to the call
    return framing(position) != framing(position % (1 << 32))


def test_truncated_positions_would_move_the_segments():
    """no GPU work: the Welch and csd position cases can fail.  Hop 3 does not divide 2^32, so the low 32 bits of a position past
    2^32 frame differently; hop 64 divides it, and there only positions that are no multiple of 64 past a segment end can tell"""
    for shape in POS_SHAPES:
        n, hop, _ = STREAM_SHAPES[shape]
        S = _welch_samples(shape)
        for position in _welch_positions(shape):
            if position >= 1 << 32:
                assert _welch_alias_differs(n, hop, position, S), (shape, position)
            else:  # the call that starts past 2^32 in the second of the two splits
                cut = _welch_cuts(hop)[1]
                assert position + cut >= 1 << 32 and _welch_alias_differs(n, hop, position + cut, S - cut), (shape, position, cut)


def _welch_cuts(hop):
    """where the two splits cut a stream that starts five hops before 2^32: the second call starts before 2^32 and ends past it, or
    starts past it"""
    return (2 * hop + 1, 7 * hop + 1)


def _welch_samples(shape):
    n, hop, _ = STREAM_SHAPES[shape]
    return 12 * hop + hop // 2


def _welch_positions(shape):
    """2^32 - 5 hop, and 2^40 + 7 -- moved up to the first position whose low-32-bit alias frames differently where it does not (hop
    64 divides 2^32 and 2^40: the alias of 2^40 + 7 is 7, below n, where no segment is complete yet, which differs already)"""
    n, hop, _ = STREAM_SHAPES[shape]
    out = [(1 << 32) - 5 * hop]
    p = (1 << 40) + 7
    while not _welch_alias_differs(n, hop, p, _welch_samples(shape)):
        p += 1
    return out + [p]


@gpu
@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("shape", POS_SHAPES)
@pytest.mark.parametrize("which", ["welch", "csd"])
def test_welch_and_csd_positions_past_32_bits(env, which, shape, precision):
    """one call and two two-call splits at each start position, against the reference at that position"""
    from csd_ref import csd_ref
    from test_gpu_csd import _peak_err as csd_err, _tol as csd_tol
    from test_gpu_welch import _peak_err as welch_err, _tol as welch_tol
    from welch_ref import welch_frames, welch_ref
    sd, torch = env.sd, env.torch
    n, hop, _ = STREAM_SHAPES[shape]
    S = _welch_samples(shape)
    w = scipy.signal.get_window("hann", n)
    rng = _rng(which, shape, precision, "pos")
    x = rng.standard_normal((CH, S)).astype(_npr(precision))
    hist = rng.standard_normal((CH, n - 1)).astype(_npr(precision))
    wr = w.astype(x.dtype).astype(np.float64)
    pairs = [(0, 1), (1, 0)]
    cplx = lambda t: _np(t).astype(np.float64)[..., 0] + 1j * _np(t).astype(np.float64)[..., 1]  # noqa: E731
    for position in _welch_positions(shape):
        crosses = position < (1 << 32) <= position + S
        assert crosses or position > 1 << 40
        if which == "welch":
            acc, F, state = welch_ref(x, n, hop, wr, "constant", position, hist, None)
        else:
            xy, au, F, state = csd_ref(x.astype(np.float64), pairs, n, hop, wr, "constant", position, hist, None, None)
        assert F == welch_frames(n, hop, position, S) >= 10
        for cut in (S, *_welch_cuts(hop)):
            if which == "welch":
                bank = sd.welch_bank(n, hop, CH, window=w, precision=_prec(sd, precision))
            else:
                bank = sd.csd_bank(n, hop, CH, pairs, window=w, precision=_prec(sd, precision))
            bank._ensure_plan()
            bank._ensure_buffers()
            bank._state.copy_(_dev(torch, hist))
            bank.position = position
            xd = _dev(torch, x)
            got = bank.process(xd[:, :cut].contiguous())
            if cut < S:
                assert not crosses or (bank.position < 1 << 32) == (cut == _welch_cuts(hop)[0])
                got += bank.process(xd[:, cut:].contiguous())
            assert got == F and bank.position == position + S, (position, cut, got, F)
            tag = (which, shape, precision, position, cut)
            assert np.array_equal(_np(bank._state), state.astype(x.dtype)), tag
            if which == "welch":
                err, tol = welch_err(_np(bank._acc), acc), welch_tol(precision)
            else:
                err = max(csd_err(cplx(bank._acc_xy), xy), csd_err(_np(bank._acc_auto), au))
                tol = csd_tol(precision)
            print(f"{tag}: {err:.3e} (bound {tol:.3e})")
            assert err <= tol, (tag, err, tol)


@gpu
@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("phase", ["time", "frame"])
@pytest.mark.parametrize("shape", POS_SHAPES)
@pytest.mark.parametrize("which", ["pfb", "pfb_synth"])
def test_polyphase_positions_past_32_bits(env, which, shape, phase, cplx, precision):
    """one call and two two-call splits (the second call starts before 2^32, or past it) at each start position against the reference
    at that position; and, m being a power of two, the same bits as at the position's low 32 bits"""
    torch = env.torch
    m, hop, _ = STREAM_SHAPES[shape]
    assert m & (m - 1) == 0
    for position in _positions(hop):
        s = (_Pfb if which == "pfb" else _PfbSynth)(env, precision, shape, cplx, phase, position, frames=12, seed=which + "pos")
        data = _dev(torch, s.x if which == "pfb" else s.X)
        per = hop if which == "pfb" else 1  # columns (pfb) or frames (pfb_synth) of `data` per frame
        runs = {}
        for label, start, cut in (("one call", position, 12), ("two calls", position, 2), ("two calls, the second past 2^32", position, 7),
                                  ("low 32 bits", position % (1 << 32), 12)):
            s.start(torch, start)
            parts = [s.bank.process(data[:, :cut * per].contiguous())]
            if cut < 12:
                assert position > 1 << 40 or (s.bank._position < 1 << 32) == (cut == 2)
                parts.append(s.bank.process(data[:, cut * per:].contiguous()))
            out = torch.cat(parts, dim=1)
            runs[label] = (out, s.bank._state.clone())
            if label != "low 32 bits":
                assert s.bank._position == position + 12 * hop
                s.check(_np(out), _np(s.bank._state), position)
        for label in ("two calls", "two calls, the second past 2^32", "low 32 bits"):
            assert arena.same_bits(runs[label][0], runs["one call"][0]), (which, shape, phase, cplx, precision, position, label)
            assert arena.same_bits(runs[label][1], runs["one call"][1]), (position, label, "state")
