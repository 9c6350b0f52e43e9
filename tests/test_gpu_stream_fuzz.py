"""The seeded random cross-check of tests/stream_fuzz.py on a real MI355X: three committed seeds of twelve cases per plan family.

One test per (family, seed) runs checks (a) to (f) of stream_fuzz.check_case on every case: one call against the family's numpy
reference, two independently drawn splits against the one call, every kernel variant against variant 0, the sentinels of every padded
row, and a subset of the optional outputs against the full call.  A refused case is a failure; nothing is skipped.  After a HIP
runtime error the driver stops (stream_fuzz.GPU_STOPPED) and every later test of this module fails at once without touching the GPU.
The last test holds the cases that ran to the coverage list of stream_fuzz.coverage_gaps.  A failure line names family, seed and
index: `python tests/stream_fuzz.py --seed S --family F --case I` rebuilds that case alone."""
import time

import pytest

import stream_fuzz as sf

pytestmark = pytest.mark.gpu

SEEN = {}   # family -> the cases that ran to their end in this session
RAN = {}    # (family, seed) -> (cases run, seconds)


@pytest.fixture(scope="module")
def env():
    assert not sf.GPU_STOPPED, sf.GPU_STOPPED
    return sf.gpu_env()


def _stopped():
    assert not sf.GPU_STOPPED, f"the driver stopped on a GPU error, nothing more is started: {sf.GPU_STOPPED[0]}"


@pytest.mark.parametrize("seed", sf.SEEDS)
@pytest.mark.parametrize("family", sorted(sf.FAMILIES))
def test_cases(request, family, seed):
    _stopped()
    env = request.getfixturevalue("env")
    t0 = time.perf_counter()
    ran, failures = sf.run_cases(env, seed, sf.CASES, [family], seen=SEEN)
    RAN[family, seed] = (ran, time.perf_counter() - t0)
    assert not failures, f"{len(failures)} failing check(s); the first: {failures[0]}"
    assert ran == sf.CASES, (family, seed, ran)


def test_coverage():
    """over the cases that ran: every variant, precision, kind and mode of every family, every forced kind of call, channel counts on
    both sides of 64, every start state, totals below, at and above the plan's unit, and for the LMS bank its four tap bounds on and
    off the bound.  After a selection (-k) it reports that selection only"""
    _stopped()
    for (family, seed), (ran, seconds) in sorted(RAN.items()):
        print(f"{family} seed {seed}: {ran} cases in {seconds:.2f} s")
    gaps = [g for family, cases in SEEN.items() for g in sf.coverage_gaps(family, cases)]
    for g in gaps:
        print(g)
    everything = {(f, s) for f in sf.FAMILIES for s in sf.SEEDS}
    if set(RAN) == everything and all(ran == sf.CASES for ran, _ in RAN.values()):
        assert sum(len(c) for c in SEEN.values()) == len(everything) * sf.CASES
        assert not gaps, gaps
        lms = {(c["bound"], c["on_bound"]) for c in SEEN["lms"]}  # also among the gaps: Lms.crosses
        assert lms == {(b, on) for b in (8, 16, 32, 64) for on in (True, False)}, sorted(lms)
        for family in ("stft", "istft", "pfb", "pfb_synth"):  # the inner transform's variant 1 as APPLIED, not as drawn
            applied = sf.VARIANT_APPLIED.get(family, set())
            print(f"{family}: (precision, requested, applied) inner-transform variants: {sorted(applied)}")
            for precision in ("f32", "f64"):
                assert {a for p, _, a in applied if p == precision} == {0, 1}, (family, precision, sorted(applied))
        slow = max(RAN, key=lambda k: RAN[k][1])
        print(f"{sum(len(c) for c in SEEN.values())} cases, {sum(s for _, s in RAN.values()):.1f} s in all; the slowest (family, seed): "
              f"{slow} {RAN[slow][1]:.2f} s")
    else:
        print(f"only {len(RAN)} of {len(everything)} (family, seed) tests ran in this session: the coverage above is partial")
