"""tests/stream_fuzz.py without a GPU: the draws are deterministic and stay inside the limits of include/sdsp_hip.h, their weights reach
every axis value within the committed seeds, and the driver's check functions report planted defects.

The banks here are stream_fuzz.StandIn: a family's numpy reference behind the session protocol the HIP banks are driven through, on
CPU tensors.  The undamaged stand-in passes every committed case; each planted defect is reported under the check letter meant for it,
with the case line, and the values of that line rebuild the case through the command line."""
import contextlib
import io
import re
import time

import pytest

import stream_fuzz as sf

FAMILY_NAMES = sorted(sf.FAMILIES)


def _draws(family):
    return [(seed, i, sf.draw_case(seed, family, i)) for seed in sf.SEEDS for i in range(sf.CASES)]


def test_draws_are_deterministic_and_independent_of_the_other_families():
    for family in FAMILY_NAMES:
        for seed in sf.SEEDS:
            alone = [sf.draw_case(seed, family, i) for i in range(sf.CASES)]
            assert alone == [sf.draw_case(seed, family, i) for i in range(sf.CASES)]
    # drawn among all of them, in another order and with other counts: the same dicts
    among = {}
    for i in reversed(range(sf.CASES + 3)):
        for family in reversed(FAMILY_NAMES):
            among[family, i] = sf.draw_case(sf.SEEDS[0], family, i)
    for family in FAMILY_NAMES:
        for i in range(sf.CASES):
            assert among[family, i] == sf.draw_case(sf.SEEDS[0], family, i), (family, i)
    assert sf.draw_case(sf.SEEDS[0], FAMILY_NAMES[0], 0) != sf.draw_case(sf.SEEDS[1], FAMILY_NAMES[0], 0)


def test_a_case_is_plain_data_on_one_line():
    for family in FAMILY_NAMES:
        for _, _, case in _draws(family):
            text = repr(case)
            assert "\n" not in text and "array(" not in text and "np." not in text, text
            assert eval(text) == case  # ints, floats, strings, lists and dicts of them only


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_every_draw_is_inside_the_header_limits(family):
    fam = sf.FAMILIES[family]
    for seed, i, case in _draws(family):
        fam.validate(case)
        assert sum(case["calls"]) == sum(case["calls2"]) == case["total"] <= 6000, (seed, i, case)
        assert case["variant"] in fam.variants and case["start"] in ("zero", "random", "null"), case
        assert case["start"] != "null" or (fam.null_state and case["calls"] == [case["total"]]), case
        assert set(case["pads"]) == set(fam.buffers) and set(case["pads"].values()) <= set(sf.PADS), case
        assert set(fam.wants(case["subset"])) < set(fam.optional) or not fam.optional, case
        assert fam.none_legal or not fam.optional or fam.wants(case["subset"]), case


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_committed_draws_reach_every_axis_value(family):
    """the plan-independent half of the coverage assertion of tests/test_gpu_stream_fuzz.py (there `unit` is the plan's, here the
    stand-in's): the weights are sufficient at three seeds of twelve cases"""
    gaps = sf.coverage_gaps(family, [case for _, _, case in _draws(family)])
    assert not gaps, gaps


def _run(family, defect=None, seeds=sf.SEEDS):
    env = sf.cpu_env()
    lines = []
    ran = 0
    for seed in seeds:
        n, found = sf.run_cases(env, seed, sf.CASES, [family], log=lambda s: None, opener=sf.stand_in_opener(defect), host=True)
        ran += n
        lines += found
    assert not sf.GPU_STOPPED
    return ran, lines


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_undamaged_stand_in_passes_every_committed_case(family):
    t0 = time.perf_counter()
    ran, lines = _run(family)
    print(f"{family}: {ran} cases through the stand-in in {time.perf_counter() - t0:.2f} s")
    assert ran == len(sf.SEEDS) * sf.CASES and not lines, lines[:3]


# defect -> (the family whose stand-in carries it, the check letter that must report it)
PLANTED = {
    "short_call_history": ("rank", "b"),   # a call shorter than the history keeps only that call's samples as the new history
    "zero_call_clears": ("rank", "b"),     # a zero-length call clears the state
    "row64_from_row0": ("rank", "a"),      # row 64 starts from row 0's state
    "variant1_ulp": ("cfar", "d"),         # variant 1 differs in one element by one ulp
    "pad_write": ("rank", "e"),            # one element is written past `samples` into the padding
    "subset_moves": ("lms", "f"),          # leaving out one optional output moves another into its buffer
    "position_stuck": ("ddc", "b"),        # the position is not advanced after a call that ends on a block edge
    "count_off_by_one": ("timing", "a"),   # a data-dependent count is off by one on one channel
}


@pytest.mark.parametrize("defect", sorted(PLANTED))
def test_planted_defect_is_reported_under_its_letter(defect):
    family, letter = PLANTED[defect]
    ran, lines = _run(family, defect)
    assert lines, (defect, "no committed case of", family, "reports it")
    letters = {re.search(r"check=(\w+)", s).group(1) for s in lines}
    assert letter in letters, (defect, letters)
    by_case = [(re.search(r"check=(\w+)", s).group(1), eval(re.search(r"case=(\{.*\}) buffer=", s).group(1))) for s in lines]
    if defect == "short_call_history":  # a defect of the carry shows in the splits -- and in the one call where that call is short itself
        assert all(l in "bc" or (l == "a" and 0 < c["total"] < c["hist"]) for l, c in by_case), letters
    elif defect == "zero_call_clears":
        assert letters <= {"b", "c"}, letters
    elif defect == "variant1_ulp":  # where the case runs variant 0, variant 1 is seen by (d) alone
        assert {l for l, c in by_case if c["variant"] == 0} == {"d"}, letters
    elif defect not in ("row64_from_row0", "position_stuck", "count_off_by_one"):
        assert letters == {letter}, letters
    hit = next(s for s in lines if f"check={letter} " in s)
    m = re.match(r"FAIL family=(\w+) seed=(\d+) index=(\d+) check=(\w+) case=(\{.*\}) buffer=(.*) differing=(-?\d+) first=(.*)$", hit)
    assert m and m.group(1) == family, hit
    seed, index = int(m.group(2)), int(m.group(3))
    assert eval(m.group(5)) == sf.draw_case(seed, family, index)  # the line carries the case, and its values rebuild it
    # the command line, given the values of the line, rebuilds exactly that case and reports the same line
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        status = sf.main(["--stand-in", "--defect", defect, "--seed", str(seed), "--family", family, "--case", str(index)])
    assert status == 1 and hit in out.getvalue().splitlines(), out.getvalue()
    with contextlib.redirect_stdout(io.StringIO()):
        assert sf.main(["--stand-in", "--seed", str(seed), "--family", family, "--case", str(index)]) == 0


def test_reference_cost_per_family():
    """prints what the references of the committed cases cost (pytest -s): the figure the shapes were sized with"""
    for family in FAMILY_NAMES:
        fam = sf.FAMILIES[family]
        t0 = time.perf_counter()
        worst = 0.0
        for _, _, case in _draws(family):
            t1 = time.perf_counter()
            data = fam.data(case)
            fam.step(case, data, fam.start_state(data, case["start"]), 0, case["total"])
            worst = max(worst, time.perf_counter() - t1)
        total = time.perf_counter() - t0
        print(f"{family}: references of {len(sf.SEEDS) * sf.CASES} cases: {total:.2f} s, {total / len(sf.SEEDS):.2f} s per seed, "
              f"the slowest case {worst:.2f} s")
