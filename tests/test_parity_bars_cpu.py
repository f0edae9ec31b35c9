"""The GPU parity bars (tests/parity_bars.py), certified without a GPU and without looking at a kernel.

Over every hand-written grid case, the 96 random draws, every snow case (model, and microclimate at MICRO_HEIGHTS):
the noise variants of the oracle keep its NaN / inf pattern; the bars they give stay far below the 1e-6 cap; every
single-precision slip variant that touches a case lies >= 100 bars away in at least one variable; and the very comparators the
GPU tests call raise on the slip variants' output and accept the oracle's and the noise variants'.
Measured figures: profiles/parity_bars_cpu.txt (tools/parity_margins.py)."""
import numpy as np
import pytest

import parity_bars as PB
from golden_util import CASES as GOLDEN_CASES, SNOW_CASES as GOLDEN_SNOW, load, load_snow
from snow_cases import assert_close

SETS = ("cases", "random", "snowmodel", "microsnow")
SLIPS32 = ("exp32", "log32", "pow32", "sqrt32")
_measured = {}


def measured(O, kind):
    """[(label, run, want, bars, N, S)] of a set, computed once per session"""
    if kind not in _measured:
        rows = []
        for _, label, run, _ in PB.case_sets(O, (kind,)):
            want, bars, noise = PB.bars_for(O, run)       # asserts that every noise variant keeps the NaN / inf pattern
            rows.append((label, run, want, bars, noise, PB.slips_for(O, run, want)))
        _measured[kind] = rows
    return _measured[kind]


def test_fma_variants_load_here_or_fail_loudly(oracle):
    """the fma builds answer their probe before any of their floating-point code runs; a host without fused multiply-add
    makes load_variant raise, and with it every test below: never a skip"""
    for v in oracle.NOISE_VARIANTS + oracle.SLIP_VARIANTS:
        assert oracle.load_variant(v).orc_variant_probe() == 1
    with pytest.raises(ValueError):
        oracle.load_variant("exp16")


@pytest.mark.parametrize("kind,count", zip(SETS, (42, 96, 14, 70)))
def test_noise_variants_keep_the_pattern_and_the_bars_follow_the_rule(oracle, kind, count):
    rows = measured(oracle, kind)
    assert len(rows) == count
    for label, _, want, bars, noise, _ in rows:
        assert list(bars) == list(want)
        for k in want:
            assert bars[k] == min(1e-6, max(2.0 ** -40, 16.0 * noise[k])), (label, k)
            assert PB.FLOOR <= bars[k] <= PB.CAP


@pytest.mark.parametrize("kind", SETS)
def test_cap_condition(oracle, kind):
    """a case at the 1e-6 cap is a case the derived bars did nothing for: none of the hand-written ones, at most 5 % of the
    random draws"""
    at_cap = [label for label, _, _, bars, _, _ in measured(oracle, kind) if max(bars.values()) >= PB.CAP]
    allowed = 0.05 * 96 if kind == "random" else 0
    assert len(at_cap) <= allowed, at_cap


@pytest.mark.parametrize("kind", SETS)
def test_power_condition(oracle, kind):
    """every *32 slip that changes a case's output at all is >= 100 bars away in at least one variable.  exp46 (a misplaced
    46-bit routine) is reported, not asserted: at K = 16 it reaches 0.002 - 3 bars, caught in the two-stream-heavy cases only."""
    weakest, e46 = (float("inf"), ""), []
    for label, _, want, bars, _, S in measured(oracle, kind):
        for v in SLIPS32:
            ratio = [S[v][k] / bars[k] for k in want if S[v][k] > 0]
            if ratio:
                assert max(ratio) >= 100.0, (label, v, max(ratio))
                weakest = min(weakest, (max(ratio), f"{label}:{v}"))
        r46 = [S["exp46"][k] / bars[k] for k in want if S["exp46"][k] > 0]
        if r46:
            e46.append(max(r46))
    print(f"{kind}: weakest *32 slip {weakest[0]:.3g} bars ({weakest[1]}); exp46 {min(e46, default=0):.3g} .. {max(e46, default=0):.3g} bars, "
          f"{sum(r > 1 for r in e46)} of {len(e46)} cases caught")
    assert weakest[0] < float("inf")                         # the slips do touch this set


def _compare_like_the_gpu_tests(kind, got, want, bars):
    if kind in ("cases", "random"):                          # test_parity_gpu.compare
        PB.compare(got, want, bars)
    else:                                                    # snow_cases.assert_close, variable by variable
        for k in want:
            assert_close(got[k], want[k], bars[k], k)


@pytest.mark.parametrize("kind", SETS)
def test_the_comparator_itself_raises_on_a_slip_and_accepts_correct_evaluations(oracle, kind):
    """the claim of power, through the comparator the GPU tests call: handed the log32 / exp32 variant's output as `got`
    with the case's bars it raises for every case the variant touches; handed the oracle's own output, or a noise
    variant's, it does not"""
    touched = {v: 0 for v in ("log32", "exp32")}
    for label, run, want, bars, _, S in measured(oracle, kind):
        _compare_like_the_gpu_tests(kind, run(None), want, bars)
        for v in oracle.NOISE_VARIANTS:
            _compare_like_the_gpu_tests(kind, run(oracle.load_variant(v)), want, bars)
        for v in touched:
            if max(S[v].values()) > 0:
                touched[v] += 1
                with pytest.raises(AssertionError):
                    _compare_like_the_gpu_tests(kind, run(oracle.load_variant(v)), want, bars)
    assert all(touched.values()), touched


def test_compare_has_no_default_tolerance():
    x = {"Tz": np.zeros((1, 1, 2))}
    with pytest.raises(TypeError):
        PB.compare(x, x)
    with pytest.raises(TypeError):
        PB.compare(x, x, {"Tz": 1e-9}, tol=1e-9)
    with pytest.raises(AssertionError):
        PB.compare(x, x, tol=1e-5)                           # nothing looser than the old bar
    assert PB.compare(x, x, tol=1e-6) == {"Tz": 0.0} and PB.compare(x, x, {"Tz": PB.FLOOR}) == {"Tz": 0.0}


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_default_oracle_is_unchanged(oracle, name):
    """the variant builds rename libm calls in builds of their own; the default library still gives the stored vectors
    (tests/golden/*.npz are its output), to the last bit"""
    a, af, expect = load(name)
    got = oracle.run_grid(**a, array_forcing=af)
    for k, w in expect.items():
        assert np.array_equal(got[k], w, equal_nan=True), k


@pytest.mark.parametrize("name", GOLDEN_SNOW)
def test_default_snow_oracle_is_unchanged(oracle, name):
    sw, af, reqhgt, mat, micro, smod, mout = load_snow(name)
    got = oracle.run_snowmodel(**sw, array_forcing=af)
    for k, w in smod.items():
        assert np.array_equal(got[k], w, equal_nan=True), k
