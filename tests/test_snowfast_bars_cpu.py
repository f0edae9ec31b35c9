"""The bars of the fast snow method's one-call comparisons (test_snowfast_onecall_gpu.py, test_snowfast2_onecall_gpu.py),
certified without a GPU and without looking at a kernel, as tests/test_parity_bars_cpu.py certifies the others.

Over the seven cases of `mcf_snowmodelq1` and the seven of `mcf_snowmodelq2` (tests/snowfast_cases.py), the oracle chain on the
oracle's own terrain: the noise variants keep the NaN / inf pattern (every case is admissible); the bars follow the rule and none
is at the 1e-6 cap; every single-precision slip that touches a case lies >= 100 bars away in at least one variable; the slips
touch at least six of each file's seven cases (the bare one runs no snow physics); and parity_bars.compare, the comparator the GPU
tests call, raises on the log32 / exp32 variants' output and accepts the oracle's and the noise variants'.  The oracle chain's new
`lib=` / `terrain=` leave its default results as they were, to the last bit.
Measured figures: profiles/parity_bars_cpu.txt (tools/parity_margins.py --sets snowfast1,snowfast2)."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import parity_bars as PB
import snowfast_cases as FC

SETS = ("snowfast1", "snowfast2")
SLIPS32 = ("exp32", "log32", "pow32", "sqrt32")
BARE = 5                                                     # case 5 of each file: no snowfall at all
_measured = {}


@pytest.fixture(scope="module", autouse=True)
def lib():
    """the cases run the host point model on the way to the oracle chain's arguments"""
    import __graft_entry__ as g
    g.build_library()


def measured(O, kind):
    """[(label, run, want, bars, N, S)] of a set, computed once per session"""
    if kind not in _measured:
        rows = []
        for _, label, run, _ in PB.case_sets(O, (kind,)):
            want, bars, noise = PB.bars_for(O, run)       # asserts that every noise variant keeps the NaN / inf pattern
            rows.append((label, run, want, bars, noise, PB.slips_for(O, run, want)))
        _measured[kind] = rows
    return _measured[kind]


def test_the_rule_is_the_one_of_parity_bars():
    assert (PB.K, PB.FLOOR, PB.CAP) == (16.0, 2.0 ** -40, 1e-6)
    assert "snowfast1" not in PB.case_sets.__defaults__[0] and "snowfast2" not in PB.case_sets.__defaults__[0]


@pytest.mark.parametrize("kind", SETS)
def test_every_case_is_admissible_and_the_bars_follow_the_rule(oracle, kind):
    rows = measured(oracle, kind)
    assert len(rows) == 7
    for label, _, want, bars, noise, _ in rows:
        assert list(bars) == list(want)
        for k in want:
            assert bars[k] == min(1e-6, max(2.0 ** -40, 16.0 * noise[k])), (label, k)
        assert max(bars.values()) < PB.CAP, (label, bars)    # none at the cap
        print(f"{kind} {label}: largest N {max(noise.values()):.2e}, largest bar {max(bars.values()):.2e}")


@pytest.mark.parametrize("kind", SETS)
def test_power_condition(oracle, kind):
    """every *32 slip that changes a case's output at all is >= 100 bars away in at least one variable (the condition of
    test_parity_bars_cpu.py); the slips touch every case but the bare one, whose depths are zero whatever the physics"""
    weakest, touched = (float("inf"), ""), set()
    for i, (label, _, want, bars, _, S) in enumerate(measured(oracle, kind)):
        for v in SLIPS32:
            ratio = [S[v][k] / bars[k] for k in want if S[v][k] > 0]
            if ratio:
                assert max(ratio) >= 100.0, (label, v, max(ratio))
                weakest = min(weakest, (max(ratio), f"{label}:{v}"))
                touched.add(i)
    print(f"{kind}: weakest *32 slip {weakest[0]:.3g} bars ({weakest[1]}); cases touched {sorted(touched)}")
    assert len(touched) >= 6 and touched >= set(range(7)) - {BARE}, touched


@pytest.mark.parametrize("kind", SETS)
def test_the_comparator_itself_raises_on_a_slip_and_accepts_correct_evaluations(oracle, kind):
    """parity_bars.compare with the case's bars: handed the log32 / exp32 variant's output as `got` it raises for every case
    the variant touches; handed the oracle's own output, or a noise variant's, it does not"""
    touched = {v: 0 for v in ("log32", "exp32")}
    for label, run, want, bars, _, S in measured(oracle, kind):
        PB.compare(run(None), want, bars)
        _, res = PB.run_variants(oracle, run, oracle.NOISE_VARIANTS + tuple(touched))
        for v in oracle.NOISE_VARIANTS:
            PB.compare(res[v], want, bars)
        for v in touched:
            if max(S[v].values()) > 0:
                touched[v] += 1
                with pytest.raises(AssertionError):
                    PB.compare(res[v], want, bars)
    assert min(touched.values()) >= 6, touched


@pytest.mark.parametrize("kind", ("q1", "q2"))
def test_the_oracle_chain_is_unchanged_by_default_and_by_its_own_terrain(oracle, kind):
    """`lib=None, terrain=None` give what the chain gave before it had either (tests/golden/snowfast_case0_digests.json: SHA-256
    of each variable of case 0, recorded from the chain as it was), and so does handing it the default library and
    terrain_oracle's terrain explicitly: the injection point is where the terrain block was"""
    c = (FC.q1_case if kind == "q1" else FC.q2_case)(0)
    recorded = json.loads((Path(__file__).parent / "golden" / "snowfast_case0_digests.json").read_text())[kind]
    got = FC.run(oracle, c)(None)
    assert list(got) == list(recorded)
    for k, v in got.items():
        assert v.tobytes() == c["want"][k].tobytes(), k
        assert hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() == recorded[k], k
    terrain = FC.oracle_terrain(c)[3]
    again = FC.run(oracle, c, terrain=terrain)(oracle.load())
    for k, v in got.items():
        assert again[k].tobytes() == v.tobytes(), k
    moved = dict(terrain, skyview=terrain["skyview"] * (1 - 1e-6))          # and the injected terrain is the one it uses
    assert any(FC.run(oracle, c, terrain=moved)(None)[k].tobytes() != v.tobytes() for k, v in got.items())
