"""Below ground at several depths from one solve (include/mcf.h mcf_plan_below_set_depths, mcf_runmicro_depths) and period
summaries below ground (mcf_plan_summary_enable_below, mcf_runmicro_depths_summary).  The yardstick is never the new code: it
is the single-depth route runmicro1Cpp(reqhgt = depths[d], pointm.Tbp = tbp[d]) on the whole-series plan
(MCF_BELOW_STREAM=0), and tests/summary_ref.py over its arrays.  Every comparison is bit for bit, NaN payloads included.
Shape: 23 x 11 cells (250 valid), nine days and seven steps, soils banded so that every regime of Tbelowgroundv occurs."""
import numpy as np
import pytest

import summary_ref as SR
from microclimf_amd import McfError, _abi, api, frontend, synthetic
from microclimf_amd.api import Plan, runmicro1Cpp, runmicro2Cpp_coarse, runmicro3Cpp
from test_below_stream_gpu import ARGS, OUT, T_ODD, approx_n, bits, same_bits, three_regimes, with_env, with_na

pytestmark = pytest.mark.gpu
DEPTHS = (-0.02, -0.1, -0.5, -20.0)
ND = T_ODD // 24
POD = [0, 0, 1, 1, 2, 2, 0, -1, 1]
STATS = _abi.STAT_NAMES
_cache = {}


def workload(complete):
    a = with_na(synthetic.workload(23, 11, T_ODD, variety=True, start_doy=140, out=OUT, complete=bool(complete)))
    return three_regimes(a, T_ODD)


def tbp_rows(a, depths):
    """a soil temperature series per depth for the point model's part (complete = 0): each row its own, with a daily cycle"""
    base = np.asarray(a["pointm"]["Tbp"], dtype=np.float64)
    k = np.arange(base.size)
    return np.stack([base + 0.2 * d + (0.5 + 2.0 / (1 + abs(d))) * np.cos(2 * np.pi * k / 24 + d) for d in depths])


def at_depth(a, depth, tbp_row):
    b = dict(a, reqhgt=float(depth))
    b["pointm"] = dict(a["pointm"], Tbp=tbp_row)
    return b


def yardstick(complete, depth):
    """the single-depth whole-series run at `depth`; made once per (complete, depth)"""
    key = (complete, depth)
    if key not in _cache:
        a = workload(complete)
        want = with_env("0", runmicro1Cpp, **at_depth(a, depth, tbp_rows(a, [depth])[0]))
        for v in want.values():
            v.setflags(write=False)
        _cache[key] = want
    return _cache[key]


def depth_args(a, depths, complete):
    b = {k: a[k] for k in ARGS if k not in ("reqhgt", "out")}
    return dict(b, depths=list(depths), tbp=None if complete else tbp_rows(a, depths))


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} values differ, first at {np.argwhere(diff)[0]}"


def test_every_regime_occurs_at_the_depths():
    """a numpy transcription of the damping depth sorts the valid cells; no regime named in the kernel goes untested"""
    a = workload(1)
    valid = ~np.isnan(a["vegp"]["hgt"])
    assert valid.sum() == 250
    n = {d: approx_n(dict(a, reqhgt=d), T_ODD)[valid] for d in DEPTHS}
    m, hiy = T_ODD, 8760
    assert (n[-0.02] <= 44).sum() > 100                                                     # complete = 1: the hourly window
    assert (n[-0.1] <= 44).any() and ((n[-0.1] >= 53) & (n[-0.1] <= m - 5)).any() and (n[-0.1] >= m + 5).any()
    assert ((n[-0.5] >= 53) & (n[-0.5] <= m - 5)).any() and (n[-0.5] >= m + 5).sum() > 100
    assert ((n[-0.02] > 2) & (n[-0.02] <= 23)).any() and ((n[-0.02] >= 26) & (n[-0.02] < hiy)).any()      # complete = 0: the blends
    assert (n[-20.0] < hiy - 50).any() and (n[-20.0] > hiy + 50).sum() > 100                 # ... and `mat`
    changed = ((n[-0.02] <= 44) & (n[-0.1] >= 53)).sum()
    assert changed > 100                                                                    # cells that change regime between depths


@pytest.mark.parametrize("complete", [0, 1])
@pytest.mark.parametrize("chunk", [1, 2, 5, 7])
def test_1_every_depth_equals_its_single_depth_run(complete, chunk):
    a = workload(complete)
    got = api.runmicro_depths(**depth_args(a, DEPTHS, complete), days_per_chunk=chunk)
    assert len(got["Tz"]) == len(DEPTHS) and got["depths"].tolist() == list(DEPTHS)
    for d, depth in enumerate(DEPTHS):
        want = yardstick(complete, depth)
        assert_bits(got["Tz"][d], want["Tz"], f"Tz at {depth}")
        assert_bits(got["soilm"], want["soilm"], "soilm")
    valid = ~np.isnan(a["vegp"]["hgt"])
    assert np.isfinite(got["Tz"][1][:, :, : ND * 24][valid]).all()
    assert (bits(got["Tz"][0]) != bits(got["Tz"][1]))[valid].any()


@pytest.mark.parametrize("complete", [0, 1])
def test_2_permuted_and_repeated_depths_keep_their_own_rows(complete):
    """no depth reads another's row of circular means or of the point model's series"""
    order = (-0.5, -0.02, -20.0, -0.1, -0.02)
    a = workload(complete)
    got = api.runmicro_depths(**depth_args(a, order, complete), days_per_chunk=2, soilm=False)
    assert "soilm" not in got
    for d, depth in enumerate(order):
        assert_bits(got["Tz"][d], yardstick(complete, depth)["Tz"], f"Tz at {depth} (place {d})")


@pytest.mark.parametrize("complete", [0, 1])
def test_3_below_ground_the_solver_reads_neither_paia_nor_leafden(complete):
    """the fact the feature rests on: two single-depth runs whose vegetation differs only in paia and leafden agree"""
    a = workload(complete)
    b = at_depth(a, -0.1, tbp_rows(a, [-0.1])[0])
    other = dict(b, vegp=dict(b["vegp"], paia=np.asfortranarray(b["vegp"]["paia"] * 0.37 + 0.11),
                              leafden=np.asfortranarray(b["vegp"]["leafden"] * 1.9 + 0.05)))
    same_bits(with_env("0", runmicro1Cpp, **other), yardstick(complete, -0.1))


@pytest.mark.parametrize("complete", [0, 1])
def test_4_plan_level_slabs_and_state_errors(complete):
    a = workload(complete)
    plan_args = dict(a, reqhgt=DEPTHS[0])
    tbp = None if complete else tbp_rows(a, DEPTHS)
    with Plan(**plan_args, ring_days=4, ring_slots=2, stream_below=True) as st:
        st.below_set_depths(DEPTHS, tbp)
        with pytest.raises(McfError, match="mcf_plan_below_set_days: a day subset together with a depth list"):
            st.below_set_days([0, 2, 3])
        st.below_prepare()
        with pytest.raises(McfError, match="error 5: mcf_plan_below_set_depths: comes before mcf_plan_below_prepare"):
            st.below_set_depths(DEPTHS, tbp)
        d0, slot = 0, 0
        while d0 < ND:
            n = min(3, ND - d0)
            st.run_days(d0, n, slot)
            steps = n * 24 + (T_ODD - ND * 24 if d0 + n == ND else 0)
            for d, depth in enumerate(DEPTHS):
                assert_bits(st.fetch_depth(slot, d, 0, steps), yardstick(complete, depth)["Tz"][:, :, d0 * 24:d0 * 24 + steps],
                            f"Tz at {depth}, days from {d0}")
            assert_bits(st.fetch(slot, "Tz", 0, steps), st.fetch_depth(slot, 0, 0, steps), "fetch(Tz) is depth 0")
            assert_bits(st.fetch(slot, "soilm", 0, n * 24), yardstick(complete, DEPTHS[0])["soilm"][:, :, d0 * 24:(d0 + n) * 24], "soilm")
            d0 += n
            slot ^= 1
        with pytest.raises(McfError, match="mcf_plan_fetch_depth: depth 4 is outside"):
            st.fetch_depth(0, 4, 0, 24)
    with Plan(**plan_args, ring_days=4, stream_below=True) as st:
        st.below_set_days([0, 2, 3])
        with pytest.raises(McfError, match="error 5: mcf_plan_below_set_depths: a depth list together with a day subset"):
            st.below_set_depths(DEPTHS, tbp)
    with Plan(**plan_args, ring_days=1) as whole:
        with pytest.raises(McfError, match="error 5: mcf_plan_below_set_depths: needs a streamed plan"):
            whole.below_set_depths(DEPTHS, tbp)
        with pytest.raises(McfError, match="error 5: mcf_plan_summary_enable_below needs a streamed plan"):
            whole.summary_enable_below(POD)
    with Plan(**dict(plan_args, out=[0, 0, 0, 1, 0, 0, 0, 0, 0, 0]), ring_days=4, stream_below=True) as st:
        with pytest.raises(McfError, match="error 5: mcf_plan_below_set_depths: the plan was created without Tz"):
            st.below_set_depths(DEPTHS, tbp)


def thresholds(complete):
    """values that occur in the series at a counted step of a valid cell: `>` and `>=` differ there"""
    w = yardstick(complete, DEPTHS[0])
    i, j = np.argwhere(~np.isnan(w["Tz"][:, :, 0]))[7]
    return {"Tz": float(w["Tz"][i, j, 60]), "soilm": float(w["soilm"][i, j, 60])}


def plan_summary(complete, chunk, depths=DEPTHS, vars=("Tz", "soilm")):
    a = workload(complete)
    thr = thresholds(complete)
    with Plan(**dict(a, reqhgt=depths[0]), ring_days=chunk + 1, stream_below=True) as st:
        st.below_set_depths(depths, None if complete else tbp_rows(a, depths))
        st.below_prepare()
        st.summary_enable_below(POD, vars, STATS, thr)
        for d0 in range(0, ND, chunk):
            n = min(chunk, ND - d0)
            st.run_days(d0, n, 0)
            st.summary_accumulate(0, 0, d0, n)
        got = {("Tz", d, s): st.fetch_summary_depth(d, "Tz", s) for d in range(len(depths)) for s in STATS}
        if "soilm" in vars:
            got.update({("soilm", 0, s): st.fetch_summary_depth(0, "soilm", s) for s in STATS})
            with pytest.raises(McfError, match="only Tz is kept per depth"):
                st.fetch_summary_depth(1, "soilm", "mean")
        with pytest.raises(McfError, match="outside the plan's list"):
            st.fetch_summary_depth(len(depths), "Tz", "mean")
        return got, st.summary_days()


def assert_summary(got, days, complete, depths=DEPTHS, vars=("Tz", "soilm")):
    thr = thresholds(complete)
    for v in vars:
        for d, depth in enumerate(depths if v == "Tz" else depths[:1]):
            want, wdays = SR.summarise(yardstick(complete, depth)[v][:, :, : ND * 24], POD, 3, thr[v])
            assert days.tolist() == wdays.tolist() == [3, 3, 2]
            for s in STATS:
                assert got[v, d, s].flags.f_contiguous
                assert_bits(got[v, d, s], want[s], f"{v} {s} at {depth}")


@pytest.mark.parametrize("complete", [0, 1])
def test_5_summaries_per_depth_equal_the_yardstick_and_do_not_depend_on_chunks(complete):
    thr = thresholds(complete)
    x = yardstick(complete, DEPTHS[0])["Tz"][:, :, : ND * 24][:, :, np.repeat(np.asarray(POD) >= 0, 24)]
    assert (x == thr["Tz"]).any() and (x > thr["Tz"]).sum() != (x >= thr["Tz"]).sum()
    ref, days = plan_summary(complete, 5)
    assert_summary(ref, days, complete)
    na = np.isnan(workload(complete)["vegp"]["hgt"])
    assert (bits(ref["Tz", 2, "max"][na]) == SR.NA_BITS).all() and np.isfinite(ref["Tz", 2, "max"][~na]).all()
    for chunk in (1, 2):
        got, d2 = plan_summary(complete, chunk)
        assert d2.tolist() == days.tolist()
        for key in ref:
            assert np.array_equal(bits(got[key]), bits(ref[key])), (key, chunk)


def test_5_one_depth_without_a_list_on_a_plain_streamed_plan():
    a = workload(1)
    thr = thresholds(1)
    with Plan(**dict(a, reqhgt=-0.1), ring_days=4, stream_below=True) as st:
        st.below_prepare()
        with pytest.raises(McfError, match="streamed plan"):
            st.summary_enable(POD, ("Tz",), STATS, thr["Tz"])
        with pytest.raises(McfError, match="below ground Tz and soilm can be summarised"):
            st.summary_enable_below(POD, ("Tz", "tleaf"), STATS, thr["Tz"])
        st.summary_enable_below(POD, ("Tz",), STATS, thr)
        for d0 in range(0, ND, 3):
            st.run_days(d0, 3, 0)
            st.summary_accumulate(0, 0, d0, 3)
        want, wdays = SR.summarise(yardstick(1, -0.1)["Tz"][:, :, : ND * 24], POD, 3, thr["Tz"])
        assert st.summary_days().tolist() == wdays.tolist()
        for s in STATS:
            assert_bits(st.fetch_summary_depth(0, "Tz", s), want[s], s)
            assert_bits(st.fetch_summary("Tz", s), want[s], s)
        st.summary_reset()
        assert st.summary_days().tolist() == [0, 0, 0]


@pytest.mark.parametrize("complete", [0, 1])
def test_6_one_call_summary_equals_the_plan_level_one(complete):
    a = workload(complete)
    got = api.runmicro_depths_summary(**depth_args(a, DEPTHS, complete), periods=POD, vars=("Tz", "soilm"), stats=STATS,
                                      thresholds=thresholds(complete), chunk_days=2)
    flat = {("Tz", d, s): got["Tz"][d][s] for d in range(len(DEPTHS)) for s in STATS}
    flat.update({("soilm", 0, s): got["soilm"][s] for s in STATS})
    assert_summary(flat, got["days"], complete)
    auto = api.runmicro_depths_summary(**depth_args(a, DEPTHS[:2], complete), periods=POD, stats=("mean",))      # chunk from free memory
    assert "soilm" not in auto
    assert_bits(auto["Tz"][1]["mean"], got["Tz"][1]["mean"], "chunk_days = 0")


@pytest.mark.parametrize("complete", [0, 1])
def test_7_layered_vegetation(complete):
    depths = (-0.05, -0.3)
    a = with_na(synthetic.workload(17, 5, T_ODD, reqhgt=-0.05, variety=True, start_doy=120, out=OUT, complete=bool(complete)))
    a = synthetic.layered(a, 3)
    dfsel = a.pop("dfsel")
    tbp = tbp_rows(a, depths)
    got = api.runmicro_depths(**depth_args(a, depths, complete), dfsel=dfsel, days_per_chunk=4)
    for d, depth in enumerate(depths):
        want = with_env("0", runmicro3Cpp, dfsel, **at_depth(a, depth, tbp[d]))
        assert_bits(got["Tz"][d], want["Tz"], f"Tz at {depth}")
        assert_bits(got["soilm"], want["soilm"], "soilm")


def test_8_coarse_array_forcing():
    depths = (-0.03, -0.1, -0.6)
    a, rp, cp = synthetic.coarse_workload(26, 26, T_ODD, 4, 4, reqhgt=-0.1, variety=True, start_doy=170, na_frac=0.03, out=OUT)
    b = {k: a[k] for k in ARGS if k not in ("reqhgt", "out")}
    got = api.runmicro_depths(**b, depths=depths, coarse={"rowpos": rp, "colpos": cp}, days_per_chunk=3)
    for d, depth in enumerate(depths):
        want = with_env("0", runmicro2Cpp_coarse, *[dict(a, reqhgt=depth)[k] for k in ARGS], rowpos=rp, colpos=cp)
        assert_bits(got["Tz"][d], want["Tz"], f"Tz at {depth}")
        assert_bits(got["soilm"], want["soilm"], "soilm")


def test_9_front_end_on_the_bundled_site():
    from bundled import load
    depths = (-0.05, -0.2)
    weather, vegp, soilc, dtm = load(3 * 24)
    vegp = {k: (v[:, :, 6] if v.ndim == 3 else v) for k, v in vegp.items()}          # July's layer, time-invariant
    mp = frontend.runpointmodel(weather, 0.05, dtm, vegp, soilc)
    got = frontend.runmicro_depths(mp, depths, vegp, soilc, dtm)
    for d, depth in enumerate(depths):
        mpd = frontend.runpointmodel(weather, depth, dtm, vegp, soilc)
        want = with_env("0", frontend.runmicro, mpd, depth, vegp, soilc, dtm)
        assert list(want) == ["Tz", "soilm"]
        assert_bits(got["Tz"][d], want["Tz"], f"Tz at {depth}")
        assert_bits(got["soilm"], want["soilm"], "soilm")
    summ = frontend.runmicro_depths_summary(mp, depths, vegp, soilc, dtm, periods="day", stats=("mean", "max"))
    assert len(summ["periods"]) == 3 and summ["days"].tolist() == [1, 1, 1]
    for d in range(2):
        want, _ = SR.summarise(got["Tz"][d][:, :, :72], [0, 1, 2], 3)
        for s in ("mean", "max"):
            assert_bits(summ["Tz"][d][s], want[s], f"{s} at {depths[d]}")
