"""The place table both sinks of a plan share (mcf_sinks_host.hpp SinkPlaces; mcf_api.hip for_sink_sources): on ONE streamed
below-ground plan with a depth list the period summaries and the series sink are enabled together and folded chunk by chunk,
and every (depth, variable) either sink hands out must equal, bit for bit, tests/summary_ref.py / tests/series_ref.py applied to
what fetch_depth / fetch of the same plan returned for the same chunks.  Shape: 10 x 5 = 50 cells in 21-cell tiles (the last
one partly filled), three days in chunks of two, three depths; complete = 0 with a soil temperature series of its own per depth,
so that no two depths hold the same values."""
import re

import numpy as np
import pytest

import series_ref as ZR
import summary_ref as SR
from microclimf_amd import McfError, _abi, api, synthetic
from microclimf_amd.api import Plan

pytestmark = pytest.mark.gpu
ROWS, COLS, ND, CHUNK = 10, 5, 3, 2
DEPTHS = (-0.05, -0.2, -0.5)
VARS = ("Tz", "soilm")
POD = [0, 1, 0]
POINTS = [3, ROWS * COLS - 1]


def zone_map():
    z = np.zeros((ROWS, COLS), dtype=np.int32, order="F")
    z[4, 1] = -1                      # in no zone
    z[7:, 3] = 1
    z[ROWS - 1, COLS - 1] = 1         # the last cell, in the partly filled tile
    return z


@pytest.fixture(scope="module")
def folded():
    """-> (the plan's own arrays {("Tz", depth) / ("soilm", 0): [rows, cols, steps]}, every fetch of the two sinks, the
    summary's counted days, the refusals' messages, the thresholds)"""
    a = synthetic.workload(ROWS, COLS, ND * 24, variety=True, start_doy=140, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0], complete=False)
    a["vegp"]["hgt"][2, 1, ...] = np.nan
    base, hour = np.asarray(a["pointm"]["Tbp"], dtype=np.float64), np.arange(ND * 24)
    tbp = np.stack([base + 0.2 * d + (0.5 + 2.0 / (1 + abs(d))) * np.cos(2 * np.pi * hour / 24 + d) for d in DEPTHS])
    # thresholds that split the values of either variable: the middle of its range in a first run through the one-call entry
    first = api.runmicro_depths(**{key: v for key, v in a.items() if key not in ("reqhgt", "out")}, depths=list(DEPTHS), tbp=tbp)
    thr = {"Tz": float(np.nanmin(first["Tz"][0]) + np.nanmax(first["Tz"][0])) / 2,
           "soilm": float(np.nanmin(first["soilm"]) + np.nanmax(first["soilm"])) / 2}
    arrays = {("Tz", d): [] for d in range(len(DEPTHS))}
    arrays["soilm", 0] = []
    with Plan(**dict(a, reqhgt=DEPTHS[0]), ring_days=CHUNK, cells_per_block=21, stream_below=True) as st:
        st.below_set_depths(DEPTHS, tbp)
        st.below_prepare()
        st.summary_enable_below(POD, VARS, _abi.STAT_NAMES, thr, nperiods=2)
        st.series_enable_below(POINTS, zone_map(), VARS, _abi.ZSTAT_NAMES, nzones=2)
        for d0 in range(0, ND, CHUNK):
            n = min(CHUNK, ND - d0)
            st.run_days(d0, n, 0)
            st.summary_accumulate(0, 0, d0, n)
            st.series_accumulate(0, 0, d0, n)
            for d in range(len(DEPTHS)):
                arrays["Tz", d].append(st.fetch_depth(0, d, 0, n * 24))
            arrays["soilm", 0].append(st.fetch(0, "soilm", 0, n * 24))
        got = {}
        for v, d in arrays:
            got["summary", v, d] = {s: st.fetch_summary_depth(d, v, s) for s in _abi.STAT_NAMES}
            got["points", v, d] = st.fetch_point_series_depth(d, v)
            got["zones", v, d] = {s: st.fetch_zone_series_depth(d, v, s) for s in _abi.ZSTAT_NAMES}
        refused = {}
        for what, fetch in (("summary", lambda d, v: st.fetch_summary_depth(d, v, "mean")), ("points", st.fetch_point_series_depth),
                            ("zones", lambda d, v: st.fetch_zone_series_depth(d, v, "mean"))):
            for d, v in ((1, "soilm"), (len(DEPTHS), "Tz")):
                with pytest.raises(McfError) as e:
                    fetch(d, v)
                refused[what, v] = str(e.value)
        days = st.summary_days()
    return {k: np.concatenate(v, axis=2) for k, v in arrays.items()}, got, days, refused, thr


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    diff = SR.bits(got) != SR.bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} values differ, first at {np.argwhere(diff)[0]}"


def test_the_plans_own_arrays_are_not_degenerate(folded):
    arrays, thr = folded[0], folded[4]
    valid = ~np.isnan(arrays["Tz", 0][:, :, 0])
    assert valid.sum() == ROWS * COLS - 1
    for d in range(len(DEPTHS)):
        for e in range(d):
            differ = SR.bits(arrays["Tz", d]) != SR.bits(arrays["Tz", e])
            assert differ[valid].any() and all(differ[c % ROWS, c // ROWS].any() for c in POINTS), (d, e)
    for v in VARS:
        x = arrays[v, 0][valid]
        assert np.isfinite(x).all() and (x > thr[v]).any() and not (x > thr[v]).all(), v


def test_every_summary_of_every_depth_equals_the_yardstick_on_the_plans_own_arrays(folded):
    arrays, got, days, _, thr = folded
    for (v, d), x in arrays.items():
        want, wdays = SR.summarise(x, POD, 2, thr[v])
        assert days.tolist() == wdays.tolist() == [2, 1]
        for s in _abi.STAT_NAMES:
            assert_bits(got["summary", v, d][s], want[s], f"summary of {v} at depth {d}: {s}")


def test_every_series_of_every_depth_equals_the_yardstick_on_the_plans_own_arrays(folded):
    arrays, got = folded[:2]
    for (v, d), x in arrays.items():
        assert_bits(got["points", v, d], ZR.point_series(x, POINTS), f"points of {v} at depth {d}")
        want = ZR.zone_series(x, zone_map(), 2)
        for s in _abi.ZSTAT_NAMES:
            assert_bits(got["zones", v, d][s], want[s], f"zones of {v} at depth {d}: {s}")
    assert (got["zones", "Tz", 2]["count"][:, 1] == 4.0).all()


def test_a_depth_of_soilm_and_a_depth_behind_the_list_are_refused(folded):
    refused = folded[3]
    entry = {"summary": "mcf_plan_summary_fetch_depth", "points": "mcf_plan_series_fetch_points_depth",
             "zones": "mcf_plan_series_fetch_zones_depth"}
    for what, who in entry.items():
        assert re.search(re.escape(f"error 1: {who}: only Tz is kept per depth (depth 0 for soilm)") + "$", refused[what, "soilm"])
        assert re.search(re.escape(f"error 1: {who}: depth 3 is outside the plan's list") + "$", refused[what, "Tz"])
