"""Period summaries on the device (include/mcf.h "period summaries") against tests/summary_ref.py on the plan's own fetch():
elementwise fp64 add, compare and divide are the device's operations, so every comparison is bit for bit, NA payload included.
Shapes: 5 x 10 cells (for 21-cell tiles two full tiles and one of 8), 96 h, all ten outputs, reqhgt 0.05."""
import numpy as np
import pytest

import stages_cases as SC
import summary_ref as SR
from microclimf_amd import _abi, api, frontend, synthetic
from microclimf_amd.api import Plan

pytestmark = pytest.mark.gpu
ALL = _abi.OUT_NAMES
STATS = _abi.STAT_NAMES
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "complete", "mat")
bits = SR.bits
_plain = {}


def plain_fetch(name):
    """every output of a whole-series plan without a summary, and its dispatch statistics; made once"""
    if name not in _plain:
        a = dict(SC.build(name))
        dfsel = a.pop("dfsel", None)
        with Plan(**a, ring_days=4, dfsel=dfsel) as p:
            p.run_days(0, 4, 0)
            _plain[name] = ({k: p.fetch(0, k, 0, 96) for k in ALL}, p.dispatch_stats())
    return _plain[name]


def thresholds(series, step=60):
    """per variable a value that occurs in its series (a cell that is not NA, noon of day 2): `>` and `>=` differ there"""
    valid = np.argwhere(~np.isnan(series["Tz"][:, :, 0]))[3]
    return {k: float(v[valid[0], valid[1], step]) for k, v in series.items()}


def run_plan(a, pod, thr, *, ring_days, vars=ALL, stats=STATS, at=0, nperiods=None, upload=False, **kw):
    """a summary plan over the whole series in chunks of `ring_days`, each chunk accumulated behind its run (`at`: the chunk
    lies at that day of the slot).  -> ({(var, stat): plane}, days, the plan's own fetch of every variable, dispatch stats)"""
    a = dict(a)
    dfsel = a.pop("dfsel", None)
    nd = len(a["obstime"]["year"]) // 24
    own = {k: [] for k in vars}
    with Plan(**a, ring_days=ring_days + at, dfsel=dfsel, **kw) as p:
        p.summary_enable(pod, vars, stats, thr, nperiods=nperiods)
        for d0 in range(0, nd, ring_days):
            n = min(ring_days, nd - d0)
            if upload:
                p.upload_forcing_days(d0, n, 0)
            p.run_days_at(d0, n, 0, at) if at else p.run_days(d0, n, 0)
            p.summary_accumulate(0, at, d0, n)
            for k in vars:
                own[k].append(p.fetch(0, k, at * 24, n * 24))
        summ = {(v, s): p.fetch_summary(v, s) for v in vars for s in stats}
        return summ, p.summary_days(), {k: np.concatenate(v, axis=2) for k, v in own.items()}, p.dispatch_stats()


def assert_matches(summ, days, own, pod, nperiods, thr, vars=ALL, stats=STATS):
    for v in vars:
        want, wdays = SR.summarise(own[v], pod, nperiods, thr[v] if isinstance(thr, dict) else thr)
        assert days.tolist() == wdays.tolist()
        for s in stats:
            got = summ[v, s]
            assert got.shape == want[s].shape and got.flags.f_contiguous, (v, s)
            diff = bits(got) != bits(want[s])
            assert not diff.any(), (v, s, int(diff.sum()), got[diff][:3], want[s][diff][:3])


@pytest.mark.parametrize("pod", ([0, 0, 1, 1], [0, -1, 1, 0]), ids=["0011", "0-110"])
def test_1_every_statistic_of_every_output_equals_the_yardstick(pod):
    a = SC.build("s170_h005")
    series, _ = plain_fetch("s170_h005")
    thr = thresholds(series)
    hgt, pai = np.asarray(a["vegp"]["hgt"]), np.asarray(a["vegp"]["pai"])
    assert np.isnan(hgt).any() and (~np.isnan(hgt) & (pai == 0)).any()          # an NA cell and a bare cell
    summ, days, own, _ = run_plan(a, pod, thr, ring_days=4)
    assert days.tolist() == [sum(1 for q in pod if q == k) for k in (0, 1)] and len(summ) == 60
    assert_matches(summ, days, own, pod, 2, thr)
    na = np.isnan(hgt)
    for v in ALL:
        # the threshold occurs among the counted steps, so `>` and `>=` would count differently
        counted = np.repeat(np.asarray(pod) >= 0, 24)
        x = own[v][:, :, counted][~na]
        assert (x == thr[v]).any() and (x > thr[v]).sum() != (x >= thr[v]).sum(), v
        for s in STATS:
            assert (bits(summ[v, s][na]) == SR.NA_BITS).all() and np.isfinite(summ[v, s][~na]).all(), (v, s)
    assert (summ["Tz", "hours_above"][~na] > 0).any() and (summ["Tz", "max"][~na] > summ["Tz", "mean"][~na]).all()


def test_2_chunking_and_slot_placement_do_not_matter():
    a = SC.build("s170_h005")
    thr = thresholds(plain_fetch("s170_h005")[0])
    pod = [0, -1, 1, 0]
    ref, days, _, _ = run_plan(a, pod, thr, ring_days=4)
    for kw in (dict(ring_days=1), dict(ring_days=2), dict(ring_days=3, at=1), dict(ring_days=2, at=1)):      # (a slot holds at most the series' four days)
        got, d2, _, _ = run_plan(a, pod, thr, **kw)
        assert d2.tolist() == days.tolist() == [2, 1]
        for key in ref:
            assert np.array_equal(bits(got[key]), bits(ref[key])), (key, kw)


@pytest.mark.parametrize("cpb", (16, 21, 32, 42))
def test_3_every_tile_size(cpb):
    a = SC.build("s355_h005")
    thr = thresholds(plain_fetch("s355_h005")[0])
    pod = [1, 0, 0, 1]
    summ, days, own, _ = run_plan(a, pod, thr, ring_days=3, cells_per_block=cpb)
    assert_matches(summ, days, own, pod, 2, thr)
    for k in ALL:        # ... which is the default tiles' fetch as well
        assert np.array_equal(bits(own[k]), bits(plain_fetch("s355_h005")[0][k])), k


def test_4_array_forcing_uploaded_per_chunk_and_coarse_array_forcing():
    a = synthetic.workload(4, 6, 48, variety=True, na_frac=0.1, start_doy=170, array_forcing=True)
    assert np.isnan(np.asarray(a["vegp"]["hgt"])).any()
    pod = [0, 1]
    summ, days, own, _ = run_plan(a, pod, 15.0, ring_days=1, array_forcing=True, upload=True, nperiods=3)
    assert days.tolist() == [1, 1, 0]
    assert_matches(summ, days, own, pod, 3, 15.0)
    assert (bits(summ["Tz", "mean"][:, :, 2]) == SR.NA_BITS).all()              # a period without a counted day
    one = api.runmicro_summary(*[a[k] for k in ARGS], periods=pod, nperiods=3, vars=ALL, stats=STATS, thresholds=15.0, chunk_days=1,
                               array_forcing=True)
    for (v, s), plane in summ.items():
        assert np.array_equal(bits(one[v][s]), bits(plane)), (v, s)
    c, rp, cp = synthetic.coarse_workload(4, 6, 48, 2, 2, variety=True, na_frac=0.1, start_doy=170)
    coarse = {"rowpos": rp, "colpos": cp}
    summ, days, own, _ = run_plan(c, pod, 15.0, ring_days=1, coarse=coarse)
    assert_matches(summ, days, own, pod, 2, 15.0)
    one = api.runmicro_summary(*[c[k] for k in ARGS], periods=pod, vars=ALL, stats=STATS, thresholds=15.0, coarse=coarse)
    for (v, s), plane in summ.items():
        assert np.array_equal(bits(one[v][s]), bits(plane)), (v, s)
    assert one["days"].tolist() == [1, 1]


def test_5_a_day_outside_every_vegetation_layer_takes_its_period():
    a = synthetic.layered(SC.build("s170_h005"), 2, cover_days=3)
    assert list(a["dfsel"]["ed"])[-1] == 71
    pod = [0, 0, 1, 1]
    summ, days, own, _ = run_plan(a, pod, 12.0, ring_days=2)
    assert (bits(own["Tz"][:, :, 72:]) == SR.NA_BITS).all() and np.isfinite(own["Tz"][:, :, :72]).any()
    assert_matches(summ, days, own, pod, 2, 12.0)
    na = np.isnan(np.asarray(a["vegp"]["hgt"])[:, :, 0])
    for (v, s), plane in summ.items():
        assert (bits(plane[:, :, 1]) == SR.NA_BITS).all(), (v, s)
        assert np.isfinite(plane[:, :, 0][~na]).all(), (v, s)
    # ... and through the one call, with dfsel
    b = dict(a)
    dfsel = b.pop("dfsel")
    one = api.runmicro_summary(*[b[k] for k in ARGS], periods=pod, vars=ALL, stats=STATS, thresholds=12.0, chunk_days=3, dfsel=dfsel)
    for (v, s), plane in summ.items():
        assert np.array_equal(bits(one[v][s]), bits(plane)), (v, s)


def test_6_the_sink_changes_nothing():
    a = dict(SC.build("s170_h005"))
    series, st0 = plain_fetch("s170_h005")
    with Plan(**a, ring_days=4) as p:
        p.summary_enable([0, 0, 1, 1], ALL, STATS, 10.0)
        p.run_days(0, 4, 0)
        before = {k: p.fetch(0, k, 0, 96) for k in ALL}
        p.summary_accumulate(0, 0, 0, 4)
        p.fetch_summary("Tz", "mean")
        after = {k: p.fetch(0, k, 0, 96) for k in ALL}
        st = p.dispatch_stats()
    for k in ALL:
        assert np.array_equal(bits(before[k]), bits(after[k])) and np.array_equal(bits(after[k]), bits(series[k])), k
    assert st == st0 and st["fast_launches"] + st["slow_launches"] >= 1


def test_7_one_call_and_row_blocks_equal_the_plan_route():
    a = synthetic.workload(6, 7, 72, variety=True, na_frac=0.05, start_doy=200)
    pod = [0, 1, 0]
    sel = ("Tz", "relhum", "Rswup")
    ref, days, own, _ = run_plan(dict(a, out=[k in sel for k in ALL]), pod, 14.0, ring_days=3, vars=sel)
    assert_matches(ref, days, own, pod, 2, 14.0, vars=sel)
    for kw in (dict(chunk_days=1), dict(chunk_days=0), dict(chunk_days=0, devices=[0], n_blocks=3), dict(chunk_days=2, devices=[0], n_blocks=3)):
        got = api.runmicro_summary(*[a[k] for k in ARGS], periods=pod, vars=sel, stats=STATS, thresholds=14.0, **kw)
        assert got["days"].tolist() == [2, 1] and sorted(k for k in got if k != "days") == sorted(sel)
        for (v, s), plane in ref.items():
            assert np.array_equal(bits(got[v][s]), bits(plane)), (v, s, kw)


def test_8_front_end_on_the_bundled_site_and_a_diagnostics_plan():
    from bundled import load
    weather, vegp, soilc, dtm = load()
    mx = frontend.subsetpointmodel(frontend.runpointmodel(weather, 0.05, dtm, vegp, soilc), what="tmax")
    assert len(mx["obstime"]["year"]) == 288
    sel, stats = ("Tz", "soilm", "Rswup"), ("mean", "max", "mean_daily_min", "hours_above")
    got = frontend.runmicro_summary(mx, 0.05, vegp, soilc, dtm, periods="month", vars=sel, stats=stats, thresholds={"Tz": 20.0, "soilm": 0.3, "Rswup": 50.0})
    full = frontend.runmicro(mx, 0.05, vegp, soilc, dtm, out=[k in sel for k in ALL])
    tab, labels = frontend.summary_periods(mx["obstime"], "month")
    assert got["periods"] == labels and len(labels) == 12 and got["days"].tolist() == [1] * 12
    for v, t in zip(sel, (20.0, 0.3, 50.0)):
        want, _ = SR.summarise(full[v], tab, 12, t)
        for s in stats:
            assert np.array_equal(bits(got[v][s]), bits(want[s])), (v, s)
    assert np.isnan(got["Tz"]["mean"]).any() and np.isfinite(got["Tz"]["mean"]).any()
    # reqhgt == 0 masks the variables as runmicro does
    g0 = frontend.runmicro_summary(mx, 0.0, vegp, soilc, dtm, periods="all", vars=("Tz", "tleaf", "windspeed"), stats=("min",))
    assert sorted(k for k in g0 if k not in ("periods", "days")) == ["Tz"] and g0["Tz"]["min"].shape[2] == 1
    # a summary on a diagnostics plan: it reads the ten outputs only
    a = dict(SC.build("s170_h005"))
    thr = thresholds(plain_fetch("s170_h005")[0])
    with Plan(**a, ring_days=4) as p:
        p.diag_enable(["T0", "uf"])
        p.summary_enable([0, 1, 1, 0], ("Tz", "windspeed"), STATS, thr)
        p.run_days(0, 4, 0)
        p.summary_accumulate(0, 0, 0, 4)
        for v in ("Tz", "windspeed"):
            want, _ = SR.summarise(p.fetch(0, v, 0, 96), [0, 1, 1, 0], 2, thr[v])
            for s in STATS:
                assert np.array_equal(bits(p.fetch_summary(v, s)), bits(want[s])), (v, s)


def test_9_refusals_and_state_errors_on_the_device():
    a = dict(SC.build("s170_h005"), out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0])
    E1, E5 = r"error 1: .*", r"error 5: .*"
    with Plan(**a, ring_days=2) as p:
        with pytest.raises(_abi.McfError, match=E5 + "mcf_plan_summary_enable first"):
            p.summary_accumulate(0, 0, 0, 1)
        with pytest.raises(_abi.McfError, match=E5 + "mcf_plan_summary_enable first"):
            p.fetch_summary("Tz", "mean")
        with pytest.raises(_abi.McfError, match=E5):
            p.summary_days()
        with pytest.raises(_abi.McfError, match=E5):
            p.summary_reset()
        with pytest.raises(_abi.McfError, match=E1 + "not requested"):
            p.summary_enable([0, 0, 1, 1], ("Tz", "tleaf"))
        with pytest.raises(_abi.McfError, match=E1 + "no variable"):
            p.summary_enable([0, 0, 1, 1], ())
        with pytest.raises(_abi.McfError, match=E1 + "no statistic"):
            p.summary_enable([0, 0, 1, 1], ("Tz",), ())
        with pytest.raises(_abi.McfError, match=E1 + "nperiods"):
            p.summary_enable([0, 0, 1, 1], ("Tz",), nperiods=0)
        with pytest.raises(_abi.McfError, match=E1 + "outside"):
            p.summary_enable([0, 0, 1, 1], ("Tz",), nperiods=1)
        with pytest.raises(_abi.McfError, match=E1 + "threshold"):
            p.summary_enable([0, 0, 1, 1], ("Tz",), ("hours_above",))
        p.summary_enable([0, 0, 1, 1], ("Tz", "soilm"), ("mean", "max"))
        with pytest.raises(_abi.McfError, match=E5 + "already enabled"):
            p.summary_enable([0, 0, 1, 1], ("Tz",))
        with pytest.raises(_abi.McfError, match=E1 + "was not selected"):
            p.fetch_summary("Tz", "min")
        with pytest.raises(_abi.McfError, match=E1 + "was not selected"):
            p.fetch_summary("tleaf", "mean")
        for bad in ((1, 0, 0, 1), (0, 1, 0, 2), (0, 0, 3, 2), (0, 0, -1, 1), (0, 0, 0, 0)):       # slot, slot days, calendar days
            with pytest.raises(_abi.McfError, match=E1):
                p.summary_accumulate(*bad)
        p.run_days(0, 2, 0)
        p.summary_accumulate(0, 0, 0, 2)
        with pytest.raises(_abi.McfError, match=E5 + "ascending order"):
            p.summary_accumulate(0, 0, 1, 1)                      # day 1 again
        with pytest.raises(_abi.McfError, match=E5 + "ascending order"):
            p.summary_accumulate(0, 0, 0, 1)
        first = p.fetch_summary("Tz", "mean")
        assert p.summary_days().tolist() == [2, 0] and (bits(first[:, :, 1]) == SR.NA_BITS).all()
        p.run_days(3, 1, 0)                                       # day 2 is never folded: a gap is fine
        p.summary_accumulate(0, 0, 3, 1)
        assert p.summary_days().tolist() == [2, 1]
        p.summary_reset()
        assert p.summary_days().tolist() == [0, 0]
        p.run_days(0, 2, 0)
        p.summary_accumulate(0, 0, 0, 2)                          # after a reset any day may come first
        assert np.array_equal(bits(p.fetch_summary("Tz", "mean")), bits(first))
    below = dict(SC.build("s170_h005"), reqhgt=-0.05, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0])
    for kw in (dict(ring_days=4), dict(ring_days=2, stream_below=True)):
        with Plan(**below, **kw) as p:
            with pytest.raises(_abi.McfError, match=E1 + ("streamed plan" if "stream_below" in kw else "reqhgt >= 0")):
                p.summary_enable([0, 0, 1, 1], ("Tz",))


@pytest.mark.parametrize("cpb", (16, 21, 32, 42))
def test_10_more_than_one_workgroup(cpb):
    """17 x 31 = 527 cells: a workgroup of the accumulate kernel takes at most 256 cells (16 x 16, 12 x 21, 8 x 32, 6 x 42), so
    every tile size has three workgroups per variable here, the last with tiles missing and a partial tile"""
    a = synthetic.workload(17, 31, 72, variety=True, na_frac=0.03, start_doy=120, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 1])
    sel = ("Tz", "soilm", "Rlwup")
    pod = [1, 0, 1]
    summ, days, own, _ = run_plan(a, pod, {"Tz": 11.0, "soilm": 0.25, "Rlwup": 380.0}, ring_days=2, vars=sel, cells_per_block=cpb)
    assert_matches(summ, days, own, pod, 2, {"Tz": 11.0, "soilm": 0.25, "Rlwup": 380.0}, vars=sel)
    assert np.isnan(summ["Tz", "mean"]).any() and np.isfinite(summ["Tz", "mean"]).sum() > 2 * 256
