"""Period summaries of the snow run and of the snowpack, folded on the device (include/mcf.h "period summaries of the snow run
and of the snowpack").  The yardstick is tests/summary_ref.summarise — the header's definition as a literal
numpy loop — on the arrays the library's own array route returns for the same inputs: every plane bit for bit, NA_real_'s
payload included."""
import numpy as np
import pytest

from microclimf_amd import McfError, _abi
from microclimf_amd import snow as S
from summary_ref import STATS, bits, summarise
from test_snowrun_gpu import MAT, _case, _steps

pytestmark = pytest.mark.gpu
SERIES = _abi.SNOWDRIVER_OUT
# straddles the 5-day chunks, has an uncounted day and a period that is not contiguous
TAB20 = np.array([0] * 7 + [-1] + [1] * 6 + [0] * 6, dtype=np.int32)
TAB22 = np.concatenate([TAB20, [-1, -1]]).astype(np.int32)      # 22 days: four chunks, the two days behind them belong to none


def _occurring(x):
    """a threshold that occurs in the series: the middle one of its finite values (0 for a series without one: a variable that
    is masked at ground level)"""
    v = np.sort(np.asarray(x)[np.isfinite(x)])
    return float(v[v.size // 2]) if v.size else 0.0


def _same_planes(planes, arrays, tab, nperiods, thr, what):
    names = [k for k in planes if k not in ("days", "snow")]
    assert names, what
    for name in names:
        want, days = summarise(arrays[name], tab, nperiods, thr[name])
        assert np.array_equal(planes["days"], days), (what, name, planes["days"], days)
        assert sorted(planes[name]) == sorted(STATS), (what, name)
        for st in STATS:
            g = planes[name][st]
            assert g.shape == want[st].shape, (what, name, st)
            bad = int(np.count_nonzero(bits(g) != bits(want[st])))
            assert bad == 0, (what, name, st, bad)


def _summary(names, thr, tab=TAB20):
    return dict(periods=tab, nperiods=2, vars=names, stats=STATS, thresholds=thr)


@pytest.fixture(scope="module")
def base():
    """22 x 13 cells x 20 days in 5-day chunks: the arrays of the one-call run, the thresholds taken from them"""
    sw, a, dtm, snow, micro = _case(0.05, 0.0, 90)
    arrays, smod = S.runmicrosnow1(a, snow, micro, MAT, want_smod=True)
    thr = {k: _occurring(v) for k, v in arrays.items()}
    return dict(sw=sw, a=a, dtm=dtm, snow=snow, micro=micro, arrays=arrays, smod=smod, thr=thr)


def test_the_base_case_is_not_degenerate(base):
    with S.SnowRun(base["a"], base["snow"]) as run:
        sd, nd = run.pass1()
    sdays, ndays_ = np.flatnonzero(sd), np.flatnonzero(nd)
    assert np.setdiff1d(ndays_, sdays).size > 0 and np.setdiff1d(sdays, ndays_).size > 0 and (sd & nd).sum() >= 1
    swe = np.nan_to_num(base["smod"]["totalSWE"])
    covered = swe[:, :, _steps(sdays)] > 0
    assert covered.any() and (~covered & ~np.isnan(base["dtm"])[:, :, None]).any() and np.isnan(base["dtm"]).any()
    assert len(base["arrays"]) == 10
    res = S.runmicrosnow1(base["a"], base["snow"], base["micro"], MAT, summary=_summary(list(base["arrays"]), base["thr"]),
                          want_arrays=False)
    assert np.array_equal(res["snowdays"], sd) and np.array_equal(res["nosnowdays"], nd) and res["out"] is None
    _same_planes(res["summary"], base["arrays"], TAB20, 2, base["thr"], "one call, summary only")
    assert np.array_equal(res["summary"]["days"], [13, 6])


def test_ground_level_masked_variables():
    sw, a, dtm, snow, micro = _case(0.0, 3.0, 120)
    arrays = S.runmicrosnow1(a, snow, micro, MAT)
    thr = {k: _occurring(v) for k, v in arrays.items()}
    res = S.runmicrosnow1(a, snow, micro, MAT, summary=_summary(list(arrays), thr), want_arrays=False)
    _same_planes(res["summary"], arrays, TAB20, 2, thr, "reqhgt 0")


def test_the_sink_changes_nothing_and_summary_only_gives_the_same_planes(base):
    a, snow, micro = base["a"], base["snow"], base["micro"]
    with S.SnowRun(a, snow) as run:
        sd0, nd0, smod0 = run.pass1(want_smod=True)
        out0, st0 = run.pass2(micro, MAT), run.stats()
    with S.SnowRun(a, snow) as run:
        run.summary_enable(_summary(list(out0), base["thr"]), dict(periods=TAB20, nperiods=2, vars=SERIES, stats=STATS, thresholds=0.0))
        sd1, nd1, smod1 = run.pass1(want_smod=True)
        out1, st1 = run.pass2(micro, MAT), run.stats()
        with_arrays = run.fetch_summary()
    assert np.array_equal(sd0, sd1) and np.array_equal(nd0, nd1) and st0 == st1, (st0, st1)
    for k in out0:
        assert np.array_equal(bits(out0[k]), bits(out1[k])) and np.array_equal(bits(out0[k]), bits(base["arrays"][k])), k
    for k in smod0:
        assert np.array_equal(bits(smod0[k]), bits(smod1[k])), k
    _same_planes(with_arrays, out0, TAB20, 2, base["thr"], "sink beside the arrays")
    with S.SnowRun(a, snow) as run:
        run.summary_enable(_summary(list(out0), base["thr"]))
        run.pass1()
        assert run.pass2(micro, MAT, want_arrays=False) is None
        only = run.fetch_summary()
    for k in out0:
        for st in STATS:
            assert np.array_equal(bits(only[k][st]), bits(with_arrays[k][st])), (k, st)


def test_row_blocks_with_host_threads(base):
    a, snow, micro = base["a"], base["snow"], base["micro"]
    kw = dict(devices=[0, 0], n_blocks=3)
    arrays, smod = S.runmicrosnow1(a, snow, micro, MAT, want_smod=True, **kw)
    thr = {k: _occurring(v) for k, v in arrays.items()}
    pthr = dict({k: _occurring(v) for k, v in smod.items()}, totalSWE=0.0)
    res = S.runmicrosnow1(a, snow, micro, MAT, summary=_summary(list(arrays), thr),
                          pack_summary=dict(periods=TAB20, nperiods=2, vars=SERIES, stats=STATS, thresholds=pthr), want_arrays=False, **kw)
    _same_planes(res["summary"], arrays, TAB20, 2, thr, "3 row blocks")
    _same_planes(res["summary"]["snow"], smod, TAB20, 2, pthr, "3 row blocks, snowpack")


def test_kept_chunks_and_a_second_year(base):
    a, snow, micro = base["a"], base["snow"], base["micro"]
    names = ["Tz", "soilm", "Rswup"]
    with S.SnowRun(a, snow) as run:
        run.keep(1.0)
        run.summary_enable(_summary(names, base["thr"]), dict(periods=TAB20, nperiods=2, vars=("totalSWE",), stats=STATS, thresholds=0.0))
        for year in (1, 2):
            run.pass1()
            run.pass2(micro, MAT, want_arrays=False)
            st = run.stats()
            res = run.fetch_summary()
            assert st["chunks_kept"] >= 1, st
            _same_planes(res, base["arrays"], TAB20, 2, base["thr"], f"kept chunks, year {year}")
            _same_planes(res["snow"], base["smod"], TAB20, 2, {"totalSWE": 0.0}, f"kept chunks, year {year}, snowpack")


def test_array_weather():
    from test_snowrun2_gpu import MAT as MAT2
    from test_snowrun2_gpu import _case as case2
    sw, a, dtm, snow, micro = case2(0.05, 0.0, 90)
    arrays = S.runmicrosnow2(a, snow, micro, MAT2)
    tab = np.array([0] * 4 + [-1] + [1] * 5 + [0] * 5, dtype=np.int32)
    thr = {k: _occurring(v) for k, v in arrays.items()}
    res = S.runmicrosnow2(a, snow, micro, MAT2, summary=_summary(list(arrays), thr, tab), want_arrays=False)
    _same_planes(res["summary"], arrays, tab, 2, thr, "array weather")


@pytest.fixture(scope="module")
def pack22():
    """22 days: four whole chunks and two days no chunk covers"""
    sw, a, dtm, snow, micro = _case(0.05, 0.0, 90, ndays=22)
    args = (sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
    series = S.snowmodel1_chunks(*args)
    assert all(np.isnan(v[:, :, 480:]).all() for v in series.values()) and (np.nan_to_num(series["totalSWE"]) > 0).any()
    thr = dict({k: _occurring(v) for k, v in series.items()}, totalSWE=0.0)
    return dict(a=a, snow=snow, micro=micro, args=args, series=series, thr=thr)


def test_snowpack_summaries(pack22):
    kw = dict(periods=TAB22, nperiods=2, vars=SERIES, stats=STATS, thresholds=pack22["thr"])
    alone = S.snowmodel1_summary(*pack22["args"], **kw)
    _same_planes(alone, pack22["series"], TAB22, 2, pack22["thr"], "snow model alone")
    # snow-cover duration and peak snow water equivalent are what the issue names
    swe = pack22["series"]["totalSWE"]
    counted = np.repeat(TAB22 >= 0, 24)
    peak = np.fmax(alone["totalSWE"]["max"][:, :, 0], alone["totalSWE"]["max"][:, :, 1])
    fin = np.isfinite(peak)
    assert fin.any() and np.array_equal(peak[fin], swe[:, :, counted].max(axis=2)[fin])
    blocks = dict(devices=[0, 0], n_blocks=3)
    series_b = S.snowmodel1_chunks(*pack22["args"], **blocks)
    _same_planes(S.snowmodel1_summary(*pack22["args"], **kw, **blocks), series_b, TAB22, 2, pack22["thr"], "snow model, 3 row blocks")
    with S.SnowRun(pack22["a"], pack22["snow"]) as run:
        run.summary_enable(None, kw)
        run.pass1()
        through = run.fetch_summary()["snow"]
    assert np.array_equal(through["days"], alone["days"])
    for k in SERIES:
        for st in STATS:
            assert np.array_equal(bits(through[k][st]), bits(alone[k][st])), (k, st)


def test_planes_kernel_geometry():
    """17 x 31 cells: three workgroups of 256 lanes, the last one partial"""
    sw, a, dtm, snow, micro = _case(0.05, 0.0, 90, rows=17, cols=31, ndays=10)
    args = (sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
    series = S.snowmodel1_chunks(*args)
    tab = np.array([1, 1, 0, -1, 0, 0, 1, 1, 1, 0], dtype=np.int32)
    thr = dict({k: _occurring(v) for k, v in series.items()}, totalSWE=0.0)
    got = S.snowmodel1_summary(*args, periods=tab, nperiods=3, vars=SERIES, stats=STATS, thresholds=thr)      # (period 2: no day)
    _same_planes(got, series, tab, 3, thr, "17 x 31")
    assert np.array_equal(got["days"], [4, 5, 0])


def test_front_end_on_the_bundled_site():
    from bundled import load
    from microclimf_amd import frontend as F
    weather, vegp, soilc, dtm = load(25 * 24)
    t = np.arange(25 * 24)
    weather = dict(weather, temp=weather["temp"] - 9.0 + 7.0 * (t > 8 * 24) + 6.0 * (t > 16 * 24))      # (test_frontend_snow_below_gpu.py)
    mp = F.runpointmodel(weather, 0.05, dtm, vegp, soilc)
    sin = F.runsnowmodel(weather, mp, vegp, soilc, dtm, inputs_only=True)
    arrays = F.runmicro_snow(mp, 0.05, vegp, soilc, dtm, None, one_call=True, snow_inputs=sin)
    tab = np.array([0] * 7 + [1] * 6 + [-1] + [1] * 11, dtype=np.int32)
    names = ("Tz", "soilm")
    thr = {k: _occurring(arrays[k]) for k in names}
    got = F.runmicro_snow_summary(mp, 0.05, vegp, soilc, dtm, sin, periods=tab, vars=names, stats=STATS, thresholds=thr,
                                  snow_vars=("totalSWE", "Tg"), snow_stats=STATS)
    assert got["snowdays"].sum() > 0 and got["nosnowdays"].sum() > 0 and got["periods"] == [0, 1]
    _same_planes({k: got[k] for k in names + ("days",)}, arrays, tab, 2, thr, "front end")
    smod = F.runsnowmodel(weather, mp, vegp, soilc, dtm)
    zero = {"totalSWE": 0.0, "Tg": 0.0}
    _same_planes(got["snow"], smod, tab, 2, zero, "front end, snowpack through the snow run")
    alone = F.runsnowmodel_summary(weather, mp, vegp, soilc, dtm, periods=tab, vars=("totalSWE", "Tg"), stats=STATS)
    assert alone.pop("periods") == [0, 1]
    _same_planes(alone, smod, tab, 2, zero, "runsnowmodel_summary")


def test_stepwise_snow_plan_entries(pack22):
    """the chunk loop driven from Python: fold behind every run_chunk; the order and mask rules of the accumulate"""
    kw = dict(vars=SERIES, stats=STATS, thresholds=pack22["thr"], nperiods=2)
    with S.SnowPlan(*pack22["args"], keep_results=False) as p:
        with pytest.raises(McfError, match="mcf_snowplan_summary_enable first"):
            p.summary_accumulate(0)
        p.summary_enable(TAB22, **kw)
        with pytest.raises(McfError, match="already enabled"):
            p.summary_enable(TAB22, **kw)
        for year in (1, 2):
            for ch in range(p.chunks):
                ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
                if ch == 1 and year == 1:
                    p.set_series(S.SnowPlan.SERIES_PASS1)
                    p.run_chunk(ch, ts / tn)
                    with pytest.raises(McfError, match="switched off"):
                        p.summary_accumulate(ch)
                    p.set_series(S.SnowPlan.SERIES_ALL)
                    break
                p.run_chunk(ch, ts / tn)
                p.summary_accumulate(ch)
                with pytest.raises(McfError, match="ascending order"):
                    p.summary_accumulate(ch)
            p.reset()
            p.summary_reset()
        for ch in range(p.chunks):
            ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
            p.run_chunk(ch, ts / tn)
            p.summary_accumulate(ch)
        _same_planes(p.fetch_summary(), pack22["series"], TAB22, 2, pack22["thr"], "stepwise")


def test_device_side_errors(base):
    a, snow, micro = base["a"], base["snow"], base["micro"]
    spec = _summary(["Tz"], base["thr"])
    with S.SnowRun(a, snow) as run:
        run.summary_enable(spec)
        with pytest.raises(McfError, match="already enabled"):
            run.summary_enable(spec)
        with pytest.raises(McfError, match="after mcf_snowrun_pass2"):
            run.fetch_summary()
    with S.SnowRun(a, snow) as run:
        run.pass1()
        with pytest.raises(McfError, match="before mcf_snowrun_pass1"):
            run.summary_enable(spec)
    with S.SnowRun(dict(a, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0]), snow) as run:
        with pytest.raises(McfError, match="not requested"):
            run.summary_enable(_summary(["Tz", "tleaf"], base["thr"]))
    sw, ab, dtm, snowb, microb = _case(-0.1, 0.0, 90, rows=10, cols=9, ndays=10)
    with S.SnowRun(ab, snowb, below=True) as run:
        with pytest.raises(McfError, match="reqhgt >= 0"):
            run.summary_enable(_summary(["Tz"], {"Tz": 0.0}, np.zeros(10, np.int32)))
