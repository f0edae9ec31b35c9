"""The series sink's further sources on the device (include/mcf.h "series sink: further sources"): the planes kernel through
mcf_zonal_series' MCF_ZONAL_CPB=0 door, the snowpack, the snow run, row blocks and soil depths.  The yardstick is
tests/series_ref.py on the arrays the library's own array route returns for the same inputs (the same devices and row blocks
where there are any: a snow model cut into row blocks differs from the one-block model in the last bits of two raster-wide
means, so "the one-block run" of the combination is the one-block fold of the same values).  Every comparison is bit for bit,
NA payload included; no tolerance appears anywhere."""
import numpy as np
import pytest

import series_ref as ZR
import stages_cases as SC
import summary_ref as SR
from microclimf_amd import McfError, _abi, api, frontend
from microclimf_amd import snow as S
from microclimf_amd.api import Plan
from test_series_gpu import crafted
from test_snowrun_gpu import MAT, _case

pytestmark = pytest.mark.gpu
ALL = _abi.OUT_NAMES
SERIES = _abi.SNOWDRIVER_OUT
ZS = _abi.ZSTAT_NAMES
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "complete", "mat")
bits = ZR.bits
NA = ZR.NA_BITS


def same(got, want, what):
    assert got.shape == want.shape and got.flags.f_contiguous, what
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:3].tolist(), got[diff][:3], want[diff][:3])


def same_sink(res, arrays, names, cells, zone, nz, steps_done, what):
    """res: {name: {"points": [T, np], "zones": {stat: [T, nz]}}} against the yardstick on arrays[name]"""
    for v in names:
        pts = ZR.point_series(arrays[v], cells)
        if steps_done is not None:
            pts.view(np.uint64)[~np.asarray(steps_done)] = NA
        same(res[v]["points"], pts, (what, v, "points"))
        want = ZR.zone_series(arrays[v], zone, nz, steps_done=steps_done)
        for s in ZS:
            same(res[v]["zones"][s], want[s], (what, v, s))


def not_degenerate(arrays, names, zone, nz, cells, na):
    """every selected variable has finite values, all inside the range; a zone-step with and one without a counted value; the
    NA cell is among the points"""
    assert na in [int(c) for c in cells]
    for v in names:
        x = arrays[v][np.isfinite(arrays[v])]
        assert x.size and (np.abs(x) < ZR.LIMIT).all(), v
        cnt = ZR.zone_series(arrays[v][:, :, :24], zone, nz)["count"]
        assert (cnt > 0).any() and (cnt == 0).any(), v


# ---- 1. the planes kernel through the door -----------------------------------------------------------------------------------
def door(x, zone, nz, monkeypatch, what):
    """x through MCF_ZONAL_CPB=0 (k_series_planes) -> compared with the yardstick and with the default tiled route"""
    monkeypatch.delenv("MCF_ZONAL_CPB", raising=False)
    tiled = api.zonal_series(x, zone, ZS, nzones=nz)
    monkeypatch.setenv("MCF_ZONAL_CPB", "0")
    got = api.zonal_series(x, zone, ZS, nzones=nz)
    want = ZR.zone_series(x, zone, nz)
    for s in ZS:
        same(got[s], want[s], (what, s))
        same(got[s], tiled[s], (what, s, "tiled route"))
    return got


@pytest.mark.parametrize("nsteps", (1, 30, 48))
def test_1_planes_kernel_on_crafted_values(nsteps, monkeypatch):
    """259 cells in two spans of 256 lanes: -0.0, half-quantum ties, NaN and NA_real_, 4096 - 2^-24, +-4096, +-inf; cells 64 ..
    127 fill exactly one wave with one label beside waves of mixed labels; cell 258 is a zone of its own.  30 steps end in a
    day of 6 steps, 1 step in a day of one, 48 are whole days."""
    x30, zone, nz = crafted()
    x = np.asfortranarray(np.concatenate([x30, x30[:, :, :18]], axis=2)[:, :, :nsteps])
    got = door(x, zone, nz, monkeypatch, f"{nsteps} steps")
    assert got["count"][0, 6] == 64 and got["count"][0, 7] == 1
    if nsteps >= 30:
        q = ZR.QUANTUM
        for s in ("mean", "min", "max"):
            assert got[s][3, 7] == 0.0 and not np.signbit(got[s][3, 7]) and got[s][16, 6] == 0.0 and not np.signbit(got[s][16, 6]), s
            for k, z in ((8, 2), (9, 3), (10, 4), (11, 6)):
                assert bits(got[s])[k, z] == NA and (bits(got[s])[k, [j for j in range(nz) if j != z]] != NA).all(), (s, k, z)
            assert bits(got[s])[13, 7] == NA and bits(got[s])[14, 6] == NA, s
        assert got["mean"][4:8, 7].tolist() == [10 * q, 12 * q, -10 * q, -12 * q] and got["max"][7, 1] == 4096.0 - q
        assert got["count"][13, 7] == 0 and got["count"][14, 6] == 0 and got["count"][11, 6] == 63


def test_1b_a_single_cell(monkeypatch):
    x = np.asfortranarray(np.arange(30, dtype=np.float64).reshape(1, 1, 30) - 7.25)
    x[0, 0, 4] = np.nan
    got = door(x, np.zeros((1, 1), np.int32), 1, monkeypatch, "1 x 1")
    assert got["mean"][5, 0] == -2.25 and got["count"][4, 0] == 0 and bits(got["max"])[4, 0] == NA


def test_1c_many_workgroups_fold_into_one_table(monkeypatch):
    """300 x 300 cells x 24 h, 64 speckled zones: 352 spans for at most one workgroup per compute unit, every wave mixed; integer
    values, so the yardstick's mean is the true mean"""
    rng = np.random.default_rng(6)
    x = np.asfortranarray(rng.integers(-3000, 3000, size=(300, 300, 24)).astype(np.float64))
    x[rng.random((300, 300)) < 0.02] = np.nan
    zone = ((np.arange(90000) * 13) % 64).reshape((300, 300), order="F").astype(np.int32)
    got = door(x, zone, 64, monkeypatch, "300 x 300")
    flat, zf = x.reshape(90000, 24, order="F"), zone.reshape(-1, order="F")
    for zz in (0, 31, 63):
        v = flat[zf == zz]
        assert (got["count"][:, zz] == (~np.isnan(v)).sum(axis=0)).all() and (got["mean"][:, zz] == np.nansum(v, axis=0) / got["count"][:, zz]).all()


# ---- the snow cases: 22 x 13 cells, 5-day chunks -----------------------------------------------------------------------------
ROWS, COLS = 22, 13
CELLS = np.arange(ROWS * COLS).reshape((ROWS, COLS), order="F")      # cell index row + rows * col
BLOCK_ROWS = [(ROWS * b // 3, ROWS * (b + 1) // 3) for b in range(3)]  # the rows of three row blocks


def snow_na_cell(x):
    """the first cell that is NA in the [rows, cols] raster x, or at every step of the [rows, cols, steps] array x"""
    na = np.isnan(x) if x.ndim == 2 else np.isnan(x).all(axis=2)
    assert na.any()
    return int(CELLS[na][0])


def snow_points(na):
    """the NA cell, the last cell, one per would-be row block, and one more"""
    return [na, ROWS * COLS - 1] + [int(CELLS[r0 + 1, 2 + b]) for b, (r0, _) in enumerate(BLOCK_ROWS)] + [int(CELLS[10, 7])]


def snow_zones(which, na):
    if which == "one":
        return np.zeros((ROWS, COLS), dtype=np.int32), 1
    if which == "bands":       # row bands with holes, the last column all zone 0; zone 3 is the NA cell alone (count 0); zone 4
        z = np.repeat(np.array([0] * 9 + [1] * 8 + [2] * 5), COLS).reshape(ROWS, COLS)      # lies inside the middle block
        z[:, COLS - 1] = 0
        z[CELLS % 7 == 3] = -1
        z[9:12, 3:6] = 4
        z[CELLS == na] = 3
        return z.astype(np.int32), 5
    z = ((CELLS * 13) % 64).astype(np.int32)
    z[CELLS == na] = 63      # (the table's last label, and a zone without a counted value)
    z[(z == 63) & (CELLS != na)] = 62
    return z, 64


@pytest.fixture(scope="module", params=(20, 22), ids=["20d", "22d"])
def pack(request):
    """the snow model's five series by the array route; 22 days: four whole chunks and two days no chunk covers"""
    nd = request.param
    sw, a, dtm, snow, micro = _case(0.05, 0.0, 90, ndays=nd)
    args = (sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
    series = S.snowmodel1_chunks(*args)
    for v in series.values():
        v.setflags(write=False)
    done = np.arange(nd * 24) < 480
    return dict(nd=nd, dtm=dtm, args=args, series=series, done=done)


# ---- 2. the snowpack -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("one", "bands", "speckled"))
def test_2_snowpack_series_of_the_snow_model_alone(pack, which):
    na = snow_na_cell(pack["dtm"])
    cells = snow_points(na)
    z, nz = snow_zones(which, na)
    if which == "bands":
        not_degenerate(pack["series"], SERIES, z, nz, cells, na)
        assert (np.nan_to_num(pack["series"]["totalSWE"]) > 0).any()
    got = S.snowmodel1_series(*pack["args"], points=cells, zones=z, nzones=nz, vars=SERIES, stats=ZS)
    res = {v: {"points": got["points"][v], "zones": got["zones"][v]} for v in SERIES}
    same_sink(res, pack["series"], SERIES, cells, z, nz, pack["done"], f"snowmodel1_series, {which}")
    for v in SERIES:
        assert np.isnan(res[v]["points"][:, 0]).all() and np.isfinite(res[v]["points"][:480, 1:]).any(), v      # (the NA cell first)
        if pack["nd"] == 22:       # the two days behind the last chunk: NA in every statistic, the count included
            for s in ZS:
                assert (bits(res[v]["zones"][s][480:]) == NA).all() and (bits(res[v]["zones"][s][:480, 0]) != NA).any(), (v, s)
            assert (bits(res[v]["points"][480:]) == NA).all()


def test_2b_stepwise_snow_plan_with_the_chunks_folded_in_descending_order(pack):
    na = snow_na_cell(pack["dtm"])
    cells = snow_points(na)
    z, nz = snow_zones("bands", na)
    with S.SnowPlan(*pack["args"], keep_results=False) as p:
        for call in (lambda: p.series_accumulate(0), p.series_reset):
            with pytest.raises(McfError, match="error 5: .*mcf_snowplan_series_enable first"):
                call()
        p.series_enable(cells, z, SERIES, ZS, nzones=nz)
        with pytest.raises(McfError, match="error 5: mcf_snowplan_series_enable: .*already enabled"):
            p.series_enable(cells, z, SERIES, ZS, nzones=nz)
        for ch in range(p.chunks):                                # the model runs forwards: the start state of every chunk is kept
            p.checkpoint(ch)
            ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
            p.run_chunk(ch, ts / tn)
        for ch in reversed(range(p.chunks)):                      # ... and each chunk is run again from it, the last one first
            if ch == 1:                                           # a run that leaves a selected series out cannot be folded
                p.restore(ch)
                ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
                p.set_series(S.SnowPlan.SERIES_PASS1)
                p.run_chunk(ch, ts / tn)
                with pytest.raises(McfError, match="error 5: mcf_snowplan_series_accumulate: .*switched off"):
                    p.series_accumulate(ch)
                p.set_series(S.SnowPlan.SERIES_ALL)
            p.restore(ch)
            ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
            p.run_chunk(ch, ts / tn)
            p.series_accumulate(ch)
            with pytest.raises(McfError, match="error 5: mcf_snowplan_series_accumulate: .*folded already"):
                p.series_accumulate(ch)
        with pytest.raises(McfError, match="error 1: mcf_snowplan_series_accumulate: chunk out of range"):
            p.series_accumulate(p.chunks)
        res = {v: {"points": p.fetch_point_series(v), "zones": {s: p.fetch_zone_series(v, s) for s in ZS}} for v in SERIES}
        same_sink(res, pack["series"], SERIES, cells, z, nz, pack["done"], "stepwise, descending")
        p.series_reset()
        assert (bits(p.fetch_zone_series("Tc", "count")) == NA).all() and (bits(p.fetch_point_series("Tc")) == NA).all()
    with S.SnowPlan(*pack["args"], keep_results=False) as p:
        with pytest.raises(McfError, match="error 1: mcf_snowplan_series_enable: .*no series selected"):
            p.series_enable(cells, z, (), ZS, nzones=nz)


# ---- 3. the snow run -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    """20 days: the arrays of the one-call run, the snow model's series and the day classes"""
    sw, a, dtm, snow, micro = _case(0.05, 0.0, 90)
    with S.SnowRun(a, snow) as run:
        sd, nd, smod = run.pass1(want_smod=True)
        arrays, stats = run.pass2(micro, MAT), run.stats()
    for v in list(arrays.values()) + list(smod.values()):
        v.setflags(write=False)
    na = snow_na_cell(arrays["Tz"])            # (NA in the solver's rasters: a cell of the snow model's NA cells)
    assert np.isnan(dtm.reshape(-1, order="F")[na])
    cells = snow_points(na)
    z, nz = snow_zones("bands", na)
    return dict(a=a, dtm=dtm, na=na, snow=snow, micro=micro, arrays=arrays, smod=smod, sd=sd, nd=nd, stats=stats, cells=cells, z=z, nz=nz,
                done=np.repeat((sd | nd).astype(bool), 24), sel=dict(points=cells, zones=z, nzones=nz, stats=ZS))


def test_3_series_only_run_equals_the_yardstick_on_the_runs_arrays(base):
    not_degenerate(base["arrays"], ALL, base["z"], base["nz"], base["cells"], base["na"])
    assert len(base["arrays"]) == 10 and base["sd"].sum() > 0 and base["nd"].sum() > 0
    res = S.runmicrosnow1(base["a"], base["snow"], base["micro"], MAT, series=dict(base["sel"], vars=ALL),
                          pack_series=dict(base["sel"], vars=SERIES), want_arrays=False)
    assert res["out"] is None and np.array_equal(res["snowdays"], base["sd"]) and np.array_equal(res["nosnowdays"], base["nd"])
    same_sink(res["series"], base["arrays"], ALL, base["cells"], base["z"], base["nz"], base["done"], "snow run, series only")
    same_sink(res["series"]["snow"], base["smod"], SERIES, base["cells"], base["z"], base["nz"], np.ones(480, bool), "snow run, snowpack")
    for which in ("one", "speckled"):
        z, nz = snow_zones(which, base["na"])
        one = S.runmicrosnow1(base["a"], base["snow"], base["micro"], MAT, series=dict(points=base["cells"], zones=z, nzones=nz, stats=ZS, vars=("Tz", "soilm")),
                              want_arrays=False)
        same_sink(one["series"], base["arrays"], ("Tz", "soilm"), base["cells"], z, nz, base["done"], f"snow run, {which}")


def test_3b_the_sink_beside_the_arrays_changes_no_bit_and_no_stats(base):
    with S.SnowRun(base["a"], base["snow"]) as run:
        run.series_enable(dict(base["sel"], vars=ALL), dict(base["sel"], vars=SERIES))
        with pytest.raises(McfError, match="error 5: mcf_snowrun_series_enable: .*already enabled"):
            run.series_enable(dict(base["sel"], vars=ALL))
        with pytest.raises(McfError, match="error 5: mcf_snowrun_series_fetch_points: .*after mcf_snowrun_pass2"):
            run.fetch_series()
        sd, nd, smod = run.pass1(want_smod=True)
        out, st = run.pass2(base["micro"], MAT), run.stats()
        res = run.fetch_series()
    assert np.array_equal(sd, base["sd"]) and np.array_equal(nd, base["nd"]) and st == base["stats"], (st, base["stats"])
    for k in out:
        same(out[k], base["arrays"][k], ("arrays beside the sink", k))
    for k in smod:
        same(smod[k], base["smod"][k], ("smod beside the sink", k))
    same_sink(res, base["arrays"], ALL, base["cells"], base["z"], base["nz"], base["done"], "sink beside the arrays")
    same_sink(res["snow"], base["smod"], SERIES, base["cells"], base["z"], base["nz"], np.ones(480, bool), "snowpack beside the arrays")
    with S.SnowRun(base["a"], base["snow"]) as run:
        run.pass1()
        with pytest.raises(McfError, match="error 5: mcf_snowrun_series_enable: .*before mcf_snowrun_pass1"):
            run.series_enable(dict(base["sel"], vars=("Tz",)))
    with S.SnowRun(dict(base["a"], out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0]), base["snow"]) as run:
        with pytest.raises(McfError, match="error 1: mcf_snowrun_series_enable: .*not requested"):
            run.series_enable(dict(base["sel"], vars=("Tz", "tleaf")))
    sw, ab, dtm, snowb, microb = _case(-0.1, 0.0, 90, rows=10, cols=9, ndays=10)
    with S.SnowRun(ab, snowb, below=True) as run:
        with pytest.raises(McfError, match="error 1: mcf_snowrun_series_enable: .*reqhgt >= 0"):
            run.series_enable(dict(zones=np.zeros((10, 9), np.int32), vars=("Tz",)))


def test_3c_ground_level_masked_variables():
    sw, a, dtm, snow, micro = _case(0.0, 3.0, 120)
    arrays = S.runmicrosnow1(a, snow, micro, MAT)
    with S.SnowRun(a, snow) as run:
        sd, nd = run.pass1()
    na = snow_na_cell(arrays["Tz"])
    cells = snow_points(na)
    z, nz = snow_zones("bands", na)
    res = S.runmicrosnow1(a, snow, micro, MAT, series=dict(points=cells, zones=z, nzones=nz, stats=ZS, vars=list(arrays)), want_arrays=False)
    assert len(arrays) > 0
    same_sink(res["series"], arrays, list(arrays), cells, z, nz, np.repeat((sd | nd).astype(bool), 24), "reqhgt 0")


def test_3d_kept_chunks_a_second_year_and_beside_the_summary(base):
    names = ["Tz", "soilm", "Rswup"]
    tab = np.array([0] * 7 + [1] * 6 + [-1] + [1] * 6, dtype=np.int32)
    thr = {k: float(np.nanmedian(base["arrays"][k])) for k in names}
    summ = dict(periods=tab, nperiods=2, vars=names, stats=SR.STATS, thresholds=thr)
    psumm = dict(periods=tab, nperiods=2, vars=("totalSWE",), stats=SR.STATS, thresholds=0.0)
    alone = S.runmicrosnow1(base["a"], base["snow"], base["micro"], MAT, summary=summ, pack_summary=psumm, want_arrays=False)["summary"]
    with S.SnowRun(base["a"], base["snow"]) as run:
        run.keep(1.0)
        run.summary_enable(summ, psumm)
        run.series_enable(dict(base["sel"], vars=names), dict(base["sel"], vars=("totalSWE", "Tg")))
        for year in (1, 2):
            run.pass1()
            assert run.pass2(base["micro"], MAT, want_arrays=False) is None
            assert run.stats()["chunks_kept"] >= 1
            res, both = run.fetch_series(), run.fetch_summary()
            same_sink(res, base["arrays"], names, base["cells"], base["z"], base["nz"], base["done"], f"kept chunks, year {year}")
            same_sink(res["snow"], base["smod"], ("totalSWE", "Tg"), base["cells"], base["z"], base["nz"], np.ones(480, bool), f"snowpack, year {year}")
            for k in names:          # the summary beside the series has its stand-alone bits
                for s in SR.STATS:
                    same(both[k][s], alone[k][s], ("summary beside the series", k, s, year))
            for s in SR.STATS:
                same(both["snow"]["totalSWE"][s], alone["snow"]["totalSWE"][s], ("snowpack summary beside the series", s, year))


# ---- 4. row blocks ----------------------------------------------------------------------------------------------------------------
def test_4_row_blocks_of_the_snow_run_and_the_snow_model(base):
    """zone 0 of the band map straddles all three blocks (borders at rows 7 and 14), zone 1 two of them, zone 4 lies inside the
    middle block, every block holds a point"""
    kw = dict(devices=[0, 0], n_blocks=3)
    z, nz, cells = base["z"], base["nz"], base["cells"]
    assert [sum(r0 <= c % ROWS < r1 for c in cells) >= 1 for r0, r1 in BLOCK_ROWS] == [True] * 3
    assert all((z[r0:r1] == 0).any() for r0, r1 in BLOCK_ROWS) and (z[7:14] == 1).any() and (z[14:] == 1).any()
    assert not (z[:7] == 4).any() and not (z[14:] == 4).any() and (z[7:14] == 4).any()
    arrays, smod = S.runmicrosnow1(base["a"], base["snow"], base["micro"], MAT, want_smod=True, **kw)
    with S.SnowRun(base["a"], base["snow"], **kw) as run:
        sd, nd = run.pass1()
    res = S.runmicrosnow1(base["a"], base["snow"], base["micro"], MAT, series=dict(base["sel"], vars=ALL),
                          pack_series=dict(base["sel"], vars=SERIES), want_arrays=False, **kw)
    same_sink(res["series"], arrays, ALL, cells, z, nz, np.repeat((sd | nd).astype(bool), 24), "snow run, 3 row blocks")
    same_sink(res["series"]["snow"], smod, SERIES, cells, z, nz, np.ones(480, bool), "snow run, 3 row blocks, snowpack")
    sw_args = (base["snow"][k] for k in ("obstime", "climdata", "pointm", "vegp", "other", "snowenv"))
    args = tuple(sw_args) + (base["dtm"], 1.0, 0.02)
    series_b = S.snowmodel1_chunks(*args, **kw)
    got = S.snowmodel1_series(*args, points=cells, zones=z, nzones=nz, vars=SERIES, stats=ZS, **kw)
    same_sink({v: {"points": got["points"][v], "zones": got["zones"][v]} for v in SERIES}, series_b, SERIES, cells, z, nz, np.ones(480, bool),
              "snowmodel1_series, 3 row blocks")


def test_4b_row_blocks_of_runmicro_series_have_the_bits_of_one_block():
    a = SC.build("s170_h005")
    args = [a[k] for k in ARGS]
    zone = np.repeat(np.array([0, 1, 1, 0, 0]), SC.COLS).reshape(SC.ROWS, SC.COLS).astype(np.int32)     # blocks: rows 0 | 1-2 | 3-4
    zone[0, 3] = zone[4, 9] = -1
    cells = [0, 1 + 5 * 3, 2 + 5 * 9, 4 + 5 * 9, 3]
    sel = dict(points=cells, zones=zone, nzones=3, vars=ALL, stats=ZS)      # (zone 2 has no cell: count 0)
    one = api.runmicro_series(*args, **sel)
    for kw in (dict(devices=[0, 0], n_blocks=3), dict(devices=[0], n_blocks=5), dict(devices=[0, 0], n_blocks=2, chunk_days=1)):
        multi = api.runmicro_series(*args, **sel, **kw)
        for v in ALL:
            same(multi["points"][v], one["points"][v], (v, "points", kw))
            for s in ZS:
                same(multi["zones"][v][s], one["zones"][v][s], (v, s, kw))
    full = api.runmicro1Cpp(*args, [1] * 10)
    same_sink({v: {"points": one["points"][v], "zones": one["zones"][v]} for v in ALL}, full, ALL, cells, zone, 3, None, "one block")
    pts_only = api.runmicro_series(*args, points=[4 + 5 * 9], vars=("Tz",), devices=[0, 0], n_blocks=3)       # blocks without a point
    same(pts_only["points"]["Tz"], ZR.point_series(full["Tz"], [49]), "one point, three blocks")


# ---- 5. below ground ----------------------------------------------------------------------------------------------------------------
DEPTHS = (-0.05, -0.2, -1.0)


def depth_case(complete):
    from test_below_depths_gpu import tbp_rows
    a = dict(SC.build("s170_h005"), complete=bool(complete))
    b = {k: a[k] for k in ARGS if k != "reqhgt"}
    return a, dict(b, depths=list(DEPTHS), tbp=None if complete else tbp_rows(a, DEPTHS))


@pytest.mark.parametrize("complete", (0, 1))
def test_5_soil_depths(complete):
    a, dargs = depth_case(complete)
    full = api.runmicro_depths(**dargs)
    hgt = np.asarray(a["vegp"]["hgt"])
    na = int(np.flatnonzero(np.isnan(hgt).reshape(-1, order="F"))[0])
    cells = [na, 49, 48, 0, 17]
    zone = np.repeat(np.array([0, 0, 1, 1, 2]), SC.COLS).reshape(SC.ROWS, SC.COLS).astype(np.int32)
    zone[np.arange(50).reshape((5, 10), order="F") % 7 == 3] = -1
    zone[np.unravel_index(na, (5, 10), order="F")] = 3
    arrays = {f"Tz{d}": full["Tz"][d] for d in range(3)}
    arrays["soilm"] = full["soilm"]
    not_degenerate(arrays, list(arrays), zone, 4, cells, na)
    done = np.arange(96) < 96
    for chunk in (1, 2, 0):
        got = api.runmicro_depths_series(**dargs, points=cells, zones=zone, nzones=4, vars=("Tz", "soilm"), stats=ZS, chunk_days=chunk)
        res = {f"Tz{d}": got["Tz"][d] for d in range(3)}
        res["soilm"] = got["soilm"]
        same_sink(res, arrays, list(arrays), cells, zone, 4, done, f"depths, complete {complete}, chunk {chunk}")
    only = api.runmicro_depths_series(**dargs, zones=zone, nzones=4, vars=("soilm",), stats=("mean",))
    assert "Tz" not in only and only["soilm"]["points"] is None
    same(only["soilm"]["zones"]["mean"], ZR.zone_series(full["soilm"], zone, 4)["mean"], "soilm alone")
    # the plan's own entries
    plan_args = dict(a, reqhgt=DEPTHS[0], out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0])
    with Plan(**plan_args, ring_days=2, stream_below=True) as st:
        st.below_set_depths(DEPTHS, dargs["tbp"])
        st.below_prepare()
        with pytest.raises(McfError, match="error 1: mcf_plan_series_enable: .*streamed plan"):
            st.series_enable(cells, zone, ("Tz",))
        with pytest.raises(McfError, match="error 1: mcf_plan_series_enable_below: below ground Tz and soilm"):
            st.series_enable_below(cells, zone, ("Tz", "tleaf"))
        st.series_enable_below(cells, zone, ("Tz", "soilm"), ZS, nzones=4)
        with pytest.raises(McfError, match="error 5: mcf_plan_series_enable_below: .*already enabled"):
            st.series_enable_below(cells, zone, ("Tz",))
        for d0 in (0, 2):
            st.run_days(d0, 2, 0)
            st.series_accumulate(0, 0, d0, 2)
        for d in range(3):
            same(st.fetch_point_series_depth(d, "Tz"), ZR.point_series(full["Tz"][d], cells), ("plan", d, "points"))
            same(st.fetch_zone_series_depth(d, "Tz", "mean"), ZR.zone_series(full["Tz"][d], zone, 4)["mean"], ("plan", d, "mean"))
        same(st.fetch_zone_series_depth(0, "soilm", "max"), ZR.zone_series(full["soilm"], zone, 4)["max"], "plan, soilm")
        same(st.fetch_zone_series("Tz", "min"), ZR.zone_series(full["Tz"][0], zone, 4)["min"], "plan, fetch_zone_series is depth 0")
        for call in (lambda: st.fetch_zone_series_depth(3, "Tz", "mean"), lambda: st.fetch_point_series_depth(3, "Tz"),
                     lambda: st.fetch_zone_series_depth(1, "soilm", "mean"), lambda: st.fetch_point_series_depth(-1, "Tz")):
            with pytest.raises(McfError, match="error 1: mcf_plan_series_fetch_(points|zones)_depth: "):
                call()
    with Plan(**plan_args, ring_days=4) as whole:
        with pytest.raises(McfError, match="error 5: mcf_plan_series_enable_below needs a streamed plan"):
            whole.series_enable_below(cells, zone, ("Tz",))


def test_5b_front_end_on_the_bundled_site():
    from bundled import load
    depths = (-0.05, -0.2)
    weather, vegp, soilc, dtm = load(3 * 24)
    vegp = {k: (v[:, :, 6] if v.ndim == 3 else v) for k, v in vegp.items()}          # July's layer, time-invariant
    mp = frontend.runpointmodel(weather, 0.05, dtm, vegp, soilc)
    full = frontend.runmicro_depths(mp, depths, vegp, soilc, dtm)
    rows, cols = np.asarray(dtm["z"]).shape
    res = dtm["res"]
    dtm = dict(dtm, xmin=1000.0, ymax=5000.0)
    zones = (np.arange(rows * cols).reshape(rows, cols) // (4 * cols)) % 16           # bands of four rows
    got = frontend.runmicro_depths_series(mp, depths, vegp, soilc, dtm, points=[(3, 4)], xy=[(1000.0 + 2.5 * res, 5000.0 - 0.5 * res)],
                                          zones=zones, vars=("Tz", "soilm"), stats=ZS)
    assert got["cells"].tolist() == [3 + rows * 4, 0 + rows * 2]
    nz = int(zones.max()) + 1
    arrays = {"Tz0": full["Tz"][0], "Tz1": full["Tz"][1], "soilm": full["soilm"]}
    same_sink({"Tz0": got["Tz"][0], "Tz1": got["Tz"][1], "soilm": got["soilm"]}, arrays, list(arrays), got["cells"], zones, nz, None, "front end")
    assert np.isfinite(got["Tz"][1]["zones"]["mean"]).any()
    with pytest.raises(ValueError, match="Tz"):
        frontend.runmicro_depths_series(mp, depths, vegp, soilc, dtm, zones=zones, vars=("tleaf",))
