"""The array-weather snow run as one device-resident call with every coarse array left coarse (include/mcf.h
mcf_runmicrosnow2_coarse, mcf_snowrun_create_coarse, mcf_microsnow_expand_coarse_device; `runmicro_snow_array(one_call=True)`):
the expansion kernel of the snow-day microclimate's weather alone against the host's `.prepsnowinputs2`
(snow._fine_micro_inputs), the run against the snow model's own one call (bytes), against its staged form (bytes), against
`.runmicrosnow2`'s orchestration on host arrays with HIP behind it (1e-12), the front end against the oracle-backed
orchestration, and what the call returns when asked for less, asked twice, or asked after a refusal."""
import functools

import numpy as np
import pytest

from microclimf_amd import _abi, api
from microclimf_amd import frontend as F
from microclimf_amd import snow as S
import parity_bars
import snowrun2_coarse_cases as CS
from test_snowrun2_coarse_cpu import micro_fields
from test_snowrun_gpu import _close, _steps

pytestmark = pytest.mark.gpu

SHAPES = [(7, 9), (23, 37), (1, 50)]      # 23 x 37 = 851 cells: several workgroups, the last one partial; 1 x 50: less than a wave
GRIDS = [(1, 1), (1, 2), (3, 1), (2, 3), (5, 4)]     # single coarse rows / columns: r1 / c1 fall back onto r0 / c0
NINE = _abi.MICRO_FINE_SERIES
MASKED = ("swdown", "difrad", "lwdown", "precip", "umu")      # `.cca`; temp, pres and the wind are resampled unmasked


# ---- the expansion kernel alone ---------------------------------------------------------------------------------------
def _host(wc, umu_c, z, dtmc, rowpos, colpos, altcorrect, sl):
    return S._fine_micro_inputs(wc, umu_c, sl, z, np.nan_to_num(dtmc, nan=0.0) if altcorrect else None, rowpos, colpos, altcorrect)


@pytest.mark.parametrize("nsteps", [1, 24, 25, 120])
@pytest.mark.parametrize("altcorrect", [0, 1, 2])
def test_the_expansion_is_the_hosts_prepsnowinputs2(nsteps, altcorrect):
    """altcorrect = 0: taps, the mask and the wind speed's sqrt are IEEE operations in the host's order: bytes.  relhum always, and
    temp / pres with altcorrect 1 / 2: the device's pow and exp differ from numpy's by ulps, which ea / es and elevd x lapse rate
    carry to about 1e-15: 1e-12 (test_snowmodel2_coarse_gpu.py's bar for the same cause).  The first hour of the window has
    relhum = 8 in every coarse cell, the second 100 % over coarse temperatures 15 degC apart: both clamps bind."""
    T, step0 = 160, 17                                       # the window starts inside a day and, at 120 steps, ends inside one
    for n, (shape, grid) in enumerate(zip(SHAPES + SHAPES[:2], GRIDS)):
        wc, umu_c, z, dtmc, rowpos, colpos = micro_fields(shape, grid, T, 500 + n, h20=step0, h100=step0 + 1)
        sl = slice(step0, step0 + nsteps)
        want = _host(wc, umu_c, z, dtmc, rowpos, colpos, altcorrect, sl)
        got = S.expand_micro_coarse(wc, umu_c, z, dtmc, rowpos=rowpos, colpos=colpos, altcorrect=altcorrect, step0=step0, nsteps=nsteps)
        assert list(got) == [*NINE, "winddir"]
        assert got["winddir"].tobytes() == np.ascontiguousarray(want["winddir"]).tobytes()
        hole = np.isnan(z)
        assert hole.sum() == 1
        # the clamps bind on the yardstick, exactly, and hold on the result
        assert (want["relhum"][:, :, 0] == 20.0).any(), (shape, grid)
        if nsteps > 1:
            assert (want["relhum"][:, :, 1] == 100.0).any(), (shape, grid)
        assert np.nanmin(got["relhum"]) >= 20.0 and np.nanmax(got["relhum"]) <= 100.0
        for k in NINE:
            g, w = got[k], want[k]
            assert g.shape == shape + (nsteps,), k
            assert np.array_equal(np.isnan(g), np.isnan(w)), (shape, grid, k)
            if k in MASKED:
                assert np.all(g[hole].view(np.uint64) == parity_bars.NA_BITS), k
            exact = k in MASKED or k == "windspeed" or (altcorrect == 0 and k in ("temp", "pres"))
            if exact:
                assert np.ascontiguousarray(g[~hole]).tobytes() == np.ascontiguousarray(w[~hole]).tobytes(), (shape, grid, k)
                if k not in MASKED:                          # unmasked: bytes everywhere
                    assert g.tobytes() == np.asfortranarray(w).tobytes(), (shape, grid, k)
            else:
                with np.errstate(invalid="ignore"):
                    d = float(np.nanmax(np.abs(g - w) / (1 + np.abs(w)), initial=0.0))
                assert d <= 1e-12, (shape, grid, k, d)


@pytest.mark.parametrize("altcorrect", [0, 2])
def test_the_series_mask_writes_what_is_asked_for(altcorrect):
    """the micro set-up's scan asks for temp and precip alone: the same bits, the other buffers untouched"""
    shape, grid, T = (23, 37), (2, 3), 72
    wc, umu_c, z, dtmc, rowpos, colpos = micro_fields(shape, grid, T, 77)
    kw = dict(rowpos=rowpos, colpos=colpos, altcorrect=altcorrect, step0=5, nsteps=49)
    full = S.expand_micro_coarse(wc, umu_c, z, dtmc, **kw)
    mark = -12345.678
    out = {k: np.full(shape + (49,), mark, order="F") for k in NINE}
    two = S.expand_micro_coarse(wc, umu_c, z, dtmc, series=("temp", "precip"), out=out, **kw)
    assert list(two) == [*NINE, "winddir"]
    for k in NINE:
        if k in ("temp", "precip"):
            assert two[k] is out[k] and out[k].tobytes() == full[k].tobytes(), k
        else:
            assert np.all(out[k] == mark), k
    one = S.expand_micro_coarse(wc, umu_c, z, dtmc, series=("relhum",), **kw)
    assert list(one) == ["relhum", "winddir"] and one["relhum"].tobytes() == full["relhum"].tobytes()


# ---- the run ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _snow_model(altcorrect):
    """the snow model's own one call on the case (the code this run is built on) and the day classes of its totalSWE"""
    args, pos, kw = CS.snow_args(CS.snow_inputs(altcorrect))
    smod = S.snowmodel2_coarse(*args, **pos, **kw)
    for v in smod.values():
        v.flags.writeable = False
    return smod


def _groups(altcorrect, reqhgt, out=(1,) * 10):
    clima, obst, mpa, vegp, soilc, dtm, kw = CS.product(altcorrect)
    return F.snow_array_groups(mpa, 2, 3, reqhgt, vegp, soilc, dtm, CS.snow_inputs(altcorrect), dtmc=kw["dtmc"], lats=kw["lats"],
                               lons=kw["lons"], altcorrect=altcorrect, out=out)


def _sub3(d, idx):
    """day-subset of a dict of vectors [T] and arrays [., ., T]"""
    return {k: (np.asarray(v)[idx] if np.ndim(v) == 1 else np.asfortranarray(np.asarray(v)[:, :, idx])) for k, v in d.items()}


def _host_orchestration(sn, mi, mat, smod, sdays, ndays_, reqhgt, altcorrect):
    """`.runmicrosnow2` on host arrays with HIP behind it: the coarse-array solver on the no-snow-day subset of the coarse arrays
    (the micropoints' day subset through `runmicro_array`, as `.runmicronosnow` hands it over: the bundled vegetation has monthly
    layers, so this is runmicro4Cpp's coarse form), gridmicrosnow2 on the snow-day subset of the expansion kernel's output, merged
    by day"""
    clima, obst, mpa, vegp, soilc, dtm, kw = CS.product(altcorrect)
    z = sn["dtm"]
    rows, cols = z.shape
    ni, si = _steps(ndays_), _steps(sdays)
    moutn = F.runmicro_array([F.subsetpointmodel(m, days=ndays_ + 1) for m in mpa], 2, 3, reqhgt, vegp, soilc, dtm, lats=kw["lats"],
                             lons=kw["lons"], tfact=1.5, altcorrect=altcorrect, dtmc=kw["dtmc"])
    micro = {}
    s1 = np.arange(si.size)[np.repeat(np.isin(sdays, ndays_), 24)]
    s2 = np.arange(ni.size)[np.repeat(np.isin(ndays_, sdays), 24)]
    for k, v in moutn.items():
        m = np.full((rows, cols, si.size), np.nan, order="F")
        m[:, :, s1] = v[:, :, s2]
        micro[k] = m
    swe = smod["totalSWE"].copy()
    swe[np.isnan(swe)] = 0.0
    swe[np.isnan(z)] = np.nan
    smods = {k: np.asfortranarray((swe if k == "totalSWE" else smod[k])[:, :, si]) for k in _abi.SNOWDRIVER_OUT}
    w = S.expand_micro_coarse(mi["clim_c"], mi["umu_c"], z, sn["dtmc"], rowpos=sn["rowpos"], colpos=sn["colpos"], altcorrect=altcorrect)
    outm = [1] * 10 if reqhgt > 0 else [1 if i in (0, 3, 5, 6, 7, 8, 9) else 0 for i in range(10)]
    mouts = S.gridmicrosnow2(reqhgt, _sub3(mi["obstime"], si), _sub3(w, si), smods, micro, mi["vegp"], mi["other"], mat, outm)
    for k in moutn:
        if k not in mouts:
            mouts[k] = micro[k]
    return S.merge_snow_outputs(moutn, mouts, sdays + 1, ndays_ + 1, rows, cols)


@pytest.mark.parametrize("reqhgt", [0.05, 0.0])
@pytest.mark.parametrize("altcorrect", [0, 1, 2])
def test_the_one_call_is_the_snow_model_the_staged_run_and_the_host_orchestration(oracle, altcorrect, reqhgt):
    ref = _snow_model(altcorrect)
    si = CS.snow_inputs(altcorrect)
    z = si["dtm"]
    hole = np.isnan(z)
    assert z.shape == (23, 37) and hole.any() and si["clim_c"]["temp"].shape == (2, 3, CS.T11)
    CS.check_classes(ref["totalSWE"], hole)                   # the case's conditions, on the snow model's own one call
    g, sn, mi, mat = _groups(altcorrect, reqhgt)
    got, smod = S.runmicrosnow2_coarse(g, sn, mi, mat, want_smod=True)
    # (a) the snow series are mcf_snowmodel2_coarse's
    assert list(smod) == list(ref)
    for k in ref:
        assert smod[k].tobytes() == ref[k].tobytes(), k
    # (b) the staged form on the coarse handle, and its day flags
    with S.SnowRun(g, sn, micro_coarse=mi) as run:
        sd, nd = run.pass1()
        got2 = run.pass2(mi, mat)
        st = run.stats()
    assert list(got2) == list(got)
    for k in got:
        assert got[k].tobytes() == got2[k].tobytes(), k
    swe = smod["totalSWE"].copy()
    swe[np.isnan(swe)] = 0.0
    swe[hole] = np.nan
    days = S.snowdaysfun(S.applycpp3(swe, "max"), S.applycpp3(swe, "min"))
    assert np.array_equal(sd, days["snowdays"]) and np.array_equal(nd, days["nosnowdays"])
    want_sd, want_nd = CS.day_classes(smod["totalSWE"], hole)
    assert np.array_equal(sd, want_sd) and np.array_equal(nd, want_nd)
    # (d) array weather solves the no-snow days whole
    assert st["tile_days_left_out"] == 0 and st["chunks_rerun"] >= 1
    # (c) the host orchestration with HIP behind it
    sdays, ndays_ = np.flatnonzero(sd), np.flatnonzero(nd)
    want = _host_orchestration(sn, mi, mat, smod, sdays, ndays_, reqhgt, altcorrect)
    for k in want:
        fin = np.isfinite(want[k])
        with np.errstate(invalid="ignore"):
            d = float(np.max(np.abs(got[k][fin] - want[k][fin]) / (1 + np.abs(want[k][fin])))) if fin.any() else 0.0
        print(f"altcorrect {altcorrect} reqhgt {reqhgt} {k:10s} largest scaled |one call - host orchestration| = {d:.3e}")
    _close(got, want, 1e-12, "host-orchestrated HIP")
    assert np.isnan(got["Tz"][hole]).all() and np.isfinite(got["Tz"][~hole][:, _steps(ndays_)]).all()


# ---- the front end ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _site():
    """test_snowfast_gpu.py::test_runmicro_with_snow_and_array_weather's inputs: the bundled 50 x 50 site under a 2 x 2 climate
    grid, fifteen days with a cold spell and a thaw"""
    from bundled import load
    weather, vegp, soilc, dtm = load(15 * 24)
    cr, cc, T = 2, 2, 15 * 24
    t = np.arange(T)
    rng = np.random.default_rng(3)
    climarray = {}
    for k in F.WEATHER:
        base = np.broadcast_to(weather[k][None, None, :], (cr, cc, T)).copy()
        if k == "temp":
            base += -9.0 + 8.0 * (t > 5 * 24) + 7.0 * (t > 10 * 24) + rng.uniform(-1.0, 1.0, (cr, cc, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (cr, cc, 1))
        climarray[k] = np.asfortranarray(base)
    climarray["difrad"] = np.minimum(climarray["difrad"], climarray["swdown"])
    clat = dtm["lat"] + 1e-4 * np.arange(cr)[:, None] + 0 * np.arange(cc)[None, :]
    clon = dtm["long"] + 1e-4 * np.arange(cc)[None, :] + 0 * np.arange(cr)[:, None]
    lats = dtm["lat"] + 9e-6 * np.arange(50)[::-1, None] + 0 * np.arange(50)[None, :]
    lons = dtm["long"] + 1.4e-5 * np.arange(50)[None, :] + 0 * np.arange(50)[:, None]
    z = np.asarray(dtm["z"])
    dtmc = np.array([[np.nanmean(z[:25, :25]), np.nanmean(z[:25, 25:])], [np.nanmean(z[25:, :25]), np.nanmean(z[25:, 25:])]]) + 30.0
    mpa = F.runpointmodela(climarray, weather["obstime"], 0.05, dtm, vegp, soilc, lats=clat, lons=clon)
    return weather, vegp, soilc, dtm, climarray, clat, clon, lats, lons, dtmc, mpa


@pytest.mark.parametrize("altcorrect", [0, 2])
def test_front_end_one_call_matches_the_oracle_backed_orchestration(oracle, altcorrect):
    """`runmicro_snow_array(one_call=True)` against the same orchestration with the oracle's solver, snow microclimate and terrain
    behind it, fed the one call's snow series; and against the default route.  The bar is
    test_snowfast_gpu.py::test_runmicro_with_snow_and_array_weather's for this comparison: identical NaN masks and 1e-6 scaled
    (parity_bars.CAP)."""
    from functools import partial
    from oracle import coarse_oracle as CO
    from oracle import terrain_oracle as TO
    weather, vegp, soilc, dtm, climarray, clat, clon, lats, lons, dtmc, mpa = _site()
    cr, cc, T, reqhgt = 2, 2, 15 * 24, 0.05
    si = F.runsnowmodela(climarray, weather["obstime"], mpa, vegp, soilc, dtm, dtmc=dtmc, lats_c=clat, lons_c=clon, lats=lats, lons=lons,
                         altcorrect=altcorrect, method="slow", inputs_only=True)
    kw = dict(dtmc=dtmc, lats=lats, lons=lons, altcorrect=altcorrect)
    got, smod = F.runmicro_snow_array(mpa, cr, cc, reqhgt, vegp, soilc, dtm, one_call=True, snow_inputs=si, want_smod=True, **kw)
    sd = S.snowdaysfun(S.applycpp3(np.nan_to_num(smod["totalSWE"]), "max"), S.applycpp3(np.nan_to_num(smod["totalSWE"]), "min"))
    assert sd["snowdays"].sum() > 0 and sd["nosnowdays"].sum() > 0

    def solve_oracle(mpx, reqhgt, **kw2):
        tf = kw2.pop("tfact", 1.5)
        zz = F.cleanvars(vegp, soilc, dtm["z"])[2]
        ter = TO.terrain(zz, dtm["res"], mpx[0]["zref"])
        a = F.prepare_grid_inputs_array(mpx, cr, cc, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons, slr=ter["slope"],
                                        apr=ter["aspect"], hor=ter["hor"], svf=ter["svfa"], wsa=ter["wsa"], **kw2)
        a["tfact"] = tf
        clim, pm = CO.expand(a["climdata"], a["pointm"], api.coarse_positions(50, cr), api.coarse_positions(50, cc),
                             altcorrect=altcorrect, dtmc=dtmc, dtm=zz)
        a.update(climdata=clim, pointm=pm)
        return oracle.run_grid(**a, array_forcing=True)

    want = F.runmicro_snow_array(mpa, cr, cc, reqhgt, vegp, soilc, dtm, smod, _solve=solve_oracle,
                                 _microsnow=partial(oracle.run_microsnow, array_forcing=True), _terrain=TO.terrain, **kw)
    default = F.runmicro_snow_array(mpa, cr, cc, reqhgt, vegp, soilc, dtm, smod, **kw)
    assert list(got) == list(want) == list(default)
    dist = {}
    for what, ref in (("oracle-backed", want), ("default route", default)):
        for k in ref:
            assert got[k].shape == (50, 50, T)
            dist[what, k] = parity_bars.distance(got[k], ref[k])
            print(f"altcorrect {altcorrect} {k:10s} largest scaled |one call - {what}| = {dist[what, k]:.3e}")
        with np.errstate(invalid="ignore"):
            e = np.abs(got["Tz"] - ref["Tz"]) / (1 + np.abs(ref["Tz"]))
        print(what, "Tz per day:", " ".join(f"{np.nanmax(e[:, :, 24 * d:24 * d + 24], initial=0.0):.1e}" for d in range(T // 24)),
              "snow", sd["snowdays"], "nosnow", sd["nosnowdays"])
    for (what, k), d in dist.items():
        ref = want if what == "oracle-backed" else default
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (what, k)
        assert d < parity_bars.CAP, (what, k, d)


# ---- the solver's side of the day subset: the temperature cap and the layers ---------------------------------------------
@pytest.mark.parametrize("altcorrect", [0, 1, 2])
def test_the_day_flagged_cap_is_the_cap_of_a_plan_on_the_subset_series(altcorrect):
    """`mcf_plan_set_mxtc_days` on a coarse plan against the create-time cap of a coarse plan made on the host-subset coarse
    arrays: the same per-step expression and an order-free maximum — bytes.  The unflagged days are the warm ones, so a kernel
    that folded every day gives another cap in every cell."""
    from microclimf_amd import synthetic
    from microclimf_amd.api import Plan
    rows, cols, nd = 23, 37, 9
    a, rp, cp = synthetic.coarse_workload(rows, cols, nd * 24, 2, 3, variety=True, start_doy=40)
    flags = np.array([1, 1, 0, 1, 0, 0, 1, 1, 0], dtype=np.int32)
    steps = np.repeat(flags.astype(bool), 24)
    clim = dict(a["climdata"])
    clim["temp"] = np.asfortranarray(clim["temp"] + 12.0 * (~steps)[None, None, :])
    a = dict(a, climdata=clim)
    coarse = {"rowpos": rp, "colpos": cp}
    if altcorrect:
        z = np.random.default_rng(5).uniform(40.0, 240.0, (rows, cols))
        coarse.update(altcorrect=altcorrect, dtmc=np.array([[100.0, 150.0, np.nan], [120.0, 90.0, 200.0]]), dtm=z)
    sub = dict(a, obstime=_sub3(a["obstime"], steps), climdata=_sub3(clim, steps), pointm=_sub3(a["pointm"], steps))
    with Plan(**a, ring_days=1, ring_slots=1, coarse=coarse) as p, Plan(**sub, ring_days=1, ring_slots=1, coarse=coarse) as q:
        whole = p.fetch_mxtc()
        p.set_mxtc_days(flags)
        got, want = p.fetch_mxtc(), q.fetch_mxtc()
        assert got.tobytes() == want.tobytes()
        assert np.all(whole > got + 1.0)                      # the warm days are left out, in every cell
        p.set_mxtc_days(np.ones(nd, dtype=np.int32))          # every day flagged: the create-time cap, started from -273.15
        assert p.fetch_mxtc().tobytes() == whole.tobytes()
        p.set_mxtc_days(np.zeros(nd, dtype=np.int32))
        assert np.all(p.fetch_mxtc() == -273.15)


@pytest.mark.parametrize("days", [(1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), (2, 3, 4, 5, 8, 9, 15), (1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)])
def test_a_whole_series_plan_solves_a_day_subset_as_the_subset_solver_does(oracle, days):
    """The bundled site's twelve vegetation layers over fifteen days.  A coarse plan of the WHOLE series with the day -> layer map
    of `frontend.subset_day_layers` and the cap over the subset's days, each day run at its own place, against `runmicro_array`
    on the micropoints' day subset (what `.runmicronosnow` hands `.runmodel4Cpp`) — subsets that cut a layer out of the arrays
    entirely (days 4 and 5 missing), that keep a few steps of a layer that is no day's mode, and with gaps of several days: the
    same kernels on the same inputs, bytes."""
    from microclimf_amd.api import Plan
    weather, vegp, soilc, dtm, climarray, clat, clon, lats, lons, dtmc, mpa = _site()
    cr, cc, alt, reqhgt = 2, 2, 2, 0.05
    days = np.array(days)
    want = F.runmicro_array([F.subsetpointmodel(m, days=days) for m in mpa], cr, cc, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons,
                            tfact=1.5, altcorrect=alt, dtmc=dtmc)
    a = F.prepare_grid_inputs_array(mpa, cr, cc, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons)
    a["tfact"] = 1.5
    z = F.cleanvars(vegp, soilc, dtm["z"])[2]
    coarse = {"rowpos": api.coarse_positions(50, cr), "colpos": api.coarse_positions(50, cc), "altcorrect": alt, "dtmc": dtmc, "dtm": z}
    lod = F.subset_day_layers(mpa[0], vegp, soilc, dtm, days)
    flags = np.zeros(15, dtype=np.int32)
    flags[days - 1] = 1
    with Plan(**a, ring_days=1, ring_slots=1, coarse=coarse) as p:
        p.set_mxtc_days(flags)
        own = {}
        for with_map in (False, True):
            if with_map:
                p.set_day_layers(lod)
            worst = 0.0
            for i, d in enumerate(days):
                p.run_days_at(int(d) - 1, 1, 0, 0)
                p.sync()
                for k in want:
                    g, w = p.fetch(0, k, 0, 24), want[k][:, :, 24 * i:24 * i + 24]
                    if with_map:
                        assert g.tobytes() == np.asfortranarray(w).tobytes(), (int(d), k)
                    else:
                        worst = max(worst, parity_bars.distance(g, w))
            own[with_map] = worst
        # the whole-series table alone is another answer where the two dealings part and the layers differ: with day 5 alone
        # missing every later day runs one layer early (1e-2 in Tz)
        print(f"days {days.tolist()}: largest scaled |whole-series table - subset solver| = {own[False]:.3e}")
        if days.size == 14:
            assert own[False] > 1e-6, own
        p.set_day_layers(None)                                # the plan's own table again
        p.run_days_at(0, 1, 0, 0)
        p.sync()


# ---- outputs and state --------------------------------------------------------------------------------------------------
def test_repeats_less_output_and_a_call_after_a_refusal(oracle):
    altcorrect, reqhgt = 1, 0.05
    g, sn, mi, mat = _groups(altcorrect, reqhgt)
    full, smod = S.runmicrosnow2_coarse(g, sn, mi, mat, want_smod=True)
    assert list(full) == list(_abi.OUT_NAMES) and list(smod) == list(_abi.SNOWFAST2_OUT)
    again = S.runmicrosnow2_coarse(g, sn, mi, mat)            # want_smod False: the outputs alone, the same bytes
    assert isinstance(again, dict) and list(again) == list(full)
    for k in full:
        assert again[k].tobytes() == full[k].tobytes(), k
    bad = dict(sn, colpos=np.array(sn["colpos"]) + 5.0)       # positions outside the climate grid
    with pytest.raises(_abi.McfError, match="mcf_runmicrosnow2_coarse: .*coarse_rowpos / coarse_colpos"):
        S.runmicrosnow2_coarse(g, bad, mi, mat)
    with pytest.raises(_abi.McfError, match="mcf_runmicrosnow2_coarse: .*chunk_steps"):
        S.runmicrosnow2_coarse(g, dict(sn, chunk_steps=100), mi, mat)
    with pytest.raises(_abi.McfError, match="mcf_snowrun_create_coarse: .*differ in altcorrect"):
        S.SnowRun(g, dict(sn, altcorrect=2), micro_coarse=mi)
    with S.SnowRun(g, sn, micro_coarse=mi) as run:            # the day -> layer map: between the passes only
        lod = np.zeros(run.days, dtype=np.int32)
        with pytest.raises(_abi.McfError, match="between mcf_snowrun_pass1"):
            run.set_day_layers(lod)
        run.pass1()
        run.set_day_layers(lod)                               # (every day on the first of the twelve layers)
        moved = run.pass2(mi, mat)
        with pytest.raises(_abi.McfError, match="between mcf_snowrun_pass1"):
            run.set_day_layers(lod)
        run.pass1()                                           # a second period: the plans' own table again
        again2 = run.pass2(mi, mat)
    assert any(moved[k].tobytes() != full[k].tobytes() for k in full)      # (the map was in force)
    for k in full:
        assert again2[k].tobytes() == full[k].tobytes(), k
    g1, sn1, mi1, mat1 = _groups(altcorrect, reqhgt, out=(1,) + (0,) * 9)      # `out[]`: Tz alone
    only = S.runmicrosnow2_coarse(g1, sn1, mi1, mat1)
    assert list(only) == ["Tz"] and only["Tz"].tobytes() == full["Tz"].tobytes()
    after, smod2 = S.runmicrosnow2_coarse(g, sn, mi, mat, want_smod=True)
    for k in full:
        assert after[k].tobytes() == full[k].tobytes(), k
    for k in smod:
        assert smod2[k].tobytes() == smod[k].tobytes(), k
