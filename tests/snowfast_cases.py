"""Inputs and oracle runs of the fast snow method's one-call tests (test_snowfast_onecall_gpu.py, test_snowfast2_onecall_gpu.py,
test_snowfast_bars_cpu.py): the cases of `mcf_snowmodelq1` (Q1_CASES, data.frame weather) and `mcf_snowmodelq2` (Q2_CASES, array
weather on a coarse climate grid), each a window of the bundled raster, a few selected days of a 50-day series and a snow
environment.

A case is ADMISSIBLE for the derived bars of parity_bars.py when every noise variant of the oracle keeps the oracle's NaN / inf
pattern (parity_bars.bars_for refuses anything else) and no bar reaches parity_bars.CAP.  test_snowfast_bars_cpu.py checks this
for all fourteen cases (on the CPU: it needs the oracle only); a case that fails is replaced by a neighbouring seed or window
chosen from the oracle's output alone, no cell, step or variable is ever excluded.

The oracle's terrain is numpy: no variant models its rounding, while 1e-10 on the terrain (what test_terrain_gpu.py allows the
device) moves `Tg` by 4e-9, thousands of floor-level bars.  `run(O, c, terrain=...)` therefore takes the terrain the snow chain
is to work on; the GPU tests hand it the device's own, after holding that to terrain_oracle ("Tolerance").
"""
import functools

import numpy as np

from bundled import load
from microclimf_amd import api
from microclimf_amd import frontend as F
from microclimf_amd.rformulas import upsample_coarse

# the cases whose window is at most 23 x 37 = 851 cells (<= 96 selected hours): the ones the GPU tests hold to derived bars
SMALL = (0, 2, 3, 4, 5, 6)

# ---- mcf_snowmodelq1 --------------------------------------------------------------------------------------------------
Q1_CASES = [
    dict(days=[2, 3, 49], window=(0, 23, 0, 37)),           # gaps of 24 h, of 2 h counting down, of 1 080 h
    dict(days=[4, 11, 12, 30, 47], window=(0, 50, 0, 50)),
    dict(days=[10, 40], window=(12, 13, 0, 50), snowenv="Prairie", cold=-14.0),          # one row: `.tpicalc`'s raster mean
    dict(days=[3, 20, 44], window=(5, 28, 10, 47), snowenv="Alpine", snowinitd=0.002, snowinita=30.0, stfact=0.03, hole=True),
    dict(days=[6, 7, 8, 35], window=(20, 50, 0, 19), snowenv="Tundra", zref=3.0, windhgt=2.0),
    dict(days=[5, 20], window=(10, 30, 5, 30), cold=5.0, bare=True),                     # no snowfall at all: msnow is NaN
    dict(days=[5, 6, 20], window=(10, 30, 5, 30), cold=-30.0),                           # every gap frozen: mu = 1
]


def _crop(vegp, soilc, dtm, r0, r1, c0, c1):
    cut = lambda a: np.array(np.asarray(a)[r0:r1, c0:c1])                # noqa: E731
    return {k: cut(v) for k, v in vegp.items()}, {k: cut(v) for k, v in soilc.items()}, dict(dtm, z=cut(dtm["z"]))


@functools.lru_cache(maxsize=None)
def q1_case(i, days=None):
    """the product's inputs of Q1_CASES[i], the day loop's arguments as the oracle chain forms them (built as
    tests/test_snowfast_gpu.py::test_fast_method_matches_the_oracle_chain builds `want`), and the oracle's result.
    days (a tuple): the case with other selected days, for the day loop's arguments alone — the oracle chain is not run"""
    from oracle import oracle as O
    from oracle import replay_reference_tests as RT
    from oracle import snowfast_oracle as SF
    O.load()
    case = Q1_CASES[i] if days is None else dict(Q1_CASES[i], days=list(days))
    weather, vegp, soilc, dtm = load(50 * 24)
    vegp, soilc, dtm = _crop(vegp, soilc, dtm, *case["window"])
    if case.get("hole"):
        dtm["z"][5:8, 6:9] = np.nan
    weather = dict(weather, temp=weather["temp"] + case.get("cold", -9.0))
    env, sd0, sa0 = case.get("snowenv", "Taiga"), case.get("snowinitd", 0.0), case.get("snowinita", 0.0)
    zref, windhgt, stfact = case.get("zref", 2.0), case.get("windhgt", case.get("zref", 2.0)), case.get("stfact", 0.01)
    mp = F.subsetpointmodel(F.runpointmodel(weather, 0.05, dtm, vegp, soilc), days=case["days"])
    kw = dict(snowenv=env, snowinitd=sd0, snowinita=sa0, zref=zref, windhgt=windhgt, stfact=stfact)
    z = np.asarray(dtm["z"])
    vg = F.cleanvegp(vegp)
    vp = F.sortvegp_point(vg)
    obst = {k: np.asarray(v) for k, v in weather["obstime"].items()}
    w = {k: np.array(weather[k], dtype=np.float64) for k in F.WEATHER}
    if zref != windhgt:
        w["windspeed"] = w["windspeed"] * np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    assert np.nanmax(vg["hgt"]) <= zref
    sdep, sage = z * 0 + sd0, z * 0 + sa0
    pm = RT.pointmodelsnow(obst, w, np.array([vp[1], vp[0], vp[5], vp[3]]),
                           np.array([0, 0, mp["lat"], mp["long"], zref, np.nanmean(sdep), np.nanmean(sage)]), env, maxiter=20)
    T = len(w["temp"])
    ai = np.asarray(mp["subs"]) - 1
    pointm = {"Gp": pm["G"], "Tc": pm["Tc"], "RswabsG": pm["RswabsG"], "RlwabsG": pm["RlwabsG"], "umu": pm["umu"], "tr": pm["tr"]}
    vs = F.sortl(vg, pm["sdepc"][:T])
    vs["leaft"] = np.where(np.isnan(vs["leaft"]), 0.01, vs["leaft"])
    other = {"zref": zref, "lat": mp["lat"], "lon": mp["long"], "isnowdc": sd0 * z, "isnowac": sage, "isnowag": sage}
    rows = lambda d: {k: np.asarray(v)[ai] for k, v in d.items()}      # noqa: E731
    args = (rows(obst), rows(w), rows(pointm), pm, w["temp"], np.where(w["temp"] > 2, 0.0, w["precip"]), mp["subs"], vs, other, env, z,
            dtm["res"], stfact)
    want = SF.snowmodelq1_days(*args) if days is None else {}
    for v in want.values():
        v.flags.writeable = False
    return dict(kind="q1", product=(weather, mp, vegp, soilc, dtm, kw), args=args, want=want, umu=pm["umu"][ai])


# ---- mcf_snowmodelq2 --------------------------------------------------------------------------------------------------
Q2_CASES = [
    dict(days=[2, 3, 49], window=(0, 23, 0, 37), grid=(2, 3), altcorrect=0),       # gaps of 24 h, of 2 h counting down, of 1 080 h
    dict(days=[4, 6, 7, 12], window=(0, 50, 0, 50), grid=(2, 3), altcorrect=2),
    dict(days=[10, 40], window=(12, 13, 0, 50), grid=(1, 2), altcorrect=1, snowenv="Prairie", cold=-14.0),   # one row: `.tpicalc`'s raster mean
    dict(days=[3, 20, 44], window=(5, 28, 10, 47), grid=(3, 1), altcorrect=2, snowenv="Alpine", snowinitd=0.002, snowinita=30.0,
         stfact=0.03, hole=True),
    dict(days=[1, 2, 8, 35], window=(20, 50, 0, 19), grid=(2, 3), altcorrect=0, snowenv="Tundra", zref=3.0, windhgt=2.0),   # the series' first day
    dict(days=[5, 20], window=(10, 30, 5, 30), grid=(1, 2), altcorrect=0, cold=5.0, bare=True),          # no snowfall at all: msnow is NaN
    dict(days=[5, 6, 20], window=(10, 30, 5, 30), grid=(2, 3), altcorrect=1, cold=-30.0),                # every gap frozen: mu = 0.5
]


@functools.lru_cache(maxsize=None)
def q2_case(i, days=None):
    """the product's inputs of Q2_CASES[i], the day loop's arguments as the oracle chain forms them (built as the `fast` case of
    tests/test_snowfast_gpu.py::test_array_weather_snow_model_matches_the_oracle_chain builds `want`), and the oracle's result.
    days (a tuple): the case with other selected days, for the day loop's arguments alone — the oracle chain is not run"""
    from oracle import oracle as O
    from oracle import replay_reference_tests as RT
    from oracle import snowfast_oracle as SF
    O.load()
    case, run_oracle = (Q2_CASES[i], True) if days is None else (dict(Q2_CASES[i], days=list(days)), False)
    weather, vegp, soilc, dtm = load(50 * 24)
    vegp, soilc, dtm = _crop(vegp, soilc, dtm, *case["window"])
    if case.get("hole"):
        dtm["z"][5:8, 6:9] = np.nan
    (cr, cc), T = case["grid"], 50 * 24
    z = np.asarray(dtm["z"])
    R, Cc = z.shape
    rng = np.random.default_rng(9 + i)
    climarray = {}
    for k in F.WEATHER:
        base = np.broadcast_to(weather[k][None, None, :], (cr, cc, T)).copy()
        if k == "temp":
            base += case.get("cold", -9.0) + rng.uniform(-1.5, 1.5, (cr, cc, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (cr, cc, 1))
        elif k == "winddir":
            base = (base + rng.integers(-1, 2, (cr, cc, T)) * 10.0) % 360
        climarray[k] = np.asfortranarray(base)
    climarray["difrad"] = np.minimum(climarray["difrad"], climarray["swdown"])
    clat = dtm["lat"] + 1e-4 * np.arange(cr)[:, None] + 0 * np.arange(cc)[None, :]
    clon = dtm["long"] + 1e-4 * np.arange(cc)[None, :] + 0 * np.arange(cr)[:, None]
    lats = dtm["lat"] + 9e-6 * np.arange(R)[::-1, None] + 0 * np.arange(Cc)[None, :]
    lons = dtm["long"] + 1.4e-5 * np.arange(Cc)[None, :] + 0 * np.arange(R)[:, None]
    dtmc = np.nanmean(z) + 40.0 + 5.0 * np.arange(cr * cc).reshape(cr, cc)
    env, sd0, sa0 = case.get("snowenv", "Taiga"), case.get("snowinitd", 0.0), case.get("snowinita", 0.0)
    zref, windhgt, stfact = case.get("zref", 2.0), case.get("windhgt", case.get("zref", 2.0)), case.get("stfact", 0.01)
    days = np.asarray(case["days"])
    subs = (np.repeat((days - 1) * 24, 24) + np.tile(np.arange(24), days.size) + 1).astype(np.int64)
    mpa = [{"subs": subs, "ntme": T, "zref": zref}] * (cr * cc)         # what runsnowmodela reads of subsetpointmodel's output
    kw = dict(dtmc=dtmc, lats_c=clat, lons_c=clon, lats=lats, lons=lons, altcorrect=case["altcorrect"], snowenv=env, snowinitd=sd0,
              snowinita=sa0, zref=zref, windhgt=windhgt, stfact=stfact)
    # the same through the oracle
    vg = F.cleanvegp(vegp)
    assert np.nanmax(vg["hgt"]) <= zref
    obst = {k: np.asarray(v) for k, v in weather["obstime"].items()}
    wdir = np.array([F.getmode(climarray["winddir"][:, :, k]) for k in range(T)])
    vc = {k: F.block_reduce(vg[k], cr, cc) for k in ("pai", "hgt", "leaft", "clump")}
    clim_c = {k: np.array(climarray[k], copy=True) for k in F.WEATHER if k != "winddir"}
    if zref != windhgt:
        clim_c["windspeed"] *= np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    clim_c["winddir"] = wdir
    names = {"Gp": "G", "Tc": "Tc", "RswabsG": "RswabsG", "RlwabsG": "RlwabsG", "umu": "umu", "tr": "tr", "sdepc": "sdepc"}
    names.update({k: k for k in ("sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc", "sdeng")})
    pointm_c = {k: np.empty((cr, cc, T)) for k in names}
    for a in range(cr):
        for b in range(cc):
            w = {k: np.ascontiguousarray(clim_c[k][a, b, :]) for k in clim_c if k != "winddir"}
            pm = RT.pointmodelsnow(obst, w, np.array([np.mean(vc[k][a, b, :]) for k in ("pai", "hgt", "leaft", "clump")]),
                                   np.array([0, 0, clat[a, b], clon[a, b], zref, sd0, sa0]), env, maxiter=10)
            for k, v in names.items():
                pointm_c[k][a, b, :] = pm[v][1:T + 1] if k == "sdepc" else pm[v][:T]
    other = {"zref": zref, "lats": lats, "lons": lons, "isnowdc": z * 0 + sd0, "isnowac": z * 0 + sa0, "isnowag": z * 0 + sa0}
    ai = subs - 1
    sel = lambda d: {k: (np.asarray(v)[ai] if np.ndim(v) == 1 else np.asfortranarray(np.asarray(v)[:, :, ai])) for k, v in d.items()}   # noqa: E731
    pm2 = {k: pointm_c[k] for k in ("sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc", "sdeng")}
    pm2["tc"] = clim_c["temp"]
    pm2["snow"] = np.where(clim_c["temp"] > 2, 0.0, clim_c["precip"])
    pm_s = sel({k: pointm_c[k] for k in ("Gp", "Tc", "RswabsG", "RlwabsG", "umu", "tr", "sdepc")})
    rowpos, colpos = api.coarse_positions(R, cr), api.coarse_positions(Cc, cc)
    args = (sel(obst), sel(clim_c), pm_s, pm2, subs, F.sortl(vg, np.max(pm_s["sdepc"], axis=(0, 1))), other, env, z, dtmc, dtm["res"],
            stfact)
    pos = dict(rowpos=rowpos, colpos=colpos, altcorrect=case["altcorrect"])
    want = SF.snowmodelq2_days(*args, rowpos, colpos, altcorrect=case["altcorrect"]) if run_oracle else {}
    for v in want.values():
        v.flags.writeable = False
    # the gaps' multipliers on the reference side: does a gap thaw somewhere (mu neither 0.5 nor NA)?
    hole = np.isnan(z)[:, :, None]
    cca = lambda a: np.where(hole, np.nan, upsample_coarse(a, rowpos, colpos))               # noqa: E731
    thaws = False
    for d in range(days.size):
        if subs[24 * d] - 1 > 1:
            sbtn = SF._colon((subs[24 * d - 1] if d else 0) + 1, int(subs[24 * d]) - 1)
            st = cca(pm2["sstemp"][:, :, sbtn])
            thaws = thaws or bool(np.any(np.nansum(np.where(st > 0, st, 0.0), axis=2) > 0))
    return dict(kind="q2", product=(climarray, weather["obstime"], mpa, vegp, soilc, dtm, kw), args=args, pos=pos, want=want, thaws=thaws,
                umu_c=pm_s["umu"], hole=np.isnan(z))


# ---- the day loop's branches that no case above takes ------------------------------------------------------------------
# One selected day: one output set, one `done` event, only the trailing download.  Ten selected days whose aggregation factors
# round(10 sqrt(mean wind) / res) are AF_DAYS: nine distinct ones against the eight position indices a call keeps, so the ninth
# is computed over the oldest slot (af = 2's) and the tenth day needs af = 2 again.  Both on case 0's window (23 x 37: every
# factor is below min(dim) / 2 = 11.5, `.tpicalc` aggregates, and a wrong slot is another position index).
ONE_DAY = (3,)
TEN_DAYS = (2, 3, 7, 11, 16, 22, 29, 37, 44, 49)
AF_DAYS = [2, 3, 4, 5, 6, 7, 8, 9, 10, 2]


def loop_args(kind, days):
    """-> (S.snowmodelq1's / S.snowmodelq2's arguments, the keywords) of case 0 with `days` selected; with TEN_DAYS every
    selected hour's wind speed is the day's (AF_DAYS res / 10)^2 (q2: in every coarse cell, the directions as they are)"""
    c = q1_case(0, days) if kind == "q1" else q2_case(0, days)
    args = list(c["args"])
    if days == TEN_DAYS:
        res = args[11] if kind == "q1" else args[10]
        wind = np.repeat((np.asarray(AF_DAYS) * res / 10) ** 2, 24)
        args[1] = dict(args[1], windspeed=wind if kind == "q1" else np.asfortranarray(np.broadcast_to(wind, args[1]["windspeed"].shape)))
    return tuple(args), c.get("pos", {})


def library_af(wind, res):
    """the aggregation factor per day as the library forms it (day_af): the day's 24 values added left to right, / 24, sqrt,
    x 10, / res, rounded half to even"""
    out = []
    for day in np.asarray(wind, dtype=np.float64).reshape(-1, 24):
        s = 0.0
        for v in day:
            s += float(v)
        out.append(int(np.rint(10 * np.sqrt(s / 24) / res)))
    return out


# ---- the oracle chain as a workload of parity_bars --------------------------------------------------------------------
def run(O, c, terrain=None):
    """run(lib) -> {variable: array} for parity_bars.bars_for / slips_for: the oracle chain of case `c` (q1_case / q2_case)
    with gridmodelsnow1 / 2 from the build `lib`, on `terrain` (a dict slope, aspect, hor, skyview, wsa; None: terrain_oracle's)"""
    from oracle import snowfast_oracle as SF
    if c["kind"] == "q1":
        return lambda lib: SF.snowmodelq1_days(*c["args"], lib=lib, terrain=terrain)
    pos = c["pos"]
    return lambda lib: SF.snowmodelq2_days(*c["args"], pos["rowpos"], pos["colpos"], altcorrect=pos["altcorrect"], lib=lib, terrain=terrain)


def oracle_terrain(c):
    """terrain_oracle's terrain of a case, as the chain forms it: what snow_terrain must give on the device"""
    from oracle import terrain_oracle as TO
    kind = c["kind"]
    z, res, zref = (c["args"][10], c["args"][11], c["args"][8]["zref"]) if kind == "q1" else (c["args"][8], c["args"][10], c["args"][6]["zref"])
    hole = np.isnan(z)
    slope, aspect = TO.slope_aspect(z, res, aspect_na=180.0)
    hor = TO.horizons24(z, res)
    return z, res, float(zref), {"slope": np.where(hole, np.nan, slope), "aspect": np.where(hole, np.nan, aspect), "hor": hor,
                                 "skyview": TO.skyview(hor), "wsa": TO.windsheltera(z, float(zref), 10 if res <= 100 else 1, res)}
