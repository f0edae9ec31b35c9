"""The fast snow method's day loop for array weather, in one run: the host loop over the selected days
(snow.snowmodelq2_days) and the one device-resident call (snow.snowmodelq2) at the bundled 50 x 50 site, then the call alone
at `--size` x `--size` cells (tools/snowfast2_rate.py > profiles/snowfast2_rate.txt 2>&1).

The reference's vignette workflow with array weather: a 3 x 3 climate grid of perturbed copies of the bundled weather made
12 degC colder, the snow point model per climate cell over the whole year, each month's coldest day selected (twelve days),
`.snowmodelq2` behind it.  The point model and `.sortl` are the same host code on both routes and are not in the times; both
routes take host arrays in and hand host arrays back, so uploads and downloads are.  One warm-up of the device route, then
the median of `--runs` calls; the host loop is timed `--loop-runs` times without a warm-up.  At `--size` the host loop is not
run: between two selected days it builds cca(sstemp) and cca(tc) as [rows, cols, gap hours] host arrays (the size is printed).
The per-stage device times are the library's own MCF_TIMING line (stderr) of one further call per size.

    python tools/snowfast2_rate.py [--size 1024] [--runs 3] [--loop-runs 1] [--device 0]"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bundled import load  # noqa: E402
from microclimf_amd import api  # noqa: E402
from microclimf_amd import frontend as F  # noqa: E402
from microclimf_amd import snow as S  # noqa: E402

CR = CC = 3


def mirrored(a, n):
    """a [r, c, ...] raster continued to n x n by reflection (no cliffs at the seams)"""
    a = np.asarray(a)
    if a.ndim < 2:
        return a
    pad = ((0, n - a.shape[0]), (0, n - a.shape[1])) + ((0, 0),) * (a.ndim - 2)
    return np.pad(a, pad, mode="symmetric") if n > a.shape[0] else a[:n, :n]


def point_stage():
    """the coarse side, the same at every raster size: climate cells, the snow point model per cell, the selected hours"""
    weather, vegp, soilc, dtm = load()
    weather = dict(weather, temp=weather["temp"] - 12.0)
    mp = F.subsetpointmodel(F.runpointmodel(weather, 0.05, dtm, vegp, soilc), tstep="month", what="tmin")
    T = len(weather["temp"])
    rng = np.random.default_rng(5)
    clim_c = {}
    for k in F.WEATHER:
        if k == "winddir":
            continue
        base = np.broadcast_to(np.asarray(weather[k], dtype=np.float64)[None, None, :], (CR, CC, T)).copy()
        if k == "temp":
            base += rng.uniform(-1.5, 1.5, (CR, CC, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (CR, CC, 1))
        clim_c[k] = np.asfortranarray(base)
    clim_c["difrad"] = np.minimum(clim_c["difrad"], clim_c["swdown"])
    clim_c["winddir"] = np.asarray(weather["winddir"], dtype=np.float64)
    ob = {k: np.asarray(weather["obstime"][k]) for k in ("year", "month", "day", "hour")}
    vg = F.cleanvegp(vegp)
    vc = {k: F.block_reduce(vg[k], CR, CC) for k in ("pai", "hgt", "leaft", "clump")}
    lat_c = dtm["lat"] + 1e-4 * np.arange(CR)[:, None] + 0 * np.arange(CC)[None, :]
    lon_c = dtm["long"] + 1e-4 * np.arange(CC)[None, :] + 0 * np.arange(CR)[:, None]
    pointm_c = F.snow_pointm_cells(ob, clim_c, vc, lat_c, lon_c, 2.0, 0.0, 0.0, "Taiga", True)
    return weather, vegp, dtm, ob, clim_c, pointm_c, np.asarray(mp["subs"], dtype=np.int64)


def day_loop_arguments(n, stage):
    """what `frontend.runsnowmodela(method = "fast")` hands the day loop, for the site mirrored out to n x n"""
    weather, vegp, dtm, ob, clim_c, pointm_c, subs = stage
    vegp = F.cleanvegp({k: mirrored(v, n) for k, v in vegp.items()})
    z = mirrored(dtm["z"], n).astype(np.float64)
    ai = subs - 1
    sel = lambda d: {k: (np.asarray(v)[ai] if np.ndim(v) == 1 else np.asfortranarray(np.asarray(v)[:, :, ai])) for k, v in d.items()}   # noqa: E731
    pm2_c = {k: pointm_c[k] for k in ("sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc", "sdeng")}
    pm2_c["tc"] = clim_c["temp"]
    pm2_c["snow"] = np.where(clim_c["temp"] > 2, 0.0, clim_c["precip"])
    pm_s = sel({k: pointm_c[k] for k in ("Gp", "Tc", "RswabsG", "RlwabsG", "umu", "tr", "sdepc")})
    vs = F.sortl(vegp, np.max(pm_s["sdepc"], axis=(0, 1)))
    lats = dtm["lat"] + 9e-6 * np.arange(n)[::-1, None] + 0 * np.arange(n)[None, :]
    lons = dtm["long"] + 1.4e-5 * np.arange(n)[None, :] + 0 * np.arange(n)[:, None]
    other = {"zref": 2.0, "lats": lats, "lons": lons, "isnowdc": 0.0 * z, "isnowac": 0.0 * z, "isnowag": 0.0 * z}
    res = dtm["res"] if np.isscalar(dtm["res"]) else dtm["res"][0]
    dtmc = np.full((CR, CC), float(np.nanmean(z))) + 10.0 * np.arange(CR * CC).reshape(CR, CC)
    args = (sel(ob), sel(clim_c), pm_s, pm2_c, subs, vs, other, "Taiga", z, dtmc, res, 0.01)
    return args, dict(rowpos=api.coarse_positions(n, CR), colpos=api.coarse_positions(n, CC), altcorrect=2)


def timed(fn, runs, warm=True):
    if warm:
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--loop-runs", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    os.environ.pop("MCF_TIMING", None)
    stage = point_stage()
    subs = stage[-1]
    days = len(subs) // 24
    gaps = np.diff(np.r_[0, subs[23::24]]) - 24
    for n in (50, a.size):
        args, kw = day_loop_arguments(n, stage)
        print(f"fast snow method, array weather over a {CR} x {CC} climate grid, {n} x {n} cells, {days} selected days of "
              f"{stage[4]['temp'].shape[2]} hours (gaps {gaps.min()} .. {gaps.max()} h), altcorrect = 2; seconds, host arrays in and out",
              flush=True)
        t_loop = None
        if n == 50:
            t_loop = timed(lambda: S.snowmodelq2_days(*args, device=a.device, **kw), a.loop_runs, warm=False)
            print(f"host day loop (snowmodelq2_days), all six series    {t_loop:9.3f} s   ({a.loop_runs} run, no warm-up)", flush=True)
        else:
            print(f"host day loop: not run — its longest gap needs two [rows, cols, gap] host arrays of "
                  f"{n * n * int(gaps.max()) * 8 / 1e9:.1f} GB each for the single-threaded host meltmu2", flush=True)
        t_all = timed(lambda: S.snowmodelq2(*args, device=a.device, **kw), a.runs)
        ratio = f"   day loop / one call {t_loop / t_all:7.1f}" if t_loop else ""
        print(f"one call (mcf_snowmodelq2), all six series          {t_all:9.3f} s{ratio}", flush=True)
        t_swe = timed(lambda: S.snowmodelq2(*args, device=a.device, series=("totalSWE",), **kw), a.runs)
        print(f"one call, totalSWE only                             {t_swe:9.3f} s   all six / totalSWE only {t_all / t_swe:5.1f}", flush=True)
        os.environ["MCF_TIMING"] = "1"                      # the library's per-stage line
        sys.stdout.flush()
        S.snowmodelq2(*args, device=a.device, **kw)
        os.environ.pop("MCF_TIMING", None)
        sys.stderr.flush()


if __name__ == "__main__":
    main()
