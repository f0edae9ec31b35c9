"""The fast snow method's day loop three ways, in one run: the host loop over the selected days (snow.snowmodelq1_days), the
one device-resident call with all five series, and the same call asked for totalSWE only
(tools/snowfast_rate.py > profiles/snowfast_rate.txt 2>&1).

The reference's vignette workflow at size: the bundled site mirrored out to `--size` x `--size` cells, a year of its weather
made 12 degC colder, the point model subset to each month's coldest day (twelve selected days), `.snowmodelq1` behind it.
The point model and `.sortl` are the same host code on all three routes and are not in the times; every route takes host
arrays in and hands host arrays back, so uploads and downloads are.  One warm-up of each device route, then the median of
`--runs` calls; the host loop is timed `--loop-runs` times without a warm-up.  The per-stage device times are the library's
own MCF_TIMING line (stderr) of one further call per device route.

    python tools/snowfast_rate.py [--size 1024] [--runs 3] [--loop-runs 1] [--device 0]"""
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
from microclimf_amd import frontend as F  # noqa: E402
from microclimf_amd import pointmodel  # noqa: E402
from microclimf_amd import snow as S  # noqa: E402


def mirrored(a, n):
    """a [r, c, ...] raster continued to n x n by reflection (no cliffs at the seams)"""
    a = np.asarray(a)
    if a.ndim < 2:
        return a
    pad = ((0, n - a.shape[0]), (0, n - a.shape[1])) + ((0, 0),) * (a.ndim - 2)
    return np.pad(a, pad, mode="symmetric") if n > a.shape[0] else a[:n, :n]


def day_loop_arguments(n):
    """what `frontend.runsnowmodel(method = "fast")` hands the day loop, for the mirrored site"""
    weather, vegp, soilc, dtm = load()
    weather = dict(weather, temp=weather["temp"] - 12.0)
    mp = F.subsetpointmodel(F.runpointmodel(weather, 0.05, dtm, vegp, soilc), tstep="month", what="tmin")
    vegp = F.cleanvegp({k: mirrored(v, n) for k, v in vegp.items()})
    z = mirrored(dtm["z"], n).astype(np.float64)
    w = {k: np.array(weather[k], dtype=np.float64) for k in F.WEATHER}
    tme = weather["obstime"]
    hour_int = {k: np.asarray(tme[k]) for k in ("year", "month", "day")}
    hour_int["hour"] = np.floor(np.asarray(tme["hour"], dtype=np.float64))
    lat, long, zref = float(mp["lat"]), float(mp["long"]), 2.0
    vp = F.sortvegp_point(vegp)
    pmod = pointmodel.pointmodelsnow(hour_int, w, np.array([vp[1], vp[0], vp[5], vp[3]]), [0.0, 0.0, lat, long, zref, 0.0, 0.0], "Taiga",
                                     maxiter=20)
    T = len(w["temp"])
    pointm = {"Gp": pmod["G"], "Tc": pmod["Tc"], "RswabsG": pmod["RswabsG"], "RlwabsG": pmod["RlwabsG"], "umu": pmod["umu"], "tr": pmod["tr"]}
    vg = F.sortl(vegp, pmod["sdepc"][:T])
    vg["leaft"] = np.where(np.isnan(vg["leaft"]), 0.01, vg["leaft"])
    subs = np.asarray(mp["subs"], dtype=np.int64)
    ai = subs - 1
    rows = lambda d: {k: np.asarray(v)[ai] for k, v in d.items()}      # noqa: E731
    clim = {k: w[k] for k in ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "winddir", "precip")}
    other = {"zref": zref, "lat": lat, "lon": long, "isnowdc": 0.0 * z, "isnowac": 0.0 * z, "isnowag": 0.0 * z}
    res = dtm["res"] if np.isscalar(dtm["res"]) else dtm["res"][0]
    return (rows(hour_int), rows(clim), rows(pointm), pmod, w["temp"], np.where(w["temp"] > 2, 0.0, w["precip"]), subs, vg, other, "Taiga", z,
            res, 0.01)


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
    args = day_loop_arguments(a.size)
    days = len(args[6]) // 24
    gaps = np.diff(np.r_[0, np.asarray(args[6])[23::24]]) - 24
    print(f"fast snow method, {a.size} x {a.size} cells, {days} selected days of {len(args[4])} hours (gaps {gaps.min()} .. {gaps.max()} h); "
          "seconds, host arrays in and out", flush=True)
    t_loop = timed(lambda: S.snowmodelq1_days(*args, device=a.device), a.loop_runs, warm=False)
    print(f"host day loop (snowmodelq1_days), all five series   {t_loop:9.3f} s   ({a.loop_runs} run, no warm-up)", flush=True)
    t_all = timed(lambda: S.snowmodelq1(*args, device=a.device), a.runs)
    print(f"one call (mcf_snowmodelq1), all five series         {t_all:9.3f} s   day loop / one call {t_loop / t_all:7.1f}", flush=True)
    t_swe = timed(lambda: S.snowmodelq1(*args, device=a.device, series=("totalSWE",)), a.runs)
    print(f"one call, totalSWE only                             {t_swe:9.3f} s   day loop / one call {t_loop / t_swe:7.1f}   "
          f"all five / totalSWE only {t_all / t_swe:5.1f}", flush=True)
    gb = 5 * 24 * days * a.size * a.size * 8 / 1e9
    print(f"all five series are {gb:.2f} GB of results: {gb / t_all:.1f} GB/s of them per second of the whole call", flush=True)
    os.environ["MCF_TIMING"] = "1"                          # the library's per-stage line, one call per route
    sys.stdout.flush()
    S.snowmodelq1(*args, device=a.device)
    S.snowmodelq1(*args, device=a.device, series=("totalSWE",))


if __name__ == "__main__":
    main()
