"""The slow snow method's chunk loop for array weather, in one run: the three routes from coarse arrays to the snow series
(tools/snowmodel2_coarse_rate.py > profiles/snowmodel2_coarse_rate.txt 2>&1)

  (a) snow.snowmodel2_chunks   the host loop: per chunk a numpy resample of thirteen arrays, one-shot gridmodelsnow2, terrain
                               and tpi calls, the redistribution in numpy
  (b) snow.snowmodel2_device   the device-resident loop fed fine arrays, INCLUDING the numpy expansion that makes them
                               (snow._fine_snow_inputs over the whole series): 13 x 8 B per cell-step over PCIe
  (c) snow.snowmodel2_coarse   the one call with the coarse arrays left coarse, all six series
  (d) (c) with series = ("totalSWE",)

at every size of `--sizes` (default the bundled 50 x 50 site and 512 x 512), and (c) and (d) alone at every size of `--big`
(default 1024): `--days` days (default 30) of the bundled weather made 12 degC colder over a 5 x 4 climate grid of perturbed
copies, altcorrect = 2.  The point model and `.sortl` are the same host code on every route and are not in the times; every
route takes host arrays in and hands host arrays back.  One process, one warm-up of (c), then ONE timed call of each route.
The ratios are against the routes that exist without the one call, measured in this same run.  The library's own MCF_TIMING
line (stderr) of one further call of (c) per size gives the chunk kernel's and k_snowmodel's device time per chunk and the
chunk kernel's write rate (13 x 8 B per cell-step).

    python tools/snowmodel2_coarse_rate.py [--sizes 50,512] [--big 1024] [--days 30] [--device 0]"""
import argparse
import os
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

CR, CC = 5, 4


def mirrored(a, n):
    """a [r, c, ...] raster continued to n x n by reflection (no cliffs at the seams)"""
    a = np.asarray(a)
    if a.ndim < 2:
        return a
    pad = ((0, n - a.shape[0]), (0, n - a.shape[1])) + ((0, 0),) * (a.ndim - 2)
    return np.pad(a, pad, mode="symmetric") if n > a.shape[0] else a[:n, :n]


def point_stage(days):
    """the coarse side, the same at every raster size: climate cells and the snow point model per cell"""
    T = 24 * days
    weather, vegp, soilc, dtm = load(T)
    rng = np.random.default_rng(5)
    clim_c = {}
    for k in F.WEATHER:
        if k == "winddir":
            continue
        base = np.broadcast_to(np.asarray(weather[k], dtype=np.float64)[None, None, :T], (CR, CC, T)).copy()
        if k == "temp":
            base += -12.0 + rng.uniform(-1.5, 1.5, (CR, CC, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (CR, CC, 1))
        clim_c[k] = np.asfortranarray(base)
    clim_c["difrad"] = np.minimum(clim_c["difrad"], clim_c["swdown"])
    clim_c["winddir"] = np.asarray(weather["winddir"], dtype=np.float64)[:T]
    ob = {k: np.asarray(weather["obstime"][k])[:T] for k in ("year", "month", "day", "hour")}
    vg = F.cleanvegp(vegp)
    vc = {k: F.block_reduce(vg[k], CR, CC) for k in ("pai", "hgt", "leaft", "clump")}
    lat_c = dtm["lat"] + 1e-4 * np.arange(CR)[:, None] + 0 * np.arange(CC)[None, :]
    lon_c = dtm["long"] + 1e-4 * np.arange(CC)[None, :] + 0 * np.arange(CR)[:, None]
    pointm_c = F.snow_pointm_cells(ob, clim_c, vc, lat_c, lon_c, 2.0, 0.0, 0.0, "Taiga", False)
    return vegp, dtm, ob, clim_c, pointm_c


def loop_arguments(n, stage):
    """what `frontend.runsnowmodela(method = "slow")` hands the chunk loop, for the site mirrored out to n x n"""
    vegp, dtm, ob, clim_c, pointm_c = stage
    vegp = F.cleanvegp({k: mirrored(v, n) for k, v in vegp.items()})
    z = mirrored(dtm["z"], n).astype(np.float64)
    vs = F.sortl(vegp, np.max(pointm_c["sdepc"], axis=(0, 1)))
    lats = dtm["lat"] + 9e-6 * np.arange(n)[::-1, None] + 0 * np.arange(n)[None, :]
    lons = dtm["long"] + 1.4e-5 * np.arange(n)[None, :] + 0 * np.arange(n)[:, None]
    other = {"zref": 2.0, "lats": lats, "lons": lons, "isnowdc": 0.0 * z, "isnowdg": 0.0 * z, "isnowac": 0.0 * z, "isnowag": 0.0 * z}
    res = dtm["res"] if np.isscalar(dtm["res"]) else dtm["res"][0]
    dtmc = np.full((CR, CC), float(np.nanmean(z))) + 10.0 * np.arange(CR * CC).reshape(CR, CC)
    args = (ob, clim_c, pointm_c, vs, other, "Taiga", z, dtmc, res, 0.01)
    return args, dict(rowpos=api.coarse_positions(n, CR), colpos=api.coarse_positions(n, CC), altcorrect=2)


def device_loop_from_host_expansion(args, kw, agg, device):
    """route (b): numpy brings the whole series to the raster, mcf_snowmodel2 uploads it chunk by chunk"""
    ob, clim_c, pointm_c, vs, other, snowenv, z, dtmc, res, tfact = args
    wd = np.asarray(clim_c["winddir"], dtype=np.float64) * np.pi / 180
    wu_c, wv_c = clim_c["windspeed"] * np.cos(wd), clim_c["windspeed"] * np.sin(wd)
    wuv, wvv = np.nanmean(wu_c, axis=(0, 1)), np.nanmean(wv_c, axis=(0, 1))
    winddir = (np.arctan2(wvv, wuv) * 180 / np.pi) % 360
    with np.errstate(invalid="ignore"):
        clim, pointm = S._fine_snow_inputs(clim_c, pointm_c, slice(0, len(winddir)), z, np.nan_to_num(dtmc, nan=0.0), kw["rowpos"],
                                           kw["colpos"], kw["altcorrect"], wu_c, wv_c, winddir)
    vg = dict(vs, leaft=np.where(np.isnan(vs["leaft"]), 0.001, vs["leaft"]))
    return S.snowmodel2_device(ob, clim, pointm, vg, other, snowenv, z, res, tfact, af_wind=np.sqrt(wuv ** 2 + wvv ** 2), wsa_s=agg,
                               device=device)


def once(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50,512")
    ap.add_argument("--big", default="1024")
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    os.environ.pop("MCF_TIMING", None)
    sizes = [int(s) for s in a.sizes.split(",") if s]
    big = [int(s) for s in a.big.split(",") if s]
    stage = point_stage(a.days)
    agg = 1                                                  # what runsnowmodela passes under a climate grid of fewer than ten cells a side
    for n in sizes + big:
        args, kw = loop_arguments(n, stage)
        T = 24 * a.days
        print(f"slow snow method, array weather over a {CR} x {CC} climate grid, {n} x {n} cells, {a.days} days ({T // 120} chunks of 120 h), "
              f"altcorrect = 2; seconds, host arrays in and out; fine inputs of the whole series {13 * 8 * n * n * T / 1e9:.2f} GB", flush=True)
        coarse = lambda **k: S.snowmodel2_coarse(*args, **kw, agg=agg, device=a.device, **k)       # noqa: E731
        coarse(series=("totalSWE",))                          # the warm-up
        t_a = t_b = None
        if n in sizes:
            t_a, ra = once(lambda: S.snowmodel2_chunks(*args, **kw, agg=agg, device=a.device))
            print(f"(a) host loop (snowmodel2_chunks), all six series            {t_a:9.3f} s", flush=True)
            t_b, rb = once(lambda: device_loop_from_host_expansion(args, kw, agg, a.device))
            print(f"(b) numpy expansion + mcf_snowmodel2, five series            {t_b:9.3f} s", flush=True)
        t_c, rc = once(coarse)
        line = f"(c) one call (mcf_snowmodel2_coarse), all six series         {t_c:9.3f} s"
        if t_a is not None:
            line += f"   (c)/(b) {t_c / t_b:6.3f}   (c)/(a) {t_c / t_a:6.3f}"
            worst = max(float(np.nanmax(np.abs(rc[k] - rb[k]) / (1 + np.abs(rb[k])), initial=0.0)) for k in rb)
            line += f"   largest scaled |(c) - (b)| {worst:.1e}"
            del ra, rb
        print(line, flush=True)
        print(f"    deepest ground snow {np.nanmax(rc['groundsnowdepth']):.3f} m", flush=True)
        del rc
        t_d, _ = once(lambda: coarse(series=("totalSWE",)))
        print(f"(d) one call, totalSWE only                                  {t_d:9.3f} s   (c)/(d) {t_c / t_d:5.2f}", flush=True)
        os.environ["MCF_TIMING"] = "1"                      # the library's per-stage line
        sys.stdout.flush()
        coarse(series=("totalSWE",))
        os.environ.pop("MCF_TIMING", None)
        sys.stderr.flush()


if __name__ == "__main__":
    main()
