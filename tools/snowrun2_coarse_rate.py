#!/usr/bin/env python3
"""What leaving the coarse arrays coarse saves the array-weather snow run: one process, one device.

    python tools/snowrun2_coarse_rate.py [--sizes bundled,512,1024] [--days 30] [--repeats 3] [--out profiles/snowrun2_coarse_rate.txt]

Routes, a host clock around each (every route ends in a device synchronise: its outputs are host arrays):
  (a) the host orchestration: `runsnowmodela(method="slow")`'s host chunk loop + `runmicro_snow_array`'s default route;
  (b) `mcf_runmicrosnow2` (snow.runmicrosnow2) fed fine arrays made on the host — the solver's fifteen (oracle/coarse_oracle.py),
      the snow model's thirteen (snow._fine_snow_inputs) and the microclimate's nine (snow._fine_micro_inputs); the call timed alone,
      the expansion timed once; skipped where the 37 arrays do not fit in host memory;
  (c) the one call `runmicro_snow_array(one_call=True)` with all ten outputs and with Tz alone.
Sizes: the bundled 50 x 50 site under a 2 x 2 climate grid (15 days), and the site tiled to N x N under a 5 x 4 grid (altcorrect 2).
Reported: medians with their spread (min .. max), the ratios c/a and c/b, the expansion kernel's time per chunk and its written
bytes/s (MCF_TIMING's line: 9 x 8 B x cells x snow steps), the peak device memory during the one call (sampled).
Order per size: (c), (b), then (a), whose time is host numpy and runs to many minutes at 512 x 512: --a-repeats limits its runs, and
--out is rewritten as the routes end, so a run that is cut short leaves what it measured and how long (a) had been running.
A size or a route that was not run is written as "not measured"."""
import argparse
import os
import statistics
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from microclimf_amd import frontend as F, snow as S      # noqa: E402


def site(n, days, grid, altcorrect):
    """the bundled site tiled to n x n (n = 0: as it is), `days` days, a cold spell and a thaw over a `grid` climate grid"""
    from bundled import load
    weather, vegp, soilc, dtm = load(days * 24)
    if n:
        reps = -(-n // 50)
        tile = lambda a: np.ascontiguousarray(np.tile(np.asarray(a), (reps, reps) + (1,) * (np.ndim(a) - 2))[:n, :n])      # noqa: E731
        vegp = {k: tile(v) for k, v in vegp.items()}
        soilc = {k: tile(v) for k, v in soilc.items()}
        dtm = dict(dtm, z=tile(dtm["z"]))
    R, Cc = np.shape(dtm["z"])
    (cr, cc), T = grid, days * 24
    t = np.arange(T)
    rng = np.random.default_rng(3)
    clima = {}
    for k in F.WEATHER:
        base = np.broadcast_to(np.asarray(weather[k])[None, None, :], (cr, cc, T)).copy()
        if k == "temp":
            base += -9.0 + 8.0 * (t > T // 3) + 7.0 * (t > 2 * T // 3) + rng.uniform(-1.0, 1.0, (cr, cc, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (cr, cc, 1))
        clima[k] = np.asfortranarray(base)
    clima["difrad"] = np.minimum(clima["difrad"], clima["swdown"])
    clat = dtm["lat"] + 1e-4 * np.arange(cr)[:, None] + 0 * np.arange(cc)[None, :]
    clon = dtm["long"] + 1e-4 * np.arange(cc)[None, :] + 0 * np.arange(cr)[:, None]
    lats = dtm["lat"] + 9e-6 * np.arange(R)[::-1, None] + 0 * np.arange(Cc)[None, :]
    lons = dtm["long"] + 1.4e-5 * np.arange(Cc)[None, :] + 0 * np.arange(R)[:, None]
    dtmc = F.block_reduce(np.nan_to_num(np.asarray(dtm["z"], dtype=np.float64), nan=float(np.nanmean(dtm["z"]))), cr, cc)[:, :, 0] + 30.0
    mpa = F.runpointmodela(clima, weather["obstime"], 0.05, dtm, vegp, soilc, lats=clat, lons=clon)
    kw = dict(dtmc=dtmc, lats_c=clat, lons_c=clon, lats=lats, lons=lons, altcorrect=altcorrect, method="slow")
    return weather, vegp, soilc, dtm, clima, mpa, kw


def fine_groups(g, sn, mi, mat):
    """route (b)'s inputs: every coarse array of the three groups on the raster, made on the host"""
    from oracle import coarse_oracle as CO
    z, alt = sn["dtm"], sn["altcorrect"]
    zc = np.nan_to_num(sn["dtmc"], nan=0.0)
    clim, pm = CO.expand(g["climdata"], g["pointm"], sn["rowpos"], sn["colpos"], altcorrect=alt, dtmc=sn["dtmc"], dtm=z)
    a = {k: v for k, v in g.items() if k != "coarse"}
    a.update(climdata=clim, pointm=pm, lats=g["lat"], lons=g["lon"])
    cc = sn["clim_c"]
    wd = np.asarray(cc["winddir"]) * np.pi / 180
    wu, wv = cc["windspeed"] * np.cos(wd), cc["windspeed"] * np.sin(wd)
    wuv, wvv = np.nanmean(wu, axis=(0, 1)), np.nanmean(wv, axis=(0, 1))
    winddir = (np.arctan2(wvv, wuv) * 180 / np.pi) % 360
    with np.errstate(invalid="ignore"):
        sclim, spm = S._fine_snow_inputs(cc, sn["pointm_c"], slice(None), z, zc, sn["rowpos"], sn["colpos"], alt, wu, wv, winddir)
        w = S._fine_micro_inputs(mi["clim_c"], mi["umu_c"], slice(None), z, zc if alt else None, sn["rowpos"], sn["colpos"], alt)
    vg = dict(sn["vegp"], leaft=np.where(np.isnan(sn["vegp"]["leaft"]), 0.001, sn["vegp"]["leaft"]))
    snow = dict(obstime=sn["obstime"], climdata=sclim, pointm=spm, vegp=vg, other=sn["other"], snowenv=sn["snowenv"], dtm=z, res=sn["res"],
                tfact=sn["tfact"], af_wind=np.sqrt(wuv ** 2 + wvv ** 2), wsa_s=sn["agg"])
    micro = {"obstime": mi["obstime"], "climdata": w, "vegp": mi["vegp"], "other": mi["other"]}
    return a, snow, micro, mat


def med(v):
    return f"{statistics.median(v):8.3f} s ({min(v):.3f} .. {max(v):.3f})" if v else "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="bundled,512,1024")
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--a-repeats", type=int, default=None, help="timed runs of route (a), the host orchestration (default: --repeats)")
    ap.add_argument("--host-gb", type=float, default=64.0, help="route (b) is skipped where its 37 fine arrays need more than this")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "snowrun2_coarse_rate.txt"))
    args = ap.parse_args()
    import torch
    lines = [f"tools/snowrun2_coarse_rate.py --sizes {args.sizes} --days {args.days} --repeats {args.repeats}"
             + (f" --a-repeats {args.a_repeats}" if args.a_repeats is not None else ""),
             "one process; per size (c), then (b), then (a), a warm-up call before (b)'s and (c)'s timed ones; host clock, every route returns host arrays", ""]
    wanted = args.sizes.split(",")
    for size in ("bundled", "512", "1024"):
        if size not in wanted:
            lines += [f"== {size}: not measured", ""]
            continue
        n, days, grid, alt = (0, 15, (2, 2), 2) if size == "bundled" else (int(size), args.days, (5, 4), 2)
        weather, vegp, soilc, dtm, clima, mpa, kw = site(n, days, grid, alt)
        R, Cc = np.shape(dtm["z"])
        cr, cc = grid
        T = days * 24
        run_kw = dict(dtmc=kw["dtmc"], lats=kw["lats"], lons=kw["lons"], altcorrect=alt)
        si = F.runsnowmodela(clima, weather["obstime"], mpa, vegp, soilc, dtm, inputs_only=True, **kw)
        fits = 37 * R * Cc * T * 8 / 2 ** 30 <= args.host_gb
        ta, tb, tbx, tc, tc1 = [], [], [], [], []
        head = f"== {size}: {R} x {Cc} cells under a {cr} x {cc} climate grid, {days} days, altcorrect {alt}"
        state = {"a": None, "a_since": None, "peak": None, "timing": None}

        def report(final=False):
            """this size's lines from what has been measured so far (rewritten into --out as the routes end)"""
            if ta:
                la = med(ta) + (f" ({len(ta)} run)" if len(ta) < args.repeats else "")
            elif state["a_since"] is not None:
                la = f"not finished: still running after {time.perf_counter() - state['a_since']:.0f} s"
            else:
                la = "not measured"
            out = [head, f"(a) host snow model loop + default route        {la}",
                   f"(b) mcf_runmicrosnow2 on host-made fine arrays  {med(tb)}   their host expansion, once: "
                   + (f"{tbx[0]:.3f} s" if tbx else "not measured"),
                   f"(c) one call, ten outputs                       {med(tc)}",
                   f"(c) one call, Tz alone                          {med(tc1)}"]
            if tc:
                mc = statistics.median(tc)
                ra = (f"c / a = {mc / statistics.median(ta):.4f}" if ta else
                      f"c / a < {mc / (time.perf_counter() - state['a_since']):.4f}" if state["a_since"] is not None else "c / a not measured")
                out.append(ra + (f", c / b = {mc / statistics.median(tb):.3f}" if tb else ", c / b not measured"))
            out.append("expansion kernel: " + (state["timing"] or "not measured"))
            out.append("peak device memory during the one call (the device's used bytes sampled every 2 ms, this process's pools included): "
                       + (f"{state['peak'] / 2 ** 30:.2f} GiB" if state["peak"] else "not measured"))
            Path(args.out).write_text("\n".join(lines + out + [""]) + "\n")
            return out

        def one_call(**kw2):
            return F.runmicro_snow_array(mpa, cr, cc, 0.05, vegp, soilc, dtm, one_call=True, snow_inputs=si, **run_kw, **kw2)

        # (c) first: a warm-up, then the timed repeats, the device's used bytes sampled beside the last one
        one_call()
        for rep in range(args.repeats):
            stop, low = threading.Event(), [None]
            if rep == args.repeats - 1:
                def sample():
                    while not stop.is_set():
                        free, total = torch.cuda.mem_get_info()
                        low[0] = free if low[0] is None else min(low[0], free)
                        time.sleep(0.002)
                th = threading.Thread(target=sample)
                th.start()
            t0 = time.perf_counter()
            one_call()
            tc.append(time.perf_counter() - t0)
            if rep == args.repeats - 1:
                stop.set()
                th.join()
                state["peak"] = torch.cuda.mem_get_info()[1] - low[0]
            t0 = time.perf_counter()
            one_call(out=(1,) + (0,) * 9)
            tc1.append(time.perf_counter() - t0)
            print(f"{size} repeat {rep}: (c) {tc[-1]:.3f} s, Tz alone {tc1[-1]:.3f} s", flush=True)
        # the expansion kernel's own time: the library's MCF_TIMING line of one more one call (device events around each launch)
        os.environ["MCF_TIMING"] = "1"
        rfd, wfd = os.pipe()
        saved = os.dup(2)
        os.dup2(wfd, 2)
        try:
            g, sn, mi, mat = F.snow_array_groups(mpa, cr, cc, 0.05, vegp, soilc, dtm, si, **run_kw)
            S.runmicrosnow2_coarse(g, sn, mi, mat)
        finally:
            os.dup2(saved, 2)
            os.close(wfd)
            os.environ.pop("MCF_TIMING")
        timing = [ln for ln in os.read(rfd, 1 << 16).decode(errors="replace").splitlines() if "microsnow coarse expansion" in ln]
        state["timing"] = timing[0].split("] ", 1)[-1] if timing else None
        report()
        # (b): the 37 fine arrays made once on the host (timed once), the call a warm-up and the timed repeats
        if fits:
            t0 = time.perf_counter()
            fg = fine_groups(g, sn, mi, mat)
            tbx.append(time.perf_counter() - t0)
            print(f"{size}: (b)'s host expansion {tbx[0]:.3f} s", flush=True)
            S.runmicrosnow2(*fg)
            for rep in range(args.repeats):
                t0 = time.perf_counter()
                S.runmicrosnow2(*fg)
                tb.append(time.perf_counter() - t0)
                print(f"{size} repeat {rep}: (b) {tb[-1]:.3f} s", flush=True)
            del fg
            report()
        # (a) last, --a-repeats times (default: as the others) without a warm-up of its own: its time is the host's; while it runs a
        # line a minute says so, and --out says how long it has been running
        stop = threading.Event()

        def beat():
            while not stop.wait(60.0):
                print(f"{size}: (a) running, {time.perf_counter() - state['a_since']:.0f} s", flush=True)
                report()
        for rep in range(args.repeats if args.a_repeats is None else args.a_repeats):
            state["a_since"] = time.perf_counter()
            stop.clear()
            th = threading.Thread(target=beat, daemon=True)
            th.start()
            smod = F.runsnowmodela(clima, weather["obstime"], mpa, vegp, soilc, dtm, **kw)
            F.runmicro_snow_array(mpa, cr, cc, 0.05, vegp, soilc, dtm, smod, **run_kw)
            ta.append(time.perf_counter() - state["a_since"])
            stop.set()
            th.join()
            print(f"{size} repeat {rep}: (a) {ta[-1]:.3f} s", flush=True)
        lines += report() + [""]
        print("\n".join(lines[-9:]), flush=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
