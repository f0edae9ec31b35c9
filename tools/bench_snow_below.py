"""Times the below-ground snow run (include/mcf.h mcf_runmicrosnow1_below) on one device, reqhgt = -0.1, complete 0 and 1:

  (a) the one call: snow model chunk loop, streamed below-ground solver over the no-snow days, snow-day kernel, merge — only
      Tz and soilm cross PCIe;
  (b) the host route the one call replaces: `.snowmodel1`'s five whole-series arrays to the host, the day classes, the solver
      on the host-subset no-snow days with the WHOLE-SERIES below-ground plan (MCF_BELOW_STREAM=0), gridmicrosnow1 on the
      snow-day subset, the merge by day — at a raster small enough for that plan (210 kB per cell-year), compared per cell-step.

Each figure: one warm-up, then the median of --reps wall-clock runs (the calls return when their outputs are on the host).
Peak device memory of (a): the least free memory a sampling thread saw during a run, against free memory before it.

  python tools/bench_snow_below.py --rows 1024 --cols 1024 --days 365 --host-rows 256 --host-cols 256
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_snow_below.py --kernel-ab      # the snow-day kernel's two
      instantiations on the same chunks: k_microsnow_tiles<true> (below ground) and <false> (MCF_MICROSNOW_GENERIC)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import threading
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact",
        "complete", "mat", "out")
MAT = 7.5
OUT = [1, 0, 0, 1, 0, 0, 0, 0, 0, 0]


def case(rows, cols, days, complete, reqhgt=-0.1, cold=0.0, doy=60):
    from microclimf_amd import synthetic
    T = days * 24
    sw = synthetic.snow_workload(rows, cols, T, cold=cold, zref=3.5, start_doy=doy)
    a = synthetic.workload(rows, cols, T, reqhgt=reqhgt, zref=3.5, hgt_range=(0.05, 3.0), start_doy=doy, variety=True,
                           complete=bool(complete), out=OUT)
    _, _, dtm = synthetic.rasters(rows, cols)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    return sw, a, dtm, snow, micro


def _steps(days0):
    return (np.repeat(np.asarray(days0) * 24, 24) + np.tile(np.arange(24), len(days0))).astype(np.int64)


def _sub(d, idx):
    return {k: (np.asarray(v)[idx] if np.ndim(v) == 1 else v) for k, v in d.items()}


def host_route(sw, a, dtm):
    """`.snowmodel1` + `.runmicrosnow1` as the host orchestrates them, HIP behind every step"""
    from microclimf_amd import snow as S
    from microclimf_amd.api import runmicro1Cpp
    rows, cols = dtm.shape
    smod = S.snowmodel1_chunks(sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
    swe = smod["totalSWE"].copy()
    swe[np.isnan(swe)] = 0.0
    swe[np.isnan(dtm)] = np.nan
    dd = S.snowdaysfun(S.applycpp3(swe, "max"), S.applycpp3(swe, "min"))
    sdays, ndays_ = np.flatnonzero(dd["snowdays"]), np.flatnonzero(dd["nosnowdays"])
    ni, si = _steps(ndays_), _steps(sdays)
    an = dict(a, obstime=_sub(a["obstime"], ni), climdata=_sub(a["climdata"], ni), pointm=_sub(a["pointm"], ni))
    moutn = runmicro1Cpp(*[an[k] for k in ARGS])
    if not sdays.size:
        return moutn, sdays.size, ndays_.size
    s1 = np.arange(si.size)[np.repeat(np.isin(sdays, ndays_), 24)]
    s2 = np.arange(ni.size)[np.repeat(np.isin(ndays_, sdays), 24)]
    micro = {}
    for k, v in moutn.items():
        m = np.full((rows, cols, si.size), np.nan, order="F")
        m[:, :, s1] = v[:, :, s2]
        micro[k] = m
    smods = {k: np.asfortranarray((swe if k == "totalSWE" else v)[:, :, si]) for k, v in smod.items()}
    mouts = S.gridmicrosnow1(a["reqhgt"], _sub(sw["obstime"], si), _sub(sw["climdata"], si), smods, micro, sw["vegp"], sw["other"],
                             MAT, OUT)
    return S.merge_snow_outputs(moutn, mouts, sdays + 1, ndays_ + 1, rows, cols), sdays.size, ndays_.size


def timed(fn, reps):
    fn()                                   # warm-up: library load, allocations' first touch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


class FreeSampler:
    """least free device memory seen while running (hipMemGetInfo through torch, every 20 ms)"""

    def __enter__(self):
        import torch
        self.torch = torch
        torch.cuda.init()
        self.before = torch.cuda.mem_get_info(0)[0]
        self.least = self.before
        self.stop = False
        self.th = threading.Thread(target=self.loop, daemon=True)
        self.th.start()
        return self

    def loop(self):
        while not self.stop:
            self.least = min(self.least, self.torch.cuda.mem_get_info(0)[0])
            time.sleep(0.02)

    def __exit__(self, *exc):
        self.stop = True
        self.th.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--days", type=int, default=365)
    ap.add_argument("--host-rows", type=int, default=256)
    ap.add_argument("--host-cols", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-ab", action="store_true", help="one run with each instantiation of the snow-day kernel, for a profiler")
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file")
    args = ap.parse_args()
    from microclimf_amd import snow as S
    lines = []
    if args.kernel_ab:
        sw, a, dtm, snow, micro = case(args.rows, args.cols, args.days, 1)
        for generic in (False, True):
            if generic:
                os.environ["MCF_MICROSNOW_GENERIC"] = "1"
            S.runmicrosnow1(a, snow, micro, MAT, below=True)
        return
    os.environ["MCF_BELOW_STREAM"] = "0"       # (b)'s solver: the whole-series plan; (a) streams by construction
    for complete in (0, 1):
        sw, a, dtm, snow, micro = case(args.rows, args.cols, args.days, complete)
        valid = int(np.count_nonzero(~np.isnan(a["vegp"]["hgt"])))
        with FreeSampler() as fs:
            med, ts = timed(lambda: S.runmicrosnow1(a, snow, micro, MAT, below=True), args.reps)
        with S.SnowRun(a, snow, below=True) as run:
            sd, nd = run.pass1()
        cs = valid * args.days * 24
        lines.append({"leg": "a: one call", "complete": complete, "rows": args.rows, "cols": args.cols, "days": args.days,
                      "valid_cells": valid, "snow_days": int(sd.sum()), "nosnow_days": int(nd.sum()), "median_s": med, "runs_s": ts,
                      "cell_steps_per_s": cs / med, "peak_device_bytes": int(fs.before - fs.least),
                      "peak_device_bytes_per_cell_year": (fs.before - fs.least) / valid * 365.0 / args.days})
        print(json.dumps(lines[-1]), flush=True)
        del sw, a, dtm, snow, micro
        sw, a, dtm, snow, micro = case(args.host_rows, args.host_cols, args.days, complete)
        valid = int(np.count_nonzero(~np.isnan(a["vegp"]["hgt"])))
        res = {}
        med, ts = timed(lambda: res.update(r=host_route(sw, a, dtm)), args.reps)
        cs = valid * args.days * 24
        lines.append({"leg": "b: host route", "complete": complete, "rows": args.host_rows, "cols": args.host_cols, "days": args.days,
                      "valid_cells": valid, "snow_days": res["r"][1], "nosnow_days": res["r"][2], "median_s": med, "runs_s": ts,
                      "cell_steps_per_s": cs / med})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
