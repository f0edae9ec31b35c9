#!/usr/bin/env python3
"""What the period-summary sinks of the snow run cost beside its only other sink, the host arrays: one process, one box.

    python tools/snowrun_summary_rate.py [--rows 1024 --cols 1024 --days 0 --max-days 40 --reps 3 --out profiles/snowrun_summary_rate.txt]

A synthetic site with data.frame weather from 1 January on (snow days, no-snow days and days of both), `Tz` the only output.
--days 0: as many whole 5-day chunks as the host-output leg can hold — a quarter of the host memory that is available when
the tool starts for the one [rows, cols, steps] array, at most --max-days.  After one short warm-up call (library, clocks),
`reps` calls each of
  arrays   mcf_runmicrosnow1 with `Tz` into a host array (the only route there was)
  summary  mcf_runmicrosnow_summary, summary only: `Tz` by month, mean / minimum / maximum — no host array, no fetch_days
  + pack   the same with the snowpack's summary of totalSWE added (mean, maximum, hours above 0), folded in pass 1
host clock around the call, inputs marshalled inside it as a host session pays for them; medians.  Then, on a snow plan of the
same raster with one chunk run,
  planes   mcf_snowplan_summary_accumulate of that chunk alone: all six statistics of totalSWE, and of all five series
  copy     a device-to-device hipMemcpy of as many bytes as the kernel reads (steps x cells x 8 per series), between two
           buffers of that size (the plan does not hand out its series' addresses)
host clock around a synchronised call; medians.  Reported: series bytes read per second by planes and by copy (a copy also
WRITES as many bytes) and planes / copy.  There is no pass threshold: the file is where the measured values go.  Needs an MI355X.
"""
import argparse
import ctypes as C
import platform
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np                                   # noqa: E402

from microclimf_amd import _abi, frontend, synthetic  # noqa: E402
from microclimf_amd import snow as S                 # noqa: E402

MAT = 7.5


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        return "unknown device"


def host_available_bytes():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) * 1024
    return 8 << 30


def head(d, n):
    return {k: (np.asarray(v)[:n] if np.ndim(v) == 1 else v) for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--days", type=int, default=0)
    ap.add_argument("--max-days", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "snowrun_summary_rate.txt"))
    o = ap.parse_args()
    N = o.rows * o.cols
    avail = host_available_bytes()
    days = o.days if o.days > 0 else min(o.max_days, int(avail / 4 // (N * 24 * 8)))
    days = max(5, days // 5 * 5)
    T = days * 24
    name = device_name()
    out = [1] + [0] * 9
    sw = synthetic.snow_workload(o.rows, o.cols, T, cold=0.0, zref=3.5, start_doy=1)
    g = synthetic.workload(o.rows, o.cols, T, reqhgt=0.05, zref=3.5, hgt_range=(0.05, 3.0), start_doy=1, variety=True, out=out)
    _, _, dtm = synthetic.rasters(o.rows, o.cols)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    valid = int(np.isfinite(dtm).sum())
    # warm-up: ten days of the same site
    S.runmicrosnow1(dict(g, obstime=head(g["obstime"], 240), climdata=head(g["climdata"], 240), pointm=head(g["pointm"], 240)),
                    dict(snow, obstime=head(sw["obstime"], 240), climdata=head(sw["climdata"], 240), pointm=head(sw["pointm"], 240)),
                    dict(micro, obstime=head(sw["obstime"], 240), climdata=head(sw["climdata"], 240)), MAT)
    print(f"inputs made ({days} days), library warm", flush=True)
    tab, labels = frontend.summary_periods(g["obstime"], "month")
    msum = dict(periods=tab, nperiods=len(labels), vars=("Tz",), stats=("mean", "min", "max"))
    psum = dict(periods=tab, nperiods=len(labels), vars=("totalSWE",), stats=("mean", "max", "hours_above"), thresholds=0.0)
    legs = (("arrays", {}), ("summary", dict(summary=msum, want_arrays=False)), ("+ pack", dict(summary=msum, pack_summary=psum, want_arrays=False)))
    t = {k: [] for k, _ in legs}
    classes = None
    for rep in range(o.reps):
        for leg, kw in legs:
            t0 = time.perf_counter()
            res = S.runmicrosnow1(g, snow, micro, MAT, **kw)
            t[leg].append(time.perf_counter() - t0)
            if leg == "summary":
                classes = (int(res["snowdays"].sum()), int(res["nosnowdays"].sum()), res["summary"]["days"].tolist())
            del res
            print(f"rep {rep} {leg}: {t[leg][-1]:.3f} s", flush=True)
    m = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"snow-run summaries on {name} (host {platform.node()}): {o.rows} x {o.cols} cells x {days} days ({T} h) from 1 January, "
             f"data.frame weather, Tz the only output, 5-day chunks, one block; host memory available {avail / 2**30:.0f} GiB, "
             f"the Tz array is {N * T * 8 / 2**30:.2f} GiB; 1 warm-up call + {o.reps} timed calls per leg, medians of the host clock",
             f"   snow days {classes[0]}, no-snow days {classes[1]}, periods {labels} with {classes[2]} counted days"]
    for leg, what in (("arrays", "Tz into a host array"), ("summary", "summary only: Tz by month, mean / min / max"),
                      ("+ pack", "the same + totalSWE by month, mean / max / hours above 0")):
        lines.append(f"   {leg:8s}: {m[leg]:8.3f} s  {valid * T / m[leg]:.3e} cell-steps/s  ratio to arrays {m[leg] / m['arrays']:.3f}  "
                     f"({what})  runs {[round(x, 3) for x in t[leg]]}")
    # ---- the planes kernel alone, beside a copy of as many bytes
    hip = C.CDLL(_abi._needed_hip_soname(_abi.LIB_PATH) or "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    D2D = 3
    ten = {k: head(sw[k], 240) for k in ("obstime", "climdata", "pointm")}
    for sel in (("totalSWE",), _abi.SNOWDRIVER_OUT):
        with S.SnowPlan(ten["obstime"], ten["climdata"], ten["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02,
                        keep_results=False) as p:
            s, n = p.surface_partial()
            ts, tn = p.prepare_chunk(0, surface_mean=s / n)
            p.run_chunk(0, ts / tn)
            p.summary_enable(np.zeros(10, dtype=np.int32), sel, _abi.STAT_NAMES, 0.0)
            read_bytes = len(sel) * 120 * N * 8
            a, b = C.c_void_p(), C.c_void_p()
            if hip.hipMalloc(C.byref(a), read_bytes) != 0 or hip.hipMalloc(C.byref(b), read_bytes) != 0:
                raise SystemExit("hipMalloc of the copy buffers failed")
            acc, cp = [], []
            for rep in range(o.reps + 3):
                p.summary_reset()
                hip.hipDeviceSynchronize()
                t0 = time.perf_counter()
                p.summary_accumulate(0)
                hip.hipDeviceSynchronize()
                t1 = time.perf_counter()
                rc = hip.hipMemcpy(b, a, read_bytes, D2D)
                hip.hipDeviceSynchronize()
                t2 = time.perf_counter()
                if rc != 0:
                    raise SystemExit(f"the yardstick copy failed ({rc})")
                if rep:
                    acc.append((t1 - t0) * 1e3)
                    cp.append((t2 - t1) * 1e3)
            hip.hipFree(a)
            hip.hipFree(b)
        ma, mc = statistics.median(acc), statistics.median(cp)
        rate = lambda ms: read_bytes / (ms * 1e-3) / 1e12                              # noqa: E731
        lines += [f"-- planes kernel, six statistics of {len(sel)} series, one period: {read_bytes / 2**30:.2f} GiB read per 5-day chunk",
                  f"   accumulate : {ma:9.3f} ms per chunk  reads {rate(ma):.2f} TB/s  runs {[round(x, 3) for x in acc]}",
                  f"   d2d copy   : {mc:9.3f} ms per chunk  reads {rate(mc):.2f} TB/s (and writes as much)  runs {[round(x, 3) for x in cp]}",
                  f"   ratio accumulate / copy (read rate): {mc / ma:.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    Path(o.out).write_text(text)


if __name__ == "__main__":
    main()
