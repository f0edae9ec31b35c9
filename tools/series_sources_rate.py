#!/usr/bin/env python3
"""What the series sink costs on the snow model and the snow run, and k_series_planes beside k_summary_planes on the same chunk.

    python tools/series_sources_rate.py [--rows 1024 --cols 1024 --days 40 --reps 5 --out profiles/series_sources_rate.txt]

Without --step this is the driver: one child process per step, each under its own `timeout`, chained with `&&` (a step that
fails or overruns ends the run; nothing is started after it), their lines gathered into --out.
  fold16 / fold64   a SnowPlan (data.frame weather) with the series sink (all four zone statistics) and the period summary
                    (mean, min, max over one period) of the same series, `totalSWE` alone and all five; zones: 16 elevation
                    bands / 64 speckled labels.  After a warm-up chunk, per chunk of 5 days: series_accumulate (k_series_planes;
                    the state reset before, outside the timer) and summary_accumulate (k_summary_planes: the same bytes) on the
                    chunk just run, host clock around a device synchronisation.
  model             the whole mcf_snowmodel1_series call and the whole mcf_snowmodel1_summary call on the same inputs (64 zones)
  run               the snow run (SnowRun, pass 1 + pass 2 without arrays) with the series sink on Tz and the snowpack's
                    totalSWE (64 zones), and with the period summary of the same two in its place: a run needs one sink or the
                    arrays, so "without the sink" is "with the summary instead"
Medians of --reps, and the ratios sink / comparator.  There is no pass threshold: the file is where the measured values go.
Needs an MI355X.
"""
import argparse
import platform
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS = ("fold16", "fold64", "model", "run")


def device_sync():
    import torch
    torch.cuda.synchronize()


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        return "unknown device"


def case(o):
    import numpy as np
    from microclimf_amd import synthetic
    T = o.days * 24
    sw = synthetic.snow_workload(o.rows, o.cols, T, cold=0.0, zref=3.5, start_doy=90)
    _, _, dtm = synthetic.rasters(o.rows, o.cols)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    args = (sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
    return sw, dtm, args


def zone_map(o, which):
    import numpy as np
    from microclimf_amd import synthetic
    N = o.rows * o.cols
    cell = np.arange(N, dtype=np.int64)
    if which == 16:
        z = synthetic.rasters(o.rows, o.cols)[2] - synthetic.uniform(47, cell.reshape((o.rows, o.cols), order="F"))   # (less its per-cell noise)
        edges = np.nanquantile(z, np.arange(1, 16) / 16)
        zones, what = np.where(np.isnan(z), -1, np.digitize(z, edges)).astype(np.int32), "16 coherent zones (elevation bands)"
    else:
        zones, what = ((cell * 13) % 64).reshape((o.rows, o.cols), order="F").astype(np.int32), "64 speckled zones ((cell * 13) % 64)"
    lab = zones.reshape(-1, order="F")[:N // 64 * 64].reshape(-1, 64)
    return zones, f"{what}: {100.0 * (lab == lab[:, :1]).all(axis=1).mean():.1f} % of 64-cell runs carry one label"


def med(v):
    return statistics.median(v)


def step_fold(o, nz):
    import numpy as np
    from microclimf_amd import _abi
    from microclimf_amd import snow as S
    sw, dtm, args = case(o)
    zones, what = zone_map(o, nz)
    lines = [f"-- fold per 5-day chunk, {what}"]
    for sel_name, sel in (("totalSWE alone", ("totalSWE",)), ("all five", _abi.SNOWDRIVER_OUT)):
        t = {"series": [], "summary": []}
        with S.SnowPlan(*args, keep_results=False) as p:
            p.series_enable(None, zones, sel, _abi.ZSTAT_NAMES)
            p.summary_enable(np.zeros(o.days, dtype=np.int32), sel, ("mean", "min", "max"))
            for ch in range(min(p.chunks, o.reps + 1)):
                ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
                p.run_chunk(ch, ts / tn)
                device_sync()
                t0 = time.perf_counter()
                p.series_accumulate(ch)
                device_sync()
                t1 = time.perf_counter()
                p.summary_accumulate(ch)
                device_sync()
                t2 = time.perf_counter()
                if ch:
                    t["series"].append((t1 - t0) * 1e3)
                    t["summary"].append((t2 - t1) * 1e3)
        read = len(sel) * o.rows * o.cols * 120 * 8
        lines += [f"   {sel_name}: {read / 2**30:.2f} GiB of series per chunk",
                  f"     series_accumulate  (k_series_planes) : {med(t['series']):9.3f} ms  reads {read / (med(t['series']) * 1e-3) / 1e12:.2f} TB/s  runs {[round(x, 3) for x in t['series']]}",
                  f"     summary_accumulate (k_summary_planes): {med(t['summary']):9.3f} ms  reads {read / (med(t['summary']) * 1e-3) / 1e12:.2f} TB/s  runs {[round(x, 3) for x in t['summary']]}",
                  f"     ratio k_series_planes / k_summary_planes (same bytes): {med(t['series']) / med(t['summary']):.2f}"]
    return lines


def step_model(o):
    import numpy as np
    from microclimf_amd import snow as S
    sw, dtm, args = case(o)
    zones, what = zone_map(o, 64)
    t = {"series": [], "summary": []}
    for rep in range(o.reps + 1):
        t0 = time.perf_counter()
        S.snowmodel1_series(*args, zones=zones, vars=("totalSWE",), stats=("mean", "min", "max", "count"))
        t1 = time.perf_counter()
        S.snowmodel1_summary(*args, periods=np.zeros(o.days, dtype=np.int32), vars=("totalSWE",), stats=("mean", "min", "max"))
        t2 = time.perf_counter()
        if rep:
            t["series"].append(t1 - t0)
            t["summary"].append(t2 - t1)
    return [f"-- the snow model alone, totalSWE, {what}",
            f"     mcf_snowmodel1_series : {med(t['series']):8.3f} s  runs {[round(x, 3) for x in t['series']]}",
            f"     mcf_snowmodel1_summary: {med(t['summary']):8.3f} s  runs {[round(x, 3) for x in t['summary']]}",
            f"     ratio series / summary (whole calls, marshalling included): {med(t['series']) / med(t['summary']):.3f}"]


def step_run(o):
    import numpy as np
    from microclimf_amd import snow as S
    from microclimf_amd import synthetic
    sw, dtm, args = case(o)
    zones, what = zone_map(o, 64)
    a = synthetic.workload(o.rows, o.cols, o.days * 24, reqhgt=0.05, zref=3.5, hgt_range=(0.05, 3.0), start_doy=90, variety=True)
    a = dict(a, out=[1] + [0] * 9)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    tab = np.zeros(o.days, dtype=np.int32)
    t = {"series": [], "summary": []}
    for rep in range(o.reps + 1):
        for kind in ("series", "summary"):
            with S.SnowRun(a, snow) as run:
                if kind == "series":
                    run.series_enable(dict(zones=zones, vars=("Tz",), stats=("mean", "min", "max", "count")),
                                      dict(zones=zones, vars=("totalSWE",), stats=("mean", "min", "max", "count")))
                else:
                    run.summary_enable(dict(periods=tab, vars=("Tz",), stats=("mean", "min", "max")),
                                       dict(periods=tab, vars=("totalSWE",), stats=("mean", "min", "max"), thresholds=0.0))
                device_sync()
                t0 = time.perf_counter()
                run.pass1()
                run.pass2(micro, 7.5, want_arrays=False)
                device_sync()
                if rep:
                    t[kind].append(time.perf_counter() - t0)
    return [f"-- the snow run (pass 1 + pass 2, no arrays), Tz and the snowpack's totalSWE, {what}",
            f"     with the series sink       : {med(t['series']):8.3f} s  runs {[round(x, 3) for x in t['series']]}",
            f"     with the summary in its place: {med(t['summary']):8.3f} s  runs {[round(x, 3) for x in t['summary']]}",
            f"     ratio series / summary: {med(t['series']) / med(t['summary']):.3f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--days", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per step")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "series_sources_rate.txt"))
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--part", help="where a step leaves its lines")
    o = ap.parse_args()
    if o.step:
        lines = step_fold(o, 16) if o.step == "fold16" else step_fold(o, 64) if o.step == "fold64" else step_model(o) if o.step == "model" else step_run(o)
        text = "\n".join(lines) + "\n"
        print(text, end="", flush=True)
        Path(o.part).write_text(text)
        return 0
    out = Path(o.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    parts = [out.with_suffix(f".{s}.part") for s in STEPS]
    common = f"--rows {o.rows} --cols {o.cols} --days {o.days} --reps {o.reps}"
    chain = " && ".join(f"timeout -k 10 {o.step_timeout} {sys.executable} {Path(__file__).resolve()} {common} --step {s} --part {q}"
                        for s, q in zip(STEPS, parts))
    rc = subprocess.run(["bash", "-c", chain]).returncode
    head = (f"series sink's further sources on {device_name()} (host {platform.node()}): {o.rows} x {o.cols} cells x {o.days} days, data.frame "
            f"weather, 5-day chunks, 1 warm-up + {o.reps} timed, medians\n")
    body = "".join(q.read_text() for q in parts if q.exists())
    for q in parts:
        q.unlink(missing_ok=True)
    if rc != 0:
        body += f"(the chain of steps ended with exit status {rc}: the steps after it were not run)\n"
    out.write_text(head + body)
    print(head + body, end="")
    return rc


if __name__ == "__main__":
    sys.exit(main())
