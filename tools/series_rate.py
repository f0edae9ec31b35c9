#!/usr/bin/env python3
"""What the series sink costs, and the device time of k_series_zones beside k_summary_acc on the same ring: one box.

    python tools/series_rate.py [--rows 1024 --cols 1024 --hours 240 --chunk 5 --reps 5 --out profiles/series_rate.txt]

Without --step this is the driver: one child process per sink set-up, each under its own `timeout`, chained with `&&` (a
set-up that fails or overruns ends the run; nothing is started after it), their lines gathered into --out.
  points   100 points alone
  zones16  16 coherent zones: elevation bands of the synthetic terrain
  zones64  64 speckled zones: (cell * 13) % 64
With --step NAME: that set-up, for `Tz` alone and for all ten outputs (one plan each; vector forcing, all ten outputs solved).
The plan carries the series sink and a period summary (mean, min, max over one period) of the same variables.  After one
warm-up pass, `reps` passes of
  plain    the run_days loop over the series in chunks of `chunk` days
  sink     the same loop with series_accumulate behind every chunk
  series   series_accumulate alone on a filled slot (series_reset before each, outside the timer): k_series_zones, and
           k_series_points where there are points
  summary  summary_accumulate alone on the same slot in the same pass: k_summary_acc reads exactly the bytes k_series_zones reads
timed with HIP events on the plan's stream.  Medians, and the ratios sink / plain and series / summary.  There is no pass
threshold: the file is where the measured values go.  Needs an MI355X.
"""
import argparse
import platform
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS = ("points", "zones16", "zones64")
# what the file says when the coherent-zone case takes more than twice k_summary_acc's time (reasoned from the three set-ups'
# figures: the reads are the same bytes in all of them, and the speckled case flushes four times the entries in half the time)
BINDS = ("     what binds: the LDS table updates, not the reads or the flush.  Where no 64-cell run carries one label every wave takes\n"
         "     the lane-by-lane path: 96 64-bit LDS atomics per cell-day (4 rows x 24 hours), and lanes of a wave that share a label hit\n"
         "     one table entry in the same instruction and are serialised - which is why a few labels per wave cost about twice what 64\n"
         "     speckled labels (no two lanes of a wave on one entry) cost.  The wave-reduced path needs zones wider than 64 cells of a column.")


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        return "unknown device"


def step(o):
    import numpy as np
    from microclimf_amd import _abi, synthetic
    from microclimf_amd.api import Plan
    nd = o.hours // 24
    if nd % o.chunk:
        raise SystemExit("--chunk must divide the days: the accumulate timings take a full slot")
    a = synthetic.workload(o.rows, o.cols, o.hours, reqhgt=0.05, variety=True, start_doy=176)
    N = o.rows * o.cols
    cell = np.arange(N, dtype=np.int64)
    points = zones = None
    what = ""
    if o.step == "points":
        points = (cell[:100] * (N // 100) + 17) % N
        what = "100 points alone"
    elif o.step == "zones16":
        z = synthetic.rasters(o.rows, o.cols)[2] - synthetic.uniform(47, cell.reshape((o.rows, o.cols), order="F"))   # (less its per-cell noise)
        edges = np.nanquantile(z, np.arange(1, 16) / 16)
        zones = np.where(np.isnan(z), -1, np.digitize(z, edges)).astype(np.int32)
        what = "16 coherent zones (elevation bands)"
    else:
        zones = ((cell * 13) % 64).reshape((o.rows, o.cols), order="F").astype(np.int32)
        what = "64 speckled zones ((cell * 13) % 64)"
    lines = []
    if zones is not None:      # waves of 64 consecutive cells with one label: the share that takes the wave-reduced path
        lab = zones.reshape(-1, order="F")[:N // 64 * 64].reshape(-1, 64)
        lines.append(f"-- {what}: {100.0 * (lab == lab[:, :1]).all(axis=1).mean():.1f} % of 64-cell runs carry one label")
    else:
        lines.append(f"-- {what}")
    for sel_name, sel in (("Tz alone", ("Tz",)), ("all ten", _abi.OUT_NAMES)):
        with Plan(**a, ring_days=o.chunk) as p:
            p.summary_enable(np.zeros(nd, dtype=np.int32), sel, ("mean", "min", "max"))
            p.series_enable(points, zones, sel, _abi.ZSTAT_NAMES)
            lay = p.ring_layout()
            ntiles = (lay["cells"] + lay["cells_per_tile"] - 1) // lay["cells_per_tile"]
            read_bytes = len(sel) * ntiles * lay["block_doubles"] * 8 * o.chunk          # what one fold of a full slot reads
            t = {"plain": [], "sink": [], "series": [], "summary": []}
            for rep in range(o.reps + 1):
                p.timer_start()
                for d0 in range(0, nd, o.chunk):
                    p.run_days(d0, o.chunk, 0)
                plain = p.timer_stop()
                p.series_reset()
                p.timer_start()
                for d0 in range(0, nd, o.chunk):
                    p.run_days(d0, o.chunk, 0)
                    p.series_accumulate(0, 0, d0, o.chunk)
                sink = p.timer_stop()
                p.series_reset()
                p.summary_reset()
                p.sync()
                p.timer_start()
                p.series_accumulate(0, 0, nd - o.chunk, o.chunk)                         # the slot holds the last chunk
                ser = p.timer_stop()
                p.timer_start()
                p.summary_accumulate(0, 0, nd - o.chunk, o.chunk)
                summ = p.timer_stop()
                if rep:
                    for k, v in (("plain", plain), ("sink", sink), ("series", ser), ("summary", summ)):
                        t[k].append(v)
            valid = p.valid_cells
        m = {k: statistics.median(v) for k, v in t.items()}
        rate = lambda ms: read_bytes / (ms * 1e-3) / 1e12                                # noqa: E731
        lines += [
            f"   {sel_name}: {read_bytes / 2**30:.2f} GiB of ring per {o.chunk}-day slot",
            f"     plain loop        : {m['plain']:9.3f} ms  ({valid * nd * 24 / (m['plain'] * 1e-3):.3e} cell-steps/s)  runs {[round(x, 2) for x in t['plain']]}",
            f"     with series sink  : {m['sink']:9.3f} ms  ratio sink / plain {m['sink'] / m['plain']:.3f}  runs {[round(x, 2) for x in t['sink']]}",
            f"     series_accumulate : {m['series']:9.3f} ms per slot" + (f"  reads {rate(m['series']):.2f} TB/s" if zones is not None else "") +
            f"  runs {[round(x, 3) for x in t['series']]}",
            f"     summary_accumulate: {m['summary']:9.3f} ms per slot  reads {rate(m['summary']):.2f} TB/s  runs {[round(x, 3) for x in t['summary']]}",
        ]
        if zones is not None:
            lines.append(f"     ratio k_series_zones / k_summary_acc (device time, same bytes): {m['series'] / m['summary']:.2f}")
            if o.step == "zones16" and m["series"] > 2 * m["summary"]:
                lines.append(BINDS)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    Path(o.part).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--hours", type=int, default=240)
    ap.add_argument("--chunk", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds per set-up")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "series_rate.txt"))
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--part", help="where a step leaves its lines")
    o = ap.parse_args()
    if o.step:
        return step(o)
    out = Path(o.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    parts = [out.with_suffix(f".{s}.part") for s in STEPS]
    common = f"--rows {o.rows} --cols {o.cols} --hours {o.hours} --chunk {o.chunk} --reps {o.reps}"
    chain = " && ".join(f"timeout -k 10 {o.step_timeout} {sys.executable} {Path(__file__).resolve()} {common} --step {s} --part {q}"
                        for s, q in zip(STEPS, parts))
    rc = subprocess.run(["bash", "-c", chain]).returncode
    head = (f"series sink on {device_name()} (host {platform.node()}): {o.rows} x {o.cols} cells x {o.hours // 24 * 24} h, vector forcing, "
            f"all ten outputs solved, chunks of {o.chunk} days, 1 warm-up + {o.reps} timed passes, medians; all four zone statistics\n")
    body = "".join(q.read_text() for q in parts if q.exists())
    for q in parts:
        q.unlink(missing_ok=True)
    if rc != 0:
        body += f"(the chain of set-ups ended with exit status {rc}: the set-ups after it were not run)\n"
    out.write_text(head + body)
    print(head + body, end="")
    return rc


if __name__ == "__main__":
    sys.exit(main())
