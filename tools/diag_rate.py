#!/usr/bin/env python3
"""What the staged diagnostics cost: a plain plan run against a run with all thirteen diagnostics, same box, same process.

    python tools/diag_rate.py [--rows 1024 --cols 1024 --hours 240 --reps 5 --out profiles/diag_rate.txt]

Both plans solve the flagship workload's geometry (synthetic.workload with variety, all ten outputs, the whole series in one
ring slot).  Each is warmed once and timed `reps` times with HIP events around mcf_plan_run_days (kernel time: no transfers);
the runs alternate so that clock drift hits both alike.  Reported: median cell-steps/s of either, their ratio, and the store
rates the two imply (10 and 23 doubles per cell-step).  Needs an MI355X; writes the figures to --out.
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from microclimf_amd import synthetic                # noqa: E402
from microclimf_amd.api import Plan                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--hours", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "diag_rate.txt"))
    o = ap.parse_args()
    ndays = o.hours // 24
    a = synthetic.workload(o.rows, o.cols, o.hours, reqhgt=0.05, variety=True, start_doy=170)
    plain = Plan(**a, ring_days=ndays)
    diag = Plan(**a, ring_days=ndays)
    diag.diag_enable("all")
    times = {"plain": [], "diag": []}
    for rep in range(o.reps + 1):
        for name, p in (("plain", plain), ("diag", diag)):
            p.timer_start()
            p.run_days(0, ndays, 0)
            ms = p.timer_stop()
            if rep:                     # rep 0 warms up (cell tables, code objects)
                times[name].append(ms)
    steps = plain.valid_cells * ndays * 24
    med = {k: statistics.median(v) for k, v in times.items()}
    rate = {k: steps / (med[k] * 1e-3) for k in med}
    lines = [
        f"staged diagnostics rate: {o.rows} x {o.cols} cells ({plain.valid_cells} valid) x {ndays * 24} h, {o.reps} timed runs each, alternating",
        f"plain run  (10 outputs)                 : median {med['plain']:9.3f} ms  {rate['plain']:.4e} cell-steps/s  stores {rate['plain'] * 80 / 1e12:.2f} TB/s  runs {[round(t, 2) for t in times['plain']]}",
        f"diagnostics (10 outputs + 13 diagnostics): median {med['diag']:9.3f} ms  {rate['diag']:.4e} cell-steps/s  stores {rate['diag'] * 184 / 1e12:.2f} TB/s  runs {[round(t, 2) for t in times['diag']]}",
        f"ratio diagnostics / plain (time)         : {med['diag'] / med['plain']:.3f}",
        f"device bytes: plain {plain.device_bytes / 2**30:.2f} GiB, diagnostics {diag.device_bytes / 2**30:.2f} GiB",
    ]
    plain.close()
    diag.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    Path(o.out).write_text(text)


if __name__ == "__main__":
    main()
