#!/usr/bin/env python3
"""What the staged diagnostics cost: a plain plan run against a run with all thirteen diagnostics, same box, same process.

    python tools/diag_rate.py [--rows 1024 --cols 1024 --hours 240 --reps 5 --out profiles/diag_rate.txt]
    python tools/diag_rate.py --forcing array        # fine weather arrays, 1024^2 x 48 h  -> profiles/diag_array_rate.txt
    python tools/diag_rate.py --forcing coarse       # 8 x 8 climate cells, 1024^2 x 240 h -> appended to the same file

Both plans solve the flagship workload's geometry (synthetic.workload with variety, all ten outputs, the whole series in one
ring slot).  Each is warmed once and timed `reps` times with HIP events around mcf_plan_run_days (kernel time: no transfers);
the runs alternate so that clock drift hits both alike.  Reported: median cell-steps/s of either, their ratio, and the store
rates the two imply (10 and 23 doubles per cell-step).  `--forcing array` / `coarse`: the same for array weather
(mcf_plan_diag_enable_array; fine arrays uploaded once before the timed runs, coarse arrays resident in the plan), one warm-up and
the median of three; no ratio is fixed in advance, the file states what was measured.  Needs an MI355X; writes the figures to --out.
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from microclimf_amd import synthetic                # noqa: E402
from microclimf_amd.api import Plan                 # noqa: E402

PROFILES = Path(__file__).resolve().parents[1] / "profiles"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forcing", choices=("vector", "array", "coarse"), default="vector")
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--hours", type=int, default=0, help="default: 240, 48 with --forcing array")
    ap.add_argument("--reps", type=int, default=0, help="default: 5, 3 for array weather")
    ap.add_argument("--coarse", type=int, nargs=2, default=(8, 8), metavar=("CROWS", "CCOLS"))
    ap.add_argument("--out", default="")
    o = ap.parse_args()
    vector = o.forcing == "vector"
    hours = o.hours or (48 if o.forcing == "array" else 240)
    reps = o.reps or (5 if vector else 3)
    out = Path(o.out) if o.out else PROFILES / ("diag_rate.txt" if vector else "diag_array_rate.txt")
    ndays = hours // 24
    kw = dict(ring_days=ndays)
    if o.forcing == "coarse":
        a, rp, cp = synthetic.coarse_workload(o.rows, o.cols, hours, o.coarse[0], o.coarse[1], reqhgt=0.05, variety=True, start_doy=170)
        kw.update(coarse={"rowpos": rp, "colpos": cp})
        what = f"coarse array weather ({o.coarse[0]} x {o.coarse[1]} climate cells)"
    else:
        a = synthetic.workload(o.rows, o.cols, hours, reqhgt=0.05, variety=True, start_doy=170, array_forcing=not vector)
        kw.update(array_forcing=not vector)
        what = "vector weather" if vector else "fine array weather"
    plain = Plan(**a, **kw)
    diag = Plan(**a, **kw)
    if vector:
        diag.diag_enable("all")
    else:
        diag.diag_enable_array("all")
    if o.forcing == "array":            # the forcing ring is filled once: the timed runs are kernels only
        plain.upload_forcing_days(0, ndays, 0)
        diag.upload_forcing_days(0, ndays, 0)
    times = {"plain": [], "diag": []}
    for rep in range(reps + 1):
        for name, p in (("plain", plain), ("diag", diag)):
            p.timer_start()
            p.run_days(0, ndays, 0)
            ms = p.timer_stop()
            if rep:                     # rep 0 warms up (cell tables, code objects)
                times[name].append(ms)
    steps = plain.valid_cells * ndays * 24
    med = {k: statistics.median(v) for k, v in times.items()}
    rate = {k: steps / (med[k] * 1e-3) for k in med}
    st = {k: p.dispatch_stats() for k, p in (("plain", plain), ("diag", diag))}
    lines = [
        f"staged diagnostics rate, {what}: {o.rows} x {o.cols} cells ({plain.valid_cells} valid) x {ndays * 24} h, one warm-up and {reps} timed runs each, alternating",
        f"plain run  (10 outputs)                 : median {med['plain']:9.3f} ms  {rate['plain']:.4e} cell-steps/s  stores {rate['plain'] * 80 / 1e12:.2f} TB/s  runs {[round(t, 2) for t in times['plain']]}",
        f"diagnostics (10 outputs + 13 diagnostics): median {med['diag']:9.3f} ms  {rate['diag']:.4e} cell-steps/s  stores {rate['diag'] * 184 / 1e12:.2f} TB/s  runs {[round(t, 2) for t in times['diag']]}",
        f"ratio diagnostics / plain (time)         : {med['diag'] / med['plain']:.3f}",
        f"device bytes: plain {plain.device_bytes / 2**30:.2f} GiB, diagnostics {diag.device_bytes / 2**30:.2f} GiB",
        f"launches (fast / slow / canary trips): plain {st['plain']['fast_launches']} / {st['plain']['slow_launches']} / {st['plain']['canary_trips']}, "
        f"diagnostics {st['diag']['fast_launches']} / {st['diag']['slow_launches']} / {st['diag']['canary_trips']}",
    ]
    plain.close()
    diag.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out.parent.mkdir(parents=True, exist_ok=True)
    if o.forcing == "coarse" and out.exists():      # the fine-array figures of the same file stay
        text = out.read_text() + "\n" + text
    out.write_text(text)


if __name__ == "__main__":
    main()
