"""Host entry against device entry of the vegetation pre-compute, in one run: one find_lref, one fill_na and the whole
leafrfromalb at 1024 x 1024 and 4096 x 4096 cells (tools/leafr_rate.py > profiles/leafr_rate.txt).

The comparison is the device entry (host pointers in and out, so uploads and downloads are inside the time) against THIS
library's host entry on one core — not against the reference, which nobody has timed at these sizes.  Synthetic raster:
gamma-distributed pai (mean 2) with 5 % holes, x in 0.3..3 with 10 % exact ones, alb in 0.05..0.4.  One warm-up call, then
the median of `--runs` calls; a host call that would take minutes (the whole loop at 4096 x 4096) is timed `--slow-runs`
times without a warm-up, and the output says so.

    python tools/leafr_rate.py [--sizes 1024 4096] [--runs 5] [--slow-runs 1] [--device 0]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from microclimf_amd import vegprep as V      # noqa: E402


def raster(n, seed=1):
    rng = np.random.default_rng(seed)
    pai = rng.gamma(2.0, 1.0, (n, n))
    pai[rng.random((n, n)) < 0.05] = np.nan
    x = rng.uniform(0.3, 3.0, (n, n))
    x[rng.random((n, n)) < 0.10] = 1.0
    alb = rng.uniform(0.05, 0.4, (n, n))
    return pai, x, alb


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
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--slow-runs", type=int, default=1)
    ap.add_argument("--slow-cells", type=int, default=4_000_000, help="host whole-loop calls above this many cells are slow ones")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    print("leafrfromalb: device entry against this library's host entry on one core (seconds, median of runs after one warm-up)")
    for n in a.sizes:
        pai, x, alb = raster(n)
        gref = np.where(np.isnan(x), np.nan, 0.15)
        holes = np.where(np.isnan(pai), np.nan, alb)
        work = (("find_lref", lambda d: V.find_lref(pai, gref, x, alb, 0.5, device=d)),
                ("fill_na", lambda d: V.fill_na(holes, x, device=d)),
                ("leafrfromalb", lambda d: V.leafrfromalb(pai, x, alb, 0.5, device=d)))
        for name, fn in work:
            slow = name == "leafrfromalb" and n * n > a.slow_cells
            th = timed(lambda: fn(None), a.slow_runs if slow else a.runs, warm=not slow)
            td = timed(lambda: fn(a.device), a.runs)
            note = f"  (host: {a.slow_runs} run, no warm-up)" if slow else ""
            print(f"{n:5d} x {n:<5d} {name:13s} host {th:10.4f} s   device {td:10.4f} s   host / device {th / td:8.1f}{note}", flush=True)
        r = V.leafrfromalb(pai, x, alb, 0.5, device=a.device)
        print(f"{n:5d} x {n:<5d} passes {r['iterations']}, lref first {r['lref_first']}, "
              f"last mean differences {r['mxdif_gref']:.3e} / {r['mxdif_leaf']:.3e}", flush=True)


if __name__ == "__main__":
    main()
