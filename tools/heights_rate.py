"""A temperature-height profile, the loop of frontend.runmicro calls against one frontend.runmicro_heights, on one device: one
process, one warm-up and five repeats of each, every span ending when the call has returned its arrays (the entries
synchronise their plan before they return).
  loop      for h in heights: frontend.runmicro(mp, h, ...)        terrain, wetness index, scipy's foliage profile, uploads,
                                                                    plan and ring once per height
  one plan  frontend.runmicro_heights(mp, heights, ...)             all of that once; per height k_foliage, the cell images, the solve
and the foliage profile alone, frontend.foliageden (scipy, host) against api.foliageden(device=0) (upload, k_foliage, download).
Two sizes: the vignette's 5 x 5 cells x 288 h x 21 heights, and 1024^2 cells x 240 h x 5 heights (Tz only).
Prints medians, ranges and ratios into profiles/heights_rate.txt; exits non-zero unless the one-plan route's slowest repeat beats
the loop's fastest at both sizes (it does a strict subset of the loop's work).
Usage: python tools/heights_rate.py [--small-only]"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bundled import load                                                     # noqa: E402
from microclimf_amd import api, frontend as F, synthetic                      # noqa: E402

TZ = (1, 0, 0, 0, 0, 0, 0, 0, 0, 0)


def vignette_site():
    weather, _, _, dtm = load()
    one = np.ones((5, 5))
    dem = {"z": 0 * one, "res": 10.0, "lat": dtm["lat"], "long": dtm["long"]}
    vegp = {"pai": 3.0 * one, "hgt": 10.0 * one, "x": one, "gsmax": 0.1 * one, "leafr": 0.3 * one, "clump": 0 * one,
            "leafd": 0.05 * one, "leaft": 0.15 * one}
    soilc = {"soiltype": 7 * one, "groundr": 0.15 * one}
    mp = F.subsetpointmodel(F.runpointmodel(weather, 10.0, dem, vegp, soilc), tstep="month", what="tmax")
    return mp, vegp, soilc, dem, [float(h) for h in 10 ** (np.arange(-10, 11) / 10)]


def big_site(n=1024, hours=240):
    weather, _, _, dtm = load(hours)
    v, _, z = synthetic.rasters(n, n, hgt_range=(0.05, 6.0), na_frac=0.01)
    vegp = {k: np.asfortranarray(v[k]) for k in F.VEG_KEYS}
    soilc = {"soiltype": np.full((n, n), 7.0), "groundr": np.full((n, n), 0.15)}
    dem = {"z": np.asfortranarray(z), "res": 5.0, "lat": dtm["lat"], "long": dtm["long"]}
    mp = F.runpointmodel(weather, 1.0, dem, vegp, soilc)
    return mp, vegp, soilc, dem, [0.05, 0.3, 1.0, 2.5, 5.0]


def loop(mp, vegp, soilc, dem, heights):
    return [F.runmicro(mp, h, vegp, soilc, dem, out=TZ)["Tz"] for h in heights]


def one_plan(mp, vegp, soilc, dem, heights):
    return F.runmicro_heights(mp, heights, vegp, soilc, dem, out=TZ)["Tz"]


def timed(fn, *args, repeats=5):
    ts = []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        res = fn(*args)
        t1 = time.perf_counter()
        del res
        print(f"  {fn.__name__} repeat {r}: {t1 - t0:.3f} s", file=sys.stderr, flush=True)
        if r:
            ts.append(t1 - t0)
    return np.array(ts)


def line(name, t):
    return f"{name} median {np.median(t):.4f} s (range {t.min():.4f} - {t.max():.4f})"


def main(argv):
    out, ok = [], True
    sites = [("vignette 5 x 5 x 288 h x 21 heights", vignette_site)]
    if "--small-only" not in argv:
        sites.append(("1024^2 x 240 h x 5 heights", big_site))
    for label, make in sites:
        mp, vegp, soilc, dem, heights = make()
        tl = timed(loop, mp, vegp, soilc, dem, heights)
        to = timed(one_plan, mp, vegp, soilc, dem, heights)
        faster = to.max() < tl.min()
        ok &= faster
        out.append(f"{label}: {line('loop of runmicro', tl)} | {line('runmicro_heights', to)} | ratio of medians "
                   f"{np.median(tl) / np.median(to):.2f} | one plan's slowest < loop's fastest: {faster}")
        hgt, pai = np.asfortranarray(vegp["hgt"]), np.asfortranarray(vegp["pai"])
        th = timed(lambda: F.foliageden(heights[1], hgt, pai))
        td = timed(lambda: api.foliageden(hgt, pai, heights[1], device=0))
        out.append(f"{label}: foliage profile of one height, {hgt.size} cells: {line('frontend.foliageden (scipy, host)', th)} | "
                   f"{line('api.foliageden(device=0), upload + k_foliage + download', td)} | ratio of medians {np.median(th) / np.median(td):.2f}")
        print(out[-2], out[-1], sep="\n", flush=True)
    (ROOT / "profiles" / "heights_rate.txt").write_text("\n".join(out) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
