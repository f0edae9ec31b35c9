"""Snow point model for array weather: the host's one-point entry in a loop against the batched device entry, in one process
on one device, the bundled site's year made cold (temp - 12 C, n = 8760), maxiter = 10 as `runsnowmodela` asks.
  (a) host loop     mcf_pointmodelsnow per point on 16 sampled points, scaled to P
  (b) batch         mcf_pointmodelsnow_batch on P points: one warm-up, three repeats, each a complete call (albedo on the host,
                    uploads, kernels, results back in host arrays)
  (c) front end     frontend.snow_pointm_cells (the point stage of runsnowmodela) on an 8 x 8 climate grid, point_device=0
                    against the host loop (point_device=None)
Prints every figure and the ratios to (a); (a) / 16 is the host loop spread over 16 cores.  Writes nothing: redirect it.
Usage: python tools/pointsnow_batch_rate.py [P ...]        (default: 25 1024 4096)"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bundled import load  # noqa: E402
from microclimf_amd import _abi, frontend as F, pointmodel as PM  # noqa: E402

COLS = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "precip")
COLD, MAXITER, ZREF = 12.0, 10, 5.0


def points(weather, P, lat0, lon0):
    """P perturbed copies of the cold bundled weather (as the climate cells of tests/test_snowfast_gpu.py are made), canopies,
    sites and packs that differ from point to point"""
    rng = np.random.default_rng(12)
    W = {k: np.repeat(np.asarray(weather[k], dtype=np.float64)[None, :], P, axis=0) for k in COLS}
    W["temp"] += -COLD + rng.uniform(-1.5, 1.5, (P, 1))
    for k in ("swdown", "difrad", "windspeed", "precip"):
        W[k] *= rng.uniform(0.9, 1.1, (P, 1))
    W["difrad"] = np.minimum(W["difrad"], W["swdown"])
    hgt = rng.choice([0.0, 0.3, 1.5, 3.0], P)
    vegp = np.stack([np.where(hgt > 0, rng.uniform(0.2, 3, P), 0.0), hgt, rng.uniform(0.02, 0.3, P), rng.uniform(0, 0.5, P)], axis=1)
    other = np.stack([rng.uniform(0, 20, P), rng.uniform(0, 360, P), lat0 + rng.uniform(-1, 1, P), lon0 + rng.uniform(-1, 1, P),
                      np.full(P, ZREF), rng.uniform(0, 0.6, P), rng.integers(0, 200, P).astype(np.float64)], axis=1)
    return W, vegp, other


def main(sizes):
    if _abi.load().mcf_device_count() < 1:
        print("no HIP device: nothing measured", file=sys.stderr)
        return 2
    weather, vegp_r, soilc, dtm = load()
    obst = weather["obstime"]
    n = len(weather["temp"])
    print(f"n = {n} hourly steps, temp - {COLD:g} C, maxiter = {MAXITER}, tol = 0.5; pointmodelsnow per point")
    # (a) the host loop on 16 sampled points (one warm-up point first)
    W, vegp, other = points(weather, 17, dtm["lat"], dtm["long"])
    one = lambda p: PM.pointmodelsnow(obst, {k: W[k][p] for k in COLS}, vegp[p], other[p], "Taiga", 0.5, MAXITER)["iters"]   # noqa: E731
    one(16)
    t0 = time.perf_counter()
    its = [one(p) for p in range(16)]
    per_point = (time.perf_counter() - t0) / 16
    print(f"(a) host loop: {per_point:.4f} s per point-year (16 points, mean {np.mean(its):.1f} passes)", flush=True)
    # (b) the batch
    batch = lambda a: PM.pointmodelsnow_batch(obst, a[0], a[1], a[2], "Taiga", 0.5, MAXITER)["iters"]   # noqa: E731
    batch(points(weather, 16, dtm["lat"], dtm["long"]))                  # warm-up: code objects, first allocations
    for P in sizes:
        args = points(weather, P, dtm["lat"], dtm["long"])
        ts = []
        for r in range(4):
            t0 = time.perf_counter()
            it = batch(args)
            if r:
                ts.append(time.perf_counter() - t0)
        host, med = per_point * P, float(np.median(ts))
        print(f"(b) P = {P}: batch median {med:.3f} s (range {min(ts):.3f} - {max(ts):.3f}; mean {it.mean():.1f} passes, max "
              f"{it.max()}) | host loop scaled {host:.1f} s | ratio {host / med:.1f} x | against the host loop on 16 cores "
              f"({host / 16:.2f} s): {host / 16 / med:.2f} x", flush=True)
        del args
    # (c) the point stage of runsnowmodela on an 8 x 8 climate grid
    cr = cc = 8
    rng = np.random.default_rng(4)
    clim_c = {}
    for k in COLS:
        base = np.broadcast_to(np.asarray(weather[k], dtype=np.float64)[None, None, :], (cr, cc, n)).copy()
        if k == "temp":
            base += -COLD + rng.uniform(-1.5, 1.5, (cr, cc, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (cr, cc, 1))
        clim_c[k] = np.asfortranarray(base)
    clim_c["difrad"] = np.minimum(clim_c["difrad"], clim_c["swdown"])
    clim_c["winddir"] = np.asarray(weather["winddir"], dtype=np.float64)
    vc = {k: F.block_reduce(F.cleanvegp(vegp_r)[k], cr, cc) for k in ("pai", "hgt", "leaft", "clump")}
    clat = dtm["lat"] + 1e-4 * np.arange(cr)[:, None] + 0 * np.arange(cc)[None, :]
    clon = dtm["long"] + 1e-4 * np.arange(cc)[None, :] + 0 * np.arange(cr)[:, None]
    ob = {k: np.asarray(obst[k]) for k in ("year", "month", "day", "hour")}
    zref = max(ZREF, float(np.nanmax(np.asarray(vegp_r["hgt"], dtype=np.float64))))
    run = lambda dev: F.snow_pointm_cells(ob, clim_c, vc, clat, clon, zref, 0.0, 0.0, "Taiga", True, dev)   # noqa: E731
    run(0)
    td = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = run(0)
        td.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = run(None)
    th = time.perf_counter() - t0
    worst = max(float(np.max(np.abs(got[k] - want[k]) / (1 + np.abs(want[k])))) for k in want)
    print(f"(c) runsnowmodela's point stage 8 x 8, n = {n}: point_device=0 median {np.median(td):.3f} s (range {min(td):.3f} - "
          f"{max(td):.3f}; packing on the host included) | host loop {th:.2f} s | ratio {th / np.median(td):.1f} x | max scaled "
          f"|device - host| over pointm_c {worst:.2e}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main([int(x) for x in sys.argv[1:]] or [25, 1024, 4096]))
