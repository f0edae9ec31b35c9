"""Point model for array weather: the host's one-point entries in a loop against the batched device entries, in one process
on one device, the bundled site's year (n = 8760).
  (a) host loop     mcf_weatherhgt + mcf_bigleaf + mcf_pointmprocess per point on 16 sampled points, scaled to P
  (b) batch         mcf_weatherhgt_batch + mcf_bigleaf_batch + mcf_pointmprocess_batch on P points: one warm-up, three repeats,
                    each a complete call (uploads, kernels, results back in host arrays)
  (c) front end     frontend.runpointmodela on an 8 x 8 climate grid, device=0 against the host loop (device=None)
Prints every figure and the ratios to (a); (a) / 16 is the host loop spread over 16 cores.  Writes nothing: redirect it.
Usage: python tools/pointmodel_batch_rate.py [P ...]        (default: 64 1024 4096)"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bundled import load  # noqa: E402
from microclimf_amd import _abi, frontend as F, pointmodel as PM  # noqa: E402

COLS = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed")
VEGP = np.array([0.5, 2.0, 1.0, 0.1, 0.4, 0.2, 0.05, 0.97, 0.33, 100.0])
GROUNDP = np.array([0.15, 0.0, 180.0, 0.97, 1.53, 0.509, 0.06, 0.5422, 5.2, -5.6, 0.42, 0.074])
ZREF, ZOUT, MAXITER = 2.0, 10.0, 20


def points(weather, P, lat0, lon0):
    """P perturbed copies of the bundled weather (as the climate cells of tests/test_frontend_gpu.py are made), canopies
    and sites that differ from point to point"""
    rng = np.random.default_rng(11)
    W = {k: np.repeat(np.asarray(weather[k], dtype=np.float64)[None, :], P, axis=0) for k in COLS}
    W["temp"] += rng.uniform(-1.5, 1.5, (P, 1))
    for k in ("swdown", "difrad", "windspeed"):
        W[k] *= rng.uniform(0.9, 1.1, (P, 1))
    W["difrad"] = np.minimum(W["difrad"], W["swdown"])
    W["windspeed"] = np.maximum(W["windspeed"], 0.5)
    n = W["temp"].shape[1]
    vegp = np.tile(VEGP, (P, 1))
    vegp[:, 0] = rng.uniform(0.1, 1.8, P)
    vegp[:, 1] = rng.uniform(0.2, 4.0, P)
    groundp = np.tile(GROUNDP, (P, 1))
    soilm = np.repeat(rng.uniform(0.1, 0.4, (P, n // 24)), 24, axis=1)
    return W, vegp, groundp, soilm, lat0 + rng.uniform(-1, 1, P), lon0 + rng.uniform(-1, 1, P)


def host_chain(obst, W, vegp, groundp, soilm, lat, lon, p):
    w = {k: W[k][p] for k in COLS}
    w = PM.weatherhgtCpp(obst, w, ZREF, ZOUT, ZOUT, lat[p], lon[p])
    bl = PM.BigLeafCpp(obst, w, vegp[p], groundp[p], soilm[p], lat[p], lon[p], 25.0, ZOUT, MAXITER, 0.5, 0.5, 0.1, True)
    PM.pointmprocess({"windspeed": w["windspeed"], "tc": w["temp"], "rh": w["relhum"], "pk": w["pres"], "uf": bl["uf"],
                      "soilm": soilm[p], "RabsG": bl["RabsG"]}, ZOUT, vegp[p, 0], vegp[p, 1], groundp[p, 4], groundp[p, 5],
                     groundp[p, 6], groundp[p, 7])
    return bl["iters"]


def device_chain(obst, W, vegp, groundp, soilm, lat, lon):
    w = PM.weatherhgt_batch(obst, W, ZREF, ZOUT, ZOUT, lat, lon)
    bl = PM.BigLeafBatch(obst, w, vegp, groundp, soilm, lat, lon, 25.0, ZOUT, MAXITER, 0.5, 0.5, True)
    PM.pointmprocess_batch({"windspeed": w["windspeed"], "tc": w["temp"], "rh": w["relhum"], "pk": w["pres"], "uf": bl["uf"],
                            "soilm": soilm, "RabsG": bl["RabsG"]}, ZOUT, vegp[:, 0], vegp[:, 1], groundp[:, 4], groundp[:, 5],
                           groundp[:, 6], groundp[:, 7])
    return bl["iters"]


def main(sizes):
    if _abi.load().mcf_device_count() < 1:
        print("no HIP device: nothing measured", file=sys.stderr)
        return 2
    weather, vegp_r, soilc, dtm = load()
    obst = weather["obstime"]
    n = len(weather["temp"])
    print(f"n = {n} hourly steps, maxiter = {MAXITER}, yearG on; weatherhgt {ZREF} m -> {ZOUT} m, BigLeaf, pointmprocess per point")
    # (a) the host loop on 16 sampled points (one warm-up point first)
    W, vegp, groundp, soilm, lat, lon = points(weather, 17, dtm["lat"], dtm["long"])
    host_chain(obst, W, vegp, groundp, soilm, lat, lon, 16)
    t0 = time.perf_counter()
    its = [host_chain(obst, W, vegp, groundp, soilm, lat, lon, p) for p in range(16)]
    per_point = (time.perf_counter() - t0) / 16
    print(f"(a) host loop: {per_point:.4f} s per point-year (16 points, mean {np.mean(its):.1f} iterations)", flush=True)
    # (b) the batch
    device_chain(obst, *points(weather, 16, dtm["lat"], dtm["long"]))                # warm-up: code objects, first allocations
    for P in sizes:
        args = points(weather, P, dtm["lat"], dtm["long"])
        ts = []
        for r in range(4):
            t0 = time.perf_counter()
            it = device_chain(obst, *args)
            if r:
                ts.append(time.perf_counter() - t0)
        host, med = per_point * P, float(np.median(ts))
        print(f"(b) P = {P}: batch median {med:.3f} s (range {min(ts):.3f} - {max(ts):.3f}; mean {it.mean():.1f} iterations, max "
              f"{it.max()}) | host loop scaled {host:.1f} s | ratio {host / med:.1f} x | against the host loop on 16 cores "
              f"({host / 16:.2f} s): {host / 16 / med:.2f} x", flush=True)
        del args
    # (c) the front end on an 8 x 8 climate grid
    cr = cc = 8
    rng = np.random.default_rng(4)
    vegp1 = {k: (v[:, :, 6] if v.ndim == 3 else v) for k, v in vegp_r.items()}
    climarray = {}
    for k in F.WEATHER:
        base = np.broadcast_to(np.asarray(weather[k], dtype=np.float64)[None, None, :], (cr, cc, n)).copy()
        if k == "temp":
            base += rng.uniform(-1.5, 1.5, (cr, cc, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (cr, cc, 1))
        climarray[k] = base
    climarray["difrad"] = np.minimum(climarray["difrad"], climarray["swdown"])
    clat = dtm["lat"] + 1e-4 * np.arange(cr)[:, None] + 0 * np.arange(cc)[None, :]
    clon = dtm["long"] + 1e-4 * np.arange(cc)[None, :] + 0 * np.arange(cr)[:, None]
    run = lambda dev: F.runpointmodela(climarray, obst, 0.05, dtm, vegp1, soilc, lats=clat, lons=clon, device=dev)   # noqa: E731
    run(0)
    td = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = run(0)
        td.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = run(None)
    th = time.perf_counter() - t0
    worst = max(float(np.max(np.abs(g["dfo"][k] - w["dfo"][k]) / (1 + np.abs(w["dfo"][k])))) for g, w in zip(got, want)
                for k in w["dfo"])
    print(f"(c) runpointmodela 8 x 8, n = {n}: device=0 median {np.median(td):.3f} s (range {min(td):.3f} - {max(td):.3f}; soilmCpp, "
          f"spline and packing on the host included) | host loop {th:.2f} s | ratio {th / np.median(td):.1f} x | max scaled "
          f"|device - host| over dfo {worst:.2e}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main([int(x) for x in sys.argv[1:]] or [64, 1024, 4096]))
