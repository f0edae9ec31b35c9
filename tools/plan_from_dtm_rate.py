"""From a dtm to a plan that is ready to run, host route against device route, on one device: vector forcing, one process, one
warm-up and five repeats of each, every one timed to a finished sync().
  host route    terrain.precompute_terrain + the NA masking of frontend.prepare_grid_inputs + terrain.topidx (host sweep) + Plan
  device route  Plan(dtm=...): the planes derived on the device into the plan's own buffers (include/mcf.h mcf_plan_create_dtm)
Prints median and range of both and the number of pointer-doubling rounds of the flow accumulation (the library reports it on
stderr under MCF_TIMING); exits non-zero unless the device route's slowest repeat beats the host route's fastest.
Usage: python tools/plan_from_dtm_rate.py [n ...]        (default: 1024 4096)"""
import os
import sys
import time
from pathlib import Path

import numpy as np

os.environ.setdefault("MCF_TIMING", "1")
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from microclimf_amd import api, synthetic                                    # noqa: E402
from microclimf_amd.terrain import precompute_terrain, topidx                # noqa: E402

SIX = api.DTM_DERIVED
# Idle seconds after a plan is released, outside every timed span.  A 4096^2 plan with its one-day ring holds 57 GB; allocating
# that again right after releasing it waits 2 - 3 s for the driver to hand the memory back (measured: device-route repeats of
# 0.07 s and of 1.7 - 3.3 s alternating, the derivation itself 17 ms in all of them).  The host route never sees this, its
# three seconds of host work lie in between — the pause gives both routes the same start.
PAUSE = 4.0


def dtm_of(n):
    i = np.arange(n, dtype=np.float64)[:, None]
    j = np.arange(n, dtype=np.float64)[None, :]
    z = 100 + 40 * np.sin(2 * np.pi * i / 257) * np.cos(2 * np.pi * j / 193) + 12 * np.sin(2 * np.pi * (i + j) / 61) \
        + np.random.default_rng(3).uniform(0, 1, (n, n))
    z[n // 3:n // 3 + n // 50, n // 2:n // 2 + n // 40] = np.nan
    return np.asfortranarray(z)


def host_route(a, z, res):
    t = precompute_terrain(z, res, a["zref"])
    na = np.isnan(z)
    for k in ("slope", "aspect"):
        t[k][np.isnan(t[k])] = 0.0
        t[k][na] = np.nan
    t["twi"] = topidx(z, res)
    b = dict(a)
    b["soilc"] = {**a["soilc"], **t}
    return api.Plan(**b)


def device_route(a, z, res):
    b = dict(a)
    b["soilc"] = {k: v for k, v in a["soilc"].items() if k not in SIX}
    return api.Plan(**b, dtm={"z": z, "res": res})


def timed(fn, *args, repeats=5):
    ts = []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        with fn(*args) as p:
            p.sync()
            t1 = time.perf_counter()
            nbytes = p.device_bytes
        t2 = time.perf_counter()
        time.sleep(PAUSE)
        print(f"  {fn.__name__} repeat {r}: to sync {t1 - t0:.3f} s, plan released in {t2 - t1:.3f} s", file=sys.stderr, flush=True)
        if r:
            ts.append(t1 - t0)
    return np.array(ts), nbytes


def main(sizes):
    ok = True
    for n in sizes:
        a = synthetic.workload(n, n, 24, start_doy=170)
        z, res = dtm_of(n), 5.0
        th, bh = timed(host_route, a, z, res)
        td, bd = timed(device_route, a, z, res)
        faster = td.max() < th.min()
        ok &= faster and bh == bd
        print(f"{n}^2: host route median {np.median(th):.3f} s (range {th.min():.3f} - {th.max():.3f}) | device route median "
              f"{np.median(td):.3f} s (range {td.min():.3f} - {td.max():.3f}) | device slowest < host fastest: {faster} | plan bytes "
              f"host {bh} device {bd}", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main([int(x) for x in sys.argv[1:]] or [1024, 4096]))
