"""Below ground, whole-series plan against the streamed plan on one device: a 1024 x 1024 year (vector forcing, Tz + soilm) for
complete = 0 and 1 — device bytes, wall time of the solve (+ prepare) and of the below-ground transforms, and whether the two
Tz agree bit for bit on a sample of cells.  Usage: python tools/below_stream_rate.py [n] [ring_days]"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from microclimf_amd import synthetic          # noqa: E402
from microclimf_amd.api import Plan           # noqa: E402


def main(n=1024, ring_days=16):
    T, nd = 8760, 365
    cells = np.sort(np.random.default_rng(7).choice(n * n, 512, replace=False)).astype(np.int64)
    for complete in (0, 1):
        a = synthetic.workload(n, n, T, reqhgt=-0.2, start_doy=1, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0], complete=bool(complete))
        with Plan(**a, ring_days=ring_days, stream_below=True) as p:
            p.sync()
            t0 = time.time()
            p.below_prepare()
            p.sync()
            t1 = time.time()
            got = np.empty((cells.size, T))
            t_run = 0.0
            for d0 in range(0, nd, ring_days):
                k = min(ring_days, nd - d0)
                ta = time.time()
                p.run_days(d0, k, 0)
                p.sync()
                t_run += time.time() - ta
                got[:, d0 * 24:(d0 + k) * 24] = p.fetch_cells(0, "Tz", 0, k * 24, cells)
            b_st = p.device_bytes
        with Plan(**a, ring_days=1) as w:
            w.sync()
            t2 = time.time()
            w.run_days(0, nd, 0)
            w.sync()
            t3 = time.time()
            w.belowground()
            w.sync()
            t4 = time.time()
            want = w.fetch_cells(0, "Tz", 0, T, cells)
            b_wh = w.device_bytes
        same = np.array_equal(got.view(np.uint64), want.view(np.uint64))
        cs = n * n * nd
        print(f"{n}^2 x {T} complete={complete}: whole-series {b_wh / 1e9:.1f} GB, solve {t3 - t2:.2f} s, belowground "
              f"{t4 - t3:.2f} s | streamed (ring {ring_days} d) {b_st / 1e9:.1f} GB, prepare {t1 - t0:.2f} s, chunks {t_run:.2f} s "
              f"| Tz bits equal on {cells.size} cells: {same} | {cs / 1e6:.0f} M cell-days")


if __name__ == "__main__":
    main(*[int(x) for x in sys.argv[1:]])
