"""2048 x 2048 x 8760 below ground on one device through the streamed plan (tests/test_below_stream_gpu.py runs it in a
child process under a time limit): a seeded sample of 256 valid cells, fetched chunk by chunk with fetch_cells, against the
oracle run on those cells with the raster's twi mean.  Prints timings and "scale ok"."""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from microclimf_amd import synthetic                     # noqa: E402
from microclimf_amd.api import Plan                      # noqa: E402
from oracle import oracle                                # noqa: E402


def main(complete: int, n: int = 2048, ring_days: int = 16, nsample: int = 256):
    T = 8760
    a = synthetic.workload(n, n, T, reqhgt=-0.2, start_doy=1, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0], complete=bool(complete))
    N = n * n
    valid = np.flatnonzero(~np.isnan(a["vegp"]["hgt"].reshape(N, order="F")))
    cells = np.sort(np.random.default_rng(20261016).choice(valid, nsample, replace=False)).astype(np.int64)
    t0 = time.time()
    got = {"Tz": np.empty((nsample, T)), "soilm": np.empty((nsample, T))}
    with Plan(**a, ring_days=ring_days, stream_below=True) as p:
        t1 = time.time()
        p.below_prepare()
        p.sync()
        t2 = time.time()
        nd = T // 24
        for d0 in range(0, nd, ring_days):
            k = min(ring_days, nd - d0)
            p.run_days(d0, k, 0)
            for v in ("Tz", "soilm"):
                got[v][:, d0 * 24:(d0 + k) * 24] = p.fetch_cells(0, v, 0, k * 24, cells)
        p.sync()
        t3 = time.time()
        gb = p.device_bytes / 1e9
    print(f"{n}x{n}x{T} complete={complete}: plan {gb:.1f} GB, create {t1 - t0:.1f} s, prepare {t2 - t1:.1f} s, "
          f"chunks {t3 - t2:.1f} s")

    def take(m):
        m = np.asarray(m)
        flat = m.reshape((N,) + m.shape[2:], order="F")[cells]
        return np.asfortranarray(flat.reshape((nsample, 1) + m.shape[2:]))
    sub = dict(a)
    sub["vegp"] = {k: take(v) for k, v in a["vegp"].items()}
    sub["soilc"] = {k: take(v) for k, v in a["soilc"].items()}
    lib = oracle.load()
    lib.orc_set_twi_mean_override.argtypes = [C.c_double, C.c_int]
    tw = a["soilc"]["twi"]
    lib.orc_set_twi_mean_override(float(np.mean(np.log(tw[~np.isnan(tw)]) / a["tfact"])), 1)
    try:
        want = oracle.run_grid(**sub)
    finally:
        lib.orc_set_twi_mean_override(0.0, 0)
    worst = 0.0
    for v in ("Tz", "soilm"):
        w = want[v].reshape(nsample, T)
        g = got[v]
        assert np.array_equal(np.isnan(g), np.isnan(w)), v
        ok = ~np.isnan(w)
        worst = max(worst, float(np.max(np.abs(g[ok] - w[ok]) / (1.0 + np.abs(w[ok])))))
    print(f"max scaled |streamed - oracle| over {nsample} cells x {T} steps = {worst:.3e}")
    assert worst < 1e-6, worst
    print("scale ok")


if __name__ == "__main__":
    main(int(sys.argv[1]))
