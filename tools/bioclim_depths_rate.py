#!/usr/bin/env python3
"""What one streamed solve for several depths saves the soil bioclim maps: one process, one MI355X.

    python tools/bioclim_depths_rate.py [--small 1024 --large 4096 --depths 1 4 --repeat 5 --out profiles/bioclim_depths_rate.txt]
    python tools/bioclim_depths_rate.py --rehearse          # no device: arguments, shapes and byte counts only

Vector forcing, 336 steps (the fourteen days of the real call), all nineteen variables, on a synthetic `small`^2 raster:
  (a) D separate runbioclim1Cpp(reqhgt = depth) calls — the whole-series route, one solve per depth — for each D of --depths;
  (b) the one runbioclim_depths call at the same depths,
each after one warm-up, the median of `repeat` calls timed between two HIP events on the null stream (the calls are synchronous
and include the plan's set-up and the uploads), with the peak device memory of the timed calls: the smallest free figure
hipMemGetInfo gives while they run, polled from a second thread, against the figure before (the plans of the one-call entries
are not reachable from outside, so mcf_plan_bytes cannot be asked).  The matrices of (a) and (b) must agree bit for bit.  At
`large`^2 (b) alone, and (a) only where its whole series (3 x 8 B x cells x steps) fits half the free memory.  The byte
counts are from the shapes: per cell-day the accumulate kernels read D + 1 slabs of 192 B.  The accumulate kernels' own device
time is not separated here (the one call does not expose its plan): their rate is "not measured".  There is no pass threshold:
the file is where the measured values go.
"""
import argparse
import platform
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np                                   # noqa: E402

from microclimf_amd import api, synthetic            # noqa: E402

T = 336
ALL_DEPTHS = (-0.02, -0.05, -0.1, -0.2, -0.4, -0.6, -0.8, -1.0)


def quarters():
    days = ((2, 3, 4), (7, 8, 9), (5, 6, 7, 12), (0, 1, 11, 13))
    return [np.concatenate([np.arange(24 * d, 24 * d + 24) for d in ds]) for ds in days]


def workload(n):
    a = synthetic.workload(n, n, T, reqhgt=-0.05, variety=True, na_frac=0.02, start_doy=150)
    for k in ("complete", "out", "reqhgt"):
        a.pop(k)
    q = quarters()
    return dict(a, out=[1] * 19, wetq=q[0], dryq=q[1], hotq=q[2], colq=q[3], air=True)


def shapes(n, D):
    """byte counts of one configuration, from the shapes alone"""
    cells, days = n * n, T // 24
    return dict(cells=cells, cell_steps=cells * T,
                whole_series_bytes=3 * 8 * cells * T,                      # tgser and the linear ring of Tz and soilm
                acc_read_bytes=(D + 1) * 192 * cells * days,               # every slab of every day, once
                state_bytes=(21 * D + 8) * 8 * cells,
                matrices_bytes=(11 * D + 8) * 8 * cells)


def describe(n, D):
    s = shapes(n, D)
    return (f"   shapes D = {D}: {s['cell_steps']:.3e} cell-steps; whole-series arrays of (a) {s['whole_series_bytes'] / 1e9:.2f} GB per call; "
            f"accumulate reads {s['acc_read_bytes'] / 1e9:.2f} GB, state {s['state_bytes'] / 1e9:.3f} GB, matrices {s['matrices_bytes'] / 1e9:.3f} GB")


def median_of(hip, fn, repeat):
    fn()                                                                   # warm-up
    res, ms, peak = None, [], 0
    for _ in range(repeat):
        res, m, p = hip.timed(fn)
        ms.append(m)
        peak = max(peak, p)
    return res, statistics.median(ms), min(ms), max(ms), peak


def same_bits(one, singles):
    ok = True
    for k, v in one.items():
        if k == "depths":
            continue
        for d, s in enumerate(singles):
            g = v[d] if v.ndim == 3 else v
            ok &= np.array_equal(np.isnan(g), np.isnan(s[k])) and np.array_equal(g[np.isfinite(g)].view(np.uint64),
                                                                                 s[k][np.isfinite(s[k])].view(np.uint64))
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=1024)
    ap.add_argument("--large", type=int, default=4096, help="0: skip the large raster")
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--rehearse", action="store_true", help="no device: arguments, shapes and byte counts only")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "bioclim_depths_rate.txt"))
    o = ap.parse_args()
    if any(D < 1 or D > len(ALL_DEPTHS) for D in o.depths) or o.repeat < 1 or o.small < 1:
        ap.error(f"--depths within 1 .. {len(ALL_DEPTHS)}, --repeat and --small at least 1")
    if o.rehearse:
        kw = workload(8)
        assert len(kw["wetq"]) == 72 and len(kw["hotq"]) == 96 and all((np.diff(kw[q]) > 0).all() for q in ("wetq", "dryq", "hotq", "colq"))
        for n in [o.small] + ([o.large] if o.large else []):
            print(f"-- {n} x {n}")
            for D in o.depths:
                print(describe(n, D))
        s = shapes(1024, 4)
        assert s["acc_read_bytes"] == 5 * 192 * 1024 * 1024 * 14 and s["whole_series_bytes"] == 24 * 1024 * 1024 * 336
        print("rehearsal ok")
        return
    from bioclim_array_rate import Hip, device_name
    hip = Hip()
    lines = [f"soil bioclim at several depths on {device_name()} (host {platform.node()}): vector forcing, {T} steps, all nineteen "
             f"variables, 1 warm-up + median of {o.repeat} timed calls (min .. max), the calls' set-up and uploads included"]
    all_same = True
    for n, large in [(o.small, False)] + ([(o.large, True)] if o.large else []):
        kw = workload(n)
        lines.append(f"-- {n} x {n}")
        for D in o.depths:
            depths = ALL_DEPTHS[:D] if D > 1 else (-0.05,)
            lines.append(describe(n, D))
            fits = shapes(n, D)["whole_series_bytes"] < 0.5 * hip.free_bytes()
            singles = None
            if not large or fits:
                singles, a_ms, a_lo, a_hi, a_peak = median_of(hip, lambda: [api.runbioclim1Cpp(**kw, reqhgt=d) for d in depths], o.repeat)
                lines.append(f"   (a) {D} x runbioclim1Cpp : {a_ms:10.1f} ms ({a_lo:.1f} .. {a_hi:.1f})  peak device memory {a_peak / 1e9:7.2f} GB")
            else:
                lines.append(f"   (a) {D} x runbioclim1Cpp : not run (its whole-series arrays do not fit half the free memory)")
            one, b_ms, b_lo, b_hi, b_peak = median_of(hip, lambda: api.runbioclim_depths(**kw, depths=depths), o.repeat)
            chunks = api.bioclim_last_chunks()
            lines.append(f"   (b) runbioclim_depths   : {b_ms:10.1f} ms ({b_lo:.1f} .. {b_hi:.1f})  peak device memory {b_peak / 1e9:7.2f} GB  "
                         f"chunks {chunks}")
            if singles is not None:
                same = same_bits(one, singles)
                all_same &= same
                lines.append(f"   ratio (b) / (a): time {b_ms / a_ms:.3f}, memory {b_peak / max(a_peak, 1):.3f}; same bits: {same}")
            del one, singles
    lines.append("accumulate kernels' own device time and bytes/s: not measured (the one call does not expose its plan)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    Path(o.out).write_text(text)
    if not all_same:
        raise SystemExit("the one call and the single-depth calls differ")


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    main()
