"""Yardstick of the series sink (include/mcf.h "series sink"): plain numpy that follows the header's definition literally on
[rows, cols, T] arrays — a Python loop over zones and steps.  The mean is an integer sum of rint(v * 2^24), so it has one value
whatever the order of the cells: device results are compared bit for bit, NA payload included."""
import numpy as np

from summary_ref import NA_BITS, bits, na_real

ZSTATS = ("mean", "min", "max", "count")
LIMIT = 4096.0
QUANTUM = 2.0 ** -24


def point_series(x, cells):
    """x: [rows, cols, T]; cells: 0-based row + rows * col -> [T, npoints], column-major, the array's own bits"""
    x = np.asarray(x, dtype=np.float64)
    rows = x.shape[0]
    out = np.empty((x.shape[2], len(cells)), order="F")
    for i, c in enumerate(cells):
        out[:, i].view(np.uint64)[:] = bits(x[int(c) % rows, int(c) // rows, :])
    return out


def zone_series(x, zone, nzones, steps_done=None):
    """x: [rows, cols, T] values of one variable; zone: [rows, cols] labels (-1: in no zone); steps_done: [T] bool, the steps
    that were folded (None: all) -> {statistic: [T, nzones]}, column-major"""
    x = np.asarray(x, dtype=np.float64)
    zone = np.asarray(zone)
    T = x.shape[2]
    out = {k: np.empty((T, nzones), order="F") for k in ZSTATS}
    for k in ZSTATS:
        out[k].view(np.uint64)[...] = NA_BITS
    with np.errstate(invalid="ignore"):      # (NA_real_ is a signalling NaN)
        for z in range(nzones):
            vals = x[zone == z]              # [cells of the zone, T]
            for k in range(T):
                if steps_done is not None and not steps_done[k]:
                    continue
                v = vals[:, k]
                v = v[~np.isnan(v)]                              # na.rm = TRUE
                bad = ~(np.abs(v) < LIMIT)
                v = v[~bad]
                n = v.size
                out["count"][k, z] = float(n)
                if bad.any() or n == 0:
                    continue
                S = np.rint(v * 2 ** 24).astype(np.int64).sum(dtype=np.int64)
                out["mean"][k, z] = np.int64(S).astype(np.float64) * 2 ** -24 / n
                out["min"][k, z] = v.min() + 0.0
                out["max"][k, z] = v.max() + 0.0
    return out


__all__ = ["NA_BITS", "bits", "na_real", "ZSTATS", "LIMIT", "QUANTUM", "point_series", "zone_series"]
