"""Yardstick of the period summaries (include/mcf.h "period summaries"): plain numpy that follows the header's definition
literally on [rows, cols, T] arrays — a Python loop over the steps in time order, vectorised over cells.  Elementwise fp64
add, compare and divide are the device's operations, so device results are compared bit for bit, NA payload included."""
import numpy as np

NA_BITS = np.uint64(0x7FF00000000007A2)
STATS = ("mean", "min", "max", "mean_daily_max", "mean_daily_min", "hours_above")


def na_real():
    """R's NA_real_"""
    return np.array([NA_BITS], dtype=np.uint64).view(np.float64)[0]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def summarise(x, period_of_day, nperiods, threshold=float("nan")):
    """x: [rows, cols, T] values of one variable; period_of_day: one entry per whole day (-1: not counted).
    -> ({statistic: [rows, cols, nperiods]}, counted days per period)"""
    x = np.asarray(x, dtype=np.float64)
    pod = np.asarray(period_of_day).astype(np.int64)
    shape = x.shape[:2]
    P = int(nperiods)
    s = [np.zeros(shape) for _ in range(P)]
    mn, mx = [None] * P, [None] * P
    dxs = [np.zeros(shape) for _ in range(P)]
    dns = [np.zeros(shape) for _ in range(P)]
    cnt = [np.zeros(shape) for _ in range(P)]
    nan = [np.zeros(shape, dtype=bool) for _ in range(P)]
    days = np.zeros(P, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):      # (NA_real_ is a signalling NaN)
        for d, p in enumerate(pod):
            if p < 0:
                continue
            dmx = dmn = None
            for h in range(24):
                v = x[:, :, 24 * d + h]
                nan[p] |= np.isnan(v)
                s[p] = s[p] + v
                if mn[p] is None:
                    mn[p], mx[p] = v.copy(), v.copy()
                else:
                    lt, gt = v < mn[p], v > mx[p]
                    mn[p][lt] = v[lt]
                    mx[p][gt] = v[gt]
                if h == 0:
                    dmx, dmn = v.copy(), v.copy()
                else:
                    gt, lt = v > dmx, v < dmn
                    dmx[gt] = v[gt]
                    dmn[lt] = v[lt]
                cnt[p] = cnt[p] + (v > threshold)
            dxs[p] = dxs[p] + dmx
            dns[p] = dns[p] + dmn
            days[p] += 1
        out = {k: np.empty(shape + (P,), order="F") for k in STATS}
        for p in range(P):
            if days[p] == 0:
                for k in STATS:
                    out[k][:, :, p] = na_real()
                continue
            vals = {"mean": s[p] / (24.0 * days[p]), "min": mn[p], "max": mx[p], "mean_daily_max": dxs[p] / float(days[p]),
                    "mean_daily_min": dns[p] / float(days[p]), "hours_above": cnt[p]}
            for k in STATS:
                plane = np.array(vals[k], dtype=np.float64, copy=True)
                bits(plane)[nan[p]] = NA_BITS
                out[k][:, :, p] = plane
    return out, days
