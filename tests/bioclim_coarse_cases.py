"""TEST INFRASTRUCTURE — the workloads of tests/test_bioclim_coarse_gpu.py (array-weather runbioclim on coarse arrays) and the
reference side of its comparisons, all of it from the oracle alone.

Two shapes, T = 336 + 4 x 72 = 624 steps (twelve monthly days, the hottest, the coldest, four quarters of three days):

    A  37 x 9 under a 2 x 3 climate grid: rows >= 32 — the LDS-staged taps, tiles that wrap a raster column, 11 tiles, more
       than one 64-lane workgroup in the sink kernels
    B  11 x 7 under a 3 x 2 grid: rows < 32 — the per-lane taps

The bar of a variable against the oracle is min(CAP, max(1e-9, K * N)): K and CAP are parity_bars', 1e-9 is what every
bioclim-against-oracle comparison asserts, and N is the oracle's own sensitivity to the rounding of the interpolation —
parity_bars.distance between oracle.run_bioclim on the expanded arrays and on the same arrays with a seeded half of their
elements moved one ulp (np.nextafter, up or down by a seeded coin).  Elements that are exactly zero stay: the interpolation
of zeros (radiation at night) is exact, there is no rounding to stand in for.  N comes from the CPU and is kept per case.
"""
import os

import numpy as np

from microclimf_amd import synthetic
from microclimf_amd.api import BIOCLIM_DFSEL
from oracle import coarse_oracle as CO
import parity_bars

T = 336 + 4 * 72
SHAPES = {"A": (37, 9, 2, 3), "B": (11, 7, 3, 2)}
NA_CELL = {"A": (33, 4), "B": (4, 2)}
OUT = [1] * 19
FLOOR = 1e-9

_built, _want, _noise = {}, {}, {}
margins = []          # (case, variable, N, bar, measured distance) of every comparison against the oracle this session


def quarters():
    return [np.arange(336 + 72 * i, 336 + 72 * (i + 1)) for i in range(4)]


def build(shape, layered=False):
    """(args for runbioclim2Cpp_coarse / 4Cpp_coarse without the quarters, rowpos, colpos); not to be modified"""
    key = (shape, layered)
    if key not in _built:
        rows, cols, cr, cc = SHAPES[shape]
        a, rp, cp = synthetic.coarse_workload(rows, cols, T, cr, cc, reqhgt=0.05, variety=True, na_frac=0.06, start_doy=150)
        a["vegp"]["hgt"][NA_CELL[shape]] = np.nan
        if layered:
            a = synthetic.layered(a, 14)
            a.pop("dfsel")
        for k in ("complete", "out"):
            a.pop(k)
        a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
        _built[key] = (a, rp, cp)
    return _built[key]


def elevations(shape):
    """(dtmc, dtm) of the altitude correction: a few hundred metres of relief, one coarse elevation missing"""
    rows, cols, cr, cc = SHAPES[shape]
    _, _, z = synthetic.rasters(rows, cols)
    z = 300.0 + 8.0 * (z - np.nanmean(z))
    zc = 350.0 + 200.0 * np.random.default_rng(3).random((cr, cc))
    zc[0, 0] = np.nan                                       # dtmc[is.na(dtmc)] <- 0
    return zc, np.asfortranarray(z)


def expanded(shape, layered=False, altcorrect=0):
    """the oracle's arguments: the coarse arrays expanded to the raster as `.runbioclim2` does before runbioclim2Cpp"""
    a, rp, cp = build(shape, layered)
    zc, z = elevations(shape) if altcorrect else (None, None)
    clim, pm = CO.expand(a["climdata"], a["pointm"], rp, cp, altcorrect, zc, z)
    b = dict(a, climdata=clim, pointm=pm)
    b["lat"], b["lon"] = b.pop("lats"), b.pop("lons")
    return b


def _run(O, b, air, layered):
    wq, dq, hq, cq = quarters()
    return O.run_bioclim(**b, out=OUT, wetq=wq, dryq=dq, hotq=hq, colq=cq, air=air, array_forcing=True,
                         dfsel=BIOCLIM_DFSEL if layered else None)


def want(O, shape, air, layered=False, altcorrect=0):
    key = (shape, air, layered, altcorrect)
    if key not in _want:
        _want[key] = _run(O, expanded(shape, layered, altcorrect), air, layered)
    return _want[key]


def nudged(b, seed):
    """the expanded arrays with a seeded half of their non-zero elements moved one ulp"""
    rng = np.random.default_rng(seed)

    def move(v):
        v = np.asarray(v, dtype=np.float64)
        pick = (rng.random(v.shape) < 0.5) & (v != 0.0)
        to = np.where(rng.random(v.shape) < 0.5, np.inf, -np.inf)
        return np.asfortranarray(np.where(pick, np.nextafter(v, to), v))
    return dict(b, climdata={k: move(v) for k, v in b["climdata"].items()}, pointm={k: move(v) for k, v in b["pointm"].items()})


def bars(O, shape, air, altcorrect=0):
    """(bar, N) per variable of the plain (non-layered) case"""
    key = (shape, air, altcorrect)
    if key not in _noise:
        w = want(O, shape, air, False, altcorrect)
        other = _run(O, nudged(expanded(shape, False, altcorrect), 20260 + altcorrect), air, False)
        noise = {}
        for k in w:
            assert parity_bars.same_pattern(other[k], w[k]), k
            noise[k] = parity_bars.distance(other[k], w[k])
        _noise[key] = ({k: min(parity_bars.CAP, max(FLOOR, parity_bars.K * n)) for k, n in noise.items()}, noise)
    return _noise[key]


def record(case, got, w, bar, noise):
    for k in w:
        margins.append((case, k, noise[k], bar[k], parity_bars.distance(got[k], w[k])))
    path = os.environ.get("MCF_BIOCLIM_MARGINS")
    if path:
        with open(path, "w") as f:
            f.write("# array-weather runbioclim on coarse arrays against expand-then-oracle (tests/test_bioclim_coarse_gpu.py)\n"
                    "# N: the oracle's distance under one-ulp moves of half its inputs; bar = min(1e-6, max(1e-9, 16 N));\n"
                    "# d: the device's distance from the oracle, max |x - y| / (1 + |y|)\n"
                    "# case variable N bar d d/bar\n")
            for c, k, n, b, d in margins:
                f.write(f"{c} {k} {n:.3e} {b:.3e} {d:.3e} {d / b:.3f}\n")
