"""Workloads of the array-weather staged-model tests (tests/test_stages_array_cpu.py, tests/test_stages_array_gpu.py): the
smallest shapes that still break things, as tests/stages_cases.py argues.

Fine arrays, 5 x 10 cells x 96 h with stages_cases' seeds (the same rasters: the NA cell and the bare cells named there), at day
170 and 355, reqhgt 0.05 and 0: array plans take 32-cell tiles, so one full tile and a partial one of 18; four days, so the three
day buffers wrap.  One layered case (two layers of two days).
Coarse arrays: 5 x 10 under a 2 x 3 grid (fewer than 32 rows: per-lane taps), the same with altcorrect 1 and 2 over a few hundred
metres of relief and an NA in dtmc, and 40 x 3 x 48 h under a 3 x 2 grid (rows >= 32, row positions that do not decrease: the taps
staged in LDS; tiles that wrap from one raster column into the next; 120 cells = three full tiles and a partial one of 24).
A coarse case's expectation is the yardstick on oracle/coarse_oracle.py's expansion of the same arrays."""
import numpy as np

from microclimf_amd import synthetic
from oracle import coarse_oracle as CO

ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact",
        "complete", "mat", "out")
_FINE = {
    "a170_h005": dict(seed=16, start_doy=170, reqhgt=0.05),
    "a355_h005": dict(seed=33, start_doy=355, reqhgt=0.05),
    "a170_h0": dict(seed=16, start_doy=170, reqhgt=0.0),
    "a355_h0": dict(seed=33, start_doy=355, reqhgt=0.0),
    "alayered": dict(seed=16, start_doy=170, reqhgt=0.05, layers=2),
}
_COARSE = {                 # rows, cols, tsteps, coarse rows, coarse cols, keywords
    "c_lane": (5, 10, 96, 2, 3, dict(seed=16, start_doy=170, reqhgt=0.05)),
    "c_lane_h0": (5, 10, 96, 2, 3, dict(seed=16, start_doy=170, reqhgt=0.0)),
    "c_lds": (40, 3, 48, 3, 2, dict(seed=33, start_doy=170, reqhgt=0.05)),
    "c_alt1": (5, 10, 48, 2, 3, dict(seed=16, start_doy=355, reqhgt=0.05, altcorrect=1)),
    "c_alt2": (5, 10, 48, 2, 3, dict(seed=33, start_doy=170, reqhgt=0.05, altcorrect=2)),
}
FINE, COARSE = tuple(_FINE), tuple(_COARSE)
CASES = FINE + COARSE
_built = {}


class Case:
    """a:       the argument dict of runmicro2Cpp (fine; runmicro4Cpp with `dfsel`) or runmicro2Cpp_coarse (coarse)
    coarse:  None, or the Plan's `coarse` dict = runmicro2Cpp_coarse's rowpos / colpos / altcorrect / dtmc / dtm
    full:    the array-forcing arguments the yardstick and the oracle take: `a` itself, or the expansion of the coarse arrays
    Built once, not to be modified."""

    def __init__(self, a, coarse, full):
        self.a, self.coarse, self.full = a, coarse, full
        self.rows, self.cols = np.shape(a["vegp"]["hgt"])[:2]
        self.tsteps = len(a["obstime"]["year"])
        self.ndays = self.tsteps // 24


def build(name) -> Case:
    if name in _built:
        return _built[name]
    if name in _FINE:
        kw = dict(_FINE[name])
        layers = kw.pop("layers", 0)
        a = synthetic.workload(5, 10, 96, variety=True, na_frac=0.04, array_forcing=True, **kw)
        if layers:
            a = synthetic.layered(a, layers)
        case = Case(a, None, a)
    else:
        rows, cols, T, cr, cc, kw = _COARSE[name]
        kw = dict(kw)
        alt = kw.pop("altcorrect", 0)
        a, rp, cp = synthetic.coarse_workload(rows, cols, T, cr, cc, variety=True, na_frac=0.04, **kw)
        coarse = {"rowpos": rp, "colpos": cp}
        z = zc = None
        if alt:
            _, _, z = synthetic.rasters(rows, cols)
            z = np.asfortranarray(300.0 + 8.0 * (z - np.nanmean(z)))        # a few hundred metres of relief
            zc = 350.0 + 200.0 * np.random.default_rng(3).random((cr, cc))
            zc[0, 0] = np.nan                                               # dtmc[is.na(dtmc)] <- 0
            coarse.update(altcorrect=alt, dtmc=zc, dtm=z)
        clim, pm = CO.expand(a["climdata"], a["pointm"], rp, cp, alt, zc, z)
        case = Case(a, coarse, dict(a, climdata=clim, pointm=pm))
    _built[name] = case
    return case
