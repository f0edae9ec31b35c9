"""Array-weather runbioclim without a device: frontend.runbioclima's selection logic against a literal transcription of the
first twenty lines of `.runbioclim2` (R/internal.R:1909-1916) with `.biomicropoint`'s array branch and `.biosel`
(1749-1750, 1690-1727), and the new entries of the C ABI and its Python mirror."""
import re
from pathlib import Path

import numpy as np

from microclimf_amd import _abi, api, frontend as F, synthetic

ROOT = Path(__file__).resolve().parent.parent


def r_order(x):
    """R's order(): ascending, ties in order of appearance; 1-based"""
    return sorted(range(1, len(x) + 1), key=lambda i: (x[i - 1], i))


def r_which(cond):
    return [i + 1 for i, c in enumerate(cond) if c]


def r_circular_filter3(agg):
    """stats::filter(agg, rep(1/3, 3), sides = 2, circular = TRUE)"""
    n = len(agg)
    return [agg[(i + 1) % n] / 3 + agg[i] / 3 + agg[(i - 1) % n] / 3 for i in range(n)]


def transcription(precip, temp, mon0, year):
    """mon0: tme$mon (0-based) and year: tme$year per step.  Returns (wq, dq, hq, cq, seld, selh), all 1-based as in R."""
    nsteps = precip.shape[2]
    # prech <- apply(.is(climarray$precip), 3, mean, na.rm = TRUE); tc likewise
    prech, tc = [], []
    for k in range(nsteps):
        for src, dst in ((precip, prech), (temp, tc)):
            v = [x for x in src[:, :, k].ravel() if not np.isnan(x)]
            dst.append(sum(v) / len(v))
    months = sorted(set(mon0))

    def aggregate(x, fun):                               # stats::aggregate(x, by = list(tme$mon), fun, na.rm = TRUE)$x
        return [fun([x[k] for k in range(nsteps) if mon0[k] == m and not np.isnan(x[k])]) for m in months]
    agg = aggregate(prech, lambda v: sum(v) / len(v))
    f = r_circular_filter3(agg)
    wq, dq = f.index(max(f)) + 1, f.index(min(f)) + 1      # which.max / which.min: the first
    agg = aggregate(tc, sum)
    f = r_circular_filter3(agg)
    hq, cq = f.index(max(f)) + 1, f.index(min(f)) + 1
    # .biosel(tme, tc)
    ndays = nsteps // 24
    tcd = [sum(tc[d * 24:(d + 1) * 24]) / 24 for d in range(ndays)]
    tmd_mon = [mon0[d * 24 + 12] for d in range(ndays)]     # the mean of a day's 24 times falls on the day itself
    tmd_year = [year[d * 24 + 12] for d in range(ndays)]
    sel_med = []
    for mth in range(1, 13):
        s = r_which([m + 1 == mth for m in tmd_mon])
        o = r_order([tcd[i - 1] for i in s])
        n = len(o) // 2
        sel_med.append(s[0] - 1 + o[n - 1])
    sel_max, sel_min = [], []
    for y in dict.fromkeys(tmd_year):
        s = r_which([v == y for v in tmd_year])
        t = [tcd[i - 1] for i in s]
        sel_max.append(t.index(max(t)) + 1 + s[0] - 1)
        sel_min.append(t.index(min(t)) + 1 + s[0] - 1)
    o1, o2 = r_order([tcd[i - 1] for i in sel_max]), r_order([tcd[i - 1] for i in sel_min])
    sel_max, sel_min = [sel_max[i - 1] for i in o1], [sel_min[i - 1] for i in o2]
    n = len(sel_max) // 2 + 1
    seld = sel_med + [sel_max[n - 1], sel_min[n - 1]]
    selh = [(d - 1) * 24 + h for d in seld for h in range(1, 25)]
    return wq, dq, hq, cq, seld, selh


def test_selection_matches_the_transcription_of_runbioclim2():
    T = 8760
    obstime, _ = synthetic.calendar(T)
    _, clim, _ = synthetic.forcing_vectors(T)
    rng = np.random.default_rng(11)
    temp = clim["temp"][None, None, :] + rng.normal(0.0, 1.5, (2, 3, T))
    precip = np.maximum(0.0, rng.gamma(0.3, 2.0, (2, 3, T)) * (1.0 + 0.8 * np.cos(2 * np.pi * np.arange(T) / T))[None, None, :])
    temp[0, 1, 100:4000] = np.nan                        # na.rm = TRUE: a cell that drops out for months
    precip[1, 2, ::7] = np.nan
    got = F.bioclima_selection({"temp": temp, "precip": precip}, obstime)
    mon0 = (np.asarray(obstime["month"]).astype(int) - 1).tolist()
    wq, dq, hq, cq, seld, selh = transcription(precip, temp, mon0, np.asarray(obstime["year"]).tolist())
    assert (got["wq"], got["dq"], got["hq"], got["cq"]) == (wq, dq, hq, cq)
    assert len({wq, dq}) == 2 and len({hq, cq}) == 2
    assert got["seld"].tolist() == seld
    assert (got["selh"] + 1).tolist() == selh            # the front end's hour indices are 0-based
    assert len(seld) == 14 and len(set(seld)) >= 13


def test_new_entries_are_exported_and_the_abi_version_stays():
    header = (ROOT / "include" / "mcf.h").read_text()
    assert re.search(r"^int mcf_bioclim_last_chunks\(void\);", header, re.M)
    assert re.search(r"#define MCF_ABI_VERSION 8\b", header) and _abi.ABI_VERSION == 8
    assert "mcf_bioclim_last_chunks" in _abi.EXPORTS
    for name in ("runbioclim2Cpp_coarse", "runbioclim4Cpp_coarse", "bioclim_last_chunks"):
        assert callable(getattr(api, name)), name
    assert callable(F.runbioclima) and callable(F.bioclima_selection)
    lib = _abi.load()
    assert lib.mcf_abi_version() == 8
    assert api.bioclim_last_chunks() == 0                # no bioclim call on this thread yet
