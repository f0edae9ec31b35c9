"""Soil bioclim variables at several depths from one streamed below-ground solve (mcf_runbioclim_depths,
api.runbioclim_depths): every matrix against the whole-series route of one depth per call (runbioclim1Cpp / 3Cpp /
2Cpp_coarse with reqhgt = depth, unchanged by this work) bit for bit, and against the oracle under derived bars.

CPU measurements of the oracle case (11 x 7 cells, T = 336, depths -0.02, -0.05, -0.2, -1.0): the largest rounding noise N
over the three noise variants is 4.0e-12 (bio3 at -0.05 m, where bio7 is near zero for some cells), a bar of 6.4e-11; every
other (depth, variable) pair has N <= 7e-13; the NaN / inf patterns of all variants agree."""
import ctypes as C

import numpy as np
import pytest

from microclimf_amd import api, synthetic
from microclimf_amd.api import runbioclim1Cpp, runbioclim2Cpp_coarse, runbioclim3Cpp, runbioclim_depths
import parity_bars

pytestmark = pytest.mark.gpu
DEPTHS = (-0.02, -0.05, -0.2, -1.0, -0.05)      # the hourly window, a mix, the daily path, the series mean; one repeated
OUT = [1] * 19
TEMP = [f"bio{i}" for i in range(1, 12)]
MOIST = [f"bio{i}" for i in range(12, 20)]
T_LONG = 336 + 4 * 72

_cache = {}


def quarters(T):
    """T = 336: inside the series, ascending, as the front end builds them (`_getselq`: every modelled hour of the quarter's
    three months, so the hottest or the coldest day may be among them); T = 624: tests/test_bioclim_gpu.py's quarters(), the
    days past day 14"""
    if T == 336:
        days = ((2, 3, 4), (7, 8, 9), (5, 6, 7, 12), (0, 1, 11, 13))
        return [np.concatenate([np.arange(24 * d, 24 * d + 24) for d in ds]) for ds in days]
    return [np.arange(336 + 72 * i, 336 + 72 * (i + 1)) for i in range(4)]


def qkw(T):
    wq, dq, hq, cq = quarters(T)
    return dict(out=OUT, wetq=wq, dryq=dq, hotq=hq, colq=cq, air=True)


def vector_case(T, layered):
    """(arguments without reqhgt, the single-depth references), made once"""
    key = ("vector", T, layered)
    if key not in _cache:
        a = synthetic.workload(29, 13, T, reqhgt=-0.05, variety=True, start_doy=150, na_frac=0.06)
        a["vegp"]["hgt"][3, 2] = np.nan
        if layered:
            a = synthetic.layered(a, 14)
            a.pop("dfsel")
        for k in ("complete", "out", "reqhgt"):
            a.pop(k)
        fn = runbioclim3Cpp if layered else runbioclim1Cpp
        refs = [fn(**a, reqhgt=d, **qkw(T)) for d in DEPTHS]
        assert api.bioclim_last_chunks() == 0                     # the whole-series route
        _cache[key] = (a, refs)
    return _cache[key]


def coarse_case():
    """shape A of tests/bioclim_coarse_cases.py (37 x 9 under a 2 x 3 climate grid, T = 624), below ground"""
    if "coarse" not in _cache:
        a, rp, cp = synthetic.coarse_workload(37, 9, T_LONG, 2, 3, reqhgt=-0.05, variety=True, na_frac=0.06, start_doy=150)
        a["vegp"]["hgt"][33, 4] = np.nan
        for k in ("complete", "out", "reqhgt"):
            a.pop(k)
        a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
        refs = [runbioclim2Cpp_coarse(**a, reqhgt=d, rowpos=rp, colpos=cp, **qkw(T_LONG)) for d in DEPTHS]
        assert api.bioclim_last_chunks() == 0
        _cache["coarse"] = (a, rp, cp, refs)
    return _cache["coarse"]


def same_bits(got, ref, what):
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.array_equal(got[fin].view(np.uint64), ref[fin].view(np.uint64)), what


def assert_matches_single_depth_runs(got, refs, what):
    assert list(got) == ["depths"] + TEMP + MOIST
    assert np.array_equal(got["depths"], np.asarray(DEPTHS))
    # the shared-moisture claim on the parent's own outputs first: no depth changes bio12 .. bio19
    for k in MOIST:
        for d in range(1, len(DEPTHS)):
            same_bits(refs[d][k], refs[0][k], (what, "references", k, d))
        same_bits(got[k], refs[0][k], (what, k))
    for k in TEMP:
        assert got[k].shape == (len(DEPTHS),) + refs[0][k].shape
        for d in range(len(DEPTHS)):
            same_bits(got[k][d], refs[d][k], (what, k, DEPTHS[d]))


@pytest.mark.parametrize("cpb", [16, 21, 42])
@pytest.mark.parametrize("chunk_days", [1, 5, 0])
@pytest.mark.parametrize("T", [336, T_LONG])
def test_bits_against_the_whole_series_route_of_each_depth(T, chunk_days, cpb):
    """29 x 13 = 377 cells (more than one workgroup at every tile size, a partial last tile, NA cells); chunks of one day, of
    five days (days 10 .. 14 share a launch: the monthly, hottest and coldest branches, and the quarters are cut) and sized
    from memory"""
    a, refs = vector_case(T, False)
    valid = np.isfinite(refs[0]["bio1"])
    assert 0 < (~valid).sum() < 0.2 * valid.size and not valid[3, 2]
    # the depths span the regimes of Tbelowgroundv: a daily range at -0.02 m, none at all at -1 m (bio3 = 0 / 0 there)
    assert (refs[0]["bio7"][valid] > 0.5).all() and (refs[3]["bio7"][valid] == 0.0).all() and np.isnan(refs[3]["bio3"]).all()
    got = runbioclim_depths(**a, depths=DEPTHS, **qkw(T), chunk_days=chunk_days, cells_per_block=cpb)
    if chunk_days:
        assert api.bioclim_last_chunks() == -(-(T // 24) // chunk_days)
    else:
        assert api.bioclim_last_chunks() >= 1
    assert_matches_single_depth_runs(got, refs, (T, chunk_days, cpb))


@pytest.mark.parametrize("T", [336, T_LONG])
def test_bits_with_layered_vegetation(T):
    """the fourteen one-day layers of runbioclim3Cpp; T = 624: the quarter days lie past the last layer, NA as in the
    whole-series route"""
    a, refs = vector_case(T, True)
    for chunk_days in (1, 5, 0):
        got = runbioclim_depths(**a, depths=DEPTHS, **qkw(T), layered=True, chunk_days=chunk_days)
        assert_matches_single_depth_runs(got, refs, ("layered", T, chunk_days))
    if T == 336:
        assert np.isfinite(got["bio1"]).any() and np.isfinite(got["bio12"]).any()


def test_bits_with_coarse_forcing():
    a, rp, cp, refs = coarse_case()
    assert np.isfinite(refs[0]["bio1"]).sum() > 0.8 * refs[0]["bio1"].size
    for chunk_days in (1, 5, 0):
        b = {k: v for k, v in a.items() if k not in ("lats", "lons")}
        got = runbioclim_depths(**b, lat=a["lats"], lon=a["lons"], depths=DEPTHS, **qkw(T_LONG),
                                coarse={"rowpos": rp, "colpos": cp}, chunk_days=chunk_days)
        assert_matches_single_depth_runs(got, refs, ("coarse", chunk_days))


def orc_bioclim_cells(lib, tz, sm, qs):
    """runbioclimCpp's reductions (the oracle's orc_bioclim_cell) of every cell of [rows, cols, T] series -> [19, rows, cols];
    oracle.run_bioclim takes no `lib`, hence this helper"""
    from oracle import oracle as O
    R, Cc, T = tz.shape
    bio = np.full((19, R, Cc), O.load().orc_na_real())
    tmp = np.zeros(19)
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    lib.orc_bioclim_cell.restype = None
    for i in range(R):
        for j in range(Cc):
            if np.isnan(tz[i, j, 0]):
                continue
            x = np.ascontiguousarray(tz[i, j, :])
            y = np.ascontiguousarray(sm[i, j, :])
            lib.orc_bioclim_cell(x.ctypes.data_as(DP), y.ctypes.data_as(DP), C.c_int(T),
                                 qs[0].ctypes.data_as(IP), C.c_int(len(qs[0])), qs[1].ctypes.data_as(IP), C.c_int(len(qs[1])),
                                 qs[2].ctypes.data_as(IP), C.c_int(len(qs[2])), qs[3].ctypes.data_as(IP), C.c_int(len(qs[3])),
                                 tmp.ctypes.data_as(DP))
            bio[:, i, j] = tmp
    return bio


def test_against_the_oracle_under_derived_bars(oracle):
    """11 x 7 cells, T = 336, four depths: `want` and the bars from parity_bars.bars_for (K, FLOOR, CAP its own); no variable
    and no cell is left out"""
    from oracle import oracle as O
    O.load().orc_na_real.restype = C.c_double
    depths = DEPTHS[:4]
    a = synthetic.workload(11, 7, 336, reqhgt=-0.05, variety=True, start_doy=120)
    a["vegp"]["hgt"][0, 0] = np.nan
    for k in ("complete", "out", "reqhgt"):
        a.pop(k)
    qs = [np.ascontiguousarray(np.asarray(q, dtype=np.int32)) for q in quarters(336)]

    def run(lib):
        lib = lib or O.load()
        res = {}
        moist = None
        for d in depths:
            r = O.run_grid(**a, reqhgt=d, complete=True, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0], lib=lib)
            bio = orc_bioclim_cells(lib, r["Tz"], r["soilm"], qs)
            for v in range(11):
                res[f"bio{v + 1}@{d:g}"] = bio[v]
            if moist is None:
                moist = bio[11:]
        for v in range(8):
            res[f"bio{v + 12}"] = moist[v]
        return res

    want, bars, noise = parity_bars.bars_for(O, run, key="bioclim_depths")
    got = runbioclim_depths(**a, depths=depths, **qkw(336))
    flat = {}
    for i, d in enumerate(depths):
        for v in range(11):
            flat[f"bio{v + 1}@{d:g}"] = got[f"bio{v + 1}"][i]
    for v in range(8):
        flat[f"bio{v + 12}"] = got[f"bio{v + 12}"]
    assert list(flat) == list(want) and len(want) == 11 * len(depths) + 8
    print("largest N", max(noise.values()), max(noise, key=noise.get))
    worst = parity_bars.compare(flat, want, bars)
    print(" ".join(f"{k}={v:.1e}/{bars[k]:.1e}" for k, v in worst.items()))
    assert np.isnan(flat["bio1@-0.02"][0, 0]) and np.isfinite(flat["bio1@-0.02"]).sum() > 0.8 * 77


def test_last_chunks_counts_sweep_two_and_stays_zero_for_the_whole_series_route():
    a, refs = vector_case(336, False)
    runbioclim_depths(**a, depths=DEPTHS[:2], **qkw(336), chunk_days=1)
    assert api.bioclim_last_chunks() == 14
    runbioclim1Cpp(**a, reqhgt=-0.05, **qkw(336))
    assert api.bioclim_last_chunks() == 0
