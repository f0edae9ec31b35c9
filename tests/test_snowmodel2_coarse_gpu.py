"""The slow snow method for array weather as one device-resident call with the coarse arrays left coarse
(mcf_snowmodel2_coarse, mcf_snow_expand_coarse_device; `runsnowmodela(..., method="slow", device_loop=True)`): the chunk
kernel alone against the host's resampling and against the day kernel of mcf_snowmodelq2, the call against the existing chunk
loop fed the kernel's output (bytes), against the oracle's restatement of `.snowmodel2` on real coarse grids, against the host
loop through the front end, and what the call returns when asked for less, asked twice, or asked after a refusal."""
import functools

import numpy as np
import pytest

from microclimf_amd import _abi, api
from microclimf_amd import frontend as F
from microclimf_amd import snow as S
import parity_bars
from snowfast_cases import q2_case

pytestmark = pytest.mark.gpu

SHAPES = [(7, 9), (23, 37), (1, 50)]      # 23 x 37 = 851 cells: several workgroups, the last one partial; 1 x 50: less than a wave
GRIDS = [(1, 1), (1, 2), (3, 1), (2, 3), (5, 4)]     # single coarse rows / columns: r1 / c1 fall back onto r0 / c0
NAMES = ("Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden", "umu")
FIVE = NAMES[:5]


# ---- the chunk kernel alone -----------------------------------------------------------------------------------------
def _coarse_fields(shape, grid, T, seed):
    """random coarse weather and point-model arrays over `grid`, a dtm with one hole over `shape`"""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: np.asfortranarray(rng.uniform(lo, hi, grid + (T,)))                 # noqa: E731
    clim_c = {"temp": u(-12.0, 6.0), "relhum": u(55.0, 100.0), "pres": u(95.0, 102.0), "swdown": u(0.0, 400.0), "difrad": u(0.0, 150.0),
              "lwdown": u(180.0, 320.0), "precip": u(0.0, 2.0), "windspeed": u(0.2, 9.0), "winddir": rng.uniform(0.0, 360.0, T)}
    pointm_c = {"Gp": u(-20.0, 20.0), "Tc": u(-14.0, 4.0), "RswabsG": u(0.0, 200.0), "RlwabsG": u(150.0, 300.0), "umu": u(0.0, 1.0),
                "tr": u(0.0, 1.0)}
    z = rng.uniform(40.0, 240.0, shape)
    z[0, min(4, shape[1] - 1)] = np.nan
    dtmc = rng.uniform(100.0, 200.0, grid)
    if dtmc.size > 1:
        dtmc[-1, -1] = np.nan                                # read as 0
    return clim_c, pointm_c, z, dtmc, api.coarse_positions(shape[0], grid[0]), api.coarse_positions(shape[1], grid[1])


def _host_fine(clim_c, pointm_c, z, dtmc, rowpos, colpos, altcorrect, sl):
    wd = np.asarray(clim_c["winddir"], dtype=np.float64) * np.pi / 180
    wu_c, wv_c = clim_c["windspeed"] * np.cos(wd), clim_c["windspeed"] * np.sin(wd)
    wuv, wvv = np.nanmean(wu_c, axis=(0, 1)), np.nanmean(wv_c, axis=(0, 1))
    winddir = (np.arctan2(wvv, wuv) * 180 / np.pi) % 360
    with np.errstate(invalid="ignore"):
        clim, pointm = S._fine_snow_inputs(clim_c, pointm_c, sl, z, np.nan_to_num(dtmc, nan=0.0), rowpos, colpos, altcorrect, wu_c, wv_c,
                                           winddir)
    return clim, pointm


@pytest.mark.parametrize("nsteps", [1, 24, 25, 120])
@pytest.mark.parametrize("altcorrect", [0, 1, 2])
def test_the_expansion_is_the_hosts_resampling(nsteps, altcorrect):
    """altcorrect = 0: taps, mask, cap and the wind speed's sqrt are IEEE operations in the host's order: bytes.  1 and 2: the
    device's pow and exp differ from numpy's by ulps, which elevd x lapse rate and ea / es carry to about 1e-15: 1e-12."""
    T, step0 = 160, 17                                       # the window starts inside a day and, at 120 steps, ends inside one
    for n, (shape, grid) in enumerate(zip(SHAPES + SHAPES[:2], GRIDS)):
        clim_c, pointm_c, z, dtmc, rowpos, colpos = _coarse_fields(shape, grid, T, 300 + n)
        sl = slice(step0, step0 + nsteps)
        want_c, want_p = _host_fine(clim_c, pointm_c, z, dtmc, rowpos, colpos, altcorrect, sl)
        got_c, got_p = S.expand_coarse(clim_c, pointm_c, z, dtmc, rowpos=rowpos, colpos=colpos, altcorrect=altcorrect, step0=step0,
                                       nsteps=nsteps, device=0)
        assert list(got_c) == [*_abi.SNOW_FINE_SERIES[:8], "winddir"] and list(got_p) == list(_abi.SNOW_FINE_SERIES[8:])
        assert got_c["winddir"].tobytes() == np.ascontiguousarray(want_c["winddir"]).tobytes()
        hole = np.isnan(z)
        for k in _abi.SNOW_FINE_SERIES:
            g, w = (got_c[k], want_c[k]) if k in got_c else (got_p[k], want_p[k])
            assert g.shape == shape + (nsteps,), k
            masked = k not in ("pres", "windspeed")          # `.cca` masks; pressure and the wind components are not masked
            if masked or (k == "pres" and altcorrect):       # (the cell's own pressure factor is NA on a hole)
                assert np.all(np.isnan(g[hole])), k
            if masked and not (altcorrect and k in ("temp", "relhum")):     # (the correction's arithmetic runs on the NA: any NaN)
                assert np.all(g[hole].view(np.uint64) == parity_bars.NA_BITS), k
            assert np.array_equal(np.isnan(g), np.isnan(w)), k
            if altcorrect == 0:
                assert np.ascontiguousarray(g[~hole]).tobytes() == np.ascontiguousarray(w[~hole]).tobytes(), (shape, grid, k)
                if not masked:
                    assert g.tobytes() == np.asfortranarray(w).tobytes(), (shape, grid, k)
            else:
                d = float(np.nanmax(np.abs(g - w) / (1 + np.abs(w)), initial=0.0))
                assert d <= 1e-12, (shape, grid, k, d)
        assert np.nanmax(got_c["relhum"]) <= 100.0


@pytest.mark.parametrize("i", [0, 1, 2, 3])                          # 2 x 3, 1 x 2 and 3 x 1 climate grids, altcorrect 0 / 2 / 1 / 2, a hole
def test_a_days_slab_has_the_bits_of_the_day_kernel(oracle, i):
    """mcf_snowmodelq2 hands out the `umu` its day kernel wrote: the chunk kernel writes the same bits for the same hours"""
    c = q2_case(i)
    args, pos = c["args"], c["pos"]
    day = S.snowmodelq2(*args, **pos, series=("umu",))["umu"]
    ndays = day.shape[2] // 24
    for d in range(ndays):
        _, p = S.expand_coarse(args[1], args[2], args[8], args[9], **pos, step0=24 * d, nsteps=24)
        assert p["umu"].tobytes() == np.asfortranarray(day[:, :, 24 * d:24 * d + 24]).tobytes(), (i, d)
    _, p = S.expand_coarse(args[1], args[2], args[8], args[9], **pos)   # every selected hour in one launch: hour groups across the days
    assert p["umu"].tobytes() == day.tobytes()


# ---- the call ---------------------------------------------------------------------------------------------------------
LOOP_CASES = [
    dict(q2=0, altcorrect=0),                                 # 23 x 37 under a 2 x 3 grid
    dict(q2=3, altcorrect=1),                                 # 23 x 37 under a 3 x 1 grid, a hole of the dtm, an initial pack
    dict(q2=3, altcorrect=2, veg_na=True),
    dict(q2=2, altcorrect=2),                                 # one row of 50 cells under a 1 x 2 grid: `.tpicalc`'s raster mean
    dict(q2=3, altcorrect=1, nopack=True),                    # the window with the hole, starting bare (see ORACLE_CASES)
    dict(q2=3, altcorrect=2, nopack=True, veg_na=True),
]
T11 = 11 * 24                                                 # two 120-step chunks and a one-day tail


@functools.lru_cache(maxsize=None)
def _loop_case(n):
    """the chunk loop's arguments as `runsnowmodela(method="slow")` forms them from the product inputs of a q2 case, cut to
    eleven days -> (args, pos): snowmodel2_chunks(*args, **pos, agg=, chunk_steps=)"""
    case = LOOP_CASES[n]
    climarray, obstime, _, vegp, soilc, dtm, kw = q2_case(case["q2"])["product"]
    cr, cc = np.shape(climarray["temp"])[:2]
    z = np.array(dtm["z"], dtype=np.float64)
    R, Cc = z.shape
    zref, windhgt = float(kw["zref"]), float(kw["windhgt"])
    if case.get("nopack"):
        kw = dict(kw, snowinitd=0.0)
    vegp = F.cleanvegp(vegp)
    ob = {k: np.asarray(obstime[k])[:T11] for k in ("year", "month", "day", "hour")}
    clim_c = {k: np.array(np.asarray(climarray[k])[:, :, :T11], dtype=np.float64, order="F") for k in F.WEATHER if k != "winddir"}
    if zref != windhgt:
        clim_c["windspeed"] *= np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    clim_c["winddir"] = np.array([F.getmode(np.asarray(climarray["winddir"])[:, :, k]) for k in range(T11)])
    vc = {k: F.block_reduce(vegp[k], cr, cc) for k in ("pai", "hgt", "leaft", "clump")}
    pointm_c = F.snow_pointm_cells(ob, clim_c, vc, kw["lats_c"], kw["lons_c"], zref, kw["snowinitd"], kw["snowinita"], kw["snowenv"],
                                   False, None)
    vg = {k: np.array(v) for k, v in F.sortl(vegp, np.max(pointm_c["sdepc"], axis=(0, 1))).items()}
    if case.get("veg_na"):
        for k in ("pai", "hgt", "leaft", "clump"):
            vg[k][2, 3] = np.nan                              # a cell without vegetation data on a good dtm cell
        vg["leaft"][4, 1] = np.nan                            # `vegp$leaft[is.na] <- 0.001`
    sdep, sage = z * 0 + kw["snowinitd"], z * 0 + kw["snowinita"]
    other = {"zref": zref, "lats": np.asarray(kw["lats"], dtype=np.float64), "lons": np.asarray(kw["lons"], dtype=np.float64),
             "isnowdc": sdep, "isnowac": sage, "isnowdg": sdep * 0.5, "isnowag": sage}
    res = dtm["res"]
    args = (ob, clim_c, pointm_c, vg, other, kw["snowenv"], z, np.asarray(kw["dtmc"], dtype=np.float64), res if np.isscalar(res) else res[0],
            kw["stfact"])
    pos = dict(rowpos=api.coarse_positions(R, cr), colpos=api.coarse_positions(Cc, cc), altcorrect=case["altcorrect"])
    return args, pos


def _af_wind(args, pos):
    """the chunk wind series the one call works with, read out of its own marshalling (which owns the array)"""
    m, cin, _ = S.marshal_snowcoarse(*args, pos["rowpos"], pos["colpos"], pos["altcorrect"])
    return np.ctypeslib.as_array(cin.drv.af_wind, (m.tsteps,)).copy()


def _is_na(a):
    return np.ascontiguousarray(a).view(np.uint64) == parity_bars.NA_BITS


@pytest.mark.parametrize("n", [0, 1, 2])                      # altcorrect 0, 1, 2
def test_the_one_call_is_the_existing_chunk_loop_on_the_expanded_inputs(oracle, n):
    """No tolerance: the same k_snowmodel<true>, terrain, position index and redistribution on the same bits."""
    args, pos = _loop_case(n)
    ob, clim_c, pointm_c, vg, other, snowenv, z, dtmc, res, tfact = args
    got = S.snowmodel2_coarse(*args, **pos, agg=10)
    assert list(got) == list(NAMES) and all(v.shape == z.shape + (T11,) for v in got.values())
    clim, pointm = S.expand_coarse(clim_c, pointm_c, z, dtmc, **pos)
    af_wind = _af_wind(args, pos)
    vg1 = dict(vg, leaft=np.where(np.isnan(vg["leaft"]), 0.001, vg["leaft"]))
    want = S.snowmodel2_device(ob, clim, pointm, vg1, other, snowenv, z, res, tfact, af_wind=af_wind, wsa_s=10)
    assert np.nanmax(want["groundsnowdepth"]) > 0.01
    hole = np.isnan(z)
    assert hole.any() or n == 0
    for k in FIVE:
        # (mcf_snowmodel2 leaves what the kernel computes from NA weather on a hole of the dtm that has vegetation; the one call
        # applies `.cleansmod` as the host loop does: bytes on every other cell, NA_real_ on the holes)
        assert np.where(hole[:, :, None], want[k], got[k]).tobytes() == want[k].tobytes(), k
        assert _is_na(got[k][hole]).all(), k                  # `.cleansmod`
        assert _is_na(got[k][:, :, 240:]).all(), k            # `1:n5days` truncates: R's pre-filled NA behind the last whole chunk
    assert got["umu"].tobytes() == pointm["umu"].tobytes()      # all 264 steps: the tail is expanded for umu alone
    assert _is_na(got["umu"][hole]).all() and np.isfinite(got["umu"][~hole]).all()


# (loop case, agg = wsa_s, chunk_steps): altcorrect 0 / 1 / 2 / 2.  The cases start bare.  `.snowmodel2` never updates
# other$isnowdg, so under an initial pack a cell whose pack has melted hands `isnowdc = asc + (0 - asc + asd) - asd` to the next
# chunk: a rounding residue of +-2^-60 m that the next chunk's first step tests with `sdepc > 0` (cpp:4336).  Two correct
# evaluations that differ in the last bit of asc take different branches there (canopy temperature 0 against 0.4 degC), so a
# case with such a hand-over says nothing at any bar; starting bare, asd = 0 and a melted pack hands over an exact 0.  The test
# asserts on the ORACLE's output that no hand-over lies within 1e-12 m of the threshold without being 0: the kernels agree
# with the oracle to 1e-14 relative on depths of at most 0.1 m, four orders below that margin.  (The initial pack stays in the
# comparisons with mcf_snowmodel2, where both sides run the same instructions.)
ORACLE_CASES = [(0, 10, 120), (4, 1, 48), (5, 10, 48), (3, 1, 120)]


@pytest.mark.parametrize("n,agg,chunk_steps", ORACLE_CASES)
def test_one_call_matches_the_oracle_on_real_coarse_grids(oracle, n, agg, chunk_steps):
    """The bar is tests/test_snowmodel2_gpu.py's for this oracle: identical NaN masks and 1e-6 scaled (parity_bars.CAP).
    Derived bars are not available here: snowarray_oracle's chunk loop takes no variant library, so there is no noise
    measurement to derive them from."""
    from oracle import snowarray_oracle as SA
    from oracle import snowdriver_oracle as SD
    args, pos = _loop_case(n)
    ob, clim_c, pointm_c, vg, other, snowenv, z, dtmc, res, tfact = args
    want = SA.snowmodel2_chunks(*args, pos["rowpos"], pos["colpos"], altcorrect=pos["altcorrect"], agg=agg, chunk_steps=chunk_steps)
    # what the case is there for, asserted on the reference side: snow on the ground, and a cell the redistribution moves
    depth = want["groundsnowdepth"]
    assert np.nanmax(depth) > 0.01
    last = np.arange(1, T11 // chunk_steps + 1) * chunk_steps - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        handed = want["totalSWE"][:, :, last] / want["snowden"][:, :, last]           # isnowdc of the next chunk
        assert not np.any((handed != 0) & (np.abs(handed) < 1e-12))                    # admissible: no hand-over on `sdepc > 0`
    wd = np.asarray(clim_c["winddir"]) * np.pi / 180
    wuv = np.nanmean(clim_c["windspeed"] * np.cos(wd), axis=(0, 1))[:chunk_steps]
    wvv = np.nanmean(clim_c["windspeed"] * np.sin(wd), axis=(0, 1))[:chunk_steps]
    af = max(int(np.round(10 * np.mean(np.sqrt(wuv ** 2 + wvv ** 2)) ** 0.5 / res)), 2)
    tpi = SD.tpicalc(af, min(z.shape), z + other["isnowdg"], tfact)
    with np.errstate(invalid="ignore"):
        grown = depth[:, :, :chunk_steps].max(axis=2) > other["isnowdg"]
        assert np.any(grown & np.isfinite(tpi) & (np.abs(tpi - 1.0) > 1e-3))
    got = S.snowmodel2_coarse(*args, **pos, agg=agg, chunk_steps=chunk_steps)
    assert list(got) == list(NAMES)
    for k in NAMES:
        print(f"loop case {n} agg {agg} chunk {chunk_steps} {k:15s} largest scaled |one call - oracle| = "
              f"{parity_bars.distance(got[k], want[k]):.3e}")
    for k in NAMES:
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert parity_bars.distance(got[k], want[k]) < parity_bars.CAP, k


# ---- the front end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 6])                            # cases that start bare: see ORACLE_CASES
def test_front_end_device_loop_matches_the_host_loop(oracle, i):
    """HIP against HIP at test_snowmodel2_gpu.py's 1e-9: the host loop does the redistribution in numpy"""
    climarray, obstime, _, vegp, soilc, dtm, kw = q2_case(i)["product"]
    cr, cc = np.shape(climarray["temp"])[:2]
    clima = {k: np.asfortranarray(np.asarray(v)[:, :, :T11]) for k, v in climarray.items()}
    obst = {k: np.asarray(v)[:T11] for k, v in obstime.items()}
    complete = [{"subs": np.arange(1, T11 + 1), "ntme": T11, "zref": kw["zref"]}] * (cr * cc)
    kw = dict(kw, method="slow")
    got = F.runsnowmodela(clima, obst, complete, vegp, soilc, dtm, device_loop=True, **kw)
    ref = F.runsnowmodela(clima, obst, complete, vegp, soilc, dtm, device_loop=False, **kw)
    assert list(got) == list(ref) == list(NAMES)
    for k in NAMES:
        assert got[k].shape == ref[k].shape == np.shape(dtm["z"]) + (T11,), k
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        d = parity_bars.distance(got[k], ref[k])
        print(f"case {i} {k:15s} largest scaled |device loop - host loop| = {d:.3e}")
        assert d < 1e-9, (k, d)
    assert np.nanmax(ref["groundsnowdepth"]) > 0.01
    # subset micropoints with the slow method: the complete run, subset along time
    days = np.array([2, 3, 10, 11])
    subs = (np.repeat((days - 1) * 24, 24) + np.tile(np.arange(24), days.size) + 1).astype(np.int64)
    some = [{"subs": subs, "ntme": T11, "zref": kw["zref"]}] * (cr * cc)
    sub = F.runsnowmodela(clima, obst, some, vegp, soilc, dtm, device_loop=True, **kw)
    if kw["zref"] == kw["windhgt"]:                              # (complete micropoints take zref = windhgt from the micropoint)
        assert list(sub) == list(NAMES)
        for k in NAMES:
            assert sub[k].tobytes() == np.asfortranarray(got[k][:, :, subs - 1]).tobytes(), k
    assert sub["Tc"].shape[2] == subs.size and _is_na(sub["Tc"][:, :, 72:]).all()     # day 11: behind the last whole chunk


# ---- outputs and state --------------------------------------------------------------------------------------------------
def test_wanted_series_repeats_and_a_call_after_a_refusal(oracle):
    args, pos = _loop_case(1)
    full = S.snowmodel2_coarse(*args, **pos)
    assert list(full) == list(NAMES)
    only = S.snowmodel2_coarse(*args, **pos, series=("totalSWE",))
    assert list(only) == ["totalSWE"]
    assert only["totalSWE"].tobytes() == full["totalSWE"].tobytes()     # bit for bit, NaN payloads included
    umu = S.snowmodel2_coarse(*args, **pos, series=("umu",))
    assert list(umu) == ["umu"] and umu["umu"].tobytes() == full["umu"].tobytes()
    again = S.snowmodel2_coarse(*args, **pos)
    for k in full:
        assert again[k].tobytes() == full[k].tobytes(), k
    bad = dict(pos, colpos=np.array(pos["colpos"]) + 5.0)               # positions outside the climate grid
    with pytest.raises(_abi.McfError, match="coarse_rowpos / coarse_colpos"):
        S.snowmodel2_coarse(*args, **bad)
    with pytest.raises(_abi.McfError, match="chunk_steps"):
        S.snowmodel2_coarse(*args, **pos, chunk_steps=100)
    after = S.snowmodel2_coarse(*args, **pos, series=("groundsnowdepth", "snowden"))
    assert list(after) == ["groundsnowdepth", "snowden"]
    for k in after:
        assert after[k].tobytes() == full[k].tobytes(), k


def test_a_partial_last_hour_group_per_chunk(oracle):
    """17 x 31 cells with chunk_steps = 24: the chunk kernel walks groups of five hours, so every chunk ends in a group of four
    (and 527 cells end in a partial workgroup); the call is still the existing loop on the expanded inputs, in bytes"""
    args, pos = _loop_case(0)
    ob, clim_c, pointm_c, vg, other, snowenv, z, dtmc, res, tfact = args
    cut = lambda a: np.array(np.asarray(a)[3:20, 2:33])                  # noqa: E731
    vg, z = {k: cut(v) for k, v in vg.items()}, cut(z)
    other = {k: (v if k == "zref" else cut(v)) for k, v in other.items()}
    R, Cc = z.shape
    assert (R, Cc) == (17, 31)
    T = 72
    ob = {k: v[:T] for k, v in ob.items()}
    clim_c = {k: (v[:T] if v.ndim == 1 else np.asfortranarray(v[:, :, :T])) for k, v in clim_c.items()}
    pointm_c = {k: np.asfortranarray(v[:, :, :T]) for k, v in pointm_c.items()}
    cr, cc = clim_c["temp"].shape[:2]
    pos = dict(pos, rowpos=api.coarse_positions(R, cr), colpos=api.coarse_positions(Cc, cc), altcorrect=2)
    a = (ob, clim_c, pointm_c, vg, other, snowenv, z, dtmc, res, tfact)
    got = S.snowmodel2_coarse(*a, **pos, agg=1, chunk_steps=24)
    clim, pointm = S.expand_coarse(clim_c, pointm_c, z, dtmc, **pos)
    af_wind = _af_wind(a, pos)
    want = S.snowmodel2_device(ob, clim, pointm, dict(vg, leaft=np.where(np.isnan(vg["leaft"]), 0.001, vg["leaft"])), other, snowenv, z, res,
                               tfact, af_wind=af_wind, wsa_s=1, chunk_steps=24)
    for k in FIVE:
        assert got[k].tobytes() == want[k].tobytes(), k
        assert not _is_na(got[k][:, :, 48:][~np.isnan(z)]).any(), k          # three whole chunks: no tail
    assert got["umu"].tobytes() == pointm["umu"].tobytes()
    for t in range(T):                                                       # hour by hour against the host's resampling
        w = _host_fine(clim_c, pointm_c, z, dtmc, pos["rowpos"], pos["colpos"], 0, slice(t, t + 1))[1]["umu"]
        assert np.ascontiguousarray(got["umu"][:, :, t][~np.isnan(z)]).tobytes() == np.ascontiguousarray(w[:, :, 0][~np.isnan(z)]).tobytes(), t
