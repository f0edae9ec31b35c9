"""The fast snow method for array weather as one device-resident call (mcf_snowmodelq2; `runsnowmodela(..., one_call=True)`):
the gap kernel alone against the host entry and the oracle, the call against the oracle's restatement of `.snowmodelq2`'s day
loop and against the host day loop it replaces, `umu` against the host's resampling bit for bit, and what the call returns
when asked for less, asked twice, or asked after a refusal."""
import functools

import numpy as np
import pytest

from bundled import load
from microclimf_amd import _abi, api
from microclimf_amd import frontend as F
from microclimf_amd import snow as S
from microclimf_amd.rformulas import upsample_coarse

pytestmark = pytest.mark.gpu

SHAPES = [(7, 9), (23, 37), (1, 50)]      # 23 x 37 = 851 cells: several workgroups, the last one partial; 1 x 50: less than a wave
GRIDS = [(1, 1), (1, 2), (3, 1), (2, 3), (5, 4)]     # single coarse rows / columns: r1 / c1 fall back onto r0 / c0


# ---- the gap kernel alone -------------------------------------------------------------------------------------------
# (the kernel taps the coarse pair of every gap hour straight through the cache: it stages nothing, so there is no piece size
# of its own to straddle; 255 / 256 / 257 and 1024 / 1025 straddle its unroll factor of 4 many times over)
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1024, 1025, 4099])
def test_meltmu2_from_coarse_series_on_the_device(n):
    from oracle import snowfast_oracle as SF
    rng = np.random.default_rng(200 + n)
    for shape, grid in zip(SHAPES + SHAPES[:2], GRIDS):
        st_c = rng.normal(0.5, 3.0, grid + (n,))
        tc_c = st_c - rng.uniform(0.0, 4.0, grid + (n,))
        sv = rng.uniform(0.3, 1.0, shape)
        z = rng.uniform(50.0, 90.0, shape)
        sv[0, 2] = np.nan
        z[0, 4] = np.nan                                     # a hole of the dtm: `.cca` masks the series, nothing thaws there
        rowpos, colpos = api.coarse_positions(shape[0], grid[0]), api.coarse_positions(shape[1], grid[1])
        hole = np.isnan(z)[:, :, None]
        mask = lambda a: np.where(hole, np.nan, upsample_coarse(a, rowpos, colpos))          # noqa: E731
        got = S.meltmu2_coarse(sv, z, st_c, tc_c, rowpos, colpos, device=0)
        want = S.meltmu2(sv, mask(st_c), mask(tc_c))
        # every term is positive: the sum's error is below n 2^-53 relative, 4.6e-13 at n = 4099
        assert np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=1e-12, equal_nan=True)
        assert np.isnan(got[0, 2]) and np.isnan(got).sum() == 1 and got[0, 4] == 0.5 and np.nanmin(got) >= 0.0
        if n <= 257:
            np.testing.assert_allclose(got, SF.meltmu2(sv, mask(st_c), mask(tc_c)), rtol=1e-12, equal_nan=True)
        frozen = S.meltmu2_coarse(sv, z, -np.abs(st_c), tc_c, rowpos, colpos, device=0)      # 0.5, not `meltmu`'s 1
        assert np.all(frozen[~np.isnan(sv)] == 0.5) and np.isnan(frozen[0, 2])


# ---- the call against the oracle chain ------------------------------------------------------------------------------
CASES = [
    dict(days=[2, 3, 49], window=(0, 23, 0, 37), grid=(2, 3), altcorrect=0),       # gaps of 24 h, of 2 h counting down, of 1 080 h
    dict(days=[4, 6, 7, 12], window=(0, 50, 0, 50), grid=(2, 3), altcorrect=2),
    dict(days=[10, 40], window=(12, 13, 0, 50), grid=(1, 2), altcorrect=1, snowenv="Prairie", cold=-14.0),   # one row: `.tpicalc`'s raster mean
    dict(days=[3, 20, 44], window=(5, 28, 10, 47), grid=(3, 1), altcorrect=2, snowenv="Alpine", snowinitd=0.002, snowinita=30.0,
         stfact=0.03, hole=True),
    dict(days=[1, 2, 8, 35], window=(20, 50, 0, 19), grid=(2, 3), altcorrect=0, snowenv="Tundra", zref=3.0, windhgt=2.0),   # the series' first day
    dict(days=[5, 20], window=(10, 30, 5, 30), grid=(1, 2), altcorrect=0, cold=5.0, bare=True),          # no snowfall at all: msnow is NaN
    dict(days=[5, 6, 20], window=(10, 30, 5, 30), grid=(2, 3), altcorrect=1, cold=-30.0),                # every gap frozen: mu = 0.5
]


def _crop(vegp, soilc, dtm, r0, r1, c0, c1):
    cut = lambda a: np.array(np.asarray(a)[r0:r1, c0:c1])                # noqa: E731
    return {k: cut(v) for k, v in vegp.items()}, {k: cut(v) for k, v in soilc.items()}, dict(dtm, z=cut(dtm["z"]))


@functools.lru_cache(maxsize=None)
def _case(i):
    """the product's inputs of CASES[i], the day loop's arguments as the oracle chain forms them (built as the `fast` case of
    tests/test_snowfast_gpu.py::test_array_weather_snow_model_matches_the_oracle_chain builds `want`), and the oracle's result"""
    from oracle import oracle as O
    from oracle import replay_reference_tests as RT
    from oracle import snowfast_oracle as SF
    O.load()
    case = CASES[i]
    weather, vegp, soilc, dtm = load(50 * 24)
    vegp, soilc, dtm = _crop(vegp, soilc, dtm, *case["window"])
    if case.get("hole"):
        dtm["z"][5:8, 6:9] = np.nan
    (cr, cc), T = case["grid"], 50 * 24
    z = np.asarray(dtm["z"])
    R, Cc = z.shape
    rng = np.random.default_rng(9 + i)
    climarray = {}
    for k in F.WEATHER:
        base = np.broadcast_to(weather[k][None, None, :], (cr, cc, T)).copy()
        if k == "temp":
            base += case.get("cold", -9.0) + rng.uniform(-1.5, 1.5, (cr, cc, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (cr, cc, 1))
        elif k == "winddir":
            base = (base + rng.integers(-1, 2, (cr, cc, T)) * 10.0) % 360
        climarray[k] = np.asfortranarray(base)
    climarray["difrad"] = np.minimum(climarray["difrad"], climarray["swdown"])
    clat = dtm["lat"] + 1e-4 * np.arange(cr)[:, None] + 0 * np.arange(cc)[None, :]
    clon = dtm["long"] + 1e-4 * np.arange(cc)[None, :] + 0 * np.arange(cr)[:, None]
    lats = dtm["lat"] + 9e-6 * np.arange(R)[::-1, None] + 0 * np.arange(Cc)[None, :]
    lons = dtm["long"] + 1.4e-5 * np.arange(Cc)[None, :] + 0 * np.arange(R)[:, None]
    dtmc = np.nanmean(z) + 40.0 + 5.0 * np.arange(cr * cc).reshape(cr, cc)
    env, sd0, sa0 = case.get("snowenv", "Taiga"), case.get("snowinitd", 0.0), case.get("snowinita", 0.0)
    zref, windhgt, stfact = case.get("zref", 2.0), case.get("windhgt", case.get("zref", 2.0)), case.get("stfact", 0.01)
    days = np.asarray(case["days"])
    subs = (np.repeat((days - 1) * 24, 24) + np.tile(np.arange(24), days.size) + 1).astype(np.int64)
    mpa = [{"subs": subs, "ntme": T, "zref": zref}] * (cr * cc)         # what runsnowmodela reads of subsetpointmodel's output
    kw = dict(dtmc=dtmc, lats_c=clat, lons_c=clon, lats=lats, lons=lons, altcorrect=case["altcorrect"], snowenv=env, snowinitd=sd0,
              snowinita=sa0, zref=zref, windhgt=windhgt, stfact=stfact)
    # the same through the oracle
    vg = F.cleanvegp(vegp)
    assert np.nanmax(vg["hgt"]) <= zref
    obst = {k: np.asarray(v) for k, v in weather["obstime"].items()}
    wdir = np.array([F.getmode(climarray["winddir"][:, :, k]) for k in range(T)])
    vc = {k: F.block_reduce(vg[k], cr, cc) for k in ("pai", "hgt", "leaft", "clump")}
    clim_c = {k: np.array(climarray[k], copy=True) for k in F.WEATHER if k != "winddir"}
    if zref != windhgt:
        clim_c["windspeed"] *= np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    clim_c["winddir"] = wdir
    names = {"Gp": "G", "Tc": "Tc", "RswabsG": "RswabsG", "RlwabsG": "RlwabsG", "umu": "umu", "tr": "tr", "sdepc": "sdepc"}
    names.update({k: k for k in ("sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc", "sdeng")})
    pointm_c = {k: np.empty((cr, cc, T)) for k in names}
    for a in range(cr):
        for b in range(cc):
            w = {k: np.ascontiguousarray(clim_c[k][a, b, :]) for k in clim_c if k != "winddir"}
            pm = RT.pointmodelsnow(obst, w, np.array([np.mean(vc[k][a, b, :]) for k in ("pai", "hgt", "leaft", "clump")]),
                                   np.array([0, 0, clat[a, b], clon[a, b], zref, sd0, sa0]), env, maxiter=10)
            for k, v in names.items():
                pointm_c[k][a, b, :] = pm[v][1:T + 1] if k == "sdepc" else pm[v][:T]
    other = {"zref": zref, "lats": lats, "lons": lons, "isnowdc": z * 0 + sd0, "isnowac": z * 0 + sa0, "isnowag": z * 0 + sa0}
    ai = subs - 1
    sel = lambda d: {k: (np.asarray(v)[ai] if np.ndim(v) == 1 else np.asfortranarray(np.asarray(v)[:, :, ai])) for k, v in d.items()}   # noqa: E731
    pm2 = {k: pointm_c[k] for k in ("sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc", "sdeng")}
    pm2["tc"] = clim_c["temp"]
    pm2["snow"] = np.where(clim_c["temp"] > 2, 0.0, clim_c["precip"])
    pm_s = sel({k: pointm_c[k] for k in ("Gp", "Tc", "RswabsG", "RlwabsG", "umu", "tr", "sdepc")})
    rowpos, colpos = api.coarse_positions(R, cr), api.coarse_positions(Cc, cc)
    args = (sel(obst), sel(clim_c), pm_s, pm2, subs, F.sortl(vg, np.max(pm_s["sdepc"], axis=(0, 1))), other, env, z, dtmc, dtm["res"],
            stfact)
    pos = dict(rowpos=rowpos, colpos=colpos, altcorrect=case["altcorrect"])
    want = SF.snowmodelq2_days(*args, rowpos, colpos, altcorrect=case["altcorrect"])
    for v in want.values():
        v.flags.writeable = False
    # the gaps' multipliers on the reference side: does a gap thaw somewhere (mu neither 0.5 nor NA)?
    hole = np.isnan(z)[:, :, None]
    cca = lambda a: np.where(hole, np.nan, upsample_coarse(a, rowpos, colpos))               # noqa: E731
    thaws = False
    for d in range(days.size):
        if subs[24 * d] - 1 > 1:
            sbtn = SF._colon((subs[24 * d - 1] if d else 0) + 1, int(subs[24 * d]) - 1)
            st = cca(pm2["sstemp"][:, :, sbtn])
            thaws = thaws or bool(np.any(np.nansum(np.where(st > 0, st, 0.0), axis=2) > 0))
    return dict(product=(climarray, weather["obstime"], mpa, vegp, soilc, dtm, kw), args=args, pos=pos, want=want, thaws=thaws,
                umu_c=pm_s["umu"], hole=np.isnan(z))


def _worst(got, want):
    """the bar of tests/test_snowfast_gpu.py: identical NaN and inf masks, every finite value within 1e-6 scaled; -> the
    largest scaled difference and where"""
    worst = (0.0, None)
    for k in want:
        g, x = got[k], want[k]
        assert g.shape == x.shape, k                                   # no cell left out
        assert np.array_equal(np.isnan(g), np.isnan(x)), k
        assert np.array_equal(np.isinf(g), np.isinf(x)), k
        fin = np.isfinite(x)
        if fin.any():
            e = np.abs(g[fin] - x[fin]) / (1 + np.abs(x[fin]))
            j = int(np.argmax(e))
            if e[j] > worst[0]:
                worst = (float(e[j]), (k,) + tuple(int(q[j]) for q in np.nonzero(fin)))
    return worst


@pytest.mark.parametrize("i", range(len(CASES)))
def test_one_call_matches_the_oracle_chain(oracle, i):
    c = _case(i)
    want = c["want"]
    # what the case is there for, asserted on the reference side
    depth = want["groundsnowdepth"][np.isfinite(want["groundsnowdepth"])]
    if CASES[i].get("bare"):
        assert np.all(depth == 0.0) and np.all(want["totalSWE"][np.isfinite(want["totalSWE"])] == 0.0)
    else:
        assert depth.max() > 0.01
    if i == 0:
        assert c["thaws"]                                               # some gap's multiplier is neither 0.5 nor NA
    if CASES[i].get("cold", 0.0) <= -30.0:
        assert not c["thaws"]
    got = S.snowmodelq2(*c["args"], **c["pos"])
    n = 24 * len(CASES[i]["days"])
    assert list(got) == ["Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden", "umu"] and got["Tc"].shape == c["hole"].shape + (n,)
    err, where = _worst(got, want)
    print(f"case {i}: largest scaled |one call - oracle| = {err:.3e} at {where}")
    assert err < 1e-6, (err, where)
    assert np.all(np.isnan(got["groundsnowdepth"][c["hole"]]))          # `.cleansmod`: NA on the holes, not 0


@pytest.mark.parametrize("i", [0, 1, 2, 3])                          # a 2 x 3, a 1 x 2 and a 3 x 1 climate grid, a hole
def test_umu_is_the_hosts_resample_bit_for_bit(oracle, i):
    c = _case(i)
    got = S.snowmodelq2(*c["args"], **c["pos"], series=("umu",))["umu"]
    want = upsample_coarse(c["umu_c"], c["pos"]["rowpos"], c["pos"]["colpos"])
    ok = ~c["hole"]
    assert got[ok].tobytes() == want[ok].tobytes()
    assert np.all(np.isnan(got[c["hole"]]))


@pytest.mark.parametrize("i", [0, 3])
def test_one_call_matches_the_host_day_loop(oracle, i):
    climarray, obstime, mpa, vegp, soilc, dtm, kw = _case(i)["product"]
    got = F.runsnowmodela(climarray, obstime, mpa, vegp, soilc, dtm, one_call=True, **kw)
    ref = F.runsnowmodela(climarray, obstime, mpa, vegp, soilc, dtm, one_call=False, **kw)
    assert list(got) == list(ref)
    err, where = _worst(got, ref)
    print(f"case {i}: largest scaled |one call - day loop| = {err:.3e} at {where}")
    assert err < 1e-6, f"largest scaled difference between the one call and the host day loop: {err:.3e} at {where}"


# ---- outputs and state ----------------------------------------------------------------------------------------------
def test_wanted_series_repeats_and_a_call_after_a_refusal(oracle):
    c = _case(0)
    args, pos = c["args"], c["pos"]
    full = S.snowmodelq2(*args, **pos)
    assert list(full) == ["Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden", "umu"]
    only = S.snowmodelq2(*args, **pos, series=("totalSWE",))
    assert list(only) == ["totalSWE"]
    assert only["totalSWE"].tobytes() == full["totalSWE"].tobytes()     # bit for bit, NaN payloads included
    again = S.snowmodelq2(*args, **pos)
    for k in full:
        assert again[k].tobytes() == full[k].tobytes(), k
    bad = list(args)
    bad[4] = np.asarray(args[4]) + 48                                    # the last selected day runs past the series' end
    with pytest.raises(_abi.McfError, match="outside"):
        S.snowmodelq2(*bad, **pos)
    after = S.snowmodelq2(*args, **pos, series=("groundsnowdepth", "snowden"))
    for k in after:
        assert after[k].tobytes() == full[k].tobytes(), k
