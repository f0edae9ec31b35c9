"""The fast snow method as one device-resident call (mcf_snowmodelq1; `runsnowmodel(..., one_call=True)`): its two kernel
entries against the host entries and the oracle, the call against the oracle's restatement of `.snowmodelq1`'s day loop and
against the host day loop it replaces, and what it returns when asked for less or asked twice."""
import functools

import numpy as np
import pytest

from bundled import load
from microclimf_amd import _abi
from microclimf_amd import frontend as F
from microclimf_amd import snow as S

pytestmark = pytest.mark.gpu

SHAPES = [(7, 9), (23, 37), (1, 50)]      # 23 x 37 = 851 cells: several workgroups, the last one partial; 1 x 50: less than a wave


# ---- the kernel entries alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_canintfrac_on_the_device(shape):
    from oracle import snowfast_oracle as SF
    rng = np.random.default_rng(shape[0])
    hgt = rng.uniform(0.0, 25.0, shape)
    pai = rng.uniform(0.0, 6.0, shape)
    hgt[0, 3] = np.nan
    hgt[0, 0], pai[0, 1] = 0.0, 0.0                      # the 0.001 floors
    got = S.canintfrac(hgt, pai, 2.0, 1.7, -3.0, 0.0, device=0)
    assert np.isnan(got[0, 3]) and np.isnan(got).sum() == 1
    np.testing.assert_allclose(got, S.canintfrac(hgt, pai, 2.0, 1.7, -3.0, 0.0), rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(got, SF.canintfrac(hgt, pai, 2.0, 1.7, -3.0, 0.0), rtol=1e-12, equal_nan=True)
    for prec in (0.0, float("nan")):                     # no snowfall in the series
        got = S.canintfrac(hgt, pai, 2.0, prec, -3.0, 0.0, device=0)
        assert np.isnan(got[0, 3]) and np.all(got[~np.isnan(hgt)] == 0.5)
        np.testing.assert_array_equal(got, S.canintfrac(hgt, pai, 2.0, prec, -3.0, 0.0))


# (the gap kernel reads a step's pair through scalar loads straight from the series: it stages nothing, so there is no piece
# size of its own to straddle)
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1024, 1025, 4099])
def test_meltmu_on_the_device(n):
    from oracle import snowfast_oracle as SF
    rng = np.random.default_rng(100 + n)
    stemp = rng.normal(0.5, 3.0, n)
    tc = stemp - rng.uniform(0.0, 4.0, n)
    for shape in SHAPES:
        sv = rng.uniform(0.3, 1.0, shape)
        sv[0, 2] = np.nan
        got = S.meltmu(sv, stemp, tc, device=0)
        # every term is positive: the sum's error is below n 2^-53 relative, 4.6e-13 at n = 4099
        np.testing.assert_allclose(got, S.meltmu(sv, stemp, tc), rtol=1e-12, equal_nan=True)
        if (stemp > 0).any():
            assert np.isnan(got[0, 2]) and np.isnan(got).sum() == 1 and np.nanmin(got) >= 0.0
        else:
            assert np.all(got == 1.0)                    # n = 0 or nothing thaws
        if n <= 257:
            np.testing.assert_allclose(got, SF.meltmu(sv, stemp, tc), rtol=1e-12, equal_nan=True)
        assert np.all(S.meltmu(sv, -np.abs(stemp), tc, device=0) == 1.0)          # frozen: 1 everywhere, the NA cell included
        np.testing.assert_allclose(S.meltmu(np.ones(shape), stemp, tc, device=0), 1.0, rtol=1e-12)   # open sky: the point model


# ---- the call against the oracle chain ------------------------------------------------------------------------------
CASES = [
    dict(days=[2, 3, 49], window=(0, 23, 0, 37)),           # gaps of 24 h, of 2 h counting down, of 1 080 h
    dict(days=[4, 11, 12, 30, 47], window=(0, 50, 0, 50)),
    dict(days=[10, 40], window=(12, 13, 0, 50), snowenv="Prairie", cold=-14.0),          # one row: `.tpicalc`'s raster mean
    dict(days=[3, 20, 44], window=(5, 28, 10, 47), snowenv="Alpine", snowinitd=0.002, snowinita=30.0, stfact=0.03, hole=True),
    dict(days=[6, 7, 8, 35], window=(20, 50, 0, 19), snowenv="Tundra", zref=3.0, windhgt=2.0),
    dict(days=[5, 20], window=(10, 30, 5, 30), cold=5.0, bare=True),                     # no snowfall at all: msnow is NaN
    dict(days=[5, 6, 20], window=(10, 30, 5, 30), cold=-30.0),                           # every gap frozen: mu = 1
]


def _crop(vegp, soilc, dtm, r0, r1, c0, c1):
    cut = lambda a: np.array(np.asarray(a)[r0:r1, c0:c1])                # noqa: E731
    return {k: cut(v) for k, v in vegp.items()}, {k: cut(v) for k, v in soilc.items()}, dict(dtm, z=cut(dtm["z"]))


@functools.lru_cache(maxsize=None)
def _case(i):
    """the product's inputs of CASES[i], the day loop's arguments as the oracle chain forms them (built as
    tests/test_snowfast_gpu.py::test_fast_method_matches_the_oracle_chain builds `want`), and the oracle's result"""
    from oracle import oracle as O
    from oracle import replay_reference_tests as RT
    from oracle import snowfast_oracle as SF
    O.load()
    case = CASES[i]
    weather, vegp, soilc, dtm = load(50 * 24)
    vegp, soilc, dtm = _crop(vegp, soilc, dtm, *case["window"])
    if case.get("hole"):
        dtm["z"][5:8, 6:9] = np.nan
    weather = dict(weather, temp=weather["temp"] + case.get("cold", -9.0))
    env, sd0, sa0 = case.get("snowenv", "Taiga"), case.get("snowinitd", 0.0), case.get("snowinita", 0.0)
    zref, windhgt, stfact = case.get("zref", 2.0), case.get("windhgt", case.get("zref", 2.0)), case.get("stfact", 0.01)
    mp = F.subsetpointmodel(F.runpointmodel(weather, 0.05, dtm, vegp, soilc), days=case["days"])
    kw = dict(snowenv=env, snowinitd=sd0, snowinita=sa0, zref=zref, windhgt=windhgt, stfact=stfact)
    z = np.asarray(dtm["z"])
    vg = F.cleanvegp(vegp)
    vp = F.sortvegp_point(vg)
    obst = {k: np.asarray(v) for k, v in weather["obstime"].items()}
    w = {k: np.array(weather[k], dtype=np.float64) for k in F.WEATHER}
    if zref != windhgt:
        w["windspeed"] = w["windspeed"] * np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    assert np.nanmax(vg["hgt"]) <= zref
    sdep, sage = z * 0 + sd0, z * 0 + sa0
    pm = RT.pointmodelsnow(obst, w, np.array([vp[1], vp[0], vp[5], vp[3]]),
                           np.array([0, 0, mp["lat"], mp["long"], zref, np.nanmean(sdep), np.nanmean(sage)]), env, maxiter=20)
    T = len(w["temp"])
    ai = np.asarray(mp["subs"]) - 1
    pointm = {"Gp": pm["G"], "Tc": pm["Tc"], "RswabsG": pm["RswabsG"], "RlwabsG": pm["RlwabsG"], "umu": pm["umu"], "tr": pm["tr"]}
    vs = F.sortl(vg, pm["sdepc"][:T])
    vs["leaft"] = np.where(np.isnan(vs["leaft"]), 0.01, vs["leaft"])
    other = {"zref": zref, "lat": mp["lat"], "lon": mp["long"], "isnowdc": sd0 * z, "isnowac": sage, "isnowag": sage}
    rows = lambda d: {k: np.asarray(v)[ai] for k, v in d.items()}      # noqa: E731
    args = (rows(obst), rows(w), rows(pointm), pm, w["temp"], np.where(w["temp"] > 2, 0.0, w["precip"]), mp["subs"], vs, other, env, z,
            dtm["res"], stfact)
    want = SF.snowmodelq1_days(*args)
    for v in want.values():
        v.flags.writeable = False
    return dict(product=(weather, mp, vegp, soilc, dtm, kw), args=args, want=want, umu=pm["umu"][ai])


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
    weather, mp, vegp, soilc, dtm, kw = c["product"]
    got = F.runsnowmodel(weather, mp, vegp, soilc, dtm, one_call=True, **kw)
    n = 24 * len(CASES[i]["days"])
    assert list(got) == ["Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden", "umu"] and got["Tc"].shape == np.shape(dtm["z"]) + (n,)
    np.testing.assert_allclose(got["umu"], c["umu"], rtol=1e-10)
    err, where = _worst(got, c["want"])
    print(f"case {i}: largest scaled |one call - oracle| = {err:.3e} at {where}")
    assert err < 1e-6, (err, where)
    depth = got["groundsnowdepth"][np.isfinite(got["groundsnowdepth"])]
    if CASES[i].get("bare"):
        assert np.all(depth == 0.0) and np.all(got["totalSWE"][np.isfinite(got["totalSWE"])] == 0.0)
    else:
        assert depth.max() > 0.01


@pytest.mark.parametrize("i", [0, 1])
def test_one_call_matches_the_host_day_loop(oracle, i):
    weather, mp, vegp, soilc, dtm, kw = _case(i)["product"]
    got = F.runsnowmodel(weather, mp, vegp, soilc, dtm, one_call=True, **kw)
    ref = F.runsnowmodel(weather, mp, vegp, soilc, dtm, one_call=False, **kw)
    assert list(got) == list(ref)
    err, where = _worst(got, ref)
    print(f"case {i}: largest scaled |one call - day loop| = {err:.3e} at {where}")
    assert err < 1e-6, f"largest scaled difference between the one call and the host day loop: {err:.3e} at {where}"


# ---- outputs and state ----------------------------------------------------------------------------------------------
def test_wanted_series_repeats_and_a_call_after_a_refusal(oracle):
    args = _case(0)["args"]
    full = S.snowmodelq1(*args)
    assert list(full) == ["Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden"]
    only = S.snowmodelq1(*args, series=("totalSWE",))
    assert list(only) == ["totalSWE"]
    assert only["totalSWE"].tobytes() == full["totalSWE"].tobytes()     # bit for bit, NaN payloads included
    again = S.snowmodelq1(*args)
    for k in full:
        assert again[k].tobytes() == full[k].tobytes(), k
    bad = list(args)
    bad[6] = np.asarray(args[6]) - 24                                    # the first selected day becomes the series' first
    with pytest.raises(_abi.McfError, match="first day"):
        S.snowmodelq1(*bad)
    after = S.snowmodelq1(*args, series=("groundsnowdepth", "snowden"))
    for k in after:
        assert after[k].tobytes() == full[k].tobytes(), k
