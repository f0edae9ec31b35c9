"""The fast snow method as one device-resident call (mcf_snowmodelq1; `runsnowmodel(..., one_call=True)`): its two kernel
entries against the host entries and the oracle, the call against the oracle's restatement of `.snowmodelq1`'s day loop and
against the host day loop it replaces, and what it returns when asked for less or asked twice."""
import numpy as np
import pytest

from microclimf_amd import _abi
from microclimf_amd import frontend as F
from microclimf_amd import snow as S
from microclimf_amd import terrain
import parity_bars
import snowfast_cases as FC
from snowfast_cases import Q1_CASES as CASES, q1_case as _case

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


# ---- the day loop's branches that the cases above do not take -------------------------------------------------------------
@pytest.mark.parametrize("days", [FC.ONE_DAY, FC.TEN_DAYS], ids=["one day", "cache eviction"])
def test_one_selected_day_and_more_factors_than_cached_match_the_host_day_loop(oracle, days):
    """One selected day: a single output set and `done` event, only the trailing download.  Ten days with the aggregation
    factors 2 .. 10, 2 (tests/test_snowfast_onecall_cpu.py): the ninth distinct factor is computed over the oldest of the eight
    kept position indices and the tenth day needs the evicted one again."""
    args, _ = FC.loop_args("q1", days)
    got, ref = S.snowmodelq1(*args), S.snowmodelq1_days(*args)
    assert list(got) == list(ref) and got["Tc"].shape[2] == 24 * len(days)
    err, where = _worst(got, ref)
    print(f"{len(days)} days: largest scaled |one call - day loop| = {err:.3e} at {where}, deepest ground snow "
          f"{np.nanmax(got['groundsnowdepth']):.4f} m")
    assert err < 1e-6, f"largest scaled difference between the one call and the host day loop: {err:.3e} at {where}"
    if days == FC.TEN_DAYS:
        assert np.nanmax(got["groundsnowdepth"]) > 0.01                # the position index matters
    only = S.snowmodelq1(*args, series=("totalSWE",))
    assert list(only) == ["totalSWE"] and only["totalSWE"].tobytes() == got["totalSWE"].tobytes()


# ---- the call and the host day loop against the oracle chain under derived bars ----------------------------------------
@pytest.mark.parametrize("i", FC.SMALL)
def test_one_call_and_day_loop_within_the_derived_bars_of_the_oracle_chain(oracle, i):
    """The 1e-6 of the product-level tests above cannot see a single-precision exp, log or sqrt in the snow day kernels, the
    gap balance or the redistribution (tests/test_snowfast_bars_cpu.py); the bars of parity_bars.py can.  They are floor-level
    (2^-40), while 1e-10 on the terrain moves Tg by 4e-9 and no oracle variant models numpy terrain: so the device's own
    terrain is first held to terrain_oracle (the bound of test_terrain_gpu.py) and then handed to the oracle chain, which
    takes the terrain out of the snow kernels' account without widening anything.  The host day loop runs the same device
    kernels on the same terrain and owes the same bars."""
    c = _case(i)
    z, res, zref, want_t = FC.oracle_terrain(c)
    dev_t = terrain.snow_terrain(z, res, zref, device=0)
    assert list(dev_t) == list(want_t)
    for k, w in want_t.items():
        assert dev_t[k].shape == w.shape and np.array_equal(np.isnan(dev_t[k]), np.isnan(w)), k
        print(f"q1 case {i} terrain {k:8s} largest |device - oracle| {np.nanmax(np.abs(dev_t[k] - w), initial=0.0):.3e}")
    for k, w in want_t.items():
        np.testing.assert_allclose(dev_t[k], w, rtol=0, atol=1e-10, err_msg=k)
    want, bars, noise = parity_bars.bars_for(oracle, FC.run(oracle, c, terrain=dev_t), ("snowfast1-device-terrain", i))
    assert max(bars.values()) < parity_bars.CAP                         # admissible (snowfast_cases.py)
    got = {"one call": S.snowmodelq1(*c["args"]), "day loop": S.snowmodelq1_days(*c["args"])}
    for name, g in got.items():
        assert list(g) == list(want)
        for k in want:
            print(f"q1 case {i} {name} {k:15s} distance {parity_bars.distance(g[k], want[k]):.3e}  bar {bars[k]:.3e}  N {noise[k]:.2e}")
    for name, g in got.items():
        parity_bars.compare(g, want, bars)


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
