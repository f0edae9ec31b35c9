"""The fast snow method for array weather as one device-resident call (mcf_snowmodelq2; `runsnowmodela(..., one_call=True)`):
the gap kernel alone against the host entry and the oracle, the call against the oracle's restatement of `.snowmodelq2`'s day
loop and against the host day loop it replaces, `umu` against the host's resampling bit for bit, and what the call returns
when asked for less, asked twice, or asked after a refusal."""
import numpy as np
import pytest

from microclimf_amd import _abi, api
from microclimf_amd import frontend as F
from microclimf_amd import snow as S
from microclimf_amd import terrain
from microclimf_amd.rformulas import upsample_coarse
import parity_bars
import snowfast_cases as FC
from snowfast_cases import Q2_CASES as CASES, q2_case as _case

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


# ---- the day loop's branches that the cases above do not take -------------------------------------------------------------
@pytest.mark.parametrize("days", [FC.ONE_DAY, FC.TEN_DAYS], ids=["one day", "cache eviction"])
def test_one_selected_day_and_more_factors_than_cached_match_the_host_day_loop(oracle, days):
    """One selected day: a single output set and `done` event, only the trailing download.  Ten days with the aggregation
    factors 2 .. 10, 2 (tests/test_snowfast_onecall_cpu.py): the ninth distinct factor is computed over the oldest of the eight
    kept position indices and the tenth day needs the evicted one again."""
    args, pos = FC.loop_args("q2", days)
    got, ref = S.snowmodelq2(*args, **pos), S.snowmodelq2_days(*args, **pos)
    assert list(got) == list(ref) and got["Tc"].shape[2] == 24 * len(days)
    err, where = _worst(got, ref)
    print(f"{len(days)} days: largest scaled |one call - day loop| = {err:.3e} at {where}, deepest ground snow "
          f"{np.nanmax(got['groundsnowdepth']):.4f} m")
    assert err < 1e-6, f"largest scaled difference between the one call and the host day loop: {err:.3e} at {where}"
    if days == FC.TEN_DAYS:
        assert np.nanmax(got["groundsnowdepth"]) > 0.01                # the position index matters
    only = S.snowmodelq2(*args, **pos, series=("totalSWE",))
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
        print(f"q2 case {i} terrain {k:8s} largest |device - oracle| {np.nanmax(np.abs(dev_t[k] - w), initial=0.0):.3e}")
    for k, w in want_t.items():
        np.testing.assert_allclose(dev_t[k], w, rtol=0, atol=1e-10, err_msg=k)
    want, bars, noise = parity_bars.bars_for(oracle, FC.run(oracle, c, terrain=dev_t), ("snowfast2-device-terrain", i))
    assert max(bars.values()) < parity_bars.CAP                         # admissible (snowfast_cases.py)
    got = {"one call": S.snowmodelq2(*c["args"], **c["pos"]), "day loop": S.snowmodelq2_days(*c["args"], **c["pos"])}
    for name, g in got.items():
        assert list(g) == list(want)
        for k in want:
            print(f"q2 case {i} {name} {k:15s} distance {parity_bars.distance(g[k], want[k]):.3e}  bar {bars[k]:.3e}  N {noise[k]:.2e}")
    for name, g in got.items():
        parity_bars.compare(g, want, bars)


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
