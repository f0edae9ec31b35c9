"""Height profiles from one plan (include/mcf.h mcf_plan_set_height, mcf_runmicro_heights).

The yardsticks are never the new code: scipy's gamma distribution (frontend.foliageden) for the foliage kernel, a FRESH Plan
created at the height with the planes the moved plan holds for re-targeting (bit for bit), the oracle under parity_bars for
the values, frontend.runmicro per height for the front end, tests/summary_ref.py for the summaries.
Shapes: 23 x 3 cells (four 21-cell tiles, three 32-cell tiles, the last one partial), 48 h, canopies from 0 to 6 m with bare
and NA cells, heights 0.02 / 0.3 / 1.5 / 4 m so that cells change sides of the canopy top between heights."""
import numpy as np
import pytest

import parity_bars
import summary_ref as SR
from microclimf_amd import McfError, _abi, api, frontend, synthetic
from microclimf_amd.api import Plan
from test_heights_cpu import BAR, rel, same_pattern, sweep

pytestmark = pytest.mark.gpu
ALL = _abi.OUT_NAMES
HEIGHTS = (0.02, 0.3, 1.5, 4.0)
T = 48
bits = SR.bits
_fresh = {}


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} values differ, first at {np.argwhere(diff)[0]}"


def shape_canopy(a):
    """canopies from 0 to 6 m, two bare cells, two NA cells; the two foliage planes are taken out"""
    v = a["vegp"]
    for (i, j) in ((4, 0), (20, 2)):
        v["hgt"][i, j, ...] = 0.0
        v["pai"][i, j, ...] = 0.0
    for (i, j) in ((0, 0), (11, 1)):
        v["hgt"][i, j, ...] = np.nan
    a["vegp"] = {k: x for k, x in v.items() if k not in ("paia", "leafden")}
    return a


def workload(case):
    """-> (arguments without reqhgt / paia / leafden, Plan keywords)"""
    a = synthetic.workload(23, 3, T, reqhgt=0.3, zref=10.0, variety=True, start_doy=170, hgt_range=(0.0, 6.0), na_frac=0.0)      # (zref above every canopy, as runpointmodel leaves it)
    kw = {}
    if case == "two":
        a = synthetic.layered(a, 2)
        kw = dict(dfsel=a.pop("dfsel"), cells_per_block=32)
    a = shape_canopy(a)
    a.pop("reqhgt")
    return a, kw


def with_planes(a, h, pa, ld):
    return dict(a, reqhgt=float(h), vegp=dict(a["vegp"], paia=pa, leafden=ld))


def moving_plan(a, kw, **more):
    z = np.zeros_like(a["vegp"]["pai"])
    return Plan(**with_planes(a, HEIGHTS[0], z, z), ring_days=2, **kw, **more)      # (set_height replaces the zeros before a run)


def solve(p):
    p.run_days(0, 2, 0)
    return {k: p.fetch(0, k, 0, T) for k in ALL}


def fresh(case, tag, a, kw, h, pa, ld):
    """a plan created at `h` with the planes the moved plan holds: made once per (case, tag, height); a second visit must hold
    the same planes"""
    key = (case, tag, h)
    if key not in _fresh:
        with Plan(**with_planes(a, h, pa, ld), ring_days=2, **kw) as p:
            got, st = solve(p), p.dispatch_stats()
        for v in got.values():
            v.setflags(write=False)
        _fresh[key] = (got, st, pa.copy(), ld.copy())
    got, st, pa0, ld0 = _fresh[key]
    assert_bits(pa, pa0, f"paia at {h} on a later visit")
    assert_bits(ld, ld0, f"leafden at {h} on a later visit")
    return got, st


def test_the_heights_split_the_cells_differently():
    hgt = workload("one")[0]["vegp"]["hgt"]
    below = [set(map(tuple, np.argwhere(hgt > h))) for h in HEIGHTS]
    assert all(below[i] > below[i + 1] for i in range(3)) and len(below[3]) > 5 and (hgt == 0).sum() >= 2 and np.isnan(hgt).sum() == 2
    assert np.nanmax(hgt) > 5 and hgt.size == 69 > 3 * 21 and hgt.size > 2 * 32 and hgt.size % 21 and hgt.size % 32


def test_1_foliage_kernel_against_the_twin_and_scipy():
    hgt, pai, z, n = sweep()
    assert hgt.size > 256 and hgt.size % 256                       # more than one workgroup, a partial last one
    ld, pa = api.foliageden(hgt, pai, z, device=0)
    t_ld, t_pa = api.foliageden(hgt, pai, z)
    want_ld, want_pa = frontend.foliageden(z, hgt, pai)
    print(f"k_foliage against the host twin: leafden {rel(ld, t_ld):.3e}, paia {rel(pa, t_pa):.3e}; "
          f"against scipy: leafden {rel(ld, want_ld):.3e}, paia {rel(pa, want_pa):.3e} (bar {BAR:.3e})")
    assert same_pattern(ld, t_ld) and same_pattern(pa, t_pa) and same_pattern(ld, want_ld) and same_pattern(pa, want_pa)
    assert rel(ld, want_ld) <= BAR and rel(pa, want_pa) <= BAR
    a = workload("two")[0]
    for h in HEIGHTS:                                             # the rasters the plans below hold
        ld, pa = api.foliageden(a["vegp"]["hgt"], a["vegp"]["pai"], h, device=0)
        want_ld, want_pa = frontend.foliageden(h, a["vegp"]["hgt"], a["vegp"]["pai"])
        assert ld.shape == (23, 3, 2) and same_pattern(ld, want_ld) and same_pattern(pa, want_pa)
        assert rel(ld, want_ld) <= BAR and rel(pa, want_pa) <= BAR


ORDERS = {"ascending": HEIGHTS, "descending": HEIGHTS[::-1], "revisit": (1.5, 0.3, 1.5)}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("case", ["one", "two"])
def test_2_retargeting_is_bitwise(case, order):
    a, kw = workload(case)
    with moving_plan(a, kw) as p:
        for h in ORDERS[order]:
            p.set_height(h)
            got = solve(p)
            pa, ld = p.fetch_foliage()
            assert pa.shape == a["vegp"]["pai"].shape
            want, st = fresh(case, "derived", a, kw, h, pa, ld)
            for k in ALL:
                assert_bits(got[k], want[k], f"{case} {order}: {k} at {h}")
            assert p.dispatch_stats()["fast_tiles"] == st["fast_tiles"]
    valid = ~np.isnan(a["vegp"]["hgt"][..., 0] if case == "two" else a["vegp"]["hgt"])
    assert np.isfinite(got["Tz"][valid]).all()


def test_2_tile_classes_follow_the_height():
    """fast clamps on: a given plant area above with one infinite value under the canopy at 0.3 m sends that cell's tile to the
    reference form there and nowhere else; the lists are rebuilt at every height"""
    a, kw = workload("one")
    hgt, pai = a["vegp"]["hgt"], a["vegp"]["pai"]
    i, j = np.argwhere((hgt > 2.0) & (pai > 0))[0]
    given = np.asfortranarray(0.5 * pai)
    given[i, j] = np.inf
    seen = {}
    with moving_plan(a, kw) as p:
        for h, g in ((0.02, None), (0.3, given), (1.5, None), (0.3, given), (4.0, None)):
            p.set_height(h, g)
            got = solve(p)
            pa, ld = p.fetch_foliage()
            if g is not None:
                assert_bits(pa, g, "the given plant area above is what the plan holds")
            want, st = fresh("one", "given" if g is not None else "derived", a, kw, h, pa, ld)
            for k in ALL:
                assert_bits(got[k], want[k], f"{k} at {h}")
            mine = p.dispatch_stats()
            assert (mine["fast_tiles"], mine["slow_tiles"]) == (st["fast_tiles"], st["slow_tiles"])
            seen[h] = (mine["fast_tiles"], mine["slow_tiles"])
    assert seen[0.02] == seen[1.5] == seen[4.0] and seen[0.3] == (seen[1.5][0] - 1, seen[1.5][1] + 1) and sum(seen[0.3]) == 4, seen


@pytest.mark.parametrize("case", ["one", "two"])
def test_3_every_height_against_the_oracle(oracle, case):
    a, kw = workload(case)
    with moving_plan(a, kw) as p:
        for h in HEIGHTS:
            p.set_height(h)
            got = solve(p)
            pa, ld = p.fetch_foliage()
            b = with_planes(a, h, pa, ld)
            if "dfsel" in kw:
                b["dfsel"] = kw["dfsel"]
            want, bars = parity_bars.grid(oracle, b, key=("heights", case, h))
            worst = parity_bars.compare(got, want, bars)
            print(f"{case} at {h} m: worst distance / bar {max(worst[k] / bars[k] for k in worst):.3f}")


def plan_loop(a, kw, heights, pai_a=None, **more):
    res = {k: [] for k in ALL}
    held = []
    with moving_plan(a, kw, **more) as p:
        for n, h in enumerate(heights):
            p.set_height(h, None if pai_a is None else pai_a[n])
            for k, v in solve(p).items():
                res[k].append(v)
            held.append(p.fetch_foliage()[0])
    return res, held


@pytest.mark.parametrize("case", ["one", "two"])
def test_4_one_call_equals_the_plan_loop(case):
    a, kw = workload(case)
    given = [None, np.asfortranarray(0.4 * a["vegp"]["pai"]), None, None]
    want, held = plan_loop(a, kw, HEIGHTS, given)
    assert_bits(held[1], given[1], "the given plant area above")
    assert (bits(held[2]) != bits(given[1])).any()
    got = api.runmicro_heights(**a, heights=HEIGHTS, pai_a=given, days_per_chunk=1, **kw)
    assert got["heights"].tolist() == list(HEIGHTS)
    for k in ALL:
        for n, h in enumerate(HEIGHTS):
            assert_bits(got[k][n], want[k][n], f"{case}: {k} at {h}")
    auto = api.runmicro_heights(**dict(a, out=[1, 0, 0, 0, 0, 0, 0, 0, 0, 1]), heights=HEIGHTS[1:3], **kw)      # chunk from free memory
    assert [k for k in auto if k != "heights"] == ["Tz", "Rlwup"]
    assert_bits(auto["Tz"][1], plan_loop(a, kw, HEIGHTS[2:3])[0]["Tz"][0], "Tz alone, derived planes")


def test_4_one_call_with_coarse_forcing():
    a, rp, cp = synthetic.coarse_workload(33, 27, T, 3, 2, reqhgt=0.3, zref=10.0, variety=True, start_doy=170, hgt_range=(0.0, 6.0), na_frac=0.02)
    a["vegp"] = {k: v for k, v in a["vegp"].items() if k not in ("paia", "leafden")}
    a.pop("reqhgt")
    kw = dict(coarse={"rowpos": rp, "colpos": cp})
    heights = (0.3, 4.0)
    want, _ = plan_loop(a, kw, heights)
    got = api.runmicro_heights(**a, heights=heights, **kw)
    for k in ALL:
        for n, h in enumerate(heights):
            assert_bits(got[k][n], want[k][n], f"coarse: {k} at {h}")
    assert (bits(got["Tz"][0]) != bits(got["Tz"][1])).any()


def site():
    """the bundled site cut to 23 x 3 cells, two days, July's vegetation with canopies reshaped to 0 .. 6 m"""
    from bundled import load
    weather, vegp, soilc, dtm = load(T)
    cut = (slice(10, 33), slice(20, 23))
    vegp = {k: np.array((v[:, :, 6] if v.ndim == 3 else v)[cut]) for k, v in vegp.items()}
    soilc = {k: np.array(v[cut]) for k, v in soilc.items()}
    dtm = dict(dtm, z=np.array(dtm["z"][cut]))
    rng = np.random.default_rng(11)
    vegp["hgt"] = rng.uniform(0.05, 6.0, (23, 3))
    vegp["pai"] = np.maximum(vegp["pai"], 0.3)
    vegp["hgt"][4, 0] = vegp["pai"][4, 0] = 0.0
    dtm["z"][11, 1] = np.nan
    return weather, vegp, soilc, dtm


def test_5_front_end_against_runmicro_per_height():
    weather, vegp, soilc, dtm = site()
    mp = frontend.runpointmodel(weather, 1.0, dtm, vegp, soilc)
    got = frontend.runmicro_heights(mp, HEIGHTS, vegp, soilc, dtm)
    assert got["heights"].tolist() == list(HEIGHTS) and len(got["Tz"]) == 4
    for n, h in enumerate(HEIGHTS):
        want = frontend.runmicro(mp, h, vegp, soilc, dtm)                  # scipy-made planes
        assert list(want) == list(ALL)
        worst = parity_bars.compare({k: got[k][n] for k in ALL}, want, tol=parity_bars.CAP)
        print(f"frontend.runmicro_heights against frontend.runmicro at {h} m: {max(worst.values()):.3e}")
    assert np.isfinite(got["Tz"][0][5, 1]).all() and np.isnan(got["Tz"][0][11, 1]).all()


def test_6_summaries_equal_numpy_over_the_arrays():
    weather, vegp, soilc, dtm = site()
    mp = frontend.runpointmodel(weather, 1.0, dtm, vegp, soilc)
    names = ("Tz", "relhum", "Rlwup")
    series = frontend.runmicro_heights(mp, HEIGHTS, vegp, soilc, dtm)
    thr = {k: float(series[k][1][5, 1, 36]) for k in names}
    summ = frontend.runmicro_heights_summary(mp, HEIGHTS, vegp, soilc, dtm, periods="day", vars=names, stats=_abi.STAT_NAMES,
                                             thresholds=thr, chunk_days=1)
    assert len(summ["periods"]) == 2 and summ["days"].tolist() == [1, 1] and summ["heights"].tolist() == list(HEIGHTS)
    for k in names:
        for n, h in enumerate(HEIGHTS):
            want, _ = SR.summarise(series[k][n], [0, 1], 2, thr[k])
            for s in _abi.STAT_NAMES:
                assert_bits(summ[k][n][s], want[s], f"{k} {s} at {h}")


def test_7_refusals_with_a_plan():
    a, kw = workload("one")
    z = np.zeros_like(a["vegp"]["pai"])
    out = [1, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    for more in (dict(), dict(stream_below=True)):
        with Plan(**dict(with_planes(a, -0.1, z, z), out=out), ring_days=2, **more) as p:
            with pytest.raises(McfError, match="error 5: mcf_plan_set_height: a below-ground plan"):
                p.set_height(0.3)
    with moving_plan(a, kw) as p:
        p.diag_enable("all")
        with pytest.raises(McfError, match="error 5: mcf_plan_set_height: the plan has diagnostics enabled"):
            p.set_height(0.3)
    with moving_plan(a, kw) as p:
        for bad, msg in ((0.0, "the ground surface"), (-0.2, "below ground: mcf_runmicro_depths"), (float("nan"), "got NaN")):
            with pytest.raises(McfError, match="error 1: mcf_plan_set_height: a height must be > 0.*" + msg):
                p.set_height(bad)
        with pytest.raises(ValueError, match="pai_a: expected 23 x 3 x 1 values"):
            p.set_height(0.3, np.zeros((5, 5)))
