"""The series sink on the device (include/mcf.h "series sink") against tests/series_ref.py on the plan's own fetch(): the mean
is an integer sum, minimum and maximum are compares, the points are copies — every comparison is bit for bit, NA payload
included.  Base shapes: 5 x 10 cells (for 21-cell tiles two full tiles and one of 8), 96 h, all ten outputs, reqhgt 0.05."""
import numpy as np
import pytest

import series_ref as ZR
import stages_cases as SC
import summary_ref as SR
from microclimf_amd import _abi, api, frontend, synthetic
from microclimf_amd.api import Plan

pytestmark = pytest.mark.gpu
ALL = _abi.OUT_NAMES
ZS = _abi.ZSTAT_NAMES
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "complete", "mat")
bits = ZR.bits
CELLS = np.arange(SC.ROWS * SC.COLS).reshape((SC.ROWS, SC.COLS), order="F")      # cell index row + rows * col
_cache = {}


def na_cell():
    hgt = np.asarray(SC.build("s170_h005")["vegp"]["hgt"])
    return int(CELLS[np.isnan(hgt)][0])


def points6():
    """the NA cell, the raster's last cell, a cell of the partial last tile of every tile size (48), and three more"""
    return [na_cell(), SC.ROWS * SC.COLS - 1, 48, 0, 17, 22]


def zone_map(which):
    if which == "one":
        return np.zeros((SC.ROWS, SC.COLS), dtype=np.int32), 1
    if which == "bands":       # rows 0-1 / 2-3 / 4 with holes, and a zone that is the NA cell alone: count 0, the rest NA
        z = np.repeat(np.array([0, 0, 1, 1, 2]), SC.COLS).reshape(SC.ROWS, SC.COLS)
        z[CELLS % 7 == 3] = -1
        z[CELLS == na_cell()] = 3
        return z.astype(np.int32), 4
    z = ((CELLS * 13) % 64).astype(np.int32)      # (50 cells reach 0 .. 61 this way: the last cell carries the table's last label)
    z[CELLS == SC.ROWS * SC.COLS - 1] = 63
    assert (z == 63).sum() == 1 and len(np.unique(z)) == 50
    return z, 64


def run_series(a, points, zones, nzones, *, ring_days, at=0, descending=False, vars=ALL, stats=ZS, upload=False, twice=False, **kw):
    """a plan with the sink over the whole series in chunks of `ring_days`, each chunk accumulated behind its run (`at`: the
    chunk lies at that day of the slot; `descending`: the last chunk first; `twice`: a reset and a second pass).
    -> ({var: points}, {(var, stat): zones}, the plan's own fetch of every variable)"""
    a = dict(a)
    dfsel = a.pop("dfsel", None)
    rows, cols = np.asarray(a["vegp"]["hgt"]).shape[:2]
    nd = len(a["obstime"]["year"]) // 24
    chunks = [(d0, min(ring_days, nd - d0)) for d0 in range(0, nd, ring_days)]
    if descending:
        chunks.reverse()
    own = {k: np.empty((rows, cols, nd * 24), order="F") for k in vars}
    with Plan(**a, ring_days=ring_days + at, dfsel=dfsel, **kw) as p:
        p.series_enable(points, zones, vars, stats, nzones=nzones)
        for rep in range(2 if twice else 1):
            if rep:
                p.series_reset()
            for d0, n in chunks:
                if upload:
                    p.upload_forcing_days(d0, n, 0)
                p.run_days_at(d0, n, 0, at) if at else p.run_days(d0, n, 0)
                p.series_accumulate(0, at, d0, n)
                for k in vars:
                    own[k][:, :, d0 * 24:(d0 + n) * 24] = p.fetch(0, k, at * 24, n * 24)
        pts = {v: p.fetch_point_series(v) for v in vars} if points is not None else {}
        zs = {(v, s): p.fetch_zone_series(v, s) for v in vars for s in stats} if zones is not None else {}
    return pts, zs, own


def assert_matches(pts, zs, own, points, zones, nzones, vars=ALL, stats=ZS):
    for v in vars:
        if points is not None:
            want = ZR.point_series(own[v], points)
            assert pts[v].shape == want.shape and pts[v].flags.f_contiguous, v
            diff = bits(pts[v]) != bits(want)
            assert not diff.any(), (v, int(diff.sum()))
        if zones is not None:
            want = ZR.zone_series(own[v], zones, nzones)
            for s in stats:
                got = zs[v, s]
                assert got.shape == want[s].shape and got.flags.f_contiguous, (v, s)
                diff = bits(got) != bits(want[s])
                assert not diff.any(), (v, s, int(diff.sum()), got[diff][:3], want[s][diff][:3])


def base(which):
    """the base case with one of the three zone maps, whole series in one chunk; made once"""
    if which not in _cache:
        z, nz = zone_map(which)
        _cache[which] = run_series(SC.build("s170_h005"), points6(), z, nz, ring_days=4)
    return _cache[which]


@pytest.mark.parametrize("which", ("one", "bands", "speckled"))
def test_1_every_statistic_of_every_output_and_every_point_equals_the_yardstick(which):
    a = SC.build("s170_h005")
    hgt, pai = np.asarray(a["vegp"]["hgt"]), np.asarray(a["vegp"]["pai"])
    assert np.isnan(hgt).any() and (~np.isnan(hgt) & (pai == 0)).any()          # an NA cell and a bare cell
    z, nz = zone_map(which)
    pts, zs, own = base(which)
    for v in ALL:                                                               # the reference case stays inside the range
        x = own[v][~np.isnan(own[v])]
        assert x.size and (np.abs(x) < ZR.LIMIT).all(), v
    assert len(pts) == 10 and len(zs) == 40
    assert_matches(pts, zs, own, points6(), z, nz)
    for v in ALL:
        assert (bits(pts[v][:, 0]) == ZR.NA_BITS).all() and np.isfinite(pts[v][:, 1:]).all(), v      # the NA cell keeps its payload
    nvalid = int((~np.isnan(hgt)).sum())
    if which == "one":
        assert (zs["Tz", "count"] == nvalid).all() and nvalid < 50 and np.isfinite(zs["Tz", "mean"]).all()
        assert (zs["Tz", "min"] <= zs["Tz", "mean"]).all() and (zs["Tz", "mean"] <= zs["Tz", "max"]).all()
    if which == "bands":
        assert (z == -1).sum() >= 5 and (z == 3).sum() == 1
        for v in ALL:
            assert (zs[v, "count"][:, 3] == 0).all(), v
            for s in ("mean", "min", "max"):
                assert (bits(zs[v, s][:, 3]) == ZR.NA_BITS).all() and np.isfinite(zs[v, s][:, :3]).all(), (v, s)


def test_2_tile_size_chunking_placement_and_day_order_do_not_matter():
    a = SC.build("s170_h005")
    z, nz = zone_map("speckled")
    rp, rz, _ = base("speckled")
    configs = [dict(ring_days=4, cells_per_block=c) for c in (16, 21, 32, 42)]
    configs += [dict(ring_days=1), dict(ring_days=3), dict(ring_days=2, at=1), dict(ring_days=1, descending=True),
                dict(ring_days=3, descending=True), dict(ring_days=2, twice=True)]
    for kw in configs:
        pts, zs, _ = run_series(a, points6(), z, nz, **kw)
        for key in rz:
            assert np.array_equal(bits(zs[key]), bits(rz[key])), (key, kw)
        for key in rp:
            assert np.array_equal(bits(pts[key]), bits(rp[key])), (key, kw)


def test_2b_state_errors_unfolded_days_and_the_tail_behind_the_last_day():
    a = dict(SC.build("s170_h005"), out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0])
    z, nz = zone_map("bands")
    E1, E5 = r"error 1: .*", r"error 5: .*"
    with Plan(**a, ring_days=2) as p:
        for call in (lambda: p.series_accumulate(0, 0, 0, 1), lambda: p.fetch_point_series("Tz"),
                     lambda: p.fetch_zone_series("Tz", "mean"), p.series_reset):
            with pytest.raises(_abi.McfError, match=E5 + "mcf_plan_series_enable first"):
                call()
        with pytest.raises(_abi.McfError, match=E1 + "mcf_plan_series_enable: .*not requested"):
            p.series_enable([0], z, ("Tz", "tleaf"))
        p.series_enable([0, 49], z, ("Tz", "soilm"), ("mean", "count"))
        with pytest.raises(_abi.McfError, match=E5 + "already enabled"):
            p.series_enable([0], None, ("Tz",))
        with pytest.raises(_abi.McfError, match=E1 + "was not selected"):
            p.fetch_zone_series("Tz", "min")
        with pytest.raises(_abi.McfError, match=E1 + "was not selected"):
            p.fetch_point_series("tleaf")
        for bad in ((1, 0, 0, 1), (0, 1, 0, 2), (0, 0, 3, 2), (0, 0, -1, 1), (0, 0, 0, 0)):       # slot, slot days, calendar days
            with pytest.raises(_abi.McfError, match=E1):
                p.series_accumulate(*bad)
        p.run_days(2, 2, 0)
        p.series_accumulate(0, 0, 2, 2)
        for again in ((0, 0, 2, 1), (0, 1, 3, 1), (0, 0, 1, 2)):
            with pytest.raises(_abi.McfError, match=E5 + "folded already"):
                p.series_accumulate(*again)
        own = p.fetch(0, "Tz", 0, 48)
        got, cnt, pts = p.fetch_zone_series("Tz", "mean"), p.fetch_zone_series("Tz", "count"), p.fetch_point_series("Tz")
        want = ZR.zone_series(own, z, nz)
        # days 0 and 1 were never folded: NA in every statistic and in the points
        assert (bits(got[:48]) == ZR.NA_BITS).all() and (bits(cnt[:48]) == ZR.NA_BITS).all() and (bits(pts[:48]) == ZR.NA_BITS).all()
        assert np.array_equal(bits(got[48:]), bits(want["mean"])) and np.array_equal(bits(cnt[48:]), bits(want["count"]))
        assert np.array_equal(bits(pts[48:]), bits(ZR.point_series(own, [0, 49])))
    # a 97-step series through the one call: step 96 belongs to no day
    b = synthetic.workload(SC.ROWS, SC.COLS, 97, variety=True, na_frac=0.05, start_doy=170)
    full = api.runmicro1Cpp(*[b[k] for k in ARGS], [1] + [0] * 9)["Tz"]
    assert full.shape[2] == 97 and np.isfinite(full[:, :, :96]).any()
    got = api.runmicro_series(*[b[k] for k in ARGS], points=[0, 49], zones=z, stats=ZS, chunk_days=3)
    want = ZR.zone_series(full[:, :, :96], z, nz)
    for s in ZS:
        assert got["zones"]["Tz"][s].shape == (97, nz) and (bits(got["zones"]["Tz"][s][96]) == ZR.NA_BITS).all(), s
        assert np.array_equal(bits(got["zones"]["Tz"][s][:96]), bits(want[s])), s
    assert (bits(got["points"]["Tz"][96]) == ZR.NA_BITS).all()
    assert np.array_equal(bits(got["points"]["Tz"][:96]), bits(ZR.point_series(full[:, :, :96], [0, 49])))
    below = dict(SC.build("s170_h005"), reqhgt=-0.05, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0])
    for kw in (dict(ring_days=4), dict(ring_days=2, stream_below=True)):
        with Plan(**below, **kw) as p:
            with pytest.raises(_abi.McfError, match=E1 + "mcf_plan_series_enable: .*" + ("streamed plan" if "stream_below" in kw else "reqhgt >= 0")):
                p.series_enable([0], None, ("Tz",))


def test_3_one_call_equals_the_plan_route_with_dfsel_and_coarse_arrays():
    z, nz = zone_map("bands")
    a = synthetic.layered(SC.build("s170_h005"), 2, cover_days=3)               # day 3 lies outside every vegetation layer
    pts, zs, own = run_series(a, points6(), z, nz, ring_days=2)
    assert (bits(own["Tz"][:, :, 72:]) == SR.NA_BITS).all() and (zs["Tz", "count"][72:] == 0).all() and (zs["Tz", "count"][:72, 0] > 0).all()
    assert_matches(pts, zs, own, points6(), z, nz)
    b = dict(a)
    dfsel = b.pop("dfsel")
    for chunk in (0, 3):
        one = api.runmicro_series(*[b[k] for k in ARGS], points=points6(), zones=z, vars=ALL, stats=ZS, chunk_days=chunk, dfsel=dfsel)
        for (v, s), plane in zs.items():
            assert np.array_equal(bits(one["zones"][v][s]), bits(plane)), (v, s, chunk)
        for v in ALL:
            assert np.array_equal(bits(one["points"][v]), bits(pts[v])), (v, chunk)
    # coarse array forcing, the existing coarse tests' inputs
    c, rp, cp = synthetic.coarse_workload(4, 6, 48, 2, 2, variety=True, na_frac=0.1, start_doy=170)
    coarse = {"rowpos": rp, "colpos": cp}
    zc = ((np.arange(24).reshape((4, 6), order="F") * 13) % 5 - 1).astype(np.int32)
    pc = [0, 23, 9]
    pts, zs, own = run_series(c, pc, zc, 4, ring_days=1, coarse=coarse)
    assert_matches(pts, zs, own, pc, zc, 4)
    one = api.runmicro_series(*[c[k] for k in ARGS], points=pc, zones=zc, vars=ALL, stats=ZS, coarse=coarse)
    for (v, s), plane in zs.items():
        assert np.array_equal(bits(one["zones"][v][s]), bits(plane)), (v, s)
    for v in ALL:
        assert np.array_equal(bits(one["points"][v]), bits(pts[v])), v
    # fine array forcing, uploaded chunk by chunk
    f = synthetic.workload(4, 6, 48, variety=True, na_frac=0.1, start_doy=170, array_forcing=True)
    pts, zs, own = run_series(f, pc, zc, 4, ring_days=1, array_forcing=True, upload=True, vars=("Tz", "relhum"))
    assert_matches(pts, zs, own, pc, zc, 4, vars=("Tz", "relhum"))
    one = api.runmicro_series(*[f[k] for k in ARGS], points=pc, zones=zc, vars=("Tz", "relhum"), stats=ZS, chunk_days=1, array_forcing=True)
    for (v, s), plane in zs.items():
        assert np.array_equal(bits(one["zones"][v][s]), bits(plane)), (v, s)


def test_3b_beside_the_period_summary_and_on_a_diagnostics_plan():
    a = dict(SC.build("s170_h005"))
    z, nz = zone_map("speckled")
    _, rz, _ = base("speckled")
    pod = [0, 1, 1, 0]
    with Plan(**a, ring_days=4) as p:
        p.diag_enable(["T0", "uf"])
        p.summary_enable(pod, ("Tz", "windspeed"), SR.STATS, 10.0)
        p.series_enable(points6(), z, ("Tz", "windspeed"), ZS)
        p.run_days(0, 4, 0)
        p.series_accumulate(0, 0, 0, 4)
        p.summary_accumulate(0, 0, 0, 4)
        for v in ("Tz", "windspeed"):
            want, _ = SR.summarise(p.fetch(0, v, 0, 96), pod, 2, 10.0)
            for s in SR.STATS:
                assert np.array_equal(bits(p.fetch_summary(v, s)), bits(want[s])), (v, s)
            for s in ZS:
                assert np.array_equal(bits(p.fetch_zone_series(v, s)), bits(rz[v, s])), (v, s)


def test_3c_front_end_on_the_bundled_site():
    from bundled import load
    weather, vegp, soilc, dtm = load()
    mx = frontend.subsetpointmodel(frontend.runpointmodel(weather, 0.05, dtm, vegp, soilc), what="tmax")
    rows, cols = np.asarray(dtm["z"]).shape
    res = dtm["res"]
    dtm = dict(dtm, xmin=1000.0, ymax=5000.0)
    zones = (np.arange(rows * cols).reshape(rows, cols) // (4 * cols)) % 16           # bands of four rows
    xy = [(1000.0 + 2.5 * res, 5000.0 - 0.5 * res), (1000.0 + (cols - 0.5) * res, 5000.0 - (rows - 0.5) * res)]
    got = frontend.runmicro_series(mx, 0.05, vegp, soilc, dtm, points=[(3, 4)], xy=xy, zones=zones, vars=("Tz", "soilm"), stats=ZS)
    assert got["cells"].tolist() == [3 + rows * 4, 0 + rows * 2, rows * cols - 1]
    full = frontend.runmicro(mx, 0.05, vegp, soilc, dtm, out=[k in ("Tz", "soilm") for k in ALL])
    for v in ("Tz", "soilm"):
        want = ZR.zone_series(full[v], zones, int(zones.max()) + 1)
        for s in ZS:
            assert np.array_equal(bits(got["zones"][v][s]), bits(want[s])), (v, s)
        assert np.array_equal(bits(got["points"][v]), bits(ZR.point_series(full[v], got["cells"]))), v
    assert np.isfinite(got["zones"]["Tz"]["mean"]).any()
    # reqhgt == 0 masks the variables as runmicro does
    g0 = frontend.runmicro_series(mx, 0.0, vegp, soilc, dtm, points=[(3, 4)], vars=("Tz", "tleaf", "windspeed"))
    assert sorted(g0["points"]) == ["Tz"] and g0["zones"] == {} and g0["points"]["Tz"].shape == (288, 1)


# ---- mcf_zonal_series on crafted arrays -----------------------------------------------------------------------------------------
def crafted():
    """7 x 37 = 259 cells x 30 steps: the cells cross a 256-lane group for every tile size, the steps are no whole number of days"""
    rng = np.random.default_rng(5)
    q = ZR.QUANTUM
    x = np.asfortranarray(np.round(rng.normal(size=(7, 37, 30)) * 40, 3))
    cell = np.arange(259)
    zone = (cell * 7) % 6                          # 0 .. 5 speckled
    zone[64:128] = 6                               # 64 cells that fill exactly one wave
    zone[258] = 7                                  # a single cell, in the second group
    zone[[5, 200, 257]] = -1
    zone = zone.reshape((7, 37), order="F").astype(np.int32)
    flat = x.reshape(259, 30, order="F")           # a view: flat[c, k]
    assert np.shares_memory(flat, x)
    one = 258
    flat[one, 3] = -0.0                            # -0.0 alone in a zone-step
    flat[one, 4], flat[one, 5] = (10 + 0.5) * q, (11 + 0.5) * q          # half-quantum ties of both parities ...
    flat[one, 6], flat[one, 7] = (-10 - 0.5) * q, (-11 - 0.5) * q        # ... and both signs
    flat[one, 13] = np.nan                         # a zone-step without a counted value
    z0 = np.flatnonzero(zone.reshape(-1, order="F") == 0)
    flat[z0[0], 6] = np.nan                        # skipped
    flat[z0[1], 6] = ZR.na_real()
    flat[np.flatnonzero(zone.reshape(-1, order="F") == 1)[0], 7] = 4096.0 - q      # counted
    flat[np.flatnonzero(zone.reshape(-1, order="F") == 2)[0], 8] = 4096.0          # bad
    flat[np.flatnonzero(zone.reshape(-1, order="F") == 3)[-1], 9] = -4096.0        # bad
    flat[np.flatnonzero(zone.reshape(-1, order="F") == 4)[0], 10] = np.inf         # bad
    flat[70, 11] = -np.inf                         # bad, in the wave of one zone
    flat[100, 12] = np.nan                         # skipped there
    flat[64:128, 14] = np.nan                      # that wave without a counted value
    flat[64:128, 15] = (np.arange(64) % 2) * -1e-300                              # -0.0 and -1e-300: ties at zero in the fixed-point sum
    flat[64:128, 16] = -0.0
    return x, zone, 8


@pytest.mark.parametrize("cpb", (16, 21, 32, 42))
def test_4_zonal_series_on_crafted_values(cpb, monkeypatch):
    monkeypatch.setenv("MCF_ZONAL_CPB", str(cpb))
    x, zone, nz = crafted()
    q = ZR.QUANTUM
    got = api.zonal_series(x, zone, ZS)
    want = ZR.zone_series(x, zone, nz)
    for s in ZS:
        assert got[s].shape == (30, nz) and got[s].flags.f_contiguous
        diff = bits(got[s]) != bits(want[s])
        assert not diff.any(), (s, np.argwhere(diff)[:5], got[s][diff][:3], want[s][diff][:3])
    NA = ZR.NA_BITS
    for s in ("mean", "min", "max"):
        assert got[s][3, 7] == 0.0 and not np.signbit(got[s][3, 7]), s                       # -0.0 alone
        assert got[s][16, 6] == 0.0 and not np.signbit(got[s][16, 6]), s                     # ... and a wave of them
        for k, z in ((8, 2), (9, 3), (10, 4), (11, 6)):                                      # bad: that zone-step alone
            assert bits(got[s])[k, z] == NA and (bits(got[s])[k, [j for j in range(nz) if j != z]] != NA).all(), (s, k, z)
        assert bits(got[s])[13, 7] == NA and bits(got[s])[14, 6] == NA, s
    assert got["mean"][4:8, 7].tolist() == [10 * q, 12 * q, -10 * q, -12 * q] and got["min"][4, 7] == 10.5 * q
    assert got["count"][13, 7] == 0 and got["count"][14, 6] == 0 and got["count"][12, 6] == 63 and got["count"][11, 6] == 63
    assert got["count"][6, 0] == (zone == 0).sum() - 2 and got["max"][7, 1] == 4096.0 - q and got["count"][8, 2] == (zone == 2).sum() - 1
    assert got["min"][15, 6] == -1e-300 and got["max"][15, 6] == 0.0 and got["mean"][15, 6] == 0.0 and got["count"][15, 6] == 64


def test_4b_many_tile_groups_fold_into_one_table():
    """300 x 300 cells x 24 h, integer values, 64 speckled zones: 90 000 cells are more tile groups than there are persistent
    workgroups, so each folds several into its table; the sums are exact, so the yardstick's mean is the true mean"""
    rng = np.random.default_rng(6)
    x = np.asfortranarray(rng.integers(-3000, 3000, size=(300, 300, 24)).astype(np.float64))
    x[rng.random((300, 300)) < 0.02] = np.nan
    zone = ((np.arange(90000) * 13) % 64).reshape((300, 300), order="F").astype(np.int32)
    got = api.zonal_series(x, zone, ZS)
    want = ZR.zone_series(x, zone, 64)
    for s in ZS:
        assert np.array_equal(bits(got[s]), bits(want[s])), s
    flat, zf = x.reshape(90000, 24, order="F"), zone.reshape(-1, order="F")
    for zz in (0, 31, 63):
        v = flat[zf == zz]
        assert (got["count"][:, zz] == (~np.isnan(v)).sum(axis=0)).all() and (got["mean"][:, zz] == np.nansum(v, axis=0) / got["count"][:, zz]).all()
