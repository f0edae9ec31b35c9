"""The batched snow point model on the device against the oracle's single-point model, point by point, under bars derived
from the oracle's own rounding sensitivity (parity_bars.py), on the batches of pointsnowbatch_cases.py — the smallest shapes
at which each piece can go wrong: one day (the 6-hour mean wraps inside it), 2 / 3 / 12 days, P = 1, 5, 67 (more than one
wave, not a multiple of one), points that stop at different passes and points that run to maxiter + 1, a bare, a buried, a
snow-free and a melting point.  Plus what no oracle is needed for: a point's results do not depend on its batch, on the
blocking or on the run, bit for bit; and `runsnowmodela(point_device=0)` against its host loop."""
import numpy as np
import pytest

import parity_bars
import pointsnowbatch_cases as SC
from microclimf_amd import frontend as F
from microclimf_amd import pointmodel as PM

pytestmark = pytest.mark.gpu
KEYS = SC.SERIES + ("mxdif", "iters")


def _device(b, sel=None, **kw):
    s = slice(None) if sel is None else sel
    return PM.pointmodelsnow_batch(b["obstime"], {k: v[s] for k, v in b["clim"].items()}, b["vegp"][s], b["other"][s],
                                   b["snowenv"][s], b["tol"], b["maxiter"], **kw)


@pytest.mark.parametrize("name", list(SC.BATCHES))
def test_snow_batch_equals_the_oracle_point_by_point(oracle, name):
    b = SC.make(name)
    want, bars, noise = parity_bars.bars_for(oracle, SC.run(oracle, b), ("pointsnowbatch", name))
    assert noise["iters"] == 0.0 and max(bars.values()) < parity_bars.CAP        # admissible (pointsnowbatch_cases.py)
    got = _device(b)
    print(name, "oracle iters", want["iters"].astype(int).tolist())
    print(name, "device iters", got["iters"].tolist())
    for k in want:
        g = np.asarray(got[k], dtype=np.float64)
        print(f"  {k:8s} distance {parity_bars.distance(g, want[k]):.3e}  bar {bars[k]:.3e}")
    assert np.array_equal(got["iters"], want["iters"].astype(np.int32))          # point by point
    parity_bars.compare({k: np.asarray(got[k], dtype=np.float64) for k in want}, want, bars)


def _same_bits(a, b, what):
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def whole67():
    return _device(SC.make("day2_p67"))


def test_a_point_does_not_depend_on_its_batch_or_on_the_blocking(whole67):
    b = SC.make("day2_p67")
    for ppb in (2, 64):
        _same_bits(_device(b, points_per_block=ppb), whole67, f"points_per_block={ppb}")
    for k in (0, 3, 63, 64, 66):                       # first and last lanes of both waves, the melting point
        alone = _device(b, slice(k, k + 1))
        _same_bits(alone, {key: whole67[key][k:k + 1] for key in KEYS}, f"point {k} alone")


def test_two_runs_are_bit_identical(whole67):
    _same_bits(_device(SC.make("day2_p67")), whole67, "second run")


def _array_weather():
    """the setup of test_snowfast_gpu.py::test_array_weather_snow_model_matches_the_oracle_chain: a 2 x 3 grid of perturbed
    cold climate cells over the bundled site, 11 days"""
    from bundled import load
    weather, vegp, soilc, dtm = load(11 * 24)
    cr, cc, T = 2, 3, 11 * 24
    rng = np.random.default_rng(9)
    climarray = {}
    for k in F.WEATHER:
        base = np.broadcast_to(weather[k][None, None, :], (cr, cc, T)).copy()
        if k == "temp":
            base += -9.0 + rng.uniform(-1.5, 1.5, (cr, cc, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (cr, cc, 1))
        elif k == "winddir":
            base = (base + rng.integers(-1, 2, (cr, cc, T)) * 10.0) % 360
        climarray[k] = np.asfortranarray(base)
    climarray["difrad"] = np.minimum(climarray["difrad"], climarray["swdown"])
    clat = dtm["lat"] + 1e-4 * np.arange(cr)[:, None] + 0 * np.arange(cc)[None, :]
    clon = dtm["long"] + 1e-4 * np.arange(cc)[None, :] + 0 * np.arange(cr)[:, None]
    lats = dtm["lat"] + 9e-6 * np.arange(50)[::-1, None] + 0 * np.arange(50)[None, :]
    lons = dtm["long"] + 1.4e-5 * np.arange(50)[None, :] + 0 * np.arange(50)[:, None]
    z = np.asarray(dtm["z"])
    dtmc = np.array([[np.nanmean(z[:25, :17]), np.nanmean(z[:25, 17:34]), np.nanmean(z[:25, 34:])],
                     [np.nanmean(z[25:, :17]), np.nanmean(z[25:, 17:34]), np.nanmean(z[25:, 34:])]]) + 40.0
    mpa = F.runpointmodela(climarray, weather["obstime"], 0.05, dtm, vegp, soilc, lats=clat, lons=clon)
    return dict(weather=weather, vegp=vegp, soilc=soilc, dtm=dtm, climarray=climarray, clat=clat, clon=clon, lats=lats, lons=lons,
                dtmc=dtmc, mpa=mpa, cr=cr, cc=cc, T=T)


@pytest.fixture(scope="module")
def array_weather():
    return _array_weather()


@pytest.mark.parametrize("method", ["slow", "fast"])
def test_runsnowmodela_on_the_device_equals_the_host_loop(array_weather, method):
    """every climate cell as one batch on the device against one cell at a time on the host (itself pinned to the oracle by
    the CPU tests): the helper's pointm_c and the six outputs under DESIGN section 2's orchestration bar, parity_bars.CAP"""
    a = array_weather
    fast = method == "fast"
    mpa = [F.subsetpointmodel(m, days=[2, 7, 8]) for m in a["mpa"]] if fast else a["mpa"]
    # the helper, as runsnowmodela calls it
    vg = F.cleanvegp(a["vegp"])
    ob = {k: np.asarray(a["weather"]["obstime"][k]) for k in ("year", "month", "day", "hour")}
    vc = {k: F.block_reduce(vg[k], a["cr"], a["cc"]) for k in ("pai", "hgt", "leaft", "clump")}
    clim_c = {k: np.array(a["climarray"][k], dtype=np.float64, order="F", copy=True) for k in F.WEATHER if k != "winddir"}
    clim_c["winddir"] = np.array([F.getmode(np.asarray(a["climarray"]["winddir"])[:, :, k]) for k in range(a["T"])])
    zref = 2.0 if fast else float(mpa[0]["zref"])
    want_p = F.snow_pointm_cells(ob, clim_c, vc, a["clat"], a["clon"], zref, 0.0, 0.0, "Taiga", fast, None)
    got_p = F.snow_pointm_cells(ob, clim_c, vc, a["clat"], a["clon"], zref, 0.0, 0.0, "Taiga", fast, 0)
    for k in want_p:
        print(f"  pointm_c {k:8s} distance {parity_bars.distance(got_p[k], want_p[k]):.3e}")
    parity_bars.compare(got_p, want_p, tol=1e-6)
    kw = dict(dtmc=a["dtmc"], lats_c=a["clat"], lons_c=a["clon"], lats=a["lats"], lons=a["lons"], method=method)
    want = F.runsnowmodela(a["climarray"], a["weather"]["obstime"], mpa, a["vegp"], a["soilc"], a["dtm"], **kw)
    got = F.runsnowmodela(a["climarray"], a["weather"]["obstime"], mpa, a["vegp"], a["soilc"], a["dtm"], point_device=0, **kw)
    assert list(got) == list(want) == ["Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden", "umu"]
    for k in want:
        print(f"  {k:16s} distance {parity_bars.distance(np.asarray(got[k]), np.asarray(want[k])):.3e}")
    parity_bars.compare({k: np.asarray(v) for k, v in got.items()}, {k: np.asarray(v) for k, v in want.items()}, tol=1e-6)
