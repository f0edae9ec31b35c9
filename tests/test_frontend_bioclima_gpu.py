"""`runbioclim()` for array weather on the reference's bundled site: frontend.runbioclima under a 2 x 3 grid of perturbed
climate cells built from the whole year (so that `biosel` has twelve months) — the point model per climate cell on the
fourteen selected days, the coarse arrays interpolated inside the solver, the nineteen layers from the streamed sink —
against the same call with the expand-then-oracle solver and the oracle's terrain behind it."""
import numpy as np
import pytest

from bundled import load
from microclimf_amd import api, frontend as F

pytestmark = pytest.mark.gpu
CR, CC = 2, 3
_site = {}


def site():
    """(climarray, obstime, vegp, soilc, dtm, lats, lons, clats, clons): the climate grid of
    test_array_weather_chain_on_the_bundled_site, from the whole year"""
    if not _site:
        weather, vegp, soilc, dtm = load()
        T = len(weather["temp"])
        rng = np.random.default_rng(4)
        climarray = {}
        for k in F.WEATHER:
            base = np.broadcast_to(weather[k][None, None, :], (CR, CC, T)).copy()
            if k == "temp":
                base += rng.uniform(-1.5, 1.5, (CR, CC, 1))
            elif k in ("swdown", "difrad", "windspeed", "precip"):
                base *= rng.uniform(0.9, 1.1, (CR, CC, 1))
            elif k == "winddir":
                base = (base + rng.integers(-1, 2, (CR, CC, T)) * 10.0) % 360
            climarray[k] = np.asfortranarray(base)
        climarray["difrad"] = np.minimum(climarray["difrad"], climarray["swdown"])
        clats = dtm["lat"] + 1e-4 * np.arange(CR)[:, None] + 0 * np.arange(CC)[None, :]
        clons = dtm["long"] + 1e-4 * np.arange(CC)[None, :] + 0 * np.arange(CR)[:, None]
        lats = dtm["lat"] + 9e-6 * np.arange(50)[::-1, None] + 0 * np.arange(50)[None, :]
        lons = dtm["long"] + 1.4e-5 * np.arange(50)[None, :] + 0 * np.arange(50)[:, None]
        _site["v"] = (climarray, weather["obstime"], vegp, soilc, dtm, lats, lons, clats, clons)
    return _site["v"]


def static_vegp(vegp):
    return {k: (v[:, :, 6] if v.ndim == 3 else v) for k, v in vegp.items()}          # July's layer, time-invariant


@pytest.mark.parametrize("layered,temp", [(True, "air"), (False, "leaf")])
def test_runbioclima_on_the_bundled_site(oracle, layered, temp):
    from microclimf_amd.api import BIOCLIM_DFSEL
    from oracle import coarse_oracle as CO
    from oracle import terrain_oracle as TO
    climarray, obstime, vegp, soilc, dtm, lats, lons, clats, clons = site()
    if not layered:
        vegp = static_vegp(vegp)
    s = F.bioclima_selection(climarray, obstime)
    assert len(s["seld"]) == 14 and len(set(np.asarray(obstime["month"])[s["selh"][::24][:12]])) == 12

    def oracle_bioclim(lay, args, kw):
        assert lay == layered
        kw = dict(kw)
        clim, pm = CO.expand(args["climdata"], args["pointm"], kw.pop("rowpos"), kw.pop("colpos"))
        a = dict(args, climdata=clim, pointm=pm)
        a["lat"], a["lon"] = a.pop("lats"), a.pop("lons")
        return oracle.run_bioclim(**a, **kw, array_forcing=True, dfsel=BIOCLIM_DFSEL if lay else None)
    common = dict(lats=lats, lons=lons, clats=clats, clons=clons, temp=temp)
    got = F.runbioclima(climarray, obstime, 0.05, vegp, soilc, dtm, **common)
    assert api.bioclim_last_chunks() >= 1                                  # the streamed sink
    want = F.runbioclima(climarray, obstime, 0.05, vegp, soilc, dtm, **common, _bioclim=oracle_bioclim, _terrain=TO.terrain)
    assert list(got) == [f"bio{i}" for i in range(1, 20)]
    na = np.isnan(F.cleanvars(vegp, soilc, dtm["z"])[2])
    for k, w in want.items():
        w = np.where(na, np.nan, w)
        assert np.array_equal(np.isnan(got[k]), np.isnan(w)), k
        np.testing.assert_allclose(got[k], w, rtol=1e-8, atol=1e-8, err_msg=k)
    fin = np.isfinite(got["bio5"]) & np.isfinite(got["bio6"])
    assert fin.sum() > 2000 and (got["bio5"][fin] > got["bio6"][fin]).all()          # warmest > coldest
    assert 5 < np.nanmean(got["bio1"]) < 25
    if not layered:
        # the batched point model on the device instead of the host's, one climate cell at a time
        dev = F.runbioclima(climarray, obstime, 0.05, vegp, soilc, dtm, **common, point_device=0)
        for k in got:
            assert np.array_equal(np.isnan(dev[k]), np.isnan(got[k])), k
            np.testing.assert_allclose(dev[k], got[k], rtol=1e-8, atol=1e-8, err_msg=k)


def test_runbioclima_refusals():
    climarray, obstime, vegp, soilc, dtm, lats, lons, clats, clons = site()
    vegp = static_vegp(vegp)
    common = dict(lats=lats, lons=lons, clats=clats, clons=clons)
    with pytest.raises(ValueError, match="below ground"):
        F.runbioclima(climarray, obstime, -0.1, vegp, soilc, dtm, **common)
    with pytest.raises(ValueError, match="dtmc"):
        F.runbioclima(climarray, obstime, 0.05, vegp, soilc, dtm, **common, altcorrect=1)
    hole = {k: v.copy() for k, v in climarray.items()}
    hole["temp"][1, 2, :] = np.nan                                         # a climate cell without data: no micropoint
    with pytest.raises(ValueError, match="micropoint"):
        F.runbioclima(hole, obstime, 0.05, vegp, soilc, dtm, **common)
