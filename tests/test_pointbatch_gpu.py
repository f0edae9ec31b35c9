"""The batched point model on the device against the oracle's single-point model, point by point, under bars derived from
the oracle's own rounding sensitivity (parity_bars.py), on the batches of pointbatch_cases.py — the smallest shapes at which
each piece can go wrong: n = 24 (yearG legal and zero), 48 / 72 (the 6-hour mean wraps round the series end), 95 x 24 (the
91-day circular mean runs and wraps); P = 1, 5, 67; maxiter 20 and 100; points that stop at different iterations and points
that run to maxiter.  Plus what no oracle is needed for: a point's results do not depend on its batch, on the blocking or
on the run, bit for bit."""
import numpy as np
import pytest

import parity_bars
import pointbatch_cases as PC
from microclimf_amd import frontend as F
from microclimf_amd import pointmodel as PM

pytestmark = pytest.mark.gpu
KEYS = PC.SERIES + ("err", "iters")


def _device(b, sel=None, **kw):
    s = slice(None) if sel is None else sel
    return PM.BigLeafBatch(b["obstime"], {k: v[s] for k, v in b["clim"].items()}, b["vegp"][s], b["groundp"][s], b["soilm"][s],
                           b["lat"][s], b["lon"][s], 25.0, b["zref"], b["maxiter"], 0.5, b["tol"], b["yearG"], **kw)


def _as_want(got, want):
    return {k: np.asarray(got[k], dtype=np.float64) for k in want}


@pytest.mark.parametrize("name", [k for k in PC.BATCHES if k not in PC.PAI0])
def test_bigleaf_batch_equals_the_oracle_point_by_point(oracle, name):
    b = PC.make(name)
    want, bars, noise = parity_bars.bars_for(oracle, PC.bigleaf_run(oracle, b), ("pointbatch", name))
    assert noise["iters"] == 0.0 and max(bars.values()) < parity_bars.CAP        # admissible (pointbatch_cases.py)
    got = _device(b)
    print(name, "oracle iters", want["iters"].astype(int).tolist())
    print(name, "device iters", got["iters"].tolist())
    for k in want:
        g = np.asarray(got[k], dtype=np.float64)
        print(f"  {k:7s} distance {parity_bars.distance(g, want[k]):.3e}  bar {bars[k]:.3e}")
    assert np.array_equal(got["iters"], want["iters"].astype(np.int32))          # point by point
    parity_bars.compare(_as_want(got, want), want, bars)
    if name == "day2_p67":
        assert len(set(want["iters"].tolist())) > 1                              # points stop at different iterations
    if name == "day3_p5":
        assert (want["iters"] == b["maxiter"]).any() and (want["iters"] < b["maxiter"]).any()


def test_bigleaf_batch_with_a_bare_point_equals_the_oracle(oracle):
    """pai = 0 (the other branch of RadswabsCpp; NaN from the canopy conductance on): no bars can be derived for this batch
    (pointbatch_cases.PAI0), so the default oracle, the NaN pattern, iters and tol = 1e-6 spelled out"""
    b = PC.make("pai0_p5")
    want = PC.bigleaf_run(oracle, b)(None)
    got = _device(b)
    print("oracle iters", want["iters"].astype(int).tolist(), "device iters", got["iters"].tolist())
    for k in want:
        print(f"  {k:7s} distance {parity_bars.distance(np.asarray(got[k], dtype=np.float64), want[k]):.3e}")
    assert np.isnan(want["Tc"][2]).all() and np.isfinite(want["albedo"][2]).all()
    assert np.array_equal(got["iters"], want["iters"].astype(np.int32))
    parity_bars.compare(_as_want(got, want), want, tol=1e-6)


def _same_bits(a, b, what):
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def whole67():
    return _device(PC.make("day2_p67"))


def test_a_point_does_not_depend_on_its_batch_or_on_the_blocking(whole67):
    b = PC.make("day2_p67")
    for ppb in (2, 64):
        _same_bits(_device(b, points_per_block=ppb), whole67, f"points_per_block={ppb}")
    for k in (0, 3, 63, 64, 66):                       # first and last lanes of both waves, the clump = 0 point
        alone = _device(b, slice(k, k + 1))
        _same_bits(alone, {key: whole67[key][k:k + 1] for key in KEYS}, f"point {k} alone")


def test_two_runs_are_bit_identical(whole67):
    _same_bits(_device(PC.make("day2_p67")), whole67, "second run")


def test_a_bare_point_does_not_depend_on_its_batch():
    b = PC.make("pai0_p5")
    whole = _device(b)
    _same_bits(_device(b, slice(2, 3)), {key: whole[key][2:3] for key in KEYS}, "pai = 0 alone")
    _same_bits(_device(b, points_per_block=2), whole, "points_per_block=2")


@pytest.mark.parametrize("name", ["day1_p5", "day95_p5"])
def test_weatherhgt_batch_equals_the_oracle(oracle, name):
    """orc_weatherhgt always asks for the annual term, so one day and 95 days (mcf_weatherhgt's yearG rule is on there)"""
    b = PC.make(name)
    zin, zout = b["zref"], b["zref"] + 8.0
    want, bars, _ = parity_bars.bars_for(oracle, PC.weatherhgt_run(oracle, b, zin, zin, zout), ("pointbatch-wh", name))
    assert max(bars.values()) < parity_bars.CAP
    got = PM.weatherhgt_batch(b["obstime"], b["clim"], zin, zin, zout, b["lat"], b["lon"])
    for k in want:
        print(f"  {k:9s} distance {parity_bars.distance(got[k], want[k]):.3e}  bar {bars[k]:.3e}")
    parity_bars.compare({k: got[k] for k in want}, want, bars)
    for k in ("pres", "swdown", "difrad", "lwdown"):   # the other columns pass through
        assert np.array_equal(got[k], b["clim"][k])


def test_weatherhgt_batch_switches_the_annual_term_off_between_2_and_89_days():
    """mcf_weatherhgt's own rule (the oracle reads outside its arrays there): against the host entry, point by point, under
    the orchestration bar"""
    b = PC.make("day3_p5")
    zin, zout = b["zref"], b["zref"] + 8.0
    got = PM.weatherhgt_batch(b["obstime"], b["clim"], zin, zin, zout, b["lat"], b["lon"])
    for p in range(b["P"]):
        want = PM.weatherhgtCpp(b["obstime"], {k: v[p] for k, v in b["clim"].items()}, zin, zin, zout, b["lat"][p], b["lon"][p])
        keys = ("temp", "relhum", "windspeed")
        parity_bars.compare({k: got[k][p] for k in keys}, {k: want[k] for k in keys}, tol=1e-6)


def test_pointmprocess_batch_equals_the_oracle_chain(oracle):
    """soilmCpp -> BigLeafCpp -> pointmprocess per point through oracle/pointchain.py (which takes no `lib=`: tol = 1e-6
    spelled out); the device runs BigLeafBatch and pointmprocess_batch on the chain's soil moisture"""
    from oracle import pointchain
    b = PC.make("day3_p5")
    P, n = b["P"], b["n"]
    rng = np.random.default_rng(77)
    precip = np.where(rng.random((P, n)) < 0.1, rng.uniform(0, 5, (P, n)), 0.0)
    wants = []
    for p in range(P):
        w = {k: v[p] for k, v in b["clim"].items()}
        w["precip"] = precip[p]
        wants.append(pointchain.pointm_chain(b["obstime"], w, float(b["lat"][p]), float(b["lon"][p]), b["zref"], b["vegp"][p],
                                             b["groundp"][p], maxiter=100))
    soilm = np.stack([w[0]["soilm"] for w in wants])
    bl = PM.BigLeafBatch(b["obstime"], b["clim"], b["vegp"], b["groundp"], soilm, b["lat"], b["lon"], 25.0, b["zref"], 100, 0.5,
                         0.5, False)
    c = b["clim"]
    pp = PM.pointmprocess_batch({"windspeed": c["windspeed"], "tc": c["temp"], "rh": c["relhum"], "pk": c["pres"],
                                 "uf": bl["uf"], "soilm": soilm, "RabsG": bl["RabsG"]}, b["zref"], b["vegp"][:, 0],
                                b["vegp"][:, 1], b["groundp"][:, 4], b["groundp"][:, 5], b["groundp"][:, 6], b["groundp"][:, 7])
    for p, (want, werr) in enumerate(wants):
        got = {"soilm": soilm[p], "Tg": bl["Tg"][p], "T0p": pp["T0p"][p], "Tbp": np.zeros(n), "G": bl["G"][p], "DDp": pp["DDp"][p],
               "umu": pp["umu"][p], "kp": pp["kp"][p], "muGp": pp["muGp"][p], "dtrp": pp["dtrp"][p]}
        parity_bars.compare(got, want, tol=1e-6)
        assert abs(bl["err"][p] - werr) <= 1e-6 * (1 + abs(werr))


@pytest.mark.parametrize("reqhgt", [0.05, -0.1])
def test_runpointmodela_on_the_device_equals_the_host_loop(reqhgt):
    """the bundled site with the 2 x 3 perturbed climate grid of test_frontend_gpu.py: the cells as one batch on the device
    against one cell at a time on the host (itself pinned to the oracle at 1e-10 by the CPU tests); DESIGN section 2's
    orchestration bar"""
    from bundled import load
    weather, vegp, soilc, dtm = load(10 * 24)
    vegp = {k: (v[:, :, 6] if v.ndim == 3 else v) for k, v in vegp.items()}
    cr, cc, T = 2, 3, 240
    rng = np.random.default_rng(4)
    climarray = {}
    for k in F.WEATHER:
        base = np.broadcast_to(weather[k][None, None, :], (cr, cc, T)).copy()
        if k == "temp":
            base += rng.uniform(-1.5, 1.5, (cr, cc, 1))
        elif k in ("swdown", "difrad", "windspeed", "precip"):
            base *= rng.uniform(0.9, 1.1, (cr, cc, 1))
        elif k == "winddir":
            base = (base + rng.integers(-1, 2, (cr, cc, T)) * 10.0) % 360
        climarray[k] = np.asfortranarray(base)
    climarray["difrad"] = np.minimum(climarray["difrad"], climarray["swdown"])
    climarray["temp"][0, 1, 0] = np.nan                # ... and one cell without data
    clat = dtm["lat"] + 1e-4 * np.arange(cr)[:, None] + 0 * np.arange(cc)[None, :]
    clon = dtm["long"] + 1e-4 * np.arange(cc)[None, :] + 0 * np.arange(cr)[:, None]
    want = F.runpointmodela(climarray, weather["obstime"], reqhgt, dtm, vegp, soilc, lats=clat, lons=clon)
    got = F.runpointmodela(climarray, weather["obstime"], reqhgt, dtm, vegp, soilc, lats=clat, lons=clon, device=0)
    assert len(got) == len(want) == cr * cc
    assert [m is None for m in got] == [m is None for m in want] == [False, True, False, False, False, False]
    for g, w in zip(got, want):
        if w is None:
            continue
        parity_bars.compare(g["dfo"], w["dfo"], tol=1e-6)
        parity_bars.compare(g["weather"], w["weather"], tol=1e-6)
        assert g["zref"] == w["zref"] and g["ntme"] == w["ntme"] and g["matemp"] == w["matemp"]
        assert abs(g["bigleaf_err"] - w["bigleaf_err"]) <= 1e-6 * (1 + abs(w["bigleaf_err"]))
        if reqhgt < 0:
            parity_bars.compare({"Tbz": g["Tbz"]}, {"Tbz": w["Tbz"]}, tol=1e-6)
        else:
            assert g["Tbz"] is None and w["Tbz"] is None
