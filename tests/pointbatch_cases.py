"""Inputs and oracle runs of the batched point model's tests (test_pointbatch_cpu.py, test_pointbatch_gpu.py).

A batch is P points that share `obstime` and n: weather from synthetic.workload per point (its own seed, latitude,
longitude and coldness), random canopies, soils, sites and one zref per batch — the generators of
test_pointmodel_cpu.py::test_random_point_model_inputs_equal_oracle.  Batches of five points and more carry the edge
points: latitude -40 with a flat site (slope 0), latitude 65, clump = 0, and sloping terrain everywhere else; the batch
"pai0_p5" has a point with pai = 0 as well (see PAI0 below for why that point has a batch of its own).

A batch is ADMISSIBLE when every noise variant of the oracle reports the oracle's own iteration count for every point and
no derived bar reaches parity_bars.CAP: the convergence gate and the |H| < 0.1 flip are discontinuous in rounding, and a
seed that sits on one says nothing about a kernel.  test_pointbatch_cpu.py checks this for every batch below (on the CPU:
it needs the oracle only); a seed that fails is replaced, no point and no variable is ever excluded.
"""
import ctypes as C

import numpy as np

from microclimf_amd import synthetic
from oracle import replay_reference_tests as RT

SERIES = ("Tc", "Tg", "H", "G", "psih", "psim", "phih", "OL", "uf", "RabsG", "albedo")
WEATHER = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed")

# name: (seed, days, P, maxiter, tol).  n = 24 (one day: yearG legal and zero), 48 and 72 (yearG off; the 6-hour mean wraps round
# the series end), 95 x 24 (the shortest series on which the 91-day circular mean runs, and it wraps); P = 1, 5 (less than a
# wave), 67 (more than one wave, not a multiple of one); maxiter 20 and 100.
BATCHES = {
    "day1_p5": (9101, 1, 5, 20, 0.5),
    "day2_p67": (9102, 2, 67, 100, 0.5),
    "day3_p5": (9103, 3, 5, 20, 0.005),      # a tight tol: two points run to maxiter
    "day95_p5": (9104, 95, 5, 100, 0.5),
    "day2_p1": (9105, 2, 1, 20, 0.5),
    "pai0_p5": (9106, 2, 5, 20, 0.5),
}
# A point with pai = 0 sits on a discontinuity BY CONSTRUCTION, not by its seed: canopy_cond divides (1 - exp(-pai)) by pai,
# 0 / 0 = NaN in the oracle, and the NaN spreads from the canopy to every series but albedo within two iterations.  The
# `ulp` noise variants move exp(-0) off 1, their quotient is +-inf, and they leave the oracle's NaN pattern — which
# parity_bars.bars_for refuses outright, whatever the seed (twenty were tried).  No bars can be derived for such a batch, so
# it is compared with the default oracle alone: identical NaN pattern, identical iters, compare(..., tol=1e-6) spelled out
# (the bound every comparison had before bars were derived).  The admissible batches above carry no pai = 0 point.
PAI0 = ("pai0_p5",)
_made = {}


def make(name):
    """The inputs of a batch: dict(obstime, clim {k: [P, n]}, vegp [P, 10], groundp [P, 12], soilm [P, n], lat, lon [P],
    zref, maxiter, tol, yearG, n, P)"""
    if name in _made:
        return _made[name]
    seed, days, P, maxiter, tol = BATCHES[name]
    rng = np.random.default_rng(seed)
    n = days * 24
    start_doy = int(rng.integers(1, 250))
    lats = rng.choice([-40.0, 10.0, 50.0, 65.0], P)
    lons = rng.choice([-5.0, 120.0], P)
    if P >= 5:
        lats[0], lats[1] = -40.0, 65.0
    clim = {k: np.zeros((P, n)) for k in WEATHER}
    vegp, groundp, soilm = np.zeros((P, 10)), np.zeros((P, 12)), np.zeros((P, n))
    obstime = None
    hmax = 0.0
    for p in range(P):
        a = synthetic.workload(2, 2, n, reqhgt=0.05, start_doy=start_doy, lat=float(lats[p]), lon=float(lons[p]),
                               cold=float(rng.choice([0.0, 10.0])), seed=int(rng.integers(1, 1 << 30)))
        c = a["climdata"]
        if obstime is None:
            obstime = {k: np.ascontiguousarray(a["obstime"][k], dtype=np.float64 if k == "hour" else np.int32)
                       for k in ("year", "month", "day", "hour")}
        else:
            assert all(np.array_equal(obstime[k], a["obstime"][k]) for k in obstime)
        clim["temp"][p] = c["temp"]
        clim["relhum"][p] = np.clip(100 * c["ea"] / c["es"], 5, 100)
        for k in ("pres", "swdown", "difrad", "lwdown"):
            clim[k][p] = c[k]
        clim["windspeed"][p] = np.maximum(c["windspeed"], 0.5)
        hgt = float(rng.uniform(0.1, 1.8))
        hmax = max(hmax, hgt)
        vegp[p] = [hgt, rng.uniform(0.2, 4), rng.uniform(0.5, 2), rng.uniform(0, 0.5), rng.uniform(0.3, 0.45),
                   rng.uniform(0.1, 0.25), rng.uniform(0.01, 0.1), 0.97, rng.uniform(0.2, 0.4), 100.0]
        groundp[p] = [rng.uniform(0.1, 0.2), rng.uniform(1, 20), rng.uniform(0, 360), 0.97, 1.53, 0.509, 0.06, 0.5422, 5.2,
                      -5.6, 0.42, 0.074]
        soilm[p] = rng.uniform(0.1, 0.4, n)
    if P >= 5:
        groundp[0, 1] = 0.0          # a flat site
        vegp[3, 3] = 0.0             # clump = 0
    if name in PAI0:
        vegp[2, 1] = 0.0             # pai = 0
    zref = float(hmax + rng.uniform(0.3, 2.0))
    _made[name] = dict(obstime=obstime, clim=clim, vegp=vegp, groundp=groundp, soilm=soilm, lat=lats, lon=lons, zref=zref,
                       maxiter=maxiter, tol=tol, yearG=days >= 90 or days == 1, n=n, P=P)
    return _made[name]


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def point_args(b, p):
    """the single-point argument list of RT.bigleaf / pointmodel.BigLeafCpp for point p of batch b"""
    clim = {k: np.ascontiguousarray(v[p]) for k, v in b["clim"].items()}
    return (b["obstime"], clim, np.ascontiguousarray(b["vegp"][p]), np.ascontiguousarray(b["groundp"][p]),
            np.ascontiguousarray(b["soilm"][p]), float(b["lat"][p]), float(b["lon"][p]), 25.0, b["zref"], b["maxiter"], 0.5,
            b["tol"], 0.1, b["yearG"])


def bigleaf_run(O, b):
    """run(lib) for parity_bars.bars_for: orc_bigleaf per point -> the eleven series [P, n], err [P], iters [P] (as doubles)"""
    def run(lib):
        lib = O.load() if lib is None else lib
        lib.orc_bigleaf.restype = C.c_int
        P, n, t = b["P"], b["n"], b["obstime"]
        res = {k: np.zeros((P, n)) for k in SERIES}
        res["err"], res["iters"] = np.zeros(P), np.zeros(P)
        for p in range(P):
            _, clim, vegp, groundp, soilm, lat, lon, dTmx, zref, maxiter, bwgt, tol, _, yearG = point_args(b, p)
            out = RT.BigLeafOut()
            rows = {k: np.zeros(n) for k in SERIES}
            for k in SERIES:
                setattr(out, k, _d(rows[k]))
            rc = lib.orc_bigleaf(C.c_int(n), _i(t["year"]), _i(t["month"]), _i(t["day"]), _d(t["hour"]), _d(clim["temp"]),
                                 _d(clim["relhum"]), _d(clim["pres"]), _d(clim["swdown"]), _d(clim["difrad"]),
                                 _d(clim["lwdown"]), _d(clim["windspeed"]), _d(vegp), _d(groundp), _d(soilm),
                                 C.c_double(lat), C.c_double(lon), C.c_double(dTmx), C.c_double(zref), C.c_int(maxiter),
                                 C.c_double(bwgt), C.c_double(tol), C.c_int(1 if yearG else 0), C.byref(out))
            assert rc == 0
            for k in SERIES:
                res[k][p] = rows[k]
            res["err"][p], res["iters"][p] = out.err, out.iters
        return res
    return run


def weatherhgt_run(O, b, zin, uzin, zout):
    """run(lib): orc_weatherhgt per point -> temp, relhum, windspeed [P, n]"""
    def run(lib):
        lib = O.load() if lib is None else lib
        lib.orc_weatherhgt.restype = C.c_int
        P, n, t = b["P"], b["n"], b["obstime"]
        res = {k: np.zeros((P, n)) for k in ("temp", "relhum", "windspeed")}
        for p in range(P):
            clim = {k: np.ascontiguousarray(v[p]) for k, v in b["clim"].items()}
            o = [np.zeros(n) for _ in range(3)]
            rc = lib.orc_weatherhgt(C.c_int(n), _i(t["year"]), _i(t["month"]), _i(t["day"]), _d(t["hour"]), _d(clim["temp"]),
                                    _d(clim["relhum"]), _d(clim["pres"]), _d(clim["swdown"]), _d(clim["difrad"]),
                                    _d(clim["lwdown"]), _d(clim["windspeed"]), C.c_double(zin), C.c_double(uzin),
                                    C.c_double(zout), C.c_double(float(b["lat"][p])), C.c_double(float(b["lon"][p])), _d(o[0]),
                                    _d(o[1]), _d(o[2]))
            assert rc == 0
            for k, v in zip(res, o):
                res[k][p] = v
        return res
    return run
