"""Inputs and oracle runs of the batched snow point model's tests (test_pointsnowbatch_cpu.py, test_pointsnowbatch_gpu.py).

A batch is P points that share `obstime` and n.  Per point, as in test_pointmodel_cpu.py::test_random_snow_point_series_equal_oracle:
weather from synthetic.workload (its own seed; start day 5 / 40 / 340, latitude 46 / 57 / 68, longitude -5 / 120, coldness 4 /
9 / 14), precipitation on 20 % of the hours (uniform 0-3 mm), a canopy of hgt 0 / 0.3 / 1.5 / 3 (pai 0.2-3, or 0 without one),
ltra 0.02-0.3, clump 0-0.5, slope 0-20, aspect 0-360, initial depth 0-0.6, initial age 0-199, one of the five snow
environments, and one zref = max hgt + 2 per batch.  Batches of five points and more carry the edge points:

    point 0   hgt = 0: no canopy, the `hgt > 0` branches of radiation and roughness are off
    point 1   hgt = 0.3 under an initial depth of 0.9: the canopy is buried (pai = hgt = 0 from the pack)
    point 2   initial depth 0
    point 3   air temperature shifted to a mean of +3 C over a 4 mm pack: the ground pack melts out (the `< 0` clamp, the
              age reset)

A batch is ADMISSIBLE when every noise variant of the oracle reports the oracle's own iteration count for every point and
no derived bar reaches parity_bars.CAP (the convergence gate is discontinuous in rounding; a seed that sits on it says
nothing about a kernel).  test_pointsnowbatch_cpu.py checks this for every batch; a seed that fails is replaced, no point
and no variable is ever excluded.
"""
import ctypes as C

import numpy as np

from microclimf_amd import synthetic
from oracle import replay_reference_tests as RT

SERIES = ("Tc", "Tg", "sdepc", "sdepg", "sdenc", "sdeng", "G", "RswabsG", "RlwabsG", "tr", "umu", "sublmelt", "tempmelt",
          "rainmelt", "sstemp")
WEATHER = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "precip")
ENVS = ("Alpine", "Maritime", "Prairie", "Tundra", "Taiga")

# name: (seed, days, P, tol, maxiter).  Seeds of the batches with edge points: the first of 94xx, 94xx + 10, ... at which the
# oracle's ground pack of point 3 does melt out (snowfall at the series' cold start usually outruns a 2 mm ground pack) and the
# batch is admissible; chosen from the oracle's output alone.
BATCHES = {
    "day1_p5": (9681, 1, 5, 0.5, 10),        # one daily mean; the 6-hour mean wraps inside one day
    "day2_p67": (9572, 2, 67, 0.5, 100),     # more than one wave and not a multiple of one; points stop at different passes
    "day3_p5": (9623, 3, 5, 0.005, 10),      # some points run to maxiter + 1 = 11 passes, others stop before
    "day12_p5": (9554, 12, 5, 0.5, 10),      # the albedo clock passes whole days without precipitation; several daily means
    "day2_p1": (9405, 2, 1, 0.5, 10),        # a single lane
}
_made = {}


def make(name):
    """The inputs of a batch: dict(obstime, clim {k: [P, n]}, vegp [P, 4], other [P, 7], snowenv [P names], tol, maxiter, n, P)"""
    if name in _made:
        return _made[name]
    seed, days, P, tol, maxiter = BATCHES[name]
    rng = np.random.default_rng(seed)
    n = days * 24
    start_doy = int(rng.choice([5, 40, 340]))
    clim = {k: np.zeros((P, n)) for k in WEATHER}
    vegp, other, env = np.zeros((P, 4)), np.zeros((P, 7)), []
    obstime = None
    for p in range(P):
        a = synthetic.workload(2, 2, n, reqhgt=0.05, start_doy=start_doy, lat=float(rng.choice([46.0, 57.0, 68.0])),
                               lon=float(rng.choice([-5.0, 120.0])), cold=float(rng.choice([4.0, 9.0, 14.0])),
                               seed=int(rng.integers(1, 1 << 30)))
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
        clim["precip"][p] = np.where(rng.random(n) < 0.2, rng.uniform(0, 3, n), 0.0)
        hgt = float(rng.choice([0.0, 0.3, 1.5, 3.0]))
        vegp[p] = [rng.uniform(0.2, 3) if hgt > 0 else 0.0, hgt, rng.uniform(0.02, 0.3), rng.uniform(0, 0.5)]
        other[p] = [rng.uniform(0, 20), rng.uniform(0, 360), a["lat"], a["lon"], 0.0, rng.uniform(0, 0.6), rng.integers(0, 200)]
        env.append(str(rng.choice(ENVS)))
    if P >= 5:
        vegp[0, 0], vegp[0, 1] = 0.0, 0.0                       # no canopy
        vegp[1, 0], vegp[1, 1], other[1, 5] = 1.2, 0.3, 0.9     # a buried canopy
        other[2, 5] = 0.0                                       # no pack to start with
        clim["temp"][3] += 3.0 - clim["temp"][3].mean()         # a thin pack that melts out
        other[3, 5] = 0.004
    other[:, 4] = vegp[:, 1].max() + 2.0                        # one zref per batch
    _made[name] = dict(obstime=obstime, clim=clim, vegp=vegp, other=other, snowenv=env, tol=tol, maxiter=maxiter, n=n, P=P)
    return _made[name]


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def point_args(b, p):
    """the single-point argument list of RT.pointmodelsnow / pointmodel.pointmodelsnow for point p of batch b"""
    clim = {k: np.ascontiguousarray(v[p]) for k, v in b["clim"].items()}
    return (b["obstime"], clim, np.ascontiguousarray(b["vegp"][p]), np.ascontiguousarray(b["other"][p]), b["snowenv"][p],
            b["tol"], b["maxiter"])


def run(O, b):
    """run(lib) for parity_bars.bars_for: orc_pointmodelsnow per point -> the fifteen series [P, n] (sdepc / sdepg
    [P, n + 1]), mxdif [P], iters [P] (as doubles)"""
    def go(lib):
        lib = O.load() if lib is None else lib
        lib.orc_pointmodelsnow.restype = C.c_int
        P, n, t = b["P"], b["n"], b["obstime"]
        res = {k: np.zeros((P, n + 1 if k in ("sdepc", "sdepg") else n)) for k in SERIES}
        res["mxdif"], res["iters"] = np.zeros(P), np.zeros(P)
        for p in range(P):
            _, clim, vegp, other, env, tol, maxiter = point_args(b, p)
            out = RT.PointSnowOut()
            rows = {k: np.zeros(res[k].shape[1]) for k in SERIES}
            for k in SERIES:
                setattr(out, k, _d(rows[k]))
            rc = lib.orc_pointmodelsnow(C.c_int(n), _i(t["year"]), _i(t["month"]), _i(t["day"]), _d(t["hour"]), _d(clim["temp"]),
                                        _d(clim["relhum"]), _d(clim["pres"]), _d(clim["swdown"]), _d(clim["difrad"]),
                                        _d(clim["lwdown"]), _d(clim["windspeed"]), _d(clim["precip"]), _d(vegp), _d(other),
                                        C.c_int(RT.SNOWENV.get(env, 0)), C.c_double(tol), C.c_double(maxiter), C.byref(out))
            assert rc == 0
            for k in SERIES:
                res[k][p] = rows[k]
            res["mxdif"][p], res["iters"][p] = out.mxdif, out.iters
        return res
    return go
