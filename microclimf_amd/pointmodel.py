"""Host-side mirror of the reference's point-model operators: `soilmCpp`, `BigLeafCpp`,
`pointmprocess`, `weatherhgtCpp` with the argument lists of R/RcppExports.R, plus `runpointmodel_chain`, the way
`runpointmodel` strings them together into the grid solver's `pointm` (R/Cppwrappers.R:119-138).

They are O(tsteps) serial series for one point and run on the host inside libmcfhip (mcf_pointmodel.cpp), as
they run on the host in the reference; the grid solver itself has no CPU path.  `BigLeafBatch`, `weatherhgt_batch`,
`pointmprocess_batch` and `pointmodelsnow_batch` run the same operators for many points at once on the device (mcf_pointbatch.hip): arrays with a
leading point axis in, the single-point wrappers' keys with a leading point axis out.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import numpy as np

from . import _abi
from .marshal import Buffers


def _vec(a, n=None, name="?"):
    v = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if n is not None and v.shape != (n,):
        raise ValueError(f"{name}: expected length {n}")
    return v


def _mat(a, shape, name):
    v = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if v.shape != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {v.shape}")
    return v


def _outputs(b: Buffers, out, fields, shape) -> dict:
    """{field: zeros of `shape` (a batch's [P, n]: one point's series after the other, C order)}, its pointer in that member of
    the struct `out`"""
    res = {}
    for f in fields:
        res[f] = np.zeros(shape(f) if callable(shape) else shape)
        setattr(out, f, b.ptr(res[f]))
    return res


def _weather(b: Buffers, climdata: Mapping, shape: tuple, need_precip: bool):
    """mcf_point_weather over series of `shape` ((n,): one point; (P, n): a batch), held by `b`; `precip` null unless it is
    needed or, for one point, given"""
    w = _abi.PointWeather()
    for f in _abi.POINT_WEATHER_FIELDS:
        if f == "precip" and not need_precip and (len(shape) == 2 or "precip" not in climdata):
            setattr(w, f, None)
            continue
        v = _vec(climdata[f], shape[0], f"climdata${f}") if len(shape) == 1 else _mat(climdata[f], shape, f"climdata${f}")
        setattr(w, f, b.ptr(v))
    return w


def _obstime(b: Buffers, obstime: Mapping, n: int):
    t = _abi.Obstime()
    for f in ("year", "month", "day"):
        setattr(t, f, b.i32_plain(obstime[f]))
    t.hour = b.ptr(_vec(obstime["hour"], n, "obstime$hour"))
    return t


def BigLeafCpp(obstime, climdata, vegp, groundp, soilm, lat, lon, dTmx=25.0, zref=2.0, maxiter=100, bwgt=0.5,
               tol=0.5, gmn=0.1, yearG=True) -> dict:
    """Drop-in for the reference's BigLeafCpp (src/microclimfCpp.cpp:710-881).  `gmn` is accepted and, as in the
    reference, unused."""
    lib = _abi.load()
    n = len(np.asarray(climdata["temp"]))
    b = Buffers()
    t, w = _obstime(b, obstime, n), _weather(b, climdata, (n,), False)
    vp, gp, sm = _vec(vegp), _vec(groundp), _vec(soilm, n, "soilm")
    if vp.size < 9 or gp.size < 12:
        raise ValueError("vegp needs >= 9 and groundp 12 entries")
    out = _abi.BigLeafOut()
    res = _outputs(b, out, _abi.BIGLEAF_FIELDS, n)
    _abi.check(lib.mcf_bigleaf(n, C.byref(t), C.byref(w), b.ptr(vp), b.ptr(gp), b.ptr(sm), float(lat),
                               float(lon), float(dTmx), float(zref), int(maxiter), float(bwgt), float(tol),
                               1 if yearG else 0, C.byref(out)))
    res["err"] = out.err
    res["iters"] = out.iters
    return res


def soilmCpp(climdata, rmu, mult, pwr, Smax, Smin, Ksat, a) -> np.ndarray:
    """Drop-in for soilmCpp (src/microclimfCpp.cpp:931-972): daily soil moisture of the two-layer bucket model."""
    lib = _abi.load()
    n = len(np.asarray(climdata["temp"]))
    b = Buffers()
    w = _weather(b, {**{f: np.zeros(n) for f in ("relhum", "pres", "difrad", "windspeed")}, **climdata}, (n,), True)
    out, optr = b.out(max(n // 24, 1), zero=True)
    nd = C.c_int64()
    _abi.check(lib.mcf_soilm(n, C.byref(w), float(rmu), float(mult), float(pwr), float(Smax), float(Smin), float(Ksat),
                             float(a), optr, C.byref(nd)))
    return out[:nd.value]


def pointmprocess(pointvars, zref, h, pai, rho, Vm, Vq, Mc) -> dict:
    """Drop-in for pointmprocess (src/microclimfCpp.cpp:5265-5323); `pointvars` has windspeed, tc, rh, pk, uf,
    soilm, RabsG."""
    lib = _abi.load()
    n = len(np.asarray(pointvars["tc"]))
    b = Buffers()
    ins = [b.ptr(_vec(pointvars[k], n, k)) for k in ("windspeed", "tc", "rh", "pk", "uf", "soilm", "RabsG")]
    res = {k: np.zeros(n) for k in ("umu", "kp", "muGp", "DDp", "T0p", "dtrp")}
    _abi.check(lib.mcf_pointmprocess(n, *ins, float(zref), float(h), float(pai), float(rho), float(Vm), float(Vq), float(Mc),
                                     *[b.ptr(v) for v in res.values()]))
    return res


def weatherhgtCpp(obstime, climdata, zin, uzin, zout, lat, lon) -> dict:
    """Drop-in for weatherhgtCpp (src/microclimfCpp.cpp:884-929): a copy of `climdata` with temp, relhum and
    windspeed moved from zin / uzin to zout."""
    lib = _abi.load()
    n = len(np.asarray(climdata["temp"]))
    b = Buffers()
    t, w = _obstime(b, obstime, n), _weather(b, climdata, (n,), False)
    res = {k: np.zeros(n) for k in ("temp", "relhum", "windspeed")}
    _abi.check(lib.mcf_weatherhgt(n, C.byref(t), C.byref(w), float(zin), float(uzin), float(zout), float(lat), float(lon),
                                  *[b.ptr(v) for v in res.values()]))
    out = {k: np.array(v, dtype=np.float64, copy=True) for k, v in climdata.items()}
    out.update(res)
    return out


# ---- many points at once, on the device (include/mcf.h: the `_batch` entries) ---------------------------------------------
def BigLeafBatch(obstime, climdata, vegp, groundp, soilm, lat, lon, dTmx=25.0, zref=2.0, maxiter=100, bwgt=0.5, tol=0.5,
                 yearG=True, *, device: int = 0, points_per_block: int = 0) -> dict:
    """BigLeafCpp for P points on device `device` (mcf_bigleaf_batch).  `climdata[k]` and `soilm`: [P, n]; `obstime`:
    shared, [n]; `vegp`: [P, >= 9]; `groundp`: [P, >= 12]; `lat`, `lon`: [P].  Whole days only (n % 24 == 0).  Returns
    BigLeafCpp's keys: the eleven series [P, n], `err` [P] and `iters` [P], each point's own."""
    lib = _abi.load()
    sm = np.ascontiguousarray(np.asarray(soilm, dtype=np.float64))
    if sm.ndim != 2:
        raise ValueError("soilm: expected [P, n]")
    P, n = sm.shape
    b = Buffers()
    t, w = _obstime(b, obstime, n), _weather(b, climdata, (P, n), False)
    vp = np.asarray(vegp, dtype=np.float64)
    gp = np.asarray(groundp, dtype=np.float64)
    if vp.ndim != 2 or gp.ndim != 2 or vp.shape[0] != P or gp.shape[0] != P or vp.shape[1] < 9 or gp.shape[1] < 12:
        raise ValueError("vegp needs [P, >= 9] and groundp [P, >= 12] entries")
    vp10 = np.zeros((P, 10))
    vp10[:, :min(vp.shape[1], 10)] = vp[:, :10]
    gp12 = np.ascontiguousarray(gp[:, :12])
    la, lo = _vec(lat, P, "lat"), _vec(lon, P, "lon")
    out = _abi.BigLeafBatchOut()
    res = _outputs(b, out, _abi.BIGLEAF_FIELDS, (P, n))
    res["err"], out.err = b.out(P, zero=True)
    res["iters"], out.iters = b.out(P, np.int32, zero=True)
    d = b.ptr
    _abi.check(lib.mcf_bigleaf_batch(P, n, C.byref(t), C.byref(w), d(vp10), d(gp12), d(sm), d(la), d(lo), float(dTmx),
                                     float(zref), int(maxiter), float(bwgt), float(tol), 1 if yearG else 0,
                                     int(points_per_block), int(device), C.byref(out)))
    return res


def weatherhgt_batch(obstime, climdata, zin, uzin, zout, lat, lon, *, device: int = 0, points_per_block: int = 0) -> dict:
    """weatherhgtCpp for P points on the device (mcf_weatherhgt_batch): a copy of `climdata` ([P, n] each) with temp,
    relhum and windspeed moved from zin / uzin to zout."""
    lib = _abi.load()
    tc = np.asarray(climdata["temp"], dtype=np.float64)
    if tc.ndim != 2:
        raise ValueError("climdata$temp: expected [P, n]")
    P, n = tc.shape
    b = Buffers()
    t, w = _obstime(b, obstime, n), _weather(b, climdata, (P, n), False)
    la, lo = _vec(lat, P, "lat"), _vec(lon, P, "lon")
    res = {k: np.zeros((P, n)) for k in ("temp", "relhum", "windspeed")}
    d = b.ptr
    _abi.check(lib.mcf_weatherhgt_batch(P, n, C.byref(t), C.byref(w), float(zin), float(uzin), float(zout), d(la), d(lo),
                                        int(points_per_block), int(device), *[d(res[k]) for k in ("temp", "relhum", "windspeed")]))
    out = {k: np.array(v, dtype=np.float64, copy=True) for k, v in climdata.items()}
    out.update(res)
    return out


def pointmprocess_batch(pointvars, zref, h, pai, rho, Vm, Vq, Mc, *, device: int = 0) -> dict:
    """pointmprocess for P points on the device (mcf_pointmprocess_batch); `pointvars` has windspeed, tc, rh, pk, uf,
    soilm, RabsG as [P, n]; h, pai, rho, Vm, Vq, Mc: [P]."""
    lib = _abi.load()
    tc = np.asarray(pointvars["tc"], dtype=np.float64)
    if tc.ndim != 2:
        raise ValueError("pointvars$tc: expected [P, n]")
    P, n = tc.shape
    ins = [_mat(pointvars[k], (P, n), k) for k in ("windspeed", "tc", "rh", "pk", "uf", "soilm", "RabsG")]
    par = [_vec(v, P, k) for k, v in (("h", h), ("pai", pai), ("rho", rho), ("Vm", Vm), ("Vq", Vq), ("Mc", Mc))]
    keys = ("umu", "kp", "muGp", "DDp", "T0p", "dtrp")
    res = {k: np.zeros((P, n)) for k in keys}
    d = Buffers().ptr
    _abi.check(lib.mcf_pointmprocess_batch(P, n, *[d(v) for v in ins], float(zref), *[d(v) for v in par], int(device),
                                           *[d(res[k]) for k in keys]))
    return res


def pointmodelsnow(obstime, climdata, vegp, other, snowenv, tol: float = 0.5, maxiter: float = 100) -> dict:
    """Drop-in for pointmodelsnow (src/microclimfCpp.cpp:4000-4169): vegp = (pai, hgt, ltra, clump), other = (slope,
    aspect, lat, lon, zref, initial snow depth, initial snow age), snowenv a name as in the reference."""
    lib = _abi.load()
    n = len(np.asarray(climdata["temp"]))
    b = Buffers()
    t, w = _obstime(b, obstime, n), _weather(b, climdata, (n,), True)
    vp, ot = _vec(vegp), _vec(other)
    if vp.size < 4 or ot.size < 7:
        raise ValueError("vegp needs 4 and other 7 entries")
    out = _abi.PointSnowOut()
    res = _outputs(b, out, _abi.POINTSNOW_FIELDS, lambda f: n + 1 if f in ("sdepc", "sdepg") else n)
    env = lib.mcf_snowenv_from_name(str(snowenv).encode())
    _abi.check(lib.mcf_pointmodelsnow(n, C.byref(t), C.byref(w), b.ptr(vp), b.ptr(ot), env, float(tol), float(maxiter), C.byref(out)))
    res["mxdif"] = out.mxdif
    res["iters"] = out.iters
    return res


def pointmodelsnow_batch(obstime, climdata, vegp, other, snowenv, tol: float = 0.5, maxiter: float = 100, *, device: int = 0,
                         points_per_block: int = 0) -> dict:
    """pointmodelsnow for P points on device `device` (mcf_pointmodelsnow_batch).  `climdata[k]`: [P, n], precip too;
    `obstime`: shared, [n]; `vegp`: [P, 4]; `other`: [P, 7]; `snowenv`: one name for every point or P names.  Whole days
    only (n % 24 == 0).  Returns pointmodelsnow's keys: thirteen series [P, n], sdepc / sdepg [P, n + 1], `mxdif` [P] and
    `iters` [P], each point's own."""
    lib = _abi.load()
    tc = np.asarray(climdata["temp"], dtype=np.float64)
    if tc.ndim != 2:
        raise ValueError("climdata$temp: expected [P, n]")
    P, n = tc.shape
    b = Buffers()
    t, w = _obstime(b, obstime, n), _weather(b, climdata, (P, n), True)
    vp = np.ascontiguousarray(np.asarray(vegp, dtype=np.float64))
    ot = np.ascontiguousarray(np.asarray(other, dtype=np.float64))
    if vp.shape != (P, 4) or ot.shape != (P, 7):
        raise ValueError("vegp needs [P, 4] and other [P, 7] entries")
    names = [snowenv] * P if isinstance(snowenv, str) else list(snowenv)
    if len(names) != P:
        raise ValueError("snowenv: one name or P names")
    env = np.array([lib.mcf_snowenv_from_name(str(s).encode()) for s in names], dtype=np.int32)
    out = _abi.PointSnowBatchOut()
    res = _outputs(b, out, _abi.POINTSNOW_FIELDS, lambda f: (P, n + 1 if f in ("sdepc", "sdepg") else n))
    res["mxdif"], out.mxdif = b.out(P, zero=True)
    res["iters"], out.iters = b.out(P, np.int32, zero=True)
    d = b.ptr
    _abi.check(lib.mcf_pointmodelsnow_batch(P, n, C.byref(t), C.byref(w), d(vp), d(ot), d(env),
                                            float(tol), float(maxiter), int(points_per_block), int(device), C.byref(out)))
    return res


def manCpp(x, n: int) -> np.ndarray:
    """Drop-in for manCpp (src/microclimfCpp.cpp:597-627)."""
    lib = _abi.load()
    b, v = Buffers(), _vec(x)
    out, optr = b.out(len(v), zero=True)
    _abi.check(lib.mcf_man(len(v), b.ptr(v), int(n), optr))
    return out


def runpointmodel_chain(obstime, weather, vegp_p, groundp_p, lat, lon, zref=2.0, soilparams=None, soilm=None,
                        dTmx=25.0, maxiter=100, yearG=True) -> dict:
    """The chain of `runpointmodel` (R/Cppwrappers.R:117-138) from a weather table to the grid solver's `pointm`:
    wind floor 0.5 m/s, soilmCpp (unless `soilm` is given; its daily values are interpolated LINEARLY to hours —
    R uses stats::spline), BigLeafCpp, pointmprocess.  Returns {"pointm": ..., "bigleaf": ..., "weather": ...}."""
    w = {k: np.array(v, dtype=np.float64, copy=True) for k, v in weather.items()}
    n = len(w["temp"])
    w["windspeed"] = np.maximum(w["windspeed"], 0.5)
    if soilm is None:
        if soilparams is None:
            raise ValueError("give soilm or soilparams (rmu, mult, pwr, Smax, Smin, Ksat, a)")
        sd = soilmCpp(w, **soilparams)
        soilm = np.interp(np.linspace(0, max(len(sd) - 1, 0), n), np.arange(len(sd)), sd)
    soilm = _vec(soilm, n, "soilm")
    bl = BigLeafCpp(obstime, w, vegp_p, groundp_p, soilm, lat, lon, dTmx, zref, maxiter, 0.5, 0.5, 0.1, yearG)
    pv = {"windspeed": w["windspeed"], "tc": w["temp"], "rh": w["relhum"], "pk": w["pres"], "uf": bl["uf"],
          "soilm": soilm, "RabsG": bl["RabsG"]}
    pp = pointmprocess(pv, zref, vegp_p[0], vegp_p[1], groundp_p[4], groundp_p[5], groundp_p[6], groundp_p[7])
    pointm = {"soilm": soilm, "Tg": bl["Tg"], "T0p": pp["T0p"], "Tbp": np.zeros(n), "G": bl["G"], "DDp": pp["DDp"],
              "umu": pp["umu"], "kp": pp["kp"], "muGp": pp["muGp"], "dtrp": pp["dtrp"]}
    return {"pointm": pointm, "bigleaf": bl, "weather": w}
