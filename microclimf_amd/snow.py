"""Host-side mirror of the reference's snow-branch operators.

`gridmodelsnow1/2` and `gridmicrosnow1/2` take the arguments of the R functions of the
same names (R/RcppExports.R:108-114, 124-130; bodies src/microclimfCpp.cpp:4172-4673,
4894-5214): R named lists / data.frames become mappings of numpy arrays, column-major,
and the returned named list becomes a dict.  All arithmetic happens in libmcfhip.so
(mcf_snow.hip); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Sequence

import numpy as np

from . import _abi
from .marshal import Buffers, SnowMarshalled, _get, alloc_outputs, build_summary_spec, marshal, summary_sink


def marshal_snow(obstime: Mapping, climdata: Mapping, vegp: Mapping, other: Mapping, array_forcing: bool,
                 pointm: Mapping | None = None, snowenv: str = "Alpine", micro: bool = False, weather: bool = True) -> SnowMarshalled:
    """Builds mcf_snow_inputs.  `pointm` (gridmodelsnow) and `micro` (gridmicrosnow: paia, leafd,
    leafden, umu, Smax) select which optional members are filled.  `weather` False: of `climdata` only `winddir` is read,
    the weather arrays stay null (the coarse snow run expands them on the device)."""
    m = SnowMarshalled()
    pai = np.asarray(vegp["pai"], dtype=np.float64)
    if pai.ndim != 2:
        raise ValueError("vegp$pai must be a rows x cols matrix")
    R, Cc = pai.shape
    T = len(np.asarray(obstime["year"]))
    m.rows, m.cols, m.tsteps = R, Cc, T
    si = m.inputs
    si.rows, si.cols, si.tsteps = R, Cc, T
    si.array_forcing = 1 if array_forcing else 0
    si.snowenv = _abi.SNOWENV.get(snowenv, 0)     # unknown names fall back to the default (cpp:3743)
    si.obstime.year = m.i32(obstime["year"], (T,), "obstime$year")
    si.obstime.month = m.i32(obstime["month"], (T,), "obstime$month")
    si.obstime.day = m.i32(obstime["day"], (T,), "obstime$day")
    si.obstime.hour = m.f64(obstime["hour"], (T,), "obstime$hour")
    fshape = (R, Cc, T) if array_forcing else (T,)
    for f in _abi.SNOW_CLIM_FIELDS:
        if (f == "umu" and not micro) or (not weather and f != "winddir"):
            setattr(si.clim, f, None)
            continue
        src = _get(climdata, *(("precip", "prec") if f == "precip" else (f,)))   # cpp:5083 reads "prec"
        setattr(si.clim, f, m.f64(src, (T,) if f == "winddir" else fshape, f"climdata${f}"))
    for f in _abi.SNOW_POINTM_FIELDS:
        setattr(si.pointm, f, m.f64(pointm[f], fshape, f"pointm${f}") if pointm is not None else None)
    for f in _abi.SNOW_VEGP_FIELDS:
        if f in ("paia", "leafd", "leafden") and not micro:
            setattr(si.vegp, f, None)
            continue
        setattr(si.vegp, f, m.f64(vegp[f], (R, Cc), f"vegp${f}"))
    o = si.other
    o.slope = m.f64(other["slope"], (R, Cc), "other$slope")
    o.aspect = m.f64(other["aspect"], (R, Cc), "other$aspect")
    o.skyview = m.f64(other["skyview"], (R, Cc), "other$skyview")
    o.wsa = m.f64(other["wsa"], (R, Cc, 8), "other$wsa")
    o.hor = m.f64(other["hor"], (R, Cc, 24), "other$hor")
    o.zref = float(other["zref"])
    if array_forcing:
        o.lats = m.f64(_get(other, "lats", "lat"), (R, Cc), "other$lats")    # cpp:4457 "lats", cpp:5091 "lat"
        o.lons = m.f64(_get(other, "lons", "lon"), (R, Cc), "other$lons")
        o.lat = o.lon = float("nan")
    else:
        o.lat, o.lon = float(other["lat"]), float(other["lon"])
        o.lats = o.lons = None
    if micro:
        o.Smax = m.f64(other["Smax"], (R, Cc), "other$Smax")
        o.isnowdc = o.isnowdg = None
        o.isnowac = o.isnowag = None
    else:
        o.Smax = None
        o.isnowdc = m.f64(other["isnowdc"], (R, Cc), "other$isnowdc")
        o.isnowdg = m.f64(other["isnowdg"], (R, Cc), "other$isnowdg")
        o.isnowac = m.i32(other["isnowac"], (R, Cc), "other$isnowac")
        o.isnowag = m.i32(other["isnowag"], (R, Cc), "other$isnowag")
    return m


def _out_arrays(out, shapes: Mapping) -> dict:
    """{member: shape} -> {member: a new column-major array}, its pointer in that member of the struct `out`, which holds the
    owner of the pointers it is given here"""
    out._owner = b = Buffers()
    arrays = {}
    for f, shape in shapes.items():
        arrays[f], ptr = b.out(shape)
        setattr(out, f, ptr)
    return arrays


def alloc_snowmodel_out(m: SnowMarshalled):
    out = _abi.SnowModelOut()
    arrays = {f: (m.rows, m.cols, m.tsteps) for f in _abi.SNOWMODEL_OUT3}
    arrays.update({f: (m.rows, m.cols) for f in _abi.SNOWMODEL_OUT2})
    return out, _out_arrays(out, arrays)


def marshal_snowm(m: SnowMarshalled, snowm: Mapping):
    s = _abi.Snowm()
    shape = (m.rows, m.cols, m.tsteps)
    for f in _abi.SNOWM_FIELDS:
        setattr(s, f, m.f64(snowm[f], shape, f"snowm${f}"))
    return s


def marshal_micro(m: SnowMarshalled, micro: Mapping, out: Sequence):
    """Copies of the requested `micro` fields (the reference updates its argument's storage and
    returns it; here the caller's arrays are left alone and the updated copies are returned)."""
    out = list(out)
    if len(out) != _abi.NOUT:
        raise ValueError("out must have 10 entries")
    sel = (C.c_int32 * _abi.NOUT)(*[1 if v else 0 for v in out])
    outs = _abi.Outputs()
    outs._owner = b = Buffers()
    arrays = {}
    shape = (m.rows, m.cols, m.tsteps)
    for v, name in enumerate(_abi.OUT_NAMES):
        if out[v]:
            arrays[name] = np.array(np.asarray(micro[name], dtype=np.float64).reshape(shape, order="F"), order="F", copy=True)
        outs.var[v] = b.ptr(arrays.get(name))
    return sel, outs, arrays


def _model(fn_name, af, obstime, climdata, pointm, vegp, other, snowenv, device):
    lib = _abi.load()
    m = marshal_snow(obstime, climdata, vegp, other, af, pointm=pointm, snowenv=snowenv)
    out, arrays = alloc_snowmodel_out(m)
    _abi.check(getattr(lib, fn_name)(C.byref(m.inputs), C.byref(out), device))
    return arrays


def gridmodelsnow1(obstime, climdata, pointm, vegp, other, snowenv, *, device: int = 0) -> dict:
    """Snowpack energy and mass balance, data.frame climate: drop-in for the reference's
    gridmodelsnow1 (src/microclimfCpp.cpp:4172-4423).  Returns Tc, Tg, sdepc, sdepg, sden
    [rows, cols, tsteps] and agec, ageg, meltc, meltg [rows, cols]."""
    return _model("mcf_gridmodelsnow1", False, obstime, climdata, pointm, vegp, other, snowenv, device)


def gridmodelsnow2(obstime, climdata, pointm, vegp, other, snowenv, *, device: int = 0) -> dict:
    """Array-climate variant: drop-in for gridmodelsnow2 (src/microclimfCpp.cpp:4426-4673)."""
    return _model("mcf_gridmodelsnow2", True, obstime, climdata, pointm, vegp, other, snowenv, device)


def _micro(fn_name, af, reqhgt, obstime, climdata, snowm, micro, vegp, other, mat, out, device):
    lib = _abi.load()
    m = marshal_snow(obstime, climdata, vegp, other, af, micro=True)
    sm = marshal_snowm(m, snowm)
    sel, outs, arrays = marshal_micro(m, micro, out)
    _abi.check(getattr(lib, fn_name)(C.byref(m.inputs), C.byref(sm), float(reqhgt), float(mat), C.byref(sel),
                                     C.byref(outs), device))
    return arrays


def gridmicrosnow1(reqhgt, obstime, climdata, snowm, micro, vegp, other, mat, out, *, device: int = 0) -> dict:
    """Microclimate of snow-covered cell-steps written over `micro`: drop-in for the reference's
    gridmicrosnow1 (src/microclimfCpp.cpp:4894-5056)."""
    return _micro("mcf_gridmicrosnow1", False, reqhgt, obstime, climdata, snowm, micro, vegp, other, mat, out,
                  device)


def gridmicrosnow2(reqhgt, obstime, climdata, snowm, micro, vegp, other, mat, out, *, device: int = 0) -> dict:
    """Array-climate variant: drop-in for gridmicrosnow2 (src/microclimfCpp.cpp:5059-5214)."""
    return _micro("mcf_gridmicrosnow2", True, reqhgt, obstime, climdata, snowm, micro, vegp, other, mat, out,
                  device)


def _terrain_placeholders(other, R, Cc) -> dict:
    """`other` with zero planes where it has no terrain: the snow drivers recompute the terrain on the device every chunk"""
    oth = dict(other)
    for k, shp in (("slope", (R, Cc)), ("aspect", (R, Cc)), ("skyview", (R, Cc)), ("wsa", (R, Cc, 8)), ("hor", (R, Cc, 24))):
        oth.setdefault(k, np.zeros(shp))
    return oth


def _driver_out(R, Cc, T):
    """-> (mcf_snowdriver_out, {name: the F-ordered [R, Cc, T] array it points to}) for the snow model's five series"""
    out = _abi.SnowDriverOut()
    return out, _out_arrays(out, {f: (R, Cc, T) for f in _abi.SNOWDRIVER_OUT})


def _driver_in(m: SnowMarshalled, dtm, res, tfact, chunk_steps: int = 0, af_wind=None, wsa_s: int = 0):
    """include/mcf.h mcf_snowdriver_in around the marshalled mcf_snow_inputs (copied as it is now); `af_wind`: the chunk wind
    series of array weather, with the wind-shelter factor `wsa_s`"""
    din = _abi.SnowDriverIn()
    din.base = m.inputs
    din.dtm = m.f64(dtm, (m.rows, m.cols), "dtm")
    din.res, din.tfact, din.chunk_steps = float(res), float(tfact), int(chunk_steps)
    if af_wind is not None:
        din.af_wsa_s = int(wsa_s)
        din.af_wind = m.f64(af_wind, (m.tsteps,), "af_wind")
    return din


def snowmodel1_chunks(obstime, climdata, pointm, vegp, other, snowenv, dtm, res, tfact=0.02, *,
                      chunk_steps: int = 120, device: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """The chunk loop of the reference's `.snowmodel1` (R/internal.R:2553-2617) resident on the
    device: per 5-day chunk terrain refresh from dtm + snow, gridmodelsnow1, `.tpicalc`
    redistribution, hand-over of depths and ages.  Arguments are what the loop works with:
    `pointm` is pointmodelsnow's output, `vegp` the snow-season means of `.sortl`, `other`
    holds lat, lon, zref and the initial isnowdc / isnowdg / isnowac / isnowag.  Returns the
    list `.snowmodel1` returns (R/internal.R:2619) minus `umu`.
    `devices` (a list of HIP ordinals, [] = all visible) / `n_blocks`: the raster in row blocks over several devices from
    this one process (include/mcf.h mcf_snowmodel1_multi); equal up to the summation order of the two raster-wide means."""
    lib = _abi.load()
    R, Cc = np.shape(vegp["pai"])
    m = marshal_snow(obstime, climdata, vegp, _terrain_placeholders(other, R, Cc), False, pointm=pointm, snowenv=snowenv)
    din = _driver_in(m, dtm, res, tfact, chunk_steps)
    out, arrays = _driver_out(R, Cc, m.tsteps)
    mu = _abi.multi(devices, n_blocks)
    if mu:
        _abi.check(lib.mcf_snowmodel1_multi(C.byref(din), C.byref(out), C.byref(mu[0])))
    else:
        _abi.check(lib.mcf_snowmodel1(C.byref(din), C.byref(out), device))
    return arrays


def snowpack_summary_spec(periods, vars=("totalSWE",), stats=("mean", "min", "max"), thresholds=None, nperiods: int | None = None):
    """include/mcf.h mcf_snowpack_summary_spec from `periods` (one integer per day, -1 = not counted; a day past the last whole
    chunk must be -1), series names of _abi.SNOWDRIVER_OUT or indices, statistics of _abi.STAT_NAMES or indices, and
    `thresholds` for hours_above: one number for every selected series or {series: number} (totalSWE with 0: the snow-cover
    duration).  -> (spec, the selected series' indices, the selected statistics' indices, the period table the spec holds)"""
    return build_summary_spec(_abi.SnowpackSummarySpec, _abi.SNOWDRIVER_OUT, "series", "snowpack summary: series", periods, vars, stats,
                              thresholds, nperiods)


def _micro_summary_spec(summary: Mapping):
    from .api import summary_spec
    sp, vi, si, pod = summary_spec(summary["periods"], summary.get("vars", ("Tz",)), summary.get("stats", ("mean", "min", "max")),
                                   summary.get("thresholds"))
    if summary.get("nperiods") is not None:
        sp.nperiods = int(summary["nperiods"])
    return sp, vi, si, pod


def _pack_summary_spec(summary: Mapping):
    return snowpack_summary_spec(summary["periods"], summary.get("vars", ("totalSWE",)), summary.get("stats", ("mean", "min", "max")),
                                 summary.get("thresholds"), summary.get("nperiods"))


def snowmodel1_summary(obstime, climdata, pointm, vegp, other, snowenv, dtm, res, tfact=0.02, *, periods, vars=("totalSWE",),
                       stats=("mean", "min", "max"), thresholds=None, nperiods: int | None = None, chunk_steps: int = 120,
                       devices=None, n_blocks: int = 0) -> dict:
    """snowmodel1_chunks with the period summaries of the five series as its only sink (include/mcf.h mcf_snowmodel1_summary):
    no [rows, cols, steps] array exists on either side.  `periods`: one integer per whole day, -1 for a day that is not counted
    and for every day past the last whole chunk.  hours_above of totalSWE with threshold 0 is the snow-cover duration, max of
    totalSWE the peak snow water equivalent.  -> {series: {statistic: [rows, cols, nperiods]}, "days": counted days per period}"""
    lib = _abi.load()
    R, Cc = np.shape(vegp["pai"])
    m = marshal_snow(obstime, climdata, vegp, _terrain_placeholders(other, R, Cc), False, pointm=pointm, snowenv=snowenv)
    din = _driver_in(m, dtm, res, tfact, chunk_steps)
    spec = snowpack_summary_spec(periods, vars, stats, thresholds, nperiods)
    so = _abi.SnowpackSummaryOut()
    planes = summary_sink(m, R, Cc, spec, _abi.SNOWDRIVER_OUT, so)
    mu = _abi.multi(devices, n_blocks)
    _abi.check(lib.mcf_snowmodel1_summary(C.byref(din), C.byref(spec[0]), C.byref(mu[0]) if mu else None, C.byref(so)))
    return planes


def snowmodel1_nc(obstime, climdata, pointm, vegp, other, snowenv, dtm, res, tfact=0.02, *, fileout: str, grid: Mapping, vars=None,
                  format: str = "classic", deflate_level: int = 0, chunk_steps: int = 120, devices=None, n_blocks: int = 0,
                  **table) -> tuple:
    """snowmodel1_chunks with the snowpack's netCDF file as its only sink (include/mcf.h mcf_snowmodel1_nc): every chunk's
    series packed on the device (k_pack_nc_planes) and written as int32 — no [rows, cols, steps] array on either side.  `vars`:
    series of _abi.SNOWDRIVER_OUT (default all five); `grid`: the mapping ncsink.writetonc takes as `dtm`; scale= / units= /
    long_name= replace entries of ncsink's SNOWPACK_* tables.  Steps past the last whole chunk hold missval.
    -> the file's series names"""
    from . import ncsink
    lib = _abi.load()
    R, Cc = np.shape(vegp["pai"])
    m = marshal_snow(obstime, climdata, vegp, _terrain_placeholders(other, R, Cc), False, pointm=pointm, snowenv=snowenv)
    din = _driver_in(m, dtm, res, tfact, chunk_steps)
    hours, east, north, crs = ncsink.grid_of(grid, obstime)
    sp, names = ncsink.ncpack_spec(R, Cc, hours, east, north, vars, crs, format, deflate_level, **table)
    mu = _abi.multi(devices, n_blocks)
    _abi.check(lib.mcf_snowmodel1_nc(C.byref(din), C.byref(mu[0]) if mu else None, str(fileout).encode(), C.byref(sp)))
    return names


def snowpack_series_spec(rows: int, cols: int, points=None, zones=None, vars=("totalSWE",), stats=("mean", "min", "max"),
                         nzones: int | None = None):
    """include/mcf.h mcf_snowpack_series_spec: api.series_spec over the five series (names of _abi.SNOWDRIVER_OUT or indices)
    -> (spec, the selected series' indices, the selected statistics' indices)"""
    from .api import series_spec
    return series_spec(rows, cols, points, zones, vars, stats, nzones, struct=_abi.SnowpackSeriesSpec, names=_abi.SNOWDRIVER_OUT,
                       field="series")


def _micro_series_spec(rows, cols, series: Mapping):
    from .api import series_spec
    return series_spec(rows, cols, series.get("points"), series.get("zones"), series.get("vars", ("Tz",)),
                       series.get("stats", ("mean", "min", "max")), series.get("nzones"))


def _pack_series_spec(rows, cols, series: Mapping):
    return snowpack_series_spec(rows, cols, series.get("points"), series.get("zones"), series.get("vars", ("totalSWE",)),
                                series.get("stats", ("mean", "min", "max")), series.get("nzones"))


def snowmodel1_series(obstime, climdata, pointm, vegp, other, snowenv, dtm, res, tfact=0.02, *, points=None, zones=None,
                      vars=("totalSWE",), stats=("mean", "min", "max"), nzones: int | None = None, chunk_steps: int = 120,
                      devices=None, n_blocks: int = 0) -> dict:
    """snowmodel1_chunks with the series sink of the five series as its only sink (include/mcf.h mcf_snowmodel1_series): the
    hourly series at `points` and per-step statistics over `zones` (as api.series_spec takes them), no [rows, cols, steps]
    array on either side.  Days past the last whole chunk are NA.
    -> {"points": {series: [tsteps, npoints]}, "zones": {series: {statistic: [tsteps, nzones]}}}"""
    from .api import _series_sink
    lib = _abi.load()
    R, Cc = np.shape(vegp["pai"])
    m = marshal_snow(obstime, climdata, vegp, _terrain_placeholders(other, R, Cc), False, pointm=pointm, snowenv=snowenv)
    din = _driver_in(m, dtm, res, tfact, chunk_steps)
    sp, vi, si = snowpack_series_spec(R, Cc, points, zones, vars, stats, nzones)
    so = _abi.SnowpackSeriesOut()
    out = _series_sink(m, m.tsteps, sp, vi, si, so, names=_abi.SNOWDRIVER_OUT)
    mu = _abi.multi(devices, n_blocks)
    _abi.check(lib.mcf_snowmodel1_series(C.byref(din), C.byref(sp), C.byref(mu[0]) if mu else None, C.byref(so)))
    return out


def _driver_in_array(obstime, climdata, pointm, vegp, other, snowenv, dtm, res, tfact, af_wind, wsa_s, chunk_steps):
    """mcf_snowdriver_in for array weather at the raster's resolution (include/mcf.h mcf_snowmodel2)"""
    R, Cc = np.shape(vegp["pai"])
    m = marshal_snow(obstime, climdata, vegp, _terrain_placeholders(other, R, Cc), True, pointm=pointm, snowenv=snowenv)
    return m, _driver_in(m, dtm, res, tfact, chunk_steps, af_wind, wsa_s)


def snowmodel2_device(obstime, climdata, pointm, vegp, other, snowenv, dtm, res, tfact=0.02, *, af_wind, wsa_s: int = 0,
                      chunk_steps: int = 120, device: int = 0) -> dict:
    """The chunk loop of `.snowmodel2` (R/internal.R:2950-3008) resident on the device, given what the loop works with: the
    climate and snow point-model arrays ALREADY at the raster's resolution ([rows, cols, T]; `climdata$winddir` [T]),
    `other` = zref, lats, lons and the initial depths / ages, `af_wind` = sqrt(wuv^2 + wvv^2) per step (the coarse wind
    components' spatial means, :2907-2908), `wsa_s` the wind-shelter factor (:2963-2964; 0: from res).  A chunk's slices are
    uploaded as the loop reaches them.  Returns `.snowmodel2`'s list minus umu (include/mcf.h mcf_snowmodel2)."""
    lib = _abi.load()
    m, din = _driver_in_array(obstime, climdata, pointm, vegp, other, snowenv, dtm, res, tfact, af_wind, wsa_s, chunk_steps)
    out, arrays = _driver_out(m.rows, m.cols, m.tsteps)
    _abi.check(lib.mcf_snowmodel2(C.byref(din), C.byref(out), device))
    return arrays


def canintfrac(hgt, pai, uf: float, prec: float, tc: float, Li: float = 0.0, *, device: int | None = None) -> np.ndarray:
    """`canintfrac` (src/microclimfCpp.cpp:5417-5450): the canopy's share of a snowfall of `prec` mm per cell.  Host code;
    `device`: that device's kernel instead (include/mcf.h mcf_canintfrac_device)"""
    lib = _abi.load()
    h = np.asfortranarray(np.asarray(hgt, dtype=np.float64))
    p = np.asfortranarray(np.asarray(pai, dtype=np.float64))
    if h.shape != p.shape:
        raise ValueError("hgt and pai differ in shape")
    b = Buffers()
    out, optr = b.out(h.shape)
    args = (C.c_int64(h.size), b.ptr(h), b.ptr(p), C.c_double(uf), C.c_double(prec), C.c_double(tc), C.c_double(Li), optr)
    _abi.check(lib.mcf_canintfrac(*args) if device is None else lib.mcf_canintfrac_device(*args, C.c_int32(device)))
    return out


def meltmu(skyview, stemp, tc, *, device: int | None = None) -> np.ndarray:
    """`meltmu` (src/microclimfCpp.cpp:5454-5492): per-cell multiplier of the point model's temperature melt.  Host code;
    `device`: that device's kernel instead (include/mcf.h mcf_meltmu_device)"""
    lib = _abi.load()
    sv = np.asfortranarray(np.asarray(skyview, dtype=np.float64))
    st = np.ascontiguousarray(stemp, dtype=np.float64)
    ta = np.ascontiguousarray(tc, dtype=np.float64)
    if st.shape != ta.shape or st.ndim != 1:
        raise ValueError("stemp and tc must be vectors of one length")
    b = Buffers()
    out, optr = b.out(sv.shape)
    args = (C.c_int64(sv.size), b.ptr(sv), C.c_int64(st.size), b.ptr(st), b.ptr(ta), optr)
    _abi.check(lib.mcf_meltmu(*args) if device is None else lib.mcf_meltmu_device(*args, C.c_int32(device)))
    return out


def tpicalc(af: int, dtm, tfact: float, *, device: int = 0) -> np.ndarray:
    """`.tpicalc(af, min(dim), dtm, tfact)` (R/internal.R:2483-2496) on the device"""
    lib = _abi.load()
    z = np.asfortranarray(np.asarray(dtm, dtype=np.float64))
    b = Buffers()
    out, optr = b.out(z.shape)
    _abi.check(lib.mcf_tpicalc(C.c_int64(z.shape[0]), C.c_int64(z.shape[1]), b.ptr(z), C.c_int32(int(af)), C.c_double(tfact), optr,
                               C.c_int32(device)))
    return out


def r_colon(a: int, b: int) -> np.ndarray:
    """R's `a:b` (counts down when a > b) as 0-based indices of 1-based positions"""
    return (np.arange(a, b + 1) if a <= b else np.arange(a, b - 1, -1)) - 1


def snowmodelq1_days(obstime, climdata, pointm, pmod, temp_all, snow_all, subs, vegp, other, snowenv, dtm, res, tfact=0.02, *,
                     device: int = 0) -> dict:
    """The day loop of the reference's fast snow method `.snowmodelq1` (R/internal.R:2690-2776).  `obstime`, `climdata`,
    `pointm`: the selected hours only (whole days); `pmod`: pointmodelsnow's output over the whole series with `temp_all`
    (air temperature) and `snow_all` (precipitation of the hours at or below 2 degC) beside it; `subs`: 1-based positions of
    the selected hours; `vegp`: `.sortl`'s means; `other`: zref, lat, lon, isnowdc, isnowac, isnowag.  Between two selected
    days the pack of every cell moves by the point model's balance, its temperature melt scaled by `meltmu`; each selected
    day runs gridmodelsnow1 on the device over terrain of the bare dtm and spreads the ground-snow change by `.tpicalc`.
    Reference behaviours kept: the ground depths stacked on the dtm for the position index are still zero when they are
    read (:2750), snow ages are not handed on, and a first selected day that is the first day of the series fails (`sbtn`
    undefined there)."""
    from . import terrain as T
    z = np.asarray(dtm, dtype=np.float64)
    subs = np.asarray(subs, dtype=np.int64)
    n = subs.size
    if n % 24 or n == 0:
        raise ValueError("the fast snow method works on whole selected days")
    if subs[0] - 1 <= 1:
        raise ValueError("the fast snow method cannot start on the first day of the series (the reference fails there: "
                         "`sbtn` not found)")
    R, Cc = z.shape
    zref = float(other["zref"])
    oth = dict(other)
    oth.update(T.snow_terrain(z, res, zref, device=device))
    temp_s = np.asarray(climdata["temp"], dtype=np.float64)
    wind_s = np.asarray(climdata["windspeed"], dtype=np.float64)
    snow_all = np.asarray(snow_all, dtype=np.float64)
    pos = snow_all[snow_all > 0]
    msnow = float(pos.mean()) if pos.size else float("nan")
    intfrac = canintfrac(vegp["hgt"], vegp["pai"], 2.0, msnow, float(temp_s.mean()), 0.0)
    isnowdc = np.array(oth["isnowdc"], dtype=np.float64)
    isnowdg = (1 - intfrac) * isnowdc
    out = {k: np.full((R, Cc, n), np.nan, order="F") for k in ("Tc", "Tg", "sdepc", "snowden")}
    out["sdepg"] = np.zeros((R, Cc, n), order="F")
    pai = np.asarray(vegp["pai"], dtype=np.float64)
    ped = 0
    with np.errstate(invalid="ignore"):
        for day in range(n // 24):
            sl = slice(day * 24, day * 24 + 24)
            first = int(subs[day * 24])
            if first - 1 > 1:
                sbtn = r_colon(ped + 1, first - 1)
                mu = meltmu(oth["skyview"], pmod["sstemp"][sbtn], np.asarray(temp_all)[sbtn])
                melt = pmod["sublmelt"][sbtn].sum() + pmod["rainmelt"][sbtn].sum() + mu * pmod["tempmelt"][sbtn].sum()
                fall = (snow_all[sbtn] / 1000).sum()
                balancec, balanceg = fall - melt, (1 - intfrac) * fall - np.exp(-pai) * melt
            else:
                balancec = balanceg = 0.0                          # sbtn of the day before stays in force
            isnowdc = isnowdc + balancec * (1000 / pmod["sdenc"][sbtn].mean())
            isnowdg = isnowdg + balanceg * (1000 / pmod["sdeng"][sbtn].mean())
            isnowdc[isnowdc < 0] = 0
            isnowdg[isnowdg < 0] = 0
            oth["isnowdc"], oth["isnowdg"] = isnowdc, isnowdg
            smod = gridmodelsnow1({k: np.asarray(v)[sl] for k, v in obstime.items()},
                                  {k: np.asarray(v)[sl] for k, v in climdata.items()},
                                  {k: np.asarray(v)[sl] for k, v in pointm.items()}, vegp, oth, snowenv, device=device)
            dsnow = smod["sdepc"] - isnowdc[:, :, None]
            dsnowg = smod["sdepg"] - isnowdg[:, :, None]
            af = int(np.round(10 * wind_s[sl].mean() ** 0.5 / res))    # half to even, like R's round
            tpi = tpicalc(af, z, tfact, device=device)
            dsnowg2 = dsnowg * tpi[:, :, None]
            sdc = (dsnow - dsnowg) + dsnowg2 + isnowdc[:, :, None]
            sdg = dsnowg2 + isnowdg[:, :, None]
            sdc[sdc < 0] = 0
            sdg[sdg < 0] = 0
            out["Tc"][:, :, sl], out["Tg"][:, :, sl], out["snowden"][:, :, sl] = smod["Tc"], smod["Tg"], smod["sden"]
            out["sdepc"][:, :, sl], out["sdepg"][:, :, sl] = sdc, sdg
            ped = int(subs[day * 24 + 23])
            isnowdc, isnowdg = sdc[:, :, 23].copy(), sdg[:, :, 23].copy()
        swe = out["sdepc"] * out["snowden"]
    return {"Tc": out["Tc"], "Tg": out["Tg"], "groundsnowdepth": out["sdepg"], "totalSWE": swe, "snowden": out["snowden"]}


def marshal_snowfast(obstime, climdata, pointm, pmod, temp_all, snow_all, subs, vegp, other, snowenv, dtm, res, tfact):
    """-> (the marshalling that keeps the arrays alive, mcf_snowfast_in) for `snowmodelq1`'s arguments"""
    R, Cc = np.shape(vegp["pai"])
    oth = _terrain_placeholders(other, R, Cc)
    oth.setdefault("isnowdg", np.zeros((R, Cc)))
    m = marshal_snow(obstime, climdata, vegp, oth, False, pointm=pointm, snowenv=snowenv)
    o = m.inputs.other                                          # ignored by the entry (isnowdg is formed on the device)
    o.slope = o.aspect = o.skyview = o.wsa = o.hor = o.isnowdg = None
    fin = _abi.SnowFastIn()
    fin.drv = _driver_in(m, dtm, res, tfact)
    n_all = len(np.asarray(temp_all))
    if np.size(subs) != m.tsteps:
        raise ValueError("subs must name every selected hour")
    fin.n_all, fin.subs = n_all, m.i64(subs)
    whole = dict(pmod, temp_all=temp_all, snow_all=snow_all)
    for k in _abi.SNOWFAST_SERIES:
        v = np.ascontiguousarray(whole[k], dtype=np.float64)
        if v.ndim != 1 or v.size < n_all:
            raise ValueError(f"{k}: expected the whole series ({n_all} hours), got shape {v.shape}")
        setattr(fin, k, m.ptr(v))
    return m, fin


def _wanted_series(m: SnowMarshalled, series, every: tuple, out) -> dict:
    """The series a one-call entry returns (`series` None: `every` one): an array [rows, cols, tsteps] each, its pointer in
    the entry's out struct; the others stay null, so the library neither finishes nor downloads them"""
    names = every if series is None else tuple(series)
    if not names or any(k not in every for k in names):
        raise ValueError(f"series: names out of {every}")
    return _out_arrays(out, {k: (m.rows, m.cols, m.tsteps) for k in every if k in names})


def snowmodelq1(obstime, climdata, pointm, pmod, temp_all, snow_all, subs, vegp, other, snowenv, dtm, res, tfact=0.02, *,
                device: int = 0, series: Sequence[str] | None = None) -> dict:
    """`snowmodelq1_days` as ONE device-resident call (include/mcf.h mcf_snowmodelq1): the same arguments, the same list.  The
    terrain, the step table and `intfrac` are made once on the device, each selected day's gap balance, grid model, position
    index and redistribution run there, and only the wanted series come back, a day's while the next day computes.
    `series`: the names to return (default all five: Tc, Tg, groundsnowdepth, totalSWE, snowden); the others are neither
    finished nor downloaded.  What the library refuses (a first selected day that is the series' first day, broken days,
    `subs` out of range) raises _abi.McfError with its message."""
    lib = _abi.load()
    m, fin = marshal_snowfast(obstime, climdata, pointm, pmod, temp_all, snow_all, subs, vegp, other, snowenv, dtm, res, tfact)
    out = _abi.SnowDriverOut()
    arrays = _wanted_series(m, series, _abi.SNOWDRIVER_OUT, out)
    _abi.check(lib.mcf_snowmodelq1(C.byref(fin), C.byref(out), device))
    return arrays


def coarse_wind(windspeed, winddir):
    """The wind of coarse array weather as the snow branch uses it (R/internal.R:2905-2908): the components of each coarse cell
    [crows, ccols, T] from speed and direction (degrees), their spatial means over the cells that have one, and from the means
    the one direction per step [T] and the chunk wind series `af_wind` = sqrt(wuv^2 + wvv^2) [T].  The device entries and the
    host loops they are compared with bit for bit all take these from here.  -> (wu_c, wv_c, winddir, af_wind)"""
    wd = np.asarray(winddir, dtype=np.float64) * np.pi / 180
    wu_c = np.asarray(windspeed, dtype=np.float64) * np.cos(wd)
    wv_c = np.asarray(windspeed, dtype=np.float64) * np.sin(wd)
    wuv, wvv = np.nanmean(wu_c, axis=(0, 1)), np.nanmean(wv_c, axis=(0, 1))
    return wu_c, wv_c, (np.arctan2(wvv, wuv) * 180 / np.pi) % 360, np.sqrt(wuv ** 2 + wvv ** 2)


def _fine_snow_inputs(clim_c, pointm_c, sl, z, zc, rowpos, colpos, altcorrect, wu_c, wv_c, winddir):
    """Steps `sl` of the coarse climate and snow point-model arrays on the fine raster, as `.snowmodel2` / `.snowmodelq2`
    prepare them (R/internal.R:2862-2925, 3108-3170): `.cca` = bilinear and masked by the dtm, pressure and wind
    components unmasked, altitude correction 0 / 1 / 2, relative humidity capped at 100"""
    from .rformulas import lapserate_R, satvap_R, upsample_coarse
    hole = np.isnan(z)
    up = lambda a: upsample_coarse(np.asarray(a)[:, :, sl], rowpos, colpos)            # noqa: E731
    cca = lambda a: np.where(hole[:, :, None], np.nan, up(a))                          # noqa: E731
    temp, relhum = cca(clim_c["temp"]), cca(clim_c["relhum"])
    if altcorrect == 0:
        pres = up(clim_c["pres"])
    else:
        ea = satvap_R(temp) * relhum / 100
        pres = up(np.asarray(clim_c["pres"]) / (((293 - 0.0065 * zc) / 293) ** 5.26)[:, :, None]) * (((293 - 0.0065 * z) / 293) ** 5.26)[:, :, None]
        elevd = (upsample_coarse(zc, rowpos, colpos) - z)[:, :, None]
        lr = 5 / 1000 if altcorrect == 1 else lapserate_R(temp, ea, pres)
        temp = lr * elevd + temp
        relhum = (ea / satvap_R(temp)) * 100
    relhum = np.where(relhum > 100, 100.0, relhum)
    clim = {"temp": temp, "relhum": relhum, "pres": pres, "swdown": cca(clim_c["swdown"]), "difrad": cca(clim_c["difrad"]),
            "lwdown": cca(clim_c["lwdown"]), "precip": cca(clim_c["precip"]),
            "windspeed": np.sqrt(up(wu_c) ** 2 + up(wv_c) ** 2), "winddir": winddir[sl]}
    return clim, {k: cca(pointm_c[k]) for k in ("Gp", "Tc", "RswabsG", "RlwabsG", "umu", "tr")}


MICRO_WEATHER = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "winddir", "precip")


def _fine_micro_inputs(clim_c, umu_c, sl, z, zc, rowpos, colpos, altcorrect):
    """Steps `sl` of the coarse weather of the snow-day microclimate on the fine raster, as `.prepsnowinputs2` prepares it
    (R/internal.R:3445-3579) — NOT `.snowmodel2`'s weather: temperature and pressure resampled unmasked, relative humidity from
    the resampled vapour pressure and kept within 20 .. 100 % in every altitude mode, the wind from each coarse cell's own
    direction, one direction per step from the components' means.  `clim_c[k]`: [crows, ccols, T] (winddir too), `umu_c` the
    point model's umu, `zc` the coarse dtm with NA read as 0 (read with altcorrect > 0 only) -> gridmicrosnow2's `climdata`.
    The host statement of what `expand_micro_coarse` computes on the device."""
    from .rformulas import lapserate_R, satvap_R, upsample_coarse
    hole = np.isnan(z)
    up = lambda a: upsample_coarse(a, rowpos, colpos)                                          # noqa: E731
    cca = lambda a: np.where(hole[:, :, None], np.nan, up(a))                                  # noqa: E731
    wc = {k: np.asarray(clim_c[k])[:, :, sl] for k in MICRO_WEATHER}
    with np.errstate(invalid="ignore"):
        ea = up(satvap_R(wc["temp"]) * (wc["relhum"] / 100))
        temp = up(wc["temp"])
        if altcorrect == 0:
            pres = up(wc["pres"])
        else:
            pres = up(wc["pres"] / (((293 - 0.0065 * zc[:, :, None]) / 293) ** 5.26)) * (((293 - 0.0065 * z[:, :, None]) / 293) ** 5.26)
            elevd = (up(zc) - z)[:, :, None]
            temp = (5 / 1000 if altcorrect == 1 else lapserate_R(temp, ea, pres)) * elevd + temp
        relhum = np.clip((ea / satvap_R(temp)) * 100, 20.0, 100.0)
        wu, wv, winddir, _ = coarse_wind(wc["windspeed"], wc["winddir"])
        return {"temp": temp, "relhum": relhum, "pres": pres, "swdown": cca(wc["swdown"]), "difrad": cca(wc["difrad"]),
                "lwdown": cca(wc["lwdown"]), "windspeed": np.sqrt(up(wu) ** 2 + up(wv) ** 2),
                "winddir": winddir,
                "precip": cca(wc["precip"]), "umu": cca(np.asarray(umu_c)[:, :, sl])}


def micro_coarse_arrays(clim_c, umu_c) -> dict:
    """The ten coarse arrays mcf_microcoarse_in takes, formed on the climate grid with `_fine_micro_inputs`' own expressions:
    the vapour pressure and the wind components of each coarse cell's own direction; the rest as given"""
    from .rformulas import satvap_R
    f = lambda k: np.asarray(clim_c[k], dtype=np.float64)                                    # noqa: E731
    windu, windv = coarse_wind(clim_c["windspeed"], clim_c["winddir"])[:2]
    a = {k: f(k) for k in ("temp", "pres", "swdown", "difrad", "lwdown", "precip")}
    a.update(ea=satvap_R(f("temp")) * (f("relhum") / 100), windu=windu, windv=windv, umu=np.asarray(umu_c, dtype=np.float64))
    return a


def marshal_microcoarse(clim_c, umu_c, dtm, dtmc, rowpos, colpos, altcorrect=0):
    """-> (the marshalling that keeps the arrays alive, mcf_microcoarse_in, the one wind direction per step [T]) for the coarse
    weather of the snow-day microclimate (`_fine_micro_inputs`' arguments)"""
    z = np.asarray(dtm, dtype=np.float64)
    R, Cc = z.shape
    arrays = micro_coarse_arrays(clim_c, umu_c)
    cr, cc, n = arrays["temp"].shape
    m = SnowMarshalled()
    m.rows, m.cols, m.tsteps = R, Cc, n
    mi = _abi.MicroCoarseIn()
    mi.rows, mi.cols, mi.tsteps = R, Cc, n
    mi.dtm = m.f64(z, (R, Cc), "dtm")
    mi.coarse_rows, mi.coarse_cols, mi.altcorrect = cr, cc, int(altcorrect)
    mi.coarse_rowpos = m.f64(rowpos, (R,), "rowpos")
    mi.coarse_colpos = m.f64(colpos, (Cc,), "colpos")
    mi.coarse_dtm = m.f64(dtmc, (cr, cc), "dtmc") if dtmc is not None else None
    for k in _abi.MICRO_COARSE:
        setattr(mi, k, m.f64(arrays[k], (cr, cc, n), k))
    with np.errstate(invalid="ignore"):
        return m, mi, coarse_wind(clim_c["windspeed"], clim_c["winddir"])[2]


def expand_micro_coarse(clim_c, umu_c, dtm, dtmc, *, rowpos, colpos, altcorrect: int = 0, step0: int = 0, nsteps: int | None = None,
                        series: Sequence[str] | None = None, out: Mapping | None = None, device: int = 0) -> dict:
    """Steps step0 .. step0 + nsteps - 1 (default: to the end) of the snow-day microclimate's coarse weather on the fine raster by
    the expansion kernel alone (include/mcf.h mcf_microsnow_expand_coarse_device) -> gridmicrosnow2's `climdata` as
    `_fine_micro_inputs` returns it: nine series [rows, cols, nsteps] and `winddir` [nsteps].  `series`: the names to expand (the
    kernel's series mask; default all nine); `out`: arrays [rows, cols, nsteps] (Fortran order) to write into — the ones that are
    not asked for are left as they are."""
    lib = _abi.load()
    m, mi, winddir = marshal_microcoarse(clim_c, umu_c, dtm, dtmc, rowpos, colpos, altcorrect)
    n = m.tsteps - step0 if nsteps is None else int(nsteps)
    names = _abi.MICRO_FINE_SERIES if series is None else tuple(series)
    if not names or any(k not in _abi.MICRO_FINE_SERIES for k in names):
        raise ValueError(f"series: names out of {_abi.MICRO_FINE_SERIES}")
    shape = (m.rows, m.cols, max(n, 0))
    fine, ptrs = {}, (_abi.c_double_p * 9)()
    for i, k in enumerate(_abi.MICRO_FINE_SERIES):
        if out is not None and k in out:
            a = out[k]
            if a.shape != shape or a.dtype != np.float64 or not a.flags.f_contiguous:
                raise ValueError(f"out[{k!r}] must be a Fortran-ordered float64 array {shape}")
            fine[k] = a
        elif k in names:
            fine[k] = np.empty(shape, dtype=np.float64, order="F")
        if k in names:
            ptrs[i] = m.ptr(fine[k])
    _abi.check(lib.mcf_microsnow_expand_coarse_device(C.byref(mi), C.c_int64(step0), C.c_int64(n), ptrs, device))
    clim = {k: fine[k] for k in _abi.MICRO_FINE_SERIES if k in fine}
    clim["winddir"] = winddir[step0:step0 + n]
    return clim


def meltmu2(mu, stemp, tc) -> np.ndarray:
    """`meltmu2` (src/microclimfCpp.cpp:5495-5527): as `meltmu` with the snow surface and air temperatures given per
    cell [rows, cols, n]; 0.5 where the surface never thaws (host code)"""
    lib = _abi.load()
    m = np.asfortranarray(np.asarray(mu, dtype=np.float64))
    st = np.asfortranarray(np.asarray(stemp, dtype=np.float64))
    ta = np.asfortranarray(np.asarray(tc, dtype=np.float64))
    if st.shape != ta.shape or st.shape[:2] != m.shape:
        raise ValueError("stemp and tc must be [rows, cols, n] over mu's raster")
    b = Buffers()
    out, optr = b.out(m.shape)
    _abi.check(lib.mcf_meltmu2(C.c_int64(m.size), C.c_int64(st.shape[2]), b.ptr(m), b.ptr(st), b.ptr(ta), optr))
    return out


def snowmodelq2_days(obstime, clim_c, pointm_c, pm2_c, subs, vegp, other, snowenv, dtm, dtmc, res, tfact=0.02, *, rowpos, colpos,
                     altcorrect: int = 0, device: int = 0) -> dict:
    """The second half of the reference's fast array-weather snow method `.snowmodelq2` (R/internal.R:3108-3283).
    `obstime`, `clim_c`, `pointm_c`: the selected hours (coarse arrays as for `snowmodel2_chunks`); `pm2_c`: coarse arrays
    over the WHOLE series — sublmelt, tempmelt, rainmelt, snow, sstemp, tc, sdenc, sdeng; `subs`: 1-based positions of the
    selected hours.  Between two selected days each cell's pack moves by the resampled point-model balance (`meltmu2`
    scaling the temperature melt by sky view), each selected day runs gridmodelsnow2 on terrain of the bare dtm and
    spreads the ground-snow change by `.tpicalc`.  Unlike `.snowmodelq1` a first selected day that is the first day of
    the series is accepted (no adjustment then)."""
    from . import terrain as T
    from .rformulas import upsample_coarse
    z = np.asarray(dtm, dtype=np.float64)
    hole = np.isnan(z)
    R, Cc = z.shape
    subs = np.asarray(subs, dtype=np.int64)
    n = subs.size
    if n % 24 or n == 0:
        raise ValueError("the fast snow method works on whole selected days")
    zc = np.nan_to_num(np.asarray(dtmc, dtype=np.float64), nan=0.0)
    wu_c, wv_c, winddir, af_wind = coarse_wind(clim_c["windspeed"], clim_c["winddir"])
    oth = dict(other)
    oth.update(T.snow_terrain(z, res, float(other["zref"]), device=device))
    vg = dict(vegp)
    vg["leaft"] = np.where(np.isnan(vg["leaft"]), 0.01, vg["leaft"])
    pai = np.asarray(vg["pai"], dtype=np.float64)
    up = lambda a: upsample_coarse(a, rowpos, colpos)                                      # noqa: E731
    cca = lambda a: np.where(hole[:, :, None], np.nan, up(a))                              # noqa: E731
    snow_c = np.asarray(pm2_c["snow"], dtype=np.float64)
    pos = snow_c[snow_c > 0]
    msnow = float(pos.mean()) if pos.size else float("nan")
    mtemp = float(np.nanmean(cca(pm2_c["tc"])))
    intfrac = canintfrac(vg["hgt"], vg["pai"], 2.0, msnow, mtemp, 0.0)
    isnowdc = np.array(oth["isnowdc"], dtype=np.float64)
    isnowdg = (1 - intfrac) * isnowdc
    names = ("Tc", "Tg", "sdepc", "snowden", "umu")
    out = {k: np.full((R, Cc, n), np.nan, order="F") for k in names}
    out["sdepg"] = np.zeros((R, Cc, n), order="F")
    ped = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for day in range(n // 24):
            sl = slice(day * 24, day * 24 + 24)
            first = int(subs[day * 24])
            if first - 1 > 1:
                sbtn = r_colon(ped + 1, first - 1)
                tot = lambda k: up(np.asarray(pm2_c[k])[:, :, sbtn].sum(axis=2))          # noqa: E731  `.resamplemelt`
                mu = meltmu2(oth["skyview"], cca(np.asarray(pm2_c["sstemp"])[:, :, sbtn]), cca(np.asarray(pm2_c["tc"])[:, :, sbtn]))
                melt = tot("sublmelt") + tot("rainmelt") + mu * tot("tempmelt")
                fall = tot("snow") / 1000
                isnowdc = isnowdc + (fall - melt) * (1000 / (tot("sdenc") / sbtn.size))
                isnowdg = isnowdg + ((1 - intfrac) * fall - np.exp(-pai) * melt) * (1000 / (tot("sdeng") / sbtn.size))
            isnowdc[isnowdc < 0] = 0
            isnowdg[isnowdg < 0] = 0
            oth["isnowdc"], oth["isnowdg"] = isnowdc, isnowdg
            clim, pointm = _fine_snow_inputs(clim_c, pointm_c, sl, z, zc, rowpos, colpos, altcorrect, wu_c, wv_c, winddir)
            smod = gridmodelsnow2({k: np.asarray(v)[sl] for k, v in obstime.items()}, clim, pointm, vg, oth, snowenv, device=device)
            dsnow = smod["sdepc"] - isnowdc[:, :, None]
            dsnowg = smod["sdepg"] - isnowdg[:, :, None]
            af = int(np.round(10 * np.mean(af_wind[sl]) ** 0.5 / res))
            tpi = tpicalc(af, z, tfact, device=device)
            dsnowg2 = dsnowg * tpi[:, :, None]
            sdc = (dsnow - dsnowg) + dsnowg2 + isnowdc[:, :, None]
            sdg = dsnowg2 + isnowdg[:, :, None]
            sdc[sdc < 0] = 0
            sdg[sdg < 0] = 0
            out["Tc"][:, :, sl], out["Tg"][:, :, sl], out["snowden"][:, :, sl] = smod["Tc"], smod["Tg"], smod["sden"]
            out["sdepc"][:, :, sl], out["sdepg"][:, :, sl], out["umu"][:, :, sl] = sdc, sdg, pointm["umu"]
            ped = int(subs[day * 24 + 23])
            isnowdc, isnowdg = sdc[:, :, 23].copy(), sdg[:, :, 23].copy()
        res_ = {"Tc": out["Tc"], "Tg": out["Tg"], "groundsnowdepth": out["sdepg"], "totalSWE": out["sdepc"] * out["snowden"],
                "snowden": out["snowden"], "umu": out["umu"]}
    for v in res_.values():                                             # `.cleansmod`
        v[hole] = np.nan
    return res_


def _marshal_coarse(cin, clim_c, pointm_c, dtm, dtmc, rowpos, colpos, altcorrect):
    """What the array-weather entries' input structs (mcf_snowfast2_in, mcf_snowcoarse_in) share, formed as the host loops form
    it: sizes, dtm, the coarse grid's geometry and dtm, the fourteen coarse arrays with the wind as components, and from the
    components' spatial means the one direction per step and `af_wind` -> (the marshalling, the direction per step)"""
    z = np.asarray(dtm, dtype=np.float64)
    R, Cc = z.shape
    cr, cc, n = np.shape(clim_c["temp"])
    m = SnowMarshalled()
    m.rows, m.cols, m.tsteps = R, Cc, n
    wu_c, wv_c, winddir, af_wind = coarse_wind(clim_c["windspeed"], clim_c["winddir"])
    si = cin.drv.base
    si.rows, si.cols, si.tsteps, si.array_forcing = R, Cc, n, 1
    cin.drv.dtm = m.f64(z, (R, Cc), "dtm")
    cin.drv.af_wind = m.f64(af_wind, (n,), "af_wind")
    cin.coarse_rows, cin.coarse_cols, cin.altcorrect = cr, cc, int(altcorrect)
    cin.coarse_rowpos = m.f64(rowpos, (R,), "rowpos")
    cin.coarse_colpos = m.f64(colpos, (Cc,), "colpos")
    cin.coarse_dtm = m.f64(dtmc, (cr, cc), "dtmc") if dtmc is not None else None
    arrays = dict(clim_c, windu=wu_c, windv=wv_c, **{k: pointm_c[k] for k in ("Gp", "Tc", "RswabsG", "RlwabsG", "umu")})
    for k in _abi.SNOWFAST2_SELECTED:
        setattr(cin, k, m.f64(arrays[k], (cr, cc, n), k))
    return m, winddir


def _marshal_model(m: SnowMarshalled, si, obstime, winddir, vegp, other, snowenv, leaft_fill: float, isnowdg: bool):
    """The point model's side of an array-weather entry's mcf_snow_inputs: snowenv, obstime, the direction per step, `.sortl`'s
    vegetation (`leaft` NA -> leaft_fill: `.snowmodelq2` and `.snowmodel2` differ in it) and `other` (isnowdg: whether the entry
    reads it)"""
    R, Cc, n = m.rows, m.cols, m.tsteps
    si.snowenv = _abi.SNOWENV.get(snowenv, 0)
    si.obstime.year = m.i32(obstime["year"], (n,), "obstime$year")
    si.obstime.month = m.i32(obstime["month"], (n,), "obstime$month")
    si.obstime.day = m.i32(obstime["day"], (n,), "obstime$day")
    si.obstime.hour = m.f64(obstime["hour"], (n,), "obstime$hour")
    si.clim.winddir = m.f64(winddir, (n,), "winddir")
    for f in ("pai", "hgt", "leaft", "clump"):
        v = np.asarray(vegp[f], dtype=np.float64)
        setattr(si.vegp, f, m.f64(np.where(np.isnan(v), leaft_fill, v) if f == "leaft" else v, (R, Cc), f"vegp${f}"))
    o = si.other
    o.zref = float(other["zref"])
    o.lat = o.lon = float("nan")
    o.lats = m.f64(_get(other, "lats", "lat"), (R, Cc), "other$lats")
    o.lons = m.f64(_get(other, "lons", "lon"), (R, Cc), "other$lons")
    o.isnowdc = m.f64(other["isnowdc"], (R, Cc), "other$isnowdc")
    if isnowdg:
        o.isnowdg = m.f64(other["isnowdg"], (R, Cc), "other$isnowdg")
    o.isnowac = m.i32(other["isnowac"], (R, Cc), "other$isnowac")
    o.isnowag = m.i32(other["isnowag"], (R, Cc), "other$isnowag")


def marshal_snowfast2(obstime, clim_c, pointm_c, pm2_c, subs, vegp, other, snowenv, dtm, dtmc, res, tfact, rowpos, colpos, altcorrect=0):
    """-> (the marshalling that keeps the arrays alive, mcf_snowfast2_in) for `snowmodelq2`'s arguments: the coarse arrays
    stay coarse; the wind components, the one direction per hour and `af_wind` are formed here as `snowmodelq2_days` forms them"""
    cr, cc, n = np.shape(clim_c["temp"])
    if np.size(subs) != n or len(np.asarray(obstime["year"])) != n:
        raise ValueError("subs and obstime must name every selected hour")
    fin = _abi.SnowFast2In()
    m, winddir = _marshal_coarse(fin, clim_c, pointm_c, dtm, dtmc, rowpos, colpos, altcorrect)
    _marshal_model(m, fin.drv.base, obstime, winddir, vegp, other, snowenv, 0.01, False)
    fin.drv.res, fin.drv.tfact = float(res), float(tfact)
    n_all = np.shape(pm2_c["tc"])[2]
    fin.n_all, fin.subs = n_all, m.i64(subs)
    for k in _abi.SNOWFAST2_SERIES:
        setattr(fin, k, m.f64(pm2_c[k], (cr, cc, n_all), k))
    return m, fin


def snowmodelq2(obstime, clim_c, pointm_c, pm2_c, subs, vegp, other, snowenv, dtm, dtmc, res, tfact=0.02, *, rowpos, colpos,
                altcorrect: int = 0, device: int = 0, series: Sequence[str] | None = None) -> dict:
    """`snowmodelq2_days` as ONE device-resident call (include/mcf.h mcf_snowmodelq2): the same arguments, the same six-entry
    list.  The coarse arrays are uploaded once and stay coarse; the terrain, the date table and `intfrac` are made once on the
    device, each selected day's gap balance (meltmu2 of the resampled temperatures fused with the resampled balance), the day's
    thirteen series on the raster, the grid model, the position index and the redistribution run there, and only the wanted
    series come back, a day's while the next day computes.  `series`: the names to return (default all six: Tc, Tg,
    groundsnowdepth, totalSWE, snowden, umu); the others are neither finished nor downloaded.  What the library refuses raises
    _abi.McfError with its message."""
    lib = _abi.load()
    m, fin = marshal_snowfast2(obstime, clim_c, pointm_c, pm2_c, subs, vegp, other, snowenv, dtm, dtmc, res, tfact, rowpos, colpos,
                               altcorrect)
    out = _abi.SnowFast2Out()
    arrays = _wanted_series(m, series, _abi.SNOWFAST2_OUT, out)
    _abi.check(lib.mcf_snowmodelq2(C.byref(fin), C.byref(out), device))
    return arrays


def meltmu2_coarse(skyview, dtm, sstemp_c, tc_c, rowpos, colpos, device: int = 0) -> np.ndarray:
    """`meltmu2` of coarse snow-surface and air temperatures [crows, ccols, n] resampled to the raster inside the kernel
    (include/mcf.h mcf_meltmu2_device): what `snowmodelq2` runs per gap; the dtm's holes mask the resampled series"""
    lib = _abi.load()
    sv = np.asfortranarray(np.asarray(skyview, dtype=np.float64))
    z = np.asfortranarray(np.asarray(dtm, dtype=np.float64))
    st = np.asfortranarray(np.asarray(sstemp_c, dtype=np.float64))
    ta = np.asfortranarray(np.asarray(tc_c, dtype=np.float64))
    rp, cp = np.ascontiguousarray(rowpos, dtype=np.float64), np.ascontiguousarray(colpos, dtype=np.float64)
    if st.shape != ta.shape or st.ndim != 3 or sv.shape != z.shape or rp.shape != (z.shape[0],) or cp.shape != (z.shape[1],):
        raise ValueError("sstemp_c and tc_c must be [crows, ccols, n], skyview and dtm one raster with a position per row and column")
    b = Buffers()
    out, p = b.out(z.shape)[0], b.ptr
    _abi.check(lib.mcf_meltmu2_device(C.c_int64(z.shape[0]), C.c_int64(z.shape[1]), p(sv), p(z), C.c_int64(st.shape[0]),
                                      C.c_int64(st.shape[1]), p(rp), p(cp), C.c_int64(st.shape[2]), p(st), p(ta), p(out),
                                      C.c_int32(device)))
    return out


def snowmodel2_chunks(obstime, clim_c, pointm_c, vegp, other, snowenv, dtm, dtmc, res, tfact=0.02, *, rowpos, colpos,
                      altcorrect: int = 0, agg: int = 10, chunk_steps: int = 120, device: int = 0) -> dict:
    """The second half of the reference's `.snowmodel2` (R/internal.R:2862-3013): coarse climate and snow point-model
    arrays [crows, ccols, T] brought to the fine raster chunk by chunk (bilinear, `.cca`; altitude correction 0 / 1 / 2 of
    :2871-2890; wind from resampled components), then per 5-day chunk the terrain of dtm + ground snow, gridmodelsnow2
    and `.tpicalc` on the device, the redistribution and the hand-over of depths and ages.  `clim_c`: temp, relhum, pres,
    swdown, difrad, lwdown, precip, windspeed [crows, ccols, T] and winddir [T] (degrees, the same in every cell as `.todf`
    makes it); `pointm_c`: Gp, Tc, RswabsG, RlwabsG, umu, tr; `vegp`: `.sortl`'s means; `other`: zref, lats, lons, isnowdc,
    isnowdg, isnowac, isnowag.  Reference behaviours kept: `other$isnowdg` is never updated, the aggregation factor of the
    position index is at least 2, `1:n5days` truncates.  The device-resident form of this loop is `snowmodel2_coarse`."""
    from . import terrain as T
    from .rformulas import upsample_coarse
    z = np.asarray(dtm, dtype=np.float64)
    R, Cc = z.shape
    h = len(np.asarray(obstime["year"]))
    nch = h // chunk_steps
    if nch < 1:
        raise ValueError("the array snow model needs at least one whole 5-day chunk")
    hole = np.isnan(z)
    zc = np.nan_to_num(np.asarray(dtmc, dtype=np.float64), nan=0.0)
    wu_c, wv_c, winddir, af_wind = coarse_wind(clim_c["windspeed"], clim_c["winddir"])
    names = ("Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden", "umu")
    out = {k: np.full((R, Cc, h), np.nan, order="F") for k in names}
    oth = dict(other)
    vg = dict(vegp)
    vg["leaft"] = np.where(np.isnan(vg["leaft"]), 0.001, vg["leaft"])
    isnowdg = np.asarray(other["isnowdg"], dtype=np.float64)
    dtms = z + isnowdg
    with np.errstate(invalid="ignore"):
        for ch in range(nch):
            sl = slice(ch * chunk_steps, min((ch + 1) * chunk_steps, h))
            oth.update(T.snow_terrain(dtms, res, float(other["zref"]), agg=agg, mask=z, device=device))
            clim, pointm = _fine_snow_inputs(clim_c, pointm_c, sl, z, zc, rowpos, colpos, altcorrect, wu_c, wv_c, winddir)
            smod = gridmodelsnow2({k: np.asarray(v)[sl] for k, v in obstime.items()}, clim, pointm, vg, oth, snowenv, device=device)
            af = max(int(np.round(10 * np.mean(af_wind[sl]) ** 0.5 / res)), 2)
            tpi = tpicalc(af, dtms, tfact, device=device)[:, :, None]
            asd = isnowdg[:, :, None]
            dsnow = smod["sdepg"] - asd
            dsnow2 = np.where(dsnow < 0, dsnow, dsnow * tpi)
            asc = np.asarray(oth["isnowdc"], dtype=np.float64)[:, :, None]
            tot = asc + (smod["sdepc"] - asc - dsnow) + dsnow2
            out["Tc"][:, :, sl], out["Tg"][:, :, sl], out["snowden"][:, :, sl] = smod["Tc"], smod["Tg"], smod["sden"]
            out["totalSWE"][:, :, sl] = tot * smod["sden"]
            out["groundsnowdepth"][:, :, sl] = asd + dsnow2
            out["umu"][:, :, sl] = pointm["umu"]                       # `umu = pointm$umu`
            oth["isnowdc"] = tot[:, :, -1]
            oth["isnowac"], oth["isnowag"] = smod["agec"], smod["ageg"]
            dtms = z + out["groundsnowdepth"][:, :, sl.stop - 1]
    tail = slice(nch * chunk_steps, h)                                  # steps past the last whole chunk: only umu is filled
    if tail.start < h:
        out["umu"][:, :, tail] = upsample_coarse(np.asarray(pointm_c["umu"])[:, :, tail], rowpos, colpos)
    for k in names:                                                     # `.cleansmod`
        out[k][hole] = np.nan
    return out


def marshal_snowcoarse(obstime, clim_c, pointm_c, vegp, other, snowenv, dtm, dtmc, res, tfact, rowpos, colpos, altcorrect=0, agg=10,
                       chunk_steps=120):
    """-> (the marshalling that keeps the arrays alive, mcf_snowcoarse_in, the one wind direction per step) for
    `snowmodel2_coarse`'s arguments: the coarse arrays stay coarse; the wind components, the direction and `af_wind` are formed
    here exactly as `snowmodel2_chunks` forms them.  `obstime` / `vegp` / `other` None: only what the expansion reads"""
    cin = _abi.SnowCoarseIn()
    m, winddir = _marshal_coarse(cin, clim_c, pointm_c, dtm, dtmc, rowpos, colpos, altcorrect)
    if obstime is None:
        return m, cin, winddir
    if len(np.asarray(obstime["year"])) != m.tsteps:
        raise ValueError("obstime must name every step of the coarse arrays")
    _marshal_model(m, cin.drv.base, obstime, winddir, vegp, other, snowenv, 0.001, True)
    cin.drv.res, cin.drv.tfact, cin.drv.chunk_steps = float(res), float(tfact), int(chunk_steps)
    cin.drv.af_wsa_s = int(agg)
    return m, cin, winddir


def snowmodel2_coarse(obstime, clim_c, pointm_c, vegp, other, snowenv, dtm, dtmc, res, tfact=0.02, *, rowpos, colpos,
                      altcorrect: int = 0, agg: int = 10, chunk_steps: int = 120, series: Sequence[str] | None = None,
                      device: int = 0) -> dict:
    """`snowmodel2_chunks` as ONE device-resident call (include/mcf.h mcf_snowmodel2_coarse): the same arguments, the same
    six-entry list.  The fourteen coarse arrays are uploaded once and stay coarse; per chunk one kernel expands the chunk's
    thirteen series on the raster into the buffers the snow kernel reads, and the chunk loop of `snowmodel2_device` (terrain
    refresh, gridmodelsnow2, position index, redistribution, hand-over) runs on them; only the wanted series come back.
    `series`: the names to return (default all six: Tc, Tg, groundsnowdepth, totalSWE, snowden, umu), as for `snowmodelq2`.
    Unlike the host loop a series shorter than one chunk runs as one short chunk (the library's `1:n5days`).  What the library
    refuses raises _abi.McfError with its message."""
    lib = _abi.load()
    m, cin, _ = marshal_snowcoarse(obstime, clim_c, pointm_c, vegp, other, snowenv, dtm, dtmc, res, tfact, rowpos, colpos, altcorrect, agg,
                                   chunk_steps)
    out = _abi.SnowFast2Out()
    arrays = _wanted_series(m, series, _abi.SNOWFAST2_OUT, out)
    _abi.check(lib.mcf_snowmodel2_coarse(C.byref(cin), C.byref(out), device))
    return arrays


def expand_coarse(clim_c, pointm_c, dtm, dtmc, *, rowpos, colpos, altcorrect: int = 0, step0: int = 0, nsteps: int | None = None,
                  device: int = 0):
    """Steps step0 .. step0 + nsteps - 1 (default: to the end) of the coarse climate and snow point-model arrays on the fine
    raster by the chunk kernel of `snowmodel2_coarse` alone (include/mcf.h mcf_snow_expand_coarse_device): -> (clim, pointm)
    as `_fine_snow_inputs` returns them (without `tr`), [rows, cols, nsteps] each and `winddir` [nsteps] — what
    `snowmodel2_device` takes"""
    lib = _abi.load()
    m, cin, winddir = marshal_snowcoarse(None, clim_c, pointm_c, None, None, None, dtm, dtmc, 1.0, 0.0, rowpos, colpos, altcorrect)
    n = m.tsteps - step0 if nsteps is None else int(nsteps)
    fine, ptrs = {}, (_abi.c_double_p * 13)()
    for i, k in enumerate(_abi.SNOW_FINE_SERIES):
        fine[k], ptrs[i] = m.out((m.rows, m.cols, max(n, 0)))
    _abi.check(lib.mcf_snow_expand_coarse_device(C.byref(cin), C.c_int64(step0), C.c_int64(n), ptrs, device))
    clim = {k: fine[k] for k in _abi.SNOW_FINE_SERIES[:8]}
    clim["winddir"] = winddir[step0:step0 + n]
    return clim, {k: fine[k] for k in _abi.SNOW_FINE_SERIES[8:]}


APPLY_FUNS ={"mean": 0, "sum": 1, "max": 2, "min": 3}


def applycpp3(a, fun_name: str, *, device: int = 0, with_count: bool = False):
    """Reduction over space per time step, NA skipped: drop-in for the reference's applycpp3
    (src/microclimfCpp.cpp:5553-5588).  `with_count=True` also returns the non-NA cell counts
    (what a row-block rank contributes to a raster-wide mean, see distributed.allreduce_apply3)."""
    if fun_name not in APPLY_FUNS:
        raise ValueError("Unknown function name")           # the reference's stop() message
    lib = _abi.load()
    arr = np.asfortranarray(np.asarray(a, dtype=np.float64))
    if arr.ndim != 3:
        raise ValueError("applycpp3 needs a [rows, cols, tsteps] array")
    R, Cc, T = arr.shape
    b = Buffers()
    res, cnt = np.empty(T), np.empty(T) if with_count else None
    _abi.check(lib.mcf_applycpp3(b.ptr(arr), R, Cc, T, APPLY_FUNS[fun_name], b.ptr(res), b.ptr(cnt), device))
    return (res, cnt) if with_count else res


def snowdaysfun(maxsnowdepth, minsnowdepth) -> dict:
    """Host-side mirror of the reference's snowdaysfun (src/microclimfCpp.cpp:5531-5550): a day is a
    snow day if any hour has snow somewhere (max > 0) and a no-snow day if any hour has a snow-free
    cell (min == 0); a day can be both."""
    mx = np.asarray(maxsnowdepth, dtype=np.float64)
    mn = np.asarray(minsnowdepth, dtype=np.float64)
    days = mx.size // 24
    with np.errstate(invalid="ignore"):
        snow = (mx[:days * 24].reshape(days, 24) > 0.0).any(axis=1)
        nosnow = (mn[:days * 24].reshape(days, 24) == 0.0).any(axis=1)
    return {"snowdays": snow.astype(np.int32), "nosnowdays": nosnow.astype(np.int32)}


def merge_snow_outputs(moutn: Mapping, mouts: Mapping, snowdays, nosnowdays, rows: int, cols: int) -> dict:
    """Step (5) of `.runmicrosnow1/2` (R/internal.R:3633-3656): days with snow anywhere take the snow
    microclimate (`mouts`, which already carries the no-snow solver's values on its snow-free cell-steps),
    the other days the no-snow solver's output (`moutn`).  `snowdays` / `nosnowdays` are 1-based day
    numbers as in R; `moutn` covers `nosnowdays` in order, `mouts` covers `snowdays` in order."""
    snowdays = np.asarray(snowdays, dtype=np.int64)
    nosnowdays = np.asarray(nosnowdays, dtype=np.int64)
    if nosnowdays.size == 0:
        return dict(mouts)
    if snowdays.size == 0:
        return dict(moutn)
    tdays = np.unique(np.concatenate([snowdays, nosnowdays]))
    nosnow = np.setdiff1d(tdays, snowdays)
    s1 = np.repeat(np.isin(nosnowdays, nosnow), 24)
    hours = np.arange(24)
    nosnowh = (np.repeat((nosnow - 1) * 24, 24) + np.tile(hours, nosnow.size)).astype(np.int64)
    snowh = (np.repeat((snowdays - 1) * 24, 24) + np.tile(hours, snowdays.size)).astype(np.int64)
    n = nosnowh.size + snowh.size
    out = {}
    for k, v in moutn.items():
        a = np.full((rows, cols, n), np.nan, order="F")
        a[:, :, nosnowh] = np.asarray(v)[:, :, s1]
        a[:, :, snowh] = np.asarray(mouts[k])
        out[k] = a
    return out


class SnowPlan:
    """One rank's row block of `.snowmodel1`'s chunk loop, resident on the device (include/mcf.h
    mcf_snowplan_*).  Arguments as snowmodel1_chunks, for the block's own rows; `row0` / `rows_total`
    place the block in the raster."""

    def __init__(self, obstime, climdata, pointm, vegp, other, snowenv, dtm, res, tfact=0.02, *, chunk_steps=120,
                 row0=0, rows_total=0, device=0, keep_results=True):
        self._lib = _abi.load()
        R, Cc = np.shape(vegp["pai"])
        self._m = marshal_snow(obstime, climdata, vegp, _terrain_placeholders(other, R, Cc), False, pointm=pointm, snowenv=snowenv)
        din = _driver_in(self._m, dtm, res, tfact, chunk_steps)
        self._p = C.c_void_p()
        _abi.check(self._lib.mcf_snowplan_create(C.byref(din), int(row0), int(rows_total), device, C.byref(self._p)))
        self.rows, self.cols, self.tsteps = R, Cc, self._m.tsteps
        self.device = int(device)
        self.chunks = int(self._lib.mcf_snowplan_chunks(self._p))
        self._chunk_steps = int(chunk_steps) if chunk_steps else 120
        # keep_results=False: the series stay on the device (null pointers, no [rows, cols, tsteps] host arrays)
        self._out, self.result = _driver_out(R, Cc, self.tsteps) if keep_results else (_abi.SnowDriverOut(), {})

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self._lib.mcf_snowplan_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def surface(self, out=None) -> np.ndarray:
        """dtm + ground snow depth of the own rows; `out`: a column-major [rows, cols] array to fill (reused across chunks)"""
        a = np.empty((self.rows, self.cols), dtype=np.float64, order="F") if out is None else out
        if a.shape != (self.rows, self.cols) or not a.flags.f_contiguous:
            raise ValueError("out must be a column-major [rows, cols] array")
        _abi.check(self._lib.mcf_snowplan_surface(self._p, Buffers().ptr(a)))
        return a

    def handover(self) -> np.ndarray:
        """The pack depth handed to the next chunk (`other$isnowdc`), own rows."""
        a, ptr = Buffers().out((self.rows, self.cols))
        _abi.check(self._lib.mcf_snowplan_handover(self._p, ptr))
        return a

    def apply3(self, chunk: int, fun_name: str):
        """applycpp3 of the chunk's totalSWE on the device: (result, non-NA counts), each [steps of the chunk]"""
        fun = {"mean": 0, "sum": 1, "max": 2, "min": 3}[fun_name]
        n = min(self._chunk_steps, self.tsteps - chunk * self._chunk_steps)
        (r, rp), (c, cp) = Buffers().out(n), Buffers().out(n)
        _abi.check(self._lib.mcf_snowplan_apply3(self._p, int(chunk), fun, rp, cp))
        return r, c

    def surface_partial(self):
        s, n = C.c_double(), C.c_double()
        _abi.check(self._lib.mcf_snowplan_surface_partial(self._p, C.byref(s), C.byref(n)))
        return s.value, n.value

    def prepare_chunk(self, chunk: int, ext=None, halo_north: int = 0, halo_south: int = 0, surface_mean: float = 0.0):
        s, n = C.c_double(), C.c_double()
        p = None
        if ext is not None:
            e = np.asfortranarray(np.asarray(ext, dtype=np.float64))
            if e.shape != (halo_north + self.rows + halo_south, self.cols):
                raise ValueError("ext must be [halo_north + rows + halo_south, cols]")
            p = Buffers().ptr(e)
        _abi.check(self._lib.mcf_snowplan_prepare_chunk(self._p, int(chunk), p, int(halo_north), int(halo_south),
                                                        float(surface_mean), C.byref(s), C.byref(n)))
        return s.value, n.value

    def pack_halo(self, north=None, south=None):
        """The own block's first / last surface rows into DEVICE tensors `north` [cols, h] / `south` (torch, float64, contiguous:
        the memory is a column-major [h, cols] piece) — what the neighbouring ranks receive as their halos.  No host staging."""
        hn, pn = _dev_piece(north, self.cols)
        hs, ps = _dev_piece(south, self.cols)
        _abi.check(self._lib.mcf_snowplan_pack_halo(self._p, hn, pn, hs, ps))

    def prepare_chunk_dev(self, chunk: int, north=None, south=None, surface_mean: float = 0.0):
        """prepare_chunk with the halo pieces as device tensors ([cols, h], as pack_halo writes them)."""
        hn, pn = _dev_piece(north, self.cols)
        hs, ps = _dev_piece(south, self.cols)
        s, n = C.c_double(), C.c_double()
        _abi.check(self._lib.mcf_snowplan_prepare_chunk_dev(self._p, int(chunk), pn, hn, ps, hs, float(surface_mean), C.byref(s),
                                                            C.byref(n)))
        return s.value, n.value

    def run_chunk(self, chunk: int, tpic_mean: float):
        _abi.check(self._lib.mcf_snowplan_run_chunk(self._p, int(chunk), float(tpic_mean), C.byref(self._out)))

    # ---- period summaries of the five series (include/mcf.h mcf_snowplan_summary_*) --------------------------------------
    def summary_enable(self, periods, vars=("totalSWE",), stats=("mean", "min", "max"), thresholds=None, nperiods: int | None = None):
        """arguments as snowpack_summary_spec; the state is allocated here"""
        self._psum = snowpack_summary_spec(periods, vars, stats, thresholds, nperiods)
        _abi.check(self._lib.mcf_snowplan_summary_enable(self._p, C.byref(self._psum[0])))

    def summary_accumulate(self, chunk: int):
        """folds the series of the chunk run last (after run_chunk, before keep_chunk): ascending chunks, each once"""
        _abi.check(self._lib.mcf_snowplan_summary_accumulate(self._p, int(chunk)))

    def summary_reset(self):
        _abi.check(self._lib.mcf_snowplan_summary_reset(self._p))

    def fetch_summary(self) -> dict:
        """-> {series: {statistic: [rows, cols, nperiods]}, "days": counted days per period}"""
        return summary_sink(Buffers(), self.rows, self.cols, self._psum, _abi.SNOWDRIVER_OUT,
                            plane=lambda v, k, ptr: _abi.check(self._lib.mcf_snowplan_summary_fetch(self._p, v, k, ptr, 0)),
                            days=lambda ptr: _abi.check(self._lib.mcf_snowplan_summary_days(self._p, ptr)))

    # ---- series sink of the five series (include/mcf.h mcf_snowplan_series_*) ------------------------------------------------
    def series_enable(self, points=None, zones=None, vars=("totalSWE",), stats=("mean", "min", "max"), nzones: int | None = None):
        """arguments as snowpack_series_spec, cells and labels of this plan's rows; the state is allocated here"""
        self._pser = snowpack_series_spec(self.rows, self.cols, points, zones, vars, stats, nzones)
        _abi.check(self._lib.mcf_snowplan_series_enable(self._p, C.byref(self._pser[0])))

    def series_accumulate(self, chunk: int):
        """folds the series of the chunk run last (after run_chunk, before keep_chunk): chunks in any order, each once"""
        _abi.check(self._lib.mcf_snowplan_series_accumulate(self._p, int(chunk)))

    def series_reset(self):
        _abi.check(self._lib.mcf_snowplan_series_reset(self._p))

    def nc_write(self, writer, chunk: int, row0: int = 0):
        """the steps of the chunk run last as rows [row0, row0 + rows) of a ncsink.SnowpackNcWriter's records, packed on the
        device (include/mcf.h mcf_snowplan_nc_write); behind the last chunk the steps no chunk covers become missval"""
        _abi.check(self._lib.mcf_snowplan_nc_write(self._p, writer._h, int(chunk), int(row0)))

    def fetch_point_series(self, var) -> np.ndarray:
        """[tsteps, npoints] of one selected series (name of _abi.SNOWDRIVER_OUT or index)"""
        v = _abi.SNOWDRIVER_OUT.index(var) if isinstance(var, str) else int(var)
        a, ptr = Buffers().out((self.tsteps, int(self._pser[0].npoints)))
        _abi.check(self._lib.mcf_snowplan_series_fetch_points(self._p, v, ptr))
        return a

    def fetch_zone_series(self, var, stat) -> np.ndarray:
        """[tsteps, nzones] of one selected statistic of one selected series (names or indices)"""
        v = _abi.SNOWDRIVER_OUT.index(var) if isinstance(var, str) else int(var)
        k = _abi.ZSTAT_NAMES.index(stat) if isinstance(stat, str) else int(stat)
        a, ptr = Buffers().out((self.tsteps, int(self._pser[0].nzones)))
        _abi.check(self._lib.mcf_snowplan_series_fetch_zones(self._p, v, k, ptr))
        return a

    # ---- the snow-day microclimate inside the chunk loop (include/mcf.h: two passes over the year) ------------------
    def reset(self):
        """Back to the series' start (hand-over depths, ages, snow surface): the second pass."""
        _abi.check(self._lib.mcf_snowplan_reset(self._p))

    FETCH = {"isnowdc": 0, "isnowac": 1, "isnowag": 2, "slope": 3, "aspect": 4, "skyview": 5, "wsa": 6, "hor": 7,
             "Tc": 8, "Tg": 9, "groundsnowdepth": 10, "snowden": 11, "totalSWE": 12}

    def fetch_cells(self, what: str, cells) -> np.ndarray:
        """[len(cells), depth] values of one of the plan's device arrays (FETCH) for a sample of cells (0-based column-major
        indices within the block): the hand-over state, the chunk's terrain, the series of the chunk run last."""
        c = np.ascontiguousarray(cells, dtype=np.int64)
        depth = {"wsa": 8, "hor": 24}.get(what, self._chunk_steps if self.FETCH[what] >= 8 else 1)
        out, optr = Buffers().out((c.size, depth))
        d = C.c_int32()
        _abi.check(self._lib.mcf_snowplan_fetch_cells(self._p, self.FETCH[what], Buffers().ptr(c), int(c.size), optr, C.byref(d)))
        assert d.value == depth
        return out

    def keep_chunk(self, chunk: int, reserve_bytes: int = 32 << 30) -> bool:
        """After run_chunk (and apply3 / meand_accumulate): the chunk's series stay on the device for the second pass if
        `reserve_bytes` of device memory remain free; True if kept (then pass 2 only calls microsnow for it)."""
        k = C.c_int32()
        _abi.check(self._lib.mcf_snowplan_keep_chunk(self._p, int(chunk), int(reserve_bytes), C.byref(k)))
        return bool(k.value)

    def can_keep(self, reserve_bytes: int = 32 << 30) -> bool:
        """Would keep_chunk keep a chunk now? (include/mcf.h mcf_snowplan_can_keep)"""
        k = C.c_int32()
        _abi.check(self._lib.mcf_snowplan_can_keep(self._p, int(reserve_bytes), C.byref(k)))
        return bool(k.value)

    SERIES_ALL, SERIES_PASS1 = 31, 4 | 16       # all five; totalSWE (day classes) + density (mean damping depth)

    def set_series(self, mask: int):
        """Which of the five device series run_chunk writes from now on (include/mcf.h mcf_snowplan_set_series)."""
        _abi.check(self._lib.mcf_snowplan_set_series(self._p, int(mask)))

    def release_kept(self):
        _abi.check(self._lib.mcf_snowplan_release_kept(self._p))

    def checkpoint(self, chunk: int):
        """Keeps the state `chunk` starts from on the device (call before its prepare_chunk, in the first pass)."""
        _abi.check(self._lib.mcf_snowplan_checkpoint(self._p, int(chunk)))

    def restore(self, chunk: int):
        """Puts the checkpointed start state of `chunk` back: the second pass re-runs only the chunks with a snow day."""
        _abi.check(self._lib.mcf_snowplan_restore(self._p, int(chunk)))

    def meand_accumulate(self, chunk: int, snowday):
        sd = np.ascontiguousarray(snowday, dtype=np.int32)
        _abi.check(self._lib.mcf_snowplan_meand_accumulate(self._p, int(chunk), Buffers().ptr(sd)))

    def micro_setup(self, reqhgt, obstime, climdata, vegp, other, mat, out, sub_of_day, reuse_static: bool = False):
        """gridmicrosnow1's inputs for the snow-day SUBSET series (what `.prepsnowinputs1` hands it: subset weather incl.
        umu, `.sortl2` vegetation, bare-ground terrain + Smax) and, per day of the whole series, its day in the subset
        (-1: not a snow day).  `reuse_static`: the matrices (vegp, other) of the previous set-up stay on the device — only the
        series and the day map are new."""
        if reuse_static and getattr(self, "_micro_static", None) is not None:
            m = self._micro_static                     # the marshalled matrices (kept alive; not uploaded again)
            T = len(np.asarray(obstime["year"]))
            si = m.inputs
            si.tsteps = m.tsteps = T
            si.obstime.year = m.i32(obstime["year"], (T,), "obstime$year")
            si.obstime.month = m.i32(obstime["month"], (T,), "obstime$month")
            si.obstime.day = m.i32(obstime["day"], (T,), "obstime$day")
            si.obstime.hour = m.f64(obstime["hour"], (T,), "obstime$hour")
            for f in _abi.SNOW_CLIM_FIELDS:
                src = _get(climdata, *(("precip", "prec") if f == "precip" else (f,)))
                setattr(si.clim, f, m.f64(src, (T,), f"climdata${f}"))
        else:
            m = marshal_snow(obstime, climdata, vegp, other, False, micro=True)
            self._micro_static = m
        sod = np.ascontiguousarray(sub_of_day, dtype=np.int32)
        sel = (C.c_int32 * _abi.NOUT)(*[1 if v else 0 for v in out])
        _abi.check(self._lib.mcf_snowplan_micro_setup(self._p, C.byref(m.inputs), Buffers().ptr(sod),
                                                      int(sod.size), float(reqhgt), float(mat), C.byref(sel), 1 if reuse_static else 0))

    def covered_tiles(self, plan, chunk: int, day: int, ndays: int):
        """uint8 [tiles of `plan`]: 1 where every cell of the tile lies under snow at every step of the chunk's days
        [day, day + ndays) — mcf_snowplan_microsnow overwrites all its values, the solver may leave the tile out
        (include/mcf.h mcf_snowplan_covered_tiles); and the number of such tiles"""
        sk, skp = Buffers().out(plan.n_tiles, np.uint8, zero=True)
        n = C.c_int64(0)
        _abi.check(self._lib.mcf_snowplan_covered_tiles(self._p, plan._p, int(chunk), int(day), int(ndays),
                                                        skp, int(sk.size), C.byref(n)))
        return sk, int(n.value)

    def free_cells(self, plan, chunk: int, day: int, ndays: int):
        """-> (device address of one byte per cell, number of ones): 1 where the cell is NOT under snow at every step of the
        chunk's days [day, day + ndays) (or has no vegetation height) — the cells whose solver values survive the merge, for
        Plan.run_days_cells (include/mcf.h mcf_snowplan_free_cells)"""
        ptr, n = C.c_void_p(0), C.c_int64(0)
        _abi.check(self._lib.mcf_snowplan_free_cells(self._p, plan._p, int(chunk), int(day), int(ndays), C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    def microsnow(self, plan, chunk: int, slot: int, nosnowday):
        """gridmicrosnow1 on the chunk's snow days, written over the solver's outputs in ring slot `slot` of `plan`."""
        nd = np.ascontiguousarray(nosnowday, dtype=np.int32)
        _abi.check(self._lib.mcf_snowplan_microsnow(self._p, plan._p, int(chunk), int(slot), Buffers().ptr(nd)))


def _dev_piece(t, cols):
    """(rows, device pointer) of a halo piece held as a torch tensor [cols, h] on the GPU"""
    if t is None or t.numel() == 0:
        return 0, None
    if not t.is_cuda or str(t.dtype) != "torch.float64" or not t.is_contiguous() or t.dim() != 2 or t.shape[0] != cols:
        raise ValueError("a halo piece is a contiguous float64 CUDA tensor of shape [cols, rows]")
    return int(t.shape[1]), C.c_void_p(t.data_ptr())


class DeviceHalo:
    """Halo exchange of a SnowPlan's surface between neighbouring ranks without host staging: the 128 boundary rows are packed
    on the device, sent / received point-to-point as device tensors (RCCL when the backend is nccl; any other backend moves
    those rows — not the block — through the host) and handed to prepare_chunk_dev.  Buffers are allocated once."""

    def __init__(self, plan, rank: int, world: int, halo: int | None = None):
        import torch
        import torch.distributed as dist
        from .terrain import HALO
        self.plan, self.rank, self.world = plan, rank, world
        halo = HALO if halo is None else halo
        dev = torch.device("cuda", plan.device)
        counts = torch.zeros(world, dtype=torch.int64, device=dev if dist.get_backend() == "nccl" else "cpu")
        counts[rank] = plan.rows
        dist.all_reduce(counts)
        counts = [int(v) for v in counts.tolist()]
        mk = lambda h: torch.empty((plan.cols, h), dtype=torch.float64, device=dev)      # noqa: E731
        own = min(halo, plan.rows)
        self.send_n = mk(own) if rank > 0 else None
        self.send_s = mk(own) if rank < world - 1 else None
        self.recv_n = mk(min(halo, counts[rank - 1])) if rank > 0 else None
        self.recv_s = mk(min(halo, counts[rank + 1])) if rank < world - 1 else None
        self.on_device = dist.get_backend() == "nccl"

    def exchange(self):
        """-> (north piece, south piece) as device tensors (None at the raster's edge)"""
        import torch
        import torch.distributed as dist
        if self.world == 1:
            return None, None
        self.plan.pack_halo(self.send_n, self.send_s)
        st = (lambda t: t) if self.on_device else (lambda t: t.cpu())
        ops, rn, rs = [], None, None
        if self.rank > 0:
            rn = self.recv_n if self.on_device else torch.empty(self.recv_n.shape, dtype=torch.float64)
            ops.append(dist.P2POp(dist.irecv, rn, self.rank - 1))
            ops.append(dist.P2POp(dist.isend, st(self.send_n), self.rank - 1))
        if self.rank < self.world - 1:
            rs = self.recv_s if self.on_device else torch.empty(self.recv_s.shape, dtype=torch.float64)
            ops.append(dist.P2POp(dist.isend, st(self.send_s), self.rank + 1))
            ops.append(dist.P2POp(dist.irecv, rs, self.rank + 1))
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        if self.on_device:
            torch.cuda.current_stream().synchronize()      # the library's kernels run on the null stream
        else:
            if rn is not None:
                self.recv_n.copy_(rn)
            if rs is not None:
                self.recv_s.copy_(rs)
            torch.cuda.synchronize()
        return self.recv_n, self.recv_s


def snowmodel1_chunks_tiled(plan, rank: int, world: int, *, exchange=None, allreduce=None) -> dict:
    """Drives one rank's SnowPlan through the chunk loop of a row-tiled raster: per chunk a halo exchange of
    the snow surface (terrain.exchange_halo, point-to-point between neighbouring ranks) and two (sum, count)
    all-reduces (the raster means of the surface and of tpic).  `exchange` / `allreduce` are injectable for
    tests; the defaults use torch.distributed (RCCL when the backend is nccl)."""
    from .terrain import exchange_halo
    from .distributed import allreduce_twi_mean
    if exchange is None:
        exchange = lambda blk: exchange_halo(blk, rank, world)          # noqa: E731
    if allreduce is None:
        allreduce = allreduce_twi_mean                                    # (sum, count) -> global mean
    for ch in range(plan.chunks):
        surf = plan.surface()
        ext, hn, hs = exchange(surf)
        s, n = plan.surface_partial()
        smean = allreduce(s, n)
        ts, tn = plan.prepare_chunk(ch, ext if (hn or hs) else None, hn, hs, smean)
        plan.run_chunk(ch, allreduce(ts, tn))
    return plan.result


def _marshal_grid(g: Mapping, array_forcing: bool, device: int, cells_per_block: int = 0, coarse: Mapping | None = None):
    """marshal() of a `grid` mapping: the arguments of api.runmicro1Cpp by name (array weather: "lats" / "lons" for lat / lon),
    with the defaults a mapping may leave out"""
    return marshal(g["obstime"], g["climdata"], g["pointm"], g["vegp"], g["soilc"], g["reqhgt"], g["zref"],
                   g["lats"] if "lats" in g else g["lat"], g["lons"] if "lons" in g else g["lon"],
                   g.get("Sminp", 0.0), g.get("Smaxp", 0.0), g["tfact"], g.get("complete", True), g.get("mat", 0.0),
                   g.get("out", (1,) * 10), array_forcing, device, 0, cells_per_block, g.get("dfsel"), coarse)


# ---- `runmicro(..., snow = TRUE)` as one library call (include/mcf.h mcf_runmicrosnow1 / mcf_snowrun_*) -------------------
class SnowRun:
    """`.snowmodel1` + `.runmicrosnow1` (R/internal.R:2498-2619, 3581-3659) device-resident, staged:
    `pass1()` walks the snow model's chunk loop and returns the day classes, `pass2(micro inputs)` the merged microclimate.

    grid   the fifteen arguments of runmicro1Cpp for the WHOLE series (mapping with the names of api.runmicro1Cpp's parameters)
    snow   {"obstime", "climdata", "pointm", "vegp", "other", "snowenv", "dtm", "res", "tfact"[, "chunk_steps"]} as for
           `SnowPlan` / snowmodel1_chunks
    devices / n_blocks: row blocks over several devices from this one process (None: one block on `device`).
    below  reqhgt < 0 (include/mcf.h mcf_snowrun_create_below): the solver streams Tbelowgroundv over the no-snow days, the
           snow-day model gives Tz and soilm; data.frame weather, one period per handle.  False: reqhgt < 0 is refused.
    handle False: the inputs are marshalled (`_in`, `_gm`, `_din`) and no library handle is made — for the entries that take them
           in one call (runmicrosnow1); pass1 / pass2 need the handle.
    micro_coarse  array weather with the coarse arrays left coarse (include/mcf.h mcf_snowrun_create_coarse): {"clim_c": the nine
           coarse weather arrays of the snow-day microclimate [crows, ccols, T] (winddir per coarse cell), "umu_c"}.  `grid` is then
           runmicro2Cpp_coarse's arguments by name with "coarse" = {"rowpos", "colpos"[, "altcorrect", "dtmc", "dtm"]}, `snow`
           snowmodel2_coarse's by name (obstime, clim_c, pointm_c, vegp, other, snowenv, dtm, dtmc, res, tfact, rowpos, colpos[,
           altcorrect, agg, chunk_steps]); pass2's `micro` carries obstime, vegp and other only.  want_umu: pass 1 fills `self.umu`,
           pointm$umu on the raster [rows, cols, tsteps] (the sixth series of `snowmodel2_coarse`)."""

    def __init__(self, grid: Mapping, snow: Mapping, *, device: int = 0, devices=None, n_blocks: int = 0, cells_per_block: int = 0,
                 below: bool = False, handle: bool = True, micro_coarse: Mapping | None = None, want_umu: bool = False):
        self._p = None
        self._msum = self._psum = self._mser = self._pser = None      # the specs of the enabled summaries and series
        self.coarse = micro_coarse is not None
        if self.coarse:
            self._marshal_coarse(grid, snow, micro_coarse, device)
        else:
            self._marshal(grid, snow, device, cells_per_block)
        if not handle:
            return
        mu = _abi.multi(devices, n_blocks)
        self._p = C.c_void_p()
        if self.coarse:
            # (pointm$umu of every step leaves with pass 1: the coarse handle hands it out of the chunks' slabs)
            self.umu, umup = self._sm.out((self.rows, self.cols, self.tsteps)) if want_umu else (None, None)
            _abi.check(self._lib.mcf_snowrun_create_coarse(C.byref(self._cin_all), C.byref(self._gm.options), C.byref(mu[0]) if mu else None,
                                                           umup, C.byref(self._p)))
            self.days = int(self._lib.mcf_snowrun_days(self._p))
            return
        create = self._lib.mcf_snowrun_create_below if below else self._lib.mcf_snowrun_create
        _abi.check(create(C.byref(self._in), C.byref(self._gm.options), C.byref(mu[0]) if mu else None, C.byref(self._p)))
        self.days = int(self._lib.mcf_snowrun_days(self._p))

    def _marshal(self, grid: Mapping, snow: Mapping, device: int, cells_per_block: int):
        self._lib = _abi.load()
        g = grid
        # array weather (mcf_runmicrosnow2): `snow` carries "af_wind" (and optionally "wsa_s"), every weather array is [rows, cols, T]
        self.array_weather = "af_wind" in snow
        self._gm = _marshal_grid(g, self.array_weather, device, cells_per_block)
        self._alloc_outputs = lambda: alloc_outputs(self._gm)
        R, Cc = np.shape(snow["vegp"]["pai"])
        oth = _terrain_placeholders(snow["other"], R, Cc)
        if self.array_weather:
            self._sm, self._din = _driver_in_array(snow["obstime"], snow["climdata"], snow["pointm"], snow["vegp"], oth,
                                                   snow.get("snowenv", "Alpine"), snow["dtm"], snow["res"], snow.get("tfact", 0.02),
                                                   snow["af_wind"], snow.get("wsa_s", 0), snow.get("chunk_steps", 120))
        else:
            self._sm = marshal_snow(snow["obstime"], snow["climdata"], snow["vegp"], oth, False, pointm=snow["pointm"],
                                    snowenv=snow.get("snowenv", "Alpine"))
            self._din = _driver_in(self._sm, snow["dtm"], snow["res"], snow.get("tfact", 0.02), snow.get("chunk_steps", 120))
        self._in = _abi.MicrosnowIn()
        self._in.grid = C.pointer(self._gm.inputs)
        self._in.snow = C.pointer(self._din)
        self._in.micro = None
        self._in.mat = 0.0
        self.rows, self.cols, self.tsteps = R, Cc, self._sm.tsteps
        self._mm = None

    def _marshal_coarse(self, grid: Mapping, snow: Mapping, micro_coarse: Mapping, device: int):
        self._lib = _abi.load()
        g = grid
        if "coarse" not in g:
            raise ValueError('the coarse snow run takes grid["coarse"] = {"rowpos", "colpos"[, "altcorrect", "dtmc", "dtm"]}')
        self.array_weather = True
        self._gm = _marshal_grid(g, True, device, 0, g["coarse"])
        self._alloc_outputs = lambda: alloc_outputs(self._gm)
        alt = int(snow.get("altcorrect", 0))
        self._sm, self._cin, _ = marshal_snowcoarse(snow["obstime"], snow["clim_c"], snow["pointm_c"], snow["vegp"], snow["other"],
                                                    snow.get("snowenv", "Alpine"), snow["dtm"], snow["dtmc"], snow["res"],
                                                    snow.get("tfact", 0.02), snow["rowpos"], snow["colpos"], alt, snow.get("agg", 10),
                                                    snow.get("chunk_steps", 120))
        self._mcm, self._mci, self._mwinddir = marshal_microcoarse(micro_coarse["clim_c"], micro_coarse["umu_c"], snow["dtm"],
                                                                   snow["dtmc"], snow["rowpos"], snow["colpos"], alt)
        self._cin_all = _abi.MicrosnowCoarseIn()
        self._cin_all.grid = C.pointer(self._gm.inputs)
        self._cin_all.snow = C.pointer(self._cin)
        self._cin_all.micro = C.pointer(self._mci)
        self._cin_all.micro_static = None
        self._cin_all.mat = 0.0
        self.rows, self.cols, self.tsteps = self._sm.rows, self._sm.cols, self._sm.tsteps
        self._mm = None

    def _marshal_micro(self, micro: Mapping):
        """gridmicrosnow's inputs for the whole series (the coarse run: no weather arrays, the direction per step its own)"""
        if self.coarse:
            return marshal_snow(micro["obstime"], {"winddir": micro.get("winddir", self._mwinddir)}, micro["vegp"], micro["other"], True,
                                micro=True, weather=False)
        return marshal_snow(micro["obstime"], micro["climdata"], micro["vegp"], micro["other"], self.array_weather, micro=True)

    def keep(self, gigabytes: float):
        """Keep pass 1's snow chunks in device memory for pass 2, up to this much (include/mcf.h mcf_snowrun_keep; 0: off).
        Pays from the handle's second period on — the sets are pooled — or when the snow series are fetched anyway."""
        _abi.check(self._lib.mcf_snowrun_keep(self._p, int(gigabytes * 2 ** 30)))

    def set_day_layers(self, layer_of_day):
        """Between pass1 and pass2, layered vegetation: the solver's day -> layer map (include/mcf.h mcf_snowrun_set_day_layers);
        one 0-based layer per day of the whole series, -1: none"""
        lod = np.ascontiguousarray(layer_of_day, dtype=np.int32)
        _abi.check(self._lib.mcf_snowrun_set_day_layers(self._p, Buffers().ptr(lod), int(lod.size)))

    def stats(self) -> dict:
        """What pass 2 was spared (include/mcf.h mcf_snowrun_stats)."""
        st = (C.c_int64 * 4)()
        _abi.check(self._lib.mcf_snowrun_stats(self._p, st))
        return dict(zip(("tile_days", "tile_days_left_out", "chunks_kept", "chunks_rerun"), (int(v) for v in st)))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self._lib.mcf_snowrun_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def summary_enable(self, summary: Mapping | None = None, pack_summary: Mapping | None = None):
        """Period summaries folded on the device (include/mcf.h mcf_snowrun_summary_enable), before pass1.  Each a mapping with
        "periods" (one integer per day, -1: not counted) and optionally "vars", "stats", "thresholds", "nperiods": `summary` over
        the merged outputs (vars: output names the run was created with; days of neither class are never counted), `pack_summary`
        over the snow model's five series (vars: names of _abi.SNOWDRIVER_OUT; days past the last whole chunk must be -1)."""
        ms = _micro_summary_spec(summary) if summary is not None else None
        ps = _pack_summary_spec(pack_summary) if pack_summary is not None else None
        _abi.check(self._lib.mcf_snowrun_summary_enable(self._p, C.byref(ms[0]) if ms else None, C.byref(ps[0]) if ps else None))
        self._msum, self._psum = ms, ps

    def fetch_summary(self) -> dict:
        """-> {variable: {statistic: [rows, cols, nperiods]}, "days": ...} of the outputs' summaries (after pass2) and, under
        "snow", {series: {statistic: plane}, "days": ...} of the snowpack's (after pass1)"""
        return _merge_micro_and_pack(self._msum, self._psum, lambda pack, spec, names: summary_sink(
            Buffers(), self.rows, self.cols, spec, names,
            plane=lambda v, k, ptr: _abi.check(self._lib.mcf_snowrun_summary_fetch(self._p, pack, v, k, ptr)),
            days=lambda ptr: _abi.check(self._lib.mcf_snowrun_summary_days(self._p, pack, ptr))))

    def series_enable(self, series: Mapping | None = None, pack_series: Mapping | None = None):
        """The series sink (include/mcf.h mcf_snowrun_series_enable), before pass1.  Each a mapping with "points" and / or "zones"
        (whole-raster cell indices and labels, as api.series_spec takes them) and optionally "vars", "stats", "nzones": `series`
        over the merged outputs (vars: output names the run was created with; days of neither class are never folded),
        `pack_series` over the snow model's five series (vars: names of _abi.SNOWDRIVER_OUT)."""
        ms = _micro_series_spec(self.rows, self.cols, series) if series is not None else None
        ps = _pack_series_spec(self.rows, self.cols, pack_series) if pack_series is not None else None
        _abi.check(self._lib.mcf_snowrun_series_enable(self._p, C.byref(ms[0]) if ms else None, C.byref(ps[0]) if ps else None))
        self._mser, self._pser = ms, ps

    def fetch_series(self) -> dict:
        """-> {variable: {"points": [tsteps, npoints], "zones": {statistic: [tsteps, nzones]}}} of the outputs' series (after
        pass2) and, under "snow", the same per series of the snowpack (after pass1)"""
        return _merge_micro_and_pack(self._mser, self._pser, lambda pack, spec, names: _series_sink_by_variable(
            Buffers(), self.tsteps, spec, names,
            points=lambda v, ptr: _abi.check(self._lib.mcf_snowrun_series_fetch_points(self._p, pack, v, ptr)),
            zones=lambda v, k, ptr: _abi.check(self._lib.mcf_snowrun_series_fetch_zones(self._p, pack, v, k, ptr))))

    def drop_days(self, days):
        """Between pass1 and pass2: the listed days (0-based; each a no-snow day that is no snow day) leave the run's classes —
        pass2 does not solve them, they are NA in the arrays and missval in the file (include/mcf.h mcf_snowrun_drop_days)"""
        drop = np.zeros(self.days, dtype=np.int32)
        drop[np.asarray(days, dtype=np.int64)] = 1
        _abi.check(self._lib.mcf_snowrun_drop_days(self._p, Buffers().ptr(drop), int(drop.size)))

    def nc_enable(self, writer=None, pack_writer=None):
        """The netCDF sink (include/mcf.h mcf_snowrun_nc_enable), before pass1: `writer` a ncsink.NcWriter for the merged outputs
        (pass2 writes every chunk's row strips, packed on the device; pass2(want_arrays=False) then moves no array), `pack_writer`
        a ncsink.SnowpackNcWriter for the snow model's series (pass1).  The caller closes the writers after the passes."""
        _abi.check(self._lib.mcf_snowrun_nc_enable(self._p, writer._h if writer is not None else None,
                                                   pack_writer._h if pack_writer is not None else None))
        self._ncw = (writer, pack_writer)

    def pass1(self, want_smod: bool = False):
        """-> (snowdays, nosnowdays[, smod]): one 0/1 flag per day; smod = `.snowmodel1`'s five [rows, cols, tsteps] arrays"""
        (sd, sdp), (nd, ndp) = Buffers().out(self.days, np.int32, zero=True), Buffers().out(self.days, np.int32, zero=True)
        so, smod = _driver_out(self.rows, self.cols, self.tsteps) if want_smod else (None, None)
        _abi.check(self._lib.mcf_snowrun_pass1(self._p, C.byref(so) if so is not None else None, sdp, ndp))
        return (sd, nd, smod) if want_smod else (sd, nd)

    def pass2(self, micro: Mapping | None, mat: float, want_arrays: bool = True):
        """micro = {"obstime", "climdata" (with umu), "vegp" (`.sortl2`), "other" (bare-ground terrain, lat, lon, zref, Smax)} for
        the WHOLE series, or None when the year has no snow day -> the ten merged outputs.  want_arrays False (with a summary
        enabled): the merged days are folded only, no [rows, cols, steps] array is allocated or filled -> None"""
        mi = None
        if micro is not None:
            self._mm = self._marshal_micro(micro)
            mi = C.byref(self._mm.inputs)
        if not want_arrays:
            _abi.check(self._lib.mcf_snowrun_pass2(self._p, mi, float(mat), None))
            return None
        outs, arrays = self._alloc_outputs()
        _abi.check(self._lib.mcf_snowrun_pass2(self._p, mi, float(mat), C.byref(outs)))
        return arrays


def _merge_micro_and_pack(micro_spec, pack_spec, sink) -> dict:
    """sink(pack, spec, names) -> dict for each of the two specs that is there: the outputs' at the top, the snowpack's under the key "snow" """
    res = {}
    for pack, spec, names in ((0, micro_spec, _abi.OUT_NAMES), (1, pack_spec, _abi.SNOWDRIVER_OUT)):
        if spec is None:
            continue
        d = sink(pack, spec, names)
        if pack:
            res["snow"] = d
        else:
            res.update(d)
    return res


def _series_sink_by_variable(b, tsteps, spec, names, **to) -> dict:
    """api._series_sink's {"points": {v: a}, "zones": {v: {stat: a}}} -> {v: {"points": a or None, "zones": {stat: a}}}"""
    from .api import _series_sink
    d = _series_sink(b, tsteps, *spec, names=names, **to)
    return {v: {"points": d["points"].get(v), "zones": d["zones"].get(v, {})} for v in list(d["points"]) + [k for k in d["zones"] if k not in d["points"]]}


def runmicrosnow1(grid: Mapping, snow: Mapping, micro: Mapping | None, mat: float, *, device: int = 0, devices=None, n_blocks: int = 0,
                  want_smod: bool = False, cells_per_block: int = 0, below: bool = False, summary: Mapping | None = None,
                  pack_summary: Mapping | None = None, want_arrays: bool = True, series: Mapping | None = None,
                  pack_series: Mapping | None = None):
    """mcf_runmicrosnow1 / mcf_runmicrosnow1_multi: the whole snow run as ONE library call (arguments as `SnowRun`, `micro` as
    `SnowRun.pass2`) -> the merged outputs[, smod].  below: reqhgt < 0 through mcf_runmicrosnow1_below / _below_multi.
    summary / pack_summary (mappings as for SnowRun.summary_enable): the run through mcf_runmicrosnow_summary, either weather
    geometry -> {"out": the merged outputs, or None with want_arrays False (nothing of size cells x steps is moved), "summary":
    as SnowRun.fetch_summary, "snowdays", "nosnowdays"[, "smod"]}"""
    with SnowRun(grid, snow, device=device, cells_per_block=cells_per_block, handle=False) as run:
        if micro is not None:
            run._mm = marshal_snow(micro["obstime"], micro["climdata"], micro["vegp"], micro["other"], run.array_weather, micro=True)
            run._in.micro = C.pointer(run._mm.inputs)
        run._in.mat = float(mat)
        if series is not None or pack_series is not None:
            if summary is not None or pack_summary is not None:
                raise ValueError("one call takes the summaries or the series sink: both on one run through SnowRun")
            return _runmicrosnow_sink(run, "series", series, pack_series, want_arrays, want_smod, devices, n_blocks)
        if summary is not None or pack_summary is not None:
            if below:
                raise ValueError("period summaries of the snow run need reqhgt >= 0")
            return _runmicrosnow_sink(run, "summary", summary, pack_summary, want_arrays, want_smod, devices, n_blocks)
        outs, arrays = alloc_outputs(run._gm)
        so, smod = _driver_out(run.rows, run.cols, run.tsteps) if want_smod else (None, None)
        sop = C.byref(so) if so is not None else None
        lib = _abi.load()
        mu = _abi.multi(devices, n_blocks)
        if mu:
            fn = lib.mcf_runmicrosnow1_below_multi if below else lib.mcf_runmicrosnow1_multi
            _abi.check(fn(C.byref(run._in), C.byref(run._gm.options), C.byref(mu[0]), C.byref(outs), sop))
        else:
            fn = lib.mcf_runmicrosnow1_below if below else lib.mcf_runmicrosnow2 if run.array_weather else lib.mcf_runmicrosnow1
            _abi.check(fn(C.byref(run._in), C.byref(run._gm.options), C.byref(outs), sop))
    return (arrays, smod) if want_smod else arrays


def runmicrosnow_nc(grid: Mapping, snow: Mapping, micro: Mapping | None, mat: float, *, fileout=None, pack_fileout=None, nc_grid: Mapping,
                    vars=None, pack_vars=None, format: str = "classic", deflate_level: int = 0, want_arrays: bool = False,
                    want_smod: bool = False, device: int = 0, devices=None, n_blocks: int = 0, cells_per_block: int = 0) -> dict:
    """The whole snow run into netCDF files as ONE library call (include/mcf.h mcf_runmicrosnow_nc; arguments as runmicrosnow1):
    `fileout` the merged outputs as a `writetonc` file (`vars`: among the run's outputs, default ncsink.default_vars(reqhgt) that
    the run has), `pack_fileout` the snow model's five series (`pack_vars`); either may be None.  reqhgt < 0 runs the below-ground
    run.  `nc_grid`: the mapping ncsink.writetonc takes as `dtm`.  The classic file is byte for byte ncsink.writetonc of
    runmicrosnow1's arrays (of the same block count).
    -> {"out": the merged outputs or None, "snowdays", "nosnowdays"[, "smod"]}"""
    from . import ncsink
    with SnowRun(grid, snow, device=device, cells_per_block=cells_per_block, handle=False) as run:
        if micro is not None:
            run._mm = marshal_snow(micro["obstime"], micro["climdata"], micro["vegp"], micro["other"], run.array_weather, micro=True)
            run._in.micro = C.pointer(run._mm.inputs)
        run._in.mat = float(mat)
        hours, east, north, crs = ncsink.grid_of(nc_grid, snow["obstime"])
        reqhgt = float(run._gm.options.reqhgt)
        sp = ps = None
        if fileout is not None:
            has = [n for n, o in zip(_abi.OUT_NAMES, run._gm.options.out) if o]
            names = [n for n in ncsink.default_vars(reqhgt) if n in has] if vars is None else vars
            sp, _ = ncsink.nc_spec(run.rows, run.cols, hours, east, north, reqhgt, names, crs, False, format, deflate_level)
        if pack_fileout is not None:
            ps, _ = ncsink.ncpack_spec(run.rows, run.cols, hours, east, north, pack_vars, crs, format, deflate_level)
        so = _abi.SnowrunNcOut()
        res = {"out": None}
        if want_arrays:
            outs, res["out"] = alloc_outputs(run._gm)
            so.arrays = C.pointer(outs)
        if want_smod:
            sm, res["smod"] = _driver_out(run.rows, run.cols, run.tsteps)
            so.smod = C.pointer(sm)
        nd = run.tsteps // 24
        res["snowdays"], so.snowday = run._gm.out(nd, np.int32, zero=True)
        res["nosnowdays"], so.nosnowday = run._gm.out(nd, np.int32, zero=True)
        mu = _abi.multi(devices, n_blocks)
        _abi.check(_abi.load().mcf_runmicrosnow_nc(C.byref(run._in), C.byref(run._gm.options), C.byref(mu[0]) if mu else None,
                                                   str(fileout).encode() if sp is not None else None, C.byref(sp) if sp is not None else None,
                                                   str(pack_fileout).encode() if ps is not None else None,
                                                   C.byref(ps) if ps is not None else None, C.byref(so)))
    return res


# kind -> the two spec builders, the out struct, the sink filler (run, spec, names, destination struct) and the library entry
_SINK_KINDS = {
    "summary": (lambda run, m: _micro_summary_spec(m), lambda run, m: _pack_summary_spec(m), _abi.SnowrunSummaryOut,
                lambda run, spec, names, dst: summary_sink(run._gm, run.rows, run.cols, spec, names, dst), "mcf_runmicrosnow_summary"),
    "series": (lambda run, m: _micro_series_spec(run.rows, run.cols, m), lambda run, m: _pack_series_spec(run.rows, run.cols, m),
               _abi.SnowrunSeriesOut, lambda run, spec, names, dst: _series_sink_by_variable(run._gm, run.tsteps, spec, names, so=dst),
               "mcf_runmicrosnow_series"),
}


def _runmicrosnow_sink(run, kind, micro, pack, want_arrays, want_smod, devices, n_blocks) -> dict:
    """-> {"out": the merged outputs or None, kind: as SnowRun.fetch_summary / fetch_series, "snowdays", "nosnowdays"[, "smod"]}"""
    micro_spec, pack_spec, out_struct, fill, entry = _SINK_KINDS[kind]
    ms = micro_spec(run, micro) if micro is not None else None
    ps = pack_spec(run, pack) if pack is not None else None
    so = out_struct()
    res = {"out": None, kind: _merge_micro_and_pack(ms, ps, lambda p, spec, names: fill(run, spec, names, so.pack if p else so.micro))}
    if want_arrays:
        outs, res["out"] = alloc_outputs(run._gm)
        so.arrays = C.pointer(outs)
    if want_smod:
        sm, res["smod"] = _driver_out(run.rows, run.cols, run.tsteps)
        so.smod = C.pointer(sm)
    nd = run.tsteps // 24
    res["snowdays"], so.snowday = run._gm.out(nd, np.int32, zero=True)
    res["nosnowdays"], so.nosnowday = run._gm.out(nd, np.int32, zero=True)
    mu = _abi.multi(devices, n_blocks)
    _abi.check(getattr(_abi.load(), entry)(C.byref(run._in), C.byref(run._gm.options), C.byref(mu[0]) if mu else None,
                                          C.byref(ms[0]) if ms else None, C.byref(ps[0]) if ps else None, C.byref(so)))
    return res


def runmicrosnow2(grid: Mapping, snow: Mapping, micro: Mapping | None, mat: float, **kw):
    """mcf_runmicrosnow2: `.snowmodel2`'s loop + `.runmicrosnow2` as ONE library call.  `grid` = runmicro2Cpp's arguments for the
    whole series (array climate / point-model arrays, "lats", "lons"), `snow` as for snowmodel2_device (with "af_wind"[, "wsa_s"]),
    `micro` = gridmicrosnow2's inputs for the whole series -> the merged outputs[, smod]"""
    if "af_wind" not in snow:
        raise ValueError("runmicrosnow2: snow['af_wind'] (the chunk wind series of `.snowmodel2`) is missing")
    return runmicrosnow1(grid, snow, micro, mat, **kw)


def runmicrosnow2_coarse(grid: Mapping, snow: Mapping, micro: Mapping | None, mat: float, *, want_smod: bool = False, device: int = 0):
    """mcf_runmicrosnow2_coarse: `.snowmodel2`'s loop + `.runmicrosnow2` as ONE library call with every coarse array left coarse.
    `grid`, `snow` as for `SnowRun(..., micro_coarse=...)`; `micro` = {"clim_c", "umu_c"} (the snow-day microclimate's coarse
    weather, `_fine_micro_inputs`' arguments) plus {"obstime", "vegp", "other"} as `SnowRun.pass2` takes them -> the merged
    outputs[, smod: Tc, Tg, groundsnowdepth, totalSWE, snowden, umu as `snowmodel2_coarse` returns them]"""
    if micro is None:
        raise ValueError("runmicrosnow2_coarse: the microclimate's coarse weather (micro['clim_c'], micro['umu_c']) is needed")
    with SnowRun(grid, snow, device=device, handle=False, micro_coarse=micro) as run:
        if "obstime" in micro:
            run._mm = run._marshal_micro(micro)
            run._cin_all.micro_static = C.pointer(run._mm.inputs)
        run._cin_all.mat = float(mat)
        outs, arrays = run._alloc_outputs()
        so, smod = None, None
        if want_smod:
            so = _abi.SnowFast2Out()
            smod = _wanted_series(run._sm, None, _abi.SNOWFAST2_OUT, so)
        _abi.check(run._lib.mcf_runmicrosnow2_coarse(C.byref(run._cin_all), C.byref(run._gm.options), C.byref(outs),
                                                     C.byref(so) if so is not None else None))
    return (arrays, smod) if want_smod else arrays
