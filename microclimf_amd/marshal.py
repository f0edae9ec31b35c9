"""Marshalling of R-style arguments (named lists of column-major arrays) into the
flat C structs of include/mcf.h.

Mirrors what Rcpp does for the reference at src/microclimfCpp.cpp:2056-2111
(runmicro1Cpp) and :2344-2399 (runmicro2Cpp): lookup is BY NAME, year/month/day
are coerced to int, every array is read as column-major fp64 with the raster
row as the fastest index.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Mapping, Sequence

import numpy as np

from . import _abi

_POINTER = {np.dtype(np.float64): _abi.c_double_p, np.dtype(np.int32): _abi.c_int32_p, np.dtype(np.int64): C.POINTER(C.c_int64),
            np.dtype(np.uint8): C.POINTER(C.c_uint8)}


class Buffers:
    """Owner of the numpy arrays behind the pointers it hands out: every such array lives as long as this object, so a pointer
    is good for as long as its owner is referenced (a call's own owner: for the call; a marshalling's: with the marshalling)."""

    def __init__(self):
        self._keep = []

    def ptr(self, a):
        """the pointer to an array as it lies in memory (None: a null pointer); the array is held from here on"""
        if a is None:
            return None
        self._keep.append(a)
        return a.ctypes.data_as(_POINTER[a.dtype])

    def f64(self, a, shape=None, name="?"):
        """column-major fp64 of `shape`; an array of another shape and the same size is read in Fortran order"""
        arr = np.asarray(a, dtype=np.float64)
        if shape is not None and tuple(arr.shape) != tuple(shape):
            if arr.size != int(np.prod(shape)):
                raise ValueError(f"{name}: expected shape {tuple(shape)}, got {arr.shape}")
            arr = arr.reshape(shape, order="F")
        return self.ptr(np.asfortranarray(arr))

    def i32_plain(self, a, n=None, name="?"):
        """numpy's own conversion to int32 (integers arrive as integers: year, month, day, step ranges, day tables)"""
        arr = np.ascontiguousarray(np.asarray(a).astype(np.int32))
        if n is not None and arr.shape != (n,):
            raise ValueError(f"{name}: expected length {n}")
        return self.ptr(arr)

    def i32_rcpp(self, a, shape, name):
        """Rcpp's as<IntegerVector/IntegerMatrix>(): doubles truncated towards zero, NA cells NA_integer_ (INT_MIN)"""
        v = np.trunc(np.asarray(a, dtype=np.float64))
        arr = np.asfortranarray(np.where(np.isnan(v), float(np.iinfo(np.int32).min), v).astype(np.int32))
        if tuple(arr.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {arr.shape}")
        return self.ptr(arr)

    def i64(self, a):
        return self.ptr(np.ascontiguousarray(a, dtype=np.int64))

    def out(self, shape, dtype=np.float64, zero=False):
        """-> (a column-major array for the library to write into, its pointer)"""
        a = (np.zeros if zero else np.empty)(shape, dtype=dtype, order="F")
        return a, self.ptr(a)


class Marshalled(Buffers):
    """GridInputs/Options plus the numpy arrays that back their pointers."""

    def __init__(self):
        super().__init__()
        self.inputs = _abi.GridInputs()
        self.options = _abi.Options()
        self.rows = self.cols = self.tsteps = 0

    i32 = Buffers.i32_plain


class SnowMarshalled(Buffers):
    """mcf_snow_inputs plus the numpy arrays that back its pointers (and those of the structs built around it)."""

    def __init__(self):
        super().__init__()
        self.inputs = _abi.SnowInputs()
        self.rows = self.cols = self.tsteps = 0

    i32 = Buffers.i32_rcpp


def _get(d: Mapping, *names):
    for n in names:
        if n in d:
            return d[n]
    raise KeyError(f"none of {names} present (have {sorted(d)})")


def marshal(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping,
            soilc: Mapping, reqhgt: float, zref: float, lat, lon, Sminp: float,
            Smaxp: float, tfact: float, complete: bool, mat: float,
            out: Sequence, array_forcing: bool, device: int = 0,
            days_per_chunk: int = 0, cells_per_block: int = 0, dfsel: Mapping | None = None,
            coarse: Mapping | None = None, soilc_optional: Sequence = (), vegp_optional: Sequence = ()) -> Marshalled:
    """`soilc_optional`: fields of soilc that may be missing (a NULL pointer: the plan derives them from the dtm); `vegp_optional`:
    likewise for vegp (paia, leafden: runmicro_heights derives them per height).  `coarse` = {"rowpos": [rows], "colpos": [cols]} switches to coarse array forcing (mcf.h, array_forcing == 2):
    climdata = {temp, relhum, pres, swdown, difrad, lwdown, windspeed, winddir} and pointm are then
    [coarse_rows, coarse_cols, tsteps] arrays."""
    m = Marshalled()
    hgt = np.asarray(vegp["hgt"], dtype=np.float64)
    if dfsel is None:
        if hgt.ndim != 2:
            raise ValueError("vegp$hgt must be a rows x cols matrix")
        L = 1
    else:                       # runmicro3Cpp/4Cpp: vegetation arrays are [rows, cols, layers]
        if hgt.ndim != 3:
            raise ValueError("vegp$hgt must be a rows x cols x layers array")
        # the reference walks dfsel's rows and indexes layer `row` of the arrays (cpp:2632, 2771): arrays may be
        # deeper than dfsel (`.runmodel3Cpp` renumbers the layers it uses, R/internal.R:1399) — the first L are read
        L = len(np.asarray(dfsel["st"]))
        if hgt.shape[2] < L:
            raise ValueError("dfsel has more rows than the vegetation arrays have layers")
    R, Cc = hgt.shape[:2]
    T = len(np.asarray(obstime["year"]))
    m.rows, m.cols, m.tsteps = R, Cc, T
    gi = m.inputs
    gi.rows, gi.cols, gi.tsteps = R, Cc, T
    gi.array_forcing = 2 if coarse is not None else 1 if array_forcing else 0
    cshape = None
    if coarse is not None:
        t0 = np.asarray(_get(climdata, "temp", "tc"))
        if t0.ndim != 3 or t0.shape[2] != T:
            raise ValueError("coarse climate arrays must be [coarse_rows, coarse_cols, tsteps]")
        cshape = t0.shape
        gi.coarse_rows, gi.coarse_cols = int(cshape[0]), int(cshape[1])
        gi.coarse_rowpos = m.f64(coarse["rowpos"], (R,), "coarse$rowpos")
        gi.coarse_colpos = m.f64(coarse["colpos"], (Cc,), "coarse$colpos")
        gi.coarse_relhum = m.f64(climdata["relhum"], cshape, "climdata$relhum")
        gi.coarse_winddir = m.f64(climdata["winddir"], cshape, "climdata$winddir")
        gi.coarse_altcorrect = int(coarse.get("altcorrect", 0))
        if gi.coarse_altcorrect:
            gi.coarse_dtm = m.f64(coarse["dtmc"], cshape[:2], "coarse$dtmc")
            gi.fine_dtm = m.f64(coarse["dtm"], (R, Cc), "coarse$dtm")
    gi.obstime.year = m.i32_plain(obstime["year"], T, "obstime$year")
    gi.obstime.month = m.i32_plain(obstime["month"], T, "obstime$month")
    gi.obstime.day = m.i32_plain(obstime["day"], T, "obstime$day")
    gi.obstime.hour = m.f64(obstime["hour"], (T,), "obstime$hour")
    fshape = cshape if coarse is not None else (R, Cc, T) if array_forcing else (T,)
    # climdata: data.frame names (1Cpp) or list names (2Cpp)
    names = {"tc": ("temp", "tc"), "pk": ("pres", "pk")}
    for f in _abi.CLIM_FIELDS:
        if coarse is not None and f in ("es", "ea", "tdew", "winddir"):     # derived inside the solver
            setattr(gi.clim, f, None)
            continue
        src = _get(climdata, *names.get(f, (f,)))
        shape = (T,) if f == "winddir" else fshape
        setattr(gi.clim, f, m.f64(src, shape, f"climdata${f}"))
    need_tgp = (reqhgt < 0) and (not complete)
    for f in _abi.POINTM_FIELDS:
        if f in ("Tg", "Tbp") and not need_tgp:
            setattr(gi.pointm, f, None)
            continue
        src = _get(pointm, *(("G", "Gp") if f == "G" else (f,)))
        if f == "Tbp" and np.ndim(src) == 0:       # `pointm$Tbp <- 0` (R/internal.R:1096)
            src = np.full(fshape, float(src))
        setattr(gi.pointm, f, m.f64(src, fshape, f"pointm${f}"))
    for f in _abi.VEGP_FIELDS:
        if f in vegp_optional and vegp.get(f) is None:
            setattr(gi.vegp, f, None)
            continue
        src = vegp[f]
        if dfsel is not None:
            src = np.asfortranarray(np.asarray(src, dtype=np.float64))
            if src.ndim != 3 or src.shape[2] < L:
                raise ValueError(f"vegp${f}: expected [rows, cols, >= {L} layers]")
            src = src[:, :, :L]            # a contiguous prefix in column-major order: no copy
        setattr(gi.vegp, f, m.f64(src, (R, Cc) if dfsel is None else (R, Cc, L), f"vegp${f}"))
    if dfsel is None:
        gi.veg_layers = 0
        gi.lyr_st = gi.lyr_ed = None
    else:
        gi.veg_layers = L
        gi.lyr_st = m.i32_plain(dfsel["st"], L, "dfsel$st")
        gi.lyr_ed = m.i32_plain(dfsel["ed"], L, "dfsel$ed")
    for f in _abi.SOILC_FIELDS:
        shape = (R, Cc, 8) if f == "wsa" else (R, Cc, 24) if f == "hor" else (R, Cc)
        if f in soilc_optional and soilc.get(f) is None:
            setattr(gi.soilc, f, None)
            continue
        setattr(gi.soilc, f, m.f64(soilc[f], shape, f"soilc${f}"))
    if array_forcing:
        gi.lats = m.f64(lat, (R, Cc), "lats")
        gi.lons = m.f64(lon, (R, Cc), "lons")
        gi.lat = gi.lon = float("nan")
    else:
        gi.lat, gi.lon = float(lat), float(lon)
        gi.lats = gi.lons = None
    op = m.options
    op.reqhgt, op.zref = float(reqhgt), float(zref)
    op.Sminp, op.Smaxp = float(Sminp), float(Smaxp)
    op.tfact, op.mat = float(tfact), float(mat)
    op.complete = 1 if complete else 0
    out = list(out)
    if len(out) != _abi.NOUT:
        raise ValueError("out must have 10 entries")
    for v in range(_abi.NOUT):
        op.out[v] = 1 if out[v] else 0     # may arrive as numeric 0/1 (R/internal.R:1161)
    op.device = device
    op.days_per_chunk = days_per_chunk
    op.cells_per_block = cells_per_block
    return m


def alloc_outputs(m: Marshalled):
    """Host output arrays [rows, cols, tsteps] (column-major) for requested vars; the struct holds the owner of its pointers."""
    outs = _abi.Outputs()
    outs._owner = b = Buffers()
    arrays = {}
    shape = (m.rows, m.cols, m.tsteps)
    for v, name in enumerate(_abi.OUT_NAMES):
        if not m.options.out[v]:
            outs.var[v] = None
        elif os.environ.get("MCF_TEST_PLAIN_OUTPUTS"):
            # (measurement aid, tools/oneshot_rate.py: an anonymous mapping without numpy's own huge-page advice —
            # what an R vector's malloc gives the library to write into)
            import mmap
            buf = mmap.mmap(-1, m.rows * m.cols * m.tsteps * 8, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
            arrays[name] = np.frombuffer(buf, dtype=np.float64).reshape(shape, order="F")
            outs.var[v] = b.ptr(arrays[name])
        else:
            arrays[name], outs.var[v] = b.out(shape)
    return outs, arrays


def build_summary_spec(struct, names, field: str, what: str, periods, vars, stats, thresholds=None, nperiods: int | None = None):
    """A summary spec of include/mcf.h (`struct`: mcf_summary_spec or mcf_snowpack_summary_spec, whose selection member is
    `field`) over the series `names`: `periods` one integer per day (-1 = not counted), `vars` names or indices, `stats` names of
    _abi.STAT_NAMES or indices, `thresholds` for hours_above — one number for every selected series or {series: number}.
    -> (spec, the selected series' indices, the selected statistics' indices, the period table); the spec holds the table."""
    pod = np.ascontiguousarray(np.asarray(periods).astype(np.int32)).ravel()
    vi = sorted({names.index(v) if isinstance(v, str) else int(v) for v in ((vars,) if isinstance(vars, str) else vars)})
    si = sorted({_abi.STAT_NAMES.index(s) if isinstance(s, str) else int(s) for s in ((stats,) if isinstance(stats, str) else stats)})
    if any(v < 0 or v >= len(names) for v in vi) or any(s < 0 or s >= _abi.NSTAT for s in si):
        raise ValueError(f"{what} of {names}, statistics of {_abi.STAT_NAMES}")
    sp = struct()
    sp.nperiods = int(nperiods) if nperiods is not None else int(pod.max()) + 1 if pod.size and pod.max() >= 0 else 1
    sp._owner = b = Buffers()
    sp.period_of_day = b.ptr(pod)
    for v in vi:
        getattr(sp, field)[v] = 1
        if isinstance(thresholds, Mapping):
            t = thresholds.get(names[v], thresholds.get(v, float("nan")))
        else:
            t = float("nan") if thresholds is None else thresholds
        sp.threshold[v] = float(t)
    for s in si:
        sp.stat[s] = 1
    return sp, vi, si, pod


def summary_sink(b: Buffers, rows: int, cols: int, spec, names, so=None, plane=None, days=None) -> dict:
    """The host side of a summary's sink for `spec` (as build_summary_spec returns it) over the series `names`: one
    [rows, cols, nperiods] plane per selected (series, statistic) and the counted days per period, held by `b`.  Their pointers
    go into `so` (a struct with `val[series][statistic]` and `days`, filled by the call that follows) or, plane by plane, to
    `plane(series, statistic, pointer)` and `days(pointer)` (fetches that fill them now; `days` None: no day counts here).
    -> {series: {statistic: plane}, "days": counted days per period (where they are asked for)}"""
    sp, vi, si, _pod = spec
    npd = max(int(sp.nperiods), 0)
    res = {}
    for v in vi:
        res[names[v]] = {}
        for k in si:
            res[names[v]][_abi.STAT_NAMES[k]], p = b.out((rows, cols, npd))
            if so is not None:
                so.val[v][k] = p
            else:
                plane(v, k, p)
    if so is not None or days is not None:
        d, p = b.out(max(npd, 1), np.int32, zero=True)
        if so is not None:
            so.days = p
        else:
            days(p)
        res["days"] = d[:npd]
    return res
