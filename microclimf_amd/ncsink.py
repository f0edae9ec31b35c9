"""Host mirror of the reference's `writetonc` (R/dataprep.R:1063-1260): the solver's outputs as a netCDF file of
int32 variables on (east, north, time).  `NcWriter` is the streaming form (day chunks straight from a `Plan`'s device
ring, packed and byte-ordered on the GPU); `writetonc` has the reference's call shape for a finished `mout`.

Two containers (`format=`): "classic" — netCDF classic / 64-bit offsets, `time` as record dimension, uncompressed, needs
nothing on the host (mcf_ncfile.hpp) — and "netcdf4", the reference's own (HDF5 by the netCDF-4 conventions, chunked,
deflate 9 unless `deflate_level` says otherwise; needs an HDF5 library on the host at run time, mcf_nc4file.hpp).
"""
from __future__ import annotations

import calendar
import ctypes as C
from typing import Mapping, Sequence

import numpy as np

from . import _abi
from .marshal import Buffers

# writetonc's default `vars` per height (dataprep.R:1108, 1179, 1232)
DEFAULT_VARS_ABOVE = ("Tz", "tleaf", "relhum", "windspeed", "Rdirdown", "Rdifdown", "Rlwdown", "Rswup", "Rlwup")
DEFAULT_VARS_SURFACE = ("Tz", "soilm", "Rdirdown", "Rdifdown", "Rlwdown", "Rswup", "Rlwup")
DEFAULT_VARS_BELOW = ("Tz", "soilm")


FORMATS = {"classic": 0, "netcdf4": 1}      # MCF_NC_CLASSIC, MCF_NC_NETCDF4


def default_vars(reqhgt: float) -> tuple:
    return DEFAULT_VARS_ABOVE if reqhgt > 0 else DEFAULT_VARS_SURFACE if reqhgt == 0 else DEFAULT_VARS_BELOW


def coords_from_extent(xmin, xmax, ymin, ymax, xres, yres=None):
    """`est` / `nth` of dataprep.R:1072-1073: cell centres, both ASCENDING (R's seq(from, to, by))."""
    yres = xres if yres is None else yres
    ne = int(np.floor((xmax - xres / 2 - (xmin + xres / 2)) / xres + 1e-10)) + 1
    nn = int(np.floor((ymax - yres / 2 - (ymin + yres / 2)) / yres + 1e-10)) + 1
    return xmin + xres / 2 + xres * np.arange(ne), ymin + yres / 2 + yres * np.arange(nn)


def hours_since_epoch(obstime: Mapping) -> np.ndarray:
    """as.numeric(as.POSIXct(tme)) / 3600 for a UTC obstime table (year, month, day, hour)."""
    y, m, d = (np.asarray(obstime[k]).astype(int) for k in ("year", "month", "day"))
    h = np.asarray(obstime["hour"], dtype=np.float64)
    return np.array([calendar.timegm((yy, mm, dd, 0, 0, 0)) / 3600.0 for yy, mm, dd in zip(y, m, d)]) + h


def _grid_fields(sp, b: Buffers, rows, cols, time_hours, east, north, crs_wkt, format, deflate_level):
    """the fields mcf_nc_spec and mcf_ncpack_spec share; -> what has to stay alive beside `b`"""
    t = np.ascontiguousarray(time_hours, dtype=np.float64)
    e = np.ascontiguousarray(east, dtype=np.float64)
    n = np.ascontiguousarray(north, dtype=np.float64)
    if e.shape != (cols,) or n.shape != (rows,):
        raise ValueError("east / north must have one entry per raster column / row")
    if format not in FORMATS:
        raise ValueError(f"format must be one of {sorted(FORMATS)}")
    sp.rows, sp.cols, sp.nsteps = rows, cols, len(t)
    sp.east, sp.north, sp.time_hours = b.ptr(e), b.ptr(n), b.ptr(t)
    wkt = (crs_wkt or "").encode()
    sp.crs_wkt = wkt
    sp.format = FORMATS[format]
    sp.deflate_level = int(deflate_level)       # netcdf4: 0 = writetonc's compression = 9, -1 = none
    return (t, e, n, wkt)


def nc_spec(rows: int, cols: int, time_hours, east, north, reqhgt: float, vars: Sequence[str] | None = None, crs_wkt: str = "",
            reference_puts_only: bool = False, format: str = "classic", deflate_level: int = 0):
    """include/mcf.h mcf_nc_spec -> (spec, the variables' names); the spec holds its arrays"""
    names = tuple(default_vars(reqhgt) if vars is None else vars)
    unknown = [v for v in names if v not in _abi.OUT_NAMES]
    if unknown:
        raise ValueError(f"unknown variables {unknown}")
    sp = _abi.NcSpec()
    sp._owner = b = Buffers()
    sp._keep = _grid_fields(sp, b, rows, cols, time_hours, east, north, crs_wkt, format, deflate_level)
    sp.reqhgt = float(reqhgt)
    for v in names:
        sp.vars[_abi.OUT_NAMES.index(v)] = 1
    sp.reference_puts_only = 1 if reference_puts_only else 0
    return sp, names


# the snowpack's file (include/mcf.h mcf_ncpack_spec): the library's table, which a caller may replace per series
SNOWPACK_SCALE = {"Tc": 100.0, "Tg": 100.0, "groundsnowdepth": 1000.0, "totalSWE": 100.0, "snowden": 1.0}
SNOWPACK_UNITS = {"Tc": "deg C x 100", "Tg": "deg C x 100", "groundsnowdepth": "mm", "totalSWE": "mm x 100", "snowden": "kg / m^3"}
SNOWPACK_LONG_NAME = {"Tc": "Canopy snow temperature", "Tg": "Ground snow temperature", "groundsnowdepth": "Ground snow depth",
                      "totalSWE": "Total snow water equivalent", "snowden": "Snow density"}


def ncpack_spec(rows: int, cols: int, time_hours, east, north, vars: Sequence[str] | None = None, crs_wkt: str = "",
                format: str = "classic", deflate_level: int = 0, scale: Mapping | None = None, units: Mapping | None = None,
                long_name: Mapping | None = None):
    """include/mcf.h mcf_ncpack_spec -> (spec, the series' names in the file's order); the spec holds its arrays"""
    sel = tuple(_abi.SNOWDRIVER_OUT if vars is None else vars)
    unknown = [v for v in sel if v not in _abi.SNOWDRIVER_OUT]
    if unknown:
        raise ValueError(f"unknown series {unknown}")
    sp = _abi.NcPackSpec()
    sp._owner = b = Buffers()
    sp._keep = [_grid_fields(sp, b, rows, cols, time_hours, east, north, crs_wkt, format, deflate_level)]
    for i, name in enumerate(_abi.SNOWDRIVER_OUT):
        if name not in sel:
            continue
        sp.series[i] = 1
        sp.scale[i] = float({**SNOWPACK_SCALE, **(scale or {})}[name])
        u = {**SNOWPACK_UNITS, **(units or {})}[name].encode()
        ln = {**SNOWPACK_LONG_NAME, **(long_name or {})}[name].encode()
        sp._keep.append((u, ln))
        sp.units[i], sp.long_name[i] = u, ln
    return sp, tuple(n for n in _abi.SNOWDRIVER_OUT if n in sel)


def grid_of(dtm: Mapping, obstime):
    """(hours since 1970, east, north, crs) of a `dtm` mapping {"xmin","xmax","ymin","ymax","res", optional "crs"} and an obstime
    table (or hours since 1970), as writetonc reads them"""
    hours = hours_since_epoch(obstime) if isinstance(obstime, Mapping) else np.asarray(obstime, dtype=np.float64)
    res = dtm["res"]
    xres, yres = (res, res) if np.isscalar(res) else res
    east, north = coords_from_extent(dtm["xmin"], dtm["xmax"], dtm["ymin"], dtm["ymax"], xres, yres)
    return hours, east, north, dtm.get("crs", "")


class NcWriter:
    def __init__(self, fileout: str, rows: int, cols: int, time_hours, east, north, reqhgt: float,
                 vars: Sequence[str] | None = None, crs_wkt: str = "", reference_puts_only: bool = False,
                 format: str = "classic", deflate_level: int = 0):
        self._lib = _abi.load()
        sp, self.vars = nc_spec(rows, cols, time_hours, east, north, reqhgt, vars, crs_wkt, reference_puts_only, format, deflate_level)
        self.rows, self.cols, self.nsteps = rows, cols, int(sp.nsteps)
        self._h = C.c_void_p()
        _abi.check(self._lib.mcf_nc_create(str(fileout).encode(), C.byref(sp), C.byref(self._h)))

    def write_host(self, step0: int, arrays: Mapping[str, np.ndarray]):
        """arrays[name]: [rows, cols, n] as runmicro*Cpp return them"""
        ptrs = (_abi.c_double_p * 10)()
        b, n = Buffers(), None
        for name in self.vars:
            if name not in arrays:
                continue
            a = np.asfortranarray(arrays[name], dtype=np.float64)
            if a.shape[:2] != (self.rows, self.cols) or (n is not None and a.shape[2] != n):
                raise ValueError(f"{name}: expected [rows, cols, n]")
            n = a.shape[2]
            ptrs[_abi.OUT_NAMES.index(name)] = b.ptr(a)
        if n is None:
            raise ValueError("no variable of the file given")
        _abi.check(self._lib.mcf_nc_write_host(self._h, int(step0), int(n), C.byref(ptrs)))

    def write_plan(self, plan, slot: int, slot_step0: int, file_step0: int, nsteps: int, timing: bool = False):
        ms = C.c_float()
        _abi.check(self._lib.mcf_nc_write_plan(self._h, plan._p, int(slot), int(slot_step0), int(file_step0), int(nsteps),
                                               C.byref(ms) if timing else None))
        return ms.value if timing else None

    def write_plan_rows(self, plan, slot: int, row0: int, slot_step0: int, file_step0: int, nsteps: int, depth: int = 0,
                        timing: bool = False):
        """the plan's rows as rows [row0, row0 + plan rows) of the file (a row block's plan); `depth`: the Tz slab of a streamed
        below-ground plan with a depth list"""
        ms = C.c_float()
        _abi.check(self._lib.mcf_nc_write_plan_rows(self._h, plan._p, int(slot), int(depth), int(row0), int(slot_step0),
                                                    int(file_step0), int(nsteps), C.byref(ms) if timing else None))
        return ms.value if timing else None

    def write_missing(self, row0: int, nrows: int, file_step0: int, nsteps: int):
        """missval in every variable of rows [row0, row0 + nrows) of records [file_step0, file_step0 + nsteps)"""
        _abi.check(self._lib.mcf_nc_write_missing(self._h, int(row0), int(nrows), int(file_step0), int(nsteps)))

    def write_host_rows(self, row0: int, step0: int, arrays: Mapping[str, np.ndarray]):
        """arrays[name]: [nrows, cols, n], rows [row0, row0 + nrows) of the file's grid"""
        ptrs = (_abi.c_double_p * 10)()
        b, shape = Buffers(), None
        for name in self.vars:
            if name not in arrays:
                continue
            a = np.asfortranarray(arrays[name], dtype=np.float64)
            if a.ndim != 3 or a.shape[1] != self.cols or (shape is not None and a.shape != shape):
                raise ValueError(f"{name}: expected [nrows, cols, n]")
            shape = a.shape
            ptrs[_abi.OUT_NAMES.index(name)] = b.ptr(a)
        if shape is None:
            raise ValueError("no variable of the file given")
        _abi.check(self._lib.mcf_nc_write_host_rows(self._h, int(row0), int(shape[0]), int(step0), int(shape[2]), C.byref(ptrs)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            h, self._h = self._h, C.c_void_p()
            _abi.check(self._lib.mcf_nc_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SnowpackNcWriter(NcWriter):
    """The snowpack's file (include/mcf.h mcf_nc_create_snowpack): the five series of the snow model as int32 variables."""

    def __init__(self, fileout: str, rows: int, cols: int, time_hours, east, north, vars: Sequence[str] | None = None,
                 crs_wkt: str = "", format: str = "classic", deflate_level: int = 0, **table):
        self._lib = _abi.load()
        sp, self.vars = ncpack_spec(rows, cols, time_hours, east, north, vars, crs_wkt, format, deflate_level, **table)
        self.rows, self.cols, self.nsteps = rows, cols, int(sp.nsteps)
        self._h = C.c_void_p()
        _abi.check(self._lib.mcf_nc_create_snowpack(str(fileout).encode(), C.byref(sp), C.byref(self._h)))

    def write_host(self, *a, **k):
        raise TypeError("a snowpack file takes planes (write_planes) or a snow plan's chunks")

    write_plan = write_plan_rows = write_host_rows = write_host

    def write_planes(self, row0: int, file_step0: int, arrays: Mapping[str, np.ndarray], device: int = 0, timing: bool = False):
        """arrays[series]: [nrows, cols, n]; packed on the device (k_pack_nc_planes) as rows [row0, row0 + nrows)"""
        ptrs = (_abi.c_double_p * 5)()
        b, shape = Buffers(), None
        for name in self.vars:
            a = np.asfortranarray(arrays[name], dtype=np.float64)      # [nrows, cols, n] column-major = step-major planes
            if a.ndim != 3 or a.shape[1] != self.cols or (shape is not None and a.shape != shape):
                raise ValueError(f"{name}: expected [nrows, cols, n]")
            shape = a.shape
            ptrs[_abi.SNOWDRIVER_OUT.index(name)] = b.ptr(a)
        ms = C.c_float()
        _abi.check(self._lib.mcf_nc_write_planes(self._h, C.byref(ptrs), int(shape[0]), int(row0), int(file_step0), int(shape[2]),
                                                 int(device), C.byref(ms) if timing else None))
        return ms.value if timing else None


def writetonc(mout: Mapping, fileout: str, dtm: Mapping, reqhgt: float, vars: Sequence[str] | None = None,
              reference_puts_only: bool = False, format: str = "classic", deflate_level: int = 0):
    """`writetonc(mout, fileout, dtm, reqhgt, vars)`: `mout` holds the output arrays and `tme` (an obstime table or
    hours since 1970); `dtm` = {"xmin","xmax","ymin","ymax","res", optional "crs"} stands for the SpatRaster."""
    names = tuple(default_vars(reqhgt) if vars is None else vars)
    first = np.asarray(mout[next(v for v in names if v in mout)])
    rows, cols = first.shape[:2]
    tme = mout["tme"]
    hours = hours_since_epoch(tme) if isinstance(tme, Mapping) else np.asarray(tme, dtype=np.float64)
    res = dtm["res"]
    xres, yres = (res, res) if np.isscalar(res) else res
    east, north = coords_from_extent(dtm["xmin"], dtm["xmax"], dtm["ymin"], dtm["ymax"], xres, yres)
    with NcWriter(fileout, rows, cols, hours, east, north, reqhgt, names, dtm.get("crs", ""), reference_puts_only,
                  format=format, deflate_level=deflate_level) as w:
        w.write_host(0, {k: mout[k] for k in names if k in mout})
