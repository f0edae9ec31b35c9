"""Host-side mirror of the reference's operator interface for the grid solver.

`runmicro1Cpp` / `runmicro2Cpp` take the same 15 positional arguments, with the
same names and meaning, as the R functions of the reference
(R/RcppExports.R:72-78) that `.runmodel1Cpp` / `.runmodel2Cpp` call
(R/internal.R:1168, 1342): R named lists / data.frames become Python mappings
of numpy arrays, R's column-major arrays become Fortran-ordered numpy arrays,
and the returned named list becomes a dict holding only the requested
variables, in the reference's order (src/microclimfCpp.cpp:2326-2335), each of
shape (rows, cols, tsteps).

All arithmetic happens in libmcfhip.so (hand-written HIP, gfx950); this module
only marshals pointers.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Sequence

import numpy as np

from . import _abi
from .marshal import Buffers, Marshalled, alloc_outputs, build_summary_spec, marshal, summary_sink


DTM_DERIVED = ("slope", "aspect", "hor", "svfa", "wsa", "twi")      # soilc entries a plan can derive from the dtm


def dtm_spec(dtm: Mapping, rows: int, cols: int):
    """include/mcf.h mcf_dtm_spec from `dtm` = {z, res[, halo_north, halo_south, row0, rows_total, agg]}: `z` is the block's
    elevations [(halo_north + rows + halo_south), cols] (NaN = NA), `res` one number or (xres, yres).  -> the spec (it holds
    the array behind its pointer)"""
    z = np.asfortranarray(np.asarray(dtm["z"], dtype=np.float64))
    hn, hs = int(dtm.get("halo_north", 0)), int(dtm.get("halo_south", 0))
    if z.shape != (hn + rows + hs, cols):
        raise ValueError(f"dtm$z: expected shape {(hn + rows + hs, cols)}, got {z.shape}")
    res = dtm["res"]
    xres, yres = (res, res) if np.isscalar(res) else res
    sp = _abi.DtmSpec()
    sp._owner = Buffers()
    sp.dtm = sp._owner.ptr(z)
    sp.halo_north, sp.halo_south = hn, hs
    sp.row0, sp.rows_total = int(dtm.get("row0", 0)), int(dtm.get("rows_total", 0))
    sp.xres, sp.yres, sp.agg = float(xres), float(yres), int(dtm.get("agg", 0))
    return sp


def diag_selection(names):
    """(int32[13] selection, the selected names in include/mcf.h mcf_diag order) from diagnostic names or indices;
    "all": every one"""
    if isinstance(names, str):
        names = _abi.DIAG_NAMES if names == "all" else (names,)
    idx = sorted({_abi.DIAG_NAMES.index(n) if isinstance(n, str) else int(n) for n in names})
    if not idx or idx[0] < 0 or idx[-1] >= _abi.NDIAG:
        raise ValueError(f"diagnostics: a non-empty selection of {_abi.DIAG_NAMES}")
    sel = (C.c_int32 * _abi.NDIAG)(*[1 if v in idx else 0 for v in range(_abi.NDIAG)])
    return sel, [_abi.DIAG_NAMES[v] for v in idx]


def summary_spec(periods, vars, stats, thresholds=None):
    """include/mcf.h mcf_summary_spec from `periods` (one integer per day, -1 = not counted), output names or indices, names
    of _abi.STAT_NAMES or indices, and `thresholds` for hours_above: one number for every selected variable or {variable:
    number}.  -> (spec, the selected variables' indices, the selected statistics' indices, the period table the spec holds)"""
    return build_summary_spec(_abi.SummarySpec, _abi.OUT_NAMES, "var", "summary: variables", periods, vars, stats, thresholds)


def runmicro_summary(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping, reqhgt: float,
                     zref: float, lat, lon, Sminp: float, Smaxp: float, tfact: float, complete: bool, mat: float, *, periods,
                     vars=("Tz",), stats=("mean", "min", "max"), thresholds=None, nperiods: int | None = None,
                     chunk_days: int = 0, array_forcing: bool = False, dfsel: Mapping | None = None, coarse: Mapping | None = None,
                     device: int = 0, cells_per_block: int = 0, devices=None, n_blocks: int = 0, dtm: Mapping | None = None) -> dict:
    """Per-cell statistics of the solver's outputs over periods of days, accumulated on the device chunk by chunk (include/mcf.h
    "period summaries", mcf_runmicro_summary): the argument lists of runmicro1Cpp .. 4Cpp (`array_forcing`, `dfsel`, and
    `coarse` as for runmicro2Cpp_coarse's marshalling) without `out` — the selection `vars` is what the solver computes.
    `periods`: one integer per whole day (-1: not counted); `nperiods` (default: the largest + 1) allows trailing periods
    without a day.  `devices` / `n_blocks`: row blocks over several devices (vector forcing), same bits.  `dtm`: missing
    terrain planes derived on the device — that route runs the plan API from here (Plan(dtm=...)), one device.
    -> {variable: {statistic: [rows, cols, nperiods]}, "days": counted days per period}"""
    sp, vi, si, _pod = summary_spec(periods, vars, stats, thresholds)
    if nperiods is not None:
        sp.nperiods = int(nperiods)
    out = [1 if v in vi else 0 for v in range(_abi.NOUT)]
    af = bool(array_forcing) or coarse is not None
    if dtm is not None:
        if devices is not None or n_blocks:
            raise ValueError("dtm= is not available with devices= / n_blocks=")
        nd = len(np.asarray(obstime["year"])) // 24
        ring = max(1, min(nd, int(chunk_days) if chunk_days else 8))
        with Plan(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, complete, mat, out,
                  array_forcing=af, ring_days=ring, device=device, cells_per_block=cells_per_block, dfsel=dfsel, coarse=coarse,
                  dtm=dtm) as p:
            p.summary_enable(_pod, vi, si, thresholds, nperiods=sp.nperiods)
            p.summarise_days(ring)
            return summary_sink(Buffers(), p.rows, p.cols, (sp, vi, si, _pod), _abi.OUT_NAMES,
                                plane=lambda v, s, ptr: _abi.check(p._lib.mcf_plan_summary_fetch(p._p, v, s, ptr)),
                                days=lambda ptr: _abi.check(p._lib.mcf_plan_summary_days(p._p, ptr)))
    lib = _abi.load()
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, complete, mat, out, af,
                device, 0, cells_per_block, dfsel, coarse)
    so = _abi.SummaryOut()
    res = summary_sink(m, m.rows, m.cols, (sp, vi, si, _pod), _abi.OUT_NAMES, so)
    mu = _abi.multi(devices, n_blocks)
    if mu:
        _abi.check(lib.mcf_runmicro_summary_multi(C.byref(m.inputs), C.byref(m.options), C.byref(sp), int(chunk_days), C.byref(mu[0]),
                                                  C.byref(so)))
    else:
        _abi.check(lib.mcf_runmicro_summary(C.byref(m.inputs), C.byref(m.options), C.byref(sp), int(chunk_days), C.byref(so)))
    return res


def _names_to_indices(sel, names, what):
    idx = sorted({names.index(v) if isinstance(v, str) else int(v) for v in ((sel,) if isinstance(sel, str) else sel)})
    if any(v < 0 or v >= len(names) for v in idx):
        raise ValueError(f"{what} of {names}")
    return idx


def series_spec(rows: int, cols: int, points=None, zones=None, vars=("Tz",), stats=("mean", "min", "max"), nzones: int | None = None,
                *, struct=_abi.SeriesSpec, names=_abi.OUT_NAMES, field: str = "var"):
    """include/mcf.h mcf_series_spec: `points` 0-based cell indices row + rows * col (None: no points), `zones` a [rows, cols]
    integer array of labels (negative or masked: in no zone; None: no zones), `nzones` default the largest label + 1, `vars`
    output names or indices, `stats` names of _abi.ZSTAT_NAMES or indices.  struct / names / field: another spec of the same
    layout (mcf_snowpack_series_spec: its five series under "series").
    -> (spec, the selected variables' indices, the selected statistics' indices); the spec holds its arrays"""
    vi = _names_to_indices(vars, names, "series: variables")
    si = _names_to_indices(stats, _abi.ZSTAT_NAMES, "series: statistics")
    sp = struct()
    sp._owner = b = Buffers()
    if points is not None:
        cells = np.ascontiguousarray(np.asarray(points, dtype=np.int64)).ravel()
        sp.npoints, sp.cells = cells.size, b.ptr(cells)
    if zones is not None:
        z = np.ma.masked_invalid(zones) if np.asarray(zones).dtype.kind == "f" else np.ma.asarray(zones)
        if z.shape != (rows, cols):
            raise ValueError(f"zones: expected shape {(rows, cols)}, got {z.shape}")
        lab = np.asfortranarray(np.where(np.ma.getmaskarray(z) | (z.filled(-1) < 0), -1, z.filled(-1)).astype(np.int32))
        sp.nzones = int(nzones) if nzones is not None else int(lab.max()) + 1
        sp.zone = b.ptr(lab)
    for v in vi:
        getattr(sp, field)[v] = 1
    for k in si:
        sp.zstat[k] = 1
    return sp, vi, si


def _series_sink(b: Buffers, tsteps: int, sp, vi, si, so=None, points=None, zones=None, names=_abi.OUT_NAMES) -> dict:
    """The host side of a series sink: one [tsteps, npoints] array per selected variable and one [tsteps, nzones] array per
    selected (variable, statistic), held by `b`; their pointers go into `so` (mcf_series_out) or to points(v, pointer) /
    zones(v, k, pointer) -> {"points": {variable: array}, "zones": {variable: {statistic: array}}}"""
    res = {"points": {}, "zones": {}}
    for v in vi:
        name = names[v]
        if sp.npoints > 0:
            res["points"][name], ptr = b.out((tsteps, int(sp.npoints)))
            if so is not None:
                so.points[v] = ptr
            else:
                points(v, ptr)
        if sp.nzones > 0:
            res["zones"][name] = {}
            for k in si:
                res["zones"][name][_abi.ZSTAT_NAMES[k]], ptr = b.out((tsteps, int(sp.nzones)))
                if so is not None:
                    so.zones[v][k] = ptr
                else:
                    zones(v, k, ptr)
    return res


def runmicro_series(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping, reqhgt: float,
                    zref: float, lat, lon, Sminp: float, Smaxp: float, tfact: float, complete: bool, mat: float, *, points=None,
                    zones=None, vars=("Tz",), stats=("mean", "min", "max"), nzones: int | None = None, chunk_days: int = 0,
                    array_forcing: bool = False, dfsel: Mapping | None = None, coarse: Mapping | None = None, device: int = 0,
                    cells_per_block: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """The hourly series at a few cells and per-step statistics over zones of the raster, accumulated on the device chunk by
    chunk (include/mcf.h "series sink", mcf_runmicro_series): runmicro_summary's argument lists; `points`, `zones`, `vars`,
    `stats`, `nzones` as series_spec takes them.  `devices` / `n_blocks`: row blocks over several devices (vector forcing;
    mcf_runmicro_series_multi), same bits.
    -> {"points": {variable: [tsteps, npoints]}, "zones": {variable: {statistic: [tsteps, nzones]}}}"""
    hgt = np.asarray(vegp["hgt"])
    sp, vi, si = series_spec(hgt.shape[0], hgt.shape[1], points, zones, vars, stats, nzones)
    out = [1 if v in vi else 0 for v in range(_abi.NOUT)]
    lib = _abi.load()
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, complete, mat, out,
                bool(array_forcing) or coarse is not None, device, 0, cells_per_block, dfsel, coarse)
    so = _abi.SeriesOut()
    res = _series_sink(m, m.tsteps, sp, vi, si, so)
    mu = _abi.multi(devices, n_blocks)
    if mu:
        _abi.check(lib.mcf_runmicro_series_multi(C.byref(m.inputs), C.byref(m.options), C.byref(sp), int(chunk_days), C.byref(mu[0]),
                                                 C.byref(so)))
    else:
        _abi.check(lib.mcf_runmicro_series(C.byref(m.inputs), C.byref(m.options), C.byref(sp), int(chunk_days), C.byref(so)))
    return res


def zonal_series(x, zones, stats=("mean", "min", "max"), device: int = 0, nzones: int | None = None) -> dict:
    """The zone series of a host array x[rows, cols, nsteps] (include/mcf.h mcf_zonal_series): `zones` and `stats` as
    series_spec takes them -> {statistic: [nsteps, nzones]}"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("x: a [rows, cols, nsteps] array")
    sp, _vi, si = series_spec(x.shape[0], x.shape[1], None, zones, (0,), stats, nzones)
    b = Buffers()
    res, ptrs = {}, (_abi.c_double_p * _abi.NZSTAT)()
    for k in si:
        res[_abi.ZSTAT_NAMES[k]], ptrs[k] = b.out((x.shape[2], max(int(sp.nzones), 0)))
    _abi.check(_abi.load().mcf_zonal_series(b.ptr(np.asfortranarray(x)), x.shape[0], x.shape[1], x.shape[2], sp.zone, sp.nzones,
                                            sp.zstat, int(device), ptrs))
    return res


def _depth_list(depths, tbp, tsteps):
    """(depths as float64, tbp as C-ordered [ndepths, tsteps] or None) for the C ABI"""
    d = np.ascontiguousarray(np.atleast_1d(np.asarray(depths, dtype=np.float64))).ravel()
    t = None
    if tbp is not None:
        t = np.ascontiguousarray(np.asarray(tbp, dtype=np.float64))
        if t.shape != (d.size, tsteps):
            raise ValueError(f"tbp: expected shape {(d.size, tsteps)} (one row of the point model's soil temperature per depth), got {t.shape}")
    return d, t


def runmicro_depths(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping, depths, zref: float,
                    lat, lon, Sminp: float, Smaxp: float, tfact: float, complete: bool, mat: float, *, tbp=None, soilm: bool = True,
                    array_forcing: bool = False, dfsel: Mapping | None = None, coarse: Mapping | None = None, device: int = 0,
                    days_per_chunk: int = 0, cells_per_block: int = 0) -> dict:
    """Below ground at several depths from one solve (include/mcf.h mcf_runmicro_depths): the argument list of runmicro1Cpp with
    `depths` (each < 0, any order, at most _abi.MAX_DEPTHS) in place of reqhgt and without `out`.  `tbp`: [ndepths, tsteps], the
    point model's soil temperature at each depth (pointm$Tbp of a run at that depth), needed with complete = False.
    `array_forcing` / `coarse` (complete = True only) and `dfsel` as for runmicro_summary.
    -> {"Tz": [one [rows, cols, tsteps] array per depth], "soilm": [rows, cols, tsteps] (with soilm=True), "depths": depths}:
    every array has the bits of runmicro1Cpp at that depth."""
    lib = _abi.load()
    af = bool(array_forcing) or coarse is not None
    T = len(np.asarray(obstime["year"]))
    d, t = _depth_list(depths, tbp, T)
    reqhgt = float(d[0]) if d.size and d[0] < 0 else -1.0          # (the library judges the list)
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, complete, mat,
                [1, 0, 0, 1 if soilm else 0, 0, 0, 0, 0, 0, 0], af, device, days_per_chunk, cells_per_block, dfsel, coarse)
    do = _abi.DepthOutputs()
    res = {"Tz": [], "depths": d.copy()}
    for i in range(min(d.size, _abi.MAX_DEPTHS)):
        a, do.tz[i] = m.out((m.rows, m.cols, m.tsteps))
        res["Tz"].append(a)
    if soilm:
        res["soilm"], do.soilm = m.out((m.rows, m.cols, m.tsteps))
    _abi.check(lib.mcf_runmicro_depths(C.byref(m.inputs), C.byref(m.options), m.ptr(d), int(d.size), m.ptr(t), C.byref(do)))
    return res


def runmicro_nc(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping, reqhgt: float, zref: float,
                lat, lon, Sminp: float, Smaxp: float, tfact: float, complete: bool, mat: float, *, fileout: str, grid: Mapping,
                vars=None, format: str = "classic", deflate_level: int = 0, reference_puts_only: bool = False,
                array_forcing: bool = False, dfsel: Mapping | None = None, coarse: Mapping | None = None, device: int = 0,
                days_per_chunk: int = 0, cells_per_block: int = 0, devices=None, n_blocks: int = 0) -> tuple:
    """The solver's outputs straight into a `writetonc` file (include/mcf.h mcf_runmicro_nc): the argument lists of runmicro1Cpp ..
    4Cpp without `out` — the file's variables `vars` (ncsink.default_vars(reqhgt) by default) are what the solver computes —
    every chunk packed on the device and written while the next is solved; no [rows, cols, tsteps] array on the host.  reqhgt < 0
    runs the streamed below-ground plan.  `grid`: the mapping ncsink.writetonc takes as `dtm` (extent, res, crs).  `devices` /
    `n_blocks`: row blocks, each writing its row strips of the one file (classic container).  The classic file is byte for byte
    ncsink.writetonc of runmicro1Cpp's arrays.  -> the file's variable names"""
    from . import ncsink
    lib = _abi.load()
    hours, east, north, crs = ncsink.grid_of(grid, obstime)
    hgt = np.asarray(vegp["hgt"])
    sp, names = ncsink.nc_spec(hgt.shape[0], hgt.shape[1], hours, east, north, reqhgt, vars, crs, reference_puts_only, format,
                               deflate_level)
    out = [1 if n in names else 0 for n in _abi.OUT_NAMES]
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, complete, mat, out,
                bool(array_forcing) or coarse is not None, device, days_per_chunk, cells_per_block, dfsel, coarse)
    mu = _abi.multi(devices, n_blocks)
    _abi.check(lib.mcf_runmicro_nc(C.byref(m.inputs), C.byref(m.options), C.byref(mu[0]) if mu else None, str(fileout).encode(),
                                   C.byref(sp)))
    return names


def runmicro_depths_nc(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping, depths, zref: float,
                       lat, lon, Sminp: float, Smaxp: float, tfact: float, complete: bool, mat: float, *, files, grid: Mapping,
                       tbp=None, soilm: bool = True, format: str = "classic", deflate_level: int = 0,
                       array_forcing: bool = False, dfsel: Mapping | None = None, coarse: Mapping | None = None, device: int = 0,
                       days_per_chunk: int = 0, cells_per_block: int = 0) -> None:
    """runmicro_depths into one `writetonc` file per depth (include/mcf.h mcf_runmicro_depths_nc): files[d] holds Tz at
    depths[d] under that depth's long name and, with soilm=True, the soil moisture (the same plane in every file)."""
    from . import ncsink
    lib = _abi.load()
    af = bool(array_forcing) or coarse is not None
    T = len(np.asarray(obstime["year"]))
    d, t = _depth_list(depths, tbp, T)
    files = [str(f).encode() for f in files]
    if len(files) != d.size:
        raise ValueError("files: one path per depth")
    reqhgt = float(d[0]) if d.size and d[0] < 0 else -1.0          # (the library judges the list)
    hours, east, north, crs = ncsink.grid_of(grid, obstime)
    hgt = np.asarray(vegp["hgt"])
    sp, names = ncsink.nc_spec(hgt.shape[0], hgt.shape[1], hours, east, north, reqhgt, ("Tz", "soilm") if soilm else ("Tz",), crs,
                               False, format, deflate_level)
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, complete, mat,
                [1, 0, 0, 1 if soilm else 0, 0, 0, 0, 0, 0, 0], af, device, days_per_chunk, cells_per_block, dfsel, coarse)
    paths = (C.c_char_p * max(len(files), 1))(*files)
    _abi.check(lib.mcf_runmicro_depths_nc(C.byref(m.inputs), C.byref(m.options), m.ptr(d), int(d.size), m.ptr(t), paths, C.byref(sp)))


def runmicro_depths_summary(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping, depths,
                            zref: float, lat, lon, Sminp: float, Smaxp: float, tfact: float, complete: bool, mat: float, *,
                            periods, tbp=None, vars=("Tz",), stats=("mean", "min", "max"), thresholds=None,
                            nperiods: int | None = None, chunk_days: int = 0, array_forcing: bool = False,
                            dfsel: Mapping | None = None, coarse: Mapping | None = None, device: int = 0,
                            cells_per_block: int = 0) -> dict:
    """Period summaries below ground at several depths (include/mcf.h mcf_runmicro_depths_summary): runmicro_depths with each
    chunk folded on the device as it is produced.  `vars` among Tz and soilm; `periods`, `stats`, `thresholds`, `nperiods` as
    for runmicro_summary.
    -> {"Tz": [per depth {statistic: [rows, cols, nperiods]}], "soilm": {statistic: ...} (if selected), "days", "depths"}"""
    lib = _abi.load()
    sp, vi, si, _pod = summary_spec(periods, vars, stats, thresholds)
    if nperiods is not None:
        sp.nperiods = int(nperiods)
    af = bool(array_forcing) or coarse is not None
    T = len(np.asarray(obstime["year"]))
    d, t = _depth_list(depths, tbp, T)
    reqhgt = float(d[0]) if d.size and d[0] < 0 else -1.0
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, complete, mat,
                [1, 0, 0, 1, 0, 0, 0, 0, 0, 0], af, device, 0, cells_per_block, dfsel, coarse)
    so = _abi.DepthSummaryOut()
    res = {"depths": d.copy()}

    def sink(name, row, **kw):
        """the planes of one variable into one row [statistic] of the out struct"""
        one = (sp, [_abi.OUT_NAMES.index(name)] if name else [], si, _pod)
        return summary_sink(m, m.rows, m.cols, one, _abi.OUT_NAMES, plane=lambda v, k, ptr: row.__setitem__(k, ptr), **kw)
    if _abi.OUT_NAMES.index("Tz") in vi:
        res["Tz"] = [sink("Tz", so.tz[i])["Tz"] for i in range(min(d.size, _abi.MAX_DEPTHS))]
    if _abi.OUT_NAMES.index("soilm") in vi:
        res["soilm"] = sink("soilm", so.soilm)["soilm"]
    res["days"] = sink(None, None, days=lambda ptr: setattr(so, "days", ptr))["days"]
    _abi.check(lib.mcf_runmicro_depths_summary(C.byref(m.inputs), C.byref(m.options), m.ptr(d), int(d.size), m.ptr(t), C.byref(sp),
                                               int(chunk_days), C.byref(so)))
    return res


def runmicro_depths_series(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping, depths,
                           zref: float, lat, lon, Sminp: float, Smaxp: float, tfact: float, complete: bool, mat: float, *,
                           points=None, zones=None, tbp=None, vars=("Tz",), stats=("mean", "min", "max"), nzones: int | None = None,
                           chunk_days: int = 0, array_forcing: bool = False, dfsel: Mapping | None = None,
                           coarse: Mapping | None = None, device: int = 0, cells_per_block: int = 0) -> dict:
    """The series sink below ground at several depths (include/mcf.h mcf_runmicro_depths_series): runmicro_depths with each
    chunk folded on the device as it is produced.  `vars` among Tz and soilm; `points`, `zones`, `stats`, `nzones` as
    series_spec takes them.
    -> {"Tz": [per depth {"points": [tsteps, npoints], "zones": {statistic: [tsteps, nzones]}}], "soilm": {...} (if selected),
    "depths"}"""
    lib = _abi.load()
    hgt = np.asarray(vegp["hgt"])
    sp, vi, si = series_spec(hgt.shape[0], hgt.shape[1], points, zones, vars, stats, nzones)
    af = bool(array_forcing) or coarse is not None
    T = len(np.asarray(obstime["year"]))
    d, t = _depth_list(depths, tbp, T)
    reqhgt = float(d[0]) if d.size and d[0] < 0 else -1.0
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, complete, mat,
                [1, 0, 0, 1, 0, 0, 0, 0, 0, 0], af, device, 0, cells_per_block, dfsel, coarse)
    so = _abi.DepthSeriesOut()
    res = {"depths": d.copy()}

    def sink(v, set_points, zrow):
        """the arrays of one (variable, depth): {"points": ..., "zones": {statistic: ...}}"""
        one = _series_sink(m, m.tsteps, sp, [v], si, points=lambda _v, ptr: set_points(ptr), zones=lambda _v, k, ptr: zrow.__setitem__(k, ptr))
        name = _abi.OUT_NAMES[v]
        return {"points": one["points"].get(name), "zones": one["zones"].get(name, {})}
    tz, sm = _abi.OUT_NAMES.index("Tz"), _abi.OUT_NAMES.index("soilm")
    if tz in vi:
        res["Tz"] = [sink(tz, lambda ptr, i=i: so.tz_points.__setitem__(i, ptr), so.tz_zones[i]) for i in range(min(d.size, _abi.MAX_DEPTHS))]
    if sm in vi:
        res["soilm"] = sink(sm, lambda ptr: setattr(so, "soilm_points", ptr), so.soilm_zones)
    _abi.check(lib.mcf_runmicro_depths_series(C.byref(m.inputs), C.byref(m.options), m.ptr(d), int(d.size), m.ptr(t), C.byref(sp),
                                              int(chunk_days), C.byref(so)))
    return res


def foliageden(hgt, pai, z: float, device: int | None = None):
    """The foliage profile of `.foliageden` (R/internal.R:937-946; include/mcf.h mcf_foliageden) at height `z`, elementwise over
    `hgt` and `pai` (any shape, the same): -> (leafden, paia).  device=None: the host twin; an ordinal: one kernel launch there.
    Both come from one copy of the arithmetic (closed-form gamma functions of shape 3/2)."""
    lib = _abi.load()
    h = np.asfortranarray(np.asarray(hgt, dtype=np.float64))
    p = np.asfortranarray(np.asarray(pai, dtype=np.float64))
    if h.shape != p.shape:
        raise ValueError(f"foliageden: hgt {h.shape} and pai {p.shape} differ in shape")
    b = Buffers()
    (ld, ldp), (pa, pap) = b.out(h.shape), b.out(h.shape)
    if device is None:
        _abi.check(lib.mcf_foliageden(int(h.size), b.ptr(h), b.ptr(p), float(z), ldp, pap))
    else:
        _abi.check(lib.mcf_foliageden_device(int(h.size), b.ptr(h), b.ptr(p), float(z), ldp, pap, int(device)))
    return ld, pa


def runmicro_heights(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping, heights, zref: float,
                     lat, lon, Sminp: float, Smaxp: float, tfact: float, complete: bool, mat: float, out: Sequence = (1,) * 10, *,
                     pai_a=None, dfsel: Mapping | None = None, coarse: Mapping | None = None, device: int = 0,
                     days_per_chunk: int = 0, cells_per_block: int = 0) -> dict:
    """A height profile from one plan (include/mcf.h mcf_runmicro_heights): the argument list of runmicro1Cpp (`dfsel`:
    runmicro3Cpp; `coarse`: runmicro2Cpp_coarse, lat / lon then the rasters) with `heights` (each > 0) in place of reqhgt.
    vegp needs no paia / leafden: both are derived on the device per height; `pai_a`: None, or one entry per height, each None or
    the plant area above that height [rows, cols(, layers)] to use instead of the derived one.
    -> {"heights": heights, variable: [one [rows, cols, tsteps] array per height]}: the bits of a Plan moved through the heights."""
    lib = _abi.load()
    hs = np.ascontiguousarray(np.atleast_1d(np.asarray(heights, dtype=np.float64))).ravel()
    m = marshal(obstime, climdata, pointm, vegp, soilc, float(hs[0]) if hs.size else 0.0, zref, lat, lon, Sminp, Smaxp, tfact,
                complete, mat, out, coarse is not None, device, days_per_chunk, cells_per_block, dfsel, coarse,
                vegp_optional=("paia", "leafden"))
    L = max(int(m.inputs.veg_layers), 1)
    outs = (_abi.Outputs * max(hs.size, 1))()
    res = {"heights": hs.copy()}
    for h in range(hs.size):
        _o, arrays = alloc_outputs(m)
        outs[h] = _o
        for k, a in arrays.items():
            res.setdefault(k, []).append(a)
    pp = None
    if pai_a is not None:
        if len(pai_a) != hs.size:
            raise ValueError(f"pai_a: one entry per height ({hs.size}), each None or an array")
        pp = (_abi.c_double_p * max(hs.size, 1))()
        for h, a in enumerate(pai_a):
            if a is None:
                continue
            a = np.asfortranarray(np.asarray(a, dtype=np.float64))
            if a.ndim == 3 and a.shape[2] > L:
                a = a[:, :, :L]                  # as marshal() reads layered vegetation: the first L layers, no copy
            if a.size != m.rows * m.cols * L:
                raise ValueError(f"pai_a[{h}]: expected {m.rows} x {m.cols} x {L} values, got shape {a.shape}")
            pp[h] = m.ptr(a)
    _abi.check(lib.mcf_runmicro_heights(C.byref(m.inputs), C.byref(m.options), m.ptr(hs) if hs.size else None, int(hs.size), pp, outs))
    return res


def _run(fn_name, array_forcing, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon,
         Sminp, Smaxp, tfact, complete, mat, out, device, days_per_chunk, cells_per_block, dfsel=None, coarse=None,
         devices=None, n_blocks=0, dtm=None, diag=None):
    lib = _abi.load()
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp,
                tfact, complete, mat, out, array_forcing, device, days_per_chunk, cells_per_block, dfsel, coarse,
                soilc_optional=DTM_DERIVED if dtm is not None else ())
    outs, arrays = alloc_outputs(m)
    mu = _abi.multi(devices, n_blocks)
    if diag is not None:
        # the staged model's diagnostics beside the outputs (include/mcf.h mcf_runmicro1_diag): one device, no dtm form
        if mu or dtm is not None:
            raise ValueError("diag= is not available with devices= / n_blocks= / dtm=")
        sel, names = diag_selection(diag)
        dout = _abi.DiagOutputs()
        darr = {}
        for n in names:
            darr[n], dout.var[_abi.DIAG_NAMES.index(n)] = m.out((m.rows, m.cols, m.tsteps))
        _abi.check(getattr(lib, fn_name + "_diag")(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(outs),
                                                   C.byref(dout)))
        arrays["diag"] = darr
        return arrays
    if dtm is not None:
        # missing terrain planes / wetness index derived on the device (include/mcf.h mcf_runmicro_dtm); the entry dispatches on
        # the inputs as mcf_runmicro1 .. 4 do
        sp = dtm_spec(dtm, m.rows, m.cols)
        _abi.check(lib.mcf_runmicro_dtm(C.byref(m.inputs), C.byref(m.options), C.byref(sp), C.byref(mu[0]) if mu else None,
                                        C.byref(outs)))
        return arrays
    if mu:
        # one process, several devices (include/mcf.h mcf_runmicro1_multi): row blocks dealt to the listed devices
        _abi.check(getattr(lib, fn_name + "_multi")(C.byref(m.inputs), C.byref(m.options), C.byref(mu[0]), C.byref(outs)))
        return arrays
    _abi.check(getattr(lib, fn_name)(C.byref(m.inputs), C.byref(m.options), C.byref(outs)))
    return arrays


def runmicro1Cpp(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping,
                 reqhgt: float, zref: float, lat: float, lon: float, Sminp: float, Smaxp: float,
                 tfact: float, complete: bool, mat: float, out: Sequence, *, device: int = 0,
                 days_per_chunk: int = 0, cells_per_block: int = 0, devices=None, n_blocks: int = 0, dtm: Mapping | None = None,
                 diag=None) -> dict:
    """Grid microclimate model, hourly, static vegetation, data.frame (vector) climate.

    Drop-in for the reference's runmicro1Cpp (src/microclimfCpp.cpp:2052-2337).  `devices` (a list of HIP ordinals, [] =
    all visible) / `n_blocks`: the raster in row blocks over several devices from this one process, same bits.
    `dtm` = {z, res[, halo_north, halo_south, row0, rows_total, agg]}: entries of `soilc` among slope, aspect, hor, svfa, wsa,
    twi that are missing are derived from the elevations on the device, straight into the plan (include/mcf.h mcf_dtm_spec).
    `diag` (names of include/mcf.h mcf_diag, or "all"; reqhgt >= 0): the staged model's diagnostics of the same run, returned
    as a dict under the key "diag"; the default None returns exactly the ten-variable dict."""
    return _run("mcf_runmicro1", False, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon,
                Sminp, Smaxp, tfact, complete, mat, out, device, days_per_chunk, cells_per_block, devices=devices, n_blocks=n_blocks, dtm=dtm,
                diag=diag)


def runmicro2Cpp(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping,
                 reqhgt: float, zref: float, lats, lons, Sminp: float, Smaxp: float, tfact: float,
                 complete: bool, mat: float, out: Sequence, *, device: int = 0,
                 days_per_chunk: int = 0, cells_per_block: int = 0, devices=None, n_blocks: int = 0, dtm: Mapping | None = None,
                 diag=None) -> dict:
    """Grid microclimate model, hourly, static vegetation, array climate inputs.

    Drop-in for the reference's runmicro2Cpp (src/microclimfCpp.cpp:2340-2621); `devices` / `n_blocks` as runmicro1Cpp;
    `diag`: as runmicro1Cpp (include/mcf.h mcf_runmicro2_diag)."""
    return _run("mcf_runmicro2", True, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons,
                Sminp, Smaxp, tfact, complete, mat, out, device, days_per_chunk, cells_per_block, devices=devices, n_blocks=n_blocks, dtm=dtm,
                diag=diag)


def coarse_positions(n_fine: int, n_coarse: int):
    """Position of each of `n_fine` equally spaced fine cells in units of `n_coarse` coarse cells covering the same
    extent (0 = centre of the first coarse cell), clamped to the coarse centres (edge replication)."""
    pos = (np.arange(n_fine) + 0.5) * (n_coarse / n_fine) - 0.5
    return np.clip(pos, 0.0, n_coarse - 1.0)


def runmicro2Cpp_coarse(obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping, soilc: Mapping,
                        reqhgt: float, zref: float, lats, lons, Sminp: float, Smaxp: float, tfact: float,
                        complete: bool, mat: float, out: Sequence, *, rowpos=None, colpos=None, altcorrect: int = 0,
                        dtmc=None, dtm=None, device: int = 0, days_per_chunk: int = 0, devices=None, n_blocks: int = 0,
                        diag=None) -> dict:
    """`.runmodel2Cpp` with the resampling fused into the solver (include/mcf.h, array_forcing == 2): `climdata` =
    {temp, relhum, pres, swdown, difrad, lwdown, windspeed, winddir} and `pointm` = {soilm, Gp, umu, kp, muGp, dtrp} as
    COARSE arrays [coarse_rows, coarse_cols, tsteps] — what `.cca(..., dtmc, dtmc)` gives before `resample` — instead of
    the full-resolution arrays runmicro2Cpp takes.  `rowpos` / `colpos`: see `coarse_positions` (default: the coarse
    grid covers the raster's extent).  `diag`: as runmicro1Cpp — the diagnostics of the interpolated (and altitude-corrected) weather."""
    coarse = _coarse_spec(vegp, climdata, rowpos, colpos, altcorrect, dtmc, dtm, refuse_missing=False)
    return _run("mcf_runmicro2", True, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons,
                Sminp, Smaxp, tfact, complete, mat, out, device, days_per_chunk, 0, None, coarse, devices=devices, n_blocks=n_blocks,
                diag=diag)


def runmicro3Cpp(dfsel: Mapping, obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping,
                 soilc: Mapping, reqhgt: float, zref: float, lat: float, lon: float, Sminp: float,
                 Smaxp: float, tfact: float, complete: bool, mat: float, out: Sequence, *, device: int = 0,
                 days_per_chunk: int = 0, cells_per_block: int = 0, devices=None, n_blocks: int = 0, dtm: Mapping | None = None,
                 diag=None) -> dict:
    """Hourly, changing vegetation, data.frame climate: drop-in for the reference's runmicro3Cpp
    (src/microclimfCpp.cpp:2624-2924).  `dfsel` has columns lyr, st, ed (0-based step ranges of
    each vegetation layer, R/internal.R:1391-1399); vegp entries are [rows, cols, layers].  `devices` / `n_blocks`: as runmicro1Cpp;
    `diag`: as runmicro1Cpp."""
    return _run("mcf_runmicro3", False, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon,
                Sminp, Smaxp, tfact, complete, mat, out, device, days_per_chunk, cells_per_block, dfsel,
                devices=devices, n_blocks=n_blocks, dtm=dtm, diag=diag)


def runmicro4Cpp(dfsel: Mapping, obstime: Mapping, climdata: Mapping, pointm: Mapping, vegp: Mapping,
                 soilc: Mapping, reqhgt: float, zref: float, lats, lons, Sminp: float, Smaxp: float,
                 tfact: float, complete: bool, mat: float, out: Sequence, *, device: int = 0,
                 days_per_chunk: int = 0, cells_per_block: int = 0, devices=None, n_blocks: int = 0, dtm: Mapping | None = None,
                 diag=None) -> dict:
    """Hourly, changing vegetation, array climate: drop-in for the reference's runmicro4Cpp
    (src/microclimfCpp.cpp:2926-3226).  `devices` / `n_blocks`: as runmicro1Cpp; `diag`: as runmicro1Cpp."""
    return _run("mcf_runmicro4", True, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons,
                Sminp, Smaxp, tfact, complete, mat, out, device, days_per_chunk, cells_per_block, dfsel,
                devices=devices, n_blocks=n_blocks, dtm=dtm, diag=diag)


BIOCLIM_DFSEL = {"lyr": np.arange(1, 15), "st": np.arange(14) * 24, "ed": np.arange(14) * 24 + 23}   # cpp:3634-3646


def _bioclim_sel(b: Buffers, wetq, dryq, hotq, colq, air, out):
    """-> (mcf_bioclim_sel: the four quarters' step lists (held by `b`), `air`, the nineteen flags of `out`; `out` as a list)"""
    sel = _abi.BioclimSel()
    for name, q in (("wet", wetq), ("dry", dryq), ("hot", hotq), ("col", colq)):
        setattr(sel, name + "q", b.i32_plain(q))
        setattr(sel, "n" + name, np.size(q))
    sel.air = 1 if air else 0
    out = list(out)
    if len(out) != _abi.NBIO:
        raise ValueError("out must have 19 entries")
    for v in range(_abi.NBIO):
        sel.out[v] = 1 if out[v] else 0
    return sel, out


def _bioclim(fn_name, array_forcing, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp,
             Smaxp, tfact, mat, out, wetq, dryq, hotq, colq, air, device, layered=False, devices=None, n_blocks=0, coarse=None):
    lib = _abi.load()
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, True, mat,
                [1] * 10, array_forcing, device, dfsel=BIOCLIM_DFSEL if layered else None, coarse=coarse)
    sel, out = _bioclim_sel(m, wetq, dryq, hotq, colq, air, out)
    bo = _abi.BioclimOut()
    res = {}
    for v in range(_abi.NBIO):
        if out[v]:
            res[f"bio{v + 1}"], bo.bio[v] = m.out((m.rows, m.cols))
        else:
            bo.bio[v] = None
    mu = _abi.multi(devices, n_blocks)
    if mu:
        # one process, several devices (include/mcf.h mcf_runbioclim1_multi): row blocks dealt to the listed devices, same bits
        _abi.check(getattr(lib, fn_name + "_multi")(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(mu[0]), C.byref(bo)))
    else:
        _abi.check(getattr(lib, fn_name)(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(bo)))
    return res


def runbioclim1Cpp(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, mat, out,
                   wetq, dryq, hotq, colq, air, *, device: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """Drop-in for the reference's runbioclim1Cpp (src/microclimfCpp.cpp:3563-3588): the grid solver on
    the selected days followed by the 19 per-cell bioclim reductions, both on the device; only the
    requested [rows, cols] matrices are copied back.  `devices` / `n_blocks`: row blocks over several devices, same bits."""
    return _bioclim("mcf_runbioclim1", False, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon,
                    Sminp, Smaxp, tfact, mat, out, wetq, dryq, hotq, colq, air, device, devices=devices, n_blocks=n_blocks)


def runbioclim2Cpp(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons, Sminp, Smaxp, tfact, mat, out,
                   wetq, dryq, hotq, colq, air, *, device: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """Drop-in for the reference's runbioclim2Cpp (src/microclimfCpp.cpp:3590-3616), array climate."""
    return _bioclim("mcf_runbioclim2", True, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons,
                    Sminp, Smaxp, tfact, mat, out, wetq, dryq, hotq, colq, air, device, devices=devices, n_blocks=n_blocks)


def _coarse_spec(vegp, climdata, rowpos, colpos, altcorrect, dtmc, dtm, refuse_missing: bool = True):
    """marshal()'s `coarse` mapping: the raster's positions on the climate grid (default: the grid covers the raster's extent)
    and, with `altcorrect` 1 / 2 (`.runmodel2Cpp`'s), the coarse (dtmc) and fine (dtm) elevations.  `refuse_missing` False: absent
    elevations are left to marshal()"""
    R, Cc = np.shape(vegp["hgt"])[:2]
    cr, cc = np.shape(climdata["temp"])[:2]
    coarse = {"rowpos": coarse_positions(R, cr) if rowpos is None else rowpos,
              "colpos": coarse_positions(Cc, cc) if colpos is None else colpos}
    if altcorrect:
        if refuse_missing and (dtmc is None or dtm is None):
            raise ValueError("altcorrect needs dtmc (the climate cells' elevations) and dtm (the raster's)")
        coarse.update(altcorrect=int(altcorrect), dtmc=dtmc, dtm=dtm)
    return coarse


def runbioclim2Cpp_coarse(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons, Sminp, Smaxp, tfact, mat, out,
                          wetq, dryq, hotq, colq, air, *, rowpos=None, colpos=None, altcorrect: int = 0, dtmc=None, dtm=None,
                          device: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """`.runbioclim2`'s solver call with the resampling fused into the solver (array_forcing == 2): `climdata` and `pointm`
    as COARSE arrays [coarse_rows, coarse_cols, tsteps], as for runmicro2Cpp_coarse (`rowpos` / `colpos`, `altcorrect` with
    `dtmc` / `dtm`: see there).  Above ground the sink is streamed: the solver runs in day chunks and nothing of size
    cells x steps exists on the device (`bioclim_last_chunks`).  `devices` / `n_blocks`: row blocks, same bits."""
    coarse = _coarse_spec(vegp, climdata, rowpos, colpos, altcorrect, dtmc, dtm)
    return _bioclim("mcf_runbioclim2", True, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons,
                    Sminp, Smaxp, tfact, mat, out, wetq, dryq, hotq, colq, air, device, devices=devices, n_blocks=n_blocks,
                    coarse=coarse)


def runbioclim4Cpp_coarse(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons, Sminp, Smaxp, tfact, mat, out,
                          wetq, dryq, hotq, colq, air, *, rowpos=None, colpos=None, altcorrect: int = 0, dtmc=None, dtm=None,
                          device: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """runbioclim2Cpp_coarse with the fourteen one-day vegetation layers of runbioclim4Cpp (`.runbioclim4`)."""
    coarse = _coarse_spec(vegp, climdata, rowpos, colpos, altcorrect, dtmc, dtm)
    return _bioclim("mcf_runbioclim4", True, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons,
                    Sminp, Smaxp, tfact, mat, out, wetq, dryq, hotq, colq, air, device, True, devices=devices, n_blocks=n_blocks,
                    coarse=coarse)


def runbioclim_depths(obstime, climdata, pointm, vegp, soilc, depths, zref, lat, lon, Sminp, Smaxp, tfact, mat, out,
                      wetq, dryq, hotq, colq, air=True, *, layered: bool = False, array_forcing: bool = False, coarse: Mapping | None = None,
                      device: int = 0, chunk_days: int = 0, cells_per_block: int = 0) -> dict:
    """Soil bioclim variables at several depths from one streamed below-ground solve (include/mcf.h mcf_runbioclim_depths):
    runbioclim1Cpp's argument list with `depths` (each < 0, any order, at most _abi.MAX_DEPTHS) in place of reqhgt.  `air`
    must be true (Tz).  `layered`: vegetation arrays [rows, cols, >= 14] under runbioclim3Cpp's fixed fourteen one-day layers.
    `coarse` as for runmicro_depths: `climdata` / `pointm` are coarse arrays and `lat` / `lon` the per-cell lats / lons
    (`array_forcing` without `coarse`, fine arrays, is refused by the library: runbioclim2Cpp serves it).
    `chunk_days`: days per solver chunk (0: sized from free device memory).  The quarter lists must be ascending.
    -> {"depths": depths, "bio1" .. "bio11": [ndepths, rows, cols], "bio12" .. "bio19": [rows, cols]} for the selected
    variables; slab d of a matrix has the bits of runbioclim1Cpp(reqhgt = depths[d])."""
    lib = _abi.load()
    d, _ = _depth_list(depths, None, 0)
    reqhgt = float(d[0]) if d.size and d[0] < 0 else -1.0          # (the library judges the list)
    m = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, True, mat,
                [1] * 10, bool(array_forcing) or coarse is not None, device, 0, cells_per_block, BIOCLIM_DFSEL if layered else None, coarse)
    sel, out = _bioclim_sel(m, wetq, dryq, hotq, colq, air, out)
    nd = min(d.size, _abi.MAX_DEPTHS)
    bo = _abi.BioclimDepthsOut()
    res = {"depths": d.copy()}
    for v in range(_abi.NBIO):
        if not out[v]:
            continue
        if v < 11:
            # (slab i is one Fortran-ordered [rows, cols] matrix)
            a = np.empty((nd, m.cols, m.rows), dtype=np.float64).transpose(0, 2, 1)
            for i in range(nd):
                bo.temp[i][v] = m.ptr(a[i])
        else:
            a, bo.moist[v - 11] = m.out((m.rows, m.cols))
        res[f"bio{v + 1}"] = a
    _abi.check(lib.mcf_runbioclim_depths(C.byref(m.inputs), C.byref(m.options), C.byref(sel), m.ptr(d), int(d.size), int(chunk_days),
                                         C.byref(bo)))
    return res


def bioclim_last_chunks() -> int:
    """Solver chunk launches of this thread's last runbioclim*Cpp call (include/mcf.h mcf_bioclim_last_chunks): > 0 — the
    streamed sink ran; 0 — the whole-series one.  The matrices do not tell."""
    return int(_abi.load().mcf_bioclim_last_chunks())


class Plan:
    """HBM-resident solver plan (include/mcf.h plan API): inputs uploaded once,
    day chunks solved into a device output ring."""

    def __init__(self, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp,
                 tfact, complete, mat, out, *, array_forcing=False, ring_days=1, ring_slots=1,
                 device=0, cells_per_block=0, dfsel=None, coarse=None, stream_below=False, dtm=None):
        """dtm: {z, res[, halo_north, halo_south, row0, rows_total, agg]} — entries of `soilc` among slope, aspect, hor, svfa, wsa,
        twi that are missing are derived from it on the device (include/mcf.h mcf_plan_create_dtm).
        stream_below: reqhgt < 0 through day chunks (include/mcf.h mcf_plan_create_streamed) — below_prepare() first, then
        run_days in day order from day 0, each chunk's final Tz in its slot; for reqhgt >= 0 the same plan as without it."""
        self._lib = _abi.load()
        self._m: Marshalled = marshal(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon,
                                      Sminp, Smaxp, tfact, complete, mat, out, array_forcing or coarse is not None, device,
                                      0, cells_per_block, dfsel, coarse,
                                      soilc_optional=DTM_DERIVED if dtm is not None else ())
        self._p = C.c_void_p()
        if dtm is not None:
            if stream_below:
                raise ValueError("streamed below-ground plans have no dtm form")
            sp = dtm_spec(dtm, self._m.rows, self._m.cols)
            _abi.check(self._lib.mcf_plan_create_dtm(C.byref(self._m.inputs), C.byref(self._m.options), C.byref(sp), int(ring_days),
                                                     int(ring_slots), C.byref(self._p)))
        else:
            create = self._lib.mcf_plan_create_streamed if stream_below else self._lib.mcf_plan_create
            _abi.check(create(C.byref(self._m.inputs), C.byref(self._m.options), int(ring_days), int(ring_slots), C.byref(self._p)))
        self.stream_below = bool(stream_below)
        self.rows, self.cols, self.tsteps = self._m.rows, self._m.cols, self._m.tsteps
        self.ndays = self.tsteps // 24
        self.array_forcing = bool(array_forcing) or coarse is not None

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self._lib.mcf_plan_destroy(self._p)
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

    @property
    def valid_cells(self) -> int:
        return int(self._lib.mcf_plan_valid_cells(self._p))

    @property
    def device_bytes(self) -> int:
        return int(self._lib.mcf_plan_bytes(self._p))

    def twi_partial(self):
        s, n = C.c_double(), C.c_int64()
        _abi.check(self._lib.mcf_plan_twi_partial(self._p, C.byref(s), C.byref(n)))
        return s.value, n.value

    def set_twi_mean(self, mean: float):
        _abi.check(self._lib.mcf_plan_set_twi_mean(self._p, float(mean)))

    def upload_forcing_days(self, day0: int, ndays: int, slot: int = 0):
        _abi.check(self._lib.mcf_plan_upload_forcing_days(self._p, C.byref(self._m.inputs), day0, ndays, slot))

    def run_days(self, day0: int, ndays: int, slot: int = 0):
        _abi.check(self._lib.mcf_plan_run_days(self._p, day0, ndays, slot))

    def run_days_at(self, day0: int, ndays: int, slot: int, slot_day0: int):
        """run_days with the days written at day `slot_day0` of the slot (include/mcf.h mcf_plan_run_days_at)."""
        _abi.check(self._lib.mcf_plan_run_days_at(self._p, day0, ndays, slot, slot_day0))

    def run_days_masked(self, day0: int, ndays: int, slot: int, slot_day0: int, skip_tile):
        """run_days_at leaving out the tiles with skip_tile[t] != 0 (include/mcf.h mcf_plan_run_days_masked)."""
        sk = np.ascontiguousarray(skip_tile, dtype=np.uint8)
        _abi.check(self._lib.mcf_plan_run_days_masked(self._p, day0, ndays, slot, slot_day0, Buffers().ptr(sk), int(sk.size)))

    def run_days_cells(self, day0: int, ndays: int, slot: int, slot_day0: int, need_cell_dev: int) -> int:
        """run_days_at for the cells marked in `need_cell_dev` — the ADDRESS of one byte per cell in this device's memory, e.g.
        SnowPlan.free_cells' or a torch uint8 tensor's data_ptr() — gathered into tiles of their own; every other cell's values
        in the slot stay (include/mcf.h mcf_plan_run_days_cells).  -> number of marked cells"""
        n = C.c_int64(0)
        _abi.check(self._lib.mcf_plan_run_days_cells(self._p, day0, ndays, slot, slot_day0, C.c_void_p(int(need_cell_dev)),
                                                     int(self.rows * self.cols), C.byref(n)))
        return int(n.value)

    @property
    def n_tiles(self) -> int:
        lay = self.ring_layout()
        return (lay["cells"] + lay["cells_per_tile"] - 1) // lay["cells_per_tile"]

    def set_mxtc(self, mxtc: float):
        """Replace the series' maximum air temperature (the snow branch solves a subset of the days)."""
        _abi.check(self._lib.mcf_plan_set_mxtc(self._p, float(mxtc)))

    def set_mxtc_days(self, dayflag):
        """array forcing: the per-cell temperature cap over the days with dayflag != 0 (include/mcf.h mcf_plan_set_mxtc_days); a
        coarse plan folds its resident series, a fine one streams its temperature array again"""
        flags = np.ascontiguousarray(dayflag, dtype=np.int32)
        _abi.check(self._lib.mcf_plan_set_mxtc_days(self._p, C.byref(self._m.inputs), Buffers().ptr(flags), int(flags.size)))

    def set_day_layers(self, layer_of_day=None):
        """layered vegetation: the day -> layer map (include/mcf.h mcf_plan_set_day_layers); None: the plan's own table again"""
        if layer_of_day is None:
            _abi.check(self._lib.mcf_plan_set_day_layers(self._p, None, self.ndays))
            return
        lod = np.ascontiguousarray(layer_of_day, dtype=np.int32)
        _abi.check(self._lib.mcf_plan_set_day_layers(self._p, Buffers().ptr(lod), int(lod.size)))

    def fetch_mxtc(self) -> np.ndarray:
        """array forcing: the per-cell maximum air temperature the plan holds now, [rows, cols]"""
        a, ptr = Buffers().out((self.rows, self.cols))
        _abi.check(self._lib.mcf_plan_fetch_mxtc(self._p, ptr))
        return a

    def set_height(self, h: float, pai_a=None):
        """Re-target the plan to height `h` > 0 above ground (include/mcf.h mcf_plan_set_height): leafden and paia of every layer
        are derived on the device from the resident hgt and pai, everything else stays; the next run has the bits of a plan
        created at `h` with those planes.  `pai_a`: the plant area above `h`, [rows, cols(, layers)], instead of the derived one."""
        L = max(int(self._m.inputs.veg_layers), 1)
        a = None
        if pai_a is not None:
            a = np.asfortranarray(np.asarray(pai_a, dtype=np.float64))
            if a.ndim == 3 and a.shape[2] > L:
                a = a[:, :, :L]
            if a.size != self.rows * self.cols * L:
                raise ValueError(f"pai_a: expected {self.rows} x {self.cols} x {L} values, got shape {a.shape}")
        _abi.check(self._lib.mcf_plan_set_height(self._p, float(h), Buffers().ptr(a)))

    def fetch_foliage(self):
        """(paia, leafden) as the plan holds them now, [rows, cols] or [rows, cols, layers]"""
        L = int(self._m.inputs.veg_layers)
        shape = (self.rows, self.cols) if L < 1 else (self.rows, self.cols, L)
        (pa, pap), (ld, ldp) = Buffers().out(shape), Buffers().out(shape)
        _abi.check(self._lib.mcf_plan_fetch_foliage(self._p, pap, ldp))
        return pa, ld

    def belowground(self):
        _abi.check(self._lib.mcf_plan_belowground(self._p))

    def below_prepare(self):
        """Streamed below-ground plan: the per-cell state of the whole series (damping-depth pre-pass, or with complete = 1 the
        solver's first sweep).  Array forcing streams the forcing through slot 0: upload the chunks' forcing again afterwards."""
        _abi.check(self._lib.mcf_plan_below_prepare(self._p, C.byref(self._m.inputs)))

    def below_set_days(self, days):
        """Streamed below-ground plan, before below_prepare(): the series Tbelowgroundv sees is the listed whole days (strictly
        ascending) joined end to end (include/mcf.h mcf_plan_below_set_days).  run_days(day0, ndays, slot) then runs the
        subset's days inside that calendar range, each at its own place day - day0 of the slot."""
        b = Buffers()
        _abi.check(self._lib.mcf_plan_below_set_days(self._p, b.i32_plain(days), int(np.size(days))))

    def below_set_depths(self, depths, tbp=None):
        """Streamed below-ground plan with Tz, before below_prepare(): Tbelowgroundv at each of `depths` (< 0, any order, at most
        _abi.MAX_DEPTHS) from the one solve (include/mcf.h mcf_plan_below_set_depths).  `tbp`: [ndepths, tsteps], the point
        model's soil temperature per depth — needed with complete = False.  fetch() and the sinks see depths[0]."""
        d, t = _depth_list(depths, tbp, self.tsteps)
        _abi.check(self._lib.mcf_plan_below_set_depths(self._p, Buffers().ptr(d), int(d.size), Buffers().ptr(t)))
        self.depths = d.copy()

    def fetch_depth(self, slot: int, depth: int, step0: int, nsteps: int) -> np.ndarray:
        """fetch() of Tz at depth index `depth` of the list (a plan without a list: 0)"""
        a, ptr = Buffers().out((self.rows, self.cols, nsteps))
        _abi.check(self._lib.mcf_plan_fetch_depth(self._p, slot, int(depth), step0, nsteps, ptr))
        return a

    def summary_enable_below(self, periods, vars=("Tz",), stats=("mean", "min", "max"), thresholds=None, *, nperiods=None):
        """summary_enable() for a streamed below-ground plan, after below_set_depths() if there is a list (include/mcf.h
        mcf_plan_summary_enable_below): `vars` among Tz and soilm, Tz kept per depth.  summary_accumulate / summary_days /
        summary_reset work as above ground; fetch_summary_depth reads the planes."""
        sp, vi, si, _pod = summary_spec(periods, vars, stats, thresholds)
        if nperiods is not None:
            sp.nperiods = int(nperiods)
        if _pod.size != self.ndays:
            raise ValueError(f"periods: one entry per day of the plan ({self.ndays}), got {_pod.size}")
        _abi.check(self._lib.mcf_plan_summary_enable_below(self._p, C.byref(sp)))
        self._summary_nperiods = int(sp.nperiods)
        return [_abi.OUT_NAMES[v] for v in vi], [_abi.STAT_NAMES[s] for s in si]

    def fetch_summary_depth(self, depth: int, var, stat) -> np.ndarray:
        """fetch_summary() of Tz at depth index `depth`; soilm has depth 0 alone"""
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        s = _abi.STAT_NAMES.index(stat) if isinstance(stat, str) else int(stat)
        a, ptr = Buffers().out((self.rows, self.cols, getattr(self, "_summary_nperiods", 1)))
        _abi.check(self._lib.mcf_plan_summary_fetch_depth(self._p, int(depth), v, s, ptr))
        return a

    def sync(self):
        _abi.check(self._lib.mcf_plan_sync(self._p))

    def diag_enable(self, names="all"):
        """Before the first run: the staged model's diagnostics (names of include/mcf.h mcf_diag, or "all") go to a second
        device ring beside the outputs, filled by run_days / run_days_at; the ten outputs keep their bits.  Vector forcing and
        reqhgt >= 0 (include/mcf.h mcf_plan_diag_enable).  -> the selected names"""
        sel, picked = diag_selection(names)
        _abi.check(self._lib.mcf_plan_diag_enable(self._p, C.byref(sel)))
        return picked

    def diag_enable_array(self, names="all"):
        """diag_enable() for an array-weather plan, fine or coarse (include/mcf.h mcf_plan_diag_enable_array): the same ring,
        fetch_diag / diag_slot_ptr / diag_ring_layout read it.  -> the selected names"""
        sel, picked = diag_selection(names)
        _abi.check(self._lib.mcf_plan_diag_enable_array(self._p, C.byref(sel)))
        return picked

    def fetch_diag(self, slot: int, dvar, step0: int, nsteps: int) -> np.ndarray:
        """fetch() for a selected diagnostic (a name or an index of include/mcf.h mcf_diag)"""
        v = _abi.DIAG_NAMES.index(dvar) if isinstance(dvar, str) else int(dvar)
        a, ptr = Buffers().out((self.rows, self.cols, nsteps))
        _abi.check(self._lib.mcf_plan_diag_fetch(self._p, slot, v, step0, nsteps, ptr))
        return a

    def diag_ring_layout(self) -> dict:
        """How a selected diagnostic of a ring slot is addressed on the device (include/mcf.h mcf_plan_diag_ring_layout)."""
        lay = _abi.RingLayout()
        _abi.check(self._lib.mcf_plan_diag_ring_layout(self._p, C.byref(lay)))
        return {n: int(getattr(lay, n)) for n, _ in lay._fields_}

    def diag_slot_ptr(self, slot: int, dvar) -> int:
        v = _abi.DIAG_NAMES.index(dvar) if isinstance(dvar, str) else int(dvar)
        q = C.c_void_p()
        _abi.check(self._lib.mcf_plan_diag_slot_ptr(self._p, slot, v, C.byref(q)))
        return int(q.value or 0)

    def summary_enable(self, periods, vars=("Tz",), stats=("mean", "min", "max"), thresholds=None, *, nperiods=None):
        """Period summaries of the plan's outputs, accumulated on the device (include/mcf.h mcf_plan_summary_enable):
        `periods` one integer per day of the plan (-1: not counted), `vars` among the plan's outputs, `stats` of
        _abi.STAT_NAMES, `thresholds` for hours_above (a number or {variable: number}).  -> (variables, statistics) selected"""
        sp, vi, si, _pod = summary_spec(periods, vars, stats, thresholds)
        if nperiods is not None:
            sp.nperiods = int(nperiods)
        if _pod.size != self.ndays:
            raise ValueError(f"periods: one entry per day of the plan ({self.ndays}), got {_pod.size}")
        _abi.check(self._lib.mcf_plan_summary_enable(self._p, C.byref(sp)))
        self._summary_nperiods = int(sp.nperiods)
        return [_abi.OUT_NAMES[v] for v in vi], [_abi.STAT_NAMES[s] for s in si]

    def summary_accumulate(self, slot: int, slot_day0: int, day0: int, ndays: int):
        """Fold days [slot_day0, slot_day0 + ndays) of the slot as calendar days [day0, day0 + ndays), behind the run that
        filled them; days in ascending order, each at most once (include/mcf.h mcf_plan_summary_accumulate)."""
        _abi.check(self._lib.mcf_plan_summary_accumulate(self._p, slot, slot_day0, day0, ndays))

    def summarise_days(self, ring: int):
        """The whole series through ring slot 0 in chunks of `ring` days, each run and then folded (array forcing: its forcing
        uploaded first)."""
        for d0 in range(0, self.ndays, ring):
            n = min(ring, self.ndays - d0)
            if self.array_forcing:
                self.upload_forcing_days(d0, n, 0)
            self.run_days(d0, n, 0)
            self.summary_accumulate(0, 0, d0, n)

    def fetch_summary(self, var, stat) -> np.ndarray:
        """[rows, cols, nperiods] of one selected statistic of one selected variable (names or indices)"""
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        s = _abi.STAT_NAMES.index(stat) if isinstance(stat, str) else int(stat)
        a, ptr = Buffers().out((self.rows, self.cols, getattr(self, "_summary_nperiods", 1)))
        _abi.check(self._lib.mcf_plan_summary_fetch(self._p, v, s, ptr))
        return a

    def summary_days(self) -> np.ndarray:
        """counted days folded so far into each period"""
        d, ptr = Buffers().out(getattr(self, "_summary_nperiods", 1), np.int32, zero=True)
        _abi.check(self._lib.mcf_plan_summary_days(self._p, ptr))
        return d

    def summary_reset(self):
        """Back to the state of summary_enable: nothing folded."""
        _abi.check(self._lib.mcf_plan_summary_reset(self._p))

    def series_enable(self, points=None, zones=None, vars=("Tz",), stats=("mean", "min", "max"), *, nzones=None):
        """The series sink (include/mcf.h mcf_plan_series_enable): the hourly series of `vars` at `points` (cell indices
        row + rows * col) and their per-step statistics `stats` (names of _abi.ZSTAT_NAMES) over `zones` ([rows, cols] labels,
        negative or masked: in no zone), kept on the device.  -> (variables, statistics) selected"""
        sp, vi, si = series_spec(self.rows, self.cols, points, zones, vars, stats, nzones)
        _abi.check(self._lib.mcf_plan_series_enable(self._p, C.byref(sp)))
        self._series_shape = (int(sp.npoints), int(sp.nzones))
        return [_abi.OUT_NAMES[v] for v in vi], [_abi.ZSTAT_NAMES[k] for k in si]

    def series_accumulate(self, slot: int, slot_day0: int, day0: int, ndays: int):
        """Fold days [slot_day0, slot_day0 + ndays) of the slot as calendar days [day0, day0 + ndays), behind the run that
        filled them; days in any order, each at most once (include/mcf.h mcf_plan_series_accumulate)."""
        _abi.check(self._lib.mcf_plan_series_accumulate(self._p, slot, slot_day0, day0, ndays))

    def fetch_point_series(self, var) -> np.ndarray:
        """[tsteps, npoints] of one selected variable (name or index)"""
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        a, ptr = Buffers().out((self.tsteps, getattr(self, "_series_shape", (1, 1))[0]))
        _abi.check(self._lib.mcf_plan_series_fetch_points(self._p, v, ptr))
        return a

    def fetch_zone_series(self, var, stat) -> np.ndarray:
        """[tsteps, nzones] of one selected statistic of one selected variable (names or indices)"""
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        k = _abi.ZSTAT_NAMES.index(stat) if isinstance(stat, str) else int(stat)
        a, ptr = Buffers().out((self.tsteps, getattr(self, "_series_shape", (1, 1))[1]))
        _abi.check(self._lib.mcf_plan_series_fetch_zones(self._p, v, k, ptr))
        return a

    def series_reset(self):
        """Back to the state of series_enable: nothing folded."""
        _abi.check(self._lib.mcf_plan_series_reset(self._p))

    def series_enable_below(self, points=None, zones=None, vars=("Tz",), stats=("mean", "min", "max"), *, nzones=None):
        """series_enable() for a streamed below-ground plan, after below_set_depths() if there is a list (include/mcf.h
        mcf_plan_series_enable_below): `vars` among Tz and soilm, Tz kept per depth.  series_accumulate / series_reset work as
        above ground; fetch_point_series_depth / fetch_zone_series_depth read the series."""
        sp, vi, si = series_spec(self.rows, self.cols, points, zones, vars, stats, nzones)
        _abi.check(self._lib.mcf_plan_series_enable_below(self._p, C.byref(sp)))
        self._series_shape = (int(sp.npoints), int(sp.nzones))
        return [_abi.OUT_NAMES[v] for v in vi], [_abi.ZSTAT_NAMES[k] for k in si]

    def fetch_point_series_depth(self, depth: int, var) -> np.ndarray:
        """fetch_point_series() of Tz at depth index `depth`; soilm has depth 0 alone"""
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        a, ptr = Buffers().out((self.tsteps, getattr(self, "_series_shape", (1, 1))[0]))
        _abi.check(self._lib.mcf_plan_series_fetch_points_depth(self._p, int(depth), v, ptr))
        return a

    def fetch_zone_series_depth(self, depth: int, var, stat) -> np.ndarray:
        """fetch_zone_series() of Tz at depth index `depth`; soilm has depth 0 alone"""
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        k = _abi.ZSTAT_NAMES.index(stat) if isinstance(stat, str) else int(stat)
        a, ptr = Buffers().out((self.tsteps, getattr(self, "_series_shape", (1, 1))[1]))
        _abi.check(self._lib.mcf_plan_series_fetch_zones_depth(self._p, int(depth), v, k, ptr))
        return a

    def fetch(self, slot: int, var, step0: int, nsteps: int) -> np.ndarray:
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        a, ptr = Buffers().out((self.rows, self.cols, nsteps))
        _abi.check(self._lib.mcf_plan_fetch(self._p, slot, v, step0, nsteps, ptr))
        return a

    def fetch_cells(self, slot: int, var, step0: int, nsteps: int, cells) -> np.ndarray:
        """[len(cells), nsteps] values of `var` for the listed cells (0-based column-major indices i + rows*j)."""
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        cells = np.ascontiguousarray(np.asarray(cells, dtype=np.int64))
        a, ptr = Buffers().out((cells.size, nsteps))
        _abi.check(self._lib.mcf_plan_fetch_cells(self._p, slot, v, step0, nsteps, Buffers().ptr(cells), cells.size, ptr))
        return a

    # writetonc's scale per variable (R/dataprep.R:1158-1167): x100 for temperatures, soil moisture, wind
    NC_SCALE = {"Tz": 100.0, "tleaf": 100.0, "relhum": 1.0, "soilm": 100.0, "windspeed": 100.0, "Rdirdown": 1.0,
                "Rdifdown": 1.0, "Rlwdown": 1.0, "Rswup": 1.0, "Rlwup": 1.0}

    def fetch_packed(self, slot: int, var, step0: int, nsteps: int, scale: float | None = None,
                     timing: bool = False):
        """`writetonc`-packed fetch: int32 [cols, rows, nsteps] (east fastest) = round(value * scale),
        NA -> INT32_MIN (R's NA_integer_).  Returns the array (and the pack kernel's ms with timing)."""
        v = _abi.OUT_NAMES.index(var) if isinstance(var, str) else int(var)
        if scale is None:
            scale = self.NC_SCALE[_abi.OUT_NAMES[v]]
        a, ptr = Buffers().out((self.cols, self.rows, nsteps), np.int32)
        ms = C.c_float()
        _abi.check(self._lib.mcf_plan_fetch_packed(self._p, slot, v, step0, nsteps, float(scale), ptr, C.byref(ms) if timing else None))
        return (a, ms.value) if timing else a

    def ring_layout(self) -> dict:
        """How a ring slot variable is addressed on the device (include/mcf.h mcf_ring_layout)."""
        lay = _abi.RingLayout()
        _abi.check(self._lib.mcf_plan_ring_layout(self._p, C.byref(lay)))
        return {n: int(getattr(lay, n)) for n, _ in lay._fields_}

    def timer_start(self):
        _abi.check(self._lib.mcf_plan_timer_start(self._p))

    def timer_stop(self) -> float:
        ms = C.c_float()
        _abi.check(self._lib.mcf_plan_timer_stop(self._p, C.byref(ms)))
        return ms.value

    def kernel_timing(self, enable: bool = True):
        _abi.check(self._lib.mcf_plan_kernel_timing(self._p, 1 if enable else 0))

    def dispatch_stats(self) -> dict:
        """Which clamp variant the launches ran (include/mcf.h mcf_dispatch_stats): diagnostics, results are identical."""
        st = _abi.DispatchStats()
        _abi.check(self._lib.mcf_plan_dispatch_stats(self._p, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def kernel_stats(self):
        ms, n = C.c_double(), C.c_int64()
        _abi.check(self._lib.mcf_plan_kernel_stats(self._p, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def below_days_range(days, total_days: int, day0: int, ndays: int):
    """(pos0, npos): the positions of the day subset `days` that lie in the calendar range [day0, day0 + ndays) of a series of
    `total_days` whole days (include/mcf.h mcf_below_days_range; the list is checked as Plan.below_set_days checks it)."""
    b, pos0, npos = Buffers(), C.c_int32(), C.c_int32()
    _abi.check(_abi.load().mcf_below_days_range(b.i32_plain(days), int(np.size(days)), int(total_days), int(day0), int(ndays),
                                                C.byref(pos0), C.byref(npos)))
    return pos0.value, npos.value


def runbioclim3Cpp(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon, Sminp, Smaxp, tfact, mat, out,
                   wetq, dryq, hotq, colq, air, *, device: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """Drop-in for runbioclim3Cpp (src/microclimfCpp.cpp:3620-3658): vegetation arrays [rows, cols, 14], one layer per
    selected day (twelve monthly days, the hottest, the coldest); steps past the 336th stay NA as in the reference."""
    return _bioclim("mcf_runbioclim3", False, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lat, lon,
                    Sminp, Smaxp, tfact, mat, out, wetq, dryq, hotq, colq, air, device, True, devices=devices, n_blocks=n_blocks)


def runbioclim4Cpp(obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons, Sminp, Smaxp, tfact, mat, out,
                   wetq, dryq, hotq, colq, air, *, device: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """Drop-in for runbioclim4Cpp (src/microclimfCpp.cpp:3660-3700), array climate."""
    return _bioclim("mcf_runbioclim4", True, obstime, climdata, pointm, vegp, soilc, reqhgt, zref, lats, lons,
                    Sminp, Smaxp, tfact, mat, out, wetq, dryq, hotq, colq, air, device, True, devices=devices, n_blocks=n_blocks)
