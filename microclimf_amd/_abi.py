"""ctypes mirror of include/mcf.h and the loader for libmcfhip.so.

The structs here are a field-for-field transcription of the C header; the
shared library is the product (hand-written HIP for gfx950).  There is no CPU
fallback: `load()` raises if the library is not built, and every solve raises
if no HIP device is usable.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

NOUT = 10
NDIAG = 13
# include/mcf.h mcf_diag: the staged model's diagnostics, in the enum's order
DIAG_NAMES = ("si", "radGsw", "radGlw", "radCsw", "radClw", "radLsw", "radLpar", "lwout", "uf", "gHa", "T0", "G", "kDDg")
OUT_NAMES = ("Tz", "tleaf", "relhum", "soilm", "windspeed", "Rdirdown",
             "Rdifdown", "Rlwdown", "Rswup", "Rlwup")

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)


class Obstime(C.Structure):
    _fields_ = [("year", c_int32_p), ("month", c_int32_p), ("day", c_int32_p),
                ("hour", c_double_p)]


CLIM_FIELDS = ("tc", "es", "ea", "tdew", "pk", "swdown", "difrad", "lwdown",
               "windspeed", "winddir")
POINTM_FIELDS = ("soilm", "Tg", "Tbp", "G", "umu", "kp", "muGp", "dtrp")
VEGP_FIELDS = ("hgt", "pai", "x", "gsmax", "leafr", "leaft", "clump", "leafd",
               "paia", "leafden")
SOILC_FIELDS = ("Smin", "Smax", "gref", "soilb", "Psie", "Vq", "Vm", "Mc", "rho",
                "slope", "aspect", "twi", "svfa", "wsa", "hor")


def _ptr_struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": [(f, c_double_p) for f in fields]})


Climate = _ptr_struct("Climate", CLIM_FIELDS)
Pointm = _ptr_struct("Pointm", POINTM_FIELDS)
Vegp = _ptr_struct("Vegp", VEGP_FIELDS)
Soilc = _ptr_struct("Soilc", SOILC_FIELDS)


class GridInputs(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int64), ("tsteps", C.c_int64),
                ("array_forcing", C.c_int32), ("veg_layers", C.c_int32),
                ("obstime", Obstime), ("clim", Climate), ("pointm", Pointm),
                ("vegp", Vegp), ("soilc", Soilc),
                ("lat", C.c_double), ("lon", C.c_double),
                ("lats", c_double_p), ("lons", c_double_p),
                ("lyr_st", c_int32_p), ("lyr_ed", c_int32_p),
                ("coarse_rows", C.c_int32), ("coarse_cols", C.c_int32),
                ("coarse_rowpos", c_double_p), ("coarse_colpos", c_double_p),
                ("coarse_relhum", c_double_p), ("coarse_winddir", c_double_p),
                ("coarse_altcorrect", C.c_int32), ("coarse_dtm", c_double_p), ("fine_dtm", c_double_p),
                ("row_pitch", C.c_int64)]


class Multi(C.Structure):
    """include/mcf.h mcf_multi: devices and row blocks of the one-process multi-device entry points."""
    _fields_ = [("n_devices", C.c_int32), ("devices", c_int32_p), ("n_blocks", C.c_int32)]


def multi(devices, n_blocks):
    """-> mcf_multi[1] (pass `C.byref(mu[0])`) for `devices` (a list of HIP ordinals, [] = all visible) / `n_blocks` row blocks,
    or None when neither is given: the single-device entry.  The returned object holds the int32 list its `devices` points into
    (ctypes keeps what a cast pointer was made from with the struct it is stored in)."""
    if devices is None and not n_blocks:
        return None
    devs = (C.c_int32 * (0 if devices is None else len(devices)))(*(() if devices is None else devices))
    return (Multi * 1)(Multi(len(devs), C.cast(devs, c_int32_p), int(n_blocks)))


class Options(C.Structure):
    _fields_ = [("reqhgt", C.c_double), ("zref", C.c_double),
                ("Sminp", C.c_double), ("Smaxp", C.c_double),
                ("tfact", C.c_double), ("mat", C.c_double),
                ("complete", C.c_int32), ("out", C.c_int32 * NOUT),
                ("device", C.c_int32), ("days_per_chunk", C.c_int32),
                ("cells_per_block", C.c_int32)]


class TerrainIn(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int64), ("halo_north", C.c_int32),
                ("halo_south", C.c_int32), ("dtm", c_double_p), ("res", C.c_double),
                ("zref", C.c_double), ("agg", C.c_int32), ("reserved0", C.c_int32),
                ("row0", C.c_int64), ("rows_total", C.c_int64)]


class TerrainOut(C.Structure):
    _fields_ = [("slope", c_double_p), ("aspect", c_double_p), ("hor", c_double_p),
                ("svfa", c_double_p), ("wsa", c_double_p)]


class DtmSpec(C.Structure):
    """include/mcf.h mcf_dtm_spec: the elevation block a plan derives its missing terrain planes / wetness index from."""
    _fields_ = [("dtm", c_double_p), ("halo_north", C.c_int32), ("halo_south", C.c_int32),
                ("row0", C.c_int64), ("rows_total", C.c_int64), ("xres", C.c_double), ("yres", C.c_double),
                ("agg", C.c_int32), ("reserved0", C.c_int32)]


NBIO = 19


class BioclimSel(C.Structure):
    _fields_ = [("wetq", c_int32_p), ("dryq", c_int32_p), ("hotq", c_int32_p), ("colq", c_int32_p),
                ("nwet", C.c_int32), ("ndry", C.c_int32), ("nhot", C.c_int32), ("ncol", C.c_int32),
                ("air", C.c_int32), ("out", C.c_int32 * NBIO)]


class BioclimOut(C.Structure):
    _fields_ = [("bio", c_double_p * NBIO)]


class Outputs(C.Structure):
    _fields_ = [("var", c_double_p * NOUT)]


NSTAT = 6
# include/mcf.h mcf_stat: the statistics of a period summary, in the enum's order
STAT_NAMES = ("mean", "min", "max", "mean_daily_max", "mean_daily_min", "hours_above")


class SummarySpec(C.Structure):
    """include/mcf.h mcf_summary_spec"""
    _fields_ = [("nperiods", C.c_int32), ("period_of_day", c_int32_p), ("var", C.c_int32 * NOUT), ("stat", C.c_int32 * NSTAT),
                ("threshold", C.c_double * NOUT)]


class SummaryOut(C.Structure):
    """include/mcf.h mcf_summary_out"""
    _fields_ = [("val", (c_double_p * NSTAT) * NOUT), ("days", c_int32_p)]


NZSTAT = 4
MAX_ZONES = 64      # include/mcf.h MCF_MAX_ZONES
# include/mcf.h mcf_zstat: the statistics of a zone series, in the enum's order
ZSTAT_NAMES = ("mean", "min", "max", "count")


class SeriesSpec(C.Structure):
    """include/mcf.h mcf_series_spec"""
    _fields_ = [("npoints", C.c_int64), ("cells", C.POINTER(C.c_int64)), ("nzones", C.c_int32), ("zone", c_int32_p),
                ("var", C.c_int32 * NOUT), ("zstat", C.c_int32 * NZSTAT)]


class SeriesOut(C.Structure):
    """include/mcf.h mcf_series_out"""
    _fields_ = [("points", c_double_p * NOUT), ("zones", (c_double_p * NZSTAT) * NOUT)]


MAX_DEPTHS = 8      # include/mcf.h MCF_MAX_DEPTHS


class DepthOutputs(C.Structure):
    """include/mcf.h mcf_depth_outputs"""
    _fields_ = [("tz", c_double_p * MAX_DEPTHS), ("soilm", c_double_p)]


class BioclimDepthsOut(C.Structure):
    """include/mcf.h mcf_bioclim_depths_out"""
    _fields_ = [("temp", (c_double_p * 11) * MAX_DEPTHS), ("moist", c_double_p * 8)]


class DepthSummaryOut(C.Structure):
    """include/mcf.h mcf_depth_summary_out"""
    _fields_ = [("tz", (c_double_p * NSTAT) * MAX_DEPTHS), ("soilm", c_double_p * NSTAT), ("days", c_int32_p)]


class SnowpackSummarySpec(C.Structure):
    """include/mcf.h mcf_snowpack_summary_spec (series in SNOWDRIVER_OUT's order)"""
    _fields_ = [("nperiods", C.c_int32), ("period_of_day", c_int32_p), ("series", C.c_int32 * 5), ("stat", C.c_int32 * NSTAT),
                ("threshold", C.c_double * 5)]


class SnowpackSummaryOut(C.Structure):
    """include/mcf.h mcf_snowpack_summary_out"""
    _fields_ = [("val", (c_double_p * NSTAT) * 5), ("days", c_int32_p)]


class DiagOutputs(C.Structure):
    """include/mcf.h mcf_diag_outputs"""
    _fields_ = [("var", c_double_p * NDIAG)]


# ---- snow branch (include/mcf.h "snow branch") ----
SNOWENV = {"Alpine": 0, "Maritime": 1, "Prairie": 2, "Tundra": 3, "Taiga": 4}
SNOW_CLIM_FIELDS = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "winddir", "precip", "umu")
SNOW_POINTM_FIELDS = ("Gp", "Tc", "RswabsG", "RlwabsG", "umu")
SNOW_VEGP_FIELDS = ("pai", "hgt", "leaft", "clump", "paia", "leafd", "leafden")
SNOWM_FIELDS = ("Tc", "Tg", "totalSWE", "groundsnowdepth", "snowden")
SNOWMODEL_OUT3 = ("Tc", "Tg", "sdepc", "sdepg", "sden")
SNOWMODEL_OUT2 = ("agec", "ageg", "meltc", "meltg")

SnowClimate = _ptr_struct("SnowClimate", SNOW_CLIM_FIELDS)
SnowPointm = _ptr_struct("SnowPointm", SNOW_POINTM_FIELDS)
SnowVegp = _ptr_struct("SnowVegp", SNOW_VEGP_FIELDS)
Snowm = _ptr_struct("Snowm", SNOWM_FIELDS)
SnowModelOut = _ptr_struct("SnowModelOut", SNOWMODEL_OUT3 + SNOWMODEL_OUT2)


class SnowOther(C.Structure):
    _fields_ = [("slope", c_double_p), ("aspect", c_double_p), ("skyview", c_double_p), ("wsa", c_double_p),
                ("hor", c_double_p), ("lat", C.c_double), ("lon", C.c_double), ("lats", c_double_p),
                ("lons", c_double_p), ("zref", C.c_double), ("isnowdc", c_double_p), ("isnowdg", c_double_p),
                ("isnowac", c_int32_p), ("isnowag", c_int32_p), ("Smax", c_double_p)]


class SnowInputs(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int64), ("tsteps", C.c_int64), ("array_forcing", C.c_int32),
                ("snowenv", C.c_int32), ("obstime", Obstime), ("clim", SnowClimate), ("pointm", SnowPointm),
                ("vegp", SnowVegp), ("other", SnowOther)]


POINT_WEATHER_FIELDS = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "precip")
PointWeather = _ptr_struct("PointWeather", POINT_WEATHER_FIELDS)
BIGLEAF_FIELDS = ("Tc", "Tg", "H", "G", "psih", "psim", "phih", "OL", "uf", "RabsG", "albedo")


class BigLeafOut(C.Structure):
    _fields_ = [(k, c_double_p) for k in BIGLEAF_FIELDS] + [("err", C.c_double), ("iters", C.c_int32)]


class BigLeafBatchOut(C.Structure):
    """include/mcf.h mcf_bigleaf_batch_out: series [P][n], err / iters [P]"""
    _fields_ = [(k, c_double_p) for k in BIGLEAF_FIELDS] + [("err", c_double_p), ("iters", c_int32_p)]


class NcSpec(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("nsteps", C.c_int64), ("east", c_double_p),
                ("north", c_double_p), ("time_hours", c_double_p), ("crs_wkt", C.c_char_p), ("reqhgt", C.c_double),
                ("vars", C.c_int32 * 10), ("reference_puts_only", C.c_int32), ("format", C.c_int32),
                ("deflate_level", C.c_int32)]


class NcPackSpec(C.Structure):
    """include/mcf.h mcf_ncpack_spec"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("nsteps", C.c_int64), ("east", c_double_p),
                ("north", c_double_p), ("time_hours", c_double_p), ("crs_wkt", C.c_char_p), ("series", C.c_int32 * 5),
                ("scale", C.c_double * 5), ("units", C.c_char_p * 5), ("long_name", C.c_char_p * 5), ("format", C.c_int32),
                ("deflate_level", C.c_int32)]


POINTSNOW_FIELDS = ("Tc", "Tg", "sdepc", "sdepg", "sdenc", "sdeng", "G", "RswabsG", "RlwabsG", "tr", "umu", "sublmelt",
                    "tempmelt", "rainmelt", "sstemp")


# mcf_pointsnow_batch_out lists the [n + 1] depths after the [n] series
POINTSNOW_BATCH_FIELDS = tuple(k for k in POINTSNOW_FIELDS if k not in ("sdepc", "sdepg")) + ("sdepc", "sdepg")


class PointSnowOut(C.Structure):
    _fields_ = [(k, c_double_p) for k in POINTSNOW_FIELDS] + [("mxdif", C.c_double), ("iters", C.c_int32)]


class PointSnowBatchOut(C.Structure):
    """include/mcf.h mcf_pointsnow_batch_out: series [P][n] (sdepc / sdepg [P][n + 1]), mxdif / iters [P]"""
    _fields_ = ([(k, c_double_p) for k in POINTSNOW_BATCH_FIELDS] + [("mxdif", c_double_p), ("iters", c_int32_p)])


class SnowDriverIn(C.Structure):
    _fields_ = [("base", SnowInputs), ("dtm", c_double_p), ("res", C.c_double), ("tfact", C.c_double),
                ("chunk_steps", C.c_int32), ("af_wsa_s", C.c_int32), ("af_wind", c_double_p)]


SNOWDRIVER_OUT = ("Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden")
SnowDriverOut = _ptr_struct("SnowDriverOut", SNOWDRIVER_OUT)

SNOWFAST_SERIES = ("sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc", "sdeng", "temp_all", "snow_all")


class SnowFastIn(C.Structure):
    """include/mcf.h mcf_snowfast_in"""
    _fields_ = ([("drv", SnowDriverIn), ("n_all", C.c_int64), ("subs", C.POINTER(C.c_int64))]
                + [(k, c_double_p) for k in SNOWFAST_SERIES])


SNOWFAST2_SELECTED = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "precip", "windu", "windv",
                      "Gp", "Tc", "RswabsG", "RlwabsG", "umu")
SNOWFAST2_SERIES = ("sublmelt", "tempmelt", "rainmelt", "snow", "sstemp", "tc", "sdenc", "sdeng")


class SnowFast2In(C.Structure):
    """include/mcf.h mcf_snowfast2_in"""
    _fields_ = ([("drv", SnowDriverIn), ("coarse_rows", C.c_int64), ("coarse_cols", C.c_int64), ("coarse_rowpos", c_double_p),
                 ("coarse_colpos", c_double_p), ("altcorrect", C.c_int32), ("reserved", C.c_int32), ("coarse_dtm", c_double_p)]
                + [(k, c_double_p) for k in SNOWFAST2_SELECTED]
                + [("n_all", C.c_int64), ("subs", C.POINTER(C.c_int64))]
                + [(k, c_double_p) for k in SNOWFAST2_SERIES])


class SnowCoarseIn(C.Structure):
    """include/mcf.h mcf_snowcoarse_in"""
    _fields_ = ([("drv", SnowDriverIn), ("coarse_rows", C.c_int64), ("coarse_cols", C.c_int64), ("coarse_rowpos", c_double_p),
                 ("coarse_colpos", c_double_p), ("altcorrect", C.c_int32), ("reserved", C.c_int32), ("coarse_dtm", c_double_p)]
                + [(k, c_double_p) for k in SNOWFAST2_SELECTED])


# the thirteen series of the snow model on the raster, in the order mcf_snow_expand_coarse_device returns them
SNOW_FINE_SERIES = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "precip", "Gp", "Tc", "RswabsG", "RlwabsG", "umu")

SNOWFAST2_OUT = SNOWDRIVER_OUT + ("umu",)
SnowFast2Out = _ptr_struct("SnowFast2Out", SNOWFAST2_OUT)      # mcf_snowfast2_out: mcf_snowdriver_out, then umu


class MicrosnowIn(C.Structure):
    """include/mcf.h mcf_microsnow_in"""
    _fields_ = [("grid", C.POINTER(GridInputs)), ("snow", C.POINTER(SnowDriverIn)), ("micro", C.POINTER(SnowInputs)),
                ("mat", C.c_double)]


# the ten coarse arrays of the snow-day microclimate's weather (mcf_microcoarse_in), and its nine series on the raster in the order
# mcf_microsnow_expand_coarse_device returns them
MICRO_COARSE = ("temp", "ea", "pres", "swdown", "difrad", "lwdown", "windu", "windv", "precip", "umu")
MICRO_FINE_SERIES = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "precip", "umu")


class MicroCoarseIn(C.Structure):
    """include/mcf.h mcf_microcoarse_in"""
    _fields_ = ([("rows", C.c_int64), ("cols", C.c_int64), ("tsteps", C.c_int64), ("dtm", c_double_p), ("coarse_rows", C.c_int64),
                 ("coarse_cols", C.c_int64), ("coarse_rowpos", c_double_p), ("coarse_colpos", c_double_p), ("altcorrect", C.c_int32),
                 ("reserved", C.c_int32), ("coarse_dtm", c_double_p)] + [(k, c_double_p) for k in MICRO_COARSE])


class MicrosnowCoarseIn(C.Structure):
    """include/mcf.h mcf_microsnow_coarse_in"""
    _fields_ = [("grid", C.POINTER(GridInputs)), ("snow", C.POINTER(SnowCoarseIn)), ("micro", C.POINTER(MicroCoarseIn)),
                ("micro_static", C.POINTER(SnowInputs)), ("mat", C.c_double)]


class SnowpackSeriesSpec(C.Structure):
    """include/mcf.h mcf_snowpack_series_spec (series in SNOWDRIVER_OUT's order)"""
    _fields_ = [("npoints", C.c_int64), ("cells", C.POINTER(C.c_int64)), ("nzones", C.c_int32), ("zone", c_int32_p),
                ("series", C.c_int32 * 5), ("zstat", C.c_int32 * NZSTAT)]


class SnowpackSeriesOut(C.Structure):
    """include/mcf.h mcf_snowpack_series_out"""
    _fields_ = [("points", c_double_p * 5), ("zones", (c_double_p * NZSTAT) * 5)]


class SnowrunSeriesOut(C.Structure):
    """include/mcf.h mcf_snowrun_series_out"""
    _fields_ = [("micro", SeriesOut), ("pack", SnowpackSeriesOut), ("arrays", C.POINTER(Outputs)), ("smod", C.POINTER(SnowDriverOut)),
                ("snowday", c_int32_p), ("nosnowday", c_int32_p)]


class SnowrunNcOut(C.Structure):
    """include/mcf.h mcf_snowrun_nc_out"""
    _fields_ = [("arrays", C.POINTER(Outputs)), ("smod", C.POINTER(SnowDriverOut)), ("snowday", c_int32_p), ("nosnowday", c_int32_p)]


class DepthSeriesOut(C.Structure):
    """include/mcf.h mcf_depth_series_out"""
    _fields_ = [("tz_points", c_double_p * MAX_DEPTHS), ("tz_zones", (c_double_p * NZSTAT) * MAX_DEPTHS), ("soilm_points", c_double_p),
                ("soilm_zones", c_double_p * NZSTAT)]


class SnowrunSummaryOut(C.Structure):
    """include/mcf.h mcf_snowrun_summary_out"""
    _fields_ = [("micro", SummaryOut), ("pack", SnowpackSummaryOut), ("arrays", C.POINTER(Outputs)), ("smod", C.POINTER(SnowDriverOut)),
                ("snowday", c_int32_p), ("nosnowday", c_int32_p)]


class LeafrOut(C.Structure):
    """include/mcf.h mcf_leafr_out"""
    _fields_ = [("leafr", c_double_p), ("leaft", c_double_p), ("gref", c_double_p), ("iterations", C.c_int32),
                ("lref_first", C.c_int32), ("mxdif_gref", C.c_double), ("mxdif_leaf", C.c_double)]


_PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = _PKG_DIR / "csrc" / "libmcfhip.so"

# every symbol include/mcf.h declares (tests check the .so exports all of them)
EXPORTS = (
    "mcf_abi_version", "mcf_last_error", "mcf_device_count",
    "mcf_runmicro1", "mcf_runmicro2", "mcf_runmicro3", "mcf_runmicro4",
    "mcf_plan_create", "mcf_plan_destroy", "mcf_plan_twi_partial",
    "mcf_plan_set_twi_mean", "mcf_plan_upload_forcing_days", "mcf_plan_run_days",
    "mcf_plan_belowground", "mcf_plan_sync", "mcf_plan_fetch", "mcf_plan_fetch_cells", "mcf_plan_fetch_packed", "mcf_plan_slot_ptr",
    "mcf_plan_ring_layout", "mcf_ring_index", "mcf_plan_run_days_at", "mcf_plan_run_days_masked", "mcf_plan_set_mxtc",
    "mcf_snowplan_covered_tiles", "mcf_plan_run_days_cells", "mcf_snowplan_free_cells",
    "mcf_runmicro1_multi", "mcf_runmicro2_multi", "mcf_runmicro3_multi", "mcf_runmicro4_multi", "mcf_plan_fetch_pitched",
    "mcf_snowplan_reset", "mcf_snowplan_checkpoint", "mcf_snowplan_restore", "mcf_snowplan_fetch_cells", "mcf_snowplan_keep_chunk", "mcf_snowplan_can_keep", "mcf_snowplan_set_keep_budget", "mcf_plan_set_mxtc_days", "mcf_snowplan_set_series",
    "mcf_snowplan_release_kept", "mcf_snowplan_meand_accumulate", "mcf_snowplan_micro_setup", "mcf_snowplan_microsnow",
    "mcf_plan_timer_start", "mcf_plan_timer_stop", "mcf_plan_kernel_timing",
    "mcf_plan_kernel_stats", "mcf_plan_dispatch_stats", "mcf_plan_valid_cells", "mcf_plan_bytes", "mcf_selftest_math",
    "mcf_precompute_terrain", "mcf_precompute_terrain_multi", "mcf_runbioclim1_multi", "mcf_runbioclim2_multi",
    "mcf_runbioclim3_multi", "mcf_runbioclim4_multi", "mcf_runbioclim1", "mcf_runbioclim2", "mcf_runbioclim3", "mcf_runbioclim4",
    "mcf_snowenv_from_name", "mcf_gridmodelsnow1", "mcf_gridmodelsnow2", "mcf_gridmicrosnow1",
    "mcf_gridmicrosnow2", "mcf_snowmodel1", "mcf_snowmodel2", "mcf_snowmodel1_multi", "mcf_applycpp3",
    "mcf_snowplan_create", "mcf_snowplan_destroy", "mcf_snowplan_chunks", "mcf_snowplan_surface", "mcf_snowplan_handover", "mcf_snowplan_apply3",
    "mcf_snowplan_surface_partial", "mcf_snowplan_prepare_chunk", "mcf_snowplan_run_chunk", "mcf_snowplan_pack_halo",
    "mcf_snowplan_prepare_chunk_dev",
    "mcf_bigleaf_batch", "mcf_weatherhgt_batch", "mcf_pointmprocess_batch", "mcf_pointmodelsnow_batch",
    "mcf_bigleaf", "mcf_soilm", "mcf_pointmprocess", "mcf_weatherhgt", "mcf_man", "mcf_pointmodelsnow", "mcf_canintfrac", "mcf_meltmu", "mcf_meltmu2", "mcf_tpicalc",
    "mcf_snowmodelq1", "mcf_canintfrac_device", "mcf_meltmu_device", "mcf_snowmodelq2", "mcf_meltmu2_device",
    "mcf_snowmodel2_coarse", "mcf_snow_expand_coarse_device",
    "mcf_nc_create", "mcf_nc_write_host", "mcf_nc_write_plan", "mcf_nc_close",
    "mcf_flowacc", "mcf_topidx",
    "mcf_runmicrosnow1", "mcf_runmicrosnow2", "mcf_runmicrosnow1_multi", "mcf_snowrun_create", "mcf_snowrun_destroy", "mcf_snowrun_days", "mcf_snowrun_stats", "mcf_snowrun_keep",
    "mcf_snowrun_pass1", "mcf_snowrun_pass2", "mcf_snowplan_run_chunk_pitched", "mcf_snowplan_chunk_af",
    "mcf_plan_create_streamed", "mcf_plan_below_prepare", "mcf_plan_below_set_days", "mcf_below_days_range",
    "mcf_runmicrosnow1_below", "mcf_runmicrosnow1_below_multi", "mcf_snowrun_create_below",
    "mcf_flowacc_device", "mcf_topidx_device", "mcf_plan_create_dtm", "mcf_runmicro_dtm",
    "mcf_find_lref", "mcf_find_gref", "mcf_fill_na", "mcf_find_lref_device", "mcf_find_gref_device", "mcf_fill_na_device",
    "mcf_leafrfromalb", "mcf_leafrfromalb_device", "mcf_selftest_vegprep",
    "mcf_plan_diag_enable", "mcf_plan_diag_fetch", "mcf_plan_diag_slot_ptr", "mcf_plan_diag_ring_layout",
    "mcf_runmicro1_diag", "mcf_runmicro3_diag",
    "mcf_plan_diag_enable_array", "mcf_runmicro2_diag", "mcf_runmicro4_diag",
    "mcf_plan_summary_enable", "mcf_plan_summary_accumulate", "mcf_plan_summary_fetch", "mcf_plan_summary_days",
    "mcf_plan_summary_reset", "mcf_runmicro_summary", "mcf_runmicro_summary_multi",
    "mcf_plan_below_set_depths", "mcf_plan_fetch_depth", "mcf_plan_fetch_depth_pitched", "mcf_plan_summary_enable_below",
    "mcf_plan_summary_fetch_depth", "mcf_runmicro_depths", "mcf_runmicro_depths_summary",
    "mcf_bioclim_last_chunks", "mcf_runbioclim_depths",
    "mcf_snowplan_summary_enable", "mcf_snowplan_summary_accumulate", "mcf_snowplan_summary_fetch", "mcf_snowplan_summary_days",
    "mcf_snowplan_summary_reset", "mcf_snowrun_summary_table", "mcf_snowrun_summary_enable", "mcf_snowrun_summary_fetch",
    "mcf_snowrun_summary_days", "mcf_runmicrosnow_summary", "mcf_snowmodel1_summary",
    "mcf_microsnow_expand_coarse_device", "mcf_runmicrosnow2_coarse", "mcf_snowrun_create_coarse",
    "mcf_plan_set_day_layers", "mcf_snowrun_set_day_layers", "mcf_plan_fetch_mxtc",
    "mcf_foliageden", "mcf_foliageden_device", "mcf_plan_set_height", "mcf_plan_fetch_foliage", "mcf_runmicro_heights",
    "mcf_selftest_step", "mcf_selftest_snow",
    "mcf_plan_series_enable", "mcf_plan_series_accumulate", "mcf_plan_series_fetch_points", "mcf_plan_series_fetch_zones",
    "mcf_plan_series_reset", "mcf_runmicro_series", "mcf_zonal_series",
    "mcf_series_state_merge", "mcf_series_state_finish", "mcf_runmicro_series_multi", "mcf_plan_series_enable_below",
    "mcf_plan_series_fetch_points_depth", "mcf_plan_series_fetch_zones_depth", "mcf_runmicro_depths_series",
    "mcf_snowplan_series_enable", "mcf_snowplan_series_accumulate", "mcf_snowplan_series_fetch_points",
    "mcf_snowplan_series_fetch_zones", "mcf_snowplan_series_reset", "mcf_snowrun_series_enable", "mcf_snowrun_series_fetch_points",
    "mcf_snowrun_series_fetch_zones", "mcf_runmicrosnow_series", "mcf_snowmodel1_series",
    "mcf_nc_write_plan_rows", "mcf_nc_write_missing", "mcf_nc_write_host_rows", "mcf_runmicro_nc", "mcf_runmicro_depths_nc",
    "mcf_nc_create_snowpack", "mcf_snowplan_nc_write", "mcf_snowmodel1_nc", "mcf_nc_write_planes",
    "mcf_snowrun_nc_enable", "mcf_runmicrosnow_nc", "mcf_snowrun_drop_days",
)

ABI_VERSION = 8     # include/mcf.h MCF_ABI_VERSION this mirror was written against
_lib = None


class McfError(RuntimeError):
    """Raised when libmcfhip reports a non-zero status."""


class DispatchStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("fast_tiles", "slow_tiles", "irregular_days", "fast_launches", "slow_launches",
                                         "canary_trips")]


class RingLayout(C.Structure):
    """include/mcf.h mcf_ring_layout: how a ring slot variable is addressed on the device."""
    _fields_ = [("tiled", C.c_int32), ("cells_per_tile", C.c_int32), ("block_doubles", C.c_int32), ("slot_days", C.c_int32),
                ("cells", C.c_int64), ("tile_stride", C.c_int64), ("day_stride", C.c_int64)]


def _needed_hip_soname(lib_path: Path):
    """DT_NEEDED entry of libmcfhip.so that names the HIP runtime (e.g. 'libamdhip64.so.7'), read from the ELF's dynamic
    section's strings; None if it cannot be found."""
    import re
    try:
        data = lib_path.read_bytes()
    except OSError:
        return None
    m = re.search(rb"libamdhip64\.so\.\d+", data)
    return m.group(0).decode() if m else None


def _share_hip_runtime(lib_path: Path):
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's); the copy
    that is loaded first serves every later user.  If libmcfhip pulled in /opt/rocm's first, a later `import torch` would
    bring a SECOND runtime into the process and find no device ("No HIP GPUs are available").  Where torch is installed but
    not imported yet, its copy is therefore loaded first — the same state as importing torch before this package.  Hosts
    without torch (an R session) use /opt/rocm's.

    Only when the wheel's runtime carries the SONAME libmcfhip was linked against (a different major would leave two runtimes
    in the process after all, silently): otherwise a warning says so and nothing is preloaded.  MCF_NO_HIP_PRELOAD=1 opts out
    (processes that will never import torch)."""
    import importlib.util
    import sys
    import warnings
    if "torch" in sys.modules or os.environ.get("MCF_NO_HIP_PRELOAD"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    cand = Path(spec.origin).parent / "lib" / "libamdhip64.so"
    if not cand.exists():
        return
    need, have = _needed_hip_soname(lib_path), _needed_hip_soname(cand)      # (a library's own SONAME string matches too)
    if need and have and need != have:
        warnings.warn(f"libmcfhip is linked against {need}, the installed torch bundles {have}: not preloading torch's HIP "
                      "runtime — import torch BEFORE microclimf_amd if both are used in this process", RuntimeWarning)
        return
    try:
        C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def load() -> C.CDLL:
    """Load libmcfhip.so (built by `make -C microclimf_amd/csrc` / build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("MCF_LIB", LIB_PATH))
    if not path.exists():
        raise McfError(
            f"{path} not found: the HIP extension is not built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C microclimf_amd/csrc`). There is no CPU fallback.")
    _share_hip_runtime(path)
    lib = C.CDLL(str(path))
    lib.mcf_abi_version.restype = C.c_int
    lib.mcf_last_error.restype = C.c_char_p
    lib.mcf_device_count.restype = C.c_int
    GI, OP, OU = C.POINTER(GridInputs), C.POINTER(Options), C.POINTER(Outputs)
    for fn in (lib.mcf_runmicro1, lib.mcf_runmicro2, lib.mcf_runmicro3, lib.mcf_runmicro4):
        fn.restype = C.c_int
        fn.argtypes = [GI, OP, OU]
    P = C.c_void_p
    lib.mcf_plan_create.restype = C.c_int
    lib.mcf_plan_create.argtypes = [GI, OP, C.c_int32, C.c_int32, C.POINTER(P)]
    lib.mcf_plan_destroy.restype = None
    lib.mcf_plan_destroy.argtypes = [P]
    lib.mcf_plan_twi_partial.restype = C.c_int
    lib.mcf_plan_twi_partial.argtypes = [P, c_double_p, C.POINTER(C.c_int64)]
    lib.mcf_plan_set_twi_mean.restype = C.c_int
    lib.mcf_plan_set_twi_mean.argtypes = [P, C.c_double]
    lib.mcf_plan_upload_forcing_days.restype = C.c_int
    lib.mcf_plan_upload_forcing_days.argtypes = [P, GI, C.c_int32, C.c_int32, C.c_int32]
    lib.mcf_plan_run_days.restype = C.c_int
    lib.mcf_plan_run_days.argtypes = [P, C.c_int32, C.c_int32, C.c_int32]
    if hasattr(lib, "mcf_plan_run_days_at"):     # (absent from an older library named by MCF_LIB for an A/B run)
        for fn in (lib.mcf_runmicro1_multi, lib.mcf_runmicro2_multi, lib.mcf_runmicro3_multi, lib.mcf_runmicro4_multi):
            fn.restype = C.c_int
            fn.argtypes = [GI, OP, C.POINTER(Multi), OU]
        lib.mcf_plan_fetch_pitched.restype = C.c_int
        lib.mcf_plan_fetch_pitched.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, c_double_p, C.c_int64]
        lib.mcf_plan_run_days_at.restype = C.c_int
        lib.mcf_plan_run_days_at.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.mcf_plan_set_mxtc.restype = C.c_int
        lib.mcf_plan_set_mxtc.argtypes = [P, C.c_double]
        lib.mcf_snowplan_reset.restype = C.c_int
        lib.mcf_snowplan_reset.argtypes = [P]
        lib.mcf_snowplan_fetch_cells.restype = C.c_int
        lib.mcf_snowplan_fetch_cells.argtypes = [P, C.c_int32, C.POINTER(C.c_int64), C.c_int32, c_double_p, C.POINTER(C.c_int32)]
        lib.mcf_snowplan_can_keep.restype = C.c_int
        lib.mcf_snowplan_can_keep.argtypes = [P, C.c_int64, C.POINTER(C.c_int32)]
        lib.mcf_snowplan_set_series.restype = C.c_int
        lib.mcf_snowplan_set_series.argtypes = [P, C.c_uint32]
        lib.mcf_snowplan_keep_chunk.restype = C.c_int
        lib.mcf_snowplan_keep_chunk.argtypes = [P, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]
        lib.mcf_snowplan_release_kept.restype = C.c_int
        lib.mcf_snowplan_release_kept.argtypes = [P]
        for fn in (lib.mcf_snowplan_checkpoint, lib.mcf_snowplan_restore):
            fn.restype = C.c_int
            fn.argtypes = [P, C.c_int32]
        lib.mcf_snowplan_meand_accumulate.restype = C.c_int
        lib.mcf_snowplan_meand_accumulate.argtypes = [P, C.c_int32, c_int32_p]
        lib.mcf_snowplan_micro_setup.restype = C.c_int
        lib.mcf_snowplan_micro_setup.argtypes = [P, C.POINTER(SnowInputs), c_int32_p, C.c_int32, C.c_double, C.c_double,
                                                 C.POINTER(C.c_int32 * NOUT), C.c_int32]
        lib.mcf_plan_run_days_masked.restype = C.c_int
        lib.mcf_plan_run_days_masked.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_int64]
        lib.mcf_snowplan_covered_tiles.restype = C.c_int
        lib.mcf_snowplan_covered_tiles.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(C.c_int64)]
        lib.mcf_plan_run_days_cells.restype = C.c_int
        lib.mcf_plan_run_days_cells.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        lib.mcf_snowplan_free_cells.restype = C.c_int
        lib.mcf_snowplan_free_cells.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        lib.mcf_snowplan_microsnow.restype = C.c_int
        lib.mcf_snowplan_microsnow.argtypes = [P, P, C.c_int32, C.c_int32, c_int32_p]
    lib.mcf_plan_belowground.restype = C.c_int
    lib.mcf_plan_belowground.argtypes = [P]
    lib.mcf_plan_create_streamed.restype = C.c_int
    lib.mcf_plan_create_streamed.argtypes = [GI, OP, C.c_int32, C.c_int32, C.POINTER(P)]
    lib.mcf_plan_below_prepare.restype = C.c_int
    lib.mcf_plan_below_prepare.argtypes = [P, GI]
    if hasattr(lib, "mcf_plan_below_set_days"):     # (absent from an older library named by MCF_LIB for an A/B run)
        lib.mcf_plan_below_set_days.restype = C.c_int
        lib.mcf_plan_below_set_days.argtypes = [P, c_int32_p, C.c_int32]
        lib.mcf_below_days_range.restype = C.c_int
        lib.mcf_below_days_range.argtypes = [c_int32_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p]
    lib.mcf_plan_sync.restype = C.c_int
    lib.mcf_plan_sync.argtypes = [P]
    if hasattr(lib, "mcf_plan_diag_enable"):
        DSEL = C.POINTER(C.c_int32 * NDIAG)
        lib.mcf_plan_diag_enable.restype = C.c_int
        lib.mcf_plan_diag_enable.argtypes = [P, DSEL]
        lib.mcf_plan_diag_fetch.restype = C.c_int
        lib.mcf_plan_diag_fetch.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, c_double_p]
        lib.mcf_plan_diag_slot_ptr.restype = C.c_int
        lib.mcf_plan_diag_slot_ptr.argtypes = [P, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        lib.mcf_plan_diag_ring_layout.restype = C.c_int
        lib.mcf_plan_diag_ring_layout.argtypes = [P, C.POINTER(RingLayout)]
        for fn in (lib.mcf_runmicro1_diag, lib.mcf_runmicro3_diag):
            fn.restype = C.c_int
            fn.argtypes = [GI, OP, DSEL, OU, C.POINTER(DiagOutputs)]
        if hasattr(lib, "mcf_plan_diag_enable_array"):      # (absent from an older library named by MCF_LIB for an A/B run)
            lib.mcf_plan_diag_enable_array.restype = C.c_int
            lib.mcf_plan_diag_enable_array.argtypes = [P, DSEL]
            for fn in (lib.mcf_runmicro2_diag, lib.mcf_runmicro4_diag):
                fn.restype = C.c_int
                fn.argtypes = [GI, OP, DSEL, OU, C.POINTER(DiagOutputs)]
    if hasattr(lib, "mcf_plan_series_enable"):      # (absent from an older library named by MCF_LIB for an A/B run)
        RS = C.POINTER(SeriesSpec)
        lib.mcf_plan_series_enable.restype = C.c_int
        lib.mcf_plan_series_enable.argtypes = [P, RS]
        lib.mcf_plan_series_accumulate.restype = C.c_int
        lib.mcf_plan_series_accumulate.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.mcf_plan_series_fetch_points.restype = C.c_int
        lib.mcf_plan_series_fetch_points.argtypes = [P, C.c_int32, c_double_p]
        lib.mcf_plan_series_fetch_zones.restype = C.c_int
        lib.mcf_plan_series_fetch_zones.argtypes = [P, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_plan_series_reset.restype = C.c_int
        lib.mcf_plan_series_reset.argtypes = [P]
        lib.mcf_runmicro_series.restype = C.c_int
        lib.mcf_runmicro_series.argtypes = [GI, OP, RS, C.c_int32, C.POINTER(SeriesOut)]
        lib.mcf_zonal_series.restype = C.c_int
        lib.mcf_zonal_series.argtypes = [c_double_p, C.c_int64, C.c_int64, C.c_int64, c_int32_p, C.c_int32, c_int32_p, C.c_int32,
                                         C.POINTER(c_double_p)]
    if hasattr(lib, "mcf_plan_summary_enable"):     # (absent from an older library named by MCF_LIB for an A/B run)
        SS, SO_ = C.POINTER(SummarySpec), C.POINTER(SummaryOut)
        lib.mcf_plan_summary_enable.restype = C.c_int
        lib.mcf_plan_summary_enable.argtypes = [P, SS]
        lib.mcf_plan_summary_accumulate.restype = C.c_int
        lib.mcf_plan_summary_accumulate.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.mcf_plan_summary_fetch.restype = C.c_int
        lib.mcf_plan_summary_fetch.argtypes = [P, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_plan_summary_days.restype = C.c_int
        lib.mcf_plan_summary_days.argtypes = [P, c_int32_p]
        lib.mcf_plan_summary_reset.restype = C.c_int
        lib.mcf_plan_summary_reset.argtypes = [P]
        lib.mcf_runmicro_summary.restype = C.c_int
        lib.mcf_runmicro_summary.argtypes = [GI, OP, SS, C.c_int32, SO_]
        lib.mcf_runmicro_summary_multi.restype = C.c_int
        lib.mcf_runmicro_summary_multi.argtypes = [GI, OP, SS, C.c_int32, C.POINTER(Multi), SO_]
    if hasattr(lib, "mcf_plan_below_set_depths"):     # (absent from an older library named by MCF_LIB for an A/B run)
        SS = C.POINTER(SummarySpec)
        lib.mcf_plan_below_set_depths.restype = C.c_int
        lib.mcf_plan_below_set_depths.argtypes = [P, c_double_p, C.c_int32, c_double_p]
        lib.mcf_plan_fetch_depth.restype = C.c_int
        lib.mcf_plan_fetch_depth.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, c_double_p]
        lib.mcf_plan_fetch_depth_pitched.restype = C.c_int
        lib.mcf_plan_fetch_depth_pitched.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, c_double_p, C.c_int64]
        lib.mcf_plan_summary_enable_below.restype = C.c_int
        lib.mcf_plan_summary_enable_below.argtypes = [P, SS]
        lib.mcf_plan_summary_fetch_depth.restype = C.c_int
        lib.mcf_plan_summary_fetch_depth.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_runmicro_depths.restype = C.c_int
        lib.mcf_runmicro_depths.argtypes = [GI, OP, c_double_p, C.c_int32, c_double_p, C.POINTER(DepthOutputs)]
        lib.mcf_runmicro_depths_summary.restype = C.c_int
        lib.mcf_runmicro_depths_summary.argtypes = [GI, OP, c_double_p, C.c_int32, c_double_p, SS, C.c_int32,
                                                    C.POINTER(DepthSummaryOut)]
    lib.mcf_plan_fetch.restype = C.c_int
    lib.mcf_plan_fetch.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, c_double_p]
    lib.mcf_plan_fetch_cells.restype = C.c_int
    lib.mcf_plan_fetch_cells.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_int64,
                                         c_double_p]
    lib.mcf_plan_fetch_packed.restype = C.c_int
    lib.mcf_plan_fetch_packed.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_double, c_int32_p,
                                          C.POINTER(C.c_float)]
    lib.mcf_plan_slot_ptr.restype = C.c_int
    lib.mcf_plan_slot_ptr.argtypes = [P, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    try:
        lib.mcf_plan_ring_layout.restype = C.c_int
        lib.mcf_plan_ring_layout.argtypes = [P, C.POINTER(RingLayout)]
        lib.mcf_ring_index.restype = C.c_int64
        lib.mcf_ring_index.argtypes = [C.POINTER(RingLayout), C.c_int64, C.c_int64]
    except AttributeError:
        if "MCF_LIB" not in os.environ:     # an older library named for a same-box A/B run (tools/ab_bench2.sh) may lack them
            raise
    lib.mcf_plan_timer_start.restype = C.c_int
    lib.mcf_plan_timer_start.argtypes = [P]
    lib.mcf_plan_timer_stop.restype = C.c_int
    lib.mcf_plan_timer_stop.argtypes = [P, C.POINTER(C.c_float)]
    lib.mcf_plan_kernel_timing.restype = C.c_int
    lib.mcf_plan_kernel_timing.argtypes = [P, C.c_int32]
    lib.mcf_plan_kernel_stats.restype = C.c_int
    lib.mcf_plan_kernel_stats.argtypes = [P, c_double_p, C.POINTER(C.c_int64)]
    lib.mcf_plan_dispatch_stats.restype = C.c_int
    lib.mcf_plan_dispatch_stats.argtypes = [P, C.POINTER(DispatchStats)]
    lib.mcf_plan_valid_cells.restype = C.c_int64
    lib.mcf_plan_valid_cells.argtypes = [P]
    lib.mcf_plan_bytes.restype = C.c_int64
    lib.mcf_plan_bytes.argtypes = [P]
    lib.mcf_selftest_math.restype = C.c_int
    lib.mcf_selftest_math.argtypes = [C.c_int32, c_double_p, c_double_p, c_double_p, C.c_int64, C.c_int32]
    if hasattr(lib, "mcf_selftest_step"):     # (absent from an older library named by MCF_LIB for an A/B run)
        lib.mcf_selftest_step.restype = C.c_int
        lib.mcf_selftest_step.argtypes = [C.c_int32, c_double_p, C.c_int32, c_double_p, C.c_int32, C.c_int64, C.c_int32]
    if hasattr(lib, "mcf_selftest_snow"):
        lib.mcf_selftest_snow.restype = C.c_int
        lib.mcf_selftest_snow.argtypes = [C.c_int32, c_double_p, C.c_int32, c_double_p, C.c_int32, C.c_int64, C.c_int32]
    for fn in (lib.mcf_runbioclim1, lib.mcf_runbioclim2, lib.mcf_runbioclim3, lib.mcf_runbioclim4):
        fn.restype = C.c_int
        fn.argtypes = [GI, OP, C.POINTER(BioclimSel), C.POINTER(BioclimOut)]
    for fn in (lib.mcf_runbioclim1_multi, lib.mcf_runbioclim2_multi, lib.mcf_runbioclim3_multi, lib.mcf_runbioclim4_multi):
        fn.restype = C.c_int
        fn.argtypes = [GI, OP, C.POINTER(BioclimSel), C.POINTER(Multi), C.POINTER(BioclimOut)]
    lib.mcf_bioclim_last_chunks.restype = C.c_int
    lib.mcf_bioclim_last_chunks.argtypes = []
    if hasattr(lib, "mcf_runbioclim_depths"):     # (absent from an older library named by MCF_LIB for an A/B run)
        lib.mcf_runbioclim_depths.restype = C.c_int
        lib.mcf_runbioclim_depths.argtypes = [GI, OP, C.POINTER(BioclimSel), c_double_p, C.c_int32, C.c_int32,
                                              C.POINTER(BioclimDepthsOut)]
    lib.mcf_snowenv_from_name.restype = C.c_int32
    lib.mcf_snowenv_from_name.argtypes = [C.c_char_p]
    SI = C.POINTER(SnowInputs)
    for fn in (lib.mcf_gridmodelsnow1, lib.mcf_gridmodelsnow2):
        fn.restype = C.c_int
        fn.argtypes = [SI, C.POINTER(SnowModelOut), C.c_int32]
    for fn in (lib.mcf_gridmicrosnow1, lib.mcf_gridmicrosnow2):
        fn.restype = C.c_int
        fn.argtypes = [SI, C.POINTER(Snowm), C.c_double, C.c_double, C.POINTER(C.c_int32 * NOUT), OU, C.c_int32]
    PW, OT = C.POINTER(PointWeather), C.POINTER(Obstime)
    lib.mcf_bigleaf.restype = C.c_int
    lib.mcf_bigleaf.argtypes = [C.c_int64, OT, PW, c_double_p, c_double_p, c_double_p, C.c_double, C.c_double, C.c_double,
                                C.c_double, C.c_int32, C.c_double, C.c_double, C.c_int32, C.POINTER(BigLeafOut)]
    lib.mcf_soilm.restype = C.c_int
    lib.mcf_soilm.argtypes = [C.c_int64, PW] + [C.c_double] * 7 + [c_double_p, C.POINTER(C.c_int64)]
    lib.mcf_pointmprocess.restype = C.c_int
    lib.mcf_pointmprocess.argtypes = [C.c_int64] + [c_double_p] * 7 + [C.c_double] * 7 + [c_double_p] * 6
    lib.mcf_weatherhgt.restype = C.c_int
    lib.mcf_weatherhgt.argtypes = [C.c_int64, OT, PW] + [C.c_double] * 5 + [c_double_p] * 3
    lib.mcf_bigleaf_batch.restype = C.c_int
    lib.mcf_bigleaf_batch.argtypes = ([C.c_int64, C.c_int64, OT, PW] + [c_double_p] * 5 + [C.c_double, C.c_double, C.c_int32,
                                      C.c_double, C.c_double, C.c_int32, C.c_int64, C.c_int32, C.POINTER(BigLeafBatchOut)])
    lib.mcf_weatherhgt_batch.restype = C.c_int
    lib.mcf_weatherhgt_batch.argtypes = ([C.c_int64, C.c_int64, OT, PW] + [C.c_double] * 3 + [c_double_p] * 2 +
                                         [C.c_int64, C.c_int32] + [c_double_p] * 3)
    lib.mcf_pointmprocess_batch.restype = C.c_int
    lib.mcf_pointmprocess_batch.argtypes = ([C.c_int64, C.c_int64] + [c_double_p] * 7 + [C.c_double] + [c_double_p] * 6 +
                                            [C.c_int32] + [c_double_p] * 6)
    lib.mcf_pointmodelsnow.restype = C.c_int
    lib.mcf_pointmodelsnow.argtypes = [C.c_int64, C.POINTER(Obstime), C.POINTER(PointWeather), c_double_p, c_double_p,
                                       C.c_int32, C.c_double, C.c_double, C.POINTER(PointSnowOut)]
    lib.mcf_pointmodelsnow_batch.restype = C.c_int
    lib.mcf_pointmodelsnow_batch.argtypes = [C.c_int64, C.c_int64, OT, PW, c_double_p, c_double_p, c_int32_p, C.c_double,
                                             C.c_double, C.c_int64, C.c_int32, C.POINTER(PointSnowBatchOut)]
    lib.mcf_man.restype = C.c_int
    lib.mcf_man.argtypes = [C.c_int64, c_double_p, C.c_int32, c_double_p]
    lib.mcf_flowacc.restype = C.c_int
    lib.mcf_flowacc.argtypes = [C.c_int64, C.c_int64, c_double_p, c_double_p]
    lib.mcf_topidx.restype = C.c_int
    lib.mcf_topidx.argtypes = [C.c_int64, C.c_int64, c_double_p, C.c_double, C.c_double, c_double_p]
    lib.mcf_flowacc_device.restype = C.c_int
    lib.mcf_flowacc_device.argtypes = [C.c_int64, C.c_int64, c_double_p, c_double_p, C.c_int32]
    lib.mcf_topidx_device.restype = C.c_int
    lib.mcf_topidx_device.argtypes = [C.c_int64, C.c_int64, c_double_p, C.c_double, C.c_double, c_double_p, C.c_int32]
    solve = [C.c_int64, C.c_int64, c_double_p, c_double_p, c_double_p, c_double_p, C.c_double, c_double_p]
    fill = [C.c_int64, C.c_int64, c_double_p, c_double_p, c_double_p]
    loop = [C.c_int64, C.c_int64, c_double_p, c_double_p, c_double_p, C.c_double, C.POINTER(LeafrOut)]
    for name, args in (("mcf_find_lref", solve), ("mcf_find_gref", solve), ("mcf_fill_na", fill), ("mcf_leafrfromalb", loop)):
        for fn, extra in ((getattr(lib, name), []), (getattr(lib, name + "_device"), [C.c_int32])):
            fn.restype = C.c_int
            fn.argtypes = args + extra
    lib.mcf_selftest_vegprep.restype = C.c_int
    lib.mcf_selftest_vegprep.argtypes = ([C.c_int32, C.c_int64, C.c_int64] + [c_double_p] * 5 + [C.c_double, c_double_p, C.c_int32,
                                                                                                C.c_int32])
    lib.mcf_plan_create_dtm.restype = C.c_int
    lib.mcf_plan_create_dtm.argtypes = [GI, OP, C.POINTER(DtmSpec), C.c_int32, C.c_int32, C.POINTER(P)]
    lib.mcf_runmicro_dtm.restype = C.c_int
    lib.mcf_runmicro_dtm.argtypes = [GI, OP, C.POINTER(DtmSpec), C.POINTER(Multi), C.POINTER(Outputs)]
    lib.mcf_nc_create.restype = C.c_int
    lib.mcf_nc_create.argtypes = [C.c_char_p, C.POINTER(NcSpec), C.POINTER(C.c_void_p)]
    lib.mcf_nc_write_host.restype = C.c_int
    lib.mcf_nc_write_host.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(c_double_p * 10)]
    lib.mcf_nc_write_plan.restype = C.c_int
    lib.mcf_nc_write_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                      C.POINTER(C.c_float)]
    lib.mcf_nc_close.restype = C.c_int
    lib.mcf_nc_close.argtypes = [C.c_void_p]
    lib.mcf_applycpp3.restype = C.c_int
    lib.mcf_applycpp3.argtypes = [c_double_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, c_double_p, c_double_p,
                                  C.c_int32]
    lib.mcf_snowplan_create.restype = C.c_int
    lib.mcf_snowplan_create.argtypes = [C.POINTER(SnowDriverIn), C.c_int64, C.c_int64, C.c_int32, C.POINTER(P)]
    lib.mcf_snowplan_destroy.restype = None
    lib.mcf_snowplan_destroy.argtypes = [P]
    lib.mcf_snowplan_chunks.restype = C.c_int32
    lib.mcf_snowplan_chunks.argtypes = [P]
    lib.mcf_snowplan_surface.restype = C.c_int
    lib.mcf_snowplan_surface.argtypes = [P, c_double_p]
    lib.mcf_snowplan_apply3.restype = C.c_int
    lib.mcf_snowplan_apply3.argtypes = [P, C.c_int32, C.c_int32, c_double_p, c_double_p]
    lib.mcf_snowplan_handover.restype = C.c_int
    lib.mcf_snowplan_handover.argtypes = [P, c_double_p]
    lib.mcf_snowplan_surface_partial.restype = C.c_int
    lib.mcf_snowplan_surface_partial.argtypes = [P, c_double_p, c_double_p]
    lib.mcf_snowplan_prepare_chunk.restype = C.c_int
    lib.mcf_snowplan_prepare_chunk.argtypes = [P, C.c_int32, c_double_p, C.c_int32, C.c_int32, C.c_double, c_double_p,
                                               c_double_p]
    lib.mcf_snowplan_pack_halo.restype = C.c_int
    lib.mcf_snowplan_pack_halo.argtypes = [P, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.mcf_snowplan_prepare_chunk_dev.restype = C.c_int
    lib.mcf_snowplan_prepare_chunk_dev.argtypes = [P, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, c_double_p,
                                                   c_double_p]
    lib.mcf_snowplan_run_chunk.restype = C.c_int
    lib.mcf_snowplan_run_chunk.argtypes = [P, C.c_int32, C.c_double, C.POINTER(SnowDriverOut)]
    lib.mcf_snowmodel1.restype = C.c_int
    lib.mcf_snowmodel1.argtypes = [C.POINTER(SnowDriverIn), C.POINTER(SnowDriverOut), C.c_int32]
    lib.mcf_snowmodel2.restype = C.c_int
    lib.mcf_snowmodel2.argtypes = [C.POINTER(SnowDriverIn), C.POINTER(SnowDriverOut), C.c_int32]
    lib.mcf_snowmodel1_multi.restype = C.c_int
    lib.mcf_snowmodel1_multi.argtypes = [C.POINTER(SnowDriverIn), C.POINTER(SnowDriverOut), C.POINTER(Multi)]
    if hasattr(lib, "mcf_snowmodelq1"):       # (absent from an older library named by MCF_LIB for an A/B run)
        lib.mcf_snowmodelq1.restype = C.c_int
        lib.mcf_snowmodelq1.argtypes = [C.POINTER(SnowFastIn), C.POINTER(SnowDriverOut), C.c_int32]
        lib.mcf_canintfrac_device.restype = C.c_int
        lib.mcf_canintfrac_device.argtypes = [C.c_int64, c_double_p, c_double_p, C.c_double, C.c_double, C.c_double, C.c_double,
                                              c_double_p, C.c_int32]
        lib.mcf_meltmu_device.restype = C.c_int
        lib.mcf_meltmu_device.argtypes = [C.c_int64, c_double_p, C.c_int64, c_double_p, c_double_p, c_double_p, C.c_int32]
    if hasattr(lib, "mcf_snowmodelq2"):       # (absent from an older library named by MCF_LIB for an A/B run)
        lib.mcf_snowmodelq2.restype = C.c_int
        lib.mcf_snowmodelq2.argtypes = [C.POINTER(SnowFast2In), C.POINTER(SnowFast2Out), C.c_int32]
        lib.mcf_meltmu2_device.restype = C.c_int
        lib.mcf_meltmu2_device.argtypes = [C.c_int64, C.c_int64, c_double_p, c_double_p, C.c_int64, C.c_int64, c_double_p, c_double_p,
                                           C.c_int64, c_double_p, c_double_p, c_double_p, C.c_int32]
    if hasattr(lib, "mcf_snowmodel2_coarse"):     # (absent from an older library named by MCF_LIB for an A/B run)
        lib.mcf_snowmodel2_coarse.restype = C.c_int
        lib.mcf_snowmodel2_coarse.argtypes = [C.POINTER(SnowCoarseIn), C.POINTER(SnowFast2Out), C.c_int32]
        lib.mcf_snow_expand_coarse_device.restype = C.c_int
        lib.mcf_snow_expand_coarse_device.argtypes = [C.POINTER(SnowCoarseIn), C.c_int64, C.c_int64, C.POINTER(c_double_p), C.c_int32]
    if hasattr(lib, "mcf_runmicrosnow1"):     # (absent from an older library named by MCF_LIB for an A/B run)
        MI, SO = C.POINTER(MicrosnowIn), C.POINTER(SnowDriverOut)
        lib.mcf_runmicrosnow1.restype = C.c_int
        lib.mcf_runmicrosnow1.argtypes = [MI, OP, OU, SO]
        lib.mcf_runmicrosnow2.restype = C.c_int
        lib.mcf_runmicrosnow2.argtypes = [MI, OP, OU, SO]
        lib.mcf_plan_set_mxtc_days.restype = C.c_int
        lib.mcf_plan_set_mxtc_days.argtypes = [P, C.POINTER(GridInputs), c_int32_p, C.c_int32]
        lib.mcf_runmicrosnow1_multi.restype = C.c_int
        lib.mcf_runmicrosnow1_multi.argtypes = [MI, OP, C.POINTER(Multi), OU, SO]
        lib.mcf_snowrun_create.restype = C.c_int
        lib.mcf_snowrun_create.argtypes = [MI, OP, C.POINTER(Multi), C.POINTER(P)]
        if hasattr(lib, "mcf_snowrun_create_below"):
            lib.mcf_runmicrosnow1_below.restype = C.c_int
            lib.mcf_runmicrosnow1_below.argtypes = [MI, OP, OU, SO]
            lib.mcf_runmicrosnow1_below_multi.restype = C.c_int
            lib.mcf_runmicrosnow1_below_multi.argtypes = [MI, OP, C.POINTER(Multi), OU, SO]
            lib.mcf_snowrun_create_below.restype = C.c_int
            lib.mcf_snowrun_create_below.argtypes = [MI, OP, C.POINTER(Multi), C.POINTER(P)]
        lib.mcf_snowrun_destroy.restype = None
        lib.mcf_snowrun_destroy.argtypes = [P]
        lib.mcf_snowrun_stats.restype = C.c_int
        lib.mcf_snowrun_stats.argtypes = [P, C.POINTER(C.c_int64)]
        lib.mcf_snowrun_keep.restype = C.c_int
        lib.mcf_snowrun_keep.argtypes = [P, C.c_int64]
        lib.mcf_snowplan_set_keep_budget.restype = C.c_int
        lib.mcf_snowplan_set_keep_budget.argtypes = [P, C.c_int64]
        lib.mcf_snowrun_days.restype = C.c_int32
        lib.mcf_snowrun_days.argtypes = [P]
        lib.mcf_snowrun_pass1.restype = C.c_int
        lib.mcf_snowrun_pass1.argtypes = [P, SO, c_int32_p, c_int32_p]
        lib.mcf_snowrun_pass2.restype = C.c_int
        lib.mcf_snowrun_pass2.argtypes = [P, C.POINTER(SnowInputs), C.c_double, OU]
        lib.mcf_snowplan_run_chunk_pitched.restype = C.c_int
        lib.mcf_snowplan_run_chunk_pitched.argtypes = [P, C.c_int32, C.c_double, SO, C.c_int64]
        lib.mcf_snowplan_chunk_af.restype = C.c_int
        lib.mcf_snowplan_chunk_af.argtypes = [P, C.c_int32, C.POINTER(C.c_int32)]
    if hasattr(lib, "mcf_snowrun_summary_enable"):     # (absent from an older library named by MCF_LIB for an A/B run)
        SS, PS, PO = C.POINTER(SummarySpec), C.POINTER(SnowpackSummarySpec), C.POINTER(SnowpackSummaryOut)
        lib.mcf_snowplan_summary_enable.restype = C.c_int
        lib.mcf_snowplan_summary_enable.argtypes = [P, PS]
        lib.mcf_snowplan_summary_accumulate.restype = C.c_int
        lib.mcf_snowplan_summary_accumulate.argtypes = [P, C.c_int32]
        lib.mcf_snowplan_summary_fetch.restype = C.c_int
        lib.mcf_snowplan_summary_fetch.argtypes = [P, C.c_int32, C.c_int32, c_double_p, C.c_int64]
        lib.mcf_snowplan_summary_days.restype = C.c_int
        lib.mcf_snowplan_summary_days.argtypes = [P, c_int32_p]
        lib.mcf_snowplan_summary_reset.restype = C.c_int
        lib.mcf_snowplan_summary_reset.argtypes = [P]
        lib.mcf_snowrun_summary_table.restype = C.c_int
        lib.mcf_snowrun_summary_table.argtypes = [c_int32_p, c_int32_p, c_int32_p, C.c_int32, c_int32_p]
        lib.mcf_snowrun_summary_enable.restype = C.c_int
        lib.mcf_snowrun_summary_enable.argtypes = [P, SS, PS]
        lib.mcf_snowrun_summary_fetch.restype = C.c_int
        lib.mcf_snowrun_summary_fetch.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_snowrun_summary_days.restype = C.c_int
        lib.mcf_snowrun_summary_days.argtypes = [P, C.c_int32, c_int32_p]
        lib.mcf_runmicrosnow_summary.restype = C.c_int
        lib.mcf_runmicrosnow_summary.argtypes = [C.POINTER(MicrosnowIn), OP, C.POINTER(Multi), SS, PS, C.POINTER(SnowrunSummaryOut)]
        lib.mcf_snowmodel1_summary.restype = C.c_int
        lib.mcf_snowmodel1_summary.argtypes = [C.POINTER(SnowDriverIn), PS, C.POINTER(Multi), PO]
    if hasattr(lib, "mcf_snowrun_series_enable"):     # (absent from an older library named by MCF_LIB for an A/B run)
        RS, ZS, ZO = C.POINTER(SeriesSpec), C.POINTER(SnowpackSeriesSpec), C.POINTER(SnowpackSeriesOut)
        c_int64_p = C.POINTER(C.c_int64)
        lib.mcf_series_state_merge.restype = C.c_int
        lib.mcf_series_state_merge.argtypes = [c_int64_p, c_int64_p, C.c_int32, C.c_int64]
        lib.mcf_series_state_finish.restype = C.c_int
        lib.mcf_series_state_finish.argtypes = [c_int64_p, C.c_int32, C.c_int64, C.c_int64, c_int32_p, C.c_int32, c_double_p]
        lib.mcf_runmicro_series_multi.restype = C.c_int
        lib.mcf_runmicro_series_multi.argtypes = [GI, OP, RS, C.c_int32, C.POINTER(Multi), C.POINTER(SeriesOut)]
        lib.mcf_plan_series_enable_below.restype = C.c_int
        lib.mcf_plan_series_enable_below.argtypes = [P, RS]
        lib.mcf_plan_series_fetch_points_depth.restype = C.c_int
        lib.mcf_plan_series_fetch_points_depth.argtypes = [P, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_plan_series_fetch_zones_depth.restype = C.c_int
        lib.mcf_plan_series_fetch_zones_depth.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_runmicro_depths_series.restype = C.c_int
        lib.mcf_runmicro_depths_series.argtypes = [GI, OP, c_double_p, C.c_int32, c_double_p, RS, C.c_int32, C.POINTER(DepthSeriesOut)]
        lib.mcf_snowplan_series_enable.restype = C.c_int
        lib.mcf_snowplan_series_enable.argtypes = [P, ZS]
        lib.mcf_snowplan_series_accumulate.restype = C.c_int
        lib.mcf_snowplan_series_accumulate.argtypes = [P, C.c_int32]
        lib.mcf_snowplan_series_fetch_points.restype = C.c_int
        lib.mcf_snowplan_series_fetch_points.argtypes = [P, C.c_int32, c_double_p]
        lib.mcf_snowplan_series_fetch_zones.restype = C.c_int
        lib.mcf_snowplan_series_fetch_zones.argtypes = [P, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_snowplan_series_reset.restype = C.c_int
        lib.mcf_snowplan_series_reset.argtypes = [P]
        lib.mcf_snowrun_series_enable.restype = C.c_int
        lib.mcf_snowrun_series_enable.argtypes = [P, RS, ZS]
        lib.mcf_snowrun_series_fetch_points.restype = C.c_int
        lib.mcf_snowrun_series_fetch_points.argtypes = [P, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_snowrun_series_fetch_zones.restype = C.c_int
        lib.mcf_snowrun_series_fetch_zones.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, c_double_p]
        lib.mcf_runmicrosnow_series.restype = C.c_int
        lib.mcf_runmicrosnow_series.argtypes = [C.POINTER(MicrosnowIn), OP, C.POINTER(Multi), RS, ZS, C.POINTER(SnowrunSeriesOut)]
        lib.mcf_snowmodel1_series.restype = C.c_int
        lib.mcf_snowmodel1_series.argtypes = [C.POINTER(SnowDriverIn), ZS, C.POINTER(Multi), ZO]
    if hasattr(lib, "mcf_nc_write_plan_rows"):     # (absent from an older library named by MCF_LIB for an A/B run)
        NS = C.POINTER(NcSpec)
        lib.mcf_nc_write_plan_rows.restype = C.c_int
        lib.mcf_nc_write_plan_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_int64, C.POINTER(C.c_float)]
        lib.mcf_nc_write_missing.restype = C.c_int
        lib.mcf_nc_write_missing.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64]
        lib.mcf_nc_write_host_rows.restype = C.c_int
        lib.mcf_nc_write_host_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(c_double_p * 10)]
        lib.mcf_runmicro_nc.restype = C.c_int
        lib.mcf_runmicro_nc.argtypes = [GI, OP, C.POINTER(Multi), C.c_char_p, NS]
        lib.mcf_runmicro_depths_nc.restype = C.c_int
        lib.mcf_runmicro_depths_nc.argtypes = [GI, OP, c_double_p, C.c_int32, c_double_p, C.POINTER(C.c_char_p), NS]
        lib.mcf_nc_create_snowpack.restype = C.c_int
        lib.mcf_nc_create_snowpack.argtypes = [C.c_char_p, C.POINTER(NcPackSpec), C.POINTER(C.c_void_p)]
        lib.mcf_snowplan_nc_write.restype = C.c_int
        lib.mcf_snowplan_nc_write.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]
        lib.mcf_snowmodel1_nc.restype = C.c_int
        lib.mcf_snowmodel1_nc.argtypes = [C.POINTER(SnowDriverIn), C.POINTER(Multi), C.c_char_p, C.POINTER(NcPackSpec)]
        lib.mcf_snowrun_nc_enable.restype = C.c_int
        lib.mcf_snowrun_nc_enable.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mcf_snowrun_drop_days.restype = C.c_int
        lib.mcf_snowrun_drop_days.argtypes = [C.c_void_p, c_int32_p, C.c_int32]
        lib.mcf_runmicrosnow_nc.restype = C.c_int
        lib.mcf_runmicrosnow_nc.argtypes = [C.POINTER(MicrosnowIn), OP, C.POINTER(Multi), C.c_char_p, NS, C.c_char_p,
                                            C.POINTER(NcPackSpec), C.POINTER(SnowrunNcOut)]
        lib.mcf_nc_write_planes.restype = C.c_int
        lib.mcf_nc_write_planes.argtypes = [C.c_void_p, C.POINTER(c_double_p * 5), C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                            C.c_int32, C.POINTER(C.c_float)]
    if hasattr(lib, "mcf_runmicrosnow2_coarse"):     # (absent from an older library named by MCF_LIB for an A/B run)
        MC = C.POINTER(MicrosnowCoarseIn)
        lib.mcf_microsnow_expand_coarse_device.restype = C.c_int
        lib.mcf_microsnow_expand_coarse_device.argtypes = [C.POINTER(MicroCoarseIn), C.c_int64, C.c_int64, C.POINTER(c_double_p), C.c_int32]
        lib.mcf_runmicrosnow2_coarse.restype = C.c_int
        lib.mcf_runmicrosnow2_coarse.argtypes = [MC, OP, OU, C.POINTER(SnowFast2Out)]
        lib.mcf_snowrun_create_coarse.restype = C.c_int
        lib.mcf_snowrun_create_coarse.argtypes = [MC, OP, C.POINTER(Multi), c_double_p, C.POINTER(P)]
        lib.mcf_plan_fetch_mxtc.restype = C.c_int
        lib.mcf_plan_fetch_mxtc.argtypes = [P, c_double_p]
        for fn in (lib.mcf_plan_set_day_layers, lib.mcf_snowrun_set_day_layers):
            fn.restype = C.c_int
            fn.argtypes = [P, c_int32_p, C.c_int32]
    if hasattr(lib, "mcf_plan_set_height"):     # (absent from an older library named by MCF_LIB for an A/B run)
        lib.mcf_foliageden.restype = C.c_int
        lib.mcf_foliageden.argtypes = [C.c_int64, c_double_p, c_double_p, C.c_double, c_double_p, c_double_p]
        lib.mcf_foliageden_device.restype = C.c_int
        lib.mcf_foliageden_device.argtypes = [C.c_int64, c_double_p, c_double_p, C.c_double, c_double_p, c_double_p, C.c_int32]
        lib.mcf_plan_set_height.restype = C.c_int
        lib.mcf_plan_set_height.argtypes = [P, C.c_double, c_double_p]
        lib.mcf_plan_fetch_foliage.restype = C.c_int
        lib.mcf_plan_fetch_foliage.argtypes = [P, c_double_p, c_double_p]
        lib.mcf_runmicro_heights.restype = C.c_int
        lib.mcf_runmicro_heights.argtypes = [GI, OP, c_double_p, C.c_int32, C.POINTER(c_double_p), OU]
    lib.mcf_precompute_terrain.restype = C.c_int
    lib.mcf_precompute_terrain.argtypes = [C.POINTER(TerrainIn), C.POINTER(TerrainOut), C.c_int32]
    lib.mcf_precompute_terrain_multi.restype = C.c_int
    lib.mcf_precompute_terrain_multi.argtypes = [C.POINTER(TerrainIn), C.POINTER(TerrainOut), C.POINTER(Multi)]
    if lib.mcf_abi_version() != ABI_VERSION:
        raise McfError("libmcfhip ABI version mismatch")
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != 0:
        msg = load().mcf_last_error()
        raise McfError(f"libmcfhip error {status}: {msg.decode() if msg else '?'}")
