"""Inputs of the coarse array-weather snow run's tests (test_snowrun2_coarse_gpu.py): snowfast_cases.q2_case(0)'s product inputs —
the bundled site's 23 x 37 window under a 2 x 3 climate grid — cut to eleven days (two 5-day chunks and a one-day tail that only
the solver runs), with a hole in the dtm, a temperature ramp (cold, then two steps up) so that the period holds snow days,
no-snow days and days of both classes, and starting bare (test_snowmodel2_coarse_gpu.py ORACLE_CASES says why).  Everything here
is host code."""
import functools

import numpy as np

from microclimf_amd import frontend as F
from snowfast_cases import q2_case

NDAYS = 11
T11 = NDAYS * 24
# the ramp, tuned on the oracle's `.snowmodel2` (oracle/snowarray_oracle.py) until the day classes below hold for it: the cold
# spell builds a pack everywhere, the first step up starts the melt, the second bares part of the raster
RAMP = (-3.0, 4 * 24, 9.0, 7 * 24, 6.0)


@functools.lru_cache(maxsize=None)
def product(altcorrect):
    """-> (climarray, obstime, micropoints, vegp, soilc, dtm, kw) of the case: what `runpointmodela` / `runsnowmodela` /
    `runmicro_snow_array` take"""
    climarray, obstime, _, vegp, soilc, dtm, kw = q2_case(0)["product"]
    t = np.arange(T11)
    clima = {k: np.array(np.asarray(v)[:, :, :T11], dtype=np.float64, order="F") for k, v in climarray.items()}
    base, t1, up1, t2, up2 = RAMP
    clima["temp"] = np.asfortranarray(clima["temp"] + (base + up1 * (t > t1) + up2 * (t > t2))[None, None, :])
    obst = {k: np.asarray(v)[:T11] for k, v in obstime.items()}
    z = np.array(dtm["z"], dtype=np.float64)
    z[5:7, 6:9] = np.nan                                     # a hole of the dtm
    dtm = dict(dtm, z=z)
    kw = dict(kw, altcorrect=altcorrect, snowinitd=0.0, method="slow")
    mpa = F.runpointmodela(clima, obst, 0.05, dtm, vegp, soilc, lats=kw["lats_c"], lons=kw["lons_c"])
    return clima, obst, mpa, vegp, soilc, dtm, kw


@functools.lru_cache(maxsize=None)
def snow_inputs(altcorrect):
    """`runsnowmodela(..., method="slow", inputs_only=True)` of the case: snow.snowmodel2_coarse's arguments by name"""
    clima, obst, mpa, vegp, soilc, dtm, kw = product(altcorrect)
    return F.runsnowmodela(clima, obst, mpa, vegp, soilc, dtm, inputs_only=True, **kw)


def snow_args(si):
    """-> (args, pos, kw): snow.snowmodel2_coarse(*args, **pos, **kw) / snowarray_oracle.snowmodel2_chunks(*args, rowpos, colpos, ...)"""
    args = tuple(si[k] for k in ("obstime", "clim_c", "pointm_c", "vegp", "other", "snowenv", "dtm", "dtmc", "res", "tfact"))
    return args, dict(rowpos=si["rowpos"], colpos=si["colpos"], altcorrect=si["altcorrect"]), dict(agg=si["agg"])


def day_classes(swe, hole):
    """snowdaysfun on host arrays: `.runmicrosnow2` reads NA as no snow, the dtm's holes as NA -> (snowdays, nosnowdays), 0 / 1 per day"""
    s = np.array(swe, dtype=np.float64, copy=True)
    s[np.isnan(s)] = 0.0
    s[hole] = np.nan
    with np.errstate(all="ignore"):
        mx, mn = np.nanmax(s, axis=(0, 1)), np.nanmin(s, axis=(0, 1))
    sd = (mx.reshape(-1, 24) > 0).any(axis=1).astype(np.int32)
    nd = (mn.reshape(-1, 24) == 0).any(axis=1).astype(np.int32)
    return sd, nd


def check_classes(swe, hole):
    """what the case is there for, asserted on a snow model's totalSWE: at least two snow days, two no-snow days, a day in both
    classes, every day in a class, covered and uncovered valid cell-steps on snow days"""
    sd, nd = day_classes(swe, hole)
    assert sd.sum() >= 2 and nd.sum() >= 2, (sd, nd)
    assert (sd & nd).any(), (sd, nd)
    assert (sd | nd).all(), (sd, nd)
    steps = np.repeat(sd.astype(bool), 24)
    s = np.nan_to_num(np.asarray(swe)[:, :, steps])
    covered = s > 0
    assert covered[~hole].any() and (~covered[~hole]).any()
    return sd, nd
