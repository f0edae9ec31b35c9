"""A null array among the inputs of a snow entry is refused by name, and of two null arrays the one that comes first in its
group's listing is the one reported (microclimf_amd/csrc/mcf_snow.hip: each_model_raster, each_micro_raster, each_model_series,
each_micro_series).  The host code walks one listing per group for the uploads, the null checks and the row gathers, so the
refusals pin the listings' coverage and order: for each entry family the first, a middle and the last array of each group is
set to null after marshalling, then two at once.

Where the library names the array, the message has to; the snow run's checks ahead of its row gathers (a gather from a null
array would fault) answer for a whole group — "a snow-model raster", "a gridmicrosnow1 raster" — and that text is matched."""
import ctypes as C

import numpy as np
import pytest

from microclimf_amd import _abi
from microclimf_amd import snow as S
from microclimf_amd import synthetic

pytestmark = pytest.mark.gpu
R, CC = 3, 2
MAT = 7.5

# (path in mcf_snow_inputs, what the message has to name): first, middle and last of each group's listing
MODEL_RASTERS = ("vegp.pai", "other.isnowdc", "other.isnowag")
MODEL_SERIES = ("clim.temp", "clim.windspeed", "pointm.umu")
MICRO_RASTERS = ("vegp.pai", "vegp.leafden", "other.hor")
MICRO_SERIES = ("clim.temp", "clim.lwdown", "clim.umu", "clim.winddir")


def _name(path):
    return path.split(".")[1]


def _null(si, path):
    group, field = path.split(".")
    setattr(getattr(si, group), field, None)


def _refused(call, pattern):
    with pytest.raises(_abi.McfError, match=pattern):
        call()


def _names(path):
    """`null input` and the array's name"""
    return r"null input.*\b" + _name(path) + r"\b"


@pytest.fixture(scope="module")
def sw24():
    return synthetic.snow_workload(R, CC, 24, cold=3.0, zref=3.5)


# ---- mcf_gridmodelsnow1 ----------------------------------------------------------------------------------------------
def _gridmodelsnow1(sw, nulls):
    m = S.marshal_snow(sw["obstime"], sw["climdata"], sw["vegp"], sw["other"], False, pointm=sw["pointm"], snowenv=sw["snowenv"])
    out, _arrays = S.alloc_snowmodel_out(m)
    for path in nulls:
        _null(m.inputs, path)
    _abi.check(_abi.load().mcf_gridmodelsnow1(C.byref(m.inputs), C.byref(out), 0))


@pytest.mark.parametrize("path", MODEL_RASTERS + ("other.hor",) + MODEL_SERIES + ("clim.winddir",))
def test_gridmodelsnow1_names_the_null_array(sw24, path):
    _refused(lambda: _gridmodelsnow1(sw24, [path]), _names(path))


@pytest.mark.parametrize("nulls,first", [(("other.isnowag", "vegp.pai"), "vegp.pai"), (("other.isnowdg", "other.isnowdc"), "other.isnowdc"),
                                         (("other.isnowdc", "other.hor"), "other.hor"), (("clim.temp", "other.isnowag"), "other.isnowag"),
                                         (("clim.relhum", "clim.precip"), "clim.precip"), (("pointm.umu", "pointm.Gp"), "pointm.Gp"),
                                         (("clim.temp", "clim.winddir"), "clim.winddir")])
def test_gridmodelsnow1_reports_the_first_of_two(sw24, nulls, first):
    _refused(lambda: _gridmodelsnow1(sw24, nulls), _names(first))


# ---- mcf_gridmicrosnow1 ----------------------------------------------------------------------------------------------
def _gridmicrosnow1(sw, nulls, out=(1,) * 10):
    T = 24
    m = S.marshal_snow(sw["obstime"], sw["climdata"], sw["vegp"], sw["other"], False, micro=True)
    z = np.zeros((R, CC, T), order="F")
    sm = S.marshal_snowm(m, {f: z for f in _abi.SNOWM_FIELDS})
    sel, outs, _arrays = S.marshal_micro(m, {n: z for n in _abi.OUT_NAMES}, out)
    for path in nulls:
        _null(m.inputs, path)
    _abi.check(_abi.load().mcf_gridmicrosnow1(C.byref(m.inputs), C.byref(sm), 0.05, MAT, C.byref(sel), C.byref(outs), 0))


@pytest.mark.parametrize("path", MICRO_RASTERS + MICRO_SERIES)
def test_gridmicrosnow1_names_the_null_array(sw24, path):
    _refused(lambda: _gridmicrosnow1(sw24, [path]), _names(path))


@pytest.mark.parametrize("nulls,first", [(("other.hor", "vegp.clump"), "vegp.clump"), (("clim.temp", "other.hor"), "other.hor"),
                                         (("clim.umu", "clim.precip"), "clim.precip"), (("clim.temp", "clim.winddir"), "clim.winddir")])
def test_gridmicrosnow1_reports_the_first_of_two(sw24, nulls, first):
    _refused(lambda: _gridmicrosnow1(sw24, nulls), _names(first))


def test_gridmicrosnow1_smax_is_needed_for_soilm_only(sw24):
    _refused(lambda: _gridmicrosnow1(sw24, ["other.Smax"]), r"soilm requested but other\$Smax is null")
    # soilm (the fourth output) not asked for: Smax is not read, the next null array is what is reported
    _refused(lambda: _gridmicrosnow1(sw24, ["other.Smax", "clim.umu"], out=(1, 1, 1, 0, 1, 1, 1, 1, 1, 1)), _names("clim.umu"))


# ---- mcf_snowplan_create ---------------------------------------------------------------------------------------------
def _snowplan_create(sw, nulls):
    lib = _abi.load()
    m = S.marshal_snow(sw["obstime"], sw["climdata"], sw["vegp"], S._terrain_placeholders(sw["other"], R, CC), False,
                       pointm=sw["pointm"], snowenv=sw["snowenv"])
    din = _abi.SnowDriverIn()
    din.base = m.inputs
    din.dtm = m.f64(synthetic.rasters(R, CC)[2], (R, CC), "dtm")
    din.res, din.tfact, din.chunk_steps = 1.0, 0.02, 24
    for path in nulls:
        _null(din.base, path)
    p = C.c_void_p()
    try:
        _abi.check(lib.mcf_snowplan_create(C.byref(din), 0, 0, 0, C.byref(p)))
    finally:
        if p.value:
            lib.mcf_snowplan_destroy(p)


@pytest.mark.parametrize("path", MODEL_RASTERS + MODEL_SERIES)
def test_snowplan_create_names_the_null_array(sw24, path):
    _refused(lambda: _snowplan_create(sw24, [path]), _names(path))


@pytest.mark.parametrize("nulls,first", [(("other.isnowag", "vegp.pai"), "vegp.pai"), (("other.isnowag", "other.isnowac"), "other.isnowac"),
                                         (("clim.temp", "other.isnowag"), "other.isnowag"), (("clim.relhum", "clim.precip"), "clim.precip"),
                                         (("clim.temp", "clim.windspeed"), "clim.windspeed"), (("pointm.umu", "pointm.Tc"), "pointm.Tc")])
def test_snowplan_create_reports_the_first_of_two(sw24, nulls, first):
    _refused(lambda: _snowplan_create(sw24, nulls), _names(first))


# ---- mcf_snowplan_micro_setup ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan24(sw24):
    with S.SnowPlan(sw24["obstime"], sw24["climdata"], sw24["pointm"], sw24["vegp"], sw24["other"], sw24["snowenv"],
                    synthetic.rasters(R, CC)[2], 1.0, chunk_steps=24, keep_results=False) as plan:
        yield plan


def _micro_setup(plan, sw, nulls):
    m = S.marshal_snow(sw["obstime"], sw["climdata"], sw["vegp"], sw["other"], False, micro=True)
    for path in nulls:
        _null(m.inputs, path)
    sod = np.zeros(1, np.int32)          # the one day of the series is the subset's day 0
    sel = (C.c_int32 * _abi.NOUT)(*([1] * _abi.NOUT))
    _abi.check(plan._lib.mcf_snowplan_micro_setup(plan._p, C.byref(m.inputs), sod.ctypes.data_as(_abi.c_int32_p), 1, 0.05, MAT,
                                                  C.byref(sel), 0))


@pytest.mark.parametrize("path", MICRO_RASTERS + MICRO_SERIES)
def test_micro_setup_names_the_null_array(plan24, sw24, path):
    _refused(lambda: _micro_setup(plan24, sw24, [path]), _names(path))


@pytest.mark.parametrize("nulls,first", [(("other.hor", "vegp.paia"), "vegp.paia"), (("clim.temp", "other.hor"), "other.hor"),
                                         (("clim.umu", "clim.relhum"), "clim.relhum"), (("clim.temp", "clim.winddir"), "clim.winddir")])
def test_micro_setup_reports_the_first_of_two(plan24, sw24, nulls, first):
    _refused(lambda: _micro_setup(plan24, sw24, nulls), _names(first))


# ---- mcf_runmicrosnow1 / mcf_runmicrosnow1_multi: two chunks of one day ------------------------------------------------
@pytest.fixture(scope="module")
def run48():
    T = 48
    sw = synthetic.snow_workload(R, CC, T, cold=3.0, zref=3.5)
    a = synthetic.workload(R, CC, T, reqhgt=0.05, zref=3.5, hgt_range=(0.05, 3.0), start_doy=15, variety=True)
    snow = dict(sw, dtm=synthetic.rasters(R, CC)[2], res=1.0, tfact=0.02, chunk_steps=24)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    return a, snow, micro


def _runmicrosnow1(case, n_blocks, snow_nulls=(), micro_nulls=()):
    from microclimf_amd.marshal import alloc_outputs
    a, snow, micro = case
    lib = _abi.load()
    with S.SnowRun(a, snow, handle=False) as run:
        run._mm = S.marshal_snow(micro["obstime"], micro["climdata"], micro["vegp"], micro["other"], False, micro=True)
        run._in.micro = C.pointer(run._mm.inputs)
        run._in.mat = MAT
        for path in snow_nulls:
            _null(run._din.base, path)
        for path in micro_nulls:
            _null(run._mm.inputs, path)
        outs, _arrays = alloc_outputs(run._gm)
        mu = _abi.multi([0], n_blocks)
        _abi.check(lib.mcf_runmicrosnow1_multi(C.byref(run._in), C.byref(run._gm.options), C.byref(mu[0]), C.byref(outs), None))


@pytest.mark.parametrize("n_blocks", [1, 2])
@pytest.mark.parametrize("path", MODEL_RASTERS)
def test_runmicrosnow1_refuses_a_null_snow_model_raster(run48, n_blocks, path):
    _refused(lambda: _runmicrosnow1(run48, n_blocks, snow_nulls=[path]), r"null input: a snow-model raster")


@pytest.mark.parametrize("n_blocks", [1, 2])
@pytest.mark.parametrize("path", MODEL_SERIES)
def test_runmicrosnow1_names_the_null_snow_model_series(run48, n_blocks, path):
    _refused(lambda: _runmicrosnow1(run48, n_blocks, snow_nulls=[path]), _names(path))


@pytest.mark.parametrize("n_blocks", [1, 2])
@pytest.mark.parametrize("path", MICRO_RASTERS)
def test_runmicrosnow1_refuses_a_null_gridmicrosnow1_raster(run48, n_blocks, path):
    _refused(lambda: _runmicrosnow1(run48, n_blocks, micro_nulls=[path]), r"null input: a gridmicrosnow1 raster")


@pytest.mark.parametrize("n_blocks", [1, 2])
@pytest.mark.parametrize("path", MICRO_SERIES)
def test_runmicrosnow1_names_the_null_gridmicrosnow1_series(run48, n_blocks, path):
    _refused(lambda: _runmicrosnow1(run48, n_blocks, micro_nulls=[path]), r"null input: gridmicrosnow1 weather\$" + _name(path) + r"\b")


@pytest.mark.parametrize("n_blocks", [1, 2])
@pytest.mark.parametrize("snow_nulls,micro_nulls,pattern", [
    ((), ("clim.umu", "clim.winddir"), r"weather\$winddir"),             # the run's check walks the ten series in their order
    ((), ("clim.winddir", "clim.lwdown"), r"weather\$lwdown"),
    ((), ("other.hor", "clim.umu"), r"weather\$umu"),                    # the series are checked ahead of the rasters
    (("clim.relhum", "clim.precip"), (), r"null input.*\bprecip\b"),
    (("clim.temp",), ("vegp.pai",), r"null input.*\btemp\b"),            # the snow model's inputs are read first (pass 1)
    (("other.isnowag",), ("clim.temp",), r"a snow-model raster")])
def test_runmicrosnow1_reports_the_first_of_two(run48, n_blocks, snow_nulls, micro_nulls, pattern):
    _refused(lambda: _runmicrosnow1(run48, n_blocks, snow_nulls=snow_nulls, micro_nulls=micro_nulls), pattern)


def test_runmicrosnow1_runs_with_nothing_null(run48):
    """(the case has snow days: the refusals above of gridmicrosnow1's inputs are reached)"""
    _runmicrosnow1(run48, 2)
