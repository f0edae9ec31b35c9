"""Period summaries of the snow run and of the snowpack, CPU side: the new entries of the C ABI exist, judge their arguments
before a device is needed and have no CPU fallback; the table rule for days of neither class; the front end's argument
errors.  (On the device: tests/test_snow_summary_gpu.py.)"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import _abi, frontend, synthetic
from microclimf_amd import snow as S

NEW = ("mcf_snowplan_summary_enable", "mcf_snowplan_summary_accumulate", "mcf_snowplan_summary_fetch", "mcf_snowplan_summary_days",
       "mcf_snowplan_summary_reset", "mcf_snowrun_summary_table", "mcf_snowrun_summary_enable", "mcf_snowrun_summary_fetch",
       "mcf_snowrun_summary_days", "mcf_runmicrosnow_summary", "mcf_snowmodel1_summary")
MAT = 7.5
ROWS, COLS, DAYS = 6, 5, 12      # two whole 5-day chunks and two days behind them


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def _case(reqhgt=0.05, chunk_steps=120):
    T = DAYS * 24
    sw = synthetic.snow_workload(ROWS, COLS, T, cold=0.0, zref=3.5, start_doy=90)
    a = synthetic.workload(ROWS, COLS, T, reqhgt=reqhgt, zref=3.5, hgt_range=(0.05, 3.0), start_doy=90, variety=True)
    _, _, dtm = synthetic.rasters(ROWS, COLS)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02, chunk_steps=chunk_steps)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    return sw, a, dtm, snow, micro


TAB = [0] * 5 + [1] * 5 + [-1] * 2


def _run(summary=None, pack=None, **case):
    sw, a, dtm, snow, micro = _case(**case)
    return S.runmicrosnow1(a, snow, micro, MAT, summary=summary, pack_summary=pack, want_arrays=False)


def _model(chunk_steps=120, **kw):
    sw, a, dtm, snow, micro = _case()
    return S.snowmodel1_summary(sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02,
                                chunk_steps=chunk_steps, **kw)


def test_new_entries_are_declared_exported_and_bound():
    lib = _lib()
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mcf.h").read_text()
    for n in NEW:
        assert n in _abi.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert getattr(lib, n).argtypes is not None, n
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION
    # the structs as the header lays them out (LP64)
    assert C.sizeof(_abi.SnowpackSummarySpec) == 4 + 4 + 8 + 20 + 24 + 4 + 40
    assert C.sizeof(_abi.SnowpackSummaryOut) == 30 * 8 + 8
    assert C.sizeof(_abi.SnowrunSummaryOut) == C.sizeof(_abi.SummaryOut) + C.sizeof(_abi.SnowpackSummaryOut) + 4 * 8
    for field in ("series[5]", "stat[MCF_NSTAT]", "threshold[5]"):
        assert field in re.search(r"typedef struct mcf_snowpack_summary_spec \{(.*?)\}", hdr, re.S).group(1), field


def test_null_handles_are_refused():
    lib = _lib()
    buf, days = np.zeros(8), (C.c_int32 * 4)()
    E = 1   # MCF_ERR_ARG
    assert lib.mcf_snowplan_summary_enable(None, C.byref(_abi.SnowpackSummarySpec())) == E and b"null" in lib.mcf_last_error()
    assert lib.mcf_snowplan_summary_accumulate(None, 0) == E
    assert lib.mcf_snowplan_summary_fetch(None, 0, 0, buf.ctypes.data_as(_abi.c_double_p), 0) == E
    assert lib.mcf_snowplan_summary_days(None, days) == E
    assert lib.mcf_snowplan_summary_reset(None) == E
    assert lib.mcf_snowrun_summary_enable(None, None, None) == E
    assert lib.mcf_snowrun_summary_fetch(None, 0, 0, 0, buf.ctypes.data_as(_abi.c_double_p)) == E
    assert lib.mcf_snowrun_summary_days(None, 0, days) == E
    assert lib.mcf_runmicrosnow_summary(None, None, None, None, None, None) == E
    assert lib.mcf_snowmodel1_summary(None, None, None, None) == E


MICRO = dict(periods=TAB, vars=("Tz",), stats=("mean",))
PACK = dict(periods=TAB, vars=("totalSWE",), stats=("mean",))


@pytest.mark.parametrize("summary,pack,case,msg", [
    (dict(MICRO, nperiods=0), None, {}, "summary: nperiods must be at least 1"),
    (None, dict(PACK, nperiods=0), {}, "snowpack summary: nperiods must be at least 1"),
    (dict(MICRO, periods=[0] * 5 + [2] + [1] * 6, nperiods=2), None, {}, r"summary: period_of_day\[5\] = 2 is outside"),
    (None, dict(PACK, periods=[0, -2] + [1] * 8 + [-1] * 2), {}, r"snowpack summary: period_of_day\[1\] = -2 is outside"),
    (dict(MICRO, stats=("mean", "hours_above")), None, {}, "summary: HOURS_ABOVE needs a threshold"),
    (None, dict(PACK, vars=("Tc", "totalSWE"), stats=("hours_above",), thresholds={"totalSWE": 0.0}), {},
     "snowpack summary: HOURS_ABOVE needs a threshold"),
    (dict(MICRO, vars=()), None, {}, "no variable selected"),
    (dict(MICRO, stats=()), None, {}, "no statistic selected"),
    (None, dict(PACK, vars=()), {}, "no series selected"),
    (None, dict(PACK, stats=()), {}, "snowpack summary: no statistic selected"),
    (None, PACK, dict(chunk_steps=100), "chunk_steps must be whole days"),
    (None, dict(PACK, periods=[0] * 5 + [1] * 6 + [-1]), {}, "day 10 is counted but lies past the last whole chunk"),
    (MICRO, None, dict(reqhgt=-0.1), "need reqhgt >= 0"),
], ids=["nperiods<1", "pack-nperiods<1", "entry-too-large", "pack-entry-below--1", "nan-threshold", "pack-nan-threshold-of-one", "no-vars",
        "no-stats", "pack-no-series", "pack-no-stats", "chunk-not-whole-days", "counted-day-past-the-chunks", "below-ground"])
def test_snow_run_refusals_that_need_no_device(summary, pack, case, msg):
    """MCF_ERR_ARG with a message, before any device is touched: the same on a host with and without one"""
    _lib()
    with pytest.raises(_abi.McfError, match=r"error 1: .*" + msg):
        _run(summary, pack, **case)


def test_null_spec_is_refused():
    lib = _lib()
    sw, a, dtm, snow, micro = _case()
    with S.SnowRun(a, snow, handle=False) as run:
        so = _abi.SnowrunSummaryOut()
        rc = lib.mcf_runmicrosnow_summary(C.byref(run._in), C.byref(run._gm.options), None, None, None, C.byref(so))
        assert rc == 1 and b"null spec" in lib.mcf_last_error()
    m = S.marshal_snow(sw["obstime"], sw["climdata"], sw["vegp"], S._terrain_placeholders(sw["other"], ROWS, COLS), False, pointm=sw["pointm"],
                       snowenv=sw["snowenv"])
    din = _abi.SnowDriverIn()
    din.base = m.inputs
    rc = lib.mcf_snowmodel1_summary(C.byref(din), None, None, C.byref(_abi.SnowpackSummaryOut()))
    assert rc == 1 and b"null mcf_snowpack_summary_spec" in lib.mcf_last_error()


@pytest.mark.parametrize("kw,chunk,msg", [
    (dict(PACK, nperiods=0), 120, "nperiods must be at least 1"),
    (dict(PACK, periods=[0] * 5 + [3] + [1] * 4 + [-1] * 2, nperiods=2), 120, r"period_of_day\[5\] = 3 is outside"),
    (dict(PACK, stats=("hours_above",)), 120, "HOURS_ABOVE needs a threshold"),
    (dict(PACK, vars=()), 120, "no series selected"),
    (PACK, 100, "chunk_steps must be a multiple of 24"),
    (dict(PACK, periods=[0] * 12), 120, "day 10 is counted but lies past the last whole chunk"),
    (dict(PACK, periods=[0] * 4 + [-1] * 8), 96, None),
], ids=["nperiods<1", "entry-too-large", "nan-threshold", "no-series", "chunk%24", "counted-day-past-the-chunks", "valid-4-day-chunks"])
@pytest.mark.parametrize("multi", (False, True))
def test_snow_model_refusals_that_need_no_device(kw, chunk, msg, multi):
    lib = _lib()
    extra = dict(devices=[0], n_blocks=2) if multi else {}
    if msg is None:      # (valid: 12 days in 4-day chunks are all covered, the table counts the first chunk)
        if lib.mcf_device_count() > 0:
            assert _model(chunk, **kw, **extra)["totalSWE"]["mean"].shape == (ROWS, COLS, 1)
        else:
            with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
                _model(chunk, **kw, **extra)
        return
    with pytest.raises(_abi.McfError, match=r"error 1: .*snowpack summary: " + msg):
        _model(chunk, **kw, **extra)


def test_valid_arguments_need_a_device():
    """no CPU fallback: MCF_ERR_NO_DEVICE where there is none (on a GPU host the entries are covered by test_snow_summary_gpu.py)"""
    lib = _lib()
    full = dict(periods=TAB, vars=("Tz", "soilm"), stats=_abi.STAT_NAMES, thresholds=1.0)
    pack = dict(periods=TAB, vars=_abi.SNOWDRIVER_OUT, stats=_abi.STAT_NAMES, thresholds=0.0)
    if lib.mcf_device_count() > 0:
        got = _run(full, pack)
        assert got["summary"]["Tz"]["mean"].shape == got["summary"]["snow"]["totalSWE"]["max"].shape == (ROWS, COLS, 2)
        return
    for summary, pk in ((full, None), (None, pack), (full, pack)):
        with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
            _run(summary, pk)


def test_the_table_of_a_run_leaves_out_days_of_neither_class():
    lib = _lib()
    p = lambda x: x.ctypes.data_as(_abi.c_int32_p)
    #                 neither  snow only  both  no-snow only  tail day (no chunk: a no-snow day)  neither, already uncounted
    pod = np.array([1,       0,         1,    2,            2,                                  -1], dtype=np.int32)
    snowday = np.array([0, 1, 1, 0, 0, 0], dtype=np.int32)
    nosnowday = np.array([0, 0, 1, 1, 1, 0], dtype=np.int32)
    out = np.full(6, 99, dtype=np.int32)
    assert lib.mcf_snowrun_summary_table(p(pod), p(snowday), p(nosnowday), 6, p(out)) == 0
    assert out.tolist() == [-1, 0, 1, 2, 2, -1]
    assert lib.mcf_snowrun_summary_table(p(pod), p(snowday), p(nosnowday), 0, p(out)) == 0 and out.tolist() == [-1, 0, 1, 2, 2, -1]
    assert lib.mcf_snowrun_summary_table(None, p(snowday), p(nosnowday), 6, p(out)) == 1 and b"null" in lib.mcf_last_error()
    assert lib.mcf_snowrun_summary_table(p(pod), p(snowday), p(nosnowday), -1, p(out)) == 1


def test_front_end_argument_errors():
    with pytest.raises(ValueError, match="reqhgt >= 0"):
        frontend.runmicro_snow_summary({}, -0.05, {}, {}, {}, {})
    with pytest.raises(ValueError, match="vars"):
        frontend.runmicro_snow_summary({}, 0.05, {}, {}, {}, {}, vars=("Tz", "nope"))
    with pytest.raises(ValueError, match="snow_vars"):
        frontend.runmicro_snow_summary({}, 0.05, {}, {}, {}, {}, snow_vars=("swe",))
    with pytest.raises(ValueError, match="nothing selected"):
        frontend.runmicro_snow_summary({}, 0.05, {}, {}, {}, {}, vars=())
    with pytest.raises(ValueError, match="snow_inputs"):
        frontend.runmicro_snow_summary({}, 0.05, {}, {}, {}, None)
    with pytest.raises(ValueError, match="complete micropoint"):
        frontend.runmicro_snow_summary({"subs": [1, 2], "ntme": 48}, 0.05, {}, {}, {}, {})
    with pytest.raises(ValueError, match="vars"):
        frontend.runsnowmodel_summary({}, {}, {}, {}, {}, vars=("Tz",))
    with pytest.raises(ValueError, match="nothing selected"):
        frontend.runsnowmodel_summary({}, {}, {}, {}, {}, vars=())
    with pytest.raises(ValueError, match="reqhgt >= 0"):
        S.runmicrosnow1(*_case(-0.1)[1:2], *_case(-0.1)[3:5], MAT, below=True, summary=MICRO)
    assert frontend._pack_table([0] * 12, 12 * 24, 120).tolist() == [0] * 10 + [-1] * 2
