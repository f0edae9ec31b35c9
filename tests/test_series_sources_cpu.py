"""Series sink for the snow run, the snowpack, soil depths and row blocks, CPU side (include/mcf.h "series sink: further
sources"): the new entries exist, every refusal that needs no device comes before one is touched with the entry's name at the
start of the message, and the combination of row blocks — a host loop — gives the bits of tests/series_ref.py on the whole
raster."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import series_ref as ZR
import stages_cases as SC
from microclimf_amd import _abi, api
from microclimf_amd import snow as S

NEW = ("mcf_series_state_merge", "mcf_series_state_finish", "mcf_runmicro_series_multi", "mcf_plan_series_enable_below",
       "mcf_plan_series_fetch_points_depth", "mcf_plan_series_fetch_zones_depth", "mcf_runmicro_depths_series",
       "mcf_snowplan_series_enable", "mcf_snowplan_series_accumulate", "mcf_snowplan_series_fetch_points",
       "mcf_snowplan_series_fetch_zones", "mcf_snowplan_series_reset", "mcf_snowrun_series_enable", "mcf_snowrun_series_fetch_points",
       "mcf_snowrun_series_fetch_zones", "mcf_runmicrosnow_series", "mcf_snowmodel1_series")
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "complete", "mat")
bits = ZR.bits
E_ARG = 1
Z0 = np.zeros((SC.ROWS, SC.COLS), dtype=np.int32)


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def test_new_entries_are_declared_exported_and_bound():
    lib = _lib()
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mcf.h").read_text()
    for n in NEW:
        assert n in _abi.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert getattr(lib, n).argtypes is not None, n
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION and "#define MCF_ABI_VERSION 8" in hdr
    # the new structs (LP64), and the existing ones as they were
    assert C.sizeof(_abi.SnowpackSeriesSpec) == 8 + 8 + 8 + 8 + 20 + 16 + 4 and C.sizeof(_abi.SnowpackSeriesOut) == 5 * 8 + 20 * 8
    assert C.sizeof(_abi.DepthSeriesOut) == 8 * 8 + 32 * 8 + 8 + 4 * 8
    assert C.sizeof(_abi.SnowrunSeriesOut) == C.sizeof(_abi.SeriesOut) + C.sizeof(_abi.SnowpackSeriesOut) + 4 * 8
    assert C.sizeof(_abi.SeriesSpec) == 8 + 8 + 8 + 8 + 40 + 16 and C.sizeof(_abi.SeriesOut) == 80 + 40 * 8
    assert "totalSWE of 4096 or more" in hdr


# ---- refusals that need no device ---------------------------------------------------------------------------------------------
SPEC_CASES = [
    (dict(zones=Z0, vars=()), "no (variable|series) selected"),
    (dict(), "neither points nor zones"),
    (dict(zones=Z0, nzones=65), "nzones = 65 is outside"),
    (dict(zones=np.where(np.arange(50).reshape(5, 10) == 7, 3, 0), nzones=3), r"zone\[\d+\] = 3 is outside -1 .. nzones - 1"),
    (dict(points=[0, SC.ROWS * SC.COLS]), r"cells\[1\] = 50 is a cell index outside the raster"),
]
SPEC_IDS = ["empty-selection", "nothing-selected", "nzones>64", "label>=nzones", "cell>=N"]


def _args(**over):
    a = dict(SC.build("s170_h005"), **over)
    return [a[k] for k in ARGS]


@pytest.mark.parametrize("kw,msg", SPEC_CASES, ids=SPEC_IDS)
def test_runmicro_series_multi_refuses_before_a_device(kw, msg):
    _lib()
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicro_series_multi: .*" + msg):
        api.runmicro_series(*_args(), devices=[0, 0], n_blocks=3, **kw)


@pytest.mark.parametrize("kw,msg", SPEC_CASES, ids=SPEC_IDS)
def test_runmicro_depths_series_refuses_before_a_device(kw, msg):
    _lib()
    a = {k: v for k, v in zip(ARGS, _args()) if k != "reqhgt"}
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicro_depths_series: .*" + msg):
        api.runmicro_depths_series(**a, depths=[-0.05, -0.2], **kw)


def test_runmicro_depths_series_takes_tz_and_soilm_alone():
    _lib()
    a = {k: v for k, v in zip(ARGS, _args()) if k != "reqhgt"}
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicro_depths_series: below ground Tz and soilm"):
        api.runmicro_depths_series(**a, depths=[-0.05], zones=Z0, vars=("Tz", "tleaf"))


def _snow_case(reqhgt=0.05, rows=6, cols=5, ndays=5):
    """the inputs of the snow entries, as tests/test_snowrun_gpu.py makes them (no device is needed to marshal them)"""
    from microclimf_amd import synthetic
    T = ndays * 24
    sw = synthetic.snow_workload(rows, cols, T, cold=0.0, zref=3.5, start_doy=90)
    a = synthetic.workload(rows, cols, T, reqhgt=reqhgt, zref=3.5, hgt_range=(0.05, 3.0), start_doy=90, variety=True)
    _, _, dtm = synthetic.rasters(rows, cols)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    args = (sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
    return a, snow, micro, args


Z65 = np.zeros((6, 5), dtype=np.int32)
SNOW_CASES = [
    (dict(zones=Z65, vars=()), "no (variable|series) selected"),
    (dict(), "neither points nor zones"),
    (dict(zones=Z65, nzones=65), "nzones = 65 is outside"),
    (dict(zones=np.where(np.arange(30).reshape(6, 5) == 7, 3, 0), nzones=3), r"zone\[\d+\] = 3 is outside -1 .. nzones - 1"),
    (dict(points=[0, 30]), r"cells\[1\] = 30 is a cell index outside the raster"),
]


@pytest.mark.parametrize("kw,msg", SNOW_CASES, ids=SPEC_IDS)
def test_snowmodel1_series_refuses_before_a_device(kw, msg):
    _lib()
    a, snow, micro, args = _snow_case()
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_snowmodel1_series: .*" + msg):
        S.snowmodel1_series(*args, **kw)


@pytest.mark.parametrize("pack", (False, True), ids=["outputs", "snowpack"])
@pytest.mark.parametrize("kw,msg", SNOW_CASES, ids=SPEC_IDS)
def test_runmicrosnow_series_refuses_before_a_device(kw, msg, pack):
    _lib()
    a, snow, micro, args = _snow_case()
    sel = dict(pack_series=kw) if pack else dict(series=kw)
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicrosnow_series: .*" + msg):
        S.runmicrosnow1(a, snow, micro, 7.5, **sel)


def test_a_below_ground_snow_run_and_null_specs_are_refused():
    lib = _lib()
    a, snow, micro, args = _snow_case(reqhgt=-0.1)
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicrosnow_series: .*needs reqhgt >= 0"):
        S.runmicrosnow1(dict(a, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0]), snow, micro, 7.5, series=dict(zones=Z65))
    so, po, do, ro = _abi.SeriesOut(), _abi.SnowpackSeriesOut(), _abi.DepthSeriesOut(), _abi.SnowrunSeriesOut()
    m = api.marshal(*_args(), [1] + [0] * 9, False)
    d = np.array([-0.05])
    dp = d.ctypes.data_as(_abi.c_double_p)
    mu = _abi.multi([0, 0], 3)
    for call, name in ((lambda: lib.mcf_runmicro_series_multi(C.byref(m.inputs), C.byref(m.options), None, 0, C.byref(mu[0]), C.byref(so)),
                        b"mcf_runmicro_series_multi"),
                       (lambda: lib.mcf_runmicro_depths_series(C.byref(m.inputs), C.byref(m.options), dp, 1, None, None, 0, C.byref(do)),
                        b"mcf_runmicro_depths_series"),
                       (lambda: lib.mcf_snowmodel1_series(None, None, None, C.byref(po)), b"mcf_snowmodel1_series"),
                       (lambda: lib.mcf_runmicrosnow_series(None, None, None, None, None, C.byref(ro)), b"mcf_runmicrosnow_series"),
                       (lambda: lib.mcf_snowplan_series_enable(None, None), b"mcf_snowplan_series_enable"),
                       (lambda: lib.mcf_snowrun_series_enable(None, None, None), b"mcf_snowrun_series_enable"),
                       (lambda: lib.mcf_plan_series_enable_below(None, None), b"mcf_plan_series_enable_below")):
        assert call() == E_ARG and lib.mcf_last_error().startswith(name) and b"null" in lib.mcf_last_error(), name


def test_more_than_2_26_cells_is_judged_on_the_whole_raster_before_an_array_is_read():
    lib = _lib()
    m = api.marshal(*_args(), [1] + [0] * 9, False)
    sp, _, _ = api.series_spec(SC.ROWS, SC.COLS, [3], Z0, ("Tz",), ("mean",))
    so, do = _abi.SeriesOut(), _abi.DepthSeriesOut()
    mu = _abi.multi([0, 0], 3)
    m.inputs.rows, m.inputs.cols = 8193, 8192
    assert lib.mcf_runmicro_series_multi(C.byref(m.inputs), C.byref(m.options), C.byref(sp), 0, C.byref(mu[0]), C.byref(so)) == E_ARG
    assert re.match(rb"mcf_runmicro_series_multi: more than 2\^26 cells", lib.mcf_last_error())
    d = np.array([-0.05])
    assert lib.mcf_runmicro_depths_series(C.byref(m.inputs), C.byref(m.options), d.ctypes.data_as(_abi.c_double_p), 1, None, C.byref(sp), 0,
                                          C.byref(do)) == E_ARG
    assert re.match(rb"mcf_runmicro_depths_series: more than 2\^26 cells", lib.mcf_last_error())
    # the snow entries: rows x cols of the driver's raster
    ps, _, _ = S.snowpack_series_spec(6, 5, [3], Z65, ("totalSWE",), ("mean",))
    din, po = _abi.SnowDriverIn(), _abi.SnowpackSeriesOut()
    din.base.rows, din.base.cols = 8193, 8192
    assert lib.mcf_snowmodel1_series(C.byref(din), C.byref(ps), None, C.byref(po)) == E_ARG
    assert re.match(rb"mcf_snowmodel1_series: more than 2\^26 cells", lib.mcf_last_error())
    gi, opt, mi, ro = _abi.GridInputs(), _abi.Options(), _abi.MicrosnowIn(), _abi.SnowrunSeriesOut()
    gi.rows, gi.cols = 8193, 8192
    mi.grid, mi.snow = C.pointer(gi), C.pointer(din)
    for micro, pack in ((sp, None), (None, ps)):
        assert lib.mcf_runmicrosnow_series(C.byref(mi), C.byref(opt), None, C.byref(micro) if micro else None,
                                           C.byref(pack) if pack else None, C.byref(ro)) == E_ARG
        assert re.match(rb"mcf_runmicrosnow_series: more than 2\^26 cells", lib.mcf_last_error())


def test_the_planes_door_refuses_a_bad_label_and_a_bad_tile_size_before_a_device(monkeypatch):
    _lib()
    x3 = np.zeros((2, 4, 30))
    monkeypatch.setenv("MCF_ZONAL_CPB", "0")
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_zonal_series: zone\[4\] = 2 is outside"):
        api.zonal_series(x3, np.array([[0, 1, 2, 1], [0, 0, 0, 0]]), nzones=2)
    monkeypatch.setenv("MCF_ZONAL_CPB", "8")
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_zonal_series: MCF_ZONAL_CPB must be 0, 16, 21, 32 or 42"):
        api.zonal_series(x3, np.zeros((2, 4), int))


# ---- the combination of row blocks: a host loop, tested here directly --------------------------------------------------------
def _state_of(x, zone, nzones, steps):
    """the zone state of include/mcf.h "Row blocks" for x[rows, cols, T] by plain numpy: [4][nzones][steps] of int64"""
    st = np.zeros((4, nzones, steps), dtype=np.int64)
    st[2], st[3] = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    T = x.shape[2]
    with np.errstate(invalid="ignore"):
        for z in range(nzones):
            vals = x[zone == z]
            for k in range(min(T, steps)):
                v = vals[:, k]
                v = v[~np.isnan(v)]
                bad = ~(np.abs(v) < ZR.LIMIT)
                ok = v[~bad]
                st[1, z, k] = ok.size + (int(bad.sum()) << 32)
                if ok.size:
                    st[0, z, k] = np.rint(ok * 2 ** 24).astype(np.int64).sum(dtype=np.int64)
                    b = ok.view(np.int64)
                    key = np.where(b >= 0, b, b ^ np.iinfo(np.int64).max)
                    st[2, z, k], st[3, z, k] = key.min(), key.max()
    return st


def _finish(lib, st, nzones, steps, nsteps, done, stat):
    out = np.empty((nsteps, nzones), order="F")
    i64 = C.POINTER(C.c_int64)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    rc = lib.mcf_series_state_finish(st.ctypes.data_as(i64), nzones, steps, nsteps, None if dn is None else dn.ctypes.data_as(_abi.c_int32_p),
                                     stat, out.ctypes.data_as(_abi.c_double_p))
    assert rc == 0, lib.mcf_last_error()
    return out


@pytest.mark.parametrize("cuts", ((0, 9), (0, 3, 6, 9), (0, 1, 2, 8, 9)), ids=["one-block", "three-blocks", "four-uneven"])
def test_blocks_states_combined_and_finished_once_have_the_bits_of_the_whole_raster(cuts):
    lib = _lib()
    rng = np.random.default_rng(3)
    q = ZR.QUANTUM
    rows, cols, T, steps, nz = 9, 7, 50, 48, 5
    x = np.asfortranarray(np.round(rng.normal(size=(rows, cols, T)) * 30, 4))
    zone = ((np.arange(rows * cols).reshape(rows, cols) * 5) % 4).astype(np.int32)      # labels 0 .. 3 in every block: they straddle
    zone[4, :] = 4                                                                       # a zone inside one block
    zone[0, 0] = zone[8, 6] = -1
    x[4, :, 7] = np.nan                                      # a zone-step without a counted value
    x[1, 1, 3], x[7, 2, 3] = -0.0, np.nan
    x[2, 3, 5], x[5, 3, 5] = (6 + 0.5) * q, (-7 - 0.5) * q   # half-quantum ties in two blocks
    x[0, 2, 9] = 4096.0                                      # bad in one block: the whole zone-step
    x[8, 1, 10] = -np.inf
    x[3, 3, 11] = 4096.0 - q
    x[6, 0, 12] = ZR.na_real()
    done = np.array([1, 0], dtype=np.int32)                  # day 1 never folded; steps 48, 49 lie behind the last whole day
    total = _state_of(x[:0], zone[:0], nz, steps)
    i64 = C.POINTER(C.c_int64)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        part = _state_of(x[r0:r1], zone[r0:r1], nz, steps)
        assert lib.mcf_series_state_merge(total.ctypes.data_as(i64), part.ctypes.data_as(i64), nz, steps) == 0
    assert np.array_equal(total, _state_of(x, zone, nz, steps))                          # integers: whatever the cut
    want_all = ZR.zone_series(x, zone, nz, steps_done=np.arange(T) < steps)
    want_day0 = ZR.zone_series(x, zone, nz, steps_done=np.arange(T) < 24)
    for k, s in enumerate(ZR.ZSTATS):
        assert np.array_equal(bits(_finish(lib, total, nz, steps, T, None, k)), bits(want_all[s])), s
        assert np.array_equal(bits(_finish(lib, total, nz, steps, T, done, k)), bits(want_day0[s])), s
    # the case is not degenerate: counted and empty zone-steps, a bad one, -0.0 finished as +0.0
    assert want_all["count"][7, 4] == 0 and want_all["count"][0, 0] > 0 and bits(want_all["mean"])[9].tolist().count(ZR.NA_BITS) == 1
    assert lib.mcf_series_state_merge(None, None, nz, steps) == E_ARG and lib.mcf_last_error().startswith(b"mcf_series_state_merge")
    assert lib.mcf_series_state_finish(None, nz, steps, T, None, 0, None) == E_ARG and lib.mcf_last_error().startswith(b"mcf_series_state_finish")
