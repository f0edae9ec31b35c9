"""Series sink, CPU side: the C ABI's new entries exist, refuse bad arguments before a device is needed and have no CPU
fallback; the yardstick (tests/series_ref.py) against exact sums and the NA / bad / empty-zone rules; the front end's
coordinates."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import series_ref as ZR
import stages_cases as SC
from microclimf_amd import _abi, api, frontend

NEW = ("mcf_plan_series_enable", "mcf_plan_series_accumulate", "mcf_plan_series_fetch_points", "mcf_plan_series_fetch_zones",
       "mcf_plan_series_reset", "mcf_runmicro_series", "mcf_zonal_series")
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "complete", "mat")
bits = ZR.bits


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def _args(**over):
    a = dict(SC.build("s170_h005"), **over)
    return [a[k] for k in ARGS]


def test_new_entries_are_declared_exported_and_bound():
    lib = _lib()
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mcf.h").read_text()
    for n in NEW:
        assert n in _abi.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert getattr(lib, n).argtypes is not None, n
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION and "#define MCF_ABI_VERSION 8" in hdr
    body = re.search(r"enum mcf_zstat \{(.*?)\};", hdr, re.S).group(1)
    found = re.findall(r"MCF_ZSTAT_(\w+) = (\d+)", body)
    assert [n.lower() for n, _ in found] == list(_abi.ZSTAT_NAMES) == ["mean", "min", "max", "count"]
    assert [int(i) for _, i in found] == list(range(4)) and "MCF_NZSTAT = 4" in body and _abi.NZSTAT == 4
    assert "#define MCF_MAX_ZONES 64" in hdr and _abi.MAX_ZONES == 64
    assert C.sizeof(_abi.SeriesSpec) == 8 + 8 + 8 + 8 + 40 + 16 and C.sizeof(_abi.SeriesOut) == 80 + 40 * 8
    # the existing structs as they were (LP64)
    assert C.sizeof(_abi.Options) == 6 * 8 + 4 + 40 + 3 * 4 and C.sizeof(_abi.Outputs) == 80
    assert C.sizeof(_abi.SummarySpec) == 4 + 4 + 8 + 40 + 24 + 80 and C.sizeof(_abi.SummaryOut) == 60 * 8 + 8


def test_null_plans_and_arguments_are_refused():
    lib = _lib()
    sp, so = _abi.SeriesSpec(), _abi.SeriesOut()
    buf = np.zeros(8).ctypes.data_as(_abi.c_double_p)
    E = 1   # MCF_ERR_ARG
    assert lib.mcf_plan_series_enable(None, C.byref(sp)) == E and lib.mcf_last_error().startswith(b"mcf_plan_series_enable")
    assert lib.mcf_plan_series_accumulate(None, 0, 0, 0, 1) == E and lib.mcf_last_error().startswith(b"mcf_plan_series_accumulate")
    assert lib.mcf_plan_series_fetch_points(None, 0, buf) == E and lib.mcf_last_error().startswith(b"mcf_plan_series_fetch_points")
    assert lib.mcf_plan_series_fetch_zones(None, 0, 0, buf) == E and lib.mcf_last_error().startswith(b"mcf_plan_series_fetch_zones")
    assert lib.mcf_plan_series_reset(None) == E and lib.mcf_last_error().startswith(b"mcf_plan_series_reset")
    assert lib.mcf_runmicro_series(None, None, None, 0, C.byref(so)) == E and lib.mcf_last_error().startswith(b"mcf_runmicro_series")
    assert lib.mcf_zonal_series(None, 1, 1, 1, None, 1, None, 0, None) == E and lib.mcf_last_error().startswith(b"mcf_zonal_series")


Z0 = np.zeros((SC.ROWS, SC.COLS), dtype=np.int32)


@pytest.mark.parametrize("kw,over,msg", [
    (dict(zones=Z0), dict(reqhgt=-0.05), "reqhgt >= 0"),
    (dict(zones=Z0, vars=()), {}, "no variable selected"),
    (dict(), {}, "neither points nor zones"),
    (dict(zones=Z0, stats=()), {}, "no statistic selected"),
    (dict(zones=Z0, nzones=65), {}, "nzones = 65 is outside"),
    (dict(zones=Z0 + 64), {}, "nzones = 65 is outside"),
    (dict(zones=np.where(np.arange(50).reshape(5, 10) == 7, 3, 0), nzones=3), {}, r"zone\[\d+\] = 3 is outside -1 .. nzones - 1"),
    (dict(points=[0, SC.ROWS * SC.COLS]), {}, r"cells\[1\] = 50 is a cell index outside the raster"),
    (dict(points=[-1]), {}, r"cells\[0\] = -1 is a cell index outside the raster"),
    (dict(zones=Z0, chunk_days=-1), {}, "negative chunk_days"),
], ids=["reqhgt<0", "no-vars", "nothing-selected", "no-stats", "nzones>64", "label>63", "label>=nzones", "cell>=N", "cell<0", "chunk<0"])
def test_refusals_that_need_no_device(kw, over, msg):
    """MCF_ERR_ARG, the message starting with the entry's name, before any device is touched: the same on a host with and
    without one"""
    _lib()
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicro_series: .*" + msg):
        api.runmicro_series(*_args(**over), **kw)


def test_null_buffers_and_too_many_cells_are_refused():
    lib = _lib()
    m = api.marshal(*_args(), [1] + [0] * 9, False)
    sp, _, _ = api.series_spec(SC.ROWS, SC.COLS, [3], Z0, ("Tz",), ("mean", "count"))
    so = _abi.SeriesOut()
    assert lib.mcf_runmicro_series(C.byref(m.inputs), C.byref(m.options), C.byref(sp), 0, C.byref(so)) == 1
    assert re.match(rb"mcf_runmicro_series: .*null point buffer", lib.mcf_last_error())
    keep = api.Buffers()
    so.points[0] = keep.out((96, 1))[1]
    so.zones[0][0] = keep.out((96, 1))[1]
    assert lib.mcf_runmicro_series(C.byref(m.inputs), C.byref(m.options), C.byref(sp), 0, C.byref(so)) == 1
    assert re.match(rb"mcf_runmicro_series: .*\(variable, statistic\) has a null buffer", lib.mcf_last_error())
    # more than 2^26 cells: judged from rows x cols alone, before an array is read
    x = np.zeros(8).ctypes.data_as(_abi.c_double_p)
    zone = np.zeros(8, dtype=np.int32).ctypes.data_as(_abi.c_int32_p)
    zs = (C.c_int32 * 4)(1, 0, 0, 0)
    out = (_abi.c_double_p * 4)(x, None, None, None)
    assert lib.mcf_zonal_series(x, 8193, 8192, 1, zone, 1, zs, 0, out) == 1 and b"2^26" in lib.mcf_last_error()
    m.inputs.rows, m.inputs.cols = 8193, 8192
    assert lib.mcf_runmicro_series(C.byref(m.inputs), C.byref(m.options), C.byref(sp), 0, C.byref(so)) == 1
    assert re.match(rb"mcf_runmicro_series: more than 2\^26 cells", lib.mcf_last_error())
    # mcf_zonal_series: its own refusals
    x3 = np.zeros((2, 4, 3))
    for kw, msg in ((dict(zones=np.zeros((2, 4), int), stats=()), "no statistic selected"),
                    (dict(zones=np.full((2, 4), 64)), "nzones = 65"),
                    (dict(zones=np.full((2, 4), -1), nzones=0), "nzones = 0"),
                    (dict(zones=np.array([[0, 1, 2, 1], [0, 0, 0, 0]]), nzones=2), r"zone\[4\] = 2 is outside")):
        with pytest.raises(_abi.McfError, match="error 1: mcf_zonal_series: .*" + msg):
            api.zonal_series(x3, **kw)
    with pytest.raises(ValueError):
        api.zonal_series(np.zeros((2, 4)), np.zeros((2, 4), int))
    with pytest.raises(ValueError, match="zones: expected shape"):
        api.zonal_series(x3, np.zeros((4, 2), int))


def test_valid_arguments_need_a_device():
    """no CPU fallback: MCF_ERR_NO_DEVICE where there is none (on a GPU host the entries are covered by tests/test_series_gpu.py)"""
    lib = _lib()
    if lib.mcf_device_count() > 0:
        got = api.runmicro_series(*_args(), points=[0, 7], zones=Z0)
        assert got["points"]["Tz"].shape == (96, 2) and got["zones"]["Tz"]["mean"].shape == (96, 1)
        return
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        api.runmicro_series(*_args(), points=[0, 7], zones=Z0, stats=_abi.ZSTAT_NAMES)
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        api.zonal_series(np.zeros((5, 10, 30)), Z0)


def test_series_spec_reads_masked_and_negative_labels_as_no_zone():
    z = np.ma.masked_array(np.arange(50).reshape(5, 10) % 4, mask=False)
    z.mask[1, 2] = True
    z.data[3, 3] = -7
    sp, vi, si = api.series_spec(5, 10, [4, 49], z, ("Tz", "soilm"), ("count",))
    lab = np.ctypeslib.as_array(sp.zone, shape=(50,)).reshape((5, 10), order="F")
    assert sp.nzones == 4 and lab[1, 2] == -1 and lab[3, 3] == -1 and lab[4, 9] == 49 % 4 and (lab >= -1).all()
    assert vi == [0, 3] and si == [3] and sp.npoints == 2 and [sp.cells[0], sp.cells[1]] == [4, 49]
    assert list(sp.var) == [1, 0, 0, 1, 0, 0, 0, 0, 0, 0] and list(sp.zstat) == [0, 0, 0, 1]
    f = np.where(np.arange(50).reshape(5, 10) % 5 == 0, np.nan, 1.0)      # float labels: NaN is no zone
    lab = np.ctypeslib.as_array(api.series_spec(5, 10, None, f)[0].zone, shape=(50,))
    assert set(lab.tolist()) == {-1, 1}
    with pytest.raises(ValueError):
        api.series_spec(5, 10, None, Z0, ("nope",))
    with pytest.raises(ValueError):
        api.series_spec(5, 10, None, Z0, ("Tz",), ("median",))


# ---- the front end's coordinates ----------------------------------------------------------------------------------------------
def test_front_end_maps_xy_to_cells_on_a_5_by_10_raster():
    dtm = {"xmin": 1000.0, "ymax": 250.0, "res": 10.0}      # columns 1000 .. 1100 eastwards, rows 250 .. 200 southwards
    xy = [(1000.0, 250.0), (1005.0, 245.0), (1099.9, 200.1), (1010.0, 240.0), (1034.0, 218.0)]
    assert frontend.series_cells(dtm, 5, 10, xy=xy).tolist() == [0, 0, 4 + 5 * 9, 1 + 5 * 1, 3 + 5 * 3]
    got = frontend.series_cells(dtm, 5, 10, points=[(4, 9), (0, 3)], xy=[(1051.0, 229.0)])
    assert got.dtype == np.int64 and got.tolist() == [49, 15, 2 + 5 * 5]
    assert frontend.series_cells(dict(dtm, res=(10.0, 5.0)), 5, 10, xy=[(1025.0, 231.0)]).tolist() == [3 + 5 * 2]
    for bad in ((999.9, 240.0), (1100.0, 240.0), (1050.0, 250.1), (1050.0, 200.0)):
        with pytest.raises(ValueError, match="outside the raster"):
            frontend.series_cells(dtm, 5, 10, xy=[bad])
    for bad in ((5, 0), (0, 10), (-1, 0)):
        with pytest.raises(ValueError, match="outside"):
            frontend.series_cells(dtm, 5, 10, points=[bad])
    with pytest.raises(ValueError, match="reqhgt >= 0"):
        frontend.runmicro_series({}, -0.05, {}, {}, {})
    with pytest.raises(ValueError, match="vars"):
        frontend.runmicro_series({}, 0.05, {}, {}, {}, vars=("Tz", "nope"))
    with pytest.raises(ValueError, match="stats"):
        frontend.runmicro_series({}, 0.05, {}, {}, {}, stats=("median",))


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def test_yardstick_mean_is_within_half_a_quantum_of_the_exact_mean():
    """each term rint(v 2^24) 2^-24 is within 2^-25 of v, so the mean of the terms is within 2^-25 of the exact mean (the sum
    here stays below 2^53: exact as a double)"""
    rng = np.random.default_rng(11)
    x = (rng.normal(size=(6, 9, 40)) * 25 + 3).copy(order="F")
    zone = (np.arange(54).reshape(6, 9) * 5) % 7 - 1                      # -1 .. 5
    out = ZR.zone_series(x, zone, 6)
    for z in range(6):
        for k in range(40):
            v = x[zone == z][:, k]
            exact = math.fsum(v) / v.size
            assert abs(out["mean"][k, z] - exact) <= 2.0 ** -25, (z, k)
            assert out["min"][k, z] == v.min() and out["max"][k, z] == v.max() and out["count"][k, z] == v.size
    # integer-valued data: exact
    xi = rng.integers(-4000, 4000, size=(6, 9, 24)).astype(np.float64)
    oi = ZR.zone_series(xi, zone, 6)
    for z in range(6):
        v = xi[zone == z]
        assert (oi["mean"][:, z] == v.sum(axis=0) / v.shape[0]).all()


def test_yardstick_rules():
    q = ZR.QUANTUM
    x = np.zeros((2, 4, 8), order="F")
    zone = np.array([[0, 0, 1, 2], [0, 0, 1, -1]])
    na = ZR.na_real()
    # step 0: NaN and NA are skipped (na.rm = TRUE)
    x[0, 0, 0], x[0, 1, 0], x[1, 1, 0] = 1.0, np.nan, 4.0
    x[1, 0, 0] = na
    # step 1: a zone-step without a counted value: count 0, the rest NA; the cell in no zone is ignored
    x[:, 2, 1] = np.nan
    x[1, 3, 1] = np.inf
    # step 2: bad values: 4096, -4096 and inf each take their zone-step; 4096 - 2^-24 is counted
    x[0, 0, 2], x[0, 2, 2], x[0, 3, 2] = 4096.0, -np.inf, 4096.0 - q
    # step 3: -4096 is bad as well
    x[1, 2, 3] = -4096.0
    # step 4: -0.0 alone: minimum and maximum +0.0
    x[0, 3, 4] = -0.0
    # steps 5, 6: half-quantum ties go to the even neighbour, both parities and both signs
    x[0, 3, 5], x[0, 3, 6] = (6 + 0.5) * q, (7 + 0.5) * q
    x[:, 2, 5], x[:, 2, 6] = (-6 - 0.5) * q, (-7 - 0.5) * q
    out = ZR.zone_series(x, zone, 3)
    NA = ZR.NA_BITS
    assert out["count"][0].tolist() == [2.0, 2.0, 1.0] and out["mean"][0, 0] == 2.5 and out["min"][0, 0] == 1.0 and out["max"][0, 0] == 4.0
    assert out["count"][1, 1] == 0.0 and all(bits(out[k])[1, 1] == NA for k in ("mean", "min", "max")) and out["mean"][1, 2] == 0.0
    assert out["count"][2].tolist() == [3.0, 1.0, 1.0]
    for z in (0, 1):
        assert all(bits(out[k])[2, z] == NA for k in ("mean", "min", "max")), z
    assert out["max"][2, 2] == 4096.0 - q == out["mean"][2, 2]
    assert out["count"][3, 1] == 1.0 and bits(out["mean"])[3, 1] == NA and out["mean"][3, 0] == 0.0
    for k in ("mean", "min", "max"):
        assert out[k][4, 2] == 0.0 and not np.signbit(out[k][4, 2]), k
    assert out["mean"][5, 2] == 6 * q and out["mean"][6, 2] == 8 * q and out["min"][5, 2] == 6.5 * q
    assert out["mean"][5, 1] == -6 * q and out["mean"][6, 1] == -8 * q and out["count"][5, 1] == 2.0
    # steps that were never folded are NA in every statistic, the count included
    part = ZR.zone_series(x, zone, 3, steps_done=np.arange(8) < 4)
    for k in ZR.ZSTATS:
        assert (bits(part[k])[4:] == NA).all() and np.array_equal(bits(part[k])[:4], bits(out[k])[:4]), k
    # the points keep the array's bits, the NA payload included
    pts = ZR.point_series(x, [0, 1, 2, 6])
    assert pts.shape == (8, 4) and bits(pts)[0, 1] == NA and np.isnan(pts[0, 2]) and bits(pts)[0, 2] != NA and pts[2, 3] == 4096.0 - q
