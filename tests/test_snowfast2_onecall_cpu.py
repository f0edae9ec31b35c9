"""The fast snow method for array weather as one device-resident call (include/mcf.h mcf_snowmodelq2, mcf_meltmu2_device):
what can be checked without a device — the entries exist in the header, the library and the binding at ABI version 8,
mcf_snowfast_in keeps its layout, every argument refusal comes before a device is looked for and names its cause, a first
selected day that is the series' first day is accepted, and `runsnowmodela(one_call=True)` refuses what is not the fast
method of subset micropoints."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import _abi
from microclimf_amd import frontend as F
from microclimf_amd import snow as S

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("mcf_snowmodelq2", "mcf_meltmu2_device")
MCF_ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def test_entries_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "mcf.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _abi.EXPORTS
        fn = getattr(lib, name)                              # AttributeError: the library does not export it
        assert fn.argtypes and fn.argtypes[-1] is C.c_int32 and fn.restype is C.c_int, name
    assert "typedef struct mcf_snowfast2_in" in header and "typedef struct mcf_snowfast2_out" in header
    assert [f[0] for f in _abi.SnowFast2In._fields_] == ["drv", "coarse_rows", "coarse_cols", "coarse_rowpos", "coarse_colpos", "altcorrect",
                                                         "reserved", "coarse_dtm", *_abi.SNOWFAST2_SELECTED, "n_all", "subs",
                                                         *_abi.SNOWFAST2_SERIES]
    assert C.sizeof(_abi.SnowFast2In) == C.sizeof(_abi.SnowDriverIn) + 8 * (2 + 2 + 1 + 1 + 14 + 2 + 8)
    assert [f[0] for f in _abi.SnowFast2Out._fields_] == [*_abi.SNOWDRIVER_OUT, "umu"]
    assert C.sizeof(_abi.SnowFast2Out) == C.sizeof(_abi.SnowDriverOut) + 8


def test_abi_version_stays_8_and_snowfast_in_keeps_its_layout(lib):
    header = (ROOT / "include" / "mcf.h").read_text()
    assert re.search(r"^#define MCF_ABI_VERSION 8\b", header, re.M)
    assert lib.mcf_abi_version() == 8 and _abi.ABI_VERSION == 8
    assert [f[0] for f in _abi.SnowFastIn._fields_] == ["drv", "n_all", "subs", "sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc",
                                                        "sdeng", "temp_all", "snow_all"]
    assert C.sizeof(_abi.SnowFastIn) == C.sizeof(_abi.SnowDriverIn) + 8 + 8 + 8 * 8


R, CC, CR, CCC, N_ALL = 6, 7, 2, 3, 5 * 24


def _args(subs=None, altcorrect=0, wind=4.0):
    """plausible inputs: 5 days of hourly weather over a 2 x 3 climate grid, the third and the fifth day selected"""
    from microclimf_amd import api
    rng = np.random.default_rng(11)
    subs = np.r_[49:73, 97:121] if subs is None else np.asarray(subs)
    n = subs.size
    hours = np.arange(n)
    full = lambda v, t=n: np.full((CR, CCC, t), v)           # noqa: E731
    obstime = {"year": np.full(n, 2019), "month": np.full(n, 1), "day": 1 + hours // 24, "hour": (hours % 24).astype(float)}
    clim = {"temp": full(-4.0), "relhum": full(80.0), "pres": full(100.0), "swdown": full(50.0), "difrad": full(30.0),
            "lwdown": full(250.0), "windspeed": full(wind), "winddir": np.full(n, 200.0), "precip": full(0.2)}
    pointm = {"Gp": full(0.0), "Tc": full(-5.0), "RswabsG": full(20.0), "RlwabsG": full(240.0), "umu": full(0.8), "tr": full(0.5)}
    pm2 = {"sublmelt": full(1e-6, N_ALL), "tempmelt": full(1e-5, N_ALL), "rainmelt": full(0.0, N_ALL), "snow": full(0.2, N_ALL),
           "sstemp": rng.normal(-1.0, 2.0, (CR, CCC, N_ALL)), "tc": rng.normal(-4.0, 2.0, (CR, CCC, N_ALL)),
           "sdenc": full(250.0, N_ALL), "sdeng": full(260.0, N_ALL)}
    vegp = {"pai": np.full((R, CC), 1.0), "hgt": np.full((R, CC), 0.5), "leaft": np.full((R, CC), 0.01), "clump": np.full((R, CC), 0.1)}
    r, c = np.meshgrid(np.arange(R), np.arange(CC), indexing="ij")
    other = {"zref": 2.0, "lats": np.full((R, CC), 50.0), "lons": np.full((R, CC), -5.0), "isnowdc": np.zeros((R, CC)),
             "isnowac": np.zeros((R, CC)), "isnowag": np.zeros((R, CC))}
    return (obstime, clim, pointm, pm2, subs, vegp, other, "Taiga", 100.0 + 2.0 * r + c, np.full((CR, CCC), 110.0), 10.0, 0.01,
            api.coarse_positions(R, CR), api.coarse_positions(CC, CCC), altcorrect)


def _status(lib, fin, out=None):
    if out is None:
        out = _abi.SnowFast2Out()
    rc = lib.mcf_snowmodelq2(C.byref(fin), C.byref(out), 0)
    return rc, (lib.mcf_last_error() or b"").decode()


@pytest.mark.parametrize("altcorrect", [0, 1, 2])
def test_plausible_inputs_pass_the_argument_checks(lib, altcorrect):
    m, fin = S.marshal_snowfast2(*_args(altcorrect=altcorrect))
    rc, msg = _status(lib, fin)
    assert rc != MCF_ERR_ARG, msg                            # no device here: MCF_ERR_NO_DEVICE; with one: the call runs


def test_a_first_selected_day_that_is_the_first_day_is_accepted(lib):
    for first in (np.r_[1:25], np.r_[2:26]):                 # subs[0] - 1 <= 1: refused by mcf_snowmodelq1, no adjustment here
        m, fin = S.marshal_snowfast2(*_args(subs=np.r_[first, 97:121]))
        rc, msg = _status(lib, fin)
        assert rc != MCF_ERR_ARG, msg


def test_null_arguments_are_refused(lib):
    out = _abi.SnowFast2Out()
    assert lib.mcf_snowmodelq2(None, C.byref(out), 0) == MCF_ERR_ARG and b"null" in lib.mcf_last_error()
    m, fin = S.marshal_snowfast2(*_args())
    assert lib.mcf_snowmodelq2(C.byref(fin), None, 0) == MCF_ERR_ARG and b"null" in lib.mcf_last_error()
    for field in ("subs", "coarse_rowpos", "coarse_colpos", *_abi.SNOWFAST2_SELECTED, *_abi.SNOWFAST2_SERIES):
        m, fin = S.marshal_snowfast2(*_args())
        setattr(fin, field, None)
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "null" in msg and field in msg, (field, rc, msg)
    for where, field, name in (("drv", "dtm", "dtm"), ("drv", "af_wind", "af_wind"), ("clim", "winddir", "winddir"), ("vegp", "hgt", "hgt"),
                               ("other", "isnowdc", "isnowdc"), ("other", "isnowag", "isnowag"), ("other", "lats", "lats"),
                               ("other", "lons", "lons"), ("obstime", "hour", "obstime")):
        m, fin = S.marshal_snowfast2(*_args())
        setattr(fin.drv if where == "drv" else getattr(fin.drv.base, where), field, None)
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "null" in msg and name in msg, (where, field, rc, msg)
    m, fin = S.marshal_snowfast2(*_args())                   # what the entry ignores may be null: the raster-sized weather, the terrain
    assert not fin.drv.base.clim.temp and not fin.drv.base.pointm.Gp and not fin.drv.base.other.hor and not fin.drv.base.other.isnowdg


def test_broken_days_are_refused(lib):
    m, fin = S.marshal_snowfast2(*_args())
    for n in (0, 23, 25, 47):
        fin.drv.base.tsteps = n
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "whole selected days" in msg, (n, rc, msg)


def test_subs_out_of_range_or_order_are_refused(lib):
    good = np.r_[49:73, 97:121]
    for bad, word in ((np.r_[49:73, 98:122], "outside"), (np.r_[np.zeros(1, dtype=int), 50:73, 97:121], "outside"),
                      (np.r_[49:73, 97:119, 120, 119], "not increasing"), (np.r_[49:73, 97:120, 119], "not increasing"),
                      (np.r_[97:121, 49:73], "not increasing")):
        assert bad.size == good.size
        m, fin = S.marshal_snowfast2(*_args(subs=bad))
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and word in msg and "subs" in msg, (bad, rc, msg)
    with pytest.raises(_abi.McfError, match="outside"):
        S.snowmodelq2(*_args(subs=np.r_[49:73, 98:122])[:12], rowpos=_args()[12], colpos=_args()[13])


def test_a_bad_coarse_grid_is_refused(lib):
    for field in ("coarse_rows", "coarse_cols"):
        for v in (0, -1):
            m, fin = S.marshal_snowfast2(*_args())
            setattr(fin, field, v)
            rc, msg = _status(lib, fin)
            assert rc == MCF_ERR_ARG and "coarse_rows" in msg, (field, v, rc, msg)
    m, fin = S.marshal_snowfast2(*_args())                   # 24 x coarse cells x 8 B = 2^32 (checked before any array is read)
    fin.coarse_rows, fin.coarse_cols = 4096, 5462
    rc, msg = _status(lib, fin)
    assert rc == MCF_ERR_ARG and "2^32" in msg, (rc, msg)


def test_positions_outside_the_coarse_grid_are_refused(lib):
    a = _args()
    for k, bad in ((12, 2.0), (12, -0.25), (12, float("nan")), (13, 2.5), (13, -1.0)):      # 2 coarse rows, 3 coarse columns
        b = list(a)
        b[k] = np.array(a[k], copy=True)
        b[k][-1] = bad
        m, fin = S.marshal_snowfast2(*b)
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "coarse_rowpos" in msg, (k, bad, rc, msg)
    x = np.ones(4)
    p = x.ctypes.data_as(_abi.c_double_p)                    # position 1 in a grid of one coarse row
    assert lib.mcf_meltmu2_device(2, 2, p, p, 1, 1, p, p, 0, None, None, p, 0) == MCF_ERR_ARG and b"rowpos" in lib.mcf_last_error()


def test_a_bad_altcorrect_is_refused(lib):
    for v in (-1, 3):
        m, fin = S.marshal_snowfast2(*_args())
        fin.altcorrect = v
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "altcorrect" in msg, (v, rc, msg)
    for v in (1, 2):
        m, fin = S.marshal_snowfast2(*_args(altcorrect=v))
        fin.coarse_dtm = None
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "altcorrect" in msg and "coarse_dtm" in msg, (v, rc, msg)
    m, fin = S.marshal_snowfast2(*_args())                   # not read without the correction
    fin.coarse_dtm = None
    assert _status(lib, fin)[0] != MCF_ERR_ARG


def test_an_aggregation_factor_of_zero_is_refused(lib):
    m, fin = S.marshal_snowfast2(*_args(wind=0.1))           # round(10 sqrt(0.1) / 10) = 0
    rc, msg = _status(lib, fin)
    assert rc == MCF_ERR_ARG and "aggregation factor" in msg, (rc, msg)


def test_the_data_frame_entry_still_refuses_array_forcing(lib):
    import test_snowfast_onecall_cpu as Q1
    m, fin = S.marshal_snowfast(*Q1._args())
    fin.drv.base.array_forcing = 1
    rc = lib.mcf_snowmodelq1(C.byref(fin), C.byref(_abi.SnowDriverOut()), 0)
    msg = (lib.mcf_last_error() or b"").decode()
    assert rc == MCF_ERR_ARG and "array_forcing" in msg and "mcf_snowmodelq2" in msg, (rc, msg)


def test_the_gap_kernel_entry_refuses_null_arguments(lib):
    x = np.ones(4)
    p = x.ctypes.data_as(_abi.c_double_p)
    assert lib.mcf_meltmu2_device(2, 2, p, p, 1, 1, p, p, 4, None, p, p, 0) == MCF_ERR_ARG
    assert lib.mcf_meltmu2_device(2, 2, None, p, 1, 1, p, p, 0, None, None, p, 0) == MCF_ERR_ARG
    assert lib.mcf_meltmu2_device(2, 2, p, p, 0, 1, p, p, 0, None, None, p, 0) == MCF_ERR_ARG
    assert lib.mcf_meltmu2_device(2, 2, p, p, 1, 1, p, None, 0, None, None, p, 0) == MCF_ERR_ARG
    assert lib.mcf_meltmu2_device(0, 2, p, p, 1, 1, p, p, 0, None, None, p, 0) == MCF_ERR_ARG


def test_one_call_is_the_fast_method_of_subset_micropoints():
    complete = {"subs": np.arange(1, 49), "ntme": 48}
    subset = {"subs": np.arange(25, 49), "ntme": 96}
    kw = dict(dtmc=None, lats_c=None, lons_c=None, lats=None, lons=None)
    with pytest.raises(ValueError, match="one_call"):
        F.runsnowmodela({}, {}, [complete, complete], {}, {}, {}, one_call=True, **kw)
    with pytest.raises(ValueError, match="one_call"):
        F.runsnowmodela({}, {}, [subset, subset], {}, {}, {}, method="slow", one_call=True, **kw)
