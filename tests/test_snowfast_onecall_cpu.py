"""The fast snow method as one device-resident call (include/mcf.h mcf_snowmodelq1, mcf_canintfrac_device, mcf_meltmu_device):
what can be checked without a device — the entries exist in the header, the library and the binding at ABI version 8, every
argument refusal comes before a device is looked for and names its cause, and `runsnowmodel(one_call=True)` refuses what is
not the fast method of a subset run."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import _abi
from microclimf_amd import frontend as F
from microclimf_amd import snow as S

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("mcf_snowmodelq1", "mcf_canintfrac_device", "mcf_meltmu_device")
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
    assert "typedef struct mcf_snowfast_in" in header
    assert [f[0] for f in _abi.SnowFastIn._fields_] == ["drv", "n_all", "subs", *_abi.SNOWFAST_SERIES]
    assert C.sizeof(_abi.SnowFastIn) == C.sizeof(_abi.SnowDriverIn) + 8 + 8 + 8 * 8


def test_abi_version_stays_8(lib):
    header = (ROOT / "include" / "mcf.h").read_text()
    assert re.search(r"^#define MCF_ABI_VERSION 8\b", header, re.M)
    assert lib.mcf_abi_version() == 8 and _abi.ABI_VERSION == 8


R, CC, N_ALL = 6, 7, 5 * 24


def _args(subs=None, n=None):
    """plausible inputs: 5 days of hourly weather, the third and the fifth day selected"""
    rng = np.random.default_rng(11)
    subs = np.r_[49:73, 97:121] if subs is None else np.asarray(subs)
    n = subs.size if n is None else n
    hours = np.arange(n)
    obstime = {"year": np.full(n, 2019), "month": np.full(n, 1), "day": 1 + hours // 24, "hour": (hours % 24).astype(float)}
    clim = {"temp": np.full(n, -4.0), "relhum": np.full(n, 80.0), "pres": np.full(n, 100.0), "swdown": np.full(n, 50.0),
            "difrad": np.full(n, 30.0), "lwdown": np.full(n, 250.0), "windspeed": np.full(n, 4.0), "winddir": np.full(n, 200.0),
            "precip": np.full(n, 0.2)}
    pointm = {"Gp": np.zeros(n), "Tc": np.full(n, -5.0), "RswabsG": np.full(n, 20.0), "RlwabsG": np.full(n, 240.0),
              "umu": np.full(n, 0.8), "tr": np.full(n, 0.5)}
    pmod = {"sublmelt": np.full(N_ALL, 1e-6), "tempmelt": np.full(N_ALL, 1e-5), "rainmelt": np.zeros(N_ALL),
            "sstemp": rng.normal(-1.0, 2.0, N_ALL), "sdenc": np.full(N_ALL, 250.0), "sdeng": np.full(N_ALL, 260.0)}
    temp_all = rng.normal(-4.0, 2.0, N_ALL)
    vegp = {"pai": np.full((R, CC), 1.0), "hgt": np.full((R, CC), 0.5), "leaft": np.full((R, CC), 0.01), "clump": np.full((R, CC), 0.1)}
    r, c = np.meshgrid(np.arange(R), np.arange(CC), indexing="ij")
    other = {"zref": 2.0, "lat": 50.0, "lon": -5.0, "isnowdc": np.zeros((R, CC)), "isnowac": np.zeros((R, CC)), "isnowag": np.zeros((R, CC))}
    return (obstime, clim, pointm, pmod, temp_all, np.full(N_ALL, 0.2), subs, vegp, other, "Taiga", 100.0 + 2.0 * r + c, 10.0, 0.01)


def _status(lib, fin, out=None):
    if out is None:
        out = _abi.SnowDriverOut()
    rc = lib.mcf_snowmodelq1(C.byref(fin), C.byref(out), 0)
    return rc, (lib.mcf_last_error() or b"").decode()


def test_plausible_inputs_pass_the_argument_checks(lib):
    m, fin = S.marshal_snowfast(*_args())
    rc, msg = _status(lib, fin)
    assert rc != MCF_ERR_ARG, msg                            # no device here: MCF_ERR_NO_DEVICE; with one: the call runs


def test_null_arguments_are_refused(lib):
    out = _abi.SnowDriverOut()
    assert lib.mcf_snowmodelq1(None, C.byref(out), 0) == MCF_ERR_ARG and b"null" in lib.mcf_last_error()
    m, fin = S.marshal_snowfast(*_args())
    assert lib.mcf_snowmodelq1(C.byref(fin), None, 0) == MCF_ERR_ARG and b"null" in lib.mcf_last_error()
    for field, name in (("subs", "subs"), ("sstemp", "sstemp"), ("sdeng", "sdeng"), ("snow_all", "snow_all"), ("temp_all", "temp_all")):
        m, fin = S.marshal_snowfast(*_args())
        setattr(fin, field, None)
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "null" in msg and name in msg, (field, rc, msg)
    for where, field, name in (("drv", "dtm", "dtm"), ("clim", "windspeed", "windspeed"), ("pointm", "Gp", "Gp"), ("vegp", "hgt", "hgt"),
                               ("other", "isnowdc", "isnowdc"), ("other", "isnowag", "isnowag"), ("obstime", "hour", "obstime")):
        m, fin = S.marshal_snowfast(*_args())
        setattr(fin.drv if where == "drv" else getattr(fin.drv.base, where), field, None)
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "null" in msg and name in msg, (where, field, rc, msg)
    m, fin = S.marshal_snowfast(*_args())                    # what the entry ignores may be null: isnowdg and the terrain are
    assert not fin.drv.base.other.isnowdg and not fin.drv.base.other.hor


def test_broken_days_are_refused(lib):
    m, fin = S.marshal_snowfast(*_args())
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
        m, fin = S.marshal_snowfast(*_args(subs=bad))
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and word in msg and "subs" in msg, (bad, rc, msg)


def test_array_forcing_is_refused(lib):
    m, fin = S.marshal_snowfast(*_args())
    fin.drv.base.array_forcing = 1
    rc, msg = _status(lib, fin)
    assert rc == MCF_ERR_ARG and "array_forcing" in msg, (rc, msg)


def test_a_first_selected_day_that_is_the_first_day_is_refused(lib):
    for first in (np.r_[1:25], np.r_[2:26]):                 # subs[0] - 1 <= 1
        m, fin = S.marshal_snowfast(*_args(subs=np.r_[first, 97:121]))
        rc, msg = _status(lib, fin)
        assert rc == MCF_ERR_ARG and "cannot start on the first day" in msg, (rc, msg)
    with pytest.raises(_abi.McfError, match="first day"):
        S.snowmodelq1(*_args(subs=np.r_[1:25, 97:121]))


def test_an_aggregation_factor_of_zero_is_refused(lib):
    a = list(_args())
    a[1] = dict(a[1], windspeed=np.full(48, 0.1))            # round(10 sqrt(0.1) / 10) = 0
    m, fin = S.marshal_snowfast(*a)
    rc, msg = _status(lib, fin)
    assert rc == MCF_ERR_ARG and "aggregation factor" in msg, (rc, msg)


def test_the_eviction_inputs_walk_the_aggregation_factors_past_the_cache(oracle, lib):
    """The ten-day inputs of the one-call GPU tests (snowfast_cases.loop_args) give, rounded as the library rounds, the factors
    2 .. 10 and 2 again: nine distinct ones for eight slots — for mcf_snowmodelq1 from the selected hours' wind speed, for
    mcf_snowmodelq2 from the `af_wind` that marshal_snowfast2 hands the library."""
    import snowfast_cases as FC
    want = [2, 3, 4, 5, 6, 7, 8, 9, 10, 2]
    assert FC.AF_DAYS == want and len(set(want)) == 9 > 8
    args, _ = FC.loop_args("q1", FC.TEN_DAYS)
    assert FC.library_af(args[1]["windspeed"], args[11]) == want
    assert max(want) < min(np.shape(args[10])) / 2                    # `.tpicalc` aggregates for every one of them
    args, pos = FC.loop_args("q2", FC.TEN_DAYS)
    m, fin = S.marshal_snowfast2(*args, **pos)
    af_wind = np.ctypeslib.as_array(fin.drv.af_wind, shape=(m.tsteps,))
    assert m.tsteps == 240 and FC.library_af(af_wind, args[10]) == want
    assert max(want) < min(np.shape(args[8])) / 2


def test_one_shot_kernel_entries_refuse_null_arguments(lib):
    x = np.ones(4)
    p = x.ctypes.data_as(_abi.c_double_p)
    assert lib.mcf_canintfrac_device(4, p, None, 2.0, 1.0, -3.0, 0.0, p, 0) == MCF_ERR_ARG
    assert lib.mcf_canintfrac_device(0, p, p, 2.0, 1.0, -3.0, 0.0, p, 0) == MCF_ERR_ARG
    assert lib.mcf_meltmu_device(4, p, 4, None, p, p, 0) == MCF_ERR_ARG
    assert lib.mcf_meltmu_device(4, None, 0, None, None, p, 0) == MCF_ERR_ARG


def test_one_call_is_the_fast_method_of_a_subset_run():
    complete = {"subs": np.arange(1, 49), "ntme": 48}
    subset = {"subs": np.arange(25, 49), "ntme": 96}
    with pytest.raises(ValueError, match="one_call"):
        F.runsnowmodel({}, complete, {}, {}, {}, one_call=True)
    with pytest.raises(ValueError, match="one_call"):
        F.runsnowmodel({}, subset, {}, {}, {}, method="slow", one_call=True)
