"""CPU-side checks of the below-ground snow run (include/mcf.h mcf_runmicrosnow1_below, mcf_runmicrosnow1_below_multi,
mcf_snowrun_create_below): declared, exported and bound with their above-ground namesakes' argument lists, the ABI version
unchanged, the Python keyword, the argument checks that run before a device is touched, and no fallback without a device."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import _abi, synthetic
from microclimf_amd import snow as S

ROOT = Path(__file__).resolve().parent.parent
MAT = 7.5


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def _case(reqhgt, rows=6, cols=5, ndays=5):
    T = ndays * 24
    sw = synthetic.snow_workload(rows, cols, T, cold=0.0, zref=3.5, start_doy=90)
    a = synthetic.workload(rows, cols, T, reqhgt=reqhgt, zref=3.5, hgt_range=(0.05, 3.0), start_doy=90, variety=True)
    _, _, dtm = synthetic.rasters(rows, cols)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    return a, snow, micro


def test_entries_are_declared_exported_and_bound_like_their_namesakes():
    hdr = (ROOT / "include" / "mcf.h").read_text()
    for name in ("mcf_runmicrosnow1", "mcf_runmicrosnow1_multi", "mcf_snowrun_create"):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        head, _, tail = name.partition("_multi")
        below = head + "_below" + ("_multi" if _ else "")
        mb = re.search(r"int %s\(([^;]*)\);" % below, hdr)
        assert m and mb, below
        assert re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", mb.group(1)), below       # the same argument list
    assert int(re.search(r"#define MCF_ABI_VERSION (\d+)", hdr).group(1)) == 8
    lib = _lib()
    assert lib.mcf_abi_version() == _abi.ABI_VERSION == 8
    for name, below in (("mcf_runmicrosnow1", "mcf_runmicrosnow1_below"), ("mcf_runmicrosnow1_multi", "mcf_runmicrosnow1_below_multi"),
                        ("mcf_snowrun_create", "mcf_snowrun_create_below")):
        assert below in _abi.EXPORTS
        assert getattr(lib, below).argtypes == getattr(lib, name).argtypes, below
        assert getattr(lib, below).restype is C.c_int


def test_python_keyword_defaults_to_todays_behaviour():
    for fn in (S.SnowRun.__init__, S.runmicrosnow1):
        p = inspect.signature(fn).parameters["below"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_argument_checks_come_before_the_device():
    _lib()
    a, snow, micro = _case(-0.1)
    # as before: the above-ground entries refuse reqhgt < 0 (and now say where to go)
    with pytest.raises(_abi.McfError, match="reqhgt < 0.*mcf_runmicrosnow1_below"):
        S.runmicrosnow1(a, snow, micro, MAT)
    with pytest.raises(_abi.McfError, match="reqhgt < 0"):
        S.SnowRun(a, snow)
    # the below-ground entries refuse reqhgt >= 0
    for rq in (0.0, 0.05):
        with pytest.raises(_abi.McfError, match="need reqhgt < 0"):
            S.runmicrosnow1(dict(a, reqhgt=rq), snow, micro, MAT, below=True)
        with pytest.raises(_abi.McfError, match="need reqhgt < 0"):
            S.SnowRun(dict(a, reqhgt=rq), snow, below=True)
        with pytest.raises(_abi.McfError, match="need reqhgt < 0"):
            S.runmicrosnow1(dict(a, reqhgt=rq), snow, micro, MAT, devices=[0], n_blocks=2, below=True)
    assert _abi.load().mcf_runmicrosnow1_below_multi(None, None, None, None, None) == 1          # MCF_ERR_ARG
    assert b"null" in _abi.load().mcf_last_error()


def test_no_cpu_fallback_without_device():
    lib = _lib()
    if lib.mcf_device_count() > 0:
        pytest.skip("a GPU is present")
    a, snow, micro = _case(-0.1)
    with pytest.raises(_abi.McfError, match="no HIP device"):
        S.runmicrosnow1(a, snow, micro, MAT, below=True)
    with pytest.raises(_abi.McfError, match="no HIP device"):
        S.runmicrosnow1(a, snow, micro, MAT, devices=[0], n_blocks=2, below=True)
    with pytest.raises(_abi.McfError, match="no HIP device"):
        S.SnowRun(a, snow, below=True)
