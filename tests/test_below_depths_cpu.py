"""Below ground at several depths, CPU side: the new entries exist, check their arguments before a device is needed — each
refusal with its sentence, which starts with the entry's name — and have no CPU fallback."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import _abi, api, frontend, synthetic

NEW = ("mcf_plan_below_set_depths", "mcf_plan_fetch_depth", "mcf_plan_fetch_depth_pitched", "mcf_plan_summary_enable_below",
       "mcf_plan_summary_fetch_depth", "mcf_runmicro_depths", "mcf_runmicro_depths_summary")
T = 24 * 3 + 5
E_ARG = 1


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def _args(**kw):
    a = synthetic.workload(5, 4, T, reqhgt=-0.1, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0], **kw)
    a.pop("reqhgt")
    a.pop("out")
    return a


def test_new_entries_are_declared_exported_and_bound():
    lib = _lib()
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mcf.h").read_text()
    for n in NEW:
        assert n in _abi.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert getattr(lib, n).argtypes is not None, n
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION and "#define MCF_ABI_VERSION 8" in hdr
    assert "#define MCF_MAX_DEPTHS 8" in hdr and _abi.MAX_DEPTHS == 8
    assert C.sizeof(_abi.DepthOutputs) == 9 * 8 and C.sizeof(_abi.DepthSummaryOut) == (8 * 6 + 6 + 1) * 8
    for m in ("below_set_depths", "fetch_depth", "summary_enable_below", "fetch_summary_depth"):
        assert callable(getattr(api.Plan, m)), m


def test_null_plans_and_arguments_are_refused():
    lib = _lib()
    d = np.array([-0.1, -0.2])
    buf = np.zeros(8)
    P = _abi.c_double_p
    sp = _abi.SummarySpec()
    assert lib.mcf_plan_below_set_depths(None, d.ctypes.data_as(P), 2, None) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_plan_below_set_depths: null plan")
    assert lib.mcf_plan_fetch_depth(None, 0, 0, 0, 1, buf.ctypes.data_as(P)) == E_ARG
    assert lib.mcf_plan_fetch_depth_pitched(None, 0, 0, 0, 1, buf.ctypes.data_as(P), 0) == E_ARG
    assert lib.mcf_plan_summary_enable_below(None, C.byref(sp)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_plan_summary_enable_below: null")
    assert lib.mcf_plan_summary_fetch_depth(None, 0, 0, 0, buf.ctypes.data_as(P)) == E_ARG
    do, so = _abi.DepthOutputs(), _abi.DepthSummaryOut()
    assert lib.mcf_runmicro_depths(None, None, d.ctypes.data_as(P), 2, None, C.byref(do)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_depths: null")
    assert lib.mcf_runmicro_depths_summary(None, None, d.ctypes.data_as(P), 2, None, C.byref(sp), 0, C.byref(so)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_depths_summary: null")
    assert lib.mcf_runmicro_depths_summary(None, None, d.ctypes.data_as(P), 2, None, None, 0, C.byref(so)) == E_ARG


LIST_REFUSALS = [
    (dict(depths=[]), {}, "a null or empty depth list"),
    (dict(depths=[-0.1] * 9), {}, "9 depths, at most MCF_MAX_DEPTHS = 8"),
    (dict(depths=[-0.1, 0.0]), {}, r"depths\[1\] is not below ground"),
    (dict(depths=[0.05]), {}, r"depths\[0\] is not below ground"),
    (dict(depths=[-0.1, -0.3, float("nan")]), {}, r"depths\[2\] is not below ground"),
    (dict(depths=[-0.1, -0.2]), dict(complete=False), "complete = 0 needs tbp"),
    (dict(depths=[-0.1, -0.2], tbp=np.zeros((2, T)), array_forcing=True), dict(complete=False, array_forcing=True),
     "array forcing with complete = 0 is not taken"),
]
IDS = ["empty", "too-long", "zero", "above-ground", "nan", "no-tbp", "array-forcing-complete-0"]


@pytest.mark.parametrize("kw,over,msg", LIST_REFUSALS, ids=IDS)
def test_depth_list_refusals_need_no_device(kw, over, msg):
    """MCF_ERR_ARG, the sentence led by the entry's name, before any device is touched: the same with and without one"""
    _lib()
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicro_depths: " + msg):
        api.runmicro_depths(**_args(**over), **kw)
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicro_depths_summary: " + msg):
        api.runmicro_depths_summary(**_args(**over), **kw, periods=[0, 0, 1])


@pytest.mark.parametrize("kw,msg", [
    (dict(periods=[0, 0, 1], vars=("Tz", "tleaf")), "mcf_runmicro_depths_summary: below ground Tz and soilm can be summarised"),
    (dict(periods=[0, 0, 1], vars=()), "no variable selected"),
    (dict(periods=[0, 0, 1], stats=()), "no statistic selected"),
    (dict(periods=[0, 0, 1], nperiods=0), "nperiods must be at least 1"),
    (dict(periods=[0, 3, 1], nperiods=2), r"period_of_day\[1\] = 3 is outside"),
    (dict(periods=[0, 0, 1], stats=("hours_above",)), "HOURS_ABOVE needs a threshold"),
    (dict(periods=[0, 0, 1], chunk_days=-1), "mcf_runmicro_depths_summary: negative chunk_days"),
], ids=["other-variable", "no-vars", "no-stats", "nperiods<1", "entry-too-large", "nan-threshold", "chunk<0"])
def test_summary_refusals_need_no_device(kw, msg):
    _lib()
    with pytest.raises(_abi.McfError, match=r"error 1: .*" + msg):
        api.runmicro_depths_summary(**_args(), depths=[-0.1, -0.4], **kw)


def test_a_series_shorter_than_a_day_and_a_misshapen_tbp():
    _lib()
    a = synthetic.workload(5, 4, 20, reqhgt=-0.1)
    a.pop("reqhgt")
    a.pop("out")
    with pytest.raises(_abi.McfError, match="error 1: mcf_runmicro_depths: the series is shorter than a day"):
        api.runmicro_depths(**a, depths=[-0.1])
    with pytest.raises(ValueError, match="tbp: expected shape"):
        api.runmicro_depths(**_args(complete=False), depths=[-0.1, -0.2], tbp=np.zeros((3, T)))


def test_valid_arguments_need_a_device():
    """no CPU fallback: MCF_ERR_NO_DEVICE where there is none (on a GPU host tests/test_below_depths_gpu.py covers the entries)"""
    lib = _lib()
    depths = [-0.05, -0.3]
    if lib.mcf_device_count() > 0:
        got = api.runmicro_depths(**_args(), depths=depths)
        assert len(got["Tz"]) == 2 and got["Tz"][1].shape == (5, 4, T)
        return
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        api.runmicro_depths(**_args(), depths=depths)
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        api.runmicro_depths(**_args(complete=False), depths=depths, tbp=np.zeros((2, T)))
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        api.runmicro_depths_summary(**_args(), depths=depths, periods=[0, 0, 1], vars=("Tz", "soilm"), stats=_abi.STAT_NAMES,
                                    thresholds=9.0)


def test_front_end_names():
    with pytest.raises(ValueError, match="vars"):
        frontend.runmicro_depths_summary({}, [-0.1], {}, {}, {}, vars=("Tz", "nope"))
    with pytest.raises(ValueError, match="runmicro_depths_summary"):       # the above-ground entry names the new one
        frontend.runmicro_summary({}, -0.05, {}, {}, {})
    with pytest.raises(ValueError, match="depths"):
        frontend.runmicro_depths({"dfo": {}}, [-0.1, 0.2], {}, {}, {})
