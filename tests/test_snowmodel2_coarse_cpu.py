"""The slow snow method for array weather as one device-resident call with the coarse arrays left coarse (include/mcf.h
mcf_snowmodel2_coarse, mcf_snow_expand_coarse_device): what can be checked without a device — the entries exist in the header,
the library and the binding at ABI version 8, every argument refusal comes before a device is looked for and names the entry
and its cause, plausible arguments pass the checks, and `runsnowmodela(device_loop=True)` refuses the fast method while
`one_call=True` goes on refusing the slow one."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import _abi
from microclimf_amd import frontend as F
from microclimf_amd import snow as S

ROOT = Path(__file__).resolve().parent.parent
MODEL, EXPAND = "mcf_snowmodel2_coarse", "mcf_snow_expand_coarse_device"
MCF_ERR_ARG = 1
R, CC, CR, CCC, T = 6, 7, 2, 3, 6 * 24


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def test_entries_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "mcf.h").read_text()
    for name in (MODEL, EXPAND):
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _abi.EXPORTS
        fn = getattr(lib, name)                              # AttributeError: the library does not export it
        assert fn.argtypes and fn.argtypes[-1] is C.c_int32 and fn.restype is C.c_int, name
        assert re.search(rf"added since, functions only:[^)]*\b{name}\b", header, re.S), name
    assert re.search(r"^#define MCF_ABI_VERSION 8\b", header, re.M) and lib.mcf_abi_version() == 8 and _abi.ABI_VERSION == 8
    assert "typedef struct mcf_snowcoarse_in" in header
    assert [f[0] for f in _abi.SnowCoarseIn._fields_] == ["drv", "coarse_rows", "coarse_cols", "coarse_rowpos", "coarse_colpos", "altcorrect",
                                                          "reserved", "coarse_dtm", *_abi.SNOWFAST2_SELECTED]
    assert C.sizeof(_abi.SnowCoarseIn) == C.sizeof(_abi.SnowDriverIn) + 8 * (2 + 2 + 1 + 1 + 14)
    # the leading members are mcf_snowfast2_in's: the two structs share the kernel's argument listing
    for a, b in zip(_abi.SnowCoarseIn._fields_, _abi.SnowFast2In._fields_):
        assert a[0] == b[0] and getattr(_abi.SnowCoarseIn, a[0]).offset == getattr(_abi.SnowFast2In, a[0]).offset


def _args(altcorrect=0, chunk_steps=120):
    """plausible inputs: 6 days of hourly weather over a 2 x 3 climate grid"""
    from microclimf_amd import api
    hours = np.arange(T)
    full = lambda v: np.full((CR, CCC, T), v)                # noqa: E731
    obstime = {"year": np.full(T, 2019), "month": np.full(T, 1), "day": 1 + hours // 24, "hour": (hours % 24).astype(float)}
    clim = {"temp": full(-4.0), "relhum": full(80.0), "pres": full(100.0), "swdown": full(50.0), "difrad": full(30.0),
            "lwdown": full(250.0), "windspeed": full(4.0), "winddir": np.full(T, 200.0), "precip": full(0.2)}
    pointm = {"Gp": full(0.0), "Tc": full(-5.0), "RswabsG": full(20.0), "RlwabsG": full(240.0), "umu": full(0.8), "tr": full(0.5)}
    vegp = {"pai": np.full((R, CC), 1.0), "hgt": np.full((R, CC), 0.5), "leaft": np.full((R, CC), 0.01), "clump": np.full((R, CC), 0.1)}
    r, c = np.meshgrid(np.arange(R), np.arange(CC), indexing="ij")
    other = {"zref": 2.0, "lats": np.full((R, CC), 50.0), "lons": np.full((R, CC), -5.0), "isnowdc": np.zeros((R, CC)),
             "isnowdg": np.zeros((R, CC)), "isnowac": np.zeros((R, CC)), "isnowag": np.zeros((R, CC))}
    return (obstime, clim, pointm, vegp, other, "Taiga", 100.0 + 2.0 * r + c, np.full((CR, CCC), 110.0), 10.0, 0.01,
            api.coarse_positions(R, CR), api.coarse_positions(CC, CCC), altcorrect, 10, chunk_steps)


def _marshal(**kw):
    m, cin, _ = S.marshal_snowcoarse(*_args(**kw))
    return m, cin


def _fine(nsteps):
    keep = [np.empty((R, CC, max(nsteps, 1)), order="F") for _ in range(13)]
    return keep, (_abi.c_double_p * 13)(*[a.ctypes.data_as(_abi.c_double_p) for a in keep])


def _model(lib, cin, out=None):
    if out is None:
        out = _abi.SnowFast2Out()
    rc = lib.mcf_snowmodel2_coarse(C.byref(cin), C.byref(out), 0)
    return rc, (lib.mcf_last_error() or b"").decode()


def _expand(lib, cin, step0=0, nsteps=24):
    keep, ptrs = _fine(nsteps)
    rc = lib.mcf_snow_expand_coarse_device(C.byref(cin), step0, nsteps, ptrs, 0)
    return rc, (lib.mcf_last_error() or b"").decode()


def _both(lib, cin):
    """-> [(entry, status, message)] of the two entries on the same arguments"""
    return [(MODEL, *_model(lib, cin)), (EXPAND, *_expand(lib, cin))]


@pytest.mark.parametrize("altcorrect", [0, 1, 2])
def test_plausible_inputs_reach_the_device_lookup(lib, altcorrect):
    m, cin = _marshal(altcorrect=altcorrect)
    for entry, rc, msg in _both(lib, cin):
        assert rc != MCF_ERR_ARG, (entry, msg)               # no device here: the error after the checks; with one: the call runs
        if lib.mcf_device_count() < 1:
            assert rc != 0 and "device" in msg.lower(), (entry, rc, msg)
    m, cin = _marshal(chunk_steps=0)                         # 0: 120
    assert _model(lib, cin)[0] != MCF_ERR_ARG


def test_null_arguments_are_refused_and_named(lib):
    out = _abi.SnowFast2Out()
    m, cin = _marshal()
    assert lib.mcf_snowmodel2_coarse(None, C.byref(out), 0) == MCF_ERR_ARG
    assert lib.mcf_last_error().decode().startswith(MODEL) and b"null argument: in" in lib.mcf_last_error()
    assert lib.mcf_snowmodel2_coarse(C.byref(cin), None, 0) == MCF_ERR_ARG and b"null argument: out" in lib.mcf_last_error()
    keep, ptrs = _fine(24)
    assert lib.mcf_snow_expand_coarse_device(None, 0, 24, ptrs, 0) == MCF_ERR_ARG
    assert lib.mcf_last_error().decode().startswith(EXPAND) and b"null argument: in" in lib.mcf_last_error()
    assert lib.mcf_snow_expand_coarse_device(C.byref(cin), 0, 24, None, 0) == MCF_ERR_ARG and b"null argument: fine" in lib.mcf_last_error()
    ptrs[5] = None
    assert lib.mcf_snow_expand_coarse_device(C.byref(cin), 0, 24, ptrs, 0) == MCF_ERR_ARG and b"fine[5]" in lib.mcf_last_error()
    for field in ("coarse_rowpos", "coarse_colpos", *_abi.SNOWFAST2_SELECTED):
        m, cin = _marshal()
        setattr(cin, field, None)
        for entry, rc, msg in _both(lib, cin):
            assert rc == MCF_ERR_ARG and msg.startswith(entry) and "null" in msg and field in msg, (field, rc, msg)
    m, cin = _marshal()
    cin.drv.dtm = None
    for entry, rc, msg in _both(lib, cin):
        assert rc == MCF_ERR_ARG and msg.startswith(entry) and "null input: dtm" in msg, (rc, msg)
    # what the model alone reads; the expansion accepts its absence
    for where, field, name in (("drv", "af_wind", "af_wind"), ("clim", "winddir", "winddir"), ("vegp", "hgt", "hgt"),
                               ("other", "isnowdc", "isnowdc"), ("other", "isnowdg", "isnowdg"), ("other", "isnowag", "isnowag"),
                               ("other", "lats", "lats"), ("other", "lons", "lons"), ("obstime", "hour", "obstime")):
        m, cin = _marshal()
        setattr(cin.drv if where == "drv" else getattr(cin.drv.base, where), field, None)
        rc, msg = _model(lib, cin)
        assert rc == MCF_ERR_ARG and msg.startswith(MODEL) and "null" in msg and name in msg, (where, field, rc, msg)
        assert _expand(lib, cin)[0] != MCF_ERR_ARG
    m, cin = _marshal()                                      # what the entries ignore may be null: the raster-sized weather, the terrain
    assert not cin.drv.base.clim.temp and not cin.drv.base.clim.windspeed and not cin.drv.base.pointm.Gp and not cin.drv.base.other.hor


def test_a_bad_coarse_grid_is_refused(lib):
    for field in ("coarse_rows", "coarse_cols"):
        for v in (0, -1):
            m, cin = _marshal()
            setattr(cin, field, v)
            for entry, rc, msg in _both(lib, cin):
                assert rc == MCF_ERR_ARG and msg.startswith(entry) and "coarse_rows" in msg, (field, v, rc, msg)
    m, cin = _marshal()                                      # 24 x coarse cells x 8 B = 2^32: mcf_snowmodelq2's bound
    cin.coarse_rows, cin.coarse_cols = 4096, 5462
    for entry, rc, msg in _both(lib, cin):
        assert rc == MCF_ERR_ARG and msg.startswith(entry) and "2^32" in msg, (rc, msg)


def test_positions_outside_the_coarse_grid_are_refused(lib):
    a = _args()
    for k, bad in ((10, 2.0), (10, -0.25), (10, float("nan")), (11, 2.5), (11, -1.0)):      # 2 coarse rows, 3 coarse columns
        b = list(a)
        b[k] = np.array(a[k], copy=True)
        b[k][-1] = bad
        m, cin, _ = S.marshal_snowcoarse(*b)
        for entry, rc, msg in _both(lib, cin):
            assert rc == MCF_ERR_ARG and msg.startswith(entry) and "coarse_rowpos" in msg, (k, bad, rc, msg)


def test_a_bad_altcorrect_is_refused(lib):
    for v in (-1, 3):
        m, cin = _marshal()
        cin.altcorrect = v
        for entry, rc, msg in _both(lib, cin):
            assert rc == MCF_ERR_ARG and msg.startswith(entry) and "altcorrect" in msg, (v, rc, msg)
    for v in (1, 2):
        m, cin = _marshal(altcorrect=v)
        cin.coarse_dtm = None
        for entry, rc, msg in _both(lib, cin):
            assert rc == MCF_ERR_ARG and msg.startswith(entry) and "altcorrect" in msg and "coarse_dtm" in msg, (v, rc, msg)
    m, cin = _marshal()                                      # not read without the correction
    cin.coarse_dtm = None
    assert all(rc != MCF_ERR_ARG for _, rc, _ in _both(lib, cin))


def test_chunks_of_broken_days_are_refused(lib):
    for v in (1, 23, 25, 100, -24):
        m, cin = _marshal(chunk_steps=v)
        rc, msg = _model(lib, cin)
        assert rc == MCF_ERR_ARG and msg.startswith(MODEL) and "chunk_steps" in msg and "whole days" in msg, (v, rc, msg)
        assert _expand(lib, cin)[0] != MCF_ERR_ARG           # (the expansion has no chunks)


def test_vector_forcing_is_refused(lib):
    m, cin = _marshal()
    cin.drv.base.array_forcing = 0
    for entry, rc, msg in _both(lib, cin):
        assert rc == MCF_ERR_ARG and msg.startswith(entry) and "array_forcing" in msg, (rc, msg)


def test_steps_outside_the_series_are_refused(lib):
    m, cin = _marshal()
    for step0, nsteps in ((-1, 24), (0, 0), (0, -3), (0, T + 1), (T - 23, 24), (T, 1)):
        rc, msg = _expand(lib, cin, step0, nsteps)
        assert rc == MCF_ERR_ARG and msg.startswith(EXPAND) and "step0" in msg and "nsteps" in msg, (step0, nsteps, rc, msg)
    for step0, nsteps in ((0, T), (T - 1, 1), (17, 25)):
        assert _expand(lib, cin, step0, nsteps)[0] != MCF_ERR_ARG
    with pytest.raises(_abi.McfError, match="step0"):
        a = _args()
        S.expand_coarse(a[1], a[2], a[6], a[7], rowpos=a[10], colpos=a[11], step0=T - 5, nsteps=6)


def test_python_names_the_series_it_can_return():
    a = _args()
    with pytest.raises(ValueError, match="series"):
        S.snowmodel2_coarse(*a[:10], rowpos=a[10], colpos=a[11], series=("sdepc",))
    with pytest.raises(ValueError, match="series"):
        S.snowmodel2_coarse(*a[:10], rowpos=a[10], colpos=a[11], series=())


def test_device_loop_is_the_slow_method_and_one_call_stays_the_fast_one():
    complete = {"subs": np.arange(1, 49), "ntme": 48}
    subset = {"subs": np.arange(25, 49), "ntme": 96}
    kw = dict(dtmc=None, lats_c=None, lons_c=None, lats=None, lons=None)
    with pytest.raises(ValueError, match="one_call"):        # the fast method's device-resident form has its own keyword
        F.runsnowmodela({}, {}, [subset, subset], {}, {}, {}, method="fast", device_loop=True, **kw)
    with pytest.raises(ValueError, match="device_loop"):
        F.runsnowmodela({}, {}, [subset, subset], {}, {}, {}, device_loop=True, **kw)          # (the default method is "fast")
    with pytest.raises(ValueError, match="one_call"):
        F.runsnowmodela({}, {}, [complete, complete], {}, {}, {}, one_call=True, **kw)
    with pytest.raises(ValueError, match="one_call"):
        F.runsnowmodela({}, {}, [subset, subset], {}, {}, {}, method="slow", one_call=True, **kw)
    with pytest.raises(ValueError, match="one_call"):
        F.runsnowmodela({}, {}, [subset, subset], {}, {}, {}, method="slow", one_call=True, device_loop=True, **kw)
    # the slow method and complete micropoints pass the keyword checks (the empty inputs fail further on)
    for mp, method in (([subset, subset], "slow"), ([complete, complete], "fast")):
        with pytest.raises(Exception) as e:
            F.runsnowmodela({}, {}, mp, {}, {}, {}, method=method, device_loop=True, **kw)
        assert "device_loop" not in str(e.value) and "one_call" not in str(e.value)
