"""mcf_runbioclim_depths / api.runbioclim_depths / frontend.runbioclim_depths, CPU side: the entry is declared, exported and
bound; every refusal that needs no plan comes before a device is touched (each is raised with a device ordinal that does not
exist) and starts with the entry's name; the front end prepares the very call runbioclim(reqhgt = depths[0]) prepares, with
one point-model run."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import bundled
from microclimf_amd import _abi, api, frontend as F, synthetic
from microclimf_amd.marshal import marshal

NAME = "mcf_runbioclim_depths"
NO_DEVICE = 4711
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc")
TAIL = ("zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "mat")


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def call(T=336, depths=(-0.05, -0.2), array_forcing=False, **over):
    a = synthetic.workload(4, 5, T, reqhgt=-0.05, array_forcing=array_forcing)
    q = np.arange(72)
    kw = dict(out=[1] * 19, wetq=q, dryq=q, hotq=q, colq=q, air=True, array_forcing=array_forcing, device=NO_DEVICE)
    kw.update(over)
    return api.runbioclim_depths(*[a[k] for k in ARGS], depths, *[a[k] for k in TAIL], **kw)


def test_the_entry_is_declared_exported_and_bound():
    lib = _lib()
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mcf.h").read_text()
    assert NAME in _abi.EXPORTS and hasattr(lib, NAME)
    assert re.search(r"\bint " + NAME + r"\(", hdr)
    assert getattr(lib, NAME).argtypes is not None
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION           # functions only: the ABI number stays
    assert C.sizeof(_abi.BioclimDepthsOut) == (8 * 11 + 8) * 8 and _abi.MAX_DEPTHS == 8
    assert "double *temp[MCF_MAX_DEPTHS][11]" in hdr and "double *moist[8]" in hdr


@pytest.mark.parametrize("kw,msg", [
    (dict(depths=()), "a null or empty depth list"),
    (dict(depths=[-0.01 * (i + 1) for i in range(9)]), "9 depths, at most MCF_MAX_DEPTHS = 8"),
    (dict(depths=(-0.05, 0.0)), r"depths\[1\] is not below ground"),
    (dict(depths=(-0.05, 0.1)), r"depths\[1\] is not below ground"),
    (dict(depths=(float("nan"),)), r"depths\[0\] is not below ground"),
    (dict(air=False), "tleaf does not exist below ground"),
    (dict(array_forcing=True), "fine array forcing is not taken.*mcf_runbioclim2"),
    (dict(T=240), ">= 336 hourly steps in whole days"),
    (dict(T=340), ">= 336 hourly steps in whole days"),
    (dict(wetq=np.arange(72)[::-1].copy()), "not in ascending order.*mcf_runbioclim1"),
    (dict(dryq=np.array([5, 4, 6])), "not in ascending order.*mcf_runbioclim1"),
    (dict(hotq=np.array([0, 336])), "quarter index outside the time series"),
    (dict(chunk_days=-1), "negative chunk_days"),
], ids=["empty", "nine", "zero", "above", "nan", "air0", "fine-arrays", "T240", "T340", "descending", "dip", "outside", "chunk<0"])
def test_refusals_come_before_any_device_and_name_the_entry(kw, msg):
    _lib()
    with pytest.raises(_abi.McfError, match=r"error 1: " + NAME + ": .*" + msg):
        call(**kw)


def test_null_arguments_and_missing_buffers_are_refused():
    lib = _lib()
    E = 1   # MCF_ERR_ARG
    a = synthetic.workload(4, 5, 336, reqhgt=-0.05)
    m = marshal(*[a[k] for k in ARGS], -0.05, *[a[k] for k in TAIL[:6]], True, a["mat"], [1] * 10, False, NO_DEVICE)
    q = np.arange(72, dtype=np.int32)
    sel = _abi.BioclimSel()
    for n in ("wet", "dry", "hot", "col"):
        setattr(sel, n + "q", q.ctypes.data_as(_abi.c_int32_p))
        setattr(sel, "n" + n, q.size)
    sel.air = 1
    d = np.array([-0.05, -0.2])
    dp = d.ctypes.data_as(_abi.c_double_p)
    buf = [np.empty((4, 5), order="F") for _ in range(3)]
    ptr = lambda x: x.ctypes.data_as(_abi.c_double_p)      # noqa: E731
    bo = _abi.BioclimDepthsOut()
    run = lambda: lib.mcf_runbioclim_depths(C.byref(m.inputs), C.byref(m.options), C.byref(sel), dp, 2, 0, C.byref(bo))      # noqa: E731
    err = lambda: lib.mcf_last_error().decode()            # noqa: E731
    assert lib.mcf_runbioclim_depths(None, C.byref(m.options), C.byref(sel), dp, 2, 0, C.byref(bo)) == E and err().startswith(NAME)
    assert lib.mcf_runbioclim_depths(C.byref(m.inputs), C.byref(m.options), None, dp, 2, 0, C.byref(bo)) == E and err().startswith(NAME)
    assert lib.mcf_runbioclim_depths(C.byref(m.inputs), C.byref(m.options), C.byref(sel), dp, 2, 0, None) == E and err().startswith(NAME)
    assert lib.mcf_runbioclim_depths(C.byref(m.inputs), C.byref(m.options), C.byref(sel), None, 2, 0, C.byref(bo)) == E
    assert err().startswith(NAME + ": a null or empty depth list")
    # bio1 selected: a buffer per listed depth
    sel.out[0] = 1
    bo.temp[0][0] = ptr(buf[0])
    assert run() == E and err().startswith(NAME) and "bio1 has a null buffer at depth 1" in err()
    bo.temp[1][0] = ptr(buf[1])
    # bio12 selected: one buffer
    sel.out[11] = 1
    assert run() == E and err().startswith(NAME) and "bio12 has a null buffer" in err()
    bo.moist[0] = ptr(buf[2])
    # everything that can be judged without a device is in order: the refusal is now the device's
    rc = run()
    assert rc != 0 and rc != E and err().startswith(NAME), err()
    # a refusal of the checks shared with the other entries is named with this entry too
    m.inputs.rows = 0
    assert run() != 0 and err().startswith(NAME)


def test_the_whole_series_entries_are_as_they_were():
    """mcf_runbioclim1 with reqhgt < 0 is not routed through the new sink: its refusals keep their wording"""
    _lib()
    a = synthetic.workload(4, 5, 240, reqhgt=-0.05)
    with pytest.raises(_abi.McfError, match=r"error 1: runbioclim needs >= 336"):
        api.runbioclim1Cpp(*[a[k] for k in ARGS], -0.05, *[a[k] for k in TAIL], [1] * 19, [0], [0], [0], [0], True, device=NO_DEVICE)


@pytest.mark.parametrize("layered", [False, True])
def test_front_end_prepares_the_call_of_runbioclim_at_the_first_depth(monkeypatch, layered):
    from oracle import terrain_oracle as TO
    weather, vegp, soilc, dtm = bundled.load()
    if not layered:
        vegp = {k: (v[:, :, 6] if v.ndim == 3 else v) for k, v in vegp.items()}
    depths = (-0.1, -0.02, -0.5)
    terrain = {}

    def terrain_once(*a):                         # (the terrain does not depend on the height: computed once for both calls)
        if "t" not in terrain:
            terrain["t"] = TO.terrain(*a)
        return terrain["t"]
    runs = []
    point = F.runpointmodel
    monkeypatch.setattr(F, "runpointmodel", lambda *a, **k: runs.append(a[1]) or point(*a, **k))
    seen = {}
    out = [1, 0, 1] + [0] * 8 + [1] + [0] * 7

    def stub(lay, args, kw):
        seen["depths"] = (lay, args, kw)
        return {"depths": np.asarray(depths), "bio1": np.zeros((3,) + np.shape(dtm["z"])), "bio12": np.zeros(np.shape(dtm["z"]))}
    got = F.runbioclim_depths(weather, depths, vegp, soilc, dtm, out=out, _bioclim=stub, _terrain=terrain_once)
    assert runs == [-0.1]                         # exactly one point-model run, at depths[0]
    assert set(got) == {"depths", "bio1", "bio12"}
    F.runbioclim(weather, -0.1, vegp, soilc, dtm, out=out, _bioclim=lambda lay, args, kw: seen.update(single=(lay, args, kw)) or {},
                 _terrain=terrain_once)
    (l1, a1, k1), (l0, a0, k0) = seen["depths"], seen["single"]
    assert l1 == l0 == layered
    assert "reqhgt" not in a1 and np.array_equal(a1["depths"], depths) and a0["reqhgt"] == -0.1
    assert set(a1) - {"depths"} == set(a0) - {"reqhgt"}

    def same(x, y, what):
        if isinstance(x, dict):
            assert list(x) == list(y), what
            for k in x:
                same(x[k], y[k], (what, k))
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), what
    for k in set(a0) - {"reqhgt"}:                # obstime, climdata, pointm, vegp, soilc, zref, lat, lon, Sminp, Smaxp
        same(a1[k], a0[k], k)
    assert list(k1) == list(k0)
    for k in k0:                                  # tfact, mat, out, wetq, dryq, hotq, colq, air
        same(k1[k], k0[k], k)
    # (a quarter's list holds every modelled hour of its three months: the hottest or coldest day may be among them)
    assert k1["air"] is True and all(len(k1[q]) >= 72 and (np.diff(k1[q]) > 0).all() for q in ("wetq", "dryq", "hotq", "colq"))
    with pytest.raises(ValueError, match="below ground"):
        F.runbioclim_depths(weather, (-0.1, 0.05), vegp, soilc, dtm, _bioclim=stub, _terrain=terrain_once)
