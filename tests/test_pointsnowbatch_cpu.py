"""The batched snow point model (mcf_pointmodelsnow_batch) as far as a host without a GPU can see it: the entry exists in
every layer, it refuses what it must before the device is touched, the batches of test_pointsnowbatch_gpu.py are admissible
and carry the edge conditions they are there for (pointsnowbatch_cases.py), and the host entry the device is compared with
through `runsnowmodela` equals the oracle on them."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import parity_bars
import pointsnowbatch_cases as SC
from microclimf_amd import _abi
from microclimf_amd import pointmodel as PM

ROOT = Path(__file__).resolve().parent.parent


def _bars(oracle, name):
    return parity_bars.bars_for(oracle, SC.run(oracle, SC.make(name)), ("pointsnowbatch", name))


def test_entry_is_declared_exported_and_bound():
    header = (ROOT / "include" / "mcf.h").read_text()
    lib = _abi.load()
    assert re.search(r"\bint\s+mcf_pointmodelsnow_batch\s*\(", header) and "mcf_pointsnow_batch_out" in header
    assert "mcf_pointmodelsnow_batch" in _abi.EXPORTS
    fn = lib.mcf_pointmodelsnow_batch                       # AttributeError if the library does not export it
    assert fn.restype is C.c_int and len(fn.argtypes) == 12
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION   # entries are added only


def _call(P=2, n=48, **kw):
    t = {"year": np.full(n, 2023, dtype=np.int32), "month": np.full(n, 1, dtype=np.int32),
         "day": (1 + np.arange(n) // 24).astype(np.int32), "hour": (np.arange(n) % 24).astype(np.float64)}
    row = {"temp": -5.0, "relhum": 70.0, "pres": 101.0, "swdown": 100.0, "difrad": 50.0, "lwdown": 250.0, "windspeed": 2.0,
           "precip": 0.1}
    W = {k: np.full((P, n), v) for k, v in row.items()}
    vegp = np.tile(np.array([1.0, 1.5, 0.1, 0.2]), (P, 1))
    other = np.tile(np.array([5.0, 180.0, 57.0, -5.0, 3.5, 0.3, 10.0]), (P, 1))
    return PM.pointmodelsnow_batch(t, W, vegp, other, "Taiga", maxiter=10, **kw)


def test_refusals_come_before_the_device_and_name_their_cause():
    with pytest.raises(_abi.McfError, match=r"error 1: .*P < 1"):
        _call(P=0)
    with pytest.raises(_abi.McfError, match=r"error 1: .*whole days"):
        _call(n=30)
    with pytest.raises(_abi.McfError, match=r"error 1: .*whole days"):
        _call(n=5)
    with pytest.raises(_abi.McfError, match=r"error 1: .*n < 24"):
        _call(n=0)
    with pytest.raises(_abi.McfError, match=r"error 1: .*points_per_block < 0"):
        _call(points_per_block=-1)


def test_null_arguments_too_long_series_and_null_output_vectors_are_refused():
    lib = _abi.load()
    null_d, null_i = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
    rc = lib.mcf_pointmodelsnow_batch(2, 48, None, None, null_d, null_d, null_i, 0.5, 10.0, 0, 0, None)
    assert rc == 1 and b"null" in lib.mcf_last_error()
    n = 24
    x, iy = np.zeros(2 * (n + 1)), np.ones(2 * n, dtype=np.int32)
    dp, ip = x.ctypes.data_as(_abi.c_double_p), iy.ctypes.data_as(_abi.c_int32_p)
    t = _abi.Obstime()
    t.year, t.month, t.day, t.hour = ip, ip, ip, dp
    w = _abi.PointWeather()
    for f in _abi.POINT_WEATHER_FIELDS:
        setattr(w, f, dp)
    out = _abi.PointSnowBatchOut()
    for f in _abi.POINTSNOW_BATCH_FIELDS:
        setattr(out, f, dp)
    out.mxdif, out.iters = dp, ip
    call = lambda n_, w_, o_: lib.mcf_pointmodelsnow_batch(2, n_, C.byref(t), C.byref(w_), dp, dp, ip, 0.5, 10.0, 0, 0,   # noqa: E731
                                                           C.byref(o_))
    assert call((1 << 28) + 8, w, out) == 1 and b"too long" in lib.mcf_last_error()       # nothing is read before the refusal
    w.precip = None
    assert call(n, w, out) == 1 and b"null weather column" in lib.mcf_last_error()
    w.precip = dp
    for f in ("sstemp", "sdepg", "mxdif", "iters"):
        keep = getattr(out, f)
        setattr(out, f, None)
        assert call(n, w, out) == 1 and b"null output vector" in lib.mcf_last_error(), f
        setattr(out, f, keep)


def test_a_well_formed_call_needs_a_device():
    if _abi.load().mcf_device_count() > 0:
        res = _call()                                      # on a GPU host the same call runs
        assert all(np.asarray(v).shape[0] == 2 for v in res.values())
        return
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        _call()
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        _call(P=1, n=24)


@pytest.mark.parametrize("name", list(SC.BATCHES))
def test_batches_are_admissible(oracle, name):
    """every noise variant reports the oracle's iteration counts and no derived bar reaches CAP (pointsnowbatch_cases.py)"""
    want, bars, noise = _bars(oracle, name)
    assert noise["iters"] == 0.0
    assert max(bars.values()) < parity_bars.CAP, bars
    assert all(np.isfinite(v).all() for v in want.values())


def test_batches_carry_their_edge_conditions(oracle):
    w67, w3, w1 = _bars(oracle, "day2_p67")[0], _bars(oracle, "day3_p5")[0], _bars(oracle, "day1_p5")[0]
    assert len(set(w67["iters"].tolist())) > 1                          # points stop at different passes
    assert (w3["iters"] == 11).any() and (w3["iters"] < 11).any()       # maxiter + 1 passes beside points that stopped before
    for name in ("day1_p5", "day2_p67", "day3_p5", "day12_p5"):
        b, want = SC.make(name), _bars(oracle, name)[0]
        g = want["sdepg"]
        assert ((g[:, 1:] == 0) & (g[:, :-1] > 0)).any(), name          # a ground pack melts out: the clamp and the age reset
        assert b["vegp"][0, 1] == 0                                      # no canopy
        assert want["sdepg"][1, 0] > b["vegp"][1, 1] > 0                 # a buried canopy
        assert want["sdepc"][2, 0] == 0
    assert ((w1["sdepg"][3, 1:] == 0)).sum() >= 1


def test_host_entry_equals_the_oracle_on_day3_p5(oracle):
    b = SC.make("day3_p5")
    want = SC.run(oracle, b)(None)
    for p in range(b["P"]):
        got = PM.pointmodelsnow(*SC.point_args(b, p))
        assert got["iters"] == want["iters"][p]
        for k in SC.SERIES:
            np.testing.assert_allclose(got[k], want[k][p], rtol=1e-9, atol=1e-9, err_msg=f"point {p} {k}")
        assert abs(got["mxdif"] - want["mxdif"][p]) <= 1e-9 * (1 + abs(want["mxdif"][p]))
