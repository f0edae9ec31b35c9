"""The batched point model (mcf_bigleaf_batch, mcf_weatherhgt_batch, mcf_pointmprocess_batch) as far as a host without a
GPU can see it: the entries exist in every layer, they refuse what the single-point entries refuse (and partial days)
before the device is touched, and the batches of test_pointbatch_gpu.py are admissible (pointbatch_cases.py)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import parity_bars
import pointbatch_cases as PC
from microclimf_amd import _abi
from microclimf_amd import pointmodel as PM

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("mcf_bigleaf_batch", "mcf_weatherhgt_batch", "mcf_pointmprocess_batch")


def test_entries_are_declared_exported_and_bound():
    header = (ROOT / "include" / "mcf.h").read_text()
    lib = _abi.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _abi.EXPORTS
        fn = getattr(lib, name)                       # AttributeError if the library does not export it
        assert fn.restype is C.c_int and fn.argtypes, name
    assert "mcf_bigleaf_batch_out" in header and "nothing to parallelise" not in header
    assert "whole days only" in header.lower()


def test_abi_version_is_still_8():
    lib = _abi.load()
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION
    assert re.search(r"#define\s+MCF_ABI_VERSION\s+8\b", (ROOT / "include" / "mcf.h").read_text())


def _inputs(P=2, n=48):
    t = {"year": np.full(n, 2023, dtype=np.int32), "month": np.full(n, 6, dtype=np.int32),
         "day": (1 + np.arange(n) // 24).astype(np.int32), "hour": (np.arange(n) % 24).astype(np.float64)}
    row = {"temp": 15.0, "relhum": 70.0, "pres": 101.0, "swdown": 200.0, "difrad": 100.0, "lwdown": 330.0, "windspeed": 2.0}
    W = {k: np.full((P, n), v) for k, v in row.items()}
    vegp = np.tile(np.array([0.5, 2.0, 1.0, 0.1, 0.4, 0.2, 0.05, 0.97, 0.33, 100.0]), (P, 1))
    groundp = np.tile(np.array([0.15, 0, 180, 0.97, 1.53, 0.509, 0.06, 0.5422, 5.2, -5.6, 0.42, 0.074]), (P, 1))
    return t, W, vegp, groundp, np.full((P, n), 0.3), np.full(P, 50.0), np.full(P, -5.0)


def _bigleaf(P=2, n=48, **kw):
    t, W, vegp, groundp, sm, lat, lon = _inputs(P, n)
    return PM.BigLeafBatch(t, W, vegp, groundp, sm, lat, lon, yearG=kw.pop("yearG", False), **kw)


def _pmp(P=2, n=48):
    t, W, vegp, groundp, sm, lat, lon = _inputs(P, n)
    pv = {"windspeed": W["windspeed"], "tc": W["temp"], "rh": W["relhum"], "pk": W["pres"], "uf": np.full((P, n), 0.3),
          "soilm": sm, "RabsG": np.full((P, n), 400.0)}
    return PM.pointmprocess_batch(pv, 2.0, vegp[:, 0], vegp[:, 1], groundp[:, 4], groundp[:, 5], groundp[:, 6], groundp[:, 7])


def _weatherhgt(P=2, n=48):
    t, W, vegp, groundp, sm, lat, lon = _inputs(P, n)
    return PM.weatherhgt_batch(t, W, 2.0, 2.0, 10.0, lat, lon)


@pytest.mark.parametrize("call", [_bigleaf, _weatherhgt, _pmp])
def test_refusals_come_before_the_device_and_name_their_cause(call):
    with pytest.raises(_abi.McfError, match=r"error 1: .*P < 1"):
        call(P=0)
    with pytest.raises(_abi.McfError, match=r"error 1: .*n < 6"):
        call(n=5)
    with pytest.raises(_abi.McfError, match=r"error 1: .*whole days"):
        call(n=30)


def test_bigleaf_batch_refuses_yearG_for_2_to_89_days_and_null_arguments():
    with pytest.raises(_abi.McfError, match=r"error 1: .*yearG"):
        _bigleaf(n=5 * 24, yearG=True)
    with pytest.raises(_abi.McfError, match=r"error 1: .*yearG"):
        _bigleaf(n=89 * 24, yearG=True)
    lib = _abi.load()
    null_d = C.POINTER(C.c_double)()
    rc = lib.mcf_bigleaf_batch(2, 48, None, None, null_d, null_d, null_d, null_d, null_d, 25.0, 2.0, 20, 0.5, 0.5, 0, 0, 0, None)
    assert rc == 1 and b"null" in lib.mcf_last_error()
    rc = lib.mcf_weatherhgt_batch(2, 48, None, None, 2.0, 2.0, 10.0, null_d, null_d, 0, 0, null_d, null_d, null_d)
    assert rc == 1 and b"null" in lib.mcf_last_error()
    rc = lib.mcf_pointmprocess_batch(2, 48, *[null_d] * 7, 2.0, *[null_d] * 6, 0, *[null_d] * 6)
    assert rc == 1 and b"null" in lib.mcf_last_error()


@pytest.mark.parametrize("call", [_bigleaf, _weatherhgt, _pmp])
def test_a_well_formed_call_needs_a_device(call):
    if _abi.load().mcf_device_count() > 0:
        res = call()                                  # on a GPU host the same call runs
        assert all(np.asarray(v).shape[0] == 2 for v in res.values())
        return
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        call()
    with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):
        _bigleaf(n=24, yearG=True)                    # one day: yearG is legal


@pytest.mark.parametrize("name", [k for k in PC.BATCHES if k not in PC.PAI0])
def test_batches_are_admissible(oracle, name):
    """every noise variant reports the oracle's iteration counts and no derived bar reaches CAP (pointbatch_cases.py)"""
    b = PC.make(name)
    want, bars, noise = parity_bars.bars_for(oracle, PC.bigleaf_run(oracle, b), ("pointbatch", name))
    assert noise["iters"] == 0.0
    assert max(bars.values()) < parity_bars.CAP, bars
    if b["yearG"]:                                    # orc_weatherhgt always asks for the annual term: one day or >= 90
        _, wbars, _ = parity_bars.bars_for(oracle, PC.weatherhgt_run(oracle, b, b["zref"], b["zref"], b["zref"] + 8.0),
                                           ("pointbatch-wh", name))
        assert max(wbars.values()) < parity_bars.CAP, wbars


def test_batches_cover_unequal_iteration_counts_and_maxiter(oracle):
    its = {name: PC.bigleaf_run(oracle, PC.make(name))(None)["iters"] for name in ("day2_p67", "day3_p5")}
    assert len(set(its["day2_p67"].tolist())) > 1                       # points stop at different iteration counts
    assert (its["day3_p5"] == PC.make("day3_p5")["maxiter"]).any()      # a point runs to maxiter ...
    assert (its["day3_p5"] < PC.make("day3_p5")["maxiter"]).any()       # ... while another of its batch has stopped


def test_the_pai0_batch_is_stable_under_contraction(oracle):
    """what CAN be checked of the pai = 0 batch on the reference side (pointbatch_cases.PAI0): the fma variant keeps the
    oracle's NaN pattern and iteration counts"""
    b = PC.make("pai0_p5")
    run = PC.bigleaf_run(oracle, b)
    want, fma = run(None), run(oracle.load_variant("fma"))
    assert np.array_equal(want["iters"], fma["iters"])
    assert np.isnan(want["Tc"][2]).all() and not np.isnan(want["albedo"][2]).any()
    for k in want:
        assert parity_bars.same_pattern(want[k], fma[k]), k
        assert parity_bars.distance(fma[k], want[k]) < parity_bars.CAP / parity_bars.K, k
