"""Below ground streamed through day chunks (include/mcf.h mcf_plan_create_streamed / mcf_plan_below_prepare): the streamed
plan's Tz and soilm have the whole-series plan's bits — NaN payloads included — across complete 0 / 1, all three smoothing
regimes of manCpp (n <= 48, 48 < n < tsteps, n >= tsteps) on one raster, a series that is not a whole number of days, NA
cells, chunk sizes that do and do not divide the day count, layered vegetation, array and coarse forcing and the
multi-block entry; and a 2048 x 2048 year that the whole-series plan could not hold, against the oracle."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import McfError, synthetic
from microclimf_amd.api import Plan, runmicro1Cpp, runmicro2Cpp, runmicro2Cpp_coarse, runmicro3Cpp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
T_ODD = 24 * 9 + 7          # nine days and seven steps
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact",
        "complete", "mat", "out")
OUT = [1, 0, 0, 1, 0, 0, 0, 0, 0, 0]     # what .runmodel1Cpp keeps below ground (Tz, soilm)
OMDY = 2 * np.pi / (24 * 3600.0)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def same_bits(got, want, names=("Tz", "soilm")):
    for k in names:
        assert got[k].shape == want[k].shape, k
        diff = bits(got[k]) != bits(want[k])
        assert not diff.any(), f"{k}: {int(diff.sum())} values differ, first at {np.argwhere(diff)[0]}"


def with_env(value, fn, *args, **kw):
    old = os.environ.get("MCF_BELOW_STREAM")
    os.environ["MCF_BELOW_STREAM"] = value
    try:
        return fn(*args, **kw)
    finally:
        if old is None:
            del os.environ["MCF_BELOW_STREAM"]
        else:
            os.environ["MCF_BELOW_STREAM"] = old


def approx_n(a, tsteps):
    """manCpp's window length n per cell, from a numpy transcription of the soil damping depth (cpp:1021-1032, 1249-1260):
    close enough to sort cells into the three regimes away from their boundaries"""
    s = a["soilc"]
    twi = s["twi"]
    tadd = np.log(twi) / a["tfact"] - np.nanmean(np.log(twi) / a["tfact"])
    sm_p = np.asarray(a["pointm"]["soilm"])
    sm_p = sm_p[None, None, : (tsteps // 24) * 24] if sm_p.ndim == 1 else sm_p[:, :, : (tsteps // 24) * 24]
    rge = s["Smax"] - s["Smin"]
    theta = np.clip((sm_p - s["Smin"][..., None]) / rge[..., None], 1e-4, 0.9999)
    soilm = 1 / (1 + np.exp(-(np.log(theta / (1 - theta)) + tadd[..., None]))) * rge[..., None] + s["Smin"][..., None]
    Vq, Vm, Mc, rho = s["Vq"][..., None], s["Vm"][..., None], s["Mc"][..., None], s["rho"][..., None]
    frs = Vm + Vq
    c1 = (0.57 + 1.73 * Vq + 0.93 * Vm) / (1 - 0.74 * Vq - 0.49 * Vm) - 2.8 * frs * (1 - frs)
    c3 = 1 + 2.6 * Mc ** -0.5
    c4 = 0.03 + 0.7 * frs * frs
    cs = 2400 * rho / 2.64 + 4180 * soilm
    ph = (rho * (1 - soilm) + soilm) * 1000
    k = c1 + 1.06 * rho * soilm * soilm - (c1 - c4) * np.exp(-(c3 * soilm) ** 4)
    meanD = np.sqrt(2 * k / (cs * ph) / OMDY).sum(axis=-1) / tsteps
    return np.round(-118.35 * a["reqhgt"] / meanD)


def three_regimes(a, tsteps):
    """soils from a light quartz-rich one (deep damping) to a dense quartz-free one (shallow damping) in bands across the
    raster, and a depth at which the deepest-damped cells take the hourly window and the shallowest the series mean"""
    s = a["soilc"]
    rows, cols = s["twi"].shape
    f = (np.arange(rows)[:, None] + rows * np.arange(cols)[None, :]) / (rows * cols - 1.0)
    s["rho"] = np.asfortranarray(0.3 + 2.3 * f)
    s["Vq"] = np.asfortranarray(0.5 * (1 - f))
    s["Vm"] = np.asfortranarray(0.3 + 0.209 * f)
    a["reqhgt"] = -1.0
    n1 = approx_n(a, tsteps)
    a["reqhgt"] = -1.2 * tsteps / np.nanmax(n1)          # the shallowest-damped cells at n ~ 1.2 tsteps
    n = approx_n(a, tsteps)
    valid = ~np.isnan(a["vegp"]["hgt"])
    if a["vegp"]["hgt"].ndim == 3:
        valid = valid[..., 0]
    nv = n[valid]
    assert (nv <= 44).any() and ((nv >= 53) & (nv <= tsteps - 5)).any() and (nv >= tsteps + 5).any(), \
        (nv.min(), nv.max(), tsteps)
    return a


def with_na(a, cells=((0, 0), (3, 2), (5, 1))):
    for (i, j) in cells:
        a["vegp"]["hgt"][i, j, ...] = np.nan
    return a


@pytest.mark.parametrize("complete", [0, 1])
@pytest.mark.parametrize("chunk", [1, 2, 5, 7])
def test_runmicro1_streamed_is_whole_series_bits(complete, chunk):
    a = with_na(synthetic.workload(23, 11, T_ODD, reqhgt=-0.2, variety=True, start_doy=140, out=OUT, complete=bool(complete)))
    a = three_regimes(a, T_ODD)
    want = with_env("0", runmicro1Cpp, **a)
    got = with_env("1", runmicro1Cpp, **a, days_per_chunk=chunk)
    same_bits(got, want)
    assert np.isfinite(want["Tz"][:, :, : 9 * 24][~np.isnan(a["vegp"]["hgt"])]).all()


def test_streamed_without_tz_is_whole_series_bits():
    # no Tz requested: no Tg ring, nothing to prepare, the other outputs through the tiled ring
    out = [0, 1, 0, 1, 1, 1, 0, 1, 0, 0]
    a = with_na(synthetic.workload(13, 6, T_ODD, reqhgt=-0.2, variety=True, start_doy=140, out=out))
    want = with_env("0", runmicro1Cpp, **a)
    got = with_env("1", runmicro1Cpp, **a, days_per_chunk=2)
    same_bits(got, want, names=("tleaf", "soilm", "windspeed", "Rdirdown", "Rlwdown"))


@pytest.mark.parametrize("complete", [0, 1])
def test_runmicro2_streamed_is_whole_series_bits(complete):
    a = with_na(synthetic.workload(19, 9, T_ODD, reqhgt=-0.2, variety=True, start_doy=200, out=OUT, complete=bool(complete),
                                   array_forcing=True))
    a = three_regimes(a, T_ODD)
    a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
    want = with_env("0", runmicro2Cpp, **a)
    got = with_env("1", runmicro2Cpp, **a, days_per_chunk=2)
    same_bits(got, want)


def test_runmicro3_streamed_is_whole_series_bits():
    a = with_na(synthetic.workload(17, 5, T_ODD, reqhgt=-0.1, variety=True, start_doy=120, out=OUT))
    a = synthetic.layered(a, 3)
    dfsel = a.pop("dfsel")
    want = with_env("0", runmicro3Cpp, dfsel, **a)
    got = with_env("1", runmicro3Cpp, dfsel, **a, days_per_chunk=4)
    same_bits(got, want)


def test_runmicro2_coarse_streamed_is_whole_series_bits():
    a, rp, cp = synthetic.coarse_workload(26, 26, T_ODD, 4, 4, reqhgt=-0.1, variety=True, start_doy=170, na_frac=0.03,
                                          out=OUT)
    want = with_env("0", runmicro2Cpp_coarse, *[a[k] for k in ARGS], rowpos=rp, colpos=cp)
    got = with_env("1", runmicro2Cpp_coarse, *[a[k] for k in ARGS], rowpos=rp, colpos=cp, days_per_chunk=3)
    same_bits(got, want)


@pytest.mark.parametrize("complete", [0, 1])
def test_multi_three_blocks_streamed_is_whole_series_bits(complete):
    a = with_na(synthetic.workload(31, 7, T_ODD, reqhgt=-0.2, variety=True, start_doy=140, out=OUT, complete=bool(complete)))
    a = three_regimes(a, T_ODD)
    want = with_env("0", runmicro1Cpp, **a)
    got = with_env("1", runmicro1Cpp, **a, devices=[0], n_blocks=3, days_per_chunk=2)
    same_bits(got, want)


def _plans(a, ring_days, slots=2):
    whole = Plan(**a, ring_days=1)
    streamed = Plan(**a, ring_days=ring_days, ring_slots=slots, stream_below=True)
    return whole, streamed


@pytest.mark.parametrize("complete", [0, 1])
def test_plan_chunks_fetch_like_the_whole_series_plan(tmp_path, complete):
    a = with_na(synthetic.workload(23, 11, T_ODD, reqhgt=-0.2, variety=True, start_doy=140, out=OUT, complete=bool(complete)))
    a = three_regimes(a, T_ODD)
    rows, cols, nd = 23, 11, 9
    whole, st = _plans(a, ring_days=4)
    with whole, st:
        whole.run_days(0, nd, 0)
        whole.belowground()
        wz, ws = whole.fetch(0, "Tz", 0, T_ODD), whole.fetch(0, "soilm", 0, nd * 24)
        cells = np.array([0, 5, 17, 100, rows * cols - 1, 77], dtype=np.int64)
        st.below_prepare()
        d0, slot = 0, 0
        east, north = np.arange(cols) + 0.5, np.arange(rows)[::-1] + 0.5
        from microclimf_amd import ncsink
        f_st, f_wh = tmp_path / "streamed.nc", tmp_path / "whole.nc"
        with ncsink.NcWriter(f_st, rows, cols, np.arange(nd * 24) + 1.0, east, north, a["reqhgt"], ("Tz",)) as w:
            while d0 < nd:
                n = min(3, nd - d0)          # 3 days per chunk in a 4-day slot: the last chunk has room for the tail
                st.run_days(d0, n, slot)
                k0 = d0 * 24
                steps = n * 24 + (T_ODD - nd * 24 if d0 + n == nd else 0)
                assert bits(st.fetch(slot, "Tz", 0, steps)).tobytes() == bits(wz[:, :, k0:k0 + steps]).tobytes()
                assert bits(st.fetch(slot, "soilm", 0, n * 24)).tobytes() == bits(ws[:, :, k0:k0 + n * 24]).tobytes()
                got_c = st.fetch_cells(slot, "Tz", 0, steps, cells)
                want_c = wz.reshape(rows * cols, -1, order="F")[cells, k0:k0 + steps]
                assert (bits(got_c) == bits(want_c)).all()
                assert np.array_equal(st.fetch_packed(slot, "Tz", 0, n * 24), whole.fetch_packed(0, "Tz", k0, n * 24))
                w.write_plan(st, slot, 0, k0, n * 24)
                d0 += n
                slot ^= 1
        with ncsink.NcWriter(f_wh, rows, cols, np.arange(nd * 24) + 1.0, east, north, a["reqhgt"], ("Tz",)) as w:
            w.write_plan(whole, 0, 0, 0, nd * 24)
        assert f_st.read_bytes() == f_wh.read_bytes()


def test_streamed_plan_argument_checks():
    a = with_na(synthetic.workload(12, 7, T_ODD, reqhgt=-0.2, variety=True, start_doy=140, out=OUT))
    with Plan(**a, ring_days=3, stream_below=True) as st:
        with pytest.raises(McfError, match="mcf_plan_below_prepare"):
            st.run_days(0, 3, 0)
        st.below_prepare()
        st.run_days(0, 3, 0)
        with pytest.raises(McfError, match="day order"):
            st.run_days(6, 2, 0)          # skips days 3..5
        with pytest.raises(McfError, match="day order"):
            st.run_days(2, 1, 0)          # goes back
        st.run_days(3, 3, 0)
        with pytest.raises(McfError, match="streamed plan"):
            st.belowground()
        with pytest.raises(McfError, match="one day more"):
            st.run_days(6, 3, 0)          # the last chunk fills its 3-day slot: no room for the 7 steps behind it
        st.run_days(0, 1, 0)              # day 0 starts a new pass
        with pytest.raises(McfError, match="tile mask"):
            st.run_days_masked(1, 1, 0, 0, np.zeros(st.n_tiles, np.uint8))
        import torch
        need = torch.ones(12 * 7, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(McfError, match="cell subset"):
            st.run_days_cells(1, 1, 0, 0, need.data_ptr())
        with pytest.raises(McfError, match="day offset"):
            st.run_days_at(1, 1, 0, 1)
    with Plan(**a, ring_days=1) as whole:       # the whole-series plan has no streamed pass
        with pytest.raises(McfError, match="streamed plan"):
            whole.below_prepare()


def _scale_args(n, complete):
    a = synthetic.workload(n, n, 8760, reqhgt=-0.2, start_doy=1, out=OUT, complete=bool(complete))
    return a


def test_footprint_1024_streamed_is_a_quarter_of_the_whole_series():
    a = _scale_args(1024, 1)
    with Plan(**a, ring_days=30, stream_below=True) as st:
        b_st = st.device_bytes
    with Plan(**a, ring_days=1) as whole:
        b_wh = whole.device_bytes
    assert b_wh > 1024 * 1024 * 8760 * 8       # the [N][tsteps] Tg series alone
    assert 4 * b_st <= b_wh, (b_st, b_wh)


@pytest.mark.parametrize("complete", [1, 0])
def test_2048_year_streamed_matches_the_oracle(complete):
    """one device, 2048 x 2048 x 8760 below ground: d_tgser alone would need 294 GB.  Run in a child process under its own
    time limit; a seeded sample of valid cells against the oracle"""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve().parent / "below_stream_scale.py"), str(complete)],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "scale ok" in r.stdout, r.stdout[-3000:]
