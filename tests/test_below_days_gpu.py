"""A streamed below-ground plan over a subset of its days (include/mcf.h mcf_plan_below_set_days): the series Tbelowgroundv
sees is the subset's days joined end to end — what `.runmicrosnow1` (R/internal.R:3581-3659) hands the grid solver for
reqhgt < 0, the no-snow days — while forcing, vegetation layer and the point model's series are read at each day's own
place.  Held bit for bit — NaN payloads included — against the whole-series plan on inputs subset on the host
(runmicro1Cpp / runmicro3Cpp with MCF_BELOW_STREAM=0): complete 0 and 1, all three regimes of manCpp's window on one
raster, NA cells, calendar chunks of 1, 2 and 5 days and chunks that straddle the subset's gaps, layered vegetation with
whole-series layers, three row blocks; the full day list against the plan without a subset; and the refusals."""
import os

import numpy as np
import pytest

from microclimf_amd import McfError, synthetic
from microclimf_amd.api import Plan, runmicro1Cpp, runmicro3Cpp

pytestmark = pytest.mark.gpu
ROWS, COLS, NDAYS = 22, 13, 20
T = NDAYS * 24
DAYS = np.array([0, 1, 4, 5, 6, 9, 12, 13, 16, 18, 19])      # 11 of the 20: the first day, gaps of 1 .. 2 days, the last day
OUT = [1, 0, 0, 1, 0, 0, 0, 0, 0, 0]                           # what .runmodel1Cpp keeps below ground (Tz, soilm)
OMDY = 2 * np.pi / (24 * 3600.0)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def same_bits(got, want, names=("Tz", "soilm")):
    for k in names:
        assert got[k].shape == want[k].shape, k
        diff = bits(got[k]) != bits(want[k])
        assert not diff.any(), f"{k}: {int(diff.sum())} values differ, first at {np.argwhere(diff)[0]}"


def whole_series(fn, *args, **kw):
    """fn with the whole-series below-ground plan (MCF_BELOW_STREAM=0)"""
    old = os.environ.get("MCF_BELOW_STREAM")
    os.environ["MCF_BELOW_STREAM"] = "0"
    try:
        return fn(*args, **kw)
    finally:
        if old is None:
            del os.environ["MCF_BELOW_STREAM"]
        else:
            os.environ["MCF_BELOW_STREAM"] = old


def steps_of(days):
    return (np.repeat(np.asarray(days) * 24, 24) + np.tile(np.arange(24), len(days))).astype(np.int64)


def subset_inputs(a, days):
    """the inputs as `.runmicrosnow1` subsets them: the data.frame columns at the days' steps, the rasters as they are"""
    idx = steps_of(days)
    sub = lambda d: {k: (np.asarray(v)[idx] if np.ndim(v) == 1 else v) for k, v in d.items()}
    return dict(a, obstime=sub(a["obstime"]), climdata=sub(a["climdata"]), pointm=sub(a["pointm"]))


def approx_n(a, tsteps):
    """manCpp's window length n per cell, from a numpy transcription of the soil damping depth (cpp:1021-1032, 1249-1260) over
    the soil-moisture series of `a`: close enough to sort cells into the three regimes away from their boundaries"""
    s = a["soilc"]
    twi = s["twi"]
    tadd = np.log(twi) / a["tfact"] - np.nanmean(np.log(twi) / a["tfact"])
    sm_p = np.asarray(a["pointm"]["soilm"])[None, None, : (tsteps // 24) * 24]
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


def three_regimes(a, days):
    """soils from a light quartz-rich one (deep damping) to a dense quartz-free one (shallow damping) in bands across the
    raster, and a depth at which — on the SUBSET's m = 24 len(days) steps and its soil moisture — the deepest-damped cells
    take the hourly window (n <= 48), the shallowest the series mean (n >= m) and cells between them the daily means"""
    s = a["soilc"]
    rows, cols = s["twi"].shape
    f = (np.arange(rows)[:, None] + rows * np.arange(cols)[None, :]) / (rows * cols - 1.0)
    s["rho"] = np.asfortranarray(0.3 + 2.3 * f)
    s["Vq"] = np.asfortranarray(0.5 * (1 - f))
    s["Vm"] = np.asfortranarray(0.3 + 0.209 * f)
    m = 24 * len(days)
    a["reqhgt"] = -1.0
    n1 = approx_n(subset_inputs(a, days), m)
    a["reqhgt"] = -1.2 * m / np.nanmax(n1)          # the shallowest-damped cells at n ~ 1.2 m
    n = approx_n(subset_inputs(a, days), m)
    hgt = a["vegp"]["hgt"]
    valid = ~np.isnan(hgt[..., 0] if hgt.ndim == 3 else hgt)
    nv = n[valid]
    assert (nv <= 44).any() and ((nv >= 53) & (nv <= m - 5)).any() and (nv >= m + 5).any(), (nv.min(), nv.max(), m)
    return a


def with_na(a, cells=((0, 0), (3, 2), (5, 1))):
    for (i, j) in cells:
        a["vegp"]["hgt"][i, j, ...] = np.nan
    return a


def case(complete, rows=ROWS, cols=COLS):
    a = with_na(synthetic.workload(rows, cols, T, reqhgt=-0.2, variety=True, start_doy=140, out=OUT, complete=bool(complete)))
    return three_regimes(a, DAYS)


def run_subset(a, days, ranges, ring_days, twi_mean=None, set_days=True, **plan_kw):
    """the streamed plan over `days`, run through the calendar ranges [(day0, ndays)] -> {Tz, soilm} [rows, cols, 24 len(days)]
    gathered from the slots at each day's own place"""
    days = np.asarray(days)
    rows, cols = a["soilc"]["twi"].shape
    got = {k: np.full((rows, cols, 24 * days.size), -1.0, order="F") for k in ("Tz", "soilm")}
    with Plan(**a, ring_days=ring_days, ring_slots=2, stream_below=True, **plan_kw) as st:
        if twi_mean is not None:
            st.set_twi_mean(twi_mean)
        st.set_mxtc(float(np.max(np.asarray(a["climdata"]["temp"])[steps_of(days)])))      # the subset's, as the snow run sets it
        if set_days:
            st.below_set_days(days)
        st.below_prepare()
        slot = 0
        for d0, nd in ranges:
            st.run_days(d0, nd, slot)
            inside = np.flatnonzero((days >= d0) & (days < d0 + nd))
            if inside.size:
                for k in got:
                    v = st.fetch(slot, k, 0, nd * 24)
                    for q in inside:
                        got[k][:, :, q * 24:(q + 1) * 24] = v[:, :, (days[q] - d0) * 24:(days[q] - d0 + 1) * 24]
            slot ^= 1
    return got


def even_ranges(chunk, ndays=NDAYS):
    return [(d, min(chunk, ndays - d)) for d in range(0, ndays, chunk)]


# 1-, 2- and 5-day chunks of the calendar (some hold no day of the subset: days 2-3, 7-8, 10-11 ...), and uneven ones that
# straddle the gaps (one range from day 1 over the gap 2-3 to day 6, one over two gaps)
RANGES = {"1": even_ranges(1), "2": even_ranges(2), "5": even_ranges(5), "straddle": [(0, 1), (1, 6), (7, 7), (14, 1), (15, 5)]}


@pytest.mark.parametrize("complete", [0, 1])
@pytest.mark.parametrize("ranges", list(RANGES))
def test_subset_plan_is_the_whole_series_plan_on_host_subset_inputs(complete, ranges):
    a = case(complete)
    want = whole_series(runmicro1Cpp, **subset_inputs(a, DAYS))
    got = run_subset(a, DAYS, RANGES[ranges], ring_days=7)
    same_bits(got, want)
    valid = ~np.isnan(a["vegp"]["hgt"])
    assert np.isfinite(want["Tz"][valid]).all() and np.isnan(want["Tz"][~valid]).all()


@pytest.mark.parametrize("complete", [0, 1])
def test_layered_vegetation_keeps_its_whole_series_layers(complete):
    """`.runmodel3Cpp` on the subset (R/internal.R:1391-1399): each day keeps the layer the whole series gives it; the
    reference leg gets a dfsel rebuilt on the subset, the plan the whole-series lyr_st / lyr_ed"""
    L = 4
    a = case(complete)
    al = synthetic.layered(a, L)
    dfsel = al.pop("dfsel")
    layer_of_day = np.zeros(NDAYS, int)
    for l in range(L):
        layer_of_day[dfsel["st"][l] // 24:(dfsel["ed"][l] + 1) // 24] = l
    lay = layer_of_day[DAYS]
    assert len(set(lay)) == L
    used, st, ed = [], [], []
    for k, l in enumerate(lay):
        if not used or used[-1] != l:
            used.append(int(l)); st.append(k * 24); ed.append(k * 24 + 23)
        else:
            ed[-1] = k * 24 + 23
    dfs = {"lyr": np.arange(1, len(used) + 1), "st": np.array(st), "ed": np.array(ed)}
    an = subset_inputs(al, DAYS)
    an["vegp"] = {k: np.asfortranarray(v[:, :, used]) for k, v in al["vegp"].items()}
    want = whole_series(runmicro3Cpp, dfs, **an)
    got = run_subset(al, DAYS, RANGES["straddle"], ring_days=7, dfsel=dfsel)
    same_bits(got, want)


@pytest.mark.parametrize("complete", [0, 1])
def test_three_row_blocks(complete):
    """the raster in three row blocks, each a plan of its own with the raster-wide wetness-index mean installed — how the
    multi-device entries run — against the reference leg on the whole raster"""
    rows = ROWS
    a = case(complete)
    want = whole_series(runmicro1Cpp, **subset_inputs(a, DAYS))
    with Plan(**a, ring_days=1) as whole:
        s, n = whole.twi_partial()
    got = {k: np.empty_like(want[k]) for k in ("Tz", "soilm")}
    for r0, r1 in ((0, 7), (7, 15), (15, rows)):
        blk = dict(a, vegp={k: np.asfortranarray(v[r0:r1]) for k, v in a["vegp"].items()},
                   soilc={k: np.asfortranarray(v[r0:r1]) for k, v in a["soilc"].items()})
        g = run_subset(blk, DAYS, RANGES["5"], ring_days=5, twi_mean=s / n)
        for k in got:
            got[k][r0:r1] = g[k]
    same_bits(got, want)


@pytest.mark.parametrize("complete", [0, 1])
def test_the_full_day_list_is_the_plan_without_a_subset(complete):
    a = case(complete)          # (on all 20 days the same soils and depth span the two upper regimes)
    every = np.arange(NDAYS)
    plain = run_subset(a, every, even_ranges(3), ring_days=3, set_days=False)
    listed = run_subset(a, every, even_ranges(3), ring_days=3)
    same_bits(listed, plain)
    same_bits(listed, whole_series(runmicro1Cpp, **a))


def test_refusals():
    a = with_na(synthetic.workload(12, 7, T, reqhgt=-0.2, variety=True, start_doy=140, out=OUT))
    with Plan(**a, ring_days=5, stream_below=True) as st:
        for bad, why in (([3, 2, 5], "strictly ascending"), ([2, 2, 5], "strictly ascending"), ([0, NDAYS], "out of range"),
                         ([-1, 4], "out of range"), ([], "no days")):
            with pytest.raises(McfError, match=why):
                st.below_set_days(bad)
        st.below_set_days(DAYS)
        with pytest.raises(McfError, match="mcf_plan_below_prepare"):
            st.run_days(0, 2, 0)
        st.below_prepare()
        with pytest.raises(McfError, match="before mcf_plan_below_prepare"):
            st.below_set_days(DAYS)
        st.run_days(0, 2, 0)              # positions 0, 1
        st.run_days(2, 2, 0)              # days 2, 3: none of the subset's — nothing happens, the order stands
        with pytest.raises(McfError, match="day order"):
            st.run_days(9, 4, 0)          # position 5 (day 9): leaves out days 4, 5, 6
        with pytest.raises(McfError, match="day order"):
            st.run_days(1, 1, 0)          # goes back to position 1
        st.run_days(4, 5, 0)              # positions 2 .. 4 (days 4, 5, 6)
        st.run_days(9, 4, 0)              # positions 5, 6 (days 9, 12)
        st.run_days(0, 1, 0)              # the subset's first day starts a new pass
        with pytest.raises(McfError, match="day offset"):
            st.run_days_at(1, 1, 0, 1)
        with pytest.raises(McfError, match="ring slot holds"):
            st.run_days(1, 6, 0)
    with Plan(**a, ring_days=1) as whole:                                       # not a streamed plan
        with pytest.raises(McfError, match="streamed plan"):
            whole.below_set_days(DAYS)
    with Plan(**dict(a, reqhgt=0.05), ring_days=1, stream_below=True) as above:   # reqhgt >= 0: mcf_plan_create
        with pytest.raises(McfError, match="reqhgt < 0"):
            above.below_set_days(DAYS)
    af = synthetic.workload(12, 7, T, reqhgt=-0.2, variety=True, start_doy=140, out=OUT, array_forcing=True)
    with Plan(**af, array_forcing=True, ring_days=5, stream_below=True) as st:
        with pytest.raises(McfError, match="vector forcing"):
            st.below_set_days(DAYS)
