"""The snow run below ground (include/mcf.h mcf_runmicrosnow1_below / mcf_runmicrosnow1_below_multi / mcf_snowrun_create_below):
`runmicro(..., snow = TRUE)` with reqhgt < 0 as one device-resident call.  `.runmicrosnow1` (R/internal.R:3581-3659) runs the
grid solver — Tbelowgroundv included — on the subset series of the no-snow days, gridmicrosnow1 with `out[c(1, 4)]` on the
snow days, and merges by day.  Held against
  (1) that orchestration on the host with HIP behind it (runmicro1Cpp on the host-subset inputs with the whole-series
      below-ground plan, gridmicrosnow1, merge_snow_outputs): Tz and soilm bit for bit, every other output 1e-12;
  (2) the same with the oracle's solver, snow microclimate and merge: 1e-6, all ten outputs, every cell-step, equal NaN masks;
for complete 0 and 1, a depth in the daily-mean regime of manCpp's window and deeper and shallower ones, time-varying
vegetation, row blocks, a deep pack (no tile may be left out below ground), a year without snow, a year without a no-snow
day, and the refusals."""
import os

import numpy as np
import pytest

from microclimf_amd import snow as S
from microclimf_amd import synthetic
from microclimf_amd.api import runmicro1Cpp, runmicro3Cpp

pytestmark = pytest.mark.gpu
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact",
        "complete", "mat", "out")
MAT = 7.5
OUTM = [1, 0, 0, 1, 0, 0, 0, 0, 0, 0]       # `out[c(1, 4)]`, R/internal.R:3621-3624
OMDY = 2 * np.pi / (24 * 3600.0)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def whole_series(fn, *args, **kw):
    """fn with the whole-series below-ground plan (MCF_BELOW_STREAM=0): the route the parent of this feature had"""
    old = os.environ.get("MCF_BELOW_STREAM")
    os.environ["MCF_BELOW_STREAM"] = "0"
    try:
        return fn(*args, **kw)
    finally:
        if old is None:
            del os.environ["MCF_BELOW_STREAM"]
        else:
            os.environ["MCF_BELOW_STREAM"] = old


def _steps(days0):
    return (np.repeat(np.asarray(days0) * 24, 24) + np.tile(np.arange(24), len(days0))).astype(np.int64)


def _sub(d, idx):
    return {k: (np.asarray(v)[idx] if np.ndim(v) == 1 else v) for k, v in d.items()}


def _case(reqhgt, cold, doy, rows=22, cols=13, ndays=20, complete=True):
    T = ndays * 24
    sw = synthetic.snow_workload(rows, cols, T, cold=cold, zref=3.5, start_doy=doy)
    a = synthetic.workload(rows, cols, T, reqhgt=reqhgt, zref=3.5, hgt_range=(0.05, 3.0), start_doy=doy, variety=True,
                           complete=bool(complete))
    _, _, dtm = synthetic.rasters(rows, cols)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    return sw, a, dtm, snow, micro


def _orchestrate(a, sw, dtm, smod, sdays, ndays_, reqhgt, solve, microsnow, oracle_merge=False):
    """`.runmicrosnow1` steps (3)-(5) on host arrays for reqhgt < 0: `solve(args of the no-snow-day subset)`, `microsnow(...)`
    on the snow-day subset with `out[c(1, 4)]`, the merge (oracle_merge: oracle/snowmerge_oracle.py's)"""
    rows, cols = dtm.shape
    ni, si = _steps(ndays_), _steps(sdays)
    an = dict(a, obstime=_sub(a["obstime"], ni), climdata=_sub(a["climdata"], ni), pointm=_sub(a["pointm"], ni))
    moutn = solve(an)
    micro = {}
    if oracle_merge:
        from oracle import snowmerge_oracle as MO
        micro = MO.prep_micro(moutn, sdays + 1, ndays_ + 1, rows, cols)
    else:
        s1 = np.arange(si.size)[np.repeat(np.isin(sdays, ndays_), 24)]
        s2 = np.arange(ni.size)[np.repeat(np.isin(ndays_, sdays), 24)]
        for k, v in moutn.items():
            m = np.full((rows, cols, si.size), np.nan, order="F")
            m[:, :, s1] = v[:, :, s2]
            micro[k] = m
    swe = smod["totalSWE"].copy()
    swe[np.isnan(swe)] = 0.0
    swe[np.isnan(dtm)] = np.nan
    smods = {k: np.asfortranarray((swe if k == "totalSWE" else v)[:, :, si]) for k, v in smod.items()}
    mouts = microsnow(reqhgt, _sub(sw["obstime"], si), _sub(sw["climdata"], si), smods, micro, sw["vegp"], sw["other"], MAT, OUTM)
    for k in moutn:
        if k not in mouts:
            mouts[k] = micro[k]
    if oracle_merge:
        return MO.merge(moutn, mouts, sdays + 1, ndays_ + 1, rows, cols)
    return S.merge_snow_outputs(moutn, mouts, sdays + 1, ndays_ + 1, rows, cols)


def _close(got, want, tol, what, exact=()):
    """identical NaN masks and `tol` relative on every variable; the variables in `exact` bit for bit wherever they hold a
    number.  (Not the NaN payloads: the host legs' blank template and merge are numpy's — np.nan, 0x7FF8000000000000 — where
    the library writes R's NA_real_, payload 1954; the masks are compared, and the payloads of the library's own two routes
    in _same.)"""
    assert list(got) == list(want)
    for k in want:
        g, w = got[k], want[k]
        assert g.shape == w.shape, (what, k)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
        fin = np.isfinite(w)
        err = float(np.max(np.abs(g[fin] - w[fin]) / (1 + np.abs(w[fin])))) if fin.any() else 0.0
        nbits = int((bits(g) != bits(w))[~np.isnan(w)].sum())
        print(f"{what}: {k}: max rel err {err:.3e}, {nbits} of {g.size} values differ in their bits")
        assert err < tol, (what, k, err)
        if k in exact:
            assert nbits == 0, (what, k, nbits, err)


def _same(got, want, what=""):
    assert list(got) == list(want)
    for k in want:
        assert (bits(got[k]) == bits(want[k])).all(), (what, k)


def approx_n(a, tsteps):
    """manCpp's window length n per cell, from a numpy transcription of the soil damping depth (cpp:1021-1032, 1249-1260) over
    the soil-moisture series of `a` (tsteps steps)"""
    s = a["soilc"]
    twi = s["twi"]
    tadd = np.log(twi) / a["tfact"] - np.nanmean(np.log(twi) / a["tfact"])
    sm_p = np.asarray(a["pointm"]["soilm"])[None, None, :tsteps]
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


def _day_classes(smod, dtm):
    swe = smod["totalSWE"].copy()
    swe[np.isnan(swe)] = 0.0
    swe[np.isnan(dtm)] = np.nan
    days = S.snowdaysfun(S.applycpp3(swe, "max"), S.applycpp3(swe, "min"))
    return swe, days["snowdays"], days["nosnowdays"]


def _hip_solver(an):
    return whole_series(runmicro1Cpp, *[an[k] for k in ARGS])


# reqhgt: -0.1 and -0.5 (on this site n ~ 130 .. 180 and ~ 650 .. 900: the daily-mean window and the series mean of the
# no-snow days' 200-odd steps), and -0.02 (n ~ 30: the hourly window, whose 47 steps reach back across the gaps of the calendar)
@pytest.mark.parametrize("complete", [1, 0])
@pytest.mark.parametrize("reqhgt", [-0.1, -0.5, -0.02])
def test_one_call_equals_the_host_orchestration_and_the_oracle_backed_one(oracle, reqhgt, complete):
    cold, doy = 0.0, 90
    sw, a, dtm, snow, micro = _case(reqhgt, cold, doy, complete=complete)
    got, smod = S.runmicrosnow1(a, snow, micro, MAT, want_smod=True, below=True)
    want_smod = S.snowmodel1_chunks(sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
    for k in smod:
        assert (bits(smod[k]) == bits(want_smod[k])).all(), k
    with S.SnowRun(a, snow, below=True) as run:
        sd, nd = run.pass1()
        got2 = run.pass2(micro, MAT)
        st = run.stats()
    _same(got2, got, "staged")
    assert st["tile_days_left_out"] == 0, st
    swe, sd_w, nd_w = _day_classes(smod, dtm)
    assert np.array_equal(sd, sd_w) and np.array_equal(nd, nd_w)
    sdays, ndays_ = np.flatnonzero(sd), np.flatnonzero(nd)
    assert sdays.size >= 3 and ndays_.size >= 3 and (sd & nd).sum() >= 1 and (sd | nd).all()
    assert np.setdiff1d(ndays_, sdays).size > 0 and np.setdiff1d(sdays, ndays_).size > 0       # days of one class only, both ways
    si = _steps(sdays)
    covered = swe[:, :, si] > 0
    assert covered.any() and (~covered & ~np.isnan(dtm)[:, :, None]).any()
    # the window regime of the solver's cells on the no-snow days' series (m steps)
    m = 24 * ndays_.size
    n = approx_n(dict(a, pointm=_sub(a["pointm"], _steps(ndays_))), m)
    n = n[~np.isnan(a["vegp"]["hgt"])]
    if reqhgt == -0.1:
        assert ((n >= 53) & (n <= m - 5)).any(), (n.min(), n.max(), m)
    elif reqhgt == -0.5:
        assert (n >= m + 5).all(), (n.min(), m)
    else:
        assert (n <= 44).all(), n.max()
    # (1) the reference's orchestration on the host, HIP behind it: the solver's Tz and soilm are the whole-series plan's bits on
    # the subset inputs, the snow-day model's the one-shot kernel's on the same operands
    want = _orchestrate(a, sw, dtm, smod, sdays, ndays_, reqhgt, _hip_solver, S.gridmicrosnow1)
    _close(got, want, 1e-12, "host-orchestrated HIP", exact=("Tz", "soilm"))
    # (2) ... and with the oracle's solver, snow microclimate and merge behind it
    want_o = _orchestrate(a, sw, dtm, smod, sdays, ndays_, reqhgt, lambda an: oracle.run_grid(**{k: an[k] for k in ARGS}),
                          oracle.run_microsnow, oracle_merge=True)
    _close(got, want_o, 1e-6, "oracle-backed orchestration")
    # on a snow-only day everything but Tz and soilm is NA
    only_s = np.setdiff1d(sdays, ndays_)
    assert np.isnan(got["relhum"][:, :, _steps(only_s)]).all()


def _subset_dfsel(layer_of_day, days0):
    """`.runmodel3Cpp` on a day subset (R/internal.R:1391-1399): the subset's days keep the layer the whole series gives them,
    consecutive days of one layer form one row of dfsel, the layers are renumbered 1.. in order — st / ed are step positions
    IN THE SUBSET.  -> (dfsel, the whole-series layers used, in order)"""
    lay = [int(layer_of_day[d]) for d in days0]
    used, st, ed = [], [], []
    for k, l in enumerate(lay):
        if not used or used[-1] != l:
            used.append(l); st.append(k * 24); ed.append(k * 24 + 23)
        else:
            ed[-1] = k * 24 + 23
    return {"lyr": np.arange(1, len(used) + 1), "st": np.array(st), "ed": np.array(ed)}, used


@pytest.mark.parametrize("complete", [1, 0])
def test_time_varying_vegetation_runs_on_the_no_snow_days_with_the_whole_series_layers(oracle, complete):
    reqhgt, L = -0.1, 4
    sw, a, dtm, snow, micro = _case(reqhgt, 0.0, 90, complete=complete)
    al = synthetic.layered(a, L)
    ndays = len(a["obstime"]["year"]) // 24
    layer_of_day = np.zeros(ndays, int)
    for l in range(L):
        layer_of_day[al["dfsel"]["st"][l] // 24:(al["dfsel"]["ed"][l] + 1) // 24] = l
    got, smod = S.runmicrosnow1(al, snow, micro, MAT, want_smod=True, below=True)
    _, sd, nd = _day_classes(smod, dtm)
    sdays, ndays_ = np.flatnonzero(sd), np.flatnonzero(nd)
    assert len(set(layer_of_day[ndays_])) >= 3          # the no-snow days span several layers
    dfs, used = _subset_dfsel(layer_of_day, ndays_)
    veg_sub = {k: np.asfortranarray(v[:, :, used]) for k, v in al["vegp"].items()}

    def solve_with(fn):
        return lambda an: fn(dfs, dict(an, vegp=veg_sub))
    want = _orchestrate(a, sw, dtm, smod, sdays, ndays_, reqhgt,
                        solve_with(lambda d, an: whole_series(runmicro3Cpp, d, *[an[k] for k in ARGS])), S.gridmicrosnow1)
    _close(got, want, 1e-12, "host-orchestrated HIP, layered", exact=("Tz", "soilm"))
    want_o = _orchestrate(a, sw, dtm, smod, sdays, ndays_, reqhgt,
                          solve_with(lambda d, an: oracle.run_grid(**{k: an[k] for k in ARGS}, dfsel=d)), oracle.run_microsnow,
                          oracle_merge=True)
    _close(got, want_o, 1e-6, "oracle-backed orchestration, layered")
    flat = S.runmicrosnow1(a, snow, micro, MAT, below=True)
    assert np.nanmax(np.abs(flat["Tz"] - got["Tz"])) > 1e-3          # and the layers matter


@pytest.mark.parametrize("complete", [1, 0])
def test_row_blocks_and_host_threads(complete):
    sw, a, dtm, snow, micro = _case(-0.1, 0.0, 90, rows=320, cols=24, ndays=10, complete=complete)
    one = S.runmicrosnow1(a, snow, micro, MAT, below=True)
    same = S.runmicrosnow1(a, snow, micro, MAT, devices=[0], n_blocks=1, below=True)
    _same(same, one, "one block")
    for devices, nb in (([0], 2), ([0, 0], 2)):                               # blocks > devices; two host threads on one device
        multi = S.runmicrosnow1(a, snow, micro, MAT, devices=devices, n_blocks=nb, below=True)
        _close(multi, one, 1e-9, f"{nb} blocks on {devices}")


@pytest.mark.parametrize("complete", [1, 0])
def test_under_a_deep_pack_every_cell_is_still_solved(oracle, complete):
    """A deep pack everywhere but on the northern rows, no snowfall: every day is a snow day and a no-snow day.  Above ground
    pass 2 leaves the tiles inside the pack out; below ground a cell's ground temperature on a no-snow day feeds its running
    means on later days whether or not it lies under snow, so every tile is solved — as the reference does."""
    reqhgt, rows, cols, ndays = -0.1, 64, 24, 10
    sw, a, dtm, snow, micro = _case(reqhgt, -2.0, 60, rows=rows, cols=cols, ndays=ndays, complete=complete)
    deep = np.asfortranarray(np.where(np.arange(rows)[:, None] >= 9, 0.9, 0.0) * np.ones((1, cols)))
    other = dict(sw["other"], isnowdc=deep, isnowdg=np.asfortranarray(0.7 * deep))
    clim = dict(sw["climdata"], precip=np.zeros(ndays * 24))
    sw = dict(sw, other=other, climdata=clim)
    snow = dict(snow, other=other, climdata=clim)
    micro = dict(micro, other=other, climdata=clim)
    with S.SnowRun(a, snow, below=True) as run:
        sd, nd, smod = run.pass1(want_smod=True)
        got = run.pass2(micro, MAT)
        st = run.stats()
    assert (sd & nd).sum() >= 5 and st["tile_days"] >= 20 and st["tile_days_left_out"] == 0, (sd, nd, st)
    sdays, ndays_ = np.flatnonzero(sd), np.flatnonzero(nd)
    want = _orchestrate(a, sw, dtm, smod, sdays, ndays_, reqhgt, _hip_solver, S.gridmicrosnow1)
    _close(got, want, 1e-12, "host-orchestrated HIP", exact=("Tz", "soilm"))
    want_o = _orchestrate(a, sw, dtm, smod, sdays, ndays_, reqhgt, lambda an: oracle.run_grid(**{k: an[k] for k in ARGS}),
                          oracle.run_microsnow, oracle_merge=True)
    _close(got, want_o, 1e-6, "oracle-backed orchestration")


@pytest.mark.parametrize("complete", [1, 0])
def test_a_year_without_snow_is_the_solver_alone(complete):
    sw, a, dtm, snow, micro = _case(-0.1, -25.0, 170, rows=10, cols=9, ndays=7, complete=complete)   # midsummer, 25 K warmer
    snow["other"] = dict(snow["other"], isnowdc=np.zeros_like(dtm), isnowdg=np.zeros_like(dtm))
    with S.SnowRun(a, snow, below=True) as run:
        sd, nd = run.pass1()
        assert not sd.any() and nd.all()
        got = run.pass2(None, MAT)                     # no snow day: gridmicrosnow1's inputs are not needed
    _same(got, whole_series(runmicro1Cpp, *[a[k] for k in ARGS]), "no snow")


def test_a_year_without_a_no_snow_day_is_the_template_and_the_snow_days(oracle):
    """a deep pack on every cell, hard frost, no NA cell without snow: no day has a snow-free cell — the solver never runs, Tz
    and soilm are gridmicrosnow1's on the blank template, everything else is NA"""
    reqhgt, rows, cols, ndays = -0.1, 12, 9, 10
    sw, a, dtm, snow, micro = _case(reqhgt, 8.0, 20, rows=rows, cols=cols, ndays=ndays)
    deep = np.asfortranarray(np.full((rows, cols), 0.9))
    other = dict(sw["other"], isnowdc=deep, isnowdg=np.asfortranarray(0.7 * deep))
    sw = dict(sw, other=other)
    snow = dict(snow, other=other)
    micro = dict(micro, other=other)
    with S.SnowRun(a, snow, below=True) as run:
        sd, nd, smod = run.pass1(want_smod=True)
        assert sd.all() and not nd.any(), (sd, nd)
        got = run.pass2(micro, MAT)
    swe, _, _ = _day_classes(smod, dtm)
    blank = {k: np.full((rows, cols, ndays * 24), np.nan, order="F") for k in got}
    want = S.gridmicrosnow1(reqhgt, sw["obstime"], sw["climdata"], dict(smod, totalSWE=swe), blank, sw["vegp"], sw["other"], MAT, OUTM)
    for k in got:
        w = want.get(k, blank[k])
        assert np.array_equal(np.isnan(got[k]), np.isnan(w)), k
        num = ~np.isnan(w)          # (the blank template here is numpy's NaN, the library's R's NA_real_: see _close)
        assert (bits(got[k]) == bits(w))[num].all() if k in ("Tz", "soilm") else np.isnan(got[k]).all(), k
    assert np.isfinite(got["Tz"]).any()
    blank_o = {k: np.full((rows, cols, ndays * 24), np.nan, order="F") for k in got}
    want_o = oracle.run_microsnow(reqhgt, sw["obstime"], sw["climdata"], dict(smod, totalSWE=swe), blank_o, sw["vegp"], sw["other"], MAT,
                                  OUTM)
    for k in ("Tz", "soilm"):
        w = want_o[k]
        assert np.array_equal(np.isnan(got[k]), np.isnan(w)), k
        fin = np.isfinite(w)
        assert np.max(np.abs(got[k][fin] - w[fin]) / (1 + np.abs(w[fin]))) < 1e-6, k


def test_refusals():
    sw, a, dtm, snow, micro = _case(-0.1, 0.0, 90, rows=10, cols=9, ndays=5)
    # the entries as they were keep refusing reqhgt < 0 ...
    with pytest.raises(Exception, match="reqhgt < 0"):
        S.runmicrosnow1(a, snow, micro, MAT)
    with pytest.raises(Exception, match="reqhgt < 0"):
        S.SnowRun(a, snow)
    with pytest.raises(Exception, match="reqhgt < 0"):
        S.runmicrosnow1(a, snow, micro, MAT, devices=[0], n_blocks=2)
    # ... and the below-ground ones reqhgt >= 0
    for rq in (0.0, 0.05):
        with pytest.raises(Exception, match="need reqhgt < 0"):
            S.runmicrosnow1(dict(a, reqhgt=rq), snow, micro, MAT, below=True)
        with pytest.raises(Exception, match="need reqhgt < 0"):
            S.SnowRun(dict(a, reqhgt=rq), snow, below=True)
    with pytest.raises(Exception, match="need reqhgt < 0"):
        S.runmicrosnow1(dict(a, reqhgt=0.05), snow, micro, MAT, devices=[0], n_blocks=2, below=True)
    # one period per handle
    with S.SnowRun(a, snow, below=True) as run:
        with pytest.raises(Exception, match="pass1 first"):
            run.pass2(micro, MAT)
        run.pass1()
        run.pass2(micro, MAT)
        run.pass1()
        with pytest.raises(Exception, match="before mcf_plan_below_prepare"):
            run.pass2(micro, MAT)


def test_array_weather_below_ground_is_refused():
    from microclimf_amd import _abi
    import ctypes as C
    sw, a, dtm, snow, micro = _case(-0.1, 0.0, 90, rows=10, cols=9, ndays=5)
    with S.SnowRun(a, snow, handle=False) as run:
        run._gm.inputs.array_forcing = 1          # (checked before any array is read)
        run._din.base.array_forcing = 1
        p = C.c_void_p()
        rc = _abi.load().mcf_snowrun_create_below(C.byref(run._in), C.byref(run._gm.options), None, C.byref(p))
        assert rc != 0 and b"array weather below ground is not supported" in _abi.load().mcf_last_error()


@pytest.mark.parametrize("out", [[1] * 10, [1, 0, 0, 1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1, 0, 0], [0, 1, 0, 1, 1, 0, 0, 0, 0, 0]])
def test_the_below_ground_instantiation_of_the_snow_day_kernel_is_the_generic_one(out):
    """k_microsnow_tiles<BELOW> (no direction planes, no step table, Tz and soilm alone through the whole-line store path)
    against the generic instantiation (MCF_MICROSNOW_GENERIC, read at every launch) on the same slots: every held variable bit
    for bit, NaN payloads included — days of each class, NA cells, snow-free cell-steps, any set of held variables"""
    sw, a, dtm, snow, micro = _case(-0.1, 0.0, 90)
    a = dict(a, out=out)
    assert "MCF_MICROSNOW_GENERIC" not in os.environ
    lean = S.runmicrosnow1(a, snow, micro, MAT, below=True)
    os.environ["MCF_MICROSNOW_GENERIC"] = "1"
    try:
        generic = S.runmicrosnow1(a, snow, micro, MAT, below=True)
    finally:
        del os.environ["MCF_MICROSNOW_GENERIC"]
    _same(lean, generic, "lean vs generic")
    assert any(np.isfinite(v).any() and np.isnan(v).any() for v in lean.values())
