"""Plans and one-shot solves that take the dtm (include/mcf.h mcf_plan_create_dtm / mcf_runmicro_dtm): the terrain planes
and the wetness index derived on the device into the plan's own buffers, against the host-array route — mcf_precompute_terrain,
the masking of frontend.prepare_grid_inputs, topidx — which they must equal bit for bit."""
import numpy as np
import pytest

from microclimf_amd import _abi, api, synthetic
from microclimf_amd import frontend as F
from microclimf_amd.terrain import precompute_terrain, topidx
from test_terrain_cpu import synth_dtm

pytestmark = pytest.mark.gpu

R, C, RES = 40, 30, 5.0
SIX = api.DTM_DERIVED


def the_dtm(rows=R, cols=C):
    z = synth_dtm(rows, cols)
    z[7, 9] = z[rows - 6, 4] = np.nan
    z[11:14, 20:22] = np.nan
    z[:, cols - 1] = np.nan                                 # an NA column at the edge
    return np.asfortranarray(z)


def host_planes(z, res, zref, twi=None, **placement):
    """what the host-array route feeds the solver: frontend.prepare_grid_inputs' terrain block"""
    hn, hs = placement.get("halo_north", 0), placement.get("halo_south", 0)
    own = z[hn:z.shape[0] - hs]
    t = precompute_terrain(z, res, zref, **placement)
    na = np.isnan(own)
    out = {"hor": t["hor"], "svfa": t["svfa"], "wsa": t["wsa"]}
    for k in ("slope", "aspect"):
        a = t[k].copy()
        a[np.isnan(a)] = 0.0
        a[na] = np.nan
        out[k] = a
    if twi is not None:
        out["twi"] = twi
    return out


def workload(tsteps=48, rows=R, cols=C, **kw):
    a = synthetic.workload(rows, cols, tsteps, variety=True, start_doy=170, **kw)
    a["soilc"] = dict(a["soilc"])
    return a


def dtm_na_where_vegetation_is(a, rows, cols):
    """Elevations that are NA exactly where the vegetation is.  The row-block comparisons below want it: a valid cell with an NA
    slope is an irregular one for the solver's clamp dispatch, which then sends its whole tile through the reference-form
    variant, and the tiles of a row block are not the tiles of the whole raster — the two variants agree to rounding, not to
    the bit, with host arrays just the same (the existing row-block tests have no such cells either)."""
    z = synth_dtm(rows, cols)
    z[np.isnan(a["vegp"]["hgt"])] = np.nan
    assert np.isnan(z).sum() >= 3
    return np.asfortranarray(z)


def without(a, keys):
    b = dict(a)
    b["soilc"] = {k: v for k, v in a["soilc"].items() if k not in keys}
    return b


def with_planes(a, planes):
    b = dict(a)
    b["soilc"] = {**a["soilc"], **planes}
    return b


def same(got, want):
    assert list(got) == list(want)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, float(np.nanmax(np.abs(got[k] - want[k]))))


def test_terrain_planes_derived_twi_supplied():
    a, z = workload(), the_dtm()
    want = api.runmicro1Cpp(**with_planes(a, host_planes(z, RES, a["zref"])))
    got = api.runmicro1Cpp(**without(a, set(SIX) - {"twi"}), dtm={"z": z, "res": RES})
    same(got, want)
    assert np.isfinite(want["Tz"]).any()


def test_twi_derived_too():
    a, z = workload(), the_dtm()
    twi = topidx(z, RES, device=0)
    want = api.runmicro1Cpp(**with_planes(a, host_planes(z, RES, a["zref"], twi)))
    same(api.runmicro1Cpp(**without(a, SIX), dtm={"z": z, "res": RES}), want)
    # ... and with rectangular cells when only twi is missing
    planes = host_planes(z, RES, a["zref"])
    twi = topidx(z, (2.0, 5.0), device=0)
    want = api.runmicro1Cpp(**with_planes(a, {**planes, "twi": twi}))
    same(api.runmicro1Cpp(**without(with_planes(a, planes), {"twi"}), dtm={"z": z, "res": (2.0, 5.0)}), want)


@pytest.mark.parametrize("given", ["slope", "aspect", "hor", "svfa", "wsa", "twi"])
def test_one_plane_supplied_the_others_derived(given):
    a, z = workload(24), the_dtm()
    planes = host_planes(z, RES, a["zref"], topidx(z, RES, device=0))
    rng = np.random.default_rng(3)
    mine = planes[given] * rng.uniform(0.9, 1.0, planes[given].shape)         # not what the dtm gives
    if given == "hor":
        # svfa then comes from the supplied hor (R/internal.R:1146-1149): the numpy formula, to the bar tests/test_terrain_gpu.py
        # holds the terrain kernels to
        svfa = 0.5 * np.cos(2 * np.tan(np.mean(np.arctan(mine), axis=2))) + 0.5
        want = api.runmicro1Cpp(**with_planes(a, {**planes, "hor": mine, "svfa": svfa}))
        got = api.runmicro1Cpp(**with_planes(without(a, SIX), {"hor": mine}), dtm={"z": z, "res": RES})
        assert list(got) == list(want)
        for k in want:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
            # the outputs are smooth in svfa (it weights the diffuse and long-wave terms): a 1e-10 change of svfa moves an
            # output by at most 1e-10 of its own size
            err = np.nanmax(np.abs(got[k] - want[k]) / (1.0 + np.abs(want[k])))
            print(f"hor supplied, svfa derived: {k} max scaled difference {err:.3e}")
            assert err <= 1e-10, k
        return
    want = api.runmicro1Cpp(**with_planes(a, {**planes, given: mine}))
    same(api.runmicro1Cpp(**with_planes(without(a, SIX), {given: mine}), dtm={"z": z, "res": RES}), want)


def test_hor_and_svfa_both_supplied_are_used_as_given():
    a, z = workload(24), the_dtm()
    planes = host_planes(z, RES, a["zref"], topidx(z, RES, device=0))
    mine = {"hor": planes["hor"] * 0.9, "svfa": planes["svfa"] * 0.95}
    want = api.runmicro1Cpp(**with_planes(a, {**planes, **mine}))
    same(api.runmicro1Cpp(**with_planes(without(a, SIX), mine), dtm={"z": z, "res": RES}), want)


@pytest.mark.parametrize("reqhgt", [0.05, 0.0, -0.1])
def test_heights(reqhgt):
    out = [1] * 10 if reqhgt > 0 else [1, 0, 0, 1, 0, 1, 1, 1, 1, 1] if reqhgt == 0 else [1, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    a, z = workload(72, reqhgt=reqhgt, out=out), the_dtm()
    want = api.runmicro1Cpp(**with_planes(a, host_planes(z, RES, a["zref"], topidx(z, RES, device=0))))
    same(api.runmicro1Cpp(**without(a, SIX), dtm={"z": z, "res": RES}), want)


def test_below_ground_streamed(monkeypatch):
    """mcf_runmicro_dtm chooses between the whole-series and the streamed plan as the one-shot entries do"""
    a, z = workload(72, reqhgt=-0.1, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0]), the_dtm()
    want = api.runmicro1Cpp(**without(a, SIX), dtm={"z": z, "res": RES})
    monkeypatch.setenv("MCF_BELOW_STREAM", "1")
    same(api.runmicro1Cpp(**without(a, SIX), dtm={"z": z, "res": RES}, days_per_chunk=2), want)


def test_array_forcing():
    a, z = workload(48, array_forcing=True), the_dtm()
    a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
    want = api.runmicro2Cpp(**with_planes(a, host_planes(z, RES, a["zref"], topidx(z, RES, device=0))))
    same(api.runmicro2Cpp(**without(a, SIX), dtm={"z": z, "res": RES}), want)


def test_layered_vegetation():
    a, z = workload(24 * 4), the_dtm()
    a = synthetic.layered(a, 3)
    dfsel = a.pop("dfsel")
    a["soilc"] = dict(a["soilc"])
    want = api.runmicro3Cpp(dfsel, **with_planes(a, host_planes(z, RES, a["zref"], topidx(z, RES, device=0))))
    same(api.runmicro3Cpp(dfsel, **without(a, SIX), dtm={"z": z, "res": RES}), want)


def run_plan(p):
    p.run_days(0, 1)
    p.sync()
    return {k: p.fetch(0, k, 0, 24) for k in _abi.OUT_NAMES}


def test_plan_for_a_row_block_with_halos():
    rows_total, cols, r0, r1, halo = 330, 12, 130, 200, 128
    whole = workload(24, rows=rows_total, cols=cols)
    z = dtm_na_where_vegetation_is(whole, rows_total, cols)
    with api.Plan(**without(whole, set(SIX) - {"twi"}), dtm={"z": z, "res": RES}) as p:
        s, n = p.twi_partial()
        want = {k: v[r0:r1] for k, v in run_plan(p).items()}
    blk = dict(whole)
    blk["vegp"] = {k: np.asfortranarray(v[r0:r1]) for k, v in whole["vegp"].items()}
    blk["soilc"] = {k: np.asfortranarray(v[r0:r1]) for k, v in whole["soilc"].items()}
    hn, hs = min(halo, r0), min(halo, rows_total - r1)
    place = dict(halo_north=hn, halo_south=hs, row0=r0, rows_total=rows_total)
    zb = np.asfortranarray(z[r0 - hn:r1 + hs])
    with api.Plan(**without(blk, set(SIX) - {"twi"}), dtm={"z": zb, "res": RES, **place}) as p:
        nbytes = p.device_bytes
        p.set_twi_mean(s / n)
        got = run_plan(p)
    same(got, want)
    # nothing of the dtm or of the scratch stays with the plan
    with api.Plan(**with_planes(blk, host_planes(zb, RES, blk["zref"], **place))) as p:
        assert p.device_bytes == nbytes
        p.set_twi_mean(s / n)
        same(run_plan(p), want)


def test_row_blocks_over_the_device_list():
    a = workload(48, rows=90)
    z = dtm_na_where_vegetation_is(a, 90, C)
    want = api.runmicro1Cpp(**without(a, SIX), dtm={"z": z, "res": RES})
    same(api.runmicro1Cpp(**without(a, SIX), dtm={"z": z, "res": RES}, devices=[0], n_blocks=3), want)
    # ... with hor supplied: a block's svfa from its rows of it
    hor = host_planes(z, RES, a["zref"])["hor"] * 0.9
    b = with_planes(without(a, SIX), {"hor": hor})
    same(api.runmicro1Cpp(**b, dtm={"z": z, "res": RES}, devices=[0], n_blocks=3), api.runmicro1Cpp(**b, dtm={"z": z, "res": RES}))


def test_errors():
    a, z = workload(24), the_dtm()
    with pytest.raises(_abi.McfError, match="square cells"):
        api.runmicro1Cpp(**without(a, SIX), dtm={"z": z, "res": (2.0, 5.0)})
    blk = dict(a)
    blk["vegp"] = {k: np.asfortranarray(v[10:30]) for k, v in a["vegp"].items()}
    blk["soilc"] = {k: np.asfortranarray(v[10:30]) for k, v in a["soilc"].items()}
    place = dict(halo_north=10, halo_south=10, row0=10, rows_total=R)
    with pytest.raises(_abi.McfError, match="does not tile"):
        api.Plan(**without(blk, SIX), dtm={"z": z, "res": RES, **place})
    with pytest.raises(_abi.McfError, match="halo rows"):
        api.Plan(**without(blk, set(SIX) - {"twi"}), dtm={"z": np.asfortranarray(z[5:35]), "res": RES, "halo_north": 5, "halo_south": 5,
                                                         "row0": 10, "rows_total": R})
    with pytest.raises(_abi.McfError, match="whole raster"):
        api.runmicro1Cpp(**without(blk, set(SIX) - {"twi"}), dtm={"z": z, "res": RES, **place}, devices=[0], n_blocks=2)
    with pytest.raises(ValueError, match="dtm\\$z"):
        api.runmicro1Cpp(**without(a, SIX), dtm={"z": z[1:], "res": RES})


# Largest |from_dtm=True - from_dtm=False| per output on the bundled site, 30 days (profiles/r07_plan_from_dtm.txt): the two
# routes differ only in the wetness index's last bits (atan / tan on the device against libm).  The bar is ten times the
# measured figure, capped at the 1e-6 the parity tests hold the GPU to against the oracle.
FROM_DTM_MEASURED = {"Tz": 1.776e-15, "tleaf": 1.776e-15, "relhum": 7.105e-14, "soilm": 1.110e-16, "windspeed": 0.0, "Rdirdown": 0.0,
                     "Rdifdown": 0.0, "Rlwdown": 0.0, "Rswup": 0.0, "Rlwup": 0.0}


def test_frontend_from_dtm_on_the_bundled_site():
    from bundled import load
    weather, vegp, soilc, dtm = load(30 * 24)
    mp = F.runpointmodel(weather, 0.05, dtm, vegp, soilc)
    want = F.runmicro(mp, 0.05, vegp, soilc, dtm)
    got = F.runmicro(mp, 0.05, vegp, soilc, dtm, from_dtm=True)
    assert list(got) == list(want)
    worst = {}
    for k in want:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        worst[k] = float(np.nanmax(np.abs(got[k] - want[k])))
        print(f"from_dtm: {k} max |difference| {worst[k]:.3e}")
    for k in want:
        assert worst[k] <= min(10.0 * FROM_DTM_MEASURED[k], 1e-6), (k, worst[k])
    # with every plane given there is nothing to derive: the same bits
    a = F.prepare_grid_inputs(mp, 0.05, vegp, soilc, dtm)
    sc = a["soilc"]
    again = F.runmicro(mp, 0.05, vegp, soilc, dtm, from_dtm=True, slr=sc["slope"], apr=sc["aspect"], hor=sc["hor"], twi=sc["twi"],
                       wsa=sc["wsa"], svf=sc["svfa"])
    same(again, want)
