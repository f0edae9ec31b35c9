"""The staged model's diagnostics for array weather on the device (include/mcf.h mcf_plan_diag_enable_array, mcf_runmicro2_diag,
mcf_runmicro4_diag) against the yardstick of tests/stages_ref_array.c — coarse cases: the yardstick on oracle/coarse_oracle.py's
expansion — and the staged front end (frontend.modelina) on the bundled site.  Bars: tests/stages_ref_array.py `bars_for`
(tests/parity_bars.py bar_of on the yardstick's own noise builds); every other comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import parity_bars as PB
import stages_array_cases as AC
import stages_ref_array as SRA
from microclimf_amd import _abi, synthetic
from microclimf_amd.api import Plan, runmicro2Cpp, runmicro2Cpp_coarse, runmicro4Cpp

pytestmark = pytest.mark.gpu
DIAG = _abi.DIAG_NAMES
STATS = ("fast_tiles", "slow_tiles", "irregular_days", "fast_launches", "slow_launches", "canary_trips")
_runs = {}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def solve(a, coarse, diag="all", ring_days=None, **kw):
    """(ten outputs, diagnostics, dispatch stats, ring layout) of a plan run over the whole series in slots of `ring_days` days;
    diag=None: a plain plan"""
    a = dict(a)
    dfsel = a.pop("dfsel", None)
    ndays = len(a["obstime"]["year"]) // 24
    ring_days = ring_days or ndays
    with Plan(**a, array_forcing=coarse is None, coarse=coarse, ring_days=ring_days, dfsel=dfsel, **kw) as p:
        names = p.diag_enable_array(diag) if diag is not None else []
        outs = {k: [] for k, on in zip(_abi.OUT_NAMES, a["out"]) if on}
        dg = {k: [] for k in names}
        for d0 in range(0, ndays, ring_days):
            nd = min(ring_days, ndays - d0)
            if coarse is None:
                p.upload_forcing_days(d0, nd, 0)
            p.run_days(d0, nd, 0)
            for k in outs:
                outs[k].append(p.fetch(0, k, 0, nd * 24))
            for k in dg:
                dg[k].append(p.fetch_diag(0, k, 0, nd * 24))
        st = p.dispatch_stats()
        lay = p.ring_layout()
    cat = lambda d: {k: np.concatenate(v, axis=2) for k, v in d.items()}
    return cat(outs), cat(dg), st, lay


def plan_run(name, diag="all", **kw):
    c = AC.build(name)
    return solve(c.a, c.coarse, diag, **kw)


def full(name):
    if name not in _runs:
        _runs[name] = plan_run(name)
    return _runs[name]


def check_against_yardstick(label, got, want, bars, noise, swdown):
    assert list(got) == list(DIAG)
    worst = {}
    for k in DIAG:
        g, w = got[k], want[k]
        assert g.shape == w.shape, k
        assert PB.same_pattern(g, w), f"{k}: NA / finite pattern differs from the yardstick's"
        na = bits(w) == PB.NA_BITS
        assert (bits(g[na]) == PB.NA_BITS).all(), k
        worst[k] = PB.distance(g, w)
        print(f"{label} {k}: distance {worst[k]:.3e} bar {bars[k]:.3e} noise {noise[k]:.3e}")
    for k in DIAG:
        assert bars[k] <= PB.CAP
        assert worst[k] <= bars[k], f"{label} {k}: distance {worst[k]:.3e} > bar {bars[k]:.3e}"
    # exactly 0 where the reference's twostreamCpp sets 0: the cell's own swdown of the step is 0
    night = (np.asarray(swdown) == 0) & ~np.isnan(want["radGsw"])
    assert night.any()
    for k in ("radGsw", "radLsw", "radLpar"):
        assert (got[k][night] == 0).all(), k


@pytest.mark.parametrize("name", AC.CASES)
def test_t1_diagnostics_match_the_yardstick(name):
    c = AC.build(name)
    want, bars, noise = SRA.bars_for(name, c.full)
    _, got, st, lay = full(name)
    check_against_yardstick(name, got, want, bars, noise, c.full["climdata"]["swdown"])
    assert all((bits(want[k]) == PB.NA_BITS).any() for k in DIAG)          # every case has its NA cell
    assert st["fast_launches"] + st["slow_launches"] >= 1
    assert lay["cells_per_tile"] == 32


def test_t1_staged_taps_switched_off(monkeypatch):
    """the LDS-staged case again through the per-lane taps: the same operations in the same order"""
    c = AC.build("c_lds")
    want, bars, noise = SRA.bars_for("c_lds", c.full)
    _, staged, _, _ = full("c_lds")
    monkeypatch.setenv("MCF_NO_COARSE_LDS", "1")
    outs, got, _, _ = plan_run("c_lds")
    check_against_yardstick("c_lds per-lane", got, want, bars, noise, c.full["climdata"]["swdown"])
    for k in DIAG:
        assert np.array_equal(bits(got[k]), bits(staged[k])), k
    for k in outs:
        assert np.array_equal(bits(outs[k]), bits(full("c_lds")[0][k])), k


@pytest.mark.parametrize("name", ("a170_h005", "a355_h0", "alayered", "c_lane", "c_lds", "c_alt2"))
def test_t2_the_ten_outputs_keep_their_bits(name):
    outs, _, st, _ = full(name)
    plain, none, st0, _ = plan_run(name, diag=None)
    assert list(outs) == list(plain) and len(plain) == 10 and none == {}
    for k in plain:
        assert np.array_equal(bits(outs[k]), bits(plain[k])), k
    # ... through the same dispatch: the same launches of the same classes
    for k in STATS:
        assert st[k] == st0[k], (k, st[k], st0[k])
    # a diagnostic of pass 2 beside outputs that need none
    c = AC.build(name)
    few, dg, _, _ = solve(dict(c.a, out=[0, 0, 0, 1, 1, 1, 1, 0, 1, 0]), c.coarse, ["T0"])
    for k in ("soilm", "windspeed", "Rdirdown", "Rdifdown", "Rswup"):
        assert np.array_equal(bits(few[k]), bits(plain[k])), k
    assert list(dg) == ["T0"] and np.array_equal(bits(dg["T0"]), bits(full(name)[1]["T0"]))


@pytest.mark.parametrize("kw", (dict(ring_days=1), dict(cells_per_block=16), dict(cells_per_block=21), dict(cells_per_block=32),
                                dict(cells_per_block=42)), ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
@pytest.mark.parametrize("name", ("a170_h005", "alayered", "c_lane", "c_lds"))
def test_t3_invariant_under_ring_days_and_tile_size(name, kw):
    _, ref, _, _ = full(name)              # the whole series in one slot, 32-cell tiles
    _, got, _, lay = plan_run(name, **kw)
    # array plans take 16-, 21- and 32-cell tiles (42 is a vector-forcing geometry: 32 instead); coarse plans force 32
    want_cpb = 32 if name in AC.COARSE else {0: 32, 42: 32}.get(kw.get("cells_per_block", 0), kw.get("cells_per_block", 0))
    assert lay["cells_per_tile"] == want_cpb
    for k in DIAG:
        assert np.array_equal(bits(got[k]), bits(ref[k])), (k, kw)


@pytest.mark.parametrize("above,ground", (("a170_h005", "a170_h0"), ("a355_h005", "a355_h0"), ("c_lane", "c_lane_h0")))
def test_t4_t0_is_the_ground_run_s_tz(above, ground):
    """both are pass 2's `Tg`: the same expression on the same operands"""
    tz = full(ground)[0]["Tz"]
    assert np.array_equal(bits(full(above)[1]["T0"]), bits(tz))
    assert np.array_equal(bits(full(ground)[1]["T0"]), bits(tz))


def test_t5_a_fast_launch_whose_canary_trips():
    """one cell-step of the pressure is negative (tests/test_dispatch_gpu.py): the lane's check trips the canary and the fix-up
    kernel redoes the tile — outputs AND diagnostics — with the reference's clamps"""
    a = synthetic.workload(32, 5, 48, reqhgt=0.05, start_doy=170, array_forcing=True)
    a["climdata"]["pk"] = a["climdata"]["pk"].copy(order="F")
    a["climdata"]["pk"][7, 2, 30] = -101.3            # tile 2, day 1, hour 6
    outs, got, st, _ = solve(a, None)
    assert st["slow_tiles"] == 0 and st["fast_launches"] == 1 and st["canary_trips"] >= 1, st
    want, bars, noise = SRA.bars_for("canary", a)
    check_against_yardstick("canary", got, want, bars, noise, a["climdata"]["swdown"])
    plain, _, st0, _ = solve(a, None, None)
    assert st0["canary_trips"] == st["canary_trips"]
    for k in plain:
        assert np.array_equal(bits(outs[k]), bits(plain[k])), k


def test_t6_selection_and_one_shot_entries():
    c = AC.build("a170_h005")
    a = [c.a[k] for k in AC.ARGS]
    outs, ref, _, _ = full("a170_h005")
    pick = ["G", "radGsw", "uf"]        # any order: returned in the enum's
    _, got, _, _ = plan_run("a170_h005", diag=pick)
    assert list(got) == ["radGsw", "uf", "G"]
    for k in got:
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    with Plan(**c.a, array_forcing=True, ring_days=c.ndays) as p:
        p.diag_enable_array(pick)
        lay, out_lay = p.diag_ring_layout(), p.ring_layout()
        assert lay["tiled"] == 1 and lay["cells_per_tile"] == out_lay["cells_per_tile"] and lay["block_doubles"] == out_lay["block_doubles"]
        assert lay["day_stride"] == 3 * lay["block_doubles"] and lay["tile_stride"] == c.ndays * lay["day_stride"]
        assert p.diag_slot_ptr(0, "uf") - p.diag_slot_ptr(0, "radGsw") == 8 * lay["block_doubles"]
        with pytest.raises(_abi.McfError, match="not selected"):
            p.fetch_diag(0, "si", 0, 24)
    # one-shot, the forcing streamed a day at a time and whole
    plain = runmicro2Cpp(*a)
    assert "diag" not in plain and list(plain) == list(outs)
    for chunk in (1, 0):
        one = runmicro2Cpp(*a, days_per_chunk=chunk, diag="all")
        assert list(one["diag"]) == list(DIAG) and [k for k in one if k != "diag"] == list(plain)
        for k in DIAG:
            assert np.array_equal(bits(one["diag"][k]), bits(ref[k])), (k, chunk)
        for k in plain:
            assert np.array_equal(bits(one[k]), bits(plain[k])) and np.array_equal(bits(one[k]), bits(outs[k])), (k, chunk)
    lay = dict(AC.build("alayered").a)
    dfsel = lay.pop("dfsel")
    one = runmicro4Cpp(dfsel, *[lay[k] for k in AC.ARGS], diag=pick)
    assert list(one["diag"]) == ["radGsw", "uf", "G"]
    for k in one["diag"]:
        assert np.array_equal(bits(one["diag"][k]), bits(full("alayered")[1][k])), k
    # coarse, with the altitude correction, the staged taps: the plan's bits again
    for name in ("c_alt2", "c_lds"):
        cc = AC.build(name)
        for chunk in (1, 0):
            one = runmicro2Cpp_coarse(*[cc.a[k] for k in AC.ARGS], **cc.coarse, days_per_chunk=chunk, diag="all")
            for k in DIAG:
                assert np.array_equal(bits(one["diag"][k]), bits(full(name)[1][k])), (name, k, chunk)
            for k, v in full(name)[0].items():
                assert np.array_equal(bits(one[k]), bits(v)), (name, k, chunk)
    # steps beyond the last whole day: NA like the ten outputs
    b = synthetic.workload(3, 4, 30, variety=True, start_doy=170, array_forcing=True)
    tail = runmicro2Cpp(*[b[k] for k in AC.ARGS], diag=["T0", "si"])
    for k in ("T0", "si"):
        assert (bits(tail["diag"][k][:, :, 24:]) == PB.NA_BITS).all() and np.isfinite(tail["diag"][k][:, :, :24]).any()
    assert (bits(tail["Tz"][:, :, 24:]) == PB.NA_BITS).all()


def test_t7_refusals():
    import stages_cases as SC
    c, cc = AC.build("a170_h005"), AC.build("c_lane")
    launches = lambda p: sum(p.dispatch_stats()[k] for k in ("fast_launches", "slow_launches"))
    with Plan(**SC.build("s170_h005"), ring_days=4) as p:
        with pytest.raises(_abi.McfError, match="error 1: .*mcf_plan_diag_enable for vector forcing"):
            p.diag_enable_array()
        assert launches(p) == 0
        p.diag_enable()                  # the plan is still good for its own entry
    for a, coarse in ((c.a, None), (cc.a, cc.coarse)):
        kw = dict(array_forcing=coarse is None, coarse=coarse, ring_days=4)
        with Plan(**a, **kw) as p:       # the old entry keeps its refusal
            with pytest.raises(_abi.McfError, match="error 1: .*array forcing"):
                p.diag_enable()
            with pytest.raises(_abi.McfError, match="error 5: .*no diagnostics ring"):
                p.fetch_diag(0, "si", 0, 24)
            with pytest.raises(_abi.McfError, match="error 1: .*no diagnostic selected"):      # (by name an empty selection is a ValueError)
                _abi.check(p._lib.mcf_plan_diag_enable_array(p._p, C.byref((C.c_int32 * 13)())))
            with pytest.raises(ValueError):
                p.diag_enable_array([])
            if coarse is None:
                p.upload_forcing_days(0, 1, 0)
            p.run_days(0, 1, 0)
            n = launches(p)
            with pytest.raises(_abi.McfError, match="error 5: .*mcf_plan_diag_enable_array comes before the plan's first run"):
                p.diag_enable_array()
            assert launches(p) == n
        with Plan(**a, **kw) as p:
            p.diag_enable_array()
            with pytest.raises(_abi.McfError, match="error 5: .*already enabled"):
                p.diag_enable_array()
            # tile masks and cell subsets: an array-weather plan refuses them with or without diagnostics
            with pytest.raises(_abi.McfError, match="error 1: .*tile mask needs vector forcing"):
                p.run_days_masked(0, 1, 0, 0, np.zeros(p.n_tiles, dtype=np.uint8))
            need = np.ones(c.rows * c.cols, dtype=np.uint8)       # (refused before the flags are looked at)
            with pytest.raises(_abi.McfError, match="error 1: .*cell subset needs vector forcing"):
                p.run_days_cells(0, 1, 0, 0, need.ctypes.data)
            assert launches(p) == 0
            if coarse is None:
                p.upload_forcing_days(0, 4, 0)
            p.run_days(0, 4, 0)              # the plan is still good
            name = "a170_h005" if coarse is None else "c_lane"
            assert np.array_equal(bits(p.fetch_diag(0, "G", 0, 96)), bits(full(name)[1]["G"]))
    with Plan(**dict(c.a, reqhgt=-0.05), array_forcing=True, ring_days=4) as p:
        with pytest.raises(_abi.McfError, match="error 1: .*reqhgt >= 0"):
            p.diag_enable_array()
        assert launches(p) == 0
    with Plan(**dict(c.a, reqhgt=-0.05), array_forcing=True, ring_days=4, stream_below=True) as p:
        with pytest.raises(_abi.McfError, match="error 1: "):
            p.diag_enable_array()
    a = [c.a[k] for k in AC.ARGS]
    with pytest.raises(ValueError):
        runmicro2Cpp(*a, diag="all", devices=[0], n_blocks=2)
    with pytest.raises(_abi.McfError, match="error 1: .*reqhgt >= 0"):
        runmicro2Cpp(*[dict(c.a, reqhgt=-0.05)[k] for k in AC.ARGS], diag="all")


def test_t8_front_end_on_the_bundled_site():
    """tests/bundled.py under the 2 x 3 grid of perturbed climate cells of tests/test_frontend_bioclima_gpu.py, the monthly-tmax
    subset (50 x 50 cells x 288 h, layered vegetation): modelina -> stages -> aboveground is runmicro_array"""
    from microclimf_amd import frontend as F
    from test_frontend_bioclima_gpu import CC, CR, site
    climarray, obstime, vegp, soilc, dtm, lats, lons, clats, clons = site()
    mpa = F.runpointmodela(climarray, obstime, 0.05, dtm, vegp, soilc, lats=clats, lons=clons)
    mx = F.subsetpointmodela(mpa, "month", "tmax")
    kw = dict(lats=lats, lons=lons)
    want = F.runmicro_array(mx, CR, CC, 0.05, vegp, soilc, dtm, **kw)
    ground = F.runmicro_array(mx, CR, CC, 0.0, vegp, soilc, dtm, **kw)["Tz"]
    micro = F.modelina(mx, CR, CC, vegp, soilc, dtm, **kw)
    assert micro["progress"] == 0 and micro["tme"] is mx[0]["obstime"] and "soilc" in micro["inputs"]
    seen = set(micro)
    for level, fn in enumerate((F.soilmdistribute, F.twostream, F.wind, F.soiltemp), start=1):
        micro = fn(micro)
        assert micro["progress"] == level
        assert set(F.STAGE_FIELDS[level]) <= set(micro) - seen, (level, set(micro) - seen)
        seen = set(micro)
        assert len(micro["_runs"]) == 1          # one diagnostics solve serves every stage
    for k in ("soilm", "radGsw", "uf", "Tg", "G"):
        assert micro[k].shape == (50, 50, 288), k
    assert np.array_equal(bits(micro["soilm"]), bits(want["soilm"])) and np.array_equal(bits(micro["uz"]), bits(want["windspeed"]))
    got = F.aboveground(micro)
    assert len(micro["_runs"]) == 1
    assert list(got) == list(want) + ["T0"] and len(got) == 11
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(bits(got["T0"]), bits(ground))
    assert np.array_equal(bits(micro["Tg"]), bits(ground)) and micro["T0"] is micro["Tg"]
    assert np.isfinite(got["T0"]).sum() > 2000 * 288
    with pytest.raises(ValueError, match="coarse array forcing below ground"):
        F.belowground(micro, -0.05)
    with pytest.raises(NotImplementedError, match="array weather"):
        F.modelin(mx, vegp, soilc, dtm)
