"""The per-cell-step sun position and humidity helpers of array forcing (mcf_device.hpp derive_time_af /
derive_time_af_pass2, satvap_r / lapserate_r / dewpoint_r; mcf_snow_device.hpp sun_cell / sun_at_cell), run elementwise by
mcf_selftest_step, against the longdouble yardstick of tests/step_ref.py on the case sets of tests/step_cases.py — which
also says how the bars are made (integers exact off the fragile cases, floating fields within 16 x the fp64 yardstick's own
error per conditioning class).  Every figure is printed before it is asserted.

The device runs each kind ONCE on all step sets back to back; the tests share those results and the two yardsticks."""
import functools

import numpy as np
import pytest

import step_cases as S
import step_ref as R
from microclimf_amd import _abi

pytestmark = pytest.mark.gpu

NOUT = {0: 29, 1: 29, 2: 21, 3: 4}
KIND1_FIELDS = tuple("EOT" if f == "COSA" else f for f in R.STEP_FIELDS)
SNOW_LITERAL = ("zend", "cosz", "cz", "sz", "tansa", "kx", "kcos", "sa", "ca", "tansa_deg", "sindex")
STEP_FLOATS = ("CZ", "SZ", "TANSA", "ZEND", "COSC", "TANC", "TAN2C", "INV2COSC", "SAZ", "CAZ", "DE", "GHRRAD", "REM", "LAPK", "WFAC",
               "RBEAM", "RB", "GHRRAD2", "REM2", "MUPM", "INVMUPM", "SINDEC", "COSDEC")
SNOW_FLOATS = ("cosz", "cz", "sz", "tansa", "kx", "kcos", "sa", "ca")


def run(kind, planes):
    lib = _abi.load()
    x = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64) for p in planes]))
    out = np.full((NOUT[kind], x.shape[1]), -7.0)
    _abi.check(lib.mcf_selftest_step(kind, x.ctypes.data_as(_abi.c_double_p), x.shape[0], out.ctypes.data_as(_abi.c_double_p),
                                     out.shape[0], x.shape[1], 0))
    return out


@functools.lru_cache(maxsize=None)
def device(kind):
    """field -> values over the pooled step sets (kind 2: the literal fields as lit_<field>); humidity for kind 3"""
    if kind == 3:
        c = S.humidity_case()
        out = run(3, [c["tc"], c["rh"], c["pk"]])
        return dict(zip(R.HUM_FIELDS, out))
    inp, _ = S.pooled()
    out = run(kind, [inp[k] for k in S.INPUTS])
    if kind == 2:
        d = dict(zip(R.SNOW_FIELDS, out[:10]))
        d.update({"lit_" + f: v for f, v in zip(SNOW_LITERAL, out[10:])})
    else:
        d = dict(zip(R.STEP_FIELDS if kind == 0 else KIND1_FIELDS, out))
    d["up"] = _up(d["ZEND" if kind < 2 else "zend"])
    for a in d.values():
        a.setflags(write=False)
    return d


def _up(zend):
    """Above the horizon: zenith <= 90.  At the zenith itself fp64 rounding can carry coh past 1; acos of that is NaN in the reference
    as on both device routes: a NaN zenith angle counts as "up" ONLY where the yardstick's 1 - coh^2 is below S2_MIN (pooled sets)."""
    truth, _ = S.yardsticks()
    return (zend <= 90.0) | (np.isnan(zend) & np.asarray(truth["sp"]["s2"] < S.LD(S.S2_MIN)))


def _check_integers(name, sindex, up, ksat, date_row, what):
    """sindex / up / ksat of one set against the yardstick: exact off the fragile cases; a fragile sector is one of the two that
    meet at the nearest boundary"""
    m = S.margins(name, date_row)
    n = len(m["up"])
    frag = {"sector": m["sector"] & m["assert_sector"], "up": m["up_f"], "ksat": m["ksat_f"]}
    print(f"{what} {name}{' (fp64 date row)' if date_row else ''}: {n} cases, E azimuth {m['e_az']:.3e} deg, E coh {m['e_coh']:.3e}; "
          f"fragile sector {frag['sector'].sum()}, horizon {frag['up'].sum()}, zenith {frag['ksat'].sum()}")
    a = m["assert_sector"]
    bad = a & ~frag["sector"] & (sindex != m["sindex"])
    print(f"  sector: {bad.sum()} wrong off the fragile cases")
    assert not bad.any(), np.nonzero(bad)[0][:10]
    in_pair = (sindex == m["pair"][0]) | (sindex == m["pair"][1])
    assert in_pair[a & frag["sector"]].all()
    bad = ~frag["up"] & (up != m["up"])
    print(f"  up: {bad.sum()} wrong off the fragile cases")
    assert not bad.any(), np.nonzero(bad)[0][:10]
    if ksat is not None:
        bad = ~frag["ksat"] & (ksat != m["ksat"])
        print(f"  ksat: {bad.sum()} wrong off the fragile cases")
        assert not bad.any(), np.nonzero(bad)[0][:10]
    return {k: v.sum() / n for k, v in frag.items()}


def _kind_integers(kind, s):
    d = device(kind)
    if kind == 2:
        return d["sindex"][s].astype(np.int64), d["up"][s], None
    return d["sindex"][s].astype(np.int64), d["up"][s], d["ksat"][s] != 0


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("name", list(S.SETS))
def test_integers_equal_the_yardstick_off_the_fragile_cases(name, kind):
    _, where = S.pooled()
    sindex, up, ksat = _kind_integers(kind, where[name])
    share = _check_integers(name, sindex, up, ksat, False, f"kind {kind}")
    if name in S.STEPPED:
        # 2^20 ulp of the hour is less than 64 E of the whole chain (the day's part rounds the declination to 2e-12): these sets are
        # judged on the fp64 values of the day's part, which both device routes share — and there the yardstick flags none
        share = _check_integers(name, sindex, up, ksat, True, f"kind {kind}")
        assert not any(share.values())
    if name != "sector_ulp":
        assert all(v <= S.MAX_FRAGILE for v in share.values()), share
    if kind == 2:
        # the literal sol_site + sun_derive beside it
        d = device(2)
        s = where[name]
        lit_up = _up(d["lit_zend"])[s]
        _check_integers(name, d["lit_sindex"][s].astype(np.int64), lit_up, None, False, "kind 2 literal")
        m = S.margins(name)
        assert (d["up"][s] == lit_up)[~m["up_f"]].all()


@pytest.mark.parametrize("kind", [0, 1])
def test_julday_and_wind_sector(kind):
    truth, _ = S.yardsticks()
    d = device(kind)
    assert np.array_equal(d["julday"], truth["julday"].astype(np.float64))
    assert np.array_equal(d["windex"], truth["windex"].astype(np.float64))


def _assert_rows(rows, title):
    print(S.format_rows(rows, title))
    assert rows
    bad = [r for r in rows if not r[4] <= S.BAR_FACTOR * r[3]]
    assert not bad, bad


@pytest.mark.parametrize("date_row", [False, True])
def test_kind0_fields_within_16_E(date_row):
    """the solver's array-forcing step; ZEND carries a value only where the zenith in degrees is below pi/2.  date_row: against the
    exact site algebra on the fp64 values of the day's part, whose E is not swamped by the declination's 2e-12.  That judgement
    relies on the device's sol_date giving numpy's fp64 day's part to about 1e-15: the operations are the same, but the device may
    contract sol_date's `m = 6.24004077 + 0.01720197 (jd - 2451545)` into one fma, which numpy does not — m (140 rad) then differs
    by an ulp and the equation of time by 3e-13 minutes.  The largest error measured on this truth, 6.4 E on COSA / SINA, is that
    effect; a toolchain that contracts differently moves it, within the bar."""
    truth, _ = S.yardsticks(date_row)
    _assert_rows(S.compare_fields(device(0), STEP_FLOATS + ("COSA", "SINA"), extra_mask={"ZEND": truth["ksat"] == 0}, date_row=date_row),
                 f"kind 0 (derive_time_af, derive_time_af_pass2){', fp64 date row' if date_row else ''}")


def test_kind1_fields_within_16_E():
    _assert_rows(S.compare_fields(device(1), STEP_FLOATS + ("EOT",)), "kind 1 (sol_site, derive_time)")
    # (the equation of time IS the day's part: on its fp64 value there is nothing to compare)
    _assert_rows(S.compare_fields(device(1), STEP_FLOATS, date_row=True), "kind 1 (sol_site, derive_time), fp64 date row")
    assert np.isnan(device(1)["SINA"]).all()
    # kind 0 against kind 1 needs no bar of its own: reported
    cl, d0, d1 = S.classes()["s2>=0.5"], device(0), device(1)           # (where both routes are well conditioned)
    for f in STEP_FLOATS:
        if f != "ZEND":
            with np.errstate(all="ignore"):
                dif = np.abs(d0[f] - d1[f])[cl]
            print(f"  kind 0 - kind 1, {f:9s} largest |difference| {np.nanmax(dif):.3e}")


def test_kind2_fields_within_16_E():
    d = device(2)
    _assert_rows(S.compare_fields(d, SNOW_FLOATS), "kind 2 (sun_cell, sun_at_cell)")
    _assert_rows(S.compare_fields(d, SNOW_FLOATS, date_row=True), "kind 2 (sun_cell, sun_at_cell), fp64 date row")
    lit = {f: d["lit_" + f] for f in SNOW_FLOATS + ("zend", "tansa_deg")}
    _assert_rows(S.compare_fields(lit, SNOW_FLOATS + ("zend", "tansa_deg")), "kind 2 literal (sol_site, sun_derive)")
    assert set(np.unique(d["zend"])) <= {45.0, 135.0}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_nan_propagates_as_the_yardstick_says(kind):
    truth, _ = S.yardsticks()
    cl = S.classes()
    keep = cl["s2>=1e-2"] | cl["1e-6<=s2<1e-2"] | cl["1e-12<=s2<1e-6"]
    inp, _ = S.pooled()
    assert np.isnan(inp["tc"]).sum() == 1 and keep[np.isnan(inp["tc"])].all()
    d = device(kind)
    for f in (STEP_FLOATS if kind < 2 else SNOW_FLOATS):
        if kind == 0 and f == "ZEND":        # 45 / 135 stand in where the yardstick has the angle: never a NaN off the zenith
            assert not np.isnan(d[f])[keep].any()
            continue
        assert np.array_equal(np.isnan(d[f])[keep], np.isnan(np.asarray(truth[f], dtype=np.float64))[keep]), f


def test_next_to_the_zenith():
    """1 - coh^2 below 1e-12: the azimuth means nothing, but the values k_solve goes on to use stay finite and the bits right;
    and the band (cos(pi/2 pi/180), 0.99962422], where the `nearzen` constant 0.99962422 set ksat against the literal route"""
    _, where = S.pooled()
    truth, _ = S.yardsticks()
    s = where["zenith"]
    coh = truth["sp"]["coh"][s]
    tiny = np.asarray(truth["sp"]["s2"][s] < S.S2_MIN)
    assert tiny.sum() >= 12 and np.asarray(1 - coh < 1e-12).sum() >= 12
    for kind in (0, 2):
        d = device(kind)
        for f in (("CZ", "COSC", "TANC", "INV2COSC", "SZ", "TANSA", "SAZ", "CAZ", "RBEAM", "RB") if kind == 0 else SNOW_FLOATS):
            assert np.isfinite(d[f][s][tiny]).all(), f
        assert d["up"][s][tiny].all()
    assert not device(0)["ksat"][s][tiny].any()
    band = np.asarray((coh > S.zenith_threshold()) & (coh <= S.LD(S.NEARZEN_BEFORE)))
    print(f"zenith set: {band.sum()} cases in the band, ksat there: kind 0 {device(0)['ksat'][s][band].sum()}, "
          f"kind 1 {device(1)['ksat'][s][band].sum()}, yardstick {truth['ksat'][s][band].sum()}")
    assert band.sum() >= 20
    assert not S.margins("zenith")["ksat_f"][band].any()
    assert not device(0)["ksat"][s][band].any() and not device(1)["ksat"][s][band].any()
    # where ksat is clear pass 2 makes the degrees-call operands from ZEND: it has to be the zenith there, not the 45 that stands in
    z0 = device(0)["ZEND"][s][band]
    assert (np.abs(z0 - np.asarray(truth["ZEND"][s][band], dtype=np.float64)) < 1e-6).all()


@pytest.mark.parametrize("kind", [0, 2])
def test_the_square_roots_carry_full_precision(kind):
    """CZ^2 + SZ^2 = 1 and SAZ^2 + CAZ^2 = 1 as far as fp64 allows.  CZ is coh itself and SZ = sqrt(fl(1 - fl(coh^2))): the two
    roundings of the radicand leave at most 2 x 2^-53, the root's relative error e (fsqrt: below 3e-16, tests/test_math_gpu.py)
    2 e s2 — together below 5 x 2^-52 = 1.1e-15.  A 46-bit root (fsqrt_m) leaves 2.8e-14 s2.  The 16 E bars cannot see that:
    the reference's own fp64 error of SZ is 8e-16 where it is best conditioned."""
    d = device(kind)
    for c, s_ in (("CZ", "SZ"), ("CAZ", "SAZ")) if kind == 0 else (("cz", "sz"), ("ca", "sa")):
        r = np.abs(d[c].astype(S.LD) ** 2 + d[s_].astype(S.LD) ** 2 - 1)
        print(f"kind {kind}: largest |{c}^2 + {s_}^2 - 1| = {float(r.max()):.3e}")
        assert float(r.max()) <= 5 * 2.0 ** -52


def test_clamps_and_signs():
    """the 1352 clamp on a sun just above the horizon, the sign of RBEAM / RB just below it, the night literals"""
    _, where = S.pooled()
    truth, _ = S.yardsticks()
    d, s = device(0), where["horizon"]
    coh = np.asarray(truth["sp"]["coh"][s], dtype=np.float64)
    inp, _ = S.pooled()
    lit_beam = (inp["rsw"] - inp["rdif"])[s] > 1.0
    grazing = (coh > 0) & (coh < 1e-6) & lit_beam
    assert grazing.sum() >= 20 and (d["RBEAM"][s][grazing] == 1352.0).all()
    below = (coh < 0) & (coh > -1e-6) & lit_beam
    assert below.sum() >= 20 and (d["RBEAM"][s][below] < -1e6).all() and (d["RB"][s][below] > 0).all()
    night = coh < 0
    assert (d["COSC"][s][night] == np.cos(np.pi / 2)).all() and (d["TANC"][s][night] == np.tan(np.pi / 2)).all()
    assert (d["INV2COSC"][s][night] > 8e15).all() and (d["ZEND"][s][night] == 135.0).all()


def test_humidity_helpers():
    t, lit = S.humidity_yardsticks()
    d = device(3)
    c = S.humidity_case()
    fragile, e_tdew = S.humidity_margin()
    print(f"humidity: {len(c['tc'])} cases, E dew point {e_tdew:.3e} K, fragile {fragile.sum()}")
    assert fragile.sum() <= S.MAX_FRAGILE * len(fragile)
    rel = lambda x, f: np.abs(np.asarray(x).astype(S.LD) - t[f]) / np.abs(t[f])           # noqa: E731
    for f in ("es", "lapse"):
        e, g = float(np.max(rel(lit[f], f))), float(np.max(rel(d[f], f)))
        print(f"  {f}: relative error, E {e:.3e}, device {g:.3e} ({g / e:.2f} E)")
        assert g <= S.BAR_FACTOR * e
    dry = c["rh"] == 0.0
    assert dry.sum() >= 20 and (d["ea"][dry] == 0.0).all() and (d["tdew"][dry] == -273.15).all()
    assert (np.asarray(t["tdew"], dtype=np.float64)[dry] == -273.15).all()
    ok = ~fragile & ~dry
    e = float(np.max(np.abs(lit["tdew"].astype(S.LD) - t["tdew"])[ok]))
    g = float(np.max(np.abs(d["tdew"].astype(S.LD) - t["tdew"])[ok]))
    print(f"  dew point: absolute error, E {e:.3e} K, device {g:.3e} K ({g / e:.2f} E)")
    assert g <= S.BAR_FACTOR * e
    # a fragile case holds one of the two branches' values
    tw = np.asarray(t["tdew_w"], dtype=np.float64)
    jump = 0.02          # dew against frost point at 0 degrees C: about 0.01 K
    assert (np.abs(d["tdew"][fragile] - tw[fragile]) < jump).all()
    near = ~dry & ~fragile & (np.abs(tw) < 1e-3)        # (the bar above is what catches a wrong branch: 16 E is far below the jump)
    assert near.sum() >= 100 and (tw[near] < 0).sum() >= 40 and (tw[near] > 0).sum() >= 40


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_results_do_not_depend_on_the_launch(kind):
    """a lane's result is its own: any n gives the bits of the full run (the last block partly filled, one lane, one wave +- 1)"""
    if kind == 3:
        c = S.humidity_case()
        planes = [c["tc"], c["rh"], c["pk"]]
    else:
        inp, _ = S.pooled()
        planes = [inp[k] for k in S.INPUTS]
    full = run(kind, planes)
    assert full.shape[1] % 256 != 0
    for n, at in ((1, 0), (63, 20000), (64, 22000), (65, 24100), (257, 25500), (1000, 19500)):
        if kind == 3:
            at = at % 8000
        part = run(kind, [p[at:at + n] for p in planes])
        assert np.array_equal(part.view(np.uint64), full[:, at:at + n].view(np.uint64)), (kind, n)
