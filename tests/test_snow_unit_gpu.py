"""The device physics of the snow kernels (mcf_snow_device.hpp: the operand guards, the two-stream coefficients, cank1, the
canopy and profile helpers, the step weather), run elementwise by mcf_selftest_snow, against the longdouble yardstick of
tests/snow_ref.py on the case sets of tests/snow_unit_cases.py — which also says how the bars are made (floating fields within
16 x the fp64 yardstick's own error per conditioning class, clamps on the yardstick's side off the fragile cases, special
operands by class with no tolerance).  Every figure is printed before it is asserted.

The device runs each kind ONCE on all its sets back to back; the tests share those results and the two yardsticks."""
import functools

import numpy as np
import pytest

import snow_ref as R
import snow_unit_cases as S
from microclimf_amd import _abi

pytestmark = pytest.mark.gpu
LD = S.LD
ULP = 2.0 ** -52


def run(kind, planes):
    lib = _abi.load()
    x = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64) for p in planes]))
    out = np.full((R.NOUT[kind], x.shape[1]), -7.0)
    _abi.check(lib.mcf_selftest_snow(kind, x.ctypes.data_as(_abi.c_double_p), x.shape[0], out.ctypes.data_as(_abi.c_double_p),
                                     out.shape[0], x.shape[1], 0))
    return out


def _planes(kind):
    c, _ = S.pooled(kind)
    return [c[k] for k in S.KEYS[kind]]


@functools.lru_cache(maxsize=None)
def device(kind):
    d = dict(zip(S.FIELDS[kind], run(kind, _planes(kind))))
    for a in d.values():
        a.setflags(write=False)
    return d


def _assert_rows(rows, title):
    print(S.format_rows(rows, title))
    assert rows
    bad = [r for r in rows if not r[4] <= S.BAR_FACTOR * r[3]]
    assert not bad, bad


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- floating fields --------------------------------------------------------------------------------------------------------------
def test_kind0_scalars_within_16_E():
    """gexp, glog, gsqrt, svp, dewpoint, rad4, latent_lt0, the albedo and the two R-side helpers on ordinary operands"""
    fields = tuple(f for f in S.classes(0) if f != "gpow0")
    _assert_rows(S.compare_fields(0, device(0), fields), "kind 0 (guards and scalars)")


def test_kind0_gpow0_within_16_E():
    """clump^Kc for clump in (0, 1], Kc in [1, 600], by classes of |e ln b|, against the C library's pow, which the reference
    calls (E = 1.2e-16).  As exp(e log b) on the lean fp64 exp and log the routine carried the rounding of e log b into the
    result |e ln b| times: 47 E for 1 <= |e ln b| < 32 and 920 E (1.1e-13 relative) from 32 on.  gpow_pos now makes the logarithm
    as a pair good to 2^-62 and keeps the product's rounding: 2.4, 2.4 and 3.0 E."""
    _assert_rows(S.compare_fields(0, device(0), ("gpow0",)), "kind 0 gpow0")


def test_kind1_radiation_within_16_E():
    """every field of ts_dif, ts_dir and cank1 per class of 1 - om and |kd - h| / h, below pait h = 30"""
    _assert_rows(S.compare_fields(1, device(1)), "kind 1 (ts_dif, ts_dir, cank1)")


def test_kind2_canopy_within_16_E():
    _assert_rows(S.compare_fields(2, device(2)), "kind 2 (canopy and profile)")


def test_kind3_step_weather_within_16_E():
    _assert_rows(S.compare_fields(3, device(3)), "kind 3 (met_derive, micro_met)")
    d = device(3)
    for a, b in (("ea", "m_ea"), ("tdew", "m_tdew"), ("rem", "m_Rem")):       # the two derive functions agree to the bit
        assert np.array_equal(d[a].view(np.uint64), d[b].view(np.uint64)), (a, b)


# ---- identities that expose a 46-bit reciprocal or root under a wide E --------------------------------------------------------------
def test_reciprocals_and_roots_carry_full_precision():
    """Where a formula cancels, E is wide (h carries 2.8e-14 of relative error in the class 1 - om >= 1e-3, the p's 1e-11 next to
    kd = h) and a 46-bit quotient or root (fdiv_m, fsqrt_m: 1.4e-14) hides under 16 E.  These do not cancel:
      x * (1 / x) = 1 for S1, D1, D2 and sig against the device's own reciprocals: fdiv is a * (1 / b) with two roundings, 1.5 x
        2^-53 relative each at most — bar 2 x 2^-52; fdiv_m leaves 64 x 2^-52;
      h^2 = a^2 + 2 a gma from the device's own a and gma: three roundings of the radicand (0.75 x 2^-52) and twice the root's
        error (fsqrt: below an ulp, 2 x 2^-52) — bar 4 x 2^-52; fsqrt_m leaves 128 x 2^-52;
      sn^2 + cs^2 = 1 on [0, pi]: both below an ulp (1.1e-16 absolute), 2 (|sn| + |cs|) 1.1e-16 <= 1.4 x 2^-52 — bar 2 x 2^-52.
        (This one sees a slip in either polynomial, not one in the reduction — sine and cosine of the same wrong angle still
        square to 1; a dropped second step of the reduction is 2e-11 of angle and fails the 16 E bar of sn / cs, E = 5.6e-17.)"""
    g = {k: v.astype(LD) for k, v in device(1).items()}
    c, _ = S.pooled(1)
    truth, _ = S.yardsticks(1)
    shallow = _f64(truth["h"] * c["pait"].astype(LD)) < S.DEEP
    with np.errstate(all="ignore"):
        for a, b in (("S1", "iS1"), ("D1", "iD1"), ("D2", "iD2"), ("sig", "isig")):
            v = _f64(np.abs(g[a] * g[b] - 1))
            m = shallow & np.isfinite(v)
            print(f"largest |{a} * {b} - 1| = {v[m].max() / ULP:.2f} x 2^-52 over {m.sum()} cases")
            assert m.sum() >= 12000 and v[m].max() <= 2 * ULP
        v = _f64(np.abs(g["h"] ** 2 - (g["a"] ** 2 + 2 * g["a"] * g["gma"])) / g["h"] ** 2)
        m = shallow & np.isfinite(v)
        print(f"largest |h^2 - (a^2 + 2 a gma)| / h^2 = {v[m].max() / ULP:.2f} x 2^-52 over {m.sum()} cases")
        assert m.sum() >= 12000 and v[m].max() <= 4 * ULP
    d = device(2)
    x = S.pooled(2)[0]["x"]
    m = (x >= 0) & (x <= 3.1416)
    v = _f64(np.abs(d["sn"].astype(LD) ** 2 + d["cs"].astype(LD) ** 2 - 1))
    print(f"largest |sn^2 + cs^2 - 1| = {v[m].max() / ULP:.2f} x 2^-52 over {m.sum()} cases")
    assert v[m].max() <= 2 * ULP


# ---- special operands: by class, no tolerance ------------------------------------------------------------------------------------
def test_kind0_special_operands_by_class():
    """Every output of kind 0 but gpow0 on the special table (NaN among the operands: the NaN propagation of kind 0): the class (NaN,
    +-inf, +-0, sign) numpy gives.
    gexp is held on its documented domain (NaN or |x| < 1e90: an infinite argument is not reachable and comes out NaN), glog on
    everything but +inf; finite non-zero results of the first six also within 16 x 2^-52 of numpy's (each is a single library call
    whose error is half an ulp; the others are under the floating bars on their own sets)."""
    c, where = S.pooled(0)
    _, lit = S.yardsticks(0)
    s = where["special"]
    x, d = c["x"][s], device(0)
    # svp is gexp of a lean quotient: its operand must leave a * tc finite (the largest double does not); dewpoint is glog's
    domain = {"gexp": np.isnan(x) | (np.abs(x) < 1e90), "glog": x != S.INF, "svp": np.isnan(x) | (np.abs(x) <= 1e300),
              "dewpoint": x != S.INF}
    for f in ("gexp", "glog", "gsqrt", "clamp01", "rad4", "latent_lt0", "svp", "dewpoint", "satvap_r", "lapserate_r", "snow_albedo"):
        m = domain.get(f, np.ones(len(x), dtype=bool))
        want, got = _f64(lit[f][s])[m], d[f][s][m]
        cw, cg = S.value_class(want), S.value_class(got)
        print(f"{f}: {m.sum()} special operands, {np.count_nonzero(cw != cg)} of another class than numpy's")
        assert np.array_equal(cw, cg), (f, x[m][cw != cg], want[cw != cg], got[cw != cg])
        if f in ("gexp", "glog", "gsqrt", "clamp01", "rad4", "latent_lt0"):
            fin = np.isfinite(want) & (want != 0) & (np.abs(want) > 2.3e-308)
            assert (np.abs(got[fin] - want[fin]) <= 16 * ULP * np.abs(want[fin])).all(), f
    # what the header promises outside the domain, so that a change is noticed
    assert np.isnan(d["gexp"][s][np.isinf(x)]).all()
    # the square root is exact at +-0 and at the switch to the library's root
    assert np.array_equal(np.signbit(d["gsqrt"][s][x == 0]), np.signbit(x[x == 0]))


# C's pow where the device deliberately differs: the sign of a zero base is not carried, and a base of exactly
# 1 with a NaN exponent goes through exp(NaN * 0)
def _gpow0_known(b, e):
    odd = (e == np.rint(e)) & (np.fmod(e, 2.0) != 0)
    return ((b == 0) & np.signbit(b) & odd) | ((b == 1.0) & np.isnan(e))


def test_kind0_gpow0_follows_c_pow():
    """every branch gpow0 spells out, b in {> 0, 0, -0, < 0, NaN} x e in {> 0, +-0, < 0, odd, even, non-integer, NaN}: the class of C's
    pow (numpy calls it), exact where pow is exact (0, 1, +-inf), within 16 x 2^-52 x max(1, |e ln |b||) elsewhere (the
    negative-base branch is exp(e log |b|) on the lean routines, whose product's rounding enters |e ln |b|| times).  Two recorded deviations are asserted as they are: a base of -0 with an odd
    integer exponent gives +0 / +inf (C: -0 / -inf; a clumping factor has no sign to carry), and pow(1, NaN) gives NaN (C: 1;
    clump = 1 makes pai / (1 - clump) a NaN in front of it, in the reference too)."""
    c, where = S.pooled(0)
    _, lit = S.yardsticks(0)
    s = where["pow_special"]
    b, e, got, want = c["x"][s], c["y"][s], device(0)["gpow0"][s], _f64(lit["gpow0"][s])
    known = _gpow0_known(b, e)
    cw, cg = S.value_class(want), S.value_class(got)
    print(f"gpow0: {len(b)} operand pairs, {np.count_nonzero(cw != cg)} of another class than C's pow, {known.sum()} of them recorded")
    assert np.array_equal(cw[~known], cg[~known]), (b[~known][cw[~known] != cg[~known]], e[~known][cw[~known] != cg[~known]])
    exact = ~known & (np.isin(want, (0.0, 1.0, -1.0)) | np.isinf(want))
    assert np.array_equal(got[exact], want[exact])
    fin = ~known & np.isfinite(want) & (want != 0)
    with np.errstate(all="ignore"):
        amp = np.maximum(1.0, np.nan_to_num(np.abs(e * np.log(np.abs(b))), nan=1.0, posinf=1.0))
    assert (np.abs(got[fin] - want[fin]) <= 16 * ULP * amp[fin] * np.abs(want[fin])).all()
    neg0 = known & (b == 0)
    assert np.array_equal(got[neg0], np.abs(want[neg0])) and not np.signbit(got[neg0]).any()
    assert np.isnan(got[known & (b == 1.0)]).all() and (known & (b == 1.0)).sum() == 1
    # clump = 0, the common special case: exactly 0 for every Kc > 0 of the bulk too
    cp = where["pow"]
    zero = c["x"][cp] == 0
    assert (device(0)["gpow0"][cp][zero] == 0).all()


def test_snow_albedo_is_the_integer_day_count():
    """hs from 0 to 47 and on: log of the INTEGER hs / 24 — 0.95 through the first day (log(0) = -inf), one value per day after"""
    c, where = S.pooled(0)
    truth, lit = S.yardsticks(0)
    s = where["albedo"]
    hs, got = c["x"][s], device(0)["snow_albedo"][s]
    assert (got[hs < 24] == 0.95).all() and (hs < 24).sum() == 24
    day1 = (hs >= 24) & (hs < 48)
    assert day1.sum() == 24 and (got[day1] == 78.3434 / 100.0).all()          # log(1) = 0: the same value all day, exactly
    for name in ("albedo_hi", "albedo_lo"):
        _check_clamp(name)
    assert (got >= 0.1).all() and (got <= 0.95).all()


# ---- branch-deciding comparisons --------------------------------------------------------------------------------------------------
def _check_clamp(name):
    _, kind, _, _, _, _, outf, _ = next(c for c in S.CLAMPS if c[0] == name)
    s, clamped, fragile, e, v = S.clamp_margin(name)
    n = len(clamped)
    print(f"{name}: {n} cases, {clamped.sum()} clamped on the yardstick, E {e:.3e}, {fragile.sum()} fragile")
    assert fragile.sum() <= S.MAX_FRAGILE * n
    if outf is None:
        print("  no device output carries this clamp by itself: nothing is checked on the device here (the floating bars hold what it enters)")
        return
    got = device(kind)[outf][s]
    hit = got == v
    sure = ~fragile
    bad = sure & (hit != clamped)
    print(f"  {bad.sum()} on the other side off the fragile cases")
    assert not bad.any(), np.nonzero(bad)[0][:10]
    assert clamped[sure].any() and (~clamped[sure]).any()
    # a fragile case holds one of the two sides' values: the clamp's own to the bit, or the unclamped one within 16 x the fp64
    # yardstick's error on it
    alt, e_alt = S.clamp_other_side(name)
    with np.errstate(all="ignore"):
        other = _f64(np.abs(got.astype(LD) - alt)) <= S.BAR_FACTOR * e_alt
    assert (hit | other)[fragile].all(), np.nonzero(fragile & ~(hit | other))[0][:10]


@pytest.mark.parametrize("name", [c[0] for c in S.CLAMPS if c[1] == 2])
def test_clamps_take_the_yardsticks_side(name):
    """inputs bisected to each clamp on the longdouble yardstick and stepped off by 2^20 ulp: where the yardstick clamps the device
    returns the clamp's value to the bit (0.9 (h - d), 0.0005, prec, 0.001, T0), where it does not, another value — which the
    16 E bars hold (the sets are part of the pooled cases).  |near| at mxnear and uzm at uf show in tv_below and the intercepted
    amount only as continuous values: the floating bars are their check."""
    _check_clamp(name)


def test_cank1_and_the_sign_of_zero():
    """si in {< 0, -0.0, 0, 1e-300, 1e-12, 1, NaN}: kd = 1 and Kc = 600 exactly for si <= 0 (-0.0 included), the quotient elsewhere;
    the extinction coefficient passes through"""
    c, where = S.pooled(1)
    _, lit = S.yardsticks(1)
    s, d = where["cank"], device(1)
    si = c["si"][s]
    off = si <= 0
    assert off.sum() >= 40 and (d["kd"][s][off] == 1.0).all() and (d["Kc"][s][off] == 600.0).all()
    assert np.array_equal(d["k"], c["kx"])
    tiny = si == 1e-300
    assert tiny.sum() == 12 and (np.abs(d["Kc"][s][tiny] / 1e300 - 1) <= 2 * ULP).all()
    assert np.isnan(d["Kc"][s][np.isnan(si)]).all() and np.isnan(d["kd"][s][np.isnan(si)]).all()
    on = si > 0
    assert (np.abs(d["kd"][s][on] - _f64(lit["kd"][s])[on]) <= 2 * ULP * np.abs(_f64(lit["kd"][s])[on])).all()


def test_deep_canopy_by_class():
    """pait h from 30 to 709, where S1 = exp(-h pait) is still a normal number: every output of ts_dif / ts_dir is finite, +-inf or
    NaN as the fp64 yardstick's.  Past 709.78 exp(h pait) overflows: the reference's 1 / S1 is inf (and its p4 exp(h pait) = 0 x
    inf a NaN) where the lean reciprocal of the denormal S1 is a NaN already — recorded, and asserted as it is."""
    c, where = S.pooled(1)
    truth, lit = S.yardsticks(1)
    s, d = where["deep"], device(1)
    depth = _f64(truth["h"][s] * c["pait"][s].astype(LD))
    normal = depth <= 709.0
    assert normal.sum() >= 590 and (depth > 700).sum() >= 8
    for f in S.DIF_FIELDS + S.DIR_FIELDS:
        cw, cg = S.value_class(_f64(lit[f][s]))[normal], S.value_class(d[f][s])[normal]
        assert np.array_equal(cw, cg), (f, depth[normal][cw != cg])
    past = depth >= 710.0
    assert past.sum() >= 6 and np.isnan(d["iS1"][s][past]).all() and not np.isfinite(_f64(lit["iS1"][s])[depth > 712]).any()
    print(f"deep canopy: {normal.sum()} cases up to pait h = 709 of the yardstick's classes; {past.sum()} past 710 with iS1 = NaN")


def test_sincos_outside_its_interval():
    """past 3.1416, negative, large: the quadrant route, within the bar (asserted with the floating fields); from 1e9 on and for NaN
    it gives NaN up, as the header says"""
    c, where = S.pooled(2)
    s, d = where["sincos"], device(2)
    x = c["x"][s]
    gone = ~(np.abs(x) < 1e9)
    assert gone.sum() >= 4 and np.isnan(d["sn"][s][gone]).all() and np.isnan(d["cs"][s][gone]).all()
    assert not np.isnan(d["sn"][s][~gone]).any()
    z = x == 0
    assert (d["sn"][s][z] == 0).all() and (d["cs"][s][z] == 1).all()
    assert (d["sn"][s][(x > 0) & (x < 3.14159)] > 0).all()


def test_profile_at_the_canopy_top_and_flags():
    """z = h takes the literal 4.293251 h branch (rz = Rc to the bit, Kh a NaN as inf / inf is in the reference); slope = +-0 is flat"""
    c, where = S.pooled(2)
    truth, lit = S.yardsticks(2)
    d = device(2)
    top = c["z"] == c["h"]
    assert top.sum() >= 16 and np.array_equal(d["rz"][top], d["Rc"][top])
    # (Kh itself is inf / 0 = inf in the reference and a NaN from the lean reciprocal of 0 here; what is made of it is a NaN in both)
    assert np.isnan(d["Kh"][top]).all() and np.isinf(_f64(lit["Kh"])[top]).all()
    assert np.isnan(d["tvb"][top]).all() and np.isnan(_f64(lit["tvb"])[top]).all()
    # just below the top cos(pi z / h) + 1 rounds to 0 and the reference's own formula is 0 x inf: for 0 < 1 - z / h <= 1.9e-9 the fp64
    # yardstick gives NaN, and so does the device, on exactly the same cases
    s = where["z_edges"]
    nan_lit = np.isnan(_f64(lit["rz"][s]))
    gap = 1.0 - c["z"][s] / c["h"][s]
    print(f"next to z = h: {nan_lit.sum()} NaN cases of the fp64 yardstick, 1 - z / h from {gap[nan_lit].min():.2e} to {gap[nan_lit].max():.2e}")
    assert nan_lit.sum() >= 300 and gap[nan_lit].min() > 0
    for f in ("rz", "Kg", "tvb"):
        assert np.array_equal(np.isnan(d[f][s]), np.isnan(_f64(lit[f][s]))), f
    assert np.array_equal(d["flat"], _f64(lit["flat"])) and (c["slope"] == 0).sum() >= 500
    flat = c["slope"] == 0
    assert np.array_equal(d["si1"][flat] > 0, _f64(lit["si1"])[flat] > 0)
    night = c["zend"] > 90.0
    assert night.sum() >= 1000 and (d["si0"][night] == 0).all()
    assert (d["si0"] >= 0).all() and (d["si1"] >= 0).all()


def test_nan_propagates_as_the_yardstick_says():
    """one NaN in every input plane of kinds 1 .. 3 in turn (a run of its own): each output is NaN exactly where the fp64
    yardstick's is"""
    for kind in (1, 2, 3):
        c, _ = S.pooled(kind)
        keys = S.KEYS[kind]
        base = {k: c[k][:len(keys)].copy() for k in keys}
        for j, k in enumerate(keys):
            base[k][j] = np.nan
        got = dict(zip(S.FIELDS[kind], run(kind, [base[k] for k in keys])))
        if kind == 1:
            want = R.twostream(np.float64, *(base[k] for k in keys[:5]))
            want.update(R.cank(np.float64, base["kx"], base["kcos"], base["si"]))
        elif kind == 2:
            want = R.canopy(np.float64, base)
        else:
            want = R.step_weather(np.float64, *(base[k] for k in keys))
        for f in S.FIELDS[kind]:
            assert np.array_equal(np.isnan(got[f]), np.isnan(_f64(want[f]))), (kind, f, np.isnan(got[f]), np.isnan(_f64(want[f])))


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_results_do_not_depend_on_the_launch(kind):
    """a lane's result is its own: any n gives the bits of the full run (the last block partly filled, one lane, one wave +- 1)"""
    planes = _planes(kind)
    full = np.stack([device(kind)[f] for f in S.FIELDS[kind]])
    assert full.shape[1] % 256 != 0
    for n, at in ((1, 0), (63, 5000), (65, 2100), (257, 5500)):
        part = run(kind, [p[at:at + n] for p in planes])
        assert np.array_equal(part.view(np.uint64), full[:, at:at + n].view(np.uint64)), (kind, n)
