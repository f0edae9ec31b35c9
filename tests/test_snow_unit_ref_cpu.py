"""The yardstick of tests/snow_ref.py itself, and the case sets of tests/snow_unit_cases.py, on the CPU: the longdouble evaluation
against mpmath at 50 digits, the fp64 evaluation against the oracle's restatements of the same reference functions, the share
of fragile cases of every clamp set, and the argument checks of mcf_selftest_snow."""
import ctypes as C

import numpy as np
import pytest

import snow_ref as R
import snow_unit_cases as S

LD = np.longdouble
F64 = np.float64


# ---- a 50-digit number type for snow_ref's formulas ---------------------------------------------------------------------------
def _mp_number():
    import mpmath            # (a missing mpmath is a failure: without this tie the truth of every GPU bar is unanchored)
    mp = mpmath.mp
    mp.dps = 50

    class N:
        """an mpf with IEEE behaviour at the poles (x / 0, log(0), sqrt(< 0)), as numpy's ufuncs find it in object arrays; an ndarray
        operand is left to numpy's elementwise loop"""
        __slots__ = ("v",)
        __hash__ = None

        def __init__(self, v):
            self.v = v.v if isinstance(v, N) else mp.mpf(v)

        def __float__(self):
            return float(self.v)

        def __neg__(self):
            return N(-self.v)

        def __abs__(self):
            return N(abs(self.v))

        def exp(self):
            return N(mp.exp(self.v))

        def log(self):
            return N(mp.nan if (self.v < 0 or mp.isnan(self.v)) else (-mp.inf if self.v == 0 else mp.log(self.v)))

        def sqrt(self):
            return N(mp.nan if self.v < 0 else mp.sqrt(self.v))

        def sin(self):
            return N(mp.nan if mp.isinf(self.v) else mp.sin(self.v))

        def cos(self):
            return N(mp.nan if mp.isinf(self.v) else mp.cos(self.v))

        def arctan(self):
            return N(mp.atan(self.v))

    def div(a, b):
        if b == 0:
            return mp.nan if (a == 0 or mp.isnan(a)) else (mp.inf if a > 0 else -mp.inf)
        return a / b

    def power(a, e):
        if a < 0 and e != mp.floor(e):
            return mp.nan
        if a == 0 and e < 0:
            return mp.inf
        return a ** e

    def binary(fn, wrap):
        def op(self, o):
            if isinstance(o, np.ndarray):
                return NotImplemented
            r = fn(self.v, o.v if isinstance(o, N) else mp.mpf(o))
            return N(r) if wrap else bool(r)
        return op
    for name, fn in (("add", lambda a, b: a + b), ("sub", lambda a, b: a - b), ("mul", lambda a, b: a * b), ("truediv", div), ("pow", power)):
        setattr(N, f"__{name}__", binary(fn, True))
        setattr(N, f"__r{name}__", binary(lambda a, b, fn=fn: fn(b, a), True))
    for name, fn in (("lt", lambda a, b: a < b), ("le", lambda a, b: a <= b), ("gt", lambda a, b: a > b), ("ge", lambda a, b: a >= b),
                     ("eq", lambda a, b: a == b), ("ne", lambda a, b: a != b)):
        setattr(N, f"__{name}__", binary(fn, False))
    return mp, N


def _mp_of(mp, x):
    """a longdouble as an mpf, exactly"""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_longdouble_yardstick_against_mpmath(kind):
    """The longdouble evaluation is the truth of the GPU tests: on a sample of every set it stays within 1/64 of the fp64
    yardstick's own error E (of the field's class) of a 50-digit evaluation of the same formulas.  It carries 11 more bits than
    fp64: 1/2048 where both round generically; on the aimed sets the fp64 operands are dyadic (z = h (1 - 2^-k)) and some of the
    fp64 evaluation's roundings are exact, which the longdouble's are not — the worst ratio measured is 1/105, for rh_canopy next
    to z = h.  1/64 of E moves an error measured against this truth by 0.1 % of the 16 E bar."""
    mp, N = _mp_number()
    c, where = S.pooled(kind)
    truth, lit = S.yardsticks(kind)
    n = len(c[S.KEYS[kind][0]])
    idx = np.concatenate([np.arange(s.start, s.stop)[::max(1, (s.stop - s.start) // 120)] for s in where.values()])
    sub = {k: c[k][idx] for k in S.KEYS[kind]}
    ref = S.evaluate(kind, N, sub)
    worst = 0.0
    for f, cl in S.classes(kind).items():
        e64 = np.asarray(S.field_error(lit[f], truth[f], f), dtype=F64)
        e_ld = np.full(len(idx), np.nan)
        for j, i in enumerate(idx):
            t, r = truth[f][i], ref[f][j].v
            if np.isfinite(t) and mp.isfinite(r) and (f in S.ABSOLUTE or r != 0):
                d = abs(_mp_of(mp, t) - r)
                e_ld[j] = float(d if f in S.ABSOLUTE or d == 0 else d / abs(r))
        for name, m in cl.items():
            full = m & np.isfinite(e64)
            ms = m[idx] & np.isfinite(e_ld)
            if ms.any() and full.any() and e64[full].max() > 0:
                ratio = e_ld[ms].max() / e64[full].max()
                worst = max(worst, ratio)
                assert ratio <= 1 / 64, (f, name, e_ld[ms].max(), e64[full].max())
    print(f"kind {kind}: longdouble against 50 digits on {len(idx)} of {n} cases: at most {worst:.2e} of the class's E")
    assert worst > 0


# ---- the fp64 yardstick against the oracle -------------------------------------------------------------------------------------
def _ulps(a, b):
    with np.errstate(all="ignore"):
        return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _report(name, a, b, bar, amp=None):
    """|a - b| in ulp against `bar` ulp, times the case's amplification `amp` (>= 1) where the formula cancels"""
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), name
    assert np.array_equal(a[~ok & ~np.isnan(a)], b[~ok & ~np.isnan(a)]), name
    u = _ulps(a[ok], b[ok])
    u[a[ok] == b[ok]] = 0
    lim = bar * (np.ones(ok.sum()) if amp is None else np.maximum(1.0, np.asarray(amp, dtype=F64)[ok]))
    print(f"  {name:12s} {np.count_nonzero(u):5d} of {ok.sum():5d} differ, at most {u.max() if u.size else 0:9.1f} ulp, {np.max(u / lim) if u.size else 0:.2f} of the bar")
    assert (u <= lim).all(), (name, np.nonzero(u > lim)[0][:5], u[u > lim][:5])


def test_fp64_yardstick_against_the_oracle(oracle):
    """The fp64 evaluation of tests/snow_ref.py against the oracle's C restatements of the same reference functions, elementwise on
    the random sets.  Both are literal fp64 evaluations on the host libm; numpy's vector exp / log / sin and the C library's differ
    in the last bit on some operands, so bit equality is not promised.  Bars, from what is measured and what amplifies it:
      4 ulp where nothing cancels (satvap, cank, the albedo, roughlength, solarindex off its zero);
      4 ulp x the amplification of the formula's own cancellation where something does: the zero-plane displacement at small pai
      (1 - exp(-s) amplifies a last-bit difference of exp by 1 / s, s = sqrt(7.5 pai), and 1 - (..) / s by h / d), the two-stream p's (the cancellation
      of D1 / D2 and of the p's own bracket, from the formula per case), Kh through Rc - rz."""
    lib = oracle.load()
    D = C.c_double
    dp = C.POINTER(D)
    lib.orc_zeroplanedis.restype = lib.orc_roughlength.restype = lib.orc_satvap.restype = lib.orc_solarindex.restype = D
    lib.orc_rhcanopy.restype = lib.orc_tvbelow.restype = lib.orc_canopysnowint.restype = D
    lib.orc_zeroplanedis.argtypes = [D] * 2
    lib.orc_roughlength.argtypes = [D] * 4
    lib.orc_satvap.argtypes = [D]
    lib.orc_solarindex.argtypes = [D] * 4 + [C.c_int]
    lib.orc_rhcanopy.argtypes = [D] * 4
    lib.orc_tvbelow.argtypes = [D] * 12
    lib.orc_canopysnowint.argtypes = [D] * 6
    lib.orc_tvabove.restype = lib.orc_twostreamdif_params.restype = lib.orc_twostreamdir_params.restype = lib.orc_snowalb.restype = None
    lib.orc_tvabove.argtypes = [D] * 9 + [dp]
    lib.orc_twostreamdif_params.argtypes = [D] * 5 + [dp]
    lib.orc_twostreamdir_params.argtypes = [D] * 13 + [dp]
    lib.orc_snowalb.argtypes = [dp, C.c_int, dp]
    eps = 2.0 ** -53

    # kind 0: satvap, the albedo
    c, where = S.pooled(0)
    _, lit = S.yardsticks(0)
    s = where["weather"]
    _report("satvap", lit["svp"][s], [lib.orc_satvap(v) for v in c["x"][s]], 4)
    prec = np.zeros(30000)
    prec[0] = 1.0
    alb = np.zeros(len(prec))
    lib.orc_snowalb(prec.ctypes.data_as(dp), len(prec), alb.ctypes.data_as(dp))        # hs = 0, 1, 2, ...: hours since the snowfall
    hs = c["x"][where["albedo"]]
    small = hs < len(prec)
    _report("snowalb", np.asarray(lit["snow_albedo"][where["albedo"]], dtype=F64)[small], alb[hs[small].astype(int)], 4)

    # kind 1: cank and the two-stream coefficients
    c, where = S.pooled(1)
    truth, lit = S.yardsticks(1)
    cls = S.classes(1)
    s = where["random"]
    idx = np.arange(s.start, s.stop)[::4]
    rng = np.random.default_rng(5)
    zen, si = rng.uniform(0, 1.7, 500), np.concatenate([rng.uniform(-0.2, 1.0, 490), [0.0, -0.0, 1e-300, 1e-12, 1.0, -1.0, 0.5, 0.25, 0.75, 0.1]])
    k, kcos = R.cank_zen(F64, zen, 0)
    mine = R.cank(F64, k, kcos, si)
    theirs = [lib.orc_cank(z, 1.0, v) for z, v in zip(zen, si)]
    for f in ("k", "kd", "Kc"):
        _report("cank " + f, mine[f], [getattr(t, f) for t in theirs], 4)
    dif, dr = np.zeros((len(idx), 14)), np.zeros((len(idx), 7))
    for j, i in enumerate(idx):
        a = [c[q][i] for q in ("pait", "lref", "ltra", "gref")]
        lib.orc_twostreamdif_params(a[0], 1.0, a[1], a[2], a[3], dif[j].ctypes.data_as(dp))
        p1, p2, p3, p4, om, aa, gma, J, dl, h, u1, S1, D1, D2 = dif[j]
        lib.orc_twostreamdir_params(a[0], om, aa, gma, J, dl, h, a[3], c["kd"][i], u1, S1, D1, D2, dr[j].ctypes.data_as(dp))

    # Only exp differs between the two libraries (S1, S2: a last bit on some operands).  What that bit grows to is the cancellation
    # of the sums it enters, (|term 1| + |term 2|) / |sum|: of D1 or D2 for p1 .. p4, plus that of the p's own bracket for p6 .. p10
    # (v1 / S1 (u1 - h) against (a + gma - h) S2 v2, p8 / (sig S1) (u2 + h) against v3, ...) — from the formula, per case.
    q = {k: np.asarray(v, dtype=F64)[idx] for k, v in lit.items()}
    ag = q["a"] + q["gma"]
    with np.errstate(all="ignore"):
        def cancel(x1, x2):
            return np.nan_to_num((np.abs(x1) + np.abs(x2)) / np.abs(x1 + x2), nan=1.0, posinf=1e300)
        cD1 = cancel((ag + q["h"]) * (q["u1"] - q["h"]) / q["S1"], -(ag - q["h"]) * (q["u1"] + q["h"]) * q["S1"])
        cD2 = cancel((q["u2"] + q["h"]) / q["S1"], -(q["u2"] - q["h"]) * q["S1"])
        amps = {"p1": cD1, "p2": cD1, "D1": cD1, "p3": cD2, "p4": cD2, "D2": cD2,
                "p6": cD1 + cancel((q["v1"] / q["S1"]) * (q["u1"] - q["h"]), -(ag - q["h"]) * q["S2"] * q["v2"]),
                "p7": cD1 + cancel((q["v1"] * q["S1"]) * (q["u1"] + q["h"]), -(ag + q["h"]) * q["S2"] * q["v2"]),
                "p9": cD2 + cancel((q["p8"] / (q["sig"] * q["S1"])) * (q["u2"] + q["h"]), q["v3"]),
                "p10": cD2 + cancel(((q["p8"] * q["S1"]) / q["sig"]) * (q["u2"] - q["h"]), q["v3"])}

    # (6 ulp, not 4, in front of it for the p's: S1's bit enters D with 1 + c, the quotient once more, and the roundings of the
    # operations behind it can fall the other way: 4 + c <= 6 c)
    def amp(f):
        return amps.get(f)
    for j, f in enumerate(("p1", "p2", "p3", "p4", "om", "a", "gma", None, "del", "h", "u1", "S1", "D1", "D2")):
        if f:
            _report(f, np.asarray(lit[f], dtype=F64)[idx], dif[:, j], 6 if f in amps and f[0] == "p" else 4, amp(f))
    for j, f in enumerate(("sig", "p5", "p6", "p7", "p8", "p9", "p10")):
        _report(f, np.asarray(lit[f], dtype=F64)[idx], dr[:, j], 6 if f in amps else 4, amp(f))

    # kind 2: zero-plane displacement, roughness length, rhcanopy, TVbelow, TVabove, canopysnowint, solarindex
    c, where = S.pooled(2)
    truth, lit = S.yardsticks(2)
    s = where["random"]
    idx = np.arange(s.start, s.stop)[::4]
    g = lambda q: c[q][idx]                      # noqa: E731
    L = lambda f: np.asarray(lit[f], dtype=F64)[idx]     # noqa: E731
    d0 = np.array([lib.orc_zeroplanedis(h, p) for h, p in zip(g("h"), g("pai"))])
    sq = np.sqrt(7.5 * np.maximum(g("pai"), 0.001))
    _report("zeroplanedis", L("d0"), d0, 4, (g("h") / L("d0")) * np.maximum(1.0, 1.0 / sq))
    _report("roughlength", L("zm0"), [lib.orc_roughlength(h, p, d, 0.0) for h, p, d in zip(g("h"), g("pai"), g("d"))], 4)
    rz = np.array([lib.orc_rhcanopy(u, h, d, z) for u, h, d, z in zip(g("uf"), g("h"), g("d"), g("z"))])
    _report("rhcanopy", L("rz"), rz, 4, 1.0 / (1.0 - g("z") / g("h")))
    tvb = [lib.orc_tvbelow(zr, z, d, h, p, u, ld, F, Fz, SH, SG, mx) for zr, z, d, h, p, u, ld, F, Fz, SH, SG, mx in
           zip(*(g(q) for q in ("zref", "z", "d", "h", "pai", "uf", "leafden", "Flux", "Fluxz", "SH", "SG", "mxnear")))]
    _report("TVbelow", L("tvb"), tvb, 4, L("Rc") / np.abs(L("Rc") - L("rz")))
    out = np.zeros((len(idx), 2))
    for j, a in enumerate(zip(*(g(q) for q in ("za", "zref", "h", "d", "zm", "T0", "tc", "ea")))):
        lib.orc_tvabove(*a, 1.0, out[j].ctypes.data_as(dp))
    with np.errstate(all="ignore"):
        lnr = np.log((g("za") - g("d")) / (0.2 * g("zm"))) / np.log((g("zref") - g("d")) / (0.2 * g("zm")))
        Tz, ez = L("Tz"), L("ez")
        amp_t = (np.abs(g("tc")) + np.abs((g("T0") - g("tc")) * (1 - lnr))) / np.abs(Tz)
        amp_e = (np.abs(g("ea")) + np.abs(ez - g("ea"))) / np.abs(ez) * 4.0          # (and satvap's own 4 ulp)
    _report("TVabove Tz", Tz, out[:, 0], 4, np.nan_to_num(amp_t, nan=1.0, posinf=1.0))
    _report("TVabove ez", ez, out[:, 1], 4, np.nan_to_num(amp_e, nan=1.0, posinf=1.0))
    # the interception model takes the air temperature: the load per branch area is made from it in both
    tc = g("tc")
    mine = R.canopysnowint(F64, g("hc"), g("pai"), g("uf"), g("prec"), R.snow_sint(F64, tc), g("Li"))
    theirs = [lib.orc_canopysnowint(h, p, u, pr, t, li) for h, p, u, pr, t, li in zip(g("hc"), g("pai"), g("uf"), g("prec"), tc, g("Li"))]
    wet = g("prec") > 0
    # three differences cancel: 1 - exp(-k2 prec) for a small exponent (1 / (k2 prec)), the canopy cover 1 - exp(-kc pai) for a thin
    # canopy (1 / (kc pai)), Lstr - Li for a nearly full one (Lstr / (Lstr - Li)); times 4 for the exponentials in a row
    pai = np.maximum(g("pai"), 0.001)
    Lstr = np.asarray(R.snow_sint(F64, tc)) * pai
    uzm = np.maximum(np.asarray(mine["uzm_raw"]), g("uf"))
    kc = 0.5 * np.sqrt(1.0 + (uzm / 0.8) ** 2)
    with np.errstate(all="ignore"):
        k2p = np.abs(np.asarray(mine["cis_raw"]) / (0.678 * (Lstr - g("Li"))))
        a_c = 4.0 * (Lstr / np.abs(Lstr - g("Li"))) * np.maximum(1.0, 1.0 / k2p) * np.maximum(1.0, 1.0 / (kc * pai))
    _report("canopysnowint", np.asarray(mine["cis"])[wet], np.asarray(theirs)[wet], 4, np.nan_to_num(a_c, nan=1.0, posinf=1e6)[wet])
    for mask, f in ((0, "si0"), (1, "si1")):
        si = np.array([lib.orc_solarindex(sl, asp, z, az, mask) for sl, asp, z, az in zip(g("slope"), g("aspect"), g("zend"), g("azid"))])
        mine = L(f)
        # cos(zend) cos(slope) + sin(zend) sin(slope) cos(azid - aspect) cancels towards grazing incidence: absolute 4 ulp of 1
        assert np.array_equal(mine == 0, si == 0) or (np.abs(mine - si)[(mine == 0) != (si == 0)] < 1e-15).all()
        print(f"  solarindex {mask}: largest |difference| {np.abs(mine - si).max():.2e}")
        assert (np.abs(mine - si) <= 4 * 2.0 ** -52).all()


# ---- the case sets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in S.CLAMPS])
def test_clamp_sets_are_stepped_off_far_enough(name):
    """At most 1 % of a clamp's set lies closer than 64 E to its threshold, judged with the two yardsticks alone; both sides of every
    clamp are met."""
    s, clamped, fragile, e, _ = S.clamp_margin(name)
    n = len(clamped)
    print(f"{name}: {n} cases, {clamped.sum()} clamped, E {e:.3e}, {fragile.sum()} fragile")
    assert fragile.sum() <= S.MAX_FRAGILE * n
    assert clamped[~fragile].sum() >= 20 and (~clamped)[~fragile].sum() >= 20


def test_case_sets_are_what_the_gpu_tests_rely_on():
    for kind in range(4):
        c, where = S.pooled(kind)
        n = len(c[S.KEYS[kind][0]])
        assert n % 256 != 0 and 2000 <= n <= 40000, (kind, n)
        assert len(S.KEYS[kind]) == R.NIN[kind] and len(S.FIELDS[kind]) == R.NOUT[kind]
    c, where = S.pooled(1)
    truth, _ = S.yardsticks(1)
    with np.errstate(all="ignore"):
        rel = np.asarray(np.abs(c["kd"].astype(LD) - truth["h"]) / truth["h"], dtype=F64)
    s = where["kd_near_h"]
    assert (rel[s] < 1e-14).sum() >= 100 and ((rel[s] > 1e-8) & (rel[s] < 1e-4)).sum() >= 100 and (c["kd"][s] > np.asarray(truth["h"][s], dtype=F64)).sum() >= 900
    om = c["lref"] + c["ltra"]
    assert (1 - om[where["om_near_1"]] < 1e-12).sum() >= 100 and (om < 1).all()
    assert (c["lref"][where["symmetric"]] == c["ltra"][where["symmetric"]]).all()
    depth = np.asarray(truth["h"], dtype=F64) * c["pait"]
    assert (depth[where["deep"]] >= 30).all() and (depth > 690).sum() >= 10
    assert set(np.unique(c["gref"][where["gref_ends"]])) == {0.1, 0.95}
    c, where = S.pooled(2)
    s = where["z_edges"]
    r = c["z"][s] / c["h"][s]
    assert (r == 1).sum() >= 16 and ((r < 1) & (1 - r < 1e-12)).sum() >= 100 and (r < 1e-12).sum() >= 100
    for q in (0.25, 0.5, 0.75):
        assert (r == q).sum() >= 4 and (r == np.nextafter(q, 0)).sum() >= 4 and (r == np.nextafter(q, 1)).sum() >= 4
    assert (c["z"] <= c["h"]).all() and ((c["z"] > 0) | (where["z_edges"].start <= np.arange(len(c["z"])))).all()
    c, where = S.pooled(0)
    x = c["x"][where["special"]]
    assert np.isnan(x).any() and (x == 0).sum() == 2 and np.isinf(x).sum() == 2 and ((x > 0) & (x < 2.3e-308)).sum() >= 2
    assert len(c["x"][where["pow_special"]]) == len(S.POW_B) * len(S.POW_E)
    hs = c["x"][where["albedo"]]
    assert set(range(48)) <= set(hs.astype(int))


def test_selftest_snow_refuses_by_name():
    """argument checks come before any device work: no GPU needed"""
    from microclimf_amd import _abi
    lib = _abi.load()
    x, out = np.zeros(32), np.zeros(29)
    p = lambda a: a.ctypes.data_as(_abi.c_double_p)       # noqa: E731
    for args in ((4, p(x), 2, p(out), 12, 1, 0), (-1, p(x), 2, p(out), 12, 1, 0), (0, p(x), 3, p(out), 12, 1, 0), (0, p(x), 2, p(out), 11, 1, 0),
                 (1, p(x), 8, p(out), 12, 1, 0), (2, p(x), 31, p(out), 23, 1, 0), (3, p(x), 5, p(out), 29, 1, 0),
                 (0, None, 2, p(out), 12, 1, 0), (0, p(x), 2, None, 12, 1, 0), (0, p(x), 2, p(out), 12, 0, 0), (0, p(x), 2, p(out), 12, 2 ** 31, 0)):
        with pytest.raises(_abi.McfError, match="mcf_selftest_snow"):
            _abi.check(lib.mcf_selftest_snow(*args))
