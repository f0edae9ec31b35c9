"""The yardstick of tests/step_ref.py itself, and the case sets of tests/step_cases.py, on the CPU:
the longdouble evaluation against mpmath at 50 digits, the fp64 evaluation against the oracle's restatement of solpositionCpp,
the Julian day against the calendar, and the properties of the case sets that tests/test_step_gpu.py relies on."""
import ctypes as C
import datetime

import numpy as np
import pytest

import step_cases as S
import step_ref as R

LD = np.longdouble


# ---- the reference's formulas once more, scalar, in mpmath ---------------------------------------------------------------------
def _mp_step(mp, jd, hour, lat, lon, winddir, tc, pk, rsw, rdif):
    f = mp.mpf
    pi, torad = f(R.PI), f(R.TORAD)
    m = f(6.24004077) + f(0.01720197) * (f(jd) - f(2451545.0))
    eot = f(-7.659) * mp.sin(m) + f(9.863) * mp.sin(2 * m + f(3.5932))
    st = f(hour) + (f(4.0) * f(lon) + eot) / f(60.0)
    latr = f(lat) * pi / f(180.0)
    tt = f(0.261799) * (st - 12)
    dec = (pi * f(23.5) / 180) * mp.cos(2 * pi * ((f(jd) - f(159.5)) / f(365.25)))
    coh = mp.sin(dec) * mp.sin(latr) + mp.cos(dec) * mp.cos(latr) * mp.cos(tt)
    z = mp.acos(coh) * (180 / pi)
    root = mp.sqrt(1 - coh * coh)
    hh = mp.atan(coh / root) if root != 0 else pi / 2
    sazi = mp.cos(dec) * mp.sin(tt) / mp.cos(hh)
    num = mp.sin(latr) * mp.cos(dec) * mp.cos(tt) - mp.cos(latr) * mp.sin(dec)
    cazi = num / mp.sqrt((mp.cos(dec) * mp.sin(tt)) ** 2 + num ** 2)
    sqt = 1 - sazi * sazi
    if sqt < 0:
        sqt = f(0)
    azi = 180 + (180 * (mp.atan(sazi / mp.sqrt(sqt)) if sqt != 0 else mp.sign(sazi) * pi / 2)) / pi
    if cazi < 0:
        azi = 180 - azi if sazi < 0 else 540 - azi
    zenr = z * torad
    o = dict(coh=coh, ZEND=z, CZ=mp.cos(zenr), SZ=mp.sin(zenr), CAZ=mp.cos(azi * torad), SAZ=mp.sin(azi * torad),
             TANSA=mp.tan(pi / 2 - zenr), SINDEC=mp.sin(dec), COSDEC=mp.cos(dec), EOT=eot, azid=azi)
    zc = pi / 2 if zenr > pi / 2 else zenr
    cc, tn = mp.cos(zc), mp.tan(zc)
    o.update(COSC=cc, TANC=tn, TAN2C=tn * tn, INV2COSC=1 / (2 * cc))
    k = 1 / (2 * cc)
    k = f(6000.0) if k > 6000 else k
    o.update(kx=k, kcos=k * cc, tansa_deg=mp.tan((90 - z) * torad), cz=mp.cos(z * torad), sz=mp.sin(z * torad))
    a = f(0.261799) * (f(hour) + eot / 60 - 12)
    o.update(COSA=mp.cos(a), SINA=mp.sin(a))
    o["sindex"] = int(mp.floor(azi / 15 + f(0.5))) % 24
    o["up"], o["ksat"] = bool(z <= 90), bool(z > pi / 2)
    if tc == tc:
        t = f(tc)
        sat = lambda x: f(0.61078) * mp.exp(f(17.27) * x / (x + f(237.3))) if x > 0 else f(0.61078) * mp.exp(f(21.875) * x / (x + f(265.5)))   # noqa: E731
        tk = t + f(273.15)
        la = f(45068.7) - f(42.8428) * t if t >= 0 else f(51078.69) - f(4.338) * t - f(0.06367) * t * t
        rbeam = (f(rsw) - f(rdif)) / o["CZ"]
        rbeam = f(1352.0) if rbeam > 1352 else rbeam
        o.update(DE=sat(t + f(0.5)) - sat(t - f(0.5)), GHRRAD=(4 * f(0.97) * f(R.SB) * tk ** 3) / f(29.3), REM=f(0.97) * f(R.SB) * tk ** 4,
                 LAPK=la / f(pk), MUPM=la * (43 / f(pk)), WFAC=f(0.018) / (f(8.31) * tk), RBEAM=rbeam, RB=rbeam * o["CZ"])
        o["INVMUPM"] = 1 / o["MUPM"]
    return o


def _mp_of(mp, x):
    """a longdouble as an mpf, exactly"""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


MP_FIELDS = ("CZ", "SZ", "TANSA", "ZEND", "COSC", "TANC", "TAN2C", "INV2COSC", "SAZ", "CAZ", "DE", "GHRRAD", "REM", "LAPK", "WFAC", "RBEAM",
             "RB", "MUPM", "INVMUPM", "SINDEC", "COSDEC", "COSA", "SINA", "EOT", "kx", "kcos", "tansa_deg", "cz", "sz")


def test_longdouble_yardstick_against_mpmath():
    """The longdouble evaluation is the truth of the GPU tests: on the directed sets it stays within 1/256 of the fp64 yardstick's
    own error E of a 50-digit evaluation, per field and conditioning class (it carries 11 more bits than fp64: 1/2048), and its
    integers are the 50-digit ones off the fragile cases."""
    import mpmath            # (a missing mpmath is a failure: without this tie the truth of every GPU bar is unanchored)
    mp = mpmath.mp
    mp.dps = 50
    inp, where = S.pooled()
    truth, lit = S.yardsticks()
    idx = np.concatenate([np.arange(where[n].start, where[n].stop)[::{"sector": 4, "sector_ulp": 8}.get(n, 1)] for n in S.SETS
                          if n != "random"] + [np.arange(0, 20000, 40)])
    frag = {k: np.zeros(len(inp["hour"]), dtype=bool) for k in ("sector", "up_f", "ksat_f")}
    for n in S.SETS:
        m = S.margins(n)
        frag["sector"][where[n]] = m["sector"] | ~m["assert_sector"]
        frag["up_f"][where[n]], frag["ksat_f"][where[n]] = m["up_f"], m["ksat_f"]
    e_ld = {f: np.full(len(idx), np.nan) for f in MP_FIELDS}
    for j, i in enumerate(idx):
        o = _mp_step(mp, int(truth["julday"][i]), *(float(inp[k][i]) for k in ("hour", "lat", "lon", "winddir", "tc", "pk", "rsw", "rdif")))
        for f in MP_FIELDS:
            if f in o:
                d = abs(_mp_of(mp, truth[f][i]) - o[f])
                e_ld[f][j] = float(d if f in S.ABSOLUTE or d == 0 else d / abs(o[f]))
        if not frag["sector"][i]:
            assert o["sindex"] == truth["sindex"][i]
        if not frag["up_f"][i]:
            assert o["up"] == bool(truth["up"][i])
        if not frag["ksat_f"][i]:
            assert o["ksat"] == bool(truth["ksat"][i])
    cl = S.classes()
    worst = 0.0
    for f in MP_FIELDS:
        e64 = np.asarray(S.field_error(lit[f], truth[f], f), dtype=np.float64)[idx]
        for c in (("s2>=1e-2", "1e-6<=s2<1e-2", "1e-12<=s2<1e-6") if f in S.SOLAR else ("_keep",)) + (("az90",) if f in S.AZIMUTH else ()):
            m = cl[c][idx] & np.isfinite(e_ld[f])
            if f in S.AZIMUTH and c != "az90":
                m &= ~cl["_near90"][idx]
            if m.any() and e64[m].max() > 0:
                ratio = e_ld[f][m].max() / e64[m].max()
                worst = max(worst, ratio)
                assert ratio <= 1 / 256, (f, c, e_ld[f][m].max(), e64[m].max())
    print(f"longdouble against 50 digits: at most {worst:.2e} of the fp64 yardstick's error E, over {len(idx)} cases")


def test_fp64_yardstick_against_the_oracle(oracle):
    """zenith and azimuth of the fp64 evaluation within 4 ulp of the oracle's restatement of solpositionCpp (both on the host libm;
    bit equality across numpy and C is not promised)"""
    lib = oracle.load()
    lib.orc_solpositionv.restype = None
    inp, where = S.pooled()
    _, lit = S.yardsticks()
    s = where["random"]
    n = s.stop - s.start
    y, m, d = (np.ascontiguousarray(inp[k][s], dtype=np.int32) for k in ("year", "month", "day"))
    hour = np.ascontiguousarray(inp["hour"][s])
    zen, azi, si = np.zeros(n), np.zeros(n), np.zeros(n)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    for i in range(n):
        at = lambda a, t: C.cast(a.ctypes.data + a.itemsize * i, t)           # noqa: E731
        lib.orc_solpositionv(C.c_int(1), at(y, ip), at(m, ip), at(d, ip), at(hour, dp), C.c_double(inp["lat"][s][i]),
                             C.c_double(inp["lon"][s][i]), C.c_double(0.0), C.c_double(180.0), at(zen, dp), at(azi, dp), at(si, dp))
    # Zenith: 4 ulp on every case.  Azimuth: 4 ulp wherever neither cancellation of the reference's formula amplifies a last-bit
    # difference between numpy's vector sin / cos and the C library's (they differ on about one operand in ten): s2 >= 1/4 (30
    # degrees from the zenith and the nadir) and 1 - sazi^2 >= 1/4 (30 degrees from azimuth 90 / 270).  Elsewhere sazi carries
    # 1 / sqrt(s2) of such a difference and the azimuth's atan 1 / sqrt(1 - sazi^2) of sazi's: there the bar is 4 ulp times that
    # amplification.  No case is left without a bar.
    s2, sq = lit["sp"]["s2"][s], np.maximum(1.0 - lit["sp"]["sazi"][s] ** 2, 1e-300)
    well = (s2 >= 0.25) & (sq >= 0.25)
    bar = np.where(well, 4.0, 4.0 / np.sqrt(s2 * sq))
    assert well.sum() >= 5000 and (bar >= 4.0).all()
    uz = np.abs(lit["sp"]["zend"][s] - zen) / np.spacing(np.abs(zen))
    ua = np.abs(lit["sp"]["azid"][s] - azi) / np.spacing(np.abs(azi))
    print(f"fp64 yardstick against the oracle: zenith {np.count_nonzero(uz)} of {n} differ, at most {uz.max():.1f} ulp; azimuth "
          f"{np.count_nonzero(ua)} differ, at most {ua[well].max():.1f} ulp on the {well.sum()} well-conditioned cases, {ua.max():.1f} ulp "
          f"overall, at most {np.max(ua / bar):.2f} of the case's bar")
    assert uz.max() <= 4.0
    assert (ua <= bar).all()


def test_julday_is_the_calendar_day():
    """every day from 1900 to 2100 (both century terms, Feb 29, the month < 3 adjustment): the astronomical Julian day number"""
    o0, o1 = datetime.date(1900, 1, 1).toordinal(), datetime.date(2100, 12, 31).toordinal()
    days = [datetime.date.fromordinal(o) for o in range(o0, o1 + 1)]
    jd = R.julday([d.year for d in days], [d.month for d in days], [d.day for d in days])
    assert np.array_equal(jd, np.arange(o0, o1 + 1) + 1721425)


def test_case_sets_are_what_the_gpu_tests_rely_on():
    inp, where = S.pooled()
    truth, _ = S.yardsticks()
    assert len(inp["hour"]) % 256 != 0 and len(S.humidity_case()["tc"]) % 256 != 0
    assert where["random"] == slice(0, 20000) and len(inp["hour"]) < 40000
    for n in S.SETS:
        m = S.margins(n)
        share = [(m["sector"] & m["assert_sector"]).mean(), m["up_f"].mean(), m["ksat_f"].mean()]
        print(f"{n}: {len(m['up'])} cases, E azimuth {m['e_az']:.2e} deg, E coh {m['e_coh']:.2e}, fragile shares {share}")
        if n in S.STEPPED:
            # judged on the fp64 values of the day's part, the yardstick flags none of the stepped-off cases
            md = S.margins(n, True)
            print(f"   on the fp64 date row: E azimuth {md['e_az']:.2e} deg, E coh {md['e_coh']:.2e}")
            assert not (md["sector"] & md["assert_sector"]).any() and not md["up_f"].any() and not md["ksat_f"].any()
        elif n != "sector_ulp":
            assert max(share) <= S.MAX_FRAGILE
    # 48 site-days, each crossing sector boundaries; sunrise and sunset on both sides
    sd, (site, lo, hi, s_lo, s_hi), (hsite, _, _, _, _) = S._boundaries()
    assert len(set(site)) >= 40 and len(site) >= 500 and len(hsite) >= 60
    m = S.margins("sector_ulp")
    k = len(site)
    assert (m["sindex"][:k] == (s_lo + 1) % 24).all() and (m["sindex"][k:2 * k] == (s_hi + 1) % 24).all()
    h = where["horizon"]
    coh = np.asarray(truth["sp"]["coh"][h], dtype=np.float64)
    assert ((coh > 0) & (coh < 1e-6)).sum() >= 40 and ((coh < 0) & (coh > -1e-6)).sum() >= 40
    lat = inp["lat"][h]
    assert ((np.abs(lat) >= 80) & (coh > 0)).sum() >= 30 and ((np.abs(lat) >= 80) & (coh < 0)).sum() >= 30        # polar day, night
    z = where["zenith"]
    coh = truth["sp"]["coh"][z]
    assert np.asarray((coh > S.zenith_threshold()) & (coh <= LD(S.NEARZEN_BEFORE))).sum() >= 20
    assert np.asarray(coh < S.zenith_threshold()).sum() >= 100 and float(coh.min()) < 0.99901
    assert np.asarray(1 - coh < 1e-12).sum() >= 12
    cl = S.classes()
    assert all(cl[c].sum() >= 50 for c in ("s2>=1e-2", "1e-6<=s2<1e-2", "1e-12<=s2<1e-6", "az90"))
    assert np.isnan(inp["tc"]).sum() == 1 and (inp["rsw"] < inp["rdif"]).sum() >= 100 and ((inp["rsw"] == 0) & (inp["rdif"] == 0)).sum() >= 100
    fragile, _ = S.humidity_margin()
    assert fragile.mean() <= S.MAX_FRAGILE


def test_selftest_step_refuses_by_name():
    """argument checks come before any device work: no GPU needed"""
    from microclimf_amd import _abi
    lib = _abi.load()
    x, out = np.zeros(11), np.zeros(29)
    p = lambda a: a.ctypes.data_as(_abi.c_double_p)       # noqa: E731
    for args in ((4, p(x), 11, p(out), 29, 1, 0), (0, p(x), 3, p(out), 29, 1, 0), (3, p(x), 3, p(out), 29, 1, 0),
                 (0, None, 11, p(out), 29, 1, 0), (0, p(x), 11, p(out), 29, 0, 0)):
        with pytest.raises(_abi.McfError, match="mcf_selftest_step"):
            _abi.check(lib.mcf_selftest_step(*args))
