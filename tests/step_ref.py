"""Yardstick for the per-cell-step sun position and humidity helpers of array forcing (tests/test_step_gpu.py,
tests/test_step_ref_cpu.py): plain numpy, in the reference's own order of operations.

    juldayCpp, soltimeCpp, solpositionCpp        src/microclimfCpp.cpp:28-83
    PenmanMonteith2Cpp's step-only terms         cpp:1220-1247, with satvapCpp (cpp:480-490)
    the beam normalisation                       cpp:1122-1124
    what the callers derive from the position    cpp:85-132 (solarindexCpp's operands, cankCpp's clamp), cpp:2166-2167, 2222-2223
    .satvap, .dewpoint, .lapserate               R/internal.R:501-521, 545-550

Every function is written once over a number type T and is evaluated two ways: with T = np.longdouble as the truth, and
with T = np.float64 as "what a literal fp64 evaluation gives" — the difference of the two is the rounding error E that the
device routes are held to.  Both start from the same fp64 inputs, and both use the reference's constants as the fp64
numbers they are there (pi, torad, 0.261799, ...): the truth is the exact value of the reference's formulas, not of the
astronomy.  Integers (the Julian day) are computed once, in fp64 as the reference does."""
import numpy as np

LD = np.longdouble
F64 = np.float64

PI = 3.14159265358979323846            # cpp:14
TORAD = 3.14159265358979323846 / 180.0  # cpp:15: a constant of the reference, rounded to fp64 there
SB = 5.67e-8                            # cpp:16


def julday(year, month, day):
    """cpp:28-37 (integer arrays in, integer array out)"""
    year, month, day = (np.asarray(a, dtype=np.int64) for a in (year, month, day))
    dd = day + 0.5
    madj = month + (month < 3) * 12
    yadj = year + (month < 3) * -1
    j = np.trunc(365.25 * (yadj + 4716)) + np.trunc(30.6001 * (madj + 1)) + dd - 1524.5
    c = np.trunc(yadj / 100.0)              # the reference divides integers: truncation (years here are positive)
    b = (2 - c + np.trunc(c / 4)).astype(np.int64)
    return (j + (j > 2299160) * b).astype(np.int64)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + x.dtype.type(0.5)), np.ceil(x - x.dtype.type(0.5)))


def dir_index(v, step, n):
    """((int)round(v / step)) % n of cpp:2166-2167, negative remainders wrapped into range"""
    r = _round_half_away(v / v.dtype.type(step)).astype(np.int64)
    return np.mod(r, n)


def date_part(T, jd):
    """The part of cpp:39-83 that depends on the day alone: the equation of time (minutes) and the declination (radians)"""
    c = T
    jdT = np.asarray(jd).astype(T)
    pi = c(PI)
    m = c(6.24004077) + c(0.01720197) * (jdT - c(2451545.0))
    eot = c(-7.659) * np.sin(m) + c(9.863) * np.sin(c(2) * m + c(3.5932))
    dec = (pi * c(23.5) / c(180)) * np.cos(c(2) * pi * ((jdT - c(159.5)) / c(365.25)))
    return eot, dec


def solposition(T, year, month, day, hour, lat, lon, date_T=None):
    """cpp:39-83 over the number type T; every intermediate the checks need.  date_T: the number type of the day's part (eot,
    dec) where it is to differ from T — np.float64 with T = np.longdouble is "the exact site algebra on the fp64 date values",
    which is what two device routes that share their date part have in common."""
    c = T
    jd = julday(year, month, day)
    lt, lat, lon = (np.asarray(a, dtype=F64).astype(T) for a in (hour, lat, lon))
    pi = c(PI)
    with np.errstate(all="ignore"):
        eot, dec = (a.astype(T) for a in date_part(date_T or T, jd))
        st = lt + (c(4.0) * lon + eot) / c(60.0)
        latr = lat * pi / c(180.0)
        tt = c(0.261799) * (st - c(12))
        sindec, cosdec, sinlat, coslat, ctt, stt = np.sin(dec), np.cos(dec), np.sin(latr), np.cos(latr), np.cos(tt), np.sin(tt)
        coh = sindec * sinlat + cosdec * coslat * ctt
        z = np.arccos(coh) * (c(180) / pi)
        sh = coh
        hh = np.arctan(sh / np.sqrt(c(1) - sh * sh))
        sazi = cosdec * stt / np.cos(hh)
        num = sinlat * cosdec * ctt - coslat * sindec
        cazi = num / np.sqrt((cosdec * stt) ** 2 + num ** 2)
        sqt = c(1) - sazi * sazi
        sqt = np.where(sqt < 0, c(0), sqt)
        azi = c(180) + (c(180) * np.arctan(sazi / np.sqrt(sqt))) / pi
        azi = np.where(cazi < 0, np.where(sazi < 0, c(180) - azi, c(540) - azi), azi)
    return dict(jd=jd, eot=eot, dec=dec, sindec=sindec, cosdec=cosdec, tt=tt, coh=coh, s2=c(1) - coh * coh, zend=z,
                zenr=z * c(TORAD), sazi=sazi, cazi=cazi, azid=azi.astype(T))


def satvap_cpp(T, tc):
    """cpp:480-490"""
    c = T
    with np.errstate(all="ignore"):
        return np.where(tc > 0, c(0.61078) * np.exp(c(17.27) * tc / (tc + c(237.3))),
                        c(0.61078) * np.exp(c(21.875) * tc / (tc + c(265.5))))


# the fields of mcf_selftest_step kinds 0 and 1, in plane order (include/mcf.h)
STEP_FIELDS = ("CZ", "SZ", "TANSA", "ZEND", "COSC", "TANC", "TAN2C", "INV2COSC", "SAZ", "CAZ", "sindex", "windex", "ksat", "DE",
               "GHRRAD", "REM", "LAPK", "WFAC", "RBEAM", "RB", "GHRRAD2", "REM2", "MUPM", "INVMUPM", "SINDEC", "COSDEC", "COSA",
               "SINA", "julday")
STEP_INT_FIELDS = ("sindex", "windex", "ksat", "julday")
# ... of kind 2: the algebraic snow sun, then the literal one
SNOW_FIELDS = ("zend", "cosz", "cz", "sz", "tansa", "kx", "kcos", "sa", "ca", "sindex")
HUM_FIELDS = ("es", "ea", "tdew", "lapse")


def step_fields(T, inp, date_T=None):
    """What the solver's time set-up derives per step: the TF_ values of derive_time (mcf_device.hpp), each from the
    reference line it stands for.  `inp`: dict of fp64 arrays year, month, day, hour, winddir, lat, lon, tc, pk, rsw, rdif.
    date_T: see solposition."""
    c = T
    sp = solposition(T, inp["year"], inp["month"], inp["day"], inp["hour"], inp["lat"], inp["lon"], date_T)
    tc, pk, rsw, rdif = (np.asarray(inp[k], dtype=F64).astype(T) for k in ("tc", "pk", "rsw", "rdif"))
    pi = c(PI)
    o = {}
    with np.errstate(all="ignore"):
        zenr, zend = sp["zenr"], sp["zend"]
        o["CZ"], o["SZ"] = np.cos(zenr), np.sin(zenr)                      # cpp:1092, 93 / 96
        azr = sp["azid"] * c(TORAD)
        o["CAZ"], o["SAZ"] = np.cos(azr), np.sin(azr)
        o["TANSA"] = np.tan(pi / c(2.0) - zenr)                            # cpp:2222-2223
        zc = np.where(zenr > pi / c(2.0), pi / c(2.0), zenr)               # cpp:106
        cc, tn = np.cos(zc), np.tan(zc)
        o["COSC"], o["TANC"], o["TAN2C"], o["INV2COSC"] = cc, tn, tn * tn, c(1.0) / (c(2.0) * cc)
        o["ZEND"] = zend
        o["sindex"] = dir_index(sp["azid"], 15.0, 24)                      # cpp:2501
        o["windex"] = dir_index(np.asarray(inp["winddir"], dtype=F64).astype(T), 45.0, 8)
        o["ksat"] = (zend > pi / c(2.0)).astype(np.int64)                  # the degrees call, cpp:1425
        o["up"] = (zend <= c(90.0)).astype(np.int64)                       # cpp:88
        o["DE"] = satvap_cpp(T, tc + c(0.5)) - satvap_cpp(T, tc - c(0.5))  # cpp:1223
        tk = tc + c(273.15)
        o["GHRRAD"] = (c(4) * c(0.97) * c(SB) * tk ** 3) / c(29.3)          # cpp:1224
        o["REM"] = c(0.97) * c(SB) * tk ** 4                                 # cpp:1225
        la = np.where(tc >= 0, c(45068.7) - c(42.8428) * tc, c(51078.69) - c(4.338) * tc - c(0.06367) * tc * tc)
        o["LAPK"] = la / pk                                                # cpp:1233 without gV
        o["MUPM"] = la * (c(43.0) / pk)                                    # cpp:1245
        o["INVMUPM"] = c(1.0) / o["MUPM"]
        o["WFAC"] = c(0.018) / (c(8.31) * tk)                              # cpp:1268 without the matric potential
        rbeam = (rsw - rdif) / o["CZ"]                                     # cpp:1122
        rbeam = np.where(rbeam > c(1352.0), c(1352.0), rbeam)
        o["RBEAM"], o["RB"] = rbeam, rbeam * o["CZ"]
        o["GHRRAD2"], o["REM2"] = o["GHRRAD"], o["REM"]
        o["SINDEC"], o["COSDEC"] = sp["sindec"], sp["cosdec"]
        a = c(0.261799) * (np.asarray(inp["hour"], dtype=F64).astype(T) + sp["eot"] / c(60.0) - c(12.0))
        o["COSA"], o["SINA"] = np.cos(a), np.sin(a)
        o["EOT"] = sp["eot"]
        o["julday"] = sp["jd"]
        # the snow kernels' sun (mcf_snow_device.hpp sun_derive): cpp:3798, 85-132, 4357-4359 / 4604-4606
        o["zend"], o["cosz"] = zend, np.cos(zenr)
        o["cz"], o["sz"] = np.cos(zend * c(TORAD)), np.sin(zend * c(TORAD))
        o["ca"], o["sa"] = o["CAZ"], o["SAZ"]
        k = c(1.0) / (c(2.0) * cc)
        k = np.where(k > c(6000.0), c(6000.0), k)
        o["kx"], o["kcos"] = k, k * cc
        o["tansa"] = o["TANSA"]
        o["tansa_deg"] = np.tan((c(90) - zend) * c(TORAD))
    o["sp"] = sp
    return o


def humidity(T, tc, rh, pk):
    """.satvap, ea = es rh / 100, .dewpoint, .lapserate (R/internal.R:501-521, 545-550, 1230-1232); `tdew_w` is the value over
    water whose sign picks the branch"""
    c = T
    tc, rh, pk = (np.asarray(a, dtype=F64).astype(T) for a in (tc, rh, pk))
    with np.errstate(all="ignore"):
        es = np.where(tc < 0, c(0.61078) * np.exp(c(21.875) * tc / (tc + c(265.5))),
                      c(0.61078) * np.exp(c(17.27) * tc / (tc + c(237.3))))
        ea = es * rh / c(100)
        e0 = c(611.2) / c(1000)
        L = c(2.501) * c(10) ** 6 - c(2340) * tc
        it = c(1) / c(273.15) - (c(461.5) / L) * np.log(ea / e0)
        tdew = c(1) / it - c(273.15)
        e0 = c(610.78) / c(1000)
        L = c(2.834) * c(10) ** 6
        it = c(1) / c(273.15) - (c(461.5) / L) * np.log(ea / e0)
        tfrost = c(1) / it - c(273.15)
        rv = c(0.622) * ea / (pk - ea)
        tk = tc + c(273.15)
        lr = c(9.8076) * (c(1) + (c(2501000) * rv) / (c(287) * tk)) / (c(1003.5) + (c(0.622) * c(2501000) ** 2 * rv) / (c(287) * tk ** 2))
    return dict(es=es, ea=ea, tdew=np.where(tdew < 0, tfrost, tdew), tdew_w=tdew, lapse=lr)
