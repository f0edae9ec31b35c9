"""Yardstick for the device physics of the snow kernels (mcf_snow_device.hpp, run elementwise by mcf_selftest_snow;
tests/test_snow_unit_gpu.py, tests/test_snow_unit_ref_cpu.py): plain numpy, in the reference's own order of operations.

    cankCpp (x = 1)                               src/microclimfCpp.cpp:104-132
    twostreamdifCpp / twostreamdirCpp (x = 1)     cpp:134-185
    zeroplanedisCpp / roughlengthCpp (psi_h = 0)  cpp:294-310
    satvapCpp, dewpointCpp, the latent heats      cpp:480-496, 502-507, 3879-3884
    TVabove, rhcanopy, TVbelow                    cpp:1298-1313, 1365-1409
    canopysnowintCpp                              cpp:3713-3739
    snowalbCpp's albedo of an hour count          cpp:3766-3768, with its INTEGER hs / 24
    the density law                               cpp:3952-3955
    the step terms                                cpp:4226-4228, 498-511, 280-291, 1220-1247
    solarindexCpp                                 cpp:85-102
    .satvap, .lapserate                           R/internal.R:501-511, 545-550

Every function is written once over a number type T and evaluated two ways, as tests/step_ref.py does: T = np.longdouble is
the truth, T = np.float64 "what a literal fp64 evaluation gives"; their difference is the rounding error E the device is
held to.  Both start from the same fp64 inputs and use the reference's constants as the fp64 numbers they are there.  The
operand order is the reference's, not the device's: quotients stay quotients (p.p8 / p.sig, 1.0 / gref), pow(x, 2.0) is a
product as the C library makes it, cos(atan(t)) stays cos(atan(t))."""
import numpy as np

LD = np.longdouble
F64 = np.float64

PI = 3.14159265358979323846
TORAD = 3.14159265358979323846 / 180.0
SB = 5.67e-8
KA = 0.4


def _cast(T, x):
    """fp64 values as numbers of type T: a numpy type, or any class of numbers built from a float (object arrays; the 50-digit
    numbers of tests/test_snow_unit_ref_cpu.py)"""
    x = np.asarray(x, dtype=F64)
    if isinstance(T, type) and issubclass(T, np.generic):
        return x.astype(T)
    out = np.empty(x.shape, dtype=object)
    out.ravel()[:] = [T(float(v)) for v in x.ravel()]
    return out


def _a(T, *xs):
    return tuple(_cast(T, x) for x in xs)


def satvap(T, tc):
    """cpp:480-490"""
    c = T
    with np.errstate(all="ignore"):
        return np.where(tc > 0, c(0.61078) * np.exp(c(17.27) * tc / (tc + c(237.3))), c(0.61078) * np.exp(c(21.875) * tc / (tc + c(265.5))))


def dewpoint(T, ea):
    """cpp:493-496"""
    c = T
    with np.errstate(all="ignore"):
        return c(243.5) * np.log(ea / c(0.6112)) / (c(17.67) - np.log(ea / c(0.6112)))


def radem(T, tc):
    """cpp:24-26: pow(tc + 273.15, 4)"""
    return (tc + T(273.15)) ** 4


def latent_lt0(T, t):
    """the `T < 0` flavour, cpp:3879-3884"""
    c = T
    return np.where(t < 0, c(51078.69) - c(4.338) * t - c(0.06367) * t * t, c(45068.7) - c(42.8428) * t)


def latent_ge0(T, t):
    """the `te >= 0` flavour, cpp:502-507, 1227-1232"""
    c = T
    return np.where(t >= 0, c(45068.7) - c(42.8428) * t, c(51078.69) - c(4.338) * t - c(0.06367) * t * t)


def snow_albedo(T, hs):
    """cpp:3766-3768 for integer hours hs since snowfall: (raw value, clamped value)"""
    c = T
    days = _cast(T, (np.asarray(hs, dtype=np.int64) // 24).astype(F64))
    with np.errstate(all="ignore"):
        raw = (c(-9.8740) * np.log(days) + c(78.3434)) / c(100.0)
    alb = np.where(raw > c(0.95), c(0.95), raw)
    alb = np.where(alb < c(0.1), c(0.1), alb)
    return raw, alb


def satvap_r(T, tc):
    """.satvap, R/internal.R:501-511"""
    c = T
    with np.errstate(all="ignore"):
        return np.where(tc < 0, c(0.61078) * np.exp(c(21.875) * tc / (tc + c(265.5))), c(0.61078) * np.exp(c(17.27) * tc / (tc + c(237.3))))


def lapserate_r(T, tc, ea, pk):
    """.lapserate, R/internal.R:545-550"""
    c = T
    with np.errstate(all="ignore"):
        rv = c(0.622) * ea / (pk - ea)
        tk = tc + c(273.15)
        return c(9.8076) * (c(1) + (c(2501000) * rv) / (c(287) * tk)) / (c(1003.5) + (c(0.622) * c(2501000) ** 2 * rv) / (c(287) * tk ** 2))


def scalars(T, x, y):
    """kind 0's floating outputs on ordinary operands"""
    c = T
    x, y = _a(T, x, y)
    with np.errstate(all="ignore"):
        ea = satvap_r(T, x) * c(80.0) / c(100)
        return dict(gexp=np.exp(x), glog=np.log(x), gsqrt=np.sqrt(x), gpow0=np.power(x, y), svp=satvap(T, x), dewpoint=dewpoint(T, x),
                    rad4=radem(T, x), latent_lt0=latent_lt0(T, x), satvap_r=satvap_r(T, x), lapserate_r=lapserate_r(T, x, ea, y))


def cank(T, k, kcos, si):
    """cpp:107, 123-126 behind the extinction coefficient k (x = 1) and k cos(zenr), which the step hands over"""
    c = T
    k, kcos, si = _a(T, k, kcos, si)
    si = np.where(si < 0, c(0), si)
    with np.errstate(all="ignore"):
        kd = np.where(si == 0, c(1.0), kcos / si)
        Kc = np.where(si == 0, c(600.0), c(1.0) / si)
    return dict(k=k, kd=kd, Kc=Kc)


def cank_zen(T, zenr, si):
    """cpp:104-132 for x = 1 from the zenith angle: (k, k cos(zenr')) as sun_derive hands them over, then cank"""
    c = T
    zenr, = _a(T, zenr)
    zr = np.where(zenr > c(PI) / c(2.0), c(PI) / c(2.0), zenr)
    k = c(1.0) / (c(2.0) * np.cos(zr))
    k = np.where(k > c(6000.0), c(6000.0), k)
    return k, k * np.cos(zr)


def twostream(T, pait, lref, ltra, gref, kd):
    """cpp:134-185 for x = 1; the device's extra fields from the reference's quantities: iS1 = 1 / S1, iD1 = 1 / D1, iD2 = 1 / D2,
    isig = 1 / sig with sig the NEGATED determinant (params.sig of cpp:179)"""
    c = T
    pait, lref, ltra, gref, kd = _a(T, pait, lref, ltra, gref, kd)
    o = {}
    with np.errstate(all="ignore"):
        om = lref + ltra
        a = c(1.0) - om
        dl = lref - ltra
        J = c(1.0) / c(3.0)
        gma = c(0.5) * (om + J * dl)
        h = np.sqrt(a * a + c(2.0) * a * gma)
        S1 = np.exp(-h * pait)
        u1 = a + gma * (c(1.0) - c(1.0) / gref)
        u2 = a + gma * (c(1.0) - gref)
        D1 = (a + gma + h) * (u1 - h) * c(1.0) / S1 - (a + gma - h) * (u1 + h) * S1
        D2 = (u2 + h) * c(1.0) / S1 - (u2 - h) * S1
        o.update(om=om, a=a, gma=gma, h=h, S1=S1, iS1=c(1.0) / S1, iD1=c(1.0) / D1, iD2=c(1.0) / D2, u1=u1, u2=u2, D1=D1, D2=D2)
        o["del"] = dl
        o["p1"] = (gma / (D1 * S1)) * (u1 - h)
        o["p2"] = (-gma * S1 / D1) * (u1 + h)
        o["p3"] = (c(1.0) / (D2 * S1)) * (u2 + h)
        o["p4"] = (-S1 / D2) * (u2 - h)
        sig = kd * kd + gma * gma - (a + gma) * (a + gma)
        ss = c(0.5) * (om + J * dl / kd) * kd
        sstr = om * kd - ss
        S2 = np.exp(-kd * pait)
        p5 = -ss * (a + gma - kd) - gma * sstr
        v1 = ss - (p5 * (a + gma + kd)) / sig
        v2 = ss - gma - (p5 / sig) * (u1 + kd)
        o["p5"] = p5
        o["p6"] = (c(1.0) / D1) * ((v1 / S1) * (u1 - h) - (a + gma - h) * S2 * v2)
        o["p7"] = (c(-1.0) / D1) * ((v1 * S1) * (u1 + h) - (a + gma + h) * S2 * v2)
        nsig = -sig
        p8 = sstr * (a + gma + kd) - gma * ss
        v3 = (sstr + gma * gref - (p8 / nsig) * (u2 - kd)) * S2
        o.update(sig=nsig, isig=c(1.0) / nsig, S2=S2, p8=p8)
        o["p9"] = (c(-1) / D2) * ((p8 / (nsig * S1)) * (u2 + h) + v3)
        o["p10"] = (c(1) / D2) * (((p8 * S1) / nsig) * (u2 - h) + v3)
        o.update(v1=v1, v2=v2, v3=v3)        # (the brackets' operands: what cancels in p6 .. p10)
        o["kd2_h2"] = kd * kd - h * h          # what sig is, algebraically: -(sig) = kd^2 - h^2 (gma^2 - (a + gma)^2 = -h^2)
    return o


def zeroplane(T, h, pai):
    """cpp:294-299"""
    c = T
    h, pai = _a(T, h, pai)
    pai = np.where(pai < c(0.001), c(0.001), pai)
    with np.errstate(all="ignore"):
        return (c(1.0) - (c(1.0) - np.exp(-np.sqrt(c(7.5) * pai))) / np.sqrt(c(7.5) * pai)) * h


def roughlength(T, h, pai, d):
    """cpp:302-310 with psi_h = 0: (zm before the clamps, 0.9 (h - d), zm)"""
    c = T
    h, pai, d = _a(T, h, pai, d)
    with np.errstate(all="ignore"):
        Be = np.sqrt(c(0.003) + (c(0.2) * pai) / c(2))
        raw = (h - d) * np.exp(-c(KA) / Be) * np.exp(c(KA) * c(0.0))
    cap = c(0.9) * (h - d)
    zm = np.where(raw > cap, cap, raw)
    zm = np.where(zm < c(0.0005), c(0.0005), zm)
    return raw, cap, zm


def snow_sint(T, tc):
    """cpp:3728-3729: the maximum snow load per branch area"""
    c = T
    tc, = _a(T, tc)
    with np.errstate(all="ignore"):
        rhos = c(67.92) + c(51.25) * np.exp(tc / c(2.59))
        return c(6.2) * (c(0.26) + c(46) / rhos)


def canopysnowint(T, hgt, pai, uf, prec, S, Li):
    """cpp:3713-3739 with S (cpp:3729) handed in: dict cis, and the operands of its two branches (uzm_raw against uf, cis_raw
    against prec)"""
    c = T
    hgt, pai, uf, prec, S, Li = _a(T, hgt, pai, uf, prec, S, Li)
    hgt = np.where(hgt < c(0.001), c(0.001), hgt)
    pai = np.where(pai < c(0.001), c(0.001), pai)
    with np.errstate(all="ignore"):
        Be = np.sqrt(c(0.003) + (c(0.2) * pai) / c(2.0))
        uh = uf / Be
        a = pai / hgt
        Lc = c(1.0) / (c(0.25) * a)
        Lm = c(2.0) * (Be * Be * Be) * Lc
        k1 = Be / Lm
        uzm_raw = (uh / (hgt * k1)) * (c(1) - np.exp(-k1 * hgt))
        uzm = np.where(uzm_raw < uf, uf, uzm_raw)
        Lstr = S * pai
        Z = np.arctan(uzm / c(0.8))
        kc = c(1.0) / (c(2.0) * np.cos(Z))
        Cp = c(1.0) - np.exp(-kc * pai)
        k2 = Cp / Lstr
        I1 = (Lstr - Li) * (c(1.0) - np.exp(-k2 * prec))
        raw = I1 * c(0.678)
        cis = np.where(raw > prec, prec, raw)
    return dict(cis=cis, cis_raw=raw, uzm_raw=uzm_raw, kcpai=kc * pai, k2prec=k2 * prec, room=(Lstr - Li) / Lstr)


def snow_density(T, sdp, depth, age_h):
    """cpp:3952-3955"""
    c = T
    s0, s1, s2, s3, depth, age_h = _a(T, *sdp, depth, age_h)
    with np.errstate(all="ignore"):
        return ((s0 - s1) * (c(1.0) - np.exp(-s2 * depth / c(100.0) - s3 * age_h / c(24.0))) + s1) * c(1000.0)


def rhcanopy(T, uf, h, d, z):
    """cpp:1365-1380: (rHa before the clamp, rHa)"""
    c = T
    uf, h, d, z = _a(T, uf, h, d, z)
    pi = c(PI)
    with np.errstate(all="ignore"):
        a2 = c(0.4) * (c(1.0) - (d / h)) / (c(1.25) * c(1.25))
        arg = (pi * z) / h
        sn, cs = np.sin(arg), np.cos(arg)
        inth = (c(2.0) * h * ((c(48) * np.arctan((np.sqrt(c(5.0)) * sn) / (cs + c(1)))) / (c(5.0) * np.sqrt(c(5.0))) +
                              (c(32.0) * sn) / ((cs + c(1)) * ((c(25.0) * (sn * sn)) / ((cs + c(1.0)) * (cs + c(1.0))) + c(5.0))))) / pi
        inth = np.where(z != h, inth, c(4.293251) * h)
        mu = uf / (a2 * h) * c(1.0) / (uf * uf)
        raw = inth * mu
    return raw, np.where(raw < c(0.001), c(0.001), raw)


def tvbelow(T, z, d, h, pai, uf, leafden, Flux, Fluxz, SH, SG, mxnear):
    """cpp:1381-1409: dict of the diffusivities (iKc = 1 / Kc, iKs = 1 / (Kg + Kh + Kc) for the device's fields), the near-field
    term before its clamp, and the result"""
    c = T
    zz, hh = z, h
    z, h, pai, leafden, Flux, Fluxz, SH, SG, mxnear = _a(T, z, h, pai, leafden, Flux, Fluxz, SH, SG, mxnear)
    with np.errstate(all="ignore"):
        Rc = rhcanopy(T, uf, hh, d, hh)[1]
        rz = rhcanopy(T, uf, hh, d, zz)[1]
        Kc = h / Rc
        Kg = c(1.0) / rz
        Kh = c(1.0) / (Rc - rz)
        Kg = Kg / z
        Kh = Kh / (h - z)
        SC = SH + Flux / Kc
        farg = (Kg * SG + Kh * SH + Kc * SC) / (Kg + Kh + Kc)
        SN = Fluxz * leafden
        near_raw = (c(3.047519) + c(0.128642) * np.log(pai)) * SN
        near = np.where(np.abs(near_raw) > mxnear, np.where(near_raw > 0, mxnear, -mxnear), near_raw)
        near = np.where(near != near, c(0), near)          # std::isnan
        return dict(Rc=Rc, rz=rz, Kg=Kg, Kh=Kh, Kc=Kc, iKc=c(1.0) / Kc, iKs=c(1.0) / (Kg + Kh + Kc), near_raw=near_raw, tvb=near + farg,
                    tvb_terms=np.abs(near) + np.abs(farg))


def tvabove(T, reqhgt, zref, d, zm, T0, tc, ea):
    """cpp:1298-1313 with surfwet = 1"""
    c = T
    reqhgt, zref, d, zm, T0, tc, ea = _a(T, reqhgt, zref, d, zm, T0, tc, ea)
    with np.errstate(all="ignore"):
        zh = c(0.2) * zm
        estl = satvap(T, T0)
        lnr = np.log((reqhgt - d) / zh) / np.log((zref - d) / zh)
        up = reqhgt > (d + zh)
        Tz = np.where(up, tc + (T0 - tc) * (c(1) - lnr), T0)
        ez = np.where(up, ea + (estl - ea) * c(1.0) * (c(1) - lnr), ea + (estl - ea) * c(1.0))
    return dict(Tz=Tz, ez=ez, margin=reqhgt - (d + zh), Tz_up=tc + (T0 - tc) * (c(1) - lnr))


def solar(T, slope, aspect, zend, azid):
    """cpp:85-102 for both shadowmask values, and the site's sines and cosines"""
    c = T
    slope, aspect, zend, azid = _a(T, slope, aspect, zend, azid)
    tr = c(TORAD)
    with np.errstate(all="ignore"):
        o = dict(cS=np.cos(slope * tr), sS=np.sin(slope * tr), cA=np.cos(aspect * tr), sA=np.sin(aspect * tr))
        tilted = np.cos(zend * tr) * np.cos(slope * tr) + np.sin(zend * tr) * np.sin(slope * tr) * np.cos((azid - aspect) * tr)
        si = np.where(slope == 0, np.cos(zend * tr), tilted)
        o["si_raw"] = si
        o["si1"] = np.where(si < 0, c(0), si)
        o["si0"] = np.where(zend > c(90.0), c(0), o["si1"])
    return o


def step_weather(T, tc, rh, pk, tci, mxtc):
    """cpp:4226-4228 and PenmanMonteithCpp's step-only terms (cpp:498-511, 280-291, 3728-3729, 3785) as MetT holds them; then
    PenmanMonteith2Cpp's (cpp:1220-1247) and cpp:4745-4747 as MicroMet holds them"""
    c = T
    tc, rh, pk, tci, mxtc = _a(T, tc, rh, pk, tci, mxtc)
    o = {}
    with np.errstate(all="ignore"):
        es = satvap(T, tc)
        ea = es * rh / c(100.0)
        te = (tci + tc) / c(2.0)
        o.update(ea=ea, te=te, rem=c(0.97) * c(SB) * radem(T, tc), rcan=c(0.97) * c(SB) * radem(T, tci))
        o["la"] = latent_ge0(T, te)
        o["cp"] = c(2e-05) * (te * te) + c(0.0002) * te + c(29.119)
        o["Da"] = es - ea
        o["gR"] = (c(4.0) * c(0.97) * c(SB) * (te + c(273.15)) ** 3) / o["cp"]
        o["De"] = satvap(T, te + c(0.5)) - satvap(T, te - c(0.5))
        o["tdew"] = dewpoint(T, ea)
        o["ph"] = c(44.6) * (pk / c(101.3)) * (c(273.15) / (tc + c(273.15)))
        rhos = c(67.92) + c(51.25) * np.exp(tc / c(2.59))
        o["sint"] = c(6.2) * (c(0.26) + c(46) / rhos)
        o.update(m_es=es, m_ea=ea, m_tdew=o["tdew"])
        o["m_De"] = satvap(T, tc + c(0.5)) - satvap(T, tc - c(0.5))
        o["m_gHrad"] = (c(4) * c(0.97) * c(SB) * (tc + c(273.15)) ** 3) / c(29.3)
        o["m_Rem"] = o["rem"]
        o["m_la_pm"] = latent_ge0(T, tc)
        o["m_lat0"] = latent_lt0(T, tc)
        o["m_dTmx"] = c(-0.6273) * mxtc + c(49.79)
        o["m_ipk"] = c(1.0) / pk
    return o


# plane order of mcf_selftest_snow (include/mcf.h)
KIND0_FIELDS = ("gexp", "glog", "gsqrt", "gpow0", "svp", "dewpoint", "rad4", "latent_lt0", "clamp01", "snow_albedo", "satvap_r", "lapserate_r")
KIND1_FIELDS = ("om", "a", "gma", "del", "h", "S1", "iS1", "iD1", "iD2", "u1", "u2", "D1", "D2", "p1", "p2", "p3", "p4", "sig", "isig", "S2",
                "p5", "p6", "p7", "p8", "p9", "p10", "k", "kd", "Kc")
KIND1_INPUTS = ("pait", "lref", "ltra", "gref", "kd", "kx", "kcos", "si")
KIND2_INPUTS = ("h", "pai", "d", "uf", "prec", "sint", "Li", "sdp0", "sdp1", "sdp2", "sdp3", "depth", "age", "x", "z", "leafden", "Flux",
                "Fluxz", "SH", "SG", "mxnear", "zm", "zref", "za", "T0", "tc", "ea", "slope", "aspect", "zend", "azid", "hc")
KIND2_FIELDS = ("d0", "zm0", "cis", "sden", "sn", "cs", "rz", "Rc", "Kg", "Kh", "Kc", "iKc", "iKs", "tvb", "Tz", "ez", "cS", "sS", "cA", "sA",
                "flat", "si0", "si1")
KIND3_INPUTS = ("tc", "rh", "pk", "tci", "mxtc")
KIND3_FIELDS = ("ea", "te", "rem", "rcan", "la", "cp", "Da", "gR", "De", "tdew", "ph", "sint", "m_es", "m_ea", "m_tdew", "m_De", "m_gHrad",
                "m_Rem", "m_la_pm", "m_lat0", "m_dTmx", "m_ipk")
NIN = {0: 2, 1: 8, 2: 32, 3: 5}
NOUT = {0: 12, 1: 29, 2: 23, 3: 22}


def canopy(T, c):
    """kind 2's outputs from its input planes (dict of fp64 arrays keyed by KIND2_INPUTS), with the branch operands"""
    o = {}
    o["d0"] = zeroplane(T, c["h"], c["pai"])
    o["zm_raw"], o["zm_cap"], o["zm0"] = roughlength(T, c["h"], c["pai"], c["d"])
    o.update(canopysnowint(T, c["hc"], c["pai"], c["uf"], c["prec"], c["sint"], c["Li"]))
    o["sden"] = snow_density(T, [c["sdp0"], c["sdp1"], c["sdp2"], c["sdp3"]], c["depth"], c["age"])
    x, = _a(T, c["x"])
    with np.errstate(all="ignore"):
        o["sn"], o["cs"] = np.sin(x), np.cos(x)
    o["rz_raw"], o["rz"] = rhcanopy(T, c["uf"], c["h"], c["d"], c["z"])
    tb = tvbelow(T, c["z"], c["d"], c["h"], c["pai"], c["uf"], c["leafden"], c["Flux"], c["Fluxz"], c["SH"], c["SG"], c["mxnear"])
    o.update({k: tb[k] for k in ("Rc", "Kg", "Kh", "Kc", "iKc", "iKs", "near_raw", "tvb", "tvb_terms")})
    ta = tvabove(T, c["za"], c["zref"], c["d"], c["zm"], c["T0"], c["tc"], c["ea"])
    o.update(Tz=ta["Tz"], ez=ta["ez"], above_margin=ta["margin"], Tz_up=ta["Tz_up"])
    o.update(solar(T, c["slope"], c["aspect"], c["zend"], c["azid"]))
    o["flat"] = (np.asarray(c["slope"], dtype=F64) == 0).astype(F64)
    return o
