"""Case sets and checks shared by tests/test_step_gpu.py (the device entry mcf_selftest_step) and tests/test_step_ref_cpu.py
(the yardstick itself): the per-cell-step sun position and humidity helpers of array forcing against tests/step_ref.py.

The sets (all site-steps: year, month, day, hour, winddir, lat, lon, tc, pk, rsw, rdif):
  random      20 000 site-steps: lat in [-89.9, 89.9], a quarter in [-24, 24]; lon in [-180, 180]; 2019-2024 with both Feb 29;
              integer and fractional hours.
  sector      48 site-days; the hour bisected ON THE LONGDOUBLE YARDSTICK to each horizon-sector boundary 7.5 + 15 k that the sun
              crosses after 8 h at 8 degrees of azimuth an hour or more, then stepped off by +-2^20 ulp of the hour (1.9e-9 h:
              1.5e-8 degrees or more).
  sector_ulp  the same boundaries at 0 and +-1 ulp: here only "one of the two sectors that meet there" is asserted.
  horizon     the hour bisected to coh = 0 at sunrise and sunset, stepped off by +-2^20 ulp; polar day and night at |lat| 80-89.9.
  zenith      lat = declination + acos(coh) at local solar noon for coh from 0.9990 up, with 24 values inside the band
              (cos(pi/2 pi/180), 0.99962422] in which derive_time_af's `nearzen` constant 0.99962422 set the ksat bit against the
              literal route, values 1e-11 and 1e-9 off the band's ends and off today's constant, 1 - coh from 1e-4 down to 1e-10
              at generic azimuths, and 1 - coh = 1e-13 and 0; each on twelve dates.
  special     lat = +-90, 0, 45; lon = 0, +-180; the equinoxes, Feb 29, the year's ends; hours 0 .. 23.999; wind directions on
              the half-sector values.
  weather     tc in [-60, 60] with +-0.5, 0.0, -0.0 and NaN; pk in [50, 110]; rsw < rdif; rsw = rdif = 0.  (The 1352 clamp on a
              tiny positive coh is met in the horizon set.)
  humidity    (tc, rh, pk): tc in [-60, 60], rh in [0, 100] with exact 0, pk in [30, 110]; ea straddling 0.6112.

Integers (sindex, windex, ksat, up, julday) must equal the longdouble yardstick except on FRAGILE cases: those whose distance
to the deciding threshold (azimuth to a sector boundary, in degrees; coh to 0; coh to cos(pi/2 pi/180); the dew point over
water to 0) is below 64 E, E being the largest error of the fp64 yardstick against the longdouble one for that quantity
over that set — taken from the two yardsticks at test time, never from the device.  A fragile sector must still be one of the
two that meet at the nearest boundary.  At most 1 % of a set may be fragile.  The sector is asserted where the yardstick's
1 - coh^2 is at least 1e-12 (closer to the zenith the azimuth is not defined to any useful accuracy), and E of the azimuth is
taken over those cases.

The day's part and the stepped-off sets.  The reference takes the declination from cos(2 pi (jd - 159.5) / 365.25), an argument
of 4e4 radians: its fp64 rounding alone moves the declination by 2e-12, so E of coh is 2.5e-12 and E of the azimuth 2e-9
degrees — 64 E is more than the 2^20 ulp by which the sector and horizon sets are stepped off.  Both device routes take the
day's part (equation of time, declination) from the same sol_date, and it is the site algebra behind it that these sets are
aimed at: they are therefore ALSO judged against the exact (longdouble) site algebra on the fp64 values of the day's part
(step_ref.solposition(date_T = np.float64)).  There E of the azimuth is 7e-11 degrees (the 1 - sazi^2 cancellation next to
azimuth 90 / 270, in the reference's formula too), the yardstick flags none of their cases, and every integer must be equal.
For the same reason the floating fields are held to 16 E twice: against the truth from the calendar inputs, and against the
truth on the fp64 day's part, whose E is the site algebra's own (1e-15 instead of 2e-12 for CZ).

Floating fields: the error against the longdouble yardstick may be at most 16 x the fp64 yardstick's own error, per field and
per conditioning class of s2 = 1 - coh^2 (>= 1e-2, [1e-6, 1e-2), [1e-12, 1e-6), and >= 0.5 on its own), pooled over all sets;
SAZ / CAZ have the extra class "azimuth within 1 degree of 90 / 270", where 1 - sazi^2 cancels in the reference's own formula
too.  The error is relative to the true value, except for the fields bounded by 1 that cross zero (CZ, SZ, SAZ, CAZ, ...),
where it is absolute.  16 allows for the algebra's extra roundings (the angle addition for the hour angle, two square roots,
the lean quotients) and the device's FMA contraction.  It does NOT reach a 46-bit square root (2^-46 = 1.4e-14 against
16 E = 1.2e-14 for SZ where it is best conditioned: the hour angle, up to 2 pi, rounds to 9e-16): that is what the identities
CZ^2 + SZ^2 = 1 and SAZ^2 + CAZ^2 = 1 are asserted for, to 5 x 2^-52.

Measured on the CPU (tests/test_step_ref_cpu.py asserts the shares):
  set          cases   E azimuth, deg   E coh      fragile: sector, horizon, zenith threshold
  random       20000   5.2e-09          2.5e-12    0, 0, 0
  sector        1332   1.6e-09          1.6e-12    1100, 0, 0     on the fp64 day's part: 7.0e-11, 5.5e-16; 0, 0, 0
  sector_ulp    2664   1.6e-09          1.6e-12    2664, 0, 0     (they sit on the boundaries; not counted against the 1 %)
  horizon        280   9.4e-11          1.5e-12    0, 12, 0       on the fp64 day's part: 3.8e-13, 8.5e-16; 0, 0, 0
  zenith        1056   4.5e-04          8.4e-14    0, 0, 0        (336 cases in the band, 24 with 1 - coh^2 < 1e-12)
  special        420   3.0e-09          2.3e-12    0, 0, 0
  weather        720   9.6e-10          2.2e-12    0, 0, 0
  humidity      9480   E of the dew point 6.7e-14 K; 34 fragile (0.36 %)
  longdouble against mpmath at 50 digits (3642 cases of all sets): at most 8.0e-4 of E in any field and class
  fp64 yardstick against the oracle's solpositionCpp (random set): 1764 zeniths and 22 azimuths of 20000 differ, by at most
  4 and 66 ulp; the azimuth by 0 ulp where neither cancellation amplifies, and by at most 0.44 of its scaled bar elsewhere
Measured on one MI355X (every integer equal off the fragile cases, on all three routes):
  largest error / E over all fields and classes: kind 0 (derive_time_af) 6.4 (COSA and SINA on the fp64 day's part; 3.3 for the
  fields that follow coh through the horizon, 3.0 for SZ), kind 1 (derive_time) 3.3, kind 2 (sun_at_cell) 5.0 (ca, 1e-6 <= s2 < 1e-2)
  |CZ^2 + SZ^2 - 1| <= 4.4e-16, |SAZ^2 + CAZ^2 - 1| <= 1.6e-16 (kinds 0 and 2)
  humidity: es 1.6e-15 relative (1.23 E), lapse rate 6.3e-16 (1.08 E), dew point 6.3e-14 K (0.95 E)
  with `nearzen` at 0.99962422 (NEARZEN_BEFORE) all 336 band cases come out with ksat = 1 against the yardstick's and the
  literal route's 0
These figures are kept here and nowhere else (DESIGN.md section 24 has the method and points here).
At the zenith itself (1 - coh = 0 of the set) fp64 rounding carries coh past 1 on one date of twelve; acos of that is NaN in
the reference, in the fp64 yardstick and on both device routes (ZEND, and what pass 2 makes of it): the device follows the
reference there, and the tests accept a NaN zenith angle as "above the horizon" only where 1 - coh^2 < 1e-12."""
import datetime
import functools

import numpy as np

import step_ref as R

LD = np.longdouble
FRAGILE_FACTOR = 64.0
BAR_FACTOR = 16.0
MAX_FRAGILE = 0.01
S2_MIN = 1e-12                 # below it only finiteness and the up / ksat bits are asserted
STEP_OFF = 2.0 ** 20           # ulps of the hour
INPUTS = ("year", "month", "day", "hour", "winddir", "lat", "lon", "tc", "pk", "rsw", "rdif")
NEARZEN_TODAY = 0.99962421     # derive_time_af / its callers: `coh > NEARZEN` takes the acos route
NEARZEN_BEFORE = 0.99962422    # ... and the constant it replaced


def zenith_threshold():
    """coh at which the zenith angle in DEGREES equals pi/2 (the degrees call, cpp:1425): cos(pi/2 pi/180), in longdouble"""
    pi = LD(R.PI)
    return np.cos((pi / LD(2.0)) / (LD(180) / pi))


def _weather(rng, n):
    rsw = rng.uniform(0.0, 1000.0, n)
    return dict(winddir=rng.uniform(0.0, 360.0, n), tc=rng.uniform(-30.0, 40.0, n), pk=rng.uniform(80.0, 105.0, n), rsw=rsw,
                rdif=rsw * rng.uniform(0.1, 1.0, n))


def _pack(year, month, day, hour, lat, lon, rng, **over):
    n = len(hour)
    d = dict(year=np.asarray(year, dtype=np.float64), month=np.asarray(month, dtype=np.float64), day=np.asarray(day, dtype=np.float64),
             hour=np.asarray(hour, dtype=np.float64), lat=np.asarray(lat, dtype=np.float64), lon=np.asarray(lon, dtype=np.float64))
    d.update(_weather(rng, n))
    d.update({k: np.asarray(v, dtype=np.float64) for k, v in over.items()})
    assert all(len(d[k]) == n for k in INPUTS)
    return {k: d[k] for k in INPUTS}


def _dates(ordinals):
    ds = [datetime.date.fromordinal(int(o)) for o in ordinals]
    return np.array([d.year for d in ds]), np.array([d.month for d in ds]), np.array([d.day for d in ds])


def _random():
    rng = np.random.default_rng(20240229)
    n = 20000
    o0, o1 = datetime.date(2019, 1, 1).toordinal(), datetime.date(2024, 12, 31).toordinal()
    ords = rng.integers(o0, o1 + 1, n)
    ords[:2] = [datetime.date(2020, 2, 29).toordinal(), datetime.date(2024, 2, 29).toordinal()]
    y, m, d = _dates(ords)
    lat = rng.uniform(-89.9, 89.9, n)
    lat[::4] = rng.uniform(-24.0, 24.0, len(lat[::4]))
    hour = np.where(rng.random(n) < 0.5, rng.integers(0, 24, n).astype(np.float64), rng.uniform(0.0, 24.0, n))
    return _pack(y, m, d, hour, lat, rng.uniform(-180.0, 180.0, n), rng)


# ---- bisection on the longdouble yardstick -------------------------------------------------------------------------------------
def _site_days():
    rng = np.random.default_rng(7)
    lats = np.array([-75.0, -60.5, -45.25, -33.0, -20.0, -10.5, -2.0, 0.0, 3.0, 12.75, 23.0, 35.5, 48.0, 55.25, 66.0, 72.5])
    lat = np.repeat(lats, 3)
    o0, o1 = datetime.date(2019, 1, 1).toordinal(), datetime.date(2024, 12, 31).toordinal()
    y, m, d = _dates(rng.integers(o0, o1 + 1, len(lat)))
    return dict(year=y, month=m, day=d, lat=lat, lon=rng.uniform(-180.0, 180.0, len(lat)))


def _sector_of(az):
    return np.floor((az - LD(7.5)) / LD(15)).astype(np.int64)


def _bisect(sd, which, key):
    """Brackets [lo, hi] of adjacent doubles of the hour around every place where `key` (an integer function of the longdouble
    solar position) changes between 4 h and 23.9 h (2^20 ulp of an hour below 4 are less than 1e-9 h), for the site-days sd[which]."""
    grid = np.linspace(4.0, 23.9, 1991)
    ns = len(which)

    def state(idx, hour):
        sp = R.solposition(LD, sd["year"][idx], sd["month"][idx], sd["day"][idx], hour, sd["lat"][idx], sd["lon"][idx])
        return key(sp), sp["azid"]

    idx = np.repeat(which, len(grid))
    st, az = state(idx, np.tile(grid, ns))
    st, az = st.reshape(ns, -1), az.reshape(ns, -1)
    hit = (st[:, 1:] != st[:, :-1]) & (np.abs(az[:, 1:] - az[:, :-1]) < 5)       # (not the 360 -> 0 wrap, not a pass through the zenith)
    i, j = np.nonzero(hit)
    site, lo, hi, s_lo, s_hi = which[i], grid[j].copy(), grid[j + 1].copy(), st[i, j], st[i, j + 1]
    rate = np.asarray(np.abs(az[i, j + 1] - az[i, j]), dtype=np.float64) / (grid[1] - grid[0])        # degrees of azimuth per hour
    for _ in range(64):
        mid = lo + (hi - lo) / 2
        open_ = (mid > lo) & (mid < hi)
        if not open_.any():
            break
        s_mid, _ = state(site, mid)
        left = open_ & (s_mid == s_lo)
        right = open_ & ~left
        lo, hi = np.where(left, mid, lo), np.where(right, mid, hi)
    assert (np.nextafter(lo, hi) == hi).all()
    return site, lo, hi, s_lo, s_hi, rate


def _at(sd, site, hour, rng):
    return _pack(sd["year"][site], sd["month"][site], sd["day"][site], hour, sd["lat"][site], sd["lon"][site], rng)


@functools.lru_cache(maxsize=None)
def _boundaries():
    sd = _site_days()
    which = np.arange(len(sd["lat"]))
    sec = _bisect(sd, which, lambda sp: _sector_of(sp["azid"]))
    # 2^20 ulp of the hour are 1.9e-9 h from 8 h on: where the azimuth moves by 8 degrees an hour or more that is 1.5e-8 degrees
    fast = (sec[1] >= 8.0) & (sec[5] >= 8.0)
    sec = tuple(a[fast] for a in sec[:5])
    hor = _bisect(sd, which, lambda sp: (sp["coh"] >= 0).astype(np.int64))[:5]
    return sd, sec, hor


def _sector(stepped):
    sd, (site, lo, hi, _, _), _ = _boundaries()
    rng = np.random.default_rng(11)
    if stepped:
        hour = np.concatenate([lo - STEP_OFF * np.spacing(lo), hi + STEP_OFF * np.spacing(hi)])
        return _at(sd, np.concatenate([site, site]), hour, rng)
    hour = np.concatenate([lo, hi, np.nextafter(lo, 0.0), np.nextafter(hi, 100.0)])
    return _at(sd, np.concatenate([site] * 4), hour, rng)


def _horizon():
    sd, _, (site, lo, hi, _, _) = _boundaries()
    rng = np.random.default_rng(12)
    hour = np.concatenate([lo - STEP_OFF * np.spacing(lo), hi + STEP_OFF * np.spacing(hi)])
    c = _at(sd, np.concatenate([site, site]), hour, rng)
    # polar day and night
    lat = np.array([80.0, 84.5, 88.0, 89.9, -80.0, -84.5, -88.0, -89.9])
    hours = np.arange(0.0, 24.0, 3.0)
    L, D, H = np.meshgrid(lat, np.arange(2), hours, indexing="ij")
    L, D, H = L.ravel(), D.ravel(), H.ravel()
    p = _pack(np.where(D == 0, 2021, 2022), np.where(D == 0, 6, 12), np.full(len(L), 21), H, L, rng.uniform(-180, 180, len(L)), rng)
    return {k: np.concatenate([c[k], p[k]]) for k in INPUTS}


def _zenith():
    rng = np.random.default_rng(13)
    c0 = float(zenith_threshold())
    band = np.linspace(c0, NEARZEN_BEFORE, 26)[1:-1]                                    # 24 strictly inside
    ends = np.concatenate([c0 + np.array([-1e-9, -1e-11, 1e-11, 1e-9]), NEARZEN_BEFORE + np.array([-1e-9, -1e-11, 1e-11, 1e-9]),
                           NEARZEN_TODAY + np.array([-1e-9, -1e-11, 1e-11, 1e-9])])
    coh = np.concatenate([np.linspace(0.9990, 0.9999, 37), band, ends, 1.0 - 10.0 ** -np.arange(4.0, 10.5, 0.5), [1.0 - 1e-13, 1.0]])
    months = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
    C, M = np.meshgrid(coh, months, indexing="ij")
    C, M = C.ravel(), M.ravel()
    n = len(C)
    year, day, lon = np.full(n, 2023), 5 + (np.arange(n) % 20), np.where(np.arange(n) % 3 == 0, 0.0, rng.uniform(-30, 30, n))
    sp = R.solposition(LD, year, M, day, np.full(n, 12.0), np.zeros(n), lon)
    delta = np.arccos(C.astype(LD))                                                        # zenith angle wanted, radians
    # the band and its ends at local solar noon exactly (coh = cos(lat - dec)); the approach to the zenith at generic azimuths
    phi = np.where(C > 0.99995, rng.uniform(0, 2 * np.pi, n), 0.0).astype(LD)
    lat = ((sp["dec"] + delta * np.cos(phi)) * LD(180) / LD(R.PI)).astype(np.float64)
    tt = delta * np.sin(phi) / np.cos(sp["dec"])
    hour = (LD(12) + tt / LD(0.261799) - (LD(4.0) * lon.astype(LD) + sp["eot"]) / LD(60)).astype(np.float64)
    return _pack(year, M, day, hour, lat, lon, rng)


def _special():
    rng = np.random.default_rng(14)
    dates = [(2021, 3, 20), (2021, 9, 22), (2020, 2, 29), (2019, 12, 31), (2024, 1, 1)]
    lat, lon, di, hour = np.meshgrid([90.0, -90.0, 0.0, 45.0], [0.0, 180.0, -180.0], np.arange(len(dates)),
                                     [0.0, 0.5, 6.0, 12.0, 18.0, 23.0, 23.999], indexing="ij")
    lat, lon, di, hour = lat.ravel(), lon.ravel(), di.ravel(), hour.ravel()
    dates = np.array(dates)
    wd = np.resize(np.array([0.0, 22.5, 67.5, 337.5, 360.0, 359.999, 22.499999, 180.0]), len(lat))
    return _pack(dates[di, 0], dates[di, 1], dates[di, 2], hour, lat, lon, rng, winddir=wd)


def _weather_set():
    rng = np.random.default_rng(15)
    n = 720
    o0 = datetime.date(2022, 1, 1).toordinal()
    y, m, d = _dates(o0 + rng.integers(0, 365, n))
    tc = np.concatenate([np.linspace(-60.0, 60.0, n - 8), [0.5, -0.5, 0.0, -0.0, np.nan, 1e-300, -1e-300, 59.999]])
    c = _pack(y, m, d, rng.uniform(0, 24, n), rng.uniform(-70, 70, n), rng.uniform(-180, 180, n), rng, tc=tc,
              pk=rng.uniform(50.0, 110.0, n))
    c["rdif"][::5] = c["rsw"][::5] * 1.25           # rsw < rdif
    c["rsw"][1::5] = 0.0
    c["rdif"][1::5] = 0.0
    return c


SETS = {"random": _random, "sector": lambda: _sector(True), "sector_ulp": lambda: _sector(False), "horizon": _horizon,
        "zenith": _zenith, "special": _special, "weather": _weather_set}
STEPPED = ("sector", "horizon")     # built so that the yardstick flags no case


@functools.lru_cache(maxsize=None)
def case(name):
    c = SETS[name]()
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def pooled():
    """every step set back to back: (inputs, {name: slice})"""
    parts, where, at = [case(n) for n in SETS], {}, 0
    for n, p in zip(SETS, parts):
        where[n] = slice(at, at + len(p["hour"]))
        at += len(p["hour"])
    inp = {k: np.concatenate([p[k] for p in parts]) for k in INPUTS}
    for a in inp.values():
        a.setflags(write=False)
    return inp, where


@functools.lru_cache(maxsize=None)
def yardsticks(date_row=False):
    """(truth, literal): step_ref.step_fields of the pooled sets in longdouble and in fp64, computed once.  date_row: the truth is
    the exact site algebra on the fp64 values of the day's part (equation of time, declination)."""
    inp, _ = pooled()
    if date_row:
        return R.step_fields(LD, inp, np.float64), yardsticks()[1]
    return R.step_fields(LD, inp), R.step_fields(np.float64, inp)


@functools.lru_cache(maxsize=None)
def humidity_case():
    rng = np.random.default_rng(16)
    tc = np.concatenate([np.linspace(-60.0, 60.0, 4500), rng.uniform(-60, 60, 4500), [0.0, -0.0, 1e-300, -1e-300]])
    n = len(tc)
    rh = rng.uniform(0.01, 100.0, n)
    rh[::7] = 100.0
    rh[3::50] = 0.0
    pk = rng.uniform(30.0, 110.0, n)
    # ea straddling 0.6112 (the dew point over water crossing 0): tc above 0, rh = 100 * 0.6112 / es (1 + d)
    t2 = rng.uniform(0.05, 40.0, 476)
    es = R.humidity(np.float64, t2, np.full(len(t2), 100.0), np.full(len(t2), 100.0))["es"]
    dl = np.resize(np.array([-1e-3, 1e-3, -1e-6, 1e-6, -1e-9, 1e-9, -1e-11, 1e-11, -1e-2, 1e-2, 0.0, -1e-1, 1e-1, 3e-4]), len(t2))
    c = dict(tc=np.concatenate([tc, t2]), rh=np.concatenate([rh, 100.0 * 0.6112 / es * (1.0 + dl)]),
             pk=np.concatenate([pk, rng.uniform(30.0, 110.0, len(t2))]))
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def humidity_yardsticks():
    c = humidity_case()
    return R.humidity(LD, c["tc"], c["rh"], c["pk"]), R.humidity(np.float64, c["tc"], c["rh"], c["pk"])


# ---- fragile cases ---------------------------------------------------------------------------------------------------------------
def _maxabs(a):
    a = np.abs(a[np.isfinite(a)])
    return float(a.max()) if a.size else 0.0


@functools.lru_cache(maxsize=None)
def margins(name, date_row=False):
    """Of one set: the yardstick's integers (sindex, up, ksat), boolean arrays `sector`, `up_f`, `ksat_f` (True: fragile),
    `assert_sector` (1 - coh^2 >= S2_MIN), `pair` (the two sectors that meet at the nearest boundary) and the E values they were
    made with.  date_row: the truth is the exact site algebra on the fp64 values of the day's part (see the module docstring)."""
    _, where = pooled()
    truth, lit = yardsticks(date_row)
    s = where[name]
    t, l = truth["sp"], lit["sp"]
    ok = np.asarray(t["s2"][s] >= LD(S2_MIN))
    az, coh, zend = t["azid"][s], t["coh"][s], t["zend"][s]
    e_az = _maxabs((l["azid"][s].astype(LD) - az)[ok])
    r = np.mod(az - LD(7.5), LD(15))
    d_sector = np.minimum(r, LD(15) - r)
    kb = np.rint(np.asarray((az - LD(7.5)) / LD(15), dtype=np.float64)).astype(np.int64)
    e_coh = _maxabs(l["coh"][s].astype(LD) - coh)
    return dict(sindex=R.dir_index(az, 15.0, 24), up=np.asarray(zend <= LD(90.0)), ksat=np.asarray(zend > LD(R.PI) / LD(2.0)),
                sector=np.asarray(d_sector < FRAGILE_FACTOR * e_az), up_f=np.asarray(np.abs(coh) < FRAGILE_FACTOR * e_coh),
                ksat_f=np.asarray(np.abs(coh - zenith_threshold()) < FRAGILE_FACTOR * e_coh), assert_sector=ok,
                pair=np.stack([np.mod(kb, 24), np.mod(kb + 1, 24)]), e_az=e_az, e_coh=e_coh)


@functools.lru_cache(maxsize=None)
def humidity_margin():
    t, l = humidity_yardsticks()
    pos = np.asarray(t["ea"] > 0)
    e = _maxabs((l["tdew_w"].astype(LD) - t["tdew_w"])[pos])
    return np.asarray(np.abs(t["tdew_w"]) < FRAGILE_FACTOR * e) & pos, e


# ---- floating fields -------------------------------------------------------------------------------------------------------------
ABSOLUTE = {"CZ", "SZ", "SAZ", "CAZ", "SINDEC", "COSDEC", "COSA", "SINA", "cosz", "cz", "sz", "sa", "ca"}     # bounded by 1
SOLAR = {"CZ", "SZ", "TANSA", "ZEND", "COSC", "TANC", "TAN2C", "INV2COSC", "SAZ", "CAZ", "RBEAM", "RB", "zend", "cosz", "cz", "sz",
         "tansa", "tansa_deg", "kx", "kcos", "sa", "ca"}
AZIMUTH = {"SAZ", "CAZ", "sa", "ca"}


@functools.lru_cache(maxsize=None)
def classes(date_row=False):
    """The conditioning classes of the pooled cases: {name: mask}; fragile horizon cases and the cases closer to the zenith than
    S2_MIN are in none."""
    _, where = pooled()
    truth, _ = yardsticks(date_row)
    s2 = truth["sp"]["s2"]
    keep = np.ones(len(s2), dtype=bool)
    for n in SETS:
        keep[where[n]] &= ~margins(n, date_row)["up_f"]
    az = truth["sp"]["azid"]
    near90 = np.asarray((np.abs(az - 90) < 1) | (np.abs(az - 270) < 1))
    return {"s2>=0.5": keep & np.asarray(s2 >= LD(0.5)), "s2>=1e-2": keep & np.asarray(s2 >= LD(1e-2)), "1e-6<=s2<1e-2": keep & np.asarray((s2 >= LD(1e-6)) & (s2 < LD(1e-2))),
            "1e-12<=s2<1e-6": keep & np.asarray((s2 >= LD(S2_MIN)) & (s2 < LD(1e-6))), "az90": keep & near90 & np.asarray(s2 >= LD(S2_MIN)),
            "_near90": near90, "_keep": keep}


def field_error(x, truth, field):
    """|x - truth|, relative to |truth| unless the field is one of ABSOLUTE; NaN where the truth is not finite"""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(x).astype(LD) - truth)
        if field not in ABSOLUTE:
            d = np.where(d == 0, LD(0), d / np.abs(truth))
        return np.where(np.isfinite(truth), d, LD(np.nan))


def compare_fields(got, fields, rename=None, extra_mask=None, date_row=False):
    """Rows (field, class, cases, E, device error) for the pooled sets: `got[field]` against the longdouble yardstick beside the
    fp64 yardstick's own error on the same cases.  `rename`: {device field: yardstick field}; extra_mask: {field: mask}; date_row:
    see yardsticks."""
    truth, lit = yardsticks(date_row)
    cl = classes(date_row)
    rows = []
    for f in fields:
        y = (rename or {}).get(f, f)
        e_lit, e_got = field_error(lit[y], truth[y], y), field_error(got[f], truth[y], y)
        names = ["s2>=0.5", "s2>=1e-2", "1e-6<=s2<1e-2", "1e-12<=s2<1e-6"] if y in SOLAR else ["all"]
        for c in names + (["az90"] if y in AZIMUTH else []):
            m = cl["_keep"].copy() if c == "all" else cl[c].copy()
            if y in AZIMUTH and c != "az90":
                m &= ~cl["_near90"]
            if extra_mask and f in extra_mask:
                m &= extra_mask[f]
            m &= np.isfinite(np.asarray(truth[y], dtype=np.float64))
            if m.any():
                rows.append((f, c, int(m.sum()), float(np.max(e_lit[m])), float(np.max(np.nan_to_num(e_got[m], nan=np.inf)))))
    return rows


def format_rows(rows, title):
    out = [f"{title}: field, class, cases, E (fp64 yardstick), error, error / E"]
    for f, c, n, e, g in rows:
        out.append(f"  {f:9s} {c:15s} {n:6d}  {e:9.3e}  {g:9.3e}  {g / e if e > 0 else (0.0 if g == 0 else np.inf):7.2f}")
    return "\n".join(out)
