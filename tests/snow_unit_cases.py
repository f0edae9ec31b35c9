"""Case sets, classes and checks shared by tests/test_snow_unit_gpu.py (the device entry mcf_selftest_snow) and
tests/test_snow_unit_ref_cpu.py (the yardstick itself): the device physics of the snow kernels against tests/snow_ref.py.

The sets, per kind of mcf_selftest_snow (include/mcf.h lists the planes):
  kind 0  weather     4 000 (tc, pk): tc in [-60, 40] with +-0, +-0.5, +-1e-300; pk in [30, 110]      svp, rad4, latent_lt0, the two _r helpers
          positive    4 000 x log-uniform in [1e-6, 1e3]                                          glog, gsqrt, dewpoint (ea in [1e-3, 10])
          gsqrt_wide  2 000 x log-uniform in [1e-305, 1e305] (both sides of gsqrt's switch at 1e-300 / 1e300)
          exp         4 000 x in [-700, 700], a quarter in [-2, 2]
          pow         4 000 (clump, Kc): clump in [0, 1], next to 0 and next to 1; Kc in [1, 600] with exact 1 and 600
          albedo      hs = 0 .. 47, 48, 71, 72, the days around the 0.1 clamp (24 x 1013 .. 1015), 100 000, 2^31 - 1, 400 random
          special     32 operands: +-0, denormals, the neighbours of 1e-300 and 1e300, the largest double, negative, +-inf, NaN, the
                      arguments at which exp leaves the normal range both ways
          pow_special b in {0.25, 1, 0.999, 3, 4 (4^600 overflows), 0, -0, -0.5, -1, -3, NaN} x e in {2.5, +-0, -2.5, 1, 3, -3, 601, 2, -2, 600, 0.5, -0.5,
                      1e-3, NaN}: every branch gpow0 spells out
  kind 1  random      8 000: pait in [0.001, 20] and kd in [0.01, 600] log-uniform, om = lref + ltra in (0.002, 0.998), gref in [0.1, 0.95]
          kd_near_h   24 leaves x kd = h (1 +- 2^-k), k = 4 .. 50, and kd = h as fp64 gives it
          om_near_1   om = 1 - 10^-j, j = 1 .. 15, 1 - 2^-50, 1 - 2^-52 (never 1: a = h = 0 is 0 / 0 in the reference), 40 each
          symmetric   600 with lref = ltra (del = 0)
          deep        pait h from 30 to 700, then 705, 709, 710, 712, 745, 750, 800, 1500: classes only (below)
          gref_ends   800 with gref = 0.1 and 0.95 alternating
          cank        si in {-1, -1e-300, -0.0, 0, 1e-300, 1e-12, 1, NaN} x 12
  kind 2  random      8 000: h in [0.001, 40] and pai in [0.001, 20] log-uniform, d = zeroplane(h, pai), 0 < z < h, all 32 planes ordinary
          z_edges     16 canopies x z = h, h (1 - 2^-k), h 2^-k (k = 1 .. 52), z / h on and +-1 ulp of 1/4, 1/2, 3/4
          sincos      x on [0, pi] at 3 000 points, +-8 ulp around pi/4, pi/2, 3 pi/4, pi, 3.1416 and the next double, 3.15, 4, 7, 100,
                      negative, 1e9 - 1, 1e9, 1e9 + 1, 1e15, NaN, +-0, 5e-324
          zm_cap, zm_floor, cis_cap, uzm_floor, rha_floor, above_branch, near_cap: 40 brackets each, the clamp's input (pai, h, prec,
                      pai, uf, za, Fluxz) bisected ON THE LONGDOUBLE YARDSTICK to adjacent doubles, then both stepped off by 2^20 ulp
          floors      the 0.001 floors of hgt and pai in the interception model, slope = +-0, zend on and next to 90
  kind 3  random      6 000 (tc, rh, pk, tci, mxtc); branches: tc and te = (tci + tc) / 2 at +-0, +-0.5 and their neighbours

Bars.
  Floating fields: the error against the longdouble yardstick may be at most 16 x the fp64 yardstick's own error E, per field and
  conditioning class; E comes from the two yardsticks at test time, never from the device.  Relative to the truth, except what is
  bounded by 1 and crosses zero (sn, cs, the site's sines and cosines, del, u1, the solar index) and temperatures in degrees C,
  which are absolute.  Classes: 1 - om in (< 1e-8, [1e-8, 1e-3), >= 1e-3) for ts_dif's fields, crossed with |kd - h| / h by
  hundreds from 1e-14 to 1e-2 for ts_dir's; pait h < 30 (deeper: classes of value only); kd pait < 700 for what S2 enters;
  1 - z / h and z / h in (< 1e-12, [1e-12, 1e-6), [1e-6, 1e-2), >= 1e-2) for the profile; |ln x|, |x|, |e ln b| for the guards;
  pai for zeroplane and roughlen0; kc pai, k2 prec and 1 - Li / Lstr (the interception model's three differences) for cis; (Rc - rz) / Rc
  for Kh, 1 / (Kg + Kh + Kc) and tv_below, which also has the cancellation of its near- and far-field terms; 100 - rh for Da.
  Clamps: the device returns the clamp's own value to the bit exactly where the yardstick clamps, unless the case is fragile
  (closer than 64 E to its threshold); at most 1 % of a set may be fragile (tests/test_snow_unit_ref_cpu.py asserts it).
  Special operands: the class of numpy's / C's result (NaN, +-inf, +-0, sign), no tolerance.

E of the fp64 yardstick (CPU; relative unless said), the figures the bars are made of:
  kind 0: svp, satvap_r 1.3e-15; rad4 5.6e-16; latent_lt0 1.4e-16; lapserate_r 5.3e-16; glog 5e-17 .. 1.1e-16; gexp, gsqrt, gpow0
          1.1 .. 1.2e-16 (one library call each); dewpoint 1.5e-14 K; albedo (hs >= 24) 9.7e-16
  kind 1, by 1 - om (>= 1e-3 | [1e-8, 1e-3) | < 1e-8): a 5.6e-14 | 5.6e-9 | 1; h 2.8e-14 | 2.8e-9 | 1 (in fp64 a = 1 - om is 0 or one
          ulp of 1 there: the reference's own h, D's and p's carry no digit); S1 5.6e-15 | 5.0e-12 | 3.2e-8; D1, D2, p1, p3 2.4 .. 3.6e-14
          | 2.8e-9 | 0.13 .. 1; p2 1.3e-13; p4 7.5e-12 ((u2 - h) cancels); om, gma, u1, u2, del: 5e-17 .. 2.4e-15 in every class
          by |kd - h| / h at 1 - om >= 1e-3 (>= 1e-2 | [1e-4, 1e-2) | [1e-6, 1e-4) | [1e-8, 1e-6) | [1e-10, 1e-8) | [1e-12, 1e-10) |
          [1e-14, 1e-12) | < 1e-14): sig, isig, p6, p9 5e-14 .. 4e-11 | 3.5e-12 | 6.3e-10 | 2.1e-8 | 6.4e-6 | 2.5e-4 | 0.08 | 1.5 .. 9;
          p10 5e-11 | 2.4e-9 | 2.5e-7 | 1.9e-5 | 2.3e-3 | 0.17 | 27 | 3e3; p5, p8 (no quotient by sig) 7e-16 .. 3.5e-15 throughout
          next to kd = h, 1e-12 and 8e-14 elsewhere; S2 4e-16, 5.6e-14 at kd pait up to 700; cank1's kd, Kc 1.1e-16
  kind 2: d0 by pai (< 0.003 | [0.003, 0.01) | [0.01, 0.03) | [0.03, 0.1) | [0.1, 0.3) | [0.3, 1) | >= 1): 1.5e-14 | 6.3e-15 | 2.1e-15 | 8.3e-16 |
          4.5e-16 | 3.0e-16 | 2.3e-16 (1 - exp(-s) and 1 - (..) / s at s = sqrt(7.5 pai)); zm0 3.1e-16 .. 1.4e-15 in the same classes; cis in 41
          classes of kc pai x k2 prec x (1 - Li / Lstr), from 3.7e-16 (kc pai >= 1, k2 prec >= 1) over 1.5 .. 7.5e-15 in the middle to 1e-13 at
          kc pai < 0.01 and 2.4e-12 at k2 prec < 1e-4; sden 2.9e-16; sn, cs 5.6e-17 absolute; Rc, Kc, iKc 1.0e-15; rz, Kg 1e-15 away from the
          top, 7.1e-13 at 1 - z / h in [1e-6, 1e-2), 3.5e-10 in [1e-12, 1e-6); Kh, iKs 5.7e-16 where (Rc - rz) / Rc >= 0.1, 1.9e-13 at 1 - z / h
          in [1e-2, 1e-1), 1.8e-6 and 3.0e-3 nearer the top; tvb 2.1e-16 .. 2.8e-15, 2.2e-13 where Rc and rz both sit at their floor; Tz
          2.5e-14 K, ez 7.1e-14; the site's sines and cosines 1.1 .. 4.5e-16; the solar index 6.9e-16
  kind 3: ea, es 1.5e-15; te 7.1e-15 K; rem, rcan, gR 6e-16; la 1.4e-16; cp 6e-17; Da by 100 - rh (>= 10 | [1, 10) | [0.1, 1) | < 0.1) 1.5e-15 | 1.0e-14 | 8.1e-14 | 5.4e-13; De 1.4 .. 1.6e-14; tdew 2.5e-14 K; ph
          3.7e-16; sint 2.9e-16; gHrad 5.5e-16; dTmx 1.6e-16; ipk 1.1e-16
  clamp sets (E of the operand relative to its threshold; fragile cases): zm_cap 9.1e-17, 0; zm_floor 8.0e-16, 0; cis_cap 2.1e-16, 0; uzm_floor 2.8e-16, 0;
          rha_floor 7.4e-16, 0; above_branch 8.7e-17 (of za), 0; near_cap 2.2e-16, 0; albedo at 0.95 1.1e-16, 0; at 0.1 1.1e-15, 0.
          2^20 ulp is 2.3e-10 relative: every bracket is 2e5 E or more from its threshold.
  longdouble against mpmath at 50 digits (a sample of every set: 948, 849, 991 and 320 cases of kinds 0 .. 3): at most 1/105 of
          the class's E (the bar is 1/64) (rh_canopy next to z = h, where the dyadic fp64 operands round less than longdouble's), 1e-3 or less elsewhere
  fp64 yardstick against the oracle (tests/test_snow_unit_ref_cpu.py, 2 000 cases of the random sets, in ulp): satvap 2, the albedo,
          cank, om .. u1, sig, p5, p8, rhcanopy, TVbelow, TVabove's Tz 0; S1 1; D1, D2, roughlength 2; p1 .. p4 4; p6 9; p7 12; p10 4;
          p9 116 and zeroplanedis 159 (0.31 of the bar with its amplification); canopysnowint 3 472 at pai = 0.001 (0.05 of its bar)

Measured on one MI355X (tests/test_snow_unit_gpu.py prints each figure before asserting it):
  largest error / E over all fields and classes: kind 0 3.0 (gpow0; glog 2.6, gexp 1.7, svp 1.3, the albedo 0.8); kind 1 3.2 (p2;
          p7 2.7, p8 2.2, cank1's kd 2.0, sig at |kd - h| / h < 1e-14 1.9; nothing above 1.3 next to kd = h or om = 1 otherwise);
          kind 2 2.5 (cis; Kh 2.1, sn 2.0, cs 1.9, d0 1.8); kind 3 1.3 (rcan)
  gpow0: 2.4 E for |e ln b| < 1, 2.4 E for 1 <= |e ln b| < 32, 3.0 E from 32 on.  BEFORE the fix (gpow0 as exp(e log b) on the lean
          exp and log, the product's rounding entering |e ln b| times): 2.4 E, 47 E (5.5e-15 relative) and 920 E (1.1e-13) against the
          C library's pow, which the reference calls — the test failed.  gpow_pos carries the logarithm as a pair good to 2^-62.
          k_snowmodel, which takes clump^Kc through it, grows by 86 and 81 instructions (3 119 -> 3 205, 4 662 -> 4 743) and 1.2 % in time
          (4.474 / 4.453 ms at the parent, 4.504 / 4.532 ms with the change); registers and scratch unchanged.  The snow-microclimate
          kernels call gpow0 (b > 0) only with the fixed exponent 0.2 (|e ln b| < 3, the lean route's 2.4 E class) and keep the lean route
          as gpow0<false> (6 973 -> 6 972, 8 210 -> 8 209, 7 284 -> 7 283 instructions) — with the precise one k_microsnow_ring took 3.9 %
          longer (3.173 / 3.148 -> 3.296 / 3.274 ms).  The other 153 of the 158 kernels of mcf_kernels.hip and mcf_snow.hip keep their code.
          micro_above ALSO raises to Kc, but not an input: trbn = clumps^Kc and trb = gi^Kc, where clumps = clump^(pais / pai) and gi =
          clump^(paia / pai) are powers themselves and the kernel makes all of them from one logarithm, exp(Kc (pais / pai) log clump).  There
          the reference's own fp64 evaluation rounds the inner power and carries that rounding Kc times: E grows with Kc (6.4e-16 | 6.0e-15 |
          6.3e-14 for Kc in [1, 8) | [8, 64) | [64, 600]), and the shared-logarithm construction stays within 9.0 E of the truth (CPU, 200 000
          cases of pow(pow(clump, r), Kc) in longdouble, fp64 and as exp(Kc r log clump); largest ratios 5.5, 1.2, 9.0 and 2.4 E by class).  It
          is not the defect of gpow0, whose base IS an input (E = 1.2e-16): left as it is; micro_above is outside this entry
  two 46-bit slips that no test sees (scratch builds): fdiv_m in zeroplane moves d0 from 1.7 E to 9.0 E in its worst
          class (7.5e-15 at pai in [0.03, 0.1)); fsqrt_m for kc in the interception model moves no class of cis (largest 2.5 E with and without)
  identities: |x (1 / x) - 1| <= 0.50 x 2^-52 for S1, D1, D2, sig; |h^2 - (a^2 + 2 a gma)| / h^2 <= 1.52 x 2^-52; |sn^2 + cs^2 - 1| <=
          0.94 x 2^-52
  special operands: no class differs from numpy's for gexp (on |x| < 1e90 or NaN), glog, gsqrt, clamp01, rad4, latent_lt0, svp (on |x| <=
          1e300), dewpoint, satvap_r, lapserate_r and the albedo; gpow0 (4^600 and 4^601 = +inf among them) differs from C's pow on 5 of 165 pairs, all recorded: base -0 with an odd integer exponent (+0 / +inf for -0 / -inf), pow(1, NaN) = NaN
  every clamp on the yardstick's side on all cases of its set (80 each, the albedo's 458; uzm_floor and near_cap have no output of their
          own and only their fragile share is checked); cank1 exact for si <= 0; the whole GPU file
          takes one second, 6 200 to 18 640 elements a kind
  deep canopy: the classes of all 26 outputs equal the fp64 yardstick's up to pait h = 709 (594 cases); from 710 on iS1 is NaN where
          the yardstick has inf (S1 is a denormal there and the lean reciprocal gives NaN; the reference's p4 exp(h pait) is 0 x inf
          = NaN from 712 on)
  next to the canopy top: for 0 < 1 - z / h <= 1.9e-9, cos(pi z / h) + 1 rounds to 0 and the reference's own rhcanopy is 0 x inf: the
          fp64 yardstick gives NaN on 384 cases of z_edges, the device on the same 384
These figures are kept here and nowhere else (DESIGN.md section 25 has the method and points here)."""
import functools

import numpy as np

import snow_ref as R

LD = np.longdouble
F64 = np.float64
BAR_FACTOR = 16.0
FRAGILE_FACTOR = 64.0
MAX_FRAGILE = 0.01
STEP_OFF = 2.0 ** 20          # ulps by which a bisected input is stepped off its clamp
NAN = float("nan")
INF = float("inf")


def _freeze(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def _pool(parts, keys):
    where, at = {}, 0
    for n, p in parts.items():
        k = len(p[keys[0]])
        assert all(len(p[q]) == k for q in keys), n
        where[n] = slice(at, at + k)
        at += k
    return _freeze({q: np.concatenate([np.asarray(p[q], dtype=F64) for p in parts.values()]) for q in keys}), where


def _loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _bisect(f, lo, hi):
    """adjacent doubles (lo, hi) around the sign change of the longdouble function f between lo and hi (arrays)"""
    lo, hi = np.array(lo, dtype=F64), np.array(hi, dtype=F64)
    s_lo = np.asarray(f(lo) > 0)
    assert (np.asarray(f(hi) > 0) != s_lo).all()
    for _ in range(1200):
        mid = lo + (hi - lo) / 2
        open_ = (mid != lo) & (mid != hi)
        if not open_.any():
            break
        left = open_ & (np.asarray(f(mid) > 0) == s_lo)
        lo, hi = np.where(left, mid, lo), np.where(open_ & ~left, mid, hi)
    assert (np.nextafter(lo, hi) == hi).all()
    return lo, hi


def _stepped(lo, hi):
    """both sides of a bisected bracket, 2^20 ulp off (away from each other)"""
    out = np.sign(hi - lo)
    return np.concatenate([lo - out * STEP_OFF * np.spacing(np.abs(lo)), hi + out * STEP_OFF * np.spacing(np.abs(hi))])


# ---- kind 0: guards and scalars ------------------------------------------------------------------------------------------------
# the special table: every operand class the guards spell out
_TINY = 5e-324
SPECIAL_X = np.array([0.0, -0.0, _TINY, -_TINY, 1e-310, 2.2250738585072014e-308, np.nextafter(1e-300, 0), 1e-300, np.nextafter(1e-300, 1),
                      np.nextafter(1e300, 0), 1e300, np.nextafter(1e300, INF), 1.7976931348623157e308, -1.0, -1e-300, -1e300, 1.0, 2.0, 0.5,
                      INF, -INF, NAN, -708.0, -745.0, -746.0, -1000.0, -1e89, 709.0, 709.78, 710.0, 1000.0, 1e89])
# gpow0: b in {> 0, 0, < 0, NaN} x e in {> 0, 0, < 0, odd, even, non-integer, NaN}
POW_B = np.array([0.25, 1.0, 0.999, 3.0, 4.0, 0.0, -0.0, -0.5, -1.0, -3.0, NAN])
POW_E = np.array([2.5, 0.0, -0.0, -2.5, 1.0, 3.0, -3.0, 601.0, 2.0, -2.0, 600.0, 0.5, -0.5, 1e-3, NAN])


def _kind0_sets():
    rng = np.random.default_rng(2501)
    s = {}
    n = 4000
    s["weather"] = dict(x=np.concatenate([rng.uniform(-60.0, 40.0, n - 8), [0.0, -0.0, 0.5, -0.5, 1e-300, -1e-300, 40.0, -60.0]]),
                        y=rng.uniform(30.0, 110.0, n))                                  # tc, pk
    s["positive"] = dict(x=_loguniform(rng, 1e-6, 1e3, n), y=rng.uniform(0.0, 1.0, n))   # log, sqrt, dew point (ea)
    s["gsqrt_wide"] = dict(x=_loguniform(rng, 1e-305, 1e305, 2000), y=np.zeros(2000))
    s["exp"] = dict(x=np.concatenate([rng.uniform(-700.0, 700.0, 3000), rng.uniform(-2.0, 2.0, 1000)]), y=np.zeros(4000))
    b = np.concatenate([rng.uniform(0.0, 1.0, 3000), 1.0 - _loguniform(rng, 1e-12, 1e-1, 500), _loguniform(rng, 1e-12, 1e-1, 500)])
    s["pow"] = dict(x=b, y=np.concatenate([_loguniform(rng, 1.0, 600.0, 3500), np.full(250, 1.0), np.full(250, 600.0)]))
    hs = np.concatenate([np.arange(0, 48), [48, 71, 72, 24 * 1013 - 1, 24 * 1013, 24 * 1014 - 1, 24 * 1014, 24 * 1015, 100000, 2 ** 31 - 1],
                         rng.integers(24, 30000, 400)])
    s["albedo"] = dict(x=hs.astype(F64), y=np.zeros(len(hs)))
    s["special"] = dict(x=SPECIAL_X, y=np.full(len(SPECIAL_X), 90.0))
    B, E = np.meshgrid(POW_B, POW_E, indexing="ij")
    s["pow_special"] = dict(x=B.ravel(), y=E.ravel())
    return s


# ---- kind 1: radiation -----------------------------------------------------------------------------------------------------------
def _h_of(lref, ltra):
    return np.asarray(R.twostream(F64, 1.0, lref, ltra, 0.5, 1.0)["h"], dtype=F64)


def _sun(rng, n):
    zen = rng.uniform(0.0, np.pi / 2 * 1.05, n)
    k, kcos = R.cank_zen(F64, zen, 0)
    return dict(kx=np.asarray(k), kcos=np.asarray(kcos), si=rng.uniform(0.0, 1.0, n))


def _leaves(rng, n, om=None):
    om = rng.uniform(0.002, 0.998, n) if om is None else om
    lref = om * rng.uniform(0.05, 0.95, n)
    return lref, om - lref


def _k1(rng, pait, lref, ltra, gref, kd):
    n = len(pait)
    d = dict(pait=pait, lref=lref, ltra=ltra, gref=gref, kd=kd)
    d.update(_sun(rng, n))
    return d


def _kind1_sets():
    rng = np.random.default_rng(2502)
    s = {}
    n = 8000
    lref, ltra = _leaves(rng, n)
    s["random"] = _k1(rng, _loguniform(rng, 0.001, 20.0, n), lref, ltra, rng.uniform(0.1, 0.95, n), _loguniform(rng, 0.01, 600.0, n))
    # kd next to h: kd = h (1 +- 2^-k), k = 4 .. 50, and kd = h as fp64 gives it
    nb = 24
    lref, ltra = _leaves(rng, nb)
    h = _h_of(lref, ltra)
    ks = np.arange(4, 51)
    f = np.concatenate([1.0 + 2.0 ** -ks, 1.0 - 2.0 ** -ks, [1.0]])
    H, Fm = np.meshgrid(h, f, indexing="ij")
    rep = lambda a: np.repeat(a, len(f))          # noqa: E731
    s["kd_near_h"] = _k1(rng, rep(_loguniform(rng, 0.05, 8.0, nb)), rep(lref), rep(ltra), rep(rng.uniform(0.1, 0.95, nb)), (H * Fm).ravel())
    # om next to 1: om = 1 - 10^-j, j = 1 .. 15, 1 - 2^-50 and 1 - 2^-52
    oms = np.concatenate([1.0 - 10.0 ** -np.arange(1.0, 16.0), [1.0 - 2.0 ** -50, 1.0 - 2.0 ** -52]])
    om = np.repeat(oms, 40)
    n2 = len(om)
    lref = om * rng.uniform(0.3, 0.7, n2)
    ltra = om - lref
    ltra = np.where(lref + ltra >= 1.0, np.nextafter(ltra, 0.0), ltra)          # (om = 1 itself is 0 / 0 in the reference)
    s["om_near_1"] = _k1(rng, _loguniform(rng, 0.01, 20.0, n2), lref, ltra, rng.uniform(0.1, 0.95, n2), _loguniform(rng, 0.01, 600.0, n2))
    # symmetric leaves: del = 0
    n3 = 600
    half = rng.uniform(0.001, 0.499, n3)
    s["symmetric"] = _k1(rng, _loguniform(rng, 0.001, 20.0, n3), half, half, rng.uniform(0.1, 0.95, n3), _loguniform(rng, 0.01, 600.0, n3))
    # deep canopy: pait h up to 700 (iS1 = exp(h pait) overflows past 709.78)
    n4 = 600
    lref, ltra = _leaves(rng, n4)
    h = _h_of(lref, ltra)
    depth = np.concatenate([np.linspace(30.0, 700.0, n4 - 8), [705.0, 709.0, 710.0, 712.0, 745.0, 750.0, 800.0, 1500.0]])
    s["deep"] = _k1(rng, depth / h, lref, ltra, rng.uniform(0.1, 0.95, n4), _loguniform(rng, 0.01, 600.0, n4))
    # negated determinant at both clamp ends of the albedo
    n5 = 800
    lref, ltra = _leaves(rng, n5)
    s["gref_ends"] = _k1(rng, _loguniform(rng, 0.001, 20.0, n5), lref, ltra, np.where(np.arange(n5) % 2 == 0, 0.1, 0.95),
                         _loguniform(rng, 0.01, 600.0, n5))
    # cank1: si in {< 0, -0.0, 0, 1e-300, 1e-12, 1}
    sis = np.array([-1.0, -1e-300, -0.0, 0.0, 1e-300, 1e-12, 1.0, NAN])
    n6 = len(sis) * 12 + 1          # (the pooled length is no multiple of the workgroup)
    lref, ltra = _leaves(rng, n6)
    c = _k1(rng, _loguniform(rng, 0.001, 20.0, n6), lref, ltra, rng.uniform(0.1, 0.95, n6), _loguniform(rng, 0.01, 600.0, n6))
    c["si"] = np.concatenate([np.tile(sis, 12), [0.5]])
    s["cank"] = c
    return s


# ---- kind 2: canopy and profile ----------------------------------------------------------------------------------------------------
SDP = np.array([[0.5975, 0.2237, 0.0012, 0.0038], [0.5979, 0.2578, 0.001, 0.0038], [0.594, 0.2332, 0.0016, 0.0031],
                [0.363, 0.2425, 0.0029, 0.0049], [0.217, 0.217, 0.0, 0.0]])      # cpp:3741-3749


def _k2_base(rng, n):
    """ordinary values of all 32 planes"""
    h = _loguniform(rng, 0.001, 40.0, n)
    pai = _loguniform(rng, 0.001, 20.0, n)
    d = np.asarray(R.zeroplane(F64, h, pai))
    zm = np.asarray(R.roughlength(F64, h, pai, d)[2])
    tc = rng.uniform(-60.0, 40.0, n)
    sint = np.asarray(R.snow_sint(F64, tc))
    env = rng.integers(0, 5, n)
    z = h * rng.uniform(0.001, 0.999, n)
    zref = h + rng.uniform(0.5, 10.0, n)
    c = dict(h=h, pai=pai, d=d, uf=_loguniform(rng, 0.001, 3.0, n), prec=np.where(rng.random(n) < 0.1, 0.0, _loguniform(rng, 0.01, 30.0, n)),
             sint=sint, Li=sint * pai * rng.uniform(0.0, 0.9, n), sdp0=SDP[env, 0], sdp1=SDP[env, 1], sdp2=SDP[env, 2], sdp3=SDP[env, 3],
             depth=_loguniform(rng, 1e-4, 10.0, n), age=rng.integers(1, 5000, n).astype(F64), x=rng.uniform(0.0, np.pi, n), z=z,
             leafden=rng.uniform(0.05, 3.0, n), Flux=rng.uniform(-200.0, 400.0, n), Fluxz=rng.uniform(-50.0, 100.0, n),
             SH=rng.uniform(230.0, 310.0, n) * 29.3 * 43.0, SG=rng.uniform(230.0, 310.0, n) * 29.3 * 43.0, mxnear=rng.uniform(100.0, 5000.0, n),
             zm=zm, zref=zref, za=h + (zref - h) * rng.uniform(0.0, 1.0, n), T0=rng.uniform(-60.0, 40.0, n), tc=tc,
             ea=rng.uniform(0.001, 2.0, n), slope=np.where(rng.random(n) < 0.1, 0.0, rng.uniform(0.0, 60.0, n)),
             aspect=rng.uniform(0.0, 360.0, n), zend=rng.uniform(0.0, 130.0, n), azid=rng.uniform(0.0, 360.0, n), hc=h)
    return c


def _with(c, **over):
    n = len(c["h"])
    c = dict(c)
    for k, v in over.items():
        c[k] = np.broadcast_to(np.asarray(v, dtype=F64), (n,)).copy()
    return c


def _kind2_sets():
    rng = np.random.default_rng(2503)
    s = {}
    s["random"] = _k2_base(rng, 8000)
    # z next to h and next to 0; z / h on and +-1 ulp of the quadrant seams of sincos_0pi
    ks = np.arange(1, 53)
    fr = np.concatenate([[1.0], 1.0 - 2.0 ** -ks, 2.0 ** -ks])
    seams = []
    for q in (0.25, 0.5, 0.75):
        seams += [np.nextafter(q, 0), q, np.nextafter(q, 1)]
    fr = np.concatenate([fr, seams])
    nb = 16
    b = _k2_base(rng, nb * len(fr))
    hb = np.repeat(np.concatenate([[1.0, 2.0, 0.5, 10.0], _loguniform(rng, 0.001, 40.0, nb - 4)]), len(fr))
    d = np.asarray(R.zeroplane(F64, hb, b["pai"]))
    s["z_edges"] = _with(b, h=hb, d=d, z=hb * np.tile(fr, nb), hc=hb)
    # sincos_0pi: [0, pi] densely, the seams in x, 3.1416 and just past it, negative, 1e9 +- 1, NaN
    xs = np.concatenate([np.linspace(0.0, np.pi, 3000), [np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi, 3.1416, np.nextafter(3.1416, 4), 3.15, 4.0,
                                                         7.0, 100.0, -1e-300, -0.5, -3.0, -100.0, 1e9 - 1, 1e9, 1e9 + 1, 1e15, NAN, 0.0, -0.0,
                                                         5e-324, 1e-300]])
    for q in (np.pi / 4, np.pi / 2, 3 * np.pi / 4):
        xs = np.concatenate([xs, q + np.arange(-8, 9) * np.spacing(q)])
    s["sincos"] = _with(_k2_base(rng, len(xs)), x=xs)
    # ---- clamps: inputs bisected on the longdouble yardstick, then stepped off by 2^20 ulp
    # zm at 0.9 (h - d): exp(-ka / Be) against 0.9 depends on pai alone
    nb = 40
    b = _k2_base(rng, nb)
    hh = _loguniform(rng, 0.1, 40.0, nb)          # (0.9 (h - d) above the 0.0005 floor, which would win otherwise)
    b = _with(b, h=hh, d=0.8 * hh, z=0.5 * hh, hc=hh)
    lo, hi = _bisect(lambda p: (lambda r: r[0] - r[1])(R.roughlength(LD, b["h"], p, b["d"])), np.full(nb, 20.0), np.full(nb, 400.0))
    b2 = {k: np.concatenate([v, v]) for k, v in b.items()}
    s["zm_cap"] = _with(b2, pai=_stepped(lo, hi))
    # zm at 0.0005: bisect h with d = 0.7 h
    b = _k2_base(rng, nb)
    dz = lambda hh: np.asarray(0.7 * np.asarray(hh, dtype=F64))      # noqa: E731
    lo, hi = _bisect(lambda hh: R.roughlength(LD, hh, b["pai"], dz(hh))[0] - LD(0.0005), np.full(nb, 1e-4), np.full(nb, 1e3))
    hh = _stepped(lo, hi)
    b2 = {k: np.concatenate([v, v]) for k, v in b.items()}
    s["zm_floor"] = _with(b2, h=hh, d=dz(hh), z=0.5 * hh, hc=hh)
    # cis at prec (reached with a negative load only: with Li >= 0 the slope of cis in prec stays below 0.678)
    b = _k2_base(rng, nb)
    b = _with(b, Li=-3.0 * b["sint"] * b["pai"], pai=rng.uniform(1.0, 10.0, nb))
    b = _with(b, Li=-3.0 * b["sint"] * b["pai"])
    f = lambda p: (lambda r: r["cis_raw"] - LD(1) * np.asarray(p, dtype=F64).astype(LD))(R.canopysnowint(LD, b["hc"], b["pai"], b["uf"], p, b["sint"], b["Li"]))  # noqa: E731
    lo, hi = _bisect(f, np.full(nb, 1e-6), np.full(nb, 1e4))
    b2 = {k: np.concatenate([v, v]) for k, v in b.items()}
    s["cis_cap"] = _with(b2, prec=_stepped(lo, hi))
    # uzm at uf: the ratio depends on pai alone
    b = _k2_base(rng, nb)
    f = lambda p: R.canopysnowint(LD, b["hc"], p, b["uf"], b["prec"], b["sint"], b["Li"])["uzm_raw"] - b["uf"].astype(LD)   # noqa: E731
    lo, hi = _bisect(f, np.full(nb, 0.01), np.full(nb, 20.0))
    b2 = {k: np.concatenate([v, v]) for k, v in b.items()}
    s["uzm_floor"] = _with(b2, pai=_stepped(lo, hi))
    # rHa at 0.001: bisect uf (rHa falls as 1 / uf)
    b = _k2_base(rng, nb)
    f = lambda u: R.rhcanopy(LD, u, b["h"], b["d"], b["z"])[0] - LD(0.001)      # noqa: E731
    lo, hi = _bisect(f, np.full(nb, 1e-3), np.full(nb, 1e9))
    b2 = {k: np.concatenate([v, v]) for k, v in b.items()}
    s["rha_floor"] = _with(b2, uf=_stepped(lo, hi))
    # z at d + 0.2 zm (TVabove's branch): bisect za
    b = _k2_base(rng, nb)
    f = lambda za: R.tvabove(LD, za, b["zref"], b["d"], b["zm"], b["T0"], b["tc"], b["ea"])["margin"]      # noqa: E731
    lo, hi = _bisect(f, b["d"] * 0.5, b["zref"])
    b2 = {k: np.concatenate([v, v]) for k, v in b.items()}
    s["above_branch"] = _with(b2, za=_stepped(lo, hi))
    # |near| at mxnear: bisect Fluxz, both signs
    b = _k2_base(rng, nb)
    sign = np.where(np.arange(nb) % 2 == 0, 1.0, -1.0)
    f = lambda q: np.abs(R.tvbelow(LD, b["z"], b["d"], b["h"], b["pai"], b["uf"], b["leafden"], b["Flux"], q, b["SH"], b["SG"], b["mxnear"])["near_raw"]) - b["mxnear"].astype(LD)  # noqa: E731
    lo, hi = _bisect(f, sign * 1e-6, sign * 1e12)
    b2 = {k: np.concatenate([v, v]) for k, v in b.items()}
    s["near_cap"] = _with(b2, Fluxz=_stepped(lo, hi))
    # the hgt and pai floors of the interception model, slope 0, the horizon of solar_index, NaN operands
    b = _k2_base(rng, 64)
    s["floors"] = _with(b, hc=np.resize([0.0, 0.0005, 0.001, np.nextafter(0.001, 1), 0.002, -1.0, 1e-300, 0.0011], 64),
                        pai=np.resize([0.0, 0.0005, 0.001, 0.0011, 2.0], 64), slope=np.resize([0.0, -0.0, 10.0, 90.0], 64),
                        zend=np.resize([90.0, np.nextafter(90.0, 91), np.nextafter(90.0, 0), 89.0, 91.0, 135.0, 0.0], 64))
    return s


# ---- kind 3: step weather ----------------------------------------------------------------------------------------------------------
def _kind3_sets():
    rng = np.random.default_rng(2504)
    n = 6000
    s = {}
    tc = rng.uniform(-60.0, 40.0, n)
    s["random"] = dict(tc=tc, rh=rng.uniform(1.0, 100.0, n), pk=rng.uniform(50.0, 110.0, n), tci=tc + rng.uniform(-15.0, 15.0, n),
                       mxtc=rng.uniform(-20.0, 50.0, n))
    # the water / ice and latent-heat branches: tc and te at +-0 and +-0.5
    v = np.array([0.0, -0.0, 0.5, -0.5, 1e-300, -1e-300, np.nextafter(0.5, 1), np.nextafter(0.5, 0), np.nextafter(-0.5, 0), np.nextafter(-0.5, -1)])
    T, TE = np.meshgrid(v, v, indexing="ij")
    T, TE = T.ravel(), TE.ravel()
    m = len(T)
    s["branches"] = dict(tc=np.concatenate([T, rng.uniform(-60, 40, m)]), rh=rng.uniform(1.0, 100.0, 2 * m), pk=rng.uniform(50.0, 110.0, 2 * m),
                         tci=np.concatenate([2.0 * TE - T, 2.0 * TE - T]), mxtc=rng.uniform(-20.0, 50.0, 2 * m))
    s["branches"]["tci"][m:] = 2.0 * TE - s["branches"]["tc"][m:]
    return s


KEYS = {0: ("x", "y"), 1: R.KIND1_INPUTS, 2: R.KIND2_INPUTS, 3: R.KIND3_INPUTS}
FIELDS = {0: R.KIND0_FIELDS, 1: R.KIND1_FIELDS, 2: R.KIND2_FIELDS, 3: R.KIND3_FIELDS}
_SETS = {0: _kind0_sets, 1: _kind1_sets, 2: _kind2_sets, 3: _kind3_sets}


@functools.lru_cache(maxsize=None)
def pooled(kind):
    """(inputs, {set: slice}) of one kind, every set back to back"""
    return _pool(_SETS[kind](), KEYS[kind])


def evaluate(kind, T, c):
    """the kind's fields (and the operands of its branches) over the number type T from input planes c"""
    if kind == 0:
        o = R.scalars(T, c["x"], c["y"])
        x, = R._a(T, c["x"])
        o["clamp01"] = np.where(x > 1, T(1), np.where(x < 0, T(0), x))
        xs = np.asarray(c["x"], dtype=F64)
        with np.errstate(all="ignore"):
            ok = (xs >= 0) & (xs < 2.0 ** 31)                   # the entry's own guard around its (int) cast, which truncates
        o["alb_raw"], o["snow_albedo"] = R.snow_albedo(T, np.where(ok, np.trunc(np.where(ok, xs, 0.0)), 0.0))
        return o
    if kind == 1:
        o = R.twostream(T, c["pait"], c["lref"], c["ltra"], c["gref"], c["kd"])
        o.update(R.cank(T, c["kx"], c["kcos"], c["si"]))
        return o
    if kind == 2:
        return R.canopy(T, c)
    return R.step_weather(T, c["tc"], c["rh"], c["pk"], c["tci"], c["mxtc"])


@functools.lru_cache(maxsize=None)
def yardsticks(kind):
    """(truth, literal): the kind's fields over its pooled sets in longdouble and in fp64, computed once"""
    c, _ = pooled(kind)
    return evaluate(kind, LD, c), evaluate(kind, F64, c)


# ---- floating fields: error against the truth, E, classes ------------------------------------------------------------------------
# absolute error for what is bounded by 1 and crosses zero, and for temperatures in degrees C; relative to the truth elsewhere
ABSOLUTE = {"sn", "cs", "cS", "sS", "cA", "sA", "del", "u1", "si0", "si1", "Tz", "tdew", "m_tdew", "te", "dewpoint"}


def field_error(x, truth, field):
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(x).astype(LD) - truth)
        if field not in ABSOLUTE:
            d = np.where(d == 0, LD(0), d / np.abs(truth))
        return np.where(np.isfinite(truth) & ((truth != 0) | (field in ABSOLUTE)), d, LD(np.nan))


def _bins(v, edges, name):
    """{class name: mask}: v < edges[0], [edges[0], edges[1]), ..., >= edges[-1]"""
    v = np.asarray(v, dtype=F64)
    out = {f"{name}<{edges[0]:g}": v < edges[0]}
    for a, b in zip(edges[:-1], edges[1:]):
        out[f"{a:g}<={name}<{b:g}"] = (v >= a) & (v < b)
    out[f"{name}>={edges[-1]:g}"] = v >= edges[-1]
    return out


DIF_FIELDS = ("om", "a", "gma", "del", "h", "S1", "iS1", "iD1", "iD2", "u1", "u2", "D1", "D2", "p1", "p2", "p3", "p4")
DIR_FIELDS = ("sig", "isig", "S2", "p5", "p6", "p7", "p8", "p9", "p10")
CANK_FIELDS = ("k", "kd", "Kc")
DEEP = 30.0           # pait h from which S1 and iS1 are 13 orders apart: only the class of each output is asserted


@functools.lru_cache(maxsize=None)
def classes(kind):
    """{field: {class: mask}} over the pooled sets of one kind.  Cases in no class of a field are not held to the 16 E bar on
    it (the special tables, the deep canopy, non-finite truths)."""
    c, where = pooled(kind)
    truth, _ = yardsticks(kind)
    n = len(c[KEYS[kind][0]])
    out = {}

    def only(*names):
        m = np.zeros(n, dtype=bool)
        for q in names:
            m[where[q]] = True
        return m
    if kind == 0:
        w, p = only("weather"), only("positive")
        out["svp"] = out["rad4"] = out["latent_lt0"] = out["satvap_r"] = out["lapserate_r"] = {"tc": w}
        with np.errstate(all="ignore"):
            lnx = np.abs(np.log(c["x"]))
        out["glog"] = _and(_bins(lnx, [1e-2, 1.0], "|ln x|"), p)
        out["dewpoint"] = {"ea": p & (c["x"] >= 1e-3) & (c["x"] <= 10.0)}
        out["gsqrt"] = {"x": p | only("gsqrt_wide")}
        out["gexp"] = _and(_bins(np.abs(c["x"]), [1.0, 30.0], "|x|"), only("exp"))
        with np.errstate(all="ignore"):
            el = np.abs(c["y"] * np.log(c["x"]))
        out["snow_albedo"] = {"hs>=24": only("albedo") & (c["x"] >= 24)}
        out["gpow0"] = _and(_bins(el, [1.0, 32.0], "|e ln b|"), only("pow") & (c["x"] > 0) & (el < 700.0))
        return out
    if kind == 1:
        t = truth
        shallow = np.asarray(t["h"] * c["pait"].astype(LD) < LD(DEEP)) & ~only("cank")
        om1 = _bins(1.0 - (c["lref"] + c["ltra"]), [1e-8, 1e-3], "1-om")
        with np.errstate(all="ignore"):
            rel = np.asarray(np.abs(c["kd"].astype(LD) - t["h"]) / t["h"], dtype=F64)
        kdh = _bins(rel, [1e-14, 1e-12, 1e-10, 1e-8, 1e-6, 1e-4, 1e-2], "|kd-h|/h")
        fin = np.isfinite(c["si"])
        for f in DIF_FIELDS:
            out[f] = _and(om1, shallow)
        # (S2 = exp(-kd pait) leaves the normal range past 708: what depends on it is held to the bar below that)
        s2ok = np.asarray(c["kd"] * c["pait"] < 700.0)
        for f in DIR_FIELDS:
            out[f] = {f"{a}, {b}": ma & mb & shallow & (s2ok | (f in ("sig", "isig", "p5", "p8"))) for a, ma in om1.items() for b, mb in kdh.items()}
        for f in CANK_FIELDS:
            out[f] = {"si>0": fin & (c["si"] > 0), "si<=0": fin & (c["si"] <= 0)}
        return out
    if kind == 2:
        okz = (c["z"] > 0) & (c["z"] < c["h"])
        zh = _bins(1.0 - c["z"] / c["h"], [1e-12, 1e-6, 1e-2, 1e-1], "1-z/h")
        zl = _bins(c["z"] / c["h"], [1e-12, 1e-6, 1e-2], "z/h")
        prof = {f"{a}, {b}": ma & mb & okz for a, ma in zh.items() for b, mb in zl.items()}
        prof = {k: m for k, m in prof.items() if m.any()}
        for f in ("rz", "Kg"):
            out[f] = prof
        # Kh = 1 / ((Rc - rz) (h - z)): Rc - rz cancels next to the top and where both sit near their 0.001 floor
        with np.errstate(all="ignore"):
            gap = _bins(np.asarray((truth["Rc"] - truth["rz"]) / truth["Rc"], dtype=F64), [1e-3, 1e-1], "(Rc-rz)/Rc")
        profk = {f"{a}, {b}": ma & mb for a, ma in prof.items() for b, mb in gap.items() if (ma & mb).any()}
        out["Kh"] = out["iKs"] = profk
        # tv_below adds the near-field term to the far-field one: where they cancel (|near| + |far| over |sum|) E grows with it
        with np.errstate(all="ignore"):
            cancel = _bins(np.asarray(truth["tvb_terms"] / np.abs(truth["tvb"]), dtype=F64), [1.5, 8.0], "cancel")
        out["tvb"] = {f"{a}, {b}": ma & mb for a, ma in profk.items() for b, mb in cancel.items() if (ma & mb).any()}
        allm = np.ones(n, dtype=bool)
        # 1 - exp(-s) and 1 - (..) / s cancel as s = sqrt(7.5 pai) falls; exp(-ka / Be) takes an argument of up to 7 at small pai
        bypai = _bins(np.maximum(c["pai"], 0.001), [0.003, 0.01, 0.03, 0.1, 0.3, 1.0], "pai")
        out["d0"] = out["zm0"] = bypai
        for f in ("sden", "Rc", "Kc", "iKc", "cS", "sS", "cA", "sA", "si0", "si1"):
            out[f] = {"all": allm}
        # the interception model's three differences: the canopy cover 1 - exp(-kc pai), 1 - exp(-k2 prec), Lstr - Li
        wet = c["prec"] > 0
        with np.errstate(all="ignore"):
            cover = _bins(np.asarray(truth["kcpai"], dtype=F64), [1e-2, 1e-1, 1.0], "kc pai")
            fill = _bins(np.asarray(truth["k2prec"], dtype=F64), [1e-4, 1e-3, 1e-2, 1e-1, 1.0], "k2 prec")
            room = _bins(np.asarray(truth["room"], dtype=F64), [0.3], "1-Li/Lstr")
        out["cis"] = {f"{a}, {b}, {d}": ma & mb & md & wet for a, ma in cover.items() for b, mb in fill.items() for d, md in room.items()
                      if (ma & mb & md & wet).any()}
        inpi = (c["x"] >= 0) & (c["x"] <= 3.1416)
        out["sn"] = out["cs"] = {"0<=x<=3.1416": inpi, "elsewhere, |x|<1e9": ~inpi & (np.abs(c["x"]) < 1e9)}
        above = np.asarray(truth["above_margin"] > 0)
        out["Tz"] = out["ez"] = {"above": above, "at or below d + zh": ~above}
        return out
    allm = np.ones(n, dtype=bool)
    out = {f: {"all": allm} for f in R.KIND3_FIELDS}
    out["Da"] = _bins(100.0 - c["rh"], [0.1, 1.0, 10.0], "100-rh")          # es - ea = es (1 - rh / 100) cancels towards saturation
    return out


def _and(d, m):
    return {k: v & m for k, v in d.items()}


def compare_fields(kind, got, fields=None):
    """Rows (field, class, cases, E, device error): `got[field]` against the longdouble yardstick beside the fp64 yardstick's own
    error on the same cases."""
    truth, lit = yardsticks(kind)
    rows = []
    for f, cl in classes(kind).items():
        if fields is not None and f not in fields:
            continue
        e_lit, e_got = field_error(lit[f], truth[f], f), field_error(got[f], truth[f], f)
        for name, m in cl.items():
            m = m & np.isfinite(np.asarray(e_lit, dtype=F64))
            if m.any():
                rows.append((f, name, int(m.sum()), float(np.max(e_lit[m])), float(np.max(np.nan_to_num(np.asarray(e_got, dtype=F64)[m], nan=np.inf)))))
    return rows


def format_rows(rows, title):
    out = [f"{title}: field, class, cases, E (fp64 yardstick), error, error / E"]
    for f, c, n, e, g in rows:
        out.append(f"  {f:11s} {c:42s} {n:6d}  {e:9.3e}  {g:9.3e}  {g / e if e > 0 else (0.0 if g == 0 else np.inf):7.2f}")
    return "\n".join(out)


def value_class(v):
    """0 NaN, 1 +inf, 2 -inf, 3 +0, 4 -0, 5 finite > 0, 6 finite < 0"""
    v = np.asarray(v, dtype=F64)
    out = np.full(v.shape, 5, dtype=np.int64)
    out[v < 0] = 6
    out[(v == 0) & ~np.signbit(v)] = 3
    out[(v == 0) & np.signbit(v)] = 4
    out[v == INF] = 1
    out[v == -INF] = 2
    out[np.isnan(v)] = 0
    return out


# ---- branch-deciding comparisons -------------------------------------------------------------------------------------------------
# (kind, set, the yardstick's operand, the threshold (field name or number), direction: clamped when operand `op` threshold, the
# output that carries the clamp, the clamp's value (field / input name or number))
CLAMPS = (
    ("zm_cap", 2, "zm_cap", "zm_raw", "zm_cap", ">", "zm0", "zm_cap"),
    ("zm_floor", 2, "zm_floor", "zm_raw", 0.0005, "<", "zm0", 0.0005),
    ("cis_cap", 2, "cis_cap", "cis_raw", "prec", ">", "cis", "prec"),
    ("uzm_floor", 2, "uzm_floor", "uzm_raw", "uf", "<", None, None),
    ("rha_floor", 2, "rha_floor", "rz_raw", 0.001, "<", "rz", 0.001),
    ("above_branch", 2, "above_branch", "above_margin", 0.0, "<=", "Tz", "T0"),
    ("near_cap", 2, "near_cap", "near_abs", "mxnear", ">", None, None),
    ("albedo_hi", 0, "albedo", "alb_raw", 0.95, ">", "snow_albedo", 0.95),
    ("albedo_lo", 0, "albedo", "alb_raw", 0.1, "<", "snow_albedo", 0.1),
)


def clamp_margin(name):
    """Of one clamp: (slice, clamped (the truth's side), fragile, E, threshold as fp64, the clamp's fp64 value or None)"""
    _, kind, sname, op, thr, rel, _, val = next(c for c in CLAMPS if c[0] == name)
    c, where = pooled(kind)
    truth, lit = yardsticks(kind)
    s = where[sname]

    def operand(y):
        if op == "near_abs":
            return np.abs(y["near_raw"][s])
        return y[op][s]

    def named(v, y):
        if isinstance(v, str):
            return (y[v][s] if v in y else c[v][s].astype(LD))
        return LD(v)
    t_op, l_op, t_thr = operand(truth), operand(lit), named(thr, truth)
    with np.errstate(all="ignore"):
        clamped = {">": t_op > t_thr, "<": t_op < t_thr, "<=": t_op <= t_thr}[rel]
        scale = np.maximum(np.abs(t_thr), LD(1e-300)) if not np.isscalar(thr) or thr != 0.0 else np.abs(c["za"][s].astype(LD))
        err = np.abs(l_op.astype(LD) - t_op) / scale
        finite = np.isfinite(np.asarray(err, dtype=F64))
        e = float(np.max(err[finite])) if finite.any() else 0.0
        fragile = np.asarray(np.abs(t_op - t_thr) / scale < FRAGILE_FACTOR * e)
    v = None if val is None else np.asarray(named(val, lit), dtype=F64) * np.ones(s.stop - s.start)
    return s, np.asarray(clamped), fragile, e, v


def clamp_other_side(name):
    """Of one clamp with a device output: (the yardstick's unclamped value of that output over the set, in longdouble, and the fp64
    yardstick's largest absolute error on it) — what a fragile case may hold instead of the clamp's own value"""
    _, kind, sname, op, _, _, outf, _ = next(c for c in CLAMPS if c[0] == name)
    _, where = pooled(kind)
    truth, lit = yardsticks(kind)
    s = where[sname]
    key = "Tz_up" if name == "above_branch" else op
    alt = truth[key][s]
    with np.errstate(all="ignore"):
        err = np.abs(lit[key][s].astype(LD) - alt)
    err = np.asarray(err, dtype=F64)
    return alt, float(err[np.isfinite(err)].max())
