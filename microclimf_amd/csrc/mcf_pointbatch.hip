// mcf_pointbatch.hip — the point models for MANY points at once (gfx950): mcf_bigleaf_batch, mcf_weatherhgt_batch,
// mcf_pointmprocess_batch and, further down with its own introduction, mcf_pointmodelsnow_batch (include/mcf.h).  One point of BigLeafCpp is a serial job; P points of `runpointmodela` are not:
// the points are independent, and inside one iteration every hour reads only its own state of the iteration before
// (mcf_pointmodel.cpp, the loop of mcf_bigleaf).  What couples hours is GFluxCpp: daily means, a 6-hour circular trailing
// mean, the day's min / max on iteration 0, and with yearG a 91-day circular mean of daily values and one sum over the
// series.  So: one lane per (point, hour), the step fastest, and short stencils between launches.
//
//   k_bl_setup        once: everything that depends on the inputs only (the host recomputes it every iteration): the sun, the
//                     whole of RadswabsCpp, the canopy conductance, ea / tdew / srh, the soil's 6-hour mean Gmud; the
//                     initial state
//   k_bl_year_setup   once, yearG: the 91-day means of k and kap, folded into Gmuy per day
//   k_bl_step         per iteration: the body of the hour loop; the point's max |dT| through an integer atomic max on the bits
//                     of a non-negative double (order independent)
//   k_bl_gflux        per iteration: GFluxCpp's daily part, a workgroup = 8 days of one point staged in LDS
//   k_bl_annual       per iteration, yearG: GFluxCpp's annual term, one workgroup per point, sums in the host's order
//   k_bl_finish       per iteration: convergence PER POINT; counts the points that go on
//
// fp64, no fast-math, no FMA contraction (this unit is compiled with -ffp-contract=off): the operands and the order of
// every expression are those of mcf_pointmodel.cpp, so that the device differs from the host library only where libm does
// (exp, log, pow, the trigonometric functions).  Constants that depend on the point or on the date alone come from the host
// (mcf_pointbatch.h).  A point's result does not depend on the batch it is in or on how the batch is cut into blocks: no
// lane reads another point's data and no sum's order depends on the launch geometry.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mcf_rowblocks.hpp"
#include "mcf_hiphost.hpp"
#include "mcf_pointbatch.h"

#pragma clang fp contract(off)

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kToRad = kPi / 180.0;
constexpr double kSb = 5.67e-8;
constexpr double kThetam = 0.365;
constexpr double kKa = 0.4;
constexpr double kOmdy = (2.0 * kPi) / (24.0 * 3600.0);
constexpr int kStepBlock = 256;
constexpr int kDaysPerGroup = 8;                    // k_bl_gflux / k_pointmprocess: 8 days = 192 lanes = 3 waves
constexpr int kGroup = kDaysPerGroup * 24;

// ---- device restatement of the host helpers (same expressions; integer powers as products, x^(1/4) as sqrt(sqrt(x))) -----
__device__ __forceinline__ double p2(double x) { return x * x; }
__device__ __forceinline__ double p3(double x) { return x * x * x; }
__device__ __forceinline__ double p4(double x) { const double y = x * x; return y * y; }
__device__ __forceinline__ double root4(double x) { return sqrt(sqrt(x)); }
__device__ __forceinline__ double radem(double tc) { return p4(tc + 273.15); }
__device__ __forceinline__ double satvap(double tc) {
    return tc > 0 ? 0.61078 * exp(17.27 * tc / (tc + 237.3)) : 0.61078 * exp(21.875 * tc / (tc + 265.5));
}
__device__ __forceinline__ double dewpoint(double ea) {
    const double l = log(ea / 0.6112);
    return 243.5 * l / (17.67 - l);
}
__device__ __forceinline__ double phair(double tc, double pk) { return 44.6 * (pk / 101.3) * (273.15 / (tc + 273.15)); }
__device__ __forceinline__ double cpair(double tc) { return 2e-05 * p2(tc) + 0.0002 * tc + 29.119; }

struct Sun { double zend, zenr, azid; };
// sun_position with the date terms (eot, sin / cos of the declination) and sin / cos of the latitude from the host
__device__ Sun sun_position(double sl, double cl, double lon, const double* __restrict__ t) {
    const double sd = t[mcf::TC_SINDEC], cd = t[mcf::TC_COSDEC];
    const double st = t[mcf::TC_HOUR] + (4.0 * lon + t[mcf::TC_EOT]) / 60.0;
    const double tt = 0.261799 * (st - 12);
    const double ct = cos(tt), stt = sin(tt);
    const double coh = sd * sl + cd * cl * ct;
    const double z = acos(coh) * (180 / kPi);
    const double sh = coh;
    const double hh = atan(sh / sqrt(1 - sh * sh));
    const double sazi = cd * stt / cos(hh);
    const double cn = sl * cd * ct - cl * sd;
    const double cazi = cn / sqrt(p2(cd * stt) + p2(cn));
    double sqt = 1 - sazi * sazi;
    if (sqt < 0) sqt = 0;
    double azi = 180 + (180 * atan(sazi / sqrt(sqt))) / kPi;
    if (cazi < 0) azi = sazi < 0 ? 180 - azi : 540 - azi;
    return {z, z * kToRad, azi};
}
// slope, its cosine and sine, aspect: s[0..3] (BC_SLOPE.. / PS_SLOPE.. of the point's table)
__device__ double solar_index(const double* __restrict__ s, double zend, double azid) {
    double si;
    if (zend > 90.0) si = 0;
    else if (s[0] == 0.0) si = cos(zend * kToRad);
    else si = cos(zend * kToRad) * s[1] + sin(zend * kToRad) * s[2] * cos((azid - s[3]) * kToRad);
    return si < 0.0 ? 0.0 : si;
}
struct Ext { double k, kd, Kc; };
__device__ Ext canopy_k(double zenr, double x, double si) {
    if (zenr > kPi / 2.0) zenr = kPi / 2.0;
    if (si < 0.0) si = 0.0;
    double k;
    if (x == 1.0) k = 1.0 / (2.0 * cos(zenr));
    else if (isinf(x)) k = 1.0;
    else if (x == 0.0) k = tan(zenr);
    else k = sqrt(x * x + tan(zenr) * tan(zenr)) / (x + 1.774 * pow(x + 1.182, -0.733));
    if (k > 6000.0) k = 6000.0;
    Ext e{k, k * cos(zenr) / si, 1.0 / si};
    if (si == 0) { e.kd = 1.0; e.Kc = 600.0; }
    return e;
}
// the diffuse two-stream coefficients the direct ones need: from the host's table (big leaf: they depend on the point
// only) or from two_stream_dif below (snow: the canopy above the pack changes with every step)
struct Dif { double om, a, gma, J, del, h, u1, S1, D1, D2, p3, p4; };
__device__ Dif two_stream_dif(double pait, double x, double lref, double ltra, double gref) {
    Dif p;
    p.om = lref + ltra; p.a = 1.0 - p.om; p.del = lref - ltra; p.J = 1.0 / 3.0;
    if (x != 1.0) {
        double mla = 9.65 * pow(3.0 + x, -1.65);
        if (mla > kPi / 2.0) mla = kPi / 2.0;
        p.J = cos(mla) * cos(mla);
    }
    p.gma = 0.5 * (p.om + p.J * p.del);
    p.h = sqrt(p.a * p.a + 2.0 * p.a * p.gma);
    p.S1 = exp(-p.h * pait);
    p.u1 = p.a + p.gma * (1.0 - 1.0 / gref);
    const double u2 = p.a + p.gma * (1.0 - gref);
    p.D1 = (p.a + p.gma + p.h) * (p.u1 - p.h) * 1.0 / p.S1 - (p.a + p.gma - p.h) * (p.u1 + p.h) * p.S1;
    p.D2 = (u2 + p.h) * 1.0 / p.S1 - (u2 - p.h) * p.S1;
    p.p3 = (1.0 / (p.D2 * p.S1)) * (u2 + p.h);
    p.p4 = (-p.S1 / p.D2) * (u2 - p.h);
    return p;
}
struct Dir { double sig, p5, p6, p7, p8, p9, p10; };
__device__ Dir two_stream_dir(double pait, const Dif& f, double gref, double kd) {
    const double a = f.a, gma = f.gma, om = f.om, J = f.J, del = f.del, u1 = f.u1, h = f.h, D1 = f.D1, D2 = f.D2, S1 = f.S1;
    Dir p;
    const double sig = kd * kd + gma * gma - p2(a + gma);
    const double ss = 0.5 * (om + J * del / kd) * kd;
    const double sstr = om * kd - ss;
    const double S2 = exp(-kd * pait);
    const double u2 = a + gma * (1.0 - gref);
    p.p5 = -ss * (a + gma - kd) - gma * sstr;
    const double v1 = ss - (p.p5 * (a + gma + kd)) / sig;
    const double v2 = ss - gma - (p.p5 / sig) * (u1 + kd);
    p.p6 = (1.0 / D1) * ((v1 / S1) * (u1 - h) - (a + gma - h) * S2 * v2);
    p.p7 = (-1.0 / D1) * ((v1 * S1) * (u1 + h) - (a + gma + h) * S2 * v2);
    p.sig = -sig;
    p.p8 = sstr * (a + gma + kd) - gma * ss;
    const double v3 = (sstr + gma * gref - (p.p8 / p.sig) * (u2 - kd)) * S2;
    p.p9 = (-1 / D2) * ((p.p8 / (p.sig * S1)) * (u2 + h) + v3);
    p.p10 = (1 / D2) * (((p.p8 * S1) / p.sig) * (u2 - h) + v3);
    return p;
}
__device__ __forceinline__ double roughlength(double hmd, double hde, double psi_h) {
    double zm = hde * exp(kKa * psi_h);
    if (zm > 0.9 * hmd) zm = 0.9 * hmd;
    if (zm < 0.0005) zm = 0.0005;
    return zm;
}
__device__ __forceinline__ double clamp_psi(double v) {
    if (v < -4.0) v = -4.0;
    if (v > 3.0) v = 3.0;
    return v;
}
__device__ double psi_m(double ze) {
    double v;
    if (ze < 0) {
        const double x = root4(1.0 - 15.0 * ze);
        v = log(p2((1.0 + x) / 2.0) * (1 + p2(x)) / 2.0) - 2.0 * atan(x) + kPi / 2.0;
    } else v = -4.7 * ze;
    return clamp_psi(v);
}
__device__ double psi_h(double ze) {
    double v;
    if (ze < 0) {
        const double y = sqrt(1.0 - 9.0 * ze);
        v = log(p2((1.0 + y) / 2.0));
    } else v = -(4.7 * ze) / 0.74;
    return clamp_psi(v);
}
__device__ double phi_h(double ze) {
    double v;
    if (ze < 0) {
        const double phim = 1 / root4(1.0 - 16.0 * ze);
        v = p2(phim);
    } else v = 1 + ((6.0 * ze) / (1.0 + ze));
    if (v > 1.5) v = 1.5;
    if (v < 0.5) v = 0.5;
    return v;
}
__device__ __forceinline__ double g_free(double d, double H) {          // d = 0.71 leafd
    const double dT = 0.7045388 * pow(d * p4(H), 0.2);
    double g = 0.0375 * root4(dT / d);
    if (g < 0.1) g = 0.1;
    return g;
}
__device__ double stom_cond(const double* __restrict__ c, double Rswabs, double theta) {
    if (Rswabs <= 0.0) return 0.0;
    const double Rsmx = c[mcf::BC_RSMX], gsmax = c[mcf::BC_GSMAX], rat = c[mcf::BC_RAT], psiw0 = c[mcf::BC_PSIW0];
    if (Rswabs > Rsmx) Rswabs = Rsmx;
    double gs = gsmax * pow(2.0, -(Rsmx - Rswabs) / (0.2 * Rsmx));
    const double thetan = rat * theta + (1 - rat) * kThetam;
    double Se = thetan / c[mcf::BC_SMAX];
    if (Se > 1.0) Se = 1.0;
    double psiw = -fabs(c[mcf::BC_PSIE]) * pow(Se, -c[mcf::BC_SOILB]) * 0.01;
    if (psiw < psiw0) psiw = psiw0;
    const double mu = 1.0 - (exp(-c[mcf::BC_KK] * psiw) - 1.0) / c[mcf::BC_MUDEN];
    const double gs2 = mu * gsmax;
    if (gs > gs2) gs = gs2;
    return gs;
}
__device__ double canopy_cond(const double* __restrict__ c, double Rsw, double Rdif, double k, double theta) {
    const double om = c[mcf::BC_OMC], PAI = c[mcf::BC_PAI];
    if (isnan(om)) return 9999.99;
    const double P_sun = (1.0 - exp(-k * PAI)) / k;
    const double P_shade = PAI - P_sun;
    const double Rshade = Rdif * c[mcf::BC_SHADEC] * (1.0 - om);
    const double Rsun = (Rsw - Rdif) * k * (1 - om) + Rshade;
    return stom_cond(c, Rsun, theta) * P_sun + stom_cond(c, Rshade, theta) * P_shade;
}
__device__ double penman(double Rabs, double gHa, double gV, double tc, double te, double pk, double ea, double em, double G,
                         double erh) {
    const double Rema = em * kSb * radem(tc);
    const double la = te >= 0 ? 45068.7 - 42.8428 * te : 51078.69 - 4.338 * te - 0.06367 * te * te;
    const double cp = cpair(te);
    const double Da = satvap(tc) - ea;
    const double gR = (4.0 * em * kSb * p3(te + 273.15)) / cp;
    const double De = satvap(te + 0.5) - satvap(te - 0.5);
    return tc + ((Rabs - Rema - la * (gV / pk) * Da * erh - G) / (cp * (gHa + gR) + la * (gV / pk) * De * erh));
}
// GFluxCpp's soil conductivity k and diffusivity kap of one hour
__device__ __forceinline__ void soil_k(const double* __restrict__ c, double sm, double& k, double& kap) {
    const double c1 = c[mcf::BC_C1], c4 = c[mcf::BC_C4], rho = c[mcf::BC_RHO];
    const double cs = c[mcf::BC_MU1] + 4180 * sm;
    const double ph = (rho * (1.0 - sm) + sm) * 1000;
    const double c2 = c[mcf::BC_MU2] * sm;
    k = c1 + c2 * sm - (c1 - c4) * exp(-p4(c[mcf::BC_C3] * sm));
    kap = k / (cs * ph);
}
__device__ __forceinline__ double soil_gmu(const double* __restrict__ c, double sm) {
    double k, kap;
    soil_k(c, sm, k, kap);
    const double DD = sqrt(2 * kap / kOmdy);
    return 1.4142135623730951 * (k / DD) * 0.5;      // sqrt(2)
}

// ---- what a block of points holds on the device ----------------------------------------------------------------------
struct BlDev {
    int64_t n, nd;                 // steps, days (n = 24 nd)
    int pb;                        // points in this block
    // inputs [pb][n]
    const double *tc, *rh, *pk, *Rsw, *Rdif, *Rlw, *ws, *soilm;
    // outputs / state [pb][n]
    double *Tc, *Tg, *H, *G, *psih, *psim, *phih, *OL, *uf, *RabsG, *albedo;
    // hoisted [pb][n]
    double *swG, *swC, *gC, *ea, *tdew, *srh, *Gmud;
    // work [pb][n]
    double *tcc, *tcg, *Gmin, *Gmax;
    // per point and day [pb][nd]
    double *Td, *Gmuy, *w1, *w2;
    const double* consts;          // [pb][BC_COUNT]
    const double* tconst;          // [n][TC_COUNT]
    unsigned long long* tst;       // [pb] bits of the iteration's max |dT|
    int* active;                   // [pb]
    int* iters;                    // [pb]
    double* err;                   // [pb]
    int* nactive;                  // [maxiter + 1] points that go on after iteration k
    double dTmx, bwgt, tol;
    int maxiter, yearG;
};

__global__ __launch_bounds__(kStepBlock) void k_bl_setup(BlDev D) {
    const int p = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (p >= D.pb || i >= D.n) return;
    const double* __restrict__ c = D.consts + (int64_t)p * mcf::BC_COUNT;
    const double* __restrict__ t = D.tconst + i * mcf::TC_COUNT;
    const int64_t q = (int64_t)p * D.n + i;
    const double* __restrict__ smrow = D.soilm + (int64_t)p * D.n;
    const double Rsw = D.Rsw[q], Rdif = D.Rdif[q], tc = D.tc[q], sm = smrow[i];
    const double pai = c[mcf::BC_PAI], gref = c[mcf::BC_GREF], lref = c[mcf::BC_LREF], x = c[mcf::BC_X];
    Sun sp = sun_position(c[mcf::BC_SINLAT], c[mcf::BC_COSLAT], c[mcf::BC_LON], t);
    // canopy conductance of the iteration body: canopy_k(zenr, x, cos zenr) with the UNCLAMPED zenith, then canopy_cond
    const Ext kb = canopy_k(sp.zenr, x, cos(sp.zenr));
    D.gC[q] = canopy_cond(c, Rsw, Rdif, kb.k, sm);
    // RadswabsCpp
    double radG = 0, radC = 0, alb;
    if (pai > 0.0) {
        alb = lref;
        if (Rsw > 0.0) {
            const double pait = c[mcf::BC_PAITSW], clump = c[mcf::BC_CLUMP], trd = c[mcf::BC_TRDSW], amx = c[mcf::BC_AMX],
                         emh = c[mcf::BC_EMH], eph = c[mcf::BC_EPH];
            const double si = solar_index(c + mcf::BC_SLOPE, sp.zend, sp.azid);
            if (sp.zenr > kPi / 2.0) sp.zenr = kPi / 2.0;
            const double cosz = cos(sp.zenr);
            const Ext kp = canopy_k(sp.zenr, x, si);
            const Dif f{c[mcf::BC_OM], c[mcf::BC_A], c[mcf::BC_GMA], c[mcf::BC_J], c[mcf::BC_DEL], c[mcf::BC_HH], c[mcf::BC_U1],
                        c[mcf::BC_S1], c[mcf::BC_D1], c[mcf::BC_D2], 0.0, 0.0};
            const Dir d = two_stream_dir(pait, f, gref, kp.kd);
            double Rbeam = (Rsw - Rdif) / cosz;
            if (Rbeam > 1352.0) Rbeam = 1352.0;
            double trb = pow(clump, kp.Kc);
            if (trb > 0.999) trb = 0.999;
            if (trb < 0.0) trb = 0.0;
            const double Rb = Rbeam * cosz;
            const double ekd = exp(-kp.kd * pait);
            const double trg = trb + (1 - trb) * ekd;
            const double Rbc = (trg * si + (1 - trg) * cosz) * Rbeam;
            double albb = trd * trb * gref + (1.0 - trd * trb) * (d.p5 / -d.sig + d.p6 + d.p7);
            if (albb > amx) albb = amx;
            if (albb < 0.01) albb = 0.01;
            double groundRbdd = trb + (1.0 - trb) * ((d.p8 / d.sig) * ekd + d.p9 * emh + d.p10 * eph);
            if (groundRbdd > amx) groundRbdd = amx;
            if (groundRbdd < 0.0) groundRbdd = 0.0;
            radC = (1.0 - c[mcf::BC_ALBD]) * Rdif + (1.0 - albb) * Rbc;
            const double Rgdif = c[mcf::BC_GRDD] * Rdif + groundRbdd * Rb;
            radG = (1.0 - gref) * (Rgdif + ekd * Rbeam * si);
            alb = 1.0 - (radC / (Rdif + Rb));
            if (alb > amx) alb = amx;
            if (alb < 0.01) alb = 0.01;
        }
    } else {
        alb = gref;
        if (Rsw > 0) {
            const double si = solar_index(c + mcf::BC_SLOPE, sp.zend, sp.azid);
            if (sp.zenr > kPi / 2.0) sp.zenr = kPi / 2.0;
            const double dirr = (Rsw - Rdif) / cos(sp.zenr);
            radG = (1 - gref) * (Rdif + si * dirr);
            radC = radG;
        }
    }
    D.swG[q] = radG; D.swC[q] = radC; D.albedo[q] = alb;
    const double ea = satvap(tc) * D.rh[q] / 100;
    D.ea[q] = ea;
    D.tdew[q] = dewpoint(ea);
    D.srh[q] = (sm - c[mcf::BC_SMIN]) / (c[mcf::BC_SMAX] - c[mcf::BC_SMIN]);
    // moving_mean(Gmu, 6): circular, the host's order of summation
    double sum = 0.0;
    for (int j = 0; j < 6; ++j) {
        int64_t idx = i - j;
        if (idx < 0) idx += D.n;
        sum += soil_gmu(c, smrow[idx]);
    }
    D.Gmud[q] = sum / 6;
    // initial state (mcf_bigleaf before its loop)
    D.Tg[q] = tc; D.Tc[q] = tc; D.tcc[q] = tc; D.tcg[q] = tc;
    D.psim[q] = 0; D.psih[q] = 0; D.phih[q] = 0; D.OL[q] = 0; D.G[q] = 0;
    D.uf[q] = 999.0; D.RabsG[q] = 999.0;
    D.H[q] = 0.5 * Rsw - c[mcf::BC_EM] * kSb * radem(tc);
    D.Gmin[q] = -999.0; D.Gmax[q] = 999.0;
}

// circular index (i - j + m) % m of maCpp in the host's int arithmetic (m >= 91 or m == 1 here)
__device__ __forceinline__ int circ(int i, int j, int m) { return (i - j + m) % m; }

// yearG: kma / kama = yearly_mean(k / kap) per day, Gmuy = sqrt(2) kma / sqrt(2 kama / omyr).  One workgroup per point.
__global__ __launch_bounds__(256) void k_bl_year_setup(BlDev D) {
    const int p = blockIdx.x;
    if (p >= D.pb) return;
    const double* __restrict__ c = D.consts + (int64_t)p * mcf::BC_COUNT;
    const double* __restrict__ sm = D.soilm + (int64_t)p * D.n;
    const int nd = (int)D.nd;
    double* dk = D.w1 + (int64_t)p * nd;
    double* dkap = D.w2 + (int64_t)p * nd;
    for (int d = threadIdx.x; d < nd; d += blockDim.x) {
        double sk = 0.0, ska = 0.0;
        for (int j = 0; j < 24; ++j) {
            double k, kap;
            soil_k(c, sm[(int64_t)d * 24 + j], k, kap);
            sk += k;
            ska += kap;
        }
        dk[d] = sk / 24.0;
        dkap[d] = ska / 24.0;
    }
    __syncthreads();
    const double omyr = (2 * kPi) / ((double)D.n * 3600.0);
    for (int d = threadIdx.x; d < nd; d += blockDim.x) {
        double sk = 0.0, ska = 0.0;
        for (int j = 0; j < 91; ++j) {
            const int idx = circ(d, j, nd);
            sk += dk[idx];
            ska += dkap[idx];
        }
        const double kma = sk / 91, kama = ska / 91;
        D.Gmuy[(int64_t)p * nd + d] = 1.4142135623730951 * kma / sqrt(2 * kama / omyr);
    }
}

// the body of mcf_bigleaf's hour loop
__global__ __launch_bounds__(kStepBlock) void k_bl_step(BlDev D) {
    const int p = blockIdx.y;
    if (!D.active[p]) return;                                  // the whole workgroup: a frozen point
    const int64_t i = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    double tst = 0;
    if (i < D.n) {
        const double* __restrict__ c = D.consts + (int64_t)p * mcf::BC_COUNT;
        const int64_t q = (int64_t)p * D.n + i;
        const double em = c[mcf::BC_EM], pai = c[mcf::BC_PAI], trd = c[mcf::BC_TRD], zrd = c[mcf::BC_ZREFD], d = c[mcf::BC_D];
        const double tc = D.tc[q], pk = D.pk[q], ea = D.ea[q], tdew = D.tdew[q], G = D.G[q];
        double Tc = D.Tc[q], Tg = D.Tg[q], H = D.H[q], psih = D.psih[q], psim = D.psim[q], tcc = D.tcc[q], tcg = D.tcg[q];
        const double RemC = em * kSb * radem(Tc);
        const double radClw = em * D.Rlw[q];
        const double radGlw = c[mcf::BC_GROUNDEM] * (trd * radClw + (1 - trd) * RemC);
        const double RabsG = D.swG[q] + radGlw;
        const double RabsC = D.swC[q] + radClw;
        const double zm = roughlength(c[mcf::BC_HMD], c[mcf::BC_HDE], psih);
        const double ln1 = log(zrd / zm);
        double uf = (kKa * D.ws[q]) / (ln1 + psim);
        if (uf < 0.0002) uf = 0.0002;
        const double gmin = g_free(c[mcf::BC_LEAFDD], fabs(H)) * 2 * pai;
        double ph = phair(tcc, pk);
        const double z0 = 0.2 * zm + d;                        // g_turb
        double gHa = (kKa * ph * uf) / (log(zrd / (z0 - d)) + psih);
        if (gHa < gmin) gHa = gmin;
        const double gC = D.gC[q];
        double gV = 1 / (1 / gHa + 1 / gC);
        if (gC == 0) gV = 0;
        double Tcn = penman(RabsC, gHa, gV, tc, tcc, pk, ea, em, G, 1);
        if (Tcn < tdew) Tcn = tdew;
        double Tgn = penman(RabsG, gHa, gHa, tcg, tcc, pk, ea, em, G, D.srh[q]);
        if (Tgn < tdew) Tgn = tdew;
        double dTc = Tcn - tc, dTg = Tgn - tc;
        if (dTc > D.dTmx) dTc = D.dTmx;
        if (dTg > D.dTmx) dTg = D.dTmx;
        Tcn = tc + dTc;
        Tgn = tc + dTg;
        const double tst2 = fabs(Tcn - Tc), tst3 = fabs(Tgn - Tg);
        if (tst2 > tst) tst = tst2;                            // a NaN difference never raises tst
        if (tst3 > tst) tst = tst3;
        Tc = D.bwgt * Tc + (1 - D.bwgt) * Tcn;
        Tg = D.bwgt * Tg + (1 - D.bwgt) * Tgn;
        tcc = (Tc + tc) / 2;
        tcg = (Tg + tc) / 2;
        const double Tk = 273.15 + tcc;
        ph = phair(tcc, pk);
        const double cp = cpair(tcc);
        H = D.bwgt * H + (1 - D.bwgt) * (gHa * cp * (Tcn - tc));
        const double Rnet = RabsC - kSb * em * radem(Tc);
        if (Rnet > 0 && H > Rnet) H = Rnet;
        if (fabs(H) < 0.1) H = 0.1;
        const double OL = (ph * cp * p3(uf) * Tk) / (-0.4 * 9.81 * H);
        psim = psi_m(zm / OL) - psi_m(zrd / OL);
        psih = psi_h((0.2 * zm) / OL) - psi_h(zrd / OL);
        const double ln2 = log(zrd / (0.2 * zm));
        if (psim < -0.9 * ln1) psim = -0.9 * ln1;
        if (psih < -0.9 * ln2) psih = -0.9 * ln2;
        if (psim > 0.9 * ln1) psim = 0.9 * ln1;
        if (psih > 0.9 * ln2) psih = 0.9 * ln2;
        if (psih > 0.9 * c[mcf::BC_BELIM]) psih = 0.9 * c[mcf::BC_BELIM];
        D.RabsG[q] = RabsG; D.uf[q] = uf; D.Tc[q] = Tc; D.Tg[q] = Tg; D.tcc[q] = tcc; D.tcg[q] = tcg; D.H[q] = H; D.OL[q] = OL;
        D.psim[q] = psim; D.psih[q] = psih; D.phih[q] = phi_h(zrd / OL);
    }
    // max over the point: non-negative doubles order like their bit patterns
    unsigned long long b = (unsigned long long)__double_as_longlong(tst);
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(b, off);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0 && b != 0) atomicMax(&D.tst[p], b);
}

// GFluxCpp without the annual term: a workgroup = kDaysPerGroup days of one point; the day before them (circular) is staged
// too, for the daily mean behind the 5-hour look-back of the first hours.
__global__ __launch_bounds__(kGroup) void k_bl_gflux(BlDev D, int iter0) {
    const int p = blockIdx.y;
    if (!D.active[p]) return;
    __shared__ double sT[kGroup + 24], sdT[kGroup + 24], sG[kGroup], sTd[kDaysPerGroup + 1];
    const int tid = threadIdx.x;
    const int64_t n = D.n, h0 = (int64_t)blockIdx.x * kGroup;
    const double* __restrict__ Tg = D.Tg + (int64_t)p * n;
    for (int k = tid; k < kGroup + 24; k += kGroup) {
        int64_t idx = h0 - 24 + k;
        if (idx < 0) idx += n;
        sT[k] = idx < n ? Tg[idx] : 0.0;
    }
    __syncthreads();
    if (tid <= kDaysPerGroup) {
        double s = 0.0;
        for (int j = 0; j < 24; ++j) s += sT[tid * 24 + j];
        s /= 24;
        sTd[tid] = s;
        const int64_t day = h0 / 24 + tid - 1;
        if (tid >= 1 && day < D.nd) D.Td[(int64_t)p * D.nd + day] = s;
    }
    __syncthreads();
    for (int k = tid; k < kGroup + 24; k += kGroup) sdT[k] = sT[k] - sTd[k / 24];
    __syncthreads();
    const int64_t i = h0 + tid;
    const bool valid = i < n;
    const int64_t q = (int64_t)p * n + i;
    double g = 0.0;
    if (valid) {
        double sum = 0.0;
        for (int j = 0; j < 6; ++j) sum += sdT[tid + 24 - j];
        g = sum / 6;
        g = g * D.Gmud[q] * 1.1171;
    }
    sG[tid] = g;
    __syncthreads();
    if (!valid) return;
    double gmin, gmax;
    if (iter0) {
        const int d0 = (tid / 24) * 24;
        gmin = sG[d0]; gmax = sG[d0];
        for (int j = 1; j < 24; ++j) {
            gmin = fmin(gmin, sG[d0 + j]);
            gmax = fmax(gmax, sG[d0 + j]);
        }
        D.Gmin[q] = gmin; D.Gmax[q] = gmax;
    } else {
        gmin = D.Gmin[q]; gmax = D.Gmax[q];
    }
    if (g < gmin) g = gmin;
    if (g > gmax) g = gmax;
    D.G[q] = g;
}

// GFluxCpp's annual term: G += yearly_mean(Td - sum(Td) / n) * Gmuy * 1.1171.  One workgroup per point; the sum over the
// series runs in the host's order (every daily mean 24 times, days in sequence) in one lane, so that it is the same for any
// batch, block size and position.
__global__ __launch_bounds__(256) void k_bl_annual(BlDev D) {
    const int p = blockIdx.x;
    if (!D.active[p]) return;
    __shared__ double s_mean;
    const int nd = (int)D.nd;
    const double* __restrict__ Td = D.Td + (int64_t)p * nd;
    double* dd = D.w1 + (int64_t)p * nd;
    double* y = D.w2 + (int64_t)p * nd;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int d = 0; d < nd; ++d) {
            const double v = Td[d];
            for (int j = 0; j < 24; ++j) s += v;
        }
        s_mean = s / (double)D.n;
    }
    __syncthreads();
    const double mean = s_mean;
    for (int d = threadIdx.x; d < nd; d += blockDim.x) {
        const double v = Td[d] - mean;
        double s = 0.0;
        for (int j = 0; j < 24; ++j) s += v;
        dd[d] = s / 24.0;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < nd; d += blockDim.x) {
        double s = 0.0;
        for (int j = 0; j < 91; ++j) s += dd[circ(d, j, nd)];
        y[d] = s / 91;
    }
    __syncthreads();
    double* G = D.G + (int64_t)p * D.n;
    const double* __restrict__ Gmuy = D.Gmuy + (int64_t)p * nd;
    for (int64_t i = threadIdx.x; i < D.n; i += blockDim.x) {
        const int64_t d = i / 24;
        G[i] = G[i] + y[d] * Gmuy[d] * 1.1171;
    }
}

// the end of an iteration, per point: mcf_bigleaf's `tstf = tst; ++iter; if (iter >= maxiter) tstf = 0; while (tstf > tol)`
__global__ __launch_bounds__(256) void k_bl_finish(BlDev D, int iter) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.pb || !D.active[p]) return;
    const double tst = __longlong_as_double((long long)D.tst[p]);
    const int it = D.iters[p] + 1;
    D.iters[p] = it;
    D.err[p] = tst;
    D.tst[p] = 0;
    if (tst > D.tol && it < D.maxiter) atomicAdd(&D.nactive[iter], 1);
    else D.active[p] = 0;
}

// weatherhgtCpp's element-wise tail (cpp:905-927) on the batched BigLeaf's Tc and psih
__global__ __launch_bounds__(kStepBlock) void k_weatherhgt_tail(int64_t total, const double* __restrict__ Tc,
                                                                  const double* __restrict__ psih, const double* __restrict__ wtemp,
                                                                  const double* __restrict__ wrh, const double* __restrict__ wws,
                                                                  double zin, double uzin, double zout, double d, double hmd,
                                                                  double hde, double* __restrict__ temp,
                                                                  double* __restrict__ relhum, double* __restrict__ windspeed) {
    const int64_t q = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (q >= total) return;
    const double zm = roughlength(hmd, hde, psih[q]);
    const double zh = 0.2 * zm;
    const double lnr = log((zout - d) / zh) / log((zin - d) / zh);
    const double t0 = wtemp[q], rh0 = wrh[q], tcq = Tc[q];
    const double tz = (tcq - t0) * (1 - lnr) + t0;
    const double ea = satvap(t0) * rh0 / 100;
    double es = satvap(tcq) * sqrt(rh0 / 100);
    const double ez = ea + (es - ea) * (1 - lnr);
    es = satvap(tz);
    double rh = (ez / es) * 100;
    if (rh < 0.25 * rh0) rh = 0.25 * rh0;
    if (rh > 100.0) rh = 100.0;
    const double lnru = log((zout - d) / zm) / log((uzin - d) / zm);
    temp[q] = tz;
    relhum[q] = rh;
    windspeed[q] = wws[q] * lnru;
}

// pointmprocess (cpp:5265-5323): element-wise, plus the day's max - min of T0p; a workgroup = kDaysPerGroup days of a point
struct PmpDev {
    int64_t n;
    const double *u2, *tc, *rh, *pk, *uf, *soilm, *RabsG;
    const double* consts;          // [pb][PC_COUNT]
    double *umu, *kp, *muGp, *DDp, *T0p, *dtrp;
};
__global__ __launch_bounds__(kGroup) void k_pointmprocess(PmpDev D) {
    __shared__ double sT[kGroup];
    const int p = blockIdx.y, tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kGroup + tid;
    const bool valid = i < D.n;
    const int64_t q = (int64_t)p * D.n + i;
    const double* __restrict__ c = D.consts + (int64_t)p * mcf::PC_COUNT;
    double T0 = 0.0;
    if (valid) {
        const double logz = c[mcf::PC_LOGZ], c1 = c[mcf::PC_C1], rho = c[mcf::PC_RHO], sm = D.soilm[q], tc = D.tc[q];
        const double ufps = (kKa * D.u2[q]) / logz;
        D.umu[q] = D.uf[q] / ufps;
        const double cs = (2400 * rho / 2.64 + 4180 * sm);
        const double ph = (rho * (1.0 - sm) + sm) * 1000;
        const double c2 = 1.06 * rho * sm;
        const double kp = c1 + c2 * sm - (c1 - c[mcf::PC_C4]) * exp(-p4(c[mcf::PC_C3] * sm));
        D.kp[q] = kp;
        const double kap = kp / (cs * ph);
        const double dd = sqrt(2.0 * kap / kOmdy);
        D.muGp[q] = dd;
        D.DDp[q] = dd;
        const double gHa = (0.4 * 43.0 * ufps) / logz;
        const double ea = satvap(tc) * D.rh[q] / 100.0;
        T0 = penman(D.RabsG[q], gHa, gHa, tc, tc, D.pk[q], ea, 0.97, 0.0, 1.0);
        D.T0p[q] = T0;
    }
    sT[tid] = T0;
    __syncthreads();
    if (!valid) return;
    const int d0 = (tid / 24) * 24;
    double mx = sT[d0], mn = sT[d0];
    for (int j = 1; j < 24; ++j) {
        mx = fmax(mx, sT[d0 + j]);
        mn = fmin(mn, sT[d0 + j]);
    }
    D.dtrp[q] = mx - mn;
}

// =====================================================================================================================
// pointmodelsnow (cpp:4000-4169) for many points: mcf_pointmodelsnow_batch.  Unlike BigLeafCpp, the hours of a pass are NOT
// independent: the pack (two depths, two ages) is carried from step to step and feeds back into the canopy above it (pai and
// hgt shrink with the ground pack; the two-stream solution, the roughness and the turbulent conductance follow).  Points are
// independent, and much of a step does not depend on the pack.  So: one lane per point marching through time, and
// everything else one lane per (point, hour) or (point, day).
//
//   k_ps_transpose    between the caller's [P][n] and the tables' [n][points]: the sweep's 64 lanes then touch whole lines
//   k_ps_setup        once, per (point, hour): what a step needs that does not depend on the pack (ea, tdew, cpair, phair, the
//                     sun, the capped beam, RswabsC and RabsC, canopy_k, exp(tc / 2.59), the rain melt), the initial state
//   k_ps_sweep        per pass, per point, serial over the steps, the pack in registers; ONE wave per workgroup, so that the
//                     waves of a batch spread over the CUs and each has a SIMD to itself (the kernel is a chain of dependent
//                     fp64 operations and nothing runs beside it)
//   k_ps_gflux        per pass, per (point, day): GFluxCppsnow — the day's mean, the 6-hour circular trailing mean of T - Td
//                     (it wraps round the series end), times Gmud 1.1171; the host's order of summation
//   k_ps_finish       per pass: convergence PER POINT, counts the points that go on
//
// The density of the pack never changes during a run: the reference keeps sdenc[i] at its initial value, and so does
// mcf_pointmodelsnow.  Gmu is then one number per point and comes, with its 6-hour mean, from the host (PS_GMUD).  The albedo
// is a serial hour counter with an integer division: host work too (mcf::ps_albedo), uploaded.
// =====================================================================================================================
struct PsDev {
    int64_t n, nd, ps;             // steps, days, the tables' row length (points of a block rounded up to whole waves)
    int pb;                        // points in this block
    // tables [n][ps], the point fastest.  inputs (ea arrives as relhum):
    double *tc, *ea, *pk, *u2, *prec, *Rsw, *Rdif, *Rlw, *alb;
    // hoisted by k_ps_setup
    double *tdew, *cp, *ph, *RabsC, *RswabsC, *cosz, *Rbeam, *kd, *Kc, *erhos, *mRc;
    // state of the relaxation
    double *Tc, *Tg, *te, *psim, *psih, *G;
    // results of the last pass
    double *RswabsG, *RlwabsG, *tr, *umu, *mSc, *mMc, *Tcp;
    double *sdepc, *sdepg;         // [n + 1][ps]
    const double* consts;          // [pb][PS_COUNT]
    const double* tconst;          // [n][TC_COUNT]
    double* mxd;                   // [ps] the pass's max |dT|
    double* mxdif;                 // [ps] ... of the point's last pass
    int* active;                   // [ps]
    int* iters;                    // [ps]
    int* going;                    // points that go on after this pass
    double tol, maxiter;
};

// dst[c * ldd + r] = src[r * lds + c] for r < rows, c < cols
__global__ __launch_bounds__(256) void k_ps_transpose(const double* __restrict__ src, int64_t rows, int64_t cols, int64_t lds,
                                                      double* __restrict__ dst, int64_t ldd) {
    __shared__ double tile[32][33];
    const int64_t tx = (cols + 31) / 32;
    const int64_t by = (int64_t)blockIdx.x / tx, bx = (int64_t)blockIdx.x - by * tx;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (int k = ly; k < 32; k += 8) {
        const int64_t r = by * 32 + k, c = bx * 32 + lx;
        if (r < rows && c < cols) tile[k][lx] = src[r * lds + c];
    }
    __syncthreads();
    for (int k = ly; k < 32; k += 8) {
        const int64_t c = bx * 32 + k, r = by * 32 + lx;
        if (r < rows && c < cols) dst[c * ldd + r] = tile[lx][k];
    }
}

__global__ __launch_bounds__(kStepBlock) void k_ps_setup(PsDev D) {
    const int64_t q = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (q >= D.n * D.ps) return;
    const int64_t i = q / D.ps;
    const int p = (int)(q - i * D.ps);
    if (p >= D.pb) return;
    const double* __restrict__ c = D.consts + (int64_t)p * mcf::PS_COUNT;
    const double* __restrict__ t = D.tconst + i * mcf::TC_COUNT;
    const double tc = D.tc[q], pk = D.pk[q], Rsw = D.Rsw[q], Rdif = D.Rdif[q], alb = D.alb[q], prec = D.prec[q];
    const double ea = satvap(tc) * D.ea[q] / 100.0;
    D.ea[q] = ea;
    D.tdew[q] = dewpoint(ea);
    D.cp[q] = cpair(tc);
    D.ph[q] = phair(tc, pk);
    // snow_radiation without the pack: the canopy's own absorption, the beam, the extinction of a spherical canopy
    const double RlwabsC = 0.97 * D.Rlw[q];
    double RabsC = RlwabsC, RswabsC = 0.0, cosz = 0.0, Rbeam = 0.0, kd = 0.0, Kc = 0.0;
    if (Rsw > 0.0) {
        const Sun sp = sun_position(c[mcf::PS_SINLAT], c[mcf::PS_COSLAT], c[mcf::PS_LON], t);
        double si = solar_index(c + mcf::PS_SLOPE, sp.zend, sp.azid);
        if (si < 0.0) si = 0.0;
        cosz = cos(sp.zenr);
        Rbeam = (Rsw - Rdif) / cosz;
        if (Rbeam > 1352.2) Rbeam = 1352.2;
        RswabsC = (1.0 - alb) * (Rdif + Rbeam * cosz);
        RabsC = RswabsC + RlwabsC;
        const Ext kp = canopy_k(sp.zenr, 1.0, si);
        kd = kp.kd; Kc = kp.Kc;
    }
    D.RabsC[q] = RabsC; D.RswabsC[q] = RswabsC; D.cosz[q] = cosz; D.Rbeam[q] = Rbeam; D.kd[q] = kd; D.Kc[q] = Kc;
    D.erhos[q] = exp(tc / 2.59);
    D.mRc[q] = tc > 0.0 ? 0.0125 * tc * prec / 1000 : 0.0;
    // mcf_pointmodelsnow before its loop
    D.Tc[q] = tc; D.Tg[q] = tc; D.te[q] = tc; D.psim[q] = 0.0; D.psih[q] = 0.0;
}

__device__ __forceinline__ double zeroplane(double h, double pai) {
    if (pai < 0.001) pai = 0.001;
    return (1.0 - (1.0 - exp(-sqrt(7.5 * pai))) / sqrt(7.5 * pai)) * h;
}
// roughlength(h, pai, d, psi_h) of the host: roughlength() above with its two factors formed here
__device__ __forceinline__ double roughlength_canopy(double h, double pai, double d, double psi_h) {
    const double Be = sqrt(0.003 + (0.2 * pai) / 2);
    return roughlength(h - d, (h - d) * exp(-kKa / Be), psi_h);
}
__device__ __forceinline__ double latent_molar(double t) {
    return t < 0.0 ? 51078.69 - 4.338 * t - 0.06367 * t * t : 45068.7 - 42.8428 * t;
}
__device__ __forceinline__ double clamp01(double v) { return v > 1.0 ? 1.0 : v < 0.0 ? 0.0 : v; }
// canopysnowintCpp with exp(tc / 2.59) from the set-up
__device__ double canopy_snow_interception(double hgt, double pai, double uf, double prec, double erhos, double Li) {
    if (hgt < 0.001) hgt = 0.001;
    if (pai < 0.001) pai = 0.001;
    const double Be = sqrt(0.003 + (0.2 * pai) / 2.0), uh = uf / Be;
    const double Lc = 1.0 / (0.25 * (pai / hgt)), Lm = 2.0 * p3(Be) * Lc, k1 = Be / Lm;
    double uzm = (uh / (hgt * k1)) * (1 - exp(-k1 * hgt));
    if (uzm < uf) uzm = uf;
    const double rhos = 67.92 + 51.25 * erhos;
    const double Lstr = 6.2 * (0.26 + 46 / rhos) * pai;
    const double kc = 1.0 / (2.0 * cos(atan(uzm / 0.8)));
    const double Cp = 1.0 - exp(-kc * pai);
    const double cis = (Lstr - Li) * (1.0 - exp(-(Cp / Lstr) * prec)) * 0.678;
    return cis > prec ? prec : cis;
}
__device__ __forceinline__ double snow_density(double a, double b, double c, double d, double depth, double age_hours) {
    return ((a - b) * (1.0 - exp(-c * depth / 100.0 - d * age_hours / 24.0)) + b) * 1000.0;
}

// a pass of mcf_pointmodelsnow's loop for one point per lane: snow_step (with snow_radiation) and the stability update
__global__ __launch_bounds__(64) void k_ps_sweep(PsDev D) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= D.pb || !D.active[p]) return;                     // a frozen point does no work
    const double* __restrict__ c = D.consts + (int64_t)p * mcf::PS_COUNT;
    const double pai0 = c[mcf::PS_PAI], hgt0 = c[mcf::PS_HGT], ltra0 = c[mcf::PS_LTRA], clump = c[mcf::PS_CLUMP],
                 zref = c[mcf::PS_ZREF], da = c[mcf::PS_DENA], db = c[mcf::PS_DENB], dc = c[mcf::PS_DENC], dd = c[mcf::PS_DEND],
                 sden = c[mcf::PS_SDEN0];
    const double cld = clump * clump;
    double sdepc = c[mcf::PS_ISNOWD], sdepg = c[mcf::PS_ISNOWD] * 0.5, agec = c[mcf::PS_ISNOWA], ageg = c[mcf::PS_ISNOWA];
    D.sdepc[p] = sdepc;
    D.sdepg[p] = sdepg;
    double mxdif = 0.0;
    int64_t q = p;
    for (int64_t i = 0; i < D.n; ++i, q += D.ps) {
        const double tc = D.tc[q], ea = D.ea[q], pk = D.pk[q], u2 = D.u2[q], prec = D.prec[q], Rsw = D.Rsw[q], Rdif = D.Rdif[q],
                     Rlw = D.Rlw[q], alb = D.alb[q], te = D.te[q], G = D.G[q], Tco = D.Tc[q], Tgo = D.Tg[q], psim0 = D.psim[q],
                     psih0 = D.psih[q];
        // ---- snow_step: the canopy above the pack
        const double pai = hgt0 > sdepg ? pai0 * (hgt0 - sdepg) / hgt0 : 0.0;
        double hgt = hgt0 - sdepg;
        if (hgt < 0.0) hgt = 0.0;
        const double zi = (sdepg > 0.0 && hgt > 0.0) ? ((sdepc - sdepg) * sden) / (hgt * 1000.0) : 0.0;
        double ltra = ltra0 * exp(-10.1 * zi);
        // ---- snow_radiation: what depends on the pack
        const double RlwabsC = 0.97 * Rlw, pait = pai / (1.0 - clump);
        double RlwabsG = RlwabsC;
        const double tr = (1.0 - cld) * exp(-pait) + cld;
        if (hgt > 0.0) RlwabsG = 0.97 * (tr * Rlw + (1.0 - tr) * 0.97 * kSb * radem(Tco));
        const double RabsC = D.RabsC[q];
        double RswabsG = 0.0;
        if (Rsw > 0.0) {
            RswabsG = D.RswabsC[q];
            if (hgt > 0.0) {
                const double cosz = D.cosz[q], Rbeam = D.Rbeam[q], kd = D.kd[q];
                if (alb + ltra > 0.999) ltra = 0.999 - alb;
                const Dif f = two_stream_dif(pait, 1.0, alb, ltra, alb);
                const Dir r = two_stream_dir(pait, f, alb, kd);
                const double clb = pow(clump, D.Kc[q]);
                const double emh = f.S1, eph = exp(f.h * pait), ekd = exp(-kd * pait);
                const double Rddm = clamp01((1.0 - cld) * (f.p3 * emh + f.p4 * eph) + cld);
                const double Rdbm = clamp01((1.0 - clb) * ((r.p8 / r.sig) * ekd + r.p9 * emh + r.p10 * eph));
                const double Rbgm = clamp01((1.0 - clb) * ekd + clb);
                RswabsG = (1.0 - alb) * (Rdbm * Rbeam * cosz) + Rddm * Rdif + (1.0 - alb) * (Rbgm * Rbeam * 0.5);
            }
        }
        // ---- roughness, friction velocity, conductance, the two temperatures
        double d = 0.0, zmr = 0.005;
        if (hgt > 0.0) { d = zeroplane(hgt, pai); zmr = roughlength_canopy(hgt, pai, d, psih0); }
        const double zm = zmr < 0.0009 ? 0.0009 : zmr;
        const double uf = (kKa * u2) / (log((zref - d) / zm) + psim0);
        const double ph = D.ph[q];
        double gHa = (kKa * ph * uf) / (log((zref - d) / ((0.2 * zm + d) - d)) + psih0);     // g_turb, gmin = 0.03
        if (gHa < 0.03) gHa = 0.03;
        double Tc = penman(RabsC, gHa, gHa, tc, te, pk, ea, 0.97, G, 1.0);
        double Tg = penman(RswabsG + RlwabsG, gHa, gHa, tc, te, pk, ea, 0.97, G, 1.0);
        const double tdew = D.tdew[q];
        if (Tc < tdew) Tc = tdew;
        if (Tg < tdew) Tg = tdew;
        // ---- the whole pack: sublimation, temperature melt, rain melt; then the ground pack
        double la = latent_molar(Tc);
        const double mSc = ((la * (gHa / pk) * (satvap(Tc) - ea)) / (la / 0.018015)) * 3.6;
        const double Tcp = Tc;
        double mMc = 0.0;
        if (Tc > 0.0) {
            mMc = ((583.3 * Tc * (sdepc * (sden / 1000))) / 334000.0) * 3.6;
            if (sdepc > 0.0) Tc = 0.0;
        }
        const double mRc = D.mRc[q];
        la = latent_molar(Tg);
        double mu = exp(-pai);
        if (mu > 1.0) mu = 1.0;
        const double mSg = ((la * (gHa / pk) * (satvap(Tg) - ea) * mu) / (la / 0.018015)) * 3.6;
        double mMg = 0.0;
        if (Tg > 0.0) {
            mMg = ((583.3 * Tg * (sdepg * (sden / 1000.0))) / 334000.0) * 3.6;
            if (sdepg > 0.0) Tg = 0.0;
        }
        double Li = 0.0;
        if (sdepc > 0.0) {
            double wg = sdepg / sdepc;
            wg = wg < 0.0 ? 0.0 : wg > 1.0 ? 1.0 : wg;
            Li = (sdepc - sdepg) * (wg * sden + (1.0 - wg) * sden);
        }
        if (Li < 0.0) Li = 0.0;
        double cis = canopy_snow_interception(hgt, pai, uf, prec, D.erhos[q], Li);
        if (cis > prec) cis = prec;
        const double mRg = tc > 0.0 ? 0.0125 * tc * (prec - cis) / 1000.0 : 0.0;
        const double snowc = tc > 2.0 ? 0.0 : prec, snowg = tc > 2.0 ? 0.0 : prec - cis;
        const double swec = snowc / 1000.0 - mSc - mMc - mRc, sweg = snowg / 1000.0 - mSg - mMg - mRg;
        agec = agec + 1.0;
        ageg = ageg + 1.0;
        const double denc = snow_density(da, db, dc, dd, sdepc, agec), deng = snow_density(da, db, dc, dd, sdepg, ageg);
        sdepc = sdepc + (swec * 1000.0) / denc;
        sdepg = sdepg + (sweg * 1000.0) / deng;
        if (sdepc < 0.0) { sdepc = 0.0; agec = 0.0; }
        if (sdepg < 0.0) { sdepg = 0.0; ageg = 0.0; }
        D.sdepc[q + D.ps] = sdepc;
        D.sdepg[q + D.ps] = sdepg;
        // ---- mcf_pointmodelsnow's loop body after snow_step: relaxation, then the stability of the surface layer
        const double Tcn = 0.5 * Tco + 0.5 * Tc, Tgn = 0.5 * Tgo + 0.5 * Tg;
        mxdif = fmax(mxdif, fmax(fabs(Tcn - Tco), fabs(Tgn - Tgo)));          // fmax: a NaN never becomes the maximum
        const double cp = D.cp[q];
        double H = cp * gHa * (Tcn - tc);
        double zm2 = hgt > 0.0 ? zmr : roughlength_canopy(hgt, pai, zeroplane(hgt, pai), psih0);
        if (zm2 < 0.001) zm2 = 0.001;
        if (fabs(H) < 0.1) H = 0.1;
        const double LL = (ph * cp * p3(uf) * (tc + 273.15)) / (-kKa * 9.81 * H);
        double psim = psi_m(zm2 / LL) - psi_m((zref - d) / LL);
        double psih = psi_h((0.2 * zm2) / LL) - psi_h((zref - d) / LL);
        const double Belim = 0.4 / sqrt(0.003 + (0.2 * pai) / 2.0);
        const double ln1 = log((zref - d) / zm2), ln2 = log((zref - d) / (0.2 * zm2));
        if (psim < -0.9 * ln1) psim = -0.9 * ln1;
        if (psih < -0.9 * ln2) psih = -0.9 * ln2;
        if (psim > 0.9 * ln1) psim = 0.9 * ln1;
        if (psih > 0.9 * ln2) psih = 0.9 * ln2;
        if (psih > 0.9 * Belim) psih = 0.9 * Belim;
        D.Tc[q] = Tcn; D.Tg[q] = Tgn; D.psim[q] = psim; D.psih[q] = psih; D.te[q] = (Tcn + tc) / 2.0;
        D.RswabsG[q] = RswabsG; D.RlwabsG[q] = RlwabsG; D.tr[q] = tr;
        D.umu[q] = uf / ((0.4 * u2) / ln1);
        D.mSc[q] = mSc; D.mMc[q] = mMc; D.Tcp[q] = Tcp;
    }
    D.mxd[p] = mxdif;
}

// GFluxCppsnow on series `Ts` (the air temperature before the first pass, Tg after each): a lane = one day of one point; the
// last five hours of the day before (circular) come with their own daily mean
__global__ __launch_bounds__(kStepBlock) void k_ps_gflux(PsDev D, const double* __restrict__ Ts, int all) {
    const int64_t q = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (q >= D.nd * D.ps) return;
    const int64_t day = q / D.ps;
    const int p = (int)(q - day * D.ps);
    if (p >= D.pb || !(all || D.active[p])) return;
    const int64_t before = day == 0 ? D.nd - 1 : day - 1;
    const double* __restrict__ a = Ts + before * 24 * D.ps + p;
    const double* __restrict__ b = Ts + day * 24 * D.ps + p;
    double v[29], sa = 0.0, sb = 0.0;
#pragma unroll
    for (int j = 0; j < 24; ++j) {
        const double x = a[j * D.ps];
        sa += x;
        if (j >= 19) v[j - 19] = x;
    }
#pragma unroll
    for (int j = 0; j < 24; ++j) {
        v[5 + j] = b[j * D.ps];
        sb += v[5 + j];
    }
    sa /= 24;
    sb /= 24;
#pragma unroll
    for (int j = 0; j < 29; ++j) v[j] = v[j] - (j < 5 ? sa : sb);
    const double gmud = D.consts[(int64_t)p * mcf::PS_COUNT + mcf::PS_GMUD];
    double* __restrict__ G = D.G + day * 24 * D.ps + p;
#pragma unroll
    for (int h = 0; h < 24; ++h) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) sum += v[5 + h - j];
        G[h * D.ps] = (sum / 6) * gmud * 1.1171;
    }
}

// the end of a pass, per point: `tst = mxdif; if (++iter > maxiter) tst = 0; while (tst > tol)`
__global__ __launch_bounds__(256) void k_ps_finish(PsDev D) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.pb || !D.active[p]) return;
    const double mx = D.mxd[p];
    const int it = D.iters[p] + 1;
    D.iters[p] = it;
    D.mxdif[p] = mx;
    double tst = mx;
    if ((double)it > D.maxiter) tst = 0;
    if (tst > D.tol) atomicAdd(D.going, 1);
    else D.active[p] = 0;
}

// ---- host side --------------------------------------------------------------------------------------------------------
bool weather_ok(const mcf_point_weather* w) {
    return w && w->temp && w->relhum && w->pres && w->swdown && w->difrad && w->lwdown && w->windspeed;
}
bool obstime_ok(const mcf_obstime* t) { return t && t->year && t->month && t->day && t->hour; }

// the refusals every batch entry shares; nothing here touches the device
int check_batch(const char* who, int64_t P, int64_t n) {
    const std::string w(who);
    if (P < 1) return mcf::api_fail(MCF_ERR_ARG, w + ": P < 1: the batch needs at least one point");
    if (n < 6) return mcf::api_fail(MCF_ERR_ARG, w + ": n < 6: the 6-hour running mean of GFluxCpp needs at least 6 steps");
    if (n % 24 != 0) return mcf::api_fail(MCF_ERR_ARG, w + ": n % 24 != 0: the batch entries take whole days only");
    if (n > (1 << 28) || P > ((int64_t)1 << 40) / n) return mcf::api_fail(MCF_ERR_ARG, w + ": series too long");
    return MCF_OK;
}

// points per block: what `series` arrays of n doubles per point leave of the free memory (80 %), at most `limit`
int block_points(int64_t P, int64_t n, int series, int64_t asked, int64_t* out) {
    constexpr int64_t kMaxGridY = 65535;
    int64_t pb = asked;
    if (pb <= 0) {
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        const double per_point = (double)series * 8.0 * (double)n + 4096.0;
        pb = (int64_t)(0.8 * (double)fr / per_point);
        if (pb < 1) return mcf::api_fail(MCF_ERR_NOMEM, "point batch: one point's series do not fit the free device memory");
    }
    *out = std::min(std::min(pb, P), kMaxGridY);
    return MCF_OK;
}

struct BlJob {
    int64_t P, n;
    const mcf_obstime* t;
    const mcf_point_weather* w;
    const double *vegp, *groundp;      // [P][10] / [P][12], or one row for every point (shared_params)
    bool shared_params;
    const double* soilm;               // [P][n]; null: 0.2 everywhere (weatherhgtCpp)
    const double *lat, *lon;
    double dTmx, zref;
    int maxiter;
    double bwgt, tol;
    int yearG;
    int64_t ppb;
    int device;
    mcf_bigleaf_batch_out* out;        // BigLeaf's own outputs, or
    double zin, uzin, zout, *wtemp, *wrh, *wws;   // weatherhgtCpp's
};

int run_bigleaf(const BlJob& J) {
    if (const int rc = mcf::check_device(J.device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(J.device));
    const int64_t n = J.n, nd = n / 24;
    int64_t PB;
    if (const int rc = block_points(J.P, n, 32, J.ppb, &PB)) return rc;
    const int64_t S = PB * n;
    mcf::DevOwner own;
    int rc;
    double* series[30];
    for (auto& s : series)
        if ((rc = own.make(&s, S))) return rc;
    double *in[8], *st[22];
    for (int k = 0; k < 8; ++k) in[k] = series[k];
    for (int k = 0; k < 22; ++k) st[k] = series[8 + k];
    double *dTd, *dGmuy, *dw1, *dw2, *dconst, *dtconst, *derr;
    unsigned long long* dtst;
    int *dactive, *diters, *dnactive;
    const int nit = std::max(J.maxiter, 1) + 1;
    if ((rc = own.make(&dTd, PB * nd)) || (rc = own.make(&dGmuy, PB * nd)) || (rc = own.make(&dw1, PB * nd)) ||
        (rc = own.make(&dw2, PB * nd)) || (rc = own.make(&dconst, PB * mcf::BC_COUNT)) ||
        (rc = own.make(&dtconst, n * mcf::TC_COUNT)) || (rc = own.make(&derr, PB)) || (rc = own.make(&dtst, PB)) ||
        (rc = own.make(&dactive, PB)) || (rc = own.make(&diters, PB)) || (rc = own.make(&dnactive, (int64_t)nit)))
        return rc;
    {
        std::vector<double> tcv((size_t)n * mcf::TC_COUNT);
        mcf::bl_time_consts(n, J.t->year, J.t->month, J.t->day, J.t->hour, tcv.data());
        HIP_TRY(hipMemcpy(dtconst, tcv.data(), tcv.size() * 8, hipMemcpyHostToDevice));
    }
    std::vector<double> hconst((size_t)PB * mcf::BC_COUNT), fill;
    std::vector<int> ones((size_t)PB, 1);
    const double* cols[7] = {J.w->temp, J.w->relhum, J.w->pres, J.w->swdown, J.w->difrad, J.w->lwdown, J.w->windspeed};
    const bool enter = J.tol * 2 > J.tol;                     // the host loop's `tstf = tol * 2; while (tstf > tol)`
    const double whd = mcf::wh_zeroplane(), whhde = mcf::wh_hde();

    for (int64_t p0 = 0; p0 < J.P; p0 += PB) {
        const int64_t pb = std::min(PB, J.P - p0);
        const size_t bytes = (size_t)(pb * n) * 8;
        for (int k = 0; k < 7; ++k) HIP_TRY(hipMemcpy(in[k], cols[k] + p0 * n, bytes, hipMemcpyHostToDevice));
        if (J.soilm) {
            HIP_TRY(hipMemcpy(in[7], J.soilm + p0 * n, bytes, hipMemcpyHostToDevice));
        } else if (p0 == 0) {
            fill.assign((size_t)S, 0.2);
            HIP_TRY(hipMemcpy(in[7], fill.data(), (size_t)S * 8, hipMemcpyHostToDevice));
        }
        for (int64_t p = 0; p < pb; ++p) {
            const int64_t g = p0 + p;
            mcf::bl_point_consts(J.vegp + (J.shared_params ? 0 : g * 10), J.groundp + (J.shared_params ? 0 : g * 12), J.lat[g],
                                 J.lon[g], J.zref, hconst.data() + p * mcf::BC_COUNT);
        }
        HIP_TRY(hipMemcpy(dconst, hconst.data(), (size_t)pb * mcf::BC_COUNT * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dactive, ones.data(), (size_t)pb * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(diters, 0, (size_t)pb * 4));
        HIP_TRY(hipMemset(derr, 0, (size_t)pb * 8));
        HIP_TRY(hipMemset(dtst, 0, (size_t)pb * 8));
        HIP_TRY(hipMemset(dnactive, 0, (size_t)nit * 4));

        BlDev D;
        D.n = n; D.nd = nd; D.pb = (int)pb;
        D.tc = in[0]; D.rh = in[1]; D.pk = in[2]; D.Rsw = in[3]; D.Rdif = in[4]; D.Rlw = in[5]; D.ws = in[6]; D.soilm = in[7];
        D.Tc = st[0]; D.Tg = st[1]; D.H = st[2]; D.G = st[3]; D.psih = st[4]; D.psim = st[5]; D.phih = st[6]; D.OL = st[7];
        D.uf = st[8]; D.RabsG = st[9]; D.albedo = st[10];
        D.swG = st[11]; D.swC = st[12]; D.gC = st[13]; D.ea = st[14]; D.tdew = st[15]; D.srh = st[16]; D.Gmud = st[17];
        D.tcc = st[18]; D.tcg = st[19]; D.Gmin = st[20]; D.Gmax = st[21];
        D.Td = dTd; D.Gmuy = dGmuy; D.w1 = dw1; D.w2 = dw2; D.consts = dconst; D.tconst = dtconst;
        D.tst = dtst; D.active = dactive; D.iters = diters; D.err = derr; D.nactive = dnactive;
        D.dTmx = J.dTmx; D.bwgt = J.bwgt; D.tol = J.tol; D.maxiter = J.maxiter; D.yearG = J.yearG;

        const dim3 gstep((unsigned)((n + kStepBlock - 1) / kStepBlock), (unsigned)pb);
        const dim3 gday((unsigned)((nd + kDaysPerGroup - 1) / kDaysPerGroup), (unsigned)pb);
        const unsigned gpoint = (unsigned)((pb + 255) / 256);
        hipLaunchKernelGGL(k_bl_setup, gstep, dim3(kStepBlock), 0, 0, D);
        if (J.yearG) hipLaunchKernelGGL(k_bl_year_setup, dim3((unsigned)pb), dim3(256), 0, 0, D);
        HIP_TRY(hipGetLastError());
        for (int iter = 0; enter; ++iter) {
            hipLaunchKernelGGL(k_bl_step, gstep, dim3(kStepBlock), 0, 0, D);
            hipLaunchKernelGGL(k_bl_gflux, gday, dim3(kGroup), 0, 0, D, iter == 0 ? 1 : 0);
            if (J.yearG) hipLaunchKernelGGL(k_bl_annual, dim3((unsigned)pb), dim3(256), 0, 0, D);
            hipLaunchKernelGGL(k_bl_finish, dim3(gpoint), dim3(256), 0, 0, D, iter);
            HIP_TRY(hipGetLastError());
            int going = 0;                                    // the one small copy of an iteration; it also reports a fault
            HIP_TRY(hipMemcpy(&going, dnactive + iter, 4, hipMemcpyDeviceToHost));
            if (going == 0 || iter + 1 >= nit - 1) break;
        }
        if (J.out) {
            double* host[11] = {J.out->Tc, J.out->Tg, J.out->H, J.out->G, J.out->psih, J.out->psim, J.out->phih, J.out->OL,
                                J.out->uf, J.out->RabsG, J.out->albedo};
            for (int k = 0; k < 11; ++k) HIP_TRY(hipMemcpy(host[k] + p0 * n, st[k], bytes, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(J.out->err + p0, derr, (size_t)pb * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(J.out->iters + p0, diters, (size_t)pb * 4, hipMemcpyDeviceToHost));
        } else {
            // swG / swC / gC are free now: the three results go there
            const int64_t total = pb * n;
            hipLaunchKernelGGL(k_weatherhgt_tail, dim3((unsigned)((total + kStepBlock - 1) / kStepBlock)), dim3(kStepBlock), 0, 0,
                               total, D.Tc, D.psih, D.tc, D.rh, D.ws, J.zin, J.uzin, J.zout, whd, 0.12 - whd, whhde, D.swG, D.swC,
                               D.gC);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(J.wtemp + p0 * n, D.swG, bytes, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(J.wrh + p0 * n, D.swC, bytes, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(J.wws + p0 * n, D.gC, bytes, hipMemcpyDeviceToHost));
        }
    }
    return MCF_OK;
}

// ---- mcf_pointmodelsnow_batch: the host side ---------------------------------------------------------------------------
constexpr int kPsTables = 35;      // tables of a block, the two [n + 1] depths last; with the staging buffer 36 series

struct PsJob {
    int64_t P, n;
    const mcf_obstime* t;
    const mcf_point_weather* w;
    const double *vegp, *other;        // [P][4] / [P][7]
    const int32_t* snowenv;            // [P]
    double tol, maxiter;
    int64_t ppb;
    int device;
    mcf_pointsnow_batch_out* out;
};

int ps_transpose(const double* src, int64_t rows, int64_t cols, int64_t lds, double* dst, int64_t ldd) {
    const int64_t tiles = ((rows + 31) / 32) * ((cols + 31) / 32);
    hipLaunchKernelGGL(k_ps_transpose, dim3((unsigned)tiles), dim3(256), 0, 0, src, rows, cols, lds, dst, ldd);
    HIP_TRY(hipGetLastError());
    return MCF_OK;
}

int run_pointsnow(const PsJob& J) {
    if (const int rc = mcf::check_device(J.device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(J.device));
    const int64_t n = J.n, nd = n / 24;
    int64_t PB;
    if (const int rc = block_points(J.P, n, 45, J.ppb, &PB)) return rc;
    const int64_t PS = (PB + 63) / 64 * 64;                  // whole waves: the sweep's lanes read whole lines
    if ((n + 1) * PS >= ((int64_t)1 << 32))                  // one lane per table element must fit a launch
        return mcf::api_fail(MCF_ERR_NOMEM, "mcf_pointmodelsnow_batch: points_per_block x n does not fit one launch");
    mcf::DevOwner own;
    int rc;
    double* tab[kPsTables];
    for (int k = 0; k < kPsTables; ++k)
        if ((rc = own.make(&tab[k], (k >= kPsTables - 2 ? n + 1 : n) * PS))) return rc;
    double *stage, *dconst, *dtconst, *dmxd, *dmxdif;
    int *dactive, *diters, *dgoing;
    if ((rc = own.make(&stage, PB * (n + 1))) || (rc = own.make(&dconst, PB * mcf::PS_COUNT)) ||
        (rc = own.make(&dtconst, n * mcf::TC_COUNT)) || (rc = own.make(&dmxd, PS)) || (rc = own.make(&dmxdif, PS)) ||
        (rc = own.make(&dactive, PS)) || (rc = own.make(&diters, PS)) || (rc = own.make(&dgoing, (int64_t)1)))
        return rc;
    {
        std::vector<double> tcv((size_t)n * mcf::TC_COUNT);
        mcf::bl_time_consts(n, J.t->year, J.t->month, J.t->day, J.t->hour, tcv.data());
        HIP_TRY(hipMemcpy(dtconst, tcv.data(), tcv.size() * 8, hipMemcpyHostToDevice));
    }
    PsDev D;
    D.n = n; D.nd = nd; D.ps = PS;
    double** slot[kPsTables] = {&D.tc, &D.ea, &D.pk, &D.u2, &D.prec, &D.Rsw, &D.Rdif, &D.Rlw, &D.alb,
                                &D.tdew, &D.cp, &D.ph, &D.RabsC, &D.RswabsC, &D.cosz, &D.Rbeam, &D.kd, &D.Kc, &D.erhos, &D.mRc,
                                &D.Tc, &D.Tg, &D.te, &D.psim, &D.psih, &D.G,
                                &D.RswabsG, &D.RlwabsG, &D.tr, &D.umu, &D.mSc, &D.mMc, &D.Tcp, &D.sdepc, &D.sdepg};
    for (int k = 0; k < kPsTables; ++k) *slot[k] = tab[k];
    D.consts = dconst; D.tconst = dtconst; D.mxd = dmxd; D.mxdif = dmxdif; D.active = dactive; D.iters = diters; D.going = dgoing;
    D.tol = J.tol; D.maxiter = J.maxiter;

    const double* cols[8] = {J.w->temp, J.w->relhum, J.w->pres, J.w->windspeed, J.w->precip, J.w->swdown, J.w->difrad, J.w->lwdown};
    double* const ins[8] = {D.tc, D.ea, D.pk, D.u2, D.prec, D.Rsw, D.Rdif, D.Rlw};
    std::vector<double> hconst((size_t)PB * mcf::PS_COUNT), halb((size_t)(PB * n)), hden;
    std::vector<int> hactive((size_t)PS);
    const bool enter = 100.0 > J.tol;                         // the host's `tst = 100.0; while (tst > tol)`
    mcf_pointsnow_batch_out* o = J.out;

    for (int64_t p0 = 0; p0 < J.P; p0 += PB) {
        const int64_t pb = std::min(PB, J.P - p0);
        const size_t bytes = (size_t)(pb * n) * 8;
        D.pb = (int)pb;
        for (int k = 0; k < 8; ++k) {
            HIP_TRY(hipMemcpy(stage, cols[k] + p0 * n, bytes, hipMemcpyHostToDevice));
            if ((rc = ps_transpose(stage, pb, n, n, ins[k], PS))) return rc;
        }
        for (int64_t p = 0; p < pb; ++p) {
            const int64_t g = p0 + p;
            mcf::ps_point_consts(J.vegp + g * 4, J.other + g * 7, J.snowenv[g], hconst.data() + p * mcf::PS_COUNT);
            mcf::ps_albedo(J.w->precip + g * n, n, halb.data() + p * n);
        }
        HIP_TRY(hipMemcpy(stage, halb.data(), bytes, hipMemcpyHostToDevice));
        if ((rc = ps_transpose(stage, pb, n, n, D.alb, PS))) return rc;
        for (int64_t p = 0; p < PS; ++p) hactive[(size_t)p] = p < pb ? 1 : 0;
        HIP_TRY(hipMemcpy(dconst, hconst.data(), (size_t)pb * mcf::PS_COUNT * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dactive, hactive.data(), (size_t)PS * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(diters, 0, (size_t)PS * 4));
        HIP_TRY(hipMemset(dmxdif, 0, (size_t)PS * 8));
        HIP_TRY(hipMemset(dmxd, 0, (size_t)PS * 8));

        const unsigned gstep = (unsigned)((n * PS + kStepBlock - 1) / kStepBlock);
        const unsigned gday = (unsigned)((nd * PS + kStepBlock - 1) / kStepBlock);
        const unsigned gwave = (unsigned)((pb + 63) / 64), gpoint = (unsigned)((pb + 255) / 256);
        hipLaunchKernelGGL(k_ps_setup, dim3(gstep), dim3(kStepBlock), 0, 0, D);
        hipLaunchKernelGGL(k_ps_gflux, dim3(gday), dim3(kStepBlock), 0, 0, D, (const double*)D.tc, 1);
        HIP_TRY(hipGetLastError());
        if (!enter) {                                          // no pass: the host leaves these vectors as the caller gave them
            double* untouched[10] = {D.RswabsG, D.RlwabsG, D.tr, D.umu, D.mSc, D.mMc, D.Tcp, D.mRc, D.sdepc, D.sdepg};
            for (int k = 0; k < 10; ++k) HIP_TRY(hipMemset(untouched[k], 0, (size_t)((k >= 8 ? n + 1 : n) * PS) * 8));
        }
        while (enter) {
            HIP_TRY(hipMemsetAsync(dgoing, 0, 4, 0));
            hipLaunchKernelGGL(k_ps_sweep, dim3(gwave), dim3(64), 0, 0, D);
            hipLaunchKernelGGL(k_ps_gflux, dim3(gday), dim3(kStepBlock), 0, 0, D, (const double*)D.Tg, 0);
            hipLaunchKernelGGL(k_ps_finish, dim3(gpoint), dim3(256), 0, 0, D);
            HIP_TRY(hipGetLastError());
            int going = 0;                                    // the one small copy of a pass; it also reports a fault
            HIP_TRY(hipMemcpy(&going, dgoing, 4, hipMemcpyDeviceToHost));
            if (going == 0) break;
        }
        double* host[11] = {o->Tc, o->Tg, o->G, o->RswabsG, o->RlwabsG, o->tr, o->umu, o->sublmelt, o->tempmelt, o->rainmelt,
                            o->sstemp};
        double* dev[11] = {D.Tc, D.Tg, D.G, D.RswabsG, D.RlwabsG, D.tr, D.umu, D.mSc, D.mMc, D.mRc, D.Tcp};
        for (int k = 0; k < 11; ++k) {
            if ((rc = ps_transpose(dev[k], n, pb, PS, stage, n))) return rc;
            HIP_TRY(hipMemcpy(host[k] + p0 * n, stage, bytes, hipMemcpyDeviceToHost));
        }
        double* hostd[2] = {o->sdepc, o->sdepg};
        double* devd[2] = {D.sdepc, D.sdepg};
        for (int k = 0; k < 2; ++k) {
            if ((rc = ps_transpose(devd[k], n + 1, pb, PS, stage, n + 1))) return rc;
            HIP_TRY(hipMemcpy(hostd[k] + p0 * (n + 1), stage, (size_t)(pb * (n + 1)) * 8, hipMemcpyDeviceToHost));
        }
        for (int64_t p = 0; p < pb; ++p) {                     // the density of the whole run
            const double den = hconst[(size_t)(p * mcf::PS_COUNT + mcf::PS_SDEN0)];
            std::fill_n(o->sdenc + (p0 + p) * n, n, den);
            std::fill_n(o->sdeng + (p0 + p) * n, n, den);
        }
        HIP_TRY(hipMemcpy(o->mxdif + p0, dmxdif, (size_t)pb * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(o->iters + p0, diters, (size_t)pb * 4, hipMemcpyDeviceToHost));
    }
    return MCF_OK;
}


}  // namespace

extern "C" int mcf_bigleaf_batch(int64_t P, int64_t n, const mcf_obstime* obstime, const mcf_point_weather* weather,
                                 const double* vegp, const double* groundp, const double* soilm, const double* lat,
                                 const double* lon, double dTmx, double zref, int32_t maxiter, double bwgt, double tol,
                                 int32_t yearG, int64_t points_per_block, int32_t device, mcf_bigleaf_batch_out* o) {
    if (!obstime_ok(obstime)) return mcf::api_fail(MCF_ERR_ARG, "mcf_bigleaf_batch: null obstime");
    if (!weather_ok(weather)) return mcf::api_fail(MCF_ERR_ARG, "mcf_bigleaf_batch: null weather column");
    if (!vegp || !groundp || !soilm || !lat || !lon || !o || !o->Tc || !o->Tg || !o->H || !o->G || !o->psih || !o->psim ||
        !o->phih || !o->OL || !o->uf || !o->RabsG || !o->albedo || !o->err || !o->iters)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_bigleaf_batch: null argument");
    if (const int rc = check_batch("mcf_bigleaf_batch", P, n)) return rc;
    if (yearG && n / 24 > 1 && n / 24 < 90)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_bigleaf_batch: yearG needs one day or at least 90 (the reference's 91-day circular "
                                          "mean reads outside its array for series in between)");
    if (points_per_block < 0) return mcf::api_fail(MCF_ERR_ARG, "mcf_bigleaf_batch: points_per_block < 0");
    BlJob J{};
    J.P = P; J.n = n; J.t = obstime; J.w = weather; J.vegp = vegp; J.groundp = groundp; J.shared_params = false; J.soilm = soilm;
    J.lat = lat; J.lon = lon; J.dTmx = dTmx; J.zref = zref; J.maxiter = maxiter; J.bwgt = bwgt; J.tol = tol;
    J.yearG = yearG ? 1 : 0; J.ppb = points_per_block; J.device = device; J.out = o;
    return run_bigleaf(J);
}

extern "C" int mcf_weatherhgt_batch(int64_t P, int64_t n, const mcf_obstime* obstime, const mcf_point_weather* weather,
                                    double zin, double uzin, double zout, const double* lat, const double* lon,
                                    int64_t points_per_block, int32_t device, double* temp, double* relhum, double* windspeed) {
    if (!obstime_ok(obstime)) return mcf::api_fail(MCF_ERR_ARG, "mcf_weatherhgt_batch: null obstime");
    if (!weather_ok(weather)) return mcf::api_fail(MCF_ERR_ARG, "mcf_weatherhgt_batch: null weather column");
    if (!lat || !lon || !temp || !relhum || !windspeed) return mcf::api_fail(MCF_ERR_ARG, "mcf_weatherhgt_batch: null argument");
    if (const int rc = check_batch("mcf_weatherhgt_batch", P, n)) return rc;
    if (points_per_block < 0) return mcf::api_fail(MCF_ERR_ARG, "mcf_weatherhgt_batch: points_per_block < 0");
    // mcf_weatherhgt's fixed canopy and ground, and its yearG rule (the annual term is off for 2..89 days)
    static const double vegp[10] = {0.12, 1, 1, 0.1, 0.4, 0.2, 0.05, 0.97, 0.33, 100.0};
    static const double groundp[12] = {0.15, 0.0, 180.0, 0.97, 1.529643, 0.509, 0.06, 0.5422, 5.2, 2.6, 0.419, 0.074};
    BlJob J{};
    J.P = P; J.n = n; J.t = obstime; J.w = weather; J.vegp = vegp; J.groundp = groundp; J.shared_params = true; J.soilm = nullptr;
    J.lat = lat; J.lon = lon; J.dTmx = 25; J.zref = 2; J.maxiter = 20; J.bwgt = 0.5; J.tol = 0.5;
    J.yearG = (n / 24 <= 1 || n / 24 >= 90) ? 1 : 0; J.ppb = points_per_block; J.device = device; J.out = nullptr;
    J.zin = zin; J.uzin = uzin; J.zout = zout; J.wtemp = temp; J.wrh = relhum; J.wws = windspeed;
    return run_bigleaf(J);
}

extern "C" int mcf_pointmprocess_batch(int64_t P, int64_t n, const double* windspeed, const double* tc, const double* rh,
                                       const double* pk, const double* uf, const double* soilm, const double* RabsG,
                                       double zref, const double* h, const double* pai, const double* rho, const double* Vm,
                                       const double* Vq, const double* Mc, int32_t device, double* umu, double* kp,
                                       double* muGp, double* DDp, double* T0p, double* dtrp) {
    if (!windspeed || !tc || !rh || !pk || !uf || !soilm || !RabsG || !h || !pai || !rho || !Vm || !Vq || !Mc || !umu || !kp ||
        !muGp || !DDp || !T0p || !dtrp)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_pointmprocess_batch: null argument");
    if (const int rc = check_batch("mcf_pointmprocess_batch", P, n)) return rc;
    if (const int rc = mcf::check_device(device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(device));
    int64_t PB;
    if (const int rc = block_points(P, n, 13, 0, &PB)) return rc;
    mcf::DevOwner own;
    int rc;
    double *buf[13], *dconst;
    for (auto& b : buf)
        if ((rc = own.make(&b, PB * n))) return rc;
    if ((rc = own.make(&dconst, PB * mcf::PC_COUNT))) return rc;
    const double* ins[7] = {windspeed, tc, rh, pk, uf, soilm, RabsG};
    double* outs[6] = {umu, kp, muGp, DDp, T0p, dtrp};
    std::vector<double> hconst((size_t)PB * mcf::PC_COUNT);
    for (int64_t p0 = 0; p0 < P; p0 += PB) {
        const int64_t pb = std::min(PB, P - p0);
        const size_t bytes = (size_t)(pb * n) * 8;
        for (int k = 0; k < 7; ++k) HIP_TRY(hipMemcpy(buf[k], ins[k] + p0 * n, bytes, hipMemcpyHostToDevice));
        for (int64_t p = 0; p < pb; ++p) {
            const int64_t g = p0 + p;
            mcf::pmp_point_consts(zref, h[g], pai[g], rho[g], Vm[g], Vq[g], Mc[g], hconst.data() + p * mcf::PC_COUNT);
        }
        HIP_TRY(hipMemcpy(dconst, hconst.data(), (size_t)pb * mcf::PC_COUNT * 8, hipMemcpyHostToDevice));
        PmpDev D;
        D.n = n; D.u2 = buf[0]; D.tc = buf[1]; D.rh = buf[2]; D.pk = buf[3]; D.uf = buf[4]; D.soilm = buf[5]; D.RabsG = buf[6];
        D.consts = dconst; D.umu = buf[7]; D.kp = buf[8]; D.muGp = buf[9]; D.DDp = buf[10]; D.T0p = buf[11]; D.dtrp = buf[12];
        hipLaunchKernelGGL(k_pointmprocess, dim3((unsigned)((n + kGroup - 1) / kGroup), (unsigned)pb), dim3(kGroup), 0, 0, D);
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < 6; ++k) HIP_TRY(hipMemcpy(outs[k] + p0 * n, buf[7 + k], bytes, hipMemcpyDeviceToHost));
    }
    return MCF_OK;
}

extern "C" int mcf_pointmodelsnow_batch(int64_t P, int64_t n, const mcf_obstime* obstime, const mcf_point_weather* weather,
                                        const double* vegp, const double* other, const int32_t* snowenv, double tol,
                                        double maxiter, int64_t points_per_block, int32_t device, mcf_pointsnow_batch_out* o) {
    const char* who = "mcf_pointmodelsnow_batch";
    if (!obstime_ok(obstime)) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": null obstime");
    if (!weather_ok(weather) || !weather->precip) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": null weather column");
    if (!vegp || !other || !snowenv || !o) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": null argument");
    const void* outs[] = {o->Tc, o->Tg, o->sdenc, o->sdeng, o->G, o->RswabsG, o->RlwabsG, o->tr, o->umu, o->sublmelt, o->tempmelt,
                          o->rainmelt, o->sstemp, o->sdepc, o->sdepg, o->mxdif, o->iters};
    for (const void* q : outs)
        if (!q) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": null output vector");
    if (P < 1) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": P < 1: the batch needs at least one point");
    if (n % 24 != 0) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": n % 24 != 0: the batch entries take whole days only");
    if (n < 24) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": n < 24: the daily mean of GFluxCppsnow needs one day");
    if (n > (1 << 28) || P > ((int64_t)1 << 40) / n) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": series too long");
    if (points_per_block < 0) return mcf::api_fail(MCF_ERR_ARG, std::string(who) + ": points_per_block < 0");
    PsJob J{};
    J.P = P; J.n = n; J.t = obstime; J.w = weather; J.vegp = vegp; J.other = other; J.snowenv = snowenv; J.tol = tol;
    J.maxiter = maxiter; J.ppb = points_per_block; J.device = device; J.out = o;
    return run_pointsnow(J);
}
