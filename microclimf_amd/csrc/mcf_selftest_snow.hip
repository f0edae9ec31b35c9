// mcf_selftest_snow.hip — diagnostics: the device physics of the snow kernels (mcf_snow_device.hpp), elementwise.
//
// The two-stream coefficients on three shared reciprocals (ts_dif / ts_dir), cank1, the [0, pi] sine and cosine behind
// rh_canopy, the square root that stands for cos(atan(t)) in the interception model and the operand guards gexp / glog /
// gsqrt / gpow0 are algebra written for this project, not a transcription of the reference.  k_selftest_snow runs those
// functions on planes of n doubles, one lane per element, so that tests/test_snow_unit_gpu.py can hold every field against a
// high-precision evaluation of the reference's own formulas (tests/snow_ref.py) exactly where such algebra goes wrong: kd
// next to h, om next to 1, z next to h, the seams of the quadrant reduction, clump = 0, the clamps.
//
// A translation unit of its own: the functions under test are header-inline, and no existing kernel's code changes with it.
// Nothing here is tuned.  The planes of each kind: include/mcf.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/mcf.h"
#include "mcf_device.hpp"
#include "mcf_snow_device.hpp"
#include "mcf_rowblocks.hpp"
#include "mcf_hiphost.hpp"

namespace {

using namespace mcf;
using namespace mcf::snow;

constexpr int kKinds = 4;
constexpr int kIn[kKinds] = {2, 8, 32, 5};
constexpr int kOut[kKinds] = {12, 29, 23, 22};

__global__ __launch_bounds__(256) void k_selftest_snow(int kind, const double* __restrict__ in, double* __restrict__ out, int64_t n) {
    snow_tables_init();        // before anything else, as in every snow kernel
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    if (!live) i = 0;          // every lane computes; only live lanes store
    auto get = [&](int f) { return in[(int64_t)f * n + i]; };
    auto put = [&](int f, double v) { if (live) out[(int64_t)f * n + i] = v; };
    if (kind == 0) {
        const double x = get(0), y = get(1);
        put(0, gexp(x)); put(1, glog(x)); put(2, gsqrt(x)); put(3, gpow0(x, y));
        put(4, svp(x)); put(5, dewpoint(x)); put(6, rad4(x)); put(7, latent_lt0(x)); put(8, clamp01(x));
        // (hs is an hour count: the cast is defined for the operands the cases read this plane on, 0 <= x < 2^31)
        put(9, snow_albedo(x >= 0.0 && x < 2147483648.0 ? (int)x : 0));
        put(10, snow_satvap_r(x));
        const double relhum = 80.0;
        const double ea = snow_satvap_r(x) * relhum / 100;      // as k_fine_* forms it
        put(11, snow_lapserate_r(x, ea, y));
        return;
    }
    if (kind == 1) {
        const double pait = get(0), lref = get(1), ltra = get(2), gref = get(3), kd = get(4), kx = get(5), kcos = get(6), si = get(7);
        const double igref = gdiv(1.0, gref);                   // as the callers form it (MetT::ialb, MicroIn::ialb)
        const TsDif f = ts_dif(pait, lref, ltra, gref, igref);
        const TsDir d = ts_dir(pait, f, gref, kd);
        const CanK k = cank1(kx, kcos, si);
        put(0, f.om); put(1, f.a); put(2, f.gma); put(3, f.del); put(4, f.h); put(5, f.S1); put(6, f.iS1); put(7, f.iD1);
        put(8, f.iD2); put(9, f.u1); put(10, f.u2); put(11, f.D1); put(12, f.D2); put(13, f.p1); put(14, f.p2); put(15, f.p3);
        put(16, f.p4);
        put(17, d.sig); put(18, d.isig); put(19, d.S2); put(20, d.p5); put(21, d.p6); put(22, d.p7); put(23, d.p8); put(24, d.p9);
        put(25, d.p10);
        put(26, k.k); put(27, k.kd); put(28, k.Kc);
        return;
    }
    if (kind == 2) {
        const double h = get(0), pai = get(1), d = get(2), uf = get(3), prec = get(4), sint = get(5), Li = get(6);
        const double sdp[4] = {get(7), get(8), get(9), get(10)};
        const double depth = get(11), age = get(12), x = get(13), z = get(14);
        const double leafden = get(15), Flux = get(16), Fluxz = get(17), SH = get(18), SG = get(19), mxnear = get(20);
        const double zm = get(21), zref = get(22), za = get(23), T0 = get(24), tc = get(25), ea = get(26);
        const double slope = get(27), aspect = get(28), zend = get(29), azid = get(30), hc = get(31);
        put(0, zeroplane(h, pai));
        put(1, roughlen0(h, pai, d));
        put(2, canopy_snow_interception(hc, pai, uf, prec, sint, Li));
        put(3, snow_density(sdp, depth, age));
        double sn, cs;
        sincos_0pi(x, sn, cs);
        put(4, sn); put(5, cs);
        const double ih = gdiv(1.0, h);
        put(6, rh_canopy(uf, h, ih, d, z));
        put(7, rh_canopy(uf, h, ih, d, h));
        const BelowK bk = below_k(z, d, h, uf);
        put(8, bk.Kg); put(9, bk.Kh); put(10, bk.Kc); put(11, bk.iKc); put(12, bk.iKs);
        put(13, tv_below(bk, glog(pai), leafden, Flux, Fluxz, SH, SG, mxnear));      // lnpai as micro_above forms it
        // the two logarithms as micro_above's wind block forms them: log((z - d) / zm) + log 5
        constexpr double kLn5 = 0x1.9c041f7ed8d33p+0;
        const double izm = gdiv(1.0, zm);
        const double Lref5 = glog((zref - d) * izm) + kLn5, Lz5 = glog((za - d) * izm) + kLn5;
        const AboveTV tv = tv_above_l(za, d, zm, Lz5, Lref5, T0, tc, ea);
        put(14, tv.Tz); put(15, tv.ez);
        const SiteK sk = site_derive(slope, aspect);
        put(16, sk.cS); put(17, sk.sS); put(18, sk.cA); put(19, sk.sA); put(20, sk.flat ? 1.0 : 0.0);
        const SolPos sp{zend, zend * kToRad, azid};
        const SunT s = sun_derive(sp, false);
        put(21, solar_index(s, sk, false)); put(22, solar_index(s, sk, true));
        return;
    }
    // kind 3: the weather-only values of a step
    const double tc = get(0), rh = get(1), pk = get(2), tci = get(3), mxtc = get(4);
    MetT m;
    met_derive(m, tc, rh, pk, tci);
    put(0, m.ea); put(1, m.te); put(2, m.rem); put(3, m.rcan); put(4, m.la); put(5, m.cp); put(6, m.Da); put(7, m.gR); put(8, m.De);
    put(9, m.tdew); put(10, m.ph); put(11, m.sint);
    const MicroMet q = micro_met(tc, rh, pk, mxtc);
    put(12, q.es); put(13, q.ea); put(14, q.tdew); put(15, q.De); put(16, q.gHrad); put(17, q.Rem); put(18, q.la_pm); put(19, q.lat0);
    put(20, q.dTmx); put(21, q.ipk);
}

}  // namespace

extern "C" int mcf_selftest_snow(int32_t kind, const double* in, int32_t nin, double* out, int32_t nout, int64_t n, int32_t device) {
    if (kind < 0 || kind >= kKinds) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_snow: kind must be 0, 1, 2 or 3");
    if (n < 1 || !in || !out) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_snow: bad length or null argument");
    if (n >= ((int64_t)1 << 31)) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_snow: at most 2^31 - 1 elements");
    if (nin != kIn[kind] || nout != kOut[kind])
        return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_snow: kind " + std::to_string(kind) + " takes " + std::to_string(kIn[kind]) +
                                              " input and " + std::to_string(kOut[kind]) + " output planes");
    if (const int rc = mcf::check_device(device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(device));
    int rc;
    mcf::DevOwner db;
    const double* d_in;
    double* d_out;
    if ((rc = db.up(&d_in, in, n * nin, "in")) || (rc = db.make(&d_out, n * nout))) return rc;
    HIP_TRY(hipMemset(d_out, 0, (size_t)n * nout * 8));      // (a plane the kernel did not store reads 0)
    hipLaunchKernelGGL(k_selftest_snow, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, kind, d_in, d_out, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out, (size_t)n * nout * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}
