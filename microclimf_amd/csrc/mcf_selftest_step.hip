// mcf_selftest_step.hip — diagnostics: the per-cell-step sun position and humidity helpers of array forcing, elementwise.
//
// With array weather every cell-step works out its own sun and humidity values on the device, by algebra written for this
// project (mcf_device.hpp derive_time_af / derive_time_af_pass2, satvap_r / lapserate_r / dewpoint_r; mcf_snow_device.hpp
// sun_cell / sun_at_cell) instead of the reference's inverse-trigonometry chain.  k_selftest_step runs those functions on
// planes of n doubles, one lane per element, so that tests/test_step_gpu.py can hold each field against a high-precision
// evaluation of the reference's formulas — at sector boundaries, at sunrise, next to the zenith — beside the literal device
// route (sol_site + derive_time, sol_site + sun_derive) on the same inputs.
//
// A translation unit of its own: the functions under test are header-inline, and no existing kernel's code changes with it.
// Nothing here is tuned: the kernel is as fast as its libm calls and its 11 + 29 streams allow.
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

constexpr int kStepIn = 11;     // year, month, day, hour, winddir, lat, lon, tc, pk, rsw, rdif
constexpr int kHumIn = 3;       // tc, rh, pk
constexpr int kSolverOut = 29, kSnowOut = 21, kHumOut = 4;

// the TF_ fields of one element, in the order include/mcf.h documents for kinds 0 and 1
template <class Put>
__device__ __forceinline__ void put_step_fields(const TimeVals& t, Put put) {
    const int fields[10] = {TF_CZ, TF_SZ, TF_TANSA, TF_ZEND, TF_COSC, TF_TANC, TF_TAN2C, TF_INV2COSC, TF_SAZ, TF_CAZ};
    for (int f = 0; f < 10; ++f) put(f, t.v[fields[f]]);
    const int idx = (int)t.v[TF_IDX];
    put(10, (double)(idx & 31));
    put(11, (double)((idx >> 5) & 7));
    put(12, (double)((idx >> 8) & 1));
    put(13, t.v[TF_DE]); put(14, t.v[TF_GHRRAD]); put(15, t.v[TF_REM]); put(16, t.v[TF_LAPK]); put(17, t.v[TF_WFAC]);
    put(18, t.v[TF_RBEAM]); put(19, t.v[TF_RB]);
}

__global__ __launch_bounds__(256) void k_selftest_step(int kind, const double* __restrict__ in, double* __restrict__ out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    if (!live) i = 0;      // every lane computes (the wave-uniform branches of satvap_nd see whole waves); only live lanes store
    MathK K;
    K.set();
    __shared__ double s_exptab[256];      // the route k_solve takes
    K.use_table(s_exptab, (int)threadIdx.x);
    __shared__ __attribute__((aligned(16))) double s_logtab[512];
    K.use_log_table(s_logtab, (int)threadIdx.x, (int)blockDim.x);
    // as k_solve pins it: (true, false, true) in the fine array-forcing kernels, whose derive_time_af kinds 0 .. 2 run;
    // (true, false, false) in the coarse ones, whose humidity helpers kind 3 runs (the exp's table index then goes the plain way)
    K.pin(true, false, kind != 3);
    __syncthreads();
    auto get = [&](int f) { return in[(int64_t)f * n + i]; };
    auto put = [&](int f, double v) { if (live) out[(int64_t)f * n + i] = v; };
    const double NaN = __longlong_as_double(0x7FF8000000000000LL);
    if (kind == 3) {
        const double tc = get(0), rh = get(1), pk = get(2);
        const double es = satvap_r(tc, K), ea = es * rh / 100.0;        // as k_solve's coarse branch forms ea
        put(0, es); put(1, ea); put(2, dewpoint_r(ea, tc, K)); put(3, lapserate_r(tc, ea, pk));
        return;
    }
    const int year = (int)get(0), month = (int)get(1), day = (int)get(2);
    const double hour = get(3), winddir = get(4), lat = get(5), lon = get(6);
    const SolDate sd = sol_date(year, month, day);
    if (kind == 0 || kind == 1) {
        TimeVals t;
        for (int f = 0; f < TF_COUNT; ++f) t.v[f] = 1.0;       // what the routes read and this entry does not supply (GP, MUGP, ...)
        t.v[TF_TC] = get(7); t.v[TF_PK] = get(8); t.v[TF_RSW] = get(9); t.v[TF_RDIF] = get(10);
        const int windex = dir_index(winddir, 45.0, 8);
        if (kind == 0) {
            // the date row as k_date_setup makes it, the cell constants as k_cell_setup makes them
            const double A = 0.261799 * (hour + sd.eot / 60.0 - 12.0);
            const DateRow dr{sd.sindec, sd.cosdec, cos(A), sin(A)};
            const double B = 0.261799 * ((4.0 * lon) / 60.0);
            derive_time_af(t, dr, sin(lat * kPi / 180.0), cos(lat * kPi / 180.0), cos(B), sin(B), windex, K);
            put_step_fields(t, put);
            derive_time_af_pass2(t);
            put(24, dr.sindec); put(25, dr.cosdec); put(26, dr.cosA); put(27, dr.sinA);
        } else {
            // the literal route, as k_time_setup runs it
            const SolPos sp = sol_site(sd, hour, sin(lat * kPi / 180.0), cos(lat * kPi / 180.0), lon);
            derive_time(t, sp, windex);
            put_step_fields(t, put);
            put(24, sd.sindec); put(25, sd.cosdec); put(26, sd.eot); put(27, NaN);
        }
        put(20, t.v[TF_GHRRAD]); put(21, t.v[TF_REM]); put(22, t.v[TF_MUPM]); put(23, t.v[TF_INVMUPM]);
        put(28, (double)julday(year, month, day));
        return;
    }
    // kind 2: the snow kernels' sun from the same date row, beside the literal sol_site + sun_derive
    const double A = 0.261799 * (hour + sd.eot / 60.0 - 12.0);
    const snow::SunCell sc = snow::sun_cell(lat, lon);
    int sindex = 0;
    const snow::SunT s = snow::sun_at_cell(sd.sindec, sd.cosdec, cos(A), sin(A), sc, sindex);
    put(0, s.zend); put(1, s.cosz); put(2, s.cz); put(3, s.sz); put(4, s.tansa); put(5, s.kx); put(6, s.kcos); put(7, s.sa);
    put(8, s.ca); put(9, (double)sindex);
    const double latr = lat * kPi / 180.0;
    const SolPos sp = sol_site(sd, hour, sin(latr), cos(latr), lon);
    const snow::SunT l = snow::sun_derive(sp, false);
    put(10, l.zend); put(11, l.cosz); put(12, l.cz); put(13, l.sz); put(14, l.tansa); put(15, l.kx); put(16, l.kcos); put(17, l.sa);
    put(18, l.ca);
    put(19, snow::sun_derive(sp, true).tansa);       // the one field that depends on `degrees`
    put(20, (double)dir_index(sp.azid, 15.0, 24));
}

}  // namespace

extern "C" int mcf_selftest_step(int32_t kind, const double* in, int32_t nin, double* out, int32_t nout, int64_t n, int32_t device) {
    if (kind < 0 || kind > 3) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_step: kind must be 0, 1, 2 or 3");
    if (n < 1 || !in || !out) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_step: bad length or null argument");
    if (n >= ((int64_t)1 << 31)) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_step: at most 2^31 - 1 elements");
    const int want_in = kind == 3 ? kHumIn : kStepIn;
    const int want_out = kind == 3 ? kHumOut : kind == 2 ? kSnowOut : kSolverOut;
    if (nin != want_in || nout != want_out)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_step: kind " + std::to_string(kind) + " takes " + std::to_string(want_in) +
                                              " input and " + std::to_string(want_out) + " output planes");
    if (const int rc = mcf::check_device(device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(device));
    int rc;
    mcf::DevOwner db;
    const double* d_in;
    double* d_out;
    if ((rc = db.up(&d_in, in, n * nin, "in")) || (rc = db.make(&d_out, n * nout))) return rc;
    HIP_TRY(hipMemset(d_out, 0, (size_t)n * nout * 8));      // (a plane the kernel did not store reads 0)
    hipLaunchKernelGGL(k_selftest_step, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, kind, d_in, d_out, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out, (size_t)n * nout * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}
