// mcf_snow.hip — the snow branch on the device: kernels and C-ABI entry points
//   mcf_gridmodelsnow1/2   per-cell, sequential-in-time snowpack model   cpp:4172-4673
//   mcf_gridmicrosnow1/2   microclimate of snow-covered cell-steps       cpp:4894-5214
// ("cpp:" = the reference's src/microclimfCpp.cpp).  Physics: mcf_snow_device.hpp.
//
// Parallel shape.  The snowpack is a recurrence in time (depth, density and age of two layers
// carried from step to step), so gridmodelsnow runs ONE LANE PER CELL with the lanes of a wave
// along the raster rows: every [rows,cols,tsteps] store is a coalesced 512-B line per wave and
// step, the state lives in registers, and — with data.frame climate — the per-step table row is
// wave-uniform (scalar loads).  gridmicrosnow has no recurrence: one lane per (cell, day) walks
// 24 hours after forming the day's mean snow temperature (snowdayan, cpp:4679-4712).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <optional>
#include <string>
#include <vector>

#include "../../include/mcf.h"
#include "mcf_rowblocks.hpp"
#include "mcf_hiphost.hpp"
#include "mcf_snow_device.hpp"
#include "mcf_snow_plan.hpp"
#include "mcf_sinks_host.hpp"
#include "mcf_ncsink.hpp"
#include "mcf_kernels.h"

// the ring kernel (lane per cell-hour, cell table in LDS, step record through scalar loads): 141 VGPRs without scratch at three
// waves per SIMD, 128 + 44 B (eight spill stores and loads per hour) at four — measured 0.515 against 0.55 s per simulated year
// of configs[4]'s share (the kernel moves ~144 B per snow cell-step: it is closer to the memory system's limit than to the
// VALU's, and the fourth wave hides more of the loads)
// waves per SIMD k_snowmodel is built for.  Round 4: with the cell's constants read from the workgroup's LDS table at their uses
// and the five output streams addressed as uniform base + 32-bit lane offset, the data.frame kernel fits 128 VGPRs without
// scratch (156 in round 3: three waves) — 105 once the step table comes through scalar loads (see the kernel's head); a fifth
// wave is out of reach through LDS, not registers (36 KB per 4-wave workgroup: the cell table + the exp / log tables).  The
// array-climate kernel derives the step's weather terms per lane and stays at three (168 VGPRs + 116 B of scratch; 232 B in round 3).
#ifndef MCF_MICRORING_WAVES
#define MCF_MICRORING_WAVES 4
#endif
#ifndef MCF_SNOW_WAVES
#define MCF_SNOW_WAVES 4
#endif
#ifndef MCF_SNOW_WAVES_AF
#define MCF_SNOW_WAVES_AF 3
#endif
#include "mcf_terrain.h"

namespace {
using namespace mcf;
using namespace mcf::snow;

// One time step with data.frame climate: everything that does not depend on the cell.
struct StepRow {
    MetT m;
    DayT d;
    SunT s;
    double rnet;     // RswabsG + RlwabsG - Rem of the point model, cpp:4229
    int32_t sindex, windex;
};
// Date part of a step for array climate (site part applied per cell).
struct DateRow2 {
    double sindec, cosdec, cosA, sinA;     // A = 0.261799 (hour + eot / 60 - 12): the hour angle without the cell's longitude
    int32_t windex, pad;
};

struct StepArgs {
    int tsteps;
    const int32_t *year, *month, *day;
    const double* hour;
    const double *temp, *relhum, *pres, *swdown, *difrad, *lwdown, *windspeed, *winddir, *precip;
    const double *Gp, *Tcp, *RswabsG, *RlwabsG, *umu;   // null for gridmicrosnow
    double lat, lon;
    int32_t degrees;   // horizon test in degrees (gridmodelsnow1) or radians
    StepRow* rows;
    DateRow2* dates;   // array climate
    double* mxtc;      // [1]
};

// ---- data.frame climate: per-step table -------------------------------------------------------
__global__ __launch_bounds__(256) void k_snow_steps(StepArgs a) {
    snow::snow_tables_init();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.tsteps) return;
    // (the record is assembled where it lives: a local StepRow — 44 doubles whose members are then copied as a block — went through
    // 352 B of scratch per lane)
    StepRow& r = a.rows[k];
    r.d = DayT{};
    r.rnet = 0.0;
    const SolDate sd = sol_date(a.year[k], a.month[k], a.day[k]);
    const double latr = a.lat * kPi / 180.0;
    const SolPos sp = sol_site(sd, a.hour[k], sin(latr), cos(latr), a.lon);
    r.s = sun_derive(sp, a.degrees != 0);
    r.sindex = dir_index(sp.azid, 15.0, 24);
    r.windex = dir_index(a.winddir[k], 45.0, 8);
    if (a.Gp) {
        met_derive(r.m, a.temp[k], a.relhum[k], a.pres[k], a.Tcp[k]);
        r.m.prec = a.precip[k];
        r.m.rsw = a.swdown[k]; r.m.rdif = a.difrad[k]; r.m.rlw = a.lwdown[k];
        r.m.umu = a.umu[k]; r.m.u2 = a.windspeed[k]; r.m.gp = a.Gp[k];
        r.rnet = a.RswabsG[k] + a.RlwabsG[k] - r.m.rem;
    } else {
        r.m = MetT{};
    }
}
// daily extremes of the point model's net radiation (cpp:4231-4282): one lane per day
__global__ __launch_bounds__(64) void k_snow_days(StepRow* rows, int tsteps) {
    snow::snow_tables_init();
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= tsteps / 24) return;
    DayT dy;
    day_init(dy);
    for (int h = 0; h < 24; ++h) {
        const StepRow& r = rows[d * 24 + h];
        day_accum(dy, r.rnet, r.m.rsw, r.m.rlw);
    }
    for (int h = 0; h < 24; ++h) rows[d * 24 + h].d = dy;
}
// snowalbCpp is a scan over time (hours since snowfall): a single lane walks the series once;
// the same walk yields the series maximum of temperature that gridmicrosnow1 needs (cpp:4973-4974)
__global__ void k_snow_alb(StepRow* rows, const double* precip, const double* temp, int tsteps, double* mxtc) {
    snow::snow_tables_init();
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int hs = 0;
    double mx = -273.15;
    for (int k = 0; k < tsteps; ++k) {
        if (k > 0) hs = precip[k] > 0 ? 0 : hs + 1;
        rows[k].m.alb = snow_albedo(hs);
        rows[k].m.ialb = gdiv(1.0, rows[k].m.alb);
        if (temp[k] > mx) mx = temp[k];
    }
    if (mxtc) *mxtc = mx;
}
// array climate: date-only part of the sun position
__global__ __launch_bounds__(256) void k_snow_dates(StepArgs a) {
    snow::snow_tables_init();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.tsteps) return;
    const SolDate sd = sol_date(a.year[k], a.month[k], a.day[k]);
    DateRow2 r;
    const double A = 0.261799 * (a.hour[k] + sd.eot / 60.0 - 12.0);             // cpp:44, 54 without the longitude term
    r.sindec = sd.sindec; r.cosdec = sd.cosdec; r.cosA = cos(A); r.sinA = sin(A);
    r.windex = dir_index(a.winddir[k], 45.0, 8);
    r.pad = 0;
    a.dates[k] = r;
}

// ---- gridmodelsnow ---------------------------------------------------------------------------------
struct ModelArgs {
    int64_t N;
    int tsteps;
    const double *pai, *hgt, *leaft, *clump, *slope, *aspect, *skyview, *wsa, *hor, *lats, *lons;
    const double *isnowdc, *isnowdg;
    const int32_t *isnowac, *isnowag;
    double zref;
    double sdp[4];
    const StepRow* rows;     // data.frame climate
    const DateRow2* dates;   // array climate
    const double *temp, *relhum, *pres, *swdown, *difrad, *lwdown, *windspeed, *precip;   // [N][T]
    const double *Gp, *Tcp, *RswabsG, *RlwabsG, *umu;                                     // [N][T]
    double *Tc, *Tg, *sdepc, *sdepg, *sden;   // [N][T] or null
    double *agec, *ageg, *meltc, *meltg;      // [N] or null
    // `.snowmodel1`'s topographic redistribution and hand-over (R/internal.R:2589-2612) fused into the chunk's model run
    // (tpic != null; the snow plan's chunk loop): the depths leave the kernel redistributed — sdepc holds totalSWE, sdepg the
    // ground snow depth — and the state of the next chunk (pack depth, snow surface, the two ages) is written by the same lane.
    // Until round 4 a second kernel re-read and re-wrote the chunk's three depth / density series: 10 GB per chunk of a
    // 512 x 4096 block, 0.21 s of a simulated year.
    const double *tpic, *dtm;
    double tpimean;
    double *isnowdc_out, *dtms;
    int32_t *isnowac_out, *isnowag_out;
    // [N][T / 24] or null (data.frame climate): the day's mean of the Tg series, as the snow-day microclimate takes it (cpp:5010-5016:
    // the 24 values added in their order, / 24; NA where the day's first value is) — made here, where the values are, its reader
    // does not read the series a second time for it
    double* tzd;
};

template <bool AF>
__global__ __launch_bounds__(256, AF ? MCF_SNOW_WAVES_AF : MCF_SNOW_WAVES) void k_snowmodel(ModelArgs a, const StepRow* __restrict__ rows,
                                                                                             const DateRow2* __restrict__ dates) {
    // (rows / dates = a.rows / a.dates as `__restrict__` kernel arguments of their own: a pointer read out of the by-value struct
    // carries no noalias, the series' stores might clobber the table for all the compiler knows, and every field of a step's
    // row came through a VECTOR load of a uniform address — 40 loads and as many VGPR pairs per step instead of scalar loads)
    snow::snow_tables_init();
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.N) return;
    const int64_t N = a.N;
    const double NA = na_real();
    const double hgt0 = a.hgt[c];
    // fused redistribution (see ModelArgs): the cell's tpi weight and the depths the chunk starts from
    const bool redist = a.tpic != nullptr;
    // (the cell's constants and the redistribution's state live in the workgroup's LDS table, lane = column: read — and the
    // two running values written — inside the step where they are used, not carried in registers)
    __shared__ double s_cv[CV_COUNT + 5 + (AF ? 4 : 0)][256];
    enum { RV_TPI = CV_COUNT, RV_ASD, RV_ASC, RV_TOT, RV_GD };
    {
        const int l = threadIdx.x;
        s_cv[RV_TPI][l] = redist ? a.tpic[c] / a.tpimean : 0.0;      // tpic / mean(tpic, na.rm = TRUE)
        s_cv[RV_ASD][l] = redist ? a.isnowdg[c] : 0.0;
        s_cv[RV_ASC][l] = redist ? a.isnowdc[c] : 0.0;
        s_cv[RV_TOT][l] = 0.0; s_cv[RV_GD][l] = 0.0;
    }
    // (dc, dg, den) of a step -> what is stored: as they are, or redistributed (int:2593-2606; the operations of the former
    // k_snow_redistribute in its order, also on an NA cell's NAs)
    auto finish = [&](double& dc, double& dg, double den) {
        if (!redist) return;
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        const double r_asd = s_cv[RV_ASD][l], r_asc = s_cv[RV_ASC][l];
        const double dsnow = dg - r_asd;
        double dsnow2 = dsnow * s_cv[RV_TPI][l];
        if (dsnow < 0) dsnow2 = dsnow;
        const double cdsnow = dc - r_asc - dsnow;
        const double r_tot = r_asc + cdsnow + dsnow2, r_gd = r_asd + dsnow2;
        s_cv[RV_TOT][l] = r_tot; s_cv[RV_GD][l] = r_gd;
        dc = r_tot * den;
        dg = r_gd;
    };
    if (isnan(hgt0)) {   // cpp:4320-4321
        for (int k = 0; k < a.tsteps; ++k) {
            const int64_t o = c + N * k;
            double dc = NA, dg = NA;
            finish(dc, dg, NA);
            if (a.Tc) a.Tc[o] = NA;
            if (a.Tg) a.Tg[o] = NA;
            if (a.sdepc) a.sdepc[o] = dc;
            if (a.sdepg) a.sdepg[o] = dg;
            if (a.sden) a.sden[o] = NA;
        }
        if constexpr (!AF) {
            if (a.tzd && a.Tg)
                for (int d = 0; d < a.tsteps / 24; ++d) a.tzd[c + N * d] = NA;
        }
        if (redist && a.tsteps > 0) { a.isnowdc_out[c] = s_cv[RV_TOT][threadIdx.x]; a.dtms[c] = a.dtm[c] + s_cv[RV_GD][threadIdx.x]; }
        if (a.agec) a.agec[c] = NA;
        if (a.ageg) a.ageg[c] = NA;
        if (a.meltc) a.meltc[c] = NA;
        if (a.meltg) a.meltg[c] = NA;
        return;
    }
    {
        const int l = threadIdx.x;
        const double slope = a.slope[c];
        const SiteK sk = site_derive(slope, a.aspect[c]);
        s_cv[CV_PAI][l] = a.pai[c]; s_cv[CV_HGT][l] = hgt0; s_cv[CV_CLUMP][l] = a.clump[c]; s_cv[CV_LTRA][l] = a.leaft[c];
        s_cv[CV_SKYVIEW][l] = a.skyview[c];
        s_cv[CV_CS][l] = sk.cS; s_cv[CV_SS][l] = sk.sS; s_cv[CV_CA][l] = sk.cA; s_cv[CV_SA][l] = sk.sA; s_cv[CV_SLOPE][l] = slope;
    }
    if (AF) {     // the cell's part of the sun position: four more rows of the LDS table, read inside the step
        const SunCell sc = sun_cell(a.lats[c], a.lons[c]);
        const int l = threadIdx.x;
        s_cv[RV_GD + 1][l] = sc.sinlat; s_cv[RV_GD + 2][l] = sc.coslat; s_cv[RV_GD + 3][l] = sc.cosB; s_cv[RV_GD + 4][l] = sc.sinB;
    }
    Pack s;   // cpp:4325-4332
    s.agec = a.isnowac[c];
    s.ageg = a.isnowag[c];
    s.sdenc = snow_density(a.sdp, a.isnowdc[c], (double)s.agec);
    s.sdeng = ((a.sdp[0] - a.sdp[1]) * (1 - exp(-a.sdp[2] * a.isnowdg[c] * 0.5 / 100.0 - a.sdp[3] * s.ageg / 24.0)) +
               a.sdp[1]) * 1000.0;
    s.sdepc = a.isnowdc[c];
    s.sdepg = a.isnowdg[c];
    double meltc = AF ? NA : 0.0;   // only gridmodelsnow1 zeroes it (cpp:4333); gridmodelsnow2 adds to NA
    double meltg = NA;              // never zeroed in either (cpp:4308, 4396)
    const double nosnow_den = a.sdp[1] * 1000.0;
    const int ndays = a.tsteps / 24;
    int hs = 0;
    DayT dy;
    [[maybe_unused]] double tzsum = 0.0;         // the day's Tg values added up (tzd)
    [[maybe_unused]] bool tz_na = false;
    for (int k = 0; k < a.tsteps; ++k) {
        const int64_t o = c + N * k;
        // (an opaque lane index per step: the table's values are read at their uses, not hoisted in front of the loop)
        int li = (int)threadIdx.x;
        asm volatile("" : "+v"(li));
        CellV cv;
        cv.p = &s_cv[0][li]; cv.cs = 256;
        double tc, prec;
        if (AF) {
            tc = a.temp[o]; prec = a.precip[o];
            if (k > 0) hs = prec > 0 ? 0 : hs + 1;
            if (k % 24 == 0) {   // the day's extremes of the point model's net radiation, cpp:4514-4566
                if (k / 24 < ndays) {
                    day_init(dy);
                    for (int h = 0; h < 24; ++h) {
                        const int64_t q = c + N * (k + h);
                        const double rnet = a.RswabsG[q] + a.RlwabsG[q] - 0.97 * kSb * rad4(a.temp[q]);
                        day_accum(dy, rnet, a.swdown[q], a.lwdown[q]);
                    }
                } else {
                    dy.rmx = dy.rmn = dy.rswmx = dy.rlwmx = dy.rswmn = dy.rlwmn = dy.gmx = 0.0;
                }
            }
        } else {
            tc = rows[k].m.tc; prec = rows[k].m.prec;
        }
        bool snowtest = s.sdepc > 0.0;                       // cpp:4336-4338
        if (tc < 2.0 && prec > 0.0) snowtest = true;
        double vTc = 0.0, vTg = 0.0, vdc = 0.0, vdg = 0.0, vden = nosnow_den;
        if (snowtest) {
            PackOut po;
            if (AF) {
                MetT m;
                met_derive(m, tc, a.relhum[o], a.pres[o], a.Tcp[o]);
                m.prec = prec;
                m.rsw = a.swdown[o]; m.rdif = a.difrad[o]; m.rlw = a.lwdown[o];
                m.umu = a.umu[o]; m.u2 = a.windspeed[o]; m.gp = a.Gp[o];
                m.alb = snow_albedo(hs);
                m.ialb = gdiv(1.0, m.alb);
                const DateRow2 dr = dates[k];
                SunCell sc;
                sc.sinlat = s_cv[RV_GD + 1][li]; sc.coslat = s_cv[RV_GD + 2][li]; sc.cosB = s_cv[RV_GD + 3][li]; sc.sinB = s_cv[RV_GD + 4][li];
                int sindex;
                const SunT sun = sun_at_cell(dr.sindec, dr.cosdec, dr.cosA, dr.sinA, sc, sindex);
                const double ha = a.hor[(int64_t)sindex * N + c];
                const double ws = a.wsa[(int64_t)dr.windex * N + c];
                pack_step(m, dy, sun, cv, ha, ws, a.sdp, a.zref, s, po);
            } else {
                const StepRow& r = rows[k];
                const double ha = a.hor[(int64_t)r.sindex * N + c];
                const double ws = a.wsa[(int64_t)r.windex * N + c];
                pack_step(r.m, r.d, r.s, cv, ha, ws, a.sdp, a.zref, s, po);
            }
            vTc = po.Tc; vTg = po.Tg; vdc = s.sdepc; vdg = s.sdepg; vden = s.sdenc;
            meltc = meltc + po.melc;                          // cpp:4394-4396 (meltc is added twice)
            meltc = meltc + gdiv(po.melc * 1000.0, s.sdenc);   // densities are >= 1000 sdp[1] > 0 (or NaN)
            meltg = meltg + gdiv(po.melg * 1000.0, s.sdeng);
        }
        finish(vdc, vdg, vden);
        // the step's slab of an output is a uniform base (scalar registers) + the lane's 32-bit byte offset: no 64-bit vector
        // address per series kept across the loop (N * 8 < 4 GB: checked by the host)
        {
            uint32_t cb = (uint32_t)c * 8u;
            asm volatile("" : "+v"(cb));
            const int64_t so = N * k;
            auto st = [&](double* base, double v) { *(double*)((char*)(base + so) + cb) = v; };
            if (a.Tc) st(a.Tc, vTc);
            if (a.Tg) st(a.Tg, vTg);
            if (a.sdepc) st(a.sdepc, vdc);
            if (a.sdepg) st(a.sdepg, vdg);
            if (a.sden) st(a.sden, vden);
        }
        if constexpr (!AF) {
            if (a.tzd && a.Tg) {
                const int h = k % 24;
                if (h == 0) { tzsum = 0.0; tz_na = isnan(vTg); }
                tzsum += vTg;
                if (h == 23) a.tzd[c + N * (k / 24)] = tz_na ? NA : tzsum / 24.0;
            }
        }
    }
    if (a.agec) a.agec[c] = (double)s.agec;
    if (a.ageg) a.ageg[c] = (double)s.ageg;
    if (a.meltc) a.meltc[c] = meltc;
    if (a.meltg) a.meltg[c] = meltg;
    if (redist && a.tsteps > 0) {      // hand-over to the next chunk, int:2607-2612
        a.isnowdc_out[c] = s_cv[RV_TOT][threadIdx.x];
        a.dtms[c] = a.dtm[c] + s_cv[RV_GD][threadIdx.x];
        a.isnowac_out[c] = s.agec;
        a.isnowag_out[c] = s.ageg;
    }
}

// ---- gridmicrosnow ---------------------------------------------------------------------------------
struct MicroArgs {
    int64_t N;
    int tsteps;
    double reqhgt, mat, zref, hiy;
    const double *pai, *hgt, *leaft, *clump, *paia, *leafd, *leafden, *slope, *aspect, *skyview, *wsa, *hor;
    const double *lats, *lons, *Smax;
    const StepRow* rows;
    const DateRow2* dates;
    const double* mxtc1;   // [1] data.frame climate
    const MicroMet* mmet;  // [T] data.frame climate: weather-only terms of every step (k_micro_steps)
    const void* mstep;     // [T] MicroStep (the snow plan's ring kernel): rows' sun / albedo, mmet and the step's weather in one record
    int32_t day0;          // first day of this launch (blockIdx.y counts from it)
    const double *temp, *relhum, *pres, *swdown, *difrad, *lwdown, *windspeed, *precip, *umu;   // [T] or [N][T]
    const double *sTc, *sTg, *swe, *sdepg, *sden;   // snowm, [N][T]
    const double* tzd;  // [N][T / 24] the days' means of sTg made by the snow model's kernel (ModelArgs::tzd), or null: made here
    double* meanD;      // [N]
    double* mxtc;       // [N]        array climate
    int32_t* hs0;       // [N][nchunks] hours since snowfall at the start of each day (array climate)
    double* out[MCF_NOUT];   // [N][T] or null
};

// data.frame climate: the weather-only terms of snowabovepoint, once per step instead of once per cell-step
__global__ __launch_bounds__(256) void k_micro_steps(const double* __restrict__ temp, const double* __restrict__ relhum,
                                                     const double* __restrict__ pres,
                                                     const double* __restrict__ mxtc1, int tsteps, MicroMet* __restrict__ out) {
    snow::snow_tables_init();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= tsteps) return;
    out[k] = micro_met(temp[k], relhum[k], pres[k], *mxtc1);
}

// per-cell reductions over the whole series: meanDsnow (cpp:4713-4737) and, with array climate, the
// cell's maximum temperature (cpp:5139-5145) and the albedo clock at every day start
// Everything k_microsnow_ring reads of a step, in one record: ONE table pointer in scalar registers instead of eleven (the
// kernel keeps ~100 uniform values alive; what does not fit the SGPR file is spilled to VGPR lanes, a VALU instruction per access)
struct MicroStep {
    SunT s;
    MicroMet mm;
    double tc, pk, u2, rsw, rdif, rlw, umu, alb, ialb;
    int32_t sindex, windex;
};
__global__ __launch_bounds__(256) void k_micro_pack(const StepRow* __restrict__ rows, const MicroMet* __restrict__ mmet,
                                                    const double* __restrict__ temp, const double* __restrict__ pres,
                                                    const double* __restrict__ wind, const double* __restrict__ sw,
                                                    const double* __restrict__ dif, const double* __restrict__ lw,
                                                    const double* __restrict__ umu, int T, MicroStep* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= T) return;
    MicroStep& m = out[k];          // (in place: a local record went through 176 B of scratch)
    m.s = rows[k].s; m.mm = mmet[k];
    m.tc = temp[k]; m.pk = pres[k]; m.u2 = wind[k]; m.rsw = sw[k]; m.rdif = dif[k]; m.rlw = lw[k]; m.umu = umu[k];
    m.alb = rows[k].m.alb; m.ialb = rows[k].m.ialb;
    m.sindex = rows[k].sindex; m.windex = rows[k].windex;
}
// a step's term of meanDsnow (cpp:4713-4737): sqrt(2 kappa / omega), kappa from the pack's density (> 0, or NaN) — with the lean
// exponential, quotient and root (the device libm's made k_meand_accumulate a compute-bound kernel: 11 000 instructions per wave)
__device__ __forceinline__ double snow_damping_term(double den) {
    const double co = 0.0442 * gexp(5.181 * den * (1.0 / 1000.0));
    const double kap = gdiv(co, den * 2090.0);
    return gsqrt(kap * (2.0 / kOmdy));
}
template <bool AF>
__global__ __launch_bounds__(256) void k_microsnow_cell(MicroArgs a) {
    snow::snow_tables_init();
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.N) return;
    if (isnan(a.hgt[c])) return;
    const int64_t N = a.N;
    double meanD = na_real();
    if (!isnan(a.sden[c])) {
        double sumD = 0.0;
        for (int k = 0; k < a.tsteps; ++k) {
            sumD += snow_damping_term(a.sden[c + N * k]);
        }
        meanD = sumD / (double)a.tsteps;
    }
    a.meanD[c] = meanD;
    if (AF) {
        const int nch = (a.tsteps + 23) / 24;
        double mx = -273.15;
        int hs = 0;
        for (int k = 0; k < a.tsteps; ++k) {
            const double t = a.temp[c + N * k];
            if (t > mx) mx = t;
            if (k > 0) hs = a.precip[c + N * k] > 0 ? 0 : hs + 1;
            if (k % 24 == 0) a.hs0[c + N * (k / 24)] = hs;
        }
        (void)nch;
        a.mxtc[c] = mx;
    }
}

// Array climate, streamed (mcf_snowplan_micro_setup with array weather): the two per-cell scans of k_microsnow_cell<true> — the
// maximum air temperature and the albedo clock at every day start over the snow-day SUBSET series (cpp:5139-5145, 3733-3739) —
// a run of consecutive subset days at a time, the state (mx, hs) carried in memory between the runs; same walk, same values.
__global__ __launch_bounds__(256) void k_micro_scan(const double* __restrict__ temp, const double* __restrict__ precip, int64_t N, int sub0,
                                                    int ndays, const double* __restrict__ hgt, double* __restrict__ mxtc,
                                                    int32_t* __restrict__ hs_state, int32_t* __restrict__ hs0) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    if (isnan(hgt[c])) return;
    double mx = sub0 == 0 ? -273.15 : mxtc[c];
    int hs = sub0 == 0 ? 0 : hs_state[c];
    for (int d = 0; d < ndays; ++d)
        for (int h = 0; h < 24; ++h) {
            const int64_t q = c + N * (int64_t)(d * 24 + h);
            const double t = temp[q];
            if (t > mx) mx = t;
            if (sub0 + d > 0 || h > 0) hs = precip[q] > 0 ? 0 : hs + 1;
            if (h == 0) hs0[c + N * (int64_t)(sub0 + d)] = hs;
        }
    mxtc[c] = mx;
    hs_state[c] = hs;
}

// ---- gridmicrosnow1 inside the chunk loop, device-resident (mcf_snowplan_micro_*) ---------------------------------
// meanDsnow (cpp:4713-4737) is the mean over the WHOLE snow-day series of sqrt(2 kappa / omega); the series lives on the
// device one chunk at a time, so a first pass over the year adds the chunk's snow days to a per-cell running sum — the
// same terms in the same order as k_microsnow_cell's loop.
__global__ __launch_bounds__(256) void k_meand_accumulate(const double* __restrict__ sden, const double* __restrict__ hgt,
                                                          int64_t N, int ndays, const int32_t* __restrict__ snowday, int first,
                                                          double* __restrict__ sumD, int32_t* __restrict__ sden_na) {
    snow::snow_tables_init();
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N || isnan(hgt[c])) return;
    double s = sumD[c];
    bool seen = !first;
    for (int d = 0; d < ndays; ++d) {
        if (!snowday[d]) continue;
        if (!seen) { sden_na[c] = isnan(sden[c + N * (d * 24)]) ? 1 : 0; seen = true; }
        for (int h = 0; h < 24; ++h) {
            s += snow_damping_term(sden[c + N * (d * 24 + h)]);
        }
    }
    sumD[c] = s;
}
__global__ __launch_bounds__(256) void k_meand_finish(const double* __restrict__ sumD, const int32_t* __restrict__ sden_na,
                                                      const double* __restrict__ hgt, int64_t N, double nsteps,
                                                      double* __restrict__ meanD) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    meanD[c] = (isnan(hgt[c]) || sden_na[c]) ? na_real() : sumD[c] / nsteps;
}

// k_microsnow on one chunk's snow days, reading the chunk's snow series where mcf_snowplan_run_chunk left them and
// writing into a ring slot of the grid solver's plan (tiled layout, RingView) — the merge of `.runmicrosnow1`
// (R/internal.R:3565-3578, 3633-3656) per cell-step:
//   snow day, SWE > 0              the snow microclimate (variables of `outsel`; the others as in the last line)
//   snow day, no snow on the cell  the no-snow solver's value if the day is a no-snow day as well, else NA
//   other days                     untouched (the solver's value)
// One lane per (cell, day of the chunk).  m.rows / m.temp ... are the SUBSET series of the snow days (daymap[d]: the
// chunk day's place in it, -1: not a snow day); m.sTc ... m.sden the chunk's series, chunk-local steps.
struct MicroRingArgs {
    MicroArgs m;
    mcf::RingView ring;          // the slot's geometry (base unused)
    // the slot's held variables lie `vstride` doubles apart in the reference's order from `base0` (the tiled ring's
    // [tile][day][variable][block]): bit i of `held` = the plan holds output i, its base = base0 + popcount(held below i) * vstride
    double* base0;
    int64_t vstride;
    uint32_t held, sel;          // sel: gridmicrosnow1's `out` mask
    const int32_t *daymap, *nosnow;
    int32_t ndays;
};
// Shape (round 4): one lane per (cell, hour).  A workgroup is 64 consecutive cells x one day of the chunk (blockIdx.y: the
// step rows are wave-uniform scalar loads); wave w takes the hours w, w + 4, ..., w + 20.  What depends on the cell only —
// the raw rasters and what is derived from them (the slope / aspect sines and cosines, log(clump), three reciprocals), the
// day's mean ground-snow temperature — is made ONCE per workgroup-day, a quarter by each wave, into LDS, and read from there
// inside the hour loop: until round 3 a lane walked the 24 hours of its cell with all of it in registers (230 VGPRs, two
// waves per SIMD).
enum MicroCell : int { MC_HGT, MC_PAI, MC_PAIA, MC_LEAFD, MC_CLUMP, MC_LTRA, MC_LEAFDEN, MC_SVFA, MC_LNCLUMP, MC_IHGT, MC_ILEAFD,
                       MC_IPAI, MC_CS, MC_SS, MC_CA, MC_SA, MC_SLOPE, MC_MEAND, MC_SMAX, MC_TZD, MC_COUNT,
                       // array climate (k_microsnow_ring<true>): the cell's part of the sun position, its maximum temperature
                       MC_SINLAT = MC_COUNT, MC_COSLAT, MC_COSB, MC_SINB, MC_MXTC, MC_COUNT_AF };
static_assert((int)MC_HGT == (int)MQ_HGT && (int)MC_PAI == (int)MQ_PAI && (int)MC_PAIA == (int)MQ_PAIA && (int)MC_LEAFD == (int)MQ_LEAFD && (int)MC_CLUMP == (int)MQ_CLUMP &&
              (int)MC_LTRA == (int)MQ_LTRA && (int)MC_LEAFDEN == (int)MQ_LEAFDEN && (int)MC_SVFA == (int)MQ_SVFA && (int)MC_LNCLUMP == (int)MQ_LNCLUMP &&
              (int)MC_IHGT == (int)MQ_IHGT && (int)MC_ILEAFD == (int)MQ_ILEAFD && (int)MC_IPAI == (int)MQ_IPAI, "micro_above reads the table's first rows");
// The per-step table and the two day lists come in as `__restrict__` kernel arguments of their own (tb = q.m.mstep): read out of
// the by-value struct a pointer carries no noalias, the ring's stores might clobber the table for all the compiler knows, and
// every field of an hour's record — ~30 doubles — came through VECTOR loads of a uniform address into VGPR pairs.  With that
// and the wave index declared uniform (readfirstlane) they are scalar loads into SGPRs.
// AF (round 5): array climate — gridmicrosnow2 (cpp:5058-5214).  The step's weather is the lane's own (nine [N][T] series), the
// sun position the cell's (sun_at_cell), the albedo clock the cell's: `hs0` holds the hours since snowfall at every day start
// (k_microsnow_cell<true>) and the day's precipitation is staged in LDS, so that a lane finds its hour's clock by walking back
// through at most 23 LDS values instead of re-reading the series.  The table argument then carries the date rows (DateRow2).
// The one-shot entries mcf_gridmicrosnow1 / 2 run this kernel too, over a linear [steps][cells] view of their output arrays
// (RingView with cpb == 0: ring_pos(N, cell, hour) = hour N + cell) — the lane-per-(cell, day) kernel k_microsnow<AF> (197-201
// VGPRs, two waves per SIMD) is gone.
template <bool AF>
__global__ __launch_bounds__(256, AF ? 3 : MCF_MICRORING_WAVES) void k_microsnow_ring(MicroRingArgs q, const void* __restrict__ tbv,
                                                                                      const int32_t* __restrict__ tb_daymap,
                                                                                      const int32_t* __restrict__ tb_nosnow) {
    snow::snow_tables_init();
    const MicroStep* __restrict__ tb = (const MicroStep*)tbv;
    const DateRow2* __restrict__ td = (const DateRow2*)tbv;
    __shared__ double s_mc[AF ? MC_COUNT_AF : MC_COUNT][64];
    __shared__ double s_prec[AF ? 24 : 1][64];
    const MicroArgs& a = q.m;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t N = a.N;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    const int day = a.day0 + (int)blockIdx.y;    // uniform: the day's rows of the step tables are scalar loads
    const int sub = tb_daymap[day];
    if (sub < 0) return;
    const bool keep = tb_nosnow[day] != 0;        // the solver ran this day: snow-free cell-steps keep its values
    const double NA = na_real();
    const bool inr = c < N;
    const int64_t cc = inr ? c : N - 1;          // lanes past the raster read the last cell and write nothing
    const int k0 = day * 24;
    const int nh = min(24, a.tsteps - k0);       // (the one-shot entries: a last day may be short; its Tzd is NA, cpp:4700-4711)
    // ---- the workgroup-day's cell table
    if (AF) {
        if (wv == 0) {
            const SunCell sc = sun_cell(a.lats[cc], a.lons[cc]);
            s_mc[MC_SINLAT][lane] = sc.sinlat; s_mc[MC_COSLAT][lane] = sc.coslat; s_mc[MC_COSB][lane] = sc.cosB; s_mc[MC_SINB][lane] = sc.sinB;
            s_mc[MC_MXTC][lane] = a.mxtc[cc];
        }
        for (int h = wv; h < nh; h += 4) s_prec[h][lane] = a.precip[cc + N * (int64_t)(sub * 24 + h)];
    }
    if (wv == 0) {
        const double hgt = a.hgt[cc], pai = a.pai[cc], leafd = a.leafd[cc];
        s_mc[MC_HGT][lane] = hgt; s_mc[MC_PAI][lane] = pai; s_mc[MC_LEAFD][lane] = leafd;
        s_mc[MC_IHGT][lane] = gdiv(1.0, hgt); s_mc[MC_ILEAFD][lane] = gdiv(1.0, leafd); s_mc[MC_IPAI][lane] = gdiv(1.0, pai);
        s_mc[MC_PAIA][lane] = a.paia[cc]; s_mc[MC_LTRA][lane] = a.leaft[cc];
    } else if (wv == 1) {
        const double slope = a.slope[cc];
        s_mc[MC_SLOPE][lane] = slope;
        s_mc[MC_CS][lane] = cos(slope * kToRad); s_mc[MC_SS][lane] = sin(slope * kToRad);
        s_mc[MC_LEAFDEN][lane] = a.leafden[cc]; s_mc[MC_SVFA][lane] = a.skyview[cc];
    } else if (wv == 2) {
        const double aspect = a.aspect[cc], clump = a.clump[cc];
        s_mc[MC_CA][lane] = cos(aspect * kToRad); s_mc[MC_SA][lane] = sin(aspect * kToRad);
        s_mc[MC_CLUMP][lane] = clump;
        s_mc[MC_LNCLUMP][lane] = clump > 0.0 ? glog(clump) : 0.0;
    } else {
        // snowdayan's daily mean of the ground-snow temperature (its NA test looks at the FIRST step of the whole series,
        // cpp:4700; a chunk sees its own days only: the first step of the day — equal unless a cell's ground-snow
        // temperature turns NA part way, which gridmodelsnow never does)
        double Tzd = NA;
        if (nh == 24 && !isnan(a.sTg[cc + N * k0])) {
            double sumd = 0.0;
            for (int h = 0; h < 24; ++h) sumd += a.sTg[cc + N * (k0 + h)];
            Tzd = sumd / 24.0;
        }
        s_mc[MC_TZD][lane] = Tzd;
        s_mc[MC_MEAND][lane] = a.meanD[cc];
        s_mc[MC_SMAX][lane] = a.Smax ? a.Smax[cc] : 0.0;
    }
    __syncthreads();
    if (!inr) return;
    // the cell's place in the ring: its tile's block of this day, then the solver's lane position of (cell, hour)
    // (cpb == 0: the linear [step][cell] view of the one-shot entries' output arrays, RingView's convention)
    const int cpb = q.ring.cpb;
    const uint32_t tile = cpb ? (uint32_t)c / (uint32_t)cpb : 0u;
    const int cell = cpb ? (int)((uint32_t)c - tile * (uint32_t)cpb) : 0;
    const int64_t blk = cpb ? (int64_t)tile * q.ring.tile_stride + (int64_t)day * q.ring.day_stride : c + N * (int64_t)k0;
    for (int h = wv; h < nh; h += 4) {
        // (an opaque lane index per hour: the table is read where a value is used, not hoisted into registers in front of the loop;
        // an opaque block offset: or the ten variables' per-lane store addresses are kept across the loop — twenty registers)
        int li = lane;
        asm volatile("" : "+v"(li));
        int64_t bo = blk;
        asm volatile("" : "+v"(bo));
        // (opaque scalars too: or each variable's presence / selection masks, rank and base — 80 SGPRs — are hoisted in front of
        // the loop as invariants and spilled to VGPR lanes, a v_readlane per use; made at each store they are a few scalar
        // instructions beside the vector work)
        uint32_t held = q.held, selm = q.sel;
        int64_t vs = q.vstride;
        asm volatile("" : "+s"(held), "+s"(selm), "+s"(vs));
        auto has = [&](int i) { return (held >> i) & 1u; };
        auto put = [&](int i, int hh, double v) {
            const int rank = __builtin_popcount(held & ((1u << i) - 1u));
            q.base0[bo + rank * vs + (cpb ? (int64_t)mcf::ring_pos(cpb, cell, hh) : N * (int64_t)hh)] = v;
        };
        auto MC = [&](int f) { return s_mc[f][li]; };
        const double hgt = MC(MC_HGT);
        if (isnan(hgt)) {            // cpp:4988-4989: the cell is skipped — the blank template's NA unless the solver wrote it
            if (!keep) {
#pragma unroll
                for (int i = 0; i < MCF_NOUT; ++i) if (has(i)) put(i, h, NA);
            }
            continue;
        }
        const int64_t o = c + N * (k0 + h);          // chunk-local
        const int f = sub * 24 + h;                   // step of the snow-day subset series
        const double swe = a.swe[o];
        if (!(swe > 0.0)) {                           // cpp:4993
            if (!keep) {
#pragma unroll
                for (int i = 0; i < MCF_NOUT; ++i) if (has(i)) put(i, h, NA);
            }
            continue;
        }
        const double sdepg = a.sdepg[o], sTg = a.sTg[o];
        const double reqhgts = a.reqhgt - sdepg;
        // an output of this cell-step into the ring: gridmicrosnow1's `out` mask, the blank template's NA otherwise
        auto emit = [&](int i, double val) {
            if (!has(i)) return;
            if ((selm >> i) & 1u) put(i, h, val);
            else if (!keep) put(i, h, NA);
        };
        double Tz, tleaf, rh;
        if (reqhgts >= 0.0) {
            SiteK site;
            site.cS = MC(MC_CS); site.sS = MC(MC_SS); site.cA = MC(MC_CA); site.sA = MC(MC_SA); site.flat = MC(MC_SLOPE) == 0.0;
            MicroIn mi;
            mi.reqhgt = reqhgts; mi.zref = a.zref;
            mi.cell = &s_mc[0][li]; mi.cs = 64;           // (MC_HGT .. MC_IPAI are MQ_HGT .. MQ_IPAI)
            mi.Tg = sTg; mi.Tc = a.sTc[o]; mi.sden = a.sden[o]; mi.sdepg = sdepg;
            mi.sdepc = swe / mi.sden;
            if (AF) {
                const DateRow2 dr = td[f];
                SunCell sc;
                sc.sinlat = MC(MC_SINLAT); sc.coslat = MC(MC_COSLAT); sc.cosB = MC(MC_COSB); sc.sinB = MC(MC_SINB);
                int sindex;
                const SunT sun = sun_at_cell(dr.sindec, dr.cosdec, dr.cosA, dr.sinA, sc, sindex);
                mi.si = solar_index(sun, site, true);
                if (isnan(mi.si)) mi.si = sun.cosz;                        // cpp:5161
                mi.shadowmask = a.hor[(int64_t)sindex * N + c] > sun.tansa ? 0 : 1;
                mi.ws = a.wsa[(int64_t)dr.windex * N + c];
                const int64_t fo = c + N * (int64_t)f;                      // the lane's step of the (subset) weather series
                mi.tc = a.temp[fo]; mi.pk = a.pres[fo]; mi.u2 = a.windspeed[fo];
                mi.Rsw = a.swdown[fo]; mi.Rdif = a.difrad[fo]; mi.Rlw = a.lwdown[fo]; mi.umu = a.umu[fo];
                // the albedo clock (snowalbCpp, cpp:3733-3739): hours since the last snowfall — the day's start value, then back
                // through the day's precipitation to the lane's hour
                int hs = a.hs0[c + N * (int64_t)sub] + h;
                for (int j = h; j >= 1; --j)
                    if (s_prec[j][li] > 0) { hs = h - j; break; }
                mi.alb = snow_albedo(hs);
                mi.ialb = gdiv(1.0, mi.alb);
                const MicroMet mm = micro_met(mi.tc, a.relhum[fo], mi.pk, MC(MC_MXTC));
                const MicroOut mo = micro_above(mi, mm, sun, [&](int i, double val) { emit(i, val); return true; });
                Tz = mo.Tz; tleaf = mo.tleaf; rh = mo.rh;
            } else {
                const MicroStep& r = tb[f];
                const SunT sun = r.s;
                mi.si = solar_index(sun, site, true);
                if (isnan(mi.si)) mi.si = sun.cz;                          // cpp:5002
                mi.shadowmask = a.hor[(int64_t)r.sindex * N + c] > sun.tansa ? 0 : 1;
                mi.ws = a.wsa[(int64_t)r.windex * N + c];
                mi.tc = r.tc; mi.pk = r.pk; mi.u2 = r.u2;
                mi.Rsw = r.rsw; mi.Rdif = r.rdif; mi.Rlw = r.rlw; mi.umu = r.umu;
                mi.alb = r.alb; mi.ialb = r.ialb;
                // (wind speed and the five radiation streams go into the ring where micro_above has them final)
                const MicroOut mo = micro_above(mi, r.mm, sun, [&](int i, double val) { emit(i, val); return true; });
                Tz = mo.Tz; tleaf = mo.tleaf; rh = mo.rh;
            }
        } else {
            const double b = micro_below(reqhgts, MC(MC_MEAND), sTg, MC(MC_TZD), a.mat, a.hiy);
            Tz = b; tleaf = b; rh = 100.0;
            for (int i = 4; i < MCF_NOUT; ++i) emit(i, 0.0);
        }
        emit(0, Tz); emit(1, tleaf); emit(2, rh);
        emit(3, MC(MC_SMAX));
    }
}

// Round 5 shape, for the solver's 21-cell tiles: a workgroup is THREE tiles (63 consecutive cells, lane 63 idle) x EVERY snow
// day of the chunk; eight waves, wave w takes the hours w, w + 8, w + 16 of each day (the hour stays wave-uniform: the step
// record comes through scalar loads as before).  What that buys (profiles/r04_c4_aux_pmc_summary.json had 1.40 x the values
// written and 1.47 x the series read):
//   * the horizon and wind-shelter planes (24 + 8 values per cell; one of each was fetched per cell-STEP: 16 B beside the
//     40 B of snow series) and the cell table are staged in LDS ONCE per workgroup = once per chunk;
//   * every store is a whole 128-byte line.  Of a tile-day block's four lines per hour group (mcf_kernels.h ring_pos: three
//     hours x cells 0-15, then cells 16-20 of the three hours) the first three are one wave's sixteen consecutive lanes; the
//     fourth was written 40 B at a time by three different waves.  Its values now meet in LDS (s_tail) and are flushed behind
//     the day's barrier, a line per sixteen lanes.  A slot nobody produced (a snow-free cell-step of a day the solver ran as
//     well: its value stays) holds a sentinel and is not stored.
constexpr int kRtCells = 63, kRtWaves = MCF_MICRORING_WAVES == 3 ? 6 : 8;      // two workgroups per CU (56 KB of LDS each): 4 or 3 waves per SIMD
constexpr unsigned long long kTailEmpty = 0x7FF8A5A5DEAD0001ULL;      // (a NaN payload no arithmetic produces)
// BELOW: reqhgt < 0 with gridmicrosnow1's `out[c(1, 4)]` (the below-ground snow run) — every snow-covered cell-step is below the
// snow surface (reqhgt - groundsnowdepth < 0, cpp:5029-5051), so the lane needs meanD, the day's mean ground-snow temperature,
// sTg, sdepg, swe, Smax and nothing else: no direction planes, no site table, no step table, no sTc / sden, and only Tz and soilm
// ever carry a value — they alone go through s_tail; the other held variables are NA on a snow-only day, stored straight.  The
// values are the generic instantiation's: the same micro_below on the same operands.  LDS: 2 + 6 + 4 KB instead of 10 + 16 + 30 + 4.
// the row of the cell table a BELOW workgroup keeps
template <bool BELOW>
__device__ __forceinline__ constexpr int mc_row(int f) {
    return !BELOW ? f : f == MC_HGT ? 0 : f == MC_MEAND ? 1 : f == MC_SMAX ? 2 : 3;
}
template <bool BELOW>
__global__ __launch_bounds__(64 * kRtWaves, BELOW ? 8 : MCF_MICRORING_WAVES) void k_microsnow_tiles(MicroRingArgs q, const MicroStep* __restrict__ tb,
                                                                                                   const int32_t* __restrict__ tb_daymap,
                                                                                                   const int32_t* __restrict__ tb_nosnow) {
    snow::snow_tables_init();
    __shared__ double s_mc[BELOW ? 4 : MC_COUNT][64];
    __shared__ double s_hw[BELOW ? 1 : 32][BELOW ? 1 : 64];   // 24 horizon + 8 wind-shelter planes of the workgroup's cells
    __shared__ double s_tail[(BELOW ? 2 : MCF_NOUT) * 3 * 8 * 16];   // [held variable][tile][hour group][15 values + padding]
    constexpr int kTzdDays = 8;
    __shared__ double s_tzd[kTzdDays][64];            // the days' mean ground-snow temperatures (chunks of up to eight days)
    const MicroArgs& a = q.m;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t N = a.N;
    const int64_t c0 = (int64_t)blockIdx.x * kRtCells;     // uniform
    const bool inr = lane < kRtCells && c0 + lane < N;
    const double NA = na_real();
    {
        const int64_t cc = c0 + lane < N ? c0 + lane : N - 1;             // idle lanes read the last cell and write nothing
        // ---- once per workgroup: the cell table (a part by each of the first three waves) and the 32 direction planes
        if constexpr (BELOW) {
            if (wv == 0) {
                s_mc[mc_row<true>(MC_HGT)][lane] = a.hgt[cc];
            } else if (wv == 2) {
                s_mc[mc_row<true>(MC_MEAND)][lane] = a.meanD[cc];
                s_mc[mc_row<true>(MC_SMAX)][lane] = a.Smax ? a.Smax[cc] : 0.0;
            }
        } else if (wv == 0) {
            const double hgt = a.hgt[cc], pai = a.pai[cc], leafd = a.leafd[cc];
            s_mc[MC_HGT][lane] = hgt; s_mc[MC_PAI][lane] = pai; s_mc[MC_LEAFD][lane] = leafd;
            s_mc[MC_IHGT][lane] = gdiv(1.0, hgt); s_mc[MC_ILEAFD][lane] = gdiv(1.0, leafd); s_mc[MC_IPAI][lane] = gdiv(1.0, pai);
            s_mc[MC_PAIA][lane] = a.paia[cc]; s_mc[MC_LTRA][lane] = a.leaft[cc];
        } else if (wv == 1) {
            const double slope = a.slope[cc];
            s_mc[MC_SLOPE][lane] = slope;
            s_mc[MC_CS][lane] = cos(slope * kToRad); s_mc[MC_SS][lane] = sin(slope * kToRad);
            s_mc[MC_LEAFDEN][lane] = a.leafden[cc]; s_mc[MC_SVFA][lane] = a.skyview[cc];
        } else if (wv == 2) {
            const double aspect = a.aspect[cc], clump = a.clump[cc];
            s_mc[MC_CA][lane] = cos(aspect * kToRad); s_mc[MC_SA][lane] = sin(aspect * kToRad);
            s_mc[MC_CLUMP][lane] = clump;
            s_mc[MC_LNCLUMP][lane] = clump > 0.0 ? glog(clump) : 0.0;
            s_mc[MC_MEAND][lane] = a.meanD[cc];
            s_mc[MC_SMAX][lane] = a.Smax ? a.Smax[cc] : 0.0;
        } else {
            for (int p = wv - 3; p < 32; p += kRtWaves - 3) s_hw[p][lane] = p < 24 ? a.hor[(int64_t)p * N + cc] : a.wsa[(int64_t)(p - 24) * N + cc];
        }
        // ... and every snow day's mean ground-snow temperature (see k_microsnow_ring), a day per wave from the last wave down:
        // made per day by one wave in front of the day's barrier, its 24 loads were what the other seven waited for (round 5:
        // -1.9 % on configs[4]'s snow-day stage)
        if (q.ndays <= kTzdDays) {
            for (int day = kRtWaves - 1 - wv; day < q.ndays; day += kRtWaves) {
                if (tb_daymap[day] < 0) continue;
                const int64_t ci = c0 + lane < N ? lane : N - 1 - c0;
                if (a.tzd) {        // the snow model's kernel made them as it wrote the series (ModelArgs::tzd): one value, not 24
                    s_tzd[day][lane] = a.tzd[N * (int64_t)day + c0 + ci];
                    continue;
                }
                const double* tg = a.sTg + (N * (int64_t)(day * 24) + c0);
                double v[24];
#pragma unroll
                for (int h = 0; h < 24; ++h) v[h] = tg[ci + N * h];
                double Tzd = NA;
                if (!isnan(v[0])) {
                    double sumd = 0.0;
#pragma unroll
                    for (int h = 0; h < 24; ++h) sumd += v[h];
                    Tzd = sumd / 24.0;
                }
                s_tzd[day][lane] = Tzd;
            }
        }
    }
    // The lane's place: in the raster a uniform base + its lane number; in the tiled ring the block of its tile (uniform base of
    // the workgroup's first tile + tl tile strides) and, for cells 0-15, its column of the hour's line; cells 16-20 go to s_tail.
    // All as 32-bit byte offsets against uniform bases: no 64-bit vector address arithmetic per load or store.
    const int tl = lane / 21, cl = lane - 21 * tl;
    const bool direct = cl < 16;
    uint32_t rofs = (uint32_t)(tl * (int)q.ring.tile_stride + cl) * 8u;            // (a tile's days x variables x 512 doubles: < 2^29)
    const int tofs = tl * 128 + (cl - 16);
    uint32_t lofs = (uint32_t)lane * 8u;
    // the variables that go through s_tail: every held one, or (BELOW) Tz and soilm
    const int nheld = BELOW ? (int)((q.held & 1u) + ((q.held >> 3) & 1u)) : __builtin_popcount(q.held);
    for (int day = 0; day < q.ndays; ++day) {
        const int sub = tb_daymap[day];               // uniform: scalar loads
        if (sub < 0) continue;
        const bool keep = tb_nosnow[day] != 0;        // the solver ran this day: snow-free cell-steps keep its values
        const int k0 = day * 24;
        // the day's mean ground-snow temperature (see k_microsnow_ring) by the last wave; the tails' slots emptied by the threads
        // that flushed them (same thread, same slots: ordered without a barrier)
        if (q.ndays > kTzdDays && wv == kRtWaves - 1) {
            const double* tg = a.sTg + (N * k0 + c0);
            const int64_t cc = c0 + lane < N ? lane : N - 1 - c0;
            double Tzd = NA;
            if (!isnan(tg[cc])) {
                double sumd = 0.0;
                for (int h = 0; h < 24; ++h) sumd += tg[cc + N * h];
                Tzd = sumd / 24.0;
            }
            s_mc[mc_row<BELOW>(MC_TZD)][lane] = Tzd;
        }
        const double* const tzd_row = q.ndays <= kTzdDays ? &s_tzd[day][0] : &s_mc[mc_row<BELOW>(MC_TZD)][0];
        for (int e = tid; e < nheld * 384; e += 64 * kRtWaves) reinterpret_cast<unsigned long long*>(s_tail)[e] = kTailEmpty;
        __syncthreads();
        // the workgroup's first tile's block of this day (uniform)
        double* const dayblk = q.base0 + ((int64_t)blockIdx.x * 3) * q.ring.tile_stride + (int64_t)day * q.ring.day_stride;
        if (inr) {
            for (int h = wv; h < 24; h += kRtWaves) {
                int li = lane;
                asm volatile("" : "+v"(li));
                uint32_t held = q.held, selm = q.sel;
                int64_t vs = q.vstride;
                asm volatile("" : "+s"(held), "+s"(selm), "+s"(vs));
                auto has = [&](int i) { return (held >> i) & 1u; };
                const int hg = h / 3, hm = h - 3 * hg;               // uniform
                auto put = [&](int i, double v) {
                    const int rank = __builtin_popcount(held & ((1u << i) - 1u));
                    if (direct) {
                        asm("" : "+v"(rofs));       // (keeps the offset's zero-extension in the store's own block: mcf_kernels.hip `put`)
                        *(double*)((char*)(dayblk + (rank * vs + (64 * hg + 16 * hm))) + rofs) = v;
                    } else if (!BELOW) {
                        s_tail[(rank * 384 + hg * 16 + 5 * hm) + tofs] = v;
                    } else if (i == 0 || i == 3) {
                        s_tail[((i == 0 ? 0 : (int)(held & 1u)) * 384 + hg * 16 + 5 * hm) + tofs] = v;
                    } else {      // (NA on a snow-only day: the fourth line's place, where the flush puts a staged value)
                        dayblk[(int64_t)tl * q.ring.tile_stride + rank * vs + 64 * hg + 48 + 5 * hm + (cl - 16)] = v;
                    }
                };
                auto MC = [&](int f) { return s_mc[mc_row<BELOW>(f)][li]; };
                const double hgt = MC(MC_HGT);
                if (isnan(hgt)) {            // cpp:4988-4989
                    if (!keep) {
#pragma unroll
                        for (int i = 0; i < MCF_NOUT; ++i) if (has(i)) put(i, NA);
                    }
                    continue;
                }
                // the step's plane of each snow series (uniform) + the lane
                const int64_t po = N * (k0 + h) + c0;
                auto ser = [&](const double* p) {
                    asm("" : "+v"(lofs));
                    return *(const double*)((const char*)(p + po) + lofs);
                };
                const int f = sub * 24 + h;                   // step of the snow-day subset series
                const double swe = ser(a.swe);
                if (!(swe > 0.0)) {                           // cpp:4993
                    if (!keep) {
#pragma unroll
                        for (int i = 0; i < MCF_NOUT; ++i) if (has(i)) put(i, NA);
                    }
                    continue;
                }
                const double sdepg = ser(a.sdepg), sTg = ser(a.sTg);
                const double reqhgts = a.reqhgt - sdepg;
                auto emit = [&](int i, double val) {
                    if (!has(i)) return;
                    if ((selm >> i) & 1u) put(i, val);
                    else if (!keep) put(i, NA);
                };
                if constexpr (BELOW) {
                    const double b = micro_below(reqhgts, MC(MC_MEAND), sTg, tzd_row[li], a.mat, a.hiy);
#pragma unroll
                    for (int i = 0; i < MCF_NOUT; ++i) emit(i, i == 0 ? b : MC(MC_SMAX));      // (sel holds Tz and soilm only)
                    continue;
                }
                double Tz, tleaf, rh;
                if (reqhgts >= 0.0) {
                    const MicroStep& r = tb[f];
                    const SunT sun = r.s;
                    SiteK site;
                    site.cS = MC(MC_CS); site.sS = MC(MC_SS); site.cA = MC(MC_CA); site.sA = MC(MC_SA); site.flat = MC(MC_SLOPE) == 0.0;
                    MicroIn mi;
                    mi.si = solar_index(sun, site, true);
                    if (isnan(mi.si)) mi.si = sun.cz;                          // cpp:5002
                    mi.shadowmask = s_hw[r.sindex][li] > sun.tansa ? 0 : 1;
                    mi.ws = s_hw[24 + r.windex][li];
                    mi.reqhgt = reqhgts; mi.zref = a.zref;
                    mi.tc = r.tc; mi.pk = r.pk; mi.u2 = r.u2;
                    mi.Rsw = r.rsw; mi.Rdif = r.rdif; mi.Rlw = r.rlw; mi.umu = r.umu;
                    mi.cell = &s_mc[0][li]; mi.cs = 64;
                    mi.Tg = sTg; mi.Tc = ser(a.sTc); mi.sden = ser(a.sden); mi.sdepg = sdepg;
                    mi.sdepc = swe / mi.sden;
                    mi.alb = r.alb; mi.ialb = r.ialb;
                    const MicroOut mo = micro_above(mi, r.mm, sun, [&](int i, double val) { emit(i, val); return true; });
                    Tz = mo.Tz; tleaf = mo.tleaf; rh = mo.rh;
                } else {
                    const double b = micro_below(reqhgts, MC(MC_MEAND), sTg, tzd_row[li], a.mat, a.hiy);
                    Tz = b; tleaf = b; rh = 100.0;
                    for (int i = 4; i < MCF_NOUT; ++i) emit(i, 0.0);
                }
                emit(0, Tz); emit(1, tleaf); emit(2, rh);
                emit(3, MC(MC_SMAX));
            }
        }
        __syncthreads();
        // flush: element e = (rank * 3 + tile) * 128 + hour group * 16 + slot -> the fourth line of that block's hour group
        for (int e = tid; e < nheld * 384; e += 64 * kRtWaves) {
            const unsigned long long bits = reinterpret_cast<const unsigned long long*>(s_tail)[e];
            if (bits == kTailEmpty) continue;
            const int slot = e & 15, g = (e >> 4) & 7, rt = e >> 7, trank = rt / 3, t3 = rt - 3 * trank;
            // the staged variable's place among the held ones (BELOW: Tz first if held, then soilm)
            const int rank = !BELOW ? trank : (trank == 0 && (q.held & 1u)) ? 0 : __builtin_popcount(q.held & 7u);
            dayblk[(int64_t)t3 * q.ring.tile_stride + rank * q.vstride + 64 * g + 48 + slot] = __longlong_as_double((long long)bits);
        }
    }
}

// ---- .snowmodel1's chunk loop (R/internal.R "int:" 2553-2617) ---------------------------------------
// albedo clock restarted at every chunk start: each gridmodelsnow1 call runs snowalbCpp on its own slice
__global__ void k_snow_alb_chunks(StepRow* rows, const double* precip, int tsteps, int chunk, int nchunks) {
    snow::snow_tables_init();
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const int k0 = c * chunk, k1 = min(tsteps, k0 + chunk);
    int hs = 0;
    for (int k = k0; k < k1; ++k) {
        if (k > k0) hs = precip[k] > 0 ? 0 : hs + 1;
        rows[k].m.alb = snow_albedo(hs);
        rows[k].m.ialb = gdiv(1.0, rows[k].m.alb);
    }
}
// dtms = dtm + ground snow depth (int:2562, 2614); NaN where the dtm is NA
__global__ __launch_bounds__(256) void k_add_snow(const double* __restrict__ dtm, const double* __restrict__ dep,
                                                  double scale, int64_t N, double* __restrict__ dtms) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < N) dtms[c] = dtm[c] + dep[c] * scale;
}
// mask(x, dtm): NA where the dtm is NA (int:2568, 2571)
__global__ __launch_bounds__(256) void k_mask2(const double* __restrict__ dtm, int64_t N, double* __restrict__ a,
                                               double* __restrict__ b) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < N && isnan(dtm[c])) { a[c] = na_real(); b[c] = na_real(); }
}
// deterministic (sum, count) of the non-NaN entries of x: kSumParts workgroups reduce fixed strided subsets with a
// fixed-shape tree, workgroup 0 of a second launch adds the partials in order (same result on every run)
constexpr int kSumParts = 128;
__global__ __launch_bounds__(256) void k_sumcount_part(const double* __restrict__ x, int64_t N, double* __restrict__ ws) {
    __shared__ double ss[256];
    __shared__ double sc[256];
    double s = 0.0, n = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)kSumParts * 256) {
        const double v = x[i];
        if (!isnan(v)) { s += v; n += 1.0; }
    }
    ss[threadIdx.x] = s; sc[threadIdx.x] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { ss[threadIdx.x] += ss[threadIdx.x + w]; sc[threadIdx.x] += sc[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { ws[2 * blockIdx.x] = ss[0]; ws[2 * blockIdx.x + 1] = sc[0]; }
}
__global__ void k_sumcount_fin(const double* __restrict__ ws, double* __restrict__ out2) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0, n = 0.0;
    for (int p = 0; p < kSumParts; ++p) { s += ws[2 * p]; n += ws[2 * p + 1]; }
    out2[0] = s; out2[1] = n;
}
// ws: 2 * kSumParts doubles of scratch
void launch_sumcount(const double* x, int64_t N, double* ws, double* out2, hipStream_t stream = nullptr) {
    hipLaunchKernelGGL(k_sumcount_part, dim3(kSumParts), dim3(256), 0, stream, x, N, ws);
    hipLaunchKernelGGL(k_sumcount_fin, dim3(1), dim3(64), 0, stream, ws, out2);
}
// .tpicalc (int:2471-2485) on a row block of the raster.  `z` is the block's surface (dtm + ground snow) with
// `hn` halo rows above: row b of z is global row row0 - hn + b; RB rows in all.
struct TpiGeo {
    int64_t rows, cols, RB, hn, row0, rows_total;
    int af;
    int64_t I0, nI, nJ, NItot;   // coarse rows [I0, I0 + nI) are held, NItot in the whole raster
};
// coarse part: aggregate(dtm, af, na.rm = TRUE) — af x af block means from the raster's top-left corner
// over the non-NA cells
__global__ __launch_bounds__(256) void k_tpi_coarse(const double* __restrict__ z, TpiGeo g, double* __restrict__ cm) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= g.nI * g.nJ) return;
    const int64_t Il = q % g.nI, J = q / g.nI;
    const int64_t ra = (g.I0 + Il) * g.af, rb = min(ra + g.af, g.rows_total), ca = J * g.af, cb = min(ca + g.af, g.cols);
    double s = 0.0, n = 0.0;
    for (int64_t c = ca; c < cb; ++c)
        for (int64_t r = ra; r < rb; ++r) {
            const double v = z[(r - (g.row0 - g.hn)) + g.RB * c];
            if (!isnan(v)) { s += v; n += 1.0; }
        }
    cm[q] = s / n;   // 0/0 = NaN for an all-NA block
}
// fine part: resample (bilinear between block centres, clamped) or the raster mean, then
// tpic = exp((dtmc - dtm) * tfact) with its two clamps (`tpic[tpic < 0.05] <- 0.1` sic)
__global__ __launch_bounds__(256) void k_tpi_fine(const double* __restrict__ z, TpiGeo g, const double* __restrict__ cm,
                                                  double surface_mean, double tfact, double* __restrict__ tpic) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= g.rows * g.cols) return;
    const int64_t r = cell % g.rows, c = cell / g.rows;
    const double z0 = z[(g.hn + r) + g.RB * c];
    double zc;
    if (cm) {
        const int af = g.af;
        const double tr = ((double)(g.row0 + r) - (af - 1) / 2.0) / af, tcc = ((double)c - (af - 1) / 2.0) / af;
        const int64_t i0 = (int64_t)floor(tr), j0 = (int64_t)floor(tcc);
        const double wr = tr - (double)i0, wc = tcc - (double)j0;
        const int64_t ia = min(max(i0, (int64_t)0), g.NItot - 1) - g.I0, ib = min(max(i0 + 1, (int64_t)0), g.NItot - 1) - g.I0;
        const int64_t ja = min(max(j0, (int64_t)0), g.nJ - 1), jb = min(max(j0 + 1, (int64_t)0), g.nJ - 1);
        const double top = cm[ia + g.nI * ja] * (1 - wc) + cm[ia + g.nI * jb] * wc;
        const double bot = cm[ib + g.nI * ja] * (1 - wc) + cm[ib + g.nI * jb] * wc;
        zc = top * (1 - wr) + bot * wr;
    } else {
        zc = z0 * 0 + surface_mean;   // dtm * 0 + mean(dtm, na.rm = TRUE)
    }
    double t = exp((zc - z0) * tfact);
    if (t < 0.05) t = 0.1;
    if (t > 10) t = 10;
    tpic[cell] = t;
}
// redistribution of the chunk's snow-depth changes and hand-over to the next chunk (int:2589-2614);
// sdepc / sdepg are overwritten by totalSWE / groundsnowdepth
// applycpp3 (cpp:5553-5588): `parts` workgroups per time step stream fixed strided subsets of the cells (coalesced),
// fixed-shape tree in LDS, partials combined in order by a second kernel -> deterministic; NaN cells are skipped
__device__ __forceinline__ double apply3_combine(int fun, double a, double b) {
    if (fun < 2) return a + b;
    if (fun == 2) return b > a ? b : a;
    return b < a ? b : a;
}
__global__ __launch_bounds__(256) void k_apply3_part(const double* __restrict__ a, int64_t N, int fun, int parts,
                                                     double* __restrict__ ws /* [tsteps][parts][2] */) {
    __shared__ double sv[256];
    __shared__ double sn[256];
    const int64_t k = blockIdx.y;
    const double* x = a + k * N;
    double v = fun == 2 ? -INFINITY : (fun == 3 ? INFINITY : 0.0), n = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)parts * 256) {
        const double q = x[i];
        if (isnan(q)) continue;
        n += 1.0;
        v = apply3_combine(fun, v, q);
    }
    sv[threadIdx.x] = v; sn[threadIdx.x] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sv[threadIdx.x] = apply3_combine(fun, sv[threadIdx.x], sv[threadIdx.x + w]);
            sn[threadIdx.x] += sn[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ws[2 * (k * parts + blockIdx.x)] = sv[0];
        ws[2 * (k * parts + blockIdx.x) + 1] = sn[0];
    }
}
// max AND min of every step in ONE pass over the series (the snow plan asks for both of every chunk: snowdaysfun's operands).
// Each of the two is folded over the same cells in the same order as k_apply3_part folds it alone — same bits.
__global__ __launch_bounds__(256) void k_apply3_minmax_part(const double* __restrict__ a, int64_t N, int parts,
                                                            double* __restrict__ ws_max, double* __restrict__ ws_min) {
    __shared__ double smx[256];
    __shared__ double smn[256];
    __shared__ double sn[256];
    const int64_t k = blockIdx.y;
    const double* x = a + k * N;
    double mx = -INFINITY, mn = INFINITY, n = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)parts * 256) {
        const double q = x[i];
        if (isnan(q)) continue;
        n += 1.0;
        mx = apply3_combine(2, mx, q);
        mn = apply3_combine(3, mn, q);
    }
    smx[threadIdx.x] = mx; smn[threadIdx.x] = mn; sn[threadIdx.x] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            smx[threadIdx.x] = apply3_combine(2, smx[threadIdx.x], smx[threadIdx.x + w]);
            smn[threadIdx.x] = apply3_combine(3, smn[threadIdx.x], smn[threadIdx.x + w]);
            sn[threadIdx.x] += sn[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t o = 2 * (k * parts + blockIdx.x);
        ws_max[o] = smx[0]; ws_max[o + 1] = sn[0];
        ws_min[o] = smn[0]; ws_min[o + 1] = sn[0];
    }
}
__global__ __launch_bounds__(256) void k_apply3_fin(const double* __restrict__ ws, int64_t tsteps, int fun, int parts,
                                                    double* __restrict__ result, double* __restrict__ count) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= tsteps) return;
    double v = fun == 2 ? -INFINITY : (fun == 3 ? INFINITY : 0.0), n = 0.0;
    for (int p = 0; p < parts; ++p) {
        v = apply3_combine(fun, v, ws[2 * (k * parts + p)]);
        n += ws[2 * (k * parts + p) + 1];
    }
    if (fun == 0) v = n > 0 ? v / n : NAN;
    result[k] = v;
    if (count) count[k] = n;
}

// ---- host side -------------------------------------------------------------------------------------
struct Events {   // timing events released on every exit path
    std::vector<hipEvent_t> e;
    ~Events() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }
    hipError_t make(int n) {
        for (int i = 0; i < n; ++i) {
            hipEvent_t x;
            hipError_t r = hipEventCreate(&x);
            if (r != hipSuccess) return r;
            e.push_back(x);
        }
        return hipSuccess;
    }
};
// An MCF_TIMING span on the null stream: end() adds the device time since the last begin() to a counter of milliseconds and
// waits for it.  MCF_TIMING unset (or `wanted` false): no event, no synchronise.
struct TimedSpan {
    Events evs;
    const bool on;
    explicit TimedSpan(bool wanted = true) : on(wanted && getenv("MCF_TIMING") != nullptr) {}
    hipError_t begin() {
        if (!on) return hipSuccess;
        if (evs.e.empty())
            if (const hipError_t r = evs.make(2)) return r;
        return hipEventRecord(evs.e[0], nullptr);
    }
    hipError_t end(double* ms_sum) {
        if (!on) return hipSuccess;
        hipError_t r;
        if ((r = hipEventRecord(evs.e[1], nullptr)) || (r = hipEventSynchronize(evs.e[1]))) return r;
        float ms = 0;
        r = hipEventElapsedTime(&ms, evs.e[0], evs.e[1]);
        *ms_sum += ms;
        return r;
    }
};

// ---- the array groups of the snow entries, each listed ONCE: every upload, null check, row gather and copy walks these.
// f(the caller's pointer — a reference: a block's copy of the inputs is re-pointed through it —, the kernel argument it
// becomes, ..., the R-side name).  A listing's order is the order in which a null array is reported.
// gridmodelsnow's rasters.  terrain: given to the one-shot entries, derived on the device per chunk by the snow plan.
template <class In, class F>
void each_model_raster(In& in, F&& f) {   // f(pointer, member, layers, terrain, name)
    f(in.vegp.pai, &ModelArgs::pai, 1, false, "vegp$pai"); f(in.vegp.hgt, &ModelArgs::hgt, 1, false, "vegp$hgt");
    f(in.vegp.leaft, &ModelArgs::leaft, 1, false, "vegp$leaft"); f(in.vegp.clump, &ModelArgs::clump, 1, false, "vegp$clump");
    f(in.other.slope, &ModelArgs::slope, 1, true, "other$slope"); f(in.other.aspect, &ModelArgs::aspect, 1, true, "other$aspect");
    f(in.other.skyview, &ModelArgs::skyview, 1, true, "other$skyview"); f(in.other.wsa, &ModelArgs::wsa, 8, true, "other$wsa");
    f(in.other.hor, &ModelArgs::hor, 24, true, "other$hor"); f(in.other.isnowdc, &ModelArgs::isnowdc, 1, false, "other$isnowdc");
    f(in.other.isnowdg, &ModelArgs::isnowdg, 1, false, "other$isnowdg"); f(in.other.isnowac, &ModelArgs::isnowac, 1, false, "other$isnowac");
    f(in.other.isnowag, &ModelArgs::isnowag, 1, false, "other$isnowag");
}
// gridmicrosnow's static rasters.  required = false: Smax, read only where soilm is asked for.
template <class In, class F>
void each_micro_raster(In& in, F&& f) {   // f(pointer, member, layers, required, name)
    f(in.vegp.pai, &MicroArgs::pai, 1, true, "vegp$pai"); f(in.vegp.hgt, &MicroArgs::hgt, 1, true, "vegp$hgt");
    f(in.vegp.leaft, &MicroArgs::leaft, 1, true, "vegp$leaft"); f(in.vegp.clump, &MicroArgs::clump, 1, true, "vegp$clump");
    f(in.vegp.paia, &MicroArgs::paia, 1, true, "vegp$paia"); f(in.vegp.leafd, &MicroArgs::leafd, 1, true, "vegp$leafd");
    f(in.vegp.leafden, &MicroArgs::leafden, 1, true, "vegp$leafden"); f(in.other.slope, &MicroArgs::slope, 1, true, "other$slope");
    f(in.other.aspect, &MicroArgs::aspect, 1, true, "other$aspect"); f(in.other.skyview, &MicroArgs::skyview, 1, true, "other$skyview");
    f(in.other.wsa, &MicroArgs::wsa, 8, true, "other$wsa"); f(in.other.hor, &MicroArgs::hor, 24, true, "other$hor");
    f(in.other.Smax, &MicroArgs::Smax, 1, false, "other$Smax");
}
// the time of every step
template <class In, class F>
void each_obstime(In& in, F&& f) {   // f(pointer, the step tables' argument, name)
    f(in.obstime.year, &StepArgs::year, "obstime$year"); f(in.obstime.month, &StepArgs::month, "obstime$month");
    f(in.obstime.day, &StepArgs::day, "obstime$day"); f(in.obstime.hour, &StepArgs::hour, "obstime$hour");
}
// the snow model's thirteen series: [T] with data.frame weather (they go into the step table), [N][T] with array weather
template <class In, class F>
void each_model_series(In& in, F&& f) {   // f(pointer, the step tables' argument, the model's, name)
    using S = StepArgs; using M = ModelArgs;
    f(in.clim.temp, &S::temp, &M::temp, "climdata$temp"); f(in.clim.relhum, &S::relhum, &M::relhum, "climdata$relhum");
    f(in.clim.pres, &S::pres, &M::pres, "climdata$pres"); f(in.clim.swdown, &S::swdown, &M::swdown, "climdata$swdown");
    f(in.clim.difrad, &S::difrad, &M::difrad, "climdata$difrad"); f(in.clim.lwdown, &S::lwdown, &M::lwdown, "climdata$lwdown");
    f(in.clim.windspeed, &S::windspeed, &M::windspeed, "climdata$windspeed"); f(in.clim.precip, &S::precip, &M::precip, "climdata$precip");
    f(in.pointm.Gp, &S::Gp, &M::Gp, "pointm$Gp"); f(in.pointm.Tc, &S::Tcp, &M::Tcp, "pointm$Tc");
    f(in.pointm.RswabsG, &S::RswabsG, &M::RswabsG, "pointm$RswabsG"); f(in.pointm.RlwabsG, &S::RlwabsG, &M::RlwabsG, "pointm$RlwabsG");
    f(in.pointm.umu, &S::umu, &M::umu, "pointm$umu");
}
// gridmicrosnow's nine series, [T] or [N][T], and the wind direction: [T] in either geometry, the step tables' alone (no member)
constexpr int kMicroSeries = 9;
template <class In, class F>
void each_micro_series(In& in, F&& f) {   // f(pointer, member or null, name)
    f(in.clim.temp, &MicroArgs::temp, "climdata$temp"); f(in.clim.relhum, &MicroArgs::relhum, "climdata$relhum");
    f(in.clim.pres, &MicroArgs::pres, "climdata$pres"); f(in.clim.swdown, &MicroArgs::swdown, "climdata$swdown");
    f(in.clim.difrad, &MicroArgs::difrad, "climdata$difrad"); f(in.clim.lwdown, &MicroArgs::lwdown, "climdata$lwdown");
    f(in.clim.windspeed, &MicroArgs::windspeed, "climdata$windspeed"); f(in.clim.winddir, (const double* MicroArgs::*)nullptr, "climdata$winddir");
    f(in.clim.precip, &MicroArgs::precip, "climdata$precip"); f(in.clim.umu, &MicroArgs::umu, "climdata$umu");
}
// the sites of array weather
template <class A>
int up_sites(mcf::DevOwner& b, A& a, const mcf_snow_inputs* in, int64_t N) {
    if (const int rc = b.up(&a.lats, in->other.lats, N, "other$lats")) return rc;
    return b.up(&a.lons, in->other.lons, N, "other$lons");
}

int hours_in_year(int y) { return (y % 4 == 0 && (y % 100 != 0 || y % 400 == 0)) ? 366 * 24 : 365 * 24; }   // cpp:4984

int pick_device(int32_t device) {
    if (const int rc = mcf::check_device(device)) return rc;
    if (hipSetDevice(device) != hipSuccess) return mcf::api_fail(MCF_ERR_HIP, "hipSetDevice failed");
    return MCF_OK;
}
int check_room(int64_t need) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return MCF_OK;
    if ((double)need > 0.95 * (double)fr) {
        char m[200];
        snprintf(m, sizeof m, "snow call needs %.2f GB of device memory, %.2f GB free; split the time range",
                 need / 1e9, fr / 1e9);
        return mcf::api_fail(MCF_ERR_NOMEM, m);
    }
    return MCF_OK;
}

void snow_density_params(int snowenv, double sdp[4]) {   // snowdenp, cpp:3741-3749
    static const double tab[5][4] = {{0.5975, 0.2237, 0.0012, 0.0038},
                                     {0.5979, 0.2578, 0.001, 0.0038},
                                     {0.594, 0.2332, 0.0016, 0.0031},
                                     {0.363, 0.2425, 0.0029, 0.0049},
                                     {0.217, 0.217, 0.0, 0.0}};
    if (snowenv < 0 || snowenv > 4) snowenv = 0;
    for (int i = 0; i < 4; ++i) sdp[i] = tab[snowenv][i];
}

int common_checks(const mcf_snow_inputs* in) {
    if (!in) return mcf::api_fail(MCF_ERR_ARG, "null snow inputs");
    if (in->rows <= 0 || in->cols <= 0 || in->tsteps <= 0) return mcf::api_fail(MCF_ERR_ARG, "bad snow dimensions");
    if (in->tsteps > (1 << 30)) return mcf::api_fail(MCF_ERR_ARG, "tsteps too large");
    // (the snow kernels address a step's slab as uniform base + 32-bit lane byte offset)
    if (in->rows * in->cols >= ((int64_t)1 << 29)) return mcf::api_fail(MCF_ERR_ARG, "at most 2^29 - 1 cells per snow call (row-tile larger rasters)");
    if (!in->obstime.year || !in->obstime.month || !in->obstime.day || !in->obstime.hour)
        return mcf::api_fail(MCF_ERR_ARG, "null obstime");
    return MCF_OK;
}

// the time-class device tables of both entry points: step rows + the series' maximum temperature, or (array weather) date rows
struct StepTables {
    const StepRow* rows = nullptr;
    const DateRow2* dates = nullptr;
    const double* mxtc1 = nullptr;
};
int build_step_tables(mcf::DevOwner& b, const mcf_snow_inputs* in, bool af, bool model, bool degrees, StepTables* tabs) {
    const int T = (int)in->tsteps;
    int rc = MCF_OK;
    StepArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.tsteps = T;
    each_obstime(*in, [&](auto* host, auto member, const char* name) { if (!rc) rc = b.up(&(sa.*member), host, T, name); });
    if (!rc) rc = b.up(&sa.winddir, in->clim.winddir, T, "climdata$winddir");
    if (rc) return rc;
    sa.lat = in->other.lat; sa.lon = in->other.lon;
    sa.degrees = degrees ? 1 : 0;
    const unsigned grid = (unsigned)((T + 255) / 256);
    *tabs = StepTables();
    if (af) {
        if ((rc = b.make(&sa.dates, T))) return rc;
        hipLaunchKernelGGL(k_snow_dates, dim3(grid), dim3(256), 0, nullptr, sa);
        tabs->dates = sa.dates;
    } else {
        // what the albedo scan reads, then (the snow model) the rest of the listing
        if ((rc = b.up(&sa.temp, in->clim.temp, T, "climdata$temp"))) return rc;
        if ((rc = b.up(&sa.precip, in->clim.precip, T, "climdata$precip"))) return rc;
        if (model)
            each_model_series(*in, [&](auto* host, auto member, auto, const char* name) {
                if (!rc && !(sa.*member)) rc = b.up(&(sa.*member), host, T, name);
            });
        if (rc) return rc;
        if ((rc = b.make(&sa.rows, T))) return rc;
        if ((rc = b.make(&sa.mxtc, 1))) return rc;
        hipLaunchKernelGGL(k_snow_steps, dim3(grid), dim3(256), 0, nullptr, sa);
        if (model && T / 24 > 0)
            hipLaunchKernelGGL(k_snow_days, dim3((unsigned)((T / 24 + 63) / 64)), dim3(64), 0, nullptr, sa.rows, T);
        hipLaunchKernelGGL(k_snow_alb, dim3(1), dim3(64), 0, nullptr, sa.rows, sa.precip, sa.temp, T, sa.mxtc);
        tabs->rows = sa.rows;
        tabs->mxtc1 = sa.mxtc;
    }
    if (hipGetLastError() != hipSuccess) return mcf::api_fail(MCF_ERR_HIP, "snow table kernels failed to launch");
    return MCF_OK;
}

// data.frame weather: every step's weather-only terms and the ring kernel's step records, from the series and step rows in `a`
int build_micro_steps(mcf::DevOwner& b, MicroArgs& a) {
    const int T = a.tsteps;
    int rc;
    MicroMet* mm;
    if ((rc = b.make(&mm, T))) return rc;
    hipLaunchKernelGGL(k_micro_steps, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, nullptr, a.temp, a.relhum, a.pres, a.mxtc1, T, mm);
    a.mmet = mm;
    MicroStep* ms;
    if ((rc = b.make(&ms, T))) return rc;
    hipLaunchKernelGGL(k_micro_pack, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, nullptr, a.rows, a.mmet, a.temp, a.pres, a.windspeed,
                       a.swdown, a.difrad, a.lwdown, a.umu, T, ms);
    a.mstep = ms;
    return MCF_OK;
}

int run_snowmodel(const mcf_snow_inputs* in, mcf_snowmodel_out* out, int32_t device, bool af) {
    int rc;
    if ((rc = common_checks(in))) return rc;
    if (!out) return mcf::api_fail(MCF_ERR_ARG, "null snow outputs");
    if ((in->array_forcing != 0) != af) return mcf::api_fail(MCF_ERR_ARG, "array_forcing does not match the entry point");
    if ((rc = pick_device(device))) return rc;
    const int64_t N = in->rows * in->cols;
    const int T = (int)in->tsteps;
    const int64_t NT = N * T;
    int nout3 = 0;
    double* host3[5] = {out->Tc, out->Tg, out->sdepc, out->sdepg, out->sden};
    for (double* p : host3) nout3 += p != nullptr;
    if ((rc = check_room((af ? 13 * NT : 0) * 8 + (int64_t)nout3 * NT * 8 + 60 * N * 8))) return rc;
    mcf::DevOwner b;
    ModelArgs a;
    memset(&a, 0, sizeof a);
    a.N = N; a.tsteps = T; a.zref = in->other.zref;
    snow_density_params(in->snowenv, a.sdp);
    each_model_raster(*in, [&](auto* host, auto member, int layers, bool, const char* name) {
        if (!rc) rc = b.up(&(a.*member), host, layers * N, name);
    });
    if (rc) return rc;
    StepTables tabs;
    if ((rc = build_step_tables(b, in, af, true, !af, &tabs))) return rc;
    a.rows = tabs.rows; a.dates = tabs.dates;
    if (af) {
        if ((rc = up_sites(b, a, in, N))) return rc;
        each_model_series(*in, [&](auto* host, auto, auto member, const char* name) { if (!rc) rc = b.up(&(a.*member), host, NT, name); });
        if (rc) return rc;
    }
    double** dev3[5] = {&a.Tc, &a.Tg, &a.sdepc, &a.sdepg, &a.sden};
    for (int v = 0; v < 5; ++v)
        if (host3[v] && (rc = b.make(dev3[v], NT))) return rc;
    double* host2[4] = {out->agec, out->ageg, out->meltc, out->meltg};
    double** dev2[4] = {&a.agec, &a.ageg, &a.meltc, &a.meltg};
    for (int v = 0; v < 4; ++v)
        if (host2[v] && (rc = b.make(dev2[v], N))) return rc;
    const unsigned grid = (unsigned)((N + 255) / 256);
    TimedSpan span;
    double ms = 0;
    HIP_TRY(span.begin());
    if (af) hipLaunchKernelGGL(k_snowmodel<true>, dim3(grid), dim3(256), 0, nullptr, a, a.rows, a.dates);
    else hipLaunchKernelGGL(k_snowmodel<false>, dim3(grid), dim3(256), 0, nullptr, a, a.rows, a.dates);
    HIP_TRY(hipGetLastError());
    HIP_TRY(span.end(&ms));
    if (span.on)
        fprintf(stderr, "[mcf] k_snowmodel<%d>: %lld cells x %d steps in %.3f ms (%.3e cell-steps/s)\n", (int)af,
                (long long)N, T, ms, (double)NT / (ms * 1e-3));
    mcf::ToHost dl;
    for (int v = 0; v < 5; ++v)
        if (host3[v]) HIP_TRY(dl.dense(host3[v], *dev3[v], (size_t)NT * 8));
    for (int v = 0; v < 4; ++v)
        if (host2[v]) HIP_TRY(hipMemcpy(host2[v], *dev2[v], (size_t)N * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}

int run_microsnow(const mcf_snow_inputs* in, const mcf_snowm* sm, double reqhgt, double mat, const int32_t* outsel,
                  mcf_outputs* micro, int32_t device, bool af) {
    int rc;
    if ((rc = common_checks(in))) return rc;
    if (!sm || !outsel || !micro) return mcf::api_fail(MCF_ERR_ARG, "null gridmicrosnow argument");
    if ((in->array_forcing != 0) != af) return mcf::api_fail(MCF_ERR_ARG, "array_forcing does not match the entry point");
    for (int v = 0; v < MCF_NOUT; ++v)
        if (outsel[v] && !micro->var[v]) return mcf::api_fail(MCF_ERR_ARG, "requested micro variable has a null buffer");
    if (outsel[MCF_OUT_SOILM] && !in->other.Smax) return mcf::api_fail(MCF_ERR_ARG, "soilm requested but other$Smax is null");
    if ((rc = pick_device(device))) return rc;
    const int64_t N = in->rows * in->cols;
    const int T = (int)in->tsteps;
    const int64_t NT = N * T;
    const int nch = (T + 23) / 24;
    int nsel = 0;
    for (int v = 0; v < MCF_NOUT; ++v) nsel += outsel[v] != 0;
    if ((rc = check_room(((af ? 9 : 0) + 5 + nsel) * NT * 8 + 60 * N * 8))) return rc;
    mcf::DevOwner b;
    MicroArgs a;
    memset(&a, 0, sizeof a);
    a.N = N; a.tsteps = T; a.reqhgt = reqhgt; a.mat = mat; a.zref = in->other.zref;
    a.hiy = hours_in_year(in->obstime.year[0]);
    each_micro_raster(*in, [&](auto* host, auto member, int layers, bool required, const char* name) {
        if (!rc && (required || outsel[MCF_OUT_SOILM])) rc = b.up(&(a.*member), host, layers * N, name);
    });
    if (rc) return rc;
    StepTables tabs;
    if ((rc = build_step_tables(b, in, af, false, false, &tabs))) return rc;
    a.rows = tabs.rows; a.dates = tabs.dates; a.mxtc1 = tabs.mxtc1;
    const int64_t F = af ? NT : T;
    if (af && (rc = up_sites(b, a, in, N))) return rc;
    each_micro_series(*in, [&](auto* host, auto member, const char* name) { if (!rc && member) rc = b.up(&(a.*member), host, F, name); });
    if (!rc) rc = b.up(&a.sTc, sm->Tc, NT, "snowm$Tc");
    if (!rc) rc = b.up(&a.sTg, sm->Tg, NT, "snowm$Tg");
    if (!rc) rc = b.up(&a.swe, sm->totalSWE, NT, "snowm$totalSWE");
    if (!rc) rc = b.up(&a.sdepg, sm->groundsnowdepth, NT, "snowm$groundsnowdepth");
    if (!rc) rc = b.up(&a.sden, sm->snowden, NT, "snowm$snowden");
    if (rc) return rc;
    if ((rc = b.make(&a.meanD, N))) return rc;
    if (af) {
        if ((rc = b.make(&a.mxtc, N))) return rc;
        if ((rc = b.make(&a.hs0, N * (int64_t)nch))) return rc;
    }
    // The requested outputs in ONE buffer, NT apart (in/out: each starts as the no-snow solver's field): the linear view the
    // (cell, hour) kernel of the chunk loop writes through (k_microsnow_ring: RingView cpb = 0) — every day a snow day, every
    // snow-free cell-step kept.
    double* outbuf = nullptr;
    if ((rc = b.make(&outbuf, (int64_t)std::max(nsel, 1) * NT))) return rc;
    MicroRingArgs q;
    memset(&q, 0, sizeof q);
    {
        int rank = 0;
        for (int v = 0; v < MCF_NOUT; ++v) {
            if (!outsel[v]) continue;
            a.out[v] = outbuf + (int64_t)rank * NT;
            HIP_TRY(hipMemcpyAsync(a.out[v], micro->var[v], (size_t)NT * 8, hipMemcpyHostToDevice, nullptr));
            q.held |= 1u << v;
            ++rank;
        }
        q.sel = q.held;
        q.base0 = outbuf; q.vstride = NT;
        q.ring.N = N; q.ring.cpb = 0;
    }
    const unsigned gridN = (unsigned)((N + 255) / 256);
    if (!af && (rc = build_micro_steps(b, a))) return rc;
    if (af) hipLaunchKernelGGL(k_microsnow_cell<true>, dim3(gridN), dim3(256), 0, nullptr, a);
    else hipLaunchKernelGGL(k_microsnow_cell<false>, dim3(gridN), dim3(256), 0, nullptr, a);
    {
        std::vector<int32_t> ident((size_t)nch), ones((size_t)nch, 1);
        for (int d = 0; d < nch; ++d) ident[(size_t)d] = d;
        int32_t *d_map = nullptr, *d_one = nullptr;
        if ((rc = b.make(&d_map, nch))) return rc;
        if ((rc = b.make(&d_one, nch))) return rc;
        HIP_TRY(hipMemcpy(d_map, ident.data(), (size_t)nch * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_one, ones.data(), (size_t)nch * 4, hipMemcpyHostToDevice));
        q.daymap = d_map; q.nosnow = d_one; q.ndays = nch;
        for (int d0 = 0; d0 < nch; d0 += 32768) {        // (cells, days): the grid's y extent is 16 bits
            a.day0 = d0;
            q.m = a;
            const dim3 grid((unsigned)((N + 63) / 64), (unsigned)std::min(32768, nch - d0));
            if (af) hipLaunchKernelGGL(k_microsnow_ring<true>, grid, dim3(256), 0, nullptr, q, (const void*)a.dates, q.daymap, q.nosnow);
            else hipLaunchKernelGGL(k_microsnow_ring<false>, grid, dim3(256), 0, nullptr, q, a.mstep, q.daymap, q.nosnow);
        }
    }
    HIP_TRY(hipGetLastError());
    mcf::ToHost dl;
    for (int v = 0; v < MCF_NOUT; ++v)
        if (outsel[v]) HIP_TRY(dl.dense(micro->var[v], a.out[v], (size_t)NT * 8));
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}

// ---- coarse array weather left coarse (mcf_snowmodelq2, mcf_snowmodel2_coarse, mcf_runmicrosnow2_coarse): where a raster cell lies
// in the coarse grid, the argument structs of the expansion, its kernels, the upload of the coarse arrays ---------------------------
// Bilinear tap into one hour of a coarse field [crows, ccols] (an R array: one hour's coarse cells are contiguous): the
// operations of rformulas.upsample_coarse in their order, no FMA contraction — a tap has the host's bits.  (CoarseTap::mix
// contracts; the solver's taps stay as they are.)  `p`: the field at one hour, uniform over the wave; the four neighbours are
// 32-bit byte offsets from it (one hour's coarse cells x 8 B < 2^32: checked by the host).
struct SnowTap {
    uint32_t o00, o01, o10, o11;
    double wx, wy;
    __device__ __forceinline__ SnowTap(double rowpos, double colpos, int crows, int ccols) {
        const double fr = floor(rowpos), fc = floor(colpos);
        const int r0 = (int)fr, c0 = (int)fc;
        const int r1 = r0 + 1 < crows ? r0 + 1 : r0, c1 = c0 + 1 < ccols ? c0 + 1 : c0;
        wy = rowpos - fr;
        wx = colpos - fc;
        o00 = 8u * (uint32_t)(r0 + crows * c0); o01 = 8u * (uint32_t)(r0 + crows * c1);
        o10 = 8u * (uint32_t)(r1 + crows * c0); o11 = 8u * (uint32_t)(r1 + crows * c1);
    }
    __device__ __forceinline__ double operator()(const double* __restrict__ p) const {
#pragma clang fp contract(off)
        const char* q = reinterpret_cast<const char*>(p);
        const double v00 = *reinterpret_cast<const double*>(q + o00), v01 = *reinterpret_cast<const double*>(q + o01),
                     v10 = *reinterpret_cast<const double*>(q + o10), v11 = *reinterpret_cast<const double*>(q + o11);
        const double top = (1.0 - wx) * v00 + wx * v01;
        const double bot = (1.0 - wx) * v10 + wx * v11;
        return (1.0 - wy) * top + wy * bot;
    }
};
// where a raster cell (column-major index c) lies in the coarse grid
struct CoarseGeo {
    int32_t rows, crows, ccols, pad;
    const double *rowpos, *colpos;      // [rows], [cols]
    __device__ __forceinline__ SnowTap tap(int64_t c) const {
        const uint32_t j = (uint32_t)c / (uint32_t)rows, i = (uint32_t)c - j * (uint32_t)rows;
        return SnowTap(rowpos[i], colpos[j], crows, ccols);
    }
};

// (`.satvap` and `.lapserate`, snow_satvap_r / snow_lapserate_r: mcf_snow_device.hpp, where mcf_selftest_snow.hip reaches them)
// A selected day's (or a chunk's) thirteen series on the raster from the coarse arrays (int:3112-3164; snow.py
// _fine_snow_inputs), [hours][N] as k_snowmodel<true> reads them.  `.cca`: bilinear, NA on the dtm's holes; pressure and the wind components
// are not masked.  altcorrect > 0: `pres` holds the coarse pressure already taken to sea level (the host divides by the
// coarse cell's factor), the cell's own factor brings it back up; the temperature moves by elevd x lapse rate, relative
// humidity keeps the vapour pressure of the uncorrected field; capped at 100.  `umu` is the day's slab of the output set when
// the caller wants pointm$umu, so what the model reads is what leaves.
struct FineArgs {
    int64_t N, hour0;                  // hour0: the day's first hour in the coarse arrays of the selected hours
    int32_t altcorrect, pad;
    CoarseGeo geo;
    const double *dtm, *zc;            // zc: coarse dtm with NA read as 0 (altcorrect > 0)
    const double *temp, *relhum, *pres, *swdown, *difrad, *lwdown, *precip, *windu, *windv, *Gp, *Tc, *RswabsG, *RlwabsG, *umu;
    double *o_temp, *o_relhum, *o_pres, *o_swdown, *o_difrad, *o_lwdown, *o_windspeed, *o_precip, *o_Gp, *o_Tc, *o_RswabsG, *o_RlwabsG,
        *o_umu;
};
// hours kb .. ke - 1 of cell c's thirteen series into [.][N]: the arithmetic, whose bits tests rely on
__device__ __forceinline__ void coarse_cell_hours(const FineArgs& a, int64_t c, int kb, int ke) {
#pragma clang fp contract(off)
    const SnowTap tap = a.geo.tap(c);
    const int64_t CC = (int64_t)a.geo.crows * a.geo.ccols;
    const double z = a.dtm[c], NA = na_real();
    const bool hole = isnan(z);
    double up = 1.0, elevd = 0.0;
    if (a.altcorrect) {
        up = pow((293 - 0.0065 * z) / 293, 5.26);
        elevd = tap(a.zc) - z;
    }
    for (int k = kb; k < ke; ++k) {
        const int64_t h = (a.hour0 + k) * CC, o = c + a.N * k;
        auto cca = [&](const double* f) { const double v = tap(f + h); return hole ? NA : v; };
        double temp = cca(a.temp), relhum = cca(a.relhum), pres = tap(a.pres + h);
        if (a.altcorrect) {
            const double ea = snow_satvap_r(temp) * relhum / 100;
            pres = pres * up;
            const double lr = a.altcorrect == 1 ? 5.0 / 1000 : snow_lapserate_r(temp, ea, pres);
            temp = lr * elevd + temp;
            relhum = (ea / snow_satvap_r(temp)) * 100;
        }
        if (relhum > 100) relhum = 100.0;
        const double wu = tap(a.windu + h), wv = tap(a.windv + h);
        a.o_temp[o] = temp; a.o_relhum[o] = relhum; a.o_pres[o] = pres;
        a.o_windspeed[o] = sqrt(wu * wu + wv * wv);
        a.o_swdown[o] = cca(a.swdown); a.o_difrad[o] = cca(a.difrad); a.o_lwdown[o] = cca(a.lwdown); a.o_precip[o] = cca(a.precip);
        a.o_Gp[o] = cca(a.Gp); a.o_Tc[o] = cca(a.Tc); a.o_RswabsG[o] = cca(a.RswabsG); a.o_RlwabsG[o] = cca(a.RlwabsG);
        a.o_umu[o] = cca(a.umu);
    }
}
// The thirteen series of the hours a.hour0 .. a.hour0 + ns - 1 into [ns][N]: a selected day of the fast method (ns = 24) or a
// chunk of the slow one.  Lanes run along the cells (a wave stores 512 contiguous bytes per series and hour), blockIdx.y over
// groups of kFineHours hours: a lane forms its tap, its pressure factor and elevd once and walks its group.  Five hours: the
// 120-hour chunk of the bundled 50 x 50 raster is 10 x 24 = 240 workgroups on 256 CUs where one lane per cell would be 10, the
// lane's set-up (two position loads, one pow with altcorrect) is spread over 5 x 14 taps, and a chunk of whole days (24, 48, 120
// hours; 24 is no multiple of 5) ends in a partial group, so the partial path is the everyday one.  g0: the first group of
// this launch (the grid's y extent is 16 bits).
constexpr int kFineHours = 5;
// one coarse plane on the raster, NA on the dtm's holes (mean(cca(tc), na.rm = TRUE) is the mean of this of tc's time sums)
__global__ __launch_bounds__(256) void k_tap_plane(CoarseGeo geo, int64_t N, const double* __restrict__ dtm, const double* __restrict__ plane,
                                                   double* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double v = geo.tap(c)(plane);
    out[c] = isnan(dtm[c]) ? na_real() : v;
}
// `.cleansmod`: NA on the dtm's holes in the series that leave, [ns][N] each (null: not written); holes are few, a lane walks
// its cell's steps
struct CleanArgs {
    int64_t N;
    const double* dtm;
    double* v[5];
};
__global__ __launch_bounds__(256) void k_clean_chunk(CleanArgs a, int ns) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.N || !isnan(a.dtm[c])) return;
    const double NA = na_real();
#pragma unroll
    for (int q = 0; q < 5; ++q)
        if (a.v[q])
            for (int k = 0; k < ns; ++k) a.v[q][c + a.N * k] = NA;
}

// the coarse arrays of the selected hours, in the order FineArgs lists them
template <class In, class F>
void each_coarse_selected(In& in, F&& f) {   // f(pointer, the kernel's argument, name)
    using A = FineArgs;
    f(in.temp, &A::temp, "temp"); f(in.relhum, &A::relhum, "relhum"); f(in.pres, &A::pres, "pres"); f(in.swdown, &A::swdown, "swdown");
    f(in.difrad, &A::difrad, "difrad"); f(in.lwdown, &A::lwdown, "lwdown"); f(in.precip, &A::precip, "precip");
    f(in.windu, &A::windu, "windu"); f(in.windv, &A::windv, "windv"); f(in.Gp, &A::Gp, "pointm$Gp"); f(in.Tc, &A::Tc, "pointm$Tc");
    f(in.RswabsG, &A::RswabsG, "pointm$RswabsG"); f(in.RlwabsG, &A::RlwabsG, "pointm$RlwabsG"); f(in.umu, &A::umu, "pointm$umu");
}

// What every entry with a coarse grid has of it, whatever struct brings it (host only): the raster, the grid, where the raster's
// rows and columns lie in it, the grid's dtm and the altitude mode
struct CoarseGrid {
    int64_t rows, cols, coarse_rows, coarse_cols;
    const double *rowpos, *colpos, *coarse_dtm;
    int32_t altcorrect;
    int64_t cells() const { return rows * cols; }
    int64_t coarse_cells() const { return coarse_rows * coarse_cols; }
};
template <class In>      // mcf_snowfast2_in, mcf_snowcoarse_in, mcf_microcoarse_in
CoarseGrid coarse_grid(const In& ci, int64_t rows, int64_t cols) {
    return {rows, cols, ci.coarse_rows, ci.coarse_cols, ci.coarse_rowpos, ci.coarse_colpos, ci.coarse_dtm, ci.altcorrect};
}
// every position inside the coarse grid: a tap reads cells floor(pos) and floor(pos) + 1 (or floor(pos) at the far edge)
bool positions_inside(const double* pos, int64_t n, int64_t ncoarse) {
    for (int64_t i = 0; i < n; ++i)
        if (!(pos[i] >= 0.0 && pos[i] <= (double)(ncoarse - 1))) return false;
    return true;
}
bool positions_inside(const CoarseGrid& g) {
    return positions_inside(g.rowpos, g.rows, g.coarse_rows) && positions_inside(g.colpos, g.cols, g.coarse_cols);
}
// a tap is a uniform base + a 32-bit byte offset; the bound of the solver's coarse forcing, which addresses a day at once
bool coarse_grid_too_large(const CoarseGrid& g) { return (double)g.coarse_rows * (double)g.coarse_cols * 24.0 * 8.0 >= 4294967296.0; }
// What the entries refuse of a coarse grid before a device is touched, under the entry's name and its group's tag ("micro: " or
// none): the grid's own conditions, then the caller's scan for null inputs (null_inputs() -> status: the order of its need()
// calls decides which missing input is named, so it stays with the caller), then the two bounds that read the positions.
template <class Scan>
int coarse_grid_checks(const CoarseGrid& g, const char* entry, const char* tag, Scan&& null_inputs) {
    auto fail = [&](const char* m) { return mcf::api_fail(MCF_ERR_ARG, std::string(entry) + ": " + tag + m); };
    if (g.coarse_rows < 1 || g.coarse_cols < 1) return fail("coarse_rows and coarse_cols must be at least 1");
    if (g.altcorrect < 0 || g.altcorrect > 2) return fail("altcorrect must be 0, 1 or 2");
    if (g.altcorrect > 0 && !g.coarse_dtm) return fail("altcorrect > 0 needs coarse_dtm (null input: coarse_dtm)");
    if (const int rc = null_inputs()) return rc;
    if (!positions_inside(g)) return fail("coarse_rowpos / coarse_colpos must lie in 0..coarse_rows - 1 / 0..coarse_cols - 1");
    if (coarse_grid_too_large(g)) return fail("coarse grid too large (24 x coarse cells x 8 B must stay below 2^32)");
    return MCF_OK;
}

// Geometry, dtm and the coarse arrays of hours h0 .. h0 + nh - 1 on the device, into either argument struct (FineArgs, MicroFineArgs).
// altcorrect > 0: the coarse dtm with NA read as 0, and the pressure taken to sea level on the coarse grid here (int:2871-2873,
// 3127-3129).  dtm: the raster's on the host; d_dtm: on the device if the caller has it there already.  each(in, f): the list of
// the struct's coarse arrays (each_coarse_selected, each_micro_coarse).
template <class Args, class In, class Each>
int coarse_upload(mcf::DevOwner& b, const CoarseGrid& g, const In* ci, Each&& each, const double* dtm, int64_t h0, int64_t nh,
                  const double* d_dtm, Args* fa) {
    const int64_t N = g.cells(), CC = g.coarse_cells();
    int rc = MCF_OK;
    memset(fa, 0, sizeof *fa);
    fa->N = N; fa->altcorrect = g.altcorrect;
    fa->geo.rows = (int32_t)g.rows; fa->geo.crows = (int32_t)g.coarse_rows; fa->geo.ccols = (int32_t)g.coarse_cols;
    if ((rc = b.up(&fa->geo.rowpos, g.rowpos, g.rows, "coarse_rowpos"))) return rc;
    if ((rc = b.up(&fa->geo.colpos, g.colpos, g.cols, "coarse_colpos"))) return rc;
    if (d_dtm) fa->dtm = d_dtm;
    else if ((rc = b.up(&fa->dtm, dtm, N, "dtm"))) return rc;
    std::vector<double> psl;
    if (g.altcorrect) {
        std::vector<double> zc((size_t)CC), down((size_t)CC);
        for (int64_t q = 0; q < CC; ++q) {
            zc[(size_t)q] = std::isnan(g.coarse_dtm[q]) ? 0.0 : g.coarse_dtm[q];
            down[(size_t)q] = pow((293 - 0.0065 * zc[(size_t)q]) / 293, 5.26);
        }
        psl.resize((size_t)(CC * nh));
        for (int64_t k = 0; k < nh; ++k)
            for (int64_t q = 0; q < CC; ++q) psl[(size_t)(k * CC + q)] = ci->pres[(h0 + k) * CC + q] / down[(size_t)q];
        if ((rc = b.up(&fa->zc, zc.data(), CC, "coarse_dtm"))) return rc;
    }
    each(*ci, [&](auto* host, auto member, const char* name) {
        if (!rc) rc = b.up(&(fa->*member), g.altcorrect && !strcmp(name, "pres") ? psl.data() : host + h0 * CC, CC * nh, name);
    });
    return rc;
}
// (the lists as coarse_upload takes them)
constexpr auto kSnowCoarseArrays = [](auto& in, auto&& f) { each_coarse_selected(in, f); };

// `.cca` of one coarse field for the hours hour0 .. hour0 + ns - 1, [ns][N]: k_coarse_hours' lane map (pointm$umu behind the last chunk)
__global__ __launch_bounds__(256) void k_fine_field(CoarseGeo geo, int64_t N, int64_t hour0, int ns, const double* __restrict__ dtm,
                                                    const double* __restrict__ field, double* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const int kb = (int)blockIdx.y * kFineHours, ke = kb + kFineHours < ns ? kb + kFineHours : ns;
    const SnowTap tap = geo.tap(c);
    const int64_t CC = (int64_t)geo.crows * geo.ccols;
    const bool hole = isnan(dtm[c]);
    for (int k = kb; k < ke; ++k) {
        const double v = tap(field + (hour0 + k) * CC);
        out[c + N * k] = hole ? na_real() : v;
    }
}

// the kernel's outputs in the order of each_model_series
void fine_outputs(FineArgs& fa, double* const d[13]) {
    fa.o_temp = d[0]; fa.o_relhum = d[1]; fa.o_pres = d[2]; fa.o_swdown = d[3]; fa.o_difrad = d[4]; fa.o_lwdown = d[5];
    fa.o_windspeed = d[6]; fa.o_precip = d[7]; fa.o_Gp = d[8]; fa.o_Tc = d[9]; fa.o_RswabsG = d[10]; fa.o_RlwabsG = d[11]; fa.o_umu = d[12];
}

// The snow-day microclimate's weather is not the snow model's: vapour pressure is resampled (the host forms it on the climate
// grid), temperature and pressure are NOT masked by the dtm, relative humidity comes from the resampled vapour pressure in every
// altitude mode and is kept within 20 .. 100.  o[]: the nine series in the order of each_micro_series, [hours][N] as
// k_microsnow_ring<true> reads them; mask bit f: series f is written (the set-up's scan reads temp and precip alone).
struct MicroFineArgs {
    int64_t N, hour0;                  // hour0: the first hour in the resident coarse arrays
    int32_t altcorrect;
    uint32_t mask;
    CoarseGeo geo;
    const double *dtm, *zc;            // zc: coarse dtm with NA read as 0 (altcorrect > 0)
    const double *temp, *ea, *pres, *swdown, *difrad, *lwdown, *windu, *windv, *precip, *umu;   // pres: at sea level when altcorrect > 0
    double* o[kMicroSeries];
};
enum { MF_TEMP = 0, MF_RELHUM, MF_PRES, MF_SWDOWN, MF_DIFRAD, MF_LWDOWN, MF_WINDSPEED, MF_PRECIP, MF_UMU };
constexpr uint32_t kMicroAll = (1u << kMicroSeries) - 1;
// hours kb .. ke - 1 of cell c: the host's operations in the host's order, no contraction (the mask is uniform: no lane diverges)
__device__ __forceinline__ void coarse_cell_hours(const MicroFineArgs& a, int64_t c, int kb, int ke) {
#pragma clang fp contract(off)
    const SnowTap tap = a.geo.tap(c);
    const int64_t CC = (int64_t)a.geo.crows * a.geo.ccols;
    const double z = a.dtm[c], NA = na_real();
    const bool hole = isnan(z);
    const uint32_t m = a.mask;
    const bool want_t = (m & (1u << MF_TEMP | 1u << MF_RELHUM)) != 0;
    const bool want_ea = (m >> MF_RELHUM & 1u) || (want_t && a.altcorrect == 2);
    const bool want_p = (m >> MF_PRES & 1u) || (want_t && a.altcorrect == 2);
    double up = 1.0, elevd = 0.0;
    if (a.altcorrect) {
        up = pow((293 - 0.0065 * z) / 293, 5.26);
        elevd = tap(a.zc) - z;
    }
    for (int k = kb; k < ke; ++k) {
        const int64_t h = (a.hour0 + k) * CC, o = c + a.N * k;
        auto cca = [&](const double* f) { const double v = tap(f + h); return hole ? NA : v; };
        double ea = 0.0, pres = 0.0;
        if (want_ea) ea = tap(a.ea + h);
        if (want_p) {
            pres = tap(a.pres + h);
            if (a.altcorrect) pres = pres * up;
        }
        if (want_t) {
            double temp = tap(a.temp + h);
            if (a.altcorrect) {
                const double lr = a.altcorrect == 1 ? 5.0 / 1000 : snow_lapserate_r(temp, ea, pres);
                temp = lr * elevd + temp;
            }
            if (m >> MF_TEMP & 1u) a.o[MF_TEMP][o] = temp;
            if (m >> MF_RELHUM & 1u) {
                double relhum = (ea / snow_satvap_r(temp)) * 100;
                if (relhum < 20.0) relhum = 20.0;              // np.clip: NaN stays NaN
                if (relhum > 100.0) relhum = 100.0;
                a.o[MF_RELHUM][o] = relhum;
            }
        }
        if (m >> MF_PRES & 1u) a.o[MF_PRES][o] = pres;
        if (m >> MF_SWDOWN & 1u) a.o[MF_SWDOWN][o] = cca(a.swdown);
        if (m >> MF_DIFRAD & 1u) a.o[MF_DIFRAD][o] = cca(a.difrad);
        if (m >> MF_LWDOWN & 1u) a.o[MF_LWDOWN][o] = cca(a.lwdown);
        if (m >> MF_WINDSPEED & 1u) {
            const double wu = tap(a.windu + h), wv = tap(a.windv + h);
            a.o[MF_WINDSPEED][o] = sqrt(wu * wu + wv * wv);
        }
        if (m >> MF_PRECIP & 1u) a.o[MF_PRECIP][o] = cca(a.precip);
        if (m >> MF_UMU & 1u) a.o[MF_UMU][o] = cca(a.umu);
    }
}
// The expansion kernel of either argument struct (FineArgs: the snow model's thirteen series, MicroFineArgs: the snow-day
// microclimate's nine) around its coarse_cell_hours, and its launches: at most 32768 groups each
template <class Args>
__global__ __launch_bounds__(256) void k_coarse_hours(Args a, int ns, int g0) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.N) return;
    const int kb = (g0 + (int)blockIdx.y) * kFineHours, ke = kb + kFineHours < ns ? kb + kFineHours : ns;
    coarse_cell_hours(a, c, kb, ke);
}
template <class Args>
void launch_coarse_hours(const Args& fa, int ns, hipStream_t stream) {
    const int groups = (ns + kFineHours - 1) / kFineHours;
    for (int g0 = 0; g0 < groups; g0 += 32768)
        hipLaunchKernelGGL(k_coarse_hours<Args>, dim3((unsigned)((fa.N + 255) / 256), (unsigned)std::min(32768, groups - g0)), dim3(256), 0,
                           stream, fa, ns, g0);
}
// the ten coarse arrays in the order of the kernel's arguments
template <class In, class F>
void each_micro_coarse(In& in, F&& f) {   // f(pointer, the kernel's argument, name)
    using A = MicroFineArgs;
    f(in.temp, &A::temp, "temp"); f(in.ea, &A::ea, "ea"); f(in.pres, &A::pres, "pres"); f(in.swdown, &A::swdown, "swdown");
    f(in.difrad, &A::difrad, "difrad"); f(in.lwdown, &A::lwdown, "lwdown"); f(in.windu, &A::windu, "windu"); f(in.windv, &A::windv, "windv");
    f(in.precip, &A::precip, "precip"); f(in.umu, &A::umu, "umu");
}
constexpr auto kMicroCoarseArrays = [](auto& in, auto&& f) { each_micro_coarse(in, f); };

// (the chunk loop lives in mcf_snowplan below)

}  // namespace

// ---- .snowmodel1's chunk loop as a stepwise, device-resident plan (one per rank's row block) ---------------
struct mcf_snowplan {
    int device = 0;
    int64_t rows = 0, cols = 0, N = 0, row0 = 0, rows_total = 0;
    int T = 0, chunk = 120, nchunks = 1, ss = 10;
    double res = 1.0, tfact = 0.02, zref = 2.0;
    mcf::DevOwner b;
    ModelArgs a;
    const StepRow* rows_tab = nullptr;
    // array weather (`.snowmodel2`'s loop): the caller's thirteen [N][T] series — a chunk's slices go up as the loop reaches it —
    // and the date rows of every step
    bool af = false;
    const double* h_series[13] = {};      // in the order of each_model_series
    double* d_series[13] = {};            // [N][chunk]
    // coarse array weather: the fourteen coarse arrays stay on the device, a chunk's thirteen series are expanded from them
    // into d_series by one kernel (no h_series).  coarse: the resident arrays of the whole series (hour 0 = step 0) and the plan's
    // dtm (mcf_snowmodel2_coarse); h_umu: [rows, cols, T] of the caller, where a chunk's pointm$umu goes, or null
    std::optional<FineArgs> coarse;
    double* h_umu = nullptr;
    const DateRow2* dates_tab = nullptr;
    const double *d_dtm = nullptr, *d_isnowdg = nullptr;
    double *d_isnowdc = nullptr, *d_dtms = nullptr, *d_slope = nullptr, *d_aspect = nullptr, *d_svf = nullptr,
           *d_wsa = nullptr, *d_hor = nullptr, *d_tpic = nullptr, *d_mean2 = nullptr, *d_cm = nullptr, *d_ext = nullptr,
           *d_sumws = nullptr;
    int64_t ext_cap = 0, cm_cap = 0;
    // the surface (own rows + halos) the terrain arrays were last derived from, and its geometry: a chunk that starts from the
    // very same surface — every snow-free stretch of the year — keeps them (bit patterns compared on the device)
    double* d_zlast = nullptr;
    int64_t zlast_n = 0, zlast_cap = 0;
    int32_t zlast_hn = -1, zlast_hs = -1;
    int32_t* d_zdiff = nullptr;
    int terrain_reused = 0, terrain_refreshed = 0;
    // mcf_snowplan_apply3: the chunk's per-step max and min of totalSWE come out of one pass (k_apply3_minmax_part) into a
    // workspace the plan owns; whichever of the two is asked for first computes both, the other is answered from here
    double* d_mm = nullptr;              // [2 x chunk x parts x 2] partials, [4 x chunk] results
    int mm_parts = 0, mm_chunk = -1;     // mm_chunk: the chunk whose run the cached values belong to (-1: none)
    std::vector<double> mm_host;         // max[chunk], count[chunk], min[chunk], count[chunk]
    int32_t *d_ac = nullptr, *d_ag = nullptr;
    std::vector<double> wind;
    mcf::ToHost dl;
    int prepared = -1;
    double t_terrain = 0, t_model = 0, t_fine = 0;   // ms, MCF_TIMING (t_fine: the chunk expansion of coarse array weather)
    mcf::TerrainWork twork;              // terrain_device's scratch, kept across the chunks
    // initial hand-over state, for mcf_snowplan_reset (the snow-day microclimate needs a second pass over the series)
    const double* d_isnowdc0 = nullptr;
    const int32_t *d_ac0 = nullptr, *d_ag0 = nullptr;
    // gridmicrosnow1 inside the chunk loop (mcf_snowplan_micro_*)
    double *d_sumD = nullptr, *d_meanD = nullptr;
    int32_t* d_sden_na = nullptr;        // the subset series' first snow density is NA (cpp:4716)
    int64_t sumD_steps = 0;
    bool micro_ready = false;
    mcf::DevOwner mb, mbs;               // the micro set-up's buffers: per-call (series) and static (vegetation, terrain)
    bool micro_static = false;
    MicroArgs ma;
    // array weather: the caller's whole-series [N][T] arrays of gridmicrosnow2's weather (temp, relhum, pres, swdown, difrad, lwdown,
    // windspeed, precip, umu) — a chunk's snow days go up when the chunk's microclimate runs — and their device slabs [N][chunk]
    bool micro_af = false;
    const double* h_micro[kMicroSeries] = {};
    double* d_micro[kMicroSeries] = {};
    const double* MicroArgs::* micro_arg[kMicroSeries] = {};      // the kernel argument each slab is
    // coarse array weather: the ten coarse arrays of the microclimate's weather stay on the device (no h_micro), a chunk's snow
    // days are expanded from them into d_micro by one kernel per run of consecutive snow days (mcf_runmicrosnow2_coarse; the
    // plan's own set, not the snow model's)
    std::optional<MicroFineArgs> mcoarse;
    double t_micro_fine = 0;             // ms, MCF_TIMING: that expansion, pass 2's launches
    int n_micro_fine = 0;
    int32_t outsel[MCF_NOUT] = {};
    std::vector<int32_t> sub_of_day;     // absolute day -> day of the snow-day subset series, or -1
    int32_t *d_daymap = nullptr, *d_nosnow = nullptr;     // [chunk days]
    // mcf_snowplan_set_series: which of the five device series (bit 0 Tc, 1 Tg, 2 totalSWE, 3 ground snow depth, 4 density) the
    // next run_chunk writes; series_valid: what the plan's working buffers hold of the chunk run last
    uint32_t series_mask = 31, series_valid = 0;
    int32_t* d_ncpack = nullptr;         // mcf_snowplan_nc_write: a piece of packed records on its way to the host
    int64_t ncpack_elems = 0;
    uint8_t* d_tflag = nullptr;          // mcf_snowplan_covered_tiles: one flag per tile of the solver plan
    int64_t tflag_cap = 0;
    uint8_t* d_need = nullptr;           // mcf_snowplan_free_cells: one flag per cell + an 8-byte count behind them
    int64_t need_cap = 0;
    // hand-over state at the start of a chunk (mcf_snowplan_checkpoint): isnowdc, the snow surface, the two age matrices
    std::vector<char*> ckpt;
    // series of chunks kept on the device between the two passes (mcf_snowplan_keep_chunk): a kept chunk's buffers are the ones
    // the model wrote — the plan goes on with fresh ones — so pass 2 neither re-runs the chunk nor copies anything
    struct Kept { double *Tc = nullptr, *Tg = nullptr, *sdepc = nullptr, *sdepg = nullptr, *sden = nullptr, *tzd = nullptr; };
    // (a kept set belongs to the run of its chunk that was current when it was handed over: running the chunk again — a new
    // pass 1 without mcf_snowplan_release_kept, a re-run after mcf_snowplan_reset — returns the stale set to the pool, so that
    // mcf_snowplan_microsnow can never read last year's series for it)
    std::vector<Kept> kept;
    std::vector<Kept> pool;              // released sets, reused by the next year's pass 1 (hipMalloc of 10 GB costs 0.25 s)
    int64_t keep_budget = -1;            // bytes of kept sets this plan may ALLOCATE in all (mcf_snowplan_set_keep_budget); -1: no limit of its own
    int64_t keep_allocated = 0;
    mcf::DevOwner kb;
    // period summaries of the five series (mcf_snowplan_summary_enable; null state: off): the state [selected series][period]
    // [state row][N] of mcf_kernels.h SummaryPlanesArgs, the day tables on the device, one statistic plane on its way to the host
    double *d_ps_state = nullptr, *d_ps_plane = nullptr;
    int32_t *d_ps_pod = nullptr, *d_ps_prev = nullptr, *d_ps_next = nullptr, *d_ps_days = nullptr;
    int ps_nperiods = 0, ps_nrows = 0, ps_nsel = 0, ps_next_chunk = 0;
    uint32_t ps_init_codes = 0, ps_bits = 0;      // ps_bits: the selected series as a mcf_snowplan_set_series mask
    int ps_row[MCF_NSTAT] = {}, ps_sel1[5] = {};  // ps_sel1: 1-based place of a series in the state, 0: not selected
    double ps_thr[5] = {};
    std::vector<int32_t> ps_pod, ps_days;
    // series sink of the five series (mcf_snowplan_series_enable; se_on): as the solver plan keeps it — the points'
    // [selected series][point][T] buffer, the zones' state (mcf_kernels.h SeriesPlanesArgs), one statistic [T][zone] on its
    // way to the host, the folded days
    bool se_on = false;
    int64_t se_npoints = 0;
    int se_nzones = 0, se_nsel = 0, se_workgroups = 0;
    uint32_t se_bits = 0;                         // the selected series as a mcf_snowplan_set_series mask
    int se_sel1[5] = {}, se_zstat[MCF_NZSTAT] = {};
    int64_t* d_se_cells = nullptr;
    int32_t *d_se_zone = nullptr, *d_se_done = nullptr;
    double *d_se_points = nullptr, *d_se_plane = nullptr;
    long long* d_se_state = nullptr;
    std::vector<int32_t> se_done;                 // [days] 1: folded
    std::vector<char> se_chunk_done;              // [chunks] 1: folded
    ~mcf_snowplan() { twork.release(); }
};

namespace {

int chunk_af(const mcf_snowplan* sp, int ch, int* af) {   // int:2589-2590
    const int k0 = ch * sp->chunk, ns = std::min(sp->chunk, sp->T - k0);
    double wsum = 0.0;
    for (int k = 0; k < ns; ++k) wsum += sp->wind[k0 + k];
    const double tpr = 10 * sqrt(wsum / ns);
    double afd = nearbyint(tpr / sp->res);                // R's round(x, 0): half to even
    if (sp->af && !(afd >= 2.0)) afd = 2.0;               // `.snowmodel2`: `if (af < 2) af <- 2`, int:2984
    if (!(afd >= 1.0))
        return mcf::api_fail(MCF_ERR_ARG, "snow driver: aggregation factor round(10*sqrt(mean wind)/res) is 0 (terra::aggregate fails)");
    *af = (int)std::min(afd, 1e9);
    return MCF_OK;
}

}  // namespace

extern "C" int mcf_snowplan_chunk_af(const mcf_snowplan* sp, int32_t chunk, int32_t* af) {
    if (!sp || !af) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (chunk < 0 || chunk >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    int a = 1;
    const int rc = chunk_af(sp, chunk, &a);
    *af = a;
    return rc;
}
// ---- the plan's coarse array weather: the snow model's resident arrays and a chunk's expansion, `.cleansmod` and pointm$umu behind
// the chunk (mcf_snowmodel2_coarse), the snow-day microclimate's expansion (mcf_runmicrosnow2_coarse)
static int coarse_attach(mcf_snowplan* sp, const mcf_snowcoarse_in* co, double* umu_out) {
    sp->h_umu = umu_out;
    sp->coarse.emplace();
    return coarse_upload(sp->b, coarse_grid(*co, sp->rows, sp->cols), co, kSnowCoarseArrays, co->drv.dtm, 0, sp->T, sp->d_dtm, &*sp->coarse);
}
static int coarse_fill_chunk(mcf_snowplan* sp, int k0, int ns) {
    FineArgs fa = *sp->coarse;
    fa.hour0 = k0;
    fine_outputs(fa, sp->d_series);
    TimedSpan span;
    HIP_TRY(span.begin());
    launch_coarse_hours(fa, ns, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(span.end(&sp->t_fine));
    return MCF_OK;
}
static void coarse_clean_chunk(mcf_snowplan* sp, double* Tc, double* Tg, double* sdepg, double* sdepc, double* sden, int ns) {
    CleanArgs cl;
    cl.N = sp->N; cl.dtm = sp->d_dtm;
    cl.v[0] = Tc; cl.v[1] = Tg; cl.v[2] = sdepg; cl.v[3] = sdepc; cl.v[4] = sden;
    hipLaunchKernelGGL(k_clean_chunk, dim3((unsigned)((sp->N + 255) / 256)), dim3(256), 0, nullptr, cl, ns);
}
static int coarse_umu_out(mcf_snowplan* sp, int k0, int ns, bool last) {
    if (!sp->h_umu) return MCF_OK;
    const FineArgs& fa = *sp->coarse;
    const int64_t N = sp->N;
    HIP_TRY(sp->dl.dense(sp->h_umu + (int64_t)k0 * N, sp->d_series[12], (size_t)ns * N * 8));
    if (!last) return MCF_OK;
    // the steps behind the last whole chunk (fewer than a chunk): umu alone, through the chunk's slab
    for (int t0 = k0 + ns; t0 < sp->T; t0 += sp->chunk) {
        const int nt = std::min(sp->chunk, sp->T - t0);
        hipLaunchKernelGGL(k_fine_field, dim3((unsigned)((N + 255) / 256), (unsigned)((nt + kFineHours - 1) / kFineHours)), dim3(256), 0,
                           nullptr, fa.geo, N, (int64_t)t0, nt, fa.dtm, fa.umu, sp->d_series[12]);
        HIP_TRY(hipGetLastError());
        HIP_TRY(sp->dl.dense(sp->h_umu + (int64_t)t0 * N, sp->d_series[12], (size_t)nt * N * 8));
    }
    return MCF_OK;
}
// hours hour0 .. hour0 + ns - 1 of the series in `mask` into the plan's slabs from step slab_off on; precip_into: where the
// precipitation goes instead of its own slab (the set-up's scan streams temp and precip through the first two slabs)
static int micro_coarse_fill(mcf_snowplan* sp, int64_t hour0, int ns, int64_t slab_off, uint32_t mask, double* precip_into) {
    MicroFineArgs fa = *sp->mcoarse;
    fa.hour0 = hour0; fa.mask = mask;
    for (int f = 0; f < kMicroSeries; ++f) fa.o[f] = sp->d_micro[f] + slab_off * sp->N;
    if (precip_into) fa.o[MF_PRECIP] = precip_into;
    TimedSpan span(mask == kMicroAll);       // (pass 2's launches: the set-up's scan is not in the figure)
    HIP_TRY(span.begin());
    launch_coarse_hours(fa, ns, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(span.end(&sp->t_micro_fine));
    if (span.on) sp->n_micro_fine += ns;
    return MCF_OK;
}
// `co`: coarse array weather (mcf_snowmodel2_coarse, which has checked its arguments) — din is &co->drv, the thirteen fine series
// of din->base are not read; umu_out: where pointm$umu goes (null: not wanted)
static int snowplan_create(const mcf_snowdriver_in* din, int64_t row0, int64_t rows_total, int32_t device, const mcf_snowcoarse_in* co,
                           double* umu_out, mcf_snowplan** out) {
    int rc;
    if (!din || !out) return mcf::api_fail(MCF_ERR_ARG, "null snow driver argument");
    const mcf_snow_inputs* in = &din->base;
    if ((rc = common_checks(in))) return rc;
    const bool af = in->array_forcing != 0;
    if (!din->dtm || !(din->res > 0)) return mcf::api_fail(MCF_ERR_ARG, "snow driver needs dtm and res > 0");
    if (!co && !in->clim.windspeed) return mcf::api_fail(MCF_ERR_ARG, "null input: windspeed");
    if (rows_total <= 0) { rows_total = in->rows; row0 = 0; }
    if (row0 < 0 || row0 + in->rows > rows_total) return mcf::api_fail(MCF_ERR_ARG, "block outside the raster");
    if (af) {
        if (row0 != 0 || rows_total != in->rows) return mcf::api_fail(MCF_ERR_ARG, "snow driver, array weather: one block (the whole raster)");
        if (!din->af_wind) return mcf::api_fail(MCF_ERR_ARG, "snow driver, array weather: af_wind (the chunk wind series) is null");
        if (!in->other.lats || !in->other.lons || !in->clim.winddir) return mcf::api_fail(MCF_ERR_ARG, "snow driver, array weather: lats / lons / winddir");
        bool given = true;
        each_model_series(*in, [&](auto* host, auto, auto, const char*) { given = given && host; });
        if (!given && !co) return mcf::api_fail(MCF_ERR_ARG, "snow driver, array weather: a climate / point-model array is null");
    }
    if ((rc = pick_device(device))) return rc;
    if (co) {                                        // the chunk's series, the plan's rasters, the resident coarse arrays
        const int64_t chunk = din->chunk_steps > 0 ? din->chunk_steps : 120, N = in->rows * in->cols;
        if ((rc = check_room((18 * chunk + 60) * N * 8 + 14 * co->coarse_rows * co->coarse_cols * in->tsteps * 8))) return rc;
    }
    mcf_snowplan* sp = new mcf_snowplan();
    struct Guard { mcf_snowplan* p; ~Guard() { delete p; } } guard{sp};
    sp->device = device;
    sp->rows = in->rows; sp->cols = in->cols; sp->N = in->rows * in->cols; sp->row0 = row0; sp->rows_total = rows_total;
    sp->T = (int)in->tsteps;
    sp->chunk = din->chunk_steps > 0 ? din->chunk_steps : 120;
    if (sp->chunk % 24) return mcf::api_fail(MCF_ERR_ARG, "snow driver: chunk_steps must be whole days");
    sp->nchunks = std::max(1, sp->T / sp->chunk);   // `for (day in 1:n5days)`: 1:x truncates, and 1:0.4 still runs once
    sp->res = din->res; sp->tfact = din->tfact; sp->zref = in->other.zref;
    sp->ss = din->res <= 100 ? 10 : 1;              // int:2577-2578
    sp->af = af;
    if (af && din->af_wsa_s > 0) sp->ss = din->af_wsa_s;                        // int:2963-2964
    if (af) sp->wind.assign(din->af_wind, din->af_wind + sp->T);                // wss, int:2981
    else sp->wind.assign(in->clim.windspeed, in->clim.windspeed + sp->T);
    const int64_t N = sp->N;
    const int T = sp->T;
    mcf::DevOwner& b = sp->b;
    ModelArgs& a = sp->a;
    memset(&a, 0, sizeof a);
    a.N = N; a.zref = sp->zref;
    snow_density_params(in->snowenv, a.sdp);
    // the rasters as the caller hands them over (the initial snow state among them: what mcf_snowplan_reset goes back to) ...
    each_model_raster(*in, [&](auto* host, auto member, int, bool terrain, const char* name) {
        if (!rc && !terrain) rc = b.up(&(a.*member), host, N, name);
    });
    if (!rc) rc = b.up(&sp->d_dtm, din->dtm, N, "dtm");
    if (!rc && co) rc = coarse_attach(sp, co, umu_out);
    if (rc) return rc;
    sp->d_isnowdg = a.isnowdg; sp->d_isnowdc0 = a.isnowdc; sp->d_ac0 = a.isnowac; sp->d_ag0 = a.isnowag;
    // ... and the state's working copies, handed on from chunk to chunk
    if ((rc = b.up_mut(&sp->d_isnowdc, in->other.isnowdc, N, "other$isnowdc"))) return rc;
    if ((rc = b.up_mut(&sp->d_ac, in->other.isnowac, N, "other$isnowac"))) return rc;
    if ((rc = b.up_mut(&sp->d_ag, in->other.isnowag, N, "other$isnowag"))) return rc;
    a.isnowdc = sp->d_isnowdc; a.isnowac = sp->d_ac; a.isnowag = sp->d_ag;
    double** const per_cell[] = {&sp->d_sumD, &sp->d_meanD, &sp->d_dtms, &sp->d_slope, &sp->d_aspect, &sp->d_svf, &sp->d_tpic, &a.agec, &a.ageg};
    for (double** q : per_cell)
        if ((rc = b.make(q, N))) return rc;
    if ((rc = b.make(&sp->d_sden_na, N))) return rc;
    if ((rc = b.make(&sp->d_daymap, sp->chunk / 24 + 1))) return rc;
    if ((rc = b.make(&sp->d_nosnow, sp->chunk / 24 + 1))) return rc;
    if ((rc = b.make(&sp->d_wsa, 8 * N))) return rc;
    if ((rc = b.make(&sp->d_hor, 24 * N))) return rc;
    if ((rc = b.make(&sp->d_mean2, 2))) return rc;
    if ((rc = b.make(&sp->d_sumws, 2 * kSumParts))) return rc;
    a.slope = sp->d_slope; a.aspect = sp->d_aspect; a.skyview = sp->d_svf; a.wsa = sp->d_wsa; a.hor = sp->d_hor;
    const int64_t CN = (int64_t)sp->chunk * N;
    StepTables tabs;
    if (af) {
        // gridmodelsnow2 on each chunk: the date rows of every step; the cell's part of the sun position and its albedo clock
        // (restarted at the chunk's first step, as every gridmodelsnow2 call does) are the kernel's
        if ((rc = build_step_tables(b, in, true, true, false, &tabs))) return rc;
        sp->dates_tab = tabs.dates;
        if ((rc = up_sites(b, a, in, N))) return rc;
        int f = 0;
        each_model_series(*in, [&](auto* host, auto, auto member, const char*) {
            sp->h_series[f] = host;
            if (!rc) rc = b.make(&sp->d_series[f], CN);
            a.*member = sp->d_series[f++];
        });
        if (rc) return rc;
    } else {
        if ((rc = build_step_tables(b, in, false, true, true, &tabs))) return rc;
        sp->rows_tab = tabs.rows;
        // albedo per chunk (overrides the whole-series scan of build_step_tables)
        const double* d_prec;
        if ((rc = b.up(&d_prec, in->clim.precip, T, "climdata$precip"))) return rc;
        hipLaunchKernelGGL(k_snow_alb_chunks, dim3((unsigned)((sp->nchunks + 63) / 64)), dim3(64), 0, nullptr,
                           const_cast<StepRow*>(sp->rows_tab), d_prec, T, sp->chunk, sp->nchunks);
    }
    double** const series[5] = {&a.Tc, &a.Tg, &a.sdepc, &a.sdepg, &a.sden};
    for (double** q : series)
        if ((rc = b.make(q, CN))) return rc;
    if (!sp->af && (rc = b.make(&a.tzd, (int64_t)std::max(sp->chunk / 24, 1) * N))) return rc;
    hipLaunchKernelGGL(k_add_snow, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, sp->d_dtm, sp->d_isnowdg, 1.0,
                       N, sp->d_dtms);   // int:2562
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    guard.p = nullptr;
    *out = sp;
    return MCF_OK;
}
extern "C" int mcf_snowplan_create(const mcf_snowdriver_in* din, int64_t row0, int64_t rows_total, int32_t device,
                                   mcf_snowplan** out) {
    return snowplan_create(din, row0, rows_total, device, nullptr, nullptr, out);
}
namespace mcf {   // mcf_snowrun.hip: the plan of mcf_snowmodel2_coarse
int snowplan_create_coarse(const mcf_snowcoarse_in* co, double* umu_out, int32_t device, mcf_snowplan** out) {
    return snowplan_create(&co->drv, 0, 0, device, co, umu_out, out);
}
}
extern "C" void mcf_snowplan_destroy(mcf_snowplan* sp) {
    if (!sp) return;
    (void)hipSetDevice(sp->device);
    delete sp;
}
extern "C" int32_t mcf_snowplan_chunks(const mcf_snowplan* sp) { return sp ? sp->nchunks : 0; }
extern "C" int mcf_snowplan_surface(mcf_snowplan* sp, double* host_own) {
    if (!sp || !host_own) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipMemcpy(host_own, sp->d_dtms, (size_t)sp->N * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}
extern "C" int mcf_snowplan_handover(mcf_snowplan* sp, double* host_isnowdc) {
    if (!sp || !host_isnowdc) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipMemcpy(host_isnowdc, sp->d_isnowdc, (size_t)sp->N * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}
extern "C" int mcf_snowplan_surface_partial(mcf_snowplan* sp, double* sum, double* count) {
    if (!sp || !sum || !count) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(sp->device));
    launch_sumcount(sp->d_dtms, sp->N, sp->d_sumws, sp->d_mean2);
    double h[2];
    HIP_TRY(hipMemcpy(h, sp->d_mean2, 16, hipMemcpyDeviceToHost));
    *sum = h[0]; *count = h[1];
    return MCF_OK;
}
// 1 into *diff if the two surfaces differ in any bit (NaN cells compare by pattern)
__global__ __launch_bounds__(256) void k_surface_differs(const double* __restrict__ a, const double* __restrict__ b, int64_t n,
                                                         int32_t* __restrict__ diff) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool d = t < n && __double_as_longlong(a[t]) != __double_as_longlong(b[t]);
    // (a wave that sees the flag up already leaves it alone: with surfaces that differ everywhere — every chunk of the snow season —
    // 40 000 atomics on one address took 0.2 ms of a launch that reads 33 MB)
    if (__builtin_amdgcn_ballot_w64(d) != 0 && (threadIdx.x & 63) == 0 && *(volatile int32_t*)diff == 0) atomicOr(diff, 1);
}
// own block + halo rows, column-major [hn + rows + hs, cols], put together on the device from three column-major pieces
__global__ void k_ext_assemble(double* __restrict__ ext, const double* __restrict__ own, const double* __restrict__ north,
                               const double* __restrict__ south, int64_t rows, int64_t cols, int hn, int hs) {
    const int64_t RB = hn + rows + hs, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= RB * cols) return;
    const int64_t r = t % RB, c = t / RB;
    ext[t] = r < hn ? north[r + (int64_t)hn * c] : r < hn + rows ? own[(r - hn) + rows * c] : south[(r - hn - rows) + (int64_t)hs * c];
}
// the own block's first hn / last hs rows as column-major [h, cols] pieces (what a neighbouring rank receives as its halo)
__global__ void k_halo_pack(const double* __restrict__ own, int64_t rows, int64_t cols, int hn, int hs, double* __restrict__ north,
                            double* __restrict__ south) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, h = hn + hs;
    if (t >= h * cols) return;
    const int64_t i = t % h, c = t / h;
    if (i < hn) north[i + (int64_t)hn * c] = own[i + rows * c];
    else south[(i - hn) + (int64_t)hs * c] = own[(rows - hs + (i - hn)) + rows * c];
}
static int ext_room(mcf_snowplan* sp, int64_t n) {
    if (sp->ext_cap < n) {
        int rc;
        if ((rc = sp->b.make(&sp->d_ext, n))) return rc;
        sp->ext_cap = n;
    }
    return MCF_OK;
}
static int prepare_chunk_on(mcf_snowplan* sp, int32_t ch, const double* d_z, int32_t hn, int32_t hs, double surface_mean,
                            double* tpic_sum, double* tpic_count);

extern "C" int mcf_snowplan_prepare_chunk(mcf_snowplan* sp, int32_t ch, const double* ext, int32_t hn, int32_t hs,
                                          double surface_mean, double* tpic_sum, double* tpic_count) {
    if (!sp || !tpic_sum || !tpic_count) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    if (hn < 0 || hs < 0 || (!ext && (hn || hs))) return mcf::api_fail(MCF_ERR_ARG, "bad halo");
    HIP_TRY(hipSetDevice(sp->device));
    const double* d_z = sp->d_dtms;
    if (ext) {
        const int64_t n = (hn + sp->rows + hs) * sp->cols;
        int rc;
        if ((rc = ext_room(sp, n))) return rc;
        HIP_TRY(hipMemcpy(sp->d_ext, ext, (size_t)n * 8, hipMemcpyHostToDevice));
        d_z = sp->d_ext;
    }
    return prepare_chunk_on(sp, ch, d_z, hn, hs, surface_mean, tpic_sum, tpic_count);
}
extern "C" int mcf_snowplan_pack_halo(mcf_snowplan* sp, int32_t hn, double* d_north, int32_t hs, double* d_south) {
    if (!sp || hn < 0 || hs < 0 || hn > sp->rows || hs > sp->rows || (hn && !d_north) || (hs && !d_south))
        return mcf::api_fail(MCF_ERR_ARG, "bad mcf_snowplan_pack_halo argument");
    HIP_TRY(hipSetDevice(sp->device));
    const int64_t n = (int64_t)(hn + hs) * sp->cols;
    if (n > 0) hipLaunchKernelGGL(k_halo_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, sp->d_dtms, sp->rows, sp->cols, hn, hs, d_north, d_south);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));      // the pieces are the caller's to send from here on
    return MCF_OK;
}
extern "C" int mcf_snowplan_prepare_chunk_dev(mcf_snowplan* sp, int32_t ch, const double* d_north, int32_t hn, const double* d_south,
                                              int32_t hs, double surface_mean, double* tpic_sum, double* tpic_count) {
    if (!sp || !tpic_sum || !tpic_count) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    if (hn < 0 || hs < 0 || (hn && !d_north) || (hs && !d_south)) return mcf::api_fail(MCF_ERR_ARG, "bad halo");
    HIP_TRY(hipSetDevice(sp->device));
    const double* d_z = sp->d_dtms;
    if (hn || hs) {
        const int64_t n = (hn + sp->rows + hs) * sp->cols;
        int rc;
        if ((rc = ext_room(sp, n))) return rc;
        hipLaunchKernelGGL(k_ext_assemble, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, sp->d_ext, sp->d_dtms, d_north, d_south,
                           sp->rows, sp->cols, hn, hs);
        HIP_TRY(hipGetLastError());
        d_z = sp->d_ext;
    }
    return prepare_chunk_on(sp, ch, d_z, hn, hs, surface_mean, tpic_sum, tpic_count);
}
namespace mcf {
// the halo rows a row block hands mcf_snowplan_prepare_chunk for a chunk of aggregation factor af: at least what
// prepare_chunk_on below asks for (the terrain stencil's reach, whole af x af blocks of the tpi)
int64_t snowplan_halo_rows(const mcf_snowplan* sp, int32_t af) { return 100 + 3 * (int64_t)sp->ss + 2 * (int64_t)af; }
// What the row-block driver (mcf_snowrun.hip) does with the listings above.  The snow model's rasters, its terrain aside: given? ...
bool model_rasters_given(const mcf_snow_inputs& in) {
    bool given = true;
    each_model_raster(in, [&](auto* host, auto, int, bool terrain, const char*) { given = given && (host || terrain); });
    return given;
}
// ... and a block's view of them: no terrain; with `rows`, the block's own rows r0 .. r0 + nr of the R x C rasters
void model_rasters_of_block(mcf_snowdriver_in& in, HostCopies* rows, int64_t R, int64_t C, int64_t r0, int64_t nr) {
    each_model_raster(in.base, [&](auto& p, auto, int, bool terrain, const char*) {
        if (terrain) p = nullptr;
        else if (rows) p = rows->rows(p, R, C, r0, nr, 1);
    });
    if (rows) { in.dtm = rows->rows(in.dtm, R, C, r0, nr, 1); in.base.rows = nr; }
}
// the same for gridmicrosnow's static rasters (Smax may be missing) ...
bool micro_rasters_given(const mcf_snow_inputs& in) {
    bool given = true;
    each_micro_raster(in, [&](auto* host, auto, int, bool required, const char*) { given = given && (host || !required); });
    return given;
}
void micro_rasters_of_block(mcf_snow_inputs& in, HostCopies& rows, int64_t R, int64_t C, int64_t r0, int64_t nr) {
    each_micro_raster(in, [&](auto& p, auto, int layers, bool, const char*) { if (p) p = rows.rows(p, R, C, r0, nr, layers); });
    in.rows = nr;
}
// ... and its weather: the field name of the first series that is null (or nullptr) ...
const char* micro_series_missing(const mcf_snow_inputs& in) {
    const char* missing = nullptr;
    each_micro_series(in, [&](auto* host, auto, const char* name) { if (!host && !missing) missing = strchr(name, '$') + 1; });
    return missing;
}
// ... and `in`'s obstime and wind direction — with `series`, its nine [T] series too — cut down to the days of HostCopies::days
void subset_days(mcf_snow_inputs& in, bool series, const int32_t* sub_of_day, int ndays, int nsub, HostCopies& keep) {
    each_obstime(in, [&](auto& p, auto, const char*) { p = keep.days(p, sub_of_day, ndays, nsub); });
    each_micro_series(in, [&](auto& p, auto member, const char*) { if (series || !member) p = keep.days(p, sub_of_day, ndays, nsub); });
    in.tsteps = (int64_t)nsub * 24;
}
// mcf_snowmodel1 / 2's MCF_TIMING line (tools/snow_rate.py reads it)
void snowplan_print_timing(const mcf_snowplan* sp) {
    if (sp->coarse) {
        const double bytes = 13.0 * 8.0 * (double)sp->N * (double)sp->chunk;
        fprintf(stderr, "[mcf] snowmodel2_coarse: %d chunks of %d steps, %lld cells: terrain + tpi %.2f ms, chunk expansion %.3f ms per "
                "chunk (%.1f GB/s written), gridmodelsnow + redistribute %.3f ms per chunk\n", sp->nchunks, sp->chunk, (long long)sp->N,
                sp->t_terrain, sp->t_fine / sp->nchunks, sp->t_fine > 0 ? bytes * sp->nchunks / (sp->t_fine * 1e6) : 0.0,
                sp->t_model / sp->nchunks);
        if (sp->mcoarse && sp->n_micro_fine > 0)      // written bytes from shapes: 9 x 8 B x N x snow steps
            fprintf(stderr, "[mcf] microsnow coarse expansion: %d snow steps, %.3f ms in all, %.3f ms per %d steps (%.1f GB/s written)\n",
                    sp->n_micro_fine, sp->t_micro_fine, sp->t_micro_fine * sp->chunk / sp->n_micro_fine, sp->chunk,
                    9.0 * 8.0 * (double)sp->N * sp->n_micro_fine / (sp->t_micro_fine * 1e6));
        return;
    }
    fprintf(stderr, "[mcf] snowmodel1: %d chunks of %d steps, %lld cells: terrain + tpi %.2f ms, gridmodelsnow + "
            "redistribute %.2f ms\n", sp->nchunks, sp->chunk, (long long)sp->N, sp->t_terrain, sp->t_model);
}
}  // namespace mcf
static int prepare_chunk_on(mcf_snowplan* sp, int32_t ch, const double* d_z, int32_t hn, int32_t hs, double surface_mean,
                            double* tpic_sum, double* tpic_count) {
    int rc, af;
    if ((rc = chunk_af(sp, ch, &af))) return rc;
    const int64_t rows = sp->rows, cols = sp->cols, N = sp->N, RB = hn + rows + hs;
    const int64_t me = std::min(sp->rows_total, cols);
    const bool coarse = (double)af < me / 2.0;
    TpiGeo g;
    g.rows = rows; g.cols = cols; g.RB = RB; g.hn = hn; g.row0 = sp->row0; g.rows_total = sp->rows_total; g.af = af;
    g.NItot = (sp->rows_total + af - 1) / af; g.nJ = (cols + af - 1) / af;
    auto clampI = [&](int64_t i) { return std::min<int64_t>(std::max<int64_t>(i, 0), g.NItot - 1); };
    g.I0 = clampI((int64_t)floor(((double)sp->row0 - (af - 1) / 2.0) / af));
    const int64_t I1 = clampI((int64_t)floor(((double)(sp->row0 + rows - 1) - (af - 1) / 2.0) / af) + 1);
    g.nI = I1 - g.I0 + 1;
    // halo rows this chunk needs (or every row up to the raster edge): the terrain stencil and, for the tpi,
    // whole af x af blocks around the own rows
    const int64_t avail_n = sp->row0, avail_s = sp->rows_total - sp->row0 - rows;
    int64_t need_n = 100 + 2 * sp->ss + sp->ss / 2, need_s = need_n;
    if (coarse) {
        need_n = std::max(need_n, sp->row0 - g.I0 * af);
        need_s = std::max(need_s, std::min<int64_t>((I1 + 1) * af, sp->rows_total) - (sp->row0 + rows));
    }
    if (hn < std::min(need_n, avail_n) || hs < std::min(need_s, avail_s)) {
        char m[200];
        snprintf(m, sizeof m, "snow plan: chunk %d needs %lld / %lld halo rows north / south (or all rows up to the raster edge)",
                 ch, (long long)need_n, (long long)need_s);
        return mcf::api_fail(MCF_ERR_ARG, m);
    }
    TimedSpan span;
    HIP_TRY(span.begin());
    // terrain of dtm + snow (int:2566-2580)
    mcf::TerrainDev td;
    memset(&td, 0, sizeof td);
    td.rows = rows; td.cols = cols; td.halo_north = hn; td.halo_south = hs; td.row0 = sp->row0; td.rows_total = sp->rows_total;
    td.d_dtm = d_z; td.res = sp->res; td.zref = sp->zref; td.agg = sp->ss; td.aspect_na = 180.0;
    td.d_slope = sp->d_slope; td.d_aspect = sp->d_aspect; td.d_hor = sp->d_hor; td.d_svfa = sp->d_svf; td.d_wsa = sp->d_wsa;
    const unsigned gridN = (unsigned)((N + 255) / 256);
    // The terrain arrays are functions of the surface alone.  If this chunk starts from the surface they were last derived
    // from, bit for bit — no snow has lain anywhere since — they are kept (MCF_SNOW_TERRAIN_ALWAYS=1: never).
    const int64_t zn = RB * cols;
    bool same = false;
    static const bool always = getenv("MCF_SNOW_TERRAIN_ALWAYS") != nullptr;
    if (!always) {
        if (!sp->d_zdiff && (rc = sp->b.make(&sp->d_zdiff, 1))) return rc;
        if (sp->d_zlast && sp->zlast_n == zn && sp->zlast_hn == hn && sp->zlast_hs == hs) {
            HIP_TRY(hipMemsetAsync(sp->d_zdiff, 0, 4, nullptr));
            hipLaunchKernelGGL(k_surface_differs, dim3((unsigned)((zn + 255) / 256)), dim3(256), 0, nullptr, d_z, (const double*)sp->d_zlast, zn,
                               sp->d_zdiff);
            int32_t diff = 1;
            HIP_TRY(hipMemcpy(&diff, sp->d_zdiff, 4, hipMemcpyDeviceToHost));
            same = diff == 0;
        }
    }
    if (same) {
        ++sp->terrain_reused;
    } else {
        if ((rc = mcf::terrain_device(td, &sp->twork))) return rc;
        hipLaunchKernelGGL(k_mask2, dim3(gridN), dim3(256), 0, nullptr, sp->d_dtm, N, sp->d_slope, sp->d_aspect);
        ++sp->terrain_refreshed;
        if (!always) {
            if (sp->zlast_cap < zn) {
                if ((rc = sp->b.make(&sp->d_zlast, zn))) return rc;
                sp->zlast_cap = zn;
            }
            HIP_TRY(hipMemcpyAsync(sp->d_zlast, d_z, (size_t)zn * 8, hipMemcpyDeviceToDevice, nullptr));
            sp->zlast_n = zn; sp->zlast_hn = hn; sp->zlast_hs = hs;
        }
    }
    // topographic positioning index (int:2589-2592, 2471-2485)
    if (coarse) {
        if (sp->cm_cap < g.nI * g.nJ) {
            if ((rc = sp->b.make(&sp->d_cm, g.nI * g.nJ))) return rc;
            sp->cm_cap = g.nI * g.nJ;
        }
        hipLaunchKernelGGL(k_tpi_coarse, dim3((unsigned)((g.nI * g.nJ + 255) / 256)), dim3(256), 0, nullptr, d_z, g, sp->d_cm);
        hipLaunchKernelGGL(k_tpi_fine, dim3(gridN), dim3(256), 0, nullptr, d_z, g, (const double*)sp->d_cm, 0.0, sp->tfact,
                           sp->d_tpic);
    } else {
        hipLaunchKernelGGL(k_tpi_fine, dim3(gridN), dim3(256), 0, nullptr, d_z, g, (const double*)nullptr, surface_mean,
                           sp->tfact, sp->d_tpic);
    }
    launch_sumcount(sp->d_tpic, N, sp->d_sumws, sp->d_mean2);
    HIP_TRY(hipGetLastError());
    double h[2];
    HIP_TRY(hipMemcpy(h, sp->d_mean2, 16, hipMemcpyDeviceToHost));
    *tpic_sum = h[0]; *tpic_count = h[1];
    HIP_TRY(span.end(&sp->t_terrain));
    sp->prepared = ch;
    return MCF_OK;
}
// host_step0: the step of the host arrays the chunk's first step goes to (the chunk's own place in whole-series arrays, or 0
// for a caller that takes the chunk into a chunk-sized buffer); fill_tail: whole-series arrays — the steps no chunk covers
// become NA behind the last chunk
// row_pitch: 0 / rows = dense [rows, cols, steps] host arrays; > rows: the host arrays are row blocks of a taller column-major
// raster with that many rows per column, written in place (one strided DMA per series: no block-sized host buffer, no scatter)
static int run_chunk_to(mcf_snowplan* sp, int32_t ch, double tpic_mean, const mcf_snowdriver_out* out, int64_t host_step0, bool fill_tail,
                        int64_t row_pitch);
extern "C" int mcf_snowplan_run_chunk(mcf_snowplan* sp, int32_t ch, double tpic_mean, mcf_snowdriver_out* out) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    return run_chunk_to(sp, ch, tpic_mean, out, (int64_t)ch * sp->chunk, true, 0);
}
extern "C" int mcf_snowplan_run_chunk_pitched(mcf_snowplan* sp, int32_t ch, double tpic_mean, const mcf_snowdriver_out* out,
                                              int64_t row_pitch) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (row_pitch != 0 && row_pitch < sp->rows) return mcf::api_fail(MCF_ERR_ARG, "row_pitch smaller than rows");
    return run_chunk_to(sp, ch, tpic_mean, out, (int64_t)ch * sp->chunk, true, row_pitch);
}
static int run_chunk_to(mcf_snowplan* sp, int32_t ch, double tpic_mean, const mcf_snowdriver_out* out, int64_t host_step0, bool fill_tail,
                        int64_t row_pitch) {
    if (!sp || !out) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (row_pitch <= 0) row_pitch = sp->rows;
    if (ch != sp->prepared) return mcf::api_fail(MCF_ERR_STATE, "snow plan: run_chunk needs prepare_chunk of the same chunk first");
    HIP_TRY(hipSetDevice(sp->device));
    sp->mm_chunk = -1;
    if ((size_t)ch < sp->kept.size() && sp->kept[(size_t)ch].Tc) {     // a set kept from an earlier run of this chunk is stale now
        sp->pool.push_back(sp->kept[(size_t)ch]);
        sp->kept[(size_t)ch] = mcf_snowplan::Kept();
    }
    const int64_t N = sp->N;
    const int k0 = ch * sp->chunk, ns = std::min(sp->chunk, sp->T - k0);
    const unsigned gridN = (unsigned)((N + 255) / 256);
    TimedSpan span;
    HIP_TRY(span.begin());
    ModelArgs a = sp->a;
    a.rows = sp->af ? nullptr : sp->rows_tab + k0;            // gridmodelsnow1 on the chunk (int:2587)
    a.dates = sp->af ? sp->dates_tab + k0 : nullptr;          // gridmodelsnow2 (int:2979)
    a.tsteps = ns;
    if (sp->coarse) {                                         // the chunk's hours expanded from the resident coarse arrays
        if (const int rc = coarse_fill_chunk(sp, k0, ns)) return rc;
        HIP_TRY(span.begin());                                // (the expansion has its own span: the model's starts behind it)
    } else if (sp->af)                                        // the chunk's slices of the caller's series: [N][T], a step's raster contiguous
        for (int f = 0; f < 13; ++f)
            HIP_TRY(hipMemcpyAsync(sp->d_series[f], sp->h_series[f] + (int64_t)k0 * N, (size_t)ns * N * 8, hipMemcpyHostToDevice, nullptr));
    // ... with the redistribution by the topographic position index and the hand-over fused in (ModelArgs)
    a.tpic = sp->d_tpic; a.tpimean = tpic_mean; a.dtm = sp->d_dtm;
    a.isnowdc_out = sp->d_isnowdc; a.dtms = sp->d_dtms; a.isnowac_out = sp->d_ac; a.isnowag_out = sp->d_ag;
    {   // series nobody will read are not written (mcf_snowplan_set_series): the kernel's stores are what a snow-free chunk costs
        const uint32_t m = sp->series_mask;
        double* const hostp[5] = {out->Tc, out->Tg, out->totalSWE, out->groundsnowdepth, out->snowden};
        for (int v = 0; v < 5; ++v)
            if (!((m >> v) & 1u) && hostp[v]) return mcf::api_fail(MCF_ERR_STATE, "snow plan: a series the caller asks for is switched off (mcf_snowplan_set_series)");
        if (!(m & 1u)) a.Tc = nullptr;
        if (!(m & 2u)) a.Tg = nullptr;
        if (!(m & 4u)) a.sdepc = nullptr;
        if (!(m & 8u)) a.sdepg = nullptr;
        if (!(m & 16u)) a.sden = nullptr;
        sp->series_valid = m;
    }
    if (sp->af) hipLaunchKernelGGL(k_snowmodel<true>, dim3(gridN), dim3(256), 0, nullptr, a, a.rows, a.dates);
    else hipLaunchKernelGGL(k_snowmodel<false>, dim3(gridN), dim3(256), 0, nullptr, a, a.rows, a.dates);
    if (sp->coarse) coarse_clean_chunk(sp, a.Tc, a.Tg, a.sdepg, a.sdepc, a.sden, ns);      // `.cleansmod` (the hand-over state is written already)
    HIP_TRY(hipGetLastError());
    HIP_TRY(span.end(&sp->t_model));
    double* hostv[5] = {out->Tc, out->Tg, out->groundsnowdepth, out->totalSWE, out->snowden};
    double* devv[5] = {a.Tc, a.Tg, a.sdepg, a.sdepc, a.sden};
    const int64_t HS = row_pitch * sp->cols;        // host doubles per step
    for (int v = 0; v < 5; ++v) {
        if (!hostv[v]) continue;
        if (row_pitch == sp->rows) HIP_TRY(sp->dl.dense(hostv[v] + host_step0 * N, devv[v], (size_t)ns * N * 8));
        else HIP_TRY(sp->dl.pitched(hostv[v] + host_step0 * HS, (size_t)row_pitch * 8, devv[v], (size_t)sp->rows * 8, (size_t)(sp->cols * ns)));
    }
    if (fill_tail && ch == sp->nchunks - 1) {   // steps that no chunk covers stay NA (R pre-fills its arrays, int:2554-2558)
        union { uint64_t u; double d; } na; na.u = kNaRealBits;
        const int covered = std::min(sp->T, sp->nchunks * sp->chunk);
        for (double* h : hostv)
            if (h)
                for (int64_t lc = (int64_t)covered * sp->cols; lc < (int64_t)sp->T * sp->cols; ++lc)
                    for (int64_t r = 0; r < sp->rows; ++r) h[r + row_pitch * lc] = na.d;
    }
    if (sp->coarse)                                           // pointm$umu leaves from the chunk's slab; behind the last chunk it alone is expanded
        if (const int rc = coarse_umu_out(sp, k0, ns, fill_tail && ch == sp->nchunks - 1)) return rc;
    sp->prepared = -1;
    return MCF_OK;
}

// applycpp3 over device-resident data: [N][tsteps] -> result / count [tsteps] on the host
static int apply3_device(const double* d_a, int64_t N, int64_t tsteps, int fun, double* result, double* count) {
    int rc;
    mcf::DevOwner b;
    double *d_r, *d_c = nullptr;
    if ((rc = b.make(&d_r, tsteps))) return rc;
    if (count && (rc = b.make(&d_c, tsteps))) return rc;
    // enough workgroups to keep the memory system busy whatever the ratio of cells to steps
    int parts = (int)std::min<int64_t>(64, std::max<int64_t>(1, N / 16384));
    if (tsteps * parts < 2048) parts = (int)std::min<int64_t>(64, std::max<int64_t>(parts, (2048 + tsteps - 1) / tsteps));
    double* d_ws;
    if ((rc = b.make(&d_ws, tsteps * parts * 2))) return rc;
    hipLaunchKernelGGL(k_apply3_part, dim3((unsigned)parts, (unsigned)tsteps), dim3(256), 0, nullptr, d_a, N, fun, parts, d_ws);
    hipLaunchKernelGGL(k_apply3_fin, dim3((unsigned)((tsteps + 255) / 256)), dim3(256), 0, nullptr, d_ws, tsteps, fun, parts, d_r,
                       d_c);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(result, d_r, (size_t)tsteps * 8, hipMemcpyDeviceToHost));
    if (count) HIP_TRY(hipMemcpy(count, d_c, (size_t)tsteps * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}
extern "C" int mcf_snowplan_apply3(mcf_snowplan* sp, int32_t chunk, int32_t fun, double* result, double* count) {
    if (!sp || !result || fun < 0 || fun > 3) return mcf::api_fail(MCF_ERR_ARG, "bad mcf_snowplan_apply3 argument");
    if (chunk < 0 || chunk >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    HIP_TRY(hipSetDevice(sp->device));
    const int ns = std::min(sp->chunk, sp->T - chunk * sp->chunk);
    // (sdepc holds totalSWE after the redistribution; the series are the ones of the chunk run last)
    if (!(sp->series_valid & 4u)) return mcf::api_fail(MCF_ERR_STATE, "snow plan: the chunk's totalSWE series was switched off (mcf_snowplan_set_series)");
    if (fun < 2) return apply3_device(sp->a.sdepc, sp->N, ns, fun, result, count);
    if (sp->mm_chunk != chunk) {
        const int64_t N = sp->N, C = sp->chunk;
        int parts = (int)std::min<int64_t>(64, std::max<int64_t>(1, N / 16384));      // (apply3_device's choice: same partials, same bits)
        if ((int64_t)ns * parts < 2048) parts = (int)std::min<int64_t>(64, std::max<int64_t>(parts, (2048 + ns - 1) / ns));
        const int pmax = 64;
        if (!sp->d_mm) {
            int rc;
            if ((rc = sp->b.make(&sp->d_mm, 2 * C * pmax * 2 + 4 * C))) return rc;
            sp->mm_host.assign((size_t)(4 * C), 0.0);
        }
        double *ws_max = sp->d_mm, *ws_min = sp->d_mm + C * pmax * 2, *d_r = sp->d_mm + 2 * C * pmax * 2;
        hipLaunchKernelGGL(k_apply3_minmax_part, dim3((unsigned)parts, (unsigned)ns), dim3(256), 0, nullptr, (const double*)sp->a.sdepc, N, parts,
                           ws_max, ws_min);
        hipLaunchKernelGGL(k_apply3_fin, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, nullptr, (const double*)ws_max, (int64_t)ns, 2, parts, d_r, d_r + C);
        hipLaunchKernelGGL(k_apply3_fin, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, nullptr, (const double*)ws_min, (int64_t)ns, 3, parts, d_r + 2 * C,
                           d_r + 3 * C);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(sp->mm_host.data(), d_r, (size_t)(4 * C) * 8, hipMemcpyDeviceToHost));
        sp->mm_chunk = chunk;
    }
    const double* h = sp->mm_host.data() + (fun == 2 ? 0 : 2 * sp->chunk);
    memcpy(result, h, (size_t)ns * 8);
    if (count) memcpy(count, h + sp->chunk, (size_t)ns * 8);
    return MCF_OK;
}
extern "C" int mcf_applycpp3(const double* a, int64_t rows, int64_t cols, int64_t tsteps, int32_t fun, double* result,
                             double* count, int32_t device) {
    if (!a || !result || rows <= 0 || cols <= 0 || tsteps <= 0 || tsteps > 65535 || fun < 0 || fun > 3)
        return mcf::api_fail(MCF_ERR_ARG, "bad applycpp3 argument");
    int rc;
    if ((rc = pick_device(device))) return rc;
    const int64_t N = rows * cols;
    if ((rc = check_room(N * tsteps * 8))) return rc;
    mcf::DevOwner b;
    const double* d_a;
    if ((rc = b.up(&d_a, a, N * tsteps, "a"))) return rc;
    return apply3_device(d_a, N, tsteps, (int)fun, result, count);
}

// k_tpi_fine's result divided by its raster mean
__global__ __launch_bounds__(256) void k_scale_by_mean(double* __restrict__ x, int64_t N, const double* __restrict__ sumcount) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) x[i] /= sumcount[0] / sumcount[1];
}
namespace {
// `.tpicalc(af, min(rows, cols), z, tfact)` of a whole raster held on the device, into d_t: the chunk loop's kernels with one
// block.  af < min(dim) / 2: block means (d_cm: tpi_coarse_cells doubles) resampled; else the raster mean `zmean` =
// mean(z, na.rm = TRUE) in their place.  d_ws: 2 * kSumParts doubles, d_m2: 2.  Launches only, all on `stream`.
bool tpi_is_coarse(int64_t rows, int64_t cols, int af) { return (double)af < std::min(rows, cols) / 2.0; }
int64_t tpi_coarse_cells(int64_t rows, int64_t cols, int af) { return ((rows + af - 1) / af) * ((cols + af - 1) / af); }
void tpi_raster(const double* d_z, int64_t rows, int64_t cols, int af, double tfact, double zmean, double* d_t, double* d_ws, double* d_m2,
                double* d_cm, hipStream_t stream) {
    const int64_t N = rows * cols;
    TpiGeo g;
    g.rows = rows; g.cols = cols; g.RB = rows; g.hn = 0; g.row0 = 0; g.rows_total = rows; g.af = af;
    g.NItot = (rows + af - 1) / af; g.nJ = (cols + af - 1) / af; g.I0 = 0; g.nI = g.NItot;
    const unsigned gridN = (unsigned)((N + 255) / 256);
    if (tpi_is_coarse(rows, cols, af)) {
        hipLaunchKernelGGL(k_tpi_coarse, dim3((unsigned)((g.nI * g.nJ + 255) / 256)), dim3(256), 0, stream, d_z, g, d_cm);
        hipLaunchKernelGGL(k_tpi_fine, dim3(gridN), dim3(256), 0, stream, d_z, g, (const double*)d_cm, 0.0, tfact, d_t);
    } else {
        hipLaunchKernelGGL(k_tpi_fine, dim3(gridN), dim3(256), 0, stream, d_z, g, (const double*)nullptr, zmean, tfact, d_t);
    }
    launch_sumcount(d_t, N, d_ws, d_m2, stream);
    hipLaunchKernelGGL(k_scale_by_mean, dim3(gridN), dim3(256), 0, stream, d_t, N, (const double*)d_m2);
}
}  // namespace
extern "C" int mcf_tpicalc(int64_t rows, int64_t cols, const double* dtm, int32_t af, double tfact, double* tpic, int32_t device) {
    if (!dtm || !tpic || rows <= 0 || cols <= 0) return mcf::api_fail(MCF_ERR_ARG, "mcf_tpicalc: null argument or empty raster");
    if (af < 1) return mcf::api_fail(MCF_ERR_ARG, "mcf_tpicalc: aggregation factor below 1 (terra::aggregate fails)");
    int rc;
    if ((rc = pick_device(device))) return rc;
    const int64_t N = rows * cols;
    if ((rc = check_room(N * 24))) return rc;
    mcf::DevOwner b;
    const double* d_z;
    double *d_t, *d_ws, *d_m2, *d_cm = nullptr;
    if ((rc = b.up(&d_z, dtm, N, "dtm"))) return rc;
    if ((rc = b.make(&d_t, N))) return rc;
    if ((rc = b.make(&d_ws, 2 * kSumParts))) return rc;
    if ((rc = b.make(&d_m2, 2))) return rc;
    double zmean = 0.0;
    if (tpi_is_coarse(rows, cols, af)) {
        if ((rc = b.make(&d_cm, tpi_coarse_cells(rows, cols, af)))) return rc;
    } else {
        launch_sumcount(d_z, N, d_ws, d_m2);
        double h[2];
        HIP_TRY(hipMemcpy(h, d_m2, 16, hipMemcpyDeviceToHost));
        zmean = h[0] / h[1];
    }
    tpi_raster(d_z, rows, cols, af, tfact, zmean, d_t, d_ws, d_m2, d_cm, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(tpic, d_t, (size_t)N * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}

// ---- `.snowmodelq1`, the fast snow method of a subset run (R/internal.R "int:" 2627-2776), as one device-resident call -------
namespace {
// canintfrac (cpp:5417-5450): the canopy's share of a snowfall of `prec` mm, one lane per cell.  sint: canopysnowintCpp's
// Sh (0.26 + 46 / rhos) of the one air temperature, formed by the host.  With dg: isnowdg = (1 - intfrac) isnowdc (int:2716).
struct CanIntArgs {
    int64_t N;
    const double *hgt, *pai;
    double uf, prec, sint, Li;
    double* frac;
    const double* dc;
    double* dg;
};
__global__ __launch_bounds__(256) void k_canintfrac(CanIntArgs a) {
    snow::snow_tables_init();
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.N) return;
    const double h = a.hgt[c];
    double f = 0.5;                                            // no snowfall in the series (prec 0 or NaN)
    if (isnan(h)) f = na_real();
    else if (a.prec > 0.0) f = canopy_snow_interception(h, a.pai[c], a.uf, a.prec, a.sint, a.Li) / a.prec;
    a.frac[c] = f;
    if (a.dg) a.dg[c] = (1 - f) * a.dc[c];
}
double canopy_sint(double tc) { return 6.2 * (0.26 + 46 / (67.92 + 51.25 * exp(tc / 2.59))); }   // cpp:3728-3729

// The pack between two selected days (int:2724-2741): meltmu (cpp:5454-5492) over the gap's hours and the point model's balance
// scaled by it, one lane per cell.  The gap's two series are the same for every lane: `st` / `tc` are the device copies of the
// WHOLE series as `__restrict__` kernel arguments (see k_snowmodel's head), hour k of the gap is element start + step k of them
// (step = -1: R's `a:b` counting down), so a step's pair comes through scalar loads and nothing is staged per day.  No FMA
// contraction: the sums are the host entry's (mcf_meltmu) bit for bit, and a pack that melts to +-0 does so on both sides.
// dc == null: meltmu alone (mcf_meltmu_device); mu: null or where the multiplier goes.
struct GapArgs {
    int64_t N, start, len;
    int32_t step;
    double dhp;                                  // sum of the gap's positive sstemp
    double subrain, tempmelt, fall, kc, kg;      // sum(sublmelt) + sum(rainmelt), sum(tempmelt), sum(snow / 1000), 1000 / mean(sdenc), 1000 / mean(sdeng)
    const double *skyview, *pai, *intfrac;
    double *dc, *dg, *mu;
};
__global__ __launch_bounds__(256) void k_gap_balance(GapArgs a, const double* __restrict__ st, const double* __restrict__ tc) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.N) return;
    const double sv = a.skyview[c];
    double mu = 1.0;                                           // a frozen gap: 1 everywhere, NA cells included (cpp:5484-5490)
    if (a.dhp > 0.0) {
        if (isnan(sv)) {
            mu = na_real();
        } else {
            double dhm = 0.0;
            for (int64_t k = 0; k < a.len; ++k) {
                const int64_t i = a.start + (int64_t)a.step * k;
                const double t = tc[i];
                const double s2 = (st[i] - t) * sv + t;
                if (s2 > 0.0) dhm += s2;
            }
            mu = dhm / a.dhp;
        }
    }
    if (a.mu) a.mu[c] = mu;
    if (!a.dc) return;
    const double melt = a.subrain + mu * a.tempmelt;
    const double balancec = a.fall - melt;
    const double balanceg = (1 - a.intfrac[c]) * a.fall - exp(-a.pai[c]) * melt;
    double dc = a.dc[c] + balancec * a.kc, dg = a.dg[c] + balanceg * a.kg;
    if (dc < 0) dc = 0;                                        // `x[x < 0] <- 0`: NA stays NA
    if (dg < 0) dg = 0;
    a.dc[c] = dc; a.dg[c] = dg;
}

// A selected day's redistribution and hand-over (int:2744-2771; the operations and their order: oracle/snowfast_oracle.py
// 131-149), one lane per cell over the day's 24 steps of gridmodelsnow1's raw depths.  In place: the pack depth's slab takes
// totalSWE, the ground depth's the redistributed ground depth — each only if it is wanted (null: not stored); step 23's depths
// are the next day's isnowdc / isnowdg.  No FMA contraction, as above.
struct DayRedistArgs {
    int64_t N;
    const double *tpi, *sdepc, *sdepg, *sden;    // raw [N][24]
    double *swe, *gd;                            // [N][24] or null (may be sdepc / sdepg)
    double *dc, *dg;                             // [N] in: the depths the day started from; out: the next day's
};
__global__ __launch_bounds__(256) void k_day_redistribute(DayRedistArgs a) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.N) return;
    const double tpi = a.tpi[c], c0 = a.dc[c], g0 = a.dg[c];
    double sdc = c0, sdg = g0;
    for (int k = 0; k < 24; ++k) {
        const int64_t o = c + a.N * k;
        const double dsnow = a.sdepc[o] - c0, dsnowg = a.sdepg[o] - g0;
        const double dsnowg2 = dsnowg * tpi;
        sdc = (dsnow - dsnowg) + dsnowg2 + c0;
        sdg = dsnowg2 + g0;
        if (sdc < 0) sdc = 0;
        if (sdg < 0) sdg = 0;
        if (a.swe) a.swe[o] = sdc * a.sden[o];
        if (a.gd) a.gd[o] = sdg;
    }
    a.dc[c] = sdc; a.dg[c] = sdg;
}

struct Streams {   // streams released on every exit path
    std::vector<hipStream_t> s;
    ~Streams() { for (hipStream_t x : s) (void)hipStreamDestroy(x); }
    hipError_t make(hipStream_t* out) {
        hipError_t r = hipStreamCreateWithFlags(out, hipStreamNonBlocking);
        if (r == hipSuccess) s.push_back(*out);
        return r;
    }
};

// the gap in front of selected day `day`: R's `(ped + 1):(subs[24 day] - 1)` as (0-based start, step, length)
struct Gap { int64_t start, len; int32_t step; };
Gap gap_of_day(const int64_t* subs, int64_t day) {
    const int64_t ped = day ? subs[24 * day - 1] : 0, a = ped + 1, b = subs[24 * day] - 1;
    Gap g;
    g.start = a - 1; g.step = a <= b ? 1 : -1; g.len = (a <= b ? b - a : a - b) + 1;
    return g;
}
// af of a selected day (int:2748-2749): round(10 sqrt(mean wind) / res), half to even
double day_af(const double* wind24, double res) {
    double s = 0.0;
    for (int k = 0; k < 24; ++k) s += wind24[k];
    return nearbyint(10 * sqrt(s / 24) / res);
}

constexpr int kTpiCache = 8;    // position indices kept per call, one per distinct af (a [rows, cols] raster each)

// What both fast methods refuse about `subs` and the days' aggregation factors.  wind / windname: the series of the selected
// hours the factor is formed from; first_day: the refusal of a first selected day that is the series' first (null: the method
// runs it).
int subs_af_checks(const char* entry, const int64_t* subs, int64_t n, int64_t n_all, const char* first_day, const double* wind,
                   const char* windname, double res) {
    char m[240];
    for (int64_t k = 0; k < n; ++k) {
        if (subs[k] < 1 || subs[k] > n_all) {
            snprintf(m, sizeof m, "%s: subs[%lld] = %lld is outside 1..n_all = %lld", entry, (long long)k, (long long)subs[k], (long long)n_all);
            return mcf::api_fail(MCF_ERR_ARG, m);
        }
        if (k && subs[k] <= subs[k - 1]) {
            snprintf(m, sizeof m, "%s: subs is not increasing at position %lld", entry, (long long)k);
            return mcf::api_fail(MCF_ERR_ARG, m);
        }
    }
    if (first_day && subs[0] - 1 <= 1) return mcf::api_fail(MCF_ERR_ARG, std::string(entry) + ": " + first_day);
    for (int64_t d = 0; d < n / 24; ++d)
        if (!(day_af(wind + 24 * d, res) >= 1.0)) {
            snprintf(m, sizeof m, "%s: aggregation factor round(10*sqrt(mean %s)/res) of selected day %lld is 0 (terra::aggregate fails)",
                     entry, windname, (long long)d);
            return mcf::api_fail(MCF_ERR_ARG, m);
        }
    return MCF_OK;
}

// ---- the day loop of the fast methods ------------------------------------------------------------------------------------------
// What a selected day computes into, [N][24] each (null: not wanted; umu: array weather only).  There are two sets: day d + 1
// computes into one while day d's wanted series leave the other.
struct DaySet { double *Tc = nullptr, *Tg = nullptr, *sdepc = nullptr, *sdepg = nullptr, *sden = nullptr, *umu = nullptr; };
// One of a method's own steps of a selected day: launches only, on the stream handed to it.  name: its sum in the MCF_TIMING line.
struct DayStage {
    const char* name;
    std::function<void(int day, const DaySet& set, hipStream_t stream)> launch;
};
// Everything `.snowmodelq1` and `.snowmodelq2` do alike.  The constructor plans on the host; prepare() puts the dtm and the
// pack depth on the device and makes what no day changes; run() is the loop over the selected days:
//     the method's stages | the day's position index | k_day_redistribute | the method's stages behind it
// on one stream, day d - 1's wanted series leaving meanwhile.  What differs between the methods is a stage or a value handed in.
struct DayLoop {
    int64_t rows, cols, N, cm_cells = 1;
    int D, nsets, nser, nslots;                  // selected days; output sets; series per set; position indices kept
    std::vector<int> af;                         // per day: round(10 sqrt(mean wind) / res)
    const mcf_snowdriver_in& drv;
    double* hostv[6];                            // the caller's Tc, Tg, groundsnowdepth, totalSWE, snowden, umu (null: not wanted)
    bool want_den, timing;
    const double* d_dtm = nullptr;
    double *d_dc = nullptr, *d_dg = nullptr;     // the pack and ground depths a day starts from, handed on by k_day_redistribute
    double *d_slope = nullptr, *d_aspect = nullptr, *d_svf = nullptr, *d_wsa = nullptr, *d_hor = nullptr;
    double *d_ws = nullptr, *d_m2 = nullptr, *d_cm = nullptr;   // launch_sumcount's and tpi_raster's scratch
    double zmean = 0.0;                          // mean(dtm, na.rm = TRUE): `.tpicalc`'s raster-mean branch
    Events tev;                                  // around the terrain

    // wind: the series of the selected hours the aggregation factors are formed from
    DayLoop(const mcf_snowdriver_in& drv_, const double* wind, const mcf_snowdriver_out& sm, double* umu)
        : rows(drv_.base.rows), cols(drv_.base.cols), N(rows * cols), D((int)(drv_.base.tsteps / 24)), nsets(std::min(2, D)), af((size_t)D),
          drv(drv_), hostv{sm.Tc, sm.Tg, sm.groundsnowdepth, sm.totalSWE, sm.snowden, umu}, want_den(sm.snowden || sm.totalSWE),
          timing(getenv("MCF_TIMING") != nullptr) {
        nser = 2 + (sm.Tc != nullptr) + (sm.Tg != nullptr) + want_den + (umu != nullptr);
        // the distinct factors, in the order they are met, share the cache's slots
        std::vector<int> distinct;
        for (int d = 0; d < D; ++d) {
            af[(size_t)d] = (int)std::min(day_af(wind + 24 * d, drv.res), 1e9);
            if (std::find(distinct.begin(), distinct.end(), af[(size_t)d]) == distinct.end()) distinct.push_back(af[(size_t)d]);
            if (tpi_is_coarse(rows, cols, af[(size_t)d])) cm_cells = std::max(cm_cells, tpi_coarse_cells(rows, cols, af[(size_t)d]));
        }
        nslots = (int)std::min<size_t>(kTpiCache, distinct.size());
    }

    // dtm and isnowdc up, the terrain of the bare dtm (int:2690-2706, 3171-3190: it does not change between the days) and its mean
    int prepare(mcf::DevOwner& b, ModelArgs& a) {
        int rc;
        if ((rc = b.up(&d_dtm, drv.dtm, N, "dtm"))) return rc;
        if ((rc = b.up_mut(&d_dc, drv.base.other.isnowdc, N, "other$isnowdc"))) return rc;
        double** const per_cell[] = {&d_dg, &d_slope, &d_aspect, &d_svf};
        for (double** q : per_cell)
            if ((rc = b.make(q, N))) return rc;
        if ((rc = b.make(&d_wsa, 8 * N))) return rc;
        if ((rc = b.make(&d_hor, 24 * N))) return rc;
        if ((rc = b.make(&d_ws, 2 * kSumParts))) return rc;
        if ((rc = b.make(&d_m2, 2))) return rc;
        if ((rc = b.make(&d_cm, cm_cells))) return rc;
        a.isnowdc = d_dc; a.isnowdg = d_dg;
        a.slope = d_slope; a.aspect = d_aspect; a.skyview = d_svf; a.wsa = d_wsa; a.hor = d_hor;
        if (timing) { HIP_TRY(tev.make(2)); HIP_TRY(hipEventRecord(tev.e[0], nullptr)); }
        mcf::TerrainDev td;
        memset(&td, 0, sizeof td);
        td.rows = rows; td.cols = cols; td.row0 = 0; td.rows_total = rows;
        td.d_dtm = d_dtm; td.res = drv.res; td.zref = drv.base.other.zref; td.agg = drv.res <= 100 ? 10 : 1; td.aspect_na = 180.0;
        td.d_slope = d_slope; td.d_aspect = d_aspect; td.d_hor = d_hor; td.d_svfa = d_svf; td.d_wsa = d_wsa;
        if ((rc = mcf::terrain_device(td))) return rc;
        hipLaunchKernelGGL(k_mask2, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, d_dtm, N, d_slope, d_aspect);
        if (timing) HIP_TRY(hipEventRecord(tev.e[1], nullptr));
        launch_sumcount(d_dtm, N, d_ws, d_m2);
        double h[2];
        HIP_TRY(hipMemcpy(h, d_m2, 16, hipMemcpyDeviceToHost));
        zmean = h[0] / h[1];
        return MCF_OK;
    }

    // The selected days.  stages: in front of the day's position index, each timed under its name; behind: after the
    // redistribution, timed with it.  entry, sizes: the head of the MCF_TIMING line ("<entry>: D days, N cells<sizes>").
    int run(mcf::DevOwner& b, const char* entry, const std::string& sizes, const std::vector<DayStage>& stages,
            const std::vector<DayStage>& behind) {
        int rc;
        const int64_t DN = 24 * N;
        DaySet sets[2];
        for (int s = 0; s < nsets; ++s) {
            if (hostv[0] && (rc = b.make(&sets[s].Tc, DN))) return rc;
            if (hostv[1] && (rc = b.make(&sets[s].Tg, DN))) return rc;
            if ((rc = b.make(&sets[s].sdepc, DN))) return rc;
            if ((rc = b.make(&sets[s].sdepg, DN))) return rc;
            if (want_den && (rc = b.make(&sets[s].sden, DN))) return rc;
            if (hostv[5] && (rc = b.make(&sets[s].umu, DN))) return rc;
        }
        // `.tpicalc` of the bare dtm (the depth the reference stacks on it is still zero when read, int:2753) per distinct af
        struct Slot { int af = 0; double* tpi = nullptr; } slots[kTpiCache];
        for (int s = 0; s < nslots; ++s)
            if ((rc = b.make(&slots[s].tpi, N))) return rc;
        int next_slot = 0, tpi_computed = 0;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        Streams streams;
        hipStream_t cs, ds;                       // the days' kernels; the stream the downloads are ordered on (idle: the host waits for a set's day itself)
        HIP_TRY(streams.make(&cs));
        HIP_TRY(streams.make(&ds));
        Events done;
        HIP_TRY(done.make(2));
        mcf::ToHost dl;
        double t_download = 0.0;
        auto download = [&](int d) -> hipError_t {                 // day d's wanted series, from the set it was computed into
            hipError_t e = hipEventSynchronize(done.e[(size_t)(d & 1)]);
            const auto t0 = std::chrono::steady_clock::now();
            const DaySet& s = sets[d % nsets];
            double* const devv[6] = {s.Tc, s.Tg, s.sdepg, s.sdepc, s.sden, s.umu};
            for (int v = 0; v < 6 && e == hipSuccess; ++v)
                if (hostv[v]) e = dl.dense(hostv[v] + (int64_t)d * DN, devv[v], (size_t)DN * 8, ds);
            t_download += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            return e;
        };
        // a day's timing events: one in front of each stage, of the position index and of the redistribution, one behind
        const int S = (int)stages.size(), E = S + 3;
        Events evs;
        if (timing) HIP_TRY(evs.make(E * D));
        const unsigned gridN = (unsigned)((N + 255) / 256);
        for (int d = 0; d < D; ++d) {
            hipEvent_t* te = timing ? &evs.e[(size_t)(E * d)] : nullptr;
            const DaySet& s = sets[d % nsets];
            for (int q = 0; q < S; ++q) {
                if (te) HIP_TRY(hipEventRecord(te[q], cs));
                stages[(size_t)q].launch(d, s, cs);
            }
            if (te) HIP_TRY(hipEventRecord(te[S], cs));
            // the day's position index: kept per af; beyond the cache's slots the oldest is computed over
            const double* d_tpi = nullptr;
            for (int q = 0; q < nslots; ++q)
                if (slots[q].af == af[(size_t)d]) d_tpi = slots[q].tpi;
            if (!d_tpi) {
                Slot& sl = slots[next_slot];
                next_slot = (next_slot + 1) % nslots;
                sl.af = af[(size_t)d];
                tpi_raster(d_dtm, rows, cols, sl.af, drv.tfact, zmean, sl.tpi, d_ws, d_m2, d_cm, cs);
                d_tpi = sl.tpi;
                ++tpi_computed;
            }
            if (te) HIP_TRY(hipEventRecord(te[S + 1], cs));
            DayRedistArgs ra;
            ra.N = N; ra.tpi = d_tpi; ra.sdepc = s.sdepc; ra.sdepg = s.sdepg; ra.sden = s.sden;
            ra.swe = hostv[3] ? s.sdepc : nullptr; ra.gd = hostv[2] ? s.sdepg : nullptr;
            ra.dc = d_dc; ra.dg = d_dg;
            hipLaunchKernelGGL(k_day_redistribute, dim3(gridN), dim3(256), 0, cs, ra);
            for (const DayStage& st : behind) st.launch(d, s, cs);
            if (te) HIP_TRY(hipEventRecord(te[S + 2], cs));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(done.e[(size_t)(d & 1)], cs));
            // the day before leaves while this one computes (with one set there is one day)
            if (d > 0) HIP_TRY(download(d - 1));
        }
        HIP_TRY(download(D - 1));
        HIP_TRY(hipDeviceSynchronize());
        if (timing) {
            float ms = 0;
            std::vector<double> t((size_t)(S + 2), 0.0);
            for (int d = 0; d < D; ++d)
                for (int q = 0; q < S + 2; ++q) {
                    HIP_TRY(hipEventElapsedTime(&ms, evs.e[(size_t)(E * d + q)], evs.e[(size_t)(E * d + q + 1)]));
                    t[(size_t)q] += ms;
                }
            HIP_TRY(hipEventElapsedTime(&ms, tev.e[0], tev.e[1]));
            fprintf(stderr, "[mcf] %s: %d days, %lld cells%s: terrain %.2f ms, ", entry, D, (long long)N, sizes.c_str(), ms);
            for (int q = 0; q < S; ++q) fprintf(stderr, "%s %.2f ms, ", stages[(size_t)q].name, t[(size_t)q]);
            fprintf(stderr, "tpi %.2f ms (%d of %d days computed), redistribute %.2f ms, downloads %.2f ms of host time\n", t[(size_t)S],
                    tpi_computed, D, t[(size_t)S + 1], t_download * 1e3);
        }
        return MCF_OK;
    }
};

int snowmodelq1_checks(const mcf_snowfast_in* fi, const mcf_snowdriver_out* out) {
    if (!fi || !out) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowmodelq1: null argument");
    const mcf_snow_inputs* in = &fi->drv.base;
    if (in->tsteps <= 0 || in->tsteps % 24)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_snowmodelq1: the fast snow method works on whole selected days (tsteps = 24 x days, at least one)");
    if (const int rc = common_checks(in)) return rc;
    if (in->array_forcing != 0)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_snowmodelq1: array_forcing must be 0 (vector forcing; array weather is mcf_snowmodelq2)");
    const char* missing = nullptr;
    auto need = [&](const void* p, const char* name) { if (!p && !missing) missing = name; };
    each_model_series(*in, [&](auto* host, auto, auto, const char* name) { need(host, name); });
    need(in->clim.winddir, "climdata$winddir");
    each_model_raster(*in, [&](auto* host, auto, int, bool terrain, const char* name) {
        if (!terrain && strcmp(name, "other$isnowdg")) need(host, name);          // (isnowdg is formed here, int:2716)
    });
    need(fi->drv.dtm, "dtm"); need(fi->subs, "subs");
    need(fi->sublmelt, "sublmelt"); need(fi->tempmelt, "tempmelt"); need(fi->rainmelt, "rainmelt"); need(fi->sstemp, "sstemp");
    need(fi->sdenc, "sdenc"); need(fi->sdeng, "sdeng"); need(fi->temp_all, "temp_all"); need(fi->snow_all, "snow_all");
    if (missing) return mcf::api_fail(MCF_ERR_ARG, std::string("mcf_snowmodelq1: null input: ") + missing);
    if (!(fi->drv.res > 0)) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowmodelq1: res must be > 0");
    return subs_af_checks("mcf_snowmodelq1", fi->subs, in->tsteps, fi->n_all,
                          "the fast snow method cannot start on the first day of the series (the reference fails there: `sbtn` not found)",
                          in->clim.windspeed, "wind", fi->drv.res);
}

int snowmodelq1(const mcf_snowfast_in* fi, const mcf_snowdriver_out* out, int32_t device) {
    int rc;
    if ((rc = snowmodelq1_checks(fi, out))) return rc;      // nothing above needs a device
    const mcf_snow_inputs* in = &fi->drv.base;
    if ((rc = pick_device(device))) return rc;
    const int64_t N = in->rows * in->cols, n_all = fi->n_all;
    const int T = (int)in->tsteps;
    DayLoop L(fi->drv, in->clim.windspeed, *out, nullptr);
    if ((rc = check_room((64 + L.nslots + (int64_t)L.nsets * L.nser * 24) * N * 8 + (2 * n_all + L.cm_cells) * 8))) return rc;
    mcf::DevOwner b;
    ModelArgs a;
    memset(&a, 0, sizeof a);
    a.N = N; a.tsteps = 24; a.zref = in->other.zref;
    snow_density_params(in->snowenv, a.sdp);
    // once per call: vegetation, ages, the dtm, the depths' working copies, the whole series' surface and air temperatures
    each_model_raster(*in, [&](auto* host, auto member, int, bool terrain, const char* name) {
        if (!rc && !terrain && strcmp(name, "other$isnowdc") && strcmp(name, "other$isnowdg")) rc = b.up(&(a.*member), host, N, name);
    });
    if (rc) return rc;
    if ((rc = L.prepare(b, a))) return rc;
    const double *d_st, *d_ta;
    double* d_intfrac;
    if ((rc = b.up(&d_st, fi->sstemp, n_all, "sstemp"))) return rc;
    if ((rc = b.up(&d_ta, fi->temp_all, n_all, "temp_all"))) return rc;
    if ((rc = b.make(&d_intfrac, N))) return rc;
    const unsigned gridN = (unsigned)((N + 255) / 256);
    // the step table of all selected hours; every day's gridmodelsnow1 call restarts the albedo clock (snowalbCpp on its slice)
    StepTables tabs;
    if ((rc = build_step_tables(b, in, false, true, true, &tabs))) return rc;
    {
        const double* d_prec;
        if ((rc = b.up(&d_prec, in->clim.precip, T, "climdata$precip"))) return rc;
        hipLaunchKernelGGL(k_snow_alb_chunks, dim3((unsigned)((L.D + 63) / 64)), dim3(64), 0, nullptr, const_cast<StepRow*>(tabs.rows), d_prec, T, 24,
                           L.D);
    }
    // intfrac of a typical snowfall and the ground layer's share of the initial depth (int:2708-2716)
    {
        double ssum = 0.0, tsum = 0.0;
        int64_t scount = 0;
        for (int64_t k = 0; k < n_all; ++k)
            if (fi->snow_all[k] > 0) { ssum += fi->snow_all[k]; ++scount; }
        for (int k = 0; k < T; ++k) tsum += in->clim.temp[k];
        CanIntArgs ca;
        ca.N = N; ca.hgt = a.hgt; ca.pai = a.pai; ca.uf = 2.0; ca.prec = scount ? ssum / (double)scount : NAN;
        ca.sint = canopy_sint(tsum / T); ca.Li = 0.0; ca.frac = d_intfrac; ca.dc = L.d_dc; ca.dg = L.d_dg;
        hipLaunchKernelGGL(k_canintfrac, dim3(gridN), dim3(256), 0, nullptr, ca);
    }
    auto gap_balance = [&](int d, const DaySet&, hipStream_t cs) {
        // the gap's scalars, in plain left-to-right order over R's `sbtn`
        const Gap g = gap_of_day(fi->subs, d);
        double sub = 0.0, rain = 0.0, tm = 0.0, fall = 0.0, sc = 0.0, sg = 0.0, dhp = 0.0;
        for (int64_t k = 0; k < g.len; ++k) {
            const int64_t i = g.start + g.step * k;
            sub += fi->sublmelt[i]; rain += fi->rainmelt[i]; tm += fi->tempmelt[i]; fall += fi->snow_all[i] / 1000;
            sc += fi->sdenc[i]; sg += fi->sdeng[i];
            if (fi->sstemp[i] > 0.0) dhp += fi->sstemp[i];
        }
        GapArgs ga;
        memset(&ga, 0, sizeof ga);
        ga.N = N; ga.start = g.start; ga.len = g.len; ga.step = g.step;
        ga.dhp = dhp; ga.subrain = sub + rain; ga.tempmelt = tm; ga.fall = fall;
        ga.kc = 1000 / (sc / (double)g.len); ga.kg = 1000 / (sg / (double)g.len);
        ga.skyview = L.d_svf; ga.pai = a.pai; ga.intfrac = d_intfrac; ga.dc = L.d_dc; ga.dg = L.d_dg; ga.mu = nullptr;
        hipLaunchKernelGGL(k_gap_balance, dim3(gridN), dim3(256), 0, cs, ga, d_st, d_ta);
    };
    // gridmodelsnow1 on the day's 24 rows, from the depths just formed and the caller's ages (they are not handed on)
    auto model = [&](int d, const DaySet& s, hipStream_t cs) {
        a.rows = tabs.rows + 24 * d;
        a.Tc = s.Tc; a.Tg = s.Tg; a.sdepc = s.sdepc; a.sdepg = s.sdepg; a.sden = s.sden;
        hipLaunchKernelGGL(k_snowmodel<false>, dim3(gridN), dim3(256), 0, cs, a, a.rows, a.dates);
    };
    return L.run(b, "snowmodelq1", "", {{"gap balance", gap_balance}, {"gridmodelsnow", model}}, {});
}
}  // namespace

extern "C" int mcf_snowmodelq1(const mcf_snowfast_in* in, mcf_snowdriver_out* out, int32_t device) { return snowmodelq1(in, out, device); }

extern "C" int mcf_canintfrac_device(int64_t cells, const double* hgt, const double* pai, double uf, double prec, double tc, double Li,
                                     double* frac, int32_t device) {
    if (cells <= 0 || !hgt || !pai || !frac) return mcf::api_fail(MCF_ERR_ARG, "mcf_canintfrac_device: null argument or no cells");
    int rc;
    if ((rc = pick_device(device))) return rc;
    if ((rc = check_room(cells * 24))) return rc;
    mcf::DevOwner b;
    CanIntArgs a;
    memset(&a, 0, sizeof a);
    a.N = cells; a.uf = uf; a.prec = prec; a.sint = canopy_sint(tc); a.Li = Li;
    if ((rc = b.up(&a.hgt, hgt, cells, "hgt"))) return rc;
    if ((rc = b.up(&a.pai, pai, cells, "pai"))) return rc;
    if ((rc = b.make(&a.frac, cells))) return rc;
    hipLaunchKernelGGL(k_canintfrac, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, nullptr, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(frac, a.frac, (size_t)cells * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}
extern "C" int mcf_meltmu_device(int64_t cells, const double* skyview, int64_t n, const double* stemp, const double* tc, double* mu,
                                 int32_t device) {
    if (cells <= 0 || n < 0 || !skyview || !mu || (n > 0 && (!stemp || !tc)))
        return mcf::api_fail(MCF_ERR_ARG, "mcf_meltmu_device: null argument or no cells");
    int rc;
    if ((rc = pick_device(device))) return rc;
    if ((rc = check_room((2 * cells + 2 * n) * 8))) return rc;
    mcf::DevOwner b;
    GapArgs a;
    memset(&a, 0, sizeof a);
    a.N = cells; a.start = 0; a.len = n; a.step = 1;
    for (int64_t k = 0; k < n; ++k)
        if (stemp[k] > 0.0) a.dhp += stemp[k];
    const double zero = 0.0;
    const double *d_st, *d_ta;
    if ((rc = b.up(&a.skyview, skyview, cells, "skyview"))) return rc;
    if ((rc = b.up(&d_st, n ? stemp : &zero, std::max<int64_t>(n, 1), "stemp"))) return rc;
    if ((rc = b.up(&d_ta, n ? tc : &zero, std::max<int64_t>(n, 1), "tc"))) return rc;
    if ((rc = b.make(&a.mu, cells))) return rc;
    hipLaunchKernelGGL(k_gap_balance, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, nullptr, a, d_st, d_ta);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(mu, a.mu, (size_t)cells * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}

// ---- `.snowmodelq2`, the fast snow method with array weather (R/internal.R "int:" 3017-3283), as one device-resident call -----
namespace {
// The pack between two selected days with array weather (int:3229-3244): meltmu2 (cpp:5495-5527) of the resampled snow-surface
// and air temperatures over the gap's hours fused with the resampled balance, one lane per cell.  `st` / `tc`: coarse sstemp /
// tc of the WHOLE series, [hour][coarse cell]; gap hour k is hour start + step k (step = -1: R's `a:b` counting down).  Per
// hour a lane taps both fields: eight loads, whose addresses the lanes of a workgroup (a stretch of one raster column, or of
// few) share among a handful of coarse cells — they go straight through the cache, nothing is staged.  A hole of the dtm reads
// NA taps (`.cca`'s mask): no term, 0.5.  sums: the six gap sums per coarse cell, [6][coarse cells] in the order sublmelt,
// rainmelt, tempmelt, snow, sdenc, sdeng, tapped here (`.resamplemelt`); the balance in the operand order of
// oracle/snowfast_oracle.py:239-251.  adjust = 0 (a first day with subs[0] - 1 <= 1): only the clamps.  dc == null: mu alone.
struct Gap2Args {
    int64_t N, start, len;
    int32_t step, adjust;
    CoarseGeo geo;
    const double *skyview, *dtm, *pai, *intfrac, *sums;
    double *dc, *dg, *mu;
};
__global__ __launch_bounds__(256) void k_gap_balance2(Gap2Args a, const double* __restrict__ st, const double* __restrict__ tc) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.N) return;
    const SnowTap tap = a.geo.tap(c);
    const int64_t CC = (int64_t)a.geo.crows * a.geo.ccols;
    double mu = 0.5;
    if (a.adjust) {
        const double sv = a.skyview[c];
        if (isnan(sv)) {
            mu = na_real();
        } else if (!isnan(a.dtm[c])) {
            double dhp = 0.0, dhm = 0.0;
            const double* ps = st + a.start * CC;
            const double* pt = tc + a.start * CC;
            const int64_t inc = (int64_t)a.step * CC;
#pragma unroll 4
            for (int64_t k = 0; k < a.len; ++k) {
                const double s = tap(ps), t = tap(pt);
                if (s > 0.0) dhp += s;
                const double s2 = (s - t) * sv + t;
                if (s2 > 0.0) dhm += s2;
                ps += inc; pt += inc;
            }
            if (dhp > 0.0) mu = dhm / dhp;
        }
    }
    if (a.mu) a.mu[c] = mu;
    if (!a.dc) return;
    double dc = a.dc[c], dg = a.dg[c];
    if (a.adjust) {
        const double sub = tap(a.sums), rain = tap(a.sums + CC), tm = tap(a.sums + 2 * CC), snowsum = tap(a.sums + 3 * CC);
        const double len = (double)a.len;
        const double melt = sub + rain + mu * tm;
        const double balancec = snowsum / 1000 - melt;
        const double balanceg = (1 - a.intfrac[c]) * snowsum / 1000 - exp(-a.pai[c]) * melt;
        const double sdec = tap(a.sums + 4 * CC) / len, sdeg = tap(a.sums + 5 * CC) / len;
        dc = dc + balancec * (1000 / sdec);
        dg = dg + balanceg * (1000 / sdeg);
    }
    if (dc < 0) dc = 0;                                        // `x[x < 0] <- 0`: NA stays NA
    if (dg < 0) dg = 0;
    a.dc[c] = dc; a.dg[c] = dg;
}

int snowmodelq2_checks(const mcf_snowfast2_in* fi, const mcf_snowfast2_out* out) {
    if (!fi || !out) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowmodelq2: null argument");
    const mcf_snow_inputs* in = &fi->drv.base;
    if (in->tsteps <= 0 || in->tsteps % 24)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_snowmodelq2: the fast snow method works on whole selected days (tsteps = 24 x days, at least one)");
    if (const int rc = common_checks(in)) return rc;
    const int rc = coarse_grid_checks(coarse_grid(*fi, in->rows, in->cols), "mcf_snowmodelq2", "", [&]() -> int {
        const char* missing = nullptr;
        auto need = [&](const void* p, const char* name) { if (!p && !missing) missing = name; };
        need(fi->coarse_rowpos, "coarse_rowpos"); need(fi->coarse_colpos, "coarse_colpos");
        each_coarse_selected(*fi, [&](auto* host, auto, const char* name) { need(host, name); });
        need(in->clim.winddir, "climdata$winddir");
        each_model_raster(*in, [&](auto* host, auto, int, bool terrain, const char* name) {
            if (!terrain && strcmp(name, "other$isnowdg")) need(host, name);          // (isnowdg is formed here)
        });
        need(in->other.lats, "other$lats"); need(in->other.lons, "other$lons");
        need(fi->drv.dtm, "dtm"); need(fi->drv.af_wind, "af_wind"); need(fi->subs, "subs");
        need(fi->sublmelt, "sublmelt"); need(fi->tempmelt, "tempmelt"); need(fi->rainmelt, "rainmelt"); need(fi->snow, "snow");
        need(fi->sstemp, "sstemp"); need(fi->tc, "tc"); need(fi->sdenc, "sdenc"); need(fi->sdeng, "sdeng");
        if (missing) return mcf::api_fail(MCF_ERR_ARG, std::string("mcf_snowmodelq2: null input: ") + missing);
        if (!(fi->drv.res > 0)) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowmodelq2: res must be > 0");
        return MCF_OK;
    });
    if (rc) return rc;
    return subs_af_checks("mcf_snowmodelq2", fi->subs, in->tsteps, fi->n_all, nullptr, fi->drv.af_wind, "af_wind", fi->drv.res);
}

int snowmodelq2(const mcf_snowfast2_in* fi, const mcf_snowfast2_out* out, int32_t device) {
    int rc;
    if ((rc = snowmodelq2_checks(fi, out))) return rc;      // nothing above needs a device
    const mcf_snow_inputs* in = &fi->drv.base;
    if ((rc = pick_device(device))) return rc;
    const int64_t N = in->rows * in->cols, n_all = fi->n_all, CC = fi->coarse_rows * fi->coarse_cols;
    const int T = (int)in->tsteps;
    const int64_t DN = 24 * N;
    // (umu is one of the day's thirteen inputs: it leaves from the set when it is wanted)
    DayLoop L(fi->drv, fi->drv.af_wind, out->smod, out->umu);
    const int D = L.D;
    if ((rc = check_room((66 + L.nslots + 13 * 24 + (int64_t)L.nsets * L.nser * 24) * N * 8 +
                         ((14 * (int64_t)T + 2 * n_all + 6 * D + 2) * CC + L.cm_cells) * 8)))
        return rc;
    mcf::DevOwner b;
    ModelArgs a;
    memset(&a, 0, sizeof a);
    a.N = N; a.tsteps = 24; a.zref = in->other.zref;
    snow_density_params(in->snowenv, a.sdp);
    each_model_raster(*in, [&](auto* host, auto member, int, bool terrain, const char* name) {
        if (!rc && !terrain && strcmp(name, "other$isnowdc") && strcmp(name, "other$isnowdg")) rc = b.up(&(a.*member), host, N, name);
    });
    if (rc) return rc;
    if ((rc = up_sites(b, a, in, N))) return rc;
    if ((rc = L.prepare(b, a))) return rc;
    // resident for the call: the coarse arrays of the selected hours, coarse sstemp / tc of the whole series
    FineArgs fa;
    if ((rc = coarse_upload(b, coarse_grid(*fi, in->rows, in->cols), fi, kSnowCoarseArrays, fi->drv.dtm, 0, T, L.d_dtm, &fa))) return rc;
    const double *d_st, *d_ta;
    double *d_intfrac, *d_sums, *d_tsum;
    if ((rc = b.up(&d_st, fi->sstemp, n_all * CC, "sstemp"))) return rc;
    if ((rc = b.up(&d_ta, fi->tc, n_all * CC, "tc"))) return rc;
    if ((rc = b.make(&d_intfrac, N))) return rc;
    if ((rc = b.make(&d_sums, 6 * CC * D))) return rc;
    if ((rc = b.make(&d_tsum, CC))) return rc;
    // the day's thirteen series on the raster (umu: in the output sets when it leaves)
    double** const fine[] = {&fa.o_temp, &fa.o_relhum, &fa.o_pres, &fa.o_swdown, &fa.o_difrad, &fa.o_lwdown, &fa.o_windspeed, &fa.o_precip,
                             &fa.o_Gp, &fa.o_Tc, &fa.o_RswabsG, &fa.o_RlwabsG};
    for (double** q : fine)
        if ((rc = b.make(q, DN))) return rc;
    if (!out->umu && (rc = b.make(&fa.o_umu, DN))) return rc;
    a.temp = fa.o_temp; a.relhum = fa.o_relhum; a.pres = fa.o_pres; a.swdown = fa.o_swdown; a.difrad = fa.o_difrad; a.lwdown = fa.o_lwdown;
    a.windspeed = fa.o_windspeed; a.precip = fa.o_precip; a.Gp = fa.o_Gp; a.Tcp = fa.o_Tc; a.RswabsG = fa.o_RswabsG; a.RlwabsG = fa.o_RlwabsG;
    const unsigned gridN = (unsigned)((N + 255) / 256);
    // the date table of all selected hours (array weather: a day's gridmodelsnow2 launch starts its own albedo clock)
    StepTables tabs;
    if ((rc = build_step_tables(b, in, true, true, false, &tabs))) return rc;
    // intfrac of a typical snowfall and the ground layer's share of the initial depth (int:3192-3200)
    {
        double ssum = 0.0;
        int64_t scount = 0;
        for (int64_t k = 0; k < n_all * CC; ++k)
            if (fi->snow[k] > 0) { ssum += fi->snow[k]; ++scount; }
        std::vector<double> tsum((size_t)CC, 0.0);               // per coarse cell: tc added over the series, left to right
        for (int64_t k = 0; k < n_all; ++k)
            for (int64_t q = 0; q < CC; ++q) tsum[(size_t)q] += fi->tc[k * CC + q];
        HIP_TRY(hipMemcpy(d_tsum, tsum.data(), (size_t)CC * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_tap_plane, dim3(gridN), dim3(256), 0, nullptr, fa.geo, N, L.d_dtm, (const double*)d_tsum, fa.o_temp);
        launch_sumcount(fa.o_temp, N, L.d_ws, L.d_m2);
        double h[2];
        HIP_TRY(hipMemcpy(h, L.d_m2, 16, hipMemcpyDeviceToHost));
        CanIntArgs ca;
        ca.N = N; ca.hgt = a.hgt; ca.pai = a.pai; ca.uf = 2.0; ca.prec = scount ? ssum / (double)scount : NAN;
        ca.sint = canopy_sint(h[0] / (h[1] * (double)n_all)); ca.Li = 0.0; ca.frac = d_intfrac; ca.dc = L.d_dc; ca.dg = L.d_dg;
        hipLaunchKernelGGL(k_canintfrac, dim3(gridN), dim3(256), 0, nullptr, ca);
    }
    // every gap's six sums per coarse cell, in plain left-to-right order over R's `sbtn` (`.resamplemelt` taps them)
    {
        std::vector<double> sums((size_t)(6 * CC * D), 0.0);
        const double* const gapv[6] = {fi->sublmelt, fi->rainmelt, fi->tempmelt, fi->snow, fi->sdenc, fi->sdeng};
        for (int d = 0; d < D; ++d) {
            if (!(fi->subs[24 * d] - 1 > 1)) continue;
            const Gap g = gap_of_day(fi->subs, d);
            for (int v = 0; v < 6; ++v)
                for (int64_t k = 0; k < g.len; ++k) {
                    const double* src = gapv[v] + (g.start + g.step * k) * CC;
                    double* dst = &sums[(size_t)((6 * d + v) * CC)];
                    for (int64_t q = 0; q < CC; ++q) dst[q] += src[q];
                }
        }
        HIP_TRY(hipMemcpy(d_sums, sums.data(), sums.size() * 8, hipMemcpyHostToDevice));
    }
    auto gap_balance = [&](int d, const DaySet&, hipStream_t cs) {
        const Gap g = gap_of_day(fi->subs, d);
        Gap2Args ga;
        memset(&ga, 0, sizeof ga);
        ga.N = N; ga.geo = fa.geo; ga.adjust = fi->subs[24 * d] - 1 > 1;
        ga.skyview = L.d_svf; ga.dtm = L.d_dtm; ga.pai = a.pai; ga.intfrac = d_intfrac; ga.sums = d_sums + 6 * CC * d;
        ga.dc = L.d_dc; ga.dg = L.d_dg;
        if (ga.adjust) { ga.start = g.start; ga.len = g.len; ga.step = g.step; }
        hipLaunchKernelGGL(k_gap_balance2, dim3(gridN), dim3(256), 0, cs, ga, d_st, d_ta);
    };
    // the day's weather and point model on the raster
    auto fine_day = [&](int d, const DaySet& s, hipStream_t cs) {
        fa.hour0 = 24 * (int64_t)d;
        if (out->umu) fa.o_umu = s.umu;
        launch_coarse_hours(fa, 24, cs);
    };
    // gridmodelsnow2 on the day's 24 hours, from the depths just formed and the caller's ages (they are not handed on)
    auto model = [&](int d, const DaySet& s, hipStream_t cs) {
        a.dates = tabs.dates + 24 * d;
        a.umu = fa.o_umu;
        a.Tc = s.Tc; a.Tg = s.Tg; a.sdepc = s.sdepc; a.sdepg = s.sdepg; a.sden = s.sden;
        hipLaunchKernelGGL(k_snowmodel<true>, dim3(gridN), dim3(256), 0, cs, a, a.rows, a.dates);
    };
    auto cleansmod = [&](int, const DaySet& s, hipStream_t cs) {
        CleanArgs cl;
        cl.N = N; cl.dtm = L.d_dtm;
        cl.v[0] = s.Tc; cl.v[1] = s.Tg; cl.v[2] = out->smod.groundsnowdepth ? s.sdepg : nullptr;
        cl.v[3] = out->smod.totalSWE ? s.sdepc : nullptr; cl.v[4] = out->smod.snowden ? s.sden : nullptr;
        hipLaunchKernelGGL(k_clean_chunk, dim3(gridN), dim3(256), 0, cs, cl, 24);
    };
    return L.run(b, "snowmodelq2", ", " + std::to_string(CC) + " coarse cells",
                 {{"gap balance", gap_balance}, {"fine day", fine_day}, {"gridmodelsnow", model}}, {{".cleansmod", cleansmod}});
}
}  // namespace

extern "C" int mcf_snowmodelq2(const mcf_snowfast2_in* in, mcf_snowfast2_out* out, int32_t device) { return snowmodelq2(in, out, device); }

extern "C" int mcf_meltmu2_device(int64_t rows, int64_t cols, const double* skyview, const double* dtm, int64_t crows, int64_t ccols,
                                  const double* rowpos, const double* colpos, int64_t n, const double* sstemp_c, const double* tc_c,
                                  double* mu_out, int32_t device) {
    if (rows <= 0 || cols <= 0 || crows < 1 || ccols < 1 || n < 0 || !skyview || !dtm || !rowpos || !colpos || !mu_out ||
        (n > 0 && (!sstemp_c || !tc_c)))
        return mcf::api_fail(MCF_ERR_ARG, "mcf_meltmu2_device: null argument, empty raster or empty coarse grid");
    // (this entry's own wording, older than coarse_grid_checks': the two bounds are the shared ones, the sentences stay)
    const CoarseGrid g{rows, cols, crows, ccols, rowpos, colpos, nullptr, 0};
    if (rows * cols >= ((int64_t)1 << 29) || coarse_grid_too_large(g))
        return mcf::api_fail(MCF_ERR_ARG, "mcf_meltmu2_device: raster or coarse grid too large");
    if (!positions_inside(g))
        return mcf::api_fail(MCF_ERR_ARG, "mcf_meltmu2_device: rowpos / colpos must lie in 0..crows - 1 / 0..ccols - 1");
    int rc;
    if ((rc = pick_device(device))) return rc;
    const int64_t N = rows * cols, CC = crows * ccols;
    if ((rc = check_room((3 * N + rows + cols + 2 * n * CC) * 8))) return rc;
    mcf::DevOwner b;
    Gap2Args a;
    memset(&a, 0, sizeof a);
    a.N = N; a.start = 0; a.len = n; a.step = 1; a.adjust = 1;
    a.geo.rows = (int32_t)rows; a.geo.crows = (int32_t)crows; a.geo.ccols = (int32_t)ccols;
    const double zero = 0.0;
    const double *d_st, *d_ta;
    if ((rc = b.up(&a.geo.rowpos, rowpos, rows, "rowpos"))) return rc;
    if ((rc = b.up(&a.geo.colpos, colpos, cols, "colpos"))) return rc;
    if ((rc = b.up(&a.skyview, skyview, N, "skyview"))) return rc;
    if ((rc = b.up(&a.dtm, dtm, N, "dtm"))) return rc;
    if ((rc = b.up(&d_st, n ? sstemp_c : &zero, std::max<int64_t>(n * CC, 1), "sstemp"))) return rc;
    if ((rc = b.up(&d_ta, n ? tc_c : &zero, std::max<int64_t>(n * CC, 1), "tc"))) return rc;
    if ((rc = b.make(&a.mu, N))) return rc;
    hipLaunchKernelGGL(k_gap_balance2, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, a, d_st, d_ta);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(mu_out, a.mu, (size_t)N * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}

// ---- the coarse arrays left coarse behind the slow snow method (`.snowmodel2`, mcf_snowmodel2_coarse) and behind gridmicrosnow2's
// nine series (`.prepsnowinputs2`, int:3445-3579; snow.py _fine_micro_inputs): what is refused, and the expansions alone ---------
namespace mcf {   // mcf_snow_plan.hpp
// What the entries that take a mcf_snowcoarse_in refuse before a device is touched; model: the snow model runs behind (the
// expansion alone reads geometry, dtm and coarse arrays); null_out: the name of the entry's output argument if that is null
int snowcoarse_checks(const mcf_snowcoarse_in* ci, bool model, const char* entry, const char* null_out) {
    const std::string e = std::string(entry) + ": ";
    auto fail = [&](const std::string& m) { return mcf::api_fail(MCF_ERR_ARG, e + m); };
    if (!ci) return fail("null argument: in");
    if (null_out) return fail(std::string("null argument: ") + null_out);
    const mcf_snow_inputs* in = &ci->drv.base;
    if (in->array_forcing == 0) return fail("drv.base.array_forcing must not be 0 (array weather; data.frame weather: mcf_snowmodel1)");
    if (in->rows <= 0 || in->cols <= 0 || in->tsteps <= 0 || in->tsteps > (1 << 30) || in->rows * in->cols >= ((int64_t)1 << 29))
        return fail("rows, cols, tsteps out of range (at least 1; at most 2^29 - 1 cells, 2^30 steps)");
    const int rc = coarse_grid_checks(coarse_grid(*ci, in->rows, in->cols), entry, "", [&]() -> int {
        const char* missing = nullptr;
        auto need = [&](const void* p, const char* name) { if (!p && !missing) missing = name; };
        need(ci->coarse_rowpos, "coarse_rowpos"); need(ci->coarse_colpos, "coarse_colpos");
        each_coarse_selected(*ci, [&](auto* host, auto, const char* name) { need(host, name); });
        need(ci->drv.dtm, "dtm");
        if (model) {
            each_obstime(*in, [&](auto* host, auto, const char* name) { need(host, name); });
            need(in->clim.winddir, "climdata$winddir");
            each_model_raster(*in, [&](auto* host, auto, int, bool terrain, const char* name) { if (!terrain) need(host, name); });
            need(in->other.lats, "other$lats"); need(in->other.lons, "other$lons");
            need(ci->drv.af_wind, "af_wind");
        }
        if (missing) return fail(std::string("null input: ") + missing);
        if (model && !(ci->drv.res > 0)) return fail("res must be > 0");
        return MCF_OK;
    });
    if (rc) return rc;
    if (model && (ci->drv.chunk_steps < 0 || ci->drv.chunk_steps % 24)) return fail("chunk_steps must be whole days (0: 120)");
    return MCF_OK;
}
// what the entries that take a mcf_microcoarse_in refuse before a device is touched
int microcoarse_checks(const mcf_microcoarse_in* mi, const char* entry) {
    const std::string e = std::string(entry) + ": ";
    auto fail = [&](const std::string& m) { return mcf::api_fail(MCF_ERR_ARG, e + m); };
    if (!mi) return fail("null argument: micro");
    if (mi->rows <= 0 || mi->cols <= 0 || mi->tsteps <= 0 || mi->tsteps > (1 << 30) || mi->rows * mi->cols >= ((int64_t)1 << 29))
        return fail("micro: rows, cols, tsteps out of range (at least 1; at most 2^29 - 1 cells, 2^30 steps)");
    return coarse_grid_checks(coarse_grid(*mi, mi->rows, mi->cols), entry, "micro: ", [&]() -> int {
        const char* missing = nullptr;
        auto need = [&](const void* p, const char* name) { if (!p && !missing) missing = name; };
        need(mi->coarse_rowpos, "coarse_rowpos"); need(mi->coarse_colpos, "coarse_colpos");
        each_micro_coarse(*mi, [&](auto* host, auto, const char* name) { need(host, name); });
        need(mi->dtm, "dtm");
        return missing ? fail(std::string("null input: micro ") + missing) : (int)MCF_OK;
    });
}
}  // namespace mcf

namespace {
using mcf::snowcoarse_checks;
using mcf::microcoarse_checks;
// The two entries that expand alone (tests and tools hold the kernels to the host's expansion through them): hours step0 ..
// step0 + nsteps - 1 of the series in `mask` — of nseries, made from nseries + 1 coarse arrays — into the host arrays fine[].
// outputs(fa, d): the device arrays d[] (null: not wanted) into the kernel's arguments.
template <class Args, class In, class Each, class Outs>
int expand_coarse_alone(const char* entry, const CoarseGrid& g, const In* in, Each&& each, const double* dtm, int64_t tsteps,
                        int64_t step0, int64_t nsteps, int nseries, uint32_t mask, double* const fine[], Outs&& outputs, int32_t device) {
    if (step0 < 0 || nsteps < 1 || step0 > tsteps - nsteps)
        return mcf::api_fail(MCF_ERR_ARG, std::string(entry) + ": step0 >= 0, nsteps >= 1 and step0 + nsteps <= tsteps are needed");
    int rc;
    if ((rc = pick_device(device))) return rc;
    const int64_t N = g.cells(), CC = g.coarse_cells();
    if ((rc = check_room((nseries * nsteps + 1) * N * 8 + (nseries + 1) * CC * nsteps * 8))) return rc;
    mcf::DevOwner b;
    Args fa;
    if ((rc = coarse_upload(b, g, in, each, dtm, step0, nsteps, nullptr, &fa))) return rc;
    double* d[13] = {};
    for (int f = 0; f < nseries; ++f)
        if ((mask >> f & 1u) && (rc = b.make(&d[f], N * nsteps))) return rc;
    outputs(fa, d);
    launch_coarse_hours(fa, (int)nsteps, nullptr);
    HIP_TRY(hipGetLastError());
    mcf::ToHost dl;
    for (int f = 0; f < nseries; ++f)
        if (d[f]) HIP_TRY(dl.dense(fine[f], d[f], (size_t)(N * nsteps) * 8));
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}
}  // namespace

extern "C" int mcf_snow_expand_coarse_device(const mcf_snowcoarse_in* in, int64_t step0, int64_t nsteps, double* const fine[13],
                                             int32_t device) {
    const char* entry = "mcf_snow_expand_coarse_device";
    if (const int rc = snowcoarse_checks(in, false, entry, fine ? nullptr : "fine")) return rc;
    for (int f = 0; f < 13; ++f)
        if (!fine[f]) return mcf::api_fail(MCF_ERR_ARG, std::string(entry) + ": null argument: fine[" + std::to_string(f) + "]");
    const mcf_snow_inputs& base = in->drv.base;
    return expand_coarse_alone<FineArgs>(entry, coarse_grid(*in, base.rows, base.cols), in, kSnowCoarseArrays, in->drv.dtm, base.tsteps, step0,
                                         nsteps, 13, (1u << 13) - 1, fine, [](FineArgs& fa, double* const d[]) { fine_outputs(fa, d); }, device);
}
extern "C" int mcf_microsnow_expand_coarse_device(const mcf_microcoarse_in* in, int64_t step0, int64_t nsteps, double* const fine[9],
                                                  int32_t device) {
    const char* entry = "mcf_microsnow_expand_coarse_device";
    if (!in) return mcf::api_fail(MCF_ERR_ARG, std::string(entry) + ": null argument: in");
    if (!fine) return mcf::api_fail(MCF_ERR_ARG, std::string(entry) + ": null argument: fine");
    if (const int rc = microcoarse_checks(in, entry)) return rc;
    uint32_t mask = 0;                   // a null fine[f]: series f is not wanted
    for (int f = 0; f < kMicroSeries; ++f) mask |= fine[f] ? 1u << f : 0u;
    if (!mask) return mcf::api_fail(MCF_ERR_ARG, std::string(entry) + ": null argument: fine[] (every series is null)");
    auto outputs = [&](MicroFineArgs& fa, double* const d[]) {
        fa.mask = mask;
        for (int f = 0; f < kMicroSeries; ++f) fa.o[f] = d[f];
    };
    return expand_coarse_alone<MicroFineArgs>(entry, coarse_grid(*in, in->rows, in->cols), in, kMicroCoarseArrays, in->dtm, in->tsteps, step0,
                                              nsteps, kMicroSeries, mask, fine, outputs, device);
}

namespace mcf {   // mcf_snow_plan.hpp
// the micro group's coarse set onto the plan (once, before mcf_snowplan_micro_setup, whose `sub` then carries no weather arrays)
int snowplan_micro_attach_coarse(mcf_snowplan* sp, const mcf_microcoarse_in* mi) {
    if (!sp || !mi) return api_fail(MCF_ERR_ARG, "null argument");
    if (sp->mcoarse) return api_fail(MCF_ERR_STATE, "snow plan: the microclimate's coarse arrays are attached already");
    if (!sp->af || mi->rows != sp->rows || mi->cols != sp->cols || mi->tsteps != sp->T)
        return api_fail(MCF_ERR_ARG, "snow plan: the microclimate's coarse arrays are not of the plan's raster and series (array weather)");
    HIP_TRY(hipSetDevice(sp->device));
    if (const int rc = check_room((int64_t)kMicroSeries * sp->chunk * sp->N * 8 + 10 * mi->coarse_rows * mi->coarse_cols * mi->tsteps * 8))
        return rc;
    sp->mcoarse.emplace();
    return coarse_upload(sp->b, coarse_grid(*mi, mi->rows, mi->cols), mi, kMicroCoarseArrays, mi->dtm, 0, sp->T, sp->d_dtm, &*sp->mcoarse);
}
// where a coarse plan's run_chunk hands pointm$umu to (null: nowhere — pass 2's re-runs of a chunk)
void snowplan_coarse_umu_out(mcf_snowplan* sp, double* umu_out) {
    if (sp && sp->coarse) sp->h_umu = umu_out;
}
}  // namespace mcf

// ---- the snow-day microclimate inside the chunk loop --------------------------------------------------------------------
extern "C" int mcf_snowplan_reset(mcf_snowplan* sp) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null snow plan");
    HIP_TRY(hipSetDevice(sp->device));
    const int64_t N = sp->N;
    HIP_TRY(hipMemcpy(sp->d_isnowdc, sp->d_isnowdc0, (size_t)N * 8, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(sp->d_ac, sp->d_ac0, (size_t)N * 4, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(sp->d_ag, sp->d_ag0, (size_t)N * 4, hipMemcpyDeviceToDevice));
    hipLaunchKernelGGL(k_add_snow, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, sp->d_dtm, sp->d_isnowdg, 1.0, N,
                       sp->d_dtms);
    HIP_TRY(hipGetLastError());
    sp->prepared = -1;
    return MCF_OK;
}
// Sparse read-back of the plan's device state: `n` cells x the array's depth (planes N apart), for in-run checks of a sample
// of cells against the oracle (tools/bench_snow.py) — the analogue of mcf_plan_fetch_cells for the snow plan.
__global__ __launch_bounds__(256) void k_gather_planes(const double* __restrict__ src, const int32_t* __restrict__ isrc, int64_t N,
                                                       const int64_t* __restrict__ cells, int n, int depth,
                                                       double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * depth) return;
    const int j = t % n, k = t / n;
    const int64_t q = cells[j] + N * (int64_t)k;
    out[t] = src ? src[q] : (double)isrc[q];
}
extern "C" int mcf_snowplan_fetch_cells(mcf_snowplan* sp, int32_t what, const int64_t* cells, int32_t n, double* out,
                                        int32_t* depth_out) {
    if (!sp || !cells || !out || n <= 0) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    const int ns = sp->chunk;
    const double* src = nullptr;
    const int32_t* isrc = nullptr;
    int depth = 1;
    switch (what) {
        case MCF_SNOWPLAN_ISNOWDC: src = sp->d_isnowdc; break;
        case MCF_SNOWPLAN_ISNOWAC: isrc = sp->d_ac; break;
        case MCF_SNOWPLAN_ISNOWAG: isrc = sp->d_ag; break;
        case MCF_SNOWPLAN_SLOPE: src = sp->d_slope; break;
        case MCF_SNOWPLAN_ASPECT: src = sp->d_aspect; break;
        case MCF_SNOWPLAN_SKYVIEW: src = sp->d_svf; break;
        case MCF_SNOWPLAN_WSA: src = sp->d_wsa; depth = 8; break;
        case MCF_SNOWPLAN_HOR: src = sp->d_hor; depth = 24; break;
        case MCF_SNOWPLAN_TC: src = sp->a.Tc; depth = ns; break;
        case MCF_SNOWPLAN_TG: src = sp->a.Tg; depth = ns; break;
        case MCF_SNOWPLAN_SDEPG: src = sp->a.sdepg; depth = ns; break;
        case MCF_SNOWPLAN_SDEN: src = sp->a.sden; depth = ns; break;
        case MCF_SNOWPLAN_TOTALSWE: src = sp->a.sdepc; depth = ns; break;
        default: return mcf::api_fail(MCF_ERR_ARG, "snow plan: unknown array");
    }
    for (int j = 0; j < n; ++j)
        if (cells[j] < 0 || cells[j] >= sp->N) return mcf::api_fail(MCF_ERR_ARG, "snow plan: cell index outside the block");
    HIP_TRY(hipSetDevice(sp->device));
    mcf::DevOwner tmp;
    int rc;
    int64_t* d_cells;
    double* d_out;
    if ((rc = tmp.make(&d_cells, n))) return rc;
    if ((rc = tmp.make(&d_out, (int64_t)n * depth))) return rc;
    HIP_TRY(hipMemcpy(d_cells, cells, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gather_planes, dim3((unsigned)((n * depth + 255) / 256)), dim3(256), 0, nullptr, src, isrc, sp->N,
                       (const int64_t*)d_cells, n, depth, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out, (size_t)n * depth * 8, hipMemcpyDeviceToHost));
    if (depth_out) *depth_out = depth;
    return MCF_OK;
}

// HBM is 288 GB and a chunk's five series of one rank's block are 10 GB: what pass 1 wrote for a chunk with a snow day can
// simply stay.  keep_chunk (after run_chunk and whatever reads the series) hands the chunk's buffers over to the cache and
// gives the plan fresh ones, as long as `reserve_bytes` of device memory stay free; mcf_snowplan_microsnow then reads a kept
// chunk where it lies, and the caller neither restores nor re-runs it.  release_kept hands the sets to a pool for the next
// year (allocation is the expensive part: the cache pays from the second year of a plan on).
extern "C" int mcf_snowplan_keep_chunk(mcf_snowplan* sp, int32_t ch, int64_t reserve_bytes, int32_t* kept) {
    if (!sp || !kept) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    *kept = 0;
    HIP_TRY(hipSetDevice(sp->device));
    if (sp->kept.size() < (size_t)sp->nchunks) sp->kept.resize((size_t)sp->nchunks);
    if (sp->kept[ch].Tc) { *kept = 1; return MCF_OK; }
    if (sp->series_valid != 31) return MCF_OK;      // (a chunk run with some series switched off cannot be kept)
    const int64_t one = (int64_t)sp->chunk * sp->N * 8;
    const int64_t small = sp->a.tzd ? (int64_t)std::max(sp->chunk / 24, 1) * sp->N * 8 : 0;      // the days' means of Tg beside them
    double* fresh[6] = {};
    if (!sp->pool.empty()) {               // a set an earlier year released
        const mcf_snowplan::Kept f = sp->pool.back();
        sp->pool.pop_back();
        fresh[0] = f.Tc; fresh[1] = f.Tg; fresh[2] = f.sdepc; fresh[3] = f.sdepg; fresh[4] = f.sden; fresh[5] = f.tzd;
    } else {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if ((int64_t)free_b < 5 * one + small + std::max<int64_t>(reserve_bytes, 0)) return MCF_OK;
        if (sp->keep_budget >= 0 && sp->keep_allocated + 5 * one > sp->keep_budget) return MCF_OK;
        for (int v = 0; v < 6; ++v) {
            if (v == 5 && !small) break;
            if (sp->kb.alloc((void**)&fresh[v], v == 5 ? small : one) != MCF_OK) {      // (another process took the room: not an error)
                (void)hipGetLastError();
                for (int u = 0; u < v; ++u) sp->kb.release(fresh[u]);
                return MCF_OK;
            }
        }
        sp->keep_allocated += 5 * one;
    }
    HIP_TRY(hipDeviceSynchronize());         // (the chunk's kernels are done before its buffers change hands)
    ModelArgs& a = sp->a;
    mcf_snowplan::Kept k;
    k.Tc = a.Tc; k.Tg = a.Tg; k.sdepc = a.sdepc; k.sdepg = a.sdepg; k.sden = a.sden; k.tzd = a.tzd;
    a.Tc = fresh[0]; a.Tg = fresh[1]; a.sdepc = fresh[2]; a.sdepg = fresh[3]; a.sden = fresh[4]; a.tzd = fresh[5];
    sp->kept[ch] = k;
    sp->mm_chunk = -1;                     // (the plan's buffers are fresh ones now)
    *kept = 1;
    return MCF_OK;
}
extern "C" int mcf_snowplan_set_series(mcf_snowplan* sp, uint32_t mask) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null snow plan");
    if (mask > 31u) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_set_series: five series, mask <= 31");
    sp->series_mask = mask;
    return MCF_OK;
}
// would mcf_snowplan_keep_chunk keep a chunk now? (a pooled set, or room for a new one beside `reserve_bytes`)
extern "C" int mcf_snowplan_can_keep(mcf_snowplan* sp, int64_t reserve_bytes, int32_t* yes) {
    if (!sp || !yes) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    *yes = 0;
    if (!sp->pool.empty()) { *yes = 1; return MCF_OK; }
    HIP_TRY(hipSetDevice(sp->device));
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t one = (int64_t)sp->chunk * sp->N * 8;
    *yes = (int64_t)free_b >= 5 * one + std::max<int64_t>(reserve_bytes, 0) ? 1 : 0;
    if (sp->keep_budget >= 0 && sp->keep_allocated + 5 * one > sp->keep_budget) *yes = 0;
    return MCF_OK;
}
extern "C" int mcf_snowplan_set_keep_budget(mcf_snowplan* sp, int64_t bytes) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null snow plan");
    sp->keep_budget = bytes;
    return MCF_OK;
}
extern "C" int mcf_snowplan_release_kept(mcf_snowplan* sp) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null snow plan");
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipDeviceSynchronize());
    // the sets go to a pool for the next year's pass 1 (allocating 10 GB takes a quarter of a second: a year's cache costs more
    // to allocate than it saves, so it is allocated once per plan); the plan's allocation lists still own every buffer
    for (auto& k : sp->kept)
        if (k.Tc) sp->pool.push_back(k);
    sp->kept.clear();
    return MCF_OK;
}

// The state a chunk starts from — the pack depth handed over, the snow surface the terrain refresh reads, the two ages:
// 24 bytes per cell.  Pass 1 of the snow-day microclimate checkpoints every chunk; pass 2 then restores and re-runs only the
// chunks that hold a snow day (the others contribute nothing but the no-snow solver's days).
extern "C" int mcf_snowplan_checkpoint(mcf_snowplan* sp, int32_t ch) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null snow plan");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    HIP_TRY(hipSetDevice(sp->device));
    const size_t N = (size_t)sp->N;
    if (sp->ckpt.size() < (size_t)sp->nchunks) sp->ckpt.resize((size_t)sp->nchunks, nullptr);
    if (!sp->ckpt[ch]) {
        int rc;
        if ((rc = sp->b.make(&sp->ckpt[ch], (int64_t)N * 24))) return rc;
    }
    char* c = sp->ckpt[ch];
    HIP_TRY(hipMemcpyAsync(c, sp->d_isnowdc, N * 8, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(c + N * 8, sp->d_dtms, N * 8, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(c + N * 16, sp->d_ac, N * 4, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(c + N * 20, sp->d_ag, N * 4, hipMemcpyDeviceToDevice, nullptr));
    return MCF_OK;
}
extern "C" int mcf_snowplan_restore(mcf_snowplan* sp, int32_t ch) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null snow plan");
    if (ch < 0 || (size_t)ch >= sp->ckpt.size() || !sp->ckpt[ch])
        return mcf::api_fail(MCF_ERR_STATE, "snow plan: no checkpoint of this chunk (mcf_snowplan_checkpoint in the first pass)");
    HIP_TRY(hipSetDevice(sp->device));
    const size_t N = (size_t)sp->N;
    const char* c = sp->ckpt[ch];
    HIP_TRY(hipMemcpyAsync(sp->d_isnowdc, c, N * 8, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(sp->d_dtms, c + N * 8, N * 8, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(sp->d_ac, c + N * 16, N * 4, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(sp->d_ag, c + N * 20, N * 4, hipMemcpyDeviceToDevice, nullptr));
    sp->prepared = -1;
    return MCF_OK;
}
extern "C" int mcf_snowplan_meand_accumulate(mcf_snowplan* sp, int32_t ch, const int32_t* snowday) {
    if (!sp || !snowday) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    HIP_TRY(hipSetDevice(sp->device));
    const int ns = std::min(sp->chunk, sp->T - ch * sp->chunk), nd = ns / 24;
    int nsnow = 0;
    for (int d = 0; d < nd; ++d) nsnow += snowday[d] != 0;
    if (ch == 0 || sp->sumD_steps < 0) sp->sumD_steps = 0;
    if (ch == 0) HIP_TRY(hipMemset(sp->d_sumD, 0, (size_t)sp->N * 8));
    if (ch == 0) HIP_TRY(hipMemset(sp->d_sden_na, 0, (size_t)sp->N * 4));
    if (nsnow == 0) return MCF_OK;
    if (!(sp->series_valid & 16u)) return mcf::api_fail(MCF_ERR_STATE, "snow plan: the chunk's snow density series was switched off (mcf_snowplan_set_series)");
    HIP_TRY(hipMemcpy(sp->d_daymap, snowday, (size_t)nd * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_meand_accumulate, dim3((unsigned)((sp->N + 255) / 256)), dim3(256), 0, nullptr, sp->a.sden, sp->a.hgt,
                       sp->N, nd, (const int32_t*)sp->d_daymap, sp->sumD_steps == 0 ? 1 : 0, sp->d_sumD, sp->d_sden_na);
    HIP_TRY(hipGetLastError());
    sp->sumD_steps += (int64_t)nsnow * 24;
    return MCF_OK;
}
extern "C" int mcf_snowplan_micro_setup(mcf_snowplan* sp, const mcf_snow_inputs* sub, const int32_t* sub_of_day, int32_t ndays,
                                        double reqhgt, double mat, const int32_t outsel[MCF_NOUT], int32_t reuse_static) {
    if (!sp || !sub || !sub_of_day || !outsel) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    int rc;
    if ((rc = common_checks(sub))) return rc;
    // Array weather (gridmicrosnow2, cpp:5058-5214): `sub` then carries the WHOLE series — obstime [T], clim.* as [rows,cols,T],
    // clim.winddir [T], other.lats / lons — and sub_of_day says which of its days form the snow-day subset series (subsetting
    // nine arrays on the host would copy them; here a chunk's snow days are uploaded when the chunk's microclimate runs).
    const bool maf = sub->array_forcing != 0;
    if (maf != sp->af) return mcf::api_fail(MCF_ERR_ARG, "micro set-up: the weather's geometry (data.frame / array) is not the snow plan's");
    if (sub->rows != sp->rows || sub->cols != sp->cols) return mcf::api_fail(MCF_ERR_ARG, "micro set-up: the raster is not the plan's");
    if (ndays * 24 > sp->T) return mcf::api_fail(MCF_ERR_ARG, "micro set-up: more days than the series");
    if (maf && sub->tsteps != sp->T) return mcf::api_fail(MCF_ERR_ARG, "micro set-up, array weather: the whole series is expected");
    if (outsel[MCF_OUT_SOILM] && !sub->other.Smax) return mcf::api_fail(MCF_ERR_ARG, "soilm requested but other$Smax is null");
    HIP_TRY(hipSetDevice(sp->device));
    sp->mb.release_all();
    sp->micro_ready = false;
    // reuse_static: vegetation, terrain and Smax are those of the previous set-up (a year's day list changes, the raster does
    // not) — 45 matrices that are not uploaded again
    const bool keep_static = reuse_static && sp->micro_static;
    const MicroArgs prev = sp->ma;
    if (!keep_static) { sp->mbs.release_all(); sp->micro_static = false; }
    const int64_t N = sp->N;
    int nsub = 0;
    for (int d = 0; d < ndays; ++d) nsub += sub_of_day[d] >= 0;
    const int T = maf ? nsub * 24 : (int)sub->tsteps;          // steps of the subset series
    for (int d = 0; d < ndays; ++d)
        if (sub_of_day[d] >= 0 && (int64_t)sub_of_day[d] * 24 + 24 > T) return mcf::api_fail(MCF_ERR_ARG, "micro set-up: day map points past the subset series");
    if (maf) {       // the subset's days in the order of the series (the albedo clock and the kernel's addressing walk them so)
        int next = 0;
        for (int d = 0; d < ndays; ++d)
            if (sub_of_day[d] >= 0 && sub_of_day[d] != next++) return mcf::api_fail(MCF_ERR_ARG, "micro set-up, array weather: the day map must number the snow days 0, 1, 2, ... in order");
    }
    sp->sub_of_day.assign(sub_of_day, sub_of_day + ndays);
    sp->micro_af = maf;
    mcf::DevOwner& b = sp->mb;
    MicroArgs& a = sp->ma;
    memset(&a, 0, sizeof a);
    a.N = N; a.tsteps = T; a.reqhgt = reqhgt; a.mat = mat; a.zref = sub->other.zref;
    int y0 = sub->obstime.year[0];          // the SUBSET series' first year (array weather: `sub` is the whole series)
    if (maf)
        for (int d = 0; d < ndays; ++d)
            if (sub_of_day[d] == 0) { y0 = sub->obstime.year[(size_t)d * 24]; break; }
    a.hiy = hours_in_year(y0);
    if (keep_static) {
        each_micro_raster(*sub, [&](auto*, auto member, int, bool, const char*) { a.*member = prev.*member; });
        if (outsel[MCF_OUT_SOILM] && !a.Smax) return mcf::api_fail(MCF_ERR_ARG, "micro set-up: soilm was not part of the static set-up being reused");
    } else {
        // (into the static buffer set: these uploads outlive the next set-up)
        each_micro_raster(*sub, [&](auto* host, auto member, int layers, bool required, const char* name) {
            if (!rc && (required || host)) rc = sp->mbs.up(&(a.*member), host, layers * N, name);
        });
        if (rc) return rc;
        sp->micro_static = true;
    }
    if (maf) {
        if (T == 0) return mcf::api_fail(MCF_ERR_ARG, "micro set-up, array weather: no snow day");
        bool given = true;
        each_micro_series(*sub, [&](auto* host, auto member, const char*) { given = given && (host || !member); });
        // (a plan with the microclimate's coarse arrays attached expands the series itself: `sub` carries none)
        if (!given && !sp->mcoarse) return mcf::api_fail(MCF_ERR_ARG, "micro set-up, array weather: a weather array is null");
        if (!sub->other.lats || !sub->other.lons || !sub->clim.winddir) return mcf::api_fail(MCF_ERR_ARG, "micro set-up, array weather: lats / lons / winddir");
        if ((rc = up_sites(b, a, sub, N))) return rc;
        // the subset series' date rows (obstime and wind direction of the snow days)
        mcf::HostCopies rows;
        mcf_snow_inputs ds = *sub;
        mcf::subset_days(ds, false, sub_of_day, ndays, nsub, rows);
        StepTables tabs;
        if ((rc = build_step_tables(b, &ds, true, false, false, &tabs))) return rc;
        a.rows = tabs.rows; a.dates = tabs.dates; a.mxtc1 = tabs.mxtc1;
        HIP_TRY(hipDeviceSynchronize());      // (the table kernels have read the host vectors' uploads)
        // the slabs a chunk's snow days are uploaded into, addressed with the subset series' step numbers (mcf_snowplan_microsnow
        // shifts the bases by the chunk's first subset day)
        const int64_t CN = (int64_t)sp->chunk * N;
        int f = 0;
        each_micro_series(*sub, [&](auto* host, auto member, const char*) {
            if (!member) return;
            sp->h_micro[f] = host;
            sp->micro_arg[f] = member;
            if (!rc) rc = b.make(&sp->d_micro[f], CN);
            ++f;
        });
        if (rc) return rc;
        const double *h_temp = sub->clim.temp, *h_precip = sub->clim.precip;
        // mxtc and the albedo clock at every subset day's start: the series' temperature and precipitation streamed once, a run of
        // consecutive snow days at a time through the first two slabs
        if ((rc = b.make(&a.mxtc, N))) return rc;
        if ((rc = b.make(&a.hs0, N * (int64_t)std::max(nsub, 1)))) return rc;
        int32_t* d_hs;
        if ((rc = b.make(&d_hs, N))) return rc;
        HIP_TRY(hipMemset(a.mxtc, 0, (size_t)N * 8));
        const int cd = sp->chunk / 24;
        for (int d = 0; d < ndays;) {
            if (sub_of_day[d] < 0) { ++d; continue; }
            int e = d;
            while (e < ndays && sub_of_day[e] >= 0 && e - d < cd) ++e;
            const int64_t off = (int64_t)d * 24 * N, n = (int64_t)(e - d) * 24 * N;
            if (sp->mcoarse) {          // the run's temp and precip expanded from the resident coarse arrays
                if ((rc = micro_coarse_fill(sp, (int64_t)d * 24, (e - d) * 24, 0, 1u << MF_TEMP | 1u << MF_PRECIP, sp->d_micro[1]))) return rc;
            } else {
                HIP_TRY(hipMemcpyAsync(sp->d_micro[0], h_temp + off, (size_t)n * 8, hipMemcpyHostToDevice, nullptr));
                HIP_TRY(hipMemcpyAsync(sp->d_micro[1], h_precip + off, (size_t)n * 8, hipMemcpyHostToDevice, nullptr));
            }
            hipLaunchKernelGGL(k_micro_scan, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, (const double*)sp->d_micro[0],
                               (const double*)sp->d_micro[1], N, sub_of_day[d], e - d, a.hgt, a.mxtc, d_hs, a.hs0);
            HIP_TRY(hipGetLastError());
            d = e;
        }
    } else {
        StepTables tabs;
        if ((rc = build_step_tables(b, sub, false, false, false, &tabs))) return rc;
        a.rows = tabs.rows; a.dates = tabs.dates; a.mxtc1 = tabs.mxtc1;
        each_micro_series(*sub, [&](auto* host, auto member, const char* name) { if (!rc && member) rc = b.up(&(a.*member), host, T, name); });
        if (!rc) rc = build_micro_steps(b, a);
        if (rc) return rc;
    }
    // the chunk's snow series, where mcf_snowplan_run_chunk leaves them (sdepc holds totalSWE after the redistribution)
    a.sTc = sp->a.Tc; a.sTg = sp->a.Tg; a.swe = sp->a.sdepc; a.sdepg = sp->a.sdepg; a.sden = sp->a.sden;
    // meanDsnow of the first pass (mcf_snowplan_meand_accumulate over every chunk)
    hipLaunchKernelGGL(k_meand_finish, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, (const double*)sp->d_sumD,
                       (const int32_t*)sp->d_sden_na, a.hgt, N, (double)std::max<int64_t>(sp->sumD_steps, 1), sp->d_meanD);
    HIP_TRY(hipGetLastError());
    a.meanD = sp->d_meanD;
    memcpy(sp->outsel, outsel, sizeof sp->outsel);
    HIP_TRY(hipDeviceSynchronize());
    sp->micro_ready = true;
    return MCF_OK;
}
// one lane per cell: a cell that is not under snow at every step of the days (or has no vegetation height: gridmicrosnow1 skips
// it) clears its tile's flag
__global__ __launch_bounds__(256) void k_tiles_covered(const double* __restrict__ swe, const double* __restrict__ hgt, int64_t N, int k0,
                                                       int nsteps, int cpb, uint8_t* __restrict__ flag) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    bool cov = !isnan(hgt[c]);
    for (int k = 0; cov && k < nsteps; ++k) cov = swe[c + N * (int64_t)(k0 + k)] > 0.0;
    if (!cov) flag[c / cpb] = 0;
}
extern "C" int mcf_snowplan_covered_tiles(mcf_snowplan* sp, mcf_plan* plan, int32_t ch, int32_t day, int32_t ndays, uint8_t* skip_tile,
                                          int64_t n_tiles, int64_t* n_covered) {
    if (!sp || !plan || !skip_tile || !n_covered) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (!sp->micro_ready) return mcf::api_fail(MCF_ERR_STATE, "snow plan: mcf_snowplan_micro_setup first");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    const int ns = std::min(sp->chunk, sp->T - ch * sp->chunk);
    if (day < 0 || ndays < 1 || (day + ndays) * 24 > ns) return mcf::api_fail(MCF_ERR_ARG, "days outside the chunk");
    hipStream_t stream;
    int64_t N;
    int device, slot_days, rc;
    mcf::RingView views[MCF_NOUT];
    int32_t has[MCF_NOUT];
    if ((rc = mcf::plan_ring_views(plan, 0, views, has, &stream, &N, &device, &slot_days))) return rc;
    int cpb = 0;
    bool all_sel = true;
    for (int v = 0; v < MCF_NOUT; ++v)
        if (has[v]) { cpb = views[v].cpb; all_sel = all_sel && sp->outsel[v] != 0; }
    if (cpb <= 0) return mcf::api_fail(MCF_ERR_STATE, "the snow-day microclimate needs a plan with the tiled ring (reqhgt >= 0)");
    if (N != sp->N || device != sp->device) return mcf::api_fail(MCF_ERR_ARG, "snow plan and solver plan differ in raster or device");
    if (n_tiles != (N + cpb - 1) / cpb) return mcf::api_fail(MCF_ERR_ARG, "n_tiles is not the solver plan's number of tiles");
    *n_covered = 0;
    memset(skip_tile, 0, (size_t)n_tiles);
    if (!all_sel) return MCF_OK;           // an output the snow microclimate does not produce stays the solver's everywhere
    HIP_TRY(hipSetDevice(sp->device));
    if (!sp->d_tflag || sp->tflag_cap < n_tiles) {
        if ((rc = sp->b.make(&sp->d_tflag, n_tiles))) return rc;
        sp->tflag_cap = n_tiles;
    }
    const bool k = (size_t)ch < sp->kept.size() && sp->kept[ch].Tc;
    if (!k && !(sp->series_valid & 4u)) return mcf::api_fail(MCF_ERR_STATE, "snow plan: the chunk's totalSWE series was switched off (mcf_snowplan_set_series)");
    const double* swe = k ? sp->kept[ch].sdepc : sp->a.sdepc;
    HIP_TRY(hipMemset(sp->d_tflag, 1, (size_t)n_tiles));
    hipLaunchKernelGGL(k_tiles_covered, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, swe, sp->ma.hgt, N, day * 24, ndays * 24, cpb,
                       sp->d_tflag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(skip_tile, sp->d_tflag, (size_t)n_tiles, hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (int64_t t = 0; t < n_tiles; ++t) n += skip_tile[t] != 0;
    *n_covered = n;
    return MCF_OK;
}
// one lane per cell: 1 where the cell's solver values of the days survive the merge (k_tiles_covered's test, negated)
__global__ __launch_bounds__(256) void k_cells_free(const double* __restrict__ swe, const double* __restrict__ hgt, int64_t N, int k0,
                                                    int nsteps, uint8_t* __restrict__ need, unsigned long long* __restrict__ count) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool cov = false;
    if (c < N) {
        cov = !isnan(hgt[c]);
        for (int k = 0; cov && k < nsteps; ++k) cov = swe[c + N * (int64_t)(k0 + k)] > 0.0;
        need[c] = cov ? 0 : 1;
    }
    __shared__ int s_n;                     // (one atomic per workgroup: a wave-level one on a single address serialises the launch)
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint64_t b = __ballot(c < N && !cov);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_n, (int)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(count, (unsigned long long)s_n);
}
extern "C" int mcf_snowplan_free_cells(mcf_snowplan* sp, mcf_plan* plan, int32_t ch, int32_t day, int32_t ndays, const uint8_t** need_cell,
                                       int64_t* n_need) {
    if (!sp || !plan || !need_cell || !n_need) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (!sp->micro_ready) return mcf::api_fail(MCF_ERR_STATE, "snow plan: mcf_snowplan_micro_setup first");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    const int ns = std::min(sp->chunk, sp->T - ch * sp->chunk);
    if (day < 0 || ndays < 1 || (day + ndays) * 24 > ns) return mcf::api_fail(MCF_ERR_ARG, "days outside the chunk");
    hipStream_t stream;
    int64_t N;
    int device, slot_days, rc;
    mcf::RingView views[MCF_NOUT];
    int32_t has[MCF_NOUT];
    if ((rc = mcf::plan_ring_views(plan, 0, views, has, &stream, &N, &device, &slot_days))) return rc;
    bool all_sel = true, any = false;
    for (int v = 0; v < MCF_NOUT; ++v)
        if (has[v]) { any = true; all_sel = all_sel && sp->outsel[v] != 0; }
    if (!any) return mcf::api_fail(MCF_ERR_STATE, "the solver plan holds no output");
    if (N != sp->N || device != sp->device) return mcf::api_fail(MCF_ERR_ARG, "snow plan and solver plan differ in raster or device");
    HIP_TRY(hipSetDevice(sp->device));
    if (!sp->d_need || sp->need_cap < N) {
        if ((rc = sp->b.make(&sp->d_need, N + 16))) return rc;
        sp->need_cap = N;
    }
    *need_cell = sp->d_need;
    unsigned long long* d_count = (unsigned long long*)(sp->d_need + (N + 7) / 8 * 8);
    if (!all_sel) {                        // an output the snow microclimate does not produce stays the solver's everywhere
        HIP_TRY(hipMemset(sp->d_need, 1, (size_t)N));
        *n_need = N;
        return MCF_OK;
    }
    const bool k = (size_t)ch < sp->kept.size() && sp->kept[ch].Tc;
    if (!k && !(sp->series_valid & 4u)) return mcf::api_fail(MCF_ERR_STATE, "snow plan: the chunk's totalSWE series was switched off (mcf_snowplan_set_series)");
    const double* swe = k ? sp->kept[ch].sdepc : sp->a.sdepc;
    HIP_TRY(hipMemset(d_count, 0, 8));
    hipLaunchKernelGGL(k_cells_free, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, swe, sp->ma.hgt, N, day * 24, ndays * 24,
                       sp->d_need, d_count);
    HIP_TRY(hipGetLastError());
    unsigned long long n = 0;
    HIP_TRY(hipMemcpy(&n, d_count, 8, hipMemcpyDeviceToHost));       // (also: the flags are complete)
    *n_need = (int64_t)n;
    return MCF_OK;
}
extern "C" int mcf_snowplan_microsnow(mcf_snowplan* sp, mcf_plan* plan, int32_t ch, int32_t slot, const int32_t* nosnowday) {
    if (!sp || !plan || !nosnowday) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (!sp->micro_ready) return mcf::api_fail(MCF_ERR_STATE, "snow plan: mcf_snowplan_micro_setup first");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    MicroRingArgs q;
    memset(&q, 0, sizeof q);
    hipStream_t stream;
    int64_t N;
    int device, slot_days, rc;
    mcf::RingView views[MCF_NOUT];
    int32_t has[MCF_NOUT];
    if ((rc = mcf::plan_ring_views(plan, slot, views, has, &stream, &N, &device, &slot_days))) return rc;
    for (int v = 0; v < MCF_NOUT; ++v) {
        if (!has[v]) continue;
        if (!q.held) { q.base0 = const_cast<double*>(views[v].base); q.ring = views[v]; }
        q.held |= 1u << v;
    }
    if (!q.held || q.ring.cpb <= 0) return mcf::api_fail(MCF_ERR_STATE, "the snow-day microclimate needs a plan with the tiled ring (reqhgt >= 0)");
    {   // the held variables' blocks follow each other at one stride (mcf_kernels.h RingView: [tile][day][variable][block])
        int rank = 0;
        const double* prev = nullptr;
        for (int v = 0; v < MCF_NOUT; ++v) {
            if (!has[v]) continue;
            if (rank == 1) q.vstride = views[v].base - prev;
            if (rank >= 1 && views[v].base - prev != q.vstride) return mcf::api_fail(MCF_ERR_STATE, "snow-day microclimate: the ring's variables are not equally spaced");
            prev = views[v].base;
            ++rank;
        }
    }
    if (N != sp->N || device != sp->device) return mcf::api_fail(MCF_ERR_ARG, "snow plan and solver plan differ in raster or device");
    const int ns = std::min(sp->chunk, sp->T - ch * sp->chunk), nd = ns / 24, day0 = ch * (sp->chunk / 24);
    if (nd > slot_days) return mcf::api_fail(MCF_ERR_ARG, "the ring slot holds fewer days than a snow chunk");
    if (day0 + nd > (int)sp->sub_of_day.size()) return mcf::api_fail(MCF_ERR_ARG, "chunk past the day map of the micro set-up");
    HIP_TRY(hipSetDevice(sp->device));
    int any = 0;
    for (int d = 0; d < nd; ++d) any |= sp->sub_of_day[day0 + d] >= 0;
    if (!any) return MCF_OK;
    // (the snow kernels run on the null stream, which orders itself against the plan's non-blocking stream only through the
    // explicit waits here: the solver's launches of this chunk first, this kernel before the plan's next use of the slot)
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(sp->d_daymap, sp->sub_of_day.data() + day0, (size_t)nd * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sp->d_nosnow, nosnowday, (size_t)nd * 4, hipMemcpyHostToDevice));
    q.m = sp->ma;
    q.m.day0 = 0;
    {   // the chunk's snow series: where pass 1 left them if the chunk was kept, the plan's working buffers otherwise
        const bool k = (size_t)ch < sp->kept.size() && sp->kept[ch].Tc;
        if (!k && sp->series_valid != 31) return mcf::api_fail(MCF_ERR_STATE, "snow plan: the chunk was run with series switched off (mcf_snowplan_set_series)");
        q.m.sTc = k ? sp->kept[ch].Tc : sp->a.Tc;
        q.m.sTg = k ? sp->kept[ch].Tg : sp->a.Tg;
        q.m.tzd = k ? sp->kept[ch].tzd : sp->a.tzd;          // (written with the Tg series: every series of the chunk is there, checked above)
        q.m.swe = k ? sp->kept[ch].sdepc : sp->a.sdepc;
        q.m.sdepg = k ? sp->kept[ch].sdepg : sp->a.sdepg;
        q.m.sden = k ? sp->kept[ch].sden : sp->a.sden;
    }
    for (int v = 0; v < MCF_NOUT; ++v) q.sel |= sp->outsel[v] ? 1u << v : 0u;
    q.daymap = sp->d_daymap; q.nosnow = sp->d_nosnow; q.ndays = nd;
    static const bool old_shape = getenv("MCF_MICRORING_OLD") != nullptr;      // A/B
    if (sp->micro_af) {
        // array weather: the chunk's snow days of the nine series into the slabs; the kernel addresses a series with the subset's
        // step number, so the bases are shifted back by the chunk's first subset day
        int sub_first = -1;
        if (sp->mcoarse) {
            // coarse array weather: one expansion launch per run of consecutive snow days (their subset numbers are consecutive
            // too); the slab offset (sub - sub_first) x 24 x N stays inside chunk x N
            for (int d = 0; d < nd;) {
                const int sb = sp->sub_of_day[day0 + d];
                if (sb < 0) { ++d; continue; }
                if (sub_first < 0) sub_first = sb;
                int e = d + 1;
                while (e < nd && sp->sub_of_day[day0 + e] >= 0) ++e;
                if ((rc = micro_coarse_fill(sp, (int64_t)(day0 + d) * 24, (e - d) * 24, (int64_t)(sb - sub_first) * 24, kMicroAll, nullptr))) return rc;
                d = e;
            }
        } else {
            for (int d = 0; d < nd; ++d) {
                const int sb = sp->sub_of_day[day0 + d];
                if (sb < 0) continue;
                if (sub_first < 0) sub_first = sb;
                for (int f = 0; f < kMicroSeries; ++f)
                    HIP_TRY(hipMemcpyAsync(sp->d_micro[f] + (int64_t)(sb - sub_first) * 24 * N, sp->h_micro[f] + (int64_t)(day0 + d) * 24 * N,
                                         (size_t)24 * N * 8, hipMemcpyHostToDevice, nullptr));
            }
        }
        const int64_t back = (int64_t)sub_first * 24 * N;
        for (int f = 0; f < kMicroSeries; ++f) q.m.*sp->micro_arg[f] = sp->d_micro[f] - back;
        hipLaunchKernelGGL(k_microsnow_ring<true>, dim3((unsigned)((N + 63) / 64), (unsigned)nd), dim3(256), 0, nullptr, q, (const void*)q.m.dates,
                           q.daymap, q.nosnow);
    } else if (q.ring.cpb == 21 && !old_shape) {
        // below ground with `out[c(1, 4)]`: the instantiation that reads nothing of the site, the radiation or the canopy
        // (MCF_MICROSNOW_GENERIC: the generic one, for A/B runs — the values are the same)
        const bool lean = q.m.reqhgt < 0 && !(q.sel & q.held & ~9u) && !getenv("MCF_MICROSNOW_GENERIC");
        if (lean)
            hipLaunchKernelGGL(k_microsnow_tiles<true>, dim3((unsigned)((N + kRtCells - 1) / kRtCells)), dim3(64 * kRtWaves), 0, nullptr, q,
                               (const MicroStep*)q.m.mstep, q.daymap, q.nosnow);
        else
            hipLaunchKernelGGL(k_microsnow_tiles<false>, dim3((unsigned)((N + kRtCells - 1) / kRtCells)), dim3(64 * kRtWaves), 0, nullptr, q,
                               (const MicroStep*)q.m.mstep, q.daymap, q.nosnow);
    }
    else
        hipLaunchKernelGGL(k_microsnow_ring<false>, dim3((unsigned)((N + 63) / 64), (unsigned)nd), dim3(256), 0, nullptr, q, q.m.mstep,
                           q.daymap, q.nosnow);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}

// ---- period summaries of the five series (include/mcf.h "period summaries of the snow run and of the snowpack"; the kernels:
// mcf_summary.hip k_summary_planes / _fin / _init) ---------------------------------------------------------------------------------
namespace mcf {   // mcf_snowrun.hip judges a spec with it before a device is needed
int snowpack_spec_check(const mcf_snowpack_summary_spec* s, int64_t tsteps, int64_t chunk_steps) {
    if (!s) return api_fail(MCF_ERR_ARG, "null mcf_snowpack_summary_spec");
    if (s->nperiods < 1) return api_fail(MCF_ERR_ARG, "snowpack summary: nperiods must be at least 1");
    if (chunk_steps <= 0) chunk_steps = 120;
    if (chunk_steps % 24) return api_fail(MCF_ERR_ARG, "snowpack summary: chunk_steps must be a multiple of 24");
    const int64_t ndays = tsteps / 24, covered = std::max<int64_t>(1, tsteps / chunk_steps) * (chunk_steps / 24);
    if (ndays > 0 && !s->period_of_day) return api_fail(MCF_ERR_ARG, "snowpack summary: null period_of_day");
    for (int64_t d = 0; d < ndays; ++d) {
        const int per = s->period_of_day[d];
        if (per < -1 || per >= s->nperiods)
            return api_fail(MCF_ERR_ARG, "snowpack summary: period_of_day[" + std::to_string(d) + "] = " + std::to_string(per) +
                                             " is outside -1 .. nperiods - 1");
        if (per >= 0 && d >= covered)
            return api_fail(MCF_ERR_ARG, "snowpack summary: day " + std::to_string(d) + " is counted but lies past the last whole chunk "
                                             "(no chunk covers it: its table entry must be -1)");
    }
    int nv = 0, ns = 0;
    for (int v = 0; v < 5; ++v) nv += s->series[v] ? 1 : 0;
    for (int k = 0; k < MCF_NSTAT; ++k) ns += s->stat[k] ? 1 : 0;
    if (nv == 0) return api_fail(MCF_ERR_ARG, "snowpack summary: no series selected");
    if (ns == 0) return api_fail(MCF_ERR_ARG, "snowpack summary: no statistic selected");
    for (int v = 0; v < 5; ++v)
        if (s->series[v] && s->stat[MCF_STAT_HOURS_ABOVE] && std::isnan(s->threshold[v]))
            return api_fail(MCF_ERR_ARG, "snowpack summary: HOURS_ABOVE needs a threshold for every selected series (NaN given)");
    return MCF_OK;
}
// the selected series as a mcf_snowplan_set_series mask (bit 2 is totalSWE, bit 3 the ground snow depth)
uint32_t snowpack_series_bits(const mcf_snowpack_summary_spec* s) {
    static const uint32_t bit[5] = {1u, 2u, 8u, 4u, 16u};
    uint32_t m = 0;
    for (int v = 0; v < 5; ++v) m |= s->series[v] ? bit[v] : 0u;
    return m;
}
}  // namespace mcf

extern "C" int mcf_snowplan_summary_reset(mcf_snowplan* sp) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null snow plan");
    if (!sp->d_ps_state) return mcf::api_fail(MCF_ERR_STATE, "the snow plan has no summary: mcf_snowplan_summary_enable first");
    HIP_TRY(hipSetDevice(sp->device));
    mcf::launch_summary_init(sp->d_ps_state, (int64_t)sp->ps_nsel * sp->ps_nperiods * sp->ps_nrows * sp->N, sp->N, sp->ps_nrows,
                             sp->ps_init_codes, nullptr);
    HIP_TRY(hipGetLastError());
    sp->ps_days.assign((size_t)sp->ps_nperiods, 0);
    sp->ps_next_chunk = 0;
    return MCF_OK;
}

extern "C" int mcf_snowplan_summary_enable(mcf_snowplan* sp, const mcf_snowpack_summary_spec* spec) {
    if (!sp || !spec) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (sp->d_ps_state) return mcf::api_fail(MCF_ERR_STATE, "snowpack summaries are already enabled on this plan");
    int rc = mcf::snowpack_spec_check(spec, sp->T, sp->chunk);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(sp->device));
    // state rows as mcf_plan_summary_enable lays them out: the sum's (it carries the NA rule), then one per other statistic
    int nrows = 1, row[MCF_NSTAT];
    uint32_t codes = 0;
    for (int k = 0; k < MCF_NSTAT; ++k) {
        row[k] = !spec->stat[k] ? -1 : k == MCF_STAT_MEAN ? 0 : nrows++;
        if (row[k] > 0 && k == MCF_STAT_MIN) codes |= 1u << (4 * row[k]);
        if (row[k] > 0 && k == MCF_STAT_MAX) codes |= 2u << (4 * row[k]);
    }
    int nsel = 0;
    for (int v = 0; v < 5; ++v) nsel += spec->series[v] ? 1 : 0;
    const int ndays = sp->T / 24;
    const int64_t nd = std::max(ndays, 1), np = spec->nperiods;
    const int64_t state_bytes = (int64_t)nsel * np * nrows * sp->N * 8, plane_bytes = np * sp->N * 8;
    if ((rc = check_room(state_bytes + plane_bytes + (3 * nd + np) * 4))) return rc;
    std::vector<int32_t> pod, prev, next;
    if ((rc = mcf::period_tables(spec->period_of_day, ndays, (int)np, pod, prev, next))) return rc;
    int32_t** tabs[3] = {&sp->d_ps_pod, &sp->d_ps_prev, &sp->d_ps_next};
    const std::vector<int32_t>* host[3] = {&pod, &prev, &next};
    for (int i = 0; i < 3; ++i) {
        if ((rc = sp->b.make(tabs[i], nd))) return rc;
        HIP_TRY(hipMemcpy(*tabs[i], host[i]->data(), (size_t)nd * 4, hipMemcpyHostToDevice));
    }
    if ((rc = sp->b.make(&sp->d_ps_days, np))) return rc;
    if ((rc = sp->b.make(&sp->d_ps_plane, np * sp->N))) return rc;
    double* state;
    if ((rc = sp->b.make(&state, (int64_t)nsel * np * nrows * sp->N))) return rc;
    sp->ps_nperiods = (int)np; sp->ps_nrows = nrows; sp->ps_nsel = nsel; sp->ps_init_codes = codes;
    for (int k = 0; k < MCF_NSTAT; ++k) sp->ps_row[k] = row[k];
    int place = 0;
    for (int v = 0; v < 5; ++v) {
        sp->ps_sel1[v] = spec->series[v] ? ++place : 0;
        sp->ps_thr[v] = spec->series[v] && spec->stat[MCF_STAT_HOURS_ABOVE] ? spec->threshold[v] : 0.0;
    }
    sp->ps_bits = mcf::snowpack_series_bits(spec);
    sp->ps_pod = std::move(pod);
    sp->d_ps_state = state;
    return mcf_snowplan_summary_reset(sp);
}

extern "C" int mcf_snowplan_summary_accumulate(mcf_snowplan* sp, int32_t ch) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "null snow plan");
    if (!sp->d_ps_state) return mcf::api_fail(MCF_ERR_STATE, "the snow plan has no summary: mcf_snowplan_summary_enable first");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "chunk out of range");
    if (ch < sp->ps_next_chunk)
        return mcf::api_fail(MCF_ERR_STATE, "snowpack summary: chunks arrive in ascending order, each at most once (chunk " + std::to_string(ch) +
                                                " after chunk " + std::to_string(sp->ps_next_chunk - 1) + ")");
    if ((sp->series_valid & sp->ps_bits) != sp->ps_bits)
        return mcf::api_fail(MCF_ERR_STATE, "snowpack summary: a selected series of the chunk was switched off (mcf_snowplan_set_series)");
    const int cd = sp->chunk / 24, day0 = ch * cd;
    const int nd = std::min(sp->chunk, sp->T - ch * sp->chunk) / 24;       // (whole days of the chunk: a one-chunk series shorter than a chunk)
    sp->ps_next_chunk = ch + 1;
    if (nd < 1) return MCF_OK;
    HIP_TRY(hipSetDevice(sp->device));
    mcf::SummaryPlanesArgs a{};
    const double* const dev[5] = {sp->a.Tc, sp->a.Tg, sp->a.sdepg, sp->a.sdepc, sp->a.sden};      // (sdepc: totalSWE after the redistribution)
    for (int v = 0; v < 5; ++v)
        if (sp->ps_sel1[v]) {
            a.series[sp->ps_sel1[v] - 1] = dev[v];
            a.threshold[sp->ps_sel1[v] - 1] = sp->ps_thr[v];
        }
    a.N = sp->N; a.nsel = sp->ps_nsel; a.nperiods = sp->ps_nperiods; a.nrows = sp->ps_nrows;
    for (int k = 0; k < MCF_NSTAT; ++k) a.row[k] = sp->ps_row[k];
    a.period_of_day = sp->d_ps_pod; a.prev_same = sp->d_ps_prev; a.next_same = sp->d_ps_next;
    a.day0 = day0; a.ndays = nd;
    a.state = sp->d_ps_state;
    mcf::launch_summary_planes(a, nullptr);          // the null stream: behind k_snowmodel, which wrote the series on it
    HIP_TRY(hipGetLastError());
    for (int d = day0; d < day0 + nd; ++d)
        if (sp->ps_pod[(size_t)d] >= 0) sp->ps_days[(size_t)sp->ps_pod[(size_t)d]] += 1;
    return MCF_OK;
}

extern "C" int mcf_snowplan_summary_fetch(mcf_snowplan* sp, int32_t series, int32_t stat, double* host_dst, int64_t row_pitch) {
    if (!sp || !host_dst) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (!sp->d_ps_state) return mcf::api_fail(MCF_ERR_STATE, "the snow plan has no summary: mcf_snowplan_summary_enable first");
    if (series < 0 || series >= 5 || stat < 0 || stat >= MCF_NSTAT) return mcf::api_fail(MCF_ERR_ARG, "bad series / statistic");
    if (!sp->ps_sel1[series]) return mcf::api_fail(MCF_ERR_ARG, "series was not selected in mcf_snowplan_summary_enable");
    if (sp->ps_row[stat] < 0) return mcf::api_fail(MCF_ERR_ARG, "statistic was not selected in mcf_snowplan_summary_enable");
    if (row_pitch == 0) row_pitch = sp->rows;
    if (row_pitch < sp->rows) return mcf::api_fail(MCF_ERR_ARG, "row_pitch smaller than rows");
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipMemcpy(sp->d_ps_days, sp->ps_days.data(), (size_t)sp->ps_nperiods * 4, hipMemcpyHostToDevice));
    mcf::SummaryFinArgs f{};
    f.state = sp->d_ps_state + (int64_t)(sp->ps_sel1[series] - 1) * sp->ps_nperiods * sp->ps_nrows * sp->N;
    f.N = sp->N; f.nperiods = sp->ps_nperiods; f.nrows = sp->ps_nrows;
    f.stat = stat; f.row = sp->ps_row[stat];
    f.days = sp->d_ps_days; f.out = sp->d_ps_plane;
    mcf::launch_summary_fin(f, nullptr);
    HIP_TRY(hipGetLastError());
    const size_t width = (size_t)sp->rows * 8, bytes = (size_t)(sp->N * sp->ps_nperiods) * 8;
    if (row_pitch != sp->rows) HIP_TRY(sp->dl.pitched(host_dst, (size_t)row_pitch * 8, sp->d_ps_plane, width, bytes / width));
    else HIP_TRY(sp->dl.dense(host_dst, sp->d_ps_plane, bytes));
    return MCF_OK;
}

extern "C" int mcf_snowplan_summary_days(mcf_snowplan* sp, int32_t* days) {
    if (!sp || !days) return mcf::api_fail(MCF_ERR_ARG, "null argument");
    if (!sp->d_ps_state) return mcf::api_fail(MCF_ERR_STATE, "the snow plan has no summary: mcf_snowplan_summary_enable first");
    for (int k = 0; k < sp->ps_nperiods; ++k) days[k] = sp->ps_days[(size_t)k];
    return MCF_OK;
}

// ---- series sink of the five series (include/mcf.h "series sink of the snow run and of the snowpack"; the kernels:
// mcf_series.hip k_series_planes / _points_planes / _fin / _init) -----------------------------------------------
namespace mcf {   // mcf_snowrun.hip judges a spec with it before a device is needed
int snowpack_series_check(const std::string& who, const mcf_snowpack_series_spec* s, int64_t rows, int64_t cols, int64_t chunk_steps) {
    if (!s) return api_fail(MCF_ERR_ARG, who + ": null mcf_snowpack_series_spec");
    const int64_t N = rows * cols;
    if (N > ((int64_t)1 << 26)) return api_fail(MCF_ERR_ARG, who + ": more than 2^26 cells (the fixed-point sum's range)");
    if (chunk_steps <= 0) chunk_steps = 120;
    if (chunk_steps % 24) return api_fail(MCF_ERR_ARG, who + ": chunk_steps must be a multiple of 24");
    int nv = 0, ns = 0;
    for (int v = 0; v < 5; ++v) nv += s->series[v] ? 1 : 0;
    for (int k = 0; k < MCF_NZSTAT; ++k) ns += s->zstat[k] ? 1 : 0;
    if (nv == 0) return api_fail(MCF_ERR_ARG, who + ": no series selected");
    if (s->npoints < 0) return api_fail(MCF_ERR_ARG, who + ": negative npoints");
    if (s->npoints == 0 && s->nzones == 0) return api_fail(MCF_ERR_ARG, who + ": neither points nor zones selected");
    if (s->nzones < 0 || s->nzones > MCF_MAX_ZONES)
        return api_fail(MCF_ERR_ARG, who + ": nzones = " + std::to_string(s->nzones) + " is outside 0 .. " + std::to_string(MCF_MAX_ZONES));
    if (s->nzones > 0) {
        if (!s->zone) return api_fail(MCF_ERR_ARG, who + ": null zone map");
        if (ns == 0) return api_fail(MCF_ERR_ARG, who + ": no statistic selected");
        for (int64_t c = 0; c < N; ++c)
            if (s->zone[c] < -1 || s->zone[c] >= s->nzones)
                return api_fail(MCF_ERR_ARG, who + ": zone[" + std::to_string(c) + "] = " + std::to_string(s->zone[c]) + " is outside -1 .. nzones - 1");
    }
    if (s->npoints > 0 && !s->cells) return api_fail(MCF_ERR_ARG, who + ": null cells");
    for (int64_t i = 0; i < s->npoints; ++i)
        if (s->cells[i] < 0 || s->cells[i] >= N)
            return api_fail(MCF_ERR_ARG, who + ": cells[" + std::to_string(i) + "] = " + std::to_string(s->cells[i]) + " is a cell index outside the raster");
    return MCF_OK;
}
// a block's raw zone state of one series, [4][nzones][whole days x 24] of int64, and its folded days (mcf_series_host.hpp
// combines the blocks'); sizes: snowplan_series_steps
int64_t snowplan_series_steps(const mcf_snowplan* sp) { return (int64_t)(sp->T / 24) * 24; }
int snowplan_series_state(mcf_snowplan* sp, int32_t series, int64_t* host_state, int32_t* day_done) {
    if (!sp || !sp->se_on || series < 0 || series >= 5 || !sp->se_sel1[series] || sp->se_nzones == 0)
        return api_fail(MCF_ERR_STATE, "snow plan: no zone state of this series");
    HIP_TRY(hipSetDevice(sp->device));
    const int64_t n = (int64_t)kSeriesRows * sp->se_nzones * snowplan_series_steps(sp);
    if (host_state) HIP_TRY(hipMemcpy(host_state, sp->d_se_state + (int64_t)(sp->se_sel1[series] - 1) * n, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (day_done) std::copy(sp->se_done.begin(), sp->se_done.end(), day_done);
    return MCF_OK;
}
}  // namespace mcf

extern "C" int mcf_snowplan_series_reset(mcf_snowplan* sp) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_reset: null snow plan");
    if (!sp->se_on) return mcf::api_fail(MCF_ERR_STATE, "the snow plan has no series sink: mcf_snowplan_series_enable first");
    HIP_TRY(hipSetDevice(sp->device));
    if (sp->d_se_points) mcf::launch_fill(sp->d_se_points, sp->se_nsel * sp->se_npoints * std::max(sp->T, 1), mcf::na_real_host(), nullptr);
    if (sp->d_se_state) mcf::launch_series_init(sp->d_se_state, sp->se_nsel, sp->se_nzones, mcf::snowplan_series_steps(sp), nullptr);
    HIP_TRY(hipGetLastError());
    sp->se_done.assign((size_t)std::max(sp->T / 24, 1), 0);
    sp->se_chunk_done.assign((size_t)std::max(sp->nchunks, 1), 0);
    return MCF_OK;
}

extern "C" int mcf_snowplan_series_enable(mcf_snowplan* sp, const mcf_snowpack_series_spec* spec) {
    const std::string who = "mcf_snowplan_series_enable";
    if (!sp || !spec) return mcf::api_fail(MCF_ERR_ARG, who + ": null argument");
    if (sp->se_on) return mcf::api_fail(MCF_ERR_STATE, who + ": the series sink is already enabled on this plan");
    int rc = mcf::snowpack_series_check(who, spec, sp->rows, sp->cols, sp->chunk);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(sp->device));
    int nsel = 0;
    for (int v = 0; v < 5; ++v) nsel += spec->series[v] ? 1 : 0;
    const int64_t np = spec->npoints, nz = spec->nzones, steps = mcf::snowplan_series_steps(sp), T = std::max(sp->T, 1);
    const int64_t point_bytes = nsel * np * T * 8, state_bytes = nsel * mcf::kSeriesRows * nz * steps * 8;
    if ((rc = check_room(point_bytes + state_bytes + nz * T * 8 + sp->N * 4))) return rc;
    if (np > 0) {
        if ((rc = sp->b.make(&sp->d_se_cells, np))) return rc;
        HIP_TRY(hipMemcpy(sp->d_se_cells, spec->cells, (size_t)np * 8, hipMemcpyHostToDevice));
        if ((rc = sp->b.make(&sp->d_se_points, nsel * np * T))) return rc;
    }
    if (nz > 0) {
        if ((rc = sp->b.make(&sp->d_se_zone, sp->N))) return rc;
        HIP_TRY(hipMemcpy(sp->d_se_zone, spec->zone, (size_t)sp->N * 4, hipMemcpyHostToDevice));
        if ((rc = sp->b.make(&sp->d_se_state, std::max<int64_t>(state_bytes / 8, 1)))) return rc;
        if ((rc = sp->b.make(&sp->d_se_plane, nz * T))) return rc;
        if ((rc = sp->b.make(&sp->d_se_done, std::max(sp->T / 24, 1)))) return rc;
    }
    sp->se_npoints = np; sp->se_nzones = (int)nz; sp->se_nsel = nsel;
    int cus = 0;      // persistent workgroups per selected series: one per compute unit
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sp->device) != hipSuccess || cus < 1) cus = 256;
    sp->se_workgroups = cus;
    static const uint32_t bit[5] = {1u, 2u, 8u, 4u, 16u};      // (as snowpack_series_bits: bit 2 is totalSWE, bit 3 the ground snow depth)
    int place = 0;
    sp->se_bits = 0;
    for (int v = 0; v < 5; ++v) {
        sp->se_sel1[v] = spec->series[v] ? ++place : 0;
        if (spec->series[v]) sp->se_bits |= bit[v];
    }
    for (int k = 0; k < MCF_NZSTAT; ++k) sp->se_zstat[k] = nz > 0 && spec->zstat[k] ? 1 : 0;
    sp->se_on = true;
    return mcf_snowplan_series_reset(sp);
}

extern "C" int mcf_snowplan_series_accumulate(mcf_snowplan* sp, int32_t ch) {
    if (!sp) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_accumulate: null snow plan");
    if (!sp->se_on) return mcf::api_fail(MCF_ERR_STATE, "the snow plan has no series sink: mcf_snowplan_series_enable first");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_accumulate: chunk out of range");
    if (sp->se_chunk_done[(size_t)ch])
        return mcf::api_fail(MCF_ERR_STATE, "mcf_snowplan_series_accumulate: chunk " + std::to_string(ch) + " has been folded already (each chunk at most once)");
    if ((sp->series_valid & sp->se_bits) != sp->se_bits)
        return mcf::api_fail(MCF_ERR_STATE, "mcf_snowplan_series_accumulate: a selected series of the chunk was switched off (mcf_snowplan_set_series)");
    const int cd = sp->chunk / 24, day0 = ch * cd;
    const int nd = std::min(sp->chunk, sp->T - ch * sp->chunk) / 24;       // (whole days of the chunk: a one-chunk series shorter than a chunk)
    sp->se_chunk_done[(size_t)ch] = 1;
    if (nd < 1) return MCF_OK;
    HIP_TRY(hipSetDevice(sp->device));
    const double* const dev[5] = {sp->a.Tc, sp->a.Tg, sp->a.sdepg, sp->a.sdepc, sp->a.sden};      // (sdepc: totalSWE after the redistribution)
    if (sp->se_npoints > 0) {
        mcf::SeriesPointsPlanesArgs a{};
        for (int v = 0; v < 5; ++v)
            if (sp->se_sel1[v]) a.series[sp->se_sel1[v] - 1] = dev[v];
        a.N = sp->N; a.nsel = sp->se_nsel; a.nsteps = (int64_t)nd * 24;
        a.cells = sp->d_se_cells; a.ncells = sp->se_npoints;
        a.dst = sp->d_se_points; a.dst_steps = std::max(sp->T, 1); a.dst_step0 = (int64_t)day0 * 24;
        mcf::launch_series_points_planes(a, nullptr);      // the null stream: behind k_snowmodel, which wrote the series on it
    }
    if (sp->se_nzones > 0) {
        mcf::SeriesPlanesArgs a{};
        for (int v = 0; v < 5; ++v)
            if (sp->se_sel1[v]) a.series[sp->se_sel1[v] - 1] = dev[v];
        a.N = sp->N; a.nsel = sp->se_nsel;
        a.zone = sp->d_se_zone; a.nzones = sp->se_nzones;
        a.steps = mcf::snowplan_series_steps(sp); a.nsteps = (int64_t)nd * 24;
        a.day0 = day0; a.ndays = nd;
        a.state = sp->d_se_state;
        mcf::launch_series_planes(a, sp->se_workgroups, nullptr);
    }
    HIP_TRY(hipGetLastError());
    for (int d = day0; d < day0 + nd; ++d) sp->se_done[(size_t)d] = 1;
    return MCF_OK;
}

extern "C" int mcf_snowplan_series_fetch_points(mcf_snowplan* sp, int32_t series, double* dst) {
    if (!sp || !dst) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_fetch_points: null argument");
    if (!sp->se_on) return mcf::api_fail(MCF_ERR_STATE, "the snow plan has no series sink: mcf_snowplan_series_enable first");
    if (series < 0 || series >= 5 || !sp->se_sel1[series])
        return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_fetch_points: series was not selected in mcf_snowplan_series_enable");
    if (sp->se_npoints == 0) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_fetch_points: no points were selected in mcf_snowplan_series_enable");
    HIP_TRY(hipSetDevice(sp->device));
    const int64_t n = sp->se_npoints * std::max(sp->T, 1);
    HIP_TRY(sp->dl.dense(dst, sp->d_se_points + (int64_t)(sp->se_sel1[series] - 1) * n, (size_t)n * 8));
    return MCF_OK;
}

extern "C" int mcf_snowplan_series_fetch_zones(mcf_snowplan* sp, int32_t series, int32_t zstat, double* dst) {
    if (!sp || !dst) return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_fetch_zones: null argument");
    if (!sp->se_on) return mcf::api_fail(MCF_ERR_STATE, "the snow plan has no series sink: mcf_snowplan_series_enable first");
    if (series < 0 || series >= 5 || !sp->se_sel1[series])
        return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_fetch_zones: series was not selected in mcf_snowplan_series_enable");
    if (zstat < 0 || zstat >= MCF_NZSTAT || !sp->se_zstat[zstat])
        return mcf::api_fail(MCF_ERR_ARG, "mcf_snowplan_series_fetch_zones: statistic was not selected in mcf_snowplan_series_enable");
    HIP_TRY(hipSetDevice(sp->device));
    const int64_t steps = mcf::snowplan_series_steps(sp), T = std::max(sp->T, 1);
    HIP_TRY(hipMemcpy(sp->d_se_done, sp->se_done.data(), (size_t)std::max(sp->T / 24, 1) * 4, hipMemcpyHostToDevice));
    mcf::launch_series_fin(sp->d_se_state + (int64_t)(sp->se_sel1[series] - 1) * mcf::kSeriesRows * sp->se_nzones * steps, sp->se_nzones,
                           steps, T, sp->d_se_done, zstat, sp->d_se_plane, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(sp->dl.dense(dst, sp->d_se_plane, (size_t)(T * sp->se_nzones) * 8));
    return MCF_OK;
}

// ---- netCDF sink of the five series (include/mcf.h "netCDF sink: further sources"; the kernel: mcf_ncpack.hip)
namespace mcf {
// Steps [step0, step0 + nsteps) of step-major device planes (dev[v]: series v of the file's, null: not held) as rows
// [row0, row0 + rows) of records [file_step0, ...) of a snowpack file: packed a piece at a time into *d_pack (grown through
// `grow`), copied and written before the next piece is packed.  On the null stream, behind the kernel that wrote the planes.
template <class Grow>
static int pack_planes_to_file(const std::string& w, mcf_ncfile* nc, const double* const dev[5], int64_t rows, int64_t cols, int64_t row0,
                               int64_t step0, int64_t file_step0, int64_t nsteps, int32_t** d_pack, int64_t* pack_elems, Grow&& grow,
                               ToHost& dl, float* kernel_ms) {
    NcFile* f = nc->f.get();
    if (!nc->snowpack) return api_fail(MCF_ERR_ARG, w + "the file does not hold the snowpack's series (mcf_nc_create_snowpack)");
    if (f->cols != cols || row0 < 0 || rows < 1 || row0 + rows > f->rows) return api_fail(MCF_ERR_ARG, w + "the rows at row0 are not a row strip of the file's grid");
    if (!(row0 == 0 && rows == f->rows) && !f->takes_strips())
        return api_fail(MCF_ERR_ARG, w + "the netCDF-4 container chunks a step into row strips of the whole raster: it takes one block, not a row strip");
    if (file_step0 < 0 || nsteps < 0 || file_step0 + nsteps > f->nsteps) return api_fail(MCF_ERR_ARG, w + "step range outside the file");
    PackNcPlanesArgs a{};
    a.nv = f->nvars; a.missval = NcFile::kMissval; a.rows = rows; a.cols = cols;
    const int64_t rb = 8 + (int64_t)a.nv * rows * cols * 4;
    a.rec_words = rb / 4;
    for (int k = 0; k < a.nv; ++k) {
        a.series[k] = dev[nc->out_of[k]];
        a.scale[k] = nc->scale[k];
        if (!a.series[k]) return api_fail(MCF_ERR_ARG, w + "a series of the file is missing");
    }
    if (kernel_ms) *kernel_ms = 0;
    if (nsteps == 0) return MCF_OK;
    const int64_t piece = std::min<int64_t>(nsteps, std::min<int64_t>(65535 / a.nv, std::max<int64_t>(1, ((int64_t)256 << 20) / rb)));
    if (*pack_elems < piece * (rb / 4)) {
        if (const int rc = grow(d_pack, piece * (rb / 4))) return rc;
        *pack_elems = piece * (rb / 4);
    }
    a.dst = *d_pack;
    std::unique_ptr<uint8_t[]> st(new uint8_t[(size_t)(piece * rb)]);      // this call's own: the blocks' workers write at the same time
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (kernel_ms) { HIP_TRY(hipEventCreate(&ev0)); HIP_TRY(hipEventCreate(&ev1)); }
    int rc = MCF_OK;
    for (int64_t s0 = 0; s0 < nsteps && !rc; s0 += piece) {
        const int64_t n = std::min(piece, nsteps - s0);
        a.step0 = step0 + s0;
        hipError_t e = kernel_ms ? hipEventRecord(ev0, nullptr) : hipSuccess;
        launch_pack_nc_planes(a, n, nullptr);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess && kernel_ms) e = hipEventRecord(ev1, nullptr);
        if (e == hipSuccess) e = dl.dense(st.get(), *d_pack, (size_t)(n * rb));
        if (e == hipSuccess && kernel_ms) {
            float ms = 0;
            e = hipEventSynchronize(ev1);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
            *kernel_ms += ms;
        }
        if (e != hipSuccess) { rc = api_fail(MCF_ERR_HIP, w + hipGetErrorString(e)); break; }
        const std::string we = f->write_strip(file_step0 + s0, n, row0, rows, st.get());
        if (!we.empty()) rc = api_fail(MCF_ERR_ARG, w + we);
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}
}  // namespace mcf

extern "C" int mcf_snowplan_nc_write(mcf_snowplan* sp, mcf_ncfile* nc, int32_t ch, int64_t row0) {
    const std::string w = "mcf_snowplan_nc_write: ";
    if (!sp || !nc) return mcf::api_fail(MCF_ERR_ARG, w + "null argument");
    if (ch < 0 || ch >= sp->nchunks) return mcf::api_fail(MCF_ERR_ARG, w + "chunk out of range");
    if (nc->f->nsteps != sp->T) return mcf::api_fail(MCF_ERR_ARG, w + "the file's steps are not the plan's");
    static const uint32_t bit[5] = {1u, 2u, 8u, 4u, 16u};      // (as the series sink: bit 2 is totalSWE, bit 3 the ground snow depth)
    for (int v = 0; v < 5; ++v)
        if (nc->snowpack && nc->var_of[v] >= 0 && !(sp->series_valid & bit[v]))
            return mcf::api_fail(MCF_ERR_STATE, w + "a series of the file was switched off for the chunk (mcf_snowplan_set_series)");
    HIP_TRY(hipSetDevice(sp->device));
    const double* const dev[5] = {sp->a.Tc, sp->a.Tg, sp->a.sdepg, sp->a.sdepc, sp->a.sden};      // (sdepc: totalSWE after the redistribution)
    const int64_t k0 = (int64_t)ch * sp->chunk, ns = std::min<int64_t>(sp->chunk, sp->T - k0);
    int rc = mcf::pack_planes_to_file(w, nc, dev, sp->rows, sp->cols, row0, 0, k0, ns, &sp->d_ncpack, &sp->ncpack_elems,
                                      [&](int32_t** d, int64_t n) { return sp->b.make(d, n); }, sp->dl, nullptr);
    if (rc || ch != sp->nchunks - 1) return rc;
    // the steps no chunk covers stay missval (R pre-fills its arrays with NA, int:2554-2558)
    const int64_t covered = std::min<int64_t>(sp->T, (int64_t)sp->nchunks * sp->chunk);
    const std::string e = mcf::nc_write_missing(nc->f.get(), row0, sp->rows, covered, sp->T - covered);
    return e.empty() ? (int)MCF_OK : mcf::api_fail(MCF_ERR_ARG, w + e);
}

extern "C" int mcf_nc_write_planes(mcf_ncfile* nc, const double* const series[5], int64_t rows, int64_t row0, int64_t file_step0,
                                   int64_t nsteps, int32_t device, float* kernel_ms) {
    const std::string w = "mcf_nc_write_planes: ";
    if (!nc || !series) return mcf::api_fail(MCF_ERR_ARG, w + "null argument");
    if (rows < 1 || nsteps < 0) return mcf::api_fail(MCF_ERR_ARG, w + "bad rows / nsteps");
    if (const int rc = mcf::check_device(device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(device));
    mcf::DevOwner b;
    mcf::ToHost dl;
    const int64_t n = rows * nc->f->cols * nsteps;
    const double* dev[5] = {};
    for (int v = 0; v < 5; ++v) {
        if (!series[v] || n == 0) continue;
        double* d = nullptr;
        if (const int rc = b.make(&d, n)) return rc;
        HIP_TRY(hipMemcpy(d, series[v], (size_t)n * 8, hipMemcpyHostToDevice));
        dev[v] = d;
    }
    int32_t* d_pack = nullptr;
    int64_t pack_elems = 0;
    return mcf::pack_planes_to_file(w, nc, dev, rows, nc->f->cols, row0, 0, file_step0, nsteps, &d_pack, &pack_elems,
                                    [&](int32_t** d, int64_t m) { return b.make(d, m); }, dl, kernel_ms);
}

extern "C" int32_t mcf_snowenv_from_name(const char* name) {
    if (!name) return MCF_SNOWENV_ALPINE;
    if (!strcmp(name, "Maritime")) return MCF_SNOWENV_MARITIME;
    if (!strcmp(name, "Prairie")) return MCF_SNOWENV_PRAIRIE;
    if (!strcmp(name, "Tundra")) return MCF_SNOWENV_TUNDRA;
    if (!strcmp(name, "Taiga")) return MCF_SNOWENV_TAIGA;
    return MCF_SNOWENV_ALPINE;
}
extern "C" int mcf_gridmodelsnow1(const mcf_snow_inputs* in, mcf_snowmodel_out* out, int32_t device) {
    return run_snowmodel(in, out, device, false);
}
extern "C" int mcf_gridmodelsnow2(const mcf_snow_inputs* in, mcf_snowmodel_out* out, int32_t device) {
    return run_snowmodel(in, out, device, true);
}
extern "C" int mcf_gridmicrosnow1(const mcf_snow_inputs* in, const mcf_snowm* snowm, double reqhgt, double mat,
                                  const int32_t out[MCF_NOUT], mcf_outputs* micro, int32_t device) {
    return run_microsnow(in, snowm, reqhgt, mat, out, micro, device, false);
}
extern "C" int mcf_gridmicrosnow2(const mcf_snow_inputs* in, const mcf_snowm* snowm, double reqhgt, double mat,
                                  const int32_t out[MCF_NOUT], mcf_outputs* micro, int32_t device) {
    return run_microsnow(in, snowm, reqhgt, mat, out, micro, device, true);
}
