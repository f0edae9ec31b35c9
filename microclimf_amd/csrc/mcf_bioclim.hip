// mcf_bioclim.hip — the streamed bioclim sink below ground at several depths (include/mcf.h mcf_runbioclim_depths; DESIGN.md
// §23).  Only adds, compares and one divide per day: nothing here can be contracted.
//
// k_bioclim_acc_depths<CPB, MOIST>  k_bioclim_acc's folds (mcf_kernels.hip), term for term, with the slabs staged as
//                 k_summary_acc stages them (mcf_tilestage.hpp): one workgroup = 256 / CPB consecutive tiles of ONE slab — a
//                 depth's Tz (MOIST = false, the depth on blockIdx.y) or the slot's soilm (MOIST = true, a launch of its own:
//                 soilm is read once per day, not once per depth).  Per day of the chunk the tiles' blocks come in through
//                 registers into LDS with 16-byte loads, every 128-byte line read once and whole; one lane per cell walks its
//                 24 places (ring_pos) in hour order and folds them into registers; the next day's loads are in flight while
//                 the lanes fold.  The quarter lists are ascending (the host checks it), so a quarter's entries of one day
//                 are one run of its list: they are folded day by day, in list order, from the block in LDS.
// k_bioclim_fin_temp  a depth's 21 temperature rows -> bio1..bio11, k_bioclim_fin's expressions; each depth under its own NA rule.
// (The moisture finish needs the solver's soil functions and lives beside k_bioclim_fin in mcf_kernels.hip.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcf.h"
#include "mcf_kernels.h"
#include "mcf_tilestage.hpp"

namespace mcf {
namespace {

constexpr unsigned long long kNaBits = 0x7FF00000000007A2ull;      // R's NA_real_

template <int CPB, bool MOIST>
__global__ __launch_bounds__(kSumLanes) void k_bioclim_acc_depths(BioAccDepthsArgs a) {
    using G = SumGeom<CPB>;
    __shared__ double lds[G::TPW * G::S];
    const int tid = (int)threadIdx.x, dep = MOIST ? 0 : (int)blockIdx.y;
    const int64_t tile0 = (int64_t)blockIdx.x * G::TPW, N = a.N;
    const int64_t left = a.ntiles - tile0;
    const int ntl = left < G::TPW ? (int)left : G::TPW;           // tiles of this group that exist in the ring
    const int tl = tid / CPB, cell = tid - tl * CPB;
    const int64_t c = tile0 * CPB + tid;
    const bool active = tid < G::TPW * CPB && c < N;              // cells >= N of the last tile: padding, never read into state
    // the slab: soilm and depth 0's Tz lie in the slot, the other depths beside it
    const bool own = MOIST || dep == 0;
    const int64_t tile_stride = own ? a.ring_tile_stride : a.tzx_tile_stride, day_stride = own ? a.ring_day_stride : a.tzx_day_stride;
    const double* src = (MOIST ? a.soilm : dep == 0 ? a.tz0 : a.tzx + (int64_t)(dep - 1) * a.tzx_stride) + tile0 * tile_stride;
    double* st = a.state + (MOIST ? (int64_t)a.ndepths * kBioTempRows * N : (int64_t)dep * kBioTempRows * N) + c;
    auto S = [&](int row) -> double& { return st[N * row]; };
    const double* L = lds + tl * G::S;
    const bool start = a.day0 == 0;

    // the running state, k_bioclim_acc's initial values on the first chunk
    double first = 0.0, s1 = 0.0, dsum = 0.0, b5 = -273.15, b6 = 273.15;          // temperature rows 0, 1, 2, 15, 16
    double me = 0.0, mx = 0.0, mn = 1.0, all = 0.0;                               // moisture rows 0 .. 3
    double qs[4] = {0.0, 0.0, 0.0, 0.0};                                          // rows 17 .. 20 / 4 .. 7
    int qpos[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) qpos[qi] = a.qlo[qi];
    if (active && !start) {
        if constexpr (MOIST) { me = S(0); mx = S(1); mn = S(2); all = S(3); }
        else { first = S(0); s1 = S(1); dsum = S(2); b5 = S(15); b6 = S(16); }
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) qs[qi] = S((MOIST ? 4 : 17) + qi);
    }

    double2 r[G::NLD];
    load_day<CPB>(r, src, tile_stride, tid, ntl);
    for (int dl = 0; dl < a.ndays; ++dl) {
        __syncthreads();                                          // the day before has left the LDS
        store_day<CPB>(lds, r, tid, ntl);
        __syncthreads();
        if (dl + 1 < a.ndays) load_day<CPB>(r, src + (int64_t)(dl + 1) * day_stride, tile_stride, tid, ntl);
        const int d = a.day0 + dl;
        if (!MOIST && start && dl == 0 && active) first = L[ring_pos(CPB, cell, 0)];
        // cpp:3505-3506: every value NA where the depth's first Tz is (k_bioclim_fin_temp); the moisture rows fold regardless
        // and take the rule from depth 0 in their finish
        if (!active || (!MOIST && first != first)) continue;
        if constexpr (MOIST) {
            if (d < 12) {                                         // bio12 cpp:3361
#pragma unroll 8
                for (int h = 0; h < 24; ++h) me = me + L[ring_pos(CPB, cell, h)];
            }
#pragma unroll 8
            for (int h = 0; h < 24; ++h) {                        // bio13, bio14, bio15's mean cpp:3371-3398
                const double v = L[ring_pos(CPB, cell, h)];
                if (v > mx) mx = v;
                if (v < mn) mn = v;
                all += v;
            }
        } else if (d < 12) {                                      // bio1 cpp:3245, bio2 cpp:3256, bio4 cpp:3279
            double tmx = -273.15, tmn = 273.15, ms = 0.0;
#pragma unroll
            for (int h = 0; h < 24; ++h) {
                const double v = L[ring_pos(CPB, cell, h)];
                s1 = s1 + v;
                if (v > tmx) tmx = v;
                if (v < tmn) tmn = v;
                ms = ms + v;
            }
            dsum = dsum + (tmx - tmn);
            S(3 + d) = ms / 24;
        } else if (d == 12) {                                     // bio5 cpp:3297
#pragma unroll
            for (int h = 0; h < 24; ++h) { const double v = L[ring_pos(CPB, cell, h)]; if (v > b5) b5 = v; }
        } else if (d == 13) {                                     // bio6 cpp:3307
#pragma unroll
            for (int h = 0; h < 24; ++h) { const double v = L[ring_pos(CPB, cell, h)]; if (v < b6) b6 = v; }
        }
        // the quarters' entries that fall into this day (cpp:3316-3358, 3406-3448), each sum in its list's order
        const int kend = (d + 1) * 24;
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            const int32_t* q = a.q[qi];
            int i = qpos[qi];
            for (; i < a.qhi[qi]; ++i) {
                const int k = q[i];
                if (k >= kend) break;
                qs[qi] = qs[qi] + L[ring_pos(CPB, cell, k - d * 24)];
            }
            qpos[qi] = i;
        }
    }
    if (!active) return;
    if constexpr (MOIST) { S(0) = me; S(1) = mx; S(2) = mn; S(3) = all; }
    else {
        if (start) S(0) = first;
        if (first != first) return;
        S(1) = s1; S(2) = dsum; S(15) = b5; S(16) = b6;
    }
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) S((MOIST ? 4 : 17) + qi) = qs[qi];
}

__global__ __launch_bounds__(256) void k_bioclim_fin_temp(const double* __restrict__ state, int64_t N, double* __restrict__ bio) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const double* st = state + (int64_t)blockIdx.y * kBioTempRows * N + c;
    auto S = [&](int row) { return st[N * row]; };
    double* out = bio + (int64_t)blockIdx.y * 11 * N + c;
    if (isnan(S(0))) {                                                  // cpp:3505-3506
        for (int b = 0; b < 11; ++b) out[N * b] = __longlong_as_double((long long)kNaBits);
        return;
    }
    double b[11];
    b[0] = S(1) / 288.0;
    b[1] = S(2) / 12;
    {
        double mean = 0.0;                                              // calc_std_dev cpp:3227
        for (int d = 0; d < 12; ++d) mean += S(3 + d);
        mean /= 12;
        double ss = 0.0;
        for (int d = 0; d < 12; ++d) ss += (S(3 + d) - mean) * (S(3 + d) - mean);
        b[3] = sqrt(ss / 11) * 100.0;
    }
    b[4] = S(15);
    b[5] = S(16);
    for (int qi = 0; qi < 4; ++qi) b[7 + qi] = S(17 + qi) / 72.0;       // cpp:3325
    b[6] = b[4] - b[5];                                                 // cpp:3533
    b[2] = b[1] / b[6];                                                 // cpp:3534
    for (int i = 0; i < 11; ++i) out[N * i] = b[i];
}

template <int CPB>
void launch_acc(const BioAccDepthsArgs& a, hipStream_t s) {
    const unsigned groups = (unsigned)((a.ntiles + SumGeom<CPB>::TPW - 1) / SumGeom<CPB>::TPW);
    hipLaunchKernelGGL((k_bioclim_acc_depths<CPB, true>), dim3(groups), dim3(kSumLanes), 0, s, a);
    hipLaunchKernelGGL((k_bioclim_acc_depths<CPB, false>), dim3(groups, (unsigned)a.ndepths), dim3(kSumLanes), 0, s, a);
}

}  // namespace

void launch_bioclim_acc_depths(const BioAccDepthsArgs& a, hipStream_t s) {
    if (a.ntiles <= 0 || a.ndepths <= 0 || a.ndays <= 0) return;
    switch (a.cpb) {
        case 16: launch_acc<16>(a, s); break;
        case 21: launch_acc<21>(a, s); break;
        case 32: launch_acc<32>(a, s); break;
        case 42: launch_acc<42>(a, s); break;
        default: break;      // (the host refuses a plan without the tiled ring)
    }
}

void launch_bioclim_fin_temp(const double* state, int64_t N, int ndepths, double* bio, hipStream_t s) {
    if (N <= 0 || ndepths <= 0) return;
    hipLaunchKernelGGL(k_bioclim_fin_temp, dim3((unsigned)((N + 255) / 256), (unsigned)ndepths), dim3(256), 0, s, state, N, bio);
}

}  // namespace mcf
