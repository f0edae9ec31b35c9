// mcf_summary.hip — period summaries of the solver's outputs, accumulated on the device from the tiled output ring
// (include/mcf.h "period summaries").  Only adds, compares and one divide: nothing here can be contracted.
//
// k_summary_acc   one workgroup = kSumLanes / cpb consecutive tiles of one selected variable.  Per day of the call the
//                 tiles' blocks ([tile][day][var][block], each block one contiguous line-aligned run) come in through
//                 registers into LDS with 16-byte loads — every 128-byte line of a selected variable is read once, whole —
//                 and one lane per cell walks its 24 places (ring_pos) in hour order, folding them into registers.  The
//                 next day's loads are in flight while the lanes fold.  The days of one period are taken together, in
//                 ascending order, so a period's state is read once and written once per call however its days lie.
// k_summary_planes  the same fold over step-major planes [step][cell] (the snow plan's chunk series): one lane
//                 per cell along the cells, one selected series per blockIdx.y; a day's 24 values are 24 independent loads,
//                 each a contiguous 512-byte run per wave, in flight together; no LDS, nothing shared between lanes.
// k_summary_fin   state -> one statistic plane [N][nperiods]: the divide, the NA rule, the count as a double.
// k_summary_init  the state before the first day: sums and counts 0, minimum +inf, maximum -inf (with the strict
//                 comparisons that is the same as starting from the period's first value).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcf.h"
#include "mcf_kernels.h"
#include "mcf_tilestage.hpp"

namespace mcf {
namespace {

constexpr unsigned long long kNaBits = 0x7FF00000000007A2ull;      // R's NA_real_

__device__ __forceinline__ double na_value() { return __longlong_as_double((long long)kNaBits); }
__device__ __forceinline__ bool is_na_bits(double x) { return (unsigned long long)__double_as_longlong(x) == kNaBits; }

template <int CPB>
__global__ __launch_bounds__(kSumLanes) void k_summary_acc(SummaryAccArgs a) {
    using G = SumGeom<CPB>;
    __shared__ double lds[G::TPW * G::S];
    const int tid = (int)threadIdx.x, k = (int)blockIdx.y;
    const int64_t tile0 = (int64_t)blockIdx.x * G::TPW;
    const int64_t left = a.ntiles - tile0;
    const int ntl = left < G::TPW ? (int)left : G::TPW;           // tiles of this group that exist in the ring
    const int tl = tid / CPB, cell = tid - tl * CPB;
    const int64_t c = tile0 * CPB + tid;
    const bool active = tid < G::TPW * CPB && c < a.N;            // cells >= N of the last tile: padding, never read into state
    int slab = 0;
    double thr = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i)                                  // (constant indices: the argument block stays in scalar registers)
        if (i == k) { slab = a.slab[i]; thr = a.threshold[i]; }
    const double* src = a.ring + (int64_t)slab * a.var_stride + tile0 * a.tile_stride;
    double* st = a.state + (int64_t)k * a.nperiods * a.nrows * a.N;
    const int end = a.day0 + a.ndays;
    const double* L = lds + tl * G::S;
    double2 r[G::NLD];

    for (int d = a.day0; d < end; ++d) {
        const int per = a.period_of_day[d];
        if (per < 0 || a.prev_same[d] >= a.day0) continue;        // not counted, or its period has been folded already
        double* sp = st + (int64_t)per * a.nrows * a.N + c;
        double s = 0.0, mn = 0.0, mx = 0.0, dxs = 0.0, dns = 0.0, cnt = 0.0;
        bool bad = false;
        if (active) {
            s = sp[0];
            bad = is_na_bits(s);
            if (a.row[MCF_STAT_MIN] >= 0) mn = sp[a.row[MCF_STAT_MIN] * a.N];
            if (a.row[MCF_STAT_MAX] >= 0) mx = sp[a.row[MCF_STAT_MAX] * a.N];
            if (a.row[MCF_STAT_MEAN_DAILY_MAX] >= 0) dxs = sp[a.row[MCF_STAT_MEAN_DAILY_MAX] * a.N];
            if (a.row[MCF_STAT_MEAN_DAILY_MIN] >= 0) dns = sp[a.row[MCF_STAT_MEAN_DAILY_MIN] * a.N];
            if (a.row[MCF_STAT_HOURS_ABOVE] >= 0) cnt = sp[a.row[MCF_STAT_HOURS_ABOVE] * a.N];
        }
        load_day<CPB>(r, src + (int64_t)(a.slot_day0 + d - a.day0) * a.day_stride, a.tile_stride, tid, ntl);
        for (int e = d;;) {
            __syncthreads();                                      // the day before has left the LDS
            store_day<CPB>(lds, r, tid, ntl);
            __syncthreads();
            const int nx = a.next_same[e];                        // the period's next day (>= the series' days: none)
            if (nx < end) load_day<CPB>(r, src + (int64_t)(a.slot_day0 + nx - a.day0) * a.day_stride, a.tile_stride, tid, ntl);
            if (active) {
                double dmx = 0.0, dmn = 0.0;
#pragma unroll
                for (int h = 0; h < 24; ++h) {
                    const double v = L[ring_pos(CPB, cell, h)];
                    bad |= v != v;
                    s = s + v;
                    if (v < mn) mn = v;
                    if (v > mx) mx = v;
                    if (h == 0) { dmx = v; dmn = v; }
                    else {
                        if (v > dmx) dmx = v;
                        if (v < dmn) dmn = v;
                    }
                    if (v > thr) cnt = cnt + 1.0;
                }
                dxs = dxs + dmx;
                dns = dns + dmn;
            }
            if (nx >= end) break;
            e = nx;
        }
        if (active) {
            sp[0] = bad ? na_value() : s;                         // the sum row carries the NA rule between calls
            if (a.row[MCF_STAT_MIN] >= 0) sp[a.row[MCF_STAT_MIN] * a.N] = mn;
            if (a.row[MCF_STAT_MAX] >= 0) sp[a.row[MCF_STAT_MAX] * a.N] = mx;
            if (a.row[MCF_STAT_MEAN_DAILY_MAX] >= 0) sp[a.row[MCF_STAT_MEAN_DAILY_MAX] * a.N] = dxs;
            if (a.row[MCF_STAT_MEAN_DAILY_MIN] >= 0) sp[a.row[MCF_STAT_MEAN_DAILY_MIN] * a.N] = dns;
            if (a.row[MCF_STAT_HOURS_ABOVE] >= 0) sp[a.row[MCF_STAT_HOURS_ABOVE] * a.N] = cnt;
        }
    }
}

__global__ __launch_bounds__(kSumLanes) void k_summary_planes(SummaryPlanesArgs a) {
    const int k = (int)blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * kSumLanes + threadIdx.x;
    if (c >= a.N) return;                                         // (no barrier below: the last group's spare lanes leave)
    const double* src = nullptr;
    double thr = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i)                                   // (constant indices: the argument block stays in scalar registers)
        if (i == k) { src = a.series[i]; thr = a.threshold[i]; }
    src += c;
    double* st = a.state + (int64_t)k * a.nperiods * a.nrows * a.N;
    const int end = a.day0 + a.ndays;

    for (int d = a.day0; d < end; ++d) {
        const int per = a.period_of_day[d];
        if (per < 0 || a.prev_same[d] >= a.day0) continue;        // not counted, or its period has been folded already
        double* sp = st + (int64_t)per * a.nrows * a.N + c;
        double s = sp[0], mn = 0.0, mx = 0.0, dxs = 0.0, dns = 0.0, cnt = 0.0;
        bool bad = is_na_bits(s);
        if (a.row[MCF_STAT_MIN] >= 0) mn = sp[a.row[MCF_STAT_MIN] * a.N];
        if (a.row[MCF_STAT_MAX] >= 0) mx = sp[a.row[MCF_STAT_MAX] * a.N];
        if (a.row[MCF_STAT_MEAN_DAILY_MAX] >= 0) dxs = sp[a.row[MCF_STAT_MEAN_DAILY_MAX] * a.N];
        if (a.row[MCF_STAT_MEAN_DAILY_MIN] >= 0) dns = sp[a.row[MCF_STAT_MEAN_DAILY_MIN] * a.N];
        if (a.row[MCF_STAT_HOURS_ABOVE] >= 0) cnt = sp[a.row[MCF_STAT_HOURS_ABOVE] * a.N];
        for (int e = d; e < end; e = a.next_same[e]) {            // the period's days inside the call, ascending
            const double* day = src + (int64_t)(e - a.day0) * 24 * a.N;
            double v[24];
#pragma unroll
            for (int h = 0; h < 24; ++h) v[h] = day[(int64_t)h * a.N];
            double dmx = v[0], dmn = v[0];
#pragma unroll
            for (int h = 0; h < 24; ++h) {
                bad |= v[h] != v[h];
                s = s + v[h];
                if (v[h] < mn) mn = v[h];
                if (v[h] > mx) mx = v[h];
                if (h > 0) {
                    if (v[h] > dmx) dmx = v[h];
                    if (v[h] < dmn) dmn = v[h];
                }
                if (v[h] > thr) cnt = cnt + 1.0;
            }
            dxs = dxs + dmx;
            dns = dns + dmn;
        }
        sp[0] = bad ? na_value() : s;                             // the sum row carries the NA rule between calls
        if (a.row[MCF_STAT_MIN] >= 0) sp[a.row[MCF_STAT_MIN] * a.N] = mn;
        if (a.row[MCF_STAT_MAX] >= 0) sp[a.row[MCF_STAT_MAX] * a.N] = mx;
        if (a.row[MCF_STAT_MEAN_DAILY_MAX] >= 0) sp[a.row[MCF_STAT_MEAN_DAILY_MAX] * a.N] = dxs;
        if (a.row[MCF_STAT_MEAN_DAILY_MIN] >= 0) sp[a.row[MCF_STAT_MEAN_DAILY_MIN] * a.N] = dns;
        if (a.row[MCF_STAT_HOURS_ABOVE] >= 0) sp[a.row[MCF_STAT_HOURS_ABOVE] * a.N] = cnt;
    }
}

__global__ __launch_bounds__(256) void k_summary_fin(SummaryFinArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N * a.nperiods) return;
    const int64_t per = i / a.N, c = i - per * a.N;
    const double* sp = a.state + per * a.nrows * a.N + c;
    const double s = sp[0];
    const int nd = a.days[per];
    double v = na_value();
    if (nd > 0 && !is_na_bits(s)) {
        const double x = a.row > 0 ? sp[a.row * a.N] : s;
        if (a.stat == MCF_STAT_MEAN) v = s / (24.0 * (double)nd);
        else if (a.stat == MCF_STAT_MEAN_DAILY_MAX || a.stat == MCF_STAT_MEAN_DAILY_MIN) v = x / (double)nd;
        else v = x;
    }
    a.out[i] = v;
}

// init_codes: 4 bits per state row — 0: 0.0, 1: +inf, 2: -inf
__global__ __launch_bounds__(256) void k_summary_init(double* state, int64_t total, int64_t N, int nrows, uint32_t init_codes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t code = (init_codes >> (4 * (uint32_t)((i / N) % nrows))) & 15u;
    state[i] = code == 1 ? __longlong_as_double(0x7FF0000000000000ll) : code == 2 ? __longlong_as_double((long long)0xFFF0000000000000ull) : 0.0;
}

template <int CPB>
void launch_acc(const SummaryAccArgs& a, hipStream_t s) {
    const int64_t groups = (a.ntiles + SumGeom<CPB>::TPW - 1) / SumGeom<CPB>::TPW;
    hipLaunchKernelGGL(k_summary_acc<CPB>, dim3((unsigned)groups, (unsigned)a.nsel), dim3(kSumLanes), 0, s, a);
}

}  // namespace

int summary_tiles_per_group(int cpb) { return cpb > 0 ? kSumLanes / cpb : 0; }

void launch_summary_acc(const SummaryAccArgs& a, hipStream_t s) {
    if (a.ntiles <= 0 || a.nsel <= 0 || a.ndays <= 0) return;
    switch (a.cpb) {
        case 16: launch_acc<16>(a, s); break;
        case 21: launch_acc<21>(a, s); break;
        case 32: launch_acc<32>(a, s); break;
        case 42: launch_acc<42>(a, s); break;
        default: break;      // (the linear ring is refused by the host)
    }
}

void launch_summary_planes(const SummaryPlanesArgs& a, hipStream_t s) {
    if (a.N <= 0 || a.nsel <= 0 || a.ndays <= 0) return;
    hipLaunchKernelGGL(k_summary_planes, dim3((unsigned)((a.N + kSumLanes - 1) / kSumLanes), (unsigned)a.nsel), dim3(kSumLanes), 0, s, a);
}

void launch_summary_fin(const SummaryFinArgs& a, hipStream_t s) {
    const int64_t n = a.N * a.nperiods;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_summary_fin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

void launch_summary_init(double* state, int64_t total, int64_t N, int nrows, uint32_t init_codes, hipStream_t s) {
    if (total <= 0) return;
    hipLaunchKernelGGL(k_summary_init, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, state, total, N, nrows, init_codes);
}

}  // namespace mcf
