// mcf_series.hip — the series sink (include/mcf.h "series sink"): per-step statistics of the solver's outputs
// over zones of the raster, and the full series at a few cells, from the tiled output ring.  Integer adds, compares, one
// multiply by a power of two, one rint and one divide: nothing here can be contracted, and nothing depends on the order in
// which workgroups arrive.
//
// k_series_zones  a few hundred persistent workgroups per selected variable.  Per day of the call a workgroup walks its tile
//                 groups (kSumLanes / cpb consecutive tiles, as k_summary_acc takes them: blocks through registers into LDS with
//                 16-byte loads, every 128-byte line read once, one lane per cell, the next group's loads in flight while the
//                 lanes fold) and reduces each hour across cells by zone label into an LDS table [row][zone][hour] of int64:
//                   - a wave whose lanes all carry one label (the common case for coherent zones; one ballot per group) is
//                     reduced across the wave first — counts by ballot, sum / minimum / maximum by a butterfly — and lanes
//                     0..23 add the 24 hours' results to the table, one LDS atomic each;
//                   - any other wave adds lane by lane with LDS integer atomics.
//                 After the day's last group the table's touched entries go to the state in global memory with integer
//                 atomics (add, signed min, signed max): per zone the day's 24 hours are one contiguous 192-byte run.
//                 No floating-point atomic anywhere; minimum and maximum travel as order-preserving int64 keys.
// k_series_fin    state -> one statistic [nsteps][zone]: the divide, the NA rules, the count as a double.
// k_series_init   the state before the first day: sums and counts 0, minimum key INT64_MAX, maximum key INT64_MIN.
// k_series_points the points' values of the chunk's days into the resident [var][point][step] buffer (k_gather_cells'
//                 addressing, a point's steps contiguous).
// k_series_planes / k_series_points_planes  the same two over step-major planes [step][cell] (the snow plan's chunk series, a
//                 host array as it lies: DESIGN.md §28), described where they stand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcf.h"
#include "mcf_kernels.h"
#include "mcf_tilestage.hpp"

namespace mcf {
namespace {

constexpr unsigned long long kNaBits = 0x7FF00000000007A2ull;      // R's NA_real_
constexpr long long kKeyMax = 0x7FFFFFFFFFFFFFFFll, kKeyMin = -kKeyMax - 1;
constexpr int kTab = MCF_MAX_ZONES * 24;                           // entries per row of the LDS table
constexpr unsigned long long kOneBad = 1ull << 32;

__device__ __forceinline__ double na_value() { return __longlong_as_double((long long)kNaBits); }
// fp64 bits <-> a signed key with the order of the values (-0.0 just below +0.0)
__device__ __forceinline__ long long key_of(double v) {
    const long long b = __double_as_longlong(v);
    return b >= 0 ? b : b ^ kKeyMax;
}
__device__ __forceinline__ double value_of(long long k) { return __longlong_as_double(k >= 0 ? k : k ^ kKeyMax); }

#define LDS_ADD(p, x) __hip_atomic_fetch_add((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LDS_MIN(p, x) __hip_atomic_fetch_min((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LDS_MAX(p, x) __hip_atomic_fetch_max((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define DEV_ADD(p, x) __hip_atomic_fetch_add((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define DEV_MIN(p, x) __hip_atomic_fetch_min((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define DEV_MAX(p, x) __hip_atomic_fetch_max((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// butterflies over the wave's 64 lanes: every lane ends with the result
__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}
__device__ __forceinline__ long long wave_min(long long x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const long long y = __shfl_xor(x, m, 64); x = y < x ? y : x; }
    return x;
}
__device__ __forceinline__ long long wave_max(long long x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const long long y = __shfl_xor(x, m, 64); x = y > x ? y : x; }
    return x;
}

template <int CPB>
__global__ __launch_bounds__(kSumLanes) void k_series_zones(SeriesZonesArgs a) {
    using G = SumGeom<CPB>;
    __shared__ double lds[G::TPW * G::S];
    __shared__ long long tab[kSeriesRows][kTab];
    static_assert(sizeof(double) * G::TPW * G::S + sizeof(long long) * kSeriesRows * kTab <= 160 * 1024, "the staged day and the table fit the LDS");
    const int tid = (int)threadIdx.x, lane = tid & 63, k = (int)blockIdx.y;
    const bool lane_has_cell = tid < G::TPW * CPB;
    const int tl = lane_has_cell ? tid / CPB : 0, cell = lane_has_cell ? tid - tl * CPB : 0;     // (spare lanes read inside the LDS)
    int slab = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i)                                  // (constant indices: the argument block stays in scalar registers)
        if (i == k) slab = a.slab[i];
    const double* src = a.ring + (int64_t)slab * a.var_stride;
    long long* st = a.state + (int64_t)k * kSeriesRows * a.nzones * a.steps;
    const int64_t groups = (a.ntiles + G::TPW - 1) / G::TPW;
    const int nmine = (int)((groups - (int64_t)blockIdx.x + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x);   // this workgroup's groups per day
    const int nent = a.nzones * 24;
    const double* L = lds + tl * G::S;
    double2 r[G::NLD];

    for (int e = tid; e < nent; e += kSumLanes) {
        tab[kSeriesSum][e] = 0; tab[kSeriesCount][e] = 0; tab[kSeriesMin][e] = kKeyMax; tab[kSeriesMax][e] = kKeyMin;
    }
    if (nmine <= 0) return;
    // item = (day of the call, group of this workgroup), day-major: the loads of the next item are in flight while this one folds
    auto item_load = [&](int d, int j) {
        const int64_t tile0 = ((int64_t)blockIdx.x + (int64_t)j * gridDim.x) * G::TPW;
        const int64_t left = a.ntiles - tile0;
        load_day<CPB>(r, src + tile0 * a.tile_stride + (int64_t)(a.slot_day0 + d) * a.day_stride, a.tile_stride, tid,
                      left < G::TPW ? (int)left : G::TPW);
    };
    item_load(0, 0);
    for (int d = 0; d < a.ndays; ++d) {
        for (int j = 0; j < nmine; ++j) {
            const int64_t tile0 = ((int64_t)blockIdx.x + (int64_t)j * gridDim.x) * G::TPW;
            const int64_t left = a.ntiles - tile0;
            const int ntl = left < G::TPW ? (int)left : G::TPW;
            const int64_t c = tile0 * CPB + tid;
            __syncthreads();                                      // the group before has left the LDS; the table is ready
            store_day<CPB>(lds, r, tid, ntl);
            __syncthreads();
            if (j + 1 < nmine) item_load(d, j + 1);
            else if (d + 1 < a.ndays) item_load(d + 1, 0);
            int z = -1;
            if (lane_has_cell && c < a.N) z = a.zone[c];           // cells >= N of the last tile: padding, in no zone
            if (z >= a.nzones) z = -1;                            // (the host has checked the labels)
            const unsigned long long in_zone = __ballot(z >= 0);
            if (in_zone == 0) continue;                           // (wave-uniform: no barrier below before the next item's)
            const int z0 = __shfl(z, __ffsll((long long)in_zone) - 1, 64);
            if (__ballot(z >= 0 && z != z0) == 0) {
                // one label in the wave: counts by ballot, the rest by butterflies; lane h keeps hour h's results
                long long rs = 0, rmn = kKeyMax, rmx = kKeyMin;
                unsigned long long rcb = 0;
#pragma unroll
                for (int h = 0; h < 24; ++h) {
                    const double v = L[ring_pos(CPB, cell, h)];
                    const bool seen = z >= 0 && v == v, ok = seen && fabs(v) < 4096.0;
                    const unsigned long long cb = (unsigned long long)__popcll(__ballot(ok)) |
                                                  ((unsigned long long)__popcll(__ballot(seen && !ok)) << 32);
                    if (cb == 0) continue;                        // (wave-uniform)
                    const long long ky = key_of(v);
                    const long long s = wave_sum(ok ? (long long)rint(v * 16777216.0) : 0ll);
                    const long long mn = wave_min(ok ? ky : kKeyMax), mx = wave_max(ok ? ky : kKeyMin);
                    if (lane == h) { rs = s; rmn = mn; rmx = mx; rcb = cb; }
                }
                if (lane < 24 && rcb != 0) {
                    const int e = z0 * 24 + lane;
                    LDS_ADD(&tab[kSeriesCount][e], (long long)rcb);
                    if ((uint32_t)rcb != 0) {
                        LDS_ADD(&tab[kSeriesSum][e], rs);
                        LDS_MIN(&tab[kSeriesMin][e], rmn);
                        LDS_MAX(&tab[kSeriesMax][e], rmx);
                    }
                }
            } else if (z >= 0) {
#pragma unroll
                for (int h = 0; h < 24; ++h) {
                    const double v = L[ring_pos(CPB, cell, h)];
                    if (v != v) continue;
                    const int e = z * 24 + h;
                    if (fabs(v) < 4096.0) {
                        const long long ky = key_of(v);
                        LDS_ADD(&tab[kSeriesCount][e], 1ll);
                        LDS_ADD(&tab[kSeriesSum][e], (long long)rint(v * 16777216.0));
                        LDS_MIN(&tab[kSeriesMin][e], ky);
                        LDS_MAX(&tab[kSeriesMax][e], ky);
                    } else {
                        LDS_ADD(&tab[kSeriesCount][e], (long long)kOneBad);
                    }
                }
            }
        }
        // the day's table to the state, touched entries only, and back to its start
        __syncthreads();
        long long* sd = st + (int64_t)(a.day0 + d) * 24;
        for (int e = tid; e < nent; e += kSumLanes) {
            const long long cb = tab[kSeriesCount][e];
            if (cb == 0) continue;
            const int zz = e / 24, h = e - zz * 24;
            long long* g = sd + (int64_t)zz * a.steps + h;
            const int64_t row = (int64_t)a.nzones * a.steps;
            DEV_ADD(g + kSeriesCount * row, cb);
            tab[kSeriesCount][e] = 0;
            if ((uint32_t)cb != 0) {
                DEV_ADD(g + kSeriesSum * row, tab[kSeriesSum][e]);
                DEV_MIN(g + kSeriesMin * row, tab[kSeriesMin][e]);
                DEV_MAX(g + kSeriesMax * row, tab[kSeriesMax][e]);
                tab[kSeriesSum][e] = 0; tab[kSeriesMin][e] = kKeyMax; tab[kSeriesMax][e] = kKeyMin;
            }
        }
    }
}

// ---- the same fold over step-major planes ---------------------------------------------------------------------
// fold_hours / flush_day are k_series_zones' per-item body and its flush, word for word, as functions.  k_series_zones keeps its
// own copy: calling these from it costs its 21-cell instantiation one more VGPR (228 against 227), and that kernel stays as
// it was measured.
// One item's 24 hours into the LDS table; z: the lane's label (-1: in no zone), value(h): its value at hour h.
template <class V>
__device__ __forceinline__ void fold_hours(long long (*tab)[kTab], int z, int lane, V value) {
    const unsigned long long in_zone = __ballot(z >= 0);
    if (in_zone == 0) return;                                     // (wave-uniform)
    const int z0 = __shfl(z, __ffsll((long long)in_zone) - 1, 64);
    if (__ballot(z >= 0 && z != z0) == 0) {
        // one label in the wave: counts by ballot, the rest by butterflies; lane h keeps hour h's results
        long long rs = 0, rmn = kKeyMax, rmx = kKeyMin;
        unsigned long long rcb = 0;
#pragma unroll
        for (int h = 0; h < 24; ++h) {
            const double v = value(h);
            const bool seen = z >= 0 && v == v, ok = seen && fabs(v) < 4096.0;
            const unsigned long long cb = (unsigned long long)__popcll(__ballot(ok)) |
                                          ((unsigned long long)__popcll(__ballot(seen && !ok)) << 32);
            if (cb == 0) continue;                                // (wave-uniform)
            const long long ky = key_of(v);
            const long long s = wave_sum(ok ? (long long)rint(v * 16777216.0) : 0ll);
            const long long mn = wave_min(ok ? ky : kKeyMax), mx = wave_max(ok ? ky : kKeyMin);
            if (lane == h) { rs = s; rmn = mn; rmx = mx; rcb = cb; }
        }
        if (lane < 24 && rcb != 0) {
            const int e = z0 * 24 + lane;
            LDS_ADD(&tab[kSeriesCount][e], (long long)rcb);
            if ((uint32_t)rcb != 0) {
                LDS_ADD(&tab[kSeriesSum][e], rs);
                LDS_MIN(&tab[kSeriesMin][e], rmn);
                LDS_MAX(&tab[kSeriesMax][e], rmx);
            }
        }
    } else if (z >= 0) {
#pragma unroll
        for (int h = 0; h < 24; ++h) {
            const double v = value(h);
            if (v != v) continue;
            const int e = z * 24 + h;
            if (fabs(v) < 4096.0) {
                const long long ky = key_of(v);
                LDS_ADD(&tab[kSeriesCount][e], 1ll);
                LDS_ADD(&tab[kSeriesSum][e], (long long)rint(v * 16777216.0));
                LDS_MIN(&tab[kSeriesMin][e], ky);
                LDS_MAX(&tab[kSeriesMax][e], ky);
            } else {
                LDS_ADD(&tab[kSeriesCount][e], (long long)kOneBad);
            }
        }
    }
}
// The day's table to the state (sd: the state's entry of zone 0 at hour 0 of the day), touched entries only, and back to its
// start.  The barriers are the caller's: one before (the day's folds are in), one behind (before the next day's folds).
__device__ __forceinline__ void flush_day(long long (*tab)[kTab], int tid, int nzones, int64_t steps, long long* sd) {
    const int nent = nzones * 24;
    const int64_t row = (int64_t)nzones * steps;
    for (int e = tid; e < nent; e += kSumLanes) {
        const long long cb = tab[kSeriesCount][e];
        if (cb == 0) continue;
        const int zz = e / 24, h = e - zz * 24;
        long long* g = sd + (int64_t)zz * steps + h;
        DEV_ADD(g + kSeriesCount * row, cb);
        tab[kSeriesCount][e] = 0;
        if ((uint32_t)cb != 0) {
            DEV_ADD(g + kSeriesSum * row, tab[kSeriesSum][e]);
            DEV_MIN(g + kSeriesMin * row, tab[kSeriesMin][e]);
            DEV_MAX(g + kSeriesMax * row, tab[kSeriesMax][e]);
            tab[kSeriesSum][e] = 0; tab[kSeriesMin][e] = kKeyMax; tab[kSeriesMax][e] = kKeyMin;
        }
    }
}

// k_series_planes  the value of (step k of the call, cell c) at series[i][k * N + c], step 0 = hour 0 of state day day0.
//                  Persistent workgroups of kSumLanes lanes per selected series; each walks every gridDim.x-th span of kSumLanes
//                  consecutive cells, one lane per cell.  Per (day, span) a lane reads its label once and issues the day's 24
//                  loads together (per hour one contiguous 512-byte run per wave: no LDS staging), then folds as above.  A last
//                  day with fewer than 24 steps loads the steps that exist; the rest count as NaN.
__global__ __launch_bounds__(kSumLanes) void k_series_planes(SeriesPlanesArgs a) {
    __shared__ long long tab[kSeriesRows][kTab];
    static_assert(sizeof(long long) * kSeriesRows * kTab <= 160 * 1024, "the table fits the LDS");
    const int tid = (int)threadIdx.x, lane = tid & 63, k = (int)blockIdx.y;
    const double* src = a.series[0];
#pragma unroll
    for (int i = 1; i < 5; ++i)                                   // (constant indices: the argument block stays in scalar registers)
        if (i == k) src = a.series[i];
    long long* st = a.state + (int64_t)k * kSeriesRows * a.nzones * a.steps;
    const int64_t spans = (a.N + kSumLanes - 1) / kSumLanes;
    const int nmine = (int)((spans - (int64_t)blockIdx.x + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x);   // this workgroup's spans per day
    if (nmine <= 0) return;                                       // (the whole workgroup: no barrier has been met)
    for (int e = tid; e < a.nzones * 24; e += kSumLanes) {
        tab[kSeriesSum][e] = 0; tab[kSeriesCount][e] = 0; tab[kSeriesMin][e] = kKeyMax; tab[kSeriesMax][e] = kKeyMin;
    }
    __syncthreads();
    for (int d = 0; d < a.ndays; ++d) {
        const int64_t left = a.nsteps - (int64_t)d * 24;
        const int nh = left < 24 ? (int)left : 24;                // steps of this day that exist
        const double* day = src + (int64_t)d * 24 * a.N;          // (64-bit: k * N + c passes 2^31 at 1024^2 cells x 2048 steps)
        for (int j = 0; j < nmine; ++j) {
            const int64_t c = ((int64_t)blockIdx.x + (int64_t)j * gridDim.x) * kSumLanes + tid;
            const bool in = c < a.N;
            int z = -1;
            if (in) z = a.zone[c];
            if (z >= a.nzones) z = -1;                            // (the host has checked the labels)
            double v[24];
#pragma unroll
            for (int h = 0; h < 24; ++h) v[h] = in && h < nh ? day[(int64_t)h * a.N + c] : __builtin_nan("");
            fold_hours(tab, z, lane, [&](int h) { return v[h]; });
        }
        __syncthreads();
        flush_day(tab, tid, a.nzones, a.steps, st + (int64_t)(a.day0 + d) * 24);
        __syncthreads();
    }
}

// dst[(i * ncells + ci) * dst_steps + dst_step0 + k] = series[i][k * N + cells[ci]], k < nsteps
__global__ __launch_bounds__(256) void k_series_points_planes(SeriesPointsPlanesArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.ncells * a.nsteps) return;
    const int k = (int)blockIdx.y;
    const double* src = a.series[0];
#pragma unroll
    for (int j = 1; j < 5; ++j)
        if (j == k) src = a.series[j];
    const int64_t ci = i / a.nsteps, kk = i - ci * a.nsteps;
    a.dst[((int64_t)k * a.ncells + ci) * a.dst_steps + a.dst_step0 + kk] = src[kk * a.N + a.cells[ci]];
}

__global__ __launch_bounds__(256) void k_series_init(long long* state, int64_t total, int64_t row_elems) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int row = (int)((i / row_elems) % kSeriesRows);
    state[i] = row == kSeriesMin ? kKeyMax : row == kSeriesMax ? kKeyMin : 0;
}

__global__ __launch_bounds__(256) void k_series_fin(const long long* __restrict__ state, int nzones, int64_t steps, int64_t nsteps,
                                                    const int32_t* __restrict__ day_done, int zstat, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nsteps * nzones) return;
    const int64_t z = i / nsteps, kk = i - z * nsteps;
    double v = na_value();
    if (kk < steps && (!day_done || day_done[kk / 24])) {
        const int64_t row = (int64_t)nzones * steps, at = z * steps + kk;
        const unsigned long long cb = (unsigned long long)state[kSeriesCount * row + at];
        const uint32_t n = (uint32_t)cb, bad = (uint32_t)(cb >> 32);
        if (zstat == MCF_ZSTAT_COUNT) v = (double)n;
        else if (n > 0 && bad == 0) {
            if (zstat == MCF_ZSTAT_MEAN) v = ((double)state[kSeriesSum * row + at] * 0x1p-24) / (double)n;
            else v = value_of(state[(zstat == MCF_ZSTAT_MIN ? kSeriesMin : kSeriesMax) * row + at]) + 0.0;
        }
    }
    out[i] = v;
}

__global__ __launch_bounds__(256) void k_series_points(SeriesPointsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.ncells * a.nsteps) return;
    const int k = (int)blockIdx.y;
    const int64_t ci = i / a.nsteps, kk = i - ci * a.nsteps;
    RingView v = a.src[0];
#pragma unroll
    for (int j = 1; j < 10; ++j)                                  // (constant indices: the argument block stays in scalar registers)
        if (j == k) v = a.src[j];
    a.dst[((int64_t)k * a.ncells + ci) * a.dst_steps + a.dst_step0 + kk] = v.at(a.cells[ci], a.step0 + kk);
}

template <int CPB>
void launch_zones(const SeriesZonesArgs& a, int workgroups, hipStream_t s) {
    const int64_t groups = (a.ntiles + SumGeom<CPB>::TPW - 1) / SumGeom<CPB>::TPW;
    const int64_t wg = groups < workgroups ? groups : workgroups;
    hipLaunchKernelGGL(k_series_zones<CPB>, dim3((unsigned)wg, (unsigned)a.nsel), dim3(kSumLanes), 0, s, a);
}

}  // namespace

void launch_series_zones(const SeriesZonesArgs& a, int workgroups, hipStream_t s) {
    if (a.ntiles <= 0 || a.nsel <= 0 || a.ndays <= 0 || a.nzones <= 0 || workgroups <= 0) return;
    switch (a.cpb) {
        case 16: launch_zones<16>(a, workgroups, s); break;
        case 21: launch_zones<21>(a, workgroups, s); break;
        case 32: launch_zones<32>(a, workgroups, s); break;
        case 42: launch_zones<42>(a, workgroups, s); break;
        default: break;      // (the linear ring is refused by the host)
    }
}

void launch_series_planes(const SeriesPlanesArgs& a, int workgroups, hipStream_t s) {
    if (a.N <= 0 || a.nsel <= 0 || a.ndays <= 0 || a.nsteps <= 0 || a.nzones <= 0 || workgroups <= 0) return;
    const int64_t spans = (a.N + kSumLanes - 1) / kSumLanes;
    const int64_t wg = spans < workgroups ? spans : workgroups;
    hipLaunchKernelGGL(k_series_planes, dim3((unsigned)wg, (unsigned)a.nsel), dim3(kSumLanes), 0, s, a);
}

void launch_series_points_planes(const SeriesPointsPlanesArgs& a, hipStream_t s) {
    const int64_t n = a.ncells * a.nsteps;
    if (n <= 0 || a.nsel <= 0) return;
    hipLaunchKernelGGL(k_series_points_planes, dim3((unsigned)((n + 255) / 256), (unsigned)a.nsel), dim3(256), 0, s, a);
}

void launch_series_init(long long* state, int64_t nsel, int64_t nzones, int64_t steps, hipStream_t s) {
    const int64_t total = nsel * kSeriesRows * nzones * steps;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_series_init, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, state, total, nzones * steps);
}

void launch_series_fin(const long long* state, int nzones, int64_t steps, int64_t nsteps, const int32_t* day_done, int zstat,
                       double* out, hipStream_t s) {
    const int64_t n = nsteps * nzones;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_series_fin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, state, nzones, steps, nsteps, day_done, zstat, out);
}

void launch_series_points(const SeriesPointsArgs& a, hipStream_t s) {
    const int64_t n = a.ncells * a.nsteps;
    if (n <= 0 || a.nsel <= 0) return;
    hipLaunchKernelGGL(k_series_points, dim3((unsigned)((n + 255) / 256), (unsigned)a.nsel), dim3(256), 0, s, a);
}

}  // namespace mcf
