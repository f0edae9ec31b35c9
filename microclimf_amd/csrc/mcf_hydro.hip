// mcf_hydro.hip — flow accumulation and `.topidx` on the device: the values of mcf_hydro.cpp (flowaccCpp, reference
// src/microclimfCpp.cpp:5326-5408; `.topidx`, R/internal.R:861-874) without the elevation-ordered host sweep.
//
// The sweep processes cells in decreasing (elevation, row-major index) order and each processed cell adds the count it holds
// AT THAT MOMENT to its receiver.  Once every edge s -> r(s) is classified the order is no longer needed:
//   * r(s): first minimum below 9999.99 of the 3 x 3 window, the cell included, scanned column-major (flow_direction of
//     mcf_hydro.cpp); `last`, the cell with the lowest key, is never processed: it sends nothing and is not doubled;
//   * pit: r(s) == s.  Otherwise the edge is EARLY if s comes before r(s) in the order (higher, or as high with the larger
//     row-major index), else LATE (only on plateaus);
//   * P(c) = 1 + sum of P(s) over the early edges into c — a subtree count in a forest, every cell has at most one way out;
//   * fa(c) = P(c) * (2 if c is a pit else 1) + sum of P(s) over the late edges into c; NA cells hold -2147483648.
// P comes from pointer doubling over the early forest: acc = 1, jump = early receiver; one round is one launch in which every
// cell with a pointer adds its acc to the cell it points at and then points at that cell's pointer (both double-buffered).
// After round k acc holds the descendants nearer than 2^k; a flag says whether any pointer is left.  The counts are integers
// added with 64-bit integer atomics: the sum does not depend on the order of arrival, the result is bit-reproducible.
// Kernel boundaries are the only synchronisation; the host loop ends after at most ceil(log2 N) + 1 rounds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mcf.h"
#include "mcf_hydro.h"
#include "mcf_rowblocks.hpp"
#include "mcf_hiphost.hpp"

// the host code this restates is built without FMA contraction
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr double kNaInt = -2147483648.0;
constexpr u64 kNaRealBits = 0x7FF00000000007A2ULL;       // R's NA_real_
enum : uint8_t { E_NONE = 0, E_PIT = 1, E_EARLY = 2, E_LATE = 3 };

// what the order's search for `last` leaves: the lowest elevation as an unsigned key, the lowest row-major index among
// the cells that have it
struct LastCell { u64 zkey; u64 rm; };

// doubles (no NaN) -> unsigned integers in the same order; -0 and +0 share a key, as they compare equal in the host's sort
__device__ __forceinline__ u64 order_key(double z) {
    const u64 u = (u64)__double_as_longlong(z + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}

__device__ __forceinline__ u64 wave_min(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = (u64)__shfl_xor((long long)v, o);
        v = w < v ? w : v;
    }
    return v;
}

// one atomic per wave: the lowest elevation key ...
__global__ __launch_bounds__(256) void k_zmin(const double* __restrict__ z, int64_t N, LastCell* last) {
    u64 m = ~0ULL;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
        const double v = z[c];
        if (!isnan(v)) { const u64 k = order_key(v); m = k < m ? k : m; }
    }
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0 && m != ~0ULL) atomicMin(&last->zkey, m);
}
// ... and the lowest row-major index that has it
__global__ __launch_bounds__(256) void k_rmmin(const double* __restrict__ z, int64_t R, int64_t C, LastCell* last) {
    const int64_t N = R * C;
    const u64 zk = last->zkey;
    u64 m = ~0ULL;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
        const double v = z[c];
        if (!isnan(v) && order_key(v) == zk) { const u64 rm = (u64)((c % R) * C + c / R); m = rm < m ? rm : m; }
    }
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0 && m != ~0ULL) atomicMin(&last->rm, m);
}

// receiver and class of every cell's edge; the start of the doubling (acc = 1, jump = early receiver)
__global__ __launch_bounds__(256) void k_edges(const double* __restrict__ z, int64_t R, int64_t C, const LastCell* __restrict__ last,
                                               int32_t* __restrict__ recv, uint8_t* __restrict__ kind, int32_t* __restrict__ jump,
                                               u64* __restrict__ acc) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= R * C) return;
    const int64_t i = c % R, j = c / R;
    const double zs = z[c];
    int32_t r = -1;
    uint8_t k = E_NONE;
    if (!isnan(zs)) {
        double minval = 9999.99;
        int64_t by = -1, bx = -1;
        for (int jj = -1; jj <= 1; ++jj)
            for (int ii = -1; ii <= 1; ++ii) {
                const int64_t y = i + ii, x = j + jj;
                if (y < 0 || y >= R || x < 0 || x >= C) continue;
                const double v = z[y + R * x];
                if (!isnan(v) && v < minval) { minval = v; by = y; bx = x; }
            }
        const int64_t rm_s = i * C + j;
        if (by >= 0 && (u64)rm_s != last->rm) {          // `last` is never processed
            r = (int32_t)(by + R * bx);
            const int64_t rm_r = by * C + bx;
            k = rm_r == rm_s ? E_PIT : (zs > minval || (zs == minval && rm_s > rm_r)) ? E_EARLY : E_LATE;
        }
    }
    recv[c] = r;
    kind[c] = k;
    jump[c] = k == E_EARLY ? r : -1;
    acc[c] = 1;
}

// one round of the doubling; accN arrives as a copy of acc
__global__ __launch_bounds__(256) void k_double(const int32_t* __restrict__ jump, int32_t* __restrict__ jumpN,
                                                const u64* __restrict__ acc, u64* __restrict__ accN, int64_t N,
                                                int32_t* __restrict__ left) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const int32_t j = jump[v];
    int32_t jn = -1;
    if (j >= 0) {
        atomicAdd(&accN[j], acc[v]);
        jn = jump[j];
        if (jn >= 0) *left = 1;
    }
    jumpN[v] = jn;
}

__global__ __launch_bounds__(256) void k_late(const int32_t* __restrict__ recv, const uint8_t* __restrict__ kind,
                                              const u64* __restrict__ P, u64* __restrict__ late, int64_t N) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    if (kind[s] == E_LATE) atomicAdd(&late[recv[s]], P[s]);
}

__global__ __launch_bounds__(256) void k_fa(const double* __restrict__ z, const uint8_t* __restrict__ kind, const u64* __restrict__ P,
                                            const u64* __restrict__ late, double* __restrict__ fa, int64_t N) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    fa[c] = isnan(z[c]) ? kNaInt : (double)(P[c] * (kind[c] == E_PIT ? 2u : 1u) + late[c]);
}

// Horn slope in radians floored at `minslope`; NaN on the raster edge, on NA cells and beside them
__global__ __launch_bounds__(256) void k_horn(const double* __restrict__ z, int64_t R, int64_t C, double xres, double yres,
                                              double minslope, double* __restrict__ B) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= R * C) return;
    const int64_t i = c % R, j = c / R;
    double b = nan("");
    if (i > 0 && i + 1 < R && j > 0 && j + 1 < C) {
        auto zz = [&](int di, int dj) { return z[(i + di) + R * (j + dj)]; };
        const double dzdx = ((zz(-1, 1) + 2 * zz(0, 1) + zz(1, 1)) - (zz(-1, -1) + 2 * zz(0, -1) + zz(1, -1))) / (8 * xres);
        const double dzdy = ((zz(-1, -1) + 2 * zz(-1, 0) + zz(-1, 1)) - (zz(1, -1) + 2 * zz(1, 0) + zz(1, 1))) / (8 * yres);
        if (!isnan(zz(0, 0))) b = atan(sqrt(dzdx * dzdx + dzdy * dzdy));
        if (b < minslope) b = minslope;
    }
    B[c] = b;
}

// one digit of the radix select over the slopes' bit patterns (positive doubles order as unsigned integers): the histogram
// of byte `shift / 8` over the values whose higher bytes equal `prefix`
__global__ __launch_bounds__(256) void k_hist(const double* __restrict__ B, int64_t N, u64 prefix, int shift, u64* __restrict__ hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
        const double b = B[c];
        if (isnan(b)) continue;
        const u64 u = (u64)__double_as_longlong(b);
        if (shift == 56 || (u >> (shift + 8)) == prefix) atomicAdd(&h[(u >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (u64)h[threadIdx.x]);
}

// how many slopes lie below the pattern `v`, and the largest of them: out[0] count, out[1] pattern
__global__ __launch_bounds__(256) void k_below(const double* __restrict__ B, int64_t N, u64 v, u64* __restrict__ out) {
    u64 n = 0, m = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
        const double b = B[c];
        if (isnan(b)) continue;
        const u64 u = (u64)__double_as_longlong(b);
        if (u < v) { ++n; m = u > m ? u : m; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        n += (u64)__shfl_xor((long long)n, o);
        const u64 w = (u64)__shfl_xor((long long)m, o);
        m = w > m ? w : m;
    }
    if ((threadIdx.x & 63) == 0 && n) { atomicAdd(&out[0], n); atomicMax(&out[1], m); }
}

__global__ __launch_bounds__(256) void k_twi(const double* __restrict__ z, const double* __restrict__ fa, const double* __restrict__ B,
                                             double med, double xres, double yres, u64* __restrict__ twi, int64_t N) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    u64 bits = kNaRealBits;             // (a signalling pattern: stored as an integer, no arithmetic touches it)
    if (!isnan(z[c])) {
        double a = (fa[c] + 1.0) * xres * yres;
        if (a < 1.0) a = 1.0;
        const double b = isnan(B[c]) ? med : B[c];
        bits = (u64)__double_as_longlong(a / tan(b));
    }
    twi[c] = bits;
}

// NaN where the block's own dtm cell is NA (`slope[is.na(dtm)] <- NA` of the host marshaller)
__global__ __launch_bounds__(256) void k_mask_na(const double* __restrict__ dtm, int64_t rows, int64_t cols, int64_t RB, int64_t hn,
                                                 u64* __restrict__ a, u64* __restrict__ b) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= rows * cols) return;
    if (isnan(dtm[hn + cell % rows + RB * (cell / rows)])) {
        if (a) a[cell] = 0x7FF8000000000000ULL;
        if (b) b[cell] = 0x7FF8000000000000ULL;
    }
}

// svfa from a horizon array that was supplied, R/internal.R:1146-1149: the sky-view step of the horizon kernel
__global__ __launch_bounds__(256) void k_svf_from_hor(const double* __restrict__ hor, int64_t N, double* __restrict__ svf) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= N) return;
    double satan = 0.0;
    for (int d = 0; d < 24; ++d) satan += atan(hor[(int64_t)d * N + cell]);
    const double msl = tan(satan / 24.0);
    svf[cell] = 0.5 * cos(2 * msl) + 0.5;
}

inline unsigned grid_for(int64_t n) { return (unsigned)((n + 255) / 256); }
// grid-stride reductions: enough workgroups to fill the device, no more
inline unsigned grid_reduce(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 4096); }

// the device part of flowacc: d_fa from d_dtm, scratch from `db`
int flowacc_launch(const double* d_dtm, int64_t R, int64_t C, double* d_fa, mcf::DevOwner& db, int* rounds_out) {
    const int64_t N = R * C;
    if (N >= ((int64_t)1 << 31)) return mcf::api_fail(MCF_ERR_ARG, "flow accumulation on the device: at most 2^31 - 1 cells");
    int rc;
    LastCell* d_last;
    int32_t *d_recv, *d_jump[2], *d_left;
    uint8_t* d_kind;
    u64* d_acc[2];
    int max_rounds = 1;                             // ceil(log2 N) + 1: no path is longer than N - 1 edges
    while (((int64_t)1 << (max_rounds - 1)) < N) ++max_rounds;
    if ((rc = db.alloc((void**)&d_last, sizeof(LastCell)))) return rc;
    if ((rc = db.alloc((void**)&d_recv, N * 4))) return rc;
    if ((rc = db.alloc((void**)&d_kind, N))) return rc;
    if ((rc = db.alloc((void**)&d_left, max_rounds * 4))) return rc;
    for (int k = 0; k < 2; ++k) {
        if ((rc = db.alloc((void**)&d_jump[k], N * 4))) return rc;
        if ((rc = db.alloc((void**)&d_acc[k], N * 8))) return rc;
    }
    HIP_TRY(hipMemsetAsync(d_left, 0, (size_t)max_rounds * 4, nullptr));
    HIP_TRY(hipMemsetAsync(d_last, 0xFF, sizeof(LastCell), nullptr));
    hipLaunchKernelGGL(k_zmin, dim3(grid_reduce(N)), dim3(256), 0, nullptr, d_dtm, N, d_last);
    hipLaunchKernelGGL(k_rmmin, dim3(grid_reduce(N)), dim3(256), 0, nullptr, d_dtm, R, C, d_last);
    hipLaunchKernelGGL(k_edges, dim3(grid_for(N)), dim3(256), 0, nullptr, d_dtm, R, C, d_last, d_recv, d_kind, d_jump[0], d_acc[0]);
    HIP_TRY(hipGetLastError());
    int cur = 0, rounds = 0;
    for (;;) {
        if (rounds == max_rounds) return mcf::api_fail(MCF_ERR_HIP, "flow accumulation: the early edges do not form a forest");
        HIP_TRY(hipMemcpyAsync(d_acc[cur ^ 1], d_acc[cur], (size_t)N * 8, hipMemcpyDeviceToDevice, nullptr));
        hipLaunchKernelGGL(k_double, dim3(grid_for(N)), dim3(256), 0, nullptr, d_jump[cur], d_jump[cur ^ 1], d_acc[cur], d_acc[cur ^ 1],
                           N, d_left + rounds);
        HIP_TRY(hipGetLastError());
        int32_t left = 0;
        HIP_TRY(hipMemcpy(&left, d_left + rounds, 4, hipMemcpyDeviceToHost));
        cur ^= 1;
        ++rounds;
        if (!left) break;
    }
    u64 *d_P = d_acc[cur], *d_late = d_acc[cur ^ 1];
    HIP_TRY(hipMemsetAsync(d_late, 0, (size_t)N * 8, nullptr));
    hipLaunchKernelGGL(k_late, dim3(grid_for(N)), dim3(256), 0, nullptr, d_recv, d_kind, d_P, d_late, N);
    hipLaunchKernelGGL(k_fa, dim3(grid_for(N)), dim3(256), 0, nullptr, d_dtm, d_kind, d_P, d_late, d_fa, N);
    HIP_TRY(hipGetLastError());
    if (rounds_out) *rounds_out = rounds;
    return MCF_OK;
}

void report_rounds(int64_t rows, int64_t cols, int rounds) {
    if (getenv("MCF_TIMING")) fprintf(stderr, "[mcf] flowacc: %lld x %lld cells, %d doubling rounds\n", (long long)rows, (long long)cols, rounds);
}

}  // namespace

namespace mcf {

// All launches on the null stream; returns after the device has finished, its temporaries released.
int flowacc_device(const double* d_dtm, int64_t rows, int64_t cols, double* d_fa) {
    mcf::DevOwner db;
    int rounds = 0;
    if (const int rc = flowacc_launch(d_dtm, rows, cols, d_fa, db, &rounds)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    report_rounds(rows, cols, rounds);
    return MCF_OK;
}

int topidx_device(const double* d_dtm, int64_t rows, int64_t cols, double xres, double yres, double* d_twi, double* d_fa) {
    const int64_t N = rows * cols;
    int rc;
    mcf::DevOwner own_fa;
    if (!d_fa && (rc = own_fa.alloc((void**)&d_fa, N * 8))) return rc;
    {
        mcf::DevOwner db;                            // the flow accumulation's scratch goes before the slopes' is taken
        int rounds = 0;
        if ((rc = flowacc_launch(d_dtm, rows, cols, d_fa, db, &rounds))) return rc;
        HIP_TRY(hipDeviceSynchronize());
        report_rounds(rows, cols, rounds);
    }
    mcf::DevOwner db;
    double* d_B;
    u64* d_hist;                                     // [8][256] digit histograms, then [2] of k_below
    if ((rc = db.alloc((void**)&d_B, N * 8))) return rc;
    if ((rc = db.alloc((void**)&d_hist, (8 * 256 + 2) * 8))) return rc;
    HIP_TRY(hipMemsetAsync(d_hist, 0, (8 * 256 + 2) * 8, nullptr));
    const double minslope = atan(0.02 / (0.5 * (xres + yres)));
    hipLaunchKernelGGL(k_horn, dim3(grid_for(N)), dim3(256), 0, nullptr, d_dtm, rows, cols, xres, yres, minslope, d_B);
    HIP_TRY(hipGetLastError());
    // R's median of the non-NA slopes: the middle order statistic, or the mean of the two middle ones
    double med = nan("");
    u64 hist[256];
    u64 prefix = 0, k = 0, n = 0;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        u64* d_h = d_hist + 256 * pass;
        hipLaunchKernelGGL(k_hist, dim3(grid_reduce(N)), dim3(256), 0, nullptr, d_B, N, prefix, shift, d_h);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(hist, d_h, 256 * 8, hipMemcpyDeviceToHost));
        if (pass == 0) {
            for (int b = 0; b < 256; ++b) n += hist[b];
            if (n == 0) break;
            k = n / 2;
        }
        int b = 0;
        for (; b < 255 && k >= hist[b]; ++b) k -= hist[b];
        prefix = (prefix << 8) | (u64)b;
    }
    if (n > 0) {
        memcpy(&med, &prefix, 8);
        if (n % 2 == 0) {
            u64* d_out = d_hist + 8 * 256;
            hipLaunchKernelGGL(k_below, dim3(grid_reduce(N)), dim3(256), 0, nullptr, d_B, N, prefix, d_out);
            HIP_TRY(hipGetLastError());
            u64 out[2];
            HIP_TRY(hipMemcpy(out, d_out, 16, hipMemcpyDeviceToHost));
            // fewer than n / 2 slopes below the upper middle one: the lower middle one equals it
            if (out[0] == n / 2) {
                double lo;
                memcpy(&lo, &out[1], 8);
                med = 0.5 * (med + lo);
            }
        }
    }
    hipLaunchKernelGGL(k_twi, dim3(grid_for(N)), dim3(256), 0, nullptr, d_dtm, d_fa, d_B, med, xres, yres, (u64*)d_twi, N);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}

int mask_na_device(const double* d_dtm, int64_t rows, int64_t cols, int32_t halo_north, int32_t halo_south, double* d_a, double* d_b) {
    hipLaunchKernelGGL(k_mask_na, dim3(grid_for(rows * cols)), dim3(256), 0, nullptr, d_dtm, rows, cols,
                       (int64_t)halo_north + rows + halo_south, (int64_t)halo_north, (u64*)d_a, (u64*)d_b);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}

int svf_from_hor_device(const double* d_hor, int64_t N, double* d_svfa) {
    hipLaunchKernelGGL(k_svf_from_hor, dim3(grid_for(N)), dim3(256), 0, nullptr, d_hor, N, d_svfa);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}

}  // namespace mcf

// ---- C ABI: host pointers in and out ---------------------------------------------------------------------------------------
static int hydro_host(int64_t rows, int64_t cols, const double* dtm, double xres, double yres, double* res, int32_t device, bool twi) {
    if (const int rc = mcf::check_device(device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(device));
    const int64_t N = rows * cols;
    mcf::DevOwner db;
    int rc;
    double *d_dtm, *d_res;
    if ((rc = db.alloc((void**)&d_dtm, N * 8))) return rc;
    if ((rc = db.alloc((void**)&d_res, N * 8))) return rc;
    HIP_TRY(hipMemcpy(d_dtm, dtm, (size_t)N * 8, hipMemcpyHostToDevice));
    if ((rc = twi ? mcf::topidx_device(d_dtm, rows, cols, xres, yres, d_res, nullptr) : mcf::flowacc_device(d_dtm, rows, cols, d_res)))
        return rc;
    HIP_TRY(hipMemcpy(res, d_res, (size_t)N * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}

extern "C" int mcf_flowacc_device(int64_t rows, int64_t cols, const double* dtm, double* fa, int32_t device) {
    if (rows <= 0 || cols <= 0 || !dtm || !fa) return mcf::api_fail(MCF_ERR_ARG, "mcf_flowacc_device: bad dimensions or null argument");
    return hydro_host(rows, cols, dtm, 1.0, 1.0, fa, device, false);
}

extern "C" int mcf_topidx_device(int64_t rows, int64_t cols, const double* dtm, double xres, double yres, double* twi, int32_t device) {
    if (rows <= 0 || cols <= 0 || !dtm || !twi || !(xres > 0) || !(yres > 0))
        return mcf::api_fail(MCF_ERR_ARG, "mcf_topidx_device: bad dimensions, resolution or null argument");
    return hydro_host(rows, cols, dtm, xres, yres, twi, device, true);
}
