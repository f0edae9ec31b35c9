// mcf_vegprep.hip — leaf and ground reflectance from albedo on the device: the values of mcf_vegprep.cpp (find_lref / find_gref,
// reference src/microclimfCpp.cpp:5675-5724; fill_naCpp, :5727-5777; the loop of leafrfromalb(), R/dataprep.R:1007-1049).
//
// Per-cell solve: one lane per cell, the bisections of mcf_vegprep.h.
//
// Nearest fill: fill_naCpp is a multi-source breadth-first search whose FIFO order decides ties.  Sources enter the queue in
// column-major order and a cell tries its neighbours as row - 1, row + 1, col - 1, col + 1, so a cell at distance d is taken
// by whichever of its neighbours at distance d - 1 was queued first, and its own place in the queue is (that neighbour's
// place, the neighbour's direction number k).  Level-synchronous restatement:
//   * a level is a list `fr` of cells in queue order; a cell's rank is its index in the list;
//   * k_claim: every (rank i, direction k) whose neighbour is inside the raster, inside the mask and still NA offers the key
//     base + 4 i + k to that neighbour with a 64-bit atomicMin: the lowest key is the first arrival of the FIFO;
//   * the offers that won are compacted IN KEY ORDER into the next list (count per workgroup, one workgroup scans the counts,
//     every workgroup scans its own 4 x 256 offers and writes): the winners' values move to the cells they took, and the
//     index in the new list is the new rank.  Ranks are renumbered every level, they never grow with depth;
//   * `base` grows by 4 x (list length) per level, so a key left behind by an earlier level never equals a current one;
//   * the host loops over the levels and reads one count per level: the next list's length, 0 = done.
// The lists hold what the queue holds, in its order, so the result is the reference's bit for bit.  Work per level is
// proportional to the level, not to the raster.
//
// Reductions: mean(pai) and the two mean absolute differences of a pass, kRedParts workgroups over fixed strided subsets with
// a fixed LDS tree, one lane adds the parts in order: the order of additions does not depend on the raster or the launch.
//
// Fused loop: pai, x, alb, lref, gref, lref2, gref2 stay in device memory through all passes; per pass the host reads the two
// means and the fills' level counts.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mcf.h"
#include "mcf_vegprep.h"
#include "mcf_rowblocks.hpp"
#include "mcf_hiphost.hpp"

// the host code this restates is built without FMA contraction
#pragma clang fp contract(off)

namespace mcf {
void vegprep_host_residual(int64_t n, const double* lref, const double* pai, const double* gref, const double* x, const double* albin,
                           double ltrr, double* out);   // mcf_vegprep.cpp
}

namespace {

namespace vp = mcf::vegprep;
typedef unsigned long long u64;


// ---- per-cell solve ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_find_lref(const double* __restrict__ pai, const double* __restrict__ gref,
                                                   const double* __restrict__ x, const double* __restrict__ alb, double ltrr, int64_t N,
                                                   u64* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    out[c] = vp::cell_lref(pai[c], gref[c], x[c], alb[c], ltrr);
}

__global__ __launch_bounds__(256) void k_find_gref(const double* __restrict__ lref, const double* __restrict__ pai,
                                                   const double* __restrict__ x, const double* __restrict__ alb, double ltrr, int64_t N,
                                                   u64* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    out[c] = vp::cell_gref(lref[c], pai[c], x[c], alb[c], ltrr);
}

__global__ __launch_bounds__(256) void k_residual(const double* __restrict__ lref, const double* __restrict__ pai,
                                                  const double* __restrict__ gref, const double* __restrict__ x,
                                                  const double* __restrict__ alb, double ltrr, int64_t N, double* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    out[c] = vp::leafr_residual(lref[c], pai[c], gref[c], x[c], alb[c], ltrr);
}

// ---- nearest fill -------------------------------------------------------------------------------------------------------------
// the neighbour of `cell` in direction k (row - 1, row + 1, col - 1, col + 1; cpp:5750-5751), -1 outside the raster
__device__ __forceinline__ int64_t neighbour(int64_t cell, int k, int64_t R, int64_t C) {
    const int64_t r = cell % R, c = cell / R;
    const int64_t rr = r + (k == 0 ? -1 : k == 1 ? 1 : 0), cc = c + (k == 2 ? -1 : k == 3 ? 1 : 0);
    if (rr < 0 || rr >= R || cc < 0 || cc >= C) return -1;
    return rr + R * cc;
}

// What an entry of a compaction contributes, in order.  Level 0: entry = cell, one flag (the cell is a source).  Later
// levels: entry = rank i of the list `fr`, four flags (offer base + 4 i + k won its neighbour).
struct Level {
    const double* m;             // the raster being filled, in place
    const double* mask;
    const int32_t* fr;           // this level's list (null: level 0)
    const u64* key;
    u64 base;
    int64_t n;                   // entries: cells at level 0, list length after
    int64_t R, C;
};

__device__ __forceinline__ int entry_flags(const Level& L, int64_t e, int64_t nb[4]) {
    int f = 0;
    if (e >= L.n) return 0;
    if (!L.fr) {
        if (!isnan(L.mask[e]) && !isnan(L.m[e])) f = 1;
        nb[0] = e;
        return f;
    }
    const int64_t cell = L.fr[e];
    for (int k = 0; k < 4; ++k) {
        nb[k] = neighbour(cell, k, L.R, L.C);
        if (nb[k] >= 0 && L.key[nb[k]] == L.base + 4 * (u64)e + (u64)k) f |= 1 << k;
    }
    return f;
}

// offers of one level
__global__ __launch_bounds__(256) void k_claim(const double* __restrict__ m, const double* __restrict__ mask,
                                               const int32_t* __restrict__ fr, int64_t n, u64 base, int64_t R, int64_t C,
                                               u64* __restrict__ key) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int64_t cell = fr[e];
    for (int k = 0; k < 4; ++k) {
        const int64_t nb = neighbour(cell, k, R, C);
        if (nb < 0 || isnan(mask[nb]) || !isnan(m[nb])) continue;
        atomicMin(&key[nb], base + 4 * (u64)e + (u64)k);
    }
}

// flags of one workgroup's entries -> sums[blockIdx.x]
__global__ __launch_bounds__(256) void k_level_count(Level L, u64* __restrict__ sums) {
    __shared__ unsigned int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int64_t nb[4];
    const int f = entry_flags(L, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nb);
    if (f) atomicAdd(&cnt, (unsigned)__popc(f));
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = cnt;
}

// exclusive scan of sums[0 .. nblocks) in place by ONE workgroup; the total goes to *total
__global__ __launch_bounds__(256) void k_scan_sums(u64* __restrict__ sums, int64_t nblocks, u64* __restrict__ total) {
    __shared__ u64 part[256];
    const int64_t per = (nblocks + 255) / 256;
    const int64_t b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    u64 s = 0;
    for (int64_t b = b0; b < b1; ++b) s += sums[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 run = 0;
        for (int t = 0; t < 256; ++t) { const u64 v = part[t]; part[t] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    u64 run = part[threadIdx.x];
    for (int64_t b = b0; b < b1; ++b) { const u64 v = sums[b]; sums[b] = run; run += v; }
}

// the winners, in key order, into the next list; their values into the cells they took
__global__ __launch_bounds__(256) void k_level_emit(Level L, const u64* __restrict__ sums, double* __restrict__ m,
                                                    int32_t* __restrict__ next) {
    __shared__ unsigned int pre[256];
    int64_t nb[4];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = entry_flags(L, e, nb);
    pre[threadIdx.x] = (unsigned)__popc(f);
    __syncthreads();
    for (unsigned o = 1; o < blockDim.x; o <<= 1) {          // inclusive scan over the workgroup
        const unsigned v = threadIdx.x >= o ? pre[threadIdx.x - o] : 0u;
        __syncthreads();
        pre[threadIdx.x] += v;
        __syncthreads();
    }
    if (!f) return;
    u64 at = sums[blockIdx.x] + pre[threadIdx.x] - (unsigned)__popc(f);
    if (!L.fr) {
        next[at] = (int32_t)e;
        return;
    }
    const double v = m[L.fr[e]];                             // set when this cell was taken, by an earlier launch
    for (int k = 0; k < 4; ++k)
        if (f & (1 << k)) {
            next[at++] = (int32_t)nb[k];
            m[nb[k]] = v;
        }
}

// ---- reductions ---------------------------------------------------------------------------------------------------------------
// a workgroup's two (sum, count) pairs through a fixed LDS tree into out[4 + 4 * blockIdx.x ..]
__device__ __forceinline__ void part_reduce(double s0, double c0, double s1, double c1, double* __restrict__ out) {
    __shared__ double sh[4][vp::kRedLanes];
    sh[0][threadIdx.x] = s0;
    sh[1][threadIdx.x] = c0;
    sh[2][threadIdx.x] = s1;
    sh[3][threadIdx.x] = c1;
    __syncthreads();
    for (int w = vp::kRedLanes / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 4) out[4 + 4 * blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void k_mean_parts(const double* __restrict__ v, int64_t N, double* __restrict__ out) {
    double s = 0.0, c = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * vp::kRedLanes + threadIdx.x; i < N; i += (int64_t)vp::kRedParts * vp::kRedLanes) {
        const double a = v[i];
        if (!isnan(a)) { s += a; c += 1.0; }
    }
    part_reduce(s, c, 0.0, 0.0, out);
}

// the half-and-half update (R/dataprep.R:1029-1030) and the sums of |new - second| (:1031-1032)
__global__ __launch_bounds__(256) void k_update_parts(double* __restrict__ gref, const double* __restrict__ gref2,
                                                      double* __restrict__ lref, const double* __restrict__ lref2, int64_t N,
                                                      double* __restrict__ out) {
    double sg = 0.0, cg = 0.0, sl = 0.0, cl = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * vp::kRedLanes + threadIdx.x; i < N; i += (int64_t)vp::kRedParts * vp::kRedLanes) {
        const double g2 = gref2[i], l2 = lref2[i];
        const double g = 0.5 * gref[i] + 0.5 * g2;
        const double l = 0.5 * lref[i] + 0.5 * l2;
        gref[i] = g;
        lref[i] = l;
        const double dg = fabs(g - g2), dl = fabs(l - l2);
        if (!isnan(dg)) { sg += dg; cg += 1.0; }
        if (!isnan(dl)) { sl += dl; cl += 1.0; }
    }
    part_reduce(sg, cg, sl, cl, out);
}

// the parts in order; out[0], out[1]: the two means
__global__ void k_means_finish(double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = 0; p < vp::kRedParts; ++p)
        for (int q = 0; q < 4; ++q) t[q] += out[4 + 4 * p + q];
    out[0] = t[0] / t[1];
    out[1] = t[2] / t[3];
}

// lref0 = 0.25 + 0.5 alb, gref0 = 0.15, NA where x is (R/dataprep.R:1006-1007)
__global__ __launch_bounds__(256) void k_start(const double* __restrict__ x, const double* __restrict__ alb, int64_t N,
                                               double* __restrict__ lref, double* __restrict__ gref) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    lref[c] = (x[c] * 0 + 0.5) * (1 - 0.5) + 0.5 * alb[c];
    gref[c] = x[c] * 0 + 0.15;
}

// the three results, NA as R's NA_real_
__global__ __launch_bounds__(256) void k_results(const double* __restrict__ lref, const double* __restrict__ gref, double ltrr, int64_t N,
                                                 u64* __restrict__ leafr, u64* __restrict__ leaft, u64* __restrict__ gout) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double l = lref[c], t = ltrr * l, g = gref[c];
    leafr[c] = isnan(l) ? vp::kNaRealBits : (u64)__double_as_longlong(l);
    leaft[c] = isnan(t) ? vp::kNaRealBits : (u64)__double_as_longlong(t);
    gout[c] = isnan(g) ? vp::kNaRealBits : (u64)__double_as_longlong(g);
}

inline unsigned grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// scratch of the fill, taken once per call (the fused loop fills up to 100 times)
struct FillScratch {
    u64* key = nullptr;
    int32_t* fr[2] = {nullptr, nullptr};
    u64* sums = nullptr;
    u64* total = nullptr;
    int alloc(mcf::DevOwner& db, int64_t n, int block) {
        int rc;
        if ((rc = db.make(&key, n))) return rc;
        if ((rc = db.make(&fr[0], n))) return rc;
        if ((rc = db.make(&fr[1], n))) return rc;
        if ((rc = db.make(&sums, (n + block - 1) / block + 1))) return rc;
        return db.make(&total, 1);
    }
};

// fill_naCpp of d_m in place; `levels`: how many lists after the sources' were not empty
int fill_launch(double* d_m, const double* d_mask, int64_t R, int64_t C, FillScratch& fs, int block, int* levels) {
    const int64_t N = R * C;
    HIP_TRY(hipMemsetAsync(fs.key, 0xFF, (size_t)N * 8, nullptr));
    Level L{d_m, d_mask, nullptr, fs.key, 0, N, R, C};
    int cur = 0, depth = 0;
    u64 base = 0;
    for (;;) {
        // the list of level `depth` into fr[cur]: level 0 from the cells, later levels from the list before
        const unsigned nblocks = grid_for(L.n, block);
        hipLaunchKernelGGL(k_level_count, dim3(nblocks), dim3(block), 0, nullptr, L, fs.sums);
        hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, nullptr, fs.sums, (int64_t)nblocks, fs.total);
        hipLaunchKernelGGL(k_level_emit, dim3(nblocks), dim3(block), 0, nullptr, L, fs.sums, d_m, fs.fr[cur]);
        HIP_TRY(hipGetLastError());
        u64 count = 0;
        HIP_TRY(hipMemcpy(&count, fs.total, 8, hipMemcpyDeviceToHost));
        if (count == 0) break;
        if ((int64_t)count > N) return mcf::api_fail(MCF_ERR_HIP, "nearest fill: a level longer than the raster");
        if (depth > 0) ++*levels;
        if (depth > N) return mcf::api_fail(MCF_ERR_HIP, "nearest fill: more levels than cells");
        base += 4 * (u64)L.n;                                  // past every key of the level before
        hipLaunchKernelGGL(k_claim, dim3(grid_for((int64_t)count, block)), dim3(block), 0, nullptr, d_m, d_mask, fs.fr[cur],
                           (int64_t)count, base, R, C, fs.key);
        L.fr = fs.fr[cur];
        L.n = (int64_t)count;
        L.base = base;
        cur ^= 1;
        ++depth;
    }
    return MCF_OK;
}

int check_block(int block) {
    if (block != 64 && block != 128 && block != 256) return mcf::api_fail(MCF_ERR_ARG, "workgroup size must be 64, 128 or 256");
    return MCF_OK;
}

// the whole loop of leafrfromalb() on the current device; results to host arrays
int leafr_loop(int64_t rows, int64_t cols, const double* pai, const double* x, const double* alb, double ltrr, mcf_leafr_out* out,
               int block) {
    const int64_t N = rows * cols;
    if (N >= ((int64_t)1 << 31)) return mcf::api_fail(MCF_ERR_ARG, "leafrfromalb on the device: at most 2^31 - 1 cells");
    int rc;
    mcf::DevOwner db;
    const double *d_pai, *d_x, *d_alb;
    double *d_lref, *d_gref, *d_lref2, *d_gref2, *d_red;
    if ((rc = db.up(&d_pai, pai, N, "pai"))) return rc;
    if ((rc = db.up(&d_x, x, N, "x"))) return rc;
    if ((rc = db.up(&d_alb, alb, N, "alb"))) return rc;
    if ((rc = db.make(&d_lref, N)) || (rc = db.make(&d_gref, N)) || (rc = db.make(&d_lref2, N)) || (rc = db.make(&d_gref2, N))) return rc;
    if ((rc = db.make(&d_red, 4 + 4 * vp::kRedParts))) return rc;
    FillScratch fs;
    if ((rc = fs.alloc(db, N, block))) return rc;

    double means[2];
    hipLaunchKernelGGL(k_mean_parts, dim3(vp::kRedParts), dim3(vp::kRedLanes), 0, nullptr, d_pai, N, d_red);
    hipLaunchKernelGGL(k_means_finish, dim3(1), dim3(1), 0, nullptr, d_red);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(means, d_red, 16, hipMemcpyDeviceToHost));
    if (isnan(means[0])) return mcf::api_fail(MCF_ERR_ARG, "mcf_leafrfromalb_device: pai holds no value");
    const double tst = exp(-means[0]);
    const bool lref_first = tst < 0.5;
    hipLaunchKernelGGL(k_start, dim3(grid_for(N, block)), dim3(block), 0, nullptr, d_x, d_alb, N, d_lref, d_gref);

    const dim3 g(grid_for(N, block)), b(block);
    double mxdif = vp::kLoopTol * 10, mx1 = 0.0, mx2 = 0.0;
    int itr = 1, passes = 0, levels = 0;
    while (mxdif > vp::kLoopTol) {
        if (lref_first) {
            hipLaunchKernelGGL(k_find_lref, g, b, 0, nullptr, d_pai, d_gref, d_x, d_alb, ltrr, N, (u64*)d_lref2);
            if ((rc = fill_launch(d_lref2, d_x, rows, cols, fs, block, &levels))) return rc;
            hipLaunchKernelGGL(k_find_gref, g, b, 0, nullptr, d_lref2, d_pai, d_x, d_alb, ltrr, N, (u64*)d_gref2);
            if ((rc = fill_launch(d_gref2, d_x, rows, cols, fs, block, &levels))) return rc;
        } else {
            hipLaunchKernelGGL(k_find_gref, g, b, 0, nullptr, d_lref, d_pai, d_x, d_alb, ltrr, N, (u64*)d_gref2);
            if ((rc = fill_launch(d_gref2, d_x, rows, cols, fs, block, &levels))) return rc;
            hipLaunchKernelGGL(k_find_lref, g, b, 0, nullptr, d_pai, d_gref2, d_x, d_alb, ltrr, N, (u64*)d_lref2);
            if ((rc = fill_launch(d_lref2, d_x, rows, cols, fs, block, &levels))) return rc;
        }
        hipLaunchKernelGGL(k_update_parts, dim3(vp::kRedParts), dim3(vp::kRedLanes), 0, nullptr, d_gref, d_gref2, d_lref, d_lref2, N,
                           d_red);
        hipLaunchKernelGGL(k_means_finish, dim3(1), dim3(1), 0, nullptr, d_red);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(means, d_red, 16, hipMemcpyDeviceToHost));
        mx1 = means[0];
        mx2 = means[1];
        mxdif = (mx1 > mx2 || isnan(mx1)) ? mx1 : mx2;
        ++passes;
        ++itr;
        if (itr > vp::kMaxPasses) mxdif = 0;
    }
    // lref2 / gref2 are free now: they and the first fill list's memory take the three results
    u64 *d_r0 = (u64*)d_lref2, *d_r1 = (u64*)d_gref2, *d_r2 = fs.key;
    hipLaunchKernelGGL(k_results, g, b, 0, nullptr, d_lref, d_gref, ltrr, N, d_r0, d_r1, d_r2);
    HIP_TRY(hipGetLastError());
    mcf::ToHost th;
    HIP_TRY(th.dense(out->leafr, d_r0, (size_t)N * 8));
    HIP_TRY(th.dense(out->leaft, d_r1, (size_t)N * 8));
    HIP_TRY(th.dense(out->gref, d_r2, (size_t)N * 8));
    out->iterations = passes;
    out->lref_first = lref_first ? 1 : 0;
    out->mxdif_gref = mx1;
    out->mxdif_leaf = mx2;
    if (getenv("MCF_TIMING"))
        fprintf(stderr, "[mcf] leafrfromalb: %lld x %lld cells, %d passes, %d fill levels\n", (long long)rows, (long long)cols, passes, levels);
    return MCF_OK;
}

// one per-cell solve or one fill with host pointers: what = 0 find_lref(a = pai, b = gref), 1 find_gref(a = lref, b = pai),
// 2 fill (a = m, b = mask)
int single_host(int what, int64_t rows, int64_t cols, const double* a, const double* b, const double* x, const double* alb, double ltrr,
                double* res, int32_t device, int block) {
    if (const int rc = mcf::check_device(device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(device));
    const int64_t N = rows * cols;
    if (N >= ((int64_t)1 << 31)) return mcf::api_fail(MCF_ERR_ARG, "vegetation pre-compute on the device: at most 2^31 - 1 cells");
    int rc;
    mcf::DevOwner db;
    const double *d_b, *d_x = nullptr, *d_alb = nullptr;
    double *d_a, *d_res;
    if ((rc = db.up_mut(&d_a, a, N, "first raster"))) return rc;
    if ((rc = db.up(&d_b, b, N, "second raster"))) return rc;
    if (what == 2) {
        FillScratch fs;
        int levels = 0;
        if ((rc = fs.alloc(db, N, block))) return rc;
        if ((rc = fill_launch(d_a, d_b, rows, cols, fs, block, &levels))) return rc;
        d_res = d_a;
    } else {
        if ((rc = db.up(&d_x, x, N, "x"))) return rc;
        if ((rc = db.up(&d_alb, alb, N, "albin"))) return rc;
        if ((rc = db.make(&d_res, N))) return rc;
        if (what == 0)
            hipLaunchKernelGGL(k_find_lref, dim3(grid_for(N, block)), dim3(block), 0, nullptr, d_a, d_b, d_x, d_alb, ltrr, N, (u64*)d_res);
        else
            hipLaunchKernelGGL(k_find_gref, dim3(grid_for(N, block)), dim3(block), 0, nullptr, d_a, d_b, d_x, d_alb, ltrr, N, (u64*)d_res);
        HIP_TRY(hipGetLastError());
    }
    mcf::ToHost th;
    HIP_TRY(th.dense(res, d_res, (size_t)N * 8));
    return MCF_OK;
}

}  // namespace

// ---- C ABI: host pointers in and out ----------------------------------------------------------------------------------------
extern "C" int mcf_find_lref_device(int64_t rows, int64_t cols, const double* pai, const double* gref, const double* x,
                                    const double* albin, double ltrr, double* lref_out, int32_t device) {
    if (rows < 1 || cols < 1 || !pai || !gref || !x || !albin || !lref_out)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_find_lref_device: bad dimensions or null argument");
    if (!isfinite(ltrr)) return mcf::api_fail(MCF_ERR_ARG, "mcf_find_lref_device: ltrr is not finite");
    return single_host(0, rows, cols, pai, gref, x, albin, ltrr, lref_out, device, 256);
}

extern "C" int mcf_find_gref_device(int64_t rows, int64_t cols, const double* lref, const double* pai, const double* x,
                                    const double* albin, double ltrr, double* gref_out, int32_t device) {
    if (rows < 1 || cols < 1 || !lref || !pai || !x || !albin || !gref_out)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_find_gref_device: bad dimensions or null argument");
    if (!isfinite(ltrr)) return mcf::api_fail(MCF_ERR_ARG, "mcf_find_gref_device: ltrr is not finite");
    return single_host(1, rows, cols, lref, pai, x, albin, ltrr, gref_out, device, 256);
}

extern "C" int mcf_fill_na_device(int64_t rows, int64_t cols, const double* m, const double* mask, double* out, int32_t device) {
    if (rows < 1 || cols < 1 || !m || !mask || !out) return mcf::api_fail(MCF_ERR_ARG, "mcf_fill_na_device: bad dimensions or null argument");
    return single_host(2, rows, cols, m, mask, nullptr, nullptr, 0.0, out, device, 256);
}

extern "C" int mcf_leafrfromalb_device(int64_t rows, int64_t cols, const double* pai, const double* x, const double* alb, double ltrr,
                                       mcf_leafr_out* out, int32_t device) {
    if (rows < 1 || cols < 1 || !pai || !x || !alb || !out || !out->leafr || !out->leaft || !out->gref)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_leafrfromalb_device: bad dimensions or null argument");
    if (!isfinite(ltrr)) return mcf::api_fail(MCF_ERR_ARG, "mcf_leafrfromalb_device: ltrr is not finite");
    if (const int rc = mcf::check_device(device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(device));
    return leafr_loop(rows, cols, pai, x, alb, ltrr, out, 256);
}

extern "C" int mcf_selftest_vegprep(int32_t kind, int64_t rows, int64_t cols, const double* a, const double* b, const double* c,
                                    const double* d, const double* e, double ltrr, double* out, int32_t block, int32_t device) {
    if (rows < 1 || cols < 1 || !a || !b || !c || !out) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_vegprep: bad dimensions or null argument");
    const int64_t N = rows * cols;
    if (kind == 0 || kind == 1) {
        if (!d || !e) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_vegprep: null argument");
        if (kind == 0) {
            mcf::vegprep_host_residual(N, a, b, c, d, e, ltrr, out);
            return MCF_OK;
        }
        if (const int rc = mcf::check_device(device)) return rc;
        mcf::RestoreDevice restore;
        HIP_TRY(hipSetDevice(device));
        int rc;
        mcf::DevOwner db;
        const double* dv[5];
        const double* hv[5] = {a, b, c, d, e};
        double* d_out;
        for (int k = 0; k < 5; ++k)
            if ((rc = db.up(&dv[k], hv[k], N, "selftest input"))) return rc;
        if ((rc = db.make(&d_out, N))) return rc;
        hipLaunchKernelGGL(k_residual, dim3(grid_for(N, 256)), dim3(256), 0, nullptr, dv[0], dv[1], dv[2], dv[3], dv[4], ltrr, N, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out, d_out, (size_t)N * 8, hipMemcpyDeviceToHost));
        return MCF_OK;
    }
    if (kind == 2) {
        if (const int rc = check_block(block)) return rc;
        if (!isfinite(ltrr)) return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_vegprep: ltrr is not finite");
        if (const int rc = mcf::check_device(device)) return rc;
        mcf::RestoreDevice restore;
        HIP_TRY(hipSetDevice(device));
        mcf_leafr_out o;
        o.leafr = out;
        o.leaft = out + N;
        o.gref = out + 2 * N;
        if (const int rc = leafr_loop(rows, cols, a, b, c, ltrr, &o, block)) return rc;
        out[3 * N] = o.iterations;
        out[3 * N + 1] = o.mxdif_gref;
        out[3 * N + 2] = o.mxdif_leaf;
        out[3 * N + 3] = o.lref_first;
        return MCF_OK;
    }
    return mcf::api_fail(MCF_ERR_ARG, "mcf_selftest_vegprep: unknown kind");
}
