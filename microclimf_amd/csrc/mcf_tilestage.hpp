// mcf_tilestage.hpp — how a 256-lane workgroup takes whole tile-day blocks of the tiled ring into LDS (k_summary_acc in
// mcf_summary.hip, k_bioclim_acc_depths in mcf_bioclim.hip): TPW consecutive tiles per workgroup, one lane per cell; a slab's
// blocks of one day come in through registers with 16-byte loads, every 128-byte line read once and whole.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcf_kernels.h"

namespace mcf {

constexpr int kSumLanes = 256;

// Geometry of a workgroup for `CPB` cells per tile: TPW tiles (<= 256 cells, one lane each), their blocks S doubles apart in
// LDS.  The pad keeps the lanes of neighbouring tiles, which read the same place of their blocks, on different banks.
template <int CPB>
struct SumGeom {
    static constexpr int B = RING_BLOCK(CPB);
    static constexpr int TPW = kSumLanes / CPB;                                   // 16, 12, 8, 6
    static constexpr int PAD = CPB == 16 ? 16 : CPB == 21 ? 22 : CPB == 42 ? 10 : 0;
    static constexpr int S = B + PAD;
    static constexpr int HALF = B / 2;                                            // 16-byte pieces per block
    static constexpr int NLD = TPW * HALF / kSumLanes;                            // pieces per lane: 12 for every CPB
    static_assert(TPW * HALF % kSumLanes == 0, "the blocks of a workgroup divide evenly over its lanes");
    static_assert(S % 2 == 0, "blocks stay 16-byte aligned in LDS");
};

// the blocks of one day of the workgroup's tiles (`day` = the first tile's block) into registers: piece j * 256 + lane of the
// tiles' pieces taken one after the other, so that a wave reads 1 KiB of one block at a time; tiles past the ring's last: none
template <int CPB>
__device__ __forceinline__ void load_day(double2 (&r)[SumGeom<CPB>::NLD], const double* day, int64_t tile_stride, int tid, int ntl) {
    using G = SumGeom<CPB>;
#pragma unroll
    for (int j = 0; j < G::NLD; ++j) {
        const int idx = j * kSumLanes + tid, t = idx / G::HALF, o = idx - t * G::HALF;
        r[j] = t < ntl ? *reinterpret_cast<const double2*>(day + (int64_t)t * tile_stride + 2 * o) : double2{0.0, 0.0};
    }
}
// ... and from the registers to their places in LDS (between two barriers of the caller's)
template <int CPB>
__device__ __forceinline__ void store_day(double* lds, const double2 (&r)[SumGeom<CPB>::NLD], int tid, int ntl) {
    using G = SumGeom<CPB>;
#pragma unroll
    for (int j = 0; j < G::NLD; ++j) {
        const int idx = j * kSumLanes + tid, t = idx / G::HALF, o = idx - t * G::HALF;
        if (t < ntl) *reinterpret_cast<double2*>(lds + t * G::S + 2 * o) = r[j];
    }
}

}  // namespace mcf
