// mcf_ncpack.hip — netCDF records from step-major planes (include/mcf.h "netCDF sink: further sources").
//
// k_pack_nc (mcf_kernels.hip) reads the solver's ring through a RingView.  The snow plan keeps a chunk's five series as plain
// step-major planes, series[k][step * N + c] with c = row + rows * col, the layout k_series_planes folds (mcf_series.hip).
// k_pack_nc_planes finishes the same records from them: per (step, variable) the [rows, cols] plane is transposed to
// [rows][cols] with east fastest, scaled, rounded half to even, NA and out-of-range values set to the file's missval, and
// stored big-endian where the classic container wants it, record `step` = [8 B time | var0[rows][cols] | var1 ...].
// 32 x 32 tiles through LDS, so that the fp64 loads run along rows (the planes' fastest index) and the int32 stores along
// columns (the file's); 12 B of HBM traffic per value.  blockIdx.z = step * nv + k.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcf_kernels.h"

namespace mcf {

__global__ __launch_bounds__(256) void k_pack_nc_planes(PackNcPlanesArgs a) {
    __shared__ int32_t tile[32][33];
    const int step = blockIdx.z / a.nv, v = blockIdx.z - step * a.nv;
    const int64_t N = a.rows * a.cols;
    int32_t* out = a.dst + (int64_t)step * a.rec_words + 2 + (int64_t)v * N;
    const double scale = a.scale[v];
    const double* src = a.series[v] + (a.step0 + step) * N;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int64_t r0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
#pragma unroll
    for (int j = ty; j < 32; j += 8) {
        const int64_t r = r0 + tx, c = c0 + j;
        int32_t q = a.missval;
        if (r < a.rows && c < a.cols) {
            const double x = rint(src[r + a.rows * c] * scale);
            if (x > -2147483648.0 && x < 2147483648.0) q = (int32_t)x;   // NaN and out-of-range keep missval
        }
        tile[j][tx] = (int32_t)__builtin_bswap32((uint32_t)q);
    }
    __syncthreads();
#pragma unroll
    for (int j = ty; j < 32; j += 8) {
        const int64_t c = c0 + tx, r = r0 + j;
        if (r < a.rows && c < a.cols) out[c + a.cols * r] = tile[tx][j];
    }
}

void launch_pack_nc_planes(const PackNcPlanesArgs& a, int64_t nsteps, hipStream_t s) {
    if (nsteps <= 0 || a.nv <= 0) return;
    dim3 grid((unsigned)((a.rows + 31) / 32), (unsigned)((a.cols + 31) / 32), (unsigned)(nsteps * a.nv));
    hipLaunchKernelGGL(k_pack_nc_planes, grid, dim3(256), 0, s, a);
}

}  // namespace mcf
