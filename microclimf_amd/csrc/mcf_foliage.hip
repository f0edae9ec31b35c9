// mcf_foliage.hip — `.foliageden` (reference R/internal.R:937-946) on the device: the values of mcf_foliage.cpp, from the same
// arithmetic (mcf_foliage.h).
//
// k_foliage: one lane per (cell, layer) of planes laid out [layers][N] as a plan's vegetation buffers are; two 8-byte loads, two
// 8-byte stores, a few dozen fp64 operations between them.  It is bound by its four streams; nothing here is tuned.
// The total pgamma(10) is computed once by the host unit and handed in, so both sides divide by the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/mcf.h"
#include "mcf_foliage.h"
#include "mcf_kernels.h"
#include "mcf_rowblocks.hpp"
#include "mcf_hiphost.hpp"

// the host code this restates is built without FMA contraction
#pragma clang fp contract(off)

namespace mcf {
double foliage_total_density();   // mcf_foliage.cpp
}

namespace {

__global__ __launch_bounds__(256) void k_foliage(const double* __restrict__ hgt, const double* __restrict__ pai, double z, double td,
                                                 int64_t n, double* __restrict__ leafden, double* __restrict__ paia) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double ld, pa;
    mcf::foliage::cell(hgt[i], pai[i], z, td, &ld, &pa);
    leafden[i] = ld;
    paia[i] = pa;
}

}  // namespace

namespace mcf {
// leafden and paia of n = cells x layers values from hgt and pai, all on the current device, queued on `s`
void launch_foliage(const double* hgt, const double* pai, double z, int64_t n, double* leafden, double* paia, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_foliage, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, hgt, pai, z, foliage_total_density(), n, leafden,
                       paia);
}
}  // namespace mcf

extern "C" int mcf_foliageden_device(int64_t n, const double* hgt, const double* pai, double z, double* leafden, double* paia,
                                     int32_t device) {
    if (n < 1 || !hgt || !pai || !leafden || !paia)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_foliageden_device: bad length or null argument");
    if (n >= ((int64_t)1 << 38)) return mcf::api_fail(MCF_ERR_ARG, "mcf_foliageden_device: at most 2^38 - 1 values");
    if (const int rc = mcf::check_device(device)) return rc;
    mcf::RestoreDevice restore;
    HIP_TRY(hipSetDevice(device));
    int rc;
    mcf::DevOwner db;
    const double *d_hgt, *d_pai;
    double *d_ld, *d_pa;
    if ((rc = db.up(&d_hgt, hgt, n, "hgt")) || (rc = db.up(&d_pai, pai, n, "pai"))) return rc;
    if ((rc = db.make(&d_ld, n)) || (rc = db.make(&d_pa, n))) return rc;
    mcf::launch_foliage(d_hgt, d_pai, z, n, d_ld, d_pa, nullptr);
    HIP_TRY(hipGetLastError());
    mcf::ToHost th;
    HIP_TRY(th.dense(leafden, d_ld, (size_t)n * 8));
    HIP_TRY(th.dense(paia, d_pa, (size_t)n * 8));
    return MCF_OK;
}
