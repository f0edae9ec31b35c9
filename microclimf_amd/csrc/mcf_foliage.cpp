// mcf_foliage.cpp — host twin of mcf_foliage.hip: `.foliageden` (reference R/internal.R:937-946) cell by cell.  The arithmetic is
// mcf_foliage.h's, shared with the device unit; this file adds the loop and the total the device side is handed.
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/mcf.h"
#include "mcf_foliage.h"

namespace mcf {
int api_fail(int code, const std::string& msg);   // mcf_api.hip

// pgamma(10, 1.5, 1.5 / 7) as this unit's compiler and libm build it: the value every device launch is handed
double foliage_total_density() { return foliage::total_density(); }
}  // namespace mcf

extern "C" int mcf_foliageden(int64_t n, const double* hgt, const double* pai, double z, double* leafden, double* paia) {
    if (n < 1 || !hgt || !pai || !leafden || !paia) return mcf::api_fail(MCF_ERR_ARG, "mcf_foliageden: bad length or null argument");
    const double td = mcf::foliage_total_density();
    for (int64_t i = 0; i < n; ++i) mcf::foliage::cell(hgt[i], pai[i], z, td, &leafden[i], &paia[i]);
    return MCF_OK;
}
