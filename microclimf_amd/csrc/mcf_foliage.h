// mcf_foliage.h — the gamma-shaped foliage profile of the reference's `.foliageden` (R/internal.R:937-946): leaf density at
// height z and plant area above z from canopy height and plant area index.
//
// The ONE copy of the arithmetic, as __host__ __device__ functions that the host unit (mcf_foliage.cpp) and the device unit
// (mcf_foliage.hip) both include; both units are built without FMA contraction and without fast-math.
//
// Every call site of `.foliageden` in the reference uses shape 1.5 and rate 1.5 / 7, and for shape 3/2 the gamma functions are
// elementary.  With t = rate * x:
//     pgamma(x, 1.5, rate) = erf(sqrt t) - (2 / sqrt pi) sqrt t exp(-t)
//     dgamma(x, 1.5, rate) = rate^1.5 sqrt x exp(-t) / (sqrt pi / 2)
// The two terms of pgamma cancel as t -> 0 (P ~ 4 t^1.5 / (3 sqrt pi)): the closed form's relative error grows like 1.5e-16 / t.
// Below kSeriesBelow the confluent series P = t^1.5 exp(-t) / Gamma(2.5) * sum_n t^n / (2.5 * 3.5 * ... * (1.5 + n)) is used
// instead: all terms positive, and kSeriesTerms of them leave less than 2^-57 of the sum at t = kSeriesBelow.  At the threshold
// the closed form is good to about 3e-16 relative, far inside the 2^-40 this project accepts in its quotients.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define MCF_FOL_HD __host__ __device__ inline
#else
#define MCF_FOL_HD inline
#endif

namespace mcf {
namespace foliage {

constexpr double kShape = 1.5, kRate = 1.5 / 7.0;            // R/internal.R:937
constexpr double kSqrtPi = 1.7724538509055160273;            // sqrt(pi)
constexpr double kRate15 = 0.09919501068991622;              // kRate^1.5
constexpr double kSeriesBelow = 0.5;
constexpr int kSeriesTerms = 14;

// pgamma(x, 1.5, kRate); x <= 0: 0, NaN flows through
MCF_FOL_HD double pgamma15(double x) {
    if (x <= 0.0) return 0.0;
    const double t = kRate * x;
    const double st = sqrt(t), e = exp(-t);
    if (t < kSeriesBelow) {
        double s = 1.0;
        for (int n = kSeriesTerms; n >= 1; --n) s = 1.0 + (t / (1.5 + n)) * s;
        return (t * st * e / (0.75 * kSqrtPi)) * s;              // Gamma(2.5) = 3 sqrt(pi) / 4
    }
    return erf(st) - (2.0 / kSqrtPi) * st * e;
}

// dgamma(x, 1.5, kRate); x <= 0: 0, NaN flows through
MCF_FOL_HD double dgamma15(double x) {
    if (x <= 0.0) return 0.0;
    return kRate15 * sqrt(x) * exp(-(kRate * x)) / (kSqrtPi / 2.0);
}

// the total the profile is normalised by, pgamma(10): computed ONCE, on the host, and handed to both sides
inline double total_density() { return pgamma15(10.0); }

// one cell of `.foliageden`.  z >= hgt: exact zeros; hgt = 0 (x = -inf): paia 0 and leafden the reference's 0 / 0 = NaN; a NaN
// hgt or pai propagates
MCF_FOL_HD void cell(double hgt, double pai, double z, double td, double* leafden, double* paia) {
    const double x = ((hgt - z) / hgt) * 10;
    *leafden = (pai / hgt) * (dgamma15(x) / td) * 10;
    *paia = pgamma15(x) * (pai / td);
}

}  // namespace foliage
}  // namespace mcf
