// mcf_vegprep.h — leaf and ground reflectance from albedo (the reference's exported leafrfromalb(), R/dataprep.R:1000-1050,
// with leafrcpp / solve_lref / solve_gref / find_lref / find_gref / fill_naCpp, src/microclimfCpp.cpp:5594-5777).
//
// The ONE copy of the arithmetic: the diffuse two-stream albedo residual and the two bisections, as __host__ __device__
// functions that the host unit (mcf_vegprep.cpp) and the device unit (mcf_vegprep.hip) both include.  Both units are built
// without FMA contraction and without fast-math, so every operation below is the reference's, in the reference's order;
// plain exp / sqrt / pow / cos, not the lean math of mcf_device.hpp.
//
// What is hoisted, each bit-neutral (the same operations on the same values, done once instead of per step):
//   * J depends on x only (cpp:5606-5611);
//   * a, gma, h, S1 and the two sums a + gma +- h depend on lref only: solve_gref computes them once per cell;
//   * 1 - 1 / gref depends on gref only: solve_lref computes it once per cell;
//   * f_lower is the value at the initial lower bound, or the f_mid of the step that moved `lower` there (cpp:5636, 5659
//     recompute it each step from the same arguments);
//   * the loop leaves once `mid` repeats: then upper and lower are neighbours or equal, every later step evaluates the same
//     `mid`, fails the same root test and leaves `mid` where it is.  (pai = 0: the residual gref - albin does not depend on
//     lref, `lower` runs up to the bracket end in ~53 steps and the remaining steps would only repeat.)
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define MCF_VP_HD __host__ __device__ inline
#else
#define MCF_VP_HD inline
#endif

namespace mcf {
namespace vegprep {

constexpr double kPi = 3.14159265358979323846;            // cpp:14
constexpr double kLrefLo = 0.0001, kLrefHi = 0.6665;      // cpp:5630-5631
constexpr double kGrefLo = 0.0001, kGrefHi = 0.9999;      // cpp:5653-5654
constexpr double kTol = 1e-6;                             // on the albedo residual (cpp:5629, 5652)
constexpr int kMaxIter = 100;
constexpr uint64_t kNaRealBits = 0x7FF00000000007A2ULL;   // R's NA_real_
constexpr int kMaxPasses = 50;                            // R/dataprep.R:1011
constexpr double kLoopTol = 0.001;                        // R/dataprep.R:1010

// cpp:5606-5611
MCF_VP_HD double leaf_J(double x) {
    double J = 1.0 / 3.0;
    if (x != 1.0) {
        double mla = 9.65 * pow((3 + x), -1.65);
        if (mla > kPi / 2) mla = kPi / 2.0;
        J = cos(mla) * cos(mla);
    }
    return J;
}

// the part of leafrcpp that does not depend on gref (cpp:5601-5605, 5612-5615)
struct LeafSide {
    double a, gma, h, S1, cp, cm;      // cp = a + gma + h, cm = a + gma - h
};

MCF_VP_HD LeafSide leaf_side(double lref, double pai, double J, double ltrr) {
    LeafSide s;
    const double ltra = ltrr * lref;
    const double om = lref + ltra;
    s.a = 1 - om;
    const double del = lref - ltra;
    s.gma = 0.5 * (om + J * del);
    s.h = sqrt(s.a * s.a + 2 * s.a * s.gma);      // a < 0 (ltrr = 1, lref > 0.5): NaN, and NaN flows on as in C++
    s.S1 = exp(-s.h * pai);
    s.cp = s.a + s.gma + s.h;
    s.cm = s.a + s.gma - s.h;
    return s;
}

// the rest of leafrcpp (cpp:5616-5625); gterm = 1 - 1 / gref
MCF_VP_HD double residual(const LeafSide& s, double gterm, double albin) {
    const double u1 = s.a + s.gma * gterm;
    const double D1 = s.cp * (u1 - s.h) * 1 / s.S1 - s.cm * (u1 + s.h) * s.S1;
    const double p1 = (s.gma / (D1 * s.S1)) * (u1 - s.h);
    const double p2 = (-s.gma * s.S1 / D1) * (u1 + s.h);
    const double albd = p1 + p2;
    return albd - albin;
}

// leafrcpp itself (diagnostics, mcf_selftest_vegprep)
MCF_VP_HD double leafr_residual(double lref, double pai, double gref, double x, double albin, double ltrr) {
    return residual(leaf_side(lref, pai, leaf_J(x), ltrr), 1 - 1 / gref, albin);
}

// solve_lref, cpp:5629-5648: the last `mid` when the steps run out
MCF_VP_HD double solve_lref(double pai, double gref, double J, double albin, double ltrr) {
    const double gterm = 1 - 1 / gref;
    double lower = kLrefLo, upper = kLrefHi;
    double f_lower = residual(leaf_side(lower, pai, J, ltrr), gterm, albin);
    double mid = 0.0, prev = -1.0;
    for (int iter = 0; iter < kMaxIter; ++iter) {
        mid = (lower + upper) / 2.0;
        if (mid == prev) break;
        const double f_mid = residual(leaf_side(mid, pai, J, ltrr), gterm, albin);
        if (fabs(f_mid) < kTol) return mid;
        if (f_lower * f_mid < 0) {
            upper = mid;
        } else {               // NaN included: the comparison is false
            lower = mid;
            f_lower = f_mid;
        }
        prev = mid;
    }
    return mid;
}

// solve_gref, cpp:5652-5672: NA when the steps run out (`found` false)
MCF_VP_HD double solve_gref(double lref, double pai, double J, double albin, double ltrr, bool* found) {
    const LeafSide s = leaf_side(lref, pai, J, ltrr);
    double lower = kGrefLo, upper = kGrefHi;
    double f_lower = residual(s, 1 - 1 / lower, albin);
    double mid = 0.0, prev = -1.0;
    *found = true;
    for (int iter = 0; iter < kMaxIter; ++iter) {
        mid = (lower + upper) / 2.0;
        if (mid == prev) break;
        const double f_mid = residual(s, 1 - 1 / mid, albin);
        if (fabs(f_mid) < kTol) return mid;
        if (f_lower * f_mid < 0) {
            upper = mid;
        } else {
            lower = mid;
            f_lower = f_mid;
        }
        prev = mid;
    }
    *found = false;
    return mid;
}

// one cell of find_lref (cpp:5675-5699) / find_gref (cpp:5701-5724) as a bit pattern: NA when any input is
MCF_VP_HD uint64_t dbits(double v) {
    union { double d; uint64_t u; } c;
    c.d = v;
    return c.u;
}
MCF_VP_HD uint64_t cell_lref(double pai, double gref, double x, double albin, double ltrr) {
    if (isnan(pai) || isnan(gref) || isnan(x) || isnan(albin)) return kNaRealBits;
    return dbits(solve_lref(pai, gref, leaf_J(x), albin, ltrr));
}
MCF_VP_HD uint64_t cell_gref(double lref, double pai, double x, double albin, double ltrr) {
    if (isnan(pai) || isnan(lref) || isnan(x) || isnan(albin)) return kNaRealBits;
    bool found;
    const double g = solve_gref(lref, pai, leaf_J(x), albin, ltrr, &found);
    return found ? dbits(g) : kNaRealBits;
}

// The two fixed-order sums of one pass.  Geometry shared by host and device: kRedParts x kRedLanes accumulators over strided
// subsets, a pairwise tree over the lanes of a part, the parts added in order.
constexpr int kRedParts = 128, kRedLanes = 256;

}  // namespace vegprep
}  // namespace mcf
