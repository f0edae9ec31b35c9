// mcf_vegprep.cpp — host twin of mcf_vegprep.hip: find_lref / find_gref (reference src/microclimfCpp.cpp:5675-5724),
// fill_naCpp (:5727-5777) and the loop of leafrfromalb() (R/dataprep.R:1007-1049).  The arithmetic is mcf_vegprep.h's, shared
// with the device unit; this file adds the per-cell loops, the literal FIFO fill and the loop's sums in the device's order.
//
// Kept from the reference on purpose:
//  * a cell is NA if any of its four inputs is (cpp:5686-5689); solve_gref gives NA when its 100 steps run out, solve_lref
//    its last `mid` (cpp:5647, 5670);
//  * the fill is a multi-source breadth-first search inside the mask, sources queued in column-major order, neighbours tried
//    as row - 1, row + 1, col - 1, col + 1; cells where the mask is NA keep what `m` holds, unreachable cells stay NA;
//  * the loop: tst = exp(-mean(pai)) picks the unknown solved first, lref starts at 0.25 + 0.5 alb and gref at 0.15 (NA where
//    x is), the update is half old and half new, and it ends when max(mean|dgref|, mean|dlref|) <= 0.001 or after 50 passes.
// Guarded: a pai without a single value (R stops at `if (tst < 0.5)` with a missing value) is refused.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mcf.h"
#include "mcf_vegprep.h"

namespace mcf {
int api_fail(int code, const std::string& msg);   // mcf_api.hip

namespace vp = vegprep;

// leafrcpp elementwise as this unit's compiler builds it (mcf_selftest_vegprep kind 0)
void vegprep_host_residual(int64_t n, const double* lref, const double* pai, const double* gref, const double* x, const double* albin,
                           double ltrr, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = vp::leafr_residual(lref[i], pai[i], gref[i], x[i], albin[i], ltrr);
}
}  // namespace mcf

namespace {

namespace vp = mcf::vegprep;

void find_lref_host(int64_t N, const double* pai, const double* gref, const double* x, const double* alb, double ltrr, double* out) {
    for (int64_t i = 0; i < N; ++i) {
        const uint64_t u = vp::cell_lref(pai[i], gref[i], x[i], alb[i], ltrr);
        memcpy(&out[i], &u, 8);
    }
}

void find_gref_host(int64_t N, const double* lref, const double* pai, const double* x, const double* alb, double ltrr, double* out) {
    for (int64_t i = 0; i < N; ++i) {
        const uint64_t u = vp::cell_gref(lref[i], pai[i], x[i], alb[i], ltrr);
        memcpy(&out[i], &u, 8);
    }
}

// fill_naCpp in place (cpp:5727-5777); the queue is a vector read from the front, nothing ever leaves it
void fill_na_host(int64_t R, int64_t C, double* m, const double* mask) {
    const int64_t N = R * C;
    std::vector<int64_t> src((size_t)N, -1), q;
    q.reserve((size_t)N);
    for (int64_t idx = 0; idx < N; ++idx)
        if (!isnan(mask[idx]) && !isnan(m[idx])) { src[(size_t)idx] = idx; q.push_back(idx); }
    static const int dr[4] = {-1, 1, 0, 0}, dc[4] = {0, 0, -1, 1};
    for (size_t head = 0; head < q.size(); ++head) {
        const int64_t cur = q[head], r = cur % R, c = cur / R;
        for (int k = 0; k < 4; ++k) {
            const int64_t rr = r + dr[k], cc = c + dc[k];
            if (rr < 0 || rr >= R || cc < 0 || cc >= C) continue;
            const int64_t nb = rr + R * cc;
            if (isnan(mask[nb]) || src[(size_t)nb] != -1) continue;
            src[(size_t)nb] = src[(size_t)cur];
            q.push_back(nb);
        }
    }
    for (int64_t idx = 0; idx < N; ++idx)
        if (!isnan(mask[idx]) && isnan(m[idx]) && src[(size_t)idx] != -1) m[idx] = m[src[(size_t)idx]];
}

// sums in the order of the device's reduction (mcf_vegprep.hip k_mean_parts / k_update_parts): element i goes to accumulator
// i mod (parts * lanes), a part's lanes are added pairwise, the parts in order
struct FixedSum {
    std::vector<double> s, c;
    FixedSum() : s((size_t)vp::kRedParts * vp::kRedLanes, 0.0), c((size_t)vp::kRedParts * vp::kRedLanes, 0.0) {}
    void add(int64_t i, double v) {
        if (isnan(v)) return;
        const size_t l = (size_t)(i % ((int64_t)vp::kRedParts * vp::kRedLanes));
        s[l] += v;
        c[l] += 1.0;
    }
    double mean() {
        double st = 0.0, ct = 0.0;
        for (int p = 0; p < vp::kRedParts; ++p) {
            double* ps = &s[(size_t)p * vp::kRedLanes];
            double* pc = &c[(size_t)p * vp::kRedLanes];
            for (int w = vp::kRedLanes / 2; w > 0; w >>= 1)
                for (int t = 0; t < w; ++t) { ps[t] += ps[t + w]; pc[t] += pc[t + w]; }
            st += ps[0];
            ct += pc[0];
        }
        return st / ct;
    }
};

bool bad_dims(int64_t rows, int64_t cols) { return rows < 1 || cols < 1; }

}  // namespace

extern "C" int mcf_find_lref(int64_t rows, int64_t cols, const double* pai, const double* gref, const double* x, const double* albin,
                             double ltrr, double* lref_out) {
    if (bad_dims(rows, cols) || !pai || !gref || !x || !albin || !lref_out)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_find_lref: bad dimensions or null argument");
    if (!isfinite(ltrr)) return mcf::api_fail(MCF_ERR_ARG, "mcf_find_lref: ltrr is not finite");
    find_lref_host(rows * cols, pai, gref, x, albin, ltrr, lref_out);
    return MCF_OK;
}

extern "C" int mcf_find_gref(int64_t rows, int64_t cols, const double* lref, const double* pai, const double* x, const double* albin,
                             double ltrr, double* gref_out) {
    if (bad_dims(rows, cols) || !lref || !pai || !x || !albin || !gref_out)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_find_gref: bad dimensions or null argument");
    if (!isfinite(ltrr)) return mcf::api_fail(MCF_ERR_ARG, "mcf_find_gref: ltrr is not finite");
    find_gref_host(rows * cols, lref, pai, x, albin, ltrr, gref_out);
    return MCF_OK;
}

extern "C" int mcf_fill_na(int64_t rows, int64_t cols, const double* m, const double* mask, double* out) {
    if (bad_dims(rows, cols) || !m || !mask || !out) return mcf::api_fail(MCF_ERR_ARG, "mcf_fill_na: bad dimensions or null argument");
    if (out != m) memcpy(out, m, (size_t)(rows * cols) * 8);
    fill_na_host(rows, cols, out, mask);
    return MCF_OK;
}

extern "C" int mcf_leafrfromalb(int64_t rows, int64_t cols, const double* pai, const double* x, const double* alb, double ltrr,
                                mcf_leafr_out* out) {
    if (bad_dims(rows, cols) || !pai || !x || !alb || !out || !out->leafr || !out->leaft || !out->gref)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_leafrfromalb: bad dimensions or null argument");
    if (!isfinite(ltrr)) return mcf::api_fail(MCF_ERR_ARG, "mcf_leafrfromalb: ltrr is not finite");
    const int64_t N = rows * cols;
    double mpai;
    {
        FixedSum f;
        for (int64_t i = 0; i < N; ++i) f.add(i, pai[i]);
        mpai = f.mean();
    }
    if (isnan(mpai)) return mcf::api_fail(MCF_ERR_ARG, "mcf_leafrfromalb: pai holds no value");
    const double tst = exp(-mpai);                                     // R/dataprep.R:1005
    const bool lref_first = tst < 0.5;
    std::vector<double> lref((size_t)N), gref((size_t)N), lref2((size_t)N), gref2((size_t)N);
    for (int64_t i = 0; i < N; ++i) {
        lref[(size_t)i] = (x[i] * 0 + 0.5) * (1 - 0.5) + 0.5 * alb[i];   // R/dataprep.R:1006-1007
        gref[(size_t)i] = x[i] * 0 + 0.15;
    }
    double mxdif = vp::kLoopTol * 10, mx1 = 0.0, mx2 = 0.0;
    int itr = 1, passes = 0;
    while (mxdif > vp::kLoopTol) {
        if (lref_first) {
            find_lref_host(N, pai, gref.data(), x, alb, ltrr, lref2.data());
            fill_na_host(rows, cols, lref2.data(), x);
            find_gref_host(N, lref2.data(), pai, x, alb, ltrr, gref2.data());
            fill_na_host(rows, cols, gref2.data(), x);
        } else {
            find_gref_host(N, lref.data(), pai, x, alb, ltrr, gref2.data());
            fill_na_host(rows, cols, gref2.data(), x);
            find_lref_host(N, pai, gref2.data(), x, alb, ltrr, lref2.data());
            fill_na_host(rows, cols, lref2.data(), x);
        }
        FixedSum fg, fl;
        for (int64_t i = 0; i < N; ++i) {
            const size_t k = (size_t)i;
            gref[k] = 0.5 * gref[k] + 0.5 * gref2[k];
            lref[k] = 0.5 * lref[k] + 0.5 * lref2[k];
            fg.add(i, fabs(gref[k] - gref2[k]));
            fl.add(i, fabs(lref[k] - lref2[k]));
        }
        mx1 = fg.mean();
        mx2 = fl.mean();
        mxdif = (mx1 > mx2 || isnan(mx1)) ? mx1 : mx2;
        ++passes;
        ++itr;
        if (itr > vp::kMaxPasses) mxdif = 0;
    }
    for (int64_t i = 0; i < N; ++i) {
        const size_t k = (size_t)i;
        const double lt = ltrr * lref[k];
        const uint64_t na = vp::kNaRealBits;
        if (isnan(lref[k])) memcpy(&out->leafr[i], &na, 8); else out->leafr[i] = lref[k];
        if (isnan(lt)) memcpy(&out->leaft[i], &na, 8); else out->leaft[i] = lt;
        if (isnan(gref[k])) memcpy(&out->gref[i], &na, 8); else out->gref[i] = gref[k];
    }
    out->iterations = passes;
    out->lref_first = lref_first ? 1 : 0;
    out->mxdif_gref = mx1;
    out->mxdif_leaf = mx2;
    return MCF_OK;
}
