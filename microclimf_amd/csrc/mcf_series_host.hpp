// mcf_series_host.hpp — the series sink over row blocks (include/mcf.h "series sink", "Row blocks"): a whole-raster
// spec cut to a block's rows, and the blocks' zone states combined and finished on the host.  The states are integers (sums
// and counts add, the minimum keys take the minimum, the maximum keys the maximum), so the combination has the bits of the
// one-block run; the finish is k_series_fin's arithmetic, once, on the combined state.  Host only.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/mcf.h"

namespace mcf {

constexpr int kSeriesStateRows = 4;      // mcf_kernels.h kSeriesRows, in its order: sum, count word, minimum key, maximum key
constexpr int64_t kSeriesMaxCells = (int64_t)1 << 26;

// rows [r0, r0 + nr) of a spec given for the whole raster (cells: row + R * col; zone: [R * cols], column-major)
struct SeriesBlockCut {
    std::vector<int64_t> cells;      // the block's points as cells of the block, row - r0 + nr * col
    std::vector<int64_t> where;      // their places in the caller's list (a point belongs to the block that holds its row)
    std::vector<int32_t> zone;       // [nr * cols]
    void cut(int64_t npoints, const int64_t* all_cells, int32_t nzones, const int32_t* all_zone, int64_t R, int64_t C, int64_t r0,
             int64_t nr) {
        cells.clear(); where.clear(); zone.clear();
        for (int64_t i = 0; i < npoints; ++i) {
            const int64_t row = all_cells[i] % R, col = all_cells[i] / R;
            if (row < r0 || row >= r0 + nr) continue;
            cells.push_back(row - r0 + nr * col);
            where.push_back(i);
        }
        if (nzones > 0) {
            zone.resize((size_t)(nr * C));
            for (int64_t c = 0; c < C; ++c) memcpy(zone.data() + c * nr, all_zone + c * R + r0, (size_t)nr * 4);
        }
    }
    bool empty(int32_t nzones) const { return cells.empty() && nzones == 0; }      // nothing of the spec falls into the block
};

// into <- into (+) from, both [4][nzones][steps]
inline void series_state_merge(int64_t* into, const int64_t* from, int32_t nzones, int64_t steps) {
    const int64_t row = (int64_t)nzones * steps;
    for (int64_t i = 0; i < row; ++i) {
        into[i] += from[i];
        into[row + i] += from[row + i];
        if (from[2 * row + i] < into[2 * row + i]) into[2 * row + i] = from[2 * row + i];
        if (from[3 * row + i] > into[3 * row + i]) into[3 * row + i] = from[3 * row + i];
    }
}
// the state nothing has been folded into
inline void series_state_init(int64_t* st, int32_t nzones, int64_t steps) {
    const int64_t row = (int64_t)nzones * steps;
    for (int64_t i = 0; i < row; ++i) {
        st[i] = 0; st[row + i] = 0; st[2 * row + i] = INT64_MAX; st[3 * row + i] = INT64_MIN;
    }
}
// one statistic [nsteps, nzones], column-major, as k_series_fin makes it; day_done: [steps / 24] or null (every day folded)
inline void series_state_finish(const int64_t* st, int32_t nzones, int64_t steps, int64_t nsteps, const int32_t* day_done,
                                int32_t zstat, double* out) {
    const uint64_t na_bits = 0x7FF00000000007A2ull;
    double na;
    memcpy(&na, &na_bits, 8);
    const int64_t row = (int64_t)nzones * steps;
    for (int64_t z = 0; z < nzones; ++z)
        for (int64_t k = 0; k < nsteps; ++k) {
            double v = na;
            if (k < steps && (!day_done || day_done[k / 24])) {
                const int64_t at = z * steps + k;
                const uint64_t cb = (uint64_t)st[row + at];
                const uint32_t n = (uint32_t)cb, bad = (uint32_t)(cb >> 32);
                if (zstat == MCF_ZSTAT_COUNT) v = (double)n;
                else if (n > 0 && bad == 0) {
                    if (zstat == MCF_ZSTAT_MEAN) v = ((double)st[at] * 0x1p-24) / (double)n;
                    else {
                        const int64_t key = st[(zstat == MCF_ZSTAT_MIN ? 2 : 3) * row + at];
                        const int64_t bits = key >= 0 ? key : key ^ INT64_MAX;
                        double x;
                        memcpy(&x, &bits, 8);
                        v = x + 0.0;
                    }
                }
            }
            out[z * nsteps + k] = v;
        }
}

}  // namespace mcf
