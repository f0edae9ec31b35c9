// mcf_kernels.h — kernel argument blocks and launchers (host-visible part).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcf {

struct Globals {
    double reqhgt;   // as given
    double reqhgt2;  // max(reqhgt, 1e-5)                       cpp:2246-2247
    double zref;
    double dTmx;     // -0.6273*mxtc + 49.79 (vector forcing)   cpp:1236
    double hf0p;     // |Hf|^0.2 of mincondCpp for gs = 999.99    cpp:1321-1328
    double hf500p;   // |Hf|^0.2 of mincondCpp for rs = 500       cpp:1321-1328
    int shadowmask;  // 1: runmicro1Cpp, 0: runmicro2Cpp         cpp:2218 vs 2499
};

// ---- the output ring as its consumers see it -------------------------------------------------------------------------
// Doubles per tile-day block of the tiled ring = lanes of the solver's workgroup for `cpb` cells per tile.
#define RING_BLOCK(cpb) ((((cpb) * 24 + 63) / 64) * 64)
__host__ __device__ inline int ring_block_doubles(int cpb) { return RING_BLOCK(cpb); }
// Place of (cell of the tile, hour of the day) inside a block: the lane that computes it in k_solve.  21-cell tiles:
// wave w = hour / 3 holds [3 hours x cells 0..15 | 3 hours x cells 16..20 | one padding double]; others hour-major.
__host__ __device__ inline int ring_pos(int cpb, int cell, int hour) {
    if (cpb == 21) {
        const int w = hour / 3, hh = hour - 3 * w;
        return 64 * w + (cell < 16 ? 16 * hh + cell : 48 + 5 * hh + (cell - 16));
    }
    return hour * cpb + cell;
}
// ... and back: the (cell, hour) of place `pos` of a block; false for a padding place
__host__ __device__ inline bool ring_unpos(int cpb, int pos, int* cell, int* hour) {
    if (cpb == 21) {
        const int w = pos >> 6, l = pos & 63;
        if (l < 48) { *cell = l & 15; *hour = 3 * w + (l >> 4); return true; }
        const int j = l - 48;
        *cell = 16 + j % 5; *hour = 3 * w + j / 5;
        return j < 15;
    }
    *cell = pos % cpb; *hour = pos / cpb;
    return pos < 24 * cpb;
}
// One variable of one ring slot: value of cell c (0-based, column-major) at step k of the slot.
//   cpb == 0  linear [step][N] (reqhgt < 0, staging buffers)
//   cpb  > 0  tiled (k_solve's layout): tile = c / cpb, block of day k / 24 at tile * tile_stride + day * day_stride
struct RingView {
    const double* base;
    int64_t N;
    int64_t tile_stride, day_stride;
    int32_t cpb;
    __host__ __device__ inline int64_t index(int64_t c, int64_t k) const {
        if (cpb == 0) return c + N * k;
        const uint32_t cc = (uint32_t)c, t = cc / (uint32_t)cpb, cell = cc - t * (uint32_t)cpb;   // N < 2^31 (checked by the host)
        const uint32_t kk = (uint32_t)k, d = kk / 24u, h = kk - 24u * d;
        return (int64_t)t * tile_stride + (int64_t)d * day_stride + ring_pos(cpb, (int)cell, (int)h);
    }
    __device__ inline double at(int64_t c, int64_t k) const { return base[index(c, k)]; }
};

struct CellSetupArgs {
    int64_t N;
    // vegp
    const double *hgt, *pai, *x, *gsmax, *leafr, *leaft, *clump, *leafd, *paia, *leafden;
    const double* hgt0;  // layer-0 height: the NA test of the cell (cpp:2182 / 2759)
    // soilc
    const double *Smin, *Smax, *gref, *soilb, *Psie, *Vq, *Vm, *Mc, *rho, *slope, *aspect, *twi, *svfa;
    const double *hor, *wsa;    // [24][N], [8][N]: only their finiteness is looked at here (FL_REGULAR)
    const double *lats, *lons;  // array forcing, else null
    const double *crowpos, *ccolpos;  // coarse array forcing: [rows], [cols]; else null
    const double *elevd, *pkfac;      // coarse array forcing with altitude correction: [N]; else null
    int64_t rows;
    double lat, lon;
    double tfact, twi_mean;
    Globals g;
    // The per-cell constant table is TILE-MAJOR: one image per (layer, tile of cpb cells), [CF_COUNT + 32 rows][cpb] doubles
    // (the 24 horizon and 8 wind-shelter values follow the CF_ rows), images tile_image_doubles(cpb) apart — what the solver
    // copies into LDS is one contiguous, line-aligned run (one page) instead of 122 row segments 8 B x N apart.
    double* cellc;      // this layer's images
    int32_t cpb;
};
// doubles between consecutive tile images: (cell fields + 32 direction rows) x cpb, rounded up to whole 128-byte lines
int64_t tile_image_doubles(int cpb);

struct TimeSetupArgs {
    int nsteps;
    const int32_t *year, *month, *day;
    const double* hour;
    const double* raw[15];  // TF_TC .. TF_DTRP, each [tsteps]
    const double* winddir;
    double lat, lon;
    double* tt;  // [ndays][TF_COUNT][24]
};

struct DateSetupArgs {
    int nsteps;
    const int32_t *year, *month, *day;
    const double* hour;
    const double* winddir;
    double* dt;       // [tsteps][4]: sin(dec), cos(dec), eot, hour
    int32_t* windex;  // [tsteps]
};

struct SolveArgs {
    int64_t N;
    const double* cellc;  // [layers][ntiles][tile image], see CellSetupArgs
    int64_t ntiles_total; // tiles of the raster = images per layer
    const int32_t* daylayer;  // [ndays] vegetation layer of each day, -1: no layer covers it; null: layer 0
    const double* tt;     // vector forcing: [ndays][TF_COUNT][24]
    // array forcing: the slot of the TILED forcing ring — block of (tile, day d of the launch, series f) at
    //   af_base + tile * af_tile_stride + d * af_day_stride + f * ring_block_doubles(cells per tile), lane order (ring_pos),
    // series in TF_TC .. TF_DTRP order.  Coarse array forcing (crows > 0): af_base = [15][crows*ccols][tsteps], af_stride
    // elements between the series.
    const double* af_base;
    int64_t af_stride;
    int64_t af_tile_stride, af_day_stride;
    const double* dt;       // [tsteps][4]
    const int32_t* windex;  // [tsteps]
    const double* mxtc;     // [N]
    // coarse array forcing (af_base = [15][crows*ccols][tsteps], whole series resident): crows > 0
    int32_t crows, ccols;
    int32_t altcorrect;     // 0, 1 (fixed lapse rate), 2 (humidity-dependent)
    // outputs.  out_sel packs, 4 bits per variable, the slab index of variable v (15 = not requested).
    // reqhgt >= 0, the TILED ring (RingView below): the block of (tile, day d of the slot, slab s) starts at
    //   out_base + tile * out_tile_stride + d * out_day_stride + s * out_var_stride
    // and holds ring_block_doubles(cells per tile) values in the solver's lane order (ring_pos).
    // reqhgt < 0, the linear ring: slab s is [slot steps][N] at out_base + s * out_stride.
    double* out_base;
    int64_t out_stride;
    uint64_t out_sel;
    int64_t slot_step0;     // linear ring: first step of this launch inside the slot
    int64_t out_tile_stride, out_day_stride, out_var_stride;
    int32_t slot_day0;      // tiled ring: first day of this launch inside the slot
    // reqhgt < 0
    double* tgser;          // [N][tsteps]
    double* ddsum;          // [N]
    int32_t day0, ndays;
    int32_t total_days;  // days of the whole series (the time table's extent)
    int32_t need_pass2;  // 0: no requested output comes from pass 2 (Tz, tleaf, relhum, Rlwdown, Rlwup)
    int32_t need_tv;     // 0: no requested output comes from TVaboveground (cpp:2287-2303)
    // tiles of this launch: tile_list[ntiles_launch] (null: tiles 0 .. ntiles_launch-1; ntiles_launch <= 0: all)
    const int32_t* tile_list;
    int64_t ntiles_launch;
    // fast-clamp launches: tiles in which a canary tripped, redone by k_solve_fix for the launch's days
    int32_t* fix_count;
    int32_t* fix_list;      // [fix_cap]
    int32_t fix_cap;
    Globals g;
    // reqhgt < 0, streamed plan (launch_solve_bg_tiled): the other outputs go to the TILED ring as for reqhgt >= 0 and the
    // ground temperature Tg of day d of the launch to the block at tg_ring + tile * tg_tile_stride + d * ring_block_doubles,
    // lane order (ring_pos); 0 where the cell is not solved.  ddsum: added to as above, or null (not summed).  (Last: the
    // other instantiations read the fields above at the offsets they always had.)
    double* tg_ring;
    int64_t tg_tile_stride;
};
// A launch of a diagnostics plan (mcf_plan_diag_enable; k_solve_diag): the same description plus a second tiled ring with the
// output ring's geometry — the block of (tile, day d of the slot, slab s) at
//   dg_base + tile * dg_tile_stride + d * dg_day_stride + s * ring_block_doubles;
// dg_sel packs, 4 bits per diagnostic (mcf_diag), its slab (15 = not selected).  A type of its own: k_solve's argument block
// stays what it was.
struct DiagSolveArgs : SolveArgs {
    double* dg_base;
    int64_t dg_tile_stride, dg_day_stride;
    uint64_t dg_sel;
};

struct BelowArgs {
    int64_t N;
    int32_t tsteps, complete, hiy, per_cell_pointm;
    double reqhgt, mat;
    const double* cellflag_hgt;  // hgt [N] (NA test)
    const double* tg;            // [N][tsteps]
    const double* ddsum;         // [N]
    const double *Tgp, *Tbp;     // [tsteps] or [N][tsteps]; complete==0 only
    double* scratch;             // [N][2*ndays]
    double* tz;                  // [N][tsteps]
};

// ---- below ground, streamed through day chunks (mcf_plan_create_streamed; DESIGN.md "Below ground in day chunks") ----------
// Tbelowgroundv (cpp:1474-1539) of k_belowground, made from per-cell state of O(days) instead of the [N][tsteps] series.
// Per-cell state, every buffer [rows][N] (cell fastest):
//   ddsum [1]      sum of the damping depth DD over every solved step (the pre-pass or sweep 1), in k_solve's order
//   hsum  [1]      complete: Tg summed over the steps in step order (meanT of n >= tsteps), tail zeros included
//   dmean [ndays]  complete: the days' means (24-sums / 24); k_below_finish turns them into the circular n/24-day means y
//   wrap  [47]     complete: Tg of the series' last 47 steps (step tsteps - 47 + j; 0 past the last whole day)
//   prev  [47]     complete, sweep 2: Tg of the 47 steps in front of the chunk being transformed
constexpr int kBelowWin = 47;
constexpr int kBelowMaxDepths = 8;      // include/mcf.h MCF_MAX_DEPTHS
struct BelowStreamArgs {
    int64_t N;
    int32_t tsteps, ndays, complete, hiy;
    double reqhgt, mat;
    const double* hgt;           // [N] (the NA test of k_belowground)
    RingView tg;                 // the chunk's Tg: step 0 = the chunk's first step
    RingView tz;                 // the slot's Tz view (written), step 0 = the chunk's first step
    int32_t day0, ndays_chunk;   // the chunk: first day, whole days
    int32_t tail;                // 1: the chunk ends on the last whole day and the slot takes the tsteps % 24 steps behind it
    double* ddsum;
    double* hsum;
    double* dmean;               // [ndays][N]: daily means, after k_below_finish the circular means y
    double* ybuf;                // [ndays][N] scratch of k_below_finish
    double* wrap;                // [47][N]
    double* prev;                // [47][N]
    // complete == 0: the point model's Tg / Tbp — [tsteps] (vector forcing, step index absolute) or the chunk's [steps][N]
    // (array forcing, step index relative to the chunk)
    const double *Tgp, *Tbp;
    int32_t per_cell_pointm;
    // a day subset (mcf_plan_below_set_days): days[q] = the calendar day of subset position q, or null — every day, q itself.
    // With it the series Tbelowgroundv sees is the subset's days joined: tsteps = 24 x ndays, ndays = the subset's length,
    // day0 / ndays_chunk count subset positions, and position q's 24 steps lie at day days[q] - cal0 of the tg / tz views
    // (cal0: the calendar day at the views' day 0); the point model's series are read at the calendar day's own steps.
    const int32_t* days;
    int32_t cal0;
    // the depths of the launch (mcf_plan_below_set_depths; without a list: one, reqhgt).  Everything above is shared by them;
    // per depth d there is depth[d], a Tz slab (slab 0: tz; slab d > 0: the view tzx moved on by (d - 1) * tzx_stride — a
    // buffer beside the ring, [depth][slot][tile][day][block]), a row of circular means (row 0: ybuf; row d > 0: ybufx +
    // (d - 1) * ndays * N) and, complete == 0 with vector forcing, the point model's series Tbp + d * tbp_stride.  (Last:
    // k_below_acc / k_below_carry read the fields above where they were.)
    int32_t ndepths;
    double depth[kBelowMaxDepths];
    RingView tzx;
    int64_t tzx_stride;
    double* ybufx;
    int64_t tbp_stride;
};
// step k of the chunk, in the order of the series Tbelowgroundv sees -> step of the chunk's tg / tz views
__host__ __device__ inline int below_view_step(const BelowStreamArgs& a, int k) {
    if (!a.days) return k;
    const int q = k / 24;
    return (a.days[a.day0 + q] - a.cal0) * 24 + (k - 24 * q);
}
// complete = 0: ddsum += DD over days [day0, day0 + ndays_chunk) from the soil moisture alone (soil_spread, soil_ksoil,
// soil_damping: the functions pass 1 and 2 use), in k_solve's order.  Vector forcing reads the time table, array forcing the
// slot's tiled forcing ring (the chunk's days).
struct BelowDDArgs {
    int64_t N;
    const double* cellc;       // tile-major constant table
    int64_t ntiles_total;
    int32_t cpb;
    const int32_t* daylayer;   // or null
    const double* tt;          // vector forcing: [ndays][TF_COUNT][24]
    const double* af_base;     // array forcing: the chunk's first day in the slot's forcing ring; else null
    int64_t af_tile_stride, af_day_stride;
    int32_t day0, ndays;
    double* ddsum;
};
void launch_below_dd(const BelowDDArgs& a, hipStream_t s);
// sweep 1 (complete = 1): fold the chunk's Tg into hsum, dmean and wrap
void launch_below_acc(const BelowStreamArgs& a, hipStream_t s);
// after the last chunk of sweep 1 / the pre-pass: tail zeros into hsum and wrap, dmean -> y for the cells of 48 < n < tsteps
void launch_below_finish(const BelowStreamArgs& a, hipStream_t s);
// sweep 2 / the day-local transform: the chunk's Tz into the slot; then (complete) prev <- the chunk's last 47 steps
void launch_below_chunk(const BelowStreamArgs& a, hipStream_t s);

struct BioclimArgs {
    int64_t N;
    int32_t tsteps;
    RingView tz;           // Tz or tleaf, tsteps steps from step 0 of the slot
    RingView soilm;
    const int32_t *wetq, *dryq, *hotq, *colq;
    int32_t nwet, ndry, nhot, ncol;
    double* bio;           // [19][N]
};
void launch_bioclim(const BioclimArgs& a, hipStream_t s);
// The same nineteen values STREAMED (round 5): the solver runs in day chunks into a small ring and each chunk is folded into
// per-cell running state — sums, day extremes, quarter sums in the reference's index order (cpp:3245-3560) — so that nothing of
// size cells x steps is ever allocated.  State rows, [kBioStateRows][N]:
//   0 tz at step 0 (the NA test, cpp:3505)   1 bio1's running sum   2 bio2's sum of daily ranges   3..14 the twelve daily means
//   15 bio5's maximum   16 bio6's minimum   17..20 tz quarter sums   21 bio12's sum   22 / 23 soil moisture max / min
//   24 its sum over all steps   25..28 soil moisture quarter sums
constexpr int kBioStateRows = 29;
struct BioAccArgs {
    int64_t N;
    RingView tz, soilm;        // step 0 of the views = the chunk's first step
    int32_t day0, ndays;       // the chunk: absolute first day, whole days
    const int32_t* q[4];       // wettest / driest / hottest / coldest quarter's step indices, ascending (checked by the host)
    int32_t qlo[4], qhi[4];    // the entries that fall into this chunk
    double* state;
};
void launch_bioclim_acc(const BioAccArgs& a, hipStream_t s);
struct BioFinArgs {
    int64_t N;
    int32_t tsteps;
    const double* state;
    double* bio;               // [19][N]
    // the soil moisture series again for the variance's second pass (cpp:3391-3398): it is a function of the cell's constants and
    // the point model's soil moisture alone (soil_spread, cpp:1021-1032), made here with the very function the solver's lanes run
    const double* cellc;       // tile-major constant table
    int64_t ntiles_total;
    int32_t cpb;
    const int32_t* daylayer;   // or null
    const double* tt;          // time table [day][TF_COUNT][24]; null with coarse array forcing
    // coarse array forcing (cforce != null) has no such table: the point model's soil moisture of a cell at a step is the
    // bilinear tap of the resident coarse series, taken as the solver's lanes take it (CoarseTap, coarse_day_field)
    const double* cforce;      // the resident series [15][crows*ccols][tsteps]
    int64_t cstride;           // doubles from one of the fifteen to the next
    int32_t crows, ccols;
    const double *crowpos, *ccolpos;   // [rows], [cols]
    int32_t rows;
};
void launch_bioclim_fin(const BioFinArgs& a, hipStream_t s);
// ---- the streamed sink below ground at several depths (mcf_bioclim.hip; include/mcf.h mcf_runbioclim_depths) ----
// The 29 state rows split: rows 0..20 (kBioTempRows, the temperature rows above) once per depth, rows 21..28 (kBioMoistRows)
// once — below ground soilm is the solver's own and no depth changes it.  State [ndepths][kBioTempRows][N], then
// [kBioMoistRows][N]: bio12's sum, the maximum, the minimum, the sum over all steps, the four quarter sums.
constexpr int kBioTempRows = 21, kBioMoistRows = 8;
struct BioAccDepthsArgs {
    // the slot's soilm and depth 0's Tz (the slot's own variables): block of (tile, day of the chunk) at tile * ring_tile_stride
    // + day * ring_day_stride
    const double *soilm, *tz0;
    int64_t ring_tile_stride, ring_day_stride;
    // depth 1's slab beside the ring (null with one depth), depth d's (d - 1) * tzx_stride behind it
    const double* tzx;
    int64_t tzx_stride, tzx_tile_stride, tzx_day_stride;
    int64_t N, ntiles;
    int32_t cpb, ndepths;      // 16, 21, 32 or 42
    int32_t day0, ndays;       // the chunk, as in BioAccArgs; likewise q, qlo, qhi
    const int32_t* q[4];
    int32_t qlo[4], qhi[4];
    double* state;
};
// k_bioclim_acc's folds, term for term, over every depth's Tz (the grid's y) and, in a launch of its own, over soilm
void launch_bioclim_acc_depths(const BioAccDepthsArgs& a, hipStream_t s);
// The finish in two parts.  Moisture (BioFinArgs: `state` = the moisture rows, `bio` = [8][N] for bio12..bio19; the variance's
// second pass once, not per depth) with the NA rule read from `first`, depth 0's row 0.  Temperature: bio1..bio11 of every depth,
// state [ndepths][kBioTempRows][N] -> bio [ndepths][11][N], each depth under its own NA rule (cpp:3505-3506).
void launch_bioclim_fin_moist(const BioFinArgs& a, const double* first, hipStream_t s);
void launch_bioclim_fin_temp(const double* state, int64_t N, int ndepths, double* bio, hipStream_t s);
void launch_fill(double* p, int64_t n, double v, hipStream_t s);
// ---- period summaries (mcf_summary.hip; include/mcf.h "period summaries") ------------------------------------
// State [selected var][period][state row][N]: row 0 the running sum (R's NA_real_ once a NaN has been met: it carries the NA
// rule from call to call), then one row per selected statistic that needs one (row[stat], -1: none; row[MCF_STAT_MEAN] = 0).
struct SummaryAccArgs {
    const double* ring;          // the slot: block of (tile, day of the slot, slab) at tile * tile_stride + day * day_stride + slab * var_stride
    int64_t tile_stride, day_stride, var_stride;
    int64_t N, ntiles;
    int32_t cpb;                 // 16, 21, 32 or 42
    int32_t nsel;                // selected variables (the grid's y)
    int32_t slab[10];            // ring slab of each selected variable
    double threshold[10];        // HOURS_ABOVE: v > threshold
    int32_t nperiods, nrows;
    int32_t row[6];
    // [days of the plan]: the period of each day (-1: not counted) and the previous / next day of the same period (-1 / the
    // plan's day count: none) — the days of one period are folded together, in ascending order
    const int32_t *period_of_day, *prev_same, *next_same;
    int32_t day0, ndays;         // calendar days of the call ...
    int32_t slot_day0;           // ... and where the first of them lies in the slot
    double* state;
};
void launch_summary_acc(const SummaryAccArgs& a, hipStream_t s);
struct SummaryFinArgs {
    const double* state;         // the variable's [period][state row][N]
    int64_t N;
    int32_t nperiods, nrows;
    int32_t stat, row;           // the statistic and its state row
    const int32_t* days;         // [nperiods] counted days
    double* out;                 // [nperiods][N]
};
void launch_summary_fin(const SummaryFinArgs& a, hipStream_t s);
// init_codes: 4 bits per state row — 0: 0.0, 1: +inf, 2: -inf
void launch_summary_init(double* state, int64_t total, int64_t N, int nrows, uint32_t init_codes, hipStream_t s);
int summary_tiles_per_group(int cpb);
// The same fold over step-major planes (the snow plan's chunk series): value of (step k of the call, cell c) at
// series[i][k * N + c], step 0 = hour 0 of calendar day `day0`.  State, tables and the meaning of `row` as in SummaryAccArgs.
struct SummaryPlanesArgs {
    const double* series[5];     // the selected series, in selection order
    double threshold[5];
    int64_t N;
    int32_t nsel;                // selected series (the grid's y)
    int32_t nperiods, nrows;
    int32_t row[6];
    const int32_t *period_of_day, *prev_same, *next_same;
    int32_t day0, ndays;
    double* state;
};
void launch_summary_planes(const SummaryPlanesArgs& a, hipStream_t s);
// ---- series sink (mcf_series.hip; include/mcf.h "series sink") ------------------------------------------------
// Zone state [selected var][kSeriesRows][zone][step] of int64, a zone's steps contiguous: the fixed-point sum, the counted
// values (low 32 bits) and the bad ones (high 32 bits) in one word, the minimum and the maximum as order-preserving keys.
constexpr int kSeriesRows = 4;
enum { kSeriesSum = 0, kSeriesCount = 1, kSeriesMin = 2, kSeriesMax = 3 };
struct SeriesZonesArgs {
    const double* ring;          // the slot, addressed as SummaryAccArgs' ring
    int64_t tile_stride, day_stride, var_stride;
    int64_t N, ntiles;
    int32_t cpb;                 // 16, 21, 32 or 42
    int32_t nsel;                // selected variables (the grid's y)
    int32_t slab[10];            // ring slab of each selected variable
    const int32_t* zone;         // [N] labels, -1 .. nzones - 1
    int32_t nzones;
    int64_t steps;               // steps per zone in the state (whole days x 24)
    int32_t day0, ndays;         // days of the state this call folds ...
    int32_t slot_day0;           // ... and where the first of them lies in the slot
    long long* state;
};
// `workgroups`: persistent workgroups per selected variable (each walks many tile groups and flushes once per day)
void launch_series_zones(const SeriesZonesArgs& a, int workgroups, hipStream_t s);
// The same fold over step-major planes (the snow plan's chunk series): value of (step k of the call, cell c) at
// series[i][k * N + c], step 0 = hour 0 of state day `day0`; nsteps <= 24 * ndays steps exist (a shorter last day: the rest
// count as NaN).  State as above; (day0 + ndays) * 24 <= steps.
struct SeriesPlanesArgs {
    const double* series[5];     // the selected series, in selection order
    int64_t N;
    int32_t nsel;                // selected series (the grid's y)
    const int32_t* zone;         // [N], -1: in no zone
    int32_t nzones;
    int64_t steps, nsteps;
    int32_t day0, ndays;
    long long* state;
};
void launch_series_planes(const SeriesPlanesArgs& a, int workgroups, hipStream_t s);
// dst[(i * ncells + ci) * dst_steps + dst_step0 + k] = series[i][k * N + cells[ci]], k < nsteps, i < nsel
struct SeriesPointsPlanesArgs {
    const double* series[5];
    int64_t N;
    int32_t nsel;
    int64_t nsteps;
    const int64_t* cells;
    int64_t ncells;
    double* dst;
    int64_t dst_steps, dst_step0;
};
void launch_series_points_planes(const SeriesPointsPlanesArgs& a, hipStream_t s);
void launch_series_init(long long* state, int64_t nsel, int64_t nzones, int64_t steps, hipStream_t s);
// one statistic of one variable's state -> out[k + nsteps * z], k < nsteps; steps >= `steps` and steps of days with
// day_done[day] == 0 (null: every day is folded) are NA
void launch_series_fin(const long long* state, int nzones, int64_t steps, int64_t nsteps, const int32_t* day_done, int zstat,
                       double* out, hipStream_t s);
// dst[(i * ncells + ci) * dst_steps + dst_step0 + k] = src[i](cells[ci], step0 + k), k < nsteps, i < nsel
struct SeriesPointsArgs {
    RingView src[10];
    int32_t nsel;
    int64_t step0, nsteps;
    const int64_t* cells;
    int64_t ncells;
    double* dst;
    int64_t dst_steps, dst_step0;
};
void launch_series_points(const SeriesPointsArgs& a, hipStream_t s);
// dst[ci + ncells*k] = src(cells[ci], step0 + k), k < nsteps
void launch_gather_cells(const RingView& src, int64_t step0, int64_t nsteps, const int64_t* cells, int64_t ncells, double* dst,
                         hipStream_t s);
// dst[c + N*k] = src(c, step0 + k), k < nsteps: the reference's [rows, cols, steps] layout out of the tiled ring
void launch_untile(const RingView& src, int64_t step0, int64_t nsteps, double* dst, hipStream_t s);
// the other way (array forcing's upload path): dst(c, k) = src[c + N*k], k < nsteps, `dst` a tiled view (its base is written)
void launch_tile_series(const double* src, int64_t nsteps, const RingView& dst, hipStream_t s);
// per-cell maximum over time of the bilinearly interpolated coarse temperature [crows*ccols][tsteps]
// `force`: the 15 coarse slabs (stride elements apart); elevd / pkfac null without altitude correction
void launch_mxtc_coarse(const double* force, int64_t stride, int crows, int ccols, int tsteps, const double* rowpos,
                        const double* colpos, int64_t rows, int64_t N, int altcorrect, const double* elevd,
                        const double* pkfac, double* mx, hipStream_t s);
// the same maximum over the days with dayflag[d] != 0 only (device array [ndays]), started from -273.15
void launch_mxtc_coarse_days(const double* force, int64_t stride, int crows, int ccols, const int32_t* dayflag, int ndays,
                             const double* rowpos, const double* colpos, int64_t rows, int64_t N, int altcorrect,
                             const double* elevd, const double* pkfac, double* mx, hipStream_t s);
struct PackNcArgs {
    RingView src[10];        // each variable's slot view
    int64_t step0;           // first step (of the slot) of this launch
    double scale[10];
    int32_t fill_only[10];
    int32_t nv;
    int32_t missval;
    int64_t rows, cols;
    int64_t rec_words;       // record length in 4-byte words (2 + nv * rows * cols)
    int32_t* dst;            // first record
};
// at most 65535 / nv steps per launch
void launch_pack_nc(const PackNcArgs& a, int64_t nsteps, hipStream_t s);
// k_pack_nc_planes (mcf_ncpack.hip): the same records from step-major planes — series[k][step * N + c], N = rows * cols,
// c = row + rows * col (the snow plan's chunk series) — for up to 5 variables, none of them null
struct PackNcPlanesArgs {
    const double* series[5];
    int64_t step0;           // first step (of the planes) of this launch
    double scale[5];
    int32_t nv;
    int32_t missval;
    int64_t rows, cols;
    int64_t rec_words;       // record length in 4-byte words (2 + nv * rows * cols)
    int32_t* dst;            // first record
};
// at most 65535 / nv steps per launch
void launch_pack_nc_planes(const PackNcPlanesArgs& a, int64_t nsteps, hipStream_t s);
void launch_pack_transpose(const RingView& src, int64_t step0, int64_t rows, int64_t cols, int64_t nsteps, double scale,
                           int32_t* dst, hipStream_t s);
// out2: twi_scratch_doubles() doubles; [0] = sum, [1] = count on completion
void launch_twi_partial(const double* twi, int64_t n, double tfact, double* out2, hipStream_t s);
int twi_scratch_doubles();
void launch_cell_setup(const CellSetupArgs& a, hipStream_t s);
void launch_time_setup(const TimeSetupArgs& a, hipStream_t s);
void launch_date_setup(const DateSetupArgs& a, hipStream_t s);
void launch_mxtc(const double* tc, int64_t N, int nsteps, double* mx, hipStream_t s);
// fast: vector forcing, reqhgt >= 0 only — the min / max clamp variant followed by the fix-up kernel (needs fix_count /
// fix_list; the caller zeroes *fix_count on the stream first); the tiles and days handed over must be REGULAR
// soil_daily: every day of the launch carries kSoilDaily (vector forcing): the per cell-day soil state is computed once per
// tile and day and shared through LDS
void launch_solve(const SolveArgs& a, int cells_per_block, bool af, bool bg, bool fast, bool soil_daily, hipStream_t s);
// the same launch of a diagnostics plan (vector forcing, reqhgt >= 0): both rings are filled; `fast` / `soil_daily` as above,
// chosen by the caller exactly as for a plain launch of the same days, so that the ten outputs keep their bits
void launch_solve_diag(const DiagSolveArgs& a, int cells_per_block, bool fast, bool soil_daily, hipStream_t s);
// the same for an array-forcing plan (mcf_plan_diag_enable_array; k_solve_diag_af): fine arrays with the plan's tile size, or — a.crows
// > 0 — coarse arrays with 32-cell tiles, `coarse_lds` as launch_solve's flag says "taps through LDS"
void launch_solve_diag_af(const DiagSolveArgs& a, int cells_per_block, bool fast, bool coarse_lds, hipStream_t s);
// reqhgt < 0 of a streamed plan: the tiled-ring instantiation (SolveArgs tg_ring); the reference-form clamps, no shared soil state,
// exactly the arithmetic of launch_solve's bg instantiation
void launch_solve_bg_tiled(const SolveArgs& a, int cells_per_block, bool af, hipStream_t s);
// out[t] = 1 if every valid cell of tile t (cpb consecutive cells) is FL_REGULAR in all layers
void launch_tile_regular(const double* cellc, int64_t N, int layers, int cpb, uint8_t* out, hipStream_t s);
// A launch over a SUBSET of the cells (mcf_plan_run_days_cells): the wanted cells gathered into dense tiles of their own.
//   cells_class  cls[c] = 0 (need[c] == 0) / 1 (wanted, its tile tile_regular — launch_tile_regular's flags; null: all) / 2 (wanted, not);
//                blockcnt[2 b + k - 1] = cells of class k among cells 256 b .. 256 b + 255
//   cells_place  list[blockoff[2 b + k - 1] + rank of the cell among its block's class-k cells] = c  (ascending in each class)
//   gather_image the sub-tiles' images [layers][ntiles_sub][tile_image_doubles] from the plan's; list entry < 0: an all-zero
//                column (flags 0: not valid)
//   scatter_cells the sub-ring's values of `ndays` days to the cells' own places in a ring slot (`ring` = the slot's first day
//                to write); both rings [tile][day][variable][block], `day_doubles` = variables x block
void launch_cells_class(const uint8_t* need, const uint8_t* tile_regular, int64_t N, int cpb, uint8_t* cls, int32_t* blockcnt,
                        hipStream_t s);
void launch_cells_place(const uint8_t* cls, int64_t N, const int32_t* blockoff, int32_t* list, hipStream_t s);
void launch_gather_image(const int32_t* list, int64_t ntiles_sub, const double* src, int64_t ntiles_src, int layers, int cpb,
                         double* dst, hipStream_t s);
void launch_scatter_cells(const int32_t* list, int64_t ntiles_sub, const double* sub, int64_t sub_tile_stride, double* ring,
                          int64_t tile_stride, int64_t day_doubles, int cpb, int ndays, hipStream_t s);
void launch_belowground(const BelowArgs& a, hipStream_t s);
void launch_selftest_math(int kind, const double* x, const double* y, double* out, int64_t n, hipStream_t s);
// mcf_foliage.hip: `.foliageden` of n = cells x layers values at height z (hgt, pai -> leafden, paia), one lane each
void launch_foliage(const double* hgt, const double* pai, double z, int64_t n, double* leafden, double* paia, hipStream_t s);

// a plan's ring slot as another translation unit's kernels address it (mcf_snow.hip writes the snow-day microclimate into it):
// views of the requested variables (has[v] = 0: not requested), the plan's stream, its cell count and its device
}  // namespace mcf
struct mcf_plan;
namespace mcf {
int plan_ring_views(mcf_plan* p, int slot, RingView views[10], int32_t has[10], hipStream_t* stream, int64_t* N, int* device,
                    int* slot_days);

int cell_field_count();
void print_variant_stats();  // hook for the timing variants under tools/variants/ (empty in the shipped library)
int soil_daily_bit();        // kSoilDaily, likewise
int step_irregular_bit();   // kStepIrregular of the packed TF_IDX value (last time field)
int time_field_count();
double hf_pow02(double rs);

}  // namespace mcf
