// mcf_snowrun.hip — `runmicro(..., snow = TRUE)` with data.frame weather, device-resident, behind ONE C entry.
//
// The reference's `.runmicrosnow1` (R/internal.R:3581-3659) takes the whole year's snow series (`smod`, the arrays
// `.snowmodel1` returned, R/internal.R:2498-2619) from host memory, solves the days with a snow-free cell somewhere with the
// grid solver, the days with snow somewhere with gridmicrosnow1 (src/microclimfCpp.cpp:4894-5056), and merges by day.  Here
// the snow series never leave the device: the entry drives `.snowmodel1`'s chunk loop (include/mcf.h mcf_snowplan_*) and
// `.runmicrosnow1`'s two models in the solver's output ring — the sequence tools/bench_snow.py times for BASELINE configs[4]
// — and only the merged output (and, if asked for, the snow series) crosses PCIe.  Host orchestration only: every kernel is
// launched through the plan entry points of mcf_api.hip / mcf_snow.hip.
//
//   pass 1   per 5-day chunk: [checkpoint] -> snow surface (halo rows of neighbouring row blocks through host memory) ->
//            terrain refresh + tpi -> gridmodelsnow1 + redistribution -> applycpp3 max / min of totalSWE -> snowdaysfun
//            (src/microclimfCpp.cpp:5531-5550) -> running sum of the snow damping depth; a snow chunk's series stay in HBM
//            while room remains
//   between  gridmicrosnow1's set-up on the snow-day SUBSET of the caller's whole-series inputs (day subsetting here, what
//            `subsetpointmodel(micropoint, days = snowdays)` does in R), the solver's maximum temperature over the no-snow subset
//   pass 2   per chunk: restore + re-run the snow chunk unless its series were kept; the solver on the chunk's no-snow days at
//            their own place in the ring slot; k_microsnow_ring over it; the slot's merged days to the caller's arrays
//   sinks    besides the host arrays: period summaries (mcf_snowrun_summary_enable) — the snowpack's series folded
//            behind every chunk of pass 1, the merged days of every ring slot behind pass 2's snow-day kernel
//
// Below ground (the `_below` entries, reqhgt < 0): the block's solver plan is a streamed below-ground plan over the no-snow days
// (mcf_plan_create_streamed, mcf_plan_below_set_days) — Tbelowgroundv's running means see those days joined end to end, as the
// reference's solver does on the subset `.runmicrosnow1` hands it.  Between the passes the plan is prepared (complete = 1: one
// more sweep of the solver over the no-snow days); pass 2 runs each chunk's no-snow days for EVERY cell (a cell's ground
// temperature under today's snow feeds its means on later days: no tile or cell is left out), the chunk's Tz is made and the
// 47-step window carried, and only then the snow-day kernel merges its Tz and soilm into the same slot.
//
// Row blocks: the raster is cut into contiguous row blocks, block b on devices[b % n_devices], one host thread per device
// (mcf_rowblocks.hpp's worker pool): per chunk the blocks' snow surfaces meet in one whole-raster host array, the two raster-wide
// means and the per-step extremes of totalSWE are combined in block order.  One block = the single-device sequence, bit for bit.
// The snow model's own entries (mcf_snowmodel1 / 2, mcf_snowmodel1_multi, at the end) run the same chunk loop (snow_chunk).
//
// Array weather with the coarse arrays left coarse (mcf_runmicrosnow2_coarse, mcf_snowrun_create_coarse): one block
// whose snow plan expands a chunk's thirteen series and a run of snow days' nine microclimate series (k_coarse_hours over either
// argument struct) from resident coarse arrays, and whose solver plan interpolates its own (array_forcing == 2) — the same two passes, nothing of
// size cells x steps uploaded; the solver's temperature cap over the no-snow days from the resident series (mcf_plan_set_mxtc_days).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mcf.h"
#include "mcf_rowblocks.hpp"
#include "mcf_snow_plan.hpp"
#include "mcf_series_host.hpp"
#include "mcf_sinks_host.hpp"
#include "mcf_ncsink.hpp"

namespace mcf {   // mcf_api.hip
int summary_spec_check(const mcf_summary_spec* s, int64_t ndays, const int32_t* out_mask);
int plan_summary_fetch_pitched(mcf_plan* p, int32_t var, int32_t stat, double* host_dst, int64_t row_pitch);
int plan_summary_retable(mcf_plan* p, const int32_t* period_of_day);
int series_spec_check(const std::string& who, const mcf_series_spec* s, int64_t rows, int64_t cols, const int32_t* out_mask);
int plan_series_state(mcf_plan* p, int32_t var, int64_t* host_state, int32_t* day_done);
}

namespace {

using mcf::api_fail;
using mcf::Worker;

struct Block {
    int64_t r0 = 0, nr = 0;
    int device = 0;
    // the block's rows of the snow model's rasters (the snow plan uploads from dense arrays) and, pass 2, of gridmicrosnow1's
    mcf::HostCopies model_rows, micro_rows;
    std::vector<double> ext;                   // its rows (+ halos) of the current chunk's snow surface
    mcf_snowplan* sp = nullptr;
    mcf_plan* plan = nullptr;
    double s = 0, n = 0, ts = 0, tn = 0, twi_s = 0;
    int64_t twi_n = 0;
    std::vector<double> mx, cmx, mn, cmn;      // applycpp3 of the chunk just run
    std::vector<char> kept;                    // per chunk: its series stayed on the device
    mcf_grid_inputs gsub{};                    // the block's view of the solver's inputs (array weather: a chunk's forcing is uploaded from it)
    std::vector<uint8_t> skip;                 // pass 2: the tiles a run of days leaves out
    bool sum_on = false;                       // the solver plan's summary has been enabled (block_setup)
    // series sink: the block's rows of the caller's specs (mcf_series_host.hpp), and whether anything of them lies in the block
    mcf::SeriesBlockCut mcut, pcut;
    bool ser_micro = false, ser_pack = false;
};

// The raster in nb contiguous row blocks, block b (rows R*b/nb ..) on devs[b % nt] driven by worker b % nt, each with its snow
// plan (and, in a snow run, its solver plan): what the snow model entries and the snow run share.
struct SnowBlocks {
    int64_t R = 0, C = 0;
    int nb = 1, nt = 1;
    std::vector<int> devs;
    std::vector<Block> blocks;
    std::vector<double> surface;               // the whole raster's snow surface of the current chunk (nb > 1)
    double smean = 0, tmean = 0;               // the current chunk's two raster-wide means (nb > 1)
    // n_blocks <= 0: one block per device; never more blocks than rows
    void cut(int n_blocks) {
        nb = (int)std::max<int64_t>(1, std::min<int64_t>(n_blocks > 0 ? n_blocks : (int)devs.size(), R));
        nt = (int)std::min<size_t>(devs.size(), (size_t)nb);
        blocks.resize((size_t)nb);
        if (nb > 1) surface.assign((size_t)(R * C), 0.0);
    }
    // body(Block&) -> status for the calling worker's blocks (mcf::for_blocks)
    template <class B>
    void each_block(Worker& w, B&& body) { mcf::for_blocks(w, nb, nt, [&](int b) { return body(blocks[(size_t)b]); }); }
    ~SnowBlocks() {
        mcf::RestoreDevice restore;
        for (Block& k : blocks) {
            if (k.plan || k.sp) (void)hipSetDevice(k.device);
            if (k.plan) mcf_plan_destroy(k.plan);
            if (k.sp) mcf_snowplan_destroy(k.sp);
        }
    }
};

// coarse array weather as a snow plan's source (one block; the driver's inputs are co->drv): the plan expands its chunks from the
// resident coarse arrays, pointm$umu goes to umu_out.  Empty: the weather is the driver's own
struct CoarseSource {
    const mcf_snowcoarse_in* co;
    double* umu_out;
};
// block b's snow plan on `device`: one block reads the caller's arrays in place, more gather their rows
int block_snowplan(SnowBlocks& sb, int b, int device, const mcf_snowdriver_in& snow, const CoarseSource& coarse = {}) {
    Block& k = sb.blocks[(size_t)b];
    const int64_t R = sb.R, C = sb.C;
    k.device = device;
    k.r0 = R * b / sb.nb; k.nr = R * (b + 1) / sb.nb - k.r0;
    if (coarse.co) return mcf::snowplan_create_coarse(coarse.co, coarse.umu_out, device, &k.sp);
    mcf_snowdriver_in bi = snow;
    mcf::model_rasters_of_block(bi, sb.nb > 1 ? &k.model_rows : nullptr, R, C, k.r0, k.nr);
    return mcf_snowplan_create(&bi, k.r0, R, k.device, &k.sp);
}

// One chunk of the snow model over every block.  Collective: every worker calls it for the same chunk.
// One block: the sequence of mcf_snowmodel1 (no host copy of the surface; the raster-wide surface mean only where .tpicalc's
// raster-mean branch reads it — mcf_snowplan_prepare_chunk ignores it otherwise).  More blocks: three phases separated by the
// workers' barrier (the phases of snow.py snowmodel1_chunks_tiled, where ranks exchange the same things over RCCL):
//   1  every block writes its rows of the surface into one whole-raster array and reports its (sum, count)
//   2  every block takes its rows plus halo out of that array, refreshes terrain + tpi, reports tpic's (sum, count)
//   3  every block runs the chunk with the raster-wide tpic mean
// Partial sums are added in block order, so a run is reproducible for a given n_blocks; against the one-block run the two
// means differ in their last bits (another summation tree), like route 1's.
// out (optional): the caller's whole-series snow arrays — a block's chunk goes straight into its rows through the row pitch; the
// steps no chunk covers become NA behind the last chunk.
void snow_chunk(SnowBlocks& sb, Worker& w, int ch, const mcf_snowdriver_out* out) {
    const int nb = sb.nb;
    const int64_t R = sb.R, C = sb.C;
    auto block_out = [&](const Block& k) {
        mcf_snowdriver_out bo{};
        if (out) {
            bo = *out;
            double** const bop[5] = {&bo.Tc, &bo.Tg, &bo.groundsnowdepth, &bo.totalSWE, &bo.snowden};
            for (double** q : bop) if (*q) *q += k.r0;
        }
        return bo;
    };
    if (nb == 1) {
        if (w.t == 0) w.guarded([&] {
            Block& k = sb.blocks[0];
            int32_t af = 1;
            double mean = 0.0, s = 0, n = 0;
            int rc = mcf_snowplan_chunk_af(k.sp, ch, &af);
            if (!rc && !((double)af < std::min(R, C) / 2.0)) {
                rc = mcf_snowplan_surface_partial(k.sp, &s, &n);
                mean = s / n;
            }
            if (!rc) rc = mcf_snowplan_prepare_chunk(k.sp, ch, nullptr, 0, 0, mean, &s, &n);
            if (!rc) { const mcf_snowdriver_out bo = block_out(k); rc = mcf_snowplan_run_chunk_pitched(k.sp, ch, s / n, &bo, R); }
            if (rc) w.fail(rc);
        });
    } else {
        sb.each_block(w, [&](Block& k) -> int {              // ---- phase 1: the surface
            k.ext.resize((size_t)(k.nr * C));
            int rc = mcf_snowplan_surface(k.sp, k.ext.data());
            if (!rc) rc = mcf_snowplan_surface_partial(k.sp, &k.s, &k.n);
            if (!rc) mcf::scatter_rows(sb.surface.data(), k.ext.data(), R, C, k.r0, k.nr);
            return rc;
        });
        mcf::reduce_on_first(w, [&] {
            double s = 0, n = 0;
            for (const Block& k : sb.blocks) { s += k.s; n += k.n; }
            sb.smean = s / n;
        });
        sb.each_block(w, [&](Block& k) -> int {              // ---- phase 2: halos, terrain, tpi
            int32_t af = 1;
            if (const int rc = mcf_snowplan_chunk_af(k.sp, ch, &af)) return rc;
            // what prepare_chunk asks for at most, or every row up to the raster edge
            const int64_t want = mcf::snowplan_halo_rows(k.sp, af);
            const int64_t hn = std::min(want, k.r0), hs = std::min(want, R - k.r0 - k.nr), RB = hn + k.nr + hs;
            mcf::gather_rows(k.ext, sb.surface.data(), R, C, k.r0 - hn, RB);
            return mcf_snowplan_prepare_chunk(k.sp, ch, (hn || hs) ? k.ext.data() : nullptr, (int32_t)hn, (int32_t)hs, sb.smean, &k.ts, &k.tn);
        });
        mcf::reduce_on_first(w, [&] {
            double s = 0, n = 0;
            for (const Block& k : sb.blocks) { s += k.ts; n += k.tn; }
            sb.tmean = s / n;
        });
        sb.each_block(w, [&](Block& k) -> int {              // ---- phase 3: the chunk
            const mcf_snowdriver_out bo = block_out(k);
            return mcf_snowplan_run_chunk_pitched(k.sp, ch, sb.tmean, &bo, R);
        });
    }
    w.wait();
}

// ---- the series sink over the blocks (include/mcf.h "Row blocks") ------------------------------------------------
// a block's snow plan takes its rows of the snowpack's spec
int block_pack_series(SnowBlocks& sb, Block& k, const mcf_snowpack_series_spec* spec) {
    k.pcut.cut(spec->npoints, spec->cells, spec->nzones, spec->zone, sb.R, sb.C, k.r0, k.nr);
    if (k.pcut.empty(spec->nzones)) return MCF_OK;
    mcf_snowpack_series_spec bs = *spec;
    bs.npoints = (int64_t)k.pcut.cells.size(); bs.cells = k.pcut.cells.data(); bs.zone = k.pcut.zone.data();
    const int rc = mcf_snowplan_series_enable(k.sp, &bs);
    k.ser_pack = !rc;
    return rc;
}
// [T, npoints] of one series / variable: every block's points into their places of the caller's list.  pack: the snow plans'
// sink, else the solver plans'
int blocks_fetch_points(SnowBlocks& sb, bool pack, int32_t var, int64_t T, double* dst) {
    mcf::RestoreDevice restore;
    std::vector<double> tmp;
    for (Block& k : sb.blocks) {
        const mcf::SeriesBlockCut& cut = pack ? k.pcut : k.mcut;
        if (!(pack ? k.ser_pack : k.ser_micro) || cut.where.empty()) continue;
        tmp.resize((size_t)(T * (int64_t)cut.where.size()));
        const int rc = pack ? mcf_snowplan_series_fetch_points(k.sp, var, tmp.data()) : mcf_plan_series_fetch_points(k.plan, var, tmp.data());
        if (rc) return rc;
        if (!pack)
            if (const int rcs = mcf_plan_sync(k.plan)) return rcs;
        for (size_t i = 0; i < cut.where.size(); ++i) memcpy(dst + cut.where[i] * T, tmp.data() + (int64_t)i * T, (size_t)T * 8);
    }
    return MCF_OK;
}
// [T, nzones] of one statistic: the blocks' states combined, finished once.  steps: whole days x 24
int blocks_fetch_zones(SnowBlocks& sb, bool pack, int32_t var, int32_t nzones, int64_t steps, int64_t T, int32_t zstat, double* dst) {
    mcf::RestoreDevice restore;
    const size_t n = (size_t)((int64_t)mcf::kSeriesStateRows * nzones * steps);
    std::vector<int64_t> state(std::max<size_t>(n, 1)), part(std::max<size_t>(n, 1));
    std::vector<int32_t> done((size_t)std::max<int64_t>(steps / 24, 1), 0);
    mcf::series_state_init(state.data(), nzones, steps);
    for (Block& k : sb.blocks) {
        if (!(pack ? k.ser_pack : k.ser_micro)) continue;
        const int rc = pack ? mcf::snowplan_series_state(k.sp, var, part.data(), done.data())      // (every block has folded the same days)
                            : mcf::plan_series_state(k.plan, var, part.data(), done.data());
        if (rc) return rc;
        mcf::series_state_merge(state.data(), part.data(), nzones, steps);
    }
    mcf::series_state_finish(state.data(), nzones, steps, T, done.data(), zstat, dst);
    return MCF_OK;
}

}  // namespace

struct mcf_snowrun : SnowBlocks {
    int64_t T = 0;
    int ndays = 0, chunk_days = 5, nchunks = 0;
    mcf_grid_inputs grid{};
    mcf_options opt{};
    mcf_snowdriver_in snow{};
    std::vector<int32_t> snowday, nosnowday;   // [ndays]
    bool pass1_done = false;
    bool af = false;                           // array weather: `.snowmodel2` + `.runmicrosnow2` (mcf_runmicrosnow2)
    bool below = false;                        // the `_below` entries: reqhgt < 0, a streamed solver plan over the no-snow days
    // mcf_runmicrosnow2_coarse: array weather with the coarse arrays left coarse — the snow plan expands its chunks and the
    // microclimate's snow days itself, the solver plan interpolates (array_forcing == 2); umu_out: pass 1's pointm$umu, or null
    bool coarse = false;
    double* umu_out = nullptr;
    bool layers_set = false;                   // mcf_snowrun_set_day_layers since the last pass 1 (which restores the plans' own table)
    int64_t keep_reserve = (int64_t)8 << 30;
    // A run is one simulated period on fresh plans: the device memory a kept chunk needs would have to be ALLOCATED for it (5 GB per
    // chunk of a 1024 x 1024 raster: 0.1 s, measured 3 s of a 6 s call) where re-running the chunk in pass 2 takes 3.5 ms — chunks are
    // kept only on request (MCF_SNOWRUN_KEEP=1); the stepwise API's pool across years (tools/bench_snow.py) is where keeping pays
    bool keep = false;
    // what pass 2 did not have to do (mcf_snowrun_stats)
    std::atomic<int64_t> st_tile_days{0}, st_tile_days_left_out{0}, st_chunks_kept{0}, st_chunks_rerun{0};
    // period summaries (mcf_snowrun_summary_enable): the caller's specs with their tables copied, the table of the current year
    // (the caller's with the days of neither class taken out)
    bool sum_micro = false, sum_pack = false, pass1_ever = false, pass2_done = false;
    mcf_summary_spec mspec{};
    mcf_snowpack_summary_spec pspec{};
    std::vector<int32_t> mtable, ptable, mtable_year;
    uint32_t pack_bits = 0;
    // series sink (mcf_snowrun_series_enable): the caller's specs with their cells and labels copied
    bool ser_micro = false, ser_pack = false;
    mcf_series_spec sspec{};
    mcf_snowpack_series_spec spspec{};
    std::vector<int64_t> scells, spcells;
    std::vector<int32_t> szone, spzone;
    uint32_t ser_pack_bits = 0;
    // netCDF sink (mcf_snowrun_nc_enable): the caller's files, not owned — the merged outputs' (pass 2) and the snowpack's (pass 1)
    mcf_ncfile *nc_micro = nullptr, *nc_pack = nullptr;
    uint32_t nc_pack_bits = 0;
};
// a run on its way to the caller, or a one-call entry's own: destroyed on every path that does not release() it
struct SnowRunDestroy { void operator()(mcf_snowrun* h) const { mcf_snowrun_destroy(h); } };
using SnowRunHolder = std::unique_ptr<mcf_snowrun, SnowRunDestroy>;

namespace {

// snowdaysfun, src/microclimfCpp.cpp:5531-5550: a snow day has snow somewhere in some hour (max > 0), a no-snow day a
// snow-free cell in some hour (min == 0); NaN compares false both ways
void snowdays_of(const double* mx, const double* mn, int nd, int32_t* snow, int32_t* nosnow) {
    for (int d = 0; d < nd; ++d) {
        int s = 0, n = 0;
        for (int hh = 0; hh < 24; ++hh) {
            s |= mx[d * 24 + hh] > 0.0;
            n |= mn[d * 24 + hh] == 0.0;
        }
        snow[d] = s; nosnow[d] = n;
    }
}

int check_create(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu, bool below) {
    if (!in || !opt || !in->grid || !in->snow) return mcf::api_fail(MCF_ERR_ARG, "null snow-run argument");
    const mcf_grid_inputs& g = *in->grid;
    const mcf_snow_inputs& sb = in->snow->base;
    // Array weather (round 5): `.snowmodel2`'s loop + `.runmicrosnow2` (R/internal.R:2950-3008, 3661-3745) — the solver's and the snow
    // model's weather as arrays at the raster's resolution, what runmicro2Cpp / gridmodelsnow2 / gridmicrosnow2 take.  Both sides in
    // the same geometry; one block (a chunk's slices are uploaded from the caller's whole-raster arrays as the loop reaches them).
    if ((g.array_forcing != 0) != (sb.array_forcing != 0))
        return mcf::api_fail(MCF_ERR_ARG, "snow run: the solver's and the snow model's weather differ in geometry (data.frame / array)");
    if (g.array_forcing == 2)
        return mcf::api_fail(MCF_ERR_ARG, "snow run: coarse array forcing is not taken here (mcf_runmicrosnow2_coarse / mcf_snowrun_create_coarse "
                                          "keep the coarse arrays coarse; or resample to the raster first, as `.snowmodel2` does)");
    if (g.array_forcing && mu && (mu->n_blocks > 1 || mu->n_devices > 1))
        return mcf::api_fail(MCF_ERR_ARG, "snow run, array weather: one block on one device");
    // Time-varying vegetation (round 5).  `.runmicronosnow` sends a layered `vegp` to `.runmodel3Cpp` on the no-snow-day SUBSET
    // (R/internal.R:3333-3342), which deals the subset's days to layers by `.sortvegp(vegp, "C", n, subs)` — the layer a step has
    // in the WHOLE series (round(seq(0.50001, dmx + 0.5, length.out = n))[subs], the day's mode, R/internal.R:252-270) — and
    // renumbers the layers it uses (:1391-1399).  Here a no-snow day runs with the layer the whole-series table gives it: the
    // solver plan takes the caller's whole-series layer table (lyr_st / lyr_ed in whole-series steps, as mcf_runmicro3) and the
    // days run at their own place in it.  That is the reference's dealing as long as the subset's two lists of layers agree —
    // `.sortvegp` cuts the arrays to the layers some STEP of the subset has, the table has a row per layer that is some DAY's mode,
    // and the solver walks the cut arrays by row: a layer that keeps a few steps of the subset without being a day's mode puts
    // every later row one layer early.  A caller that wants that dealing passes it between the passes
    // (mcf_snowrun_set_day_layers; frontend.subset_day_layers forms it).  The snow model's and gridmicrosnow1's rasters are
    // `.sortl` / `.sortl2` means — single-layer — either way.
    if (g.veg_layers > 1 && (!g.lyr_st || !g.lyr_ed))
        return mcf::api_fail(MCF_ERR_ARG, "mcf_runmicrosnow1: layered vegetation needs lyr_st / lyr_ed (whole-series steps)");
    if (opt->reqhgt < 0 && !below)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_runmicrosnow1: reqhgt < 0 takes the below-ground entries (mcf_runmicrosnow1_below, "
                                          "mcf_runmicrosnow1_below_multi, mcf_snowrun_create_below), which stream Tbelowgroundv over the "
                                          "no-snow days");
    if (below && !(opt->reqhgt < 0))
        return mcf::api_fail(MCF_ERR_ARG, "mcf_runmicrosnow1_below: the below-ground entries need reqhgt < 0 (reqhgt >= 0: mcf_runmicrosnow1)");
    if (below && g.array_forcing)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_runmicrosnow1_below: array weather below ground is not supported (data.frame weather only)");
    if (g.rows <= 0 || g.cols <= 0 || g.tsteps < 24) return mcf::api_fail(MCF_ERR_ARG, "bad dimensions");
    if (sb.rows != g.rows || sb.cols != g.cols || sb.tsteps != g.tsteps)
        return mcf::api_fail(MCF_ERR_ARG, "mcf_runmicrosnow1: the solver's and the snow model's inputs differ in shape");
    if (g.row_pitch > 0 && g.row_pitch != g.rows) return mcf::api_fail(MCF_ERR_ARG, "mcf_runmicrosnow1 takes dense rasters");
    if (!in->snow->dtm || !mcf::model_rasters_given(sb))
        return mcf::api_fail(MCF_ERR_ARG, "null input: a snow-model raster");
    if (!g.clim.tc) return mcf::api_fail(MCF_ERR_ARG, "null input: climdata$temp");
    if (in->snow->chunk_steps != 0 && in->snow->chunk_steps % 24)
        return mcf::api_fail(MCF_ERR_ARG, "snow driver: chunk_steps must be whole days");
    return MCF_OK;
}

// the coarse run's arguments, each refusal before a device is touched and under the entry's name
int check_create_coarse(const mcf_microsnow_coarse_in* in, const mcf_options* opt, const mcf_multi* mu, const char* entry) {
    const std::string e = std::string(entry) + ": ";
    auto fail = [&](const std::string& m) { return mcf::api_fail(MCF_ERR_ARG, e + m); };
    if (!in) return fail("null argument: in");
    if (!opt) return fail("null argument: opt");
    if (!in->grid) return fail("null argument: in->grid");
    if (!in->snow) return fail("null argument: in->snow");
    if (!in->micro) return fail("null argument: in->micro");
    const mcf_grid_inputs& g = *in->grid;
    const mcf_snowcoarse_in& s = *in->snow;
    const mcf_microcoarse_in& m = *in->micro;
    if (g.array_forcing != 2) return fail("grid->array_forcing must be 2 (coarse array forcing; arrays at the raster's resolution: mcf_runmicrosnow2)");
    if (opt->reqhgt < 0) return fail("reqhgt < 0 is not supported with coarse array weather");
    if (mu && (mu->n_blocks > 1 || mu->n_devices > 1)) return fail("one block on one device");
    int rc;
    if ((rc = mcf::snowcoarse_checks(in->snow, true, entry, nullptr))) return rc;
    if ((rc = mcf::microcoarse_checks(in->micro, entry))) return rc;
    const mcf_snow_inputs& sb = s.drv.base;
    if (g.rows != sb.rows || g.cols != sb.cols || g.tsteps != sb.tsteps || m.rows != sb.rows || m.cols != sb.cols || m.tsteps != sb.tsteps)
        return fail("grid, snow and micro differ in rows / cols / tsteps");
    if (g.tsteps < 24) return fail("tsteps: at least one day");
    if (g.coarse_rows != s.coarse_rows || g.coarse_cols != s.coarse_cols || m.coarse_rows != s.coarse_rows || m.coarse_cols != s.coarse_cols)
        return fail("grid, snow and micro differ in coarse_rows / coarse_cols");
    if (g.coarse_altcorrect != s.altcorrect || m.altcorrect != s.altcorrect) return fail("grid, snow and micro differ in altcorrect");
    if (!g.coarse_rowpos || !g.coarse_colpos) return fail("null input: grid coarse_rowpos / coarse_colpos");
    if (memcmp(g.coarse_rowpos, s.coarse_rowpos, (size_t)sb.rows * 8) || memcmp(m.coarse_rowpos, s.coarse_rowpos, (size_t)sb.rows * 8) ||
        memcmp(g.coarse_colpos, s.coarse_colpos, (size_t)sb.cols * 8) || memcmp(m.coarse_colpos, s.coarse_colpos, (size_t)sb.cols * 8))
        return fail("grid, snow and micro differ in coarse_rowpos / coarse_colpos");
    if (g.row_pitch > 0 && g.row_pitch != g.rows) return fail("dense rasters are taken (row_pitch)");
    if (g.veg_layers > 1 && (!g.lyr_st || !g.lyr_ed)) return fail("layered vegetation needs lyr_st / lyr_ed (whole-series steps)");
    return MCF_OK;
}

}  // namespace

// co: the coarse run (mcf_snowrun_create_coarse, which has checked its arguments) — `in` is then null
static int snowrun_create(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu, bool below, mcf_snowrun** out,
                          const mcf_microsnow_coarse_in* co = nullptr, double* umu_out = nullptr) {
    try {
        if (!out) return api_fail(MCF_ERR_ARG, "null snow-run argument");
        int rc = co ? MCF_OK : check_create(in, opt, mu, below);
        if (rc) return rc;
        mcf_snowrun* h = new mcf_snowrun();
        SnowRunHolder holder(h);
        h->below = below;
        h->coarse = co != nullptr; h->umu_out = umu_out;
        if ((rc = mcf::device_list(mu, opt->device, &h->devs))) return rc;
        h->grid = co ? *co->grid : *in->grid; h->opt = *opt; h->snow = co ? co->snow->drv : *in->snow;
        h->af = h->grid.array_forcing != 0;
        const int64_t R = h->R = h->grid.rows;
        h->C = h->grid.cols;
        h->T = h->grid.tsteps;
        h->ndays = (int)(h->T / 24);
        const int chunk = h->snow.chunk_steps > 0 ? h->snow.chunk_steps : 120;
        h->chunk_days = chunk / 24;
        h->nchunks = std::max(1, (int)(h->T / chunk));          // `for (day in 1:n5days)`, R/internal.R:2553-2565
        h->cut(h->af ? 1 : mu ? mu->n_blocks : 0);
        h->snowday.assign((size_t)std::max(h->ndays, h->nchunks * h->chunk_days), 0);
        h->nosnowday.assign(h->snowday.size(), 0);
        if (const char* e = getenv("MCF_SNOW_KEEP_RESERVE_GB")) h->keep_reserve = (int64_t)(atof(e) * 1073741824.0);
        h->keep = getenv("MCF_SNOWRUN_KEEP") != nullptr;
        rc = mcf::run_workers(h->nt, [&](Worker& w) {
            mcf::for_blocks(w, h->nb, h->nt, [&](int b) -> int {
                Block& k = h->blocks[(size_t)b];
                // (the coarse run: one block, whose snow plan expands its chunks, and the microclimate's snow days, from coarse arrays)
                int rc2 = block_snowplan(*h, b, h->devs[(size_t)w.t], h->snow, {co ? co->snow : nullptr, umu_out});
                if (!rc2 && co) rc2 = mcf::snowplan_micro_attach_coarse(k.sp, co->micro);
                if (rc2) return rc2;
                // ---- ... and its solver plan: the caller's arrays read in place through the row pitch
                k.gsub = mcf::narrow_rows(h->grid, k.r0, k.nr, R);
                mcf_options o = h->opt;
                o.device = k.device;
                rc2 = below ? mcf_plan_create_streamed(&k.gsub, &o, h->chunk_days, 2, &k.plan)
                            : mcf_plan_create(&k.gsub, &o, h->chunk_days, 2, &k.plan);
                if (!rc2 && h->nb > 1) rc2 = mcf_plan_twi_partial(k.plan, &k.twi_s, &k.twi_n);
                if (!rc2) k.kept.assign((size_t)h->nchunks, 0);
                return rc2;
            });
            w.wait();
            // the solver's one global reduction (src/microclimfCpp.cpp:993-1004): partial sums in block order, by every worker
            if (h->nb > 1) {
                double s = 0; int64_t n = 0;
                for (const Block& k : h->blocks) { s += k.twi_s; n += k.twi_n; }
                h->each_block(w, [&](Block& k) { return mcf_plan_set_twi_mean(k.plan, s / (double)n); });
            }
        });
        if (rc) return rc;
        *out = holder.release();
        return MCF_OK;
    } catch (const std::exception& e) {
        return api_fail(MCF_ERR_NOMEM, std::string("mcf_snowrun_create: ") + e.what());
    }
}

extern "C" int mcf_snowrun_create(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu, mcf_snowrun** out) {
    return snowrun_create(in, opt, mu, false, out);
}
extern "C" int mcf_snowrun_create_below(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu, mcf_snowrun** out) {
    return snowrun_create(in, opt, mu, true, out);
}

extern "C" void mcf_snowrun_destroy(mcf_snowrun* h) { delete h; }

// Pass 1's snow chunks stay in device memory for pass 2, up to `bytes` in all (shared out among the row blocks by their rows);
// 0 switches keeping off.  The sets are allocated as pass 1 first needs them and POOLED in the handle's snow plans: a handle that
// runs a second period (mcf_snowrun_pass1 again) allocates nothing — where allocating 10 GB costs more than re-running the chunk
// (the struct's comment), keeping pays from the second period on, or on the first when the caller wants `smod` anyway.
extern "C" int mcf_snowrun_keep(mcf_snowrun* h, int64_t bytes) {
    if (!h) return api_fail(MCF_ERR_ARG, "null snow run");
    if (bytes < 0) return api_fail(MCF_ERR_ARG, "mcf_snowrun_keep: bytes >= 0");
    h->keep = bytes > 0;
    for (Block& k : h->blocks) {
        const int rc = mcf_snowplan_set_keep_budget(k.sp, bytes > 0 ? (int64_t)((double)bytes * (double)k.nr / (double)h->R) : 0);
        if (rc) return rc;
    }
    return MCF_OK;
}

extern "C" int32_t mcf_snowrun_days(const mcf_snowrun* h) { return h ? h->ndays : 0; }
// between the passes: every block's solver plan takes this day -> layer map (include/mcf.h)
extern "C" int mcf_snowrun_set_day_layers(mcf_snowrun* h, const int32_t* layer_of_day, int32_t ndays) {
    if (!h || !layer_of_day) return api_fail(MCF_ERR_ARG, "mcf_snowrun_set_day_layers: null argument");
    if (ndays != h->ndays) return api_fail(MCF_ERR_ARG, "mcf_snowrun_set_day_layers: one entry per day of the run");
    if (!h->pass1_done || h->pass2_done)
        return api_fail(MCF_ERR_STATE, "mcf_snowrun_set_day_layers: between mcf_snowrun_pass1 (which gives the no-snow days) and mcf_snowrun_pass2");
    mcf::RestoreDevice restore;
    for (Block& k : h->blocks)
        if (const int rc = mcf_plan_set_day_layers(k.plan, layer_of_day, ndays)) return rc;
    h->layers_set = true;
    return MCF_OK;
}
// between the passes: days that are no-snow days only leave the run's classes (include/mcf.h)
extern "C" int mcf_snowrun_drop_days(mcf_snowrun* h, const int32_t* drop, int32_t ndays) {
    const std::string w = "mcf_snowrun_drop_days: ";
    if (!h || !drop) return api_fail(MCF_ERR_ARG, w + "null argument");
    if (ndays != h->ndays) return api_fail(MCF_ERR_ARG, w + "one entry per day of the run");
    if (!h->pass1_done || h->pass2_done) return api_fail(MCF_ERR_STATE, w + "between mcf_snowrun_pass1 (which gives the day classes) and mcf_snowrun_pass2");
    for (int d = 0; d < ndays; ++d)
        if (drop[d] && h->snowday[(size_t)d])
            return api_fail(MCF_ERR_ARG, w + "day " + std::to_string(d) + " is a snow day: pass 1 has folded it into the snow model's means, only a day of the solver alone can be left out");
    for (int d = 0; d < ndays; ++d)
        if (drop[d]) h->nosnowday[(size_t)d] = 0;
    return MCF_OK;
}
extern "C" int mcf_snowrun_stats(const mcf_snowrun* h, int64_t stats[4]) {
    if (!h || !stats) return api_fail(MCF_ERR_ARG, "null argument");
    stats[0] = h->st_tile_days; stats[1] = h->st_tile_days_left_out; stats[2] = h->st_chunks_kept; stats[3] = h->st_chunks_rerun;
    return MCF_OK;
}

extern "C" int mcf_snowrun_pass1(mcf_snowrun* h, const mcf_snowdriver_out* smod, int32_t* snowday, int32_t* nosnowday) {
    if (!h) return api_fail(MCF_ERR_ARG, "null snow run");
    try {
        const int cd = h->chunk_days, ns = cd * 24;
        std::fill(h->snowday.begin(), h->snowday.end(), 0);
        std::fill(h->nosnowday.begin(), h->nosnowday.end(), 0);
        h->pass1_done = false;
        h->pass1_ever = true;
        h->pass2_done = false;
        const int rc = mcf::run_workers(h->nt, [&](Worker& w) {
            h->each_block(w, [&](Block& k) -> int {
                int rc2 = mcf_snowplan_reset(k.sp);
                if (!rc2 && h->layers_set) rc2 = mcf_plan_set_day_layers(k.plan, nullptr, h->ndays);      // (a period's map is its own)
                if (h->coarse) mcf::snowplan_coarse_umu_out(k.sp, h->umu_out);      // (pass 1 hands pointm$umu out, pass 2's re-runs do not)
                if (!rc2 && h->sum_pack) rc2 = mcf_snowplan_summary_reset(k.sp);      // (a second year starts the summaries over)
                if (!rc2 && k.ser_pack) rc2 = mcf_snowplan_series_reset(k.sp);        // (and the series)
                if (!rc2 && k.ser_micro) rc2 = mcf_plan_series_reset(k.plan);
                if (!rc2) rc2 = mcf_snowplan_release_kept(k.sp);
                if (!rc2) std::fill(k.kept.begin(), k.kept.end(), 0);
                return rc2;
            });
            w.wait();
            for (int ch = 0; ch < h->nchunks; ++ch) {
                h->each_block(w, [&](Block& k) -> int {
                    int rc2 = mcf_snowplan_checkpoint(k.sp, ch);      // pass 2 starts any chunk from here
                    // a chunk that could not stay in HBM is re-run by pass 2 if it holds a snow day: unless the caller wants the snow
                    // series, pass 1 writes only what it reads itself of such a chunk (totalSWE, density: mcf_snowplan_set_series)
                    int32_t room = 0;
                    if (!rc2 && h->keep) rc2 = mcf_snowplan_can_keep(k.sp, h->keep_reserve, &room);
                    if (!rc2) rc2 = mcf_snowplan_set_series(k.sp, (room || smod) ? 31u : (4u | 16u | h->pack_bits | h->ser_pack_bits | h->nc_pack_bits));
                    return rc2;
                });
                snow_chunk(*h, w, ch, smod);
                h->each_block(w, [&](Block& k) -> int {              // applycpp3 max / min of totalSWE
                    k.mx.assign((size_t)ns, 0.0); k.cmx.assign((size_t)ns, 0.0); k.mn.assign((size_t)ns, 0.0); k.cmn.assign((size_t)ns, 0.0);
                    int rc2 = mcf_snowplan_apply3(k.sp, ch, MCF_APPLY_MAX, k.mx.data(), k.cmx.data());
                    if (!rc2) rc2 = mcf_snowplan_apply3(k.sp, ch, MCF_APPLY_MIN, k.mn.data(), k.cmn.data());
                    // the snowpack's summaries: from the series where they lie, before keep_chunk hands the buffers over
                    if (!rc2 && h->sum_pack) rc2 = mcf_snowplan_summary_accumulate(k.sp, ch);
                    if (!rc2 && k.ser_pack) rc2 = mcf_snowplan_series_accumulate(k.sp, ch);
                    if (!rc2 && h->nc_pack) rc2 = mcf_snowplan_nc_write(k.sp, h->nc_pack, ch, k.r0);      // (its strips of the snowpack's file)
                    return rc2;
                });
                mcf::reduce_on_first(w, [&] {
                    // extremes over the blocks (max / min skip blocks whose step held no value), then the chunk's day classes
                    std::vector<double> mx((size_t)ns, -INFINITY), mn((size_t)ns, INFINITY);
                    for (const Block& k : h->blocks)
                        for (int q = 0; q < ns; ++q) {
                            if (k.cmx[(size_t)q] > 0 && k.mx[(size_t)q] > mx[(size_t)q]) mx[(size_t)q] = k.mx[(size_t)q];
                            if (k.cmn[(size_t)q] > 0 && k.mn[(size_t)q] < mn[(size_t)q]) mn[(size_t)q] = k.mn[(size_t)q];
                        }
                    snowdays_of(mx.data(), mn.data(), cd, &h->snowday[(size_t)(ch * cd)], &h->nosnowday[(size_t)(ch * cd)]);
                });
                bool any = false;
                for (int d = 0; d < cd; ++d) any |= h->snowday[(size_t)(ch * cd + d)] != 0;
                h->each_block(w, [&](Block& k) -> int {
                    int rc2 = mcf_snowplan_meand_accumulate(k.sp, ch, &h->snowday[(size_t)(ch * cd)]);
                    int32_t kept = 0;
                    if (!rc2 && any && h->keep) rc2 = mcf_snowplan_keep_chunk(k.sp, ch, h->keep_reserve, &kept);
                    if (!rc2) k.kept[(size_t)ch] = (char)kept;
                    return rc2;
                });
                w.wait();
            }
        });
        if (rc) return rc;
        // steps past the last whole chunk: the snow model leaves them NA (R/internal.R:2554-2558), `.runmicrosnow1` turns NA
        // into 0 (:3586) — days without snow anywhere, solved by the grid solver
        for (int d = h->nchunks * cd; d < h->ndays; ++d) { h->snowday[(size_t)d] = 0; h->nosnowday[(size_t)d] = 1; }
        h->layers_set = false;
        h->pass1_done = true;
        if (snowday) memcpy(snowday, h->snowday.data(), (size_t)h->ndays * 4);
        if (nosnowday) memcpy(nosnowday, h->nosnowday.data(), (size_t)h->ndays * 4);
        return MCF_OK;
    } catch (const std::exception& e) {
        return api_fail(MCF_ERR_NOMEM, std::string("mcf_snowrun_pass1: ") + e.what());
    }
}

// ---- pass 2, step by step: what the steps of one mcf_snowrun_pass2 call share -----------------------------------
namespace {
struct Pass2 {
    mcf_snowrun* h;
    const mcf_snow_inputs* micro;
    double mat;
    mcf_outputs* out;
    std::vector<int32_t> sdays, ndays_;         // the snow days, the no-snow days
    std::vector<int32_t> sub_of_day;            // day -> its place among the snow days, or -1
    int32_t outm[MCF_NOUT];                     // gridmicrosnow1's `out`
    mcf_snow_inputs sub{};                      // gridmicrosnow1's inputs on the snow-day subset (array weather: the whole series)
    mcf::HostCopies sub_series;
    double mxtc = -INFINITY;                    // the solver's maximum air temperature over the no-snow days (data.frame weather)
    bool no_skip = false, no_cells = false;
    const double NA = mcf::na_real_host();
};

// the day lists and gridmicrosnow1's `out` (R/internal.R:3616-3622)
void day_lists(Pass2& p) {
    const mcf_snowrun* h = p.h;
    for (int d = 0; d < h->ndays; ++d) {
        if (h->snowday[(size_t)d]) p.sdays.push_back(d);
        if (h->nosnowday[(size_t)d]) p.ndays_.push_back(d);
    }
    p.sub_of_day.assign(h->snowday.size(), -1);
    for (size_t i = 0; i < p.sdays.size(); ++i) p.sub_of_day[(size_t)p.sdays[i]] = (int32_t)i;
    for (int v = 0; v < MCF_NOUT; ++v) p.outm[v] = h->opt.out[v] ? 1 : 0;
    if (h->opt.reqhgt == 0.0) {
        static const int32_t ground[MCF_NOUT] = {1, 0, 0, 1, 0, 1, 1, 1, 1, 1};
        memcpy(p.outm, ground, sizeof p.outm);
    }
    if (h->below)       // `out[c(1, 4)]`: Tz and soilm only
        for (int v = 0; v < MCF_NOUT; ++v) p.outm[v] = p.outm[v] && (v == MCF_OUT_TZ || v == MCF_OUT_SOILM);
}

// `micro` checked, and the snow-day subset of its whole-series inputs (subsetpointmodel(micropoint, days = snowdays),
// R/internal.R:3599); the solver's maximum air temperature over the NO-snow subset (src/microclimfCpp.cpp:2159-2168 on what
// `.runmicronosnow` hands it, R/internal.R:3605)
int snow_day_inputs(Pass2& p) {
    const mcf_snowrun* h = p.h;
    const mcf_snow_inputs* micro = p.micro;
    if (!p.sdays.empty()) {
        if (!micro) return api_fail(MCF_ERR_ARG, "snow run: the year has snow days, gridmicrosnow1's inputs are needed");
        if (micro->rows != h->R || micro->cols != h->C || micro->tsteps != h->T || (micro->array_forcing != 0) != h->af)
            return api_fail(MCF_ERR_ARG, "snow run: gridmicrosnow's inputs must be the whole series on the whole raster, in the run's weather geometry");
        if (const char* missing = h->coarse ? nullptr : mcf::micro_series_missing(*micro))      // (a coarse run expands them itself)
            return api_fail(MCF_ERR_ARG, std::string("null input: gridmicrosnow1 weather$") + missing);
        const mcf_obstime& ob = micro->obstime;
        if (!ob.year || !ob.month || !ob.day || !ob.hour) return api_fail(MCF_ERR_ARG, "null obstime");
        if (!mcf::micro_rasters_given(*micro)) return api_fail(MCF_ERR_ARG, "null input: a gridmicrosnow1 raster");
        if (p.outm[MCF_OUT_SOILM] && h->opt.out[MCF_OUT_SOILM] && !micro->other.Smax)
            return api_fail(MCF_ERR_ARG, "soilm requested but other$Smax is null");
        p.sub = *micro;
        // (array weather: the snow plan takes the whole series and the day map — nine arrays are not copied)
        if (!h->af) mcf::subset_days(p.sub, true, p.sub_of_day.data(), h->ndays, (int)p.sdays.size(), p.sub_series);
    }
    if (!h->af)
        for (int d : p.ndays_)
            for (int hh = 0; hh < 24; ++hh) { const double v = h->grid.clim.tc[(int64_t)d * 24 + hh]; if (v > p.mxtc) p.mxtc = v; }
    return MCF_OK;
}

// a block's set-up between the passes: gridmicrosnow1's on its rows, the solver plan's for the no-snow days
int block_setup(Pass2& p, Block& k) {
    mcf_snowrun* h = p.h;
    int rc = MCF_OK;
    if (h->coarse) mcf::snowplan_coarse_umu_out(k.sp, nullptr);
    if (!p.sdays.empty()) {
        mcf_snow_inputs bs = p.sub;
        k.micro_rows = mcf::HostCopies();
        if (h->nb > 1) mcf::micro_rasters_of_block(bs, k.micro_rows, h->R, h->C, k.r0, k.nr);
        rc = mcf_snowplan_micro_setup(k.sp, &bs, p.sub_of_day.data(), (int32_t)p.sub_of_day.size(), h->opt.reqhgt, p.mat, p.outm, 0);
    }
    const bool solver = !p.ndays_.empty();
    // below ground: the series Tbelowgroundv sees is the no-snow days joined ...
    if (!rc && h->below && solver) rc = mcf_plan_below_set_days(k.plan, p.ndays_.data(), (int32_t)p.ndays_.size());
    if (!rc && solver)                         // (array weather: per cell, cpp:2467-2471, over the no-snow days)
        rc = h->af ? mcf_plan_set_mxtc_days(k.plan, &k.gsub, h->nosnowday.data(), h->ndays) : mcf_plan_set_mxtc(k.plan, p.mxtc);
    // ... and its per-cell state comes from a pass over them (complete = 1: the solver's first sweep)
    if (!rc && h->below && solver) rc = mcf_plan_below_prepare(k.plan, nullptr);
    if (!rc) rc = mcf_snowplan_set_series(k.sp, 31u);         // (pass 2's re-runs feed the snow microclimate)
    // the summaries of the merged outputs: the day classes are known, the plan has not run — enabled with this year's table
    // (a later year on the handle: the table replaced, nothing folded)
    if (!rc && h->sum_micro) {
        if (k.sum_on) rc = mcf::plan_summary_retable(k.plan, h->mtable_year.data());
        else {
            mcf_summary_spec spec = h->mspec;
            spec.period_of_day = h->mtable_year.data();
            rc = mcf_plan_summary_enable(k.plan, &spec);
            k.sum_on = !rc;
        }
    }
    return rc;
}

// The solver on the no-snow days among d0 .. d0 + nd, each at its own place in the ring slot: one function per mode.
// Below ground: the chunk's no-snow days in one call, EVERY cell — a cell's ground temperature under today's snow feeds its
// running means on later days, so nothing is left out (and a chunk without a no-snow day does not touch the plan's carried window)
int solver_days_below(Pass2& p, Block& k, int slot, int d0, int nd, bool has_snow) {
    mcf_snowrun* h = p.h;
    int n_both = 0;
    for (int d = 0; d < nd; ++d) n_both += h->nosnowday[(size_t)(d0 + d)] && h->snowday[(size_t)(d0 + d)];
    if (has_snow && n_both) {
        mcf_ring_layout lay;
        if (const int rc = mcf_plan_ring_layout(k.plan, &lay)) return rc;
        h->st_tile_days += (lay.cells + lay.cells_per_tile - 1) / lay.cells_per_tile * n_both;
    }
    return mcf_plan_run_days_at(k.plan, d0, nd, slot, 0);
}
// Data.frame weather: the runs of consecutive no-snow days, a run ending where the days' class changes (on a day without snow
// anywhere every cell is the solver's).  Where a run lies in a chunk with snow (ch >= 0), the tiles whose cells are all under snow
// for the whole run are left out (include/mcf.h mcf_plan_run_days_masked): gridmicrosnow1 overwrites every one of their values
int solver_days_vector(Pass2& p, Block& k, int slot, int ch, int d0, int nd, bool has_snow) {
    mcf_snowrun* h = p.h;
    for (int q = 0, e; q < nd; q = e) {
        e = q + 1;
        if (!h->nosnowday[(size_t)(d0 + q)]) continue;
        const bool both = h->snowday[(size_t)(d0 + q)] != 0;
        while (e < nd && h->nosnowday[(size_t)(d0 + e)] && (h->snowday[(size_t)(d0 + e)] != 0) == both) ++e;
        int rc;
        if (!(has_snow && both && !p.no_skip && ch >= 0)) {
            if ((rc = mcf_plan_run_days_at(k.plan, d0 + q, e - q, slot, q))) return rc;
            continue;
        }
        mcf_ring_layout lay;
        if ((rc = mcf_plan_ring_layout(k.plan, &lay))) return rc;
        const int64_t nt = (lay.cells + lay.cells_per_tile - 1) / lay.cells_per_tile;
        const uint8_t* need = nullptr;
        int64_t n_need = lay.cells;
        if (!p.no_cells && (rc = mcf_snowplan_free_cells(k.sp, k.plan, ch, q, e - q, &need, &n_need))) return rc;
        if (!p.no_cells && 16 * n_need <= lay.cells) {
            // the few cells that are not under snow throughout, gathered into tiles of their own (scattered cells
            // pay below ~ 8 % of the raster, profiles/r05_cells_rate.txt: their values reach the ring 8 bytes at a time)
            rc = mcf_plan_run_days_cells(k.plan, d0 + q, e - q, slot, q, need, lay.cells, nullptr);
            h->st_tile_days += nt * (e - q);
            h->st_tile_days_left_out += (nt - (n_need + lay.cells_per_tile - 1) / lay.cells_per_tile) * (e - q);
        } else {
            int64_t ncov = 0;
            k.skip.resize((size_t)nt);
            if ((rc = mcf_snowplan_covered_tiles(k.sp, k.plan, ch, q, e - q, k.skip.data(), nt, &ncov))) return rc;
            rc = mcf_plan_run_days_masked(k.plan, d0 + q, e - q, slot, q, ncov ? k.skip.data() : nullptr, ncov ? nt : 0);
            h->st_tile_days += nt * (e - q);
            h->st_tile_days_left_out += ncov * (e - q);
        }
        if (rc) return rc;
    }
    return MCF_OK;
}
// Array weather: the chunk's forcing into the slot once (all its days: the runs address them by day), then the same runs, whole
int solver_days_array(Pass2& p, Block& k, int slot, int d0, int nd) {
    const int rc = mcf_plan_upload_forcing_days(k.plan, &k.gsub, d0, nd, slot);
    return rc ? rc : solver_days_vector(p, k, slot, -1, d0, nd, false);
}
int solver_days(Pass2& p, Block& k, int slot, int ch, int d0, int nd, bool has_snow) {
    const mcf_snowrun* h = p.h;
    bool any = false;
    for (int d = 0; d < nd; ++d) any |= h->nosnowday[(size_t)(d0 + d)] != 0;
    if (!any) return MCF_OK;
    return h->below ? solver_days_below(p, k, slot, d0, nd, has_snow)
           : h->af  ? solver_days_array(p, k, slot, d0, nd)
                    : solver_days_vector(p, k, slot, ch, d0, nd, has_snow);
}

// the merged days of a ring slot to the caller: the block's rows in place, through the row pitch
int fetch_days(Pass2& p, Block& k, int slot, int d0, int nd) {
    const mcf_snowrun* h = p.h;
    const int64_t R = h->R, C = h->C;
    for (int v = 0; v < MCF_NOUT; ++v) {
        if (!h->opt.out[v] || !p.out || !p.out->var[v]) continue;      // (no host array: a variable that is only summarised)
        double* dst = p.out->var[v] + k.r0 + R * C * (int64_t)d0 * 24;
        if (const int rc = mcf_plan_fetch_pitched(k.plan, slot, v, 0, (int64_t)nd * 24, dst, R)) return rc;
        // a day in NEITHER class (a melted pack's negative rounding residue: max <= 0 and min != 0) is no day of either
        // model; the reference's merge indexes past its arrays there (R/internal.R:3650-3655) — NA here
        for (int d = 0; d < nd; ++d)
            if (!h->snowday[(size_t)(d0 + d)] && !h->nosnowday[(size_t)(d0 + d)])
                for (int64_t lc = (int64_t)(d0 + d) * 24 * C; lc < (int64_t)(d0 + d + 1) * 24 * C; ++lc)
                    for (int64_t r = 0; r < k.nr; ++r) p.out->var[v][k.r0 + r + R * lc] = p.NA;
    }
    return MCF_OK;
}

// the series sink of the merged outputs: the slot's days that are in a class, run by run (a day in neither class is no day of
// either model, fetch_days: never folded)
int fold_series_days(const mcf_snowrun* h, Block& k, int slot, int d0, int nd) {
    for (int q = 0, e; q < nd; q = e) {
        e = q + 1;
        if (!h->snowday[(size_t)(d0 + q)] && !h->nosnowday[(size_t)(d0 + q)]) continue;
        while (e < nd && (h->snowday[(size_t)(d0 + e)] || h->nosnowday[(size_t)(d0 + e)])) ++e;
        if (const int rc = mcf_plan_series_accumulate(k.plan, slot, q, d0 + q, e - q)) return rc;
    }
    return MCF_OK;
}

// the netCDF sink of the merged outputs: the block's row strips of the slot's days — runs of days in a class packed on the
// device, days in neither class (NA for every cell, fetch_days) as missval
int write_nc_days(const mcf_snowrun* h, Block& k, int slot, int d0, int nd) {
    for (int q = 0, e; q < nd; q = e) {
        e = q + 1;
        const bool in_class = h->snowday[(size_t)(d0 + q)] || h->nosnowday[(size_t)(d0 + q)];
        while (e < nd && (h->snowday[(size_t)(d0 + e)] || h->nosnowday[(size_t)(d0 + e)]) == in_class) ++e;
        const int rc = in_class ? mcf_nc_write_plan_rows(h->nc_micro, k.plan, slot, 0, k.r0, (int64_t)q * 24, (int64_t)(d0 + q) * 24,
                                                         (int64_t)(e - q) * 24, nullptr)
                                : mcf_nc_write_missing(h->nc_micro, k.r0, k.nr, (int64_t)(d0 + q) * 24, (int64_t)(e - q) * 24);
        if (rc) return rc;
    }
    return MCF_OK;
}

// a slot's merged days [d0, d0 + nd): into the summary, into the series sink, into the file, to the caller
int fold_and_fetch(Pass2& p, Block& k, int slot, int d0, int nd) {
    const mcf_snowrun* h = p.h;
    int rc = MCF_OK;
    if (h->sum_micro) rc = mcf_plan_summary_accumulate(k.plan, slot, 0, d0, nd);
    if (!rc && k.ser_micro) rc = fold_series_days(h, k, slot, d0, nd);
    if (!rc && h->nc_micro) rc = write_nc_days(h, k, slot, d0, nd);
    return rc ? rc : fetch_days(p, k, slot, d0, nd);
}

// per chunk: restore + re-run the snow chunk unless its series were kept; the solver on its no-snow days; the snow-day kernel
// over the slot; the slot's merged days to the caller.  Collective: every worker walks every chunk.
void chunk_loop(Pass2& p, Worker& w) {
    mcf_snowrun* h = p.h;
    const int cd = h->chunk_days;
    int slot = 0;
    for (int ch = 0; ch < h->nchunks; ++ch, slot ^= 1) {
        const int d0 = ch * cd, nd = std::min(cd, h->ndays - d0);
        bool has_snow = false, kept_all = true;
        for (int d = 0; d < cd; ++d) has_snow |= h->snowday[(size_t)(d0 + d)] != 0;
        for (const Block& k : h->blocks) kept_all = kept_all && k.kept[(size_t)ch];
        if (w.t == 0 && has_snow) ++(kept_all ? h->st_chunks_kept : h->st_chunks_rerun);
        if (has_snow && !kept_all) {          // collective: the blocks' surfaces couple through their halos
            h->each_block(w, [&](Block& k) { return mcf_snowplan_restore(k.sp, ch); });
            w.wait();
            snow_chunk(*h, w, ch, nullptr);
        }
        h->each_block(w, [&](Block& k) -> int {
            int rc = solver_days(p, k, slot, ch, d0, nd, has_snow);
            if (!rc && has_snow) rc = mcf_snowplan_microsnow(k.sp, k.plan, ch, slot, &h->nosnowday[(size_t)d0]);
            // the slot holds the merged days: folded on the plan's stream — behind the solver's launches on it, and behind the
            // snow-day kernel, whose null stream mcf_snowplan_microsnow has synchronised the device on before it returned
            if (!rc && nd > 0) rc = fold_and_fetch(p, k, slot, d0, nd);
            return rc;
        });
        w.wait();
    }
}

// days past the last whole chunk: the solver's alone; steps past the last whole day stay NA (src/microclimfCpp.cpp:2116)
void tail_days(Pass2& p, Worker& w) {
    mcf_snowrun* h = p.h;
    const int cd = h->chunk_days;
    const int64_t R = h->R, C = h->C;
    h->each_block(w, [&](Block& k) -> int {
        for (int d0 = h->nchunks * cd; d0 < h->ndays && !w.failed(); d0 += cd) {
            const int nd = std::min(cd, h->ndays - d0);
            int rc = solver_days(p, k, 0, -1, d0, nd, false);
            if (!rc) rc = fold_and_fetch(p, k, 0, d0, nd);
            if (rc) return rc;
        }
        if (h->sum_micro || h->ser_micro)          // (a sink-only run has no fetch that waits for the plan's stream)
            if (const int rc = mcf_plan_sync(k.plan)) return rc;
        if (h->nc_micro && h->T > (int64_t)h->ndays * 24)      // the steps past the last whole day: missval, as the arrays' NA
            if (const int rc = mcf_nc_write_missing(h->nc_micro, k.r0, k.nr, (int64_t)h->ndays * 24, h->T - (int64_t)h->ndays * 24)) return rc;
        for (int v = 0; v < MCF_NOUT; ++v)
            if (h->opt.out[v] && p.out && p.out->var[v])
                for (int64_t lc = (int64_t)h->ndays * 24 * C; lc < h->T * C; ++lc)
                    for (int64_t r = 0; r < k.nr; ++r) p.out->var[v][k.r0 + r + R * lc] = p.NA;
        return MCF_OK;
    });
}

}  // namespace

extern "C" int mcf_snowrun_pass2(mcf_snowrun* h, const mcf_snow_inputs* micro, double mat, mcf_outputs* out) {
    if (!h || (!out && !h->sum_micro && !h->ser_micro && !h->nc_micro)) return api_fail(MCF_ERR_ARG, "null snow-run argument");
    if (!h->pass1_done) return api_fail(MCF_ERR_STATE, "snow run: mcf_snowrun_pass1 first");
    try {
        for (int v = 0; v < MCF_NOUT; ++v)       // (with a summary enabled a variable may go without a host array: it is folded only)
            if (!h->sum_micro && !h->ser_micro && !h->nc_micro && h->opt.out[v] && !out->var[v]) return api_fail(MCF_ERR_ARG, "null output array for a requested variable");
        Pass2 p{h, micro, mat, out};
        p.no_skip = getenv("MCF_SNOW_NO_TILE_SKIP") != nullptr;
        p.no_cells = getenv("MCF_SNOW_NO_CELL_GATHER") != nullptr;      // (A/B: tiles as the unit, as in round 4)
        day_lists(p);
        if (const int rc = snow_day_inputs(p)) return rc;
        if (h->sum_micro) {
            h->mtable_year.assign((size_t)std::max(h->ndays, 1), -1);
            if (const int rc = mcf_snowrun_summary_table(h->mtable.data(), h->snowday.data(), h->nosnowday.data(), h->ndays, h->mtable_year.data()))
                return rc;
        }
        h->pass2_done = false;
        const int rc = mcf::run_workers(h->nt, [&](Worker& w) {
            h->each_block(w, [&](Block& k) { return block_setup(p, k); });
            w.wait();
            chunk_loop(p, w);
            tail_days(p, w);
        });
        h->pass2_done = !rc;
        return rc;
    } catch (const std::exception& e) {
        return api_fail(MCF_ERR_NOMEM, std::string("mcf_snowrun_pass2: ") + e.what());
    }
}

// ---- period summaries of the run (include/mcf.h "period summaries of the snow run and of the snowpack") --------
extern "C" int mcf_snowrun_summary_table(const int32_t* period_of_day, const int32_t* snowday, const int32_t* nosnowday, int32_t ndays,
                                         int32_t* out) {
    if (ndays < 0 || (ndays > 0 && (!period_of_day || !snowday || !nosnowday || !out)))
        return api_fail(MCF_ERR_ARG, "mcf_snowrun_summary_table: null argument");
    // a day in neither class is no day of either model (fetch_days: NA for every cell): never counted
    for (int d = 0; d < ndays; ++d) out[d] = snowday[d] || nosnowday[d] ? period_of_day[d] : -1;
    return MCF_OK;
}

static const char* const kSummaryBelow =
    "period summaries of the snow run need reqhgt >= 0 (a below-ground run's solver plan is a streamed plan, which takes no summary)";

// what can be judged of the two specs from the arguments alone
static int check_summary_specs(const mcf_summary_spec* micro, const mcf_snowpack_summary_spec* pack, const mcf_options& opt, int64_t tsteps,
                               int64_t chunk_steps) {
    if (!micro && !pack) return api_fail(MCF_ERR_ARG, "snow-run summaries: null spec (one of the two is needed)");
    if (opt.reqhgt < 0) return api_fail(MCF_ERR_ARG, kSummaryBelow);
    if (micro)
        if (const int rc = mcf::summary_spec_check(micro, tsteps / 24, opt.out)) return rc;
    return pack ? mcf::snowpack_spec_check(pack, tsteps, chunk_steps) : MCF_OK;
}

extern "C" int mcf_snowrun_summary_enable(mcf_snowrun* h, const mcf_summary_spec* micro, const mcf_snowpack_summary_spec* pack) {
    if (!h) return api_fail(MCF_ERR_ARG, "null snow run");
    if (h->below) return api_fail(MCF_ERR_ARG, kSummaryBelow);
    if (const int rc = check_summary_specs(micro, pack, h->opt, h->T, h->snow.chunk_steps)) return rc;
    if (h->sum_micro || h->sum_pack) return api_fail(MCF_ERR_STATE, "snow-run summaries are already enabled on this run");
    if (h->pass1_ever) return api_fail(MCF_ERR_STATE, "snow-run summaries are enabled before mcf_snowrun_pass1");
    try {
        if (pack) {
            h->pspec = *pack;
            h->ptable.assign(pack->period_of_day, pack->period_of_day + h->ndays);
            h->pspec.period_of_day = h->ptable.data();
            mcf::RestoreDevice restore;
            for (Block& k : h->blocks)
                if (const int rc = mcf_snowplan_summary_enable(k.sp, &h->pspec)) return rc;
            h->pack_bits = mcf::snowpack_series_bits(pack);
            h->sum_pack = true;
        }
        if (micro) {      // (the plans' own enable waits for the day classes: block_setup)
            h->mspec = *micro;
            h->mtable.assign(micro->period_of_day, micro->period_of_day + h->ndays);
            h->mspec.period_of_day = h->mtable.data();
            h->sum_micro = true;
        }
        return MCF_OK;
    } catch (const std::exception& e) {
        return api_fail(MCF_ERR_NOMEM, std::string("mcf_snowrun_summary_enable: ") + e.what());
    }
}

extern "C" int mcf_snowrun_summary_fetch(mcf_snowrun* h, int32_t pack, int32_t var, int32_t stat, double* host_dst) {
    if (!h || !host_dst) return api_fail(MCF_ERR_ARG, "null argument");
    if (!(pack ? h->sum_pack : h->sum_micro)) return api_fail(MCF_ERR_STATE, "snow run: this summary was not enabled (mcf_snowrun_summary_enable)");
    if (pack ? !h->pass1_done : !h->pass2_done)
        return api_fail(MCF_ERR_STATE, pack ? "snow run: the snowpack's summaries are there after mcf_snowrun_pass1"
                                            : "snow run: the summaries of the outputs are there after mcf_snowrun_pass2");
    mcf::RestoreDevice restore;
    for (Block& k : h->blocks) {      // a block's rows in place, through the row pitch
        const int rc = pack ? mcf_snowplan_summary_fetch(k.sp, var, stat, host_dst + k.r0, h->R)
                            : mcf::plan_summary_fetch_pitched(k.plan, var, stat, host_dst + k.r0, h->R);
        if (rc) return rc;
    }
    return MCF_OK;
}

extern "C" int mcf_snowrun_summary_days(mcf_snowrun* h, int32_t pack, int32_t* days) {
    if (!h || !days) return api_fail(MCF_ERR_ARG, "null argument");
    if (!(pack ? h->sum_pack : h->sum_micro)) return api_fail(MCF_ERR_STATE, "snow run: this summary was not enabled (mcf_snowrun_summary_enable)");
    if (pack ? !h->pass1_done : !h->pass2_done) return api_fail(MCF_ERR_STATE, "snow run: no summary before the pass that folds it");
    return pack ? mcf_snowplan_summary_days(h->blocks[0].sp, days) : mcf_plan_summary_days(h->blocks[0].plan, days);
}

// The one-call entries with a sink: `check` (the entry's refusals, none of which needs a device), the run created and held, the
// sink enabled, pass 1 — where a run for the snowpack's sink alone ends, unless the caller asks for the arrays — pass 2, `fetch`
template <class Outs, class Check, class Enable, class Fetch>
static int run_with_sink(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu, bool micro, Outs* outs, Check&& check,
                         Enable&& enable, Fetch&& fetch, bool below = false) {
    int rc = check();
    if (rc) return rc;
    mcf_snowrun* h = nullptr;
    if ((rc = snowrun_create(in, opt, mu, below, &h))) return rc;
    SnowRunHolder holder(h);
    if ((rc = enable(h))) return rc;
    if ((rc = mcf_snowrun_pass1(h, outs->smod, outs->snowday, outs->nosnowday))) return rc;
    if ((micro || outs->arrays) && (rc = mcf_snowrun_pass2(h, in->micro, in->mat, outs->arrays))) return rc;
    return fetch(h);
}

extern "C" int mcf_runmicrosnow_summary(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu,
                                        const mcf_summary_spec* micro_spec, const mcf_snowpack_summary_spec* pack_spec,
                                        mcf_snowrun_summary_out* outs) {
    if (!outs) return api_fail(MCF_ERR_ARG, "null snow-run argument");
    return run_with_sink(in, opt, mu, micro_spec != nullptr, outs, [&]() -> int {
        if (!micro_spec && !pack_spec) return api_fail(MCF_ERR_ARG, "snow-run summaries: null spec (one of the two is needed)");
        if (opt && opt->reqhgt < 0) return api_fail(MCF_ERR_ARG, kSummaryBelow);
        int rc = check_create(in, opt, mu, false);
        if (!rc) rc = check_summary_specs(micro_spec, pack_spec, *opt, in->grid->tsteps, in->snow->chunk_steps);
        if (!rc && micro_spec) rc = mcf::check_summary_out(micro_spec, &outs->micro);
        if (!rc && pack_spec) rc = mcf::check_snowpack_summary_out(pack_spec, &outs->pack);
        return rc;
    }, [&](mcf_snowrun* h) { return mcf_snowrun_summary_enable(h, micro_spec, pack_spec); }, [&](mcf_snowrun* h) -> int {
        int rc;
        for (int k = 0; k < MCF_NSTAT; ++k) {
            for (int v = 0; micro_spec && v < MCF_NOUT; ++v)
                if (micro_spec->var[v] && micro_spec->stat[k] && (rc = mcf_snowrun_summary_fetch(h, 0, v, k, outs->micro.val[v][k]))) return rc;
            for (int v = 0; pack_spec && v < 5; ++v)
                if (pack_spec->series[v] && pack_spec->stat[k] && (rc = mcf_snowrun_summary_fetch(h, 1, v, k, outs->pack.val[v][k]))) return rc;
        }
        if (micro_spec && outs->micro.days && (rc = mcf_snowrun_summary_days(h, 0, outs->micro.days))) return rc;
        if (pack_spec && outs->pack.days && (rc = mcf_snowrun_summary_days(h, 1, outs->pack.days))) return rc;
        return MCF_OK;
    });
}

// ---- series sink of the run (include/mcf.h "series sink of the snow run and of the snowpack") -------------------
static const char* const kSeriesBelow =
    ": the series sink of the snow run needs reqhgt >= 0 (a below-ground run's solver plan is a streamed plan over the no-snow days)";

// what can be judged of the two specs from the arguments alone; `who`: the entry's name, at the start of every message
static int check_series_specs(const std::string& who, const mcf_series_spec* micro, const mcf_snowpack_series_spec* pack, const int32_t* out_mask,
                              double reqhgt, int64_t rows, int64_t cols, int64_t chunk_steps) {
    if (!micro && !pack) return api_fail(MCF_ERR_ARG, who + ": null spec (one of the two is needed)");
    if (reqhgt < 0) return api_fail(MCF_ERR_ARG, who + kSeriesBelow);
    if (micro)
        if (const int rc = mcf::series_spec_check(who, micro, rows, cols, out_mask)) return rc;
    return pack ? mcf::snowpack_series_check(who, pack, rows, cols, chunk_steps) : MCF_OK;
}

extern "C" int mcf_snowrun_series_enable(mcf_snowrun* h, const mcf_series_spec* micro, const mcf_snowpack_series_spec* pack) {
    const std::string who = "mcf_snowrun_series_enable";
    if (!h) return api_fail(MCF_ERR_ARG, who + ": null snow run");
    if (h->below) return api_fail(MCF_ERR_ARG, who + kSeriesBelow);
    if (const int rc = check_series_specs(who, micro, pack, h->opt.out, h->opt.reqhgt, h->R, h->C, h->snow.chunk_steps)) return rc;
    if (h->ser_micro || h->ser_pack) return api_fail(MCF_ERR_STATE, who + ": the series sink is already enabled on this run");
    if (h->pass1_ever) return api_fail(MCF_ERR_STATE, who + ": the series sink is enabled before mcf_snowrun_pass1");
    try {
        mcf::RestoreDevice restore;
        if (pack) {
            h->spspec = *pack;
            if (pack->npoints > 0) h->spcells.assign(pack->cells, pack->cells + pack->npoints);
            if (pack->nzones > 0) h->spzone.assign(pack->zone, pack->zone + h->R * h->C);
            h->spspec.cells = h->spcells.data(); h->spspec.zone = h->spzone.data();
            for (Block& k : h->blocks)
                if (const int rc = block_pack_series(*h, k, &h->spspec)) return rc;
            static const uint32_t bit[5] = {1u, 2u, 8u, 4u, 16u};      // (mcf_snowplan_set_series: bit 2 is totalSWE, bit 3 the ground snow depth)
            for (int v = 0; v < 5; ++v) h->ser_pack_bits |= pack->series[v] ? bit[v] : 0u;
            h->ser_pack = true;
        }
        if (micro) {
            h->sspec = *micro;
            if (micro->npoints > 0) h->scells.assign(micro->cells, micro->cells + micro->npoints);
            if (micro->nzones > 0) h->szone.assign(micro->zone, micro->zone + h->R * h->C);
            h->sspec.cells = h->scells.data(); h->sspec.zone = h->szone.data();
            for (Block& k : h->blocks) {
                k.mcut.cut(micro->npoints, h->sspec.cells, micro->nzones, h->sspec.zone, h->R, h->C, k.r0, k.nr);
                if (k.mcut.empty(micro->nzones)) continue;
                mcf_series_spec bs = h->sspec;
                bs.npoints = (int64_t)k.mcut.cells.size(); bs.cells = k.mcut.cells.data(); bs.zone = k.mcut.zone.data();
                if (const int rc = mcf_plan_series_enable(k.plan, &bs)) return rc;
                k.ser_micro = true;
            }
            h->ser_micro = true;
        }
        return MCF_OK;
    } catch (const std::exception& e) {
        return api_fail(MCF_ERR_NOMEM, who + ": " + e.what());
    }
}

// the checks the two fetches share
static int series_fetch_ready(const char* who, mcf_snowrun* h, int32_t pack, int32_t var, const void* dst) {
    const std::string w = who;
    if (!h || !dst) return api_fail(MCF_ERR_ARG, w + ": null argument");
    if (!(pack ? h->ser_pack : h->ser_micro)) return api_fail(MCF_ERR_STATE, w + ": this series was not enabled (mcf_snowrun_series_enable)");
    if (pack ? !h->pass1_done : !h->pass2_done)
        return api_fail(MCF_ERR_STATE, w + (pack ? ": the snowpack's series are there after mcf_snowrun_pass1" : ": the series of the outputs are there after mcf_snowrun_pass2"));
    if (var < 0 || var >= (pack ? 5 : MCF_NOUT) || !(pack ? h->spspec.series[var] : h->sspec.var[var]))
        return api_fail(MCF_ERR_ARG, w + ": variable was not selected in mcf_snowrun_series_enable");
    return MCF_OK;
}
extern "C" int mcf_snowrun_series_fetch_points(mcf_snowrun* h, int32_t pack, int32_t var, double* dst) {
    if (const int rc = series_fetch_ready("mcf_snowrun_series_fetch_points", h, pack, var, dst)) return rc;
    const int64_t np = pack ? h->spspec.npoints : h->sspec.npoints, T = std::max<int64_t>(h->T, 1);
    if (np == 0) return api_fail(MCF_ERR_ARG, "mcf_snowrun_series_fetch_points: no points were selected in mcf_snowrun_series_enable");
    return blocks_fetch_points(*h, pack != 0, var, T, dst);
}
extern "C" int mcf_snowrun_series_fetch_zones(mcf_snowrun* h, int32_t pack, int32_t var, int32_t zstat, double* dst) {
    if (const int rc = series_fetch_ready("mcf_snowrun_series_fetch_zones", h, pack, var, dst)) return rc;
    const int32_t nz = pack ? h->spspec.nzones : h->sspec.nzones;
    if (zstat < 0 || zstat >= MCF_NZSTAT || nz == 0 || !(pack ? h->spspec.zstat[zstat] : h->sspec.zstat[zstat]))
        return api_fail(MCF_ERR_ARG, "mcf_snowrun_series_fetch_zones: statistic was not selected in mcf_snowrun_series_enable");
    return blocks_fetch_zones(*h, pack != 0, var, nz, (int64_t)h->ndays * 24, std::max<int64_t>(h->T, 1), zstat, dst);
}

extern "C" int mcf_runmicrosnow_series(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu,
                                       const mcf_series_spec* micro_spec, const mcf_snowpack_series_spec* pack_spec,
                                       mcf_snowrun_series_out* outs) {
    const std::string who = "mcf_runmicrosnow_series";
    if (!micro_spec && !pack_spec) return api_fail(MCF_ERR_ARG, who + ": null spec (one of the two is needed)");
    if (!outs || !in || !in->grid || !in->snow || !opt) return api_fail(MCF_ERR_ARG, who + ": null argument");
    return run_with_sink(in, opt, mu, micro_spec != nullptr, outs, [&]() -> int {
        int rc = check_series_specs(who, micro_spec, pack_spec, opt->out, opt->reqhgt, in->grid->rows, in->grid->cols, in->snow->chunk_steps);
        if (!rc) rc = check_create(in, opt, mu, false);             // (nothing above needs a device or reads an input array)
        if (!rc && micro_spec) rc = mcf::check_series_out(who, micro_spec, &outs->micro);
        if (!rc && pack_spec) rc = mcf::check_snowpack_series_out(who, pack_spec, &outs->pack);
        return rc;
    }, [&](mcf_snowrun* h) { return mcf_snowrun_series_enable(h, micro_spec, pack_spec); }, [&](mcf_snowrun* h) -> int {
        int rc;
        for (int v = 0; micro_spec && v < MCF_NOUT; ++v) {
            if (!micro_spec->var[v]) continue;
            if (micro_spec->npoints > 0 && (rc = mcf_snowrun_series_fetch_points(h, 0, v, outs->micro.points[v]))) return rc;
            for (int k = 0; k < MCF_NZSTAT; ++k)
                if (micro_spec->nzones > 0 && micro_spec->zstat[k] && (rc = mcf_snowrun_series_fetch_zones(h, 0, v, k, outs->micro.zones[v][k]))) return rc;
        }
        for (int v = 0; pack_spec && v < 5; ++v) {
            if (!pack_spec->series[v]) continue;
            if (pack_spec->npoints > 0 && (rc = mcf_snowrun_series_fetch_points(h, 1, v, outs->pack.points[v]))) return rc;
            for (int k = 0; k < MCF_NZSTAT; ++k)
                if (pack_spec->nzones > 0 && pack_spec->zstat[k] && (rc = mcf_snowrun_series_fetch_zones(h, 1, v, k, outs->pack.zones[v][k]))) return rc;
        }
        return MCF_OK;
    });
}

// ---- netCDF sink of the run (include/mcf.h "netCDF sink: further sources") -------------------------------------
// what can be judged of a pair of files for a run of these dimensions and variables; nb: the run's row blocks (0: not known yet)
static int check_nc_files(const std::string& w, const mcf_ncfile* micro, const mcf_ncfile* pack, int64_t R, int64_t C, int64_t T,
                          const int32_t* out, int nb) {
    if (!micro && !pack) return api_fail(MCF_ERR_ARG, w + "null files (one of the two is needed)");
    for (const mcf_ncfile* f : {micro, pack}) {
        if (!f) continue;
        const char* what = f == pack ? "the snowpack's file" : "the outputs' file";
        if (f->snowpack != (f == pack))
            return api_fail(MCF_ERR_ARG, w + what + (f == pack ? " was not made by mcf_nc_create_snowpack" : " holds the snowpack's series"));
        if (f->f->rows != R || f->f->cols != C) return api_fail(MCF_ERR_ARG, w + what + ": its grid is not the run's");
        if (f->f->nsteps != T) return api_fail(MCF_ERR_ARG, w + what + ": its steps are not the run's");
        if (nb > 1 && !f->f->takes_strips())
            return api_fail(MCF_ERR_ARG, w + what + ": the netCDF-4 container chunks a step into row strips of the whole raster: it takes one block");
    }
    for (int k = 0; micro && k < micro->f->nvars; ++k)
        if (!micro->fill_only[k] && !out[micro->out_of[k]])
            return api_fail(MCF_ERR_ARG, w + "a variable of the outputs' file is not among the run's (opt->out)");
    return MCF_OK;
}
extern "C" int mcf_snowrun_nc_enable(mcf_snowrun* h, mcf_ncfile* micro_file, mcf_ncfile* pack_file) {
    const std::string w = "mcf_snowrun_nc_enable: ";
    if (!h) return api_fail(MCF_ERR_ARG, w + "null snow run");
    if (const int rc = check_nc_files(w, micro_file, pack_file, h->R, h->C, h->T, h->opt.out, h->nb)) return rc;
    if (h->nc_micro || h->nc_pack) return api_fail(MCF_ERR_STATE, w + "the files are already enabled on this run");
    if (h->pass1_ever) return api_fail(MCF_ERR_STATE, w + "the files are enabled before mcf_snowrun_pass1");
    static const uint32_t bit[5] = {1u, 2u, 8u, 4u, 16u};      // (bit 2 is totalSWE, bit 3 the ground snow depth)
    for (int v = 0; pack_file && v < 5; ++v)
        if (pack_file->var_of[v] >= 0) h->nc_pack_bits |= bit[v];
    h->nc_micro = micro_file; h->nc_pack = pack_file;
    return MCF_OK;
}

using mcf::NcHolder;

extern "C" int mcf_runmicrosnow_nc(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu, const char* path,
                                   const mcf_nc_spec* spec, const char* pack_path, const mcf_ncpack_spec* pack_spec, mcf_snowrun_nc_out* outs) {
    const std::string who = "mcf_runmicrosnow_nc", w = who + ": ";
    if ((!path || !spec) && (!pack_path || !pack_spec)) return api_fail(MCF_ERR_ARG, w + "null path / spec (one of the two files is needed)");
    if ((path != nullptr) != (spec != nullptr) || (pack_path != nullptr) != (pack_spec != nullptr))
        return api_fail(MCF_ERR_ARG, w + "null path / spec: a file needs both");
    if (!outs || !in || !in->grid || !in->snow || !opt) return api_fail(MCF_ERR_ARG, w + "null argument");
    const bool below = opt->reqhgt < 0;
    NcHolder micro_file, pack_file;
    return run_with_sink(in, opt, mu, spec != nullptr, outs, [&]() -> int {
        int rc = check_create(in, opt, mu, below);
        if (rc) {
            if (strncmp(mcf_last_error(), w.c_str(), w.size()) != 0) rc = api_fail(rc, w + mcf_last_error());      // (the shared checks' messages)
            return rc;
        }
        const mcf_grid_inputs& g = *in->grid;
        const bool several = mu && mu->n_blocks != 1;
        if (spec && (rc = mcf::nc_spec_check(w, spec, g.rows, g.cols, g.tsteps, opt->reqhgt, opt->out, several))) return rc;
        if (pack_spec && (rc = mcf::ncpack_spec_check(w, pack_spec, g.rows, g.cols, g.tsteps, several))) return rc;
        return MCF_OK;
    }, [&](mcf_snowrun* h) -> int {      // the run exists, so there is a device to fill the files
        mcf_ncfile* nc = nullptr;
        int rc = spec ? mcf_nc_create(path, spec, &nc) : (int)MCF_OK;
        micro_file.reset(nc);
        nc = nullptr;
        if (!rc && pack_spec) rc = mcf_nc_create_snowpack(pack_path, pack_spec, &nc);
        pack_file.reset(nc);
        return rc ? rc : mcf_snowrun_nc_enable(h, micro_file.get(), pack_file.get());
    }, [&](mcf_snowrun*) -> int {
        const int rc = mcf::close_file(micro_file), rc2 = mcf::close_file(pack_file);
        return rc ? rc : rc2;
    }, below);
}

static int runmicrosnow1_impl(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* mu, mcf_outputs* out,
                              const mcf_snowdriver_out* smod, bool below = false) {
    mcf_snowrun* h = nullptr;
    int rc = snowrun_create(in, opt, mu, below, &h);
    if (rc) return rc;
    SnowRunHolder holder(h);
    if ((rc = mcf_snowrun_pass1(h, smod, nullptr, nullptr))) return rc;
    return mcf_snowrun_pass2(h, in->micro, in->mat, out);
}
extern "C" int mcf_runmicrosnow1(const mcf_microsnow_in* in, const mcf_options* opt, mcf_outputs* out, const mcf_snowdriver_out* smod) {
    if (in && in->grid && in->grid->array_forcing) return api_fail(MCF_ERR_ARG, "mcf_runmicrosnow1 takes data.frame (vector) weather; array weather: mcf_runmicrosnow2");
    return runmicrosnow1_impl(in, opt, nullptr, out, smod);
}
// `.snowmodel2`'s loop + `.runmicrosnow2` (R/internal.R:2950-3008, 3661-3745): the same run with array weather
extern "C" int mcf_runmicrosnow2(const mcf_microsnow_in* in, const mcf_options* opt, mcf_outputs* out, const mcf_snowdriver_out* smod) {
    if (in && in->grid && !in->grid->array_forcing) return api_fail(MCF_ERR_ARG, "mcf_runmicrosnow2 takes array weather; data.frame weather: mcf_runmicrosnow1");
    return runmicrosnow1_impl(in, opt, nullptr, out, smod);
}
extern "C" int mcf_runmicrosnow1_multi(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* multi, mcf_outputs* out,
                                       const mcf_snowdriver_out* smod) {
    if (!multi) return api_fail(MCF_ERR_ARG, "null argument");
    return runmicrosnow1_impl(in, opt, multi, out, smod);
}

// The array-weather run with every coarse array left coarse (include/mcf.h mcf_runmicrosnow2_coarse): the chunk loop of
// mcf_snowmodel2_coarse, a coarse solver plan, and the microclimate's snow days expanded on the device (mcf_snow.hip k_coarse_hours)
extern "C" int mcf_snowrun_create_coarse(const mcf_microsnow_coarse_in* in, const mcf_options* opt, const mcf_multi* mu, double* umu_out,
                                         mcf_snowrun** out) {
    const char* entry = "mcf_snowrun_create_coarse";
    if (!out) return api_fail(MCF_ERR_ARG, std::string(entry) + ": null argument: run");
    if (const int rc = check_create_coarse(in, opt, mu, entry)) return rc;      // nothing above needs a device
    return snowrun_create(nullptr, opt, mu, false, out, in, umu_out);
}
extern "C" int mcf_runmicrosnow2_coarse(const mcf_microsnow_coarse_in* in, const mcf_options* opt, mcf_outputs* out,
                                        const mcf_snowfast2_out* smod) {
    const char* entry = "mcf_runmicrosnow2_coarse";
    if (!out) return api_fail(MCF_ERR_ARG, std::string(entry) + ": null argument: out");
    if (const int rc = check_create_coarse(in, opt, nullptr, entry)) return rc;
    for (int v = 0; v < MCF_NOUT; ++v)
        if (opt->out[v] && !out->var[v]) return api_fail(MCF_ERR_ARG, std::string(entry) + ": null argument: out->var[" + std::to_string(v) + "]");
    mcf_snowrun* h = nullptr;
    int rc = snowrun_create(nullptr, opt, nullptr, false, &h, in, smod ? smod->umu : nullptr);
    if (rc) return rc;
    SnowRunHolder holder(h);
    if ((rc = mcf_snowrun_pass1(h, smod ? &smod->smod : nullptr, nullptr, nullptr))) return rc;
    rc = mcf_snowrun_pass2(h, in->micro_static, in->mat, out);
    if (!rc && getenv("MCF_TIMING")) mcf::snowplan_print_timing(h->blocks[0].sp);
    return rc;
}

// reqhgt < 0: the same run with a streamed below-ground solver plan over the no-snow days (data.frame weather)
extern "C" int mcf_runmicrosnow1_below(const mcf_microsnow_in* in, const mcf_options* opt, mcf_outputs* out, const mcf_snowdriver_out* smod) {
    return runmicrosnow1_impl(in, opt, nullptr, out, smod, true);
}
extern "C" int mcf_runmicrosnow1_below_multi(const mcf_microsnow_in* in, const mcf_options* opt, const mcf_multi* multi, mcf_outputs* out,
                                             const mcf_snowdriver_out* smod) {
    if (!multi) return api_fail(MCF_ERR_ARG, "null argument");
    return runmicrosnow1_impl(in, opt, multi, out, smod, true);
}

// ---- the snow model alone: `.snowmodel1` / `.snowmodel2`'s chunk loop (mcf_snowmodel1 / 2: one plan on `device`, mu = NULL)
// or over row blocks of ONE raster held by this process (include/mcf.h mcf_snowmodel1_multi: block b on devices[b % n_devices];
// EVERY block's plan stays resident, the chunk loop couples the blocks at every chunk)
// The snowpack's sinks, each folded behind every chunk: spec / sout, the period summaries (mcf_snowmodel1_summary, which has
// checked them); zspec / zout, the series sink (mcf_snowmodel1_series, which has checked them)
struct PackSinks {
    const mcf_snowpack_summary_spec* spec;
    mcf_snowpack_summary_out* sout;
    const mcf_snowpack_series_spec* zspec;
    mcf_snowpack_series_out* zout;
    mcf_ncfile* nc;      // the snowpack's file (mcf_snowmodel1_nc, which has made it): every block writes its strips
};
// coarse: mcf_snowmodel2_coarse, which has checked it (`in` is &coarse.co->drv)
static int snowmodel(const mcf_snowdriver_in* in, mcf_snowdriver_out* out, const mcf_multi* mu, int32_t device, const PackSinks& sinks = {},
                     const CoarseSource& coarse = {}) {
    if (!in || !out) return api_fail(MCF_ERR_ARG, "null snow driver argument");
    try {
        SnowBlocks sb;
        sb.R = in->base.rows; sb.C = in->base.cols;
        int rc;
        if (!mu) sb.devs.push_back(device);                        // (mcf_snowplan_create checks it)
        else if ((rc = mcf::device_list(mu, 0, &sb.devs))) return rc;
        sb.cut(mu ? mu->n_blocks : 1);
        rc = mcf::run_workers(sb.nt, [&](Worker& w) {
            mcf::for_blocks(w, sb.nb, sb.nt, [&](int b) { return block_snowplan(sb, b, sb.devs[(size_t)w.t], *in, coarse); });
        });
        if (rc) return rc;
        const int nchunks = mcf_snowplan_chunks(sb.blocks[0].sp);
        rc = mcf::run_workers(sb.nt, [&](Worker& w) {
            if (sinks.spec) {
                sb.each_block(w, [&](Block& k) { return mcf_snowplan_summary_enable(k.sp, sinks.spec); });
                w.wait();
            }
            if (sinks.zspec) {
                sb.each_block(w, [&](Block& k) { return block_pack_series(sb, k, sinks.zspec); });
                w.wait();
            }
            for (int ch = 0; ch < nchunks; ++ch) {
                snow_chunk(sb, w, ch, out);
                if (sinks.spec) sb.each_block(w, [&](Block& k) { return mcf_snowplan_summary_accumulate(k.sp, ch); });
                if (sinks.zspec) sb.each_block(w, [&](Block& k) { return k.ser_pack ? mcf_snowplan_series_accumulate(k.sp, ch) : (int)MCF_OK; });
                if (sinks.nc) sb.each_block(w, [&](Block& k) { return mcf_snowplan_nc_write(k.sp, sinks.nc, ch, k.r0); });
            }
            if (sinks.spec)      // every block's rows of the planes in place, through the row pitch
                sb.each_block(w, [&](Block& k) -> int {
                    for (int v = 0; v < 5; ++v)
                        for (int q = 0; q < MCF_NSTAT; ++q)
                            if (sinks.spec->series[v] && sinks.spec->stat[q])
                                if (const int rc2 = mcf_snowplan_summary_fetch(k.sp, v, q, sinks.sout->val[v][q] + k.r0, sb.R)) return rc2;
                    return MCF_OK;
                });
        });
        if (!rc && sinks.spec && sinks.sout->days) rc = mcf_snowplan_summary_days(sb.blocks[0].sp, sinks.sout->days);
        // the series: the blocks' points to their places, their zone states combined and finished once
        const int64_t T = std::max<int64_t>(in->base.tsteps, 1);
        for (int v = 0; !rc && sinks.zspec && v < 5; ++v) {
            if (!sinks.zspec->series[v]) continue;
            if (sinks.zspec->npoints > 0) rc = blocks_fetch_points(sb, true, v, T, sinks.zout->points[v]);
            for (int q = 0; !rc && q < MCF_NZSTAT; ++q)
                if (sinks.zspec->nzones > 0 && sinks.zspec->zstat[q])
                    rc = blocks_fetch_zones(sb, true, v, sinks.zspec->nzones, in->base.tsteps / 24 * 24, T, q, sinks.zout->zones[v][q]);
        }
        if (!rc && !mu && getenv("MCF_TIMING")) mcf::snowplan_print_timing(sb.blocks[0].sp);
        return rc;
    } catch (const std::exception& e) {
        return api_fail(MCF_ERR_NOMEM, std::string("snow driver: ") + e.what());
    }
}
extern "C" int mcf_snowmodel1(const mcf_snowdriver_in* in, mcf_snowdriver_out* out, int32_t device) {
    if (in && in->base.array_forcing) return api_fail(MCF_ERR_ARG, "mcf_snowmodel1 takes data.frame (vector) climate; array weather: mcf_snowmodel2");
    return snowmodel(in, out, nullptr, device);
}
extern "C" int mcf_snowmodel2(const mcf_snowdriver_in* in, mcf_snowdriver_out* out, int32_t device) {
    if (in && !in->base.array_forcing) return api_fail(MCF_ERR_ARG, "mcf_snowmodel2 takes array weather; data.frame climate: mcf_snowmodel1");
    return snowmodel(in, out, nullptr, device);
}
// mcf_snowmodel1 / _multi with the snowpack's period summaries as the only sink: no series leaves the device
extern "C" int mcf_snowmodel1_summary(const mcf_snowdriver_in* in, const mcf_snowpack_summary_spec* spec, const mcf_multi* mu,
                                      mcf_snowpack_summary_out* out) {
    if (!in || !out) return api_fail(MCF_ERR_ARG, "null snow driver argument");
    if (in->base.array_forcing) return api_fail(MCF_ERR_ARG, "mcf_snowmodel1_summary takes data.frame (vector) climate");
    if (const int rc = mcf::snowpack_spec_check(spec, in->base.tsteps, in->chunk_steps)) return rc;
    if (const int rc = mcf::check_snowpack_summary_out(spec, out)) return rc;
    if (in->base.rows <= 0 || in->base.cols <= 0 || !in->dtm) return api_fail(MCF_ERR_ARG, "snow driver needs the raster and its dtm");
    if (!mcf::model_rasters_given(in->base)) return api_fail(MCF_ERR_ARG, "null input: a vegetation or initial-snow raster");
    mcf_snowdriver_out none{};
    return snowmodel(in, &none, mu, 0, {spec, out, nullptr, nullptr, nullptr});
}
// mcf_snowmodel1 / _multi with the snowpack's series sink as the only sink
extern "C" int mcf_snowmodel1_series(const mcf_snowdriver_in* in, const mcf_snowpack_series_spec* spec, const mcf_multi* mu,
                                     mcf_snowpack_series_out* out) {
    const std::string who = "mcf_snowmodel1_series";
    if (!spec) return api_fail(MCF_ERR_ARG, who + ": null mcf_snowpack_series_spec");
    if (!in || !out) return api_fail(MCF_ERR_ARG, who + ": null snow driver argument");
    if (const int rc = mcf::snowpack_series_check(who, spec, in->base.rows, in->base.cols, in->chunk_steps)) return rc;      // no device yet
    if (in->base.array_forcing) return api_fail(MCF_ERR_ARG, who + " takes data.frame (vector) climate");
    if (const int rc = mcf::check_snowpack_series_out(who, spec, out)) return rc;
    if (in->base.rows <= 0 || in->base.cols <= 0 || !in->dtm) return api_fail(MCF_ERR_ARG, who + ": snow driver needs the raster and its dtm");
    if (!mcf::model_rasters_given(in->base)) return api_fail(MCF_ERR_ARG, who + ": null input: a vegetation or initial-snow raster");
    mcf_snowdriver_out none{};
    return snowmodel(in, &none, mu, 0, {nullptr, nullptr, spec, out, nullptr});
}
// mcf_snowmodel1 / _multi with the snowpack's netCDF file as the only sink: 4 B per value leave the device, no series array on the host
extern "C" int mcf_snowmodel1_nc(const mcf_snowdriver_in* in, const mcf_multi* mu, const char* path, const mcf_ncpack_spec* spec) {
    const std::string who = "mcf_snowmodel1_nc";
    if (!in || !path || !spec) return api_fail(MCF_ERR_ARG, who + ": null argument");
    if (in->base.array_forcing) return api_fail(MCF_ERR_ARG, who + " takes data.frame (vector) climate");
    if (in->base.rows <= 0 || in->base.cols <= 0 || !in->dtm) return api_fail(MCF_ERR_ARG, who + ": snow driver needs the raster and its dtm");
    if (!mcf::model_rasters_given(in->base)) return api_fail(MCF_ERR_ARG, who + ": null input: a vegetation or initial-snow raster");
    if (const int rc = mcf::ncpack_spec_check(who + ": ", spec, in->base.rows, in->base.cols, in->base.tsteps, mu && mu->n_blocks != 1)) return rc;
    if (const int rc = mcf::device_list(mu, 0, nullptr)) return rc;      // no file without a device to fill it
    mcf_ncfile* nc = nullptr;
    if (const int rc = mcf_nc_create_snowpack(path, spec, &nc)) return rc;
    mcf_snowdriver_out none{};
    NcHolder holder(nc);
    const int rc = snowmodel(in, &none, mu, 0, {nullptr, nullptr, nullptr, nullptr, nc});
    return rc ? rc : mcf::close_file(holder);
}
// `.snowmodel2` from the coarse arrays: the same chunk loop over one block whose plan expands a chunk's series on the device
// (mcf_snow.hip, k_coarse_hours) and hands pointm$umu out of the chunk's slab
extern "C" int mcf_snowmodel2_coarse(const mcf_snowcoarse_in* in, mcf_snowfast2_out* out, int32_t device) {
    if (const int rc = mcf::snowcoarse_checks(in, true, "mcf_snowmodel2_coarse", out ? nullptr : "out")) return rc;      // no device yet
    return snowmodel(&in->drv, &out->smod, nullptr, device, {}, {in, out->umu});
}
extern "C" int mcf_snowmodel1_multi(const mcf_snowdriver_in* in, mcf_snowdriver_out* out, const mcf_multi* mu) {
    if (!in || !out || !mu) return api_fail(MCF_ERR_ARG, "null snow driver argument");
    const mcf_snow_inputs& base = in->base;
    if (base.rows <= 0 || base.cols <= 0 || !in->dtm) return api_fail(MCF_ERR_ARG, "snow driver needs the raster and its dtm");
    if (!mcf::model_rasters_given(base))
        return api_fail(MCF_ERR_ARG, "null input: a vegetation or initial-snow raster");
    return snowmodel(in, out, mu, 0);
}
