// mcf_api.hip — the C ABI of include/mcf.h: plan management, day-chunk streaming
// through HBM, and the one-shot host-to-host entry points that stand in for the
// reference's _microclimf_runmicro1Cpp / _microclimf_runmicro2Cpp
// (src/RcppExports.cpp:250-297).
//
// No CPU fallback: every entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mcf.h"
#include "mcf_kernels.h"
#include "mcf_hydro.h"
#include "mcf_terrain.h"
#include "mcf_ncfile.hpp"
#include "mcf_nc4file.hpp"
#include "mcf_ncsink.hpp"
#include "mcf_rowblocks.hpp"
#include "mcf_hiphost.hpp"
#include "mcf_series_host.hpp"
#include "mcf_sinks_host.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace

namespace mcf {
int api_fail(int code, const std::string& msg) { return fail(code, msg); }
}

using mcf::SinkPlaces;

struct mcf_plan {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int64_t rows = 0, cols = 0, N = 0, tsteps = 0;
    int64_t pitch = 0;      // rows of the (taller) column-major raster the host arrays are blocks of; = rows: dense
    int ndays = 0;
    bool af = false, bg = false;
    bool coarse = false;                 // array_forcing == 2: coarse arrays interpolated in the solver
    bool coarse_lds = false;             // ... with the taps staged in LDS: every 32-cell tile touches <= 4 coarse rows per column
    int crows = 0, ccols = 0;
    const double *d_crowpos = nullptr, *d_ccolpos = nullptr;
    int altcorrect = 0;
    const double *d_elevd = nullptr, *d_pkfac = nullptr;
    int cpb = 16;
    int layers = 1;
    int32_t* d_daylayer = nullptr;
    std::vector<int32_t> daylayer0;      // the day -> layer map of lyr_st / lyr_ed (mcf_plan_set_day_layers(NULL) goes back to it)
    mcf_options opt{};
    mcf::Globals g{};
    int hiy = 8760;
    double lat = 0, lon = 0;
    mcf::DevOwner dev;          // every device buffer of the plan; dev.bytes is what mcf_plan_bytes reports
    // static inputs
    const double* d_veg[10] = {};
    const double* d_soil[13] = {};
    const double *d_wsa = nullptr, *d_hor = nullptr, *d_lats = nullptr, *d_lons = nullptr;
    double* d_cellc = nullptr;
    double* d_tt = nullptr;
    double* d_twi2 = nullptr;
    double twi_sum = 0;
    int64_t twi_count = 0;
    double twi_mean = 0;
    bool cells_ready = false;
    // fast-clamp dispatch (vector forcing, reqhgt >= 0): tiles whose valid cells are all FL_REGULAR run the min / max
    // variant of the solver, the others the reference's compare-and-select form; days with an irregular forcing step
    // send the whole launch through the latter (mcf_device.hpp `cap`, mcf_kernels.hip k_solve / k_solve_fix)
    bool fast_enabled = false;
    std::vector<char> day_irregular, day_soil_daily;
    int32_t *d_tiles_fast = nullptr, *d_tiles_slow = nullptr;
    // mcf_plan_run_days_masked: the tile classes on the host, and the launch's own lists on the device
    std::vector<int32_t> h_tiles_fast, h_tiles_slow, h_tiles_sub;
    int32_t* d_tiles_sub = nullptr;
    int64_t masked_tiles_skipped = 0;
    // mcf_plan_run_days_cells: the cells' classes, the per-256-cell counts / list offsets, the list of gathered cells, the
    // gathered tiles' images and their ring (grown as needed)
    uint8_t* d_cls = nullptr;
    uint8_t* d_tile_regular = nullptr;      // [ntiles] 1: a tile of the fast list (null: no fast list)
    int32_t *d_blockcnt = nullptr, *d_celllist = nullptr;
    double *d_subimg = nullptr, *d_subring = nullptr;
    int64_t cls_cap = 0, blockcnt_cap = 0, celllist_cap = 0, subimg_cap = 0, subring_cap = 0;      // bytes
    std::vector<int32_t> h_blockcnt, h_cells_slow;
    int32_t* d_cells_slow = nullptr;
    int64_t cells_slow_cap = 0;
    hipStream_t prep = nullptr;              // the list is made beside the plan's stream, which is not drained for it
    hipEvent_t ev_prep = nullptr, ev_cells_done = nullptr;
    bool cells_inflight = false;
    int64_t cells_runs = 0, cells_gathered = 0;
    int64_t n_fast = 0, n_slow = 0;
    int32_t *d_fix_count = nullptr, *d_fix_list = nullptr;
    int fix_cap = 8192;
    int64_t fast_launches = 0, slow_launches = 0;
    // array forcing
    double* d_dt = nullptr;
    int32_t* d_windex = nullptr;
    double* d_mxtc = nullptr;
    double* d_force = nullptr;  // array forcing: tiled ring (see mcf_plan_create); coarse: [15][crows*ccols][T]
    double* d_force_stage = nullptr;
    int64_t force_tile_stride = 0, force_day_stride = 0, force_slot_elems = 0;
    std::vector<int> force_day0, force_ndays;
    // outputs
    int ring_days = 0, ring_slots = 0;
    // reqhgt >= 0: TILED, [slots][tile][day][var][ring_block_doubles(cpb)] in the solver's lane order (mcf_kernels.h
    // RingView); reqhgt < 0: linear, [slots][nvars][N*ring_days*24]
    double* d_ring = nullptr;
    bool tiled = false;
    int64_t ntiles = 0, slot_elems = 0;                        // elements per slot (all variables)
    int64_t ring_tile_stride = 0, ring_day_stride = 0, ring_var_stride = 0;
    double* d_stage = nullptr;   // untiled [N][steps] pieces on their way to the host (mcf_plan_fetch)
    int64_t stage_elems = 0;
    int var_slot[MCF_NOUT];     // index among enabled vars or -1
    int nvars = 0;
    // diagnostics (mcf_plan_diag_enable; null: off): a second tiled ring, [slots][tile][day][selected diagnostic][block]
    double* d_dring = nullptr;
    int dg_slab1[MCF_NDIAG] = {};   // 1 + slab among the selected diagnostics, 0: not selected
    int ndiag = 0;
    int64_t dg_tile_stride = 0, dg_day_stride = 0, dg_slot_elems = 0;
    bool has_run = false;           // a solver launch has been described (mcf_plan_diag_enable comes before)
    // period summaries (mcf_plan_summary_enable; null state: off): the state [selected var][period][state row][N]
    // (mcf_kernels.h SummaryAccArgs), the day tables on the device, one statistic plane on its way to the host
    double *d_sum_state = nullptr, *d_sum_plane = nullptr;
    int32_t *d_sum_pod = nullptr, *d_sum_prev = nullptr, *d_sum_next = nullptr, *d_sum_days = nullptr;
    int sum_nperiods = 0, sum_nrows = 0;
    SinkPlaces sum_places;
    int sum_row[MCF_NSTAT] = {};    // state row of a statistic, -1: not selected
    double sum_thr[MCF_NOUT] = {};
    uint32_t sum_init_codes = 0;
    std::vector<int32_t> sum_pod, sum_days;
    int sum_next_day = 0;           // the first day that may still be folded
    // series sink (mcf_plan_series_enable; ser_on): the points' [selected var][point][tsteps] buffer, the zones' state
    // (mcf_kernels.h SeriesZonesArgs), one statistic [tsteps][zone] on its way to the host, the folded days
    bool ser_on = false;
    int64_t ser_npoints = 0;
    int ser_nzones = 0, ser_workgroups = 0;
    SinkPlaces ser_places;
    int ser_zstat[MCF_NZSTAT] = {};
    int64_t* d_ser_cells = nullptr;
    int32_t *d_ser_zone = nullptr, *d_ser_done = nullptr;
    double *d_ser_points = nullptr, *d_ser_plane = nullptr;
    long long* d_ser_state = nullptr;
    std::vector<int32_t> ser_done;  // [days] 1: folded
    // reqhgt < 0
    double *d_tgser = nullptr, *d_ddsum = nullptr, *d_scratch = nullptr;
    const double *d_Tgp = nullptr, *d_Tbp = nullptr;
    // reqhgt < 0 streamed through day chunks (mcf_plan_create_streamed): the tiled ring, the chunk's Tg ring and per-cell state
    // (mcf_kernels.h BelowStreamArgs); array forcing with complete = 0: the point model's Tg / Tbp of each slot's days
    bool bg_stream = false;
    bool below_ready = false;            // mcf_plan_below_prepare has run
    int below_next = 0;                  // the day the next chunk has to start on (or 0: a new pass)
    // mcf_plan_below_set_days: the calendar day of each subset position (empty: every day), and its copy on the device;
    // below_next then counts subset positions
    std::vector<int32_t> below_days;
    int32_t* d_below_days = nullptr;
    double *d_tgring = nullptr, *d_hsum = nullptr, *d_dmean = nullptr, *d_ybuf = nullptr, *d_wrap = nullptr, *d_prev = nullptr;
    double *d_Tgp_slots = nullptr, *d_Tbp_slots = nullptr;      // [slots][ring_days * 24][N]
    int64_t tg_tile_stride = 0;
    // mcf_plan_below_set_depths (empty: one depth, opt.reqhgt): the depths; beside the ring the Tz slabs of depths 1 .. D - 1,
    // [depth][slot][tile][day][block] (the Tg ring's geometry per slot); their rows of circular means [depth][days][N]; with
    // complete = 0 the point model's Tbp per depth [D][tsteps]
    std::vector<double> depths;
    double *d_tzx = nullptr, *d_ybufx = nullptr;
    const double* d_Tbp_depths = nullptr;
    // timing
    bool ktiming = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kev;
    double ktotal_ms = 0;
    int64_t klaunches = 0;
    int64_t valid_cells = 0;
    // packed sink staging
    int32_t* d_pack = nullptr;
    int64_t pack_elems = 0;
    // device -> pageable host copies of results (mcf_hiphost.hpp)
    mcf::ToHost tohost;
};

namespace {

// a plan on its way to the caller, or a one-call entry's own: destroyed on every path that does not release() it
struct PlanDestroy { void operator()(mcf_plan* p) const { mcf_plan_destroy(p); } };
using PlanHolder = std::unique_ptr<mcf_plan, PlanDestroy>;

// rows of the (taller) column-major raster the caller's arrays are blocks of
int64_t host_pitch(const mcf_grid_inputs* in) { return in->row_pitch > 0 ? in->row_pitch : in->rows; }

// fn() between two events on the plan's stream when kernel timing is on (mcf_plan_kernel_stats adds the pairs up)
template <class F>
int timed(mcf_plan* p, F&& fn) {
    if (!p->ktiming) { fn(); return MCF_OK; }
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, p->stream));
    fn();
    HIP_TRY(hipEventRecord(e1, p->stream));
    p->kev.emplace_back(e0, e1);
    return MCF_OK;
}

// variable `var` (requested) of ring slot `slot` as its consumers address it
mcf::RingView ring_view(const mcf_plan* p, int slot, int var) {
    mcf::RingView v{};
    v.N = p->N;
    const double* sb = p->d_ring + (int64_t)slot * p->slot_elems;
    if (p->tiled) {
        v.base = sb + (int64_t)p->var_slot[var] * p->ring_var_stride;
        v.tile_stride = p->ring_tile_stride; v.day_stride = p->ring_day_stride; v.cpb = p->cpb;
    } else {
        v.base = sb + (int64_t)p->var_slot[var] * (p->N * (int64_t)p->ring_days * 24);
        v.cpb = 0;
    }
    return v;
}

// selected diagnostic `dvar` of ring slot `slot` (the diagnostics ring is always tiled)
mcf::RingView diag_view(const mcf_plan* p, int slot, int dvar) {
    mcf::RingView v{};
    v.N = p->N;
    v.base = p->d_dring + (int64_t)slot * p->dg_slot_elems + (int64_t)(p->dg_slab1[dvar] - 1) * mcf::ring_block_doubles(p->cpb);
    v.tile_stride = p->dg_tile_stride; v.day_stride = p->dg_day_stride; v.cpb = p->cpb;
    return v;
}
int check_diag_range(const mcf_plan* p, int32_t slot, int32_t dvar, int64_t step0, int64_t nsteps) {
    if (!p->d_dring) return fail(MCF_ERR_STATE, "the plan has no diagnostics ring: mcf_plan_diag_enable first");
    if (slot < 0 || slot >= p->ring_slots || dvar < 0 || dvar >= MCF_NDIAG) return fail(MCF_ERR_ARG, "bad slot/diagnostic");
    if (!p->dg_slab1[dvar]) return fail(MCF_ERR_ARG, "diagnostic was not selected in mcf_plan_diag_enable");
    if (step0 < 0 || nsteps < 0 || step0 + nsteps > (int64_t)p->ring_days * 24) return fail(MCF_ERR_ARG, "step range out of slot");
    return MCF_OK;
}

// steps [step0, step0 + nsteps) of variable `var` in ring slot `slot`: a slot of the plan, a requested variable (kAnyVar: the
// caller checks its variables itself), a range inside the slot
constexpr int kAnyVar = -1;
int check_slot_range(const mcf_plan* p, int32_t slot, int32_t var, int64_t step0, int64_t nsteps) {
    if (slot < 0 || slot >= p->ring_slots || (var != kAnyVar && (var < 0 || var >= MCF_NOUT))) return fail(MCF_ERR_ARG, "bad slot/var");
    if (var != kAnyVar && p->var_slot[var] < 0) return fail(MCF_ERR_ARG, "variable was not requested in out[]");
    if (step0 < 0 || nsteps < 0 || step0 + nsteps > (int64_t)p->ring_days * 24) return fail(MCF_ERR_ARG, "step range out of slot");
    return MCF_OK;
}

// host [rows x ncols] with leading dimension p->pitch -> dense device memory (and the other way): plain copies for dense hosts
hipError_t copy_in(mcf_plan* p, void* dev, const double* host, int64_t ncols) {
    if (p->pitch == p->rows) return hipMemcpyAsync(dev, host, (size_t)(p->rows * ncols) * 8, hipMemcpyHostToDevice, p->stream);
    return hipMemcpy2DAsync(dev, (size_t)p->rows * 8, host, (size_t)p->pitch * 8, (size_t)p->rows * 8, (size_t)ncols,
                            hipMemcpyHostToDevice, p->stream);
}
// `spatial`: n = rows x (cols x layers) values of a raster array (read with the plan's row pitch); else a plain vector
int upload(mcf_plan* p, const double* host, int64_t n, const double** dev, const char* name, bool spatial = true) {
    if (!host) return fail(MCF_ERR_ARG, std::string("missing input array: ") + name);
    double* d = nullptr;
    if (const int rc = p->dev.make(&d, n)) return rc;
    if (spatial && p->pitch != p->rows) HIP_TRY(copy_in(p, d, host, n / p->rows));
    else HIP_TRY(hipMemcpyAsync(d, host, (size_t)n * 8, hipMemcpyHostToDevice, p->stream));
    *dev = d;
    return MCF_OK;
}
// with a dtm, a terrain plane or the wetness index that is not given gets its buffer here and its values in derive_from_dtm
int upload_or_derive(mcf_plan* p, bool have_dtm, const double* host, int64_t n, const double** dev, const char* name) {
    if (host || !have_dtm) return upload(p, host, n, dev, name);
    return p->dev.make(dev, n);
}
// a set-up temporary of `own` with the host array's copy queued on the plan's stream (null host: the buffer alone)
template <class T>
int upload_temp(mcf_plan* p, mcf::DevOwner& own, const T* host, int64_t n, const T** dev) {
    T* d = nullptr;
    if (const int rc = own.make(&d, n)) return rc;
    if (host) HIP_TRY(hipMemcpyAsync(d, host, (size_t)n * sizeof(T), hipMemcpyHostToDevice, p->stream));
    *dev = d;
    return MCF_OK;
}

int check_inputs(const mcf_grid_inputs* in, const mcf_options* opt) {
    if (!in || !opt) return fail(MCF_ERR_ARG, "null inputs/options");
    if (in->rows <= 0 || in->cols <= 0) return fail(MCF_ERR_ARG, "rows/cols must be positive");
    if (in->tsteps < 0) return fail(MCF_ERR_ARG, "negative tsteps");
    if (in->tsteps > 0 && (!in->obstime.year || !in->obstime.month || !in->obstime.day || !in->obstime.hour))
        return fail(MCF_ERR_ARG, "obstime columns missing");
    if (in->array_forcing && (!in->lats || !in->lons)) return fail(MCF_ERR_ARG, "lats/lons missing");
    if (in->veg_layers > 1) {
        if (!in->lyr_st || !in->lyr_ed) return fail(MCF_ERR_ARG, "dfsel (lyr_st / lyr_ed) missing");
        for (int l = 0; l < in->veg_layers; ++l) {
            int span = in->lyr_ed[l] - in->lyr_st[l] + 1;
            if (span < 24)      // the reference's Rcpp::stop, src/microclimfCpp.cpp:2636-2637
                return fail(MCF_ERR_ARG, "Too many layers in vegp. Max layers must be <= max days");
            if (in->lyr_st[l] < 0 || in->lyr_st[l] % 24 != 0 || in->lyr_st[l] + (span / 24) * 24 > in->tsteps)
                return fail(MCF_ERR_ARG, "dfsel: layer ranges must start on whole days inside the series");
        }
    }
    if (!(opt->cells_per_block == 0 || opt->cells_per_block == 16 || opt->cells_per_block == 21 ||
          opt->cells_per_block == 32 || opt->cells_per_block == 42))
        return fail(MCF_ERR_ARG, "cells_per_block must be 0, 16, 21, 32 or 42");
    return MCF_OK;
}

int ensure_device(int device) {
    if (const int rc = mcf::check_device(device)) return rc;
    HIP_TRY(hipSetDevice(device));
    return MCF_OK;
}

const double* const* clim_ptrs(const mcf_grid_inputs* in, const double* out[15]) {
    // TF_TC .. TF_DTRP order
    out[0] = in->clim.tc; out[1] = in->clim.es; out[2] = in->clim.ea; out[3] = in->clim.tdew;
    out[4] = in->clim.pk; out[5] = in->clim.swdown; out[6] = in->clim.difrad; out[7] = in->clim.lwdown;
    out[8] = in->clim.windspeed; out[9] = in->pointm.soilm; out[10] = in->pointm.G;
    out[11] = in->pointm.umu; out[12] = in->pointm.kp; out[13] = in->pointm.muGp; out[14] = in->pointm.dtrp;
    return out;
}
const char* kRawNames[15] = {"tc", "es", "ea", "tdew", "pk", "swdown", "difrad", "lwdown", "windspeed",
                             "pointm$soilm", "pointm$G", "pointm$umu", "pointm$kp", "pointm$muGp",
                             "pointm$dtrp"};

// ---- plans that take the dtm (include/mcf.h mcf_dtm_spec) ---------------------------------------------------------------
struct DtmNeeds {
    bool slope, aspect, hor, svfa, wsa, twi;
    bool terrain() const { return slope || aspect || hor || wsa || svfa; }
    bool any() const { return terrain() || twi; }
};
DtmNeeds dtm_needs(const mcf_grid_inputs* in) {
    const mcf_soilc& s = in->soilc;
    return DtmNeeds{!s.slope, !s.aspect, !s.hor, !s.svfa, !s.wsa, !s.twi};
}
// halo rows the missing planes' stencils reach (mcf_precompute_terrain's rule; svfa from a given hor needs none)
int64_t dtm_halo_need(const DtmNeeds& nd, int s) {
    return nd.wsa ? 100 + 2 * s + s / 2 : (nd.hor ? 100 : (nd.slope || nd.aspect) ? 1 : 0);
}

int check_dtm(const mcf_grid_inputs* in, const mcf_dtm_spec* dtm) {
    if (!dtm->dtm) return fail(MCF_ERR_ARG, "mcf_dtm_spec: null dtm");
    if (dtm->halo_north < 0 || dtm->halo_south < 0 || !(dtm->xres > 0) || !(dtm->yres > 0))
        return fail(MCF_ERR_ARG, "mcf_dtm_spec: bad geometry or resolution");
    const int64_t rows_total = dtm->rows_total > 0 ? dtm->rows_total : in->rows;
    const int64_t row0 = dtm->rows_total > 0 ? dtm->row0 : 0;
    if (row0 < 0 || row0 + in->rows > rows_total) return fail(MCF_ERR_ARG, "block outside the raster");
    const DtmNeeds nd = dtm_needs(in);
    if ((nd.slope || nd.aspect || nd.hor || nd.wsa) && dtm->xres != dtm->yres)
        return fail(MCF_ERR_ARG, "terrain planes from the dtm need square cells (xres == yres), as the reference's .horizon does");
    if (nd.twi && (rows_total > in->rows || dtm->halo_north || dtm->halo_south))
        return fail(MCF_ERR_ARG, "flow accumulation does not tile: a row block of a larger raster must bring its twi");
    const int s = dtm->agg > 0 ? dtm->agg : 10;
    const int64_t need = dtm_halo_need(nd, s);
    if (dtm->halo_north < std::min(need, row0) || dtm->halo_south < std::min(need, rows_total - row0 - in->rows)) {
        char b[200];
        snprintf(b, sizeof b, "terrain block needs %lld halo rows (or all rows up to the raster edge)", (long long)need);
        return fail(MCF_ERR_ARG, b);
    }
    return MCF_OK;
}

// The missing planes, on the device, into the plan's buffers.  The dtm block and every scratch buffer are released on return.
int derive_from_dtm(mcf_plan* p, const mcf_grid_inputs* in, const mcf_dtm_spec* dtm) {
    const DtmNeeds nd = dtm_needs(in);
    if (!nd.any()) return MCF_OK;
    const double t_enter = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    HIP_TRY(hipStreamSynchronize(p->stream));           // the given planes are in place (svfa may read hor)
    const int64_t N = p->N;
    if (nd.svfa && !nd.hor) {                           // R/internal.R:1146-1149
        if (const int rc = mcf::svf_from_hor_device(p->d_hor, N, (double*)p->d_soil[12])) return rc;
        if (!(nd.slope || nd.aspect || nd.wsa || nd.twi)) return MCF_OK;
    }
    const int64_t RB = (int64_t)dtm->halo_north + p->rows + dtm->halo_south, NB = RB * p->cols;
    const bool timing = getenv("MCF_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    double t1 = t0, t2 = t0;
    mcf::DevOwner tmp;
    double* d_dtm = nullptr;
    if (const int rc = tmp.alloc((void**)&d_dtm, NB * 8)) return rc;
    HIP_TRY(hipMemcpy(d_dtm, dtm->dtm, (size_t)NB * 8, hipMemcpyHostToDevice));
    t1 = t2 = now();
    if (nd.slope || nd.aspect || nd.hor || nd.wsa) {
        mcf::TerrainDev t;
        memset(&t, 0, sizeof t);
        t.rows = p->rows; t.cols = p->cols; t.halo_north = dtm->halo_north; t.halo_south = dtm->halo_south;
        t.row0 = dtm->row0; t.rows_total = dtm->rows_total;
        t.d_dtm = d_dtm; t.res = dtm->xres; t.zref = p->opt.zref; t.agg = dtm->agg; t.aspect_na = 0.0;     // R/internal.R:1132-1136
        if (nd.slope) t.d_slope = (double*)p->d_soil[9];
        if (nd.aspect) t.d_aspect = (double*)p->d_soil[10];
        if (nd.hor) t.d_hor = (double*)p->d_hor;
        if (nd.hor && nd.svfa) t.d_svfa = (double*)p->d_soil[12];
        if (nd.wsa) t.d_wsa = (double*)p->d_wsa;
        if (const int rc = mcf::terrain_device(t)) return rc;
        // `slope[is.na(dtm)] <- NA` of the host marshaller
        if (nd.slope || nd.aspect)
            if (const int rc = mcf::mask_na_device(d_dtm, p->rows, p->cols, dtm->halo_north, dtm->halo_south, t.d_slope, t.d_aspect))
                return rc;
        t2 = now();
    }
    if (nd.twi)
        if (const int rc = mcf::topidx_device(d_dtm, p->rows, p->cols, dtm->xres, dtm->yres, (double*)p->d_soil[11], nullptr)) return rc;
    if (timing)
        fprintf(stderr, "[mcf] planes from the dtm: given planes in place %.3f s, dtm upload %.3f s, terrain %.3f s, wetness index %.3f s\n",
                t0 - t_enter, t1 - t0, t2 - t1, now() - t2);
    return MCF_OK;
}

int ensure_cells(mcf_plan* p) {
    if (p->cells_ready) return MCF_OK;
    for (int l = 0; l < p->layers; ++l) {
        mcf::CellSetupArgs a{};
        a.N = p->N;
        const int64_t lo = (int64_t)l * p->N;      // layer l of the [rows,cols,layers] vegetation arrays
        a.hgt = p->d_veg[0] + lo; a.pai = p->d_veg[1] + lo; a.x = p->d_veg[2] + lo; a.gsmax = p->d_veg[3] + lo;
        a.leafr = p->d_veg[4] + lo; a.leaft = p->d_veg[5] + lo; a.clump = p->d_veg[6] + lo; a.leafd = p->d_veg[7] + lo;
        a.paia = p->d_veg[8] + lo; a.leafden = p->d_veg[9] + lo;
        a.hgt0 = p->d_veg[0];
        a.Smin = p->d_soil[0]; a.Smax = p->d_soil[1]; a.gref = p->d_soil[2]; a.soilb = p->d_soil[3];
        a.Psie = p->d_soil[4]; a.Vq = p->d_soil[5]; a.Vm = p->d_soil[6]; a.Mc = p->d_soil[7];
        a.rho = p->d_soil[8]; a.slope = p->d_soil[9]; a.aspect = p->d_soil[10]; a.twi = p->d_soil[11];
        a.svfa = p->d_soil[12];
        a.hor = p->d_hor; a.wsa = p->d_wsa;
        a.lats = p->d_lats; a.lons = p->d_lons; a.lat = p->lat; a.lon = p->lon;
        a.crowpos = p->d_crowpos; a.ccolpos = p->d_ccolpos; a.rows = p->rows;
        a.elevd = p->d_elevd; a.pkfac = p->d_pkfac;
        a.tfact = p->opt.tfact;
        a.twi_mean = p->twi_mean;
        a.g = p->g;
        a.cpb = p->cpb;
        a.cellc = p->d_cellc + (int64_t)l * p->ntiles * mcf::tile_image_doubles(p->cpb);
        mcf::launch_cell_setup(a, p->stream);
        HIP_TRY(hipGetLastError());
    }
    if (!p->af && p->day_irregular.empty() && p->ndays > 0) {
        // the per-day flags of the time table, once: kStepIrregular and kSoilDaily in TF_IDX (its last field)
        const int tfc = mcf::time_field_count();
        std::vector<double> idx((size_t)p->ndays * 24);
        HIP_TRY(hipMemcpy2DAsync(idx.data(), 24 * 8, p->d_tt + (int64_t)(tfc - 1) * 24, (size_t)tfc * 24 * 8, 24 * 8,
                                 (size_t)p->ndays, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        static const bool no_share = getenv("MCF_NO_SOIL_SHARE") != nullptr;     // A/B runs
        p->day_irregular.assign((size_t)p->ndays, 0);
        p->day_soil_daily.assign((size_t)p->ndays, 0);
        for (int d = 0; d < p->ndays; ++d) {
            for (int h = 0; h < 24; ++h)
                if ((int)idx[(size_t)d * 24 + h] & mcf::step_irregular_bit()) p->day_irregular[(size_t)d] = 1;
            p->day_soil_daily[(size_t)d] = (!no_share && ((int)idx[(size_t)d * 24] & mcf::soil_daily_bit())) ? 1 : 0;
        }
    }
    if (p->fast_enabled) {
        int rc;
        const int64_t ntiles = p->ntiles;
        if (!p->d_tiles_slow && ((rc = p->dev.make(&p->d_tiles_fast, ntiles)) || (rc = p->dev.make(&p->d_tiles_slow, ntiles)))) return rc;
        if (!p->d_fix_count) {
            if ((rc = p->dev.make(&p->d_fix_count, 16))) return rc;
            HIP_TRY(hipMemsetAsync(p->d_fix_count, 0, 64, p->stream));
            if ((rc = p->dev.make(&p->d_fix_list, (int64_t)p->fix_cap * 2))) return rc;
        }
        // tile classes (the flags stay on the device for mcf_plan_run_days_cells)
        if (!p->d_tile_regular && (rc = p->dev.make(&p->d_tile_regular, ntiles))) return rc;
        uint8_t* d_flag = p->d_tile_regular;
        mcf::launch_tile_regular(p->d_cellc, p->N, p->layers, p->cpb, d_flag, p->stream);
        HIP_TRY(hipGetLastError());
        std::vector<uint8_t> flag((size_t)ntiles);
        HIP_TRY(hipMemcpyAsync(flag.data(), d_flag, (size_t)ntiles, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        std::vector<int32_t> fastl, slowl;
        fastl.reserve((size_t)ntiles);
        for (int64_t t = 0; t < ntiles; ++t) (flag[(size_t)t] ? fastl : slowl).push_back((int32_t)t);
        p->n_fast = (int64_t)fastl.size();
        p->n_slow = (int64_t)slowl.size();
        p->h_tiles_fast = fastl; p->h_tiles_slow = slowl;
        if (p->n_slow > 0) {     // with no irregular tile the fast launch needs no list (identity)
            HIP_TRY(hipMemcpy(p->d_tiles_fast, fastl.data(), fastl.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(p->d_tiles_slow, slowl.data(), slowl.size() * 4, hipMemcpyHostToDevice));
        }
    }
    p->cells_ready = true;     // only now: a failed allocation or copy above leaves the plan to try again, not half set up
    return MCF_OK;
}

// ---- plan set-up, step by step (plan_create is the list; the steps run in this order, and so do their refusals) -------------
// What steps hand to later ones and what the copies and kernels queued on the stream read: plan_create holds it until its last synchronise.
struct SetupScratch {
    std::vector<double> cpk_sea;            // coarse pressure reduced to sea level (altitude correction), [crows*ccols][T]
    std::vector<double> cwu, cwv, cwd;      // coarse wind components [crows*ccols][T] and the raster-mean direction per step
    mcf::DevOwner temps;                    // device copies of obstime, winddir and the vector forcing; the mxtc slab
    const int32_t *year = nullptr, *month = nullptr, *day = nullptr;
    const double *hour = nullptr, *winddir = nullptr;
};

// coarse array forcing, what the host can judge; leaves: crows / ccols, altcorrect, coarse_lds
int coarse_check(mcf_plan* p, const mcf_grid_inputs* in, const mcf_options* opt) {
    if (!p->coarse) return MCF_OK;
    if (in->coarse_rows < 1 || in->coarse_cols < 1 || !in->coarse_rowpos || !in->coarse_colpos || !in->coarse_relhum ||
        !in->coarse_winddir)
        return fail(MCF_ERR_ARG, "coarse array forcing needs coarse_rows/cols, coarse_rowpos/colpos, coarse_relhum and coarse_winddir");
    // (the solver addresses a day of a coarse field with 32-bit byte offsets: 24 x cells x 8 B < 2^32)
    if ((int64_t)in->coarse_rows * in->coarse_cols > 11000000) return fail(MCF_ERR_ARG, "coarse grid too large (more than 1.1e7 cells)");
    if (p->bg && !opt->complete) return fail(MCF_ERR_ARG, "coarse array forcing: reqhgt < 0 needs complete = 1");
    for (int64_t i = 0; i < in->rows; ++i)
        if (!(in->coarse_rowpos[i] >= 0.0 && in->coarse_rowpos[i] <= in->coarse_rows - 1))
            return fail(MCF_ERR_ARG, "coarse_rowpos must lie in [0, coarse_rows - 1]");
    for (int64_t j = 0; j < in->cols; ++j)
        if (!(in->coarse_colpos[j] >= 0.0 && in->coarse_colpos[j] <= in->coarse_cols - 1))
            return fail(MCF_ERR_ARG, "coarse_colpos must lie in [0, coarse_cols - 1]");
    p->crows = in->coarse_rows; p->ccols = in->coarse_cols;
    p->altcorrect = in->coarse_altcorrect;
    // the LDS-staged taps (k_solve, CLDS): a tile's 32 cells lie in at most two raster columns and, in each, reach at most
    // four coarse rows (the rows of its first and last cell and one more)
    p->coarse_lds = in->rows >= 32 && getenv("MCF_NO_COARSE_LDS") == nullptr;
    // ... with row positions that do not decrease down a raster column: the kernel finds a tile's wrap into the next column
    // where the position falls back, and the window test below looks at a window's two ends only.  A flipped or otherwise
    // non-monotone coarse grid takes the per-lane taps, which make no such assumption.
    for (int64_t i = 1; p->coarse_lds && i < in->rows; ++i)
        if (in->coarse_rowpos[i] < in->coarse_rowpos[i - 1]) p->coarse_lds = false;
    for (int64_t i = 0; p->coarse_lds && i < in->rows; ++i) {
        const int64_t l = std::min<int64_t>(i + 31, in->rows - 1);
        if (floor(in->coarse_rowpos[l]) - floor(in->coarse_rowpos[i]) + 2 > 4) p->coarse_lds = false;
    }
    if (p->altcorrect < 0 || p->altcorrect > 2) return fail(MCF_ERR_ARG, "coarse_altcorrect must be 0, 1 or 2");
    if (p->altcorrect && (!in->coarse_dtm || !in->fine_dtm))
        return fail(MCF_ERR_ARG, "altitude correction needs coarse_dtm and fine_dtm");
    return MCF_OK;
}

// leaves: geometry and pitch, the plan's kind (af, coarse, bg, bg_stream), coarse_check's, cpb / ntiles, layers, opt, the ring's days and slots
int plan_shape(mcf_plan* p, const mcf_grid_inputs* in, const mcf_options* opt, int32_t ring_days, int32_t ring_slots, bool streamed) {
    p->rows = in->rows; p->cols = in->cols; p->N = in->rows * in->cols; p->tsteps = in->tsteps;
    p->pitch = host_pitch(in);
    if (p->pitch < p->rows) return fail(MCF_ERR_ARG, "row_pitch smaller than rows");
    p->ndays = (int)(in->tsteps / 24);                       // cpp:2116 truncation
    p->af = in->array_forcing != 0;
    p->coarse = in->array_forcing == 2;
    p->bg = opt->reqhgt < 0.0;
    p->bg_stream = p->bg && streamed;
    if (const int rc = coarse_check(p, in, opt)) return rc;
    // vector forcing: two 8-wave workgroups per CU (21 cells); array forcing: one 12-wave workgroup
    p->cpb = opt->cells_per_block ? opt->cells_per_block : (in->array_forcing ? 32 : 21);
    // coarse array forcing is built for 32-cell tiles only: tile classes, tile lists and the ring's blocks must agree
    if (p->coarse) p->cpb = 32;
    if (in->array_forcing && p->cpb == 42) p->cpb = 32;      // 42-cell tiles are built for vector forcing only (they would spill)
    if (p->N >= ((int64_t)1 << 31)) return fail(MCF_ERR_ARG, "at most 2^31 - 1 cells per plan (row-tile larger rasters)");
    p->ntiles = (p->N + p->cpb - 1) / p->cpb;
    static const bool no_fast = getenv("MCF_NO_FAST_CLAMPS") != nullptr;     // A/B runs
    p->fast_enabled = !no_fast && !(opt->reqhgt < 0.0);
    p->layers = in->veg_layers > 1 ? in->veg_layers : 1;
    p->opt = *opt;
    p->lat = in->lat; p->lon = in->lon;
    if (ring_slots < 1) ring_slots = 1;
    if (ring_days < 1) ring_days = 1;
    // (streamed below ground: a slot may hold one day more, for the steps behind the last whole day)
    const int max_days = p->bg_stream ? (int)std::max<int64_t>((in->tsteps + 23) / 24, 1) : std::max(p->ndays, 1);
    if (ring_days > max_days) ring_days = max_days;
    // reqhgt < 0 smooths the whole series (incl. steps past the last whole day, which read as 0)
    if (p->bg && !p->bg_stream) { ring_slots = 1; ring_days = (int)std::max<int64_t>((in->tsteps + 23) / 24, 1); }
    // array forcing re-lays a slot's series with one launch row per step (gridDim.y <= 65535): 2730 whole days at most
    if (in->array_forcing == 1 && ring_days > 2730) ring_days = 2730;
    p->ring_days = ring_days; p->ring_slots = ring_slots;
    return MCF_OK;
}

// leaves: d_veg, d_soil, d_wsa, d_hor (given, or derived from the dtm), d_lats / d_lons (array forcing), valid_cells
// foliage_later: paia and leafden get their buffers only; mcf_plan_set_height fills them before the first run (mcf_runmicro_heights)
int upload_static(mcf_plan* p, const mcf_grid_inputs* in, const mcf_dtm_spec* dtm, bool foliage_later) {
    int rc;
    const int64_t N = p->N;
    const double* veg[10] = {in->vegp.hgt, in->vegp.pai, in->vegp.x, in->vegp.gsmax, in->vegp.leafr,
                             in->vegp.leaft, in->vegp.clump, in->vegp.leafd, in->vegp.paia, in->vegp.leafden};
    const char* vegn[10] = {"hgt", "pai", "x", "gsmax", "leafr", "leaft", "clump", "leafd", "paia", "leafden"};
    for (int i = 0; i < 10; ++i)
        if ((rc = foliage_later && i >= 8 ? p->dev.make(&p->d_veg[i], N * p->layers) : upload(p, veg[i], N * p->layers, &p->d_veg[i], vegn[i])))
            return rc;
    const double* soil[13] = {in->soilc.Smin, in->soilc.Smax, in->soilc.gref, in->soilc.soilb, in->soilc.Psie,
                              in->soilc.Vq, in->soilc.Vm, in->soilc.Mc, in->soilc.rho, in->soilc.slope,
                              in->soilc.aspect, in->soilc.twi, in->soilc.svfa};
    const char* soiln[13] = {"Smin", "Smax", "gref", "soilb", "Psie", "Vq", "Vm", "Mc", "rho", "slope",
                             "aspect", "twi", "svfa"};
    for (int i = 0; i < 13; ++i)      // (slope, aspect, twi and svfa can come from the dtm)
        if ((rc = upload_or_derive(p, dtm && i >= 9, soil[i], N, &p->d_soil[i], soiln[i]))) return rc;
    if ((rc = upload_or_derive(p, dtm, in->soilc.wsa, N * 8, &p->d_wsa, "wsa"))) return rc;
    if ((rc = upload_or_derive(p, dtm, in->soilc.hor, N * 24, &p->d_hor, "hor"))) return rc;
    if (dtm && (rc = derive_from_dtm(p, in, dtm))) return rc;
    if (p->af) {
        if ((rc = upload(p, in->lats, N, &p->d_lats, "lats"))) return rc;
        if ((rc = upload(p, in->lons, N, &p->d_lons, "lons"))) return rc;
    }
    p->valid_cells = 0;
    for (int64_t j = 0; j < in->cols; ++j)
        for (int64_t i = 0; i < in->rows; ++i) p->valid_cells += !std::isnan(in->vegp.hgt[i + p->pitch * j]);
    return MCF_OK;
}

// coarse array forcing; leaves: d_crowpos / d_ccolpos, with altitude correction d_elevd / d_pkfac and s.cpk_sea
int coarse_planes(mcf_plan* p, const mcf_grid_inputs* in, SetupScratch& s) {
    if (!p->coarse) return MCF_OK;
    int rc;
    const int64_t N = p->N;
    if ((rc = upload(p, in->coarse_rowpos, in->rows, &p->d_crowpos, "coarse_rowpos", false))) return rc;
    if ((rc = upload(p, in->coarse_colpos, in->cols, &p->d_ccolpos, "coarse_colpos", false))) return rc;
    if (!p->altcorrect) return MCF_OK;
    // R/internal.R:1236-1241: psl = pk / ((293 - 0.0065 zc) / 293)^5.26 on the coarse grid, back up with the
    // fine elevation after resampling; elevd = resample(dtmc) - dtm
    const int cr = p->crows, cc = p->ccols;
    std::vector<double> zc((size_t)cr * cc), elevd((size_t)N), pkfac((size_t)N);
    for (size_t q = 0; q < zc.size(); ++q) zc[q] = std::isnan(in->coarse_dtm[q]) ? 0.0 : in->coarse_dtm[q];
    for (int64_t j = 0; j < in->cols; ++j) {
        const double cp = in->coarse_colpos[j], fc = floor(cp), wx = cp - fc;
        const int c0 = (int)fc, c1 = c0 + 1 < cc ? c0 + 1 : c0;
        for (int64_t i = 0; i < in->rows; ++i) {
            const double rp = in->coarse_rowpos[i], fr = floor(rp), wy = rp - fr;
            const int r0 = (int)fr, r1 = r0 + 1 < cr ? r0 + 1 : r0;
            const double top = (1.0 - wx) * zc[(size_t)(r0 + cr * c0)] + wx * zc[(size_t)(r0 + cr * c1)];
            const double bot = (1.0 - wx) * zc[(size_t)(r1 + cr * c0)] + wx * zc[(size_t)(r1 + cr * c1)];
            const double z = in->fine_dtm[i + p->pitch * j];
            elevd[(size_t)(i + in->rows * j)] = ((1.0 - wy) * top + wy * bot) - z;
            pkfac[(size_t)(i + in->rows * j)] = pow((293.0 - 0.0065 * z) / 293.0, 5.26);
        }
    }
    if ((rc = upload(p, elevd.data(), N, &p->d_elevd, "elevd", false))) return rc;
    if ((rc = upload(p, pkfac.data(), N, &p->d_pkfac, "pkfac", false))) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));      // elevd and pkfac have been read
    if (in->tsteps > 0 && in->clim.pk) {
        const int64_t cN = (int64_t)cr * cc;
        s.cpk_sea.resize((size_t)(cN * in->tsteps));
        for (int64_t k = 0; k < in->tsteps; ++k)
            for (int64_t q = 0; q < cN; ++q)
                s.cpk_sea[(size_t)(q + cN * k)] = in->clim.pk[q + cN * k] / pow((293.0 - 0.0065 * zc[(size_t)q]) / 293.0, 5.26);
    }
    return MCF_OK;
}

// leaves: the solver's globals g (dTmx: the time tables), hiy, and the one global reduction — the mean of log(twi)/tfact, cpp:993-1004
int solver_constants(mcf_plan* p, const mcf_grid_inputs* in, const mcf_options* opt) {
    p->g.reqhgt = opt->reqhgt;
    p->g.reqhgt2 = opt->reqhgt < 0.00001 ? 0.00001 : opt->reqhgt;      // cpp:2246-2247
    p->g.zref = opt->zref;
    p->g.hf0p = mcf::hf_pow02(1 / 999.99);   // mincondCpp(leafabs, 999.99, ...) at cpp:1348
    p->g.hf500p = mcf::hf_pow02(500.0);      // rs capped at 500 (gs <= 0.002), cpp:1321-1323
    p->g.shadowmask = p->af ? 0 : 1;
    p->g.dTmx = 0.0;
    p->hiy = 365 * 24;
    if (p->tsteps > 0 && in->obstime.year[0] % 4 == 0) p->hiy = 366 * 24;      // cpp:2171-2172
    if (const int rc = p->dev.make(&p->d_twi2, (int64_t)mcf::twi_scratch_doubles())) return rc;
    mcf::launch_twi_partial(p->d_soil[11], p->N, opt->tfact, p->d_twi2, p->stream);
    double h2[2];
    HIP_TRY(hipMemcpyAsync(h2, p->d_twi2, 16, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->twi_sum = h2[0];
    p->twi_count = (int64_t)h2[1];
    p->twi_mean = h2[0] / h2[1];
    return MCF_OK;
}

// leaves: d_cellc zeroed (ensure_cells fills it before the first run), with layered vegetation d_daylayer / daylayer0
int cell_images(mcf_plan* p, const mcf_grid_inputs* in) {
    int rc;
    // per-cell constants, tile-major (mcf_kernels.h CellSetupArgs); zeroed once: the cells past the raster's end in the last
    // tile's image are read (not used) by the solver
    const int64_t cellc_doubles = (int64_t)p->layers * p->ntiles * mcf::tile_image_doubles(p->cpb);
    if ((rc = p->dev.make(&p->d_cellc, cellc_doubles))) return rc;
    HIP_TRY(hipMemsetAsync(p->d_cellc, 0, (size_t)cellc_doubles * 8, p->stream));
    if (p->layers <= 1) return MCF_OK;
    // day -> layer map from dfsel (cpp:2629-2640, k = dy*24 + hr + st[lyr]); -1 = not covered
    std::vector<int32_t> dl((size_t)std::max(p->ndays, 1), -1);
    for (int l = 0; l < p->layers; ++l) {
        int nd = (in->lyr_ed[l] - in->lyr_st[l] + 1) / 24, d0 = in->lyr_st[l] / 24;
        for (int d = d0; d < d0 + nd && d < p->ndays; ++d) dl[d] = l;
    }
    if ((rc = p->dev.make(&p->d_daylayer, (int64_t)dl.size()))) return rc;
    p->daylayer0 = dl;
    HIP_TRY(hipMemcpyAsync(p->d_daylayer, dl.data(), dl.size() * 4, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MCF_OK;
}

// leaves: s.cwu / s.cwv, the wind components per coarse cell, and s.cwd, the raster-mean direction per step (R/internal.R:1255-1264)
void coarse_wind(const mcf_plan* p, const mcf_grid_inputs* in, SetupScratch& s) {
    const int64_t T = p->tsteps, cN = (int64_t)p->crows * p->ccols;
    s.cwu.resize((size_t)(cN * T)); s.cwv.resize((size_t)(cN * T)); s.cwd.resize((size_t)T);
    for (int64_t k = 0; k < T; ++k) {
        double su = 0, sv = 0;
        int64_t nu = 0, nv = 0;
        for (int64_t q = 0; q < cN; ++q) {
            const double u2 = in->clim.windspeed[q + cN * k], wd = in->coarse_winddir[q + cN * k] * M_PI / 180.0;
            const double u = u2 * cos(wd), v = u2 * sin(wd);
            s.cwu[(size_t)(q + cN * k)] = u; s.cwv[(size_t)(q + cN * k)] = v;
            if (!std::isnan(u)) { su += u; ++nu; }               // apply(wu, 3, mean, na.rm = TRUE)
            if (!std::isnan(v)) { sv += v; ++nv; }
        }
        double d = fmod(atan2(sv / (double)nv, su / (double)nu) * 180.0 / M_PI, 360.0);
        if (d < 0) d += 360.0;                                    // R's %% takes the sign of the divisor
        s.cwd[(size_t)k] = d;
    }
}

// the plan's forcing series are all there; leaves: the device copies of obstime and of the wind direction (coarse: coarse_wind's) in s
int time_inputs(mcf_plan* p, const mcf_grid_inputs* in, SetupScratch& s) {
    const int64_t T = p->tsteps;
    if (T <= 0) return MCF_OK;
    const double* raw[15];
    clim_ptrs(in, raw);
    for (int f = 0; f < 15; ++f)
        if (!raw[f] && !(p->coarse && f >= 1 && f <= 3))     // es, ea, tdew are derived in coarse mode
            return fail(MCF_ERR_ARG, std::string("missing forcing array: ") + kRawNames[f]);
    if (!p->coarse && !in->clim.winddir) return fail(MCF_ERR_ARG, "missing forcing array: winddir");
    if (p->coarse) coarse_wind(p, in, s);
    int rc;
    if ((rc = upload_temp(p, s.temps, in->obstime.year, T, &s.year)) || (rc = upload_temp(p, s.temps, in->obstime.month, T, &s.month)) ||
        (rc = upload_temp(p, s.temps, in->obstime.day, T, &s.day)) || (rc = upload_temp(p, s.temps, in->obstime.hour, T, &s.hour)))
        return rc;
    return upload_temp(p, s.temps, p->coarse ? s.cwd.data() : in->clim.winddir, T, &s.winddir);
}

// vector forcing; leaves: g.dTmx from the series' maximum air temperature, and d_tt, the table of every day's 24 steps
int time_tables_vector(mcf_plan* p, const mcf_grid_inputs* in, SetupScratch& s) {
    int rc;
    const int64_t T = p->tsteps;
    double mxtc = -273.15;                                           // cpp:2159-2168
    for (int64_t k = 0; k < T; ++k)
        if (in->clim.tc[k] > mxtc) mxtc = in->clim.tc[k];
    p->g.dTmx = -0.6273 * mxtc + 49.79;                              // cpp:1236
    if ((rc = p->dev.make(&p->d_tt, (int64_t)std::max(p->ndays, 1) * mcf::time_field_count() * 24))) return rc;
    if (p->ndays <= 0) return MCF_OK;
    const double* raw[15];
    clim_ptrs(in, raw);
    mcf::TimeSetupArgs ta{};
    ta.nsteps = p->ndays * 24;
    ta.year = s.year; ta.month = s.month; ta.day = s.day; ta.hour = s.hour; ta.winddir = s.winddir;
    for (int f = 0; f < 15; ++f)
        if ((rc = upload_temp(p, s.temps, raw[f], T, &ta.raw[f]))) return rc;
    ta.lat = in->lat; ta.lon = in->lon;
    ta.tt = p->d_tt;
    mcf::launch_time_setup(ta, p->stream);
    HIP_TRY(hipGetLastError());
    return MCF_OK;
}
// array forcing, fine and coarse; leaves: d_dt and d_windex filled from the dates, d_mxtc allocated
int time_tables_array(mcf_plan* p, SetupScratch& s) {
    int rc;
    const int64_t T = p->tsteps;
    if ((rc = p->dev.make(&p->d_dt, std::max<int64_t>(T, 1) * 4)) || (rc = p->dev.make(&p->d_windex, std::max<int64_t>(T, 1))) ||
        (rc = p->dev.make(&p->d_mxtc, p->N)))
        return rc;
    if (T <= 0) return MCF_OK;
    mcf::DateSetupArgs da{};
    da.nsteps = (int)T;
    da.year = s.year; da.month = s.month; da.day = s.day; da.hour = s.hour; da.winddir = s.winddir;
    da.dt = p->d_dt; da.windex = p->d_windex;
    mcf::launch_date_setup(da, p->stream);
    HIP_TRY(hipGetLastError());
    return MCF_OK;
}
// coarse array forcing; leaves: d_force, the 15 coarse slabs' whole series resident ([15][crows*ccols][T]), d_mxtc (k_mxtc_coarse)
int time_tables_coarse(mcf_plan* p, const mcf_grid_inputs* in, SetupScratch& s) {
    int rc;
    if ((rc = time_tables_array(p, s))) return rc;
    const int64_t T = p->tsteps, cN = (int64_t)p->crows * p->ccols, slab = cN * std::max<int64_t>(T, 1);
    if ((rc = p->dev.make(&p->d_force, 15 * slab))) return rc;
    const double* src[15];
    clim_ptrs(in, src);
    src[1] = in->coarse_relhum;                    // slot TF_ES
    src[2] = s.cwv.data();                         // slot TF_EA: v component
    src[3] = nullptr;                              // slot TF_TDEW unused
    if (p->altcorrect) src[4] = s.cpk_sea.data();  // slot TF_PK: sea-level pressure
    src[8] = s.cwu.data();                         // slot TF_U2: u component
    for (int f = 0; f < 15 && T > 0; ++f)
        if (src[f]) HIP_TRY(hipMemcpyAsync(p->d_force + f * slab, src[f], (size_t)(cN * T * 8), hipMemcpyHostToDevice, p->stream));
    if (T > 0) {
        mcf::launch_mxtc_coarse(p->d_force, slab, p->crows, p->ccols, (int)T, p->d_crowpos, p->d_ccolpos, p->rows, p->N,
                                p->altcorrect, p->d_elevd, p->d_pkfac, p->d_mxtc, p->stream);
        HIP_TRY(hipGetLastError());
    } else {
        mcf::launch_fill(p->d_mxtc, p->N, -273.15, p->stream);
    }
    // the slabs are on the device before anything else is queued (their sources: s.cwu / s.cwv / s.cpk_sea, which plan_create
    // holds until its own synchronise, and the caller's arrays)
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->force_day0.assign(p->ring_slots, 0);
    p->force_ndays.assign(p->ring_slots, p->ndays);
    return MCF_OK;
}
// fine array forcing; leaves: d_mxtc over the WHOLE series (cpp:2467-2471), the tiled forcing ring d_force (empty) and its staging slab
int time_tables_fine(mcf_plan* p, const mcf_grid_inputs* in, SetupScratch& s) {
    int rc;
    if ((rc = time_tables_array(p, s))) return rc;
    const int64_t T = p->tsteps, N = p->N;
    mcf::launch_fill(p->d_mxtc, N, -273.15, p->stream);
    const int64_t slab_steps = std::max<int64_t>(1, std::min<int64_t>(T, (int64_t)(256LL << 20) / (N * 8)));
    if (T > 0) {      // streamed in slabs
        const double* dslab = nullptr;
        if ((rc = upload_temp<double>(p, s.temps, nullptr, slab_steps * N, &dslab))) return rc;
        for (int64_t k0 = 0; k0 < T; k0 += slab_steps) {
            const int64_t ns = std::min(slab_steps, T - k0);
            HIP_TRY(copy_in(p, const_cast<double*>(dslab), in->clim.tc + p->pitch * p->cols * k0, p->cols * ns));
            mcf::launch_mxtc(dslab, N, (int)ns, p->d_mxtc, p->stream);
        }
        HIP_TRY(hipGetLastError());
    }
    // forcing ring, TILED like the output ring: [slots][tile][day][15 series][ring_block_doubles(cpb)] in the solver's lane
    // order, so that a workgroup's 360 loads per day (15 series x 24 hours, each 8 B x N x hour apart in the caller's
    // arrays) become whole lines of one contiguous 90 KB run; mcf_plan_upload_forcing_days re-lays each series on the
    // device behind its host-to-device copy
    p->force_day_stride = 15 * (int64_t)mcf::ring_block_doubles(p->cpb);
    p->force_tile_stride = (int64_t)p->ring_days * p->force_day_stride;
    p->force_slot_elems = p->ntiles * p->force_tile_stride;
    if ((rc = p->dev.make(&p->d_force, (int64_t)p->ring_slots * p->force_slot_elems))) return rc;
    if ((rc = p->dev.make(&p->d_force_stage, N * (int64_t)p->ring_days * 24))) return rc;     // one series of one slot, as uploaded
    p->force_day0.assign(p->ring_slots, -1);
    p->force_ndays.assign(p->ring_slots, 0);
    return MCF_OK;
}

// leaves: var_slot / nvars, the ring's geometry — tiled, or linear for whole-series below ground — and d_ring
int output_ring(mcf_plan* p, const mcf_options* opt) {
    p->nvars = 0;
    for (int v = 0; v < MCF_NOUT; ++v) p->var_slot[v] = opt->out[v] ? p->nvars++ : -1;
    p->tiled = !p->bg || p->bg_stream;
    if (p->tiled) {
        const int64_t blk = mcf::ring_block_doubles(p->cpb);
        p->ring_var_stride = blk;
        p->ring_day_stride = (int64_t)std::max(p->nvars, 1) * blk;
        p->ring_tile_stride = (int64_t)p->ring_days * p->ring_day_stride;
        p->slot_elems = p->ntiles * p->ring_tile_stride;
    } else {
        p->slot_elems = (int64_t)std::max(p->nvars, 1) * p->N * (int64_t)p->ring_days * 24;
    }
    return p->dev.make(&p->d_ring, (int64_t)p->ring_slots * p->slot_elems);
}

// below ground in day chunks: O(cells x days) of state, no [N][tsteps] buffer.  Leaves: the Tg ring, d_ddsum, the sweep's state or Tgp / Tbp
int below_stream_state(mcf_plan* p, const mcf_grid_inputs* in, const mcf_options* opt) {
    if (!(p->bg_stream && opt->out[MCF_OUT_TZ])) return MCF_OK;
    int rc;
    const int64_t N = p->N, nd = std::max(p->ndays, 1);
    p->tg_tile_stride = (int64_t)p->ring_days * mcf::ring_block_doubles(p->cpb);
    if ((rc = p->dev.make(&p->d_tgring, p->ntiles * p->tg_tile_stride)) || (rc = p->dev.make(&p->d_ddsum, N))) return rc;
    if (opt->complete) {
        if ((rc = p->dev.make(&p->d_hsum, N)) || (rc = p->dev.make(&p->d_dmean, N * nd)) || (rc = p->dev.make(&p->d_ybuf, N * nd)) ||
            (rc = p->dev.make(&p->d_wrap, N * mcf::kBelowWin)))
            return rc;
        return p->dev.make(&p->d_prev, N * mcf::kBelowWin);
    }
    if (p->af) {
        // per cell-step: each slot's days, uploaded with its forcing (mcf_plan_upload_forcing_days)
        const int64_t n = (int64_t)p->ring_slots * p->ring_days * 24 * N;
        if ((rc = p->dev.make(&p->d_Tgp_slots, n)) || (rc = p->dev.make(&p->d_Tbp_slots, n))) return rc;
        if (!in->pointm.Tg || !in->pointm.Tbp) return fail(MCF_ERR_ARG, "missing input array: pointm$Tg / pointm$Tbp");
        return MCF_OK;
    }
    if ((rc = upload(p, in->pointm.Tg, p->tsteps, &p->d_Tgp, "pointm$Tg", false))) return rc;
    return upload(p, in->pointm.Tbp, p->tsteps, &p->d_Tbp, "pointm$Tbp", false);
}
// below ground over the whole series; leaves: d_tgser and d_ddsum zeroed, d_scratch, with complete = 0 the point model's Tg / Tbp
int below_series_state(mcf_plan* p, const mcf_grid_inputs* in, const mcf_options* opt) {
    if (!(p->bg && !p->bg_stream)) return MCF_OK;
    int rc;
    const int64_t N = p->N, T = p->tsteps;
    if ((rc = p->dev.make(&p->d_tgser, N * std::max<int64_t>(T, 1)))) return rc;
    // steps past the last whole day read as 0 in the reference (std::vector<double> Tg(tsteps))
    mcf::launch_fill(p->d_tgser, N * T, 0.0, p->stream);
    if ((rc = p->dev.make(&p->d_ddsum, N))) return rc;
    mcf::launch_fill(p->d_ddsum, N, 0.0, p->stream);
    if ((rc = p->dev.make(&p->d_scratch, N * 2 * (int64_t)std::max(p->ndays, 1)))) return rc;
    if (opt->complete) return MCF_OK;
    const int64_t n = p->af ? N * T : T;
    if ((rc = upload(p, in->pointm.Tg, n, &p->d_Tgp, "pointm$Tg", p->af))) return rc;
    return upload(p, in->pointm.Tbp, n, &p->d_Tbp, "pointm$Tbp", p->af);
}

// ---- what the one-call entries share (run_oneshot, run_summary, run_depths, run_bioclim) ------------------------------------
// The day-chunk driver: days [0, ndays) through slot 0 of `p`, `chunk` at a time — the chunk's forcing uploaded (array
// forcing; a coarse plan's series is resident and the upload returns at once), its days run, then sink(d0, nd).
template <class Sink>
int for_day_chunks(mcf_plan* p, const mcf_grid_inputs* in, int ndays, int chunk, Sink&& sink) {
    for (int d0 = 0; d0 < ndays; d0 += chunk) {
        const int nd = std::min(chunk, ndays - d0);
        int rc;
        if (in->array_forcing && (rc = mcf_plan_upload_forcing_days(p, in, d0, nd, 0))) return rc;
        if ((rc = mcf_plan_run_days(p, d0, nd, 0))) return rc;
        if ((rc = sink(d0, nd))) return rc;
    }
    return MCF_OK;
}

// Chunk size, ring-budget family (the sinks that keep nothing but a ring: bioclim, summaries): the days of a tiled ring of
// `slabs` blocks per tile and day that fit the budget of environment variable `env` in GB (default 14), at least one.
int ring_budget_days(const char* env, int slabs, int64_t N, int cpb) {
    const double day_bytes = 8.0 * slabs * (double)((N + cpb - 1) / cpb) * (double)mcf::ring_block_doubles(cpb);
    const char* e = getenv(env);
    const double budget = (e && atof(e) > 0.0 ? atof(e) : 14.0) * 1e9;     // (4096^2 bioclim: 0.80 s with 14 GB = two-day chunks, 0.85 s with 8, 2.3 s with 27 — the allocation; profiles/r05_sink_rates.txt)
    return (int)std::max(1.0, floor(budget / day_bytes));
}

// Chunk size, free-memory family (the entries whose chunks go to the host: run_oneshot, run_depths): the days of `slabs`
// untiled [N][24] slabs that fit 0.6 of this caller's share of the free HBM, less 200 doubles per cell for the plan's planes,
// less `state_doubles` per cell of below-ground state, less one day more in the slot for a tail; 1 .. 64, and no more than ndays.
// (The amounts taken off are whole numbers of bytes: each subtraction is exact while the budget stays positive, so their
// order is free, and a negative budget gives one day whatever its value.)
int free_memory_chunk_days(int64_t N, int ndays, int sharers, int slabs, double state_doubles, bool tail, int* chunk) {
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    const double per_day = (double)N * 24 * 8 * slabs;
    const double budget = 0.6 * (double)fr / std::max(sharers, 1) - (double)N * 8 * 200 - (double)N * 8 * state_doubles -
                          (tail ? per_day : 0.0);
    *chunk = std::min((int)std::max(1.0, std::min((double)std::max(ndays, 1), budget / std::max(per_day, 1.0))), 64);
    return MCF_OK;
}
// per-cell doubles of a streamed below-ground plan's state with D depths: dmean and a ybuf per depth, wrap, prev, the two sums
double below_state_doubles(int D, int ndays) { return (1.0 + D) * ndays + 2 * mcf::kBelowWin + 2; }
// ... and of the bioclim sink on it: 21 temperature rows per depth and 8 moisture rows, then the matrices of the finish
double bioclim_state_doubles(int D) { return (mcf::kBioTempRows + 11.0) * D + 2 * mcf::kBioMoistRows; }

// steps past the last whole day of a caller's [rows, cols, tsteps] array: never computed by the reference, they stay NA (cpp:2116)
void fill_tail_na(double* buf, const mcf_grid_inputs* in, int ndays) {
    const int64_t pitch = host_pitch(in), HS = pitch * in->cols;
    const double na = mcf::na_real_host();
    for (int64_t k = (int64_t)ndays * 24; k < in->tsteps; ++k)
        for (int64_t j = 0; j < in->cols; ++j)
            for (int64_t i = 0; i < in->rows; ++i) buf[i + pitch * j + HS * k] = na;
}

// The sink of a one-call entry's chunked run (run_sink above ground, run_depths below), built by the entry that has judged its
// arguments.  What the driver needs before the plan exists: the variables the plan is created with, the per-cell doubles of
// device state the sink adds to a below-ground plan's, and `check` (may be empty), the sink's refusals that need no device,
// made behind the driver's own.  Then its three steps on the plan.
struct RunSink {
    int32_t out[MCF_NOUT] = {};
    double state_doubles = 0.0;
    std::function<int()> check;
    std::function<int(mcf_plan*)> enable;
    std::function<int(mcf_plan*, int, int)> fold;      // days [d0, d0 + nd) lie in slot 0
    std::function<int(mcf_plan*)> finish;
};
int run_sink_chunks(mcf_plan* p, const mcf_grid_inputs* in, int ndays, int chunk, const RunSink& sink) {
    int rc = sink.enable(p);
    if (rc) return rc;
    if ((rc = for_day_chunks(p, in, ndays, chunk, [&](int d0, int nd) { return sink.fold(p, d0, nd); }))) return rc;
    if ((rc = sink.finish(p))) return rc;
    return mcf_plan_sync(p);
}

// the four quarter-index vectors of a bioclim call (wet, dry, hot, cold) as plan buffers, their copies queued on its stream
int upload_quarters(mcf_plan* p, const int32_t* const q[4], const int32_t nq[4], const int32_t* dq[4]) {
    for (int i = 0; i < 4; ++i) {
        int32_t* d = nullptr;
        if (const int rc = p->dev.make(&d, (int64_t)std::max(nq[i], 1))) return rc;
        if (nq[i] > 0) HIP_TRY(hipMemcpyAsync(d, q[i], (size_t)nq[i] * 4, hipMemcpyHostToDevice, p->stream));
        dq[i] = d;
    }
    return MCF_OK;
}

}  // namespace

// ---- writetonc sink (R/dataprep.R:1063-1260) -------------------------------------------------------------------
// struct mcf_ncfile: mcf_ncsink.hpp (mcf_snow.hip writes the snowpack's records into it too)

namespace {

std::string r_number(double x) {   // as.character(<double>): 15 significant digits
    char b[64];
    snprintf(b, sizeof b, "%.15g", x);
    return b;
}

// variables writetonc defines for a height, with its long names and units (dataprep.R:1097-1157, 1180-1214, 1234-1244)
bool nc_var_def(int v, double reqhgt, mcf::NcVarDef* d, double* scale, bool* put_by_reference) {
    static const char* names[MCF_NOUT] = {"Tz", "tleaf", "relhum", "soilm", "windspeed", "Rdirdown", "Rdifdown",
                                          "Rlwdown", "Rswup", "Rlwup"};
    static const char* radlong[5] = {"Downward direct shortwave radiation", "Downward diffuse shortwave radiation",
                                     "Downward longwave radiation", "Upward shortwave radiation", "Upward longwave radiation"};
    d->name = names[v];
    *put_by_reference = true;
    const std::string h = r_number(fabs(reqhgt));
    if (v >= 5) {
        if (reqhgt < 0) return false;
        d->long_name = radlong[v - 5]; d->units = "W/m^2"; *scale = 1;
        *put_by_reference = false;   // `if ("raddir" %in% vars)` never holds for the documented names (dataprep.R:1163-1167)
        return true;
    }
    switch (v) {
    case 0:
        d->long_name = reqhgt > 0 ? "Air temperature at height " + h + " m"
                     : reqhgt == 0 ? std::string("Soil surface temperature") : "Soil temperature at depth " + h + " m";
        d->units = "deg C x 100"; *scale = 100; return true;
    case 1:
        if (!(reqhgt > 0)) return false;
        d->long_name = "Leaf temperature at height " + h + " m"; d->units = "deg C x 100"; *scale = 100; return true;
    case 2:
        if (!(reqhgt > 0)) return false;
        d->long_name = "Relative humidity at height " + h + " m"; d->units = "Percentage"; *scale = 1; return true;
    case 3:
        d->long_name = "Soil surface moisture";
        d->units = reqhgt < 0 ? "Percentage volume" : "Volume percentage soil moisture in top 10 cm of soil";
        *scale = 100;
        *put_by_reference = false;   // `ncvar_put(nccew, …)`: an undefined object, the put is an R error (dataprep.R:1161)
        return true;
    default:
        if (!(reqhgt > 0)) return false;
        d->long_name = "Wind speed at height " + h + " m"; d->units = "m/s x 100"; *scale = 100; return true;
    }
}

inline int32_t nc_pack(double x, double scale) {
    const double q = rint(x * scale);
    return (q > -2147483648.0 && q < 2147483648.0) ? (int32_t)q : mcf::NcFile::kMissval;
}

// the container of a judged handle: created, or the handle deleted with the reason set
int nc_open(const char* who, mcf_ncfile* nc, const char* path, int32_t format, int32_t deflate_level, int64_t rows, int64_t cols,
            int64_t nsteps, const double* east, const double* north, const double* time_hours, const char* crs_wkt,
            const std::vector<mcf::NcVarDef>& defs, mcf_ncfile** out) {
    std::string e;
    if (format == MCF_NC_NETCDF4) {
        // the reference's container (dataprep.R:1110: compression = 9); deflate_level 0 = the reference's 9, -1 = none
        const int level = deflate_level == 0 ? 9 : deflate_level < 0 ? 0 : deflate_level;
        mcf::Nc4File* f4 = new mcf::Nc4File();
        nc->f.reset(f4);
        if (nsteps == 0) e = "a netCDF-4 file needs at least one time step";
        else if (level > 9) e = "deflate_level above 9";
        else e = f4->create4(path, rows, cols, nsteps, east, north, time_hours, crs_wkt, defs, level);
    } else if (format == MCF_NC_CLASSIC) {
        nc->f.reset(new mcf::NcFile());
        e = nc->f->create(path, rows, cols, nsteps, east, north, time_hours, crs_wkt, defs);
    } else {
        e = "unknown format";
    }
    if (!e.empty()) { delete nc; return fail(MCF_ERR_ARG, std::string(who) + ": " + e); }
    *out = nc;
    return MCF_OK;
}

}  // namespace

extern "C" {

int mcf_abi_version(void) { return MCF_ABI_VERSION; }
const char* mcf_last_error(void) { return g_err.c_str(); }
int mcf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void mcf_plan_destroy(mcf_plan* p) {
    if (!p) return;
    mcf::print_variant_stats();
    hipSetDevice(p->device);
    if (p->stream) hipStreamSynchronize(p->stream);
    if (p->prep) { hipStreamSynchronize(p->prep); hipStreamDestroy(p->prep); }
    if (p->ev_prep) hipEventDestroy(p->ev_prep);
    if (p->ev_cells_done) hipEventDestroy(p->ev_cells_done);
    for (auto& e : p->kev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    p->dev.release_all();
    if (p->ev0) hipEventDestroy(p->ev0);
    if (p->ev1) hipEventDestroy(p->ev1);
    if (p->stream) hipStreamDestroy(p->stream);
    delete p;
}

static int plan_create(const mcf_grid_inputs* in, const mcf_options* opt, int32_t ring_days, int32_t ring_slots, bool streamed,
                       mcf_plan** out, const mcf_dtm_spec* dtm = nullptr, bool foliage_later = false) {
    if (!out) return fail(MCF_ERR_ARG, "null plan pointer");
    *out = nullptr;
    int rc;
    if ((rc = check_inputs(in, opt))) return rc;
    if (dtm && (rc = check_dtm(in, dtm))) return rc;
    if ((rc = ensure_device(opt->device))) return rc;
    PlanHolder holder(new mcf_plan());
    mcf_plan* p = holder.get();
    p->device = opt->device;
    HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&p->ev0));
    HIP_TRY(hipEventCreate(&p->ev1));
    SetupScratch s;      // (after the holder: on a refusal it goes first, as the set-up temporaries always have)
    if ((rc = plan_shape(p, in, opt, ring_days, ring_slots, streamed))) return rc;      // (with coarse_check)
    if ((rc = upload_static(p, in, dtm, foliage_later))) return rc;
    if ((rc = coarse_planes(p, in, s))) return rc;
    if ((rc = solver_constants(p, in, opt))) return rc;
    if ((rc = cell_images(p, in))) return rc;
    if ((rc = time_inputs(p, in, s))) return rc;      // (with coarse_wind)
    if ((rc = !p->af ? time_tables_vector(p, in, s) : p->coarse ? time_tables_coarse(p, in, s) : time_tables_fine(p, in, s))) return rc;
    if ((rc = output_ring(p, opt))) return rc;
    if ((rc = below_stream_state(p, in, opt))) return rc;
    if ((rc = below_series_state(p, in, opt))) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));      // every queued copy has read its source: s and the caller's arrays are free
    *out = holder.release();
    return MCF_OK;
}

int mcf_plan_create(const mcf_grid_inputs* in, const mcf_options* opt, int32_t ring_days, int32_t ring_slots,
                    mcf_plan** out) {
    return plan_create(in, opt, ring_days, ring_slots, false, out);
}
int mcf_plan_create_streamed(const mcf_grid_inputs* in, const mcf_options* opt, int32_t ring_days, int32_t ring_slots,
                             mcf_plan** out) {
    return plan_create(in, opt, ring_days, ring_slots, true, out);
}
int mcf_plan_create_dtm(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_dtm_spec* dtm, int32_t ring_days,
                        int32_t ring_slots, mcf_plan** out) {
    if (!dtm) return fail(MCF_ERR_ARG, "null mcf_dtm_spec");
    return plan_create(in, opt, ring_days, ring_slots, false, out, dtm);
}

}  // extern "C"
namespace mcf {
int plan_ring_views(mcf_plan* p, int slot, RingView views[10], int32_t has[10], hipStream_t* stream, int64_t* N, int* device,
                    int* slot_days) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    if (slot < 0 || slot >= p->ring_slots) return fail(MCF_ERR_ARG, "slot out of range");
    for (int v = 0; v < MCF_NOUT; ++v) {
        has[v] = p->var_slot[v] >= 0;
        if (has[v]) views[v] = ring_view(p, slot, v);
    }
    *stream = p->stream; *N = p->N; *device = p->device; *slot_days = p->ring_days;
    return MCF_OK;
}
}  // namespace mcf
extern "C" {

int mcf_plan_set_mxtc(mcf_plan* p, double mxtc) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    if (p->af) return fail(MCF_ERR_STATE, "array forcing takes the maximum per cell from its series");
    p->g.dTmx = -0.6273 * mxtc + 49.79;                              // cpp:1236 (every launch takes the plan's globals)
    return MCF_OK;
}

// array forcing: the per-cell maximum air temperature (src/microclimfCpp.cpp:2467-2471) over the days with dayflag != 0 only — what
// runmicro2Cpp computes when `.runmicronosnow` hands it the no-snow-day SUBSET (R/internal.R:3689); streamed through the plan's
// forcing stage, a run of consecutive flagged days at a time
int mcf_plan_set_mxtc_days(mcf_plan* p, const mcf_grid_inputs* in, const int32_t* dayflag, int32_t ndays) {
    if (!p || !dayflag || (!in && !p->coarse)) return fail(MCF_ERR_ARG, "null argument");
    if (!p->af) return fail(MCF_ERR_STATE, "mcf_plan_set_mxtc_days: a plan with array forcing");
    if (ndays < 0 || ndays > p->ndays) return fail(MCF_ERR_ARG, "day range out of bounds");
    if (p->coarse) {
        // coarse forcing: the flagged days of the resident series, folded by the day-flagged form of the create-time kernel
        HIP_TRY(hipSetDevice(p->device));
        if (ndays == 0) { mcf::launch_fill(p->d_mxtc, p->N, -273.15, p->stream); return MCF_OK; }
        int32_t* d_flag = nullptr;
        if (const int rc = p->dev.make(&d_flag, ndays)) return rc;
        struct Release { mcf_plan* p; int32_t* buf; ~Release() { p->dev.release(buf); } } release{p, d_flag};      // on every exit path
        HIP_TRY(hipMemcpyAsync(d_flag, dayflag, (size_t)ndays * 4, hipMemcpyHostToDevice, p->stream));
        const int64_t slab = (int64_t)p->crows * p->ccols * std::max<int64_t>(p->tsteps, 1);
        mcf::launch_mxtc_coarse_days(p->d_force, slab, p->crows, p->ccols, d_flag, ndays, p->d_crowpos, p->d_ccolpos,
                                     p->rows, p->N, p->altcorrect, p->d_elevd, p->d_pkfac, p->d_mxtc, p->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(p->stream));      // (the caller's flags have been read, the kernel has read its copy)
        return MCF_OK;
    }
    if (!in->clim.tc) return fail(MCF_ERR_ARG, "missing forcing array: tc");
    HIP_TRY(hipSetDevice(p->device));
    mcf::launch_fill(p->d_mxtc, p->N, -273.15, p->stream);
    for (int d = 0; d < ndays;) {
        if (!dayflag[d]) { ++d; continue; }
        int e = d;
        while (e < ndays && dayflag[e] && e - d < p->ring_days) ++e;
        HIP_TRY(copy_in(p, p->d_force_stage, in->clim.tc + p->pitch * p->cols * (int64_t)d * 24, p->cols * (int64_t)(e - d) * 24));
        mcf::launch_mxtc((const double*)p->d_force_stage, p->N, (e - d) * 24, p->d_mxtc, p->stream);
        HIP_TRY(hipGetLastError());
        d = e;
    }
    return MCF_OK;
}

// layered vegetation: the day -> layer map replaced (mcf_snowrun_set_day_layers: a snow run's solver sees the no-snow days only, and
// a caller that mirrors how `.runmodel3Cpp` deals a day SUBSET to layers knows the subset after pass 1)
int mcf_plan_set_day_layers(mcf_plan* p, const int32_t* layer_of_day, int32_t ndays) {
    if (!p) return fail(MCF_ERR_ARG, "null argument");
    if (p->layers <= 1 || !p->d_daylayer) return fail(MCF_ERR_STATE, "mcf_plan_set_day_layers: the plan's vegetation has one layer");
    if (ndays != p->ndays) return fail(MCF_ERR_ARG, "mcf_plan_set_day_layers: one entry per day of the plan");
    if (!layer_of_day) layer_of_day = p->daylayer0.data();      // null: the table made from lyr_st / lyr_ed again
    for (int d = 0; d < ndays; ++d)
        if (layer_of_day[d] < -1 || layer_of_day[d] >= p->layers)
            return fail(MCF_ERR_ARG, "mcf_plan_set_day_layers: layer_of_day[" + std::to_string(d) + "] is no layer of the plan (-1: none)");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(p->d_daylayer, layer_of_day, (size_t)ndays * 4, hipMemcpyHostToDevice));
    return MCF_OK;
}

// array forcing: the per-cell maximum air temperature the plan holds now, [rows, cols] (diagnostics; tests compare the day-flagged
// form with a plan created on the subset series)
int mcf_plan_fetch_mxtc(mcf_plan* p, double* host_dst) {
    if (!p || !host_dst) return fail(MCF_ERR_ARG, "null argument");
    if (!p->af || !p->d_mxtc) return fail(MCF_ERR_STATE, "mcf_plan_fetch_mxtc: a plan with array forcing");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(host_dst, p->d_mxtc, (size_t)p->N * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}

int mcf_plan_twi_partial(mcf_plan* p, double* sum, int64_t* count) {
    if (!p || !sum || !count) return fail(MCF_ERR_ARG, "null argument");
    *sum = p->twi_sum;
    *count = p->twi_count;
    return MCF_OK;
}

int mcf_plan_set_twi_mean(mcf_plan* p, double mean) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    p->twi_mean = mean;
    p->cells_ready = false;
    return MCF_OK;
}

// ---- height profiles from one plan (include/mcf.h mcf_plan_set_height) ----------------------------------------
// what every entry that takes a height above ground refuses, before any device is touched
static int check_height_above(const char* who, double h) {
    if (h > 0.0) return MCF_OK;
    const std::string w = std::string(who) + ": ";
    if (h == 0.0) return fail(MCF_ERR_ARG, w + "a height must be > 0 (the ground surface, reqhgt = 0: mcf_runmicro1 .. mcf_runmicro4)");
    if (h < 0.0) return fail(MCF_ERR_ARG, w + "a height must be > 0 (below ground: mcf_runmicro_depths)");
    return fail(MCF_ERR_ARG, w + "a height must be > 0, got NaN");
}

int mcf_plan_set_height(mcf_plan* p, double reqhgt, const double* paia) {
    if (!p) return fail(MCF_ERR_ARG, "mcf_plan_set_height: null plan");
    if (const int rc = check_height_above("mcf_plan_set_height", reqhgt)) return rc;
    if (p->bg || !p->tiled || p->opt.reqhgt < 0.0)
        return fail(MCF_ERR_STATE, "mcf_plan_set_height: a below-ground plan (reqhgt < 0 at creation) cannot be moved above ground");
    if (p->d_dring) return fail(MCF_ERR_STATE, "mcf_plan_set_height: the plan has diagnostics enabled");
    HIP_TRY(hipSetDevice(p->device));
    // every launch that reads the planes, the images or the tile lists of the height before has finished
    if (p->cells_inflight) { HIP_TRY(hipEventSynchronize(p->ev_cells_done)); p->cells_inflight = false; }
    HIP_TRY(hipStreamSynchronize(p->stream));
    const int64_t n = p->N * p->layers;
    mcf::launch_foliage(p->d_veg[0], p->d_veg[1], reqhgt, n, const_cast<double*>(p->d_veg[9]), const_cast<double*>(p->d_veg[8]), p->stream);
    HIP_TRY(hipGetLastError());
    if (paia) {      // (stream order: behind the kernel's store; read with the plan's row pitch, as vegp$paia is)
        HIP_TRY(copy_in(p, const_cast<double*>(p->d_veg[8]), paia, p->cols * p->layers));
        HIP_TRY(hipStreamSynchronize(p->stream));      // the caller's array has been read
    }
    p->opt.reqhgt = reqhgt;
    p->g.reqhgt = reqhgt;
    p->g.reqhgt2 = reqhgt < 0.00001 ? 0.00001 : reqhgt;      // cpp:2246-2247, as solver_constants
    p->cells_ready = false;                                  // ensure_cells: the per-layer images and the fast / slow tile lists
    return MCF_OK;
}

int mcf_plan_fetch_foliage(mcf_plan* p, double* paia, double* leafden) {
    if (!p) return fail(MCF_ERR_ARG, "mcf_plan_fetch_foliage: null plan");
    if (!p->d_veg[8] || !p->d_veg[9]) return fail(MCF_ERR_STATE, "mcf_plan_fetch_foliage: the plan holds no vegetation planes");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    const size_t bytes = (size_t)(p->N * p->layers) * 8;
    if (paia) HIP_TRY(hipMemcpy(paia, p->d_veg[8], bytes, hipMemcpyDeviceToHost));
    if (leafden) HIP_TRY(hipMemcpy(leafden, p->d_veg[9], bytes, hipMemcpyDeviceToHost));
    return MCF_OK;
}

int mcf_plan_upload_forcing_days(mcf_plan* p, const mcf_grid_inputs* in, int32_t day0, int32_t ndays, int32_t slot) {
    if (!p || !in) return fail(MCF_ERR_ARG, "null argument");
    if (!p->af) return fail(MCF_ERR_STATE, "plan uses vector forcing");
    if (p->coarse) return MCF_OK;            // the coarse series is resident since mcf_plan_create
    if (slot < 0 || slot >= p->ring_slots) return fail(MCF_ERR_ARG, "slot out of range");
    if (day0 < 0 || ndays < 1 || ndays > p->ring_days || day0 + ndays > p->ndays)
        return fail(MCF_ERR_ARG, "day range out of bounds");
    HIP_TRY(hipSetDevice(p->device));
    const double* raw[15];
    clim_ptrs(in, raw);
    const int64_t N = p->N;
    for (int f = 0; f < 15; ++f)
        if (!raw[f]) return fail(MCF_ERR_ARG, std::string("missing forcing array: ") + kRawNames[f]);
    for (int f = 0; f < 15; ++f) {
        // the series as the caller holds it ([rows, cols, steps]) into the staging slab, then into its tiled place on the device
        // (stream order: the next copy into the slab waits for this series' kernel)
        const double* src = raw[f] + p->pitch * p->cols * (int64_t)day0 * 24;
        HIP_TRY(copy_in(p, p->d_force_stage, src, p->cols * (int64_t)ndays * 24));
        mcf::RingView v{};
        v.base = p->d_force + (int64_t)slot * p->force_slot_elems + (int64_t)f * mcf::ring_block_doubles(p->cpb);
        v.N = N; v.tile_stride = p->force_tile_stride; v.day_stride = p->force_day_stride; v.cpb = p->cpb;
        mcf::launch_tile_series(p->d_force_stage, (int64_t)ndays * 24, v, p->stream);
        HIP_TRY(hipGetLastError());
    }
    if (p->d_Tgp_slots) {
        // streamed below ground, complete = 0: the point model's Tg / Tbp of these days, [step][N] as the caller holds them
        if (!in->pointm.Tg || !in->pointm.Tbp) return fail(MCF_ERR_ARG, "missing input array: pointm$Tg / pointm$Tbp");
        const int64_t off = (int64_t)slot * p->ring_days * 24 * N, src = p->pitch * p->cols * (int64_t)day0 * 24;
        HIP_TRY(copy_in(p, p->d_Tgp_slots + off, in->pointm.Tg + src, p->cols * (int64_t)ndays * 24));
        HIP_TRY(copy_in(p, p->d_Tbp_slots + off, in->pointm.Tbp + src, p->cols * (int64_t)ndays * 24));
    }
    p->force_day0[slot] = day0;
    p->force_ndays[slot] = ndays;
    return MCF_OK;
}

int mcf_plan_run_days(mcf_plan* p, int32_t day0, int32_t ndays, int32_t slot) {
    return mcf_plan_run_days_at(p, day0, ndays, slot, 0);
}

int mcf_plan_run_days_at(mcf_plan* p, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0) {
    return mcf_plan_run_days_masked(p, day0, ndays, slot, slot_day0, nullptr, 0);
}

namespace {
// the launch description of days [day0, day0 + ndays) into `slot` from its day `slot_day0` on — everything but the tile list —,
// and which instantiation the days allow: `fast` (the min / max clamps: every day regular), `soil_daily` (the per cell-day soil
// state shared through LDS)
int check_days(const mcf_plan* p, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0) {
    if (slot < 0 || slot >= p->ring_slots) return fail(MCF_ERR_ARG, "slot out of range");
    if (day0 < 0 || ndays < 1 || day0 + ndays > p->ndays) return fail(MCF_ERR_ARG, "day range out of bounds");
    if ((!p->bg || p->bg_stream) && (slot_day0 < 0 || slot_day0 + ndays > p->ring_days))
        return fail(MCF_ERR_ARG, "more days than the ring slot holds");
    if (slot_day0 != 0 && p->bg && !p->bg_stream) return fail(MCF_ERR_ARG, "a day offset inside the slot needs reqhgt >= 0");
    return MCF_OK;
}
int solve_args(mcf_plan* p, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0, mcf::SolveArgs& a, bool& fast, bool& soil_daily) {
    int rc = check_days(p, day0, ndays, slot, slot_day0);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if ((rc = ensure_cells(p))) return rc;
    a = mcf::SolveArgs{};
    a.N = p->N;
    a.cellc = p->d_cellc; a.ntiles_total = p->ntiles; a.tt = p->d_tt;
    a.daylayer = p->d_daylayer;
    const int64_t cap = p->N * (int64_t)p->ring_days * 24;
    if (p->af && p->coarse) {
        a.af_base = p->d_force;
        a.af_stride = (int64_t)p->crows * p->ccols * std::max<int64_t>(p->tsteps, 1);
        a.crows = p->crows; a.ccols = p->ccols;
        a.altcorrect = p->altcorrect;
        a.dt = p->d_dt; a.windex = p->d_windex; a.mxtc = p->d_mxtc;
    } else if (p->af) {
        // (the days may be a run INSIDE what the slot's forcing holds — the snow run solves a chunk's no-snow days at their own
        // place: the kernel counts forcing days from its first day, so the base is moved to that day's block)
        if (p->force_day0[slot] > day0 || p->force_day0[slot] + p->force_ndays[slot] < day0 + ndays)
            return fail(MCF_ERR_STATE, "forcing for these days has not been uploaded to this slot");
        a.af_base = p->d_force + (int64_t)slot * p->force_slot_elems + (int64_t)(day0 - p->force_day0[slot]) * p->force_day_stride;
        a.af_tile_stride = p->force_tile_stride; a.af_day_stride = p->force_day_stride;
        a.dt = p->d_dt; a.windex = p->d_windex; a.mxtc = p->d_mxtc;
    }
    a.out_base = p->d_ring + (int64_t)slot * p->slot_elems;
    a.out_stride = cap;
    a.out_tile_stride = p->ring_tile_stride; a.out_day_stride = p->ring_day_stride; a.out_var_stride = p->ring_var_stride;
    a.slot_day0 = slot_day0;
    a.out_sel = 0;
    for (int v = 0; v < MCF_NOUT; ++v)
        a.out_sel |= (uint64_t)(p->var_slot[v] < 0 ? 15 : p->var_slot[v]) << (4 * v);
    a.slot_step0 = p->bg ? (int64_t)day0 * 24 : 0;
    a.tgser = p->d_tgser; a.ddsum = p->d_ddsum;
    if (p->bg_stream) {
        // Tg into the chunk's Tg ring, Tz itself is made from it by k_below_chunk; the damping-depth sum only in sweep 1
        a.out_sel |= (uint64_t)15 << (4 * MCF_OUT_TZ);
        a.tg_ring = p->d_tgring; a.tg_tile_stride = p->tg_tile_stride;
        a.ddsum = nullptr;
    }
    a.day0 = day0; a.ndays = ndays; a.total_days = p->ndays;
    {
        // pass 2 yields Tz (+ tleaf, relhum for reqhgt > 0) and the long-wave fluxes; requests for
        // soilm / windspeed / short-wave fluxes alone are served by pass 1
        const bool o0 = p->var_slot[MCF_OUT_TZ] >= 0, o1 = p->var_slot[MCF_OUT_TLEAF] >= 0,
                   o2 = p->var_slot[MCF_OUT_RELHUM] >= 0, o7 = p->var_slot[MCF_OUT_RLWDOWN] >= 0,
                   o9 = p->var_slot[MCF_OUT_RLWUP] >= 0;
        const double rq = p->opt.reqhgt;
        a.need_tv = (rq > 0.0 && (o0 || o1 || o2 || o7 || o9)) || (rq == 0.0 && (o7 || o9));
        a.need_pass2 = p->bg ? (o0 ? 1 : 0) : (a.need_tv || (rq == 0.0 && o0));
    }
    a.g = p->g;
    a.fix_count = p->d_fix_count; a.fix_list = p->d_fix_list; a.fix_cap = p->fix_cap;
    if (p->d_dring) {
        // (the diagnostics ring itself: dispatch_solve)  T0, G and kDDg are pass 2's first values (the requested outputs are written as without them: a variable that is not
        // requested is not stored, and what pass 2 stores for a requested one is what the NA branch stores when it is all NA)
        if (p->dg_slab1[MCF_DIAG_T0] || p->dg_slab1[MCF_DIAG_G] || p->dg_slab1[MCF_DIAG_KDDG]) a.need_pass2 = 1;
    }
    p->has_run = true;
    fast = p->fast_enabled && p->n_fast > 0;
    for (int d = day0; fast && !p->af && d < day0 + ndays; ++d)     // array forcing: every lane checks its own forcing values
        if (p->day_irregular[(size_t)d]) fast = false;
    soil_daily = !p->af && !p->day_soil_daily.empty();
    for (int d = day0; soil_daily && d < day0 + ndays; ++d)
        if (!p->day_soil_daily[(size_t)d]) soil_daily = false;
    if (p->coarse) soil_daily = p->coarse_lds;      // (coarse array forcing: the same launch flag selects the LDS-staged taps)
    return MCF_OK;
}

// The tiles of a launch by class.  A null list with a count: tiles 0 .. n - 1; no list and no count at all: every tile of the
// raster.
struct SolveTiles {
    const int32_t* fast_list = nullptr;
    int64_t n_fast = 0;
    const int32_t* slow_list = nullptr;
    int64_t n_slow = 0;
    bool whole_raster() const { return !fast_list && !slow_list && n_fast == 0 && n_slow == 0; }
};

// The k_solve launches of `t` on the plan's stream: with `fast`, the fix-up count cleared, then the fast part through the
// min / max clamps and the slow part through the reference form; without it (an irregular day, or no fast class at all) one
// reference-form launch of the first part, or of the whole raster.  An empty part launches nothing.
// A diagnostics plan (mcf_plan_diag_enable, mcf_plan_diag_enable_array) sends the same launches, with the same choices, through
// k_solve_diag / k_solve_diag_af: the slot's place in the diagnostics ring rides along.
void dispatch_solve(mcf_plan* p, mcf::SolveArgs& a, bool fast, bool soil_daily, const SolveTiles& t, int slot) {
    auto launch = [&](bool bg, bool f) {
        if (!p->d_dring) { mcf::launch_solve(a, p->cpb, p->af, bg, f, soil_daily, p->stream); return; }
        mcf::DiagSolveArgs d{};
        static_cast<mcf::SolveArgs&>(d) = a;
        d.dg_base = p->d_dring + (int64_t)slot * p->dg_slot_elems;
        d.dg_tile_stride = p->dg_tile_stride; d.dg_day_stride = p->dg_day_stride;
        for (int v = 0; v < MCF_NDIAG; ++v) d.dg_sel |= (uint64_t)(p->dg_slab1[v] ? p->dg_slab1[v] - 1 : 15) << (4 * v);
        if (p->af) mcf::launch_solve_diag_af(d, p->cpb, f, soil_daily, p->stream);      // (coarse: the flag says "taps through LDS")
        else mcf::launch_solve_diag(d, p->cpb, f, soil_daily, p->stream);
    };
    if (!fast) {
        if (!t.whole_raster() && t.n_fast == 0) return;
        a.tile_list = t.fast_list; a.ntiles_launch = t.n_fast;
        launch(p->bg, false);
        ++p->slow_launches;
        return;
    }
    (void)hipMemsetAsync(p->d_fix_count, 0, 4, p->stream);
    if (t.n_fast > 0) {
        a.tile_list = t.fast_list; a.ntiles_launch = t.n_fast;
        launch(false, true);
        ++p->fast_launches;
    }
    if (t.n_slow > 0) {
        a.tile_list = t.slow_list; a.ntiles_launch = t.n_slow;
        launch(false, false);
        ++p->slow_launches;
    }
}

// ---- below ground streamed through day chunks (DESIGN.md "Below ground in day chunks") ----------------------------------
static_assert(mcf::kBelowMaxDepths == MCF_MAX_DEPTHS, "mcf_kernels.h and mcf.h agree on the depth count");
// Tz at depth `depth` of ring slot `slot`: depth 0 is the slot's own variable, the others have a slab beside the ring
mcf::RingView depth_view(const mcf_plan* p, int slot, int depth) {
    if (depth == 0) return ring_view(p, slot, MCF_OUT_TZ);
    mcf::RingView v{};
    v.N = p->N; v.cpb = p->cpb;
    v.tile_stride = p->tg_tile_stride; v.day_stride = mcf::ring_block_doubles(p->cpb);
    v.base = p->d_tzx + ((int64_t)(depth - 1) * p->ring_slots + slot) * p->ntiles * p->tg_tile_stride;
    return v;
}
// What a sink folds out of ring slot `slot`, launch by launch: `nsel` variables, the i-th in slab slab[i] (var_stride apart) of
// `view` and requested as var[i]; its results start at `place` of the sink's state.
struct SinkSource {
    mcf::RingView view;
    int64_t var_stride;
    int nsel, place;
    int slab[MCF_NOUT], var[MCF_NOUT];
};
// f(source) for the slot itself with the selected variables' slabs, then for Tz at depths 1 .. D - 1 of a below-ground sink, each
// one variable of its own slab beside the ring
extern "C++" template <class F>
void for_sink_sources(const mcf_plan* p, const SinkPlaces& places, int slot, F&& f) {
    SinkSource s{};
    s.view.N = p->N; s.view.cpb = p->cpb;
    s.view.base = p->d_ring + (int64_t)slot * p->slot_elems;
    s.view.tile_stride = p->ring_tile_stride; s.view.day_stride = p->ring_day_stride;
    s.var_stride = p->ring_var_stride;
    s.nsel = places.nmain;
    for (int v = 0; v < MCF_NOUT; ++v)
        if (places.sel1[v]) { s.slab[places.sel1[v] - 1] = p->var_slot[v]; s.var[places.sel1[v] - 1] = v; }
    f(s);
    for (int d = 1; d <= places.nsel - places.nmain; ++d) {
        s.view = depth_view(p, slot, d);
        s.var_stride = 0; s.nsel = 1; s.place = places.nmain + d - 1;
        s.slab[0] = 0; s.var[0] = MCF_OUT_TZ;
        f(s);
    }
}
// the state of a streamed plan as k_below_* see it; the chunk fields are the caller's
mcf::BelowStreamArgs below_args(mcf_plan* p, int slot) {
    mcf::BelowStreamArgs b{};
    b.N = p->N; b.tsteps = (int)p->tsteps; b.ndays = p->ndays;
    if (!p->below_days.empty()) {       // a day subset: the series is its days joined, whole days only
        b.ndays = (int)p->below_days.size(); b.tsteps = 24 * b.ndays;
        b.days = p->d_below_days;
    }
    b.complete = p->opt.complete; b.hiy = p->hiy;
    b.reqhgt = p->opt.reqhgt; b.mat = p->opt.mat;
    b.hgt = p->d_veg[0];
    b.tg.base = p->d_tgring; b.tg.N = p->N; b.tg.cpb = p->cpb;
    b.tg.tile_stride = p->tg_tile_stride; b.tg.day_stride = mcf::ring_block_doubles(p->cpb);
    if (p->var_slot[MCF_OUT_TZ] >= 0) b.tz = ring_view(p, slot, MCF_OUT_TZ);
    b.ddsum = p->d_ddsum; b.hsum = p->d_hsum; b.dmean = p->d_dmean; b.ybuf = p->d_ybuf; b.wrap = p->d_wrap; b.prev = p->d_prev;
    b.Tgp = p->d_Tgp; b.Tbp = p->d_Tbp;
    b.per_cell_pointm = p->af ? 1 : 0;
    b.ndepths = std::max<int>(1, (int)p->depths.size());
    b.depth[0] = p->opt.reqhgt;
    for (size_t d = 0; d < p->depths.size(); ++d) b.depth[d] = p->depths[d];
    b.reqhgt = b.depth[0];
    if (p->d_tzx) {
        b.tzx = depth_view(p, slot, 1);
        b.tzx_stride = (int64_t)p->ring_slots * p->ntiles * p->tg_tile_stride;
    }
    b.ybufx = p->d_ybufx;
    if (p->d_Tbp_depths) { b.Tbp = p->d_Tbp_depths; b.tbp_stride = p->tsteps; }
    return b;
}

// the part of a streamed below-ground plan's series that calendar days [day0, day0 + ndays) hold: positions [pos0, pos0 + npos)
// of the series Tbelowgroundv sees, and their calendar days as runs (first day, days) of consecutive days.  Without a day
// subset that is the range itself.
struct BelowRange {
    int pos0 = 0, npos = 0;
    std::vector<std::pair<int, int>> runs;
};
void below_range(const mcf_plan* p, int32_t day0, int32_t ndays, BelowRange& r) {
    r = BelowRange{};
    if (p->below_days.empty()) {
        r.pos0 = day0; r.npos = ndays;
        r.runs.emplace_back(day0, ndays);
        return;
    }
    mcf_below_days_range(p->below_days.data(), (int32_t)p->below_days.size(), p->ndays, day0, ndays, &r.pos0, &r.npos);
    for (int q = r.pos0; q < r.pos0 + r.npos; ++q) {
        const int d = p->below_days[(size_t)q];
        if (!r.runs.empty() && r.runs.back().first + r.runs.back().second == d) ++r.runs.back().second;
        else r.runs.emplace_back(d, 1);
    }
}

// the solver's launches for the runs of `r`, each at its days' own place (day - day0) of `slot` and of the Tg ring
int below_solve_args(mcf_plan* p, const BelowRange& r, int32_t day0, int32_t slot, std::vector<mcf::SolveArgs>& as) {
    for (const auto& run : r.runs) {
        mcf::SolveArgs a{};
        bool fast = false, soil_daily = false;
        int rc = solve_args(p, run.first, run.second, slot, run.first - day0, a, fast, soil_daily);
        if (rc) return rc;
        if (a.tg_ring) a.tg_ring += (int64_t)(run.first - day0) * mcf::ring_block_doubles(p->cpb);
        as.push_back(a);
    }
    return MCF_OK;
}

// days [day0, day0 + ndays) of a streamed below-ground plan into `slot`: the solver (Tg into the Tg ring, the other outputs into
// the slot), then Tz made from Tg and the per-cell state.  Chunks run in day order from day 0; the chunk that ends on the last
// whole day also writes the tsteps % 24 steps behind it (the slot needs a day more for them).  With a day subset
// (mcf_plan_below_set_days) the subset's days inside the range are run, each at its own place day - day0 of the slot, in
// subset order from the subset's first day; a range that holds none of them does nothing.
int run_below_chunk(mcf_plan* p, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0) {
    const bool tz = p->var_slot[MCF_OUT_TZ] >= 0;
    if (slot_day0 != 0) return fail(MCF_ERR_ARG, "a day offset inside the slot needs reqhgt >= 0");
    if (tz && !p->below_ready)
        return fail(MCF_ERR_STATE, "streamed below-ground plan: call mcf_plan_below_prepare before running days");
    // (the whole range, once, before the day-order check: solve_args sees the range's runs of days only, and none of them when
    // the range holds no day of a subset)
    int rc = check_days(p, day0, ndays, slot, 0);
    if (rc) return rc;
    const bool sub = !p->below_days.empty();
    BelowRange r;
    below_range(p, day0, ndays, r);
    if (tz && r.pos0 != 0 && r.pos0 != p->below_next && r.npos > 0)
        return fail(MCF_ERR_STATE, std::string("streamed below-ground plan: chunks run in day order from day 0 without gaps (expected ") +
                                   (sub ? "subset position " : "day ") + std::to_string(p->below_next) + " or 0, got " +
                                   std::to_string(r.pos0) + ")");
    if (r.npos == 0) return MCF_OK;
    std::vector<mcf::SolveArgs> as;
    if ((rc = below_solve_args(p, r, day0, slot, as))) return rc;
    const bool tail = !sub && day0 + ndays == p->ndays && p->tsteps > (int64_t)p->ndays * 24;
    if (tz && tail && ndays + 1 > p->ring_days)
        return fail(MCF_ERR_ARG, "streamed below-ground plan: the chunk that ends on the last whole day needs one day more in its "
                                 "slot, for the steps behind that day");
    rc = timed(p, [&] {
        for (const mcf::SolveArgs& a : as) {
            mcf::launch_solve_bg_tiled(a, p->cpb, p->af, p->stream);
            ++p->slow_launches;
        }
        if (!tz) return;
        mcf::BelowStreamArgs b = below_args(p, slot);
        b.day0 = r.pos0; b.ndays_chunk = r.npos; b.cal0 = day0; b.tail = tail ? 1 : 0;
        if (p->d_Tgp_slots) {      // the slot's point-model series start at the slot's first uploaded day
            const int64_t off = ((int64_t)slot * p->ring_days * 24 + (int64_t)(day0 - p->force_day0[slot]) * 24) * p->N;
            b.Tgp = p->d_Tgp_slots + off; b.Tbp = p->d_Tbp_slots + off;
        }
        mcf::launch_below_chunk(b, p->stream);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    p->below_next = r.pos0 + r.npos;
    return MCF_OK;
}
}  // namespace

int mcf_below_days_range(const int32_t* days, int32_t n, int32_t total_days, int32_t day0, int32_t ndays, int32_t* pos0,
                         int32_t* npos) {
    if (n < 1) return fail(MCF_ERR_ARG, "day subset: no days");
    if (!days || !pos0 || !npos) return fail(MCF_ERR_ARG, "null argument");
    for (int32_t q = 0; q < n; ++q) {
        if (days[q] < 0 || days[q] >= total_days)
            return fail(MCF_ERR_ARG, "day subset: day " + std::to_string(days[q]) + " is out of range (the series has " +
                                     std::to_string(total_days) + " whole days)");
        if (q > 0 && days[q] <= days[q - 1])
            return fail(MCF_ERR_ARG, "day subset: the days have to be strictly ascending (position " + std::to_string(q) + ")");
    }
    if (day0 < 0 || ndays < 0 || (int64_t)day0 + ndays > total_days) return fail(MCF_ERR_ARG, "day range out of bounds");
    const int32_t* lo = std::lower_bound(days, days + n, day0);
    const int32_t* hi = std::lower_bound(lo, days + n, day0 + ndays);
    *pos0 = (int32_t)(lo - days);
    *npos = (int32_t)(hi - lo);
    return MCF_OK;
}

int mcf_plan_below_set_days(mcf_plan* p, const int32_t* days, int32_t n) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    if (!p->bg_stream)
        return fail(MCF_ERR_STATE, "mcf_plan_below_set_days needs a streamed plan (mcf_plan_create_streamed) with reqhgt < 0");
    if (p->af) return fail(MCF_ERR_STATE, "mcf_plan_below_set_days: a day subset needs vector forcing");
    if (p->below_ready) return fail(MCF_ERR_STATE, "mcf_plan_below_set_days comes before mcf_plan_below_prepare");
    if (!p->depths.empty()) return fail(MCF_ERR_STATE, "mcf_plan_below_set_days: a day subset together with a depth list is not taken");
    int32_t pos0, npos;
    int rc = mcf_below_days_range(days, n, p->ndays, 0, 0, &pos0, &npos);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if (!p->d_below_days && (rc = p->dev.make(&p->d_below_days, (int64_t)std::max(p->ndays, 1)))) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->below_days.assign(days, days + n);
    HIP_TRY(hipMemcpy(p->d_below_days, p->below_days.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    return MCF_OK;
}

// what a depth list can be refused for without a plan or a device; `who`: the entry's name
static int check_depths(const char* who, const double* depths, int32_t ndepths, const double* tbp, bool complete, bool af) {
    const std::string w = std::string(who) + ": ";
    if (!depths || ndepths < 1) return fail(MCF_ERR_ARG, w + "a null or empty depth list");
    if (ndepths > MCF_MAX_DEPTHS)
        return fail(MCF_ERR_ARG, w + std::to_string(ndepths) + " depths, at most MCF_MAX_DEPTHS = " + std::to_string(MCF_MAX_DEPTHS));
    for (int d = 0; d < ndepths; ++d)
        if (!(depths[d] < 0.0))
            return fail(MCF_ERR_ARG, w + "depths[" + std::to_string(d) + "] is not below ground (every depth is < 0)");
    if (af && !complete)
        return fail(MCF_ERR_ARG, w + "array forcing with complete = 0 is not taken (per-cell Tbp for several depths)");
    if (!complete && !tbp) return fail(MCF_ERR_ARG, w + "complete = 0 needs tbp, the point model's soil temperature at each depth");
    return MCF_OK;
}

int mcf_plan_below_set_depths(mcf_plan* p, const double* depths, int32_t ndepths, const double* tbp) {
    const char* who = "mcf_plan_below_set_depths";
    const std::string w = std::string(who) + ": ";
    if (!p) return fail(MCF_ERR_ARG, w + "null plan");
    if (!p->bg_stream) return fail(MCF_ERR_STATE, w + "needs a streamed plan (mcf_plan_create_streamed) with reqhgt < 0");
    if (p->below_ready) return fail(MCF_ERR_STATE, w + "comes before mcf_plan_below_prepare");
    if (!p->below_days.empty()) return fail(MCF_ERR_STATE, w + "a depth list together with a day subset is not taken");
    if (p->var_slot[MCF_OUT_TZ] < 0) return fail(MCF_ERR_STATE, w + "the plan was created without Tz");
    if (!p->depths.empty()) return fail(MCF_ERR_STATE, w + "the plan has its depth list already");
    if (p->d_sum_state) return fail(MCF_ERR_STATE, w + "comes before mcf_plan_summary_enable_below");
    const bool complete = p->opt.complete != 0;
    int rc = check_depths(who, depths, ndepths, tbp, complete, p->af);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    const int64_t extra = ndepths - 1, nd = std::max(p->ndays, 1);
    if (extra > 0) {
        if ((rc = p->dev.make(&p->d_tzx, extra * p->ring_slots * p->ntiles * p->tg_tile_stride))) return rc;
        if (complete && (rc = p->dev.make(&p->d_ybufx, extra * nd * p->N))) return rc;
    }
    if (!complete && (rc = upload(p, tbp, (int64_t)ndepths * p->tsteps, &p->d_Tbp_depths, "tbp", false))) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->depths.assign(depths, depths + ndepths);
    return MCF_OK;
}

int mcf_plan_below_prepare(mcf_plan* p, const mcf_grid_inputs* in) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    if (!p->bg_stream)
        return fail(MCF_ERR_STATE, "mcf_plan_below_prepare needs a streamed plan (mcf_plan_create_streamed) with reqhgt < 0");
    HIP_TRY(hipSetDevice(p->device));
    p->below_ready = false;
    p->below_next = 0;
    if (p->var_slot[MCF_OUT_TZ] < 0) { p->below_ready = true; return MCF_OK; }      // cpp:2307 `&& out[0]`
    const bool upload_days = p->af && !p->coarse;
    if (upload_days && !in) return fail(MCF_ERR_ARG, "array forcing: mcf_plan_below_prepare streams the forcing and needs the inputs");
    int rc = ensure_cells(p);
    if (rc) return rc;
    const int64_t N = p->N;
    HIP_TRY(hipMemsetAsync(p->d_ddsum, 0, (size_t)N * 8, p->stream));
    const bool complete = p->opt.complete != 0;
    if (complete) {
        HIP_TRY(hipMemsetAsync(p->d_hsum, 0, (size_t)N * 8, p->stream));
        HIP_TRY(hipMemsetAsync(p->d_wrap, 0, (size_t)(N * mcf::kBelowWin) * 8, p->stream));
    }
    if (!complete && !p->af) {
        // the damping-depth pre-pass over the whole series (a day subset: its runs of days, in order) from the time table
        BelowRange whole;
        below_range(p, 0, p->ndays, whole);
        for (const auto& run : whole.runs) {
            mcf::BelowDDArgs d{};
            d.N = N; d.cellc = p->d_cellc; d.ntiles_total = p->ntiles; d.cpb = p->cpb; d.daylayer = p->d_daylayer; d.tt = p->d_tt;
            d.day0 = run.first; d.ndays = run.second; d.ddsum = p->d_ddsum;
            mcf::launch_below_dd(d, p->stream);
        }
        HIP_TRY(hipGetLastError());
    } else {
        // chunk by chunk through slot 0: the pre-pass on the uploaded forcing (complete = 0), or sweep 1 — the solver with the
        // damping-depth sum on and its Tg folded into the per-cell state (complete = 1)
        const int chunk = std::max(1, std::min(p->ring_days, std::max(p->ndays, 1)));
        for (int d0 = 0; d0 < p->ndays; d0 += chunk) {
            const int nd = std::min(chunk, p->ndays - d0);
            if (upload_days && (rc = mcf_plan_upload_forcing_days(p, in, d0, nd, 0))) return rc;
            if (!complete) {
                mcf::BelowDDArgs d{};
                d.N = N; d.cellc = p->d_cellc; d.ntiles_total = p->ntiles; d.cpb = p->cpb; d.daylayer = p->d_daylayer;
                d.af_base = p->d_force; d.af_tile_stride = p->force_tile_stride; d.af_day_stride = p->force_day_stride;
                d.day0 = d0; d.ndays = nd; d.ddsum = p->d_ddsum;
                mcf::launch_below_dd(d, p->stream);
            } else {
                BelowRange r;
                below_range(p, d0, nd, r);
                if (r.npos == 0) continue;      // none of the subset's days
                std::vector<mcf::SolveArgs> as;
                if ((rc = below_solve_args(p, r, d0, 0, as))) return rc;
                for (mcf::SolveArgs& a : as) {
                    a.out_sel = ~(uint64_t)0;       // nothing into the ring
                    a.ddsum = p->d_ddsum;
                    mcf::launch_solve_bg_tiled(a, p->cpb, p->af, p->stream);
                }
                mcf::BelowStreamArgs b = below_args(p, 0);
                b.day0 = r.pos0; b.ndays_chunk = r.npos; b.cal0 = d0;
                mcf::launch_below_acc(b, p->stream);
            }
            HIP_TRY(hipGetLastError());
        }
        if (complete) {
            mcf::BelowStreamArgs b = below_args(p, 0);
            mcf::launch_below_finish(b, p->stream);
            HIP_TRY(hipGetLastError());
        }
    }
    if (upload_days) {      // slot 0's forcing now holds the last chunk of the pass: the caller uploads again
        p->force_day0[0] = -1;
        p->force_ndays[0] = 0;
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->below_ready = true;
    return MCF_OK;
}

int mcf_plan_run_days_masked(mcf_plan* p, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0, const uint8_t* skip_tile,
                             int64_t n_skip_tile) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    if (skip_tile && (p->bg || p->af)) return fail(MCF_ERR_ARG, "a tile mask needs vector forcing and reqhgt >= 0");
    if (skip_tile && p->d_dring) return fail(MCF_ERR_ARG, "a tile mask on a diagnostics plan is not supported");
    if (skip_tile && n_skip_tile != (p->ntiles > 0 ? p->ntiles : (p->N + p->cpb - 1) / p->cpb))
        return fail(MCF_ERR_ARG, "the tile mask's length is not the plan's number of tiles");
    if (p->bg_stream) return run_below_chunk(p, day0, ndays, slot, slot_day0);
    mcf::SolveArgs a{};
    bool fast = false, soil_daily = false;
    int rc = solve_args(p, day0, ndays, slot, slot_day0, a, fast, soil_daily);
    if (rc) return rc;
    // a tile mask: the launch's tile lists are the plan's minus the masked tiles (the kernel takes any list; a tile it is not
    // given is simply not touched in the slot)
    const int32_t *sub_fast = nullptr, *sub_slow = nullptr;
    int64_t n_sub_fast = 0, n_sub_slow = 0;
    if (skip_tile) {
        const int64_t ntiles = p->ntiles;
        if (!p->d_tiles_sub && (rc = p->dev.make(&p->d_tiles_sub, ntiles))) return rc;
        // (the lists live in the plan: they go up on the plan's own stream, in order with the launches that read them, and an
        // earlier masked launch may still be reading the device copy or an earlier copy the host one)
        HIP_TRY(hipStreamSynchronize(p->stream));
        std::vector<int32_t>& l = p->h_tiles_sub;
        l.clear();
        l.reserve((size_t)ntiles);
        if (fast) {
            for (int32_t t : p->h_tiles_fast) if (!skip_tile[t]) l.push_back(t);
            n_sub_fast = (int64_t)l.size();
            for (int32_t t : p->h_tiles_slow) if (!skip_tile[t]) l.push_back(t);
            n_sub_slow = (int64_t)l.size() - n_sub_fast;
        } else {
            for (int64_t t = 0; t < ntiles; ++t) if (!skip_tile[t]) l.push_back((int32_t)t);
            n_sub_fast = (int64_t)l.size();
        }
        p->masked_tiles_skipped += ntiles - n_sub_fast - n_sub_slow;
        if (!l.empty()) HIP_TRY(hipMemcpyAsync(p->d_tiles_sub, l.data(), l.size() * 4, hipMemcpyHostToDevice, p->stream));
        sub_fast = p->d_tiles_sub; sub_slow = p->d_tiles_sub + n_sub_fast;
    }
    SolveTiles tiles;      // (an irregular day: the whole raster, or the mask's one list, in the reference form)
    if (skip_tile) tiles = SolveTiles{sub_fast, n_sub_fast, sub_slow, n_sub_slow};
    // with no irregular tile the plan's fast launch needs no list (identity)
    else if (fast) tiles = SolveTiles{p->n_slow > 0 ? p->d_tiles_fast : nullptr, p->n_fast, p->d_tiles_slow, p->n_slow};
    if ((rc = timed(p, [&] { dispatch_solve(p, a, fast, soil_daily, tiles, slot); }))) return rc;
    HIP_TRY(hipGetLastError());
    return MCF_OK;
}

int mcf_plan_run_days_cells(mcf_plan* p, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0, const uint8_t* need_cell,
                            int64_t n_cells, int64_t* n_gathered) {
    if (!p || !need_cell) return fail(MCF_ERR_ARG, "null argument");
    if (p->bg || p->af || !p->tiled) return fail(MCF_ERR_ARG, "a cell subset needs vector forcing and reqhgt >= 0");
    if (p->d_dring) return fail(MCF_ERR_ARG, "a cell subset on a diagnostics plan is not supported");
    if (n_cells != p->N) return fail(MCF_ERR_ARG, "the cell flags' length is not the plan's number of cells");
    mcf::SolveArgs a{};
    bool fast = false, soil_daily = false;
    int rc = solve_args(p, day0, ndays, slot, slot_day0, a, fast, soil_daily);
    if (rc) return rc;
    if (n_gathered) *n_gathered = 0;
    const int64_t N = p->N;
    const int cpb = p->cpb;
    const int64_t nb = (N + 255) / 256, IMG = mcf::tile_image_doubles(cpb), blk = mcf::ring_block_doubles(cpb);
    // The list of cells is made on a stream of its own: the plan's stream — the previous chunk's solver launches, the snow-day
    // microclimate over them — is not drained for it, only made to wait for the list.  An earlier call's launches and copies may
    // still read the buffers and host vectors: its last event first.
    if (!p->prep) {
        HIP_TRY(hipStreamCreateWithFlags(&p->prep, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&p->ev_prep, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&p->ev_cells_done, hipEventDisableTiming));
    }
    const bool trace = getenv("MCF_CELLS_TRACE") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    if (p->cells_inflight) { HIP_TRY(hipEventSynchronize(p->ev_cells_done)); p->cells_inflight = false; }
    const double t1 = now();
    if ((rc = p->dev.regrow(&p->d_cls, &p->cls_cap, N))) return rc;
    if ((rc = p->dev.regrow(&p->d_blockcnt, &p->blockcnt_cap, nb * 2))) return rc;
    // 1. the wanted cells by class, counted per 256 cells; the list offsets are the host's prefix sums of those counts
    mcf::launch_cells_class(need_cell, p->fast_enabled ? p->d_tile_regular : nullptr, N, cpb, p->d_cls, p->d_blockcnt, p->prep);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t>& cnt = p->h_blockcnt;
    cnt.resize((size_t)nb * 2);
    HIP_TRY(hipMemcpyAsync(cnt.data(), p->d_blockcnt, (size_t)nb * 8, hipMemcpyDeviceToHost, p->prep));
    HIP_TRY(hipStreamSynchronize(p->prep));
    const double t2 = now();
    int64_t n1 = 0, n2 = 0;
    for (int64_t b = 0; b < nb; ++b) { n1 += cnt[(size_t)(2 * b)]; n2 += cnt[(size_t)(2 * b + 1)]; }
    if (n_gathered) *n_gathered = n1 + n2;
    if (n1 + n2 == 0) return MCF_OK;
    // the cells of the plan's fast tiles first, in whole tiles; those of its other tiles in tiles of their own behind them: every
    // cell meets the instantiation it meets in a launch of the plan's own tiles (the two differ in the last bits)
    const int64_t base2 = (n1 + cpb - 1) / cpb * cpb, total = base2 + (n2 + cpb - 1) / cpb * cpb;
    const int64_t nt_sub = total / cpb, nt_fast = base2 / cpb, nt_slow = nt_sub - nt_fast;
    if (total > INT32_MAX) return fail(MCF_ERR_ARG, "too many cells");
    {
        int64_t o1 = 0, o2 = base2;
        for (int64_t b = 0; b < nb; ++b) {
            const int32_t c1 = cnt[(size_t)(2 * b)], c2 = cnt[(size_t)(2 * b + 1)];
            cnt[(size_t)(2 * b)] = (int32_t)o1; cnt[(size_t)(2 * b + 1)] = (int32_t)o2;
            o1 += c1; o2 += c2;
        }
    }
    // (buffers that grow are released first: hipFree waits for the device)
    if ((rc = p->dev.regrow(&p->d_celllist, &p->celllist_cap, total))) return rc;
    if ((rc = p->dev.regrow(&p->d_subimg, &p->subimg_cap, (int64_t)p->layers * nt_sub * IMG))) return rc;
    const int64_t day_doubles = p->ring_day_stride;                  // variables x block
    const double budget_gb = getenv("MCF_CELLS_RING_GB") ? atof(getenv("MCF_CELLS_RING_GB")) : 0.0;
    const int64_t budget = budget_gb > 0.0 ? (int64_t)(budget_gb * 1e9)
                                           : std::max<int64_t>((int64_t)512 << 20, (int64_t)p->ring_slots * p->slot_elems);       // (bytes: an eighth of the ring)
    const int pass_days = (int)std::max<int64_t>(1, std::min<int64_t>(ndays, budget / (nt_sub * day_doubles * 8)));
    if ((rc = p->dev.regrow(&p->d_subring, &p->subring_cap, nt_sub * pass_days * day_doubles))) return rc;
    if (nt_slow > 0 && fast && (rc = p->dev.regrow(&p->d_cells_slow, &p->cells_slow_cap, nt_slow))) return rc;
    const double t3 = now();
    HIP_TRY(hipMemcpyAsync(p->d_blockcnt, cnt.data(), (size_t)nb * 8, hipMemcpyHostToDevice, p->prep));
    HIP_TRY(hipMemsetAsync(p->d_celllist, 0xFF, (size_t)total * 4, p->prep));         // -1: no cell (a class's last tile)
    mcf::launch_cells_place(p->d_cls, N, p->d_blockcnt, p->d_celllist, p->prep);
    HIP_TRY(hipGetLastError());
    if (nt_slow > 0 && fast) {          // the second class's tile numbers, for the launch that takes a list
        std::vector<int32_t>& l = p->h_cells_slow;
        l.resize((size_t)nt_slow);
        for (int64_t t = 0; t < nt_slow; ++t) l[(size_t)t] = (int32_t)(nt_fast + t);
        HIP_TRY(hipMemcpyAsync(p->d_cells_slow, l.data(), l.size() * 4, hipMemcpyHostToDevice, p->prep));
    }
    HIP_TRY(hipEventRecord(p->ev_prep, p->prep));
    HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_prep, 0));
    // 2. their tiles' images
    mcf::launch_gather_image(p->d_celllist, nt_sub, p->d_cellc, p->ntiles, p->layers, cpb, p->d_subimg, p->stream);
    HIP_TRY(hipGetLastError());
    // 3. the solver on them, into a ring of their own — as many days at a time as the budget holds —, and from there to the
    // cells' places in the slot
    a.cellc = p->d_subimg; a.ntiles_total = nt_sub; a.N = total;
    a.out_base = p->d_subring;
    a.out_tile_stride = (int64_t)pass_days * day_doubles; a.out_day_stride = day_doubles; a.out_var_stride = blk;
    a.slot_day0 = 0;
    double* const slot_base = p->d_ring + (int64_t)slot * p->slot_elems + (int64_t)slot_day0 * p->ring_day_stride;
    for (int d = 0; d < ndays; d += pass_days) {
        const int nd = std::min(pass_days, ndays - d);
        a.day0 = day0 + d; a.ndays = nd;
        // (vector forcing above ground, as checked on entry: the plan's af and bg, which dispatch_solve passes on, are false;
        // these launches are not timed for mcf_plan_kernel_stats)
        dispatch_solve(p, a, fast, soil_daily, fast ? SolveTiles{nullptr, nt_fast, p->d_cells_slow, nt_slow} : SolveTiles{nullptr, nt_sub, nullptr, 0}, slot);
        HIP_TRY(hipGetLastError());
        mcf::launch_scatter_cells(p->d_celllist, nt_sub, p->d_subring, a.out_tile_stride, slot_base + (int64_t)d * p->ring_day_stride,
                                  p->ring_tile_stride, day_doubles, cpb, nd, p->stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(p->ev_cells_done, p->stream));
    if (trace)
        fprintf(stderr, "[mcf] run_days_cells: %lld cells x %d days; host ms: wait %.3f, class+counts %.3f, offsets+buffers %.3f, enqueue %.3f\n",
                (long long)(n1 + n2), (int)ndays, t1 - t0, t2 - t1, t3 - t2, now() - t3);
    p->cells_inflight = true;
    ++p->cells_runs;
    p->cells_gathered += (n1 + n2) * ndays;
    return MCF_OK;
}

int mcf_plan_dispatch_stats(mcf_plan* p, mcf_dispatch_stats* st) {
    if (!p || !st) return fail(MCF_ERR_ARG, "null argument");
    memset(st, 0, sizeof *st);
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    st->fast_tiles = p->fast_enabled ? p->n_fast : 0;
    st->slow_tiles = p->fast_enabled ? p->n_slow : (p->N + p->cpb - 1) / p->cpb;
    for (char c : p->day_irregular) st->irregular_days += c ? 1 : 0;
    st->fast_launches = p->fast_launches;
    st->slow_launches = p->slow_launches;
    if (p->d_fix_count) {
        int32_t v[2] = {0, 0};
        HIP_TRY(hipMemcpy(v, p->d_fix_count, 8, hipMemcpyDeviceToHost));
        st->canary_trips = v[1];
    }
    return MCF_OK;
}

int mcf_plan_belowground(mcf_plan* p) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    if (!p->bg) return fail(MCF_ERR_STATE, "reqhgt >= 0: nothing to smooth");
    if (p->bg_stream)
        return fail(MCF_ERR_STATE, "mcf_plan_belowground: a streamed plan leaves the final Tz in each chunk's slot "
                                   "(mcf_plan_below_prepare, then mcf_plan_run_days in day order)");
    if (p->var_slot[MCF_OUT_TZ] < 0) return MCF_OK;                      // cpp:2307 `&& out[0]`
    HIP_TRY(hipSetDevice(p->device));
    mcf::BelowArgs b{};
    b.N = p->N; b.tsteps = (int)p->tsteps; b.complete = p->opt.complete; b.hiy = p->hiy;
    b.per_cell_pointm = p->af ? 1 : 0;
    b.reqhgt = p->opt.reqhgt; b.mat = p->opt.mat;
    b.cellflag_hgt = p->d_veg[0];
    b.tg = p->d_tgser; b.ddsum = p->d_ddsum; b.Tgp = p->d_Tgp; b.Tbp = p->d_Tbp;
    b.scratch = p->d_scratch;
    b.tz = const_cast<double*>(ring_view(p, 0, MCF_OUT_TZ).base);      // reqhgt < 0: the linear ring
    if (p->tsteps > (int64_t)p->ring_days * 24)
        return fail(MCF_ERR_STATE, "ring slot smaller than the series");
    mcf::launch_belowground(b, p->stream);
    HIP_TRY(hipGetLastError());
    return MCF_OK;
}

int mcf_plan_sync(mcf_plan* p) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MCF_OK;
}

int mcf_plan_fetch(mcf_plan* p, int32_t slot, int32_t var, int64_t step0, int64_t nsteps, double* host_dst) {
    return mcf_plan_fetch_pitched(p, slot, var, step0, nsteps, host_dst, 0);
}

// `bytes` of dense [rows, ...] device memory into the caller's array (a block of a taller raster goes column by column into its place)
static int to_host(mcf_plan* p, double* dst, const double* src, size_t bytes, int64_t row_pitch) {
    const size_t width = (size_t)p->rows * 8;
    if (row_pitch != p->rows) HIP_TRY(p->tohost.pitched(dst, (size_t)row_pitch * 8, src, width, bytes / width, p->stream));
    else HIP_TRY(p->tohost.dense(dst, src, bytes, p->stream));
    return MCF_OK;
}
// steps [step0, step0 + nsteps) of `view` (a variable of the output ring, a diagnostic of the diagnostics ring) to the host
static int fetch_view(mcf_plan* p, const mcf::RingView& view, bool tiled, int64_t step0, int64_t nsteps, double* host_dst, int64_t row_pitch) {
    HIP_TRY(hipSetDevice(p->device));
    if (nsteps == 0) return MCF_OK;
    if (!tiled) return to_host(p, host_dst, view.base + p->N * step0, (size_t)(p->N * nsteps) * 8, row_pitch);
    // tiled ring: the reference's [rows, cols, steps] layout is made on the device (k_untile), in pieces of <= 1 GB
    const int64_t piece = std::max<int64_t>(1, std::min<int64_t>(nsteps, ((int64_t)1 << 27) / std::max<int64_t>(p->N, 1)));
    if (p->stage_elems < piece * p->N) {
        double* d = nullptr;
        if (const int rc = p->dev.make(&d, piece * p->N)) return rc;      // an earlier (smaller) buffer is released with the plan
        p->d_stage = d;
        p->stage_elems = piece * p->N;
    }
    for (int64_t k0 = 0; k0 < nsteps; k0 += piece) {
        const int64_t n = std::min(piece, nsteps - k0);
        mcf::launch_untile(view, step0 + k0, n, p->d_stage, p->stream);
        HIP_TRY(hipGetLastError());
        if (const int rc = to_host(p, host_dst + row_pitch * p->cols * k0, p->d_stage, (size_t)(p->N * n) * 8, row_pitch)) return rc;
    }
    return MCF_OK;
}

int mcf_plan_fetch_pitched(mcf_plan* p, int32_t slot, int32_t var, int64_t step0, int64_t nsteps, double* host_dst, int64_t row_pitch) {
    if (!p || !host_dst) return fail(MCF_ERR_ARG, "null argument");
    if (row_pitch == 0) row_pitch = p->rows;
    if (row_pitch < p->rows) return fail(MCF_ERR_ARG, "row_pitch smaller than rows");
    if (const int rc = check_slot_range(p, slot, var, step0, nsteps)) return rc;
    return fetch_view(p, ring_view(p, slot, var), p->tiled, step0, nsteps, host_dst, row_pitch);
}

static int diag_fetch_pitched(mcf_plan* p, int32_t slot, int32_t dvar, int64_t step0, int64_t nsteps, double* host_dst, int64_t row_pitch) {
    if (!p || !host_dst) return fail(MCF_ERR_ARG, "null argument");
    if (row_pitch == 0) row_pitch = p->rows;
    if (row_pitch < p->rows) return fail(MCF_ERR_ARG, "row_pitch smaller than rows");
    if (const int rc = check_diag_range(p, slot, dvar, step0, nsteps)) return rc;
    return fetch_view(p, diag_view(p, slot, dvar), true, step0, nsteps, host_dst, row_pitch);
}
int mcf_plan_diag_fetch(mcf_plan* p, int32_t slot, int32_t dvar, int64_t step0, int64_t nsteps, double* host_dst) {
    return diag_fetch_pitched(p, slot, dvar, step0, nsteps, host_dst, 0);
}

int mcf_plan_fetch_depth_pitched(mcf_plan* p, int32_t slot, int32_t depth, int64_t step0, int64_t nsteps, double* host_dst,
                                 int64_t row_pitch) {
    if (!p || !host_dst) return fail(MCF_ERR_ARG, "null argument");
    if (!p->bg_stream || p->var_slot[MCF_OUT_TZ] < 0)
        return fail(MCF_ERR_STATE, "mcf_plan_fetch_depth needs a streamed below-ground plan with Tz");
    if (depth < 0 || depth >= std::max<int>(1, (int)p->depths.size()))
        return fail(MCF_ERR_ARG, "mcf_plan_fetch_depth: depth " + std::to_string(depth) + " is outside the plan's list");
    if (row_pitch == 0) row_pitch = p->rows;
    if (row_pitch < p->rows) return fail(MCF_ERR_ARG, "row_pitch smaller than rows");
    if (const int rc = check_slot_range(p, slot, MCF_OUT_TZ, step0, nsteps)) return rc;
    return fetch_view(p, depth_view(p, slot, depth), true, step0, nsteps, host_dst, row_pitch);
}
int mcf_plan_fetch_depth(mcf_plan* p, int32_t slot, int32_t depth, int64_t step0, int64_t nsteps, double* host_dst) {
    return mcf_plan_fetch_depth_pitched(p, slot, depth, step0, nsteps, host_dst, 0);
}

int mcf_plan_fetch_cells(mcf_plan* p, int32_t slot, int32_t var, int64_t step0, int64_t nsteps, const int64_t* cells,
                         int64_t ncells, double* host_dst) {
    if (!p || !host_dst || !cells) return fail(MCF_ERR_ARG, "null argument");
    if (const int rc = check_slot_range(p, slot, var, step0, nsteps)) return rc;
    if (ncells < 0) return fail(MCF_ERR_ARG, "negative cell count");
    for (int64_t i = 0; i < ncells; ++i)
        if (cells[i] < 0 || cells[i] >= p->N) return fail(MCF_ERR_ARG, "cell index outside the raster");
    if (ncells == 0 || nsteps == 0) return MCF_OK;
    HIP_TRY(hipSetDevice(p->device));
    mcf::DevOwner tmp;
    int64_t* d_cells = nullptr;
    double* d_dst = nullptr;
    int rc;
    if ((rc = tmp.alloc((void**)&d_cells, ncells * 8))) return rc;
    if ((rc = tmp.alloc((void**)&d_dst, ncells * nsteps * 8))) return rc;
    HIP_TRY(hipMemcpyAsync(d_cells, cells, (size_t)ncells * 8, hipMemcpyHostToDevice, p->stream));
    mcf::launch_gather_cells(ring_view(p, slot, var), step0, nsteps, d_cells, ncells, d_dst, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_dst, d_dst, (size_t)(ncells * nsteps) * 8, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MCF_OK;
}

int mcf_plan_fetch_packed(mcf_plan* p, int32_t slot, int32_t var, int64_t step0, int64_t nsteps, double scale,
                          int32_t* host_dst, float* kernel_ms) {
    if (!p || !host_dst) return fail(MCF_ERR_ARG, "null argument");
    if (const int rc = check_slot_range(p, slot, var, step0, nsteps)) return rc;
    if (nsteps > 65535) return fail(MCF_ERR_ARG, "at most 65535 steps per packed fetch");
    HIP_TRY(hipSetDevice(p->device));
    if (p->pack_elems < p->N * nsteps) {
        int32_t* d = nullptr;
        if (const int rc = p->dev.make(&d, p->N * nsteps)) return rc;     // earlier (smaller) buffers are released with the plan
        p->d_pack = d;
        p->pack_elems = p->N * nsteps;
    }
    if (kernel_ms) HIP_TRY(hipEventRecord(p->ev0, p->stream));
    mcf::launch_pack_transpose(ring_view(p, slot, var), step0, p->rows, p->cols, nsteps, scale, p->d_pack, p->stream);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) HIP_TRY(hipEventRecord(p->ev1, p->stream));
    HIP_TRY(hipMemcpyAsync(host_dst, p->d_pack, (size_t)(p->N * nsteps) * 4, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, p->ev0, p->ev1));
    return MCF_OK;
}

int mcf_nc_create(const char* path, const mcf_nc_spec* sp, mcf_ncfile** out) {
    if (!path || !sp || !out) return fail(MCF_ERR_ARG, "null argument");
    if (sp->rows <= 0 || sp->cols <= 0 || sp->nsteps < 0 || !sp->east || !sp->north || (sp->nsteps > 0 && !sp->time_hours))
        return fail(MCF_ERR_ARG, "mcf_nc_create: bad dimensions or null coordinate vector");
    mcf_ncfile* nc = new mcf_ncfile();
    std::vector<mcf::NcVarDef> defs;
    for (int v = 0; v < MCF_NOUT; ++v) {
        nc->var_of[v] = -1;
        if (!sp->vars[v]) continue;
        mcf::NcVarDef d;
        double sc;
        bool put;
        if (!nc_var_def(v, sp->reqhgt, &d, &sc, &put)) {
            delete nc;
            return fail(MCF_ERR_ARG, "mcf_nc_create: writetonc defines no variable '" + d.name + "' at this reqhgt");
        }
        const int k = (int)defs.size();
        nc->var_of[v] = k; nc->out_of[k] = v; nc->scale[k] = sc;
        nc->fill_only[k] = (sp->reference_puts_only && !put) ? 1 : 0;
        defs.push_back(d);
    }
    if (defs.empty()) { delete nc; return fail(MCF_ERR_ARG, "mcf_nc_create: no variable selected"); }
    return nc_open("mcf_nc_create", nc, path, sp->format, sp->deflate_level, sp->rows, sp->cols, sp->nsteps, sp->east, sp->north,
                   sp->time_hours, sp->crs_wkt, defs, out);
}

// The snowpack's file (include/mcf.h "netCDF sink: further sources"): the five series of mcf_snowdriver_out as int variables
int mcf_nc_create_snowpack(const char* path, const mcf_ncpack_spec* sp, mcf_ncfile** out) {
    const std::string w = "mcf_nc_create_snowpack: ";
    if (!path || !sp || !out) return fail(MCF_ERR_ARG, w + "null argument");
    if (sp->rows <= 0 || sp->cols <= 0 || sp->nsteps < 0 || !sp->east || !sp->north || (sp->nsteps > 0 && !sp->time_hours))
        return fail(MCF_ERR_ARG, w + "bad dimensions or null coordinate vector");
    static const char* names[5] = {"Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden"};
    static const char* longs[5] = {"Canopy snow temperature", "Ground snow temperature", "Ground snow depth", "Total snow water equivalent",
                                   "Snow density"};
    static const char* units[5] = {"deg C x 100", "deg C x 100", "mm", "mm x 100", "kg / m^3"};
    static const double scales[5] = {100, 100, 1000, 100, 1};
    mcf_ncfile* nc = new mcf_ncfile();
    nc->snowpack = true;
    std::vector<mcf::NcVarDef> defs;
    for (int v = 0; v < MCF_NOUT; ++v) nc->var_of[v] = -1;
    for (int v = 0; v < 5; ++v) {
        if (!sp->series[v]) continue;
        if (!(sp->scale[v] >= 0.0 && sp->scale[v] < HUGE_VAL)) { delete nc; return fail(MCF_ERR_ARG, w + "scale of '" + names[v] + "' is negative or not finite"); }
        const int k = (int)defs.size();
        nc->var_of[v] = k; nc->out_of[k] = v; nc->scale[k] = sp->scale[v] > 0.0 ? sp->scale[v] : scales[v];
        nc->fill_only[k] = 0;
        mcf::NcVarDef d;
        d.name = names[v];
        d.long_name = sp->long_name[v] ? sp->long_name[v] : longs[v];
        d.units = sp->units[v] ? sp->units[v] : units[v];
        defs.push_back(d);
    }
    if (defs.empty()) { delete nc; return fail(MCF_ERR_ARG, w + "no series selected"); }
    return nc_open("mcf_nc_create_snowpack", nc, path, sp->format, sp->deflate_level, sp->rows, sp->cols, sp->nsteps, sp->east, sp->north,
                   sp->time_hours, sp->crs_wkt, defs, out);
}

int mcf_nc_close(mcf_ncfile* nc) {
    if (!nc) return MCF_OK;
    const std::string e = nc->f->close();
    delete nc;
    return e.empty() ? MCF_OK : fail(MCF_ERR_ARG, "mcf_nc_close: " + e);
}

int mcf_nc_write_host(mcf_ncfile* nc, int64_t step0, int64_t nsteps, const double* const vars[MCF_NOUT]) {
    if (!nc || !vars) return fail(MCF_ERR_ARG, "null argument");
    if (step0 < 0 || nsteps < 0 || step0 + nsteps > nc->f->nsteps) return fail(MCF_ERR_ARG, "mcf_nc_write_host: step range outside the file");
    const int64_t R = nc->f->rows, C = nc->f->cols, N = R * C, rb = nc->f->rec_bytes;
    for (int k = 0; k < nc->f->nvars; ++k)
        if (!nc->fill_only[k] && !vars[nc->out_of[k]]) return fail(MCF_ERR_ARG, "mcf_nc_write_host: a variable of the file is missing");
    const int64_t piece = std::max<int64_t>(1, ((int64_t)64 << 20) / rb);
    for (int64_t s0 = 0; s0 < nsteps; s0 += piece) {
        const int64_t n = std::min(piece, nsteps - s0);
        uint8_t* st = nc->staging(0, (size_t)(n * rb));
        for (int64_t s = 0; s < n; ++s)
            for (int k = 0; k < nc->f->nvars; ++k) {
                uint8_t* dst = st + s * rb + 8 + (int64_t)k * N * 4;
                const double* src = nc->fill_only[k] ? nullptr : vars[nc->out_of[k]] + (s0 + s) * N;
                for (int64_t r = 0; r < R; ++r)
                    for (int64_t c = 0; c < C; ++c)
                        mcf::NcFile::store_i32(dst + 4 * (c + C * r), src ? nc_pack(src[r + R * c], nc->scale[k]) : mcf::NcFile::kMissval);
            }
        const std::string e = nc->f->write_records(step0 + s0, n, st);
        if (!e.empty()) return fail(MCF_ERR_ARG, "mcf_nc_write_host: " + e);
    }
    return MCF_OK;
}

// Steps [slot_step0, slot_step0 + nsteps) of ring slot `slot` as rows [row0, row0 + plan rows) of records [file_step0, ...):
// k_pack_nc packs the plan's rows as records of their own ([step][8 B | var][plan rows][cols]), which are the file's records
// where the plan's grid is the file's and a row strip of them otherwise.  tz_only: every variable but Tz holds missval (the steps a
// streamed below-ground chunk leaves behind its last whole day).
static int nc_write_rows(const std::string& w, mcf_ncfile* nc, mcf_plan* p, int32_t slot, int32_t depth, int64_t row0, int64_t slot_step0,
                         int64_t file_step0, int64_t nsteps, float* kernel_ms, bool tz_only) {
    if (!nc || !p) return fail(MCF_ERR_ARG, "null argument");
    if (nc->snowpack) return fail(MCF_ERR_ARG, w + "the file holds the snowpack's series (mcf_snowplan_nc_write)");
    const bool whole = row0 == 0 && nc->f->rows == p->rows;
    if (nc->f->cols != p->cols || row0 < 0 || row0 + p->rows > nc->f->rows)
        return fail(MCF_ERR_ARG, w + (row0 == 0 ? "the file's grid is not the plan's" : "the plan's rows at row0 are not a row strip of the file's grid"));
    if (!whole && !nc->f->takes_strips())
        return fail(MCF_ERR_ARG, w + "the netCDF-4 container chunks a step into row strips of the whole raster: it takes one block, not a row strip");
    if (depth != 0 && (!p->bg_stream || depth < 0 || depth >= std::max<int>(1, (int)p->depths.size())))
        return fail(MCF_ERR_ARG, w + "depth " + std::to_string(depth) + " is outside the plan's list (0 unless the plan is streamed below ground with depths)");
    if (const int rc = check_slot_range(p, slot, kAnyVar, slot_step0, nsteps)) return rc;
    if (file_step0 < 0 || file_step0 + nsteps > nc->f->nsteps) return fail(MCF_ERR_ARG, w + "step range outside the file");
    mcf::PackNcArgs a{};
    a.nv = nc->f->nvars; a.missval = mcf::NcFile::kMissval; a.rows = p->rows; a.cols = p->cols;
    const int64_t rb = 8 + (int64_t)a.nv * p->N * 4;      // a packed record of the plan's rows: the file's own where the grids agree
    a.rec_words = rb / 4;
    for (int k = 0; k < a.nv; ++k) {
        const int v = nc->out_of[k];
        a.scale[k] = nc->scale[k];
        a.fill_only[k] = nc->fill_only[k] || (tz_only && v != MCF_OUT_TZ);
        if (a.fill_only[k]) { a.src[k] = mcf::RingView{p->d_ring, p->N, 0, 0, 0}; continue; }   // never read
        if (p->var_slot[v] < 0) return fail(MCF_ERR_ARG, w + "a variable of the file was not requested in out[]");
        a.src[k] = v == MCF_OUT_TZ && depth != 0 ? depth_view(p, slot, depth) : ring_view(p, slot, v);
    }
    HIP_TRY(hipSetDevice(p->device));
    int64_t piece = std::min<int64_t>(65535 / a.nv, std::max<int64_t>(1, ((int64_t)256 << 20) / rb));
    piece = std::min(piece, std::max<int64_t>(nsteps, 1));
    if (p->pack_elems < piece * (rb / 4)) {
        int32_t* d = nullptr;
        if (const int rc = p->dev.make(&d, piece * (rb / 4))) return rc;
        p->d_pack = d;
        p->pack_elems = piece * (rb / 4);
    }
    a.dst = p->d_pack;
    // a row strip is staged in this call's own buffers: the blocks' workers write strips of one file at the same time
    std::unique_ptr<uint8_t[]> own[2];
    std::future<std::string> pending;            // the previous piece going to disk while this one is packed and copied
    float kms = 0;
    int rc = MCF_OK;
    std::string werr;
    for (int64_t s0 = 0, i = 0; s0 < nsteps && rc == MCF_OK; s0 += piece, ++i) {
        const int64_t n = std::min(piece, nsteps - s0);
        mcf::PackNcArgs b = a;
        b.step0 = slot_step0 + s0;
        hipError_t e = hipSuccess;
        if (kernel_ms) e = hipEventRecord(p->ev0, p->stream);
        mcf::launch_pack_nc(b, n, p->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess && kernel_ms) e = hipEventRecord(p->ev1, p->stream);
        // stage[i & 1] was handed to the writer two pieces ago: that write has been joined (below) before piece i-1 began
        const size_t bytes = (size_t)(n * rb);
        uint8_t* st;
        if (whole) st = nc->staging((int)(i & 1), bytes);
        else {
            if (!own[i & 1]) own[i & 1].reset(new uint8_t[(size_t)(piece * rb)]);
            st = own[i & 1].get();
        }
        if (e == hipSuccess) e = p->tohost.dense(st, p->d_pack, bytes, p->stream);
        if (e == hipSuccess && kernel_ms) {
            float ms = 0;
            e = hipEventElapsedTime(&ms, p->ev0, p->ev1);
            kms += ms;
        }
        if (pending.valid()) werr = pending.get();
        if (e != hipSuccess) { rc = fail(MCF_ERR_HIP, w + hipGetErrorString(e)); break; }
        if (!werr.empty()) break;
        mcf::NcFile* f = nc->f.get();
        uint8_t* data = st;
        const int64_t fs = file_step0 + s0, nr = p->rows;
        if (whole) pending = std::async(std::launch::async, [f, fs, n, data] { return f->write_records(fs, n, data); });
        else pending = std::async(std::launch::async, [f, fs, n, row0, nr, data] { return f->write_strip(fs, n, row0, nr, data); });
    }
    if (pending.valid()) {
        const std::string e2 = pending.get();
        if (werr.empty()) werr = e2;
    }
    if (rc != MCF_OK) return rc;
    if (!werr.empty()) return fail(MCF_ERR_ARG, w + werr);
    if (kernel_ms) *kernel_ms = kms;
    return MCF_OK;
}
int mcf_nc_write_plan(mcf_ncfile* nc, mcf_plan* p, int32_t slot, int64_t slot_step0, int64_t file_step0, int64_t nsteps,
                      float* kernel_ms) {
    if (nc && p && nc->f->rows != p->rows) return fail(MCF_ERR_ARG, "mcf_nc_write_plan: the file's grid is not the plan's");
    return nc_write_rows("mcf_nc_write_plan: ", nc, p, slot, 0, 0, slot_step0, file_step0, nsteps, kernel_ms, false);
}
int mcf_nc_write_plan_rows(mcf_ncfile* nc, mcf_plan* p, int32_t slot, int32_t depth, int64_t row0, int64_t slot_step0, int64_t file_step0,
                           int64_t nsteps, float* kernel_ms) {
    return nc_write_rows("mcf_nc_write_plan_rows: ", nc, p, slot, depth, row0, slot_step0, file_step0, nsteps, kernel_ms, false);
}
// Host only: missval in every variable of rows [row0, row0 + nrows) of records [file_step0, file_step0 + nsteps)
int mcf_nc_write_missing(mcf_ncfile* nc, int64_t row0, int64_t nrows, int64_t file_step0, int64_t nsteps) {
    const std::string w = "mcf_nc_write_missing: ";
    if (!nc) return fail(MCF_ERR_ARG, w + "null argument");
    if (file_step0 < 0 || nsteps < 0 || file_step0 + nsteps > nc->f->nsteps) return fail(MCF_ERR_ARG, w + "step range outside the file");
    if (row0 < 0 || nrows < 1 || row0 + nrows > nc->f->rows) return fail(MCF_ERR_ARG, w + "row strip outside the file's grid");
    if (!(row0 == 0 && nrows == nc->f->rows) && !nc->f->takes_strips())
        return fail(MCF_ERR_ARG, w + "the netCDF-4 container chunks a step into row strips of the whole raster: it takes one block, not a row strip");
    const std::string e = mcf::nc_write_missing(nc->f.get(), row0, nrows, file_step0, nsteps);
    return e.empty() ? (int)MCF_OK : fail(MCF_ERR_ARG, w + e);
}
// Host only: rows [row0, row0 + nrows) of records [step0, step0 + nsteps) from host arrays, vars[v] = [nrows, cols, nsteps]
// column-major doubles (a row block's arrays); mcf_nc_write_host is this with the whole raster
int mcf_nc_write_host_rows(mcf_ncfile* nc, int64_t row0, int64_t nrows, int64_t step0, int64_t nsteps, const double* const vars[MCF_NOUT]) {
    const std::string w = "mcf_nc_write_host_rows: ";
    if (!nc || !vars) return fail(MCF_ERR_ARG, w + "null argument");
    if (step0 < 0 || nsteps < 0 || step0 + nsteps > nc->f->nsteps) return fail(MCF_ERR_ARG, w + "step range outside the file");
    if (row0 < 0 || nrows < 1 || row0 + nrows > nc->f->rows) return fail(MCF_ERR_ARG, w + "row strip outside the file's grid");
    if (!(row0 == 0 && nrows == nc->f->rows) && !nc->f->takes_strips())
        return fail(MCF_ERR_ARG, w + "the netCDF-4 container chunks a step into row strips of the whole raster: it takes one block, not a row strip");
    const int nv = nc->f->nvars;
    const int64_t R = nrows, C = nc->f->cols, N = R * C, rb = 8 + (int64_t)nv * N * 4;
    for (int k = 0; k < nv; ++k)
        if (!nc->fill_only[k] && !vars[nc->out_of[k]]) return fail(MCF_ERR_ARG, w + "a variable of the file is missing");
    const int64_t piece = std::max<int64_t>(1, std::min(std::max<int64_t>(nsteps, 1), ((int64_t)64 << 20) / rb));
    std::unique_ptr<uint8_t[]> st(new uint8_t[(size_t)(piece * rb)]);      // (this call's own: several threads write strips at once)
    for (int64_t s0 = 0; s0 < nsteps; s0 += piece) {
        const int64_t n = std::min(piece, nsteps - s0);
        for (int64_t s = 0; s < n; ++s)
            for (int k = 0; k < nv; ++k) {
                uint8_t* dst = st.get() + s * rb + 8 + (int64_t)k * N * 4;
                const double* src = nc->fill_only[k] ? nullptr : vars[nc->out_of[k]] + (s0 + s) * N;
                for (int64_t r = 0; r < R; ++r)
                    for (int64_t c = 0; c < C; ++c)
                        mcf::NcFile::store_i32(dst + 4 * (c + C * r), src ? nc_pack(src[r + R * c], nc->scale[k]) : mcf::NcFile::kMissval);
            }
        const std::string e = nc->f->write_strip(step0 + s0, n, row0, nrows, st.get());
        if (!e.empty()) return fail(MCF_ERR_ARG, w + e);
    }
    return MCF_OK;
}

int mcf_plan_slot_ptr(mcf_plan* p, int32_t slot, int32_t var, void** dev_ptr) {
    if (!p || !dev_ptr) return fail(MCF_ERR_ARG, "null argument");
    if (const int rc = check_slot_range(p, slot, var, 0, 0)) return rc;
    *dev_ptr = const_cast<double*>(ring_view(p, slot, var).base);
    return MCF_OK;
}

int mcf_plan_ring_layout(mcf_plan* p, mcf_ring_layout* out) {
    if (!p || !out) return fail(MCF_ERR_ARG, "null argument");
    memset(out, 0, sizeof *out);
    out->tiled = p->tiled ? 1 : 0;
    out->cells = p->N;
    out->slot_days = p->ring_days;
    if (p->tiled) {
        out->cells_per_tile = p->cpb;
        out->block_doubles = mcf::ring_block_doubles(p->cpb);
        out->tile_stride = p->ring_tile_stride;
        out->day_stride = p->ring_day_stride;
    }
    return MCF_OK;
}

// the diagnostics ring of a plan whose kind of forcing the caller has checked: one set of rules for both entries
static int diag_enable(mcf_plan* p, const int32_t sel[MCF_NDIAG], const char* entry) {
    if (p->bg || p->opt.reqhgt < 0.0) return fail(MCF_ERR_ARG, "diagnostics need reqhgt >= 0");
    if (p->bg_stream) return fail(MCF_ERR_ARG, "diagnostics are not available on a streamed plan");
    if (p->d_dring) return fail(MCF_ERR_STATE, "diagnostics are already enabled on this plan");
    if (p->has_run) return fail(MCF_ERR_STATE, std::string(entry) + " comes before the plan's first run");
    int n = 0;
    for (int v = 0; v < MCF_NDIAG; ++v) n += sel[v] ? 1 : 0;
    if (n == 0) return fail(MCF_ERR_ARG, "no diagnostic selected");
    HIP_TRY(hipSetDevice(p->device));
    const int64_t blk = mcf::ring_block_doubles(p->cpb);
    const int64_t day_stride = (int64_t)n * blk, tile_stride = (int64_t)p->ring_days * day_stride, slot_elems = p->ntiles * tile_stride;
    if (const int rc = p->dev.make(&p->d_dring, (int64_t)p->ring_slots * slot_elems)) return rc;
    p->dg_day_stride = day_stride; p->dg_tile_stride = tile_stride; p->dg_slot_elems = slot_elems;
    p->ndiag = 0;
    for (int v = 0; v < MCF_NDIAG; ++v) p->dg_slab1[v] = sel[v] ? ++p->ndiag : 0;
    return MCF_OK;
}

int mcf_plan_diag_enable(mcf_plan* p, const int32_t sel[MCF_NDIAG]) {
    if (!p || !sel) return fail(MCF_ERR_ARG, "null argument");
    if (p->af) return fail(MCF_ERR_ARG, p->coarse ? "diagnostics are not available with coarse array forcing"
                                                  : "diagnostics are not available with array forcing");
    return diag_enable(p, sel, "mcf_plan_diag_enable");
}
// array forcing, fine or coarse: the same ring filled by k_solve_diag_af (the entry above keeps its refusal, as
// mcf_plan_summary_enable does beside mcf_plan_summary_enable_below)
int mcf_plan_diag_enable_array(mcf_plan* p, const int32_t sel[MCF_NDIAG]) {
    if (!p || !sel) return fail(MCF_ERR_ARG, "null argument");
    if (!p->af) return fail(MCF_ERR_ARG, "mcf_plan_diag_enable_array needs an array-forcing plan: mcf_plan_diag_enable for vector forcing");
    return diag_enable(p, sel, "mcf_plan_diag_enable_array");
}

int mcf_plan_diag_slot_ptr(mcf_plan* p, int32_t slot, int32_t dvar, void** dev_ptr) {
    if (!p || !dev_ptr) return fail(MCF_ERR_ARG, "null argument");
    if (const int rc = check_diag_range(p, slot, dvar, 0, 0)) return rc;
    *dev_ptr = const_cast<double*>(diag_view(p, slot, dvar).base);
    return MCF_OK;
}

int mcf_plan_diag_ring_layout(mcf_plan* p, mcf_ring_layout* out) {
    if (!p || !out) return fail(MCF_ERR_ARG, "null argument");
    if (!p->d_dring) return fail(MCF_ERR_STATE, "the plan has no diagnostics ring: mcf_plan_diag_enable first");
    memset(out, 0, sizeof *out);
    out->tiled = 1;
    out->cells = p->N;
    out->slot_days = p->ring_days;
    out->cells_per_tile = p->cpb;
    out->block_doubles = mcf::ring_block_doubles(p->cpb);
    out->tile_stride = p->dg_tile_stride;
    out->day_stride = p->dg_day_stride;
    return MCF_OK;
}

int64_t mcf_ring_index(const mcf_ring_layout* l, int64_t cell, int64_t step) {
    if (!l || cell < 0 || cell >= l->cells || step < 0 || step >= (int64_t)l->slot_days * 24) return -1;
    mcf::RingView v{nullptr, l->cells, l->tile_stride, l->day_stride, l->tiled ? l->cells_per_tile : 0};
    return v.index(cell, step);
}

int mcf_plan_timer_start(mcf_plan* p) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    return MCF_OK;
}

int mcf_plan_timer_stop(mcf_plan* p, float* ms) {
    if (!p || !ms) return fail(MCF_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    HIP_TRY(hipEventSynchronize(p->ev1));
    HIP_TRY(hipEventElapsedTime(ms, p->ev0, p->ev1));
    return MCF_OK;
}

int mcf_plan_kernel_timing(mcf_plan* p, int32_t enable) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    p->ktiming = enable != 0;
    if (!enable) return MCF_OK;
    for (auto& e : p->kev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    p->kev.clear();
    p->ktotal_ms = 0;
    p->klaunches = 0;
    return MCF_OK;
}

int mcf_plan_kernel_stats(mcf_plan* p, double* total_ms, int64_t* launches) {
    if (!p || !total_ms || !launches) return fail(MCF_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    for (auto& e : p->kev) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
        p->ktotal_ms += ms;
        p->klaunches += 1;
        hipEventDestroy(e.first);
        hipEventDestroy(e.second);
    }
    p->kev.clear();
    *total_ms = p->ktotal_ms;
    *launches = p->klaunches;
    return MCF_OK;
}

int mcf_selftest_math(int32_t kind, const double* x, const double* y, double* out, int64_t n, int32_t device) {
    if (!x || !out || n < 0) return fail(MCF_ERR_ARG, "null argument");
    int rc = ensure_device(device);
    if (rc) return rc;
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    mcf::DevOwner tmp;
    const int64_t nb = std::max<int64_t>(n, 1) * 8;
    if ((rc = tmp.alloc((void**)&dx, nb))) return rc;
    if ((rc = tmp.alloc((void**)&dout, nb))) return rc;
    HIP_TRY(hipMemcpy(dx, x, (size_t)n * 8, hipMemcpyHostToDevice));
    if (y) {
        if ((rc = tmp.alloc((void**)&dy, nb))) return rc;
        HIP_TRY(hipMemcpy(dy, y, (size_t)n * 8, hipMemcpyHostToDevice));
    }
    mcf::launch_selftest_math(kind, dx, dy, dout, n, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost));
    return MCF_OK;
}

static const int32_t kBioSt[14] = {0, 24, 48, 72, 96, 120, 144, 168, 192, 216, 240, 264, 288, 312};
static const int32_t kBioEd[14] = {23, 47, 71, 95, 119, 143, 167, 191, 215, 239, 263, 287, 311, 335};
// the requested matrices of bio [19][N] into the caller's arrays (out_pitch > rows: a row block's rows of taller matrices)
static int bioclim_download(mcf_plan* p, const mcf_grid_inputs* in, const mcf_bioclim_sel* sel, mcf_bioclim_out* out, const double* bio,
                            int64_t out_pitch) {
    const int64_t N = in->rows * in->cols;
    for (int v = 0; v < MCF_NBIO; ++v)
        if (sel->out[v]) {
            if (!out->bio[v]) return fail(MCF_ERR_ARG, "requested bioclim variable has a null buffer");
            if (out_pitch > in->rows)
                HIP_TRY(hipMemcpy2DAsync(out->bio[v], (size_t)out_pitch * 8, bio + (int64_t)v * N, (size_t)in->rows * 8,
                                         (size_t)in->rows * 8, (size_t)in->cols, hipMemcpyDeviceToHost, p->stream));
            else
                HIP_TRY(hipMemcpyAsync(out->bio[v], bio + (int64_t)v * N, (size_t)N * 8, hipMemcpyDeviceToHost, p->stream));
        }
    return mcf_plan_sync(p);
}
// solver chunk launches of this thread's last bioclim call (mcf_bioclim_last_chunks); 0: the whole-series route
static thread_local int g_bioclim_chunks = 0;
// twi_mean / out_pitch: a row block of a taller raster (the bioclim `_multi` entries): the raster-wide twi mean to install, and
// the rows of the caller's [rows_total, cols] matrices the block's rows are written into in place
static int run_bioclim(const mcf_grid_inputs* in_caller, const mcf_options* opt_in, const mcf_bioclim_sel* sel,
                       mcf_bioclim_out* out, int want_af, int layered = 0, const double* twi_mean = nullptr, int64_t out_pitch = 0) {
    g_bioclim_chunks = 0;
    if (!sel || !out || !in_caller) return fail(MCF_ERR_ARG, "null bioclim argument");
    // runbioclim3Cpp / 4Cpp (cpp:3620-3658 / 3660-3700): vegetation arrays [rows, cols, >= 14] and a fixed dfsel of
    // fourteen one-day layers — the twelve monthly days, the hottest and the coldest day; later steps (the quarter
    // days) belong to no layer and stay NA, as in the reference
    mcf_grid_inputs in_l;
    if (layered) {
        in_l = *in_caller;
        in_l.veg_layers = 14;
        in_l.lyr_st = kBioSt;
        in_l.lyr_ed = kBioEd;
    }
    const mcf_grid_inputs* in = layered ? &in_l : in_caller;
    int rc = check_inputs(in, opt_in);
    if (rc) return rc;
    if ((in->array_forcing != 0) != (want_af != 0)) return fail(MCF_ERR_ARG, "forcing geometry does not match the entry point");
    const int64_t T = in->tsteps, N = in->rows * in->cols;
    if (T < 336 || T % 24 != 0) return fail(MCF_ERR_ARG, "runbioclim needs >= 336 hourly steps in whole days");
    const int32_t* q[4] = {sel->wetq, sel->dryq, sel->hotq, sel->colq};
    const int32_t nq[4] = {sel->nwet, sel->ndry, sel->nhot, sel->ncol};
    for (int i = 0; i < 4; ++i) {
        if (nq[i] < 0 || (nq[i] > 0 && !q[i])) return fail(MCF_ERR_ARG, "bad quarter index vector");
        for (int j = 0; j < nq[i]; ++j)
            if (q[i][j] < 0 || q[i][j] >= T) return fail(MCF_ERR_ARG, "quarter index outside the time series");
    }
    mcf_options opt = *opt_in;
    opt.complete = 1;                                                   // cpp:3576: complete = true
    for (int v = 0; v < MCF_NOUT; ++v) opt.out[v] = 0;
    const int tvar = sel->air ? MCF_OUT_TZ : MCF_OUT_TLEAF;              // cpp:3569-3575
    opt.out[tvar] = 1;
    opt.out[MCF_OUT_SOILM] = 1;
    if ((rc = ensure_device(opt.device))) return rc;
    const int ndays = (int)(T / 24);
    // Streamed (round 5; vector or coarse array forcing above ground, quarter lists in ascending order — what runbioclim passes):
    // the solver runs in day chunks into a ring of a few GB and k_bioclim_acc folds each chunk into 29 doubles of running state per cell;
    // nothing of size cells x steps is allocated (the whole-series form below needs 2 x 8 B x cells x steps: 167 GB for a 4096^2
    // raster, most of the call's time).  Same accumulation order, same operands: the matrices are bit for bit the whole-series
    // form's (MCF_BIOCLIM_WHOLE=1 selects that one: the A/B of tests/test_bioclim_gpu.py, tests/test_bioclim_coarse_gpu.py).
    // Fine array forcing stays whole-series: its inputs are cells x steps by themselves.  Coarse array forcing keeps its series
    // resident on the coarse grid, so nothing but the ring and the running state scales with the raster.
    bool streamed = in->array_forcing != 1 && !(opt.reqhgt < 0.0) && getenv("MCF_BIOCLIM_WHOLE") == nullptr;
    for (int i = 0; streamed && i < 4; ++i)
        for (int j = 1; j < nq[i]; ++j)
            if (q[i][j] < q[i][j - 1]) streamed = false;
    int chunk_days = ndays;
    if (streamed) {      // the ring of the two variables, on mcf_plan_create's tiles
        const int cpb = in->array_forcing == 2 ? 32 : opt.cells_per_block ? opt.cells_per_block : 21;
        chunk_days = std::min(ndays, ring_budget_days("MCF_BIOCLIM_RING_GB", 2, N, cpb));
    }
    mcf_plan* p = nullptr;
    if ((rc = mcf_plan_create(in, &opt, chunk_days, 1, &p))) return rc;
    PlanHolder holder(p);
    if (twi_mean && (rc = mcf_plan_set_twi_mean(p, *twi_mean))) return rc;
    if (streamed && p->tiled) {
        mcf::BioAccArgs acc{};
        acc.N = N;
        acc.tz = ring_view(p, 0, tvar); acc.soilm = ring_view(p, 0, MCF_OUT_SOILM);
        if ((rc = upload_quarters(p, q, nq, acc.q))) return rc;
        if ((rc = p->dev.make(&acc.state, (int64_t)mcf::kBioStateRows * N))) return rc;
        // (the streamed route takes vector or coarse forcing: the driver has no forcing to upload)
        rc = for_day_chunks(p, in, ndays, p->ring_days, [&](int d0, int nd) -> int {
            ++g_bioclim_chunks;
            acc.day0 = d0; acc.ndays = nd;
            for (int i = 0; i < 4; ++i) {
                acc.qlo[i] = (int32_t)(std::lower_bound(q[i], q[i] + nq[i], d0 * 24) - q[i]);
                acc.qhi[i] = (int32_t)(std::lower_bound(q[i], q[i] + nq[i], (d0 + nd) * 24) - q[i]);
            }
            mcf::launch_bioclim_acc(acc, p->stream);
            HIP_TRY(hipGetLastError());
            return MCF_OK;
        });
        if (rc) return rc;
        mcf::BioFinArgs fin{};
        fin.N = N; fin.tsteps = (int)T; fin.state = acc.state;
        fin.cellc = p->d_cellc; fin.ntiles_total = p->ntiles; fin.cpb = p->cpb; fin.daylayer = p->d_daylayer; fin.tt = p->d_tt;
        if (p->coarse) {
            // no per-day table: the second pass taps the resident coarse soil moisture series as the solver does (mcf_kernels.h)
            fin.cforce = p->d_force;
            fin.cstride = (int64_t)p->crows * p->ccols * std::max<int64_t>(p->tsteps, 1);
            fin.crows = p->crows; fin.ccols = p->ccols;
            fin.crowpos = p->d_crowpos; fin.ccolpos = p->d_ccolpos; fin.rows = (int32_t)p->rows;
        }
        if ((rc = p->dev.make(&fin.bio, (int64_t)MCF_NBIO * N))) return rc;
        mcf::launch_bioclim_fin(fin, p->stream);
        HIP_TRY(hipGetLastError());
        return bioclim_download(p, in, sel, out, fin.bio, out_pitch);
    }
    if (streamed) return fail(MCF_ERR_STATE, "bioclim: the streamed sink expects the tiled ring");
    if (in->array_forcing && (rc = mcf_plan_upload_forcing_days(p, in, 0, ndays, 0))) return rc;
    if ((rc = mcf_plan_run_days(p, 0, ndays, 0))) return rc;
    if (p->bg && (rc = mcf_plan_belowground(p))) return rc;
    mcf::BioclimArgs b{};
    b.N = N; b.tsteps = (int)T;
    b.tz = ring_view(p, 0, tvar); b.soilm = ring_view(p, 0, MCF_OUT_SOILM);
    const int32_t* dq[4];
    if ((rc = upload_quarters(p, q, nq, dq))) return rc;
    b.wetq = dq[0]; b.dryq = dq[1]; b.hotq = dq[2]; b.colq = dq[3];
    b.nwet = nq[0]; b.ndry = nq[1]; b.nhot = nq[2]; b.ncol = nq[3];
    if ((rc = p->dev.make(&b.bio, (int64_t)MCF_NBIO * N))) return rc;
    mcf::launch_bioclim(b, p->stream);
    HIP_TRY(hipGetLastError());
    return bioclim_download(p, in, sel, out, b.bio, out_pitch);
}
int mcf_runbioclim1(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, mcf_bioclim_out* out) {
    return run_bioclim(in, opt, sel, out, 0);
}
int mcf_runbioclim3(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, mcf_bioclim_out* out) {
    return run_bioclim(in, opt, sel, out, 0, 1);
}
int mcf_runbioclim4(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, mcf_bioclim_out* out) {
    return run_bioclim(in, opt, sel, out, 1, 1);
}
int mcf_runbioclim2(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, mcf_bioclim_out* out) {
    return run_bioclim(in, opt, sel, out, 1);
}
int mcf_bioclim_last_chunks(void) { return g_bioclim_chunks; }

// ---- period summaries (include/mcf.h "period summaries"; kernels: mcf_summary.hip) -----------------------------------------
// everything of a summary that can be judged without a device; `requested`: the plan's var_slot (null: any variable)
static int check_summary_spec(const mcf_summary_spec* s, int64_t ndays, const int* requested) {
    if (!s) return fail(MCF_ERR_ARG, "null mcf_summary_spec");
    if (s->nperiods < 1) return fail(MCF_ERR_ARG, "summary: nperiods must be at least 1");
    if (ndays > 0 && !s->period_of_day) return fail(MCF_ERR_ARG, "summary: null period_of_day");
    for (int64_t d = 0; d < ndays; ++d)
        if (s->period_of_day[d] < -1 || s->period_of_day[d] >= s->nperiods)
            return fail(MCF_ERR_ARG, "summary: period_of_day[" + std::to_string(d) + "] = " + std::to_string(s->period_of_day[d]) +
                                         " is outside -1 .. nperiods - 1");
    int nv = 0, ns = 0;
    for (int v = 0; v < MCF_NOUT; ++v) nv += s->var[v] ? 1 : 0;
    for (int k = 0; k < MCF_NSTAT; ++k) ns += s->stat[k] ? 1 : 0;
    if (nv == 0) return fail(MCF_ERR_ARG, "summary: no variable selected");
    if (ns == 0) return fail(MCF_ERR_ARG, "summary: no statistic selected");
    for (int v = 0; v < MCF_NOUT; ++v) {
        if (!s->var[v]) continue;
        if (requested && requested[v] < 0) return fail(MCF_ERR_ARG, "summary: a selected variable was not requested in out[] at plan creation");
        if (s->stat[MCF_STAT_HOURS_ABOVE] && std::isnan(s->threshold[v]))
            return fail(MCF_ERR_ARG, "summary: HOURS_ABOVE needs a threshold for every selected variable (NaN given)");
    }
    return MCF_OK;
}
static int check_room(int64_t need, const char* what) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return MCF_OK;
    if ((double)need > 0.95 * (double)fr) {
        char m[200];
        snprintf(m, sizeof m, "%s needs %.2f GB of device memory, %.2f GB free", what, need / 1e9, fr / 1e9);
        return fail(MCF_ERR_NOMEM, m);
    }
    return MCF_OK;
}

// the sink switched on for a checked spec; extra_places: places of the state behind the selected variables' (Tz at depths
// 1 .. D - 1 of a below-ground plan)
static int summary_enable_checked(mcf_plan* p, const mcf_summary_spec* spec, int extra_places) {
    int rc;
    HIP_TRY(hipSetDevice(p->device));
    // state rows: the sum's (it carries the NA rule), then one per selected statistic that needs one
    int nrows = 1, row[MCF_NSTAT];
    uint32_t codes = 0;
    for (int k = 0; k < MCF_NSTAT; ++k) {
        row[k] = !spec->stat[k] ? -1 : k == MCF_STAT_MEAN ? 0 : nrows++;
        if (row[k] > 0 && k == MCF_STAT_MIN) codes |= 1u << (4 * row[k]);
        if (row[k] > 0 && k == MCF_STAT_MAX) codes |= 2u << (4 * row[k]);
    }
    SinkPlaces places;
    places.select(spec->var, extra_places);
    const int64_t nd = std::max(p->ndays, 1), np = spec->nperiods;
    const int64_t state_bytes = (int64_t)places.nsel * np * nrows * p->N * 8, plane_bytes = np * p->N * 8;
    if ((rc = check_room(state_bytes + plane_bytes + (3 * nd + np) * 4, "the summary state"))) return rc;
    std::vector<int32_t> pod, prev, next;
    if ((rc = mcf::period_tables(spec->period_of_day, p->ndays, (int)np, pod, prev, next))) return rc;
    int32_t** tabs[3] = {&p->d_sum_pod, &p->d_sum_prev, &p->d_sum_next};
    const std::vector<int32_t>* host[3] = {&pod, &prev, &next};
    for (int i = 0; i < 3; ++i) {
        if ((rc = p->dev.make(tabs[i], nd))) return rc;
        HIP_TRY(hipMemcpy(*tabs[i], host[i]->data(), (size_t)nd * 4, hipMemcpyHostToDevice));
    }
    if ((rc = p->dev.make(&p->d_sum_days, np))) return rc;
    if ((rc = p->dev.make(&p->d_sum_plane, plane_bytes / 8))) return rc;
    double* state = nullptr;      // (the plan gets it last: d_sum_state says that the summary is on)
    if ((rc = p->dev.make(&state, state_bytes / 8))) return rc;
    p->sum_nperiods = (int)np; p->sum_nrows = nrows; p->sum_places = places; p->sum_init_codes = codes;
    for (int k = 0; k < MCF_NSTAT; ++k) p->sum_row[k] = row[k];
    for (int v = 0; v < MCF_NOUT; ++v) p->sum_thr[v] = spec->var[v] && spec->stat[MCF_STAT_HOURS_ABOVE] ? spec->threshold[v] : 0.0;
    p->sum_pod = std::move(pod);
    p->d_sum_state = state;
    return mcf_plan_summary_reset(p);
}

int mcf_plan_summary_enable(mcf_plan* p, const mcf_summary_spec* spec) {
    if (!p || !spec) return fail(MCF_ERR_ARG, "null argument");
    if (p->bg_stream) return fail(MCF_ERR_ARG, "period summaries are not available on a streamed plan");
    if (p->bg || p->opt.reqhgt < 0.0 || !p->tiled) return fail(MCF_ERR_ARG, "period summaries need reqhgt >= 0 (the tiled ring)");
    if (p->d_sum_state) return fail(MCF_ERR_STATE, "period summaries are already enabled on this plan");
    int rc = check_summary_spec(spec, p->ndays, p->var_slot);
    if (rc) return rc;
    return summary_enable_checked(p, spec, 0);
}

int mcf_plan_summary_enable_below(mcf_plan* p, const mcf_summary_spec* spec) {
    const char* who = "mcf_plan_summary_enable_below";
    if (!p || !spec) return fail(MCF_ERR_ARG, std::string(who) + ": null argument");
    if (!p->bg_stream || !p->tiled)
        return fail(MCF_ERR_STATE, std::string(who) + " needs a streamed plan (mcf_plan_create_streamed) with reqhgt < 0");
    if (p->d_sum_state) return fail(MCF_ERR_STATE, "period summaries are already enabled on this plan");
    int rc = mcf::check_below_vars(who, spec->var, "can be summarised");
    if (rc) return rc;
    if ((rc = check_summary_spec(spec, p->ndays, p->var_slot))) return rc;
    const int D = std::max<int>(1, (int)p->depths.size());
    if ((rc = summary_enable_checked(p, spec, spec->var[MCF_OUT_TZ] ? D - 1 : 0))) return rc;
    p->sum_places.below = true;
    return MCF_OK;
}

int mcf_plan_summary_reset(mcf_plan* p) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    if (!p->d_sum_state) return fail(MCF_ERR_STATE, "the plan has no summary: mcf_plan_summary_enable first");
    HIP_TRY(hipSetDevice(p->device));
    mcf::launch_summary_init(p->d_sum_state, (int64_t)p->sum_places.nsel * p->sum_nperiods * p->sum_nrows * p->N, p->N, p->sum_nrows,
                             p->sum_init_codes, p->stream);
    HIP_TRY(hipGetLastError());
    p->sum_days.assign((size_t)p->sum_nperiods, 0);
    p->sum_next_day = 0;
    return MCF_OK;
}

int mcf_plan_summary_accumulate(mcf_plan* p, int32_t slot, int32_t slot_day0, int32_t day0, int32_t ndays) {
    if (!p) return fail(MCF_ERR_ARG, "null plan");
    if (!p->d_sum_state) return fail(MCF_ERR_STATE, "the plan has no summary: mcf_plan_summary_enable first");
    if (const int rc = mcf::check_fold_range("", p->ring_slots, p->ring_days, p->ndays, slot, slot_day0, day0, ndays)) return rc;
    if (day0 < p->sum_next_day)
        return fail(MCF_ERR_STATE, "summary: days arrive in ascending order, each at most once (day " + std::to_string(day0) +
                                       " after day " + std::to_string(p->sum_next_day - 1) + ")");
    HIP_TRY(hipSetDevice(p->device));
    mcf::SummaryAccArgs a{};
    a.N = p->N; a.ntiles = p->ntiles; a.cpb = p->cpb;
    a.nperiods = p->sum_nperiods; a.nrows = p->sum_nrows;
    for (int k = 0; k < MCF_NSTAT; ++k) a.row[k] = p->sum_row[k];
    a.period_of_day = p->d_sum_pod; a.prev_same = p->d_sum_prev; a.next_same = p->d_sum_next;
    a.day0 = day0; a.ndays = ndays; a.slot_day0 = slot_day0;
    for_sink_sources(p, p->sum_places, slot, [&](const SinkSource& s) {
        a.ring = s.view.base; a.tile_stride = s.view.tile_stride; a.day_stride = s.view.day_stride; a.var_stride = s.var_stride;
        a.nsel = s.nsel;
        for (int i = 0; i < s.nsel; ++i) { a.slab[i] = s.slab[i]; a.threshold[i] = p->sum_thr[s.var[i]]; }
        a.state = p->d_sum_state + (int64_t)s.place * p->sum_nperiods * p->sum_nrows * p->N;
        mcf::launch_summary_acc(a, p->stream);
    });
    HIP_TRY(hipGetLastError());
    for (int d = day0; d < day0 + ndays; ++d)
        if (p->sum_pod[(size_t)d] >= 0) p->sum_days[(size_t)p->sum_pod[(size_t)d]] += 1;
    p->sum_next_day = day0 + ndays;
    return MCF_OK;
}

// one statistic plane [rows, cols, nperiods] into the caller's array (row_pitch > rows: a row block's rows of taller planes)
static int summary_fetch_pitched(mcf_plan* p, int32_t var, int32_t stat, double* host_dst, int64_t row_pitch, int32_t depth = 0) {
    if (!p || !host_dst) return fail(MCF_ERR_ARG, "null argument");
    if (!p->d_sum_state) return fail(MCF_ERR_STATE, "the plan has no summary: mcf_plan_summary_enable first");
    if (var < 0 || var >= MCF_NOUT || stat < 0 || stat >= MCF_NSTAT) return fail(MCF_ERR_ARG, "bad variable / statistic");
    if (!p->sum_places.sel1[var]) return fail(MCF_ERR_ARG, "variable was not selected in mcf_plan_summary_enable");
    if (p->sum_row[stat] < 0) return fail(MCF_ERR_ARG, "statistic was not selected in mcf_plan_summary_enable");
    const int place = p->sum_places.place("mcf_plan_summary_fetch_depth", var, depth);
    if (place < 0) return MCF_ERR_ARG;
    if (row_pitch == 0) row_pitch = p->rows;
    if (row_pitch < p->rows) return fail(MCF_ERR_ARG, "row_pitch smaller than rows");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(p->d_sum_days, p->sum_days.data(), (size_t)p->sum_nperiods * 4, hipMemcpyHostToDevice, p->stream));
    mcf::SummaryFinArgs f{};
    f.state = p->d_sum_state + (int64_t)place * p->sum_nperiods * p->sum_nrows * p->N;
    f.N = p->N; f.nperiods = p->sum_nperiods; f.nrows = p->sum_nrows;
    f.stat = stat; f.row = p->sum_row[stat];
    f.days = p->d_sum_days; f.out = p->d_sum_plane;
    mcf::launch_summary_fin(f, p->stream);
    HIP_TRY(hipGetLastError());
    return to_host(p, host_dst, p->d_sum_plane, (size_t)(p->N * p->sum_nperiods) * 8, row_pitch);
}
int mcf_plan_summary_fetch(mcf_plan* p, int32_t var, int32_t stat, double* host_dst) {
    return summary_fetch_pitched(p, var, stat, host_dst, 0);
}
int mcf_plan_summary_fetch_depth(mcf_plan* p, int32_t depth, int32_t var, int32_t stat, double* host_dst) {
    if (p && !p->sum_places.below) return fail(MCF_ERR_STATE, "mcf_plan_summary_fetch_depth: the plan has no below-ground summary (mcf_plan_summary_enable_below)");
    return summary_fetch_pitched(p, var, stat, host_dst, 0, depth);
}

int mcf_plan_summary_days(mcf_plan* p, int32_t* days) {
    if (!p || !days) return fail(MCF_ERR_ARG, "null argument");
    if (!p->d_sum_state) return fail(MCF_ERR_STATE, "the plan has no summary: mcf_plan_summary_enable first");
    for (int k = 0; k < p->sum_nperiods; ++k) days[k] = p->sum_days[(size_t)k];
    return MCF_OK;
}

}  // extern "C"
namespace mcf {   // mcf_snowrun.hip: the snow run's summaries
// a spec judged without a plan; out_mask: the variables a run was created with (null: any)
int summary_spec_check(const mcf_summary_spec* s, int64_t ndays, const int32_t* out_mask) {
    int requested[MCF_NOUT];
    for (int v = 0; v < MCF_NOUT; ++v) requested[v] = !out_mask || out_mask[v] ? 0 : -1;
    return check_summary_spec(s, ndays, requested);
}
int plan_summary_fetch_pitched(mcf_plan* p, int32_t var, int32_t stat, double* host_dst, int64_t row_pitch) {
    return summary_fetch_pitched(p, var, stat, host_dst, row_pitch);
}
// Another table for an enabled summary (a second year on one snow-run handle: the day classes, and with them the days that are
// never counted, belong to the year), and the state of the enable: nothing folded.
int plan_summary_retable(mcf_plan* p, const int32_t* period_of_day) {
    if (!p || !period_of_day) return fail(MCF_ERR_ARG, "null argument");
    if (!p->d_sum_state) return fail(MCF_ERR_STATE, "the plan has no summary: mcf_plan_summary_enable first");
    const int64_t nd = std::max(p->ndays, 1);
    std::vector<int32_t> pod, prev, next;
    if (const int rc = period_tables(period_of_day, p->ndays, p->sum_nperiods, pod, prev, next)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));                     // (a fold of the year before may still read the tables)
    HIP_TRY(hipMemcpy(p->d_sum_pod, pod.data(), (size_t)nd * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p->d_sum_prev, prev.data(), (size_t)nd * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p->d_sum_next, next.data(), (size_t)nd * 4, hipMemcpyHostToDevice));
    p->sum_pod = std::move(pod);
    return mcf_plan_summary_reset(p);
}
}  // namespace mcf
extern "C" {

// The chunked run of the tiled-ring sinks (period summaries, the series sink) for an entry that has judged its arguments: a plan
// of the sink's variables whose ring holds `chunk_days` days (0: what the ring budget gives), the sink's three steps on it.
// twi_mean: a row block of a taller raster (the `_multi` entries), as for run_bioclim
static int run_sink(const mcf_grid_inputs* in, const mcf_options* opt_in, int32_t chunk_days, const RunSink& sink, const double* twi_mean) {
    mcf_options opt = *opt_in;
    int nsel = 0, rc;
    for (int v = 0; v < MCF_NOUT; ++v) nsel += (opt.out[v] = sink.out[v]);
    if ((rc = ensure_device(opt.device))) return rc;
    const int ndays = (int)(in->tsteps / 24);
    int chunk = chunk_days;
    // the ring of the selected variables (and, fine array forcing, the forcing ring's 15 series) from the byte budget
    if (chunk == 0)
        chunk = ring_budget_days("MCF_SUMMARY_RING_GB", nsel + (in->array_forcing == 1 ? 15 : 0), in->rows * in->cols,
                                 opt.cells_per_block ? opt.cells_per_block : 21);
    chunk = std::max(1, std::min(chunk, std::max(ndays, 1)));
    mcf_plan* p = nullptr;
    if ((rc = plan_create(in, &opt, chunk, 1, false, &p, nullptr))) return rc;
    PlanHolder holder(p);
    if (twi_mean && (rc = mcf_plan_set_twi_mean(p, *twi_mean))) return rc;
    return run_sink_chunks(p, in, ndays, chunk, sink);
}

// twi_mean / out_pitch: a row block of a taller raster (mcf_runmicro_summary_multi)
static int run_summary(const mcf_grid_inputs* in, const mcf_options* opt_in, const mcf_summary_spec* spec, int32_t chunk_days,
                       mcf_summary_out* out, const double* twi_mean = nullptr, int64_t out_pitch = 0) {
    if (!spec || !out) return fail(MCF_ERR_ARG, "null summary argument");
    int rc = check_inputs(in, opt_in);
    if (rc) return rc;
    if (opt_in->reqhgt < 0.0) return fail(MCF_ERR_ARG, "period summaries need reqhgt >= 0 (the tiled ring)");
    if (chunk_days < 0) return fail(MCF_ERR_ARG, "summary: negative chunk_days");
    if ((rc = check_summary_spec(spec, in->tsteps / 24, nullptr))) return rc;
    if ((rc = mcf::check_summary_out(spec, out))) return rc;
    RunSink sink;
    for (int v = 0; v < MCF_NOUT; ++v) sink.out[v] = spec->var[v] ? 1 : 0;
    sink.enable = [&](mcf_plan* p) { return mcf_plan_summary_enable(p, spec); };
    sink.fold = [](mcf_plan* p, int d0, int nd) { return mcf_plan_summary_accumulate(p, 0, 0, d0, nd); };
    sink.finish = [&](mcf_plan* p) -> int {
        for (int v = 0; v < MCF_NOUT; ++v)
            for (int k = 0; k < MCF_NSTAT; ++k)
                if (spec->var[v] && spec->stat[k])
                    if (const int rcf = summary_fetch_pitched(p, v, k, out->val[v][k], out_pitch)) return rcf;
        return out->days ? mcf_plan_summary_days(p, out->days) : (int)MCF_OK;
    };
    return run_sink(in, opt_in, chunk_days, sink, twi_mean);
}
int mcf_runmicro_summary(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_summary_spec* spec, int32_t chunk_days,
                         mcf_summary_out* out) {
    return run_summary(in, opt, spec, chunk_days, out);
}

// ---- series sink (include/mcf.h "series sink"; kernels: mcf_series.hip) ---------------------------------------
// the zones of a spec, judged without a device: the count, the labels, a statistic
static int check_series_zones(const std::string& who, const int32_t* zone, int64_t N, int32_t nzones, const int32_t* zstat) {
    if (nzones < 0 || nzones > MCF_MAX_ZONES)
        return fail(MCF_ERR_ARG, who + ": nzones = " + std::to_string(nzones) + " is outside 0 .. " + std::to_string(MCF_MAX_ZONES));
    if (nzones == 0) return MCF_OK;
    if (!zone) return fail(MCF_ERR_ARG, who + ": null zone map");
    int ns = 0;
    for (int k = 0; k < MCF_NZSTAT; ++k) ns += zstat[k] ? 1 : 0;
    if (ns == 0) return fail(MCF_ERR_ARG, who + ": no statistic selected");
    for (int64_t c = 0; c < N; ++c)
        if (zone[c] < -1 || zone[c] >= nzones)
            return fail(MCF_ERR_ARG, who + ": zone[" + std::to_string(c) + "] = " + std::to_string(zone[c]) + " is outside -1 .. nzones - 1");
    return MCF_OK;
}
// everything of a series spec that can be judged without a device; `requested`: the plan's var_slot (null: any variable)
static int check_series_spec(const std::string& who, const mcf_series_spec* s, int64_t rows, int64_t cols, const int* requested) {
    if (!s) return fail(MCF_ERR_ARG, who + ": null mcf_series_spec");
    const int64_t N = rows * cols;
    if (N > ((int64_t)1 << 26)) return fail(MCF_ERR_ARG, who + ": more than 2^26 cells (the fixed-point sum's range)");
    int nv = 0;
    for (int v = 0; v < MCF_NOUT; ++v) nv += s->var[v] ? 1 : 0;
    if (nv == 0) return fail(MCF_ERR_ARG, who + ": no variable selected");
    if (s->npoints < 0) return fail(MCF_ERR_ARG, who + ": negative npoints");
    if (s->npoints == 0 && s->nzones == 0) return fail(MCF_ERR_ARG, who + ": neither points nor zones selected");
    for (int v = 0; v < MCF_NOUT; ++v)
        if (s->var[v] && requested && requested[v] < 0)
            return fail(MCF_ERR_ARG, who + ": a selected variable was not requested in out[] at plan creation");
    if (const int rc = check_series_zones(who, s->zone, N, s->nzones, s->zstat)) return rc;
    if (s->npoints > 0 && !s->cells) return fail(MCF_ERR_ARG, who + ": null cells");
    for (int64_t i = 0; i < s->npoints; ++i)
        if (s->cells[i] < 0 || s->cells[i] >= N)
            return fail(MCF_ERR_ARG, who + ": cells[" + std::to_string(i) + "] = " + std::to_string(s->cells[i]) + " is a cell index outside the raster");
    return MCF_OK;
}
// persistent workgroups per selected variable: one per compute unit (the kernel's LDS lets one reside on each)
static int series_workgroups(int device) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n < 1) n = 256;
    return n;
}

// the enable behind its checks; extra: places behind the selected variables' (below ground: Tz at depths 1 .. D - 1)
static int series_enable_checked(const std::string& who, mcf_plan* p, const mcf_series_spec* spec, int extra) {
    if (p->ser_on) return fail(MCF_ERR_STATE, who + ": the series sink is already enabled on this plan");
    int rc = check_series_spec(who, spec, p->rows, p->cols, p->var_slot);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    SinkPlaces places;
    places.select(spec->var, extra);
    const int nsel = places.nsel;
    const int64_t np = spec->npoints, nz = spec->nzones, steps = (int64_t)p->ndays * 24, T = std::max<int64_t>(p->tsteps, 1);
    const int64_t point_bytes = nsel * np * T * 8, state_bytes = nsel * mcf::kSeriesRows * nz * steps * 8;
    if ((rc = check_room(point_bytes, "mcf_plan_series_enable: the point buffer"))) return rc;
    if ((rc = check_room(point_bytes + state_bytes + nz * T * 8 + p->N * 4, "mcf_plan_series_enable: the zone state"))) return rc;
    if (np > 0) {
        if ((rc = p->dev.make(&p->d_ser_cells, np))) return rc;
        HIP_TRY(hipMemcpy(p->d_ser_cells, spec->cells, (size_t)np * 8, hipMemcpyHostToDevice));
        if ((rc = p->dev.make(&p->d_ser_points, nsel * np * T))) return rc;
    }
    if (nz > 0) {
        if ((rc = p->dev.make(&p->d_ser_zone, p->N))) return rc;
        HIP_TRY(hipMemcpy(p->d_ser_zone, spec->zone, (size_t)p->N * 4, hipMemcpyHostToDevice));
        if ((rc = p->dev.make(&p->d_ser_state, state_bytes / 8))) return rc;
        if ((rc = p->dev.make(&p->d_ser_plane, nz * T))) return rc;
        if ((rc = p->dev.make(&p->d_ser_done, std::max(p->ndays, 1)))) return rc;
    }
    p->ser_npoints = np; p->ser_nzones = (int)nz; p->ser_places = places;
    p->ser_workgroups = series_workgroups(p->device);
    for (int k = 0; k < MCF_NZSTAT; ++k) p->ser_zstat[k] = nz > 0 && spec->zstat[k] ? 1 : 0;
    p->ser_on = true;
    return mcf_plan_series_reset(p);
}

int mcf_plan_series_enable(mcf_plan* p, const mcf_series_spec* spec) {
    const std::string who = "mcf_plan_series_enable";
    if (!p || !spec) return fail(MCF_ERR_ARG, who + ": null argument");
    if (p->bg_stream) return fail(MCF_ERR_ARG, who + ": the series sink is not available on a streamed plan");
    if (p->bg || p->opt.reqhgt < 0.0 || !p->tiled) return fail(MCF_ERR_ARG, who + ": the series sink needs reqhgt >= 0 (the tiled ring)");
    return series_enable_checked(who, p, spec, 0);
}

int mcf_plan_series_enable_below(mcf_plan* p, const mcf_series_spec* spec) {
    const std::string who = "mcf_plan_series_enable_below";
    if (!p || !spec) return fail(MCF_ERR_ARG, who + ": null argument");
    if (!p->bg_stream || !p->tiled) return fail(MCF_ERR_STATE, who + " needs a streamed plan (mcf_plan_create_streamed) with reqhgt < 0");
    if (const int rc = mcf::check_below_vars(who, spec->var, "have a series")) return rc;
    const int D = std::max<int>(1, (int)p->depths.size());
    if (const int rc = series_enable_checked(who, p, spec, spec->var[MCF_OUT_TZ] ? D - 1 : 0)) return rc;
    p->ser_places.below = true;
    return MCF_OK;
}

int mcf_plan_series_reset(mcf_plan* p) {
    if (!p) return fail(MCF_ERR_ARG, "mcf_plan_series_reset: null plan");
    if (!p->ser_on) return fail(MCF_ERR_STATE, "the plan has no series sink: mcf_plan_series_enable first");
    HIP_TRY(hipSetDevice(p->device));
    if (p->d_ser_points)
        mcf::launch_fill(p->d_ser_points, p->ser_places.nsel * p->ser_npoints * std::max<int64_t>(p->tsteps, 1), mcf::na_real_host(), p->stream);
    if (p->d_ser_state) mcf::launch_series_init(p->d_ser_state, p->ser_places.nsel, p->ser_nzones, (int64_t)p->ndays * 24, p->stream);
    HIP_TRY(hipGetLastError());
    p->ser_done.assign((size_t)std::max(p->ndays, 1), 0);
    return MCF_OK;
}

int mcf_plan_series_accumulate(mcf_plan* p, int32_t slot, int32_t slot_day0, int32_t day0, int32_t ndays) {
    if (!p) return fail(MCF_ERR_ARG, "mcf_plan_series_accumulate: null plan");
    if (!p->ser_on) return fail(MCF_ERR_STATE, "the plan has no series sink: mcf_plan_series_enable first");
    if (const int rc = mcf::check_fold_range("mcf_plan_series_accumulate", p->ring_slots, p->ring_days, p->ndays, slot, slot_day0, day0, ndays))
        return rc;
    for (int d = day0; d < day0 + ndays; ++d)
        if (p->ser_done[(size_t)d])
            return fail(MCF_ERR_STATE, "mcf_plan_series_accumulate: day " + std::to_string(d) + " has been folded already (each day at most once)");
    HIP_TRY(hipSetDevice(p->device));
    if (p->ser_npoints > 0) {
        mcf::SeriesPointsArgs a{};
        a.step0 = (int64_t)slot_day0 * 24; a.nsteps = (int64_t)ndays * 24;
        a.cells = p->d_ser_cells; a.ncells = p->ser_npoints;
        a.dst_steps = std::max<int64_t>(p->tsteps, 1); a.dst_step0 = (int64_t)day0 * 24;
        for_sink_sources(p, p->ser_places, slot, [&](const SinkSource& s) {
            for (int i = 0; i < s.nsel; ++i) {
                a.src[i] = s.view;
                a.src[i].base += s.slab[i] * s.var_stride;
            }
            a.nsel = s.nsel;
            a.dst = p->d_ser_points + (int64_t)s.place * p->ser_npoints * a.dst_steps;
            mcf::launch_series_points(a, p->stream);
        });
    }
    if (p->ser_nzones > 0) {
        mcf::SeriesZonesArgs a{};
        a.N = p->N; a.ntiles = p->ntiles; a.cpb = p->cpb;
        a.zone = p->d_ser_zone; a.nzones = p->ser_nzones;
        a.steps = (int64_t)p->ndays * 24;
        a.day0 = day0; a.ndays = ndays; a.slot_day0 = slot_day0;
        for_sink_sources(p, p->ser_places, slot, [&](const SinkSource& s) {      // (one kernel serves: only the view changes)
            a.ring = s.view.base; a.tile_stride = s.view.tile_stride; a.day_stride = s.view.day_stride; a.var_stride = s.var_stride;
            a.nsel = s.nsel;
            for (int i = 0; i < s.nsel; ++i) a.slab[i] = s.slab[i];
            a.state = p->d_ser_state + (int64_t)s.place * mcf::kSeriesRows * p->ser_nzones * a.steps;
            mcf::launch_series_zones(a, p->ser_workgroups, p->stream);
        });
    }
    HIP_TRY(hipGetLastError());
    for (int d = day0; d < day0 + ndays; ++d) p->ser_done[(size_t)d] = 1;
    return MCF_OK;
}

// the place of (variable, depth) in the point buffer and the zone state; -1 with the error set
static int series_place(const std::string& who, mcf_plan* p, int32_t var, int32_t depth) {
    if (var < 0 || var >= MCF_NOUT || !p->ser_places.sel1[var])
        return fail(MCF_ERR_ARG, who + ": variable was not selected in mcf_plan_series_enable"), -1;
    return p->ser_places.place(who, var, depth);
}
static int series_fetch_points(const std::string& who, mcf_plan* p, int32_t depth, int32_t var, double* dst) {
    if (!p || !dst) return fail(MCF_ERR_ARG, who + ": null argument");
    if (!p->ser_on) return fail(MCF_ERR_STATE, "the plan has no series sink: mcf_plan_series_enable first");
    const int place = series_place(who, p, var, depth);
    if (place < 0) return MCF_ERR_ARG;
    if (p->ser_npoints == 0) return fail(MCF_ERR_ARG, who + ": no points were selected in mcf_plan_series_enable");
    HIP_TRY(hipSetDevice(p->device));
    const int64_t n = p->ser_npoints * std::max<int64_t>(p->tsteps, 1);
    HIP_TRY(p->tohost.dense(dst, p->d_ser_points + (int64_t)place * n, (size_t)n * 8, p->stream));
    return MCF_OK;
}
int mcf_plan_series_fetch_points(mcf_plan* p, int32_t var, double* dst) {
    return series_fetch_points("mcf_plan_series_fetch_points", p, 0, var, dst);
}
int mcf_plan_series_fetch_points_depth(mcf_plan* p, int32_t depth, int32_t var, double* dst) {
    if (p && !p->ser_places.below)
        return fail(MCF_ERR_STATE, "mcf_plan_series_fetch_points_depth: the plan has no below-ground series sink (mcf_plan_series_enable_below)");
    return series_fetch_points("mcf_plan_series_fetch_points_depth", p, depth, var, dst);
}

static int series_fetch_zones(const std::string& who, mcf_plan* p, int32_t depth, int32_t var, int32_t zstat, double* dst) {
    if (!p || !dst) return fail(MCF_ERR_ARG, who + ": null argument");
    if (!p->ser_on) return fail(MCF_ERR_STATE, "the plan has no series sink: mcf_plan_series_enable first");
    const int place = series_place(who, p, var, depth);
    if (place < 0) return MCF_ERR_ARG;
    if (zstat < 0 || zstat >= MCF_NZSTAT || !p->ser_zstat[zstat])
        return fail(MCF_ERR_ARG, who + ": statistic was not selected in mcf_plan_series_enable");
    HIP_TRY(hipSetDevice(p->device));
    const int64_t steps = (int64_t)p->ndays * 24, T = std::max<int64_t>(p->tsteps, 1);
    HIP_TRY(hipMemcpyAsync(p->d_ser_done, p->ser_done.data(), (size_t)std::max(p->ndays, 1) * 4, hipMemcpyHostToDevice, p->stream));
    mcf::launch_series_fin(p->d_ser_state + (int64_t)place * mcf::kSeriesRows * p->ser_nzones * steps, p->ser_nzones,
                           steps, T, p->d_ser_done, zstat, p->d_ser_plane, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(p->tohost.dense(dst, p->d_ser_plane, (size_t)(T * p->ser_nzones) * 8, p->stream));
    return MCF_OK;
}
int mcf_plan_series_fetch_zones(mcf_plan* p, int32_t var, int32_t zstat, double* dst) {
    return series_fetch_zones("mcf_plan_series_fetch_zones", p, 0, var, zstat, dst);
}
int mcf_plan_series_fetch_zones_depth(mcf_plan* p, int32_t depth, int32_t var, int32_t zstat, double* dst) {
    if (p && !p->ser_places.below)
        return fail(MCF_ERR_STATE, "mcf_plan_series_fetch_zones_depth: the plan has no below-ground series sink (mcf_plan_series_enable_below)");
    return series_fetch_zones("mcf_plan_series_fetch_zones_depth", p, depth, var, zstat, dst);
}

// the combination of row blocks and the finish, on the host (include/mcf.h "Row blocks"; mcf_series_host.hpp)
int mcf_series_state_merge(int64_t* into, const int64_t* from, int32_t nzones, int64_t steps) {
    if (!into || !from || nzones < 0 || steps < 0) return fail(MCF_ERR_ARG, "mcf_series_state_merge: null or negative argument");
    mcf::series_state_merge(into, from, nzones, steps);
    return MCF_OK;
}
int mcf_series_state_finish(const int64_t* state, int32_t nzones, int64_t steps, int64_t nsteps, const int32_t* day_done,
                            int32_t zstat, double* out) {
    if (!state || !out || nzones < 0 || steps < 0 || nsteps < 0 || steps % 24) return fail(MCF_ERR_ARG, "mcf_series_state_finish: bad argument");
    if (zstat < 0 || zstat >= MCF_NZSTAT) return fail(MCF_ERR_ARG, "mcf_series_state_finish: statistic out of range");
    mcf::series_state_finish(state, nzones, steps, nsteps, day_done, zstat, out);
    return MCF_OK;
}

}  // extern "C"
namespace mcf {   // mcf_snowrun.hip: the snow run's series over row blocks
// what mcf_series_spec can be refused for without a plan; out_mask: the variables a run was created with (null: any)
int series_spec_check(const std::string& who, const mcf_series_spec* s, int64_t rows, int64_t cols, const int32_t* out_mask) {
    int requested[MCF_NOUT];
    for (int v = 0; v < MCF_NOUT; ++v) requested[v] = !out_mask || out_mask[v] ? 0 : -1;
    return check_series_spec(who, s, rows, cols, requested);
}
// a plan's raw zone state of one variable, [4][nzones][whole days x 24] of int64, and its folded days [days] (either may be
// null), behind everything on the plan's stream
int plan_series_state(mcf_plan* p, int32_t var, int64_t* host_state, int32_t* day_done) {
    if (!p || !p->ser_on || var < 0 || var >= MCF_NOUT || !p->ser_places.sel1[var] || p->ser_nzones == 0)
        return fail(MCF_ERR_STATE, "plan: no zone state of this variable");
    HIP_TRY(hipSetDevice(p->device));
    const int64_t n = (int64_t)kSeriesRows * p->ser_nzones * p->ndays * 24;
    if (host_state && n > 0)
        HIP_TRY(hipMemcpyAsync(host_state, p->d_ser_state + (int64_t)(p->ser_places.sel1[var] - 1) * n, (size_t)n * 8, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (day_done) std::copy(p->ser_done.begin(), p->ser_done.begin() + p->ndays, day_done);
    return MCF_OK;
}
}  // namespace mcf
extern "C" {

// a row block's results on their way to the combination (mcf_runmicro_series_multi): per selected variable the points'
// [tsteps, block's points] and the raw zone state; the folded days
struct SeriesRaw {
    std::vector<double> points[MCF_NOUT];
    std::vector<int64_t> state[MCF_NOUT];
    std::vector<int32_t> done;
};
// twi_mean / raw: a row block of a taller raster (mcf_runmicro_series_multi) — the results stay raw, `out` is not read
static int run_series(const std::string& who, const mcf_grid_inputs* in, const mcf_options* opt_in, const mcf_series_spec* spec,
                      int32_t chunk_days, mcf_series_out* out, const double* twi_mean = nullptr, SeriesRaw* raw = nullptr) {
    if (!spec || (!out && !raw)) return fail(MCF_ERR_ARG, who + ": null argument");
    int rc = check_inputs(in, opt_in);
    if (rc) return rc;
    if (opt_in->reqhgt < 0.0) return fail(MCF_ERR_ARG, who + ": the series sink needs reqhgt >= 0 (the tiled ring)");
    if (chunk_days < 0) return fail(MCF_ERR_ARG, who + ": negative chunk_days");
    if ((rc = check_series_spec(who, spec, in->rows, in->cols, nullptr))) return rc;
    if (!raw && (rc = mcf::check_series_out(who, spec, out))) return rc;
    RunSink sink;
    for (int v = 0; v < MCF_NOUT; ++v) sink.out[v] = spec->var[v] ? 1 : 0;
    sink.enable = [&](mcf_plan* p) { return mcf_plan_series_enable(p, spec); };
    sink.fold = [](mcf_plan* p, int d0, int nd) { return mcf_plan_series_accumulate(p, 0, 0, d0, nd); };
    sink.finish = [&](mcf_plan* p) -> int {
        const int ndays = (int)(in->tsteps / 24);
        const int64_t T = std::max<int64_t>(in->tsteps, 1);
        int rcf;
        for (int v = 0; v < MCF_NOUT; ++v) {
            if (!spec->var[v]) continue;
            if (raw) {
                if (spec->npoints > 0) {
                    raw->points[v].resize((size_t)(T * spec->npoints));
                    if ((rcf = mcf_plan_series_fetch_points(p, v, raw->points[v].data()))) return rcf;
                }
                if (spec->nzones > 0) {
                    raw->state[v].resize((size_t)((int64_t)mcf::kSeriesRows * spec->nzones * ndays * 24));
                    raw->done.assign((size_t)std::max(ndays, 1), 0);
                    if ((rcf = mcf::plan_series_state(p, v, raw->state[v].data(), raw->done.data()))) return rcf;
                }
                continue;
            }
            if (spec->npoints > 0 && (rcf = mcf_plan_series_fetch_points(p, v, out->points[v]))) return rcf;
            for (int k = 0; k < MCF_NZSTAT; ++k)
                if (spec->nzones > 0 && spec->zstat[k] && (rcf = mcf_plan_series_fetch_zones(p, v, k, out->zones[v][k]))) return rcf;
        }
        return MCF_OK;
    };
    return run_sink(in, opt_in, chunk_days, sink, twi_mean);
}
int mcf_runmicro_series(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_series_spec* spec, int32_t chunk_days,
                        mcf_series_out* out) {
    return run_series("mcf_runmicro_series", in, opt, spec, chunk_days, out);
}

// MCF_ZONAL_CPB = 0: a column-major x[rows, cols, nsteps] IS step-major planes, so it goes up in pieces of whole days as it lies
// and k_series_planes folds it (the last piece may end in a day shorter than 24 steps)
static int zonal_series_planes(const double* x, int64_t N, int64_t nsteps, const int32_t* zone, int32_t nzones, const int32_t* zstat,
                               int32_t device, double* const* out) {
    int rc;
    const int64_t ndays = (nsteps + 23) / 24, steps = ndays * 24;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(ndays, (int64_t)(1e9 / (8.0 * 24.0 * (double)N))));
    mcf::DevOwner own;
    double *d_lin = nullptr, *d_plane = nullptr;
    int32_t* d_zone = nullptr;
    long long* d_state = nullptr;
    if ((rc = own.make(&d_lin, N * 24 * chunk))) return rc;
    if ((rc = own.make(&d_plane, nsteps * nzones))) return rc;
    if ((rc = own.make(&d_state, mcf::kSeriesRows * (int64_t)nzones * steps))) return rc;
    if ((rc = own.up(const_cast<const int32_t**>(&d_zone), zone, N, "zone"))) return rc;
    hipStream_t s = nullptr;
    mcf::launch_series_init(d_state, 1, nzones, steps, s);
    const int workgroups = series_workgroups(device);
    for (int64_t d0 = 0; d0 < ndays; d0 += chunk) {
        const int64_t nd = std::min(chunk, ndays - d0), ns = std::min(nd * 24, nsteps - d0 * 24);
        HIP_TRY(hipMemcpyAsync(d_lin, x + N * d0 * 24, (size_t)(N * ns) * 8, hipMemcpyHostToDevice, s));
        mcf::SeriesPlanesArgs a{};
        a.series[0] = d_lin; a.N = N; a.nsel = 1;
        a.zone = d_zone; a.nzones = nzones; a.steps = steps; a.nsteps = ns;
        a.day0 = (int)d0; a.ndays = (int)nd;
        a.state = d_state;
        mcf::launch_series_planes(a, workgroups, s);
        HIP_TRY(hipGetLastError());
    }
    mcf::ToHost tohost;
    for (int k = 0; k < MCF_NZSTAT; ++k) {
        if (!zstat[k]) continue;
        mcf::launch_series_fin(d_state, nzones, steps, nsteps, nullptr, k, d_plane, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(tohost.dense(out[k], d_plane, (size_t)(nsteps * nzones) * 8));
    }
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}

int mcf_zonal_series(const double* x, int64_t rows, int64_t cols, int64_t nsteps, const int32_t* zone, int32_t nzones,
                     const int32_t* zstat, int32_t device, double* const* out) {
    const std::string who = "mcf_zonal_series";
    if (!x || !zone || !zstat || !out) return fail(MCF_ERR_ARG, who + ": null argument");
    if (rows <= 0 || cols <= 0 || nsteps < 1) return fail(MCF_ERR_ARG, who + ": rows, cols and nsteps must be positive");
    const int64_t N = rows * cols;
    if (N > ((int64_t)1 << 26)) return fail(MCF_ERR_ARG, who + ": more than 2^26 cells (the fixed-point sum's range)");
    if (nzones < 1) return fail(MCF_ERR_ARG, who + ": nzones = " + std::to_string(nzones) + " is outside 1 .. " + std::to_string(MCF_MAX_ZONES));
    int rc = check_series_zones(who, zone, N, nzones, zstat);
    if (rc) return rc;
    for (int k = 0; k < MCF_NZSTAT; ++k)
        if (zstat[k] && !out[k]) return fail(MCF_ERR_ARG, who + ": a selected statistic has a null buffer");
    int cpb = 32;
    if (const char* e = getenv("MCF_ZONAL_CPB")) {
        cpb = atoi(e);
        if (!(cpb == 0 || cpb == 16 || cpb == 21 || cpb == 32 || cpb == 42))
            return fail(MCF_ERR_ARG, who + ": MCF_ZONAL_CPB must be 0, 16, 21, 32 or 42");
    }
    if ((rc = ensure_device(device))) return rc;
    if (cpb == 0) return zonal_series_planes(x, N, nsteps, zone, nzones, zstat, device, out);
    const int64_t ndays = (nsteps + 23) / 24, steps = ndays * 24, ntiles = (N + cpb - 1) / cpb, B = mcf::ring_block_doubles(cpb);
    // pieces of whole days: about 1 GB of staging (the array's steps as they lie, and their tiled copy)
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ndays, 2730), (int64_t)(1e9 / (8.0 * (24.0 * N + (double)ntiles * B)))));
    mcf::DevOwner own;
    double *d_lin = nullptr, *d_til = nullptr, *d_plane = nullptr;
    int32_t* d_zone = nullptr;
    long long* d_state = nullptr;
    if ((rc = own.make(&d_lin, N * 24 * chunk))) return rc;
    if ((rc = own.make(&d_til, ntiles * chunk * B))) return rc;
    if ((rc = own.make(&d_plane, nsteps * nzones))) return rc;
    if ((rc = own.make(&d_state, mcf::kSeriesRows * (int64_t)nzones * steps))) return rc;
    if ((rc = own.up(const_cast<const int32_t**>(&d_zone), zone, N, "zone"))) return rc;
    hipStream_t s = nullptr;
    mcf::launch_series_init(d_state, 1, nzones, steps, s);
    const int workgroups = series_workgroups(device);
    for (int64_t d0 = 0; d0 < ndays; d0 += chunk) {
        const int64_t nd = std::min(chunk, ndays - d0), ns = std::min(nd * 24, nsteps - d0 * 24);
        // the hours behind the array's last step are NaN: skipped, and never asked for
        if (ns < nd * 24) mcf::launch_fill(d_til, ntiles * chunk * B, __builtin_nan(""), s);
        HIP_TRY(hipMemcpyAsync(d_lin, x + N * d0 * 24, (size_t)(N * ns) * 8, hipMemcpyHostToDevice, s));
        mcf::RingView til{};
        til.base = d_til; til.N = N; til.tile_stride = chunk * B; til.day_stride = B; til.cpb = cpb;
        mcf::launch_tile_series(d_lin, ns, til, s);
        mcf::SeriesZonesArgs a{};
        a.ring = d_til; a.tile_stride = til.tile_stride; a.day_stride = til.day_stride; a.var_stride = 0;
        a.N = N; a.ntiles = ntiles; a.cpb = cpb; a.nsel = 1; a.slab[0] = 0;
        a.zone = d_zone; a.nzones = nzones; a.steps = steps;
        a.day0 = (int)d0; a.ndays = (int)nd; a.slot_day0 = 0;
        a.state = d_state;
        mcf::launch_series_zones(a, workgroups, s);
        HIP_TRY(hipGetLastError());
    }
    mcf::ToHost tohost;
    for (int k = 0; k < MCF_NZSTAT; ++k) {
        if (!zstat[k]) continue;
        mcf::launch_series_fin(d_state, nzones, steps, nsteps, nullptr, k, d_plane, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(tohost.dense(out[k], d_plane, (size_t)(nsteps * nzones) * 8));
    }
    HIP_TRY(hipDeviceSynchronize());
    return MCF_OK;
}

// ---- below ground at several depths from one solve (include/mcf.h mcf_runmicro_depths) ----------------------
// the bioclim sink's arguments (mcf_runbioclim_depths)
struct BioDepthsSink {
    const mcf_bioclim_sel* sel;
    mcf_bioclim_depths_out* out;
};
// what that sink can be refused for without a plan or a device
static int check_bioclim_depths(const std::string& w, const mcf_grid_inputs* in, const BioDepthsSink* bio, int32_t D) {
    const mcf_bioclim_sel* sel = bio->sel;
    if (!sel || !bio->out) return fail(MCF_ERR_ARG, w + "null argument");
    if (sel->air != 1) return fail(MCF_ERR_ARG, w + "air = 0 is not taken: tleaf does not exist below ground (air = 1: Tz)");
    if (in->array_forcing == 1)
        return fail(MCF_ERR_ARG, w + "fine array forcing is not taken (its inputs are cells x steps by themselves): mcf_runbioclim2 serves it");
    const int64_t T = in->tsteps;
    if (T < 336 || T % 24 != 0) return fail(MCF_ERR_ARG, w + "runbioclim needs >= 336 hourly steps in whole days");
    const int32_t* q[4] = {sel->wetq, sel->dryq, sel->hotq, sel->colq};
    const int32_t nq[4] = {sel->nwet, sel->ndry, sel->nhot, sel->ncol};
    for (int i = 0; i < 4; ++i) {
        if (nq[i] < 0 || (nq[i] > 0 && !q[i])) return fail(MCF_ERR_ARG, w + "bad quarter index vector");
        for (int j = 0; j < nq[i]; ++j) {
            if (q[i][j] < 0 || q[i][j] >= T) return fail(MCF_ERR_ARG, w + "quarter index outside the time series");
            if (j > 0 && q[i][j] < q[i][j - 1])
                return fail(MCF_ERR_ARG, w + "a quarter list that is not in ascending order is not taken by the streamed sink: "
                                             "mcf_runbioclim1 (the whole-series form, one depth per call) takes any order");
        }
    }
    for (int v = 0; v < MCF_NBIO; ++v) {
        if (!sel->out[v]) continue;
        if (v >= 11 && !bio->out->moist[v - 11])
            return fail(MCF_ERR_ARG, w + "requested bioclim variable bio" + std::to_string(v + 1) + " has a null buffer");
        for (int d = 0; v < 11 && d < D; ++d)
            if (!bio->out->temp[d][v])
                return fail(MCF_ERR_ARG, w + "requested bioclim variable bio" + std::to_string(v + 1) + " has a null buffer at depth " +
                                             std::to_string(d));
    }
    return MCF_OK;
}
// the sink itself on a prepared plan: the accumulate launches' arguments and the state, [D][21][N] then [8][N]
static int bioclim_depths_begin(mcf_plan* p, const mcf_bioclim_sel* sel, mcf::BioAccDepthsArgs& acc) {
    if (!p->tiled) return fail(MCF_ERR_STATE, "bioclim: the streamed sink expects the tiled ring");
    const int D = (int)p->depths.size();
    const mcf::RingView sm = ring_view(p, 0, MCF_OUT_SOILM), tz = depth_view(p, 0, 0);
    acc.soilm = sm.base; acc.tz0 = tz.base;
    acc.ring_tile_stride = tz.tile_stride; acc.ring_day_stride = tz.day_stride;
    if (D > 1) {
        const mcf::RingView x = depth_view(p, 0, 1);
        acc.tzx = x.base; acc.tzx_tile_stride = x.tile_stride; acc.tzx_day_stride = x.day_stride;
        acc.tzx_stride = (int64_t)p->ring_slots * p->ntiles * p->tg_tile_stride;
    }
    acc.N = p->N; acc.ntiles = p->ntiles; acc.cpb = p->cpb; acc.ndepths = D;
    const int32_t* q[4] = {sel->wetq, sel->dryq, sel->hotq, sel->colq};
    const int32_t nq[4] = {sel->nwet, sel->ndry, sel->nhot, sel->ncol};
    if (const int rc = upload_quarters(p, q, nq, acc.q)) return rc;
    return p->dev.make(&acc.state, ((int64_t)mcf::kBioTempRows * D + mcf::kBioMoistRows) * p->N);
}
// days [d0, d0 + nd) of slot 0, behind the run that filled them, into the state
static int bioclim_depths_fold(mcf_plan* p, const mcf_bioclim_sel* sel, mcf::BioAccDepthsArgs& acc, int d0, int nd) {
    const int32_t* q[4] = {sel->wetq, sel->dryq, sel->hotq, sel->colq};
    const int32_t nq[4] = {sel->nwet, sel->ndry, sel->nhot, sel->ncol};
    acc.day0 = d0; acc.ndays = nd;
    for (int i = 0; i < 4; ++i) {
        acc.qlo[i] = (int32_t)(std::lower_bound(q[i], q[i] + nq[i], d0 * 24) - q[i]);
        acc.qhi[i] = (int32_t)(std::lower_bound(q[i], q[i] + nq[i], (d0 + nd) * 24) - q[i]);
    }
    mcf::launch_bioclim_acc_depths(acc, p->stream);
    HIP_TRY(hipGetLastError());
    return MCF_OK;
}
// the two finishes, then a pitched download per (depth, variable)
static int bioclim_depths_finish(mcf_plan* p, const mcf_grid_inputs* in, const BioDepthsSink* bio, const mcf::BioAccDepthsArgs& acc) {
    const int64_t N = p->N;
    const int D = acc.ndepths;
    double* out = nullptr;      // [D][11][N], then [8][N]
    int rc = p->dev.make(&out, (11 * (int64_t)D + mcf::kBioMoistRows) * N);
    if (rc) return rc;
    mcf::launch_bioclim_fin_temp(acc.state, N, D, out, p->stream);
    mcf::BioFinArgs fin{};
    fin.N = N; fin.tsteps = (int)p->tsteps; fin.state = acc.state + (int64_t)mcf::kBioTempRows * D * N; fin.bio = out + 11 * (int64_t)D * N;
    fin.cellc = p->d_cellc; fin.ntiles_total = p->ntiles; fin.cpb = p->cpb; fin.daylayer = p->d_daylayer; fin.tt = p->d_tt;
    if (p->coarse) {      // as run_bioclim: the second pass taps the resident coarse soil moisture series
        fin.cforce = p->d_force;
        fin.cstride = (int64_t)p->crows * p->ccols * std::max<int64_t>(p->tsteps, 1);
        fin.crows = p->crows; fin.ccols = p->ccols;
        fin.crowpos = p->d_crowpos; fin.ccolpos = p->d_ccolpos; fin.rows = (int32_t)p->rows;
    }
    mcf::launch_bioclim_fin_moist(fin, acc.state, p->stream);
    HIP_TRY(hipGetLastError());
    const int64_t pitch = host_pitch(in);
    for (int v = 0; v < MCF_NBIO; ++v) {
        if (!bio->sel->out[v]) continue;
        if (v >= 11) {
            if ((rc = to_host(p, bio->out->moist[v - 11], fin.bio + (int64_t)(v - 11) * N, (size_t)N * 8, pitch))) return rc;
            continue;
        }
        for (int d = 0; d < D; ++d)
            if ((rc = to_host(p, bio->out->temp[d][v], out + ((int64_t)d * 11 + v) * N, (size_t)N * 8, pitch))) return rc;
    }
    return mcf_plan_sync(p);
}

// The one-call entries' driver: a streamed below-ground plan with the depth list, through day chunks of `chunk_days` days (0: what
// the free memory gives), for the entry's sink: every step of every depth, the period summaries, the bioclim variables or the series
// D = 0 (depths null): no list, the one depth of opt->reqhgt (mcf_runmicro_nc below ground); twi_mean / sharers: a row block of a
// taller raster, as for run_oneshot
static int run_depths(const char* who, const mcf_grid_inputs* in, const mcf_options* opt_in, const double* depths, int32_t D,
                      const double* tbp, int32_t chunk_days, const RunSink& sink, const double* twi_mean = nullptr, int sharers = 1) {
    const std::string w = std::string(who) + ": ";
    if (!in || !opt_in) return fail(MCF_ERR_ARG, w + "null argument");
    mcf_options opt = *opt_in;
    const bool listed = depths != nullptr || D != 0;
    int rc = listed ? check_depths(who, depths, D, tbp, opt.complete != 0, in->array_forcing != 0) : (int)MCF_OK;
    if (rc) return rc;
    if (listed) opt.reqhgt = depths[0];
    else D = 1;
    if ((rc = check_inputs(in, &opt))) return rc;
    const int64_t T = in->tsteps;
    const int ndays = (int)(T / 24);
    if (ndays < 1) return fail(MCF_ERR_ARG, w + "the series is shorter than a day");
    if (chunk_days < 0) return fail(MCF_ERR_ARG, w + "negative chunk_days");
    if (sink.check && (rc = sink.check())) return rc;
    for (int v = 0; v < MCF_NOUT; ++v) opt.out[v] = sink.out[v];
    if ((rc = ensure_device(opt.device))) return rc;
    const int nvars = 1 + opt.out[MCF_OUT_SOILM];
    const bool tail = T > (int64_t)ndays * 24;      // the steps behind the last whole day: one day more per slot
    int chunk = chunk_days;
    // (the solver's variables, the forcing ring, the chunk's Tg ring and the D - 1 depth slabs per day)
    if (chunk <= 0 && (rc = free_memory_chunk_days(in->rows * in->cols, ndays, sharers, nvars + (in->array_forcing ? 15 : 0) + 1 + (D - 1),
                                                   below_state_doubles(D, ndays) + sink.state_doubles, tail, &chunk)))
        return rc;
    chunk = std::max(1, std::min(chunk, ndays));
    mcf_plan* p = nullptr;
    if ((rc = plan_create(in, &opt, chunk + (tail ? 1 : 0), 1, true, &p, nullptr))) return rc;
    PlanHolder holder(p);
    if (twi_mean && (rc = mcf_plan_set_twi_mean(p, *twi_mean))) return rc;
    if (listed && (rc = mcf_plan_below_set_depths(p, depths, D, tbp))) return rc;
    if ((rc = mcf_plan_below_prepare(p, in))) return rc;
    return run_sink_chunks(p, in, ndays, chunk, sink);
}
// every step of every depth; the chunk size is the options' own (days_per_chunk)
int mcf_runmicro_depths(const mcf_grid_inputs* in, const mcf_options* opt, const double* depths, int32_t D, const double* tbp,
                        mcf_depth_outputs* out) {
    const std::string w = "mcf_runmicro_depths: ";
    if (!out) return fail(MCF_ERR_ARG, w + "null argument");
    RunSink sink;
    sink.out[MCF_OUT_TZ] = 1;
    sink.out[MCF_OUT_SOILM] = out->soilm ? 1 : 0;
    sink.check = [&]() -> int {
        for (int d = 0; d < D; ++d)
            if (!out->tz[d]) return fail(MCF_ERR_ARG, w + "tz[" + std::to_string(d) + "] is a null buffer");
        return MCF_OK;
    };
    sink.enable = [](mcf_plan*) { return (int)MCF_OK; };
    sink.fold = [&](mcf_plan* p, int d0, int nd) -> int {
        const int64_t T = in->tsteps, pitch = host_pitch(in), HS = pitch * in->cols;
        // ... the last chunk with the steps it left behind its days
        const int64_t steps = (int64_t)nd * 24 + (d0 + nd == (int)(T / 24) ? T % 24 : 0);
        for (int d = 0; d < D; ++d)
            if (const int rcf = mcf_plan_fetch_depth_pitched(p, 0, d, 0, steps, out->tz[d] + HS * (int64_t)d0 * 24, pitch)) return rcf;
        if (!out->soilm) return MCF_OK;
        return mcf_plan_fetch_pitched(p, 0, MCF_OUT_SOILM, 0, (int64_t)nd * 24, out->soilm + HS * (int64_t)d0 * 24, pitch);
    };
    sink.finish = [&](mcf_plan*) {
        if (out->soilm) fill_tail_na(out->soilm, in, (int)(in->tsteps / 24));
        return (int)MCF_OK;
    };
    return run_depths("mcf_runmicro_depths", in, opt, depths, D, tbp, opt ? std::max(opt->days_per_chunk, 0) : 0, sink);
}
int mcf_runmicro_depths_summary(const mcf_grid_inputs* in, const mcf_options* opt, const double* depths, int32_t D,
                                const double* tbp, const mcf_summary_spec* spec, int32_t chunk_days, mcf_depth_summary_out* out) {
    const char* who = "mcf_runmicro_depths_summary";
    if (!out || !spec) return fail(MCF_ERR_ARG, std::string(who) + ": null argument");
    RunSink sink;
    // (the depth list lives on a plan with Tz; soilm alone is summarised beside it)
    sink.out[MCF_OUT_TZ] = 1;
    sink.out[MCF_OUT_SOILM] = spec->var[MCF_OUT_SOILM] ? 1 : 0;
    sink.check = [&]() -> int {
        int rc = mcf::check_below_vars(who, spec->var, "can be summarised");
        if (!rc) rc = check_summary_spec(spec, in->tsteps / 24, nullptr);
        return rc ? rc : mcf::check_depth_summary_out(who, spec, D, out);
    };
    sink.enable = [&](mcf_plan* p) { return mcf_plan_summary_enable_below(p, spec); };
    sink.fold = [](mcf_plan* p, int d0, int nd) { return mcf_plan_summary_accumulate(p, 0, 0, d0, nd); };
    sink.finish = [&](mcf_plan* p) -> int {
        int rc;
        for (int k = 0; k < MCF_NSTAT; ++k) {
            if (!spec->stat[k]) continue;
            for (int d = 0; spec->var[MCF_OUT_TZ] && d < D; ++d)
                if ((rc = summary_fetch_pitched(p, MCF_OUT_TZ, k, out->tz[d][k], 0, d))) return rc;
            if (spec->var[MCF_OUT_SOILM] && (rc = summary_fetch_pitched(p, MCF_OUT_SOILM, k, out->soilm[k], 0))) return rc;
        }
        return out->days ? mcf_plan_summary_days(p, out->days) : (int)MCF_OK;
    };
    return run_depths(who, in, opt, depths, D, tbp, chunk_days, sink);
}

int mcf_runmicro_depths_series(const mcf_grid_inputs* in, const mcf_options* opt, const double* depths, int32_t D,
                               const double* tbp, const mcf_series_spec* spec, int32_t chunk_days, mcf_depth_series_out* out) {
    const std::string who = "mcf_runmicro_depths_series";
    if (!spec) return fail(MCF_ERR_ARG, who + ": null mcf_series_spec");
    if (!out || !in) return fail(MCF_ERR_ARG, who + ": null argument");
    int rc = check_series_spec(who, spec, in->rows, in->cols, nullptr);      // (nothing here needs a device)
    if (!rc) rc = mcf::check_below_vars(who, spec->var, "have a series");
    if (rc) return rc;
    RunSink sink;
    sink.out[MCF_OUT_TZ] = 1;
    sink.out[MCF_OUT_SOILM] = spec->var[MCF_OUT_SOILM] ? 1 : 0;
    sink.check = [&] { return mcf::check_depth_series_out(who, spec, D, out); };
    sink.enable = [&](mcf_plan* p) { return mcf_plan_series_enable_below(p, spec); };
    sink.fold = [](mcf_plan* p, int d0, int nd) { return mcf_plan_series_accumulate(p, 0, 0, d0, nd); };
    sink.finish = [&](mcf_plan* p) -> int {
        int rcf;
        for (int d = 0; spec->var[MCF_OUT_TZ] && d < D; ++d) {
            if (spec->npoints > 0 && (rcf = mcf_plan_series_fetch_points_depth(p, d, MCF_OUT_TZ, out->tz_points[d]))) return rcf;
            for (int k = 0; k < MCF_NZSTAT; ++k)
                if (spec->nzones > 0 && spec->zstat[k] && (rcf = mcf_plan_series_fetch_zones_depth(p, d, MCF_OUT_TZ, k, out->tz_zones[d][k]))) return rcf;
        }
        if (!spec->var[MCF_OUT_SOILM]) return MCF_OK;
        if (spec->npoints > 0 && (rcf = mcf_plan_series_fetch_points_depth(p, 0, MCF_OUT_SOILM, out->soilm_points))) return rcf;
        for (int k = 0; k < MCF_NZSTAT; ++k)
            if (spec->nzones > 0 && spec->zstat[k] && (rcf = mcf_plan_series_fetch_zones_depth(p, 0, MCF_OUT_SOILM, k, out->soilm_zones[k]))) return rcf;
        return MCF_OK;
    };
    return run_depths("mcf_runmicro_depths_series", in, opt, depths, D, tbp, chunk_days, sink);
}

// the bioclim sink on that driver (include/mcf.h); layered vegetation as run_bioclim takes it
int mcf_runbioclim_depths(const mcf_grid_inputs* in, const mcf_options* opt_in, const mcf_bioclim_sel* sel, const double* depths,
                          int32_t D, int32_t chunk_days, mcf_bioclim_depths_out* out) {
    const char* who = "mcf_runbioclim_depths";
    g_bioclim_chunks = 0;
    if (!in || !opt_in || !sel || !out) return fail(MCF_ERR_ARG, std::string(who) + ": null argument");
    mcf_grid_inputs in_l = *in;
    if (in->veg_layers > 1) {      // runbioclim3Cpp's fixed dfsel: fourteen one-day layers; later days belong to no layer
        if (in->veg_layers < 14) return fail(MCF_ERR_ARG, std::string(who) + ": layered vegetation needs the fourteen layers of runbioclim3Cpp");
        in_l.veg_layers = 14; in_l.lyr_st = kBioSt; in_l.lyr_ed = kBioEd;
    }
    mcf_options opt = *opt_in;
    opt.complete = 1;                                                   // cpp:3576: complete = true
    const BioDepthsSink bio{sel, out};
    mcf::BioAccDepthsArgs acc{};
    // the sink's own refusals come behind the depth list's (they read D buffers) and ahead of the driver's other checks
    int rc = check_depths(who, depths, D, nullptr, true, in_l.array_forcing != 0);
    if (!rc) rc = check_bioclim_depths(std::string(who) + ": ", &in_l, &bio, D);
    if (!rc) {
        RunSink sink;
        sink.out[MCF_OUT_TZ] = sink.out[MCF_OUT_SOILM] = 1;             // cpp:3569-3575 with air = 1
        sink.state_doubles = bioclim_state_doubles(D);
        sink.enable = [&](mcf_plan* p) { return bioclim_depths_begin(p, sel, acc); };
        sink.fold = [&](mcf_plan* p, int d0, int nd) {
            ++g_bioclim_chunks;
            return bioclim_depths_fold(p, sel, acc, d0, nd);
        };
        sink.finish = [&](mcf_plan* p) { return bioclim_depths_finish(p, &in_l, &bio, acc); };
        rc = run_depths(who, &in_l, &opt, depths, D, nullptr, chunk_days, sink);
    }
    if (rc && g_err.compare(0, strlen(who), who) != 0) g_err = std::string(who) + ": " + g_err;      // (the shared checks' messages)
    return rc;
}

int64_t mcf_plan_valid_cells(const mcf_plan* p) { return p ? p->valid_cells : 0; }
int64_t mcf_plan_bytes(const mcf_plan* p) { return p ? p->dev.bytes : 0; }

// ---- one-shot host-to-host solve ---------------------------------------------------------
// twi_mean: null, or the raster-wide mean of log(twi)/tfact to install (a row block of a larger raster, run_multi)
// sharers: host threads that solve their blocks on this device at the same time (one-process multi-device route with a device
// listed more than once): each sizes its ring from its share of the free HBM
// dsel / dout: the diagnostics to fetch beside the outputs (mcf_runmicro1_diag), or null
static int run_oneshot(const mcf_grid_inputs* in, const mcf_options* opt, mcf_outputs* out, int want_af,
                       const double* twi_mean = nullptr, int sharers = 1, const mcf_dtm_spec* dtm = nullptr,
                       const int32_t* dsel = nullptr, mcf_diag_outputs* dout = nullptr) {
    int rc = check_inputs(in, opt);
    if (rc) return rc;
    if (!out) return fail(MCF_ERR_ARG, "null outputs");
    int ndiag = 0;
    if (dsel) {
        if (opt->reqhgt < 0.0) return fail(MCF_ERR_ARG, "diagnostics need reqhgt >= 0");
        for (int v = 0; v < MCF_NDIAG; ++v) {
            if (dsel[v] && !dout->var[v]) return fail(MCF_ERR_ARG, "selected diagnostic has a null buffer");
            ndiag += dsel[v] ? 1 : 0;
        }
        if (ndiag == 0) return fail(MCF_ERR_ARG, "no diagnostic selected");
    }
    if ((in->array_forcing != 0) != (want_af != 0))
        return fail(MCF_ERR_ARG, want_af ? "mcf_runmicro2 needs array_forcing = 1" : "mcf_runmicro1 needs array_forcing = 0");
    for (int v = 0; v < MCF_NOUT; ++v)
        if (opt->out[v] && !out->var[v]) return fail(MCF_ERR_ARG, "requested output has a null buffer");
    if ((rc = ensure_device(opt->device))) return rc;
    const int64_t N = in->rows * in->cols, T = in->tsteps;
    // host arrays may be row blocks of a taller raster (row_pitch): a time step of an output is then pitch x cols values on
    const int64_t pitch = host_pitch(in), HS = pitch * in->cols;
    const int ndays = (int)(T / 24);
    int nvars = 0;
    for (int v = 0; v < MCF_NOUT; ++v) nvars += opt->out[v] ? 1 : 0;
    // reqhgt < 0: the whole-series plan ([N][tsteps] Tg plus a linear output ring of every step), or — when that does not fit in
    // free HBM, or MCF_BELOW_STREAM=1 — the plan streamed through day chunks; the same bits either way.  MCF_BELOW_STREAM=0: the
    // whole-series plan always.
    bool stream_bg = false;
    if (opt->reqhgt < 0.0 && ndays > 0) {
        const char* env = getenv("MCF_BELOW_STREAM");
        if (env && env[0] == '1') stream_bg = true;
        else if (!(env && env[0] == '0')) {
            size_t fr = 0, tot = 0;
            HIP_TRY(hipMemGetInfo(&fr, &tot));
            const double whole = (double)N * 8 * ((double)T * (1 + std::max(nvars, 1)) + 2.0 * ndays) +
                                 (in->array_forcing == 1 ? (opt->complete ? 16.0 : 18.0) * N * T * 8 : 0.0);    // forcing ring, Tg / Tbp
            stream_bg = whole > 0.8 * (double)fr / std::max(sharers, 1);
        }
    }
    const bool bg = opt->reqhgt < 0.0 && !stream_bg;
    const bool tail = stream_bg && T > (int64_t)ndays * 24;      // the steps behind the last whole day: one day more per slot
    // ---- chunk size from free HBM
    int chunk = opt->days_per_chunk;
    if (bg) {
        chunk = std::max(ndays, 1);
    } else if (chunk <= 0) {
        // the solver's variables and the forcing ring; streamed below ground the chunk's Tg ring (and, array forcing with
        // complete = 0, the point model's Tg / Tbp) and the per-cell state of one depth
        const int slabs = nvars + ndiag + (in->array_forcing ? 15 : 0) +
                          (stream_bg ? 1 + (in->array_forcing == 1 && !opt->complete ? 2 : 0) : 0);
        if ((rc = free_memory_chunk_days(N, ndays, sharers, slabs, stream_bg ? below_state_doubles(1, ndays) : 0.0, tail, &chunk)))
            return rc;
    }
    chunk = std::max(1, std::min(chunk, std::max(ndays, 1)));
    const bool timing = getenv("MCF_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now(), t_solve = 0, t_fetch = 0;
    mcf_plan* p = nullptr;
    if ((rc = plan_create(in, opt, stream_bg ? chunk + (tail ? 1 : 0) : chunk, 1, stream_bg, &p, dtm))) return rc;
    PlanHolder holder(p);
    if (twi_mean && (rc = mcf_plan_set_twi_mean(p, *twi_mean))) return rc;
    if (stream_bg && (rc = mcf_plan_below_prepare(p, in))) return rc;
    if (dsel && (rc = want_af ? mcf_plan_diag_enable_array(p, dsel) : mcf_plan_diag_enable(p, dsel))) return rc;
    double t_create = now() - t0;
    // the timing split: the driver's half (a chunk's forcing upload and its days, synchronised) and the sink's half (its fetches)
    double ta = now();
    rc = for_day_chunks(p, in, ndays, chunk, [&](int d0, int nd) -> int {
        if (timing) { mcf_plan_sync(p); t_solve += now() - ta; ta = now(); }
        for (int v = 0; !bg && v < MCF_NOUT; ++v)
            if (opt->out[v])
                if (const int rcf = mcf_plan_fetch_pitched(p, 0, v, 0, (int64_t)nd * 24, out->var[v] + HS * (int64_t)d0 * 24, pitch))
                    return rcf;
        for (int v = 0; !bg && dsel && v < MCF_NDIAG; ++v)
            if (dsel[v])
                if (const int rcf = diag_fetch_pitched(p, 0, v, 0, (int64_t)nd * 24, dout->var[v] + HS * (int64_t)d0 * 24, pitch))
                    return rcf;
        if (timing) { t_fetch += now() - ta; ta = now(); }
        return MCF_OK;
    });
    if (rc) return rc;
    if (timing)
        fprintf(stderr, "[mcf] one-shot: chunk %d days%s, plan create %.3f s, solve %.3f s, fetch %.3f s\n", chunk,
                stream_bg ? " (below ground streamed)" : "", t_create, t_solve, t_fetch);
    if (bg && ndays > 0) {
        for (int v = 0; v < MCF_NOUT; ++v)
            if (opt->out[v] && v != MCF_OUT_TZ)
                if ((rc = mcf_plan_fetch_pitched(p, 0, v, 0, (int64_t)ndays * 24, out->var[v], pitch))) return rc;
    }
    for (int v = 0; v < MCF_NOUT; ++v)
        if (opt->out[v]) fill_tail_na(out->var[v], in, ndays);
    for (int v = 0; dsel && v < MCF_NDIAG; ++v)
        if (dsel[v]) fill_tail_na(dout->var[v], in, ndays);
    if (bg && opt->out[MCF_OUT_TZ] && T > 0) {
        // Tbelowgroundv runs over all tsteps (cpp:2314-2319)
        if ((rc = mcf_plan_belowground(p))) return rc;
        if ((rc = mcf_plan_fetch_pitched(p, 0, MCF_OUT_TZ, 0, T, out->var[MCF_OUT_TZ], pitch))) return rc;
    }
    if (tail && opt->out[MCF_OUT_TZ]) {
        // ... whose steps behind the last whole day the last chunk left in its slot, behind that chunk's days
        const int last = (ndays - 1) / chunk * chunk, nd = ndays - last;
        if ((rc = mcf_plan_fetch_pitched(p, 0, MCF_OUT_TZ, (int64_t)nd * 24, T - (int64_t)ndays * 24,
                                         out->var[MCF_OUT_TZ] + HS * (int64_t)ndays * 24, pitch)))
            return rc;
    }
    return mcf_plan_sync(p);
}

// ---- a height profile from one plan (include/mcf.h mcf_runmicro_heights) ------------------------------------
int mcf_runmicro_heights(const mcf_grid_inputs* in, const mcf_options* opt_in, const double* heights, int32_t nheights,
                         const double* const* paia, mcf_outputs* out) {
    const std::string w = "mcf_runmicro_heights: ";
    if (!heights || nheights < 1) return fail(MCF_ERR_ARG, w + "a null or empty list of heights");
    for (int h = 0; h < nheights; ++h)
        if (const int rc = check_height_above("mcf_runmicro_heights", heights[h])) return rc;
    if (!in || !opt_in || !out) return fail(MCF_ERR_ARG, w + "null argument");
    mcf_options opt = *opt_in;
    opt.reqhgt = heights[0];
    int rc = check_inputs(in, &opt);
    if (rc) return rc;
    if (in->array_forcing == 1) return fail(MCF_ERR_ARG, w + "vector forcing or coarse array forcing (array_forcing = 0 or 2)");
    int nvars = 0;
    for (int v = 0; v < MCF_NOUT; ++v) {
        nvars += opt.out[v] ? 1 : 0;
        for (int h = 0; opt.out[v] && h < nheights; ++h)
            if (!out[h].var[v]) return fail(MCF_ERR_ARG, w + "a requested output of height " + std::to_string(h) + " has a null buffer");
    }
    if ((rc = ensure_device(opt.device))) return rc;
    const int64_t N = in->rows * in->cols, pitch = host_pitch(in), HS = pitch * in->cols;
    const int ndays = (int)(in->tsteps / 24);
    int chunk = opt.days_per_chunk;
    if (chunk <= 0 && (rc = free_memory_chunk_days(N, ndays, 1, nvars + (in->array_forcing ? 15 : 0), 0.0, false, &chunk))) return rc;
    chunk = std::max(1, std::min(chunk, std::max(ndays, 1)));
    // one plan and one ring: everything but the two foliage planes and reqhgt itself is set up once
    mcf_plan* p = nullptr;
    if ((rc = plan_create(in, &opt, chunk, 1, false, &p, nullptr, true))) return rc;
    PlanHolder holder(p);
    for (int h = 0; h < nheights; ++h) {
        if ((rc = mcf_plan_set_height(p, heights[h], paia ? paia[h] : nullptr))) return rc;
        rc = for_day_chunks(p, in, ndays, chunk, [&](int d0, int nd) -> int {
            for (int v = 0; v < MCF_NOUT; ++v)
                if (opt.out[v])
                    if (const int rcf = mcf_plan_fetch_pitched(p, 0, v, 0, (int64_t)nd * 24, out[h].var[v] + HS * (int64_t)d0 * 24, pitch))
                        return rcf;
            return MCF_OK;
        });
        if (rc) return rc;
        for (int v = 0; v < MCF_NOUT; ++v)
            if (opt.out[v]) fill_tail_na(out[h].var[v], in, ndays);
    }
    return mcf_plan_sync(p);
}

// ---- one process, several devices --------------------------------------------------------------------------------------
// The raster is cut into contiguous row blocks holding about the same number of valid cells (boundaries on multiples of 10
// rows, as microclimf_amd/distributed.py balanced_row_blocks); block b is solved on devices[b % n_devices] by that device's
// host thread with its own plan and stream.  Cells are independent inside the solver; its one global reduction — the mean
// of log(twi)/tfact over the raster (src/microclimfCpp.cpp:993-1004) — is taken over the WHOLE raster first, with the
// kernels a single-device plan uses, and installed in every block's plan: the result is bit for bit the single-device one.
// Host arrays are not copied: a block reads and writes its rows in place through the row pitch.
static std::vector<std::pair<int64_t, int64_t>> row_blocks(const mcf_grid_inputs* in, int nb) {
    const int64_t R = in->rows, pitch = host_pitch(in);
    const int64_t mult = R / 10 >= nb ? 10 : 1, ng = (R + mult - 1) / mult;
    std::vector<double> cum((size_t)ng + 1, 0.0);
    for (int64_t j = 0; j < in->cols; ++j)
        for (int64_t i = 0; i < R; ++i)
            if (!std::isnan(in->vegp.hgt[i + pitch * j])) cum[(size_t)(i / mult) + 1] += 1.0;
    for (int64_t g = 0; g < ng; ++g) cum[(size_t)g + 1] += cum[(size_t)g];
    const double total = cum[(size_t)ng];
    std::vector<int64_t> cuts{0};
    for (int r = 1; r < nb; ++r) {
        int64_t g = ng * r / nb;
        if (total > 0) {
            const double want = total * r / nb;
            g = std::lower_bound(cum.begin(), cum.end(), want) - cum.begin();
            if (g > 0 && std::fabs(cum[(size_t)g - 1] - want) <= std::fabs(cum[(size_t)std::min(g, ng)] - want)) --g;
        }
        g = std::min(std::max(g, cuts.back() + 1), ng - (nb - r));
        cuts.push_back(g);
    }
    cuts.push_back(ng);
    std::vector<std::pair<int64_t, int64_t>> out;
    for (int r = 0; r < nb; ++r) {
        const int64_t r0 = cuts[(size_t)r] * mult, r1 = std::min(cuts[(size_t)r + 1] * mult, R);
        out.emplace_back(r0, r1 - r0);
    }
    return out;
}

extern "C++" {
// block_fn(sub, o, r0, twi_mean, sharers): one row block — `sub` is the caller's inputs narrowed to the block's rows (same arrays, offset,
// read through the row pitch), `o` the options with the block's device, r0 the block's first row
template <class F>
static int for_row_blocks(const mcf_grid_inputs* in_caller, const mcf_options* opt, const mcf_multi* mu, F&& block_fn,
                          const mcf_dtm_spec* dtm = nullptr) {
    int rc = check_inputs(in_caller, opt);
    if (rc) return rc;
    if (!mu) return fail(MCF_ERR_ARG, "null argument");
    // what row_blocks and the whole-raster twi mean read, before any plan has validated the inputs
    if (!in_caller->vegp.hgt) return fail(MCF_ERR_ARG, "missing input array: vegp$hgt");
    const bool derive_twi = dtm && !in_caller->soilc.twi;
    if (!in_caller->soilc.twi && !derive_twi) return fail(MCF_ERR_ARG, "missing input array: twi");
    mcf_grid_inputs in_twi = *in_caller;       // (with a derived twi: the caller's inputs with the derived plane in place)
    const mcf_grid_inputs* in = &in_twi;
    std::vector<double> twi_host;              // the derived plane, laid out with the caller's row pitch: the blocks' plans upload their rows
    std::vector<int> devs;
    if ((rc = mcf::device_list(mu, 0, &devs))) return rc;
    mcf::RestoreDevice restore_dev;          // (the twi reduction below runs on the first device)
    int nb = mu->n_blocks > 0 ? mu->n_blocks : (int)devs.size();
    nb = (int)std::min<int64_t>(nb, in->rows);
    const int64_t pitch = host_pitch(in);
    // ---- the one global reduction, over the whole raster, on the first device (the kernels of mcf_plan_create)
    double twi_mean;
    {
        HIP_TRY(hipSetDevice(devs[0]));
        const int64_t N = in->rows * in->cols;
        double *d_twi = nullptr, *d_ws = nullptr;
        mcf::DevOwner tmp;
        if ((rc = tmp.alloc((void**)&d_twi, N * 8))) return rc;
        if ((rc = tmp.alloc((void**)&d_ws, (int64_t)mcf::twi_scratch_doubles() * 8))) return rc;
        if (derive_twi) {
            // the wetness index of the whole raster, once, on the first device (flow accumulation does not tile)
            double* d_dtm = nullptr;
            mcf::DevOwner tmp_dtm;      // (released before the reduction below)
            if ((rc = tmp_dtm.alloc((void**)&d_dtm, N * 8))) return rc;
            HIP_TRY(hipMemcpy(d_dtm, dtm->dtm, (size_t)N * 8, hipMemcpyHostToDevice));
            if ((rc = mcf::topidx_device(d_dtm, in->rows, in->cols, dtm->xres, dtm->yres, d_twi, nullptr))) return rc;
            twi_host.resize((size_t)(pitch * in->cols));
            HIP_TRY(hipMemcpy2D(twi_host.data(), (size_t)pitch * 8, d_twi, (size_t)in->rows * 8, (size_t)in->rows * 8, (size_t)in->cols,
                                hipMemcpyDeviceToHost));
            in_twi.soilc.twi = twi_host.data();
        } else {
            HIP_TRY(hipMemcpy2D(d_twi, (size_t)in->rows * 8, in->soilc.twi, (size_t)pitch * 8, (size_t)in->rows * 8, (size_t)in->cols,
                                hipMemcpyHostToDevice));
        }
        mcf::launch_twi_partial(d_twi, N, opt->tfact, d_ws, nullptr);
        double h2[2];
        HIP_TRY(hipMemcpy(h2, d_ws, 16, hipMemcpyDeviceToHost));
        twi_mean = h2[0] / h2[1];
    }
    const auto blocks = row_blocks(in, nb);
    const int nt = (int)std::min<size_t>(devs.size(), (size_t)nb);
    return mcf::run_workers(nt, [&](mcf::Worker& w) {
        mcf_options o = *opt;
        o.device = devs[(size_t)w.t];
        int sharers = 0;
        for (int d : devs) sharers += d == o.device;
        mcf::for_blocks(w, nb, nt, [&](int b) -> int {
            const int64_t r0 = blocks[(size_t)b].first, nr = blocks[(size_t)b].second;
            if (nr <= 0) return MCF_OK;
            return block_fn(mcf::narrow_rows(*in, r0, nr, pitch), o, r0, &twi_mean, sharers);
        });
    });
}

}  // extern "C++"
// dtm: null, or the WHOLE raster's (no halos, no placement) — a block then derives its missing terrain planes from its dtm
// rows plus the halo rows their stencils reach, gathered out of the caller's array as mcf_precompute_terrain_multi does
static int run_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_multi* mu, mcf_outputs* out, int want_af,
                     const mcf_dtm_spec* dtm = nullptr) {
    if (!out) return fail(MCF_ERR_ARG, "null argument");
    if (dtm && in) {
        if (dtm->halo_north || dtm->halo_south || (dtm->rows_total > 0 && (dtm->row0 != 0 || dtm->rows_total != in->rows)))
            return fail(MCF_ERR_ARG, "mcf_runmicro_dtm over several devices takes the whole raster (no halos, no placement)");
        if (in->rows <= 0 || in->cols <= 0) return fail(MCF_ERR_ARG, "rows/cols must be positive");
        if (const int rc = check_dtm(in, dtm)) return rc;
    }
    return for_row_blocks(in, opt, mu, [&](const mcf_grid_inputs& sub, const mcf_options& o, int64_t r0, const double* twi_mean, int sharers) {
        mcf_outputs so = *out;
        for (int v = 0; v < MCF_NOUT; ++v) if (so.var[v]) so.var[v] += r0;
        if (!dtm) return run_oneshot(&sub, &o, &so, want_af, twi_mean, sharers);
        const int64_t R = in->rows, nr = sub.rows;
        const int64_t need = dtm_halo_need(dtm_needs(&sub), dtm->agg > 0 ? dtm->agg : 10);
        const int64_t hn = std::min(need, r0), hs = std::min(need, R - r0 - nr);
        std::vector<double> ext;
        mcf::gather_rows(ext, dtm->dtm, R, in->cols, r0 - hn, hn + nr + hs);
        mcf_dtm_spec bd = *dtm;
        bd.dtm = ext.data(); bd.halo_north = (int32_t)hn; bd.halo_south = (int32_t)hs; bd.row0 = r0; bd.rows_total = R;
        return run_oneshot(&sub, &o, &so, want_af, twi_mean, sharers, &bd);
    }, dtm);
}
// the fused bioclim sink over row blocks: a block's nineteen [rows, cols] matrices go into its rows of the caller's
static int run_bioclim_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, const mcf_multi* mu,
                             mcf_bioclim_out* out, int want_af, int layered) {
    if (!out || !sel || !in) return fail(MCF_ERR_ARG, "null bioclim argument");
    const int64_t pitch = host_pitch(in);
    mcf_grid_inputs in_l = *in;
    if (layered) { in_l.veg_layers = 14; in_l.lyr_st = kBioSt; in_l.lyr_ed = kBioEd; }     // as run_bioclim: the fixed dfsel
    std::atomic<int> chunks{0};               // the blocks run on worker threads: their counts, summed for the caller's thread
    const int rc = for_row_blocks(&in_l, opt, mu, [&](const mcf_grid_inputs& sub, const mcf_options& o, int64_t r0, const double* twi_mean, int) {
        mcf_bioclim_out bo = *out;
        for (int v = 0; v < MCF_NBIO; ++v) if (bo.bio[v]) bo.bio[v] += r0;
        const int rcb = run_bioclim(&sub, &o, sel, &bo, want_af, layered, twi_mean, pitch);
        chunks += g_bioclim_chunks;
        return rcb;
    });
    g_bioclim_chunks = chunks;
    return rc;
}
int mcf_runbioclim1_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, const mcf_multi* mu, mcf_bioclim_out* out) {
    return run_bioclim_multi(in, opt, sel, mu, out, 0, 0);
}
int mcf_runbioclim2_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, const mcf_multi* mu, mcf_bioclim_out* out) {
    return run_bioclim_multi(in, opt, sel, mu, out, 1, 0);
}
int mcf_runbioclim3_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, const mcf_multi* mu, mcf_bioclim_out* out) {
    return run_bioclim_multi(in, opt, sel, mu, out, 0, 1);
}
int mcf_runbioclim4_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_bioclim_sel* sel, const mcf_multi* mu, mcf_bioclim_out* out) {
    return run_bioclim_multi(in, opt, sel, mu, out, 1, 1);
}

// period summaries over row blocks: a block's [rows, cols, nperiods] planes go into its rows of the caller's
int mcf_runmicro_summary_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_summary_spec* spec, int32_t chunk_days,
                               const mcf_multi* mu, mcf_summary_out* out) {
    if (!out || !spec || !in || !opt) return fail(MCF_ERR_ARG, "null summary argument");
    if (in->array_forcing != 0) return fail(MCF_ERR_ARG, "mcf_runmicro_summary_multi takes vector forcing (array_forcing = 0)");
    if (opt->reqhgt < 0.0) return fail(MCF_ERR_ARG, "period summaries need reqhgt >= 0 (the tiled ring)");
    if (chunk_days < 0) return fail(MCF_ERR_ARG, "summary: negative chunk_days");
    if (const int rc = check_summary_spec(spec, in->tsteps / 24, nullptr)) return rc;
    const int64_t pitch = host_pitch(in);
    return for_row_blocks(in, opt, mu, [&](const mcf_grid_inputs& sub, const mcf_options& o, int64_t r0, const double* twi_mean, int) {
        mcf_summary_out so = *out;
        for (int v = 0; v < MCF_NOUT; ++v)
            for (int k = 0; k < MCF_NSTAT; ++k)
                if (so.val[v][k]) so.val[v][k] += r0;
        if (r0 != 0) so.days = nullptr;      // (the same for every block: the first one reports them)
        return run_summary(&sub, &o, spec, chunk_days, &so, twi_mean, pitch);
    });
}

// the series sink over row blocks: each block folds its rows of the spec; the points go to their places in the caller's list,
// the blocks' zone states are combined and finished on the host (mcf_series_host.hpp)
int mcf_runmicro_series_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_series_spec* spec, int32_t chunk_days,
                              const mcf_multi* mu, mcf_series_out* out) {
    const std::string who = "mcf_runmicro_series_multi";
    if (!spec) return fail(MCF_ERR_ARG, who + ": null mcf_series_spec");
    if (!out || !in || !opt) return fail(MCF_ERR_ARG, who + ": null argument");
    if (in->array_forcing != 0) return fail(MCF_ERR_ARG, who + " takes vector forcing (array_forcing = 0)");
    if (opt->reqhgt < 0.0) return fail(MCF_ERR_ARG, who + ": the series sink needs reqhgt >= 0 (the tiled ring)");
    if (chunk_days < 0) return fail(MCF_ERR_ARG, who + ": negative chunk_days");
    int rc = check_series_spec(who, spec, in->rows, in->cols, nullptr);
    if (rc) return rc;
    if ((rc = mcf::check_series_out(who, spec, out))) return rc;
    struct BlockResult { mcf::SeriesBlockCut cut; SeriesRaw raw; };
    std::vector<std::unique_ptr<BlockResult>> results;
    std::mutex results_lock;
    rc = for_row_blocks(in, opt, mu, [&](const mcf_grid_inputs& sub, const mcf_options& o, int64_t r0, const double* twi_mean, int) {
        auto res = std::make_unique<BlockResult>();
        res->cut.cut(spec->npoints, spec->cells, spec->nzones, spec->zone, in->rows, in->cols, r0, sub.rows);
        if (res->cut.empty(spec->nzones)) return (int)MCF_OK;      // none of the points lies in this block, and there are no zones
        mcf_series_spec bs = *spec;
        bs.npoints = (int64_t)res->cut.cells.size(); bs.cells = res->cut.cells.data(); bs.zone = res->cut.zone.data();
        const int rcb = run_series(who, &sub, &o, &bs, chunk_days, nullptr, twi_mean, &res->raw);
        if (rcb) return rcb;
        std::lock_guard<std::mutex> hold(results_lock);
        results.push_back(std::move(res));
        return (int)MCF_OK;
    });
    if (rc) return rc;
    const int64_t T = std::max<int64_t>(in->tsteps, 1), steps = in->tsteps / 24 * 24;
    std::vector<int64_t> state;
    for (int v = 0; v < MCF_NOUT; ++v) {
        if (!spec->var[v]) continue;
        for (const auto& res : results)
            for (size_t i = 0; i < res->cut.where.size(); ++i)
                memcpy(out->points[v] + res->cut.where[i] * T, res->raw.points[v].data() + (int64_t)i * T, (size_t)T * 8);
        if (spec->nzones == 0) continue;
        state.resize((size_t)((int64_t)mcf::kSeriesStateRows * spec->nzones * steps));
        mcf::series_state_init(state.data(), spec->nzones, steps);
        for (const auto& res : results) mcf::series_state_merge(state.data(), res->raw.state[v].data(), spec->nzones, steps);
        for (int k = 0; k < MCF_NZSTAT; ++k)      // (every block has folded every whole day)
            if (spec->zstat[k]) mcf::series_state_finish(state.data(), spec->nzones, steps, T, nullptr, k, out->zones[v][k]);
    }
    return MCF_OK;
}

// ---- netCDF sink: the one-call solver entries (include/mcf.h "netCDF sink: further sources") ------------------
}  // extern "C"
namespace mcf {   // mcf_ncsink.hpp: the one-call entries' refusals that need no device, shared with mcf_snowrun.hip
static const char* const kNc4OneBlock =
    "the netCDF-4 container chunks a step into row strips of the whole raster: it takes one block (multi = NULL or n_blocks = 1)";
int nc_spec_check(const std::string& w, const mcf_nc_spec* spec, int64_t rows, int64_t cols, int64_t tsteps, double reqhgt,
                  const int32_t* out, bool several_blocks) {
    if (spec->rows != rows) return fail(MCF_ERR_ARG, w + "rows of the mcf_nc_spec are not the inputs' rows");
    if (spec->cols != cols) return fail(MCF_ERR_ARG, w + "cols of the mcf_nc_spec are not the inputs' cols");
    if (spec->nsteps != tsteps) return fail(MCF_ERR_ARG, w + "nsteps of the mcf_nc_spec is not the inputs' tsteps");
    if (!(spec->reqhgt == reqhgt)) return fail(MCF_ERR_ARG, w + "reqhgt of the mcf_nc_spec is not the run's");
    if (!spec->east || !spec->north || (spec->nsteps > 0 && !spec->time_hours)) return fail(MCF_ERR_ARG, w + "null coordinate vector");
    int n = 0;
    for (int v = 0; v < MCF_NOUT; ++v) {
        if (!spec->vars[v]) continue;
        mcf::NcVarDef d;
        double sc;
        bool put;
        if (!nc_var_def(v, reqhgt, &d, &sc, &put)) return fail(MCF_ERR_ARG, w + "writetonc defines no variable '" + d.name + "' at this reqhgt");
        if (out && !out[v]) return fail(MCF_ERR_ARG, w + "a variable of the mcf_nc_spec is not among the run's (opt->out)");
        ++n;
    }
    if (n == 0) return fail(MCF_ERR_ARG, w + "no variable selected");
    if (spec->format != MCF_NC_CLASSIC && spec->format != MCF_NC_NETCDF4) return fail(MCF_ERR_ARG, w + "unknown format");
    if (spec->format == MCF_NC_NETCDF4 && several_blocks) return fail(MCF_ERR_ARG, w + kNc4OneBlock);
    return MCF_OK;
}
int ncpack_spec_check(const std::string& w, const mcf_ncpack_spec* spec, int64_t rows, int64_t cols, int64_t tsteps, bool several_blocks) {
    if (spec->rows != rows) return fail(MCF_ERR_ARG, w + "rows of the mcf_ncpack_spec are not the inputs' rows");
    if (spec->cols != cols) return fail(MCF_ERR_ARG, w + "cols of the mcf_ncpack_spec are not the inputs' cols");
    if (spec->nsteps != tsteps) return fail(MCF_ERR_ARG, w + "nsteps of the mcf_ncpack_spec is not the inputs' tsteps");
    if (!spec->east || !spec->north || (spec->nsteps > 0 && !spec->time_hours)) return fail(MCF_ERR_ARG, w + "null coordinate vector");
    int n = 0;
    for (int v = 0; v < 5; ++v) n += spec->series[v] ? 1 : 0;
    if (n == 0) return fail(MCF_ERR_ARG, w + "no series selected");
    if (spec->format != MCF_NC_CLASSIC && spec->format != MCF_NC_NETCDF4) return fail(MCF_ERR_ARG, w + "unknown format");
    if (spec->format == MCF_NC_NETCDF4 && several_blocks) return fail(MCF_ERR_ARG, w + kNc4OneBlock);
    return MCF_OK;
}
}  // namespace mcf
extern "C" {
using mcf::NcHolder;

// the sink of one block (or the whole raster, r0 = 0) at a height above ground, and below ground with the tail's Tz
static RunSink nc_run_sink(const std::string& w, mcf_ncfile* nc, const mcf_nc_spec* spec, const mcf_grid_inputs* in, int64_t r0, bool below) {
    RunSink sink;
    for (int v = 0; v < MCF_NOUT; ++v) sink.out[v] = spec->vars[v] ? 1 : 0;      // the plan has exactly the file's variables
    const int64_t T = in->tsteps, nrows = in->rows;
    const int ndays = (int)(T / 24);
    sink.enable = [](mcf_plan*) { return (int)MCF_OK; };
    sink.fold = [=](mcf_plan* p, int d0, int nd) -> int {
        int rc = nc_write_rows(w, nc, p, 0, 0, r0, 0, (int64_t)d0 * 24, (int64_t)nd * 24, nullptr, false);
        // below ground the last chunk leaves the steps behind the last whole day in its slot, Tz only
        if (!rc && below && d0 + nd == ndays && T % 24)
            rc = nc_write_rows(w, nc, p, 0, 0, r0, (int64_t)nd * 24, (int64_t)ndays * 24, T % 24, nullptr, true);
        return rc;
    };
    sink.finish = [=](mcf_plan*) -> int {
        if (below || T % 24 == 0) return MCF_OK;
        const std::string e = mcf::nc_write_missing(nc->f.get(), r0, nrows, (int64_t)ndays * 24, T % 24);
        return e.empty() ? (int)MCF_OK : fail(MCF_ERR_ARG, w + e);
    };
    return sink;
}

int mcf_runmicro_nc(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_multi* mu, const char* path, const mcf_nc_spec* spec) {
    const char* who = "mcf_runmicro_nc";
    const std::string w = std::string(who) + ": ";
    if (!in || !opt || !path || !spec) return fail(MCF_ERR_ARG, w + "null argument");
    int rc = check_inputs(in, opt);
    if (!rc) rc = mcf::nc_spec_check(w, spec, in->rows, in->cols, in->tsteps, opt->reqhgt, nullptr, mu && mu->n_blocks != 1);
    const bool below = opt->reqhgt < 0.0;
    if (!rc && below && in->tsteps < 24) rc = fail(MCF_ERR_ARG, w + "the series is shorter than a day");
    if (!rc && opt->days_per_chunk < 0) rc = fail(MCF_ERR_ARG, w + "negative days_per_chunk");
    if (!rc && mu && mu->n_devices > 0 && !mu->devices) rc = fail(MCF_ERR_ARG, w + "n_devices > 0 with a null device list");
    if (rc) {
        if (g_err.compare(0, w.size(), w) != 0) g_err = w + g_err;      // (the shared checks' messages)
        return rc;
    }
    if ((rc = mu ? mcf::device_list(mu, 0, nullptr) : ensure_device(opt->device))) return rc;      // no file without a device to fill it
    mcf_ncfile* nc = nullptr;
    if ((rc = mcf_nc_create(path, spec, &nc))) return rc;
    NcHolder holder(nc);
    const int chunk_days = opt->days_per_chunk;
    auto block = [&](const mcf_grid_inputs& sub, const mcf_options& o, int64_t r0, const double* twi_mean, int sharers) -> int {
        const RunSink sink = nc_run_sink(w, nc, spec, &sub, r0, below);
        if (below) return run_depths(who, &sub, &o, nullptr, 0, nullptr, chunk_days, sink, twi_mean, sharers);
        return run_sink(&sub, &o, chunk_days, sink, twi_mean);
    };
    rc = mu ? for_row_blocks(in, opt, mu, block) : block(*in, *opt, 0, nullptr, 1);
    return rc ? rc : mcf::close_file(holder);      // (a failed run's file is closed by its holder, the run's message kept)
}

int mcf_runmicro_depths_nc(const mcf_grid_inputs* in, const mcf_options* opt, const double* depths, int32_t D, const double* tbp,
                           const char* const* paths, const mcf_nc_spec* spec) {
    const char* who = "mcf_runmicro_depths_nc";
    const std::string w = std::string(who) + ": ";
    if (!in || !opt || !paths || !spec) return fail(MCF_ERR_ARG, w + "null argument");
    int rc = check_depths(who, depths, D, tbp, opt->complete != 0, in->array_forcing != 0);
    if (rc) return rc;
    for (int d = 0; d < D; ++d)
        if (!paths[d]) return fail(MCF_ERR_ARG, w + "paths[" + std::to_string(d) + "] is null");
    if (!spec->vars[MCF_OUT_TZ]) return fail(MCF_ERR_ARG, w + "a file per depth holds Tz (vars[MCF_OUT_TZ])");
    {   // (the spec's own reqhgt is not read: file d is made at depths[d])
        mcf_nc_spec s0 = *spec;
        s0.reqhgt = depths[0];
        if ((rc = mcf::nc_spec_check(w, &s0, in->rows, in->cols, in->tsteps, depths[0], nullptr, false))) return rc;
    }
    if (opt->days_per_chunk < 0) return fail(MCF_ERR_ARG, w + "negative days_per_chunk");
    if (in->tsteps < 24) return fail(MCF_ERR_ARG, w + "the series is shorter than a day");
    if ((rc = ensure_device(opt->device))) return rc;
    std::vector<NcHolder> files;
    for (int d = 0; d < D; ++d) {
        mcf_nc_spec sd = *spec;
        sd.reqhgt = depths[d];
        mcf_ncfile* nc = nullptr;
        if ((rc = mcf_nc_create(paths[d], &sd, &nc))) return rc;
        files.emplace_back(nc);
    }
    const int64_t T = in->tsteps;
    const int ndays = (int)(T / 24);
    RunSink sink;
    sink.out[MCF_OUT_TZ] = 1;
    sink.out[MCF_OUT_SOILM] = spec->vars[MCF_OUT_SOILM] ? 1 : 0;
    sink.enable = [](mcf_plan*) { return (int)MCF_OK; };
    sink.fold = [&](mcf_plan* p, int d0, int nd) -> int {
        for (int d = 0; d < D; ++d) {
            int rcf = nc_write_rows(w, files[(size_t)d].get(), p, 0, d, 0, 0, (int64_t)d0 * 24, (int64_t)nd * 24, nullptr, false);
            if (!rcf && d0 + nd == ndays && T % 24)
                rcf = nc_write_rows(w, files[(size_t)d].get(), p, 0, d, 0, (int64_t)nd * 24, (int64_t)ndays * 24, T % 24, nullptr, true);
            if (rcf) return rcf;
        }
        return MCF_OK;
    };
    sink.finish = [](mcf_plan*) { return (int)MCF_OK; };
    rc = run_depths(who, in, opt, depths, D, tbp, opt->days_per_chunk, sink);
    for (auto& f : files) {
        const int rcc = rc ? (int)MCF_OK : mcf::close_file(f);
        if (rcc) rc = rcc;
    }
    return rc;
}

int mcf_runmicro1(const mcf_grid_inputs* in, const mcf_options* opt, mcf_outputs* out) {
    return run_oneshot(in, opt, out, 0);
}
int mcf_runmicro_dtm(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_dtm_spec* dtm, const mcf_multi* multi, mcf_outputs* out) {
    if (!in || !dtm) return fail(MCF_ERR_ARG, "null inputs / mcf_dtm_spec");
    const int want_af = in->array_forcing != 0;
    if (multi) {
        if (!dtm->dtm) return fail(MCF_ERR_ARG, "mcf_dtm_spec: null dtm");
        return run_multi(in, opt, multi, out, want_af, dtm);
    }
    return run_oneshot(in, opt, out, want_af, nullptr, 1, dtm);
}
int mcf_runmicro1_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_multi* multi, mcf_outputs* out) {
    return run_multi(in, opt, multi, out, 0);
}
int mcf_runmicro2_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_multi* multi, mcf_outputs* out) {
    return run_multi(in, opt, multi, out, 1);
}
int mcf_runmicro2(const mcf_grid_inputs* in, const mcf_options* opt, mcf_outputs* out) {
    return run_oneshot(in, opt, out, 1);
}
int mcf_runmicro1_diag(const mcf_grid_inputs* in, const mcf_options* opt, const int32_t sel[MCF_NDIAG], mcf_outputs* out,
                       mcf_diag_outputs* diag_out) {
    if (!sel || !diag_out) return fail(MCF_ERR_ARG, "null argument");
    if (in && in->array_forcing != 0) return fail(MCF_ERR_ARG, "diagnostics are not available with array forcing");
    return run_oneshot(in, opt, out, 0, nullptr, 1, nullptr, sel, diag_out);
}
int mcf_runmicro3_diag(const mcf_grid_inputs* in, const mcf_options* opt, const int32_t sel[MCF_NDIAG], mcf_outputs* out,
                       mcf_diag_outputs* diag_out) {
    if (!sel || !diag_out) return fail(MCF_ERR_ARG, "null argument");
    if (in && in->veg_layers < 1) return fail(MCF_ERR_ARG, "mcf_runmicro3_diag needs veg_layers >= 1 and dfsel");
    if (in && in->array_forcing != 0) return fail(MCF_ERR_ARG, "diagnostics are not available with array forcing");
    return run_oneshot(in, opt, out, 0, nullptr, 1, nullptr, sel, diag_out);
}
// array weather, fine or coarse as `in` says (the entries above keep their refusals)
int mcf_runmicro2_diag(const mcf_grid_inputs* in, const mcf_options* opt, const int32_t sel[MCF_NDIAG], mcf_outputs* out,
                       mcf_diag_outputs* diag_out) {
    if (!sel || !diag_out) return fail(MCF_ERR_ARG, "null argument");
    return run_oneshot(in, opt, out, 1, nullptr, 1, nullptr, sel, diag_out);
}
int mcf_runmicro4_diag(const mcf_grid_inputs* in, const mcf_options* opt, const int32_t sel[MCF_NDIAG], mcf_outputs* out,
                       mcf_diag_outputs* diag_out) {
    if (!sel || !diag_out) return fail(MCF_ERR_ARG, "null argument");
    if (in && in->veg_layers < 1) return fail(MCF_ERR_ARG, "mcf_runmicro4_diag needs veg_layers >= 1 and dfsel");
    return run_oneshot(in, opt, out, 1, nullptr, 1, nullptr, sel, diag_out);
}
int mcf_runmicro3(const mcf_grid_inputs* in, const mcf_options* opt, mcf_outputs* out) {
    if (in && in->veg_layers < 1) return fail(MCF_ERR_ARG, "mcf_runmicro3 needs veg_layers >= 1 and dfsel");
    return run_oneshot(in, opt, out, 0);
}
int mcf_runmicro4(const mcf_grid_inputs* in, const mcf_options* opt, mcf_outputs* out) {
    if (in && in->veg_layers < 1) return fail(MCF_ERR_ARG, "mcf_runmicro4 needs veg_layers >= 1 and dfsel");
    return run_oneshot(in, opt, out, 1);
}
// time-varying vegetation over row blocks: the layered arrays [rows, cols, layers] are read through the same row pitch
int mcf_runmicro3_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_multi* multi, mcf_outputs* out) {
    if (in && in->veg_layers < 1) return fail(MCF_ERR_ARG, "mcf_runmicro3_multi needs veg_layers >= 1 and dfsel");
    return run_multi(in, opt, multi, out, 0);
}
int mcf_runmicro4_multi(const mcf_grid_inputs* in, const mcf_options* opt, const mcf_multi* multi, mcf_outputs* out) {
    if (in && in->veg_layers < 1) return fail(MCF_ERR_ARG, "mcf_runmicro4_multi needs veg_layers >= 1 and dfsel");
    return run_multi(in, opt, multi, out, 1);
}

}  // extern "C"
