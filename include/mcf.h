/*
 * mcf.h — C ABI of libmcfhip: the MI355X (gfx950) grid microclimate solver.
 *
 * Drop-in boundary for the reference's `.Call` entry points (all paths below are
 * under the upstream repository root):
 *
 *   mcf_runmicro1()  replaces  _microclimf_runmicro1Cpp   src/RcppExports.cpp:250-272
 *                    (R stub   runmicro1Cpp               R/RcppExports.R:72-74,
 *                     body     runmicro1Cpp               src/microclimfCpp.cpp:2052-2337)
 *   mcf_runmicro2()  replaces  _microclimf_runmicro2Cpp   src/RcppExports.cpp:275-297
 *                    (R stub   runmicro2Cpp               R/RcppExports.R:76-78,
 *                     body     runmicro2Cpp               src/microclimfCpp.cpp:2340-2621)
 *   mcf_runmicro3/4() replace  _microclimf_runmicro3Cpp/4Cpp (time-varying vegetation,
 *                     bodies src/microclimfCpp.cpp:2624-3226), R stubs R/RcppExports.R:80-86
 *
 * Everything is plain pointers + sizes; no R, Rcpp or torch types.  All arrays
 * are IEEE fp64, column-major with the raster row as the fastest index, exactly
 * as R hands them to the reference:
 *
 *   matrix  [rows, cols]          element (i,j)     at  i + rows*j
 *   3-D     [rows, cols, n]       element (i,j,k)   at  i + rows*j + rows*cols*k
 *
 * "NA" follows Rcpp's NumericVector::is_na, i.e. any NaN.  Cells whose `hgt`
 * is NA are skipped and every requested output holds R's NA_real_ bit pattern
 * (0x7FF00000000007A2) there, as do time steps past the last whole day
 * (ndays = tsteps / 24 truncates, src/microclimfCpp.cpp:2116).
 *
 * Two levels:
 *   1. one-shot host calls (mcf_runmicro1 / mcf_runmicro2): host pointers in,
 *      host pointers out; the library stages everything through HBM in day
 *      chunks.  This is what the R glue binds.
 *   2. the plan API: inputs are uploaded once and stay resident in HBM, day
 *      chunks are solved into a device-resident output ring, and the caller
 *      decides what (if anything) is copied back.  bench.py and multi-GPU row
 *      tiling use this level.
 *
 * There is no CPU fallback: every solver / kernel entry point fails with
 * MCF_ERR_NO_DEVICE when no HIP device is usable.  Host-side by nature, as in the
 * reference, and therefore usable without a device: the one-point time-series model
 * (mcf_bigleaf, mcf_soilm, mcf_pointmprocess, mcf_weatherhgt; their `_batch` forms for many points are device entries) and the file side of
 * the writetonc sink (mcf_nc_create, mcf_nc_write_host, mcf_nc_close), and the
 * flow-accumulation sweep behind soilc$twi (mcf_flowacc, mcf_topidx; on the device: mcf_flowacc_device, mcf_topidx_device).
 */
#ifndef MCF_H
#define MCF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCF_ABI_VERSION 8   /* 2: mcf_grid_inputs grew the coarse-forcing fields; 3: tiled output ring (mcf_plan_ring_layout);
                             * 4: mcf_nc_spec grew format / deflate_level (zero = the behaviour of version 3); 5: mcf_runmicrosnow1 / mcf_snowrun_*;
                             * 6: mcf_snowdriver_in grew af_wsa_s (the former `reserved`) / af_wind at its end — read only with array weather;
                             * 7: below ground streamed through day chunks (mcf_plan_create_streamed, mcf_plan_below_prepare);
                             * 8: plans and one-shot solves that take the dtm (mcf_dtm_spec), flow accumulation / wetness index on the device
                             *    (added since, functions only: mcf_plan_below_set_days, mcf_below_days_range, mcf_runmicrosnow1_below,
                             *    mcf_runmicrosnow1_below_multi, mcf_snowrun_create_below, mcf_snowmodelq1, mcf_canintfrac_device,
                             *    mcf_meltmu_device, mcf_snowmodelq2, mcf_meltmu2_device, mcf_plan_summary_*, mcf_runmicro_summary,
                             *    mcf_runmicro_summary_multi, mcf_snowmodel2_coarse, mcf_snow_expand_coarse_device, mcf_snowplan_summary_*,
                             *    mcf_snowrun_summary_*, mcf_runmicrosnow_summary, mcf_snowmodel1_summary,
                             *    mcf_microsnow_expand_coarse_device, mcf_runmicrosnow2_coarse, mcf_snowrun_create_coarse,
                             *    mcf_plan_set_day_layers, mcf_snowrun_set_day_layers, mcf_plan_fetch_mxtc, mcf_plan_below_set_depths,
                             *    mcf_plan_fetch_depth*, mcf_plan_summary_enable_below, mcf_plan_summary_fetch_depth, mcf_runmicro_depths,
                             *    mcf_runmicro_depths_summary, mcf_plan_diag_enable_array, mcf_runmicro2_diag, mcf_runmicro4_diag,
                             *    mcf_foliageden, mcf_foliageden_device, mcf_plan_set_height, mcf_plan_fetch_foliage, mcf_runmicro_heights,
                             *    mcf_plan_series_*, mcf_runmicro_series, mcf_zonal_series, mcf_series_state_merge, mcf_series_state_finish,
                             *    mcf_runmicro_series_multi, mcf_runmicro_depths_series, mcf_snowplan_series_*, mcf_snowrun_series_*,
                             *    mcf_runmicrosnow_series, mcf_snowmodel1_series) */

/* Output variables, in the order of the reference's returned list
 * (src/microclimfCpp.cpp:2326-2335) and of its `out` logical(10). */
enum {
    MCF_OUT_TZ = 0,       /* "Tz"        air T at reqhgt (reqhgt>0), ground T (==0), soil T (<0) */
    MCF_OUT_TLEAF = 1,    /* "tleaf"     leaf T (reqhgt>0 only)                              */
    MCF_OUT_RELHUM = 2,   /* "relhum"    relative humidity % (reqhgt>0 only)                 */
    MCF_OUT_SOILM = 3,    /* "soilm"     distributed volumetric soil moisture                */
    MCF_OUT_WINDSPEED = 4,/* "windspeed" wind speed at reqhgt                                */
    MCF_OUT_RDIRDOWN = 5, /* "Rdirdown"  downward direct SW at reqhgt                        */
    MCF_OUT_RDIFDOWN = 6, /* "Rdifdown"  downward diffuse SW                                 */
    MCF_OUT_RLWDOWN = 7,  /* "Rlwdown"   downward LW (reqhgt>=0)                             */
    MCF_OUT_RSWUP = 8,    /* "Rswup"     upward SW                                           */
    MCF_OUT_RLWUP = 9,    /* "Rlwup"     upward LW (reqhgt>=0)                               */
    MCF_NOUT = 10
};

/* Error codes (0 = success).  mcf_last_error() gives the message of the most
 * recent failure on the calling thread. */
enum {
    MCF_OK = 0,
    MCF_ERR_ARG = 1,        /* NULL/ill-sized argument                                  */
    MCF_ERR_NO_DEVICE = 2,  /* no usable HIP device / kernels not loadable              */
    MCF_ERR_HIP = 3,        /* a HIP runtime call failed (message has the HIP error)    */
    MCF_ERR_NOMEM = 4,      /* request does not fit device memory                       */
    MCF_ERR_STATE = 5       /* plan used out of order                                   */
};

/* obstime data.frame (src/microclimfCpp.cpp:2057-2060).  R passes year/month/day
 * as doubles that Rcpp coerces to int; the glue does that coercion. */
typedef struct mcf_obstime {
    const int32_t *year, *month, *day; /* [tsteps] */
    const double *hour;                /* [tsteps] decimal hour */
} mcf_obstime;

/* climdata (src/microclimfCpp.cpp:2062-2071 data.frame columns temp, es, ea,
 * tdew, pres, swdown, difrad, lwdown, windspeed, winddir; :2350-2359 list
 * entries tc, es, ea, tdew, pk, ...).  Vector forcing: each [tsteps].  Array
 * forcing: each [rows,cols,tsteps] except winddir, which stays [tsteps]. */
typedef struct mcf_climate {
    const double *tc, *es, *ea, *tdew, *pk, *swdown, *difrad, *lwdown, *windspeed, *winddir;
} mcf_climate;

/* pointm (src/microclimfCpp.cpp:2073-2082; :2361-2370, where G is named Gp).
 * T0p and DDp are accepted by the reference but never read; they are not part
 * of this ABI.  Tg/Tbp are only read when reqhgt < 0 and complete == 0 and may
 * be NULL otherwise.  Shapes as mcf_climate. */
typedef struct mcf_pointm {
    const double *soilm, *Tg, *Tbp, *G, *umu, *kp, *muGp, *dtrp;
} mcf_pointm;

/* vegp list (src/microclimfCpp.cpp:2084-2094), each [rows,cols]; with time-varying
 * vegetation (runmicro3Cpp / runmicro4Cpp, src/microclimfCpp.cpp:2667-2679) each is
 * [rows,cols,veg_layers]. */
typedef struct mcf_vegp {
    const double *hgt, *pai, *x, *gsmax, *leafr, *leaft, *clump, *leafd, *paia, *leafden;
} mcf_vegp;

/* soilc list (src/microclimfCpp.cpp:2096-2111): 13 matrices + wsa[rows,cols,8]
 * + hor[rows,cols,24]. */
typedef struct mcf_soilc {
    const double *Smin, *Smax, *gref, *soilb, *Psie, *Vq, *Vm, *Mc, *rho;
    const double *slope, *aspect, *twi, *svfa;
    const double *wsa; /* [rows,cols,8]  */
    const double *hor; /* [rows,cols,24] */
} mcf_soilc;

typedef struct mcf_grid_inputs {
    int64_t rows, cols, tsteps;
    int32_t array_forcing; /* 0: runmicro1Cpp/3Cpp geometry, 1: runmicro2Cpp/4Cpp geometry, 2: coarse arrays (below) */
    int32_t veg_layers;    /* 0 or 1: static vegetation; >1: runmicro3Cpp/4Cpp `dfsel` layers    */
    mcf_obstime obstime;
    mcf_climate clim;
    mcf_pointm pointm;
    mcf_vegp vegp;
    mcf_soilc soilc;
    double lat, lon;           /* vector forcing (runmicro1Cpp args lat, lon)            */
    const double *lats, *lons; /* array forcing  (runmicro2Cpp args lats, lons), [rows,cols] */
    /* dfsel of runmicro3Cpp/4Cpp (src/microclimfCpp.cpp:2629-2640): layer l drives the steps
     * lyr_st[l] .. lyr_ed[l] (0-based, whole days); NULL when veg_layers <= 1 */
    const int32_t *lyr_st, *lyr_ed;
    /* array_forcing == 2 — COARSE array forcing, the MI355X-native form of `.runmodel2Cpp` (R/internal.R:1175-1343):
     * the reference resamples every coarse climate / point-model variable to the fine raster (`.cca` ->
     * terra::resample, bilinear; R/internal.R:523-542, 1224-1277) and hands runmicro2Cpp full [rows,cols,T] arrays —
     * 120 B per cell-step to upload, hold and read back, the reason a tile is capped at 2e7 cell-steps
     * (R/Cppwrappers.R:469).  Here the coarse arrays stay coarse: clim.{tc,pk,swdown,difrad,lwdown,windspeed},
     * coarse_relhum, coarse_winddir and pointm.{soilm,G,umu,kp,muGp,dtrp} are [coarse_rows, coarse_cols, tsteps]; the
     * solver interpolates them bilinearly per cell-step and derives es, ea, tdew (.satvap, .dewpoint after
     * interpolating temp and relhum), wind speed (from interpolated u, v components) and the raster-mean wind
     * direction exactly where `.runmodel2Cpp` does.  clim.es, ea, tdew, winddir are ignored.
     * coarse_rowpos[i] / coarse_colpos[j]: position of raster row i / column j in units of coarse rows / columns,
     * 0 = centre of the first coarse row / column, clamped by the caller to [0, coarse_rows-1] / [0, coarse_cols-1]
     * (edge replication).  reqhgt < 0 needs complete = 1 in this mode. */
    int32_t coarse_rows, coarse_cols;
    const double *coarse_rowpos, *coarse_colpos;
    const double *coarse_relhum, *coarse_winddir;
    /* `.runmodel2Cpp`'s altcorrect (R/internal.R:1233-1251): 0 none; 1 fixed lapse rate 5 K/km; 2 humidity-dependent
     * lapse rate (`.lapserate`, R/internal.R:545-550).  With 1 or 2: coarse_dtm [coarse_rows, coarse_cols] (elevation
     * of the climate cells, NA read as 0) and fine_dtm [rows, cols]; pressure goes to sea level on the coarse grid and
     * back up on the fine one, temperature moves by lapse rate x (interpolated coarse elevation - fine elevation);
     * es, ea, tdew come from the UNcorrected temperature, as in the reference. */
    int32_t coarse_altcorrect;
    const double *coarse_dtm, *fine_dtm;
    /* 0 or rows: dense arrays.  > rows: every raster array above ([rows, cols(, layers | steps)]: vegp, soilc, wsa, hor, lats,
     * lons, fine_dtm, the array-forcing series) AND the output arrays of the one-shot entry points are row blocks of a
     * taller column-major raster with `row_pitch` rows — read and written in place (how mcf_runmicro1_multi hands a block
     * to a device without copying the host arrays). */
    int64_t row_pitch;
} mcf_grid_inputs;

typedef struct mcf_options {
    double reqhgt, zref;
    double Sminp, Smaxp; /* accepted for signature parity; unused by the reference (cpp:975) */
    double tfact;
    double mat;          /* mean annual temperature, reqhgt<0 && !complete */
    int32_t complete;
    int32_t out[MCF_NOUT];
    int32_t device;          /* HIP device ordinal                                      */
    int32_t days_per_chunk;  /* 0 = choose from free HBM                                */
    int32_t cells_per_block; /* 0 = default (21: two 8-wave workgroups per CU); 16, 21, 32, 42 (42: vector forcing only —
                              * array forcing is given its 32-cell tiles instead) */
} mcf_options;

/* Host output buffers, each [rows,cols,tsteps] or NULL when out[v]==0. */
typedef struct mcf_outputs {
    double *var[MCF_NOUT];
} mcf_outputs;

int mcf_abi_version(void);
const char *mcf_last_error(void);
/* Number of visible HIP devices (0 when none); never fails. */
int mcf_device_count(void);

/* One-shot host-to-host solves. */
int mcf_runmicro1(const mcf_grid_inputs *in, const mcf_options *opt, mcf_outputs *out);
int mcf_runmicro2(const mcf_grid_inputs *in, const mcf_options *opt, mcf_outputs *out);
/* The same solves on several devices of one node from ONE process — the R drop-in's way to a multi-GPU node (R has no
 * torch.distributed): the raster is cut into `n_blocks` contiguous row blocks of about equal valid-cell count (boundaries
 * on multiples of 10 rows; R/internal.R:909-925 is the reference's own tiling), block b goes to devices[b % n_devices],
 * one host thread per device.  The solver's one global reduction (mean of log(twi)/tfact, src/microclimfCpp.cpp:993-1004)
 * is taken over the whole raster first and installed in every block, so the result is bit for bit the single-device one.
 * n_devices = 0: every visible device; n_blocks = 0: one block per device (more blocks than devices are time-sliced).
 * mcf_runmicro3_multi / 4_multi: the same with time-varying vegetation (declared behind mcf_runmicro3 / 4 below). */
typedef struct mcf_multi {
    int32_t n_devices;
    const int32_t *devices;
    int32_t n_blocks;
} mcf_multi;
int mcf_runmicro1_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_multi *multi, mcf_outputs *out);
int mcf_runmicro2_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_multi *multi, mcf_outputs *out);

/* Time-varying vegetation: replace _microclimf_runmicro3Cpp / _microclimf_runmicro4Cpp
 * (src/RcppExports.cpp:300-322 / 326-348; bodies src/microclimfCpp.cpp:2624-2924 / 2926-3226).
 * Same physics with the vegetation layer chosen per day from `dfsel`; steps outside every
 * layer's range stay NA. */
int mcf_runmicro3(const mcf_grid_inputs *in, const mcf_options *opt, mcf_outputs *out);
int mcf_runmicro4(const mcf_grid_inputs *in, const mcf_options *opt, mcf_outputs *out);
int mcf_runmicro3_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_multi *multi, mcf_outputs *out);
int mcf_runmicro4_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_multi *multi, mcf_outputs *out);

/* ---- plan API: HBM-resident inputs, device output ring ---------------------- */
typedef struct mcf_plan mcf_plan;

/* Uploads all static inputs (and, for vector forcing, builds the per-timestep
 * table on the device).  `ring_days` is the capacity of each output ring slot in
 * days, `ring_slots` the number of slots (>=1).  For reqhgt<0 the ring must hold
 * the whole series (ring_days >= tsteps/24, enforced). */
int mcf_plan_create(const mcf_grid_inputs *in, const mcf_options *opt,
                    int32_t ring_days, int32_t ring_slots, mcf_plan **plan);
void mcf_plan_destroy(mcf_plan *plan);

/* Raster-wide mean of log(twi)/tfact over non-NA cells (src/microclimfCpp.cpp:
 * 993-1004) is the solver's only global reduction.  mcf_plan_create computes it
 * for the plan's own cells; row-tiled multi-GPU runs fetch the partial
 * (sum,count), all-reduce them (RCCL) and install the global mean. */
int mcf_plan_twi_partial(mcf_plan *plan, double *sum, int64_t *count);
int mcf_plan_set_twi_mean(mcf_plan *plan, double mean);

/* Array forcing only: upload the [rows,cols,24*ndays] slabs of every forcing
 * array for days [day0, day0+ndays) into the plan's forcing buffer (slot). */
int mcf_plan_upload_forcing_days(mcf_plan *plan, const mcf_grid_inputs *in,
                                 int32_t day0, int32_t ndays, int32_t slot);

/* Solve days [day0, day0+ndays) into ring slot `slot` (async on the plan's
 * stream).  The slot holds the reference's [rows,cols,24*ndays] arrays
 * (src/microclimfCpp.cpp:2292-2303) in a device-internal order — see
 * mcf_plan_ring_layout; mcf_plan_fetch* / mcf_nc_write_plan return them in the
 * reference's layout. */
int mcf_plan_run_days(mcf_plan *plan, int32_t day0, int32_t ndays, int32_t slot);
/* The same with the days written at day `slot_day0` of the slot instead of its start (vector forcing, reqhgt >= 0): several
 * runs of days of one chunk, each at its own place (the snow branch's no-snow days). */
int mcf_plan_run_days_at(mcf_plan *plan, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0);
/* ... and for a SUBSET of the tiles: skip_tile[t] != 0 (t < n_tiles = ceil(cells / mcf_ring_layout.cells_per_tile); tile t =
 * cells t * cells_per_tile ... of the column-major raster) leaves tile t's blocks of these days untouched in the slot.  The
 * snow run uses it for the days that are no-snow days AND snow days: `.runmicrosnow1` (R/internal.R:3632-3655) overwrites
 * every snow-covered cell-step of such a day with gridmicrosnow1's value, so the solver's values of a tile whose cells all lie
 * under snow for the whole run of days are dead — mcf_snowplan_covered_tiles finds those tiles.  skip_tile = NULL: all. */
int mcf_plan_run_days_masked(mcf_plan *plan, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0,
                             const uint8_t *skip_tile, int64_t n_tiles);
/* ... and for a SUBSET of the CELLS (vector forcing, reqhgt >= 0): need_cell — DEVICE memory on the plan's device, complete when
 * the call is made, one byte per cell of the column-major raster (n_cells = rows x cols) — marks the cells whose values of these
 * days are wanted; every other cell's values in the slot stay as they are.  The marked cells are gathered into dense tiles of
 * their own (their constants copied from the plan's tiles; the cells of the plan's regular tiles and those of its other tiles
 * apart, so that every cell meets the instantiation it meets in a launch of the plan's own tiles), solved into a ring of their
 * own and copied to their places in the slot: the same bits as mcf_plan_run_days_at's.  Where tiles are the unit (mcf_plan_run_days_masked) one snow-free cell keeps its
 * whole 21-cell tile in the launch; on a day that is both a snow day and a no-snow day the cells the merge of `.runmicrosnow1`
 * (R/internal.R:3632-3655) keeps from the no-snow model are a few per cent scattered over most tiles —
 * mcf_snowplan_free_cells finds them.  *n_gathered (may be NULL) = marked cells.  Memory: the gathered tiles' constants, and
 * their ring for as many of the days at a time as an eighth of the plan's ring holds (MCF_CELLS_RING_GB overrides). */
int mcf_plan_run_days_cells(mcf_plan *plan, int32_t day0, int32_t ndays, int32_t slot, int32_t slot_day0,
                            const uint8_t *need_cell, int64_t n_cells, int64_t *n_gathered);
/* Vector forcing: replace the series' maximum air temperature (src/microclimfCpp.cpp:2159-2168; it caps the
 * Penman-Monteith temperature excess, cpp:1236).  The snow branch solves a SUBSET of the days and the reference takes
 * the maximum over that subset. */
int mcf_plan_set_mxtc(mcf_plan *plan, double mxtc);
/* Array forcing (at the raster's resolution): the same per CELL (src/microclimfCpp.cpp:2467-2471) over the days with
 * dayflag[d] != 0 — the temperature series of `in` streamed once more, a run of flagged days at a time.  Also since this
 * version: mcf_plan_run_days_at accepts a run of days INSIDE the days a slot's forcing was uploaded for, with array forcing.
 * A plan with COARSE array forcing (array_forcing == 2) folds the flagged days of its resident series (`in` is not read, may be
 * NULL): the interpolated, altitude-corrected temperature of the plan's create-time maximum, started from -273.15 — a maximum is
 * order-free, so bit for bit the cap of a coarse plan created on the host-subset coarse arrays. */
int mcf_plan_set_mxtc_days(mcf_plan *plan, const mcf_grid_inputs *in, const int32_t *dayflag, int32_t ndays);
/* Layered vegetation (veg_layers > 1): replace the day -> layer map the plan made from lyr_st / lyr_ed; layer_of_day[d] in
 * 0 .. veg_layers - 1, or -1 for a day no layer covers; ndays = tsteps / 24.  For callers that solve a SUBSET of the days and deal
 * the subset to layers themselves (`.runmodel3Cpp` on `.runmicronosnow`'s day subset renumbers the layers it uses,
 * R/internal.R:1391-1399, so a layer that serves no day of the subset shifts the ones behind it). */
int mcf_plan_set_day_layers(mcf_plan *plan, const int32_t *layer_of_day, int32_t ndays);   /* layer_of_day NULL: the plan's own table again */
/* Array forcing (fine or coarse): the per-cell temperature cap's maximum air temperature as the plan holds it now, [rows, cols]. */
int mcf_plan_fetch_mxtc(mcf_plan *plan, double *host_dst);
/* reqhgt<0: after every day has been solved into slot 0, smooth the stored
 * ground-temperature series into Tz (Tbelowgroundv, cpp:1474-1539).  Not for a streamed plan (MCF_ERR_STATE). */
int mcf_plan_belowground(mcf_plan *plan);
/* Below ground streamed through day chunks.  For reqhgt >= 0 mcf_plan_create_streamed is mcf_plan_create.  For reqhgt < 0 it
 * keeps the requested ring (tiled, as for reqhgt >= 0: mcf_plan_ring_layout) and allocates nothing of size cells x steps: the
 * chunk's ground temperature (one more ring slot variable) and O(cells x days) of per-cell state — the damping-depth sum, and
 * with complete = 1 the hourly sum, the daily means and the series' last 47 hours.  A slot may hold tsteps / 24 + 1 days: the
 * chunk that ends on the last whole day also leaves the tsteps % 24 steps behind it (Tz only) in its slot, behind its days.
 * mcf_plan_below_prepare computes that state: complete = 0 a damping-depth pre-pass over the soil-moisture series, complete = 1
 * a first sweep of the solver over every day (chunks of ring_days through slot 0).  Array forcing: it streams the forcing of
 * `in` through slot 0 (upload the chunks' forcing again afterwards); `in` may be NULL otherwise.  Then mcf_plan_run_days runs
 * chunks in day order from day 0 (a chunk starting at day 0 begins a new pass) and each leaves the final Tz — the bits of the
 * whole-series plan's mcf_plan_belowground — in its slot for mcf_plan_fetch*, mcf_plan_fetch_cells, mcf_plan_fetch_packed and
 * mcf_nc_write_plan.  Running days before the prepare, out of order or with a gap is MCF_ERR_STATE; the refusals of below-ground
 * plans (a tile mask, a cell subset, a day offset inside the slot) hold as for mcf_plan_create.  mcf_plan_bytes reports the
 * device bytes either plan holds.  The one-shot entries take this route for reqhgt < 0 when the whole-series plan does not fit
 * in free HBM (MCF_BELOW_STREAM=1 forces it, =0 forbids it). */
int mcf_plan_create_streamed(const mcf_grid_inputs *in, const mcf_options *opt,
                             int32_t ring_days, int32_t ring_slots, mcf_plan **plan);
int mcf_plan_below_prepare(mcf_plan *plan, const mcf_grid_inputs *in);
/* A streamed below-ground plan over a subset of its days (vector forcing), before mcf_plan_below_prepare: `days` = n whole days
 * of the plan's series, strictly ascending.  From then on the series Tbelowgroundv sees is those days joined end to end
 * (24 n steps, no steps behind the last day): the damping-depth mean, the hourly sum, the daily means and the 47-step windows
 * run over the subset in its order, across the gaps of the calendar, while forcing, vegetation layer and the point model's
 * Tg / Tbp are read at each day's own place — the bits of a whole-series plan made from inputs subset to those days (whose
 * maximum air temperature mcf_plan_set_mxtc supplies).  mcf_plan_below_prepare sweeps the subset's days only.
 * mcf_plan_run_days(day0, ndays, slot) then runs the subset's days inside the calendar range [day0, day0 + ndays), each at its
 * own place day - day0 of the slot (the other days of the slot are not touched); the ranges have to take the subset in order
 * from its first day without leaving one out ("day order", MCF_ERR_STATE), and a range that holds none of its days does
 * nothing.  MCF_ERR_STATE after the prepare, on a plan that is not streamed below ground or has array forcing; MCF_ERR_ARG for
 * a list that is empty, unsorted, repeats a day or leaves the series. */
int mcf_plan_below_set_days(mcf_plan *plan, const int32_t *days, int32_t n);
/* The host bookkeeping of the above, no device needed: checks `days` (as mcf_plan_below_set_days does, against a series of
 * total_days whole days) and gives the subset positions [*pos0, *pos0 + *npos) whose days lie in the calendar range
 * [day0, day0 + ndays); *npos = 0: none. */
int mcf_below_days_range(const int32_t *days, int32_t n, int32_t total_days, int32_t day0, int32_t ndays, int32_t *pos0,
                         int32_t *npos);
/* Below ground at several depths from one solve.  Below ground the solver's work does not depend on the depth (reqhgt2 =
 * max(reqhgt, 1e-5); Tg, the damping depth and soilm read neither paia nor leafden); only the tail of Tbelowgroundv does: the
 * window length n = round(-118.35 reqhgt / meanD), the circular n/24-day means and, complete = 0, the point model's Tbp.
 * mcf_plan_below_set_depths hands a streamed below-ground plan that was created with Tz requested a list of depths, before
 * mcf_plan_below_prepare: depths[d] < 0 in any order (a depth may repeat), 1 <= ndepths <= MCF_MAX_DEPTHS.  The list replaces
 * opt.reqhgt for everything Tbelowgroundv does.  tbp: [ndepths][tsteps], the point model's soil temperature at each depth
 * (pointm$Tbp of a run at that depth); read only with complete = 0, where NULL is MCF_ERR_ARG.  The prepare and
 * mcf_plan_run_days keep their contracts (day order from day 0, the steps behind the last whole day); the damping-depth sum,
 * the hourly sum, the daily means, the 47-step windows and the chunk's Tg are shared by all depths, and per depth there is one
 * row of circular means (days x cells, complete = 1) and one Tz slab per ring slot.  Slab 0 is the slot's own Tz:
 * mcf_plan_fetch*, mcf_plan_fetch_packed and mcf_nc_write_plan see depths[0] there.  Every depth's Tz has the bits of a
 * single-depth run at that depth.
 * MCF_ERR_STATE: a plan that is not streamed below ground (the whole-series plan of mcf_plan_create refuses depth lists and
 * below-ground summaries alike), a plan without Tz, a call after the prepare or a second call, a plan with a day subset
 * (mcf_plan_below_set_days; that call in turn refuses a plan with a depth list).  MCF_ERR_ARG: a null, empty or too long list, a
 * depth >= 0 or NaN, a null tbp with complete = 0, array forcing (fine or coarse) together with complete = 0 — per-cell Tbp for
 * several depths is not taken.  Every message starts with the entry's name. */
#define MCF_MAX_DEPTHS 8
int mcf_plan_below_set_depths(mcf_plan *plan, const double *depths, int32_t ndepths, const double *tbp);
/* mcf_plan_fetch / mcf_plan_fetch_pitched for depth `depth` (0 .. ndepths - 1; a plan without a list has depth 0 alone) of a
 * streamed below-ground plan's Tz. */
int mcf_plan_fetch_depth(mcf_plan *plan, int32_t slot, int32_t depth, int64_t step0, int64_t nsteps, double *host_dst);
int mcf_plan_fetch_depth_pitched(mcf_plan *plan, int32_t slot, int32_t depth, int64_t step0, int64_t nsteps, double *host_dst,
                                 int64_t row_pitch);
/* One call, host to host: a streamed plan at depths[0] (opt->reqhgt is ignored), the depths set, the prepare, the chunks in
 * order.  opt->out is ignored: Tz at every depth and, where out->soilm is not NULL, soilm.  tz[d]: caller-allocated [rows, cols,
 * tsteps] per depth, the steps behind the last whole day included (soilm's are NA there).  Chunks of opt->days_per_chunk days
 * (0: sized from free device memory, the depth slabs counted).  Vector forcing with or without dfsel for complete 0 and 1;
 * array and coarse array forcing for complete = 1.  The refusals of mcf_plan_below_set_depths that need no plan come before a
 * device is needed; a series shorter than a day is MCF_ERR_ARG. */
typedef struct mcf_depth_outputs {
    double *tz[MCF_MAX_DEPTHS];
    double *soilm;                 /* or NULL */
} mcf_depth_outputs;
int mcf_runmicro_depths(const mcf_grid_inputs *in, const mcf_options *opt, const double *depths, int32_t ndepths,
                        const double *tbp, mcf_depth_outputs *out);
int mcf_plan_sync(mcf_plan *plan);

/* Copy `nsteps` time steps of variable `var` from ring slot `slot` (starting at
 * step `step0` within the slot) to host memory. */
int mcf_plan_fetch(mcf_plan *plan, int32_t slot, int32_t var, int64_t step0,
                   int64_t nsteps, double *host_dst);
/* ... into a row block of a taller column-major array (row_pitch rows per column; 0 = dense). */
int mcf_plan_fetch_pitched(mcf_plan *plan, int32_t slot, int32_t var, int64_t step0,
                           int64_t nsteps, double *host_dst, int64_t row_pitch);
/* Sparse read-back for verification and point queries: `nsteps` steps of variable `var` for the `ncells`
 * cells listed in `cells` (0-based column-major cell indices i + rows*j, any order), gathered on the device
 * and returned as host_dst[ci + ncells*k].  Moves ncells*nsteps values instead of a whole [rows,cols,nsteps]
 * slab (bench.py checks a sample of the timed run's last ring slot against the oracle with it). */
int mcf_plan_fetch_cells(mcf_plan *plan, int32_t slot, int32_t var, int64_t step0, int64_t nsteps,
                         const int64_t *cells, int64_t ncells, double *host_dst);
/* The same, packed as `writetonc` stores it (R/dataprep.R:1064-1069 `atonc`, :1158-1167): int32
 * round-half-even(value * scale), transposed per step to [cols, rows] (east fastest), NA ->
 * NA_integer_ (INT32_MIN; ncvar_put writes the variable's missval -9999 for it).  writetonc's scales:
 * 100 for Tz, tleaf, soilm, windspeed; 1 for relhum and the radiation terms.  Halves the bytes that
 * cross PCIe and arrives in the file's layout.  `kernel_ms` (optional) receives the device time of the
 * pack kernel. */
int mcf_plan_fetch_packed(mcf_plan *plan, int32_t slot, int32_t var, int64_t step0, int64_t nsteps,
                          double scale, int32_t *host_dst, float *kernel_ms);
/* ---- writetonc sink ---------------------------------------------------------------------
 * Replaces `writetonc(mout, fileout, dtm, reqhgt, vars)` (R/dataprep.R:1063-1260; called per tile by
 * runmicro_big, R/Cppwrappers.R:531): the solver's outputs as int32 (x100 for Tz, tleaf, soilm,
 * windspeed; x1 for relhum and the radiation terms; round half even; NA -> missval -9999) on the
 * dimensions east, north, time, with writetonc's variable names, long names, units, `crs` variable and
 * time attributes.  Two containers (`format`):
 *   MCF_NC_CLASSIC  netCDF classic, 64-bit offsets, `time` as the record dimension, uncompressed — needs nothing on the
 *                   host and streams at disk speed (mcf_ncfile.hpp); every netCDF reader opens it like the reference's file;
 *   MCF_NC_NETCDF4  the reference's own container (ncvar_def(..., compression = 9), dataprep.R:1110-1111): HDF5 laid out by
 *                   the netCDF-4 conventions, chunked [1 step][row strip][cols], deflate `deflate_level`; written through
 *                   the host's HDF5 library, bound at run time (MCF_ERR_ARG with the reason if there is none), the chunks
 *                   deflated by a team of host threads (mcf_nc4file.hpp).
 * Both take the same records (the device packs them once, k_pack_nc).  The dataset keeps writetonc's orientation: north[i] belongs to raster row i,
 * with `north` the ASCENDING northings of dataprep.R:1073 (the reference does not flip the rows).
 *
 * `vars[v]` selects solver output v (MCF_OUT order); writetonc defines Tz, tleaf, relhum, soilm,
 * windspeed and the five radiation terms for reqhgt > 0, Tz, soilm and radiation for reqhgt == 0, Tz and
 * soilm below ground — anything else is MCF_ERR_ARG.  `reference_puts_only` = 1 reproduces the file the
 * reference really produces: its `ncvar_put` guards test names ("raddir", …) that never occur in `vars`
 * (dataprep.R:1163-1167) and the soilm put refers to an undefined object (:1161), so those variables
 * are defined but hold missval throughout; 0 writes what was evidently meant. */
enum { MCF_NC_CLASSIC = 0, MCF_NC_NETCDF4 = 1 };
typedef struct mcf_nc_spec {
    int32_t rows, cols;          /* raster rows (= length of north), columns (= length of east) */
    int64_t nsteps;
    const double *east;          /* [cols]  seq(xmin + res/2, xmax - res/2, res)                 */
    const double *north;         /* [rows]  seq(ymin + res/2, ymax - res/2, res)                 */
    const double *time_hours;    /* [nsteps] hours since 1970-01-01 00:00                        */
    const char *crs_wkt;         /* crs(dtm); may be NULL                                        */
    double reqhgt;
    int32_t vars[MCF_NOUT];
    int32_t reference_puts_only;
    int32_t format;              /* MCF_NC_CLASSIC (0) or MCF_NC_NETCDF4                                    */
    int32_t deflate_level;       /* MCF_NC_NETCDF4: 0 = writetonc's compression = 9, 1..9, -1 = none      */
} mcf_nc_spec;
typedef struct mcf_ncfile mcf_ncfile;
/* Host only (no device needed): create the file with header, coordinates and room for every record. */
int mcf_nc_create(const char *path, const mcf_nc_spec *spec, mcf_ncfile **nc);
/* Host only: records [step0, step0+nsteps) from host arrays; vars[v] = [rows, cols, nsteps] column-major
 * doubles as mcf_runmicro1..4 return them (NULL for variables the file does not hold). */
int mcf_nc_write_host(mcf_ncfile *nc, int64_t step0, int64_t nsteps, const double *const vars[MCF_NOUT]);
/* Records [file_step0, file_step0+nsteps) straight from a plan's ring slot: packed, transposed and
 * byte-ordered on the device (k_pack_nc, 4 B per value over PCIe instead of 8), written to the file
 * while the next piece is being packed and copied. */
int mcf_nc_write_plan(mcf_ncfile *nc, mcf_plan *plan, int32_t slot, int64_t slot_step0, int64_t file_step0,
                      int64_t nsteps, float *kernel_ms);
int mcf_nc_close(mcf_ncfile *nc);

/* Device address of a ring slot variable, for device-side consumers, and the layout it is to be read with.
 * reqhgt >= 0: the ring is TILED — the values k_solve's workgroup produces for one variable on one day (cells_per_tile
 * consecutive cells x 24 hours) are one block of block_doubles doubles in the workgroup's lane order, so that the solver
 * stores whole 128-byte lines of one contiguous run per tile and day instead of 240 row segments 8 B x cells apart.
 * Value (cell c, step k of the slot) of the variable is at dev_ptr[mcf_ring_index(layout, c, k)]:
 *   (c / cells_per_tile) * tile_stride + (k / 24) * day_stride + pos(c % cells_per_tile, k % 24),
 *   pos(cell, h) = h * cells_per_tile + cell, except for 21-cell tiles:
 *   64 * (h / 3) + (cell < 16 ? 16 * (h % 3) + cell : 48 + 5 * (h % 3) + cell - 16).
 * reqhgt < 0 (tiled == 0): linear, dev_ptr[c + cells * k], the reference's layout. */
int mcf_plan_slot_ptr(mcf_plan *plan, int32_t slot, int32_t var, void **dev_ptr);
typedef struct mcf_ring_layout {
    int32_t tiled;            /* 0: linear [step][cell]                                  */
    int32_t cells_per_tile;
    int32_t block_doubles;    /* doubles per (tile, day, variable) block                 */
    int32_t slot_days;
    int64_t cells;            /* rows * cols                                             */
    int64_t tile_stride;      /* doubles between consecutive tiles                       */
    int64_t day_stride;       /* doubles between consecutive days of a tile              */
} mcf_ring_layout;
int mcf_plan_ring_layout(mcf_plan *plan, mcf_ring_layout *layout);
/* Host-side index helper (no device needed); -1 when (cell, step) is outside the slot. */
int64_t mcf_ring_index(const mcf_ring_layout *layout, int64_t cell, int64_t step);

/* ---- staged model outputs: the solver's own intermediates ----------------------------------------------------------------
 * What the reference's staged workflow (twostream / wind / soiltemp, src/microclimfCpp.cpp:1545-2046, cited as cpp:LINE)
 * shows of a run: thirteen fp64 diagnostics per cell-step.  They are the COMPILED path's values — the very ones that
 * produce the ten outputs of the same run (one solar position per time step, runmicro1Cpp's soil moisture clamp) — not the
 * R-mode re-derivation, which takes the solar position per cell and clamps soil moisture differently.  NA cells, steps
 * outside every vegetation layer of a layered run and (one-shot entries) steps beyond the last whole day hold NA_real_,
 * like the ten outputs. */
enum mcf_diag {
    MCF_DIAG_SI = 0,       /* "si"      solar index after the horizon test                      cpp:2218-2223            */
    MCF_DIAG_RADGSW = 1,   /* "radGsw"  short wave absorbed by the ground                       cpp:1131 (bare: 1148)    */
    MCF_DIAG_RADGLW = 2,   /* "radGlw"  long wave absorbed by the ground                        cpp:1165-1175            */
    MCF_DIAG_RADCSW = 3,   /* "radCsw"  short wave absorbed by the canopy                       cpp:1136 (bare: 1149)    */
    MCF_DIAG_RADCLW = 4,   /* "radClw"  long wave absorbed by the canopy (bare: radGlw)         cpp:1170 / 1174          */
    MCF_DIAG_RADLSW = 5,   /* "radLsw"  short wave absorbed by a leaf at reqhgt                 cpp:1151-1162            */
    MCF_DIAG_RADLPAR = 6,  /* "radLpar" PAR absorbed by a leaf at reqhgt; both exactly 0 at night and for pai == 0       */
    MCF_DIAG_LWOUT = 7,    /* "lwout"   0.97 sb (tc + 273.15)^4                                 cpp:1166                 */
    MCF_DIAG_UF = 8,       /* "uf"      friction velocity                                       cpp:1189-1196            */
    MCF_DIAG_GHA = 9,      /* "gHa"     convective conductance                                  cpp:1217                 */
    MCF_DIAG_T0 = 10,      /* "T0"      ground surface temperature (Tg of soiltemp_hrCpp)       cpp:1277-1296            */
    MCF_DIAG_G = 11,       /* "G"       ground heat flux after its +-0.6 Rmx clamp              cpp:1290                 */
    MCF_DIAG_KDDG = 12,    /* "kDDg"    damping depth                                           cpp:1249-1260            */
    MCF_NDIAG = 13
};
/* Switches a plan's diagnostics on: sel[d] != 0 selects diagnostic d.  Call it after the create and before the first run
 * (MCF_ERR_STATE afterwards, or when called twice); it allocates a second device ring beside the output ring (MCF_ERR_NOMEM
 * like that one).  From then on mcf_plan_run_days / mcf_plan_run_days_at fill both rings; the ten outputs keep their bits.
 * For plans with vector forcing (static or layered vegetation) and reqhgt >= 0.  MCF_ERR_ARG with a message for array and
 * coarse forcing, reqhgt < 0, streamed plans and an empty selection; on a diagnostics plan mcf_plan_run_days_masked with a
 * mask and mcf_plan_run_days_cells return MCF_ERR_ARG, and the snow run's and the `_multi` entries' plans never enable it. */
int mcf_plan_diag_enable(mcf_plan *plan, const int32_t sel[MCF_NDIAG]);
/* steps [step0, step0 + nsteps) of a selected diagnostic in ring slot `slot` as [rows, cols, nsteps], like mcf_plan_fetch */
int mcf_plan_diag_fetch(mcf_plan *plan, int32_t slot, int32_t dvar, int64_t step0, int64_t nsteps, double *host_dst);
/* Device address of a selected diagnostic of a ring slot and the diagnostics ring's layout: the output ring's geometry
 * (always tiled; its own day stride — one block per SELECTED diagnostic), to be read with mcf_ring_index. */
int mcf_plan_diag_slot_ptr(mcf_plan *plan, int32_t slot, int32_t dvar, void **dev_ptr);
int mcf_plan_diag_ring_layout(mcf_plan *plan, mcf_ring_layout *layout);
/* One-shot, host to host: mcf_runmicro1 / mcf_runmicro3 with the selected diagnostics beside the requested outputs, in day
 * chunks through the device.  diag_out->var[d]: caller-allocated [rows, cols, tsteps] for every selected d.  reqhgt >= 0. */
typedef struct mcf_diag_outputs {
    double *var[MCF_NDIAG];
} mcf_diag_outputs;
int mcf_runmicro1_diag(const mcf_grid_inputs *in, const mcf_options *opt, const int32_t sel[MCF_NDIAG], mcf_outputs *out,
                       mcf_diag_outputs *diag_out);
int mcf_runmicro3_diag(const mcf_grid_inputs *in, const mcf_options *opt, const int32_t sel[MCF_NDIAG], mcf_outputs *out,
                       mcf_diag_outputs *diag_out);
/* Array weather (array_forcing 1: fine arrays; 2: coarse arrays interpolated in the solver, with or without altcorrect).
 * mcf_plan_diag_enable_array is mcf_plan_diag_enable for such a plan: the same ring, layout, fetch, slot_ptr, ring_layout,
 * pass-2 rule and state rules.  MCF_ERR_ARG on a vector-forcing plan (use mcf_plan_diag_enable), reqhgt < 0, streamed plans and
 * an empty selection; MCF_ERR_STATE after the first run or on a second enable; tile masks and cell subsets are refused on the
 * plan as above.  mcf_runmicro2_diag / mcf_runmicro4_diag: mcf_runmicro2 / mcf_runmicro4 (fine or coarse as `in` says) with the
 * selected diagnostics beside the outputs, the forcing streamed in day chunks.  reqhgt >= 0. */
int mcf_plan_diag_enable_array(mcf_plan *plan, const int32_t sel[MCF_NDIAG]);
int mcf_runmicro2_diag(const mcf_grid_inputs *in, const mcf_options *opt, const int32_t sel[MCF_NDIAG], mcf_outputs *out,
                       mcf_diag_outputs *diag_out);
int mcf_runmicro4_diag(const mcf_grid_inputs *in, const mcf_options *opt, const int32_t sel[MCF_NDIAG], mcf_outputs *out,
                       mcf_diag_outputs *diag_out);

/* HIP-event timing on the plan's stream: start records an event, stop records
 * another, synchronises and returns the elapsed milliseconds between them. */
int mcf_plan_timer_start(mcf_plan *plan);
int mcf_plan_timer_stop(mcf_plan *plan, float *ms);
/* Accumulated device time (ms) and launch count of the solver kernel alone,
 * measured with per-launch HIP events when enabled. */
int mcf_plan_kernel_timing(mcf_plan *plan, int32_t enable);
int mcf_plan_kernel_stats(mcf_plan *plan, double *total_ms, int64_t *launches);

/* How the plan's launches were dispatched (vector forcing, reqhgt >= 0): the solver has two instantiations of its
 * clamps — one v_min_f64 / v_max_f64 each ("fast") for tiles whose cells' constants are all finite and in range, and the
 * reference's compare-and-select form for the others, for launches that contain a step with non-finite forcing, and for
 * tiles in which a fast wave met a NaN at a watched clamp (redone by a fix-up kernel).  Results are identical either way;
 * the counts are diagnostics (tests assert which path ran).  Synchronises the plan's stream. */
typedef struct mcf_dispatch_stats {
    int64_t fast_tiles, slow_tiles;   /* tiles per class (cells_per_block cells each)                    */
    int64_t irregular_days;           /* days with a non-finite / out-of-range forcing step             */
    int64_t fast_launches, slow_launches;
    int64_t canary_trips;             /* tiles redone by the fix-up kernel, summed over launches (one entry per
                                       * tile and launch, however many of its waves tripped)            */
} mcf_dispatch_stats;
int mcf_plan_dispatch_stats(mcf_plan *plan, mcf_dispatch_stats *stats);

/* ---- fused bioclim sink --------------------------------------------------------------
 * Replace _microclimf_runbioclim1Cpp / _microclimf_runbioclim2Cpp (bodies
 * src/microclimfCpp.cpp:3563-3588 / 3590-3616): the grid solver run with
 * out = {Tz | tleaf, soilm} followed by runbioclimCpp's per-cell reductions over time
 * (src/microclimfCpp.cpp:3245-3560).  Both stages stay on the device; only the requested
 * [rows,cols] matrices come back.  `opt->out` and `opt->complete` are ignored (the reference
 * passes its own mask and complete = true).  Time layout expected by the reference: steps
 * 0..287 twelve monthly days, 288..311 hottest day, 312..335 coldest day, then the quarter days
 * addressed by the 0-based index vectors. */
#define MCF_NBIO 19
typedef struct mcf_bioclim_sel {
    const int32_t *wetq, *dryq, *hotq, *colq; /* 0-based step indices                 */
    int32_t nwet, ndry, nhot, ncol;
    int32_t air;                              /* 1: Tz, 0: tleaf (runbioclim*Cpp `air`) */
    int32_t out[MCF_NBIO];                    /* bio1..bio19 requested                */
} mcf_bioclim_sel;
typedef struct mcf_bioclim_out {
    double *bio[MCF_NBIO]; /* each [rows,cols] or NULL; NA_real_ where the first step of Tz is NA */
} mcf_bioclim_out;
int mcf_runbioclim1(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel,
                    mcf_bioclim_out *out);
int mcf_runbioclim2(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel,
                    mcf_bioclim_out *out);
/* The time-varying-vegetation variants _microclimf_runbioclim3Cpp / 4Cpp (src/microclimfCpp.cpp:3620-3658 /
 * 3660-3700): vegetation arrays [rows, cols, 14] (deeper arrays: the first 14 layers) with the reference's fixed
 * dfsel of fourteen one-day layers; steps past the 336th belong to no layer and stay NA there too. */
int mcf_runbioclim3(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel,
                    mcf_bioclim_out *out);
int mcf_runbioclim4(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel,
                    mcf_bioclim_out *out);
/* The four over row blocks on several devices from one process (mcf_multi as for mcf_runmicro1_multi: the whole-raster twi
 * mean installed in every block, inputs read and the [rows, cols] results written in place through the row pitch): bit for
 * bit the single-device matrices. */
int mcf_runbioclim1_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel, const mcf_multi *multi,
                          mcf_bioclim_out *out);
int mcf_runbioclim2_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel, const mcf_multi *multi,
                          mcf_bioclim_out *out);
int mcf_runbioclim3_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel, const mcf_multi *multi,
                          mcf_bioclim_out *out);
int mcf_runbioclim4_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel, const mcf_multi *multi,
                          mcf_bioclim_out *out);
/* How the calling thread's last bioclim call ran: the number of solver chunk launches of the streamed sink (vector forcing
 * and coarse array forcing, array_forcing == 2, above ground with ascending quarter lists: the solver runs in day chunks and
 * nothing of size cells x steps is allocated), summed over the row blocks of a `_multi` call; 0: the whole-series route
 * (fine array forcing, reqhgt < 0, MCF_BIOCLIM_WHOLE set) or no call yet.  The matrices are the same bits either way: a
 * read-only observation, like mcf_plan_kernel_stats. */
int mcf_bioclim_last_chunks(void);
/* Soil bioclim variables at several depths from ONE streamed below-ground solve: mcf_runmicro_depths' driver (a streamed plan,
 * mcf_plan_below_set_depths, sweep 1, then the solver in day chunks) with each chunk folded on the device into 21 doubles of
 * running state per cell and depth and 8 per cell for the soil moisture, which below ground does not depend on the depth.
 * Nothing of size cells x steps exists on either side.  Every matrix has the bits of mcf_runbioclim1 / 3 / 2 (coarse) with
 * opt->reqhgt = depths[d] — the whole-series route, one solve per depth.
 *   opt      reqhgt, out and complete are ignored: the run is made at depths[0] with complete = 1, as runbioclim*Cpp pass it.
 *   sel      air must be 1 (Tz; tleaf does not exist below ground); out[v] selects as in mcf_runbioclim1; the quarter lists
 *            must be in ascending order (what runbioclim passes) — mcf_runbioclim1 keeps taking any order.
 *   in       vector forcing with static vegetation, or with in->veg_layers > 1: vegetation arrays [rows, cols, >= 14] under
 *            the fixed dfsel of mcf_runbioclim3 (steps past the 336th belong to no layer, as there); coarse array forcing
 *            (array_forcing == 2).  Fine array forcing (array_forcing == 1) is refused: mcf_runbioclim2 serves it.
 *            tsteps >= 336 in whole days.
 *   depths   as mcf_plan_below_set_depths: each < 0, any order, a depth may repeat, 1 <= ndepths <= MCF_MAX_DEPTHS.
 *   chunk_days  days per solver chunk; 0: sized from free device memory as mcf_runmicro_depths does.
 *   out      temp[d][v]: bio1..bio11 at depths[d]; moist[v]: bio12..bio19, once.  A selected variable with a null buffer — at
 *            any listed depth for bio1..bio11 — is MCF_ERR_ARG.  NA_real_ where the depth's first Tz is NA (bio1..bio11, each
 *            depth by its own first value) and where depths[0]'s is (bio12..bio19).
 * Every refusal that needs no plan comes before a device is touched; every message starts with the entry's name.
 * mcf_bioclim_last_chunks reports this entry's chunk launches of sweep 2. */
typedef struct mcf_bioclim_depths_out {
    double *temp[MCF_MAX_DEPTHS][11]; /* bio1..bio11 per depth, each [rows, cols] or NULL */
    double *moist[8];                 /* bio12..bio19, once: below ground soilm does not depend on the depth */
} mcf_bioclim_depths_out;
int mcf_runbioclim_depths(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_bioclim_sel *sel, const double *depths,
                          int32_t ndepths, int32_t chunk_days, mcf_bioclim_depths_out *out);

/* ---- period summaries --------------------------------------------------------------------------------------------------
 * Per-cell statistics of the solver's outputs over caller-defined periods (what users of the reference do with
 * apply(mout$Tz, c(1, 2), mean) and with monthly mean / minimum / maximum maps), accumulated on the device from each ring
 * chunk as it is produced: nothing of size cells x steps exists on either side.  For reqhgt >= 0 (the tiled ring).
 *
 * `summary`, defined here once.  A summary is
 *   - a table period_of_day[days of the plan], values 0 .. nperiods - 1, or -1 for a day that is not counted (periods need not
 *     be contiguous: "all Januaries" is a period);
 *   - a selection var[] of output variables, each one the plan was created with;
 *   - a selection stat[] of the six statistics below; HOURS_ABOVE takes one threshold per variable.
 * Per (cell, period, variable), over the counted days in ascending day order, v the value of a step:
 *   sum       s = s + v from s = 0, step by step in time order, in fp64, never reassociated;  MEAN = s / (24 days)
 *   MIN, MAX  the strict comparisons v < mn, v > mx in time order, from the period's first counted value
 *   MEAN_DAILY_MAX / _MIN  the day's maximum / minimum formed the same way over its 24 hours, added day by day from 0, then
 *             divided by `days`
 *   HOURS_ABOVE  the number of steps with v > threshold[var], as a double
 *   NA rule   if any value of the (cell, period, variable) is NaN — NA cells, days outside every vegetation layer — every
 *             statistic of it is NA_real_ (R's bit pattern), as is every statistic of a period without a counted day.
 * The result is a function of the ring's values alone: it does not depend on ring days, chunking, slot placement or tile size. */
enum mcf_stat {
    MCF_STAT_MEAN = 0,
    MCF_STAT_MIN = 1,
    MCF_STAT_MAX = 2,
    MCF_STAT_MEAN_DAILY_MAX = 3,
    MCF_STAT_MEAN_DAILY_MIN = 4,
    MCF_STAT_HOURS_ABOVE = 5,
    MCF_NSTAT = 6
};
typedef struct mcf_summary_spec {
    int32_t nperiods;
    const int32_t *period_of_day;  /* [tsteps / 24] */
    int32_t var[MCF_NOUT];         /* != 0: summarised                             */
    int32_t stat[MCF_NSTAT];       /* != 0: kept                                   */
    double threshold[MCF_NOUT];    /* HOURS_ABOVE; read for selected variables only */
} mcf_summary_spec;
/* Switches the sink on: allocates the state, nvars x nperiods x rows x cells x 8 bytes (rows: the sum's, and one per selected
 * statistic other than MEAN), MCF_ERR_NOMEM when it does not fit.  MCF_ERR_ARG with a message: reqhgt < 0 or a streamed plan, a
 * selected variable that was not requested at plan creation, an empty selection of variables or statistics, nperiods < 1, a
 * table entry outside -1 .. nperiods - 1, a NaN threshold of a selected variable with HOURS_ABOVE selected.  MCF_ERR_STATE when
 * called twice.  May be enabled on a diagnostics plan (it reads the ten outputs only). */
int mcf_plan_summary_enable(mcf_plan *plan, const mcf_summary_spec *spec);
/* Folds days [slot_day0, slot_day0 + ndays) of ring slot `slot` as calendar days [day0, day0 + ndays), on the plan's stream
 * behind the run that filled them (however it filled them: plain, masked or cell-subset runs).  Days arrive in ascending
 * order, each at most once: a day at or before one that has been folded is MCF_ERR_STATE, as is a call before the enable. */
int mcf_plan_summary_accumulate(mcf_plan *plan, int32_t slot, int32_t slot_day0, int32_t day0, int32_t ndays);
/* One statistic of one variable as [rows, cols, nperiods], column-major (both selected in the enable: MCF_ERR_ARG otherwise). */
int mcf_plan_summary_fetch(mcf_plan *plan, int32_t var, int32_t stat, double *host_dst);
/* days[nperiods]: the counted days folded so far into each period */
int mcf_plan_summary_days(mcf_plan *plan, int32_t *days);
/* Back to the state of the enable: nothing folded, any day may come next. */
int mcf_plan_summary_reset(mcf_plan *plan);
/* One call, host to host: the solver in day chunks through a ring of `chunk_days` days (0: sized from a byte budget of 14 GB,
 * MCF_SUMMARY_RING_GB overrides), each chunk folded as it is produced — vector forcing, array forcing (each chunk's forcing
 * uploaded before its run) and coarse array forcing, with or without dfsel, as `in` says.  The plan is created with
 * out = spec->var (`opt->out` is ignored); opt->reqhgt >= 0.  val[v][s]: caller-allocated [rows, cols, nperiods] for every
 * selected pair (a null one is MCF_ERR_ARG); days: [nperiods] or NULL. */
typedef struct mcf_summary_out {
    double *val[MCF_NOUT][MCF_NSTAT];
    int32_t *days;
} mcf_summary_out;
int mcf_runmicro_summary(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_summary_spec *spec, int32_t chunk_days,
                         mcf_summary_out *out);
/* The same over row blocks on several devices from one process (vector forcing; mcf_multi as for mcf_runmicro1_multi: the
 * whole-raster twi mean installed in every block, inputs read and results written in place through the row pitch): bit for
 * bit the single-device arrays. */
int mcf_runmicro_summary_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_summary_spec *spec, int32_t chunk_days,
                               const mcf_multi *multi, mcf_summary_out *out);
/* Period summaries below ground: the sink on a streamed below-ground plan (mcf_plan_create_streamed, reqhgt < 0), with or
 * without a depth list (without one: one depth, opt.reqhgt).  spec->var may select Tz and soilm (MCF_ERR_ARG otherwise); Tz is
 * kept per depth.  The summary, its state rows, the NA rule and the day-order rule are the ones defined above;
 * mcf_plan_summary_accumulate / _days / _reset work on such a plan as they do above ground (the fold reads each depth's slab of
 * the slot, behind the mcf_plan_run_days that filled it; the steps behind the last whole day belong to no day).  With a depth
 * list, mcf_plan_below_set_depths comes first.  mcf_plan_summary_enable itself keeps refusing streamed and below-ground plans,
 * and the whole-series plan (mcf_plan_create, reqhgt < 0) is refused here as there (MCF_ERR_STATE). */
int mcf_plan_summary_enable_below(mcf_plan *plan, const mcf_summary_spec *spec);
/* mcf_plan_summary_fetch for one depth's Tz; with var = MCF_OUT_SOILM the depth must be 0. */
int mcf_plan_summary_fetch_depth(mcf_plan *plan, int32_t depth, int32_t var, int32_t stat, double *host_dst);
/* One call, host to host, as mcf_runmicro_depths runs it, each chunk folded as it is produced: nothing of size cells x steps
 * exists on either side.  chunk_days = 0: sized from free device memory as mcf_runmicro_depths does.  tz[d][s] / soilm[s]:
 * caller-allocated [rows, cols, nperiods] for every depth and selected statistic (a null one is MCF_ERR_ARG); days: [nperiods]
 * or NULL. */
typedef struct mcf_depth_summary_out {
    double *tz[MCF_MAX_DEPTHS][MCF_NSTAT];
    double *soilm[MCF_NSTAT];
    int32_t *days;
} mcf_depth_summary_out;
int mcf_runmicro_depths_summary(const mcf_grid_inputs *in, const mcf_options *opt, const double *depths, int32_t ndepths,
                                const double *tbp, const mcf_summary_spec *spec, int32_t chunk_days, mcf_depth_summary_out *out);

/* ---- series sink --------------------------------------------------------------------------------------------------------
 * The sinks above reduce over time or keep everything; this one reduces over SPACE, or keeps the full hourly series at a few
 * cells: per-step statistics of the outputs over zones of the raster (terra::zonal / global(..., na.rm = TRUE) layer by layer)
 * and the series at logger sites, accumulated on the device from each ring chunk as it is produced.  For reqhgt >= 0 (the
 * tiled ring).  DESIGN.md §27.
 *
 * `series`, defined here once.  A series spec is
 *   - npoints cells[npoints]: int64, 0-based, row + rows * col, as mcf_plan_fetch_cells takes them;
 *   - nzones, 0 .. MCF_MAX_ZONES, and zone[rows * cols]: int32, column-major, -1 = in no zone, else 0 .. nzones - 1.  A point
 *     needs no zone; npoints or nzones may be 0, not both;
 *   - a selection var[] of output variables, each one the plan was created with;
 *   - a selection zstat[] of the four statistics below (read when nzones > 0).
 * Point series of a selected variable: [tsteps, npoints], column-major (each point's series contiguous); every step holds the
 * ring's value bit for bit, NA payload included; steps of days never folded, and steps behind the last whole day, are NA_real_.
 * Zone series of a selected (variable, statistic): [tsteps, nzones], column-major.  For one (zone z, step k, variable), over
 * the cells with zone == z: a NaN value is skipped (na.rm = TRUE); a value that is not NaN with !(|v| < 4096) is BAD (that covers
 * +-inf); n = the number of values neither skipped nor bad.
 *   COUNT   (double)n
 *   MEAN    ((double)S * 2^-24) / (double)n with S = sum of (int64)rint(v * 2^24) over the counted values, rint rounding half to
 *           even: an INTEGER sum, so it does not depend on order, tiling, chunking or device count.  Its distance from the exact
 *           mean of the counted values is at most 2^-25 (each term is off by at most 2^-25, so is their mean; (double)S is exact
 *           while |S| < 2^53 and rounds once beyond; the divide rounds once).  |v| < 4096 keeps |S| < 2^62 for up to 2^26 cells; a
 *           larger raster is MCF_ERR_ARG.
 *   MIN, MAX  the minimum / maximum of the counted values, with + 0.0 applied (a -0.0 never appears)
 *   If any value of the zone-step is bad, or n == 0, every statistic except COUNT is NA_real_ (with n == 0, COUNT is 0).
 *   Steps of days never folded, and steps behind the last whole day, are NA_real_ in every statistic.
 * The result is a function of the ring's values alone: it does not depend on ring days, chunking, slot placement, tile size or
 * the order in which days are folded. */
#define MCF_MAX_ZONES 64
enum mcf_zstat {
    MCF_ZSTAT_MEAN = 0,
    MCF_ZSTAT_MIN = 1,
    MCF_ZSTAT_MAX = 2,
    MCF_ZSTAT_COUNT = 3,
    MCF_NZSTAT = 4
};
typedef struct mcf_series_spec {
    int64_t npoints;
    const int64_t *cells;          /* [npoints]                                    */
    int32_t nzones;
    const int32_t *zone;           /* [rows * cols]; read when nzones > 0          */
    int32_t var[MCF_NOUT];         /* != 0: kept                                   */
    int32_t zstat[MCF_NZSTAT];     /* != 0: kept (nzones > 0)                      */
} mcf_series_spec;
/* Switches the sink on: allocates the point buffer, nvars x npoints x tsteps x 8 bytes, and the zone state, nvars x 4 x nzones x
 * whole days x 24 x 8 bytes (MCF_ERR_NOMEM when they do not fit).  MCF_ERR_ARG, the message starting with the entry's name:
 * reqhgt < 0 or a streamed plan, a selected variable the plan was not created with, an empty selection (no variable; neither
 * points nor zones; zones without a statistic), nzones > MCF_MAX_ZONES, a label outside -1 .. nzones - 1, a cell index outside
 * the raster, more than 2^26 cells.  MCF_ERR_STATE when called twice.  May be enabled beside the period summary and on a
 * diagnostics plan (it reads the ten outputs only). */
int mcf_plan_series_enable(mcf_plan *plan, const mcf_series_spec *spec);
/* Folds days [slot_day0, slot_day0 + ndays) of ring slot `slot` as calendar days [day0, day0 + ndays), on the plan's stream
 * behind the run that filled them.  Days may come in any order, each at most once: a second fold of a day is MCF_ERR_STATE,
 * as is a call before the enable. */
int mcf_plan_series_accumulate(mcf_plan *plan, int32_t slot, int32_t slot_day0, int32_t day0, int32_t ndays);
/* dst: [tsteps, npoints] / [tsteps, nzones], column-major (selected in the enable: MCF_ERR_ARG otherwise; MCF_ERR_STATE
 * before the enable) */
int mcf_plan_series_fetch_points(mcf_plan *plan, int32_t var, double *dst);
int mcf_plan_series_fetch_zones(mcf_plan *plan, int32_t var, int32_t zstat, double *dst);
/* Back to the state of the enable: nothing folded, any day may come next. */
int mcf_plan_series_reset(mcf_plan *plan);
/* One call, host to host, as mcf_runmicro_summary runs it (vector, fine array and coarse array forcing, with or without dfsel;
 * the plan is created with out = spec->var; chunk_days = 0: the same ring budget).  points[v]: caller-allocated
 * [tsteps, npoints] for every selected variable when npoints > 0; zones[v][s]: [tsteps, nzones] for every selected pair when
 * nzones > 0 (a null one is MCF_ERR_ARG). */
typedef struct mcf_series_out {
    double *points[MCF_NOUT];
    double *zones[MCF_NOUT][MCF_NZSTAT];
} mcf_series_out;
int mcf_runmicro_series(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_series_spec *spec, int32_t chunk_days,
                        mcf_series_out *out);
/* The zone series of a caller's host array x[rows, cols, nsteps] (column-major, any nsteps >= 1: the arrays mcf_runmicro*
 * returned, the snow series), by the same kernel: out[s] = [nsteps, nzones] for every selected statistic (a null one is
 * MCF_ERR_ARG).  The array goes through the device in pieces of whole days, tiled as the output ring is (32-cell tiles;
 * MCF_ZONAL_CPB = 16, 21, 32 or 42 overrides).  Refusals as for the enable, before a device is touched. */
int mcf_zonal_series(const double *x, int64_t rows, int64_t cols, int64_t nsteps, const int32_t *zone, int32_t nzones,
                     const int32_t zstat[MCF_NZSTAT], int32_t device, double *const out[MCF_NZSTAT]);
/* MCF_ZONAL_CPB = 0 takes another route to the same numbers: a column-major x[rows, cols, nsteps] IS step-major planes, so it
 * goes up in pieces of whole days without re-tiling and is folded by the planes kernel (below), a last day shorter than 24
 * steps included.  The default route does not change. */

/* ---- series sink: further sources ----------------------------------------------------------------------------
 * Everything of the block above holds unchanged for every source below: NaN skipped, !(|v| < 4096) BAD, the mean from the integer
 * sum of rint(v * 2^24), minimum and maximum with + 0.0 applied, a bad value or n == 0 makes everything but COUNT NA_real_,
 * steps never folded and steps behind the last whole day NA_real_ in every statistic (COUNT too), point series bit for bit.
 *
 * Row blocks.  The zone state of one (variable, zone, step) is four integers: S, the sum of rint(v * 2^24); a count word, its low
 * half the values kept (n), its high half the bad ones; the minimum and the maximum as order-preserving keys.  The state of a
 * raster cut into row blocks is the element-wise combination of the blocks' states: S adds, the count words add, the minimum
 * keys take the minimum, the maximum keys the maximum.  All of it is integer, so the result has the bits of the one-block
 * run, whatever the number of blocks or devices.  The finish (the divide and the NA rules) runs once, on the combined state.
 * The 2^26-cell limit is tested on the whole raster.  A point belongs to the block that holds its row.  The caller's cells[]
 * and zone[] are given for the whole raster (row + R * col; [R * cols], column-major); each block takes its rows of them.
 * The combination is a host loop over the blocks' fetched states (a few MB); the two functions below are that loop and the
 * finish, as pure host functions: state [4][nzones][steps] of int64 in the order S, count word, minimum key, maximum key
 * (untouched: 0, 0, INT64_MAX, INT64_MIN; key of a value: its bits if they are >= 0 as int64, else bits ^ INT64_MAX).
 * finish: out [nsteps, nzones], column-major; steps >= `steps`, and steps of days with day_done[day] == 0 (NULL: all done), NA. */
int mcf_series_state_merge(int64_t *into, const int64_t *from, int32_t nzones, int64_t steps);
int mcf_series_state_finish(const int64_t *state, int32_t nzones, int64_t steps, int64_t nsteps, const int32_t *day_done,
                            int32_t zstat, double *out);
/* The one-call form over row blocks on several devices from one process, as mcf_runmicro_summary_multi (vector forcing):
 * bit for bit mcf_runmicro_series' results. */
int mcf_runmicro_series_multi(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_series_spec *spec, int32_t chunk_days,
                              const mcf_multi *multi, mcf_series_out *out);
/* Below ground: the sink on a streamed below-ground plan (mcf_plan_create_streamed, reqhgt < 0), after
 * mcf_plan_below_set_depths if there is a depth list.  spec->var may select Tz and soilm (MCF_ERR_ARG otherwise); Tz is kept per
 * depth, soilm has depth 0 alone, as mcf_plan_summary_enable_below lays out its places.  mcf_plan_series_accumulate / _reset
 * work on such a plan as above ground (the fold reads each depth's slab of the slot).  The whole-series plan (mcf_plan_create,
 * reqhgt < 0) is refused (MCF_ERR_STATE), and mcf_plan_series_enable keeps refusing streamed and below-ground plans.
 * fetch_*_depth: mcf_plan_series_fetch_* for one depth's Tz; with var = MCF_OUT_SOILM the depth must be 0; a depth outside the
 * list is MCF_ERR_ARG. */
int mcf_plan_series_enable_below(mcf_plan *plan, const mcf_series_spec *spec);
int mcf_plan_series_fetch_points_depth(mcf_plan *plan, int32_t depth, int32_t var, double *dst);
int mcf_plan_series_fetch_zones_depth(mcf_plan *plan, int32_t depth, int32_t var, int32_t zstat, double *dst);
/* One call, host to host, as mcf_runmicro_depths_summary drives the plan.  tz_points[d] / soilm_points: [tsteps, npoints] when
 * npoints > 0; tz_zones[d][s] / soilm_zones[s]: [tsteps, nzones] for every depth and selected statistic when nzones > 0 (a
 * null one of a selected variable is MCF_ERR_ARG). */
typedef struct mcf_depth_series_out {
    double *tz_points[MCF_MAX_DEPTHS];
    double *tz_zones[MCF_MAX_DEPTHS][MCF_NZSTAT];
    double *soilm_points;
    double *soilm_zones[MCF_NZSTAT];
} mcf_depth_series_out;
int mcf_runmicro_depths_series(const mcf_grid_inputs *in, const mcf_options *opt, const double *depths, int32_t ndepths,
                               const double *tbp, const mcf_series_spec *spec, int32_t chunk_days, mcf_depth_series_out *out);

/* ---- terrain pre-compute (the solver's terrain inputs, built on the device) ------
 * Restates the R-side arithmetic of the reference's marshaller (R/internal.R):
 *   hor   = .horizon(dtm, 15*d), d = 0..23            R/internal.R:909-925, 1144
 *   svfa  = 0.5*cos(2*tan(mean(atan(hor))))+0.5       R/internal.R:1147-1148
 *   wsa   = .windsheltera(dtm, zref, s)               R/internal.R:949-991
 *   slope, aspect = terra::terrain (Horn), NA -> 0    R/internal.R:1124-1136
 * `dtm` is the caller's row block of the raster plus `halo_north` / `halo_south` extra rows
 * (column-major [(halo_north+rows+halo_south), cols]).  Outside the raster the reference's
 * zero padding applies; inside it a block needs 100 halo rows for hor/svfa and
 * 100 + 2.5*s for wsa (or every row up to the raster edge).  Outputs cover the own rows only
 * and may be NULL individually.  rows_total = 0 means "the block is the whole raster". */
typedef struct mcf_terrain_in {
    int64_t rows, cols;
    int32_t halo_north, halo_south;
    const double *dtm;
    double res;           /* cell size (m)                                   */
    double zref;          /* wind-shelter height, .windsheltera's whgt       */
    int32_t agg;          /* .windsheltera's s (0 -> 10)                     */
    int32_t reserved0;
    int64_t row0, rows_total;
} mcf_terrain_in;

typedef struct mcf_terrain_out {
    double *slope, *aspect; /* [rows,cols]    degrees                        */
    double *hor;            /* [rows,cols,24] tan(horizon angle)             */
    double *svfa;           /* [rows,cols]                                   */
    double *wsa;            /* [rows,cols,8]                                 */
} mcf_terrain_out;

int mcf_precompute_terrain(const mcf_terrain_in *in, const mcf_terrain_out *out, int32_t device);
/* The same for a WHOLE raster (no halos, no placement in `in`) over several devices from one process — the companion of
 * mcf_runmicro1_multi for BASELINE configs[3]'s geometry: contiguous row blocks, block b on devices[b % n_devices], each
 * with the halo rows its stencils need gathered out of the caller's array (the rows the one-process-per-GPU route exchanges
 * between ranks), results written into the caller's arrays in place.  n_devices = 0: every visible device; n_blocks = 0: one
 * block per device (more blocks than devices are time-sliced).  The values are those of the single-device call. */
int mcf_precompute_terrain_multi(const mcf_terrain_in *in, const mcf_terrain_out *out, const mcf_multi *multi);

/* ---- plans and one-shot solves that take the dtm --------------------------------------------------------------------------
 * What the solver needs that is a function of the elevation raster alone, built on the device straight into the plan's own
 * buffers: each of in->soilc.{slope, aspect, hor, svfa, wsa, twi} may be NULL and is then derived from `dtm` (no host copy in
 * either direction); one that is given is uploaded as by mcf_plan_create.  The derived values are those of the host route, bit
 * for bit: mcf_precompute_terrain with zref = opt->zref (slope and aspect NaN where the dtm is NA) and mcf_topidx_device.  With
 * `hor` given and `svfa` not, svfa comes from the given hor (R/internal.R:1146-1149).  The terrain planes need square cells
 * (xres == yres) and, for a row block of a larger raster (rows_total > rows), the halo rows mcf_precompute_terrain asks for;
 * flow accumulation does not tile: a row block must bring its twi.  Nothing of the dtm or of the scratch stays allocated:
 * mcf_plan_bytes equals that of the plan created from host arrays.
 * mcf_runmicro_dtm is mcf_runmicro1 .. 4 (by in->array_forcing / in->veg_layers) on such a plan.  With `multi` (NULL: one
 * device, opt->device) the raster — the whole one: no halos, no placement — goes in row blocks over the listed devices as by
 * mcf_runmicro1_multi: twi is derived once for the whole raster on the first device, every block derives its terrain from its
 * dtm rows plus halos on its own device.  Same bits as the single-device call. */
typedef struct mcf_dtm_spec {
    const double *dtm;                 /* [(halo_north + rows + halo_south), cols] column-major, NaN = NA */
    int32_t halo_north, halo_south;    /* as mcf_terrain_in */
    int64_t row0, rows_total;          /* 0, 0: the block is the whole raster */
    double xres, yres;
    int32_t agg, reserved0;            /* .windsheltera's s, 0 -> 10 */
} mcf_dtm_spec;
int mcf_plan_create_dtm(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_dtm_spec *dtm,
                        int32_t ring_days, int32_t ring_slots, mcf_plan **plan);
int mcf_runmicro_dtm(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_dtm_spec *dtm,
                     const mcf_multi *multi /* NULL: one device */, mcf_outputs *out);

/* ---- snow branch ----------------------------------------------------------------------
 *   mcf_gridmodelsnow1/2()  replace  _microclimf_gridmodelsnow1 / _microclimf_gridmodelsnow2
 *                           src/RcppExports.cpp:483-514  (R stubs R/RcppExports.R:108-114,
 *                           bodies src/microclimfCpp.cpp:4172-4423 / 4426-4673): the per-cell,
 *                           sequential-in-time snowpack energy and mass balance (snowoneB,
 *                           src/microclimfCpp.cpp:3835-3972) that `.snowmodel1/2` call once per
 *                           5-day chunk (R/internal.R:2587).
 *   mcf_gridmicrosnow1/2()  replace  _microclimf_gridmicrosnow1 / _microclimf_gridmicrosnow2
 *                           src/RcppExports.cpp:542-578  (R stubs R/RcppExports.R:124-130,
 *                           bodies src/microclimfCpp.cpp:4894-5056 / 5059-5214): the microclimate
 *                           of snow-covered cell-steps, written over the no-snow solver's output
 *                           (`.runmicrosnow1/2`, R/internal.R:3625).
 * Vector forcing (…1): climate and pointm entries are [tsteps]; array forcing (…2): they are
 * [rows,cols,tsteps] except winddir, and lats/lons replace lat/lon. */
enum { /* snowdenp's snow environments (src/microclimfCpp.cpp:3741-3749); any other name = Alpine */
    MCF_SNOWENV_ALPINE = 0, MCF_SNOWENV_MARITIME = 1, MCF_SNOWENV_PRAIRIE = 2, MCF_SNOWENV_TUNDRA = 3,
    MCF_SNOWENV_TAIGA = 4
};
/* Maps the reference's `snowenv` string to the enum (exact, case-sensitive match as in the reference). */
int32_t mcf_snowenv_from_name(const char *name);

/* climdata columns temp, relhum, pres, swdown, difrad, lwdown, windspeed, winddir, precip
 * (src/microclimfCpp.cpp:4206-4214; gridmicrosnow2 names the last one "prec", :5083) and, for
 * gridmicrosnow only, umu (:4911). */
typedef struct mcf_snow_climate {
    const double *temp, *relhum, *pres, *swdown, *difrad, *lwdown, *windspeed, *winddir, *precip, *umu;
} mcf_snow_climate;
/* pointm of gridmodelsnow (src/microclimfCpp.cpp:4181-4186): output of pointmodelsnow.  `tr` is
 * only used for its length (ndays = tr.size()/24, :4231) and is not part of this ABI. */
typedef struct mcf_snow_pointm {
    const double *Gp, *Tc, *RswabsG, *RlwabsG, *umu;
} mcf_snow_pointm;
/* vegp (src/microclimfCpp.cpp:4188-4191; gridmicrosnow adds paia, leafd, leafden :4913-4919). */
typedef struct mcf_snow_vegp {
    const double *pai, *hgt, *leaft, *clump; /* [rows,cols] */
    const double *paia, *leafd, *leafden;    /* gridmicrosnow only */
} mcf_snow_vegp;
/* other (src/microclimfCpp.cpp:4193-4204, :4921-4929). */
typedef struct mcf_snow_other {
    const double *slope, *aspect, *skyview; /* [rows,cols]                                   */
    const double *wsa;                      /* [rows,cols,8]                                 */
    const double *hor;                      /* [rows,cols,24]                                */
    double lat, lon;                        /* vector forcing                                */
    const double *lats, *lons;              /* array forcing, [rows,cols]                    */
    double zref;
    const double *isnowdc, *isnowdg;        /* gridmodelsnow: initial snow depth (m)         */
    const int32_t *isnowac, *isnowag;       /* gridmodelsnow: initial snow age (h), IntegerMatrix */
    const double *Smax;                     /* gridmicrosnow: written to soilm under snow    */
} mcf_snow_other;
typedef struct mcf_snow_inputs {
    int64_t rows, cols, tsteps;
    int32_t array_forcing;
    int32_t snowenv; /* MCF_SNOWENV_* (gridmodelsnow only) */
    mcf_obstime obstime;
    mcf_snow_climate clim;
    mcf_snow_pointm pointm; /* gridmodelsnow only */
    mcf_snow_vegp vegp;
    mcf_snow_other other;
} mcf_snow_inputs;
/* Returned list of gridmodelsnow (src/microclimfCpp.cpp:4412-4422): Tc, Tg, sdepc, sdepg, sden are
 * [rows,cols,tsteps]; agec, ageg, meltc, meltg are [rows,cols].  Any pointer may be NULL (not
 * wanted).  Cells with NA hgt hold NA_real_ everywhere. */
typedef struct mcf_snowmodel_out {
    double *Tc, *Tg, *sdepc, *sdepg, *sden;
    double *agec, *ageg, *meltc, *meltg;
} mcf_snowmodel_out;
int mcf_gridmodelsnow1(const mcf_snow_inputs *in, mcf_snowmodel_out *out, int32_t device);
int mcf_gridmodelsnow2(const mcf_snow_inputs *in, mcf_snowmodel_out *out, int32_t device);

/* snowm list of gridmicrosnow (src/microclimfCpp.cpp:4935-4939), each [rows,cols,tsteps]. */
typedef struct mcf_snowm {
    const double *Tc, *Tg, *totalSWE, *groundsnowdepth, *snowden;
} mcf_snowm;
/* `micro` holds the no-snow solver's output on entry and is updated IN PLACE for every cell-step
 * with totalSWE > 0 (src/microclimfCpp.cpp:4993-5038); only variables with out[v] != 0 are read
 * or written, their pointers must then be non-NULL. */
int mcf_gridmicrosnow1(const mcf_snow_inputs *in, const mcf_snowm *snowm, double reqhgt, double mat,
                       const int32_t out[MCF_NOUT], mcf_outputs *micro, int32_t device);
int mcf_gridmicrosnow2(const mcf_snow_inputs *in, const mcf_snowm *snowm, double reqhgt, double mat,
                       const int32_t out[MCF_NOUT], mcf_outputs *micro, int32_t device);

/* The chunk loop of `.snowmodel1` (R/internal.R:2553-2617) resident on the device: for every chunk of
 * `chunk_steps` hours (5 days) the terrain inputs are re-derived from dtm + ground snow depth
 * (slope/aspect with NA -> 0/180, hor x24, sky view, wsa with s = 10 if res <= 100 else 1:
 * R/internal.R:2566-2580 — the kernels of mcf_precompute_terrain), gridmodelsnow1 runs on the chunk
 * (:2587), snow-depth changes are redistributed by the topographic position index `.tpicalc`
 * (:2471-2485, 2589-2600) and depths / ages are fed back (:2607-2612).  Only the requested series cross
 * PCIe.  `base` carries obstime / clim / pointm for the whole series (vector forcing), vegp, and
 * other.{lat, lon, zref, isnowdc, isnowdg, isnowac, isnowag}; other.{slope, aspect, skyview, wsa, hor}
 * are ignored.  As in R, n5days = tsteps / chunk_steps chunks are run (`1:n5days` truncates; at least
 * one); later steps stay NA.  Kept on purpose: other$isnowdg is never updated inside the loop
 * (every chunk restarts the ground layer from the initial depth) and each chunk restarts the albedo
 * clock (gridmodelsnow1 calls snowalbCpp on its own slice).  terra's aggregate/resample inside
 * .tpicalc are restated as in mcf_precompute_terrain (block means from the top-left, bilinear between
 * block centres). */
typedef struct mcf_snowdriver_in {
    mcf_snow_inputs base;
    const double *dtm;      /* [rows,cols] elevations (m), NaN = NA                        */
    double res;             /* cell size (m)                                              */
    double tfact;           /* .tpicalc's tfact (runsnowmodel default 0.02)               */
    int32_t chunk_steps;    /* 0 -> 120                                                   */
    /* Array weather only (base.array_forcing != 0: `.snowmodel2`'s loop, R/internal.R:2950-3008; mcf_snowmodel2 and the
     * array-weather snow run).  af_wsa_s: the wind-shelter smoothing factor — `.snowmodel2` takes 10 only when res <= 100 AND
     * the coarse weather grid has at least ten cells a side (:2963-2964), which the fine arrays here no longer say; 0: as
     * `.snowmodel1` (10 if res <= 100 else 1).  af_wind: [tsteps] sqrt(wuv^2 + wvv^2) of the coarse wind components' spatial
     * means (:2907-2908), whose chunk means set the aggregation factor of the position index (:2981-2984, at least 2). */
    int32_t af_wsa_s;
    const double *af_wind;
} mcf_snowdriver_in;
/* Returned list of .snowmodel1 (R/internal.R:2619): each [rows,cols,tsteps] or NULL. */
typedef struct mcf_snowdriver_out {
    double *Tc, *Tg, *groundsnowdepth, *totalSWE, *snowden;
} mcf_snowdriver_out;
int mcf_snowmodel1(const mcf_snowdriver_in *in, mcf_snowdriver_out *out, int32_t device);
/* The chunk loop of `.snowmodel2` (R/internal.R:2950-3008: the part behind the resampling of the coarse arrays), device-resident:
 * `base` carries array weather at the raster's resolution — clim.{temp, relhum, pres, swdown, difrad, lwdown, windspeed, precip}
 * and pointm.{Gp, Tc, RswabsG, RlwabsG, umu} as [rows,cols,tsteps], clim.winddir [tsteps], other.{lats, lons} [rows,cols] —
 * what gridmodelsnow2 takes; a chunk's slices are uploaded as the loop reaches them (13 x 8 B per cell-step over PCIe: this is
 * the boundary the reference's own binding has).  Differences to the data.frame loop kept as the reference has them: the
 * aggregation factor from af_wind with a floor of 2, af_wsa_s.  One block (no `_multi` form yet). */
int mcf_snowmodel2(const mcf_snowdriver_in *in, mcf_snowdriver_out *out, int32_t device);
/* The same loop over several devices from ONE process (the companion of mcf_runmicro1_multi for BASELINE configs[4]): the
 * raster in `n_blocks` contiguous row blocks, block b a snow plan on devices[b % n_devices] driven by that device's host
 * thread; per chunk the blocks' snow surfaces meet in one host array (each block takes its halo rows from it) and the two
 * raster-wide means are formed from the blocks' (sum, count) in block order — the exchanges of the stepwise API below,
 * done in host memory.  Equal to mcf_snowmodel1 up to the summation order of those two means (1e-9 in the tests); a block's
 * series reach the caller's arrays chunk by chunk, downloaded through the row pitch straight into their rows.  n_devices = 0:
 * every visible device; n_blocks = 0: one per device.  Unlike the solver's _multi entries, EVERY block's snow plan stays
 * resident for the whole run (the chunk loop couples the blocks at every chunk): more blocks than devices do not lower a
 * device's memory footprint here, they only share its time. */
int mcf_snowmodel1_multi(const mcf_snowdriver_in *in, mcf_snowdriver_out *out, const mcf_multi *multi);

/* The same loop one step at a time, for a row block of a tiled raster (one plan per rank): between the
 * steps the caller exchanges what couples the blocks — halo rows of the snow surface for the terrain
 * stencil and .tpicalc's block means (point-to-point), and two raster-wide means as (sum, count)
 * all-reduces.  mcf_snowmodel1 is this sequence with one block.  `in->base` and `in->dtm` describe the own
 * rows; row0 / rows_total place them (rows_total = 0: the block is the raster).  Per chunk c:
 *   mcf_snowplan_surface()          own rows of dtm + ground snow depth          -> halo exchange
 *   mcf_snowplan_surface_partial()  (sum, count) of it over non-NA cells         -> all-reduce (only used when
 *                                   round(10*sqrt(mean wind)/res) >= min(dim)/2, .tpicalc's fallback)
 *   mcf_snowplan_prepare_chunk(c, ext, hn, hs, surface_mean, &s, &n)
 *                                   ext = [hn + rows + hs, cols] surface with halos (NULL, 0, 0: no
 *                                   neighbours); terrain refresh + tpic; returns the partial (sum, count)
 *                                   of tpic                                       -> all-reduce
 *   mcf_snowplan_run_chunk(c, tpic_mean, out)   gridmodelsnow1 on the chunk, redistribution, hand-over;
 *                                   copies the chunk into the block's [rows, cols, tsteps] host arrays
 * Halo needed: 100 + 2.5 s rows (s = 10 if res <= 100 else 1) and whole af x af blocks around the own
 * rows, or every row up to the raster edge; checked. */
typedef struct mcf_snowplan mcf_snowplan;
int mcf_snowplan_create(const mcf_snowdriver_in *in, int64_t row0, int64_t rows_total, int32_t device,
                        mcf_snowplan **plan);
void mcf_snowplan_destroy(mcf_snowplan *plan);
int32_t mcf_snowplan_chunks(const mcf_snowplan *plan);
int mcf_snowplan_surface(mcf_snowplan *plan, double *host_own);
/* The pack depth the loop hands from the chunk just run to the next one (`other$isnowdc <- (asc + cdsnow + dsnow2)[,,last]`,
 * R/internal.R:2607), own rows, [rows, cols].  Once a pack has melted this is a rounding residue (0 or +-1e-17 m) and
 * `sdepcp > 0` (src/microclimfCpp.cpp:4337) decides on it whether the next chunk runs the model: the reference's loop is
 * discontinuous in its own rounding there.  Exposed so that a checker can tell such ill-conditioned hand-overs from
 * wrong ones (tests/test_snow_gpu.py::test_full_year_chunk_loop_*). */
int mcf_snowplan_handover(mcf_snowplan *plan, double *host_isnowdc);
int mcf_snowplan_surface_partial(mcf_snowplan *plan, double *sum, double *count);
int mcf_snowplan_prepare_chunk(mcf_snowplan *plan, int32_t chunk, const double *ext, int32_t halo_north,
                               int32_t halo_south, double surface_mean, double *tpic_sum, double *tpic_count);
/* The same exchange without host staging (one process per GPU, RCCL send / recv on device buffers): pack_halo copies the own
 * block's first `rows_north` / last `rows_south` surface rows into the caller's DEVICE buffers as column-major
 * [rows_north, cols] / [rows_south, cols] pieces — what the neighbouring ranks receive as their halos — and returns when they
 * are complete; prepare_chunk_dev takes the received pieces as device pointers and puts [north; own; south] together on the
 * device.  Same results as the host-pointer pair above, bit for bit. */
int mcf_snowplan_pack_halo(mcf_snowplan *plan, int32_t rows_north, double *d_north, int32_t rows_south, double *d_south);
int mcf_snowplan_prepare_chunk_dev(mcf_snowplan *plan, int32_t chunk, const double *d_halo_north, int32_t halo_north,
                                   const double *d_halo_south, int32_t halo_south, double surface_mean, double *tpic_sum,
                                   double *tpic_count);
int mcf_snowplan_run_chunk(mcf_snowplan *plan, int32_t chunk, double tpic_mean, mcf_snowdriver_out *out);
/* ... with the chunk's series written into row blocks of taller column-major host arrays (`row_pitch` rows per column; 0 =
 * dense): one strided DMA per series straight into the caller's rows, no block-sized host buffer (mcf_snowmodel1_multi). */
int mcf_snowplan_run_chunk_pitched(mcf_snowplan *plan, int32_t chunk, double tpic_mean, const mcf_snowdriver_out *out, int64_t row_pitch);
/* `.tpicalc`'s aggregation factor of a chunk, round(10 * sqrt(mean wind speed of the chunk) / res) (R/internal.R:2589-2590):
 * what sizes the halo a row block needs around its rows (100 + 3 s + 2 af rows, or all rows up to the raster edge). */
int mcf_snowplan_chunk_af(const mcf_snowplan *plan, int32_t chunk, int32_t *af);
/* applycpp3 (src/microclimfCpp.cpp:5553-5588) of the totalSWE series of the chunk just run, straight from the device:
 * result / count [steps of that chunk] as mcf_applycpp3 gives them.  `.runmicrosnow1` decides snow / no-snow days on the
 * per-step minimum and maximum of totalSWE (R/internal.R:3592-3594); row-block ranks combine them with one all-reduce. */
int mcf_snowplan_apply3(mcf_snowplan *plan, int32_t chunk, int32_t fun, double *result, double *count);

/* ---- the snow-day microclimate inside the chunk loop: `.runmicrosnow1` (R/internal.R:3581-3659) device-resident ----------
 * The reference runs the no-snow solver on the days with a snow-free cell somewhere, gridmicrosnow1
 * (src/microclimfCpp.cpp:4894-5056) on the days with snow somewhere, and merges by day, with the whole year's snow series in
 * memory.  Here the series exist one 5-day chunk at a time, and gridmicrosnow1 needs two things of the WHOLE snow-day series
 * before its first step — the per-cell mean snow damping depth (cpp:4713-4737) and the day list itself (its albedo clock and
 * maximum temperature run over the subset) — so the year is walked twice:
 *   pass 1  chunk loop as before (prepare_chunk, run_chunk, apply3 -> snowdaysfun); per chunk
 *           mcf_snowplan_meand_accumulate(chunk, snowday[]) adds the chunk's snow days to the running sum
 *   between mcf_snowplan_micro_setup(subset inputs, day map, reqhgt, mat, out mask): the snow-day subset's weather (incl. umu),
 *           `.sortl2` vegetation, bare-ground terrain, Smax; builds its step table; finishes the mean damping depth;
 *           mcf_plan_set_mxtc(solver plan, max temperature of the NO-snow subset) (cpp:2159-2168 over the subset the
 *           reference hands to runmicro1Cpp); mcf_snowplan_reset() puts the hand-over state back to the series' start
 *   pass 2  chunk loop again; per chunk the solver on the chunk's no-snow days at their own place in the ring slot
 *           (mcf_plan_run_days_at), then mcf_snowplan_microsnow(solver plan, chunk, slot, nosnowday[]) writes the snow
 *           microclimate over it: snow-covered cell-steps of snow days get gridmicrosnow1's values, snow-free cell-steps keep
 *           the solver's value when the day is a no-snow day as well and are NA otherwise (the reference's blank template).
 * The slot then holds `.runmicrosnow1`'s merged output for the chunk's days. */
int mcf_snowplan_reset(mcf_snowplan *plan);
/* Pass 2 need not walk the whole series again: mcf_snowplan_checkpoint(chunk), called in pass 1 BEFORE the chunk's
 * prepare_chunk, keeps the state the chunk starts from (pack depth handed over, snow surface, the two ages: 24 bytes per cell)
 * on the device; mcf_snowplan_restore(chunk) puts it back.  A chunk without a snow day contributes only the no-snow solver's
 * days to the merged output, so pass 2 restores and re-runs the chunks that hold one and skips the others.  (On a row-tiled
 * raster every rank takes the same decision: the day classes come from all-reduced extremes.) */
/* Sparse read-back of the plan's device arrays for n cells (0-based, column-major index within the block): out is
 * [n, depth] column-major, depth = 1 (hand-over state, slope, aspect, sky view), 8 (wind shelter), 24 (horizons) or the
 * chunk's steps (the series of the chunk run last; MCF_SNOWPLAN_TOTALSWE after the redistribution).  For in-run checks of a
 * sample of cells against a CPU model (bench.py --config 4); no counterpart in the reference. */
enum {
    MCF_SNOWPLAN_ISNOWDC = 0, MCF_SNOWPLAN_ISNOWAC = 1, MCF_SNOWPLAN_ISNOWAG = 2, MCF_SNOWPLAN_SLOPE = 3, MCF_SNOWPLAN_ASPECT = 4,
    MCF_SNOWPLAN_SKYVIEW = 5, MCF_SNOWPLAN_WSA = 6, MCF_SNOWPLAN_HOR = 7, MCF_SNOWPLAN_TC = 8, MCF_SNOWPLAN_TG = 9,
    MCF_SNOWPLAN_SDEPG = 10, MCF_SNOWPLAN_SDEN = 11, MCF_SNOWPLAN_TOTALSWE = 12
};
int mcf_snowplan_fetch_cells(mcf_snowplan *plan, int32_t what, const int64_t *cells, int32_t n, double *out, int32_t *depth);
/* ... and need not re-run a chunk whose series still fit the device: mcf_snowplan_keep_chunk(chunk, reserve_bytes, &kept),
 * called in pass 1 after run_chunk and everything that reads the chunk's series (apply3, meand_accumulate), hands the chunk's
 * five series buffers over to a cache and gives the plan fresh ones — as long as `reserve_bytes` of device memory stay free
 * (kept = 0 otherwise; a year of one rank's block of configs[4] is 38 snow chunks x 10 GB against 288 GB of HBM).
 * mcf_snowplan_microsnow reads a kept chunk where it lies: pass 2 skips restore / prepare_chunk / run_chunk for it.
 * mcf_snowplan_release_kept (before the next year's pass 1) returns the sets to a pool the next year draws from: allocating
 * 10 GB takes about 0.25 s, more than re-running the chunk — the cache pays from a plan's second year on. */
int mcf_snowplan_keep_chunk(mcf_snowplan *plan, int32_t chunk, int64_t reserve_bytes, int32_t *kept);
/* Would mcf_snowplan_keep_chunk keep a chunk now (a pooled set, or room for a new one beside reserve_bytes)? */
int mcf_snowplan_can_keep(mcf_snowplan *plan, int64_t reserve_bytes, int32_t *yes);
/* A ceiling on what mcf_snowplan_keep_chunk may ALLOCATE over the plan's lifetime (pooled sets count once); < 0: none. */
int mcf_snowplan_set_keep_budget(mcf_snowplan *plan, int64_t bytes);
/* Which of the five device series the following mcf_snowplan_run_chunk calls write: bit 0 Tc, 1 Tg, 2 totalSWE, 3 ground snow
 * depth, 4 snow density (default 31).  Pass 1 of the two-pass run needs only totalSWE (the day classes) and the density (the
 * mean damping depth) of a chunk that will not stay in HBM — pass 2 re-runs it —, and the five stores per cell-step are what a
 * snow-free chunk costs.  A series that is off cannot be asked for in run_chunk's host outputs; a chunk run with series off
 * cannot be kept or handed to mcf_snowplan_microsnow (MCF_ERR_STATE). */
int mcf_snowplan_set_series(mcf_snowplan *plan, uint32_t mask);
int mcf_snowplan_release_kept(mcf_snowplan *plan);
int mcf_snowplan_checkpoint(mcf_snowplan *plan, int32_t chunk);
int mcf_snowplan_restore(mcf_snowplan *plan, int32_t chunk);
int mcf_snowplan_meand_accumulate(mcf_snowplan *plan, int32_t chunk, const int32_t *snowday /* [days of the chunk] */);
/* reuse_static != 0: the vegetation, terrain and Smax matrices of the previous set-up stay (only the series and the day map
 * are new). */
int mcf_snowplan_micro_setup(mcf_snowplan *plan, const mcf_snow_inputs *subset, const int32_t *subset_day_of_day,
                             int32_t ndays, double reqhgt, double mat, const int32_t out[MCF_NOUT], int32_t reuse_static);
/* Pass 2, before the solver's run of the chunk's days [day, day + ndays) (days of the chunk, 0-based): skip_tile[t] = 1
 * where every cell of the solver plan's tile t has a vegetation height and a snow water equivalent > 0 at every step of
 * those days — mcf_snowplan_microsnow will overwrite all of the tile's values of these days —, 0 elsewhere; all 0 when the
 * solver plan holds an output gridmicrosnow1's `out` mask leaves to the solver.  *n_covered = number of ones. */
int mcf_snowplan_covered_tiles(mcf_snowplan *plan, mcf_plan *solver, int32_t chunk, int32_t day, int32_t ndays,
                               uint8_t *skip_tile, int64_t n_tiles, int64_t *n_covered);
/* The same question per cell, answered on the device: (*need_cell)[c] = 1 where cell c is NOT under snow at every step of
 * those days, or has no vegetation height (gridmicrosnow1 skips it) — the cells whose solver values survive the merge —, 0
 * elsewhere; all 1 when the solver plan holds an output gridmicrosnow1's `out` mask leaves to the solver.  *need_cell is device
 * memory of the snow plan (valid until the next call, complete on return), for mcf_plan_run_days_cells; *n_need = number of
 * ones. */
int mcf_snowplan_free_cells(mcf_snowplan *plan, mcf_plan *solver, int32_t chunk, int32_t day, int32_t ndays,
                            const uint8_t **need_cell, int64_t *n_need);
int mcf_snowplan_microsnow(mcf_snowplan *plan, mcf_plan *solver, int32_t chunk, int32_t slot,
                           const int32_t *nosnowday /* [days of the chunk] */);

/* ---- `runmicro(..., snow = TRUE)` for data.frame weather as ONE call: `.snowmodel1` + `.runmicrosnow1` -----------------------
 * The reference's `.runmicrosnow1(micropoint, reqhgt, vegp, soilc, dtm, smod, ...)` (R/internal.R:3581-3659, called from
 * runmicro at R/Cppwrappers.R:382) takes `smod` — five [rows, cols, tsteps] arrays that `runsnowmodel` -> `.snowmodel1`
 * (R/internal.R:2498-2619) produced — from host memory, runs the grid solver on the days with a snow-free cell somewhere
 * (`.runmicronosnow` on subsetpointmodel(days = nosnowdays), :3603-3606), gridmicrosnow1 on the days with snow somewhere
 * (:3612-3625) and merges by day (:3633-3656).  This entry is that whole sequence with the snow series kept on the device:
 * the chunk loop of `.snowmodel1` is driven here (mcf_snowplan_*), the two models meet in the solver's output ring, and only
 * the merged [rows, cols, tsteps] outputs — and the snow series too, if `smod` asks for them — cross PCIe.  An R session
 * reaches it through r/mcfhip_overrides.R (runsnowmodel returns a light handle instead of the arrays, `.runmicrosnow1` passes
 * it on).
 *   grid    what `.runmicronosnow` -> runmicro1Cpp would get for EVERY day of the series (vector forcing); with time-varying
 *           vegetation (veg_layers > 1: runmicro3Cpp) the WHOLE-series layer table — a no-snow day runs with the layer it has
 *           in the whole series, which is what `.runmodel3Cpp` on the day subset comes to (R/internal.R:252-270, 1391-1399)
 *   snow    `.snowmodel1`'s inputs as for mcf_snowmodel1 (obstime / climate / pointmodelsnow output for the whole series, the
 *           `.sortl` vegetation, initial depths and ages, dtm, res, tfact)
 *   micro   gridmicrosnow1's inputs as `.prepsnowinputs1` (R/internal.R:3375-3443) makes them, but for the WHOLE series
 *           (tsteps = the series' length; the entry takes the snow-day subset itself): obstime, climate incl. umu =
 *           smod$umu, `.sortl2` vegetation, bare-ground terrain (slope, aspect, skyview, wsa, hor), lat, lon, zref, Smax.
 *           May be NULL only if the year has no snow day.
 *   mat     micropoint$matemp
 * `opt`: reqhgt >= 0 (reqhgt < 0: the `_below` entries further down), out[] as for mcf_runmicro1; with reqhgt == 0 gridmicrosnow1 is given the reference's fixed mask (:3616-3619).
 * `out`: [rows, cols, tsteps] per requested variable; `smod` (optional, members may be NULL): `.snowmodel1`'s returned arrays.
 * Days that are in neither class (max totalSWE <= 0 and min != 0: a melted pack's negative rounding residue) are NA in
 * `out` — the reference's merge indexes past its arrays there (:3650-3655).  Steps past the last whole 5-day chunk are
 * no-snow days, as `.runmicrosnow1`'s NA -> 0 makes them (:3586).
 * The staged form, for callers whose gridmicrosnow1 inputs depend on the day classes (`.sortl2` weights time-varying
 * vegetation layers by the snow-covered steps): create -> pass1 (returns snowday[] / nosnowday[], one flag per day) -> pass2. */
typedef struct mcf_microsnow_in {
    const mcf_grid_inputs *grid;
    const mcf_snowdriver_in *snow;
    const mcf_snow_inputs *micro;
    double mat;
} mcf_microsnow_in;
int mcf_runmicrosnow1(const mcf_microsnow_in *in, const mcf_options *opt, mcf_outputs *out, const mcf_snowdriver_out *smod);
/* The same run with ARRAY weather: `.snowmodel2`'s loop (R/internal.R:2950-3008) + `.runmicrosnow2` (:3661-3745).  Everything is
 * at the raster's resolution, as the reference's bindings take it after `.cca` / resample:
 *   grid    runmicro2Cpp's arguments for every day (array_forcing = 1: climate and point-model arrays [rows,cols,tsteps], lats / lons)
 *   snow    mcf_snowmodel2's input (gridmodelsnow2's arrays, af_wind, af_wsa_s)
 *   micro   gridmicrosnow2's inputs for the WHOLE series (array_forcing = 1: weather arrays incl. umu, winddir [tsteps], lats / lons)
 *   mat     the point models' mean annual temperature (`matemp`, :3682-3687)
 * A chunk's slices of the snow model's arrays, its no-snow days of the solver's fifteen and its snow days of the microclimate's nine
 * are uploaded as the loops reach them (the boundary is PCIe-bound by construction: 8 B x 13 / 15 / 9 per cell-step); the solver's
 * per-cell temperature cap is taken over the no-snow days (mcf_plan_set_mxtc_days), the microclimate's over the snow days.  One
 * block on one device (no _multi form); the staged entries below take either geometry. */
int mcf_runmicrosnow2(const mcf_microsnow_in *in, const mcf_options *opt, mcf_outputs *out, const mcf_snowdriver_out *smod);
/* The same over row blocks on several devices from one process (mcf_multi as for mcf_runmicro1_multi; equal-row blocks as
 * mcf_snowmodel1_multi): per chunk the blocks' snow surfaces meet in one host array, the raster-wide means (snow surface, tpi,
 * the solver's twi mean) and the per-step extremes of totalSWE are combined in block order.  One block: bit for bit
 * mcf_runmicrosnow1; more blocks: equal up to the summation order of those means. */
int mcf_runmicrosnow1_multi(const mcf_microsnow_in *in, const mcf_options *opt, const mcf_multi *multi, mcf_outputs *out,
                            const mcf_snowdriver_out *smod);
typedef struct mcf_snowrun mcf_snowrun;
/* `in->micro` and `in->mat` are not read here; multi = NULL: one block on opt->device.  The caller's arrays must stay valid
 * until mcf_snowrun_destroy. */
int mcf_snowrun_create(const mcf_microsnow_in *in, const mcf_options *opt, const mcf_multi *multi, mcf_snowrun **run);
/* Below ground (reqhgt < 0, data.frame weather; MCF_ERR_ARG otherwise): mcf_runmicrosnow1 / mcf_runmicrosnow1_multi /
 * mcf_snowrun_create with the same arguments.  `.runmicrosnow1` gives the grid solver the NO-SNOW days' subset series, so
 * Tbelowgroundv's running means (cpp:1474-1539) see those days joined end to end: each block's solver plan is a streamed
 * below-ground plan over them (mcf_plan_create_streamed, mcf_plan_below_set_days) — O(cells x days) of state, no whole-series
 * buffer, and with complete = 1 one more solver sweep over the no-snow days between the passes.  Pass 2 solves EVERY cell of a
 * chunk's no-snow days (a cell's ground temperature under today's snow feeds its means on later days: mcf_snowrun_stats
 * reports no tile-day left out), makes the chunk's Tz, and then the snow-day model (gridmicrosnow1 with `out[c(1, 4)]`,
 * R/internal.R:3621-3624: Tz and soilm; every snow-covered cell-step is below the snow surface, cpp:5029-5051) merges into the
 * same slot.  On a day of both classes the other requested outputs keep the solver's values, on a snow-only day they are NA.
 * Steps behind the last whole day are NA.  A handle runs one period: a second mcf_snowrun_pass2 is MCF_ERR_STATE. */
int mcf_runmicrosnow1_below(const mcf_microsnow_in *in, const mcf_options *opt, mcf_outputs *out, const mcf_snowdriver_out *smod);
int mcf_runmicrosnow1_below_multi(const mcf_microsnow_in *in, const mcf_options *opt, const mcf_multi *multi, mcf_outputs *out,
                                  const mcf_snowdriver_out *smod);
int mcf_snowrun_create_below(const mcf_microsnow_in *in, const mcf_options *opt, const mcf_multi *multi, mcf_snowrun **run);
void mcf_snowrun_destroy(mcf_snowrun *run);
int32_t mcf_snowrun_days(const mcf_snowrun *run);     /* tsteps / 24 */
/* Between mcf_snowrun_pass1 and mcf_snowrun_pass2, layered vegetation: the solver plans' day -> layer map (mcf_plan_set_day_layers).
 * The run solves the no-snow days with the layer the WHOLE-series table gives them; a caller that wants `.runmodel3Cpp`'s dealing of
 * the no-snow SUBSET passes that here, in whole-series days and rows of the whole series' arrays (the two differ when a layer keeps
 * steps of the subset without being any of its days' mode: `.sortvegp` cuts the arrays by steps, the table has a row per day mode).
 * MCF_ERR_STATE outside the two passes.  The map holds for this period: the next mcf_snowrun_pass1 puts the plans' own table back. */
int mcf_snowrun_set_day_layers(mcf_snowrun *run, const int32_t *layer_of_day, int32_t ndays);
/* What pass 2 was spared (diagnostics; tests assert which path ran): stats[0] tile-days of the solver's days that are snow days as
 * well, [1] of them left out (tiles wholly under snow, mcf_plan_run_days_masked; or, where few cells are not under snow, all tiles
 * but the ones those cells fill, mcf_plan_run_days_cells), [2] snow chunks whose series had stayed in HBM,
 * [3] snow chunks re-run from their checkpoints. */
int mcf_snowrun_stats(const mcf_snowrun *run, int64_t stats[4]);
/* Keep pass 1's snow chunks in device memory for pass 2, up to `bytes` in all (0: off, the default — on a fresh handle the
 * allocation costs more than re-running the chunks).  The sets are pooled in the handle: a second period on the same handle
 * (mcf_snowrun_pass1 again) allocates nothing and pass 2 re-runs only what did not fit.  Outputs are bit for bit the unkept
 * run's.  Reference: none (`.runmicrosnow1`, R/internal.R:3581-3659, holds the whole series in host memory). */
int mcf_snowrun_keep(mcf_snowrun *run, int64_t bytes);
/* snowday / nosnowday: [mcf_snowrun_days] or NULL */
int mcf_snowrun_pass1(mcf_snowrun *run, const mcf_snowdriver_out *smod, int32_t *snowday, int32_t *nosnowday);
int mcf_snowrun_pass2(mcf_snowrun *run, const mcf_snow_inputs *micro, double mat, mcf_outputs *out);

/* ---- period summaries of the snow run and of the snowpack, folded on the device -------------------------------
 * The `summary` of "period summaries" above (same table, statistics, order of evaluation and NA rule) kept over
 *   - the snow run's merged outputs: each block's solver plan carries a mcf_summary_spec, and pass 2 folds every merged ring
 *     chunk behind the snow-day kernel (or behind the solver alone) with mcf_plan_summary_accumulate;
 *   - the snowpack's five series (mcf_snowdriver_out's order: Tc, Tg, groundsnowdepth, totalSWE, snowden), folded from a
 *     chunk's device series right after run_chunk — the values mcf_snowmodel1 copies to its host arrays, totalSWE after the
 *     redistribution.  HOURS_ABOVE of totalSWE with threshold 0 is the snow-cover duration, MAX of totalSWE the peak snow
 *     water equivalent.
 * Nothing of size cells x steps crosses PCIe or exists on the host.  reqhgt >= 0 (a below-ground run is refused: its solver
 * plan is a streamed plan). */
typedef struct mcf_snowpack_summary_spec {
    int32_t nperiods;
    const int32_t *period_of_day;  /* [tsteps / 24]; a day past the last whole chunk must be -1 (no chunk covers it) */
    int32_t series[5];             /* != 0: summarised (Tc, Tg, groundsnowdepth, totalSWE, snowden)  */
    int32_t stat[MCF_NSTAT];       /* != 0: kept                                                      */
    double threshold[5];           /* HOURS_ABOVE; read for selected series only                      */
} mcf_snowpack_summary_spec;
typedef struct mcf_snowpack_summary_out {
    double *val[5][MCF_NSTAT];     /* [rows, cols, nperiods] for every selected pair */
    int32_t *days;                 /* [nperiods] or NULL */
} mcf_snowpack_summary_out;
/* The snow plan's sink.  enable: allocates nsel x nperiods x state rows x cells x 8 bytes (MCF_ERR_NOMEM when it does not
 * fit); MCF_ERR_ARG with a message for a null spec, nperiods < 1, a table entry outside -1 .. nperiods - 1, an empty selection,
 * a NaN threshold of a selected series with HOURS_ABOVE selected, chunk_steps that are not whole days, a counted day past the
 * last whole chunk; MCF_ERR_STATE when called twice.  accumulate(chunk): folds the series of the chunk run last (after
 * run_chunk, before mcf_snowplan_keep_chunk hands the buffers over), on the stream the model wrote them on; chunks arrive in
 * ascending order, each at most once, and every selected series must have been written (mcf_snowplan_set_series):
 * MCF_ERR_STATE otherwise.  fetch: one statistic of one series as [rows, cols, nperiods], column-major, `row_pitch` rows per
 * column on the host (0: dense).  reset: nothing folded, chunk 0 may come next. */
int mcf_snowplan_summary_enable(mcf_snowplan *plan, const mcf_snowpack_summary_spec *spec);
int mcf_snowplan_summary_accumulate(mcf_snowplan *plan, int32_t chunk);
int mcf_snowplan_summary_fetch(mcf_snowplan *plan, int32_t series, int32_t stat, double *host_dst, int64_t row_pitch);
int mcf_snowplan_summary_days(mcf_snowplan *plan, int32_t *days);
int mcf_snowplan_summary_reset(mcf_snowplan *plan);
/* The summary table of a snow run from the caller's: days in NEITHER class (no day of either model: NA for every cell in the
 * run's arrays) are never counted, out[d] = -1 there and period_of_day[d] elsewhere.  Pure host function. */
int mcf_snowrun_summary_table(const int32_t *period_of_day, const int32_t *snowday, const int32_t *nosnowday, int32_t ndays,
                              int32_t *out);
/* Switches the sinks of a run on, before mcf_snowrun_pass1 (MCF_ERR_STATE after it, or when called twice); either spec may be
 * NULL, not both.  `micro` selects among the variables the run was created with.  With a summary enabled mcf_snowrun_pass2
 * accepts out == NULL or null arrays: variables without a host array are folded only.  mcf_snowrun_pass1 starts the summaries
 * over (a second year on one handle). */
int mcf_snowrun_summary_enable(mcf_snowrun *run, const mcf_summary_spec *micro, const mcf_snowpack_summary_spec *pack);
/* One plane [rows, cols, nperiods] of the whole raster, every block's rows in place; pack = 0: variable `var` of the merged
 * outputs (after pass 2), pack != 0: series `var` of the snowpack (after pass 1).  MCF_ERR_STATE before that. */
int mcf_snowrun_summary_fetch(mcf_snowrun *run, int32_t pack, int32_t var, int32_t stat, double *host_dst);
int mcf_snowrun_summary_days(mcf_snowrun *run, int32_t pack, int32_t *days);
/* One call: mcf_runmicrosnow1 / 2 / _multi (by `in`'s weather geometry and `multi`, which may be NULL) with the sinks on.
 * micro / pack: the planes of the enabled specs (the struct of a NULL spec is not read); arrays (optional): host arrays for
 * some or all requested variables, as mcf_runmicrosnow1's `out`; smod (optional) as there; snowday / nosnowday: [days] or NULL. */
typedef struct mcf_snowrun_summary_out {
    mcf_summary_out micro;
    mcf_snowpack_summary_out pack;
    mcf_outputs *arrays;
    const mcf_snowdriver_out *smod;
    int32_t *snowday, *nosnowday;
} mcf_snowrun_summary_out;
int mcf_runmicrosnow_summary(const mcf_microsnow_in *in, const mcf_options *opt, const mcf_multi *multi,
                             const mcf_summary_spec *micro_spec, const mcf_snowpack_summary_spec *pack_spec,
                             mcf_snowrun_summary_out *outs);
/* The snow model alone with the snowpack sink and no series output: data.frame weather, mcf_snowmodel1's loop on device 0
 * (multi == NULL) or mcf_snowmodel1_multi's over `multi`'s devices and row blocks (another single device: a mcf_multi that
 * names it). */
int mcf_snowmodel1_summary(const mcf_snowdriver_in *in, const mcf_snowpack_summary_spec *spec, const mcf_multi *multi,
                           mcf_snowpack_summary_out *out);

/* ---- series sink of the snow run and of the snowpack (definitions: "series sink" and "series sink: further sources" above;
 * DESIGN.md §28) ------------------------------------------------------------------------------------------------------------
 * Snowpack: the five series in mcf_snowdriver_out's order (Tc, Tg, groundsnowdepth, totalSWE, snowden; totalSWE after the
 * redistribution), folded from a chunk's device series right after run_chunk — the values mcf_snowmodel1 copies to the host.
 * The whole days of a folded chunk are done; days behind the last whole chunk are never folded (NA in every statistic).  A
 * totalSWE of 4096 or more in its own unit falls under the BAD rule like any other value.
 * Snow run, merged outputs: pass 2 folds every merged ring chunk.  A day in neither class (no-snow days and snow days are the
 * run's two classes) is never folded: its steps are NA in every statistic, COUNT too.  reqhgt >= 0. */
typedef struct mcf_snowpack_series_spec {      /* as mcf_series_spec, over the five snowpack series */
    int64_t npoints;
    const int64_t *cells;
    int32_t nzones;
    const int32_t *zone;
    int32_t series[5];
    int32_t zstat[MCF_NZSTAT];
} mcf_snowpack_series_spec;
typedef struct mcf_snowpack_series_out {
    double *points[5];                 /* [tsteps, npoints] for every selected series when npoints > 0 */
    double *zones[5][MCF_NZSTAT];      /* [tsteps, nzones] for every selected pair when nzones > 0     */
} mcf_snowpack_series_out;
/* The snow plan's sink.  enable: MCF_ERR_ARG, the message starting with the entry's name, for a null spec, an empty selection,
 * nzones > MCF_MAX_ZONES, a label or cell out of range, more than 2^26 cells, chunk_steps that are not whole days;
 * MCF_ERR_STATE when called twice.  accumulate(chunk): folds the series of the chunk run last, on the stream the model wrote
 * them on; chunks may come in any order, each at most once (a second fold is MCF_ERR_STATE), and every selected series must have
 * been written (mcf_snowplan_set_series): MCF_ERR_STATE otherwise.  fetch: [tsteps, npoints] / [tsteps, nzones], column-major.
 * reset: nothing folded. */
int mcf_snowplan_series_enable(mcf_snowplan *plan, const mcf_snowpack_series_spec *spec);
int mcf_snowplan_series_accumulate(mcf_snowplan *plan, int32_t chunk);
int mcf_snowplan_series_fetch_points(mcf_snowplan *plan, int32_t series, double *dst);
int mcf_snowplan_series_fetch_zones(mcf_snowplan *plan, int32_t series, int32_t zstat, double *dst);
int mcf_snowplan_series_reset(mcf_snowplan *plan);
/* Switches the sinks of a run on, before mcf_snowrun_pass1 (MCF_ERR_STATE after it, or when called twice); either spec may be
 * NULL, not both; both are given for the whole raster.  `micro` selects among the variables the run was created with.  May sit
 * beside mcf_snowrun_summary_enable.  A reqhgt < 0 run is refused (MCF_ERR_ARG).  With a series enabled mcf_snowrun_pass2 accepts
 * out == NULL or null arrays; mcf_snowrun_pass1 starts the series over (a second year on one handle).  The fetches combine the
 * row blocks; pack = 0: variable `var` of the merged outputs (after pass 2), pack != 0: series `var` of the snowpack (after
 * pass 1); MCF_ERR_STATE before that. */
int mcf_snowrun_series_enable(mcf_snowrun *run, const mcf_series_spec *micro, const mcf_snowpack_series_spec *pack);
int mcf_snowrun_series_fetch_points(mcf_snowrun *run, int32_t pack, int32_t var, double *dst);
int mcf_snowrun_series_fetch_zones(mcf_snowrun *run, int32_t pack, int32_t var, int32_t zstat, double *dst);
/* One call, as mcf_runmicrosnow_summary: data.frame weather with or without `multi`, array weather as one block. */
typedef struct mcf_snowrun_series_out {
    mcf_series_out micro;
    mcf_snowpack_series_out pack;
    mcf_outputs *arrays;
    const mcf_snowdriver_out *smod;
    int32_t *snowday, *nosnowday;
} mcf_snowrun_series_out;
int mcf_runmicrosnow_series(const mcf_microsnow_in *in, const mcf_options *opt, const mcf_multi *multi,
                            const mcf_series_spec *micro_spec, const mcf_snowpack_series_spec *pack_spec,
                            mcf_snowrun_series_out *outs);
/* The snow model alone with the snowpack series sink and no series output, as mcf_snowmodel1_summary (`multi` may be NULL). */
int mcf_snowmodel1_series(const mcf_snowdriver_in *in, const mcf_snowpack_series_spec *spec, const mcf_multi *multi,
                          mcf_snowpack_series_out *out);

/* ---- netCDF sink: further sources --------------------------------------------------------------------------
 * The `writetonc` file (mcf_nc_create above) behind more than the ring slot of one plan: a row block's plan as a row strip of
 * the file, a depth slab of a streamed below-ground plan, the snow plan's chunk series; and the one-call entries that end in
 * a file instead of [rows, cols, tsteps] doubles on the host.  The ABI version stays: entries and structs are added, none
 * changes.
 *
 * Row strips.  The device packs a plan's rows as records of their own, [step][8 B | var][plan rows][cols] (k_pack_nc with the
 * plan's rows), and the file side writes one run per (step, variable) at
 *     rec_begin + step * rec_bytes + 8 + var * rows * cols * 4 + row0 * cols * 4
 * of the classic container, with the step's time word beside it: a record has its time value whichever block wrote it, in
 * whatever order.  Several host threads (the row-block workers) may write strips of one file at once, as long as their strips
 * do not overlap.  The netCDF-4 container chunks a step into row strips of the whole raster, which a block cut need not respect:
 * it takes whole rasters only (MCF_ERR_ARG for a strip, and for a one-call entry with more than one block).
 *
 * mcf_nc_write_plan_rows: the plan's rows are rows [row0, row0 + plan rows) of the file, the columns are the file's.  `depth`
 * selects the Tz slab of a streamed below-ground plan with a depth list (mcf_plan_below_set_depths); 0 otherwise, anything else
 * is MCF_ERR_ARG.  mcf_nc_write_plan is this call with row0 = 0, depth = 0 and a plan of the file's grid.
 * mcf_nc_write_missing (host only): missval in every variable of those rows of records [file_step0, file_step0 + nsteps) —
 * steps past the last whole day, the snow run's days of neither class.
 * mcf_nc_write_host_rows (host only): mcf_nc_write_host for a row block's arrays, vars[v] = [nrows, cols, nsteps]. */
int mcf_nc_write_plan_rows(mcf_ncfile *nc, mcf_plan *plan, int32_t slot, int32_t depth, int64_t row0, int64_t slot_step0,
                           int64_t file_step0, int64_t nsteps, float *kernel_ms);
int mcf_nc_write_missing(mcf_ncfile *nc, int64_t row0, int64_t nrows, int64_t file_step0, int64_t nsteps);
int mcf_nc_write_host_rows(mcf_ncfile *nc, int64_t row0, int64_t nrows, int64_t step0, int64_t nsteps,
                           const double *const vars[MCF_NOUT]);
/* One call: plan, file, chunk loop and close.  The file holds every step of tsteps; a step past the last whole day holds what
 * the array entry of the same run returns there — missval above ground; below ground Tz's values (Tbelowgroundv runs over every
 * step) with soilm missval — so the classic file is, byte for byte, the file mcf_nc_write_host writes from the arrays of
 * mcf_runmicro1 / 2 of the same run.  reqhgt >= 0: vector, fine-array and coarse-array forcing; reqhgt < 0: the streamed
 * below-ground plan, complete 0 and 1.  Chunks of opt->days_per_chunk days (0: sized as for the other sinks).  `multi` NULL: one
 * device (opt->device); set: row blocks as in mcf_runmicro_summary_multi, each block writing its strips (the blocks' values are
 * bit for bit the single device's, and so is the file).  The spec's rows, cols, nsteps and reqhgt must agree with `in` / `opt`
 * (MCF_ERR_ARG naming the field); the plan is created with exactly the file's variables.  Every refusal that needs no device —
 * null arguments, a variable writetonc does not define at that height, netcdf4 with several blocks (`multi` with n_blocks
 * other than 1) — comes before a device is touched, and its message starts with the entry's name. */
int mcf_runmicro_nc(const mcf_grid_inputs *in, const mcf_options *opt, const mcf_multi *multi, const char *path,
                    const mcf_nc_spec *spec);
/* One streamed solve, one file per depth: file d (paths[d]) holds Tz at depths[d] with that depth's long name ("Soil
 * temperature at depth h m") and, when selected, soilm — the same plane in every file.  The spec's reqhgt is not read.  The
 * refusals of mcf_plan_below_set_depths that need no plan come before a device is touched, under this entry's name. */
int mcf_runmicro_depths_nc(const mcf_grid_inputs *in, const mcf_options *opt, const double *depths, int32_t ndepths,
                           const double *tbp, const char *const *paths, const mcf_nc_spec *spec);
/* The snowpack's file.  The reference defines no such file (writetonc knows the solver's outputs only), so the convention is
 * this project's: variables named as mcf_snowdriver_out's fields, int32, missval -9999, on writetonc's dimensions, with
 *     series           stored as   units            long_name
 *     Tc               x 100       "deg C x 100"    "Canopy snow temperature"
 *     Tg               x 100       "deg C x 100"    "Ground snow temperature"
 *     groundsnowdepth  x 1000      "mm"             "Ground snow depth"            (the series is in m)
 *     totalSWE         x 100       "mm x 100"       "Total snow water equivalent"  (the series is in mm, after the redistribution)
 *     snowden          x 1         "kg / m^3"       "Snow density"
 * round half to even, NA and values outside int32 -> missval.  series[5] selects, in that order; scale[v] = 0 and a NULL
 * units[v] / long_name[v] take the table's.  Grid, coordinates, time, crs, format and deflate level as in mcf_nc_spec. */
typedef struct mcf_ncpack_spec {
    int32_t rows, cols;
    int64_t nsteps;
    const double *east, *north, *time_hours;
    const char *crs_wkt;
    int32_t series[5];
    double scale[5];
    const char *units[5];
    const char *long_name[5];
    int32_t format;
    int32_t deflate_level;
} mcf_ncpack_spec;
int mcf_nc_create_snowpack(const char *path, const mcf_ncpack_spec *spec, mcf_ncfile **nc);
/* The steps of chunk `chunk`, run last on the plan (mcf_snowplan_run_chunk), as rows [row0, row0 + plan rows) of a snowpack
 * file's records: packed on the device from the plan's step-major chunk series (k_pack_nc_planes; 4 B per value leave the
 * device), on the stream the model wrote them on.  Behind the last chunk the steps no chunk covers are written as missval.
 * MCF_ERR_STATE when a series of the file was switched off for the chunk (mcf_snowplan_set_series); MCF_ERR_ARG for a file that
 * is not a snowpack file, whose columns or steps are not the plan's, or a strip outside its grid. */
int mcf_snowplan_nc_write(mcf_snowplan *plan, mcf_ncfile *nc, int32_t chunk, int64_t row0);
/* The snow model alone (data.frame weather) with the file as its only sink: mcf_snowmodel1's chunk loop on device 0 (`multi`
 * NULL) or over row blocks, mcf_snowplan_nc_write behind every chunk.  The spec's rows, cols and nsteps must be the inputs'. */
int mcf_snowmodel1_nc(const mcf_snowdriver_in *in, const mcf_multi *multi, const char *path, const mcf_ncpack_spec *spec);
/* The snow run's files.  mcf_snowrun_nc_enable comes before mcf_snowrun_pass1, like the run's other two sinks (MCF_ERR_STATE
 * after it, or when called twice); either file may be NULL, not both; the run does not own them (close them after the passes).
 * micro_file (mcf_nc_create): pass 2 writes every merged ring chunk — runs of days in a class through mcf_nc_write_plan_rows at the
 * block's first row, days of neither class through mcf_nc_write_missing — then the days past the last whole chunk the same way and
 * the steps past the last whole day as missval: what the arrays of mcf_runmicrosnow1 / 2 hold there.  reqhgt >= 0 and the
 * below-ground run alike (the merged days lie in the slot either way).  Its variables must be among the run's.  pack_file
 * (mcf_nc_create_snowpack): mcf_snowplan_nc_write behind every chunk of pass 1.  With micro_file enabled mcf_snowrun_pass2 accepts
 * out == NULL or null arrays.  The grids and steps must be the run's; netcdf4 with more than one block is MCF_ERR_ARG.  Works on a
 * handle of mcf_snowrun_create_coarse as on any other (enable acts on the handle).
 * mcf_runmicrosnow_nc: one call — data.frame or array weather (mcf_runmicrosnow1 / 2 geometry), `multi` as there, reqhgt < 0 the
 * below-ground run; path / spec and pack_path / pack_spec: either pair may be NULL.  The files are created once the run exists
 * (no file without a device); every refusal that needs no device comes first, under the entry's name.  outs: all optional. */
typedef struct mcf_snowrun_nc_out {
    mcf_outputs *arrays;               /* or NULL: no host array */
    const mcf_snowdriver_out *smod;    /* or NULL */
    int32_t *snowday, *nosnowday;      /* [days] or NULL */
} mcf_snowrun_nc_out;
int mcf_snowrun_nc_enable(mcf_snowrun *run, mcf_ncfile *micro_file, mcf_ncfile *pack_file);
/* Between mcf_snowrun_pass1 and mcf_snowrun_pass2 (MCF_ERR_STATE otherwise): days with drop[d] != 0 leave the run's classes, so
 * that pass 2 treats them as days of neither class — not solved, NA in the arrays, missval in the file, never folded by a sink.
 * Only a day that is a no-snow day and no snow day may be dropped (MCF_ERR_ARG for a snow day: pass 1 has folded it into the
 * snow model's means).  For a caller that wants days left out of pass 2 (a gap it will not read), and the way the tests reach
 * the path that a melted pack's rounding residue takes by itself.  ndays: mcf_snowrun_days. */
int mcf_snowrun_drop_days(mcf_snowrun *run, const int32_t *drop, int32_t ndays);
int mcf_runmicrosnow_nc(const mcf_microsnow_in *in, const mcf_options *opt, const mcf_multi *multi, const char *path,
                        const mcf_nc_spec *spec, const char *pack_path, const mcf_ncpack_spec *pack_spec, mcf_snowrun_nc_out *outs);
/* Packs host planes through the device kernel, for its tests: series[v] = [nsteps][rows * cols] step-major doubles (cell
 * row + rows * col) or NULL for a series the file does not hold, as rows [row0, row0 + rows) of records [file_step0, ...). */
int mcf_nc_write_planes(mcf_ncfile *nc, const double *const series[5], int64_t rows, int64_t row0, int64_t file_step0,
                        int64_t nsteps, int32_t device, float *kernel_ms);

/* applycpp3 (src/microclimfCpp.cpp:5553-5588; `.runmicrosnow1/2` use it on totalSWE, R/internal.R:3592-3593):
 * reduction of a [rows,cols,tsteps] array over space, per time step, skipping NA.  fun: 0 mean, 1 sum,
 * 2 max, 3 min (max / min of an all-NA step: -Inf / +Inf, mean: NaN).  `count` (optional, [tsteps])
 * receives the number of non-NA cells so that row blocks of a tiled raster can be combined: sum and
 * count add, max / min combine by max / min (microclimf_amd/distributed.py).  At most 65535 steps per call. */
enum { MCF_APPLY_MEAN = 0, MCF_APPLY_SUM = 1, MCF_APPLY_MAX = 2, MCF_APPLY_MIN = 3 };
int mcf_applycpp3(const double *a, int64_t rows, int64_t cols, int64_t tsteps, int32_t fun, double *result,
                  double *count, int32_t device);

/* ---- host-side point model ---------------------------------------------------------
 * The O(tsteps) serial series that produce the grid solver's `pointm` in the reference:
 *   mcf_soilm()          soilmCpp        src/microclimfCpp.cpp:931-972   (_microclimf_soilmCpp)
 *   mcf_bigleaf()        BigLeafCpp      src/microclimfCpp.cpp:710-881   (_microclimf_BigLeafCpp)
 *   mcf_pointmprocess()  pointmprocess   src/microclimfCpp.cpp:5265-5323 (_microclimf_pointmprocess)
 *   mcf_weatherhgt()     weatherhgtCpp   src/microclimfCpp.cpp:884-929   (_microclimf_weatherhgtCpp)
 * as `runpointmodel` chains them (R/Cppwrappers.R:119-138).  They run on the HOST, as in the reference: ONE
 * point is a serial job (an energy balance iterated over the whole series, coupled through running means) and is
 * not part of the grid solver's hot path.  MANY points are not serial: the points of `runpointmodela` are
 * independent, and inside one BigLeaf iteration every hour reads only its own state of the iteration before; the
 * `_batch` entries below run them on the device, one lane per (point, hour).  vegp / groundp are read positionally as the reference does:
 * vegp = (h, pai, x, clump, lref, ltra, leafd, em, gsmax, q50), groundp = (gref, slope, aspect, em, rho, Vm, Vq,
 * Mc, b, psi_e, Smax, Smin).  One guard the reference lacks: its circular means index outside their arrays when
 * the window is longer than the series; mcf_bigleaf rejects yearG for 2..89 days and series under 6 steps. */
typedef struct mcf_point_weather {
    const double *temp, *relhum, *pres, *swdown, *difrad, *lwdown, *windspeed, *precip; /* [n]; precip: soilm only */
} mcf_point_weather;
typedef struct mcf_bigleaf_out { /* caller-allocated [n] each (src/microclimfCpp.cpp:867-879) */
    double *Tc, *Tg, *H, *G, *psih, *psim, *phih, *OL, *uf, *RabsG, *albedo;
    double err;
    int32_t iters;
} mcf_bigleaf_out;
int mcf_bigleaf(int64_t n, const mcf_obstime *obstime, const mcf_point_weather *weather, const double *vegp,
                const double *groundp, const double *soilm, double lat, double lon, double dTmx, double zref,
                int32_t maxiter, double bwgt, double tol, int32_t yearG, mcf_bigleaf_out *out);
int mcf_soilm(int64_t n, const mcf_point_weather *weather, double rmu, double mult, double pwr, double Smax,
              double Smin, double Ksat, double a, double *soilm_days /* [n / 24] */, int64_t *ndays);
int mcf_pointmprocess(int64_t n, const double *windspeed, const double *tc, const double *rh, const double *pk,
                      const double *uf, const double *soilm, const double *RabsG, double zref, double h, double pai,
                      double rho, double Vm, double Vq, double Mc, double *umu, double *kp, double *muGp,
                      double *DDp, double *T0p, double *dtrp);
int mcf_weatherhgt(int64_t n, const mcf_obstime *obstime, const mcf_point_weather *weather, double zin, double uzin,
                   double zout, double lat, double lon, double *temp, double *relhum, double *windspeed);
/* ---- the same three operators for P points at once, on the device (mcf_pointbatch.hip) ----
 *   mcf_bigleaf_batch()        BigLeafCpp      src/microclimfCpp.cpp:710-881   per point
 *   mcf_weatherhgt_batch()     weatherhgtCpp   src/microclimfCpp.cpp:884-929   per point
 *   mcf_pointmprocess_batch()  pointmprocess   src/microclimfCpp.cpp:5265-5323 per point
 * Semantics are those of the single-point entries, per point and without cross-talk: a point converges on its own
 * (`iters[p]`, `err[p]`; it is frozen after the ground-flux update of the iteration in which its largest temperature
 * change drops to `tol`, the others go on up to `maxiter`), and its results are bit-identical whatever batch it is in
 * and however the batch is cut into blocks.  Series are [P][n], a point's series contiguous; `obstime` [n] is shared;
 * vegp [P][10], groundp [P][12], lat / lon [P].  The batch entries take WHOLE DAYS only (n % 24 == 0); the other
 * refusals are mcf_bigleaf's (null arguments, P < 1, n < 6, yearG with 2..89 days) and are returned before the device
 * is touched; then MCF_ERR_NO_DEVICE without a HIP device.  About 30 series of 8 n bytes per point live on the device:
 * points are processed in blocks sized from the free memory, or of `points_per_block` points (0 = from free memory).
 * mcf_weatherhgt_batch runs mcf_weatherhgt's fixed canopy and ground through the batched BigLeaf (the annual term on
 * for one day or >= 90 days, as there). */
typedef struct mcf_bigleaf_batch_out { /* caller-allocated; series [P][n], a point's series contiguous */
    double *Tc, *Tg, *H, *G, *psih, *psim, *phih, *OL, *uf, *RabsG, *albedo;
    double *err;    /* [P] */
    int32_t *iters; /* [P] */
} mcf_bigleaf_batch_out;
int mcf_bigleaf_batch(int64_t P, int64_t n, const mcf_obstime *obstime, const mcf_point_weather *weather,
                      const double *vegp, const double *groundp, const double *soilm, const double *lat,
                      const double *lon, double dTmx, double zref, int32_t maxiter, double bwgt, double tol,
                      int32_t yearG, int64_t points_per_block, int32_t device, mcf_bigleaf_batch_out *out);
int mcf_weatherhgt_batch(int64_t P, int64_t n, const mcf_obstime *obstime, const mcf_point_weather *weather, double zin,
                         double uzin, double zout, const double *lat, const double *lon, int64_t points_per_block,
                         int32_t device, double *temp, double *relhum, double *windspeed);
int mcf_pointmprocess_batch(int64_t P, int64_t n, const double *windspeed, const double *tc, const double *rh,
                            const double *pk, const double *uf, const double *soilm, const double *RabsG, double zref,
                            const double *h, const double *pai, const double *rho, const double *Vm, const double *Vq,
                            const double *Mc, int32_t device, double *umu, double *kp, double *muGp, double *DDp,
                            double *T0p, double *dtrp);
/* _microclimf_pointmodelsnow (src/microclimfCpp.cpp:4000-4169; called by `.snowmodel1`, R/internal.R:2536): the snow
 * branch's point model.  vegp = (pai, hgt, ltra, clump), other = (slope, aspect, lat, lon, zref, initial depth,
 * initial age); snowenv: MCF_SNOWENV_*; the reference's defaults are tol = 0.5, maxiter = 100.  Outputs: [n] each,
 * sdepc / sdepg [n + 1] (the depth after the last step is kept, as in the reference).  Host code. */
typedef struct mcf_pointsnow_out {
    double *Tc, *Tg, *sdepc, *sdepg, *sdenc, *sdeng, *G, *RswabsG, *RlwabsG, *tr, *umu, *sublmelt, *tempmelt, *rainmelt,
        *sstemp;
    double mxdif;
    int32_t iters;
} mcf_pointsnow_out;
int mcf_pointmodelsnow(int64_t n, const mcf_obstime *obstime, const mcf_point_weather *weather, const double *vegp,
                       const double *other, int32_t snowenv, double tol, double maxiter, mcf_pointsnow_out *out);
/* mcf_pointmodelsnow for P points at once, on the device (mcf_pointbatch.hip): what `runsnowmodel` runs once per cell of
 * the climate grid with array weather.  Semantics are those of mcf_pointmodelsnow, per point and without cross-talk.
 * Layout: series [P][n] (sdepc / sdepg [P][n + 1]), a point's series contiguous; `weather` [P][n] each, precip too;
 * `obstime` [n] is shared; vegp [P][4], other [P][7], snowenv [P]; mxdif / iters [P], each point's own.
 * Freeze rule: a pass is the sweep over the series and GFluxCppsnow on the new Tg; a point stops after the ground-flux
 * update of the pass in which its mxdif <= tol, or when ++iter > maxiter (at most floor(maxiter) + 1 passes, as on the
 * host); a stopped point is frozen while the others go on, and G is its flux after its last update.  The running maximum
 * ignores NaN as fmax does.  A point's bits do not depend on the batch it is in, on `points_per_block` or on the run.
 * Refusals, returned before the device is touched: null arguments or null output vectors, P < 1, n % 24 != 0 (WHOLE
 * DAYS only, as for the other `_batch` entries), n < 24, n > 2^28, points_per_block < 0; then MCF_ERR_NO_DEVICE without
 * a HIP device.  Memory: 36 series of 8 n bytes per point live on the device (rows padded to whole waves of 64 points;
 * sized as 45 to leave room): points are processed in blocks sized from the free memory, or of `points_per_block`
 * points (0 = from free memory); all points of a block are in flight in one launch. */
typedef struct mcf_pointsnow_batch_out { /* caller-allocated; a point's series contiguous */
    double *Tc, *Tg, *sdenc, *sdeng, *G, *RswabsG, *RlwabsG, *tr, *umu, *sublmelt, *tempmelt, *rainmelt, *sstemp; /* [P][n] */
    double *sdepc, *sdepg; /* [P][n+1] */
    double *mxdif;         /* [P] */
    int32_t *iters;        /* [P] */
} mcf_pointsnow_batch_out;
int mcf_pointmodelsnow_batch(int64_t P, int64_t n, const mcf_obstime *obstime,
                             const mcf_point_weather *weather /* [P][n], precip too */, const double *vegp /* [P][4] */,
                             const double *other /* [P][7] */, const int32_t *snowenv /* [P] */, double tol, double maxiter,
                             int64_t points_per_block, int32_t device, mcf_pointsnow_batch_out *out);
/* ---- fast snow method for subset runs (R/internal.R:2627-2776 `.snowmodelq1`): its three kernels of arithmetic ----
 * mcf_canintfrac replaces _microclimf_canintfrac (src/microclimfCpp.cpp:5417-5450): frac = canopysnowintCpp(hgt, pai,
 *   uf, prec, tc, Li) / prec per cell, 0.5 everywhere when prec is not > 0, NaN where hgt is NA.  Host code.
 * mcf_meltmu replaces _microclimf_meltmu (:5454-5492): per cell sum over the n steps of max(0, (stemp - tc) * skyview +
 *   tc) over sum of max(0, stemp); 1 everywhere when the denominator is 0; NaN where skyview is NA.  Host code.
 * mcf_tpicalc replaces `.tpicalc` (R/internal.R:2483-2496) on the device: exp((aggregate(dtm, af, na.rm) resampled
 *   bilinearly - dtm) * tfact), or the raster mean in place of the aggregate when af >= min(dim) / 2, values below 0.05
 *   set to 0.1 and above 10 to 10 as in the reference, divided by the raster mean.  [rows, cols] column-major. */
int mcf_canintfrac(int64_t cells, const double *hgt, const double *pai, double uf, double prec, double tc, double Li,
                   double *frac);
int mcf_meltmu(int64_t cells, const double *skyview, int64_t n, const double *stemp, const double *tc, double *mu);
/* mcf_meltmu2 replaces _microclimf_meltmu2 (:5495-5527, `.snowmodelq2`): the same with stemp / tc per cell, [cells, n]
 * with the cell index fastest (an R array [rows, cols, n]); 0.5 where the denominator is 0.  Host code. */
int mcf_meltmu2(int64_t cells, int64_t n, const double *mu, const double *stemp, const double *tc, double *out);
int mcf_tpicalc(int64_t rows, int64_t cols, const double *dtm, int32_t af, double tfact, double *tpic, int32_t device);
/* mcf_snowmodelq1: the day loop of `.snowmodelq1` (R/internal.R:2690-2776) resident on the device — what
 * runsnowmodel(method = "fast") runs for a subset point model (R/Cppwrappers.R:717-735).  Once per call the terrain of the
 * bare dtm (:2690-2706: slope / aspect with NA -> 0 / 180 and masked by the dtm, hor x24, sky view, wsa with s = 10 if
 * res <= 100 else 1), the step table of the n selected hours (each day's gridmodelsnow1 call restarts the albedo clock) and
 * intfrac = canintfrac(hgt, pai, 2, mean(snow_all[snow_all > 0]), mean(selected temp), 0) with isnowdg = (1 - intfrac)
 * isnowdc (:2708-2716).  Per selected day: the pack moved over the gap `sbtn = (ped + 1):(subs[first] - 1)` (R's `a:b`: two
 * consecutive selected days give the two hours ped + 1, ped) by the point model's balance, its temperature melt scaled per
 * cell by meltmu (:2724-2741; the gap's sums and means formed by the host left to right), gridmodelsnow1 on the day's 24
 * hours (:2742), `.tpicalc(af, min(dim), dtm, tfact)` with af = round(10 sqrt(mean wind of the day) / res) — of the BARE dtm:
 * the ground depth the reference stacks on it is still zero when read (:2750-2753) —, the redistribution of the ground
 * layer's change and the hand-over of step 24's depths (:2744-2771).  Snow ages are not handed on (every day starts from
 * isnowac / isnowag).  Nothing per cell crosses PCIe but the inputs, once, and the wanted series, each day's while the next
 * day computes.  `out`: `.snowmodelq1`'s list minus umu, [rows,cols,n] each, NULL = not wanted (neither finished nor
 * downloaded); totalSWE = sdepc * sden, as the reference returns it.
 * MCF_ERR_ARG before any device is touched: null arguments, n = 0 or not whole days, subs outside 1..n_all or not
 * increasing, array_forcing != 0, a first selected day that is the first day of the series (subs[0] - 1 <= 1: the reference
 * fails there, `sbtn` not found), a day whose aggregation factor rounds to 0.  One device, one block: a raster that does not
 * fit is MCF_ERR_NOMEM (the position index and the terrain stencil couple row blocks; no `_multi` form).
 * mcf_canintfrac_device / mcf_meltmu_device: mcf_canintfrac / mcf_meltmu through the two kernels the call above uses
 * (upload, one launch, download). */
typedef struct mcf_snowfast_in {
    mcf_snowdriver_in drv;  /* drv.base: obstime / clim / pointm of the n = base.tsteps SELECTED hours (vector forcing, whole days),
                               vegp = .sortl's means (leaft NA -> 0.01 done by the caller), other.{lat, lon, zref, isnowdc, isnowac, isnowag};
                               other.{isnowdg, slope, aspect, skyview, wsa, hor} ignored; drv.dtm, drv.res, drv.tfact; chunk_steps, af_* ignored */
    int64_t n_all;          /* length of the complete hourly series */
    const int64_t *subs;    /* [n] 1-based positions of the selected hours in it */
    const double *sublmelt, *tempmelt, *rainmelt, *sstemp, *sdenc, *sdeng;   /* [n_all] pointmodelsnow over the whole series */
    const double *temp_all, *snow_all;                                        /* [n_all] air temperature; precip where temp <= 2, else 0 */
} mcf_snowfast_in;
int mcf_snowmodelq1(const mcf_snowfast_in *in, mcf_snowdriver_out *out, int32_t device);
int mcf_canintfrac_device(int64_t cells, const double *hgt, const double *pai, double uf, double prec, double tc, double Li, double *frac, int32_t device);
int mcf_meltmu_device(int64_t cells, const double *skyview, int64_t n, const double *stemp, const double *tc, double *mu, int32_t device);
/* mcf_snowmodelq2: the day loop of `.snowmodelq2` (R/internal.R:3219-3286), the fast snow method for ARRAY weather, resident on
 * the device with the coarse climate and point-model arrays left coarse.  Coarse arrays are R arrays [coarse_rows, coarse_cols,
 * hours] (column-major: one hour's coarse cells are contiguous); coarse_rowpos / coarse_colpos as in mcf_grid_inputs.  Every
 * resampling is the bilinear tap (1 - wx) a00 + wx a01, the same for the lower pair, (1 - wy) top + wy bot, without FMA
 * contraction: a tap has the bits of the host's resampling, so thresholds (`stemp > 0`, the clamps at 0) fall on the same side.
 * Once per call: the terrain of the bare dtm, the date table, the dtm's mean and the position-index cache as in
 * mcf_snowmodelq1; intfrac = canintfrac(hgt, pai, 2, msnow, mtemp, 0) with msnow the mean of the positive entries of coarse
 * `snow` and mtemp = mean(cca(tc), na.rm = TRUE) formed as (sum over the non-hole cells of the tap of the per-coarse-cell time
 * sums) / (count x n_all) by the device's deterministic reduction — the reference adds the [rows, cols, n_all] array left to
 * right; the two differ by rounding only, and mtemp feeds canopysnowintCpp's storage term alone.
 * Per selected day: the pack moved over the gap by the resampled point-model balance, its temperature melt scaled per cell by
 * meltmu2 of the resampled sstemp / tc (:3229-3244; the six gap sums per coarse cell formed by the host left to right, the
 * taps and the balance in one kernel); no adjustment, only the clamps, on a first day with subs[0] - 1 <= 1 (accepted here);
 * the day's thirteen series on the raster from the coarse arrays (:3112-3164: `.cca` masked by the dtm, pressure and wind
 * unmasked, altcorrect 0 / 1 / 2, relhum capped at 100); gridmodelsnow2; `.tpicalc` with af = round(10 sqrt(mean af_wind) /
 * res); redistribution and hand-over as in mcf_snowmodelq1; all outputs NA on the dtm's holes (`.cleansmod`).
 * MCF_ERR_ARG before any device is touched: null arguments (named), n = 0 or not whole days, subs outside 1..n_all or not
 * increasing, coarse_rows / coarse_cols < 1, null positions or one outside the coarse grid, altcorrect outside 0..2 or > 0
 * without coarse_dtm, a day whose
 * aggregation factor rounds to 0, 24 x coarse cells x 8 B >= 2^32.  One device, one block: MCF_ERR_NOMEM if the raster does
 * not fit (the day's thirteen series are 13 x 24 x 8 B per cell).
 * mcf_meltmu2_device: the gap kernel alone — mu [rows, cols] from skyview, the dtm (its holes mask the taps) and coarse
 * sstemp / tc [crows, ccols, n] (upload, one launch, download). */
typedef struct mcf_snowfast2_in {
    mcf_snowdriver_in drv;  /* drv.base: rows, cols, tsteps = n SELECTED hours (whole days), snowenv, obstime [n], clim.winddir [n] = the
                               one direction per hour the model takes (atan2 of the wind components' spatial means), vegp = .sortl's
                               means (leaft NA -> 0.01 done by the caller), other.{lats, lons, zref, isnowdc, isnowac, isnowag}; the
                               other members of clim / pointm / other are ignored.  drv.dtm, drv.res, drv.tfact; drv.af_wind [n] =
                               sqrt(wuv^2 + wvv^2) of the components' spatial means; chunk_steps, af_wsa_s ignored */
    int64_t coarse_rows, coarse_cols;
    const double *coarse_rowpos, *coarse_colpos;   /* [rows], [cols] */
    int32_t altcorrect;                             /* 0, 1 (fixed lapse rate), 2 (moist adiabatic) */
    int32_t reserved;
    const double *coarse_dtm;                       /* [crows, ccols], NA read as 0; needed when altcorrect > 0 */
    /* the selected hours, [crows, ccols, n].  windu / windv: windspeed x cos / sin of the coarse direction, formed by the caller */
    const double *temp, *relhum, *pres, *swdown, *difrad, *lwdown, *precip, *windu, *windv;
    const double *Gp, *Tc, *RswabsG, *RlwabsG, *umu;   /* the snow point model per climate cell */
    int64_t n_all;          /* length of the complete hourly series */
    const int64_t *subs;    /* [n] 1-based positions of the selected hours in it */
    const double *sublmelt, *tempmelt, *rainmelt, *snow, *sstemp, *tc, *sdenc, *sdeng;   /* the whole series, [crows, ccols, n_all] */
} mcf_snowfast2_in;
typedef struct mcf_snowfast2_out {
    mcf_snowdriver_out smod;   /* as mcf_snowmodelq1 */
    double *umu;               /* [rows,cols,n] pointm$umu on the raster, the list's sixth element; NULL = not wanted */
} mcf_snowfast2_out;
int mcf_snowmodelq2(const mcf_snowfast2_in *in, mcf_snowfast2_out *out, int32_t device);
int mcf_meltmu2_device(int64_t rows, int64_t cols, const double *skyview, const double *dtm, int64_t crows, int64_t ccols,
                       const double *rowpos, const double *colpos, int64_t n, const double *sstemp_c, const double *tc_c,
                       double *mu_out, int32_t device);
/* mcf_snowmodel2_coarse: the chunk loop of `.snowmodel2` (the slow snow method for ARRAY weather, R/internal.R:2862-3013) with the
 * coarse climate and point-model arrays left coarse on the device — mcf_snowmodel2's loop, its thirteen uploads per chunk replaced
 * by one kernel that expands the chunk's hours from the resident coarse arrays (14 x coarse cells x T x 8 B, uploaded once) into
 * the buffers the snow kernel reads: `.cca` masked by the dtm, pressure and wind components unmasked, altcorrect 0 / 1 / 2 (the
 * host takes the coarse pressure to sea level), relhum capped at 100 — the arithmetic and the bits of mcf_snowmodelq2's day
 * expansion.  Terrain refresh, position index (af_wind, floor of 2), af_wsa_s, `1:n5days` truncation with at least one chunk,
 * other$isnowdg never updated: as mcf_snowmodel2.  out->umu: pointm$umu on the raster for ALL T steps (the steps behind the last
 * whole chunk too, where the other five stay NA); every series is NA on the dtm's holes.  One device, one block: MCF_ERR_NOMEM if
 * the chunk's series (18 x chunk_steps x 8 B per cell) do not fit.
 * mcf_snow_expand_coarse_device: the expansion kernel alone (upload, one launch, download) for steps step0 .. step0 + nsteps - 1;
 * fine[k]: [rows, cols, nsteps] in the order temp, relhum, pres, swdown, difrad, lwdown, windspeed, precip, Gp, Tc, RswabsG,
 * RlwabsG, umu (what mcf_snowmodel2 takes as clim / pointm).  It reads drv.base.{rows, cols, tsteps}, drv.dtm, the positions, the
 * coarse arrays, coarse_dtm and altcorrect only.
 * MCF_ERR_ARG before any device is touched, the message naming the entry and the input: a null argument, coarse_rows /
 * coarse_cols < 1, a position outside the coarse grid, altcorrect outside 0..2 or > 0 without coarse_dtm, 24 x coarse cells x
 * 8 B >= 2^32, chunk_steps not whole days, drv.base.array_forcing == 0; for the expansion step0 < 0, nsteps < 1 or step0 +
 * nsteps > T. */
typedef struct mcf_snowcoarse_in {
    mcf_snowdriver_in drv;  /* drv.base: rows, cols, tsteps = T, array_forcing != 0, snowenv, obstime [T], clim.winddir [T] (one
                               direction per hour), vegp, other.{lats, lons, zref, isnowdc, isnowdg, isnowac, isnowag}; drv.dtm,
                               res, tfact, chunk_steps, af_wsa_s, af_wind [T]; the other members of clim / pointm are ignored */
    int64_t coarse_rows, coarse_cols;
    const double *coarse_rowpos, *coarse_colpos;   /* [rows], [cols] */
    int32_t altcorrect;                             /* 0, 1 (fixed lapse rate), 2 (moist adiabatic) */
    int32_t reserved;
    const double *coarse_dtm;                       /* [crows, ccols], NA read as 0; needed when altcorrect > 0 */
    /* [crows, ccols, T].  windu / windv: windspeed x cos / sin of the coarse direction, formed by the caller */
    const double *temp, *relhum, *pres, *swdown, *difrad, *lwdown, *precip, *windu, *windv;
    const double *Gp, *Tc, *RswabsG, *RlwabsG, *umu;   /* the snow point model per climate cell */
} mcf_snowcoarse_in;
int mcf_snowmodel2_coarse(const mcf_snowcoarse_in *in, mcf_snowfast2_out *out, int32_t device);
int mcf_snow_expand_coarse_device(const mcf_snowcoarse_in *in, int64_t step0, int64_t nsteps, double *const fine[13], int32_t device);
/* The snow-day microclimate's weather from coarse arrays: `.prepsnowinputs2` (R/internal.R:3445-3579) on the device.  Its nine
 * series are NOT `.snowmodel2`'s: temperature and pressure are resampled unmasked, the vapour pressure is resampled (the caller
 * forms `ea` = satvap(temp) x relhum / 100 on the climate grid, as it forms windu / windv), with altcorrect 1 / 2 the temperature
 * moves by elevd x lapse rate (5 / 1000, or the moist adiabatic one of the resampled temp / ea / pres), relative humidity is
 * ea / satvap(temp) x 100 kept within 20 .. 100 in every altitude mode, swdown / difrad / lwdown / precip / umu are `.cca`
 * (NA on the dtm's holes), the wind speed comes from the resampled components.  `pres` is the coarse pressure as the climate
 * data have it; with altcorrect > 0 the library takes it to sea level on the coarse grid and back up by the cell's own factor.
 * mcf_microsnow_expand_coarse_device: the expansion kernel alone (upload, one launch, download) for steps step0 .. step0 +
 * nsteps - 1; fine[k]: [rows, cols, nsteps] in the order temp, relhum, pres, swdown, difrad, lwdown, windspeed, precip, umu (what
 * mcf_gridmicrosnow2 takes as clim); a NULL fine[k] is a series that is not wanted (the kernel's series mask), at least one is
 * needed.  MCF_ERR_ARG before any device is touched, the message starting with the entry's name: a null argument, coarse_rows /
 * coarse_cols < 1, a position outside the coarse grid, altcorrect outside 0..2 or > 0 without coarse_dtm, 24 x coarse cells x
 * 8 B >= 2^32, step0 < 0, nsteps < 1 or step0 + nsteps > tsteps. */
typedef struct mcf_microcoarse_in {
    int64_t rows, cols, tsteps;
    const double *dtm;                              /* [rows, cols], NaN = NA */
    int64_t coarse_rows, coarse_cols;
    const double *coarse_rowpos, *coarse_colpos;   /* [rows], [cols] */
    int32_t altcorrect;                             /* 0, 1 (fixed lapse rate), 2 (moist adiabatic) */
    int32_t reserved;
    const double *coarse_dtm;                       /* [crows, ccols], NA read as 0; needed when altcorrect > 0 */
    /* [crows, ccols, tsteps].  windu / windv: windspeed x cos / sin of the coarse CELL's own direction */
    const double *temp, *ea, *pres, *swdown, *difrad, *lwdown, *windu, *windv, *precip, *umu;
} mcf_microcoarse_in;
int mcf_microsnow_expand_coarse_device(const mcf_microcoarse_in *in, int64_t step0, int64_t nsteps, double *const fine[9], int32_t device);
/* mcf_runmicrosnow2_coarse: the array-weather snow run (mcf_runmicrosnow2) with every coarse array left coarse — `.snowmodel2`'s
 * loop as mcf_snowmodel2_coarse runs it, the solver on a coarse plan (grid->array_forcing == 2: the whole coarse series resident,
 * mcf_plan_upload_forcing_days a no-op), and gridmicrosnow2 on slabs the kernel above fills per run of consecutive snow days.
 * Nothing of size cells x steps goes up; the ten outputs (and smod, if asked for) come down.
 *   grid    runmicro2Cpp's coarse arguments (array_forcing = 2)
 *   snow    as for mcf_snowmodel2_coarse
 *   micro   the ten coarse arrays of the microclimate's weather; its own set (the two preparations differ in wind direction and
 *           in the reference-height scaling), resident beside the snow model's: 10 x coarse cells x T x 8 B
 *   micro_static  gridmicrosnow2's other inputs for the WHOLE series as mcf_runmicrosnow2's `micro`, the nine weather arrays
 *           null: obstime [T], clim.winddir [T], `.sortl2` vegetation, bare-ground terrain, lats / lons, zref, Smax.  May be
 *           NULL only if the period has no snow day
 *   mat     as mcf_runmicrosnow2
 * Pass 2 re-runs a snow chunk from its checkpoint (the expansion runs again inside it), solves the chunk's no-snow days whole
 * (mcf_snowrun_stats reports nothing left out; the per-cell temperature cap is taken over the no-snow days by
 * mcf_plan_set_mxtc_days, bit for bit that of a coarse plan made on the host-subset arrays) and runs the snow-day kernel over
 * the slot.  smod->umu: all T steps, the series NA on the dtm's holes, as mcf_snowmodel2_coarse.  One block on one device.
 * mcf_snowrun_create_coarse: the staged form; mcf_snowrun_pass1 / _pass2 (its `micro` = micro_static) / _destroy work on the
 * handle.  multi: NULL, or one block on one device; umu_out: where pass 1 hands pointm$umu [rows, cols, T], or NULL.
 * MCF_ERR_ARG before a device is touched, the message starting with the entry's name: a null argument (named); the three groups
 * disagreeing in rows / cols / T, coarse rows / cols, positions or altcorrect; grid->array_forcing != 2; reqhgt < 0; more than
 * one block or device; what mcf_snowmodel2_coarse and the expansion entry refuse of their groups.  MCF_ERR_NOMEM if a chunk's
 * series and the nine slabs do not fit. */
typedef struct mcf_microsnow_coarse_in {
    const mcf_grid_inputs *grid;
    const mcf_snowcoarse_in *snow;
    const mcf_microcoarse_in *micro;
    const mcf_snow_inputs *micro_static;
    double mat;
} mcf_microsnow_coarse_in;
int mcf_runmicrosnow2_coarse(const mcf_microsnow_coarse_in *in, const mcf_options *opt, mcf_outputs *out, const mcf_snowfast2_out *smod);
int mcf_snowrun_create_coarse(const mcf_microsnow_coarse_in *in, const mcf_options *opt, const mcf_multi *multi, double *umu_out,
                              mcf_snowrun **run);
/* manCpp(src/microclimfCpp.cpp:597-627): circular trailing mean, via daily means for windows beyond 48 steps. */
int mcf_man(int64_t n, const double *x, int32_t window, double *out);

/* ---- topographic wetness index (soilc$twi) ------------------------------------------------
 * mcf_flowacc replaces _microclimf_flowaccCpp (src/microclimfCpp.cpp:5368-5408, with flowdirCpp :5326-5366),
 * mcf_topidx the R function `.topidx` around it (R/internal.R:861-874).  Host code as in the reference: one
 * elevation-ordered sweep over the whole raster, run once per raster (see mcf_hydro.cpp for the reference
 * behaviours kept: self-pointing pits, the 9999.99 m ceiling, tie order, NA cells = -2147483648 in `fa`).
 * `dtm`, `fa`, `twi`: [rows, cols] column-major; NaN = NA. */
int mcf_flowacc(int64_t rows, int64_t cols, const double *dtm, double *fa);
int mcf_topidx(int64_t rows, int64_t cols, const double *dtm, double xres, double yres, double *twi);
/* The same on the device (mcf_hydro.hip; host pointers in and out): the elevation-ordered sweep restated as a subtree count
 * over the forest of the edges that run forward in the order, found by pointer doubling with integer atomics — `fa` equals
 * mcf_flowacc's exactly, ties and plateaus included, and is bit-reproducible; `twi` equals mcf_topidx's up to the last bits of
 * atan / tan (the median of the slopes is the exact order statistic).  At most 2^31 - 1 cells. */
int mcf_flowacc_device(int64_t rows, int64_t cols, const double *dtm, double *fa, int32_t device);
int mcf_topidx_device(int64_t rows, int64_t cols, const double *dtm, double xres, double yres, double *twi, int32_t device);

/* ---- leaf and ground reflectance from albedo (vegp$leafr, vegp$leaft, soilc$gref) -------------
 * The reference's exported leafrfromalb() (R/dataprep.R:1000-1050) inverts the diffuse two-stream albedo per cell by
 * bisection.  mcf_find_lref / mcf_find_gref replace _microclimf_find_lref / _microclimf_find_gref
 * (src/microclimfCpp.cpp:5675-5724, with leafrcpp :5594-5626, solve_lref :5629-5648, solve_gref :5652-5672), mcf_fill_na
 * replaces _microclimf_fill_naCpp (:5727-5777).  Rasters are [rows, cols] column-major, NaN = NA; a result cell is NA
 * (R's NA_real_) where any of its four inputs is, and in find_gref where the 100 steps find no root.  Brackets 0.0001..0.6665
 * (lref) and 0.0001..0.9999 (gref), tolerance 1e-6 on the albedo residual; a step whose f_lower * f_mid < 0 is false moves
 * `lower`, a NaN product included.  mcf_fill_na: every NA cell inside the mask (mask not NA) takes the value of the source
 * the reference's breadth-first search reaches it from first (4 neighbours, sources queued column-major, neighbours tried as
 * row - 1, row + 1, col - 1, col + 1); cells where the mask is NA keep what `m` holds, unreachable cells stay NA.  `out` may
 * be `m`.  Host code; `ltrr` must be finite. */
int mcf_find_lref(int64_t rows, int64_t cols, const double *pai, const double *gref, const double *x, const double *albin,
                  double ltrr, double *lref_out);
int mcf_find_gref(int64_t rows, int64_t cols, const double *lref, const double *pai, const double *x, const double *albin,
                  double ltrr, double *gref_out);
int mcf_fill_na(int64_t rows, int64_t cols, const double *m, const double *mask, double *out);
/* The same on the device (mcf_vegprep.hip; host pointers in and out), from the same arithmetic (mcf_vegprep.h): bit for bit
 * the host entries' values unless exp / pow / cos of the two math libraries differ by enough to flip one root test; the fill
 * is exact.  At most 2^31 - 1 cells. */
int mcf_find_lref_device(int64_t rows, int64_t cols, const double *pai, const double *gref, const double *x,
                         const double *albin, double ltrr, double *lref_out, int32_t device);
int mcf_find_gref_device(int64_t rows, int64_t cols, const double *lref, const double *pai, const double *x,
                         const double *albin, double ltrr, double *gref_out, int32_t device);
int mcf_fill_na_device(int64_t rows, int64_t cols, const double *m, const double *mask, double *out, int32_t device);
/* The whole loop of leafrfromalb() (R/dataprep.R:1007-1049): tst = exp(-mean(pai)) < 0.5 solves lref first, lref starts at
 * 0.25 + 0.5 alb and gref at 0.15 (NA where x is), both solves are filled inside the mask x, the update is half old and half
 * new, and the loop ends when max(mean|gref - gref2|, mean|lref - lref2|) <= 0.001 or after 50 passes.  leaft = ltrr * leafr.
 * On the device the rasters go up once and the three results come down once.  A pai without a single value is refused
 * (R stops there with a missing value). */
typedef struct {
    double *leafr, *leaft, *gref; /* [rows, cols] each, caller-owned */
    int32_t iterations;           /* passes done */
    int32_t lref_first;           /* 1: the tst < 0.5 branch was taken */
    double mxdif_gref, mxdif_leaf;/* the two mean absolute differences of the last pass */
} mcf_leafr_out;
int mcf_leafrfromalb(int64_t rows, int64_t cols, const double *pai, const double *x, const double *alb, double ltrr,
                     mcf_leafr_out *out);
int mcf_leafrfromalb_device(int64_t rows, int64_t cols, const double *pai, const double *x, const double *alb, double ltrr,
                            mcf_leafr_out *out, int32_t device);
/* Diagnostics of the above, used by tests.  kind 0 / 1: leafrcpp(a = lref, b = pai, c = gref, d = x, e = albin, ltrr)
 * elementwise as the host unit / the device unit evaluates it, out[rows * cols].  kind 2: mcf_leafrfromalb_device(a = pai,
 * b = x, c = alb) with `block` (64, 128 or 256) threads per workgroup in the per-cell and fill kernels; out[3 rows cols + 4]:
 * leafr, leaft, gref, then iterations, mxdif_gref, mxdif_leaf, lref_first. */
int mcf_selftest_vegprep(int32_t kind, int64_t rows, int64_t cols, const double *a, const double *b, const double *c,
                         const double *d, const double *e, double ltrr, double *out, int32_t block, int32_t device);

/* ---- height profiles from one plan ---------------------------------------------------------------------
 * The foliage profile of `.foliageden` (R/internal.R:937-946) with the shape 1.5 and rate 1.5 / 7 every call site of the
 * reference uses: for each of n values, x = ((hgt - z) / hgt) 10, leafden = (pai / hgt) (dgamma(x) / td) 10 and
 * paia = pgamma(x) (pai / td), td = pgamma(10).  z >= hgt gives exact zeros, hgt = 0 gives paia 0 and leafden NaN (the
 * reference's 0 / 0), a NaN hgt or pai propagates.  The gamma functions are the closed forms of shape 3/2 with a series near
 * the canopy top (mcf_foliage.h): within 2^-40 relative of R's pgamma / dgamma.  mcf_foliageden is the host twin;
 * mcf_foliageden_device is upload, one launch (k_foliage) and download. */
int mcf_foliageden(int64_t n, const double *hgt, const double *pai, double z, double *leafden, double *paia);
int mcf_foliageden_device(int64_t n, const double *hgt, const double *pai, double z, double *leafden, double *paia,
                          int32_t device);
/* Re-targets a plan to another height above ground: everything but vegp$paia, vegp$leafden and reqhgt itself stays resident.
 * The plan's stream is synchronised, leafden and paia of every layer are derived on the device from the resident hgt and pai
 * (k_foliage), reqhgt is replaced and the per-cell images and tile classes are rebuilt before the next run: the outputs are
 * bit for bit those of a plan created at `reqhgt` with these two planes.  `paia`: NULL, or a host [rows, cols, layers]
 * array, laid out as vegp$paia was at creation (row_pitch included), that takes the place of the derived plant area above
 * (leafden is always derived, as in the reference).
 * For a tiled plan created with reqhgt >= 0: vector, array or coarse array forcing, any number of vegetation layers, with or
 * without period summaries (mcf_plan_summary_reset starts the next height's statistics).  MCF_ERR_ARG: a null plan, reqhgt <= 0
 * or NaN (0: mcf_runmicro*; below ground: mcf_runmicro_depths); MCF_ERR_STATE: a below-ground plan, a plan with diagnostics
 * enabled.  Every message starts with the entry's name. */
int mcf_plan_set_height(mcf_plan *plan, double reqhgt, const double *paia);
/* The two planes the plan holds now, [rows, cols, layers] each, dense (either may be NULL). */
int mcf_plan_fetch_foliage(mcf_plan *plan, double *paia, double *leafden);
/* One call for a profile: one plan and one ring; per height mcf_plan_set_height, the day-chunk driver of mcf_runmicro1 and the
 * fetches.  heights: nheights values > 0; out: nheights caller-allocated mcf_outputs structs, opt->out selecting the variables
 * of every height; paia: NULL, or nheights pointers each of which may be NULL (mcf_plan_set_height's `paia`).  in->vegp.paia and
 * in->vegp.leafden are not read and may be NULL; opt->reqhgt is ignored.  Vector forcing (static or layered vegetation) and
 * coarse array forcing (array_forcing = 2); no `_multi` form.  A null or empty list and a height <= 0 or NaN are refused
 * before any device is touched (MCF_ERR_ARG, the message starting with the entry's name). */
int mcf_runmicro_heights(const mcf_grid_inputs *in, const mcf_options *opt, const double *heights, int32_t nheights,
                         const double *const *paia, mcf_outputs *out);

/* Diagnostics: evaluate one of the solver's lean device elementary functions
 * elementwise on host arrays (kind 0 exp, 1 log, 2 x/y, 3 sqrt, 4 1/x, 5 satvap
 * (cpp:480-490), 6 x^y); used by tests to bound their error against libm. */
int mcf_selftest_math(int32_t kind, const double *x, const double *y, double *out, int64_t n,
                      int32_t device);

/* Diagnostics: the per-cell-step sun position and humidity helpers of array forcing, elementwise, one lane per element.
 * `in` holds nin planes of n doubles, `out` nout planes of n doubles (plane f of element i at [f * n + i]); used by tests to
 * hold each field against a high-precision evaluation of the reference's formulas.
 *   kind 0, 1, 2: nin = 11: year, month, day, hour, winddir, lat, lon, tc, pk, rsw, rdif.
 *   kind 0 (nout = 29): the solver's array-forcing step — the date row as the date set-up makes it, the cell constants
 *     (sin / cos of the latitude and of B = 0.261799 * 4 lon / 60) as the cell set-up makes them, then derive_time_af and
 *     derive_time_af_pass2.  Planes: 0 CZ, 1 SZ, 2 TANSA, 3 ZEND, 4 COSC, 5 TANC, 6 TAN2C, 7 INV2COSC, 8 SAZ, 9 CAZ, 10 sindex,
 *     11 windex, 12 ksat, 13 DE, 14 GHRRAD, 15 REM, 16 LAPK, 17 WFAC, 18 RBEAM, 19 RB; after pass 2: 20 GHRRAD, 21 REM, 22 MUPM,
 *     23 INVMUPM; the date row: 24 sin dec, 25 cos dec, 26 cos A, 27 sin A (A = 0.261799 * (hour + eot / 60 - 12)); 28 julday.
 *   kind 1 (nout = 29): the literal device route of vector forcing (sol_date, sol_site, derive_time) on the same inputs, the
 *     same planes; 26 holds the equation of time (minutes), 27 NaN.  Fields the route reads and this entry does not supply
 *     (Gp, muGp, ...) are 1.
 *   kind 2 (nout = 21): the snow kernels' sun (sun_cell + sun_at_cell) from the same date row: 0 zend, 1 cosz, 2 cz, 3 sz,
 *     4 tansa, 5 kx, 6 kcos, 7 sa, 8 ca, 9 sindex; beside it the literal sol_site + sun_derive(degrees = 0): 10 .. 18 in the same
 *     order, 19 tansa of sun_derive(degrees = 1), 20 the literal horizon sector.
 *   kind 3 (nin = 3: tc, rh, pk; nout = 4): the R-side humidity helpers: 0 es = satvap_r(tc), 1 ea = es rh / 100,
 *     2 dewpoint_r(ea, tc), 3 lapserate_r(tc, ea, pk), exp and log through the tables in LDS. */
int mcf_selftest_step(int32_t kind, const double *in, int32_t nin, double *out, int32_t nout, int64_t n, int32_t device);

/* Diagnostics: the device physics of the snow kernels (mcf_snow_device.hpp), elementwise, one lane per element; planes as in
 * mcf_selftest_step.  Used by tests to hold each field against a high-precision evaluation of the reference's formulas.
 *   kind 0 (nin = 2: x, y; nout = 12), guards and scalars: 0 gexp(x), 1 glog(x), 2 gsqrt(x), 3 gpow0(x, y), 4 svp(x),
 *     5 dewpoint(x), 6 rad4(x), 7 latent_lt0(x), 8 clamp01(x), 9 snow_albedo((int)x) (0 <= x < 2^31, else of 0),
 *     10 snow_satvap_r(x), 11 snow_lapserate_r(x, ea, y) with ea = snow_satvap_r(x) * 80 / 100 as the coarse expansion forms it.
 *   kind 1 (nin = 8: pait, lref, ltra, gref, kd, kx, kcos, si; nout = 29), radiation: ts_dif(pait, lref, ltra, gref, 1 / gref):
 *     0 om, 1 a, 2 gma, 3 del, 4 h, 5 S1, 6 iS1, 7 iD1, 8 iD2, 9 u1, 10 u2, 11 D1, 12 D2, 13 p1, 14 p2, 15 p3, 16 p4;
 *     ts_dir(pait, that, gref, kd): 17 sig, 18 isig (both of the NEGATED determinant), 19 S2, 20 p5, 21 p6, 22 p7, 23 p8, 24 p9,
 *     25 p10; cank1(kx, kcos, si): 26 k, 27 kd, 28 Kc.
 *   kind 2 (nin = 32; nout = 23), canopy and profile.  In: 0 h, 1 pai, 2 d, 3 uf, 4 prec, 5 sint, 6 Li, 7 .. 10 sdp[0 .. 3],
 *     11 depth, 12 age (hours), 13 x, 14 z, 15 leafden, 16 Flux, 17 Fluxz, 18 SH, 19 SG, 20 mxnear, 21 zm, 22 zref, 23 za, 24 T0,
 *     25 tc, 26 ea, 27 slope, 28 aspect, 29 zend, 30 azid, 31 hc.  Out: 0 zeroplane(h, pai), 1 roughlen0(h, pai, d),
 *     2 canopy_snow_interception(hc, pai, uf, prec, sint, Li), 3 snow_density(sdp, depth, age), 4 / 5 sin / cos of
 *     sincos_0pi(x), 6 rh_canopy(uf, h, 1 / h, d, z), 7 rh_canopy(.., h), below_k(z, d, h, uf): 8 Kg, 9 Kh, 10 Kc, 11 iKc, 12 iKs,
 *     13 tv_below(that, glog(pai), leafden, Flux, Fluxz, SH, SG, mxnear), tv_above_l(za, d, zm, log((za - d) / zm) + log 5,
 *     log((zref - d) / zm) + log 5, T0, tc, ea): 14 Tz, 15 ez; site_derive(slope, aspect): 16 cS, 17 sS, 18 cA, 19 sA, 20 flat;
 *     solar_index of sun_derive(zend, zend torad, azid) at that site: 21 shadowmask = 0, 22 shadowmask = 1.
 *   kind 3 (nin = 5: tc, rh, pk, tci, mxtc; nout = 22), step weather.  met_derive(tc, rh, pk, tci): 0 ea, 1 te, 2 rem, 3 rcan,
 *     4 la, 5 cp, 6 Da, 7 gR, 8 De, 9 tdew, 10 ph, 11 sint; micro_met(tc, rh, pk, mxtc): 12 es, 13 ea, 14 tdew, 15 De, 16 gHrad,
 *     17 Rem, 18 la_pm, 19 lat0, 20 dTmx, 21 ipk. */
int mcf_selftest_snow(int32_t kind, const double *in, int32_t nin, double *out, int32_t nout, int64_t n, int32_t device);

/* Information. */
int64_t mcf_plan_valid_cells(const mcf_plan *plan); /* cells with non-NA hgt */
int64_t mcf_plan_bytes(const mcf_plan *plan);       /* device bytes held      */

#ifdef __cplusplus
}
#endif
#endif /* MCF_H */
