/*
 * stages_ref_array.c — TEST INFRASTRUCTURE: the yardstick of the staged model's diagnostics (include/mcf.h mcf_diag) for
 * array weather.
 *
 * tests/stages_ref.c for the array_forcing branch of the oracle's grid driver (oracle/mcf_oracle.c orc_run_grid): the
 * oracle's own static functions called in the driver's order with the driver's array-forcing choices — the sun's position
 * from the cell's own latitude and longitude, the solar index with the driver's shadowmask argument (0: cpp:2497-2504), the
 * forcing read at [cell, step], mxtc per cell (cpp:2467-2471), the wind-shelter index from the winddir vector — and the
 * intermediates the driver throws away written out: the thirteen diagnostics plus the five values that tie this file to the
 * unchanged oracle bit for bit (Rbdown, Rddown, Rdup, uz, soilm).  The oracle is read, not modified: it is included as it
 * stands, so a perturbed build of this file perturbs the same calls as the oracle's variant libraries.  Coarse weather comes
 * here already expanded to the raster (oracle/coarse_oracle.py), as it comes to the oracle.
 *
 * Build: tests/stages_ref_array.py, with the flags of oracle/Makefile.
 */
#include "../oracle/mcf_oracle.c"

enum { SR_RBDOWN = MCF_NDIAG, SR_RDDOWN, SR_RDUP, SR_UZ, SR_SOILM, SR_COUNT };

typedef struct stages_out {
    double *var[SR_COUNT];      /* [rows, cols, tsteps] each, or NULL */
} stages_out;

int stages_count(void) { return SR_COUNT; }

int stages_run_array(const mcf_grid_inputs *in, const mcf_options *opt, stages_out *out) {
    if (in->array_forcing != 1) return 1;
    const int64_t rows = in->rows, cols = in->cols, N = rows * cols;
    const int tsteps = (int)in->tsteps;
    const int ndays = tsteps / 24;
    const int layered = in->veg_layers > 1;
    const int nlyrs = layered ? in->veg_layers : 1;
    const double reqhgt = opt->reqhgt, zref = opt->zref;
    const double na = orc_na_real();
    double **O = out->var;
    for (int v = 0; v < SR_COUNT; ++v)
        if (O[v]) for (int64_t q = 0; q < N * (int64_t)tsteps; ++q) O[v][q] = na;
    int *windex = (int *)calloc((size_t)(tsteps > 0 ? tsteps : 1), sizeof(int));
    for (int k = 0; k < tsteps; ++k) windex[k] = dir_index(in->clim.winddir[k], 45.0, 8);
    double *tadd = (double *)calloc((size_t)(N > 0 ? N : 1), sizeof(double));
    orc_soild_tadd(in->soilc.twi, N, rows, cols, opt->tfact, tadd);
    const mcf_vegp *V = &in->vegp;
    const mcf_soilc *S = &in->soilc;
#define PUT(v, val) do { if (O[v]) O[v][idx] = (val); } while (0)
    for (int64_t i = 0; i < rows; ++i) {
        for (int64_t j = 0; j < cols; ++j) {
            const int64_t c = i + rows * j;
            if (isnan(V->hgt[c])) continue;
            const double gref = S->gref[c];
            soilp_t spa;
            spa.Smax = S->Smax[c]; spa.Smin = S->Smin[c]; spa.soilb = S->soilb[c]; spa.psi_e = S->Psie[c];
            spa.Vq = S->Vq[c]; spa.Vm = S->Vm[c]; spa.Mc = S->Mc[c]; spa.rho = S->rho[c];
            soilc_t sc = soilpfun(S->Vm[c], S->Vq[c], S->Mc[c], S->rho[c]);
            double mxtc = -273.15;      /* cpp:2467-2471 */
            for (int k = 0; k < tsteps; ++k)
                if (in->clim.tc[c + N * k] > mxtc) mxtc = in->clim.tc[c + N * k];
            for (int lyr = 0; lyr < nlyrs; ++lyr) {
                const int64_t cl = c + N * lyr;
                const double hgt = V->hgt[cl], pai = V->pai[cl], x = V->x[cl];
                tir_t tir = twostreamdif(pai, V->paia[cl], x, V->leafr[cl], V->leaft[cl], V->clump[cl], gref);
                tiw_t tiw = windti(hgt, pai);
                const int lst = layered ? in->lyr_st[lyr] : 0;
                const int lnd = layered ? (in->lyr_ed[lyr] - in->lyr_st[lyr] + 1) / 24 : ndays;
                for (int dy = 0; dy < lnd; ++dy) {
                    double Rmx = -999.9, tmx = -999.0, tmn = 999.0;
                    double surfwet[24], radabs[24], soilmday[24], gHa[24];
                    for (int hr = 0; hr < 24; ++hr) {
                        const int k = dy * 24 + hr + lst;
                        const int64_t idx = c + N * k;
                        const int64_t f = idx;      /* forcing index */
                        /* cpp:2497-2504 (shadowmask defaults to false) */
                        orc_solmodel solp = orc_solposition(in->lats[c], in->lons[c], in->obstime.year[k], in->obstime.month[k],
                                                            in->obstime.day[k], in->obstime.hour[k]);
                        double si = orc_solarindex(S->slope[c], S->aspect[c], solp.zend, solp.azid, 0);
                        const int sidx = dir_index(solp.azid, 15.0, 24);
                        if (si < 0.0) si = 0.0;
                        double ws = S->wsa[windex[k] * N + c];
                        double ha = S->hor[sidx * N + c];
                        double sa = (PI_ / 2.0) - solp.zenr;
                        if (ha > tan(sa)) si = 0.0;
                        PUT(MCF_DIAG_SI, si);
                        /* soilmdistribute */
                        double soild = orc_soild(in->pointm.soilm[f], S->Smin[c], S->Smax[c], tadd[c]);
                        soilmday[hr] = soild;
                        PUT(SR_SOILM, soild);
                        /* twostream */
                        orc_kstruct kpp = orc_cank(solp.zenr, x, si);
                        tsdir_t tsd = twostreamdir_params(tir.pait, tir.om, tir.a, tir.gma, tir.J, tir.del, tir.h, gref,
                                                          kpp.kd, tir.u1, tir.S1, tir.D1, tir.D2);
                        rad_t rm = twostream(pai, V->clump[cl], gref, S->svfa[c], si, in->clim.tc[f], in->clim.swdown[f],
                                             in->clim.difrad[f], in->clim.lwdown[f], solp, kpp, tsd, tir);
                        PUT(MCF_DIAG_RADGSW, rm.radGsw); PUT(MCF_DIAG_RADGLW, rm.radGlw);
                        PUT(MCF_DIAG_RADCSW, rm.radCsw); PUT(MCF_DIAG_RADCLW, rm.radClw);
                        PUT(MCF_DIAG_RADLSW, rm.radLsw); PUT(MCF_DIAG_RADLPAR, rm.radLpar);
                        PUT(MCF_DIAG_LWOUT, rm.lwout);
                        PUT(SR_RBDOWN, rm.Rbdown); PUT(SR_RDDOWN, rm.Rddown); PUT(SR_RDUP, rm.Rdup);
                        /* wind */
                        double reqhgt2 = reqhgt;
                        if (reqhgt2 < 0.00001) reqhgt2 = 0.00001;
                        wind_t wm = wind(reqhgt2, zref, hgt, pai, in->clim.windspeed[f], in->pointm.umu[f], ws, tiw);
                        gHa[hr] = wm.gHa;
                        PUT(MCF_DIAG_UF, wm.uf); PUT(MCF_DIAG_GHA, wm.gHa); PUT(SR_UZ, wm.uz);
                        /* soiltemp, first half: G = 0 */
                        soilG0_t g0 = soiltempG0(in->clim.tc[f], in->clim.es[f], in->clim.ea[f], in->clim.pk[f], rm.radGsw,
                                                 rm.radGlw, in->clim.tdew[f], wm.gHa, soild, mxtc, spa);
                        double Rval = fabs(g0.Rnet);
                        if (Rmx < Rval) Rmx = Rval;
                        if (tmx < g0.Tg) tmx = g0.Tg;
                        if (tmn > g0.Tg) tmn = g0.Tg;
                        surfwet[hr] = g0.surfwet;
                        radabs[hr] = g0.radabs;
                    }
                    double dtr = tmx - tmn;
                    for (int hr = 0; hr < 24; ++hr) {
                        const int k = dy * 24 + hr + lst;
                        const int64_t idx = c + N * k;
                        const int64_t f = idx;
                        soilhr_t gv = soiltemp_hr(in->clim.tc[f], in->clim.es[f], in->clim.ea[f], in->clim.pk[f], radabs[hr],
                                                  surfwet[hr], in->clim.tdew[f], gHa[hr], soilmday[hr], mxtc, in->pointm.G[f],
                                                  dtr, in->pointm.dtrp[f], in->pointm.muGp[f], in->pointm.kp[f], Rmx, sc, spa);
                        PUT(MCF_DIAG_T0, gv.Tg); PUT(MCF_DIAG_G, gv.G); PUT(MCF_DIAG_KDDG, gv.DD);
                    }
                }
            }
        }
    }
#undef PUT
    free(windex); free(tadd);
    return 0;
}
