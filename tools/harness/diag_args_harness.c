/* diag_args_harness.c — stand-alone host program for tools/diag_sanitizers.sh: the argument checks and refusals of the staged
 * diagnostics' entry points (include/mcf.h mcf_plan_diag_*, mcf_runmicro1_diag, mcf_runmicro3_diag), linked against a build of
 * the library whose HOST code carries AddressSanitizer and UndefinedBehaviorSanitizer.  Runs on a machine without a device:
 * every call must return before one is needed, or report MCF_ERR_NO_DEVICE. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mcf.h"

static int fails = 0;
#define EXPECT(call, code)                                                                         \
    do {                                                                                           \
        const int rc_ = (call);                                                                    \
        if (rc_ != (code)) { printf("FAIL %s -> %d (%s), expected %d\n", #call, rc_, mcf_last_error(), (code)); ++fails; } \
        else printf("ok   %-70.70s -> %d %s\n", #call, rc_, rc_ ? mcf_last_error() : "");          \
    } while (0)

enum { R = 3, Cc = 4, T = 48, N = R * Cc };

int main(void) {
    int32_t sel[MCF_NDIAG], none[MCF_NDIAG];
    for (int v = 0; v < MCF_NDIAG; ++v) { sel[v] = 1; none[v] = 0; }
    void *q = NULL;
    mcf_ring_layout lay;
    double buf[8];
    /* plan entries: a null plan / null argument */
    EXPECT(mcf_plan_diag_enable(NULL, sel), MCF_ERR_ARG);
    EXPECT(mcf_plan_diag_fetch(NULL, 0, 0, 0, 1, buf), MCF_ERR_ARG);
    EXPECT(mcf_plan_diag_slot_ptr(NULL, 0, 0, &q), MCF_ERR_ARG);
    EXPECT(mcf_plan_diag_ring_layout(NULL, &lay), MCF_ERR_ARG);
    /* one-shot entries on a small, fully populated problem */
    static int32_t year[T], month[T], day[T];
    static double hour[T], series[15][T], plane[N], cube[24 * N], zero[T];
    for (int k = 0; k < T; ++k) { year[k] = 2023; month[k] = 6; day[k] = 1 + k / 24; hour[k] = k % 24; }
    for (int f = 0; f < 15; ++f) for (int k = 0; k < T; ++k) series[f][k] = 1.0 + f;
    for (int c = 0; c < N; ++c) plane[c] = 0.5;
    for (int c = 0; c < 24 * N; ++c) cube[c] = 0.1;
    mcf_grid_inputs in;
    memset(&in, 0, sizeof in);
    in.rows = R; in.cols = Cc; in.tsteps = T;
    in.obstime.year = year; in.obstime.month = month; in.obstime.day = day; in.obstime.hour = hour;
    {   /* every pointer member of the three input groups: a valid series / plane */
        const double **p = (const double **)&in.clim;
        for (size_t i = 0; i < sizeof in.clim / sizeof(double *); ++i) p[i] = series[i % 15];
        p = (const double **)&in.pointm;
        for (size_t i = 0; i < sizeof in.pointm / sizeof(double *); ++i) p[i] = zero;
        p = (const double **)&in.vegp;
        for (size_t i = 0; i < sizeof in.vegp / sizeof(double *); ++i) p[i] = plane;
        p = (const double **)&in.soilc;
        for (size_t i = 0; i < sizeof in.soilc / sizeof(double *); ++i) p[i] = cube;
    }
    in.lat = 50.0; in.lon = -5.0;
    mcf_options opt;
    memset(&opt, 0, sizeof opt);
    opt.reqhgt = 0.05; opt.zref = 2.0; opt.tfact = 1.5; opt.complete = 1; opt.mat = 10.0;
    mcf_outputs out;
    mcf_diag_outputs dout;
    memset(&out, 0, sizeof out);
    memset(&dout, 0, sizeof dout);
    static double ovar[N * T], dvar[MCF_NDIAG][N * T];
    opt.out[MCF_OUT_TZ] = 1; out.var[MCF_OUT_TZ] = ovar;
    EXPECT(mcf_runmicro1_diag(&in, &opt, NULL, &out, &dout), MCF_ERR_ARG);
    EXPECT(mcf_runmicro1_diag(&in, &opt, sel, &out, NULL), MCF_ERR_ARG);
    EXPECT(mcf_runmicro1_diag(NULL, &opt, sel, &out, &dout), MCF_ERR_ARG);
    EXPECT(mcf_runmicro1_diag(&in, NULL, sel, &out, &dout), MCF_ERR_ARG);
    EXPECT(mcf_runmicro1_diag(&in, &opt, sel, NULL, &dout), MCF_ERR_ARG);
    EXPECT(mcf_runmicro1_diag(&in, &opt, sel, &out, &dout), MCF_ERR_ARG);      /* selected diagnostics without buffers */
    for (int v = 0; v < MCF_NDIAG; ++v) dout.var[v] = dvar[v];
    EXPECT(mcf_runmicro1_diag(&in, &opt, none, &out, &dout), MCF_ERR_ARG);     /* empty selection */
    opt.reqhgt = -0.05;
    EXPECT(mcf_runmicro1_diag(&in, &opt, sel, &out, &dout), MCF_ERR_ARG);      /* below ground */
    opt.reqhgt = 0.05;
    in.array_forcing = 1; in.lats = plane; in.lons = plane;
    EXPECT(mcf_runmicro1_diag(&in, &opt, sel, &out, &dout), MCF_ERR_ARG);      /* array forcing */
    in.array_forcing = 0;
    EXPECT(mcf_runmicro3_diag(&in, &opt, sel, &out, &dout), MCF_ERR_ARG);      /* no vegetation layers */
    opt.cells_per_block = 17;
    EXPECT(mcf_runmicro1_diag(&in, &opt, sel, &out, &dout), MCF_ERR_ARG);
    opt.cells_per_block = 0;
    /* all arguments good: the first thing needed is a device */
    const int want = mcf_device_count() > 0 ? MCF_OK : MCF_ERR_NO_DEVICE;
    EXPECT(mcf_runmicro1_diag(&in, &opt, sel, &out, &dout), want);
    printf(fails ? "%d FAILED\n" : "all argument checks hold\n", fails);
    return fails ? 1 : 0;
}
