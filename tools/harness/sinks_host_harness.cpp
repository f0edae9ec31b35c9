// The sinks' host-only decisions (microclimf_amd/csrc/mcf_sinks_host.hpp) under AddressSanitizer + UBSan, no device and no library:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Imicroclimf_amd/csrc
//       -o /tmp/mcf_sinks_asan tools/harness/sinks_host_harness.cpp && /tmp/mcf_sinks_asan      (one command)
#include "mcf_sinks_host.hpp"

#include <cstdio>
#include <cstdlib>

static std::string g_msg;
namespace mcf { int api_fail(int code, const std::string& msg) { g_msg = msg; return code; } }

#define EXPECT(cond) do { if (!(cond)) { printf("line %d: %s (last message: %s)\n", __LINE__, #cond, g_msg.c_str()); exit(1); } } while (0)

int main() {
    using namespace mcf;
    // ---- places: soilm and Tz selected on a plan of four depths, every other variable on a plan without a list
    {
        int32_t var[MCF_NOUT] = {};
        var[MCF_OUT_TZ] = var[MCF_OUT_SOILM] = 1;
        SinkPlaces s;
        s.select(var, 3);
        EXPECT(s.nmain == 2 && s.nsel == 5);
        const int tz = s.sel1[MCF_OUT_TZ] - 1, sm = s.sel1[MCF_OUT_SOILM] - 1;
        EXPECT(tz >= 0 && sm >= 0 && tz != sm && tz < 2 && sm < 2);
        EXPECT(s.place("w", MCF_OUT_TZ, 0) == tz && s.place("w", MCF_OUT_SOILM, 0) == sm);
        for (int d = 1; d <= 3; ++d) EXPECT(s.place("w", MCF_OUT_TZ, d) == 1 + d);
        EXPECT(s.place("w", MCF_OUT_TZ, 4) == -1 && g_msg == "w: depth 4 is outside the plan's list");
        EXPECT(s.place("w", MCF_OUT_TZ, -1) == -1);
        EXPECT(s.place("w", MCF_OUT_SOILM, 1) == -1 && g_msg == "w: only Tz is kept per depth (depth 0 for soilm)");
        for (int v = 0; v < MCF_NOUT; ++v) var[v] = 1;
        s.select(var, 0);
        EXPECT(s.nmain == MCF_NOUT && s.nsel == MCF_NOUT);
        for (int v = 0; v < MCF_NOUT; ++v) EXPECT(s.place("w", v, 0) == v && s.place("w", v, 1) == -1);
    }
    // ---- fold ranges against a plan of 9 days whose two slots hold 4
    EXPECT(check_fold_range("", 2, 4, 9, 1, 0, 5, 4) == MCF_OK);
    EXPECT(check_fold_range("", 2, 4, 9, 2, 0, 0, 1) == MCF_ERR_ARG && g_msg == "slot out of range");
    EXPECT(check_fold_range("e", 2, 4, 9, -1, 0, 0, 1) == MCF_ERR_ARG && g_msg == "e: slot out of range");
    EXPECT(check_fold_range("e", 2, 4, 9, 0, 0, 8, 2) == MCF_ERR_ARG && g_msg == "e: day range out of bounds");
    EXPECT(check_fold_range("e", 2, 4, 9, 0, 0, 0, 0) == MCF_ERR_ARG);
    EXPECT(check_fold_range("e", 2, 4, 9, 0, 0, 2147483647, 2147483647) == MCF_ERR_ARG);
    EXPECT(check_fold_range("e", 2, 4, 9, 0, 1, 0, 4) == MCF_ERR_ARG && g_msg == "e: more days than the ring slot holds");
    EXPECT(check_fold_range("e", 2, 4, 9, 0, 2147483647, 0, 2) == MCF_ERR_ARG);
    // ---- period tables: every day's neighbours of its period, an empty plan, a table entry out of range at either end
    {
        const int32_t pod_in[9] = {0, 0, 1, 1, 2, 2, 0, -1, 1};
        std::vector<int32_t> pod, prev, next;
        EXPECT(period_tables(pod_in, 9, 3, pod, prev, next) == MCF_OK && pod.size() == 9 && prev.size() == 9 && next.size() == 9);
        const int32_t want_prev[9] = {-1, 0, -1, 2, -1, 4, 1, -1, 3}, want_next[9] = {1, 6, 3, 8, 5, 9, 9, 9, 9};
        for (int d = 0; d < 9; ++d) EXPECT(pod[d] == pod_in[d] && prev[d] == want_prev[d] && next[d] == want_next[d]);
        EXPECT(period_tables(nullptr, 0, 1, pod, prev, next) == MCF_OK && pod.size() == 1 && pod[0] == -1 && next[0] == 0);
        const int32_t high[2] = {0, 3}, low[2] = {-2, 0};
        EXPECT(period_tables(high, 2, 3, pod, prev, next) == MCF_ERR_ARG);
        EXPECT(period_tables(low, 2, 3, pod, prev, next) == MCF_ERR_ARG && g_msg == "summary: a table entry is outside -1 .. nperiods - 1");
    }
    // ---- below ground, and the null buffers of every output struct: the first missing one is named, a full set passes
    {
        int32_t var[MCF_NOUT] = {};
        var[MCF_OUT_TZ] = var[MCF_OUT_SOILM] = 1;
        EXPECT(check_below_vars("e", var, "have a series") == MCF_OK);
        for (int v = MCF_NOUT - 1; v >= 0; --v)
            if (v != MCF_OUT_TZ && v != MCF_OUT_SOILM) { var[v] = 1; break; }
        EXPECT(check_below_vars("e", var, "have a series") == MCF_ERR_ARG && g_msg == "e: below ground Tz and soilm have a series, nothing else");
        double buf = 0;
        mcf_summary_spec ss{};
        mcf_summary_out so{};
        ss.var[MCF_OUT_TZ] = 1; ss.stat[MCF_STAT_MEAN] = ss.stat[MCF_STAT_MAX] = 1;
        so.val[MCF_OUT_TZ][MCF_STAT_MEAN] = &buf;
        EXPECT(check_summary_out(&ss, &so) == MCF_ERR_ARG);
        so.val[MCF_OUT_TZ][MCF_STAT_MAX] = &buf;
        EXPECT(check_summary_out(&ss, &so) == MCF_OK);
        mcf_depth_summary_out dso{};
        ss.var[MCF_OUT_SOILM] = 1;
        for (int d = 0; d < 2; ++d) dso.tz[d][MCF_STAT_MEAN] = dso.tz[d][MCF_STAT_MAX] = &buf;
        dso.soilm[MCF_STAT_MEAN] = &buf;
        EXPECT(check_depth_summary_out("e", &ss, 3, &dso) == MCF_ERR_ARG && g_msg == "e: a selected (depth, statistic) has a null buffer");
        EXPECT(check_depth_summary_out("e", &ss, 2, &dso) == MCF_ERR_ARG && g_msg == "e: a selected statistic of soilm has a null buffer");
        dso.soilm[MCF_STAT_MAX] = &buf;
        EXPECT(check_depth_summary_out("e", &ss, 2, &dso) == MCF_OK);
        mcf_snowpack_summary_spec ps{};
        mcf_snowpack_summary_out pso{};
        ps.series[4] = 1; ps.stat[MCF_NSTAT - 1] = 1;
        EXPECT(check_snowpack_summary_out(&ps, &pso) == MCF_ERR_ARG);
        pso.val[4][MCF_NSTAT - 1] = &buf;
        EXPECT(check_snowpack_summary_out(&ps, &pso) == MCF_OK);
        mcf_series_spec zs{};
        mcf_series_out zo{};
        zs.var[MCF_OUT_TZ] = zs.var[MCF_OUT_SOILM] = 1; zs.npoints = 2; zs.nzones = 3; zs.zstat[MCF_NZSTAT - 1] = 1;
        EXPECT(check_series_out("e", &zs, &zo) == MCF_ERR_ARG && g_msg == "e: a selected variable has a null point buffer");
        zo.points[MCF_OUT_TZ] = zo.points[MCF_OUT_SOILM] = &buf;
        zo.zones[MCF_OUT_TZ][MCF_NZSTAT - 1] = &buf;
        EXPECT(check_series_out("e", &zs, &zo) == MCF_ERR_ARG && g_msg == "e: a selected (variable, statistic) has a null buffer");
        zo.zones[MCF_OUT_SOILM][MCF_NZSTAT - 1] = &buf;
        EXPECT(check_series_out("e", &zs, &zo) == MCF_OK);
        mcf_depth_series_out dzo{};
        dzo.tz_points[0] = &buf; dzo.tz_zones[0][MCF_NZSTAT - 1] = &buf;
        EXPECT(check_depth_series_out("e", &zs, 2, &dzo) == MCF_ERR_ARG && g_msg == "e: a depth has a null point buffer");
        EXPECT(check_depth_series_out("e", &zs, 1, &dzo) == MCF_ERR_ARG && g_msg == "e: soilm has a null point buffer");
        dzo.soilm_points = &buf;
        EXPECT(check_depth_series_out("e", &zs, 1, &dzo) == MCF_ERR_ARG && g_msg == "e: a selected statistic of soilm has a null buffer");
        dzo.soilm_zones[MCF_NZSTAT - 1] = &buf;
        EXPECT(check_depth_series_out("e", &zs, 1, &dzo) == MCF_OK);
        zs.npoints = 0; zs.nzones = 0;
        mcf_depth_series_out none{};
        EXPECT(check_depth_series_out("e", &zs, MCF_MAX_DEPTHS, &none) == MCF_OK);
        mcf_snowpack_series_spec pz{};
        mcf_snowpack_series_out pzo{};
        pz.series[0] = 1; pz.npoints = 1;
        EXPECT(check_snowpack_series_out("e", &pz, &pzo) == MCF_ERR_ARG && g_msg == "e: a selected series has a null point buffer");
        pzo.points[0] = &buf;
        EXPECT(check_snowpack_series_out("e", &pz, &pzo) == MCF_OK);
    }
    printf("sinks' host decisions through ASan + UBSan: clean\n");
    return 0;
}
