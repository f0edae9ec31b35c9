// mcf_sinks_host.hpp — what the sinks of a plan (period summaries, the series sink) decide without a
// device: the place of a (variable, depth) in a sink's state, the range of a fold, the day tables of the periods, and the
// null-buffer checks of the one-call entries' output structs.  Host only; a refusal goes through mcf::api_fail.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mcf.h"

namespace mcf {

int api_fail(int code, const std::string& msg);   // mcf_api.hip: sets the calling thread's mcf_last_error()

// The places of a sink's state: the first nmain are the ring's selected variables, the places behind them Tz at depths
// 1 .. D - 1 of a below-ground plan (the `_enable_below` entries; nmain = nsel everywhere else).
struct SinkPlaces {
    int sel1[MCF_NOUT] = {};    // 1 + place among the selected variables, 0: not selected
    int nmain = 0, nsel = 0;
    bool below = false;
    void select(const int32_t* var, int extra) {
        nmain = 0;
        for (int v = 0; v < MCF_NOUT; ++v) sel1[v] = var[v] ? ++nmain : 0;
        nsel = nmain + extra;
    }
    // the place of a selected variable at `depth`: its own, or that of Tz at a depth behind the first; -1 with the error set
    int place(const std::string& who, int32_t var, int32_t depth) const {
        if (depth < 0 || depth > (var == MCF_OUT_TZ ? nsel - nmain : 0))
            return api_fail(MCF_ERR_ARG, var == MCF_OUT_TZ ? who + ": depth " + std::to_string(depth) + " is outside the plan's list"
                                                           : who + ": only Tz is kept per depth (depth 0 for soilm)"), -1;
        return depth == 0 ? sel1[var] - 1 : nmain + depth - 1;
    }
};

// days [day0, day0 + ndays) of a plan of plan_days days, lying in ring slot `slot` from its day slot_day0 on; who: the entry's
// name in front of the message, or empty
inline int check_fold_range(const std::string& who, int ring_slots, int ring_days, int plan_days, int32_t slot, int32_t slot_day0,
                            int32_t day0, int32_t ndays) {
    const std::string w = who.empty() ? who : who + ": ";
    if (slot < 0 || slot >= ring_slots) return api_fail(MCF_ERR_ARG, w + "slot out of range");
    if (day0 < 0 || ndays < 1 || (int64_t)day0 + ndays > plan_days) return api_fail(MCF_ERR_ARG, w + "day range out of bounds");
    if (slot_day0 < 0 || (int64_t)slot_day0 + ndays > ring_days) return api_fail(MCF_ERR_ARG, w + "more days than the ring slot holds");
    return MCF_OK;
}

// each day's period, and the previous / next day of the same period (-1 / ndays: none); the tables are at least one entry long
inline int period_tables(const int32_t* period_of_day, int ndays, int nperiods, std::vector<int32_t>& pod, std::vector<int32_t>& prev,
                         std::vector<int32_t>& next) {
    const size_t nd = (size_t)(ndays > 1 ? ndays : 1);
    pod.assign(nd, -1); prev.assign(nd, -1); next.assign(nd, (int32_t)ndays);
    std::vector<int32_t> last((size_t)nperiods, -1);
    for (int d = 0; d < ndays; ++d) {
        const int per = pod[(size_t)d] = period_of_day[d];
        if (per < -1 || per >= nperiods) return api_fail(MCF_ERR_ARG, "summary: a table entry is outside -1 .. nperiods - 1");
        if (per < 0) continue;
        prev[(size_t)d] = last[(size_t)per];
        if (last[(size_t)per] >= 0) next[(size_t)last[(size_t)per]] = d;
        last[(size_t)per] = d;
    }
    return MCF_OK;
}

// below ground only Tz and soilm exist (what .runmodel1Cpp keeps there); phrase: what the sink would have done with another
inline int check_below_vars(const std::string& who, const int32_t* var, const char* phrase) {
    for (int v = 0; v < MCF_NOUT; ++v)
        if (var[v] && v != MCF_OUT_TZ && v != MCF_OUT_SOILM) return api_fail(MCF_ERR_ARG, who + ": below ground Tz and soilm " + phrase + ", nothing else");
    return MCF_OK;
}

// ---- a selected result with a null buffer, per output struct -----------------------------------------------------------------
inline int check_summary_out(const mcf_summary_spec* s, const mcf_summary_out* o) {
    for (int v = 0; v < MCF_NOUT; ++v)
        for (int k = 0; k < MCF_NSTAT; ++k)
            if (s->var[v] && s->stat[k] && !o->val[v][k]) return api_fail(MCF_ERR_ARG, "summary: a selected (variable, statistic) has a null buffer");
    return MCF_OK;
}
inline int check_snowpack_summary_out(const mcf_snowpack_summary_spec* s, const mcf_snowpack_summary_out* o) {
    for (int v = 0; v < 5; ++v)
        for (int k = 0; k < MCF_NSTAT; ++k)
            if (s->series[v] && s->stat[k] && !o->val[v][k])
                return api_fail(MCF_ERR_ARG, "snowpack summary: a selected (series, statistic) has a null buffer");
    return MCF_OK;
}
// the points' and the zones' buffers of one selected variable / series (`what`), shared by the three series structs
inline int check_series_buffers(const std::string& who, int64_t npoints, int32_t nzones, const int32_t* zstat, const double* points,
                                double* const* zones, const char* no_points, const char* no_zones) {
    if (npoints > 0 && !points) return api_fail(MCF_ERR_ARG, who + ": " + no_points);
    for (int k = 0; k < MCF_NZSTAT; ++k)
        if (nzones > 0 && zstat[k] && !zones[k]) return api_fail(MCF_ERR_ARG, who + ": " + no_zones);
    return MCF_OK;
}
inline int check_series_out(const std::string& who, const mcf_series_spec* s, const mcf_series_out* o) {
    for (int v = 0; v < MCF_NOUT; ++v)
        if (s->var[v])
            if (const int rc = check_series_buffers(who, s->npoints, s->nzones, s->zstat, o->points[v], o->zones[v],
                                                    "a selected variable has a null point buffer", "a selected (variable, statistic) has a null buffer"))
                return rc;
    return MCF_OK;
}
inline int check_snowpack_series_out(const std::string& who, const mcf_snowpack_series_spec* s, const mcf_snowpack_series_out* o) {
    for (int v = 0; v < 5; ++v)
        if (s->series[v])
            if (const int rc = check_series_buffers(who, s->npoints, s->nzones, s->zstat, o->points[v], o->zones[v],
                                                    "a selected series has a null point buffer", "a selected (series, statistic) has a null buffer"))
                return rc;
    return MCF_OK;
}
inline int check_depth_summary_out(const std::string& who, const mcf_summary_spec* s, int32_t D, const mcf_depth_summary_out* o) {
    for (int k = 0; k < MCF_NSTAT; ++k) {
        if (!s->stat[k]) continue;
        for (int d = 0; s->var[MCF_OUT_TZ] && d < D; ++d)
            if (!o->tz[d][k]) return api_fail(MCF_ERR_ARG, who + ": a selected (depth, statistic) has a null buffer");
        if (s->var[MCF_OUT_SOILM] && !o->soilm[k]) return api_fail(MCF_ERR_ARG, who + ": a selected statistic of soilm has a null buffer");
    }
    return MCF_OK;
}
inline int check_depth_series_out(const std::string& who, const mcf_series_spec* s, int32_t D, const mcf_depth_series_out* o) {
    for (int d = 0; s->var[MCF_OUT_TZ] && d < D; ++d)
        if (const int rc = check_series_buffers(who, s->npoints, s->nzones, s->zstat, o->tz_points[d], o->tz_zones[d],
                                                "a depth has a null point buffer", "a selected (depth, statistic) has a null buffer"))
            return rc;
    if (!s->var[MCF_OUT_SOILM]) return MCF_OK;
    return check_series_buffers(who, s->npoints, s->nzones, s->zstat, o->soilm_points, o->soilm_zones, "soilm has a null point buffer",
                                "a selected statistic of soilm has a null buffer");
}

}  // namespace mcf
