// mcf_snow_plan.hpp — what mcf_snowrun.hip (the row-block drivers of the snow model and the snow run) calls in mcf_snow.hip
// besides the C entries of include/mcf.h: declared once, included by both.  Host only.
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/mcf.h"
#include "mcf_rowblocks.hpp"

namespace mcf {
int64_t snowplan_halo_rows(const mcf_snowplan* sp, int32_t af);
void snowplan_print_timing(const mcf_snowplan* sp);      // mcf_snowmodel1 / 2's MCF_TIMING line
// Coarse array weather.  What is refused of a mcf_snowcoarse_in / mcf_microcoarse_in before a device is touched, under the entry's
// name (model: the snow model runs behind; null_out: the name of the entry's output argument if that is null) ...
int snowcoarse_checks(const mcf_snowcoarse_in* in, bool model, const char* entry, const char* null_out);
int microcoarse_checks(const mcf_microcoarse_in* in, const char* entry);
// ... the plan whose chunks are expanded from the resident coarse arrays, the microclimate's coarse set onto it, and where its
// chunks hand pointm$umu to
int snowplan_create_coarse(const mcf_snowcoarse_in* co, double* umu_out, int32_t device, mcf_snowplan** out);
int snowplan_micro_attach_coarse(mcf_snowplan* sp, const mcf_microcoarse_in* mi);
void snowplan_coarse_umu_out(mcf_snowplan* sp, double* umu_out);
// (over the listings of the snow entries' array groups, kept in mcf_snow.hip next to the kernels' argument structs)
bool model_rasters_given(const mcf_snow_inputs& in);
void model_rasters_of_block(mcf_snowdriver_in& in, HostCopies* rows, int64_t R, int64_t C, int64_t r0, int64_t nr);
bool micro_rasters_given(const mcf_snow_inputs& in);
void micro_rasters_of_block(mcf_snow_inputs& in, HostCopies& rows, int64_t R, int64_t C, int64_t r0, int64_t nr);
const char* micro_series_missing(const mcf_snow_inputs& in);
void subset_days(mcf_snow_inputs& in, bool series, const int32_t* sub_of_day, int ndays, int nsub, HostCopies& keep);
// the summaries' specs judged without a device, and the selected series as a mcf_snowplan_set_series mask
int snowpack_spec_check(const mcf_snowpack_summary_spec* s, int64_t tsteps, int64_t chunk_steps);
uint32_t snowpack_series_bits(const mcf_snowpack_summary_spec* s);
// the series sink's spec judged without a device (`who`: the entry's name, at the start of every message), and a block's raw
// zone state of one series, [4][nzones][snowplan_series_steps] of int64, with its folded days [steps / 24] (either may be null)
int snowpack_series_check(const std::string& who, const mcf_snowpack_series_spec* s, int64_t rows, int64_t cols, int64_t chunk_steps);
int64_t snowplan_series_steps(const mcf_snowplan* sp);
int snowplan_series_state(mcf_snowplan* sp, int32_t series, int64_t* host_state, int32_t* day_done);
}  // namespace mcf
