// mcf_ncsink.hpp — the handle behind mcf_ncfile (include/mcf.h "writetonc sink", "netCDF sink: further sources"), for the units
// that write records into it: mcf_api.hip (the solver's ring slots) and mcf_snow.hip (the snow plan's chunk series).  Host only.
#pragma once

#include <stdint.h>

#include <memory>

#include "../../include/mcf.h"
#include "mcf_ncfile.hpp"

struct mcf_ncfile {
    std::unique_ptr<mcf::NcFile> f;
    bool snowpack = false;       // mcf_nc_create_snowpack: the variables are the snowpack's five series, not solver outputs
    int var_of[MCF_NOUT];        // file variable index of solver output (or series) v, or -1
    int out_of[MCF_NOUT];        // solver output (or series) of file variable k
    double scale[MCF_NOUT];      // per file variable
    int fill_only[MCF_NOUT];
    // staging of whole-raster records on their way to the file; plain arrays, not vectors: no zero-fill of memory about to be
    // overwritten.  One writer at a time: a row block's strips are staged in the writing call's own buffers.
    std::unique_ptr<uint8_t[]> stage[2];
    size_t stage_bytes[2] = {0, 0};
    uint8_t* staging(int i, size_t n) {
        if (stage_bytes[i] < n) { stage[i].reset(new uint8_t[n]); stage_bytes[i] = n; }
        return stage[i].get();
    }
};

namespace mcf {

// a file on its way through a one-call entry: closed on every path; close_file(h): the close's own status for the path that succeeds
struct NcCloser { void operator()(mcf_ncfile* nc) const { mcf_nc_close(nc); } };
using NcHolder = std::unique_ptr<mcf_ncfile, NcCloser>;
inline int close_file(NcHolder& h) { return mcf_nc_close(h.release()); }

// What a file's spec has to say for a run of rows x cols cells x tsteps steps, judged without a device (mcf_api.hip); w: the
// entry's name and a colon in front of the message; several_blocks: the run is cut into row blocks, which netcdf4 does not take.
// nc_spec_check: reqhgt the run's; out (may be null): the run's variables, which the file's must be among.
int nc_spec_check(const std::string& w, const mcf_nc_spec* spec, int64_t rows, int64_t cols, int64_t tsteps, double reqhgt,
                  const int32_t* out, bool several_blocks);
int ncpack_spec_check(const std::string& w, const mcf_ncpack_spec* spec, int64_t rows, int64_t cols, int64_t tsteps, bool several_blocks);

// rows [row0, row0 + nrows) of steps [step0, step0 + nsteps) of every variable as missval; "" or the reason
inline std::string nc_write_missing(NcFile* f, int64_t row0, int64_t nrows, int64_t step0, int64_t nsteps) {
    if (nsteps <= 0) return "";
    if (row0 < 0 || nrows < 1 || row0 + nrows > f->rows) return "row strip outside the file's grid";
    const int64_t srec = 8 + (int64_t)f->nvars * nrows * f->cols * 4;
    const int64_t piece = std::max<int64_t>(1, std::min(nsteps, ((int64_t)64 << 20) / srec));
    std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)(piece * srec)]);
    for (int64_t s = 0; s < piece; ++s) {
        memset(buf.get() + s * srec, 0, 8);
        for (int64_t i = 0; i < (srec - 8) / 4; ++i) NcFile::store_i32(buf.get() + s * srec + 8 + 4 * i, NcFile::kMissval);
    }
    for (int64_t s0 = 0; s0 < nsteps; s0 += piece) {
        const std::string e = f->write_strip(step0 + s0, std::min(piece, nsteps - s0), row0, nrows, buf.get());
        if (!e.empty()) return e;
    }
    return "";
}

}  // namespace mcf
