// mcf_hydro.h — device-level entries of the flow accumulation / wetness index (mcf_hydro.hip) and of the two small steps a plan
// built from a dtm needs beside mcf::terrain_device.  Every pointer is device memory of the current device; all launches on the
// null stream; each returns after the device has finished, its temporaries released.
#pragma once
#include <stdint.h>

namespace mcf {
// flowaccCpp of [rows, cols] column-major elevations (NaN = NA): the values of mcf_flowacc
int flowacc_device(const double* d_dtm, int64_t rows, int64_t cols, double* d_fa);
// `.topidx`: the values of mcf_topidx up to the last bits of atan / tan.  d_fa: null, or where the flow accumulation goes too
int topidx_device(const double* d_dtm, int64_t rows, int64_t cols, double xres, double yres, double* d_twi, double* d_fa);
// NaN into a / b (each [rows, cols] or null) where the block's dtm [(halo_north + rows + halo_south), cols] is NA
int mask_na_device(const double* d_dtm, int64_t rows, int64_t cols, int32_t halo_north, int32_t halo_south, double* d_a, double* d_b);
// svfa = 0.5 cos(2 tan(mean(atan(hor)))) + 0.5 of a supplied hor[N, 24] (R/internal.R:1146-1149)
int svf_from_hor_device(const double* d_hor, int64_t N, double* d_svfa);
}  // namespace mcf
