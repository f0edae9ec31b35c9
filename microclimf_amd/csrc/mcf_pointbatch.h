// mcf_pointbatch.h — what the batched point model's two halves share: the per-point and per-step constant tables that
// mcf_pointmodel.cpp fills on the host (with the host point model's own functions and evaluation order, so that the
// constants carry the very bits mcf_bigleaf computes) and that the kernels of mcf_pointbatch.hip read.
#pragma once
#include <stdint.h>

namespace mcf {

// per point, [BC_COUNT] doubles: everything of BigLeafCpp / RadswabsCpp / GFluxCpp that depends on vegp, groundp, lat, lon
// and zref only (cpp:187-278, 641-707, 710-770)
enum BlConst : int {
    BC_PAI = 0, BC_X, BC_CLUMP, BC_LREF, BC_EM, BC_GSMAX, BC_GREF, BC_GROUNDEM, BC_SMAX, BC_SMIN, BC_SOILB, BC_PSIE,
    BC_LON, BC_SINLAT, BC_COSLAT,                 // sun_position
    BC_SLOPE, BC_COSSL, BC_SINSL, BC_ASPECT,      // solar_index
    // RadswabsCpp: two-stream diffuse coefficients and what follows from them alone
    BC_PAITSW, BC_A, BC_GMA, BC_OM, BC_J, BC_DEL, BC_U1, BC_HH, BC_D1, BC_D2, BC_S1, BC_EMH, BC_EPH, BC_TRDSW, BC_AMX,
    BC_ALBD, BC_GRDD,
    // BigLeafCpp
    BC_TRD, BC_D, BC_HMD, BC_HDE, BC_BELIM, BC_ZREFD, BC_LEAFDD, BC_OMC, BC_SHADEC,
    BC_RSMX, BC_PSIW0, BC_KK, BC_RAT, BC_MUDEN,   // stomata
    // GFluxCpp
    BC_C1, BC_C3, BC_C4, BC_MU1, BC_MU2, BC_RHO,
    BC_COUNT
};
// per step, [n][TC_COUNT] doubles: the part of sun_position that depends on the date only
enum BlTime : int { TC_HOUR = 0, TC_EOT, TC_SINDEC, TC_COSDEC, TC_COUNT };
// per point of mcf_pointmprocess_batch
enum PmpConst : int { PC_LOGZ = 0, PC_C1, PC_C3, PC_C4, PC_RHO, PC_COUNT };
// per point of mcf_pointmodelsnow_batch, [PS_COUNT] doubles: what pointmodelsnow derives from vegp, other and snowenv alone
// (cpp:4000-4169): the site for the sun, the canopy without snow, the pack's start, snowdenp's row, the density of the whole
// run (the reference never updates it) and GFluxCppsnow's 6-hour mean of the constant Gmu that follows from it
enum PsConst : int {
    PS_SINLAT = 0, PS_COSLAT, PS_LON, PS_SLOPE, PS_COSSL, PS_SINSL, PS_ASPECT,
    PS_PAI, PS_HGT, PS_LTRA, PS_CLUMP, PS_ZREF, PS_ISNOWD, PS_ISNOWA,
    PS_DENA, PS_DENB, PS_DENC, PS_DEND, PS_SDEN0, PS_GMUD,
    PS_COUNT
};

void bl_point_consts(const double* vegp, const double* groundp, double lat, double lon, double zref, double* out);
void bl_time_consts(int64_t n, const int32_t* year, const int32_t* month, const int32_t* day, const double* hour, double* out);
void pmp_point_consts(double zref, double h, double pai, double rho, double Vm, double Vq, double Mc, double* out);
void ps_point_consts(const double* vegp, const double* other, int32_t snowenv, double* out);
void ps_albedo(const double* prec, int64_t n, double* alb);   // snowalbCpp: a serial hour counter, host work
double wh_zeroplane();   // zeroplane(0.12, 1) of weatherhgtCpp's fixed canopy
double wh_hde();         // ... and its (h - d) exp(-ka / Be)

}  // namespace mcf
