// Galaxy power-spectrum likelihoods (source/mpk.f90, source/wigglez.f90): what
// the loaders read and derive at load time (MPK_ReadIni mpk.f90:117-244,
// TWiggleZCommon_ReadIni and WiggleZ_ReadIni wigglez.f90:203-437,
// GiggleZinfo_init :44-76).  Host only; mpk.hip uploads it.  Values the
// reference holds in single precision (Ag, Q_mid, Q_sigma read with Read_Real,
// the literal dQ = 0.4, the last GiggleZ coefficient of bins 3 and 4) are
// widened to double here as it widens them (mpk_f32).
#pragma once

#include "common.h"

namespace cmamd {

enum { MPK_Q_NONE = 0, MPK_Q_FLAT = 1, MPK_Q_GAUSS = 2, MPK_Q_POINT = 3 };   // cmbl_mpk_info's Q mode
constexpr int MPK_NQ = 6;             // the Q grid runs over iQ = -6 .. 6
constexpr int MPK_NV = 2 * MPK_NQ + 1;
constexpr int MPK_MAXR = 7;           // WiggleZ regions
constexpr int MPK_MAXP = 64;          // points used: four 16-row tiles a wave keeps in registers
constexpr int MPK_GIGGLEZ_NUMK = 500;

inline double mpk_f32(float x) { return (double)x; }

struct MpkData {
    std::string name;
    bool wigglez = false;
    int np = 0, nk = 0, nr = 1, zbin = 0, q_mode = MPK_Q_NONE;
    bool q_marge = false, has_cov = false, use_scaling = false, use_gigglez = false, nonlinear = false;
    double Q_mid = 0, Q_sigma = 0, Ag = mpk_f32(1.4f), DV_fid = 0, redshift = 0;
    std::vector<double> k;          // [nk]
    std::vector<double> P;          // [nr][np]
    std::vector<double> sdev;       // [np] ("MPK")
    std::vector<double> W;          // [nr][np][nk]
    std::vector<double> invcov;     // [nr][np][np]; without a cov_file diag(1 / sdev^2)
    std::vector<double> gk, gf, gdd;   // GiggleZ spline of the bin: knots k, ln P, second derivatives
};

MpkData load_mpk(const Ini &ini, bool wigglez);

// loader quantities for the tests (cmbl_mpk_info / cmbl_mpk_arrays)
bool mpk_info(const Like *like, int *dims);
bool mpk_arrays(const Like *like, double *k, double *data, double *invcov);

}  // namespace cmamd
