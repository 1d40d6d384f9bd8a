// Polynomial theory calculator (cmbt_*): a response surface of D_l in the slow
// parameters, evaluated on the device straight into a theory buffer.  It takes
// the place of the reference's calculator object in its emulator form
// (Calculator_PICO.f90: a polynomial fit of the C_l; a point outside the
// training box gives error = 1, which TheoryLike_GetLogLikeMain turns into
// logZero, calclike.f90:308-313).  Its derived outputs are the
// parameterization's derived parameters and, with ranges, the hard cuts of
// TP_NonBaseParameterPriors (CosmologyParameterizations.f90:90-112, 189-272).
// A Gaussian likelihood on such surfaces (cmbg_*) is its Gaussian priors
// (:105-110) and the Gaussian BAO likelihood (bao.f90:265-308).
#pragma once

#include <string>
#include <vector>

#include "common.h"

namespace cmamd {
// theory_calc_kernel's tile: TC_TW walkers x TC_TN consecutive l of one field
// per workgroup, the coefficient table staged through LDS TC_KC terms at a time
constexpr int TC_TW = 32, TC_TN = 256, TC_KC = 8, TC_THREADS = 256;
constexpr int TC_MAXIN = 16, TC_MAXTERMS = 256, TC_MAXORDER = 4;
// theory_derived_kernel's tile: a point per thread, all its (up to TD_ND)
// scalar outputs in the thread's registers
constexpr int TD_TM = 256, TD_ND = CMBT_MAXDERIVED, TD_THREADS = 256;
}  // namespace cmamd

struct cmbt {
    int n_in = 0, K = 0, Kp = 0, n_fields = 0, lmax = 0, Lp = 0;
    std::vector<int> pidx;        // 1-based indices into P
    std::string last_error;
    // device tables: meta [4][TC_MAXIN] (lo, hi, center, scale), pidx [n_in],
    // fields [n_fields], expo [Kp] (4 bits per input), coef [n_fields][Kp][Lp]
    // (terms padded to TC_KC and l to TC_TN with zeros)
    cmamd::DevBuf meta, pidx_d, fields_d, expo, coef;
    // derived outputs (cmbt_set_derived; n_derived == 0: none): dcoef
    // [Kp][TD_ND] (terms and outputs padded with zeros), dlim [2][TD_ND] (lo
    // then hi, -inf / +inf where there is no limit); ranged: a lo or hi table
    // was given, so the failure flags include the range test
    int n_derived = 0;
    bool ranged = false;
    cmamd::DevBuf dcoef, dlim;
};

// Likelihood on derived quantities (cmbg_*): n scalar surfaces over the
// calculator's monomials with coefficient columns of its own.  form 0: the
// Gaussian (cmbg_create); CMBG_TABLE_1D / CMBG_TABLE_2D: a tabulated
// likelihood on 1 / 2 surfaces (cmbg_create_table)
struct cmbg {
    cmbt *calc = nullptr;         // not owned
    int n = 0, form = 0;
    std::string last_error;
    // device tables: dcoef [Kp][TD_ND] as cmbt's, obs [TD_ND] (padded with
    // zeros), invcov [n][n]
    cmamd::DevBuf dcoef, obs, invcov;
    // tabulated forms.  1-D: table [tn] and p = scale, x_min, x_max, step.
    // 2-D: table = perp [tn], plel [tn], prob [tn][tn] (perp outer) and p =
    // DA_rd_fid, Hrd_fid, d_perp, d_plel, perp[0], perp[tn - 2], plel[0],
    // plel[tn - 2]
    int tn = 0;
    double p[8] = {};
    cmamd::DevBuf table;
};

namespace cmamd {
void theorygauss_create(cmbg *g, cmbt *calc, const cmbg_config_t *cfg);
void theorytable_create(cmbg *g, cmbt *calc, const cmbg_table_config_t *cfg);
void theorygauss_eval(cmbg *g, int M, const double *P, long long ld, int num_params, double *out, int *fail_flags,
                      hipStream_t stream);
void theorycalc_create(cmbt *t, const cmbt_config_t *cfg);
void theorycalc_eval(cmbt *t, int W, const double *P, long long ld, int num_params, double *dl, long long ld_field,
                     long long ld_walker, int *fail_flags, hipStream_t stream);
void theorycalc_range_flags(cmbt *t, int W, const double *P, long long ld, int *fail_flags, hipStream_t stream);
void theorycalc_set_derived(cmbt *t, const cmbt_derived_config_t *cfg);
void theorycalc_derived_eval(cmbt *t, int M, const double *P, long long ld, int num_params, double *out,
                             long long ld_out, int *fail_flags, hipStream_t stream);
}  // namespace cmamd
