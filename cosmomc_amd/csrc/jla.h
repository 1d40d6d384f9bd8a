// JLA supernova likelihood (source/supernovae_JLA.f90): what the loader reads
// from a jla.dataset and derives at load time (read_jla_dataset :602-760,
// jla_prep :874-957).  Host only; jla.hip uploads it.
#pragma once

#include "common.h"

namespace cmamd {

// the six component matrices of V(alpha, beta), in the order
// invert_covariance_matrix adds them (:813-824)
enum { JLA_MAG, JLA_STRETCH, JLA_COLOUR, JLA_MAG_STRETCH, JLA_MAG_COLOUR, JLA_STRETCH_COLOUR, JLA_NCOMP };

struct JlaData {
    std::string name;          // the dataset's own name key
    int nsn = 0;
    bool twoscriptmfit = false;
    bool diag_errors = true;   // no covariance matrix at all (:677-715)
    std::vector<double> zcmb, zhel, mag, stretch, colour, thirdvar;
    std::vector<double> stretch_var, colour_var;       // single-precision squares (:475-479)
    std::vector<double> cov_ms, cov_mc, cov_sc;        // per-SN covariances of the light-curve fit
    std::vector<double> pre_vars;                      // :912-921
    std::vector<double> one, A2;                       // A1 (twoscriptmfit) or ones, and A2 or zeros
    bool has[JLA_NCOMP] = {false, false, false, false, false, false};
    // [nsn][nsn], the file's upper triangle mirrored (uplo = 'U', :135)
    std::vector<double> comp[JLA_NCOMP];
};

// marginalised: the caller serves JLA_marginalize = T (jlamarge.hip); otherwise the key is refused
JlaData load_jla(const Ini &ini, bool marginalised = false);

}  // namespace cmamd
