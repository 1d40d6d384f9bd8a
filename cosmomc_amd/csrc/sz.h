// Planck SZ cluster-counts likelihood (source/szcounts.f90, the 2D form): what
// the loader reads and derives at load time (SZLikelihood_Add :1385-1499,
// SZ_init :1501-1821, the fixed grids of deltaN_yz :649-694 and grid_C_2d
// :958-990, the bin limits of integrate_m_zq :845-852).  Host only; sz.hip
// uploads it.  Default-real literals of the reference are widened to double
// here as it widens them (sz_f32).
#pragma once

#include "common.h"

namespace cmamd {

enum { SZ_PRIOR_YSTAR, SZ_PRIOR_ALPHA, SZ_PRIOR_SCATTER, SZ_PRIOR_BETA, SZ_PRIOR_NS, SZ_PRIOR_OMBH2, SZ_PRIOR_LENS,
       SZ_PRIOR_WTG, SZ_PRIOR_CCCP, SZ_NPRIORS };   // in the order SZCC_Cash adds them (:1954-1972)

inline double sz_f32(float x) { return (double)x; }

struct SzData {
    std::string param_names;
    int n_params = 0;
    int Nz = 0, nq = 0;                       // redshift bins, S/N bins (Ny + 1)
    int nthetas = 0, npatches = 0, n_cat = 0;
    int nzs = 0, nm = 0, nlny = 0;            // steps in z, in ln M, nodes in ln Y
    double binz = 0, fsky = 0;
    std::vector<double> Z, logq;              // [Nz], [nq]
    std::vector<double> qmin, qmax;           // [nq] S/N limits of the bins (grid_C_2d :987-990)
    std::vector<double> thetas, skyfracs;     // [nthetas], [npatches]
    std::vector<double> ylims;                // [npatches][nthetas]
    std::vector<double> DNcat;                // [Nz][nq]
    std::vector<double> lnfact;               // [Nz][nq] ln_factorial of the Cash statistic (:1928-1941)
    std::vector<double> steps_z, steps_m;     // [nzs], [nm]
    std::vector<int> j1, j2;                  // [Nz] 0-based: the z trapezoid runs over steps j1 .. j2
    std::vector<double> lny, y0;              // [nlny] lny accumulated, y0 = exp(lny)
    double prior_on[SZ_NPRIORS] = {0};        // 0 or 1, multiplied into the priors as the reference does
};

SzData load_sz(const Ini &ini);

// loader quantities for the tests (cmbl_sz_info / cmbl_sz_arrays)
bool sz_info(const Like *like, int *dims);
bool sz_arrays(const Like *like, double *steps_z, double *dncat, int *j1, int *j2);

}  // namespace cmamd
