// DES-format weak-lensing and galaxy-clustering likelihood (source/wl.f90): what
// the loader reads from a dataset and derives at load time (WL_ReadIni :104-299,
// init_bessel_integration :320-369).  Host only; wl.hip uploads it.
#pragma once

#include "common.h"

namespace cmamd {

enum { WL_XIP, WL_XIM, WL_GAMMAT, WL_WTHETA, WL_NTYPES };   // measurement_names (:16-19), 0-based

struct WlColumn {   // one Limber sum: a bin pair of a wanted type other than xim (:570-595)
    int type, f1, f2;   // bins 1-based as in the measurement files
};

struct WlData {
    std::string name, param_names;
    int n_params = 0;
    int nzb = 0, ngal = 0, ntheta = 0, nz = 0, nl = 0;
    double acc = 1.0, ah_factor = 1.0;
    int lmax = 50000;
    bool ia_des1yr = true, use_weyl = false;
    std::vector<double> z_p;                  // [nz]
    std::vector<double> p_src, d2_src;        // [nzb][nz] n(z) knots and natural-spline second derivatives
    std::vector<double> p_gal, d2_gal;        // [ngal][nz]
    std::vector<double> theta_bins, theta_rad;
    std::vector<int> data_types;              // the dataset's data_types, 0-based type codes
    bool want[WL_NTYPES] = {false, false, false, false};
    std::vector<std::vector<std::pair<int, int>>> pairs;   // per data type, in file order
    int n_used = 0, first_theta_bin_used = 0, xim_index = 0;
    std::vector<int> used_items;              // [n_used][4]: type index (1-based), bin1, bin2, theta bin
    std::vector<int> used_indices;            // [n_used] 1-based rows of the covariance file
    std::vector<double> data_vector;          // [n_used]
    std::vector<double> invcov;               // [n_used][n_used]
    std::vector<int> ls_cl;                   // [nl]
    std::vector<double> ls_bessel;            // [nb]
    std::vector<double> bessel;               // [3][nb][nth]: orders 0, 2, 4; nth = ntheta - first + 1
    std::vector<WlColumn> columns;
};

WlData load_wl(const Ini &ini);

// loader quantities for the tests (cmbl_wl_info / cmbl_wl_arrays)
bool wl_info(const Like *like, int *dims);
bool wl_arrays(const Like *like, int *ls_cl, double *ls_bessel, int *used_items);

}  // namespace cmamd
