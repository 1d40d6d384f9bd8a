// The alpha, beta-marginalised JLA likelihood (JLA_marginalize = T,
// source/supernovae_JLA.f90:235-252, 1207-1217): cmbl_open tag "JLA_MARGE".
// jlamarge.hip holds its set-up at open (V(alpha_g, beta_g)^-1 of every grid
// point, formed on the device) and the kernels of an evaluation.
#pragma once

#include "jla.h"

namespace cmamd {

// the reference's single-precision literals (:119-120), promoted as it promotes them
inline double jla_marge_alpha_center() { return (double)0.14f; }
inline double jla_marge_beta_center() { return (double)3.123f; }
static constexpr int JLA_MARGE_MAX_STEPS = 16;

// The grid of JLALikelihood_Add (:243-251): alpha_i outer, beta_i inner, the
// points with alpha_i^2 + beta_i^2 <= steps^2.
void jla_marge_grid(int steps, double width_alpha, double width_beta, double center_alpha, double center_beta,
                    std::vector<double> &alpha, std::vector<double> &beta);

std::unique_ptr<Like> make_jla_marge(const Ini &ini);
// false when the likelihood is not a marginalised JLA; n_points: the grid's
// points, n_grid: those the reference keeps, grid_bytes: device bytes of their inverses
bool jla_marge_info(const Like *like, int *n_grid, int *n_points, size_t *grid_bytes);

}  // namespace cmamd
