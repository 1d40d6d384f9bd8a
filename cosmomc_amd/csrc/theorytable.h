// Tabulated likelihoods on derived quantities (cmbg_create_table,
// theory_table_kernel): the reference's BAO likelihoods that are no Gaussians,
// BAO_MGS_loglike (bao.f90:390-410: a chi^2 tabulated in alpha = (D_V / r_drag)
// / (D_V / r_drag)_fid) and BAO_DR1x_loglike (:346-376: a probability on a grid
// of alpha_perp x alpha_plel, interpolated bilinearly).  Included by
// theorycalc.hip behind tc_basis_tile.
//
// The surfaces are columns 0 and 1 of theory_gauss_kernel's accumulator group
// 0 (dcoef [Kp][TD_ND], the same fma chain per column), so v has
// cmbt_derived_eval's bits.  A thread owns one point; LDS holds the scaled
// inputs alone.  Every division is an IEEE division and every operation stands
// in the reference's order (the build has -ffp-contract=off); the table is read
// from global memory, two (1-D) or four (2-D) entries a point, beside the four
// knots of the cell.
#pragma once

namespace cmamd {

struct TheoryTableArgs {
    TheoryBasisArgs b;
    const double *dcoef;                 // [Kp][TD_ND]
    const double *table;                 // 1-D: [tn]; 2-D: perp [tn], plel [tn], prob [tn][tn]
    int form, tn;
    double p[8];                         // cmbg::p
    double *out;                         // [M]
    int *fail;
};

// 1-D (BAO_MGS_loglike): alpha = v0 / scale; outside [x_min, x_max] logZero;
// ii = floor((alpha - x_min) / step); out = ((table[ii] + table[ii + 1]) / 2) / 2
__device__ __forceinline__ double tt_eval_1d(const TheoryTableArgs &a, double v0)
{
    const double scale = a.p[0], x_min = a.p[1], x_max = a.p[2], step = a.p[3];
    const double alpha = v0 / scale;
    if (!(alpha >= x_min && alpha <= x_max)) return CMBL_LOGZERO;       // a NaN alpha as well
    const double c = floor((alpha - x_min) / step);
    // cmbg_create_table has checked the cell at x_max, the largest there is;
    // the test here only keeps any index off the table's end
    if (!(c >= 0.0 && c < (double)(a.tn - 1))) return CMBL_LOGZERO;
    const int ii = (int)c;
    const double chi2 = (a.table[ii] + a.table[ii + 1]) / 2.0;
    return chi2 / 2.0;
}

// 2-D (BAO_DR1x_loglike): a_perp = v0 / DA_rd_fid, a_plel = Hrd_fid / v1;
// outside [perp[0], perp[tn - 2]] x [plel[0], plel[tn - 2]] logZero; the cell
// from floor((a - knot[0]) / (knot[1] - knot[0])); prob bilinear in the knots of
// that cell; out = -log(prob) for prob > 0, else logZero
__device__ __forceinline__ double tt_eval_2d(const TheoryTableArgs &a, double v0, double v1)
{
    const int np = a.tn;
    const double a_perp = v0 / a.p[0], a_plel = a.p[1] / v1;
    if (!(a_perp >= a.p[4] && a_perp <= a.p[5] && a_plel >= a.p[6] && a_plel <= a.p[7])) return CMBL_LOGZERO;
    const double ci = floor((a_perp - a.p[4]) / a.p[2]), cj = floor((a_plel - a.p[6]) / a.p[3]);
    if (!(ci >= 0.0 && ci < (double)(np - 1) && cj >= 0.0 && cj < (double)(np - 1))) return CMBL_LOGZERO;
    const int ii = (int)ci, jj = (int)cj;
    const double *__restrict__ perp = a.table, *__restrict__ plel = a.table + np;
    const double *__restrict__ pr = a.table + 2 * (size_t)np + (size_t)ii * np + jj;
    const double x0 = perp[ii], x1 = perp[ii + 1], y0 = plel[jj], y1 = plel[jj + 1];
    const double p00 = pr[0], p01 = pr[1], p10 = pr[np], p11 = pr[np + 1];
    const double lead = 1.0 / ((x1 - x0) * (y1 - y0));
    const double t1 = p00 * (x1 - a_perp) * (y1 - a_plel);
    const double t2 = p10 * (x0 - a_perp) * (y1 - a_plel);
    const double t3 = p01 * (x1 - a_perp) * (y0 - a_plel);
    const double t4 = p11 * (x0 - a_perp) * (y0 - a_plel);
    const double prob = lead * (((t1 - t2) - t3) + t4);
    return prob > 0.0 ? -log(prob) : CMBL_LOGZERO;
}

__global__ __launch_bounds__(TD_THREADS) void theory_table_kernel(TheoryTableArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];   // [n_in][TD_TM] scaled inputs
    const int m = blockIdx.x * TD_TM + threadIdx.x;
    const double *__restrict__ dcoef = a.dcoef;
    double acc[2] = {0.0, 0.0};                    // the two columns in use of group 0
    const int bad = tc_basis_tile<TD_TM, TD_THREADS>(a.b, blockIdx.x * TD_TM, lds, [&](int k, int, double b) {
        const double *__restrict__ c = dcoef + (size_t)k * TD_ND;
        acc[0] = __builtin_fma(b, c[0], acc[0]);
        acc[1] = __builtin_fma(b, c[1], acc[1]);
    });
    if (m >= a.b.W) return;
    double r = CMBL_LOGZERO;
    if (!bad) r = a.form == CMBG_TABLE_1D ? tt_eval_1d(a, acc[0]) : tt_eval_2d(a, acc[0], acc[1]);
    a.out[m] = r;
    if (a.fail) a.fail[m] = bad;
}

}  // namespace cmamd
