// CMBlikes after the window stage: binned spectra, and the small gaussian chi^2.
// (included by cmblikes.hip inside namespace cmamd)
#pragma once

// Binned spectra per (walker, element e = bin * ncl + cl): window columns in
// window order (TBinWindows_bin :1230-1256), each column the l-chunk partials
// in order, plus the linear correction (GetBinnedMapCls :981-995).  Gaussian:
// writes bigX = C - Chat for the used spectra; HL: writes C (+ noise) for the
// transform.  Block (0, 0) zeroes the quadratic-form tickets; element 0 also
// pads the bigX row and writes the calibration-prior addend.
__global__ __launch_bounds__(256) void cmbl_reduce_kernel(CLDev c, const double *__restrict__ partial,
                                                         const double *__restrict__ nuis, long long ld_nuis,
                                                         double *__restrict__ xrows, double *__restrict__ cmat,
                                                         double *__restrict__ addend, unsigned int *__restrict__ counters,
                                                         int n_counters, int W)
{
    // a workgroup is 64 walkers x four elements, one per wave (BK15's 702 elements
    // have 3 partial rows each: 702 x 16 four-wave workgroups, three waves of each
    // mostly idle, took 11.8 us)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.y * 4 + wave;
    const int w = blockIdx.x * 64 + lane;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < n_counters; i += 256) counters[i] = 0u;
    const int Wc = live_walkers(c.wcount, W);
    if (blockIdx.x * 64 >= Wc || e >= c.nE) return;
    // window columns in window order, each the l-chunk partials in order (flattened on
    // the host); four interleaved sums k over rows k, k+4, ... eight loads at a time,
    // combined in fixed order: deterministic (and the order the earlier four-wave
    // form had, wave k taking sum k)
    auto rows_sum = [&](const int *off, const int *rows) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (w < Wc) {
            const int q0 = off[e], q1 = off[e + 1];
#pragma unroll
            for (int k = 0; k < 4; k++)
                for (int q = q0 + k; q < q1; q += 32) {
                    double t[8];
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        t[u] = (q + 4 * u < q1) ? partial[(long long)rows[q + 4 * u] * W + w] : 0.0;
#pragma unroll
                    for (int u = 0; u < 8; u++) v[k] += t[u];
                }
        }
        return ((v[0] + v[1]) + v[2]) + v[3];
    };
    const double main = rows_sum(c.e_main_off, c.e_main_rows);
    const double corr = c.has_corr ? rows_sum(c.e_corr_off, c.e_corr_rows) : 0.0;
    if (w >= Wc) return;
    double s = c.e_main_const[e] + main;
    if (c.has_corr) {
        const double cs = c.e_corr_const[e] + corr;
        s = s + (cs - c.fidcorr[e]);
    }
    double *x = xrows + (long long)w * c.Np;
    if (c.approx == 2) {
        const int ix = c.e_to_x[e];
        if (ix >= 0) x[ix] = s - c.chat[e];
    } else {
        cmat[(long long)w * c.nE + e] = s + c.noise[e];
    }
    if (e == 0) {
        for (int k = c.nX; k < c.Np; k++) x[k] = 0.0;
        if (addend) {
            double a = 0.0;
            if (c.log_cal_prior > 0 && c.cal_index >= 0) {
                const double t = log(nuis[(long long)w * ld_nuis + c.cal_index]) / c.log_cal_prior;
                a = t * t / 2;
            }
            addend[w] = a;
        }
    }
}

// Small gaussian likelihoods (nX <= 64, e.g. lensing 9, SPT-SZ 47): the
// whole chi^2 in one kernel (smallgauss.h).  The host cuts the partial rows of
// every element into tasks of <= 8 rows.
template <int WT>
__global__ __launch_bounds__(256) void cmbl_gauss_small_kernel(SmallGaussLaunch a, int ng)
{
    __shared__ double lds[small_gauss_lds_doubles<WT>()];
    const int q = small_gauss_group(blockIdx.x, ng);
    if (q < ng) small_gauss_body<WT>(a, lds, q);
}
