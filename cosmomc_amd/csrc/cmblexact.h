// (included by cmblikes.hip inside namespace cmamd)
#pragma once

// ------------------------------------------------------- exact (unbinned)
// like_approx = exact: per l, C = MapCl(l) + N_l (n x n over the used maps) and
// ExactChiSq (CMBlikes.f90:967-979)
//   chi2_l = (2l+1) fksy (tr M - n - ln det M),  M = C^-1/2 Chat_l C^-1/2.
// tr M = tr(C^-1 Chat) = |L^-1 R|_F^2 with C = L L^T and Chat = R R^T (R and
// ln det Chat = 2 sum ln R_ii from the host), and ln det M = ln det Chat - ln det C,
// so a thread needs one n x n Cholesky and a triangular solve instead of two
// eigendecompositions.  A C that is not positive definite gives NaN (the
// reference's C^-1/2 takes a negative eigenvalue to the power -1/2).
template <int N>
__global__ __launch_bounds__(256) void cmbl_exact_kernel(ExactDev x, const double *__restrict__ dl, long long ld_field,
                                                         long long ld_walker, const double *__restrict__ nuis,
                                                         long long ld_nuis, double *__restrict__ out, int W)
{
    constexpr int NC = N * (N + 1) / 2;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * EXACT_WPB + (threadIdx.x >> 6);
    if (w >= W) return;                                   // wave-uniform
    double calsq = 1.0;
    if (x.cal_index >= 0) {
        const double cal = nuis[(long long)w * ld_nuis + x.cal_index];
        calsq = cal * cal;
    }
    const double *Dw = dl + (long long)w * ld_walker;
    double acc = 0.0;
    for (int b = lane; b < x.nb; b += 64) {
        const int l = x.bmin + b;
        const double *t = x.tab + (long long)b * x.K;
        double C[NC];
#pragma unroll
        for (int e = 0; e < NC; e++) {                    // GetTheoryMapCls + AdaptTheoryForMaps :1022-1126
            const double *Df = Dw + (long long)x.field[e] * ld_field;
            double v = Df[l];
            if (x.aberration != 0.0 && x.cmb[e]) {        // AddAberration :1062-1101
                int la = l - 1, lb = l + 1;
                if (l == x.lmin) { la = l; lb = l + 2; }
                else if (l == x.lmax) { la = l - 2; lb = l; }
                const double ea = la, eb = lb, el = l;
                const double ca = Df[la] / (ea * (ea + 1)), cb = Df[lb] / (eb * (eb + 1));
                const double deriv = 0.5 * (cb - ca);
                v = v + x.aberration * (el * el * (el + 1) * deriv);
            }
            if (x.cal_index >= 0 && x.cmb[e]) v = v / calsq;
            C[e] = v + t[e];                              // C + NoiseM(bin) :1200-1202
        }
        // C = L L^T (lower packed, in place); ln det C
        double lndet_c = 0.0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            double d = C[j * (j + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; k++) d -= C[j * (j + 1) / 2 + k] * C[j * (j + 1) / 2 + k];
            d = sqrt(d);                                  // NaN when C is not positive definite
            C[j * (j + 1) / 2 + j] = d;
            lndet_c += log(d);
#pragma unroll
            for (int i = j + 1; i < N; i++) {
                double s = C[i * (i + 1) / 2 + j];
#pragma unroll
                for (int k = 0; k < j; k++) s -= C[i * (i + 1) / 2 + k] * C[j * (j + 1) / 2 + k];
                C[i * (i + 1) / 2 + j] = s / d;
            }
        }
        // tr(C^-1 Chat) = |L^-1 R|_F^2, column by column of R (lower triangular)
        double tr = 0.0;
#pragma unroll
        for (int c = 0; c < N; c++) {
            double y[N];
#pragma unroll
            for (int i = 0; i < N; i++) {
                double s = (i >= c) ? t[x.ncl + i * (i + 1) / 2 + c] : 0.0;
#pragma unroll
                for (int k = 0; k < i; k++) s -= C[i * (i + 1) / 2 + k] * y[k];
                y[i] = s / C[i * (i + 1) / 2 + i];
                tr += y[i] * y[i];
            }
        }
        const double lndet_m = t[2 * x.ncl] - 2.0 * lndet_c;
        acc += t[2 * x.ncl + 1] * (tr - N - lndet_m);
    }
    // fixed-order wave reduction (deterministic)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
        double chisq = acc;
        if (x.log_cal_prior > 0 && x.cal_index >= 0) {   // :1222-1223
            const double lc = log(nuis[(long long)w * ld_nuis + x.cal_index]) / x.log_cal_prior;
            chisq = chisq + lc * lc;
        }
        out[w] = chisq / 2;
    }
}
