// Polynomial theory calculator: dl[w][field][l] = sum_k basis_k(w) coef[k][field][l],
// a GEMM out[W x N] = B[W x K] . C[K x N] whose left operand (the monomials of
// every walker's scaled slow parameters) is built in the launch from the
// sampler's parameter rows and whose right operand (the coefficient table)
// stays on the device.  One launch fills one theory buffer.
//
// Arithmetic: explicit f64 fma in ascending k from +0.0 (the build has
// -ffp-contract=off, so the fusion is written out).  On gfx950 the vector and
// the matrix f64 peak rates are the same, so the register-tiled fma gives up
// no throughput against v_mfma_f64_16x16x4f64 and keeps the summation order
// plain: a walker's bits depend on neither W, its place in the batch nor the
// strides, and the zero padding of k adds exact zeros.
//
// Derived parameters (cmbt_set_derived / cmbt_derived_eval): up to 32 scalar
// surfaces over the same monomials, summed by the same chain, in a kernel of
// their own (theory_derived_kernel) tiled for few outputs and many points.
//
// Gaussian likelihoods on such surfaces (cmbg_*, theory_gauss_kernel): the
// same accumulators, then (v - obs)^T invcov (v - obs) / 2 per point.
//
// Tabulated likelihoods on 1 or 2 such surfaces (cmbg_create_table,
// theory_table_kernel in theorytable.h): a table lookup with a hard edge.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "theorycalc.h"

namespace cmamd {

// What a kernel needs to form the monomials of a tile of points
struct TheoryBasisArgs {
    const double *meta;                  // [4][TC_MAXIN]: lo, hi, center, scale
    const int *pidx;
    const unsigned long long *expo;      // [Kp] 4 bits per input, input 0 lowest
    int n_in, K, Kp, W;
    const double *P;
    long long ld;
};

struct TheoryCalcArgs {
    TheoryBasisArgs b;
    const int *fields;
    const double *coef;                  // [n_fields][Kp][Lp]
    int lmax, Lp, ntl;
    double *dl;
    long long ld_field, ld_walker;
    int *fail;
};

struct TheoryDerivedArgs {
    TheoryBasisArgs b;
    const double *dcoef;                 // [Kp][TD_ND]
    const double *dlim;                  // [2][TD_ND] lo, hi; null: no range test
    int nd;
    double *out;                         // [nd][ld_out]; null: the flags only
    long long ld_out;
    int *fail;
};

struct TheoryGaussArgs {
    TheoryBasisArgs b;
    const double *dcoef;                 // [Kp][TD_ND]
    const double *obs;                   // [TD_ND]
    const double *invcov;                // [n][n]
    int n;
    double *out;                         // [M]
    int *fail;
};

// Box test and monomials of points w0 .. w0 + TW - 1 by the NT threads of a
// workgroup, for both kernels (xs [n_in][TW]: LDS for the scaled inputs).
// Each pass forms NT / TW terms: thread t hands term k = k0 + t / TW of point
// w0 + t % TW to sink(k, point in tile, value), its k ascending up to Kp.
// With NT == TW a thread owns one point and k is uniform (scalar exponent
// loads and loops).  Returns, in thread t < TW, whether point w0 + t fails the
// box; no barrier after the last sink.
template <int TW, int NT, class Sink>
__device__ __forceinline__ int tc_basis_tile(const TheoryBasisArgs &a, int w0, double *xs, Sink &&sink)
{
    static_assert(NT % TW == 0, "whole terms per pass");
    constexpr int KS = NT / TW;
    const int t = threadIdx.x;
    int bad = 0;
    // validity box on the raw parameters (equality passes, NaN fails); a failed
    // walker is evaluated at its inputs clamped into the box (NaN: the centre),
    // so the buffer never holds junk
    if (t < TW) {
        const int w = w0 + t;
        for (int i = 0; i < a.n_in; i++) {
            double x = 0.0;
            if (w < a.W) {
                double p = a.P[(size_t)(a.pidx[i] - 1) * a.ld + w];
                const double lo = a.meta[i], hi = a.meta[TC_MAXIN + i];
                const double c = a.meta[2 * TC_MAXIN + i], s = a.meta[3 * TC_MAXIN + i];
                if (!(p >= lo && p <= hi)) {
                    bad = 1;
                    if (p != p) p = c;
                    p = p < lo ? lo : (p > hi ? hi : p);
                }
                x = (p - c) / s;
            }
            xs[i * TW + t] = x;
        }
    }
    __syncthreads();
    // basis_k = prod_i x_i^e_ki from 1.0, inputs ascending, powers by repeated multiplication
    const int wl = KS == 1 ? t : t % TW, kq = KS == 1 ? 0 : t / TW;
    for (int k0 = 0; k0 < a.Kp; k0 += KS) {        // (Kp is a multiple of TC_KC, and so of KS)
        const int k = k0 + kq;
        double b = 0.0;                            // the padding of k: exact zeros
        if (k < a.K) {
            unsigned long long e = a.expo[k];
            b = 1.0;
            for (int i = 0; i < a.n_in; i++, e >>= 4) {
                const double x = xs[i * TW + wl];
                for (int r = (int)(e & 15); r > 0; r--) b *= x;
            }
        }
        sink(k, wl, b);
    }
    return bad;
}

// Workgroup (x: field j and l tile, y: walker tile): TC_TW walkers x TC_TN l.
// Thread t holds 8 walkers (its wave's) x 4 l (2 * lane, + 1 and the same 128
// further on), so a wave stores two 1 KB runs of consecutive l per walker row.
__global__ __launch_bounds__(TC_THREADS) void theory_calc_kernel(TheoryCalcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int Kp = a.b.Kp;
    double *Bs = lds;                              // [Kp][TC_TW] monomials
    double *Cs = Bs + (size_t)Kp * TC_TW;          // [TC_KC][TC_TN] coefficient chunk
    double *xs = Cs;                               // before the first chunk: [n_in][TC_TW] scaled inputs
    const int t = threadIdx.x;
    const int w0 = blockIdx.y * TC_TW;
    const int j = blockIdx.x / a.ntl, l0 = (blockIdx.x % a.ntl) * TC_TN;

    static_assert(TC_KC % (TC_THREADS / TC_TW) == 0, "the terms of a pass divide the padding of K");
    const int bad =
        tc_basis_tile<TC_TW, TC_THREADS>(a.b, w0, xs, [&](int k, int wl, double b) { Bs[k * TC_TW + wl] = b; });
    if (t < TC_TW && a.fail && blockIdx.x == 0 && w0 + t < a.b.W) a.fail[w0 + t] = bad;

    const int lane = t & 63, wv = t >> 6;
    double acc[8][4];
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[r][q] = 0.0;
    // chunk loads: TC_KC rows x TC_TN doubles = 4 double2 a thread, the next
    // chunk fetched into registers while this one is multiplied
    const double *Cg = a.coef + (size_t)j * Kp * a.Lp + l0;
    constexpr int C2 = TC_TN / 2;                  // double2 per chunk row
    constexpr int NPRE = TC_KC * C2 / TC_THREADS;
    static_assert(NPRE == 4, "four double2 of the chunk a thread");
    // this thread's pieces of chunk row r = q * (TC_THREADS / C2) + t / C2
    const double *Ct = Cg + (size_t)(t / C2) * a.Lp + 2 * (t % C2);
    const size_t rstep = (size_t)(TC_THREADS / C2) * a.Lp;
#define TC_FETCH(k0)                                                                  \
    p0 = *reinterpret_cast<const double2 *>(Ct + (size_t)(k0) * a.Lp);                \
    p1 = *reinterpret_cast<const double2 *>(Ct + (size_t)(k0) * a.Lp + rstep);        \
    p2 = *reinterpret_cast<const double2 *>(Ct + (size_t)(k0) * a.Lp + 2 * rstep);    \
    p3 = *reinterpret_cast<const double2 *>(Ct + (size_t)(k0) * a.Lp + 3 * rstep);
    double2 p0, p1, p2, p3;
    TC_FETCH(0)
    double2 *Cs2 = reinterpret_cast<double2 *>(Cs);
    for (int k0 = 0; k0 < Kp; k0 += TC_KC) {
        __syncthreads();                           // xs / the previous chunk have been read
        Cs2[t] = p0;
        Cs2[t + TC_THREADS] = p1;
        Cs2[t + 2 * TC_THREADS] = p2;
        Cs2[t + 3 * TC_THREADS] = p3;
        __syncthreads();
        if (k0 + TC_KC < Kp) {
            TC_FETCH(k0 + TC_KC)
        }
#pragma unroll
        for (int kk = 0; kk < TC_KC; kk++) {
            const double2 c01 = Cs2[kk * C2 + lane], c23 = Cs2[kk * C2 + 64 + lane];   // 16-byte lane stride: no bank conflict
            const double2 *bp = reinterpret_cast<const double2 *>(Bs + (size_t)(k0 + kk) * TC_TW + wv * 8);
            const double2 b01 = bp[0], b23 = bp[1], b45 = bp[2], b67 = bp[3];
#define TC_ROW(r, bb)                                   \
    acc[r][0] = __builtin_fma(bb, c01.x, acc[r][0]);    \
    acc[r][1] = __builtin_fma(bb, c01.y, acc[r][1]);    \
    acc[r][2] = __builtin_fma(bb, c23.x, acc[r][2]);    \
    acc[r][3] = __builtin_fma(bb, c23.y, acc[r][3]);
            TC_ROW(0, b01.x) TC_ROW(1, b01.y) TC_ROW(2, b23.x) TC_ROW(3, b23.y)
            TC_ROW(4, b45.x) TC_ROW(5, b45.y) TC_ROW(6, b67.x) TC_ROW(7, b67.y)
#undef TC_ROW
        }
    }
#undef TC_FETCH
    // stores: per walker row two wave-wide runs of consecutive l (1 KB each),
    // 16 bytes a lane; a row that is only 8-byte aligned (odd ld_field or
    // ld_walker) and the row's tail take 8-byte stores
    double *colp = a.dl + (long long)a.fields[j] * a.ld_field;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int w = w0 + wv * 8 + r;
        if (w < a.b.W) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int l = l0 + h * (TC_TN / 2) + 2 * lane;
                double *p = colp + (long long)w * a.ld_walker + l;
                const double v0 = acc[r][2 * h], v1 = acc[r][2 * h + 1];
                if (l + 1 <= a.lmax && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                    *reinterpret_cast<double2 *>(p) = make_double2(v0, v1);
                } else {
                    if (l <= a.lmax) p[0] = v0;
                    if (l + 1 <= a.lmax) p[1] = v1;
                }
            }
        }
    }
}

// Derived outputs out[d][m] = sum_k basis_k(m) dcoef[k][d]: the same monomials
// and the same fma chain as theory_calc_kernel, so an output whose coefficients
// are a D_l column has that D_l's bits.  A thread owns one point and all its
// outputs (up to 32 accumulators in registers, in groups of 8 behind uniform
// branches); term k is uniform over the workgroup, so its exponents and its
// coefficient row come by scalar loads and a monomial costs a thread its
// n_in LDS reads and at most 4 multiplications for up to 32 fma.  LDS holds
// only the scaled inputs (n_in x 2 KB), so a CU keeps several workgroups.
// Output rows are stored in 2 KB runs of consecutive points.
__global__ __launch_bounds__(TD_THREADS) void theory_derived_kernel(TheoryDerivedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];   // [n_in][TD_TM] scaled inputs
    const int m = blockIdx.x * TD_TM + threadIdx.x;
    const int ng = (a.nd + 7) >> 3;                // groups of 8 outputs in use
    const double *__restrict__ dcoef = a.dcoef;
    double acc[TD_ND];
#pragma unroll
    for (int d = 0; d < TD_ND; d++) acc[d] = 0.0;
#define TD_GROUP(g)                                                                              \
    _Pragma("unroll") for (int q = 8 * (g); q < 8 * (g) + 8; q++) acc[q] = __builtin_fma(b, c[q], acc[q]);
    const int bad = tc_basis_tile<TD_TM, TD_THREADS>(a.b, blockIdx.x * TD_TM, lds, [&](int k, int, double b) {
        const double *__restrict__ c = dcoef + (size_t)k * TD_ND;
        TD_GROUP(0)
        if (ng > 1) { TD_GROUP(1) }
        if (ng > 2) { TD_GROUP(2) }
        if (ng > 3) { TD_GROUP(3) }
    });
#undef TD_GROUP
    if (m >= a.b.W) return;
    // range test lo <= v <= hi (equality passes, NaN fails) and the stores
    int out_of_range = 0;
#pragma unroll
    for (int d = 0; d < TD_ND; d++) {
        if (d < a.nd) {
            if (a.dlim && !(acc[d] >= a.dlim[d] && acc[d] <= a.dlim[TD_ND + d])) out_of_range = 1;
            if (a.out) a.out[(long long)d * a.ld_out + m] = acc[d];
        }
    }
    if (a.fail) a.fail[m] = bad | out_of_range;
}

// Gaussian likelihood on derived quantities: out[m] = (v - obs)^T invcov
// (v - obs) / 2 with v the n surfaces of theory_derived_kernel (the same
// accumulator groups, so v_i has its bits).  A thread owns one point.  Its
// residuals r_i = v_i - obs_i go to an LDS column of its own ([n][TD_TM],
// consecutive threads in consecutive doubles: no bank conflict), which lies
// over the scaled inputs: with a point per thread tc_basis_tile reads and
// writes only the thread's own column of them, and is done with it.  The
// quadratic form's loops then run over LDS addresses, not over a register
// array; obs and invcov are uniform and come by scalar loads.
//   y_i = fma(invcov[i][j], r_j, y_i), j ascending from +0.0
//   s   = fma(r_i, y_i, s),            i ascending from +0.0;   out = s / 2
// A point outside the box gets logZero.
__global__ __launch_bounds__(TD_THREADS) void theory_gauss_kernel(TheoryGaussArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];   // [max(n_in, n)][TD_TM]
    const int m = blockIdx.x * TD_TM + threadIdx.x;
    const int n = a.n, ng = (n + 7) >> 3;
    const double *__restrict__ dcoef = a.dcoef;
    double acc[TD_ND];
#pragma unroll
    for (int d = 0; d < TD_ND; d++) acc[d] = 0.0;
#define TD_GROUP(g)                                                                              \
    _Pragma("unroll") for (int q = 8 * (g); q < 8 * (g) + 8; q++) acc[q] = __builtin_fma(b, c[q], acc[q]);
    const int bad = tc_basis_tile<TD_TM, TD_THREADS>(a.b, blockIdx.x * TD_TM, lds, [&](int k, int, double b) {
        const double *__restrict__ c = dcoef + (size_t)k * TD_ND;
        TD_GROUP(0)
        if (ng > 1) { TD_GROUP(1) }
        if (ng > 2) { TD_GROUP(2) }
        if (ng > 3) { TD_GROUP(3) }
    });
#undef TD_GROUP
    double *r = lds + threadIdx.x;
    const double *__restrict__ obs = a.obs;
#pragma unroll
    for (int d = 0; d < TD_ND; d++)
        if (d < n) r[d * TD_TM] = acc[d] - obs[d];
    const double *__restrict__ ic = a.invcov;
    double s = 0.0;
    for (int i = 0; i < n; i++) {
        double y = 0.0;
        for (int j = 0; j < n; j++) y = __builtin_fma(ic[i * n + j], r[j * TD_TM], y);
        s = __builtin_fma(r[i * TD_TM], y, s);
    }
    if (m >= a.b.W) return;
    a.out[m] = bad ? CMBL_LOGZERO : s / 2;
    if (a.fail) a.fail[m] = bad;
}

}  // namespace cmamd

#include "theorytable.h"

namespace cmamd {

static size_t tc_lds_bytes(int Kp) { return ((size_t)Kp * TC_TW + (size_t)TC_KC * TC_TN) * 8; }
static size_t td_lds_bytes(int n_in) { return (size_t)n_in * TD_TM * 8; }

void theorycalc_create(cmbt *t, const cmbt_config_t *c) {
    if (c->n_in < 1 || c->n_in > TC_MAXIN) fail(CMBL_ERR_ARG, "cmbt_create: n_in must be in 1..%d", TC_MAXIN);
    if (c->n_terms < 1 || c->n_terms > TC_MAXTERMS)
        fail(CMBL_ERR_ARG, "cmbt_create: n_terms must be in 1..%d", TC_MAXTERMS);
    if (c->n_fields < 1 || c->n_fields > CMBL_NFIELDS)
        fail(CMBL_ERR_ARG, "cmbt_create: n_fields must be in 1..%d", CMBL_NFIELDS);
    if (c->lmax < 0) fail(CMBL_ERR_ARG, "cmbt_create: lmax must not be negative");
    if (!c->param_index || !c->center || !c->scale || !c->lo || !c->hi || !c->exponents || !c->fields || !c->coef)
        fail(CMBL_ERR_ARG, "cmbt_create: null table");
    const int n_in = c->n_in, K = c->n_terms, nf = c->n_fields;
    std::vector<double> meta(4 * TC_MAXIN, 0.0);
    for (int i = 0; i < n_in; i++) {
        if (c->param_index[i] < 1) fail(CMBL_ERR_ARG, "cmbt_create: param_index %d is not 1-based", c->param_index[i]);
        if (!(c->scale[i] != 0.0)) fail(CMBL_ERR_ARG, "cmbt_create: scale of input %d must not be 0", i);
        if (!(c->lo[i] <= c->hi[i])) fail(CMBL_ERR_ARG, "cmbt_create: input %d has lo > hi", i);
        meta[i] = c->lo[i];
        meta[TC_MAXIN + i] = c->hi[i];
        meta[2 * TC_MAXIN + i] = c->center[i];
        meta[3 * TC_MAXIN + i] = c->scale[i];
    }
    const int Kp = (K + TC_KC - 1) / TC_KC * TC_KC;
    std::vector<unsigned long long> expo(Kp, 0ull);
    for (int k = 0; k < K; k++) {
        int sum = 0;
        for (int i = 0; i < n_in; i++) {
            const int e = c->exponents[(size_t)k * n_in + i];
            if (e < 0) fail(CMBL_ERR_ARG, "cmbt_create: negative exponent in term %d", k);
            sum += e;
            if (sum > TC_MAXORDER) fail(CMBL_ERR_ARG, "cmbt_create: term %d has order above %d", k, TC_MAXORDER);
            expo[k] |= (unsigned long long)e << (4 * i);
        }
    }
    bool seen[CMBL_NFIELDS] = {};
    for (int j = 0; j < nf; j++) {
        const int f = c->fields[j];
        if (f < 0 || f >= CMBL_NFIELDS) fail(CMBL_ERR_ARG, "cmbt_create: field %d outside 0..%d", f, CMBL_NFIELDS - 1);
        if (seen[f]) fail(CMBL_ERR_ARG, "cmbt_create: field %d repeated", f);
        seen[f] = true;
    }
    const int L = c->lmax + 1, Lp = (L + TC_TN - 1) / TC_TN * TC_TN;
    std::vector<double> coef((size_t)nf * Kp * Lp, 0.0);
    for (int k = 0; k < K; k++)
        for (int j = 0; j < nf; j++)
            std::copy(c->coef + ((size_t)k * nf + j) * L, c->coef + ((size_t)k * nf + j + 1) * L,
                      coef.begin() + ((size_t)j * Kp + k) * Lp);
    t->n_in = n_in;
    t->K = K;
    t->Kp = Kp;
    t->n_fields = nf;
    t->lmax = c->lmax;
    t->Lp = Lp;
    t->pidx.assign(c->param_index, c->param_index + n_in);
    upload(t->meta, meta);
    upload(t->pidx_d, t->pidx);
    upload(t->fields_d, std::vector<int>(c->fields, c->fields + nf));
    upload(t->expo, expo);
    upload(t->coef, coef);
    HIP_CHECK(hipFuncSetAttribute((const void *)theory_calc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)tc_lds_bytes(TC_MAXTERMS)));
}

static TheoryBasisArgs basis_args(const cmbt *t, int W, const double *P, long long ld) {
    TheoryBasisArgs b{};
    b.meta = t->meta.as<double>();
    b.pidx = t->pidx_d.as<int>();
    b.expo = t->expo.as<unsigned long long>();
    b.n_in = t->n_in;
    b.K = t->K;
    b.Kp = t->Kp;
    b.W = W;
    b.P = P;
    b.ld = ld;
    return b;
}

// out == nullptr: the failure flags only
static void launch_derived(cmbt *t, int M, const double *P, long long ld, double *out, long long ld_out,
                           int *fail_flags, hipStream_t stream) {
    TheoryDerivedArgs a{};
    a.b = basis_args(t, M, P, ld);
    a.dcoef = t->dcoef.as<double>();
    a.dlim = t->ranged ? t->dlim.as<double>() : nullptr;
    a.nd = t->n_derived;
    a.out = out;
    a.ld_out = ld_out;
    a.fail = fail_flags;
    timed_launch("theory_derived_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
        hipExtLaunchKernelGGL(theory_derived_kernel, dim3((M + TD_TM - 1) / TD_TM), dim3(TD_THREADS),
                              td_lds_bytes(t->n_in), stream, e0, e1, 0, a);
    });
    HIP_CHECK(hipGetLastError());
}

void theorycalc_eval(cmbt *t, int W, const double *P, long long ld, int num_params, double *dl, long long ld_field,
                     long long ld_walker, int *fail_flags, hipStream_t stream) {
    if (W <= 0) fail(CMBL_ERR_ARG, "cmbt_eval: W must be positive");
    if (!P || !dl) fail(CMBL_ERR_ARG, "cmbt_eval: null buffer");
    if (ld < W) fail(CMBL_ERR_ARG, "cmbt_eval: ld %lld below W %d", ld, W);
    for (int p : t->pidx)
        if (p > num_params) fail(CMBL_ERR_ARG, "cmbt_eval: param_index %d outside 1..%d", p, num_params);
    if (ld_walker == 0) fail(CMBL_ERR_ARG, "cmbt_eval: per-walker theory rows needed (ld_walker != 0)");
    if (ld_field < t->lmax + 1) fail(CMBL_ERR_ARG, "cmbt_eval: ld_field %lld below lmax + 1 = %d", ld_field, t->lmax + 1);
    TheoryCalcArgs a{};
    a.b = basis_args(t, W, P, ld);
    a.fields = t->fields_d.as<int>();
    a.coef = t->coef.as<double>();
    a.lmax = t->lmax;
    a.Lp = t->Lp;
    a.ntl = t->Lp / TC_TN;
    a.dl = dl;
    a.ld_field = ld_field;
    a.ld_walker = ld_walker;
    a.fail = fail_flags;
    const dim3 grid(t->n_fields * a.ntl, (W + TC_TW - 1) / TC_TW);
    timed_launch("theory_calc_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
        hipExtLaunchKernelGGL(theory_calc_kernel, grid, dim3(TC_THREADS), tc_lds_bytes(t->Kp), stream, e0, e1, 0, a);
    });
    HIP_CHECK(hipGetLastError());
    // with ranges set the flags take the range test in as well: the derived
    // kernel, storing no output, writes box-or-range over the box flags in
    // stream order
    if (t->ranged && fail_flags) launch_derived(t, W, P, ld, nullptr, 0, fail_flags, stream);
}

// With ranges set: box-or-range over the box flags of points that no
// theorycalc_eval has flagged (a sampler with derived likelihoods alone)
void theorycalc_range_flags(cmbt *t, int W, const double *P, long long ld, int *fail_flags, hipStream_t stream) {
    if (t->ranged) launch_derived(t, W, P, ld, nullptr, 0, fail_flags, stream);
}

void theorycalc_set_derived(cmbt *t, const cmbt_derived_config_t *c) {
    if (!c) {
        t->n_derived = 0;
        t->ranged = false;
        t->dcoef.release();
        t->dlim.release();
        return;
    }
    if (c->n_derived < 1 || c->n_derived > TD_ND)
        fail(CMBL_ERR_ARG, "cmbt_set_derived: n_derived must be in 1..%d", TD_ND);
    if (!c->coef) fail(CMBL_ERR_ARG, "cmbt_set_derived: null coefficient table");
    const int nd = c->n_derived;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> lim(2 * TD_ND);
    for (int d = 0; d < TD_ND; d++) {
        lim[d] = c->lo && d < nd ? c->lo[d] : -inf;
        lim[TD_ND + d] = c->hi && d < nd ? c->hi[d] : inf;
        if (!(lim[d] <= lim[TD_ND + d])) fail(CMBL_ERR_ARG, "cmbt_set_derived: output %d has lo > hi", d);
    }
    std::vector<double> coef((size_t)t->Kp * TD_ND, 0.0);
    for (int k = 0; k < t->K; k++)
        std::copy(c->coef + (size_t)k * nd, c->coef + (size_t)(k + 1) * nd, coef.begin() + (size_t)k * TD_ND);
    upload(t->dcoef, coef);
    upload(t->dlim, lim);
    t->n_derived = nd;
    t->ranged = c->lo || c->hi;
}

void theorycalc_derived_eval(cmbt *t, int M, const double *P, long long ld, int num_params, double *out,
                             long long ld_out, int *fail_flags, hipStream_t stream) {
    if (t->n_derived == 0) fail(CMBL_ERR_ARG, "cmbt_derived_eval: no derived outputs set (cmbt_set_derived)");
    if (M <= 0 || M > std::numeric_limits<int>::max() - TD_TM)
        fail(CMBL_ERR_ARG, "cmbt_derived_eval: M must be in 1..%d", std::numeric_limits<int>::max() - TD_TM);
    if (!P || !out) fail(CMBL_ERR_ARG, "cmbt_derived_eval: null buffer");
    if (ld < M) fail(CMBL_ERR_ARG, "cmbt_derived_eval: ld %lld below M %d", ld, M);
    if (ld_out < M) fail(CMBL_ERR_ARG, "cmbt_derived_eval: ld_out %lld below M %d", ld_out, M);
    for (int p : t->pidx)
        if (p > num_params) fail(CMBL_ERR_ARG, "cmbt_derived_eval: param_index %d outside 1..%d", p, num_params);
    launch_derived(t, M, P, ld, out, ld_out, fail_flags, stream);
}

void theorygauss_create(cmbg *g, cmbt *calc, const cmbg_config_t *c) {
    if (c->n < 1 || c->n > CMBG_MAXN) fail(CMBL_ERR_ARG, "cmbg_create: n must be in 1..%d", CMBG_MAXN);
    if (!c->coef || !c->obs || !c->invcov) fail(CMBL_ERR_ARG, "cmbg_create: null table");
    const int n = c->n;
    for (int i = 0; i < n; i++) {
        if (!std::isfinite(c->obs[i])) fail(CMBL_ERR_ARG, "cmbg_create: obs %d is not finite", i);
        for (int j = 0; j < n; j++) {
            if (!std::isfinite(c->invcov[i * n + j])) fail(CMBL_ERR_ARG, "cmbg_create: invcov %d, %d is not finite", i, j);
            if (c->invcov[i * n + j] != c->invcov[j * n + i])
                fail(CMBL_ERR_ARG, "cmbg_create: invcov is not symmetric at %d, %d", i, j);
        }
    }
    static_assert(CMBG_MAXN == TD_ND, "the accumulator groups of theory_derived_kernel");
    std::vector<double> coef((size_t)calc->Kp * TD_ND, 0.0), obs(TD_ND, 0.0);
    for (int k = 0; k < calc->K; k++)
        std::copy(c->coef + (size_t)k * n, c->coef + (size_t)(k + 1) * n, coef.begin() + (size_t)k * TD_ND);
    std::copy(c->obs, c->obs + n, obs.begin());
    g->calc = calc;
    g->n = n;
    upload(g->dcoef, coef);
    upload(g->obs, obs);
    upload(g->invcov, std::vector<double>(c->invcov, c->invcov + (size_t)n * n));
}

// the cell index the kernels form at the upper end of an axis:
// floor((hi - lo) / d), the largest any point inside [lo, hi] gets (the
// subtraction, the division and floor are monotone)
static double table_top_cell(double lo, double hi, double d) { return std::floor((hi - lo) / d); }

void theorytable_create(cmbg *g, cmbt *calc, const cmbg_table_config_t *c) {
    if (c->form != CMBG_TABLE_1D && c->form != CMBG_TABLE_2D)
        fail(CMBL_ERR_ARG, "cmbg_create_table: form must be CMBG_TABLE_1D or CMBG_TABLE_2D");
    if (!c->coef) fail(CMBL_ERR_ARG, "cmbg_create_table: null coefficient table");
    const int ns = c->form == CMBG_TABLE_1D ? 1 : 2;
    std::vector<double> tab;
    if (c->form == CMBG_TABLE_1D) {
        if (!c->table) fail(CMBL_ERR_ARG, "cmbg_create_table: null table");
        if (c->n < 2) fail(CMBL_ERR_ARG, "cmbg_create_table: n must be at least 2");
        if (!std::isfinite(c->scale) || c->scale == 0.0) fail(CMBL_ERR_ARG, "cmbg_create_table: scale must be finite and not 0");
        if (!std::isfinite(c->x_min) || !std::isfinite(c->x_max) || !(c->x_min < c->x_max))
            fail(CMBL_ERR_ARG, "cmbg_create_table: x_min must be below x_max, both finite");
        if (!std::isfinite(c->step) || !(c->step > 0.0)) fail(CMBL_ERR_ARG, "cmbg_create_table: step must be positive");
        for (int i = 0; i < c->n; i++)
            if (!std::isfinite(c->table[i])) fail(CMBL_ERR_ARG, "cmbg_create_table: table entry %d is not finite", i);
        const double top = table_top_cell(c->x_min, c->x_max, c->step);
        if (!(top + 1 < (double)c->n))
            fail(CMBL_ERR_ARG, "cmbg_create_table: at x_max the cell is %.0f, and its upper entry lies beyond the %d of the table",
                 top, c->n);
        tab.assign(c->table, c->table + c->n);
        g->tn = c->n;
        const double p[8] = {c->scale, c->x_min, c->x_max, c->step, 0, 0, 0, 0};
        std::copy(p, p + 8, g->p);
    } else {
        if (!c->perp || !c->plel || !c->prob) fail(CMBL_ERR_ARG, "cmbg_create_table: null table");
        const int np = c->np;
        if (np < 3 || np > 32768) fail(CMBL_ERR_ARG, "cmbg_create_table: np must be in 3..32768");
        if (!std::isfinite(c->DA_rd_fid) || c->DA_rd_fid == 0.0 || !std::isfinite(c->Hrd_fid) || c->Hrd_fid == 0.0)
            fail(CMBL_ERR_ARG, "cmbg_create_table: DA_rd_fid and Hrd_fid must be finite and not 0");
        for (int i = 0; i < np; i++)
            if (!std::isfinite(c->perp[i]) || !std::isfinite(c->plel[i]))
                fail(CMBL_ERR_ARG, "cmbg_create_table: knot %d is not finite", i);
        for (size_t i = 0; i < (size_t)np * np; i++)
            if (!std::isfinite(c->prob[i])) fail(CMBL_ERR_ARG, "cmbg_create_table: prob entry %zu is not finite", i);
        const double *axis[2] = {c->perp, c->plel};
        double d[2];
        for (int x = 0; x < 2; x++) {
            d[x] = axis[x][1] - axis[x][0];
            if (!(d[x] > 0.0)) fail(CMBL_ERR_ARG, "cmbg_create_table: axis %d has knot[1] - knot[0] <= 0", x);
            const double top = table_top_cell(axis[x][0], axis[x][np - 2], d[x]);
            if (!(top + 1 < (double)np))
                fail(CMBL_ERR_ARG, "cmbg_create_table: axis %d: at knot[np - 2] the cell is %.0f, beyond the grid", x, top);
        }
        tab.reserve(2 * (size_t)np + (size_t)np * np);
        tab.insert(tab.end(), c->perp, c->perp + np);
        tab.insert(tab.end(), c->plel, c->plel + np);
        tab.insert(tab.end(), c->prob, c->prob + (size_t)np * np);
        g->tn = np;
        const double p[8] = {c->DA_rd_fid, c->Hrd_fid, d[0], d[1], c->perp[0], c->perp[np - 2], c->plel[0], c->plel[np - 2]};
        std::copy(p, p + 8, g->p);
    }
    std::vector<double> coef((size_t)calc->Kp * TD_ND, 0.0);
    for (int k = 0; k < calc->K; k++) {
        for (int s = 0; s < ns; s++)
            if (!std::isfinite(c->coef[(size_t)k * ns + s]))
                fail(CMBL_ERR_ARG, "cmbg_create_table: coefficient %d, %d is not finite", k, s);
        std::copy(c->coef + (size_t)k * ns, c->coef + (size_t)(k + 1) * ns, coef.begin() + (size_t)k * TD_ND);
    }
    g->calc = calc;
    g->n = ns;
    g->form = c->form;
    upload(g->dcoef, coef);
    upload(g->table, tab);
}

static void theorytable_eval(cmbg *g, int M, const double *P, long long ld, double *out, int *fail_flags,
                             hipStream_t stream) {
    cmbt *t = g->calc;
    TheoryTableArgs a{};
    a.b = basis_args(t, M, P, ld);
    a.dcoef = g->dcoef.as<double>();
    a.table = g->table.as<double>();
    a.form = g->form;
    a.tn = g->tn;
    std::copy(g->p, g->p + 8, a.p);
    a.out = out;
    a.fail = fail_flags;
    timed_launch("theory_table_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
        hipExtLaunchKernelGGL(theory_table_kernel, dim3((M + TD_TM - 1) / TD_TM), dim3(TD_THREADS),
                              td_lds_bytes(t->n_in), stream, e0, e1, 0, a);
    });
    HIP_CHECK(hipGetLastError());
}

void theorygauss_eval(cmbg *g, int M, const double *P, long long ld, int num_params, double *out, int *fail_flags,
                      hipStream_t stream) {
    cmbt *t = g->calc;
    if (M <= 0 || M > std::numeric_limits<int>::max() - TD_TM)
        fail(CMBL_ERR_ARG, "cmbg_eval: M must be in 1..%d", std::numeric_limits<int>::max() - TD_TM);
    if (!P || !out) fail(CMBL_ERR_ARG, "cmbg_eval: null buffer");
    if (ld < M) fail(CMBL_ERR_ARG, "cmbg_eval: ld %lld below M %d", ld, M);
    for (int p : t->pidx)
        if (p > num_params) fail(CMBL_ERR_ARG, "cmbg_eval: param_index %d outside 1..%d", p, num_params);
    if (g->form != 0) {
        theorytable_eval(g, M, P, ld, out, fail_flags, stream);
        return;
    }
    TheoryGaussArgs a{};
    a.b = basis_args(t, M, P, ld);
    a.dcoef = g->dcoef.as<double>();
    a.obs = g->obs.as<double>();
    a.invcov = g->invcov.as<double>();
    a.n = g->n;
    a.out = out;
    a.fail = fail_flags;
    timed_launch("theory_gauss_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
        hipExtLaunchKernelGGL(theory_gauss_kernel, dim3((M + TD_TM - 1) / TD_TM), dim3(TD_THREADS),
                              td_lds_bytes(std::max(t->n_in, g->n)), stream, e0, e1, 0, a);
    });
    HIP_CHECK(hipGetLastError());
}

}  // namespace cmamd
