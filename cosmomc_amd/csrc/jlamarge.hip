// The alpha, beta-marginalised JLA likelihood (JLA_marginalize = T,
// source/supernovae_JLA.f90:235-252, 1207-1217).  The reference evaluates
// JLA_alpha_beta_like at every point of a fixed (alpha, beta) grid and
// integrates; none of the V(alpha_g, beta_g) depends on the theory, so they
// are factored and inverted once at open, on the device, and an evaluation is
// G batched quadratic forms over the walkers:
//
//   open   jla_marge_chol_kernel   V_g = L L^T, a workgroup per grid point (a bad pivot drops the point)
//          jla_marge_inv_kernel    M_g = L^-T L^-1 column by column, a thread per column
//          jla_marge_consts_kernel M_g A1, M_g A2 and amarg_E, D, F
//   eval   jla_marge_pro_kernel    estimated_scriptm, amarg_B, amarg_C per (grid point, walker)
//          jla_marge_qf_kernel     partial sums of amarg_A = d^T M_g d on v_mfma_f64_16x16x4_f64
//          jla_marge_chi_kernel    chi^2 / 2 per (grid point, walker)
//          jla_marge_fin_kernel    the minimum and the log-sum per walker
//
// The stages are separate launches in stream order and every sum has a fixed
// order, so a walker's bits do not depend on the batch it is evaluated in.
#include <cmath>

#include "jlamarge.h"

namespace cmamd {

static constexpr int JM_THREADS = 256;   // 4 waves
static constexpr int JM_NB = 16;         // tile edge: one v_mfma_f64_16x16x4_f64 result
static constexpr int JM_MAXW = 1024;     // walkers per launch (workspace_size)
static constexpr int JM_WT = 128;        // walkers of a workgroup of the quadratic form: 8 column tiles
static constexpr int JM_NT = JM_WT / JM_NB;
static constexpr int JM_R = 64;          // rows of M_g of a workgroup: a 16-row tile per wave
static constexpr int JM_KC = 32;         // k of one LDS chunk of the diffmag operand
static constexpr int JM_LD = JM_KC + 2;  // its row stride in doubles (16-byte rows)
static constexpr int JM_SETUP_CHUNK = 32;   // grid points factored at a time: Np^2 doubles of workspace each

typedef double jm_f64x4 __attribute__((ext_vector_type(4)));

void jla_marge_grid(int steps, double width_alpha, double width_beta, double center_alpha, double center_beta,
                    std::vector<double> &alpha, std::vector<double> &beta) {
    alpha.clear();
    beta.clear();
    for (int ai = -steps; ai <= steps; ai++)
        for (int bi = -steps; bi <= steps; bi++)
            if (ai * ai + bi * bi <= steps * steps) {
                alpha.push_back(center_alpha + ai * width_alpha);
                beta.push_back(center_beta + bi * width_beta);
            }
}

// ------------------------------------------------------------ set-up at open

struct JmSetup {
    int n, Np;
    const double *pre, *svar, *cvar, *cms, *cmc, *csc;
    const double *comp[JLA_NCOMP];   // null when absent
    const double *alpha, *beta;      // [points]
};

// V(alpha, beta)[i][j], i >= j, summed as invert_covariance_matrix does (:813-837)
__device__ __forceinline__ double jm_V(const JmSetup &s, double alpha, double beta, int i, int j) {
    const double a2 = alpha * alpha, b2 = beta * beta, ta = 2.0 * alpha, tb = 2.0 * beta, tab = 2.0 * (alpha * beta);
    const size_t ix = (size_t)i * s.n + j;
    double x = 0.0;
    if (s.comp[JLA_MAG]) x = s.comp[JLA_MAG][ix];
    if (s.comp[JLA_STRETCH]) x = x + a2 * s.comp[JLA_STRETCH][ix];
    if (s.comp[JLA_COLOUR]) x = x + b2 * s.comp[JLA_COLOUR][ix];
    if (s.comp[JLA_MAG_STRETCH]) x = x + ta * s.comp[JLA_MAG_STRETCH][ix];
    if (s.comp[JLA_MAG_COLOUR]) x = x - tb * s.comp[JLA_MAG_COLOUR][ix];
    if (s.comp[JLA_STRETCH_COLOUR]) x = x - tab * s.comp[JLA_STRETCH_COLOUR][ix];
    if (i == j) x = x + (s.pre[i] + a2 * s.svar[i] + b2 * s.cvar[i] + ta * s.cms[i] - tb * s.cmc[i] - tab * s.csc[i]);
    return x;
}

// V_g = L L^T by a left-looking column Cholesky, a workgroup per listed grid
// point.  S [Np][Np] of the point receives L in its lower triangle and L^T in
// its upper, so that both substitutions of jla_marge_inv_kernel, and this
// kernel's own update, read along rows.  bad[point] = 1 on a pivot that is not
// positive (DPOTRF status /= 0, a NaN included).
__global__ __launch_bounds__(JM_THREADS) void jla_marge_chol_kernel(JmSetup s, const int *__restrict__ list,
                                                                    double *__restrict__ Sall, int *__restrict__ bad)
{
    const int g = list[blockIdx.x], tid = threadIdx.x, n = s.n;
    const size_t ld = (size_t)s.Np;
    double *S = Sall + (size_t)blockIdx.x * ld * ld;
    const double alpha = s.alpha[g], beta = s.beta[g];
    __shared__ double spiv;
    for (int j = 0; j < n; j++) {
        const double *cj = S + j;
        for (int i = j + tid; i < n; i += JM_THREADS) {
            double v = jm_V(s, alpha, beta, i, j);
            const double *ci = S + i;
            for (int k = 0; k < j; k++) v -= ci[k * ld] * cj[k * ld];
            S[j * ld + i] = v;
            if (i == j) spiv = v;   // thread 0's
        }
        __syncthreads();
        const double piv = spiv;   // one value for the whole workgroup: the exit below is uniform
        if (!(piv > 0.0)) {
            if (tid == 0) bad[g] = 1;
            return;
        }
        const double rt = sqrt(piv);
        for (int i = j + tid; i < n; i += JM_THREADS) {
            const double v = i == j ? rt : S[j * ld + i] / rt;
            S[j * ld + i] = v;
            S[i * ld + j] = v;
        }
        __syncthreads();
    }
}

// M = L^-T L^-1 of a listed grid point that factored, a thread per column c: L y = e_c
// forwards, then L^T m = y backwards, both in the column's own place in M
// [Np][Np] (rows and columns from n on stay zero).  The loops run from the
// workgroup's first column so that they are uniform over it.
__global__ __launch_bounds__(64) void jla_marge_inv_kernel(int n, int Np, const double *__restrict__ Sall,
                                                           const int *__restrict__ list, const int *__restrict__ bad,
                                                           double *__restrict__ Mall)
{
    const size_t ld = (size_t)Np;
    const int g = list[blockIdx.y];
    const double *S = Sall + (size_t)blockIdx.y * ld * ld;
    double *M = Mall + (size_t)g * ld * ld;
    const int c0 = blockIdx.x * 64, c = c0 + (int)threadIdx.x;
    if (c >= n || bad[g]) return;   // a dropped point has no factor
    double *m = M + c;
    for (int i = c0; i < n; i++) {
        const double *row = S + (size_t)i * ld;
        double v = i == c ? 1.0 : 0.0;
        for (int k = c0; k < i; k++) v -= row[k] * m[k * ld];
        m[i * ld] = v / row[i];
    }
    for (int i = n - 1; i >= 0; i--) {
        const double *row = S + (size_t)i * ld;
        double v = i >= c0 ? m[i * ld] : 0.0;
        for (int k = i + 1; k < n; k++) v -= row[k] * m[k * ld];
        m[i * ld] = v / row[i];
    }
}

// fixed-order sum over the workgroup; every thread gets it
__device__ __forceinline__ double jm_block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = JM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// u1 = M A1 (or M 1), u2 = M A2 and amarg_E = A1^T u1, amarg_D = A2^T u1,
// amarg_F = A2^T u2 of a kept grid point (:1107-1131): out [kept][3]
__global__ __launch_bounds__(JM_THREADS) void jla_marge_consts_kernel(int n, int Np, const double *__restrict__ Mall,
                                                                      const double *__restrict__ one,
                                                                      const double *__restrict__ A2,
                                                                      double *__restrict__ u1, double *__restrict__ u2,
                                                                      double *__restrict__ out)
{
    __shared__ double red[JM_THREADS];
    const int g = blockIdx.x, tid = threadIdx.x;
    const double *M = Mall + (size_t)g * Np * Np;
    double e = 0.0, dd = 0.0, f = 0.0;
    for (int i = tid; i < Np; i += JM_THREADS) {
        double a = 0.0, b = 0.0;
        if (i < n) {
            const double *row = M + (size_t)i * Np;
            for (int j = 0; j < n; j++) {
                a += row[j] * one[j];
                b += row[j] * A2[j];
            }
            e += one[i] * a;
            dd += A2[i] * a;
            f += A2[i] * b;
        }
        u1[(size_t)g * Np + i] = a;
        u2[(size_t)g * Np + i] = b;
    }
    e = jm_block_sum(e, red);
    dd = jm_block_sum(dd, red);
    f = jm_block_sum(f, red);
    if (tid == 0) out[3 * g] = e, out[3 * g + 1] = dd, out[3 * g + 2] = f;
}

// ------------------------------------------------------------ evaluation

struct JmDev {
    int n, Np, G, RB, diag, two;
    const double *mag, *stretch, *colour;   // [n]
    const double *alpha, *beta, *sumiv;     // [G]
    const double *iv, *u1, *u2;             // [G][Np], zero from n on
    const double *M;                        // [G][Np][Np]; null with diag_errors
    const double *cst;                      // [G][6]: E, D, F, tempG, log(E / 2 pi), log(tempG / 2 pi)
    double width_alpha, width_beta;
};

// one launch's walkers and its tables in the workspace, each [G][ld] but part [G][RB][ld]
struct JmBatch {
    const double *dl;
    long long ld_walker;
    int W, w0, ld;
    const int *wcount;   // live walkers of the whole batch [0, *wcount), or null: all
    double *scr, *B, *C, *L, *part;
    double *out;
};

__device__ __forceinline__ int jm_live(const JmBatch &b) {
    if (!b.wcount) return b.W;
    return max(0, min(b.W, *b.wcount - b.w0));
}

// fixed-order sum over the wave; every lane gets it
__device__ __forceinline__ double jm_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// A wave per (grid point, walker): estimated_scriptm (:1062-1063), then with
// diffmag (:1064-1065) amarg_B = (M A1)^T diffmag, amarg_C = (M A2)^T diffmag
// and, with diag_errors, amarg_A = SUM(invvars * diffmag^2).
__global__ __launch_bounds__(JM_THREADS) void jla_marge_pro_kernel(JmDev d, JmBatch b)
{
    const int lane = threadIdx.x & 63, w = 4 * blockIdx.x + (threadIdx.x >> 6), g = blockIdx.y, n = d.n;
    if (w >= jm_live(b)) return;
    const double *mu = b.dl + (size_t)w * b.ld_walker;
    const double *iv = d.iv + (size_t)g * d.Np, *u1 = d.u1 + (size_t)g * d.Np, *u2 = d.u2 + (size_t)g * d.Np;
    const double alpha = d.alpha[g], beta = d.beta[g];
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += (d.mag[i] - mu[i]) * iv[i];
    const double scriptm = jm_wave_sum(s) / d.sumiv[g];
    double pa = 0.0, pb = 0.0, pc = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double x = d.mag[i] - mu[i] + alpha * d.stretch[i] - beta * d.colour[i] - scriptm;
        pb += u1[i] * x;
        pc += u2[i] * x;
        if (d.diag) pa += iv[i] * (x * x);
    }
    pb = jm_wave_sum(pb);
    pc = jm_wave_sum(pc);
    if (d.diag) pa = jm_wave_sum(pa);
    if (lane == 0) {
        const size_t o = (size_t)g * b.ld + w;
        b.scr[o] = scriptm;
        b.B[o] = pb;
        b.C[o] = pc;
        if (d.diag) b.part[o] = pa;
    }
}

__device__ __forceinline__ void jm_load4(const double *p, double (&x)[4]) {
    const double2 lo = *reinterpret_cast<const double2 *>(p);
    const double2 hi = *reinterpret_cast<const double2 *>(p + 2);
    x[0] = lo.x, x[1] = lo.y, x[2] = hi.x, x[3] = hi.y;
}

// A thread's share of one chunk of the diffmag operand: k = k0 + (tid & 31) of
// the walkers (tid >> 5) + 8 p of the workgroup's tile.
struct JmFetch {
    double mu[JM_WT / 8], mag, stretch, colour;
};
__device__ __forceinline__ void jm_fetch(const JmDev &d, const double *__restrict__ mu0, long long ldw, int nlive,
                                         int nt, int k0, JmFetch &f) {
    const int k = k0 + (threadIdx.x & 31), wq = threadIdx.x >> 5;
    const bool kin = k < d.n;
    f.mag = kin ? d.mag[k] : 0.0;
    f.stretch = kin ? d.stretch[k] : 0.0;
    f.colour = kin ? d.colour[k] : 0.0;
#pragma unroll
    for (int p = 0; p < JM_WT / 8; p++) {
        const int wl = wq + 8 * p;
        f.mu[p] = (kin && wl < nlive && wl < JM_NB * nt) ? mu0[(size_t)wl * ldw + k] : 0.0;
    }
}
// diffmag (:1064-1065) of the fetched entries into the LDS chunk, zero beyond
// the supernovae and the live walkers
__device__ __forceinline__ void jm_store(const JmDev &d, double alpha, double beta, const double *scr, int nlive,
                                         int nt, int k0, const JmFetch &f, double (*Dl)[JM_LD]) {
    const int kk = threadIdx.x & 31, wq = threadIdx.x >> 5;
    const bool kin = k0 + kk < d.n;
#pragma unroll
    for (int p = 0; p < JM_WT / 8; p++) {
        const int wl = wq + 8 * p;
        if (wl >= JM_NB * nt) continue;
        Dl[wl][kk] = (kin && wl < nlive) ? f.mag - f.mu[p] + alpha * f.stretch - beta * f.colour - scr[wl] : 0.0;
    }
}

// Partial sums of amarg_A = diffmag^T M_g diffmag (:1098-1100).  A workgroup
// takes (grid point g, 64 rows of M_g, 128 walkers): the diffmag operand of its
// walkers is formed chunk by chunk in LDS from their distance moduli, each wave
// multiplies its 16 rows of M_g (read once, from global memory) into all 8
// walker tiles, Q = M_g[rows, :] D, and the epilogue contracts Q with the same
// rows of D.  part[g][row block][walker] receives the four waves' sum.
// Workgroups that share rows of M_g are neighbours on one XCD (the hardware
// deals consecutive workgroups to the 8 XCDs in turn), so its L2 serves all
// but the first of them.
__global__ __launch_bounds__(JM_THREADS, 2) void jla_marge_qf_kernel(JmDev d, JmBatch b, int nwt, int total)
{
    __shared__ __attribute__((aligned(16))) double Dl[JM_WT][JM_LD];
    __shared__ double scr[JM_WT];
    __shared__ double red[4][JM_WT];
    const int per = gridDim.x / 8;
    const int id = (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);
    if (id >= total) return;
    const int wt = id % nwt, rb = (id / nwt) % d.RB, g = id / (nwt * d.RB);
    const int w_first = JM_WT * wt, nlive = min(JM_WT, jm_live(b) - w_first);
    if (nlive <= 0) return;
    const int nt = (nlive + JM_NB - 1) / JM_NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Np = d.Np;
    const double alpha = d.alpha[g], beta = d.beta[g];
    const double *mu0 = b.dl + (size_t)w_first * b.ld_walker;
    if (tid < JM_WT) scr[tid] = tid < nlive ? b.scr[(size_t)g * b.ld + w_first + tid] : 0.0;
    const int row0 = JM_R * rb + JM_NB * wave;     // the wave's rows of M_g
    const bool rows = row0 < Np;
    const double *pa = d.M + (size_t)g * Np * Np + (size_t)(row0 + (lane & 15)) * Np + 4 * (lane >> 4);
    const int lcol = lane & 15, lk = 4 * (lane >> 4);

    jm_f64x4 acc[JM_NT];
#pragma unroll
    for (int t = 0; t < JM_NT; t++) acc[t] = jm_f64x4{0.0, 0.0, 0.0, 0.0};
    JmFetch f;
    jm_fetch(d, mu0, b.ld_walker, nlive, nt, 0, f);
    const int nchunk = (Np + JM_KC - 1) / JM_KC;
    for (int c = 0; c < nchunk; c++) {
        const int k0 = JM_KC * c;
        double a[2][4];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (rows && k0 + 16 * u < Np) jm_load4(pa + k0 + 16 * u, a[u]);
            else a[u][0] = a[u][1] = a[u][2] = a[u][3] = 0.0;
        }
        __syncthreads();   // the last chunk has been read (and scr is there)
        jm_store(d, alpha, beta, scr, nlive, nt, k0, f, Dl);
        __syncthreads();
        if (c + 1 < nchunk) jm_fetch(d, mu0, b.ld_walker, nlive, nt, k0 + JM_KC, f);
        if (!rows) continue;
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (k0 + 16 * u >= Np) continue;
#pragma unroll
            for (int t = 0; t < JM_NT; t++) {
                if (t >= nt) continue;
                double x[4];
                jm_load4(&Dl[JM_NB * t + lcol][16 * u + lk], x);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][q], x[q], acc[t], 0, 0, 0);
            }
        }
    }
    // sum over the wave's rows of Q[row][w] D[row][w]: the rows' chunk of D again,
    // one half of the row block at a time.  Result lane layout: column lane & 15,
    // rows (lane >> 4) + 4 r.
    double p[JM_NT];
#pragma unroll
    for (int t = 0; t < JM_NT; t++) p[t] = 0.0;
    for (int h = 0; h < 2; h++) {
        const int k0 = JM_R * rb + JM_KC * h;
        __syncthreads();
        jm_fetch(d, mu0, b.ld_walker, nlive, nt, k0, f);
        jm_store(d, alpha, beta, scr, nlive, nt, k0, f, Dl);
        __syncthreads();
        if (!rows || (wave >> 1) != h) continue;
#pragma unroll
        for (int t = 0; t < JM_NT; t++) {
            if (t >= nt) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) p[t] += acc[t][r] * Dl[JM_NB * t + lcol][16 * (wave & 1) + (lane >> 4) + 4 * r];
        }
    }
#pragma unroll
    for (int t = 0; t < JM_NT; t++) {
        p[t] += __shfl_xor(p[t], 16, 64);
        p[t] += __shfl_xor(p[t], 32, 64);
        if (lane < JM_NB) red[wave][JM_NB * t + lane] = p[t];
    }
    __syncthreads();
    if (tid < nlive)
        b.part[((size_t)g * d.RB + rb) * b.ld + w_first + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// A thread per (grid point, walker): amarg_A from its partial sums in row-block
// order and L_g = chi^2 / 2 (:1135-1148).
__global__ __launch_bounds__(JM_THREADS) void jla_marge_chi_kernel(JmDev d, JmBatch b)
{
    const int w = blockIdx.x * JM_THREADS + threadIdx.x, g = blockIdx.y;
    if (w >= jm_live(b)) return;
    const int nrb = d.diag ? 1 : d.RB;
    const size_t o = (size_t)g * b.ld + w;
    double A = 0.0;
    for (int r = 0; r < nrb; r++) A += b.part[((size_t)g * nrb + r) * b.ld + w];
    const double B = b.B[o], C = b.C[o];
    const double *k = d.cst + 6 * g;
    const double E = k[0], D = k[1], F = k[2], tempG = k[3];
    double chisq;
    if (d.two)
        chisq = A + k[4] + k[5] - C * C / tempG - B * B * F / (E * tempG) + 2.0 * B * C * D / (E * tempG);
    else
        chisq = A + k[4] - B * B / E;
    b.L[o] = chisq / 2;
}

// A thread per walker: jla_LnLike's integral (:1215-1217) over the kept points,
// the minimum and then the sum in grid order.  A value that is not finite gives
// CMBL_LOGZERO.
__global__ __launch_bounds__(64) void jla_marge_fin_kernel(JmDev d, JmBatch b)
{
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= jm_live(b)) return;
    double best = INFINITY;
    for (int g = 0; g < d.G; g++) {
        const double L = b.L[(size_t)g * b.ld + w];
        if (L < best) best = L;
    }
    double sum = 0.0;
    for (int g = 0; g < d.G; g++) sum += exp(-b.L[(size_t)g * b.ld + w] + best);
    const double v = best - log(sum * d.width_alpha * d.width_beta);
    b.out[w] = isfinite(v) ? v : CMBL_LOGZERO;
}

// ------------------------------------------------------------ likelihood

static double jm_option(const Ini &ini, const char *key, double def) {
    const std::string v = ini.str(key);
    if (v.empty()) return def;
    try {
        return parse_fortran_double(v);
    } catch (const std::exception &) {
        fail(CMBL_ERR_FORMAT, "JLA_MARGE: bad number %s = %s", key, v.c_str());
    }
}

struct JlaMargeLike : Like {
    JlaData h;
    JmDev dev{};
    int n_points = 0;
    size_t grid_bytes = 0;
    DevBuf b_mag, b_stretch, b_colour, b_alpha, b_beta, b_sumiv, b_iv, b_u1, b_u2, b_M, b_cst;

    explicit JlaMargeLike(const Ini &ini) {
        int steps = 7;
        const std::string sv = ini.str("JLA_marge_steps");
        if (!sv.empty()) {
            try {
                steps = std::stoi(sv);
            } catch (const std::exception &) {
                fail(CMBL_ERR_FORMAT, "JLA_MARGE: bad integer JLA_marge_steps = %s", sv.c_str());
            }
        }
        const double wa = jm_option(ini, "JLA_step_width_alpha", 0.003), wb = jm_option(ini, "JLA_step_width_beta", 0.04);
        if (steps < 0 || steps > JLA_MARGE_MAX_STEPS)
            fail(CMBL_ERR_ARG, "JLA_MARGE: JLA_marge_steps = %d outside 0..%d", steps, JLA_MARGE_MAX_STEPS);
        if (!(wa > 0.0) || !(wb > 0.0))
            fail(CMBL_ERR_ARG, "JLA_MARGE: JLA_step_width_alpha = %g and JLA_step_width_beta = %g must be positive", wa, wb);
        // not keys of the reference, whose centres are constants (:119-120)
        const double ca = jm_option(ini, "JLA_alpha_center", jla_marge_alpha_center());
        const double cb = jm_option(ini, "JLA_beta_center", jla_marge_beta_center());
        h = load_jla(ini, true);

        name = "JLA";
        tag = "JLA_MARGE";
        n_nuis = 0;        // JLALikelihood_Add loads no JLA.paramnames (:236-255)
        speed = 0;
        theory_len = h.nsn;
        const int n = h.nsn, Np = (n + JM_NB - 1) / JM_NB * JM_NB;
        std::vector<double> alpha, beta;
        jla_marge_grid(steps, wa, wb, ca, cb, alpha, beta);
        n_points = (int)alpha.size();

        std::vector<int> kept;
        std::vector<double> EDF;   // [kept][3]
        if (h.diag_errors) {
            for (int g = 0; g < n_points; g++) kept.push_back(g);
        } else {
            invert_on_device(alpha, beta, Np, kept, EDF);
        }
        const int G = (int)kept.size();
        if (G == 0)
            fail(CMBL_ERR_FORMAT, "JLA_MARGE: V(alpha, beta) is not positive definite at any of the %d grid points",
                 n_points);

        // per kept point: invvars (:1056-1060) and its sum, and the constants of chi^2
        std::vector<double> ka(G), kb(G), sumiv(G), iv((size_t)G * Np, 0.0), cst((size_t)G * 6, 0.0);
        std::vector<double> u1, u2;
        if (h.diag_errors) u1.assign((size_t)G * Np, 0.0), u2.assign((size_t)G * Np, 0.0);
        const double inv_twopi = 1.0 / (2.0 * 3.14159265358979323846);
        for (int q = 0; q < G; q++) {
            const double a = ka[q] = alpha[kept[q]], bt = kb[q] = beta[kept[q]];
            const double a2 = a * a, b2 = bt * bt, ta = 2.0 * a, tb = 2.0 * bt, tab = 2.0 * (a * bt);
            double s = 0.0, E = 0.0, F = 0.0;
            for (int i = 0; i < n; i++) {
                const double dv = h.pre_vars[i] + a2 * h.stretch_var[i] + b2 * h.colour_var[i] + ta * h.cov_ms[i] -
                                  tb * h.cov_mc[i] - tab * h.cov_sc[i];
                const double v = 1.0 / dv;
                iv[(size_t)q * Np + i] = v;
                s += v;
                if (h.diag_errors) {   // V^-1 = diag(invvars) (:1067-1078)
                    u1[(size_t)q * Np + i] = v * h.one[i];
                    u2[(size_t)q * Np + i] = v * h.A2[i];
                    E += v * h.one[i];
                    F += v * h.A2[i];
                }
            }
            sumiv[q] = s;
            double *k = &cst[(size_t)q * 6];
            if (h.diag_errors) k[0] = E, k[1] = 0.0, k[2] = F;
            else k[0] = EDF[3 * q], k[1] = EDF[3 * q + 1], k[2] = EDF[3 * q + 2];
            k[3] = 1.0;
            if (h.twoscriptmfit) {
                k[3] = k[2] - k[1] * k[1] / k[0];
                if (!(k[3] > 0.0))   // the reference stops ("Twoscriptm assumption violation")
                    fail(CMBL_ERR_FORMAT,
                         "JLA_MARGE: twoscriptm assumption violation (tempG = %g) at grid point %d, alpha = %g beta = %g",
                         k[3], kept[q] + 1, a, bt);
            }
            k[4] = std::log(k[0] * inv_twopi);
            k[5] = std::log(k[3] * inv_twopi);
        }

        dev.n = n, dev.Np = Np, dev.G = G, dev.RB = (Np + JM_R - 1) / JM_R;
        dev.diag = h.diag_errors, dev.two = h.twoscriptmfit;
        dev.width_alpha = wa, dev.width_beta = wb;
        dev.mag = upload(b_mag, h.mag);
        dev.stretch = upload(b_stretch, h.stretch);
        dev.colour = upload(b_colour, h.colour);
        dev.alpha = upload(b_alpha, ka);
        dev.beta = upload(b_beta, kb);
        dev.sumiv = upload(b_sumiv, sumiv);
        dev.iv = upload(b_iv, iv);
        dev.cst = upload(b_cst, cst);
        if (h.diag_errors) {
            dev.u1 = upload(b_u1, u1);
            dev.u2 = upload(b_u2, u2);
            dev.M = nullptr;
        } else {
            dev.u1 = b_u1.as<double>();
            dev.u2 = b_u2.as<double>();
            dev.M = b_M.as<double>();
        }
        for (int c = 0; c < JLA_NCOMP; c++) std::vector<double>().swap(h.comp[c]);
    }

    // The kept points and, in b_M, b_u1 and b_u2, their V^-1, V^-1 A1 and V^-1 A2.
    // Every point is factored and, unless a pivot drops it, inverted into a
    // place of its own; if points were dropped (rare), the kept inverses are then
    // moved together so that no matrix is stored for a dropped one.
    void invert_on_device(const std::vector<double> &alpha, const std::vector<double> &beta, int Np,
                          std::vector<int> &kept, std::vector<double> &EDF) {
        const int n = h.nsn, P = (int)alpha.size();
        const size_t mat = (size_t)Np * Np * 8;
        DevBuf t_tab[6], t_comp[JLA_NCOMP], t_alpha, t_beta, t_one, t_A2, t_S, t_list, t_bad, t_out;
        JmSetup s{};
        s.n = n, s.Np = Np;
        const std::vector<double> *tab[6] = {&h.pre_vars, &h.stretch_var, &h.colour_var, &h.cov_ms, &h.cov_mc, &h.cov_sc};
        const double **dst[6] = {&s.pre, &s.svar, &s.cvar, &s.cms, &s.cmc, &s.csc};
        for (int i = 0; i < 6; i++) *dst[i] = upload(t_tab[i], *tab[i]);
        for (int c = 0; c < JLA_NCOMP; c++) s.comp[c] = h.has[c] ? upload(t_comp[c], h.comp[c]) : nullptr;
        s.alpha = upload(t_alpha, alpha);
        s.beta = upload(t_beta, beta);
        const int chunk = std::min(P, JM_SETUP_CHUNK);
        t_S.alloc((size_t)chunk * mat);
        t_bad.alloc((size_t)P * sizeof(int));
        b_M.alloc((size_t)P * mat);
        std::vector<int> list(P);
        for (int g = 0; g < P; g++) list[g] = g;
        upload(t_list, list);
        for (int first = 0; first < P; first += chunk) {
            const int count = std::min(chunk, P - first);
            hipLaunchKernelGGL(jla_marge_chol_kernel, dim3(count), dim3(JM_THREADS), 0, 0, s, t_list.as<int>() + first,
                               t_S.as<double>(), t_bad.as<int>());
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(jla_marge_inv_kernel, dim3((n + 63) / 64, count), dim3(64), 0, 0, n, Np,
                               t_S.as<double>(), t_list.as<int>() + first, t_bad.as<int>(), b_M.as<double>());
            HIP_CHECK(hipGetLastError());
        }
        std::vector<int> bad(P);
        HIP_CHECK(hipMemcpy(bad.data(), t_bad.p, (size_t)P * sizeof(int), hipMemcpyDeviceToHost));
        for (int g = 0; g < P; g++)
            if (!bad[g]) kept.push_back(g);
        const int G = (int)kept.size();
        if (G == 0) return;
        grid_bytes = (size_t)G * mat;
        if (G < P) {
            DevBuf packed(grid_bytes);
            for (int q = 0; q < G; q++)
                HIP_CHECK(hipMemcpy(packed.as<char>() + q * mat, b_M.as<char>() + kept[q] * mat, mat,
                                    hipMemcpyDeviceToDevice));
            std::swap(b_M.p, packed.p);
            std::swap(b_M.bytes, packed.bytes);
        }
        b_u1.alloc((size_t)G * Np * 8);
        b_u2.alloc((size_t)G * Np * 8);
        t_out.alloc((size_t)G * 3 * 8);
        hipLaunchKernelGGL(jla_marge_consts_kernel, dim3(G), dim3(JM_THREADS), 0, 0, n, Np, b_M.as<double>(),
                           upload(t_one, h.one), upload(t_A2, h.A2), b_u1.as<double>(), b_u2.as<double>(),
                           t_out.as<double>());
        HIP_CHECK(hipGetLastError());
        EDF.resize((size_t)G * 3);
        HIP_CHECK(hipMemcpy(EDF.data(), t_out.p, EDF.size() * 8, hipMemcpyDeviceToHost));
    }

    // doubles per walker of a launch: scriptm, B, C and L per point, and the partials of A
    size_t ws_rows() const { return (size_t)dev.G * (4 + (dev.diag ? 1 : dev.RB)); }
    size_t workspace_size(int W) const override { return ws_rows() * 8 * (size_t)std::max(0, std::min(W, JM_MAXW)); }

    void run(int W, const double *dl, long long ld_walker, double *out, void *ws, hipStream_t stream, const int *wcount) {
        if (W <= 0) return;
        if (ld_walker != 0 && ld_walker < h.nsn)
            fail(CMBL_ERR_ARG, "JLA_MARGE: ld_walker %lld < the %d distance moduli of a walker", ld_walker, h.nsn);
        if (!ws) {
            own_ws.grow(workspace_size(W));
            ws = own_ws.p;
        }
        // batches beyond the workspace's walkers run in chunks, one after another in stream order
        for (int w0 = 0; w0 < W; w0 += JM_MAXW) {
            const int Wc = std::min(JM_MAXW, W - w0);
            const size_t gl = (size_t)dev.G * Wc;
            JmBatch b{};
            b.dl = dl + (size_t)w0 * ld_walker, b.ld_walker = ld_walker;
            b.W = Wc, b.w0 = w0, b.ld = Wc, b.wcount = wcount;
            b.scr = static_cast<double *>(ws), b.B = b.scr + gl, b.C = b.B + gl, b.L = b.C + gl, b.part = b.L + gl;
            b.out = out + w0;
            timed_launch("jla_marge_pro_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(jla_marge_pro_kernel, dim3((Wc + 3) / 4, dev.G), dim3(JM_THREADS), 0, stream, e0,
                                      e1, 0, dev, b);
            });
            HIP_CHECK(hipGetLastError());
            if (!dev.diag) {
                const int nwt = (Wc + JM_WT - 1) / JM_WT, total = dev.G * dev.RB * nwt;
                timed_launch("jla_marge_qf_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                    hipExtLaunchKernelGGL(jla_marge_qf_kernel, dim3((total + 7) / 8 * 8), dim3(JM_THREADS), 0, stream,
                                          e0, e1, 0, dev, b, nwt, total);
                });
                HIP_CHECK(hipGetLastError());
            }
            timed_launch("jla_marge_chi_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(jla_marge_chi_kernel, dim3((Wc + JM_THREADS - 1) / JM_THREADS, dev.G),
                                      dim3(JM_THREADS), 0, stream, e0, e1, 0, dev, b);
            });
            HIP_CHECK(hipGetLastError());
            timed_launch("jla_marge_fin_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(jla_marge_fin_kernel, dim3((Wc + 63) / 64), dim3(64), 0, stream, e0, e1, 0, dev,
                                      b);
            });
            HIP_CHECK(hipGetLastError());
        }
    }

    void loglike_batch(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                       long long ld_nuis, double *out, void *ws, hipStream_t stream) override {
        (void)ld_field, (void)nuis, (void)ld_nuis;   // one field: the distance moduli; no nuisance parameters
        run(W, dl, ld_walker, out, ws, stream, nullptr);
    }
    bool sparse_capable() const override { return true; }
    void loglike_batch_sparse(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                              long long ld_nuis, double *out, void *ws, hipStream_t stream,
                              const int *wcount) override {
        (void)ld_field, (void)nuis, (void)ld_nuis;
        run(W, dl, ld_walker, out, ws, stream, wcount);
    }
};

std::unique_ptr<Like> make_jla_marge(const Ini &ini) { return std::unique_ptr<Like>(new JlaMargeLike(ini)); }

bool jla_marge_info(const Like *like, int *n_grid, int *n_points, size_t *grid_bytes) {
    const JlaMargeLike *m = dynamic_cast<const JlaMargeLike *>(like);
    if (!m) return false;
    if (n_grid) *n_grid = m->dev.G;
    if (n_points) *n_points = m->n_points;
    if (grid_bytes) *grid_bytes = m->grid_bytes;
    return true;
}

}  // namespace cmamd
