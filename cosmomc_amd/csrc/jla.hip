// JLA supernova likelihood (source/supernovae_JLA.f90): the dataset loader and
// the batched f64 kernel of its fast step.  Per walker, from (alpha, beta) and
// the distance moduli: the diagonal terms and estimated_scriptm (:1056-1065),
// V(alpha, beta) = L L^T by a blocked left-looking Cholesky whose block columns
// are formed from the component matrices as they are first needed (:813-837),
// the forward solve of [diffmag, A1-or-ones, A2] carried as extra rows of the
// factorisation, their Gram matrix and the marginalised chi^2 (:1135-1148).
// The reference's explicit inverse (DPOTRI) is not formed: amarg_* are the
// entries of Y^T Y with Y = L^-1 [diffmag, A1, A2].
#include <cmath>
#include <fstream>
#include <sstream>

#include "jla.h"

namespace cmamd {

// ------------------------------------------------------------ loader

static bool jla_logical(const Ini &ini, const std::string &key, bool def) {
    std::string v = ini.str(key);
    if (v.empty()) return def;
    const char ch = (char)std::toupper(v[0] == '.' && v.size() > 1 ? v[1] : v[0]);
    if (ch == 'T' || ch == '1' || ch == 'Y') return true;
    if (ch == 'F' || ch == '0' || ch == 'N') return false;
    fail(CMBL_ERR_FORMAT, "%s: bad logical %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
}

static double jla_double(const Ini &ini, const std::string &key, double def) {
    std::string v = ini.str(key);
    return v.empty() ? def : parse_fortran_double(v);
}

// The reference's plain OPEN takes the name as written (relative to the working
// directory); a dataset kept beside its files is found relative to the dataset.
static std::string jla_path(const Ini &ini, const std::string &value) {
    if (value.empty() || value[0] == '/' || file_exists(value)) return value;
    const std::string cand = dirname_of(ini.filename()) + value;
    return file_exists(cand) ? cand : value;
}

static double sq_single(double x) {   // REAL :: dz, dm, ds, dc, dt squared before promotion (:378, 475-479)
    const float f = (float)x;
    const float s = f * f;
    return (double)s;
}

// read_cov_matrix (:311-357): n on the first line, then n * n numbers in any line layout
static std::vector<double> jla_read_cov(const std::string &path, int n) {
    std::ifstream f(path);
    if (!f) fail(CMBL_ERR_IO, "JLA: failed to open cov matrix file %s", path.c_str());
    std::string line;
    if (!std::getline(f, line)) fail(CMBL_ERR_FORMAT, "JLA: matrix file %s is the wrong size", path.c_str());
    int nfile = 0;
    try {
        nfile = std::stoi(line);
    } catch (const std::exception &) {
        fail(CMBL_ERR_FORMAT, "JLA: matrix file %s: no size on its first line", path.c_str());
    }
    if (nfile != n) fail(CMBL_ERR_FORMAT, "JLA: for file %s expected size %d got %d", path.c_str(), n, nfile);
    std::vector<double> file((size_t)n * n);
    size_t got = 0;
    std::string tok;
    while (f >> tok) {
        if (got == file.size()) fail(CMBL_ERR_FORMAT, "JLA: matrix file %s is the wrong size (expected %d by %d)",
                                     path.c_str(), n, n);
        file[got++] = parse_fortran_double(tok);
    }
    if (got != file.size())
        fail(CMBL_ERR_FORMAT, "JLA: matrix file %s is the wrong size (expected %d by %d)", path.c_str(), n, n);
    // DPOTRF with uplo = 'U' reads mat(j, k), j <= k, only
    std::vector<double> m((size_t)n * n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) m[(size_t)i * n + j] = file[(size_t)std::min(i, j) * n + std::max(i, j)];
    return m;
}

JlaData load_jla(const Ini &ini, bool marginalised) {
    JlaData d;
    if (!marginalised && jla_logical(ini, "JLA_marginalize", false))
        fail(CMBL_ERR_UNSUPPORTED, "JLA: JLA_marginalize = T is not supported under this tag (alpha_JLA, beta_JLA are "
                                   "sampled); open the dataset with the tag JLA_MARGE");
    // has_absdist is read as a logical from the key absdist_file, and the file
    // name it would open is never assigned (:621, 654)
    if (jla_logical(ini, "absdist_file", false))
        fail(CMBL_ERR_UNSUPPORTED, "JLA: absdist_file is not supported (the reference never assigns its file name)");
    d.name = ini.str("name");
    const double pecz = jla_double(ini, "pecz", 0.001);
    d.twoscriptmfit = jla_logical(ini, "twoscriptmfit", false);
    const double scriptmcut = jla_double(ini, "scriptmcut", 10.0);
    const double idisp_zero = jla_double(ini, "intrinsicdisp", 0.13);
    double intrinsicsq[10];
    for (int i = 0; i < 10; i++) {
        const double v = jla_double(ini, "intrinsicdisp" + std::to_string(i), idisp_zero);
        intrinsicsq[i] = v * v;
    }

    const std::string data_file = jla_path(ini, ini.str("data_file", "data/jla_lcparams.txt"));
    std::ifstream f(data_file);
    if (!f) fail(CMBL_ERR_IO, "JLA: error reading %s", data_file.c_str());
    std::vector<int> dataset;
    std::vector<double> mag_var;
    std::string line;
    while (std::getline(f, line)) {
        const size_t p = line.find_first_not_of(" \t\r");
        if (p == std::string::npos || line[p] == '#') continue;
        const std::vector<std::string> t = split_ws(line);
        // name zcmb zhel dz mb dmb x1 dx1 color dcolor 3rdvar d3rdvar cov_m_s cov_m_c cov_s_c set
        if (t.size() != 16)
            fail(CMBL_ERR_UNSUPPORTED,
                 "JLA: %s has a row of %zu columns; only the 16-column layout (third variable and set) is read",
                 data_file.c_str(), t.size());
        double v[16] = {0};
        try {
            for (int c = 1; c < 15; c++) v[c] = parse_fortran_double(t[c]);
            v[15] = std::stoi(t[15]);
        } catch (const std::exception &) {
            fail(CMBL_ERR_FORMAT, "JLA: %s: bad number in row %zu", data_file.c_str(), dataset.size() + 1);
        }
        d.zcmb.push_back(v[1]);
        d.zhel.push_back(v[2]);
        d.mag.push_back(v[4]);
        mag_var.push_back(sq_single(v[5]));
        d.stretch.push_back(v[6]);
        d.stretch_var.push_back(sq_single(v[7]));
        d.colour.push_back(v[8]);
        d.colour_var.push_back(sq_single(v[9]));
        d.thirdvar.push_back(v[10]);
        d.cov_ms.push_back(v[12]);
        d.cov_mc.push_back(v[13]);
        d.cov_sc.push_back(v[14]);
        const int set = (int)v[15];
        if (set < 0 || set > 9)
            fail(CMBL_ERR_FORMAT, "JLA: %s: invalid dataset number %d (0..9 allowed)", data_file.c_str(), set);
        dataset.push_back(set);
    }
    const int n = d.nsn = (int)dataset.size();
    if (n < 1) fail(CMBL_ERR_FORMAT, "JLA: no SN read from %s", data_file.c_str());

    static const char *comp_key[JLA_NCOMP] = {"mag", "stretch", "colour", "mag_stretch", "mag_colour", "stretch_colour"};
    d.diag_errors = true;
    for (int c = 0; c < JLA_NCOMP; c++) {
        d.has[c] = jla_logical(ini, std::string("has_") + comp_key[c] + "_covmat", false);
        if (!d.has[c]) continue;
        d.diag_errors = false;
        d.comp[c] = jla_read_cov(jla_path(ini, ini.str_required(std::string(comp_key[c]) + "_covmat_file")), n);
    }

    // jla_prep: zfacsq = 25.0/(LOG(10.0))**2 is a single-precision constant (:882)
    const float ln10 = (float)std::log(10.0);
    const float zfac_f = 25.0f / (ln10 * ln10);
    const double zfacsq = (double)zfac_f;
    d.pre_vars.resize(n);
    for (int i = 0; i < n; i++) {
        const double z = d.zcmb[i];
        const double r = (1.0 + z) / (z * (1 + 0.5 * z));
        d.pre_vars[i] = mag_var[i] + intrinsicsq[dataset[i]];
        d.pre_vars[i] = d.pre_vars[i] + zfacsq * (pecz * pecz) * (r * r);
    }
    d.one.assign(n, 1.0);
    d.A2.assign(n, 0.0);
    if (d.twoscriptmfit) {
        bool has_A2 = false;
        for (int i = 0; i < n; i++)
            if (!(d.thirdvar[i] <= scriptmcut)) has_A2 = true;
        // has_A1 starts true in the reference, so only an empty second set switches the fit off (:924-957)
        if (!has_A2) d.twoscriptmfit = false;
        else
            for (int i = 0; i < n; i++) {
                const bool first = d.thirdvar[i] <= scriptmcut;
                d.one[i] = first ? 1.0 : 0.0;
                d.A2[i] = first ? 0.0 : 1.0;
            }
    }
    return d;
}

// ------------------------------------------------------------ kernel

static constexpr int JLA_THREADS = 256;   // 4 waves
static constexpr int JLA_NB = 16;         // tile edge: one v_mfma_f64_16x16x4_f64 result
static constexpr int JLA_MAXW = 1024;     // walkers per launch (workspace_size)

typedef double jla_f64x4 __attribute__((ext_vector_type(4)));

struct JlaDev {
    int n, Np, two, diag;
    const double *mag, *stretch, *colour, *pre, *svar, *cvar, *cms, *cmc, *csc, *one, *A2;
    const double *comp[JLA_NCOMP];   // null when absent
};

struct JlaCoef {
    double a2, b2, ta, tb, tab;   // alpha^2, beta^2, 2 alpha, 2 beta, 2 alpha beta
};

// doubles of one walker's workspace: L [Np + 16][Np] (the last 16 rows carry the
// right-hand sides), dvar [Np], diffmag [Np]
__host__ __device__ inline size_t jla_ws_doubles(int Np) { return (size_t)(Np + JLA_NB) * Np + 2 * (size_t)Np; }

// fixed-order sum over the workgroup; every thread gets it
__device__ __forceinline__ double jla_block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = JLA_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// One 16 x 16 tile of the augmented matrix before its update: row tile I < T of
// V(alpha, beta) (lower triangle; identity where padded), or the right-hand
// sides (I == T).  Lane layout of the MFMA result: column lane & 15, rows
// (lane >> 4) + 4 r.
__device__ __forceinline__ void jla_tile(const JlaDev &d, const JlaCoef &c, int I, int J, int T, int lane,
                                         const double *__restrict__ dvar, const double *__restrict__ dm, double (&v)[4])
{
    const int gj = JLA_NB * J + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = (lane >> 4) + 4 * r;
        double x = 0.0;
        if (I < T) {
            const int gi = JLA_NB * I + i;
            if (gi < d.n && gj <= gi) {
                const size_t ix = (size_t)gi * d.n + gj;
                if (d.comp[JLA_MAG]) x = d.comp[JLA_MAG][ix];
                if (d.comp[JLA_STRETCH]) x = x + c.a2 * d.comp[JLA_STRETCH][ix];
                if (d.comp[JLA_COLOUR]) x = x + c.b2 * d.comp[JLA_COLOUR][ix];
                if (d.comp[JLA_MAG_STRETCH]) x = x + c.ta * d.comp[JLA_MAG_STRETCH][ix];
                if (d.comp[JLA_MAG_COLOUR]) x = x - c.tb * d.comp[JLA_MAG_COLOUR][ix];
                if (d.comp[JLA_STRETCH_COLOUR]) x = x - c.tab * d.comp[JLA_STRETCH_COLOUR][ix];
                if (gi == gj) x = x + dvar[gi];
            } else if (gi >= d.n && gi == gj) {
                x = 1.0;
            }
        } else if (gj < d.n) {
            if (i == 0) x = dm[gj];
            else if (i == 1) x = d.one[gj];
            else if (i == 2) x = d.A2[gj];
        }
        v[r] = x;
    }
}

// acc += L[rows of tile I][0 .. kend) . L[rows of tile J][0 .. kend)^T.  A lane
// feeds the MFMA 4 consecutive k of its row, so the k of one instruction are
// k0 + 4 (lane >> 4) + q in both operands.
__device__ __forceinline__ void jla_load4(const double *p, double (&x)[4]) {
    const double2 lo = *reinterpret_cast<const double2 *>(p);
    const double2 hi = *reinterpret_cast<const double2 *>(p + 2);
    x[0] = lo.x, x[1] = lo.y, x[2] = hi.x, x[3] = hi.y;
}

// One 16-column step of a slab's update: the block column's operand b and the
// operands a of the slab's nt row tiles, then their MFMAs.
__device__ __forceinline__ void jla_slab_load(const double *pb, const double *pa, size_t tstep, int nt, double (&b)[4],
                                              double (&a)[4][4]) {
    jla_load4(pb, b);
#pragma unroll
    for (int t = 0; t < 4; t++)
        if (t < nt) jla_load4(pa + t * tstep, a[t]);
}
__device__ __forceinline__ void jla_slab_mfma(int nt, const double (&b)[4], const double (&a)[4][4],
                                              jla_f64x4 (&acc)[4]) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t >= nt) continue;
#pragma unroll
        for (int q = 0; q < 4; q++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][q], b[q], acc[t], 0, 0, 0);
    }
}

// Two waves a SIMD (256 VGPRs): two walkers' workgroups share a CU, each hiding
// the other's load latency (MI355X, nsn = 740, W = 1024: 15.3 ms; a variant
// with two operand sets in flight at 268 VGPRs, one workgroup a CU, took 24.6).
__global__ __launch_bounds__(JLA_THREADS, 2) void jla_chol_kernel(JlaDev d, const double *__restrict__ dl,
                                                               long long ld_walker, const double *__restrict__ nuis,
                                                               long long ld_nuis, double *__restrict__ out,
                                                               double *__restrict__ ws, const int *__restrict__ wcount,
                                                               int w0)
{
    // w: the walker's place in this launch and in the workspace; w0: the launch's first slot in the batch
    const int w = blockIdx.x;
    if (wcount && w0 + w >= *wcount) return;
    __shared__ double red[JLA_THREADS];
    __shared__ double dg[JLA_NB][JLA_NB + 1];             // the block column's diagonal tile
    __shared__ double slab[4][64][JLA_NB + 1];            // per wave: 4 row tiles on their way to the solve
    __shared__ int sbad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = d.n, Np = d.Np, T = Np / JLA_NB;
    const double alpha = nuis[(size_t)w * ld_nuis], beta = nuis[(size_t)w * ld_nuis + 1];
    const double *mu = dl + (size_t)w * ld_walker;
    double *L = ws + (size_t)w * jla_ws_doubles(Np);
    double *dvar = L + (size_t)(Np + JLA_NB) * Np, *dm = dvar + Np;
    JlaCoef c;
    c.a2 = alpha * alpha, c.b2 = beta * beta;
    c.ta = 2.0 * alpha, c.tb = 2.0 * beta, c.tab = 2.0 * (alpha * beta);
    if (tid == 0) sbad = 0;

    // diagonal terms and estimated_scriptm (:1056-1065)
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < n; i += JLA_THREADS) {
        const double dv = d.pre[i] + c.a2 * d.svar[i] + c.b2 * d.cvar[i] + c.ta * d.cms[i] - c.tb * d.cmc[i] -
                          c.tab * d.csc[i];
        const double iv = 1.0 / dv;
        dvar[i] = dv;
        s1 += iv;
        s2 += (d.mag[i] - mu[i]) * iv;
    }
    const double wtval = jla_block_sum(s1, red);
    const double scriptm = jla_block_sum(s2, red) / wtval;
    for (int i = tid; i < Np; i += JLA_THREADS)
        dm[i] = i < n ? d.mag[i] - mu[i] + alpha * d.stretch[i] - beta * d.colour[i] - scriptm : 0.0;
    __syncthreads();

    double G[6];   // A = G00, B = G01, C = G02, E = G11, D = G12, F = G22
    if (d.diag) {
        // diag_errors (:1067-1078)
        double p[6] = {0, 0, 0, 0, 0, 0};
        for (int i = tid; i < n; i += JLA_THREADS) {
            const double iv = 1.0 / dvar[i], x = dm[i], o = d.one[i], a2 = d.A2[i];
            p[0] += iv * x * x;
            p[1] += iv * x * o;
            p[2] += iv * x * a2;
            p[3] += iv * o * o;
            p[4] += iv * o * a2;
            p[5] += iv * a2 * a2;
        }
#pragma unroll
        for (int q = 0; q < 6; q++) G[q] = jla_block_sum(p[q], red);
    } else {
        const size_t ld = (size_t)Np;
        const size_t lrow = (size_t)(lane & 15) * ld + 4 * (lane >> 4);   // a lane's operand row and k offset
        bool bad = false;
        for (int J = 0; J < T; J++) {
            const int kend = JLA_NB * J;
            const double *pj = L + (size_t)JLA_NB * J * ld + lrow;
            if (wave == 0) {
                // the diagonal tile: update, then its 16 x 16 Cholesky in registers,
                // a lane per row (the four 16-lane groups compute the same rows)
                // (32 columns' loads in flight at a time; a chunk past kend is zeros, which add nothing)
                jla_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < kend; k0 += 32) {
                    double b[2][4];
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        if (k0 + 16 * u < kend) jla_load4(pj + k0 + 16 * u, b[u]);
                        else b[u][0] = b[u][1] = b[u][2] = b[u][3] = 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++)
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(b[u][q], b[u][q], acc, 0, 0, 0);
                }
                double v[4];
                jla_tile(d, c, J, J, T, lane, dvar, dm, v);
#pragma unroll
                for (int r = 0; r < 4; r++) dg[(lane >> 4) + 4 * r][lane & 15] = v[r] - acc[r];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int row = lane & 15;
                double x[JLA_NB];
#pragma unroll
                for (int k = 0; k < JLA_NB; k++) x[k] = dg[row][k];
                bool nonpos = false;
#pragma unroll
                for (int j = 0; j < JLA_NB; j++) {
                    double s = x[j];
#pragma unroll
                    for (int k = 0; k < j; k++) s -= x[k] * __shfl(x[k], j, 16);
                    const double piv = __shfl(s, j, 16);
                    if (!(piv > 0.0)) nonpos = true;     // DPOTRF status /= 0, a NaN pivot included
                    const double rt = sqrt(piv);
                    x[j] = row == j ? rt : (row > j ? s / rt : 0.0);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (lane < JLA_NB) {
                    double *g = L + (size_t)(JLA_NB * J + row) * ld + JLA_NB * J;
#pragma unroll
                    for (int k = 0; k < JLA_NB; k++) {
                        dg[row][k] = x[k];
                        g[k] = x[k];
                    }
                    if (nonpos && lane == 0) sbad = 1;
                }
            }
            // the row tiles below it (the right-hand sides last), 4 to a slab, slabs dealt to the waves
            const int nslab = (T - J + 3) / 4;
            bool first = true;
            for (int s = (wave + 3) & 3; s < nslab || first; s += 4) {   // wave 0, which factors the diagonal tile, last
                const bool live = s < nslab;
                const int I0 = J + 1 + 4 * s;
                jla_f64x4 acc[4];
                if (live) {
#pragma unroll
                    for (int t = 0; t < 4; t++) acc[t] = jla_f64x4{0.0, 0.0, 0.0, 0.0};
                    const double *pa = L + (size_t)JLA_NB * I0 * ld + lrow;
                    const size_t tstep = (size_t)JLA_NB * ld;
                    const int nt = min(4, T - I0 + 1);
                    for (int k0 = 0; k0 < kend; k0 += 16) {
                        double b[4], a[4][4];
                        jla_slab_load(pj + k0, pa + k0, tstep, nt, b, a);
                        jla_slab_mfma(nt, b, a, acc);
                    }
                }
                if (first) {
                    __syncthreads();   // the diagonal tile is in dg
                    first = false;
                    bad = sbad != 0;
                }
                if (bad || !live) continue;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (I0 + t > T) continue;
                    double v[4];
                    jla_tile(d, c, I0 + t, J, T, lane, dvar, dm, v);
#pragma unroll
                    for (int r = 0; r < 4; r++) slab[wave][JLA_NB * t + (lane >> 4) + 4 * r][lane & 15] = v[r] - acc[t][r];
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                // X L_JJ^T = A by forward substitution, a lane per row
                if (I0 + (lane >> 4) <= T) {
                    double x[JLA_NB];
#pragma unroll
                    for (int j = 0; j < JLA_NB; j++) {
                        double sum = slab[wave][lane][j];
#pragma unroll
                        for (int k = 0; k < j; k++) sum -= x[k] * dg[j][k];
                        x[j] = sum / dg[j][j];
                    }
                    double2 *g = reinterpret_cast<double2 *>(L + ((size_t)JLA_NB * I0 + lane) * ld + JLA_NB * J);
#pragma unroll
                    for (int k = 0; k < JLA_NB / 2; k++) g[k] = make_double2(x[2 * k], x[2 * k + 1]);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();   // the block column is in L for the next one's updates; dg and sbad are free
            if (bad) break;
        }
        if (bad) {
            if (tid == 0) out[w] = CMBL_LOGZERO;
            return;
        }
        // G = Y^T Y over the right-hand-side rows of L
        const double *y0 = L + (size_t)Np * ld, *y1 = y0 + ld, *y2 = y1 + ld;
        double p[6] = {0, 0, 0, 0, 0, 0};
        for (int k = tid; k < Np; k += JLA_THREADS) {
            const double a = y0[k], b = y1[k], e = y2[k];
            p[0] += a * a;
            p[1] += a * b;
            p[2] += a * e;
            p[3] += b * b;
            p[4] += b * e;
            p[5] += e * e;
        }
#pragma unroll
        for (int q = 0; q < 6; q++) G[q] = jla_block_sum(p[q], red);
    }
    if (tid != 0) return;
    const double inv_twopi = 1.0 / (2.0 * 3.14159265358979323846);
    const double A = G[0], B = G[1], C = G[2], E = G[3], D = G[4], F = G[5];
    double chisq;
    if (d.two) {
        const double tempG = F - D * D / E;
        if (!(tempG > 0.0)) {   // the reference stops ("Twoscriptm assumption violation")
            out[w] = CMBL_LOGZERO;
            return;
        }
        chisq = A + log(E * inv_twopi) + log(tempG * inv_twopi) - C * C / tempG - B * B * F / (E * tempG) +
                2.0 * B * C * D / (E * tempG);
    } else {
        chisq = A + log(E * inv_twopi) - B * B / E;
    }
    out[w] = chisq / 2;
}

// ------------------------------------------------------------ likelihood

struct JlaLike : Like {
    JlaData h;
    JlaDev dev{};
    DevBuf b_tab[11], b_comp[JLA_NCOMP];

    explicit JlaLike(JlaData &&data) : h(std::move(data)) {
        name = "JLA";
        tag = "JLA";
        n_nuis = 2;
        nuisance_names = "alpha_JLA beta_JLA";   // data/JLA.paramnames
        speed = 0;                               // TDataLikelihood's default: JLALikelihood_Add sets none
        theory_len = h.nsn;
        dev.n = h.nsn;
        dev.Np = (h.nsn + JLA_NB - 1) / JLA_NB * JLA_NB;
        dev.two = h.twoscriptmfit;
        dev.diag = h.diag_errors;
        const std::vector<double> *tab[11] = {&h.mag, &h.stretch, &h.colour, &h.pre_vars, &h.stretch_var, &h.colour_var,
                                              &h.cov_ms, &h.cov_mc, &h.cov_sc, &h.one, &h.A2};
        const double **dst[11] = {&dev.mag, &dev.stretch, &dev.colour, &dev.pre, &dev.svar, &dev.cvar,
                                  &dev.cms, &dev.cmc, &dev.csc, &dev.one, &dev.A2};
        for (int i = 0; i < 11; i++) *dst[i] = upload(b_tab[i], *tab[i]);
        for (int c = 0; c < JLA_NCOMP; c++) {
            dev.comp[c] = h.has[c] ? upload(b_comp[c], h.comp[c]) : nullptr;
            std::vector<double>().swap(h.comp[c]);
        }
    }

    size_t workspace_size(int W) const override {
        return jla_ws_doubles(dev.Np) * 8 * (size_t)std::max(0, std::min(W, JLA_MAXW));
    }

    void run(int W, const double *dl, long long ld_walker, const double *nuis, long long ld_nuis, double *out, void *ws,
             hipStream_t stream, const int *wcount) {
        if (W <= 0) return;
        nuis = nuisance_rows(nuis, nullptr);
        if (ld_nuis < n_nuis) fail(CMBL_ERR_ARG, "JLA: ld_nuis %lld < %d", ld_nuis, n_nuis);
        if (ld_walker != 0 && ld_walker < h.nsn)
            fail(CMBL_ERR_ARG, "JLA: ld_walker %lld < the %d distance moduli of a walker", ld_walker, h.nsn);
        if (!ws) {
            own_ws.grow(workspace_size(W));
            ws = own_ws.p;
        }
        // batches beyond the workspace's walkers run in chunks, one after another in stream order
        for (int w0 = 0; w0 < W; w0 += JLA_MAXW) {
            const int Wc = std::min(JLA_MAXW, W - w0);
            timed_launch("jla_chol_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(jla_chol_kernel, dim3(Wc), dim3(JLA_THREADS), 0, stream, e0, e1, 0, dev,
                                      dl + (size_t)w0 * ld_walker, ld_walker, nuis + (size_t)w0 * ld_nuis, ld_nuis,
                                      out + w0, static_cast<double *>(ws), wcount, w0);
            });
            HIP_CHECK(hipGetLastError());
        }
    }

    void loglike_batch(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                       long long ld_nuis, double *out, void *ws, hipStream_t stream) override {
        (void)ld_field;   // one field: the distance moduli
        run(W, dl, ld_walker, nuis, ld_nuis, out, ws, stream, nullptr);
    }
    bool sparse_capable() const override { return true; }
    void loglike_batch_sparse(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                              long long ld_nuis, double *out, void *ws, hipStream_t stream,
                              const int *wcount) override {
        (void)ld_field;
        run(W, dl, ld_walker, nuis, ld_nuis, out, ws, stream, wcount);
    }
};

std::unique_ptr<Like> make_jla(const Ini &ini) { return std::unique_ptr<Like>(new JlaLike(load_jla(ini))); }

}  // namespace cmamd
