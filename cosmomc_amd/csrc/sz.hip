// Planck SZ cluster-counts likelihood (source/szcounts.f90, the 2D form N(z, q)):
// the loader (SZLikelihood_Add :1385-1499, SZ_init :1501-1821) and the batched
// evaluation of grid_C_2d / integrate_m_zq / SZCC_Cash (:827-1059, 1825-1975).
//
// A walker's theory is one row [H0, ns, ombh2, E[nzs], dA[nzs], grid[nzs][nm]]
// (cosmomc_amd.h).  At open, once:
//   sz_erfs_kernel    the table erfs(k, theta, qbin) the reference rebuilds on
//                     every call (:975-1000), a thread per entry, the patches
//                     summed in order, and beside it the slope
//                     (erfs(k, t + 1) - erfs(k, t)) / (theta_{t+1} - theta_t) of
//                     every theta interval: the quotient :1041 forms per use.
// Per evaluation:
//   sz_compl_kernel   the selection function of a walker with scatter_SZ != 0
//                     (:1003-1052): 16 lanes per (m, z), a lane per node of ln Y;
//   sz_compl0_kernel  the same for scatter_SZ == 0 exactly (:907-955), a thread
//                     per (m, z) looping over the patches;
//   sz_counts_kernel  DN (:854-866), the Cash sum and the priors (:1924-1972),
//                     a workgroup per walker.
// A completeness is rounded to single precision where the reference stores it
// in its real(sp) table.  No kernel uses atomics or waits for another
// workgroup, and every sum has a fixed order, so a walker's bits do not depend
// on W, its slot, ld_walker or the chunking.
//
// The ln Y trapezoid of :1036-1047 is summed by nodes instead of intervals:
// sum_k (f_k + f_{k+1}) / 2 * dy_k = sum_k f_k * (dy_{k-1} + dy_k) / 2, with
// f_k = win_k fac / y_k exp(-arg_k^2); the node weight over y_k is a table
// formed at open, fac is applied to the sum and arg is (lny_k - mu) times
// 1 / (sqrt(2) sigma).  Nodes where exp(-arg^2) is
// exactly 0 add nothing and are not visited: the window of nodes is
// |lny_k - mu| <= sqrt(746) sqrt(2) sigma plus one node on either side.
#include <cmath>
#include <set>

#include "sz.h"

namespace cmamd {

// ------------------------------------------------------------ loader

static bool sz_logical(const Ini &ini, const std::string &key, bool def) {
    const std::string v = ini.str(key);
    if (v.empty()) return def;
    const char ch = (char)std::toupper(v[0] == '.' && v.size() > 1 ? v[1] : v[0]);
    if (ch == 'T' || ch == '1' || ch == 'Y') return true;
    if (ch == 'F' || ch == '0' || ch == 'N') return false;
    fail(CMBL_ERR_FORMAT, "%s: bad logical %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
}

static std::vector<double> sz_column(const Ini &ini, const std::string &key, size_t col = 0) {
    const auto rows = load_txt(ini.relative_filename(key, true));
    std::vector<double> out;
    for (const auto &r : rows) {
        if (r.size() <= col) fail(CMBL_ERR_FORMAT, "SZ: %s needs %zu columns", key.c_str(), col + 1);
        out.push_back(r[col]);
    }
    return out;
}

// next_z (:601-615)
static double sz_next_z(double zi, double binz) {
    if (zi < sz_f32(0.2f)) return zi + sz_f32(1.e-3f);
    if (zi <= 1.0) return zi + sz_f32(1.e-2f);
    return zi + binz;
}

static int sz_minloc(const std::vector<double> &x, double v) {
    int best = 0;
    for (int i = 1; i < (int)x.size(); i++)
        if (std::fabs(x[i] - v) < std::fabs(x[best] - v)) best = i;   // the first minimum wins a tie
    return best;
}

SzData load_sz(const Ini &ini) {
    static const char *prior_keys[SZ_NPRIORS] = {"prior_ystar_SZ", "prior_alpha_SZ", "prior_scatter_SZ",
                                                 "prior_beta_SZ",  "prior_ns",       "prior_omegabh2",
                                                 "prior_lens",     "prior_wtg",      "prior_cccp"};
    std::set<std::string> served = {"name", "cat_file", "thetas_file", "skyfracs_file", "ylims_file", "nuisance_params",
                                    "1D",   "2D"};
    for (const char *k : prior_keys) served.insert(k);
    for (const std::string &k : ini.keys())
        if (!served.count(k)) fail(CMBL_ERR_UNSUPPORTED, "SZ: key %s is not supported", k.c_str());
    if (sz_logical(ini, "1D", false))
        fail(CMBL_ERR_UNSUPPORTED, "SZ: 1D = T (the N(z) form, SZ_switch = 1) is not supported");
    (void)sz_logical(ini, "2D", true);
    SzData d;
    for (int p = 0; p < SZ_NPRIORS; p++) d.prior_on[p] = sz_logical(ini, prior_keys[p], false) ? 1.0 : 0.0;
    if (ini.has("nuisance_params")) {
        d.param_names = load_paramnames(ini.relative_filename("nuisance_params", true), &d.n_params);
        if (d.n_params != 5) fail(CMBL_ERR_FORMAT, "SZ: nuisance_params names %d parameters, not 5", d.n_params);
    } else {
        d.param_names = "alpha_SZ ystar_SZ bias_SZ scatter_SZ beta_SZ";
        d.n_params = 5;
    }

    d.thetas = sz_column(ini, "thetas_file");
    d.skyfracs = sz_column(ini, "skyfracs_file");
    d.nthetas = (int)d.thetas.size(), d.npatches = (int)d.skyfracs.size();
    if (d.nthetas < 2) fail(CMBL_ERR_FORMAT, "SZ: thetas_file holds %d thetas, fewer than two", d.nthetas);
    if (d.npatches < 1) fail(CMBL_ERR_FORMAT, "SZ: skyfracs_file holds no patch");
    // The neighbour of the nearest theta on thp's side (:1020-1027) lies outside the reference's table when the
    // nearest is the first entry and larger than thp, or the last and smaller: only a first entry that is the
    // least and a last that is the greatest rule that out for every thp.  The order in between is free.
    for (int t = 0; t < d.nthetas; t++)
        if (d.thetas[t] < d.thetas[0] || d.thetas[t] > d.thetas[d.nthetas - 1])
            fail(CMBL_ERR_UNSUPPORTED,
                 "SZ: thetas_file must begin with its least theta and end with its greatest (entry %d is %g, the first "
                 "%g, the last %g): the reference reads outside its table otherwise",
                 t + 1, d.thetas[t], d.thetas[0], d.thetas[d.nthetas - 1]);
    const std::vector<double> yl = sz_column(ini, "ylims_file");
    if (yl.size() != (size_t)d.npatches * d.nthetas)
        fail(CMBL_ERR_FORMAT, "SZ: ylims_file holds %zu rows, expected %d patches x %d thetas", yl.size(), d.npatches,
             d.nthetas);
    d.ylims.resize(yl.size());
    for (int t = 0; t < d.nthetas; t++)   // the patch runs fastest in the file (:1640-1648)
        for (int i = 0; i < d.npatches; i++) d.ylims[(size_t)i * d.nthetas + t] = yl[(size_t)t * d.npatches + i];
    d.fsky = 0;
    for (double s : d.skyfracs) d.fsky += s;

    // the catalogue: rows with S/N >= q.  The compiled reference's second pass
    // (:1600-1608) reads one line more than the file holds; the failed read
    // leaves the last row's values in place, so a last row at or above the
    // threshold enters twice (its "total cat" line shows it).  Followed here.
    const double q = 6.0;
    std::vector<double> cz = sz_column(ini, "cat_file", 0), cq = sz_column(ini, "cat_file", 2);
    if (!cq.empty() && cq.back() >= q) cz.push_back(cz.back()), cq.push_back(cq.back());
    std::vector<double> zc, qc;
    for (size_t i = 0; i < cq.size(); i++)
        if (cq[i] >= q) zc.push_back(cz[i]), qc.push_back(cq[i]);
    d.n_cat = (int)zc.size();

    const double z0 = 0.0, dz = 0.1, zmaxs = 1.0;
    const double logymin = sz_f32(0.7f), logymax = sz_f32(1.5f), dlogy = 0.25;
    d.Nz = (int)((zmaxs - z0) / dz) + 1;
    const int Ny = (int)((logymax - logymin) / dlogy) + 1;
    d.nq = Ny + 1;
    d.logq.resize(d.nq);
    double yi = logymin + dlogy / 2.0;
    for (int j = 0; j < d.nq; j++) d.logq[j] = yi, yi = yi + dlogy;
    d.Z.resize(d.Nz);
    for (int i = 0; i < d.Nz; i++) d.Z[i] = z0 + i * dz + 0.5 * dz;
    d.Z[0] = d.Z[0] + sz_f32(1.e-8f);

    // catalogue counts in (z, q) and the clusters without a redshift (:1743-1797)
    std::vector<double> lo(Ny), hi(Ny);
    for (int j = 0; j < Ny; j++) lo[j] = std::pow(10.0, d.logq[j] - dlogy / 2.0), hi[j] = std::pow(10.0, d.logq[j] + dlogy / 2.0);
    auto in_bin = [&](double qv, int j) { return j < Ny ? (qv < hi[j] && qv >= lo[j]) : qv >= hi[Ny - 1]; };
    d.DNcat.assign((size_t)d.Nz * d.nq, 0.0);
    double zlo = z0, zhi = z0 + dz;
    for (int i = 0; i < d.Nz; i++) {
        for (int j = 0; j < d.nq; j++)
            for (size_t c = 0; c < zc.size(); c++)
                if (zc[c] >= zlo && zc[c] < zhi && in_bin(qc[c], j)) d.DNcat[(size_t)i * d.nq + j] += 1.0;
        zlo = zlo + dz, zhi = zhi + dz;
    }
    for (int j = 0; j < d.nq; j++)
        for (size_t c = 0; c < zc.size(); c++)
            if (zc[c] == -1 && in_bin(qc[c], j)) {
                double norm = 0.0;
                for (int k = 0; k < d.Nz; k++) norm = norm + d.DNcat[(size_t)k * d.nq + j];
                for (int k = 0; k < d.Nz; k++) d.DNcat[(size_t)k * d.nq + j] = d.DNcat[(size_t)k * d.nq + j] * (norm + 1.0) / norm;
            }
    d.lnfact.assign(d.DNcat.size(), 0.0);
    for (size_t i = 0; i < d.DNcat.size(); i++) {
        const double c = d.DNcat[i];
        if (c != 0.0) {
            if (c > 10.0) d.lnfact[i] = sz_f32(0.918939f) + (c + 0.5) * std::log(c) - c;   // Stirling
            else {
                double fact = 1.0;
                for (int ii = 1; ii <= (int)c; ii++) fact = ii * fact;
                d.lnfact[i] = std::log(fact);
            }
        }
    }

    // steps in z and ln M (:649-694) and the z range of every bin (:847-852)
    const double binz = d.binz = d.Z[1] - d.Z[0];
    const double min_z = d.Z[0] - 0.5 * binz, max_z = d.Z[d.Nz - 1] + 0.5 * binz;
    double zi = min_z < 0 ? 0.0 : min_z;
    while (zi <= max_z) d.steps_z.push_back(zi), zi = sz_next_z(zi, binz);
    if (d.steps_z[0] == 0) d.steps_z[0] = sz_f32(1.e-5f);
    d.nzs = (int)d.steps_z.size();
    const double dlnm = 0.05;
    d.nm = (int)((sz_f32(37.f) - sz_f32(31.f)) / dlnm);
    double lnm = 31.0;
    for (int i = 0; i < d.nm; i++) d.steps_m.push_back(lnm + dlnm / 2.0), lnm = lnm + dlnm;
    for (int i = 0; i < d.Nz; i++) {
        d.j1.push_back(sz_minloc(d.steps_z, d.Z[i] - 0.5 * binz));
        d.j2.push_back(sz_minloc(d.steps_z, d.Z[i] + 0.5 * binz));
    }

    // the nodes in ln Y (:958-963, 977-980) and the S/N limits of the bins (:987-990)
    const double lnymin = -11.5, lnymax = 10.0, dlny = sz_f32(0.05f);
    d.nlny = (int)((lnymax - lnymin) / dlny);
    double lny = lnymin;
    for (int k = 0; k < d.nlny; k++) d.lny.push_back(lny), d.y0.push_back(std::exp(lny)), lny = lny + dlny;
    const double dlq = d.logq[1] - d.logq[0];
    for (int j = 0; j < d.nq; j++) {
        d.qmin.push_back(std::pow(10.0, d.logq[j] - dlq / 2.0));
        d.qmax.push_back(std::pow(10.0, d.logq[j] + dlq / 2.0));
    }
    return d;
}

// ------------------------------------------------------------ kernels

static constexpr int SZ_THREADS = 256;   // 4 waves
static constexpr int SZ_MAXW = 1024;     // walkers per launch of the per-walker kernels (workspace_size)
static constexpr int SZ_NQ = 5;          // S/N bins (Ny + 1): fixed by the reference's constants
static constexpr int SZ_GROUP = 16;      // lanes that share one (m, z) in sz_compl_kernel
static constexpr int SZ_PTS = 240;       // (m, z) per workgroup there: 15 rounds of its 16 groups
static constexpr int SZ_MAXK = 432;      // ln Y nodes (429) the tables in LDS hold
static constexpr int SZ_MAXM = 128;      // steps in ln M (120) the tables in LDS hold
static constexpr int SZ_ZBLK = 4;        // steps in z a workgroup's SZ_PTS points can meet (nm >= SZ_PTS / 2)

#define SZ_SQRT2 ((double)1.41421354f)      // sqrt(2.) is a single-precision intrinsic in the reference
#define SZ_PI 3.141592653589793238463

struct SzDev {
    int nzs, nm, npts, Nz, nlny, nthetas, npatches;
    int sorted;                          // thetas strictly ascending: the nearest theta by bisection
    double fsky, theta_min, theta_max;
    const double *em;                    // [nm] exp(steps_m)
    const double *thetas, *skyfracs;     // [nthetas], [npatches]
    const double *ylims;                 // [npatches][nthetas]
    const double *lny, *y0, *wy;         // [nlny] nodes, exp(lny), node weight (dy_{k-1} + dy_k) / 2 / y0
    const double *erfs, *slope;          // [nthetas][SZ_NQ][nlny], [nthetas - 1][SZ_NQ][nlny]
    const double *dzs;                   // [nzs - 1] steps_z[j + 1] - steps_z[j]
    const int *j1, *j2;                  // [Nz]
    const double *DNcat, *lnfact;        // [Nz][SZ_NQ]
    double qmin[SZ_NQ], qmax[SZ_NQ];
    double prior_on[SZ_NPRIORS], prior_c[SZ_NPRIORS], prior_d[SZ_NPRIORS];
};

// erf_compl (:245-250)
__device__ __forceinline__ double sz_erf_compl(double y, double sn, double q) {
    const double arg = (y - q * sn) / SZ_SQRT2 / sn;
    return (erf(arg) + 1.0) / 2.0;
}

// c2 of :991-993 and :949-951: the product for S/N bin b
__device__ __forceinline__ double sz_bin_compl(const SzDev &d, double y, double sn, int b) {
    const double e0 = sz_erf_compl(y, sn, 6.0);
    if (b == 0) return e0 * (1.0 - sz_erf_compl(y, sn, d.qmax[0]));
    if (b == SZ_NQ - 1) return e0 * sz_erf_compl(y, sn, d.qmin[b]);
    return e0 * sz_erf_compl(y, sn, d.qmin[b]) * (1.0 - sz_erf_compl(y, sn, d.qmax[b]));
}

__device__ __forceinline__ double sz_sum_patches(const SzDev &d, double y, int t, int b) {
    double s = 0.0;
    for (int i = 0; i < d.npatches; i++) s = s + sz_bin_compl(d, y, d.ylims[(size_t)i * d.nthetas + t], b) * d.skyfracs[i];
    return s;
}

__global__ __launch_bounds__(SZ_THREADS) void sz_erfs_kernel(SzDev d, double *__restrict__ erfs,
                                                             double *__restrict__ slope)
{
    const int n = d.nthetas * SZ_NQ * d.nlny;
    const int idx = blockIdx.x * SZ_THREADS + threadIdx.x;
    if (idx >= n) return;
    const int k = idx % d.nlny, b = (idx / d.nlny) % SZ_NQ, t = idx / (d.nlny * SZ_NQ);
    const double e = sz_sum_patches(d, d.y0[k], t, b);
    erfs[idx] = e;
    if (t + 1 < d.nthetas) slope[idx] = (sz_sum_patches(d, d.y0[k], t + 1, b) - e) / (d.thetas[t + 1] - d.thetas[t]);
}

struct SzPoint {
    double thp, yp;
    int l1, l2;
};

// The theta bracket (:1010-1028): the nearest theta (the first of two equally
// near) and its neighbour on thp's side, or the end pair beyond either end.
// thp equal to the last theta would make the reference read one theta past its
// table with weight (thp - th1) = 0; l2 stays inside.  The thetas need not
// ascend, but the first is the least and the last the greatest (load_sz).
__device__ __forceinline__ void sz_bracket(const SzDev &d, SzPoint &p) {
    const int nth = d.nthetas;
    if (p.thp > d.theta_max) p.l1 = nth - 1, p.l2 = nth - 2;
    else if (p.thp < d.theta_min) p.l1 = 0, p.l2 = 1;
    else {
        int best = 0;
        if (d.sorted) {
            int lo = 0, hi = nth - 1;   // thetas[lo] <= thp <= thetas[hi]
            while (hi - lo > 1) {
                const int k = (hi + lo) / 2;
                if (d.thetas[k] > p.thp) hi = k;
                else lo = k;
            }
            best = fabs(d.thetas[hi] - p.thp) < fabs(d.thetas[lo] - p.thp) ? hi : lo;
        } else {
            double db = fabs(d.thetas[0] - p.thp);
            for (int t = 1; t < nth; t++) {
                const double dt = fabs(d.thetas[t] - p.thp);
                if (dt < db) db = dt, best = t;
            }
        }
        p.l1 = best;
        p.l2 = d.thetas[best] > p.thp ? best - 1 : best + 1;
        if (p.l2 >= nth) p.l2 = nth - 2;
        // l2 >= 0: best == 0 with thetas[0] > thp >= theta_min needs a first theta that is not the least, which
        // load_sz refuses; a NaN thp compares false and takes best + 1
    }
}

// theta500 and y500 (:221-243) from their factors: c_th = thetastar (H0/70)^(-2/3), c_y = ystar (H0/70)^(-2+alpha),
// the powers of m2 / 3e14 (100 / H0) and of E(z), dfac = 100 dA / 500 / H0
__device__ __forceinline__ SzPoint sz_scaling(const SzDev &d, double c_th, double c_y, double m13, double ma, double e23,
                                              double eb, double dfac) {
    SzPoint p;
    p.thp = c_th * m13 * e23 / dfac;
    p.yp = c_y * ma * eb / (dfac * dfac);
    sz_bracket(d, p);
    return p;
}

struct SzWalker {   // what a walker's H0 and nuisance values fix
    double c_th, c_y, mscale, alpha, beta, H0;
};

__device__ __forceinline__ SzWalker sz_walker(const double *__restrict__ row, const double *__restrict__ nu) {
    SzWalker k;
    k.H0 = row[0], k.alpha = nu[0], k.beta = nu[4];
    const double ystar = pow(10.0, nu[1]) / pow(2.0, k.alpha) * (double)0.00472724f;
    const double h70 = k.H0 / 70.0;
    k.c_th = (double)6.997f * pow(h70, (double)(-2.f / 3.f));
    k.c_y = ystar * pow(h70, -2.0 + k.alpha);
    k.mscale = nu[2];
    return k;
}

// m2 / 3.e14 * (100 / H0) of mass step m
__device__ __forceinline__ double sz_mfac(const SzDev &d, const SzWalker &k, int m) {
    return d.em[m] * k.mscale / (double)3.e14f * (100.0 / k.H0);
}

__device__ __forceinline__ SzPoint sz_point(const SzDev &d, const double *__restrict__ row,
                                            const double *__restrict__ nu, int j, int m) {
    const SzWalker k = sz_walker(row, nu);
    const double E = row[3 + j], dA = row[3 + d.nzs + j], mfac = sz_mfac(d, k, m);
    const double m23 = (double)(-2.f / 3.f);
    return sz_scaling(d, k.c_th, k.c_y, pow(mfac, (double)(1.f / 3.f)), pow(mfac, k.alpha), pow(E, m23), pow(E, k.beta),
                      100.0 * dA / 500.0 / k.H0);
}

// comp[w][b][p], p = j * nm + m: single precision as completeness_2d is
__global__ __launch_bounds__(SZ_THREADS) void sz_compl_kernel(SzDev d, const double *__restrict__ dl, long long ld_walker,
                                                              const double *__restrict__ nuis, long long ld_nuis,
                                                              float *__restrict__ comp, const int *__restrict__ wcount,
                                                              int w0)
{
    const int w = blockIdx.y;
    if (wcount && w0 + w >= *wcount) return;
    const double *nu = nuis + (size_t)w * ld_nuis;
    const double sigmaM = nu[3];
    if (sigmaM == 0) return;   // sz_compl0_kernel's walker
    __shared__ double s_lny[SZ_MAXK], s_wy[SZ_MAXK];
    __shared__ double s_m13[SZ_MAXM], s_ma[SZ_MAXM], s_e23[SZ_ZBLK], s_eb[SZ_ZBLK], s_df[SZ_ZBLK];
    const int tid = threadIdx.x, N = d.nlny;
    const double *row = dl + (size_t)w * ld_walker;
    const SzWalker wk = sz_walker(row, nu);
    const int pbeg = blockIdx.x * SZ_PTS, jbeg = pbeg / d.nm;
    for (int k = tid; k < N; k += SZ_THREADS) s_lny[k] = d.lny[k], s_wy[k] = d.wy[k];
    // the powers of the mass factor, one per mass, and of E(z), one per step in z this workgroup meets
    if (tid < d.nm) {
        const double mfac = sz_mfac(d, wk, tid);
        s_m13[tid] = pow(mfac, (double)(1.f / 3.f)), s_ma[tid] = pow(mfac, wk.alpha);
    } else if (tid >= SZ_MAXM && tid < SZ_MAXM + SZ_ZBLK && jbeg + tid - SZ_MAXM < d.nzs) {
        const int jz = tid - SZ_MAXM, j = jbeg + jz;
        const double E = row[3 + j], dA = row[3 + d.nzs + j];
        s_e23[jz] = pow(E, (double)(-2.f / 3.f)), s_eb[jz] = pow(E, wk.beta), s_df[jz] = 100.0 * dA / 500.0 / wk.H0;
    }
    __syncthreads();
    float *cw = comp + (size_t)w * SZ_NQ * d.npts;
    const int grp = tid / SZ_GROUP, gl = tid % SZ_GROUP;
    const double fac = 1.0 / sqrt(2.0 * SZ_PI * (sigmaM * sigmaM));
    const double rs = SZ_SQRT2 * sigmaM, inv_rs = 1.0 / rs;
    const double reach = sqrt(746.0) * fabs(rs), lnymin = d.lny[0], dlny = (double)0.05f;
    const int pend = min(pbeg + SZ_PTS, d.npts);
    for (int p = pbeg + grp; p < pend; p += SZ_THREADS / SZ_GROUP) {
        const int j = p / d.nm, m = p - j * d.nm, jz = j - jbeg;
        const SzPoint pt = sz_scaling(d, wk.c_th, wk.c_y, s_m13[m], s_ma[m], s_e23[jz], s_eb[jz], s_df[jz]);
        const double mu = log(pt.yp);
        const double wth = pt.thp - d.thetas[pt.l1];
        // the nodes whose exp(-arg^2) can differ from 0, one more on either side; all of them when mu is not finite
        int klo = 0, khi = N - 1;
        const double a = (mu - reach - lnymin) / dlny, b = (mu + reach - lnymin) / dlny;
        if (fabs(a) <= 1e9 && fabs(b) <= 1e9) {
            klo = max(0, (int)floor(a) - 1);
            khi = min(N - 1, (int)ceil(b) + 1);
        }
        const double *e1 = d.erfs + (size_t)pt.l1 * SZ_NQ * N;
        const double *sl = d.slope + (size_t)min(pt.l1, pt.l2) * SZ_NQ * N;
        double acc[SZ_NQ];
#pragma unroll
        for (int q = 0; q < SZ_NQ; q++) acc[q] = 0.0;
        for (int k = klo + gl; k <= khi; k += SZ_GROUP) {
            const double arg = (s_lny[k] - mu) * inv_rs;
            const double g = exp(-(arg * arg)) * s_wy[k];
#pragma unroll
            for (int q = 0; q < SZ_NQ; q++) {
                const double win = e1[(size_t)q * N + k] + sl[(size_t)q * N + k] * wth;
                acc[q] = acc[q] + win * g;
            }
        }
#pragma unroll
        for (int q = 0; q < SZ_NQ; q++) {
            double v = acc[q];
#pragma unroll
            for (int o = SZ_GROUP / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, SZ_GROUP);
            v = v * fac;
            if (v > d.fsky) v = d.fsky;
            if (v < 0.0) v = 0.0;
            if (gl == 0) cw[(size_t)q * d.npts + p] = (float)v;
        }
    }
}

// scatter_SZ == 0 exactly (:907-955): the patches at y500, the running sum kept in single precision as the
// reference's real(sp) table keeps it
__global__ __launch_bounds__(SZ_THREADS) void sz_compl0_kernel(SzDev d, const double *__restrict__ dl,
                                                               long long ld_walker, const double *__restrict__ nuis,
                                                               long long ld_nuis, float *__restrict__ comp,
                                                               const int *__restrict__ wcount, int w0)
{
    const int w = blockIdx.y;
    if (wcount && w0 + w >= *wcount) return;
    const double *nu = nuis + (size_t)w * ld_nuis;
    if (!(nu[3] == 0)) return;
    const int p = blockIdx.x * SZ_THREADS + threadIdx.x;
    if (p >= d.npts) return;
    const double *row = dl + (size_t)w * ld_walker;
    float *cw = comp + (size_t)w * SZ_NQ * d.npts;
    const int j = p / d.nm, m = p - j * d.nm;
    const SzPoint pt = sz_point(d, row, nu, j, m);
    const double th1 = d.thetas[pt.l1], th2 = d.thetas[pt.l2];
    float c[SZ_NQ];
#pragma unroll
    for (int q = 0; q < SZ_NQ; q++) c[q] = 0.f;
    for (int i = 0; i < d.npatches; i++) {
        const double y1 = d.ylims[(size_t)i * d.nthetas + pt.l1], y2 = d.ylims[(size_t)i * d.nthetas + pt.l2];
        const double y = y1 + (y2 - y1) / (th2 - th1) * (pt.thp - th1);
        const double e0 = sz_erf_compl(pt.yp, y, 6.0), sky = d.skyfracs[i];
#pragma unroll
        for (int q = 0; q < SZ_NQ; q++) {
            double c2;
            if (q == 0) c2 = e0 * (1.0 - sz_erf_compl(pt.yp, y, d.qmax[0]));
            else if (q == SZ_NQ - 1) c2 = e0 * sz_erf_compl(pt.yp, y, d.qmin[q]);
            else c2 = e0 * sz_erf_compl(pt.yp, y, d.qmin[q]) * (1.0 - sz_erf_compl(pt.yp, y, d.qmax[q]));
            c[q] = (float)((double)c[q] + c2 * sky);
        }
    }
#pragma unroll
    for (int q = 0; q < SZ_NQ; q++) cw[(size_t)q * d.npts + p] = c[q];
}

// DN(i, b) (:854-866): a wave per (z bin, S/N bin), a lane every 64th term, then the lanes in a fixed tree; the
// Cash sum and the priors by one thread in the reference's order.  A non-finite -lnL is logZero, for that walker alone.
__global__ __launch_bounds__(SZ_THREADS) void sz_counts_kernel(SzDev d, const double *__restrict__ dl,
                                                               long long ld_walker, const double *__restrict__ nuis,
                                                               long long ld_nuis, const float *__restrict__ comp,
                                                               double *__restrict__ out, const int *__restrict__ wcount,
                                                               int w0)
{
    const int w = blockIdx.x;
    if (wcount && w0 + w >= *wcount) return;
    __shared__ double s_dn[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nm = d.nm;
    const double *row = dl + (size_t)w * ld_walker, *nu = nuis + (size_t)w * ld_nuis;
    const double *grid = row + 3 + 2 * (size_t)d.nzs;
    const float *cw = comp + (size_t)w * SZ_NQ * d.npts;
    const double dlnm = 0.05;
    for (int it = wave; it < d.Nz * SZ_NQ; it += SZ_THREADS / 64) {
        const int i = it / SZ_NQ, b = it - i * SZ_NQ;
        const int ja = d.j1[i], n = (d.j2[i] - ja) * nm;
        const float *c = cw + (size_t)b * d.npts;
        double s = 0.0;
        for (int t = lane; t < n; t += 64) {
            const int jj = ja + t / nm, p = ja * nm + t;
            const double f1 = grid[p], f2 = grid[p + nm], c1 = (double)c[p], c2 = (double)c[p + nm];
            s = s + 0.5 * (f1 * c1 + f2 * c2) * d.dzs[jj] * dlnm;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
        if (lane == 0) s_dn[it] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    double sum = 0.0;
    for (int it = 0; it < d.Nz * SZ_NQ; it++) {
        const double DN = s_dn[it];
        if (DN != 0.0) sum = sum - 1.0 * (d.DNcat[it] * log(DN) - DN - d.lnfact[it]);
    }
    const double x[SZ_NPRIORS] = {nu[1], nu[0], nu[3], nu[4], row[1], row[2], 1.0 / nu[2], nu[2], nu[2]};
    double pr[SZ_NPRIORS];
#pragma unroll
    for (int p = 0; p < SZ_NPRIORS; p++) {
        const double dx = x[p] - d.prior_c[p];
        pr[p] = d.prior_on[p] * (dx * dx) / d.prior_d[p];
    }
    sum = sum + pr[SZ_PRIOR_YSTAR] + pr[SZ_PRIOR_ALPHA] + pr[SZ_PRIOR_SCATTER];
    sum = sum + pr[SZ_PRIOR_BETA];
    sum = sum + pr[SZ_PRIOR_NS] + pr[SZ_PRIOR_OMBH2];
    sum = sum + pr[SZ_PRIOR_LENS];
    sum = sum + pr[SZ_PRIOR_WTG];
    sum = sum + pr[SZ_PRIOR_CCCP];
    if (!(fabs(sum) <= 1.79769313486231570e308)) sum = CMBL_LOGZERO;
    out[w0 + w] = sum;
}

// ------------------------------------------------------------ likelihood

// 2.*x**2. in single precision: the denominators of the priors (:1954-1972)
static double sz_two_sq(float x) {
    const float sq = x * x;
    return (double)(2.f * sq);
}

struct SzLike : Like {
    SzData h;
    SzDev dev{};
    DevBuf b_em, b_th, b_sky, b_yl, b_lny, b_y0, b_wy, b_erfs, b_slope, b_dzs, b_j1, b_j2, b_dn, b_lf;

    explicit SzLike(SzData &&data) : h(std::move(data)) {
        name = "SZ";
        tag = "SZ";
        n_nuis = h.n_params;
        nuisance_names = h.param_names;
        speed = 0;   // TDataLikelihood's default; SZLikelihood_Add sets none
        theory_len = 3 + 2 * h.nzs + h.nzs * h.nm;
        if (h.nq != SZ_NQ || h.nlny > SZ_MAXK || h.Nz * h.nq > 64 || h.nm > SZ_MAXM || 2 * h.nm < SZ_PTS)
            fail(CMBL_ERR_UNSUPPORTED, "SZ: %d S/N bins, %d ln Y nodes, %d z bins, %d masses", h.nq, h.nlny, h.Nz, h.nm);
        dev.nzs = h.nzs, dev.nm = h.nm, dev.npts = h.nzs * h.nm, dev.Nz = h.Nz, dev.nlny = h.nlny;
        dev.nthetas = h.nthetas, dev.npatches = h.npatches, dev.fsky = h.fsky;
        dev.theta_min = *std::min_element(h.thetas.begin(), h.thetas.end());
        dev.theta_max = *std::max_element(h.thetas.begin(), h.thetas.end());
        dev.sorted = 1;
        for (int t = 0; t + 1 < h.nthetas; t++)
            if (!(h.thetas[t] < h.thetas[t + 1])) dev.sorted = 0;
        std::vector<double> em, wy(h.nlny), dzs;
        for (double lm : h.steps_m) em.push_back(std::exp(lm));
        for (int k = 0; k < h.nlny; k++) {
            const double dl = k > 0 ? h.y0[k] - h.y0[k - 1] : 0.0, dr = k + 1 < h.nlny ? h.y0[k + 1] - h.y0[k] : 0.0;
            wy[k] = (dl + dr) * 0.5 / h.y0[k];
        }
        for (int j = 0; j + 1 < h.nzs; j++) dzs.push_back(h.steps_z[j + 1] - h.steps_z[j]);
        dev.em = upload(b_em, em);
        dev.thetas = upload(b_th, h.thetas), dev.skyfracs = upload(b_sky, h.skyfracs), dev.ylims = upload(b_yl, h.ylims);
        dev.lny = upload(b_lny, h.lny), dev.y0 = upload(b_y0, h.y0), dev.wy = upload(b_wy, wy);
        dev.dzs = upload(b_dzs, dzs);
        dev.j1 = upload(b_j1, h.j1), dev.j2 = upload(b_j2, h.j2);
        dev.DNcat = upload(b_dn, h.DNcat), dev.lnfact = upload(b_lf, h.lnfact);
        for (int q = 0; q < SZ_NQ; q++) dev.qmin[q] = h.qmin[q], dev.qmax[q] = h.qmax[q];
        const float pc[SZ_NPRIORS] = {-0.186f, 1.789f, 0.075f, 0.6666666f, 0.9624f, 0.022f, 0.99f, 0.688f, 0.780f};
        const float ps[SZ_NPRIORS] = {0.021f, 0.084f, 0.01f, 0.5f, 0.014f, 0.002f, 0.19f, 0.072f, 0.092f};
        for (int p = 0; p < SZ_NPRIORS; p++)
            dev.prior_on[p] = h.prior_on[p], dev.prior_c[p] = (double)pc[p], dev.prior_d[p] = sz_two_sq(ps[p]);
        // the constant table, once
        const size_t ne = (size_t)h.nthetas * SZ_NQ * h.nlny;
        b_erfs.alloc(ne * 8), b_slope.alloc(ne * 8);
        dev.erfs = b_erfs.as<double>(), dev.slope = b_slope.as<double>();
        hipLaunchKernelGGL(sz_erfs_kernel, dim3((unsigned)((ne + SZ_THREADS - 1) / SZ_THREADS)), dim3(SZ_THREADS), 0, 0,
                           dev, b_erfs.as<double>(), b_slope.as<double>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
    }

    // The workspace is the completeness table of min(W, SZ_MAXW) walkers and nothing else: float32
    // comp[w][q][j * nm + m], q the S/N bin (SZ_NQ = 5), j the step in z (nzs), m the step in ln M (nm), so
    // 5 * nzs * nm * 4 bytes a walker.  After a call it holds the walkers of the last chunk, slot w0 + w at w
    // (INTEGRATION.md states the same; tests/test_gpu_sz_edges.py reads it).
    size_t ws_floats() const { return (size_t)SZ_NQ * dev.npts; }
    size_t workspace_size(int W) const override {
        if (W <= 0) return 0;
        return ws_floats() * 4 * (size_t)std::min(W, SZ_MAXW);
    }

    void run(int W, const double *dl, long long ld_walker, const double *nuis, long long ld_nuis, double *out, void *ws,
             hipStream_t stream, const int *wcount) {
        if (W <= 0) return;
        nuis = nuisance_rows(nuis, nullptr);
        if (W > 1 && ld_nuis < n_nuis) fail(CMBL_ERR_ARG, "SZ: ld_nuis %lld < %d", ld_nuis, n_nuis);   // one row has no stride
        if (ld_walker != 0 && ld_walker < theory_len)
            fail(CMBL_ERR_ARG, "SZ: ld_walker %lld < the %d doubles of a walker's theory row", ld_walker, theory_len);
        if (!ws) {
            own_ws.grow(workspace_size(W));
            ws = own_ws.p;
        }
        float *comp = static_cast<float *>(ws);
        // batches beyond the workspace's walkers run in chunks, one after another in stream order
        for (int w0 = 0; w0 < W; w0 += SZ_MAXW) {
            const int Wc = std::min(SZ_MAXW, W - w0);
            const double *dlc = dl + (size_t)w0 * ld_walker, *nuc = nuis + (size_t)w0 * ld_nuis;
            timed_launch("sz_compl_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(sz_compl_kernel, dim3((dev.npts + SZ_PTS - 1) / SZ_PTS, Wc), dim3(SZ_THREADS), 0,
                                      stream, e0, e1, 0, dev, dlc, ld_walker, nuc, ld_nuis, comp, wcount, w0);
            });
            HIP_CHECK(hipGetLastError());
            timed_launch("sz_compl0_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(sz_compl0_kernel, dim3((dev.npts + SZ_THREADS - 1) / SZ_THREADS, Wc),
                                      dim3(SZ_THREADS), 0, stream, e0, e1, 0, dev, dlc, ld_walker, nuc, ld_nuis, comp,
                                      wcount, w0);
            });
            HIP_CHECK(hipGetLastError());
            timed_launch("sz_counts_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(sz_counts_kernel, dim3(Wc), dim3(SZ_THREADS), 0, stream, e0, e1, 0, dev, dlc,
                                      ld_walker, nuc, ld_nuis, comp, out, wcount, w0);
            });
            HIP_CHECK(hipGetLastError());
        }
    }

    void loglike_batch(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                       long long ld_nuis, double *out, void *ws, hipStream_t stream) override {
        (void)ld_field;   // one field: the theory row
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

std::unique_ptr<Like> make_sz(const Ini &ini) { return std::unique_ptr<Like>(new SzLike(load_sz(ini))); }

bool sz_info(const Like *like, int *dims) {
    const SzLike *L = dynamic_cast<const SzLike *>(like);
    if (!L) return false;
    const int v[8] = {L->h.nzs, L->h.nm, L->h.Nz, L->h.nq, L->h.nthetas, L->h.npatches, L->h.nlny, L->h.n_cat};
    if (dims) std::copy(v, v + 8, dims);
    return true;
}

bool sz_arrays(const Like *like, double *steps_z, double *dncat, int *j1, int *j2) {
    const SzLike *L = dynamic_cast<const SzLike *>(like);
    if (!L) return false;
    if (steps_z) std::copy(L->h.steps_z.begin(), L->h.steps_z.end(), steps_z);
    if (dncat) std::copy(L->h.DNcat.begin(), L->h.DNcat.end(), dncat);
    if (j1) std::copy(L->h.j1.begin(), L->h.j1.end(), j1);
    if (j2) std::copy(L->h.j2.begin(), L->h.j2.end(), j2);
    return true;
}

}  // namespace cmamd
