// Galaxy power-spectrum likelihoods (source/mpk.f90, source/wigglez.f90; tags
// "MPK" and "WIGGLEZ"): the dataset loaders and the batched f64 evaluation of
// MPK_LnLike (mpk.f90:289-407) and WiggleZ_LnLike (wigglez.f90:524-641).
//
// A walker's theory is one row [a_scl, kh_min, P[nk]] (cosmomc_amd.h): P as the
// provider's PowerAt returns it at max(kh_min, a_scl k_i).  Two launches in
// stream order, shared by both tags ("MPK" is the one-region case):
//   mpk_prologue_kernel  a lane per (k, walker): k_scaled, mpk_lin = P / a_scl^3,
//       the GiggleZ factor 10^fidz(k) / exp(spline(k)) (a bisection into the 500
//       knots, TSpline1D_Value's formula in its order), and the operand vectors:
//       Pth and Pth k^2 (Q_flat), the one Pth (Q_marge = F or Q_sigma = 0), or the
//       13 Pth of the Q grid; into the workspace as [k][vector][walker].  A lane
//       whose inputs the reference would stop on writes NaN, which the walker's
//       column then carries to the tail.
//   mpk_contract_kernel  a workgroup per 16-walker tile, a wave per (region,
//       vector): W_r [np x nk] . Pth [nk x 16 walkers] on v_mfma_f64_16x16x4_f64,
//       16 x 16 tiles kept in registers; the result tiles are the B operands of
//       C_r^-1 [np x np] . (W_r Pth) as they lie (a lane's four results are four
//       k of the second product), so nothing is staged between the two.  Rows,
//       columns and k beyond np, the live walkers and nk are zeros formed in
//       registers: nothing is read past an array.  The dot products are taken
//       per lane in a fixed order and over the four lane groups in a fixed
//       order, one number per (region, vector, walker) into LDS.  Then a thread
//       per walker: regions summed in region order, the 2 x 2 solve or the Q
//       grid, WiggleZ's single-precision normV (kept running over the grid), Q
//       and minchisq, the logs, logZero.
// No atomics, no wait between workgroups; an MFMA column sees only its own
// walker, so a walker's bits depend on neither W, its slot nor the chunking.
//
// Without a cov_file ("MPK" only) C^-1 is the diagonal matrix of 1 / sdev^2, and
// outside Q_flat the reference's tmp = sum(WPth P w) / normV form (:372-375)
// needs W Pth point by point: the contraction stores it for the tail.
#include <cctype>
#include <cmath>
#include <fstream>
#include <set>

#include "mpk.h"

namespace cmamd {

// ------------------------------------------------------------ loader

static bool mpk_logical(const Ini &ini, const std::string &key, bool def) {
    const std::string v = ini.str(key);
    if (v.empty()) return def;
    const char ch = (char)std::toupper(v[0] == '.' && v.size() > 1 ? v[1] : v[0]);
    if (ch == 'T' || ch == '1' || ch == 'Y') return true;
    if (ch == 'F' || ch == '0' || ch == 'N') return false;
    fail(CMBL_ERR_FORMAT, "%s: bad logical %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
}

static int mpk_int(const Ini &ini, const std::string &key, int def) {
    const std::string v = ini.str(key);
    if (v.empty()) return def;
    try {
        return std::stoi(v);
    } catch (const std::exception &) {
        fail(CMBL_ERR_FORMAT, "%s: bad integer %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
    }
}

static double mpk_double(const Ini &ini, const std::string &key, double def) {
    const std::string v = ini.str(key);
    if (v.empty()) return def;
    try {
        return parse_fortran_double(v);
    } catch (const std::exception &) {
        fail(CMBL_ERR_FORMAT, "%s: bad number %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
    }
}

// Read_Real: the value as a single-precision number, widened
static double mpk_real(const Ini &ini, const std::string &key, float def) {
    const std::string v = ini.str(key);
    if (v.empty()) return mpk_f32(def);
    try {
        return mpk_f32(std::stof(fortran_real(v)));
    } catch (const std::exception &) {
        fail(CMBL_ERR_FORMAT, "%s: bad number %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
    }
}

// the lines of a text file that are not blank, each split at white space
static std::vector<std::vector<std::string>> mpk_lines(const std::string &path, bool keep_comments) {
    std::ifstream f(path);
    if (!f) fail(CMBL_ERR_IO, "cannot read %s", path.c_str());
    std::vector<std::vector<std::string>> out;
    std::string line;
    while (std::getline(f, line)) {
        std::vector<std::string> t = split_ws(line);
        if (t.empty()) continue;
        if (!keep_comments && t[0][0] == '#') continue;
        out.push_back(std::move(t));
    }
    return out;
}

static double mpk_number(const std::string &path, const std::string &t) {
    try {
        return parse_fortran_double(t);
    } catch (const std::exception &) {
        fail(CMBL_ERR_FORMAT, "%s: '%s' is not a number", path.c_str(), t.c_str());
    }
}

// File%ReadTextVector / ReadTextMatrix: the first n numbers of the first m data lines
static std::vector<double> mpk_matrix(const std::string &path, int m, int n) {
    const auto rows = mpk_lines(path, false);
    if ((int)rows.size() < m) fail(CMBL_ERR_FORMAT, "%s holds %zu rows, fewer than %d", path.c_str(), rows.size(), m);
    std::vector<double> out((size_t)m * n);
    for (int i = 0; i < m; i++) {
        if ((int)rows[i].size() < n)
            fail(CMBL_ERR_FORMAT, "%s: row %d holds %zu numbers, fewer than %d", path.c_str(), i + 1, rows[i].size(), n);
        for (int j = 0; j < n; j++) out[(size_t)i * n + j] = mpk_number(path, rows[i][j]);
    }
    return out;
}

// ReadWiggleZMatrices (wigglez.f90:439-471): a comment line, then m rows of n numbers, for every region
static std::vector<double> mpk_region_matrices(const std::string &path, int nreg, int m, int n) {
    const auto rows = mpk_lines(path, true);
    if ((int)rows.size() < nreg * (m + 1))
        fail(CMBL_ERR_FORMAT, "%s holds %zu lines, fewer than %d regions x (1 + %d)", path.c_str(), rows.size(), nreg, m);
    std::vector<double> out((size_t)nreg * m * n);
    for (int r = 0; r < nreg; r++)
        for (int i = 0; i < m; i++) {
            const auto &t = rows[(size_t)r * (m + 1) + 1 + i];
            if ((int)t.size() < n)
                fail(CMBL_ERR_FORMAT, "%s: region %d row %d holds %zu numbers, fewer than %d", path.c_str(), r + 1, i + 1,
                     t.size(), n);
            for (int j = 0; j < n; j++) out[((size_t)r * m + i) * n + j] = mpk_number(path, t[j]);
        }
    return out;
}

// Matrix_Inverse (dpotrf 'L', dpotri 'L', mirrored) of a symmetric positive
// definite block, the sums taken in extended precision
static void mpk_chol_inverse(const std::string &what, std::vector<double> &M, int n) {
    std::vector<long double> L((size_t)n * n, 0.0L), Li((size_t)n * n, 0.0L);
    for (int j = 0; j < n; j++) {
        long double d = M[(size_t)j * n + j];
        for (int k = 0; k < j; k++) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0)) fail(CMBL_ERR_NUMERIC, "%s: the covariance is not positive definite", what.c_str());
        L[(size_t)j * n + j] = sqrtl(d);
        for (int i = j + 1; i < n; i++) {
            long double s = M[(size_t)i * n + j];
            for (int k = 0; k < j; k++) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = s / L[(size_t)j * n + j];
        }
    }
    for (int j = 0; j < n; j++) {
        Li[(size_t)j * n + j] = 1.0L / L[(size_t)j * n + j];
        for (int i = j + 1; i < n; i++) {
            long double s = 0.0L;
            for (int k = j; k < i; k++) s -= L[(size_t)i * n + k] * Li[(size_t)k * n + j];
            Li[(size_t)i * n + j] = s / L[(size_t)i * n + i];
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j <= i; j++) {
            long double s = 0.0L;
            for (int k = i; k < n; k++) s += Li[(size_t)k * n + i] * Li[(size_t)k * n + j];
            M[(size_t)i * n + j] = M[(size_t)j * n + i] = (double)s;
        }
}

// spline (Interpolation.f90:693-734) with both ends natural
static std::vector<double> mpk_spline(const std::vector<double> &x, const std::vector<double> &y) {
    const int n = (int)x.size();
    std::vector<double> d2(n, 0.0), u(n, 0.0);
    double d1r = (y[1] - y[0]) / (x[1] - x[0]);
    for (int i = 1; i < n - 1; i++) {
        const double d1l = d1r;
        d1r = (y[i + 1] - y[i]) / (x[i + 1] - x[i]);
        const double xxdiv = 1.0 / (x[i + 1] - x[i - 1]);
        const double sig = (x[i] - x[i - 1]) * xxdiv;
        const double xp = 1.0 / (sig * d2[i - 1] + 2.0);
        d2[i] = (sig - 1.0) * xp;
        u[i] = (6.0 * (d1r - d1l) * xxdiv - sig * u[i - 1]) * xp;
    }
    d2[n - 1] = 0.0;
    for (int i = n - 2; i >= 0; i--) d2[i] = d2[i] * d2[i + 1] + u[i];
    return d2;
}

MpkData load_mpk(const Ini &ini, bool wigglez) {
    static const char *region_keys[MPK_MAXR] = {"Use_9-hr_region", "Use_11-hr_region", "Use_15-hr_region",
                                                "Use_22-hr_region", "Use_1-hr_region", "Use_3-hr_region",
                                                "Use_0-hr_region"};   // the reference's key order (wigglez.f90:234-251)
    static const double zeval[4] = {0.22, 0.41, 0.6, 0.78};
    const char *what = wigglez ? "WiggleZ" : "MPK";
    std::set<std::string> served = {"name", "num_mpk_points_full", "num_mpk_kbands_full", "min_mpk_points_use",
                                    "max_mpk_points_use", "min_mpk_kbands_use", "max_mpk_kbands_use", "kbands_file",
                                    "measurements_file", "windows_file", "cov_file", "use_scaling", "DV_fid", "redshift",
                                    "Q_marge", "Q_flat", "Q_mid", "Q_sigma", "Ag", "num_conflicts", "type_conflict1",
                                    "name_conflict1"};
    if (wigglez) {
        for (const char *k : region_keys) served.insert(k);
        served.insert("Use_gigglez"), served.insert("nonlinear_wigglez"), served.insert("gigglez_dir");
    } else {
        served.insert("mpk_dataset_nonlinear");
    }
    for (const std::string &k : ini.keys())
        if (!served.count(k)) fail(CMBL_ERR_UNSUPPORTED, "%s: key %s is not supported", what, k.c_str());
    MpkData d;
    d.wigglez = wigglez;
    d.name = ini.str("name");
    if (d.name == "twodf" || d.name == "lrg_2009")
        fail(CMBL_ERR_UNSUPPORTED, "%s: %s is not supported (the reference stops on it)", what, d.name.c_str());
    const int npf = mpk_int(ini, "num_mpk_points_full", 0), nkf = mpk_int(ini, "num_mpk_kbands_full", 0);
    if (npf <= 0 || nkf <= 0) fail(CMBL_ERR_FORMAT, "%s: num_mpk_points_full and num_mpk_kbands_full must be set", what);
    const int minp = mpk_int(ini, "min_mpk_points_use", 1), maxp = mpk_int(ini, "max_mpk_points_use", npf);
    const int mink = mpk_int(ini, "min_mpk_kbands_use", 1), maxk = mpk_int(ini, "max_mpk_kbands_use", nkf);
    if (minp < 1 || maxp < minp || maxp > npf || mink < 1 || maxk < mink || maxk > nkf)
        fail(CMBL_ERR_FORMAT, "%s: the points %d..%d of %d or the kbands %d..%d of %d are no selection", what, minp, maxp,
             npf, mink, maxk, nkf);
    const int np = d.np = maxp - minp + 1, nk = d.nk = maxk - mink + 1;
    if (np > MPK_MAXP) fail(CMBL_ERR_UNSUPPORTED, "%s: %d points used, more than %d", what, np, MPK_MAXP);

    std::vector<int> regions;   // 0-based regions in use
    if (wigglez) {
        for (int r = 0; r < MPK_MAXR; r++)
            if (mpk_logical(ini, region_keys[r], false)) regions.push_back(r);
        if (regions.empty()) fail(CMBL_ERR_FORMAT, "WiggleZ_mpk: no regions being used in this data set");
        d.use_gigglez = mpk_logical(ini, "Use_gigglez", false);
        d.nonlinear = mpk_logical(ini, "nonlinear_wigglez", false);
        if (d.use_gigglez && !d.nonlinear)
            fail(CMBL_ERR_FORMAT, "WiggleZ: the GiggleZ prescription needs nonlinear_wigglez = T");
        d.redshift = mpk_double(ini, "redshift", 0.0);
        if (d.redshift == 0.0) fail(CMBL_ERR_FORMAT, "WiggleZMPK: failed to read in WiggleZ redshift");
        for (int i = 0; i < 4; i++)
            if (std::fabs(d.redshift - zeval[i]) <= 0.001) d.zbin = i + 1;
        if (d.zbin == 0) fail(CMBL_ERR_FORMAT, "WiggleZMPK: could not identify redshift %g", d.redshift);
    } else {
        regions.push_back(0);
        d.nonlinear = mpk_logical(ini, "mpk_dataset_nonlinear", false);
        d.redshift = mpk_double(ini, "redshift", 0.35);
    }
    const int nr = d.nr = (int)regions.size();

    d.use_scaling = mpk_logical(ini, "use_scaling", false);
    if (d.use_scaling) {
        d.DV_fid = mpk_double(ini, "DV_fid", -1.0);
        if (d.DV_fid == -1.0)
            fail(CMBL_ERR_FORMAT, "%s: use_scaling = T and no DV_fid given for dataset %s", what, d.name.c_str());
    }
    d.q_marge = mpk_logical(ini, "Q_marge", false);
    if (d.q_marge) {
        const bool flat = mpk_logical(ini, "Q_flat", false);
        if (!flat) {
            if (!ini.has("Q_mid") || !ini.has("Q_sigma"))
                fail(CMBL_ERR_FORMAT, "%s: Q_marge = T without Q_flat needs Q_mid and Q_sigma", what);
            d.Q_mid = mpk_real(ini, "Q_mid", 0.f), d.Q_sigma = mpk_real(ini, "Q_sigma", 0.f);
        }
        d.Ag = mpk_real(ini, "Ag", 1.4f);
        d.q_mode = flat ? MPK_Q_FLAT : d.Q_sigma == 0 ? MPK_Q_POINT : MPK_Q_GAUSS;
    }

    {
        const std::vector<double> kfull = mpk_matrix(ini.relative_filename("kbands_file", true), nkf, 1);
        d.k.assign(kfull.begin() + (mink - 1), kfull.begin() + maxk);
    }
    d.P.resize((size_t)nr * np);
    const std::string mfile = ini.relative_filename("measurements_file", true);
    const auto mrows = mpk_lines(mfile, true);
    if (!wigglez) {
        // two header lines, the rows below min skipped; columns keff klo khi P sdev fiducial
        d.sdev.resize(np);
        if ((int)mrows.size() < 2 + maxp) fail(CMBL_ERR_FORMAT, "Error reading mpk file %s", mfile.c_str());
        for (int i = 0; i < np; i++) {
            const auto &t = mrows[2 + (minp - 1) + i];
            if (t.size() < 6) fail(CMBL_ERR_FORMAT, "Error reading mpk file %s", mfile.c_str());
            d.P[i] = mpk_number(mfile, t[3]), d.sdev[i] = mpk_number(mfile, t[4]);
        }
    } else {
        // per region two comment lines, then num_mpk_points_full rows (an active region) or 50 (:345-378)
        size_t at = 0;
        int count = 0;
        for (int r = 0; r < MPK_MAXR; r++) {
            const bool active = std::find(regions.begin(), regions.end(), r) != regions.end();
            const int rows = active ? npf : 50;
            if (mrows.size() < at + 2 + rows) fail(CMBL_ERR_FORMAT, "Error reading WiggleZ mpk file %s", mfile.c_str());
            if (active) {
                for (int i = 0; i < np; i++) {
                    const auto &t = mrows[at + 2 + (minp - 1) + i];
                    if (t.size() < 6) fail(CMBL_ERR_FORMAT, "Error reading WiggleZ mpk file %s", mfile.c_str());
                    d.P[(size_t)count * np + i] = mpk_number(mfile, t[3]);
                }
                count++;
            }
            at += 2 + rows;
        }
    }

    const std::string wfile = ini.relative_filename("windows_file", true);
    const std::vector<double> wfull = wigglez ? mpk_region_matrices(wfile, MPK_MAXR, npf, nkf) : mpk_matrix(wfile, npf, nkf);
    d.W.resize((size_t)nr * np * nk);
    for (int c = 0; c < nr; c++)
        for (int i = 0; i < np; i++)
            for (int j = 0; j < nk; j++)
                d.W[((size_t)c * np + i) * nk + j] = wfull[((size_t)regions[c] * npf + (minp - 1 + i)) * nkf + (mink - 1 + j)];

    d.invcov.assign((size_t)nr * np * np, 0.0);
    const std::string cfile = ini.relative_filename("cov_file", false);
    if (!cfile.empty()) {
        d.has_cov = true;
        const std::vector<double> cfull = wigglez ? mpk_region_matrices(cfile, MPK_MAXR, npf, npf) : mpk_matrix(cfile, npf, npf);
        for (int c = 0; c < nr; c++) {
            std::vector<double> blk((size_t)np * np);
            for (int i = 0; i < np; i++)
                for (int j = 0; j < np; j++)
                    blk[(size_t)i * np + j] = cfull[((size_t)regions[c] * npf + (minp - 1 + i)) * npf + (minp - 1 + j)];
            mpk_chol_inverse(d.name + " " + cfile, blk, np);
            std::copy(blk.begin(), blk.end(), d.invcov.begin() + (size_t)c * np * np);
        }
    } else {
        if (wigglez) fail(CMBL_ERR_FORMAT, "WiggleZ: cov_file is missing");   // WiggleZ_LnLike reads mpk_invcov unconditionally
        for (int i = 0; i < np; i++) d.invcov[(size_t)i * np + i] = 1 / (d.sdev[i] * d.sdev[i]);
    }

    if (d.use_gigglez) {
        static const char *names = "abcd";
        std::string dir = ini.str("gigglez_dir");
        if (dir.empty()) dir = dirname_of(ini.filename());
        if (!dir.empty() && dir.back() != '/') dir += '/';
        const std::string gfile = dir + "gigglezfiducialmodel_matterpower_" + names[d.zbin - 1] + ".dat";
        const auto rows = mpk_lines(gfile, false);
        if ((int)rows.size() < MPK_GIGGLEZ_NUMK) fail(CMBL_ERR_FORMAT, "Error reading model or fiducial theory file %s", gfile.c_str());
        for (int i = 0; i < MPK_GIGGLEZ_NUMK; i++) {
            if (rows[i].size() < 2) fail(CMBL_ERR_FORMAT, "Error reading model or fiducial theory file %s", gfile.c_str());
            d.gk.push_back(mpk_number(gfile, rows[i][0]));
            const double p = mpk_number(gfile, rows[i][1]);
            if (!(p > 0) || (i > 0 && !(d.gk[i] > d.gk[i - 1])))
                fail(CMBL_ERR_FORMAT, "%s: row %d is no knot of ln P over rising k", gfile.c_str(), i + 1);
            d.gf.push_back(std::log(p));
        }
        d.gdd = mpk_spline(d.gk, d.gf);
    }
    return d;
}

// ------------------------------------------------------------ kernels

static constexpr int MPK_THREADS = 256;   // 4 waves
static constexpr int MPK_MAXW = 1024;     // walkers per launch (workspace_size)
static constexpr int MPK_NRES = 3;        // numbers a (region, vector, walker) leaves: covth.WPth, covdat.WPth, covth.WPth_k2

typedef double mpk_f64x4 __attribute__((ext_vector_type(4)));

struct MpkDev {
    int np, nk, nr, nv, npt;              // points, kbands, regions, operand vectors per walker, 16-row tiles of np
    int flat, q_marge, wigglez, gig, ngk, tmp_form;
    const double *k, *W, *Ci, *covdat, *P, *w, *gk, *gf, *gdd;
    double pcd;                           // sum(P covdat) over every region's points, in their order
    double Ag;
    double Q[MPK_NV], cw[MPK_NV], cwsum;  // Q and calweights of the grid points, sum(calweights)
    double gc[6];                         // the bin's GiggleZ polynomial, lowest order first
};

__global__ __launch_bounds__(MPK_THREADS) void mpk_prologue_kernel(MpkDev d, const double *__restrict__ dl,
                                                                   long long ld_walker, double *__restrict__ ops, int Wc,
                                                                   int Wp, const int *__restrict__ wcount, int w0)
{
    const long long idx = (long long)blockIdx.x * MPK_THREADS + threadIdx.x;
    if (idx >= (long long)d.nk * Wp) return;
    const int k = (int)(idx / Wp), w = (int)(idx - (long long)k * Wp);
    if (w >= Wc || (wcount && w0 + w >= *wcount)) return;
    const double *row = dl + (size_t)w * ld_walker;
    const double a = row[0], khmin = row[1], P = row[2 + k];
    const double big = 1.79769313486231570e308;
    bool ok = fabs(a) <= big && fabs(khmin) <= big && fabs(P) <= big && a > 0.0;
    const double ak = a * d.k[k];
    const double ks = ak > khmin ? ak : khmin;       // max(exp(PK%x(1)), a_scl k)
    double lin = P / (a * a * a);
    if (d.gig && ok) {
        const int n = d.ngk;
        const double tol = (d.gk[1] - d.gk[0]) * 1.e-5;
        if (ks < d.gk[0] - tol || ks > d.gk[n - 1]) {
            ok = false;                              // outside the spline: the reference stops
        } else {
            const double k2 = ks * ks, k3 = k2 * ks, k4 = k2 * k2, k5 = k4 * ks;
            const double fidz = d.gc[0] + d.gc[1] * ks + d.gc[2] * k2 + d.gc[3] * k3 + d.gc[4] * k4 + d.gc[5] * k5;
            int lo = 0, hi = n - 1;                  // X(lo) < ks <= X(lo + 1), as FindNext leaves llo
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (d.gk[mid] < ks) lo = mid;
                else hi = mid;
            }
            const double xlo = d.gk[lo], xhi = d.gk[lo + 1], ho = xhi - xlo;
            const double a0 = (xhi - ks) / ho, b0 = 1.0 - a0;
            const double s = b0 * d.gf[lo + 1] +
                             a0 * (d.gf[lo] - b0 * ((a0 + 1.0) * d.gdd[lo] + (2.0 - a0) * d.gdd[lo + 1]) * (ho * ho) / 6.0);
            lin = lin * pow(10.0, fidz) / exp(s);
        }
    }
    double *o = ops + (size_t)k * d.nv * Wp + w;
    if (!ok) {
        for (int v = 0; v < d.nv; v++) o[(size_t)v * Wp] = __builtin_nan("");
        return;
    }
    if (d.flat) {
        const double pth = lin / (1.0 + d.Ag * ks);
        o[0] = pth;
        o[Wp] = pth * (ks * ks);
    } else if (d.q_marge) {
        for (int v = 0; v < d.nv; v++) o[(size_t)v * Wp] = lin * (1.0 + d.Q[v] * (ks * ks)) / (1.0 + d.Ag * ks);
    } else {
        o[0] = lin;
    }
}

// One (region, first vector) of a 16-walker tile: NV operand vectors through both products, then the dots.
template <int NV>
__device__ __forceinline__ void mpk_task(const MpkDev &d, const double *__restrict__ ops, int Wp, int wl, bool colok, int r,
                                         int v0, int lane, double *s_res, double *__restrict__ wp_out)
{
    const int c = lane & 15, g = lane >> 4, np = d.np, nk = d.nk, npt = d.npt;
    const double *Wr = d.W + (size_t)r * np * nk, *Cr = d.Ci + (size_t)r * np * np;
    mpk_f64x4 acc[NV][4], ct[NV][4];
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
        for (int pt = 0; pt < 4; pt++) acc[j][pt] = mpk_f64x4{0.0, 0.0, 0.0, 0.0}, ct[j][pt] = mpk_f64x4{0.0, 0.0, 0.0, 0.0};
    // W_r . Pth: a lane feeds 4 consecutive k of its row; the k of instruction q are k0 + 4 g + q in both operands
    for (int k0 = 0; k0 < nk; k0 += 16) {
        const int kb = k0 + 4 * g;
        double b[NV][4];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < NV; j++)
                b[j][q] = (colok && kb + q < nk) ? ops[((size_t)(kb + q) * d.nv + v0 + j) * Wp + wl] : 0.0;
#pragma unroll
        for (int pt = 0; pt < 4; pt++) {
            if (pt < npt) {
                const int row = 16 * pt + c;
                const double *wr = Wr + (size_t)(row < np ? row : 0) * nk;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const double a = (row < np && kb + q < nk) ? wr[kb + q] : 0.0;
#pragma unroll
                    for (int j = 0; j < NV; j++) acc[j][pt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j][q], acc[j][pt], 0, 0, 0);
                }
            }
        }
    }
    // C_r^-1 . (W_r Pth): result q of tile pt is row 16 pt + g + 4 q of W_r Pth -- the k of instruction q
#pragma unroll
    for (int po = 0; po < 4; po++) {
        if (po < npt) {
            const int row = 16 * po + c;
            const double *cr = Cr + (size_t)(row < np ? row : 0) * np;
#pragma unroll
            for (int pt = 0; pt < 4; pt++) {
                if (pt < npt) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int col = 16 * pt + g + 4 * q;
                        const double a = (row < np && col < np) ? cr[col] : 0.0;
#pragma unroll
                        for (int j = 0; j < NV; j++)
                            ct[j][po] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, acc[j][pt][q], ct[j][po], 0, 0, 0);
                    }
                }
            }
        }
    }
    // the dots: a lane's rows in rising order, then the four lane groups in rising order
    double s[NV][MPK_NRES];
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
        for (int i = 0; i < MPK_NRES; i++) s[j][i] = 0.0;
#pragma unroll
    for (int pt = 0; pt < 4; pt++) {
        if (pt < npt) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int rho = 16 * pt + g + 4 * q;
                const double cd = rho < np ? d.covdat[(size_t)r * np + rho] : 0.0;
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    s[j][0] = s[j][0] + ct[j][pt][q] * acc[j][pt][q];
                    s[j][1] = s[j][1] + cd * acc[j][pt][q];
                }
                if (NV == 2) s[0][2] = s[0][2] + ct[0][pt][q] * acc[1][pt][q];
                if (wp_out && rho < np && colok) wp_out[((size_t)v0 * np + rho) * 16 + c] = acc[0][pt][q];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
        for (int i = 0; i < MPK_NRES; i++) {
            const double x = s[j][i];
            double t = __shfl(x, c, 64);
            t = t + __shfl(x, c + 16, 64);
            t = t + __shfl(x, c + 32, 64);
            t = t + __shfl(x, c + 48, 64);
            if (g == 0) s_res[(((size_t)r * d.nv + v0 + j) * MPK_NRES + i) * 16 + c] = t;
        }
}

__global__ __launch_bounds__(MPK_THREADS) void mpk_contract_kernel(MpkDev d, const double *__restrict__ ops,
                                                                   double *__restrict__ wpbuf, double *__restrict__ out,
                                                                   int Wc, int Wp, const int *__restrict__ wcount, int w0)
{
    __shared__ double s_res[MPK_MAXR * MPK_NV * MPK_NRES * 16];
    __shared__ double s_chi[MPK_NV * 16];
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nlive = Wc;
    if (wcount) nlive = min(Wc, *wcount - w0);
    if (tile * 16 >= nlive) return;
    const int wl = tile * 16 + (lane & 15);
    const bool colok = wl < nlive;
    double *wp_tile = d.tmp_form ? wpbuf + (size_t)tile * d.nv * d.np * 16 : nullptr;
    if (d.flat) {
        for (int r = wave; r < d.nr; r += MPK_THREADS / 64) mpk_task<2>(d, ops, Wp, wl, colok, r, 0, lane, s_res, nullptr);
    } else {
        for (int t = wave; t < d.nr * d.nv; t += MPK_THREADS / 64)
            mpk_task<1>(d, ops, Wp, wl, colok, t / d.nv, t % d.nv, lane, s_res, wp_tile);
    }
    __syncthreads();   // s_res (and the tile's W Pth in wpbuf) are there for the tail
    if (tid >= 16 || tile * 16 + tid >= nlive) return;
    const int c = tid;
    auto res = [&](int r, int v, int i) { return s_res[(((size_t)r * d.nv + v) * MPK_NRES + i) * 16 + c]; };
    const double big = 1.79769313486231570e308;
    double lnl;
    bool bad = false;
    if (d.flat) {
        // Mat, vec2 summed over the regions before the log and the inverse (mpk.f90:339-347, wigglez.f90:556-583)
        double M11 = 0.0, M22 = 0.0, M12 = 0.0, v1 = 0.0, v2 = 0.0;
        for (int r = 0; r < d.nr; r++) {
            M11 = M11 + res(r, 0, 0), M22 = M22 + res(r, 1, 0), M12 = M12 + res(r, 0, 2);
            v1 = v1 + res(r, 0, 1), v2 = v2 + res(r, 1, 1);
        }
        const double det = M11 * M22 - M12 * M12;
        bad = !(det > 0.0) || !(M11 >= 1.e-30) || !(M22 >= 1.e-30);
        // Matrix_Inverse: dpotrf 'L', dpotri 'L'
        const double L11 = sqrt(M11), L21 = M12 / L11, dd = M22 - L21 * L21;
        bad = bad || !(dd > 0.0);
        const double L22 = sqrt(dd), i11 = 1.0 / L11, i22 = 1.0 / L22, i21 = -(L21 * i11) * i22;
        const double A11 = i11 * i11 + i21 * i21, A21 = i22 * i21, A22 = i22 * i22;
        const double quad = v1 * (A11 * v1 + A21 * v2) + v2 * (A21 * v1 + A22 * v2);
        lnl = (d.pcd - quad + log(det)) / 2.0;
    } else {
        float normVf = 0.f;                      // WiggleZ: real, and not reset between the grid points
        double mn = 0.0;
        for (int v = 0; v < d.nv; v++) {
            double sn = 0.0, sd = 0.0;
            for (int r = 0; r < d.nr; r++) sn = sn + res(r, v, 0), sd = sd + res(r, v, 1);
            double chi;
            if (d.wigglez) {
                normVf = (float)((double)normVf + sn);
                const double nv = (double)normVf;
                bad = bad || !(nv > 0.0);
                chi = d.pcd - sd * sd / nv;
            } else if (!d.tmp_form) {
                bad = bad || !(sn > 0.0);
                chi = d.pcd - sd * sd / sn + log(sn);
            } else {
                bad = bad || !(sn > 0.0);
                const double tmp = sd / sn;      // avoid subtracting one large number from another (:374)
                const double *wp = wp_tile + (size_t)v * d.np * 16 + c;
                double sum = 0.0;
                for (int p = 0; p < d.np; p++) sum = sum + d.P[p] * (d.P[p] - wp[(size_t)p * 16] * tmp) * d.w[p];
                chi = sum + log(sn);
            }
            s_chi[v * 16 + c] = chi;
            mn = (v == 0 || chi < mn) ? chi : mn;
        }
        if (d.nv == 1) {
            lnl = s_chi[c] / 2.0;
        } else {
            const float mnf = (float)mn;         // WiggleZ: minchisq is real
            const double m = d.wigglez ? (double)mnf : mn;
            double sum = 0.0;
            for (int v = 0; v < d.nv; v++) sum = sum + exp(-(s_chi[v * 16 + c] - m) / 2.0) * d.cw[v];
            const double like = sum / d.cwsum;
            if (like == 0.0) bad = true;
            lnl = -log(like) + (d.wigglez ? (double)(mnf / 2.f) : m / 2.0);
        }
    }
    if (bad || !(fabs(lnl) <= big)) lnl = CMBL_LOGZERO;
    out[w0 + tile * 16 + c] = lnl;
}

// ------------------------------------------------------------ likelihood

struct MpkLike : Like {
    MpkData h;
    MpkDev dev{};
    DevBuf b_k, b_W, b_Ci, b_cd, b_P, b_w, b_gk, b_gf, b_gdd;

    explicit MpkLike(MpkData &&data) : h(std::move(data)) {
        name = h.name;
        tag = h.wigglez ? "WIGGLEZ" : "MPK";
        n_nuis = 0;
        speed = 0;   // TDataLikelihood's default; neither *_Add sets one
        theory_len = 2 + h.nk;
        const int np = h.np;
        dev.np = np, dev.nk = h.nk, dev.nr = h.nr, dev.npt = (np + 15) / 16;
        dev.flat = h.q_mode == MPK_Q_FLAT, dev.q_marge = h.q_marge, dev.wigglez = h.wigglez;
        dev.nv = dev.flat ? 2 : h.q_mode == MPK_Q_GAUSS ? MPK_NV : 1;
        dev.tmp_form = !h.wigglez && !h.has_cov && !dev.flat;
        dev.gig = h.use_gigglez, dev.ngk = (int)h.gk.size();
        dev.Ag = h.Ag;
        const double dQ = mpk_f32(0.4f);
        dev.cwsum = 0.0;
        for (int v = 0; v < MPK_NV; v++) {
            const int iQ = v - MPK_NQ;
            const double Q = h.Q_mid + iQ * h.Q_sigma * dQ;
            dev.Q[v] = h.wigglez ? (double)(float)Q : Q;          // WiggleZ_LnLike declares Q real
            const double x = iQ * dQ;
            dev.cw[v] = std::exp(-(x * x) / 2);
            dev.cwsum = dev.cwsum + dev.cw[v];
        }
        if (h.use_gigglez) {
            static const double poly[4][6] = {
                // log10 of the GiggleZ-to-initial-conditions ratio per bin (Parkinson et al. 2012, arXiv:1210.2130)
                {4.619, -13.7787, 58.941, -175.24, 284.321, -187.284},
                {4.63079, -12.6293, 42.9265, -91.8068, 97.808, -37.633},
                {4.69659, -12.7287, 42.5681, -89.5578, 96.664, -mpk_f32(41.2564f)},
                {4.6849, -13.4747, 53.7172, -145.832, 216.638, -mpk_f32(132.782f)}};
            for (int i = 0; i < 6; i++) dev.gc[i] = poly[h.zbin - 1][i];
        }
        // covdat = C^-1 P (or P w) and sum(P covdat), once
        std::vector<double> covdat((size_t)h.nr * np), w;
        double pcd = 0.0;
        for (int r = 0; r < h.nr; r++)
            for (int i = 0; i < np; i++) {
                double s = 0.0;
                if (h.has_cov) {
                    for (int j = 0; j < np; j++) s = s + h.invcov[((size_t)r * np + i) * np + j] * h.P[(size_t)r * np + j];
                } else {
                    s = h.P[i] * h.invcov[(size_t)i * np + i];
                }
                covdat[(size_t)r * np + i] = s;
            }
        for (size_t i = 0; i < covdat.size(); i++) pcd = pcd + h.P[i] * covdat[i];
        dev.pcd = pcd;
        if (!h.has_cov)
            for (int i = 0; i < np; i++) w.push_back(h.invcov[(size_t)i * np + i]);
        dev.k = upload(b_k, h.k), dev.W = upload(b_W, h.W), dev.Ci = upload(b_Ci, h.invcov);
        dev.covdat = upload(b_cd, covdat), dev.P = upload(b_P, h.P), dev.w = upload(b_w, w);
        dev.gk = upload(b_gk, h.gk), dev.gf = upload(b_gf, h.gf), dev.gdd = upload(b_gdd, h.gdd);
    }

    static int padded(int W) { return (std::min(W, MPK_MAXW) + 15) / 16 * 16; }
    size_t ops_doubles(int Wp) const { return (size_t)dev.nk * dev.nv * Wp; }
    size_t workspace_size(int W) const override {
        if (W <= 0) return 0;
        const int Wp = padded(W);
        return (ops_doubles(Wp) + (dev.tmp_form ? (size_t)dev.nv * dev.np * Wp : 0)) * 8;
    }

    void run(int W, const double *dl, long long ld_walker, double *out, void *ws, hipStream_t stream, const int *wcount) {
        if (W <= 0) return;
        if (ld_walker != 0 && ld_walker < theory_len)
            fail(CMBL_ERR_ARG, "%s: ld_walker %lld < the %d doubles of a walker's theory row", tag.c_str(), ld_walker,
                 theory_len);
        if (!ws) {
            own_ws.grow(workspace_size(W));
            ws = own_ws.p;
        }
        const int Wp = padded(W);
        double *ops = static_cast<double *>(ws), *wpbuf = ops + ops_doubles(Wp);
        // batches beyond the workspace's walkers run in chunks, one after another in stream order
        for (int w0 = 0; w0 < W; w0 += MPK_MAXW) {
            const int Wc = std::min(MPK_MAXW, W - w0);
            const double *dlc = dl + (size_t)w0 * ld_walker;
            const unsigned nblk = (unsigned)(((size_t)dev.nk * Wp + MPK_THREADS - 1) / MPK_THREADS);
            timed_launch("mpk_prologue_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(mpk_prologue_kernel, dim3(nblk), dim3(MPK_THREADS), 0, stream, e0, e1, 0, dev, dlc,
                                      ld_walker, ops, Wc, Wp, wcount, w0);
            });
            HIP_CHECK(hipGetLastError());
            timed_launch("mpk_contract_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(mpk_contract_kernel, dim3((Wc + 15) / 16), dim3(MPK_THREADS), 0, stream, e0, e1, 0,
                                      dev, ops, wpbuf, out, Wc, Wp, wcount, w0);
            });
            HIP_CHECK(hipGetLastError());
        }
    }

    void loglike_batch(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                       long long ld_nuis, double *out, void *ws, hipStream_t stream) override {
        (void)ld_field, (void)nuis, (void)ld_nuis;   // one field: the theory row; no nuisance parameters
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

std::unique_ptr<Like> make_mpk(const Ini &ini, bool wigglez) {
    return std::unique_ptr<Like>(new MpkLike(load_mpk(ini, wigglez)));
}

bool mpk_info(const Like *like, int *dims) {
    const MpkLike *L = dynamic_cast<const MpkLike *>(like);
    if (!L) return false;
    const int v[8] = {L->h.np, L->h.nk, L->h.nr, L->h.zbin, L->h.q_mode, L->h.has_cov, L->h.use_scaling, L->h.use_gigglez};
    if (dims) std::copy(v, v + 8, dims);
    return true;
}

bool mpk_arrays(const Like *like, double *k, double *data, double *invcov) {
    const MpkLike *L = dynamic_cast<const MpkLike *>(like);
    if (!L) return false;
    if (k) std::copy(L->h.k.begin(), L->h.k.end(), k);
    if (data) std::copy(L->h.P.begin(), L->h.P.end(), data);
    if (invcov) std::copy(L->h.invcov.begin(), L->h.invcov.end(), invcov);
    return true;
}

}  // namespace cmamd
