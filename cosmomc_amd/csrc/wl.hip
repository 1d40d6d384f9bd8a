// DES-format weak-lensing and galaxy-clustering likelihood (source/wl.f90): the
// dataset loader (WL_ReadIni :104-299, init_bessel_integration :320-369) and
// the batched f64 evaluation of calc_theory / cl2corr / WL_LnLike (:301-653).
//
// A walker's theory is one row [h, omm, chis[nz], Hs[nz], D_growth[nz],
// P[nl][nz]] (cosmomc_amd.h).  Per walker, one workgroup each:
//   wl_kernel_q     n_chi, qgal and qs (:486-530) from the row and the nuisance
//                   values: a lane per z for the knot search and the spline, the
//                   O(nz^2) lensing-efficiency sum done literally;
//   wl_kernel_corr  the Limber sums (:549-597) as a [nl x nz] . [nz x columns]
//                   product on v_mfma_f64_16x16x4_f64, then the used entries of
//                   xi+- / gamma_t / w(theta) from the operator formed at open,
//                   times the (1 + m) factors, minus the data vector;
// then the shared quadratic form (quadform.hip) and wl_kernel_finish, which
// turns a non-finite -lnL into logZero.  cl2corr's natural spline in l (fixed
// knots) and its Bessel sum are both linear in C_l: their product is formed
// once at open, in long double, as one [l][theta] operator per Bessel order,
// and only the used (pair, theta) entries are contracted with it.
// Every sum of the three kernels here has a fixed order and none of them uses
// atomics or waits for another workgroup (the shared quadratic form combines
// its split-K partials behind arrival counters, in a fixed order of its own),
// so a walker's bits do not depend on W, its slot, ld_walker or the chunking.
#include <cmath>
#include <fstream>
#include <set>

#include "quadform.h"
#include "wl.h"

namespace cmamd {

// ------------------------------------------------------------ loader

static const char *WL_TYPE_NAMES[WL_NTYPES] = {"xip", "xim", "gammat", "wtheta"};

static int wl_type(const std::string &s) {
    for (int t = 0; t < WL_NTYPES; t++)
        if (s == WL_TYPE_NAMES[t]) return t;
    return -1;
}

static bool wl_logical(const Ini &ini, const std::string &key, bool def) {
    const std::string v = ini.str(key);
    if (v.empty()) return def;
    const char ch = (char)std::toupper(v[0] == '.' && v.size() > 1 ? v[1] : v[0]);
    if (ch == 'T' || ch == '1' || ch == 'Y') return true;
    if (ch == 'F' || ch == '0' || ch == 'N') return false;
    fail(CMBL_ERR_FORMAT, "%s: bad logical %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
}

static double wl_double(const Ini &ini, const std::string &key, double def) {
    const std::string v = ini.str(key);
    if (v.empty()) return def;
    try {
        size_t used = 0;
        const double r = std::stod(fortran_real(v), &used);
        if (used != v.size()) throw std::invalid_argument(v);
        return r;
    } catch (const std::exception &) {
        fail(CMBL_ERR_FORMAT, "%s: bad number %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
    }
}

static int wl_int(const Ini &ini, const std::string &key, int def) {
    const std::string v = ini.str(key);
    if (v.empty()) return def;
    try {
        size_t used = 0;
        const int r = std::stoi(v, &used);
        if (used != v.size()) throw std::invalid_argument(v);
        return r;
    } catch (const std::exception &) {
        fail(CMBL_ERR_FORMAT, "%s: bad integer %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
    }
}

static std::vector<int> wl_type_list(const Ini &ini, const std::string &key) {
    std::vector<int> out;
    for (const std::string &s : split_ws(ini.str_required(key))) {
        const int t = wl_type(s);
        if (t < 0) fail(CMBL_ERR_FORMAT, "WL: %s names an unknown measurement type %s", key.c_str(), s.c_str());
        out.push_back(t);
    }
    return out;
}

// second derivatives of the natural ("dangle") cubic spline (Interpolation.f90:693-734)
template <class T, class X> static std::vector<T> wl_spline_d2(const std::vector<X> &x, const std::vector<T> &y) {
    const int n = (int)x.size();
    std::vector<T> d2(n, T(0)), u(n, T(0));
    T d1r = (y[1] - y[0]) / (T(x[1]) - T(x[0]));
    for (int i = 1; i < n - 1; i++) {
        const T d1l = d1r;
        d1r = (y[i + 1] - y[i]) / (T(x[i + 1]) - T(x[i]));
        const T xxdiv = T(1) / (T(x[i + 1]) - T(x[i - 1]));
        const T sig = (T(x[i]) - T(x[i - 1])) * xxdiv;
        const T xp = T(1) / (sig * d2[i - 1] + T(2));
        d2[i] = (sig - T(1)) * xp;
        u[i] = (T(6) * (d1r - d1l) * xxdiv - sig * u[i - 1]) * xp;
    }
    d2[n - 1] = T(0);
    for (int i = n - 2; i >= 0; i--) d2[i] = d2[i] * d2[i + 1] + u[i];
    return d2;
}

WlData load_wl(const Ini &ini) {
    static const std::set<std::string> served = {
        "name", "measurements_format", "nz_wl", "max_z", "num_z_bins", "num_gal_bins", "acc", "lmax", "nz_file",
        "nz_gal_file", "theta_bins_file", "num_theta_bins", "kmax", "ah_factor", "cov_file",
        "intrinsic_alignment_model", "data_types", "used_data_types", "nuisance_params", "data_selection",
        "wl_use_weyl", "measurements[xip]", "measurements[xim]", "measurements[gammat]", "measurements[wtheta]"};
    for (const std::string &k : ini.keys())
        if (!served.count(k)) fail(CMBL_ERR_UNSUPPORTED, "WL: key %s is not supported", k.c_str());
    WlData d;
    d.name = ini.str("name");
    if (d.name.empty()) {
        std::string fn = ini.filename();
        const size_t s = fn.find_last_of('/');
        fn = fn.substr(s == std::string::npos ? 0 : s + 1);
        const size_t dot = fn.find_last_of('.');
        d.name = dot == std::string::npos ? fn : fn.substr(0, dot);
    }
    const std::string fmt = ini.str_required("measurements_format");
    if (fmt != "DES")
        fail(CMBL_ERR_UNSUPPORTED, "WL: measurements_format = %s is not supported (only DES)", fmt.c_str());
    d.use_weyl = wl_logical(ini, "wl_use_weyl", false);
    d.nzb = wl_int(ini, "num_z_bins", 0);
    d.ngal = wl_int(ini, "num_gal_bins", 0);
    if (d.nzb < 1 || d.ngal < 0) fail(CMBL_ERR_FORMAT, "WL: num_z_bins = %d, num_gal_bins = %d", d.nzb, d.ngal);
    const int maxbin = std::max(d.nzb, d.ngal);
    d.acc = wl_double(ini, "acc", 1.0);
    d.lmax = wl_int(ini, "lmax", 50000);
    if (!(d.acc > 0.0) || d.lmax < 2) fail(CMBL_ERR_FORMAT, "WL: acc = %g, lmax = %d", d.acc, d.lmax);
    d.ah_factor = wl_double(ini, "ah_factor", 1.0);   // read and, as in the reference, not applied

    // n(z): z_p is column 2 plus two extrapolated knots whose n is zero (:140-169)
    const auto nzs = load_txt(ini.relative_filename("nz_file", true));
    if (nzs.size() < 2 || (int)nzs[0].size() < 3 + d.nzb)
        fail(CMBL_ERR_FORMAT, "WL: nz_file needs two rows and %d columns", 3 + d.nzb);
    const int rows = (int)nzs.size(), nz = d.nz = rows + 2;
    d.z_p.resize(nz);
    for (int i = 0; i < rows; i++) d.z_p[i] = nzs[i][1];
    d.z_p[nz - 2] = 2 * d.z_p[nz - 3] - d.z_p[nz - 4];
    d.z_p[nz - 1] = 3 * d.z_p[nz - 3] - 2 * d.z_p[nz - 4];
    for (int i = 1; i < nz; i++)
        if (!(d.z_p[i] > d.z_p[i - 1])) fail(CMBL_ERR_FORMAT, "WL: the redshifts of nz_file must increase");
    auto splines = [&](const std::vector<std::vector<double>> &tab, int nb, std::vector<double> &p,
                       std::vector<double> &d2) {
        p.assign((size_t)nb * nz, 0.0);
        d2.assign((size_t)nb * nz, 0.0);
        for (int b = 0; b < nb; b++) {
            std::vector<double> y(nz, 0.0);
            for (int i = 0; i < rows; i++) y[i] = tab[i][3 + b];
            const std::vector<double> s = wl_spline_d2<double>(d.z_p, y);
            std::copy(y.begin(), y.end(), p.begin() + (size_t)b * nz);
            std::copy(s.begin(), s.end(), d2.begin() + (size_t)b * nz);
        }
    };
    splines(nzs, d.nzb, d.p_src, d.d2_src);
    if (d.ngal > 0) {
        const auto nzg = load_txt(ini.relative_filename("nz_gal_file", true));
        if ((int)nzg.size() != rows || (int)nzg[0].size() < 3 + d.ngal)
            fail(CMBL_ERR_FORMAT, "WL: wl assumes windows used same bins");
        for (int i = 0; i < rows; i++)
            if (nzg[i][1] != d.z_p[i]) fail(CMBL_ERR_FORMAT, "WL: wl assumes windows used same bins");
        splines(nzg, d.ngal, d.p_gal, d.d2_gal);
    }
    for (const auto &r : load_txt(ini.relative_filename("theta_bins_file", true)))
        for (double v : r) d.theta_bins.push_back(v);
    d.ntheta = wl_int(ini, "num_theta_bins", (int)d.theta_bins.size());
    if ((int)d.theta_bins.size() != d.ntheta || d.ntheta < 1)
        fail(CMBL_ERR_FORMAT, "WL: size mismatch in theta_bins_file");
    const double pi = 3.14159265358979323846264338328;
    for (double t : d.theta_bins) d.theta_rad.push_back(t / 60 * pi / 180);
    const auto cov = load_txt(ini.relative_filename("cov_file", true));

    const std::string ia = ini.str("intrinsic_alignment_model", "DES1YR");
    if (ia != "none" && ia != "DES1YR")
        fail(CMBL_ERR_UNSUPPORTED, "WL: intrinsic_alignment_model = %s is not supported", ia.c_str());
    d.ia_des1yr = ia == "DES1YR";
    d.data_types = wl_type_list(ini, "data_types");
    for (int t : ini.has("used_data_types") ? wl_type_list(ini, "used_data_types") : d.data_types) d.want[t] = true;
    if (d.use_weyl && (d.want[WL_GAMMAT] || d.want[WL_WTHETA]))   // :201-203
        fail(CMBL_ERR_UNSUPPORTED, "WL: wl_use_weyl can only be used with weak lensing data (xip, xim)");
    d.param_names = load_paramnames(ini.relative_filename("nuisance_params", true), &d.n_params);
    if (d.n_params != 2 * (d.ngal + d.nzb) + 3)
        fail(CMBL_ERR_FORMAT, "WL: nuisance_params has %d names, %d expected (b, m, A, alpha, z0, DzL, DzS)",
             d.n_params, 2 * (d.ngal + d.nzb) + 3);

    // data_selection: a single-precision array, -1 where no row sets it (:207-221)
    std::vector<double> sel((size_t)WL_NTYPES * (maxbin + 1) * (maxbin + 1) * 2, -1.0);
    auto sel_at = [&](int tp, int b1, int b2) { return &sel[(((size_t)tp * (maxbin + 1) + b1) * (maxbin + 1) + b2) * 2]; };
    auto lines_of = [&](const std::string &path, auto &&each) {
        std::ifstream f(path);
        if (!f) fail(CMBL_ERR_IO, "WL: cannot read %s", path.c_str());
        std::string line;
        while (std::getline(f, line)) {
            const std::vector<std::string> t = split_ws(line);
            if (t.empty() || t[0][0] == '#') continue;
            each(t, line);
        }
    };
    lines_of(ini.relative_filename("data_selection", true), [&](const std::vector<std::string> &t, const std::string &line) {
        if (t.size() < 5) fail(CMBL_ERR_FORMAT, "WL: Error reading data_selection: %s", line.c_str());
        const int tp = wl_type(t[0]);
        if (tp < 0) fail(CMBL_ERR_FORMAT, "WL: data_selection has unknown measurement type %s", t[0].c_str());
        int b1, b2;
        double lo, hi;
        try {
            b1 = std::stoi(t[1]), b2 = std::stoi(t[2]);
            lo = parse_fortran_double(t[3]), hi = parse_fortran_double(t[4]);
        } catch (const std::exception &) {
            fail(CMBL_ERR_FORMAT, "WL: Error reading data_selection: %s", line.c_str());
        }
        if (b1 < 1 || b1 > maxbin || b2 < 1 || b2 > maxbin) fail(CMBL_ERR_FORMAT, "WL: data_selection: invalid bin");
        if (d.want[tp]) {
            sel_at(tp, b1, b2)[0] = (double)(float)lo;
            sel_at(tp, b1, b2)[1] = (double)(float)hi;
        }
    });

    // the measurement files in data_types order: covariance rows, bin pairs, used items (:223-275)
    int cov_ix = 0;
    d.first_theta_bin_used = d.ntheta;
    d.pairs.resize(d.data_types.size());
    for (size_t ti = 0; ti < d.data_types.size(); ti++) {
        const int tp = d.data_types[ti];
        int last1 = 0, last2 = 0;
        lines_of(ini.relative_filename(std::string("measurements[") + WL_TYPE_NAMES[tp] + "]", true),
                 [&](const std::vector<std::string> &t, const std::string &line) {
            int b1, b2, tb;
            double dat;
            try {
                if (t.size() < 4) throw std::invalid_argument("short");
                b1 = std::stoi(t[0]), b2 = std::stoi(t[1]), tb = std::stoi(t[2]);
                dat = parse_fortran_double(t[3]);
            } catch (const std::exception &) {
                fail(CMBL_ERR_FORMAT, "WL: Error reading measurements %s", WL_TYPE_NAMES[tp]);
            }
            if (tb < 1 || tb > d.ntheta) fail(CMBL_ERR_FORMAT, "WL: invalid theta bin: %s", line.c_str());
            if (b1 < 1 || b1 > maxbin || b2 < 1 || b2 > maxbin)
                fail(CMBL_ERR_FORMAT, "WL: invalid bin: %s", line.c_str());
            cov_ix++;
            if (last1 != b1 || last2 != b2) {
                d.pairs[ti].push_back({b1, b2});
                last1 = b1, last2 = b2;
            }
            if (!d.want[tp]) return;
            const double *r = sel_at(tp, b1, b2);
            const double theta = d.theta_bins[tb - 1];
            if (theta >= r[0] && theta <= r[1]) {
                const int item[4] = {(int)ti + 1, b1, b2, tb};
                d.used_items.insert(d.used_items.end(), item, item + 4);
                d.used_indices.push_back(cov_ix);
                d.data_vector.push_back(dat);
                d.first_theta_bin_used = std::min(d.first_theta_bin_used, tb);
            }
        });
        // a bin of the wrong kind would index past a kernel's tables
        for (const auto &pr : d.pairs[ti]) {
            const int n1 = (tp == WL_XIP || tp == WL_XIM) ? d.nzb : d.ngal, n2 = tp == WL_WTHETA ? d.ngal : d.nzb;
            if (pr.first > n1 || pr.second > n2)
                fail(CMBL_ERR_FORMAT, "WL: measurements[%s] has the bin pair %d %d", WL_TYPE_NAMES[tp], pr.first, pr.second);
        }
    }
    if (cov_ix != (int)cov.size() || (cov_ix > 0 && cov_ix != (int)cov[0].size()))
        fail(CMBL_ERR_FORMAT, "WL: cov size does not match data size");
    const int nu = d.n_used = (int)d.data_vector.size();
    if (nu < 1) fail(CMBL_ERR_FORMAT, "WL: the selection keeps no data point");
    d.invcov.resize((size_t)nu * nu);
    for (int i = 0; i < nu; i++)
        for (int j = 0; j < nu; j++) d.invcov[(size_t)i * nu + j] = cov[d.used_indices[i] - 1][d.used_indices[j] - 1];
    spd_inverse(d.invcov, nu);

    // ls_cl: linear then log (:284-297); 0.1266 * i is a single-precision product
    const int step = std::max(1, (int)(4 / d.acc));
    for (int i = 2; i <= 100 - (int)(4 / d.acc); i += step) d.ls_cl.push_back(i);
    if (d.ls_cl.empty()) fail(CMBL_ERR_FORMAT, "WL: acc = %g leaves no linear l", d.acc);
    for (int i = 0; d.ls_cl.back() < d.lmax; i++)
        d.ls_cl.push_back((int)std::lround(100 * std::exp((double)(0.1266f * (float)i) / d.acc)));
    d.nl = (int)d.ls_cl.size();

    // init_bessel_integration (:320-369); dlog is a single-precision quotient
    const int n = (int)(500 * d.acc);
    const double dlog = (double)((std::log((float)d.lmax) - std::log(1.0f)) / (float)n);
    std::vector<int> lo, hi;
    int ell = 2, ell_last = 1;
    for (int i = 1; i <= n; i++) {
        const int e = (int)std::exp(i * dlog);
        if (e == ell_last) continue;
        const int de = e - ell_last;
        ell_last = e;
        d.ls_bessel.push_back((double)((float)(2 * ell + de) - 1.0f) / 2);
        lo.push_back(ell);
        hi.push_back(ell + de - 1);
        ell += de;
    }
    const int nb = (int)d.ls_bessel.size(), nth = d.ntheta - d.first_theta_bin_used + 1;
    if (nb < 1 || d.ls_bessel.front() < d.ls_cl.front() || d.ls_bessel.back() > d.ls_cl.back())
        fail(CMBL_ERR_FORMAT, "WL: ls_bessel leaves the range of ls_cl (acc = %g, lmax = %d)", d.acc, d.lmax);
    d.bessel.assign((size_t)3 * nb * nth, 0.0);
    for (int i = 0; i < nb; i++)
        for (int j = 0; j < nth; j++) {
            double t0 = 0, t2 = 0, t4 = 0;
            for (int l = lo[i]; l <= hi[i]; l++) {
                const double x = l * d.theta_rad[d.first_theta_bin_used - 1 + j];
                t0 = t0 + l * j0(x);
                t2 = t2 + l * jn(2, x);
                t4 = t4 + l * jn(4, x);
            }
            d.bessel[((size_t)0 * nb + i) * nth + j] = t0 / (2 * pi);
            d.bessel[((size_t)1 * nb + i) * nth + j] = t2 / (2 * pi);
            d.bessel[((size_t)2 * nb + i) * nth + j] = t4 / (2 * pi);
        }
    for (size_t ti = 0; ti < d.data_types.size(); ti++) {
        const int tp = d.data_types[ti];
        if (tp == WL_XIM && d.xim_index == 0) d.xim_index = (int)ti + 1;
        if (tp == WL_XIM || !d.want[tp]) continue;
        for (const auto &pr : d.pairs[ti]) d.columns.push_back(WlColumn{tp, pr.first, pr.second});
    }
    return d;
}

// The operator of cl2corr (:619-653), transposed: opT[o][l][theta] with
// corr_o(theta) = sum_l opT[o][l][theta] C_l, o = 0, 1, 2 for J0, J2, J4.
static std::vector<double> wl_operator(const WlData &d) {
    typedef long double R;
    const int nl = d.nl, nb = (int)d.ls_bessel.size(), nth = d.ntheta - d.first_theta_bin_used + 1;
    // S[b][l]: the value at ls_bessel[b] of the natural spline through the unit vector e_l
    std::vector<R> S((size_t)nb * nl);
    std::vector<int> klo(nb);
    for (int b = 0, llo = 0; b < nb; b++) {   // TCubicSpline_FindNext (:498-511)
        while (llo < nl - 2 && d.ls_cl[llo + 1] < d.ls_bessel[b]) llo++;
        klo[b] = llo;
    }
    for (int l = 0; l < nl; l++) {
        std::vector<R> y(nl, R(0));
        y[l] = R(1);
        const std::vector<R> d2 = wl_spline_d2<R>(d.ls_cl, y);
        for (int b = 0; b < nb; b++) {
            const int k = klo[b];
            const R ho = R(d.ls_cl[k + 1]) - R(d.ls_cl[k]);
            const R a0 = (R(d.ls_cl[k + 1]) - R(d.ls_bessel[b])) / ho, b0 = R(1) - a0;
            S[(size_t)b * nl + l] =
                b0 * y[k + 1] + a0 * (y[k] - b0 * ((a0 + R(1)) * d2[k] + (R(2) - a0) * d2[k + 1]) * ho * ho / R(6));
        }
    }
    std::vector<double> op((size_t)3 * nl * nth);
    for (int o = 0; o < 3; o++)
        for (int l = 0; l < nl; l++)
            for (int j = 0; j < nth; j++) {
                R s = 0;
                for (int b = 0; b < nb; b++) s += R(d.bessel[((size_t)o * nb + b) * nth + j]) * S[(size_t)b * nl + l];
                op[((size_t)o * nl + l) * nth + j] = (double)s;
            }
    return op;
}

// ------------------------------------------------------------ kernels

static constexpr int WL_THREADS = 256;   // 4 waves
static constexpr int WL_MAXW = 1024;     // walkers per launch of the per-walker kernels (workspace_size)

typedef double wl_f64x4 __attribute__((ext_vector_type(4)));

struct WlDev {
    int nz, nl, nlp, nzb, ngal, nq, ncol, n_used, Np, nth, ia, weyl;
    const double *z, *p_src, *d2_src, *p_gal, *d2_gal;
    const int *col_a, *col_b;            // [ncol] rows of Q whose product is the column's right operand
    const double *opT;                   // [3][nl][nth]
    const int *u_col, *u_op, *u_th;      // [n_used] Limber column (-1: the theory is 0), operator, theta - first
    const int *u_m1, *u_m2;              // [n_used] shear calibrations of the (1 + m) factors, -1: none
    const double *data;                  // [n_used]
};

// doubles of one walker's workspace: Q [nq][nz] (qs of the source bins, then
// qgal of the lens bins), dchis / chis^2 (/ h^3) [nz], dchis [nz], n_chi
// [nzb][nz], then the Limber sums C [ncol][nlp]
__host__ __device__ inline size_t wl_ws_doubles(const WlDev &d) {
    return (size_t)(d.nq + 2 + d.nzb) * d.nz + (size_t)d.ncol * d.nlp;
}

// the n(z) spline at zs, 0 where zs leaves the table (:499-512); the knot by
// TCubicSpline_FindValue's bisection (Interpolation.f90:531-542)
__device__ __forceinline__ double wl_shifted(const double *__restrict__ z, const double *__restrict__ y,
                                             const double *__restrict__ d2, int n, double zs) {
    if (zs < z[0] || zs > z[n - 1]) return 0.0;
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int k = (hi + lo) / 2;
        if (z[k] > zs) hi = k;
        else lo = k;
    }
    const double ho = z[lo + 1] - z[lo];
    const double a0 = (z[lo + 1] - zs) / ho, b0 = 1.0 - a0;
    return b0 * y[lo + 1] + a0 * (y[lo] - b0 * ((a0 + 1.0) * d2[lo] + (2.0 - a0) * d2[lo + 1]) * (ho * ho) / 6.0);
}

__global__ __launch_bounds__(WL_THREADS) void wl_kernel_q(WlDev d, const double *__restrict__ dl, long long ld_walker,
                                                          const double *__restrict__ nuis, long long ld_nuis, double *ws,
                                                          const int *__restrict__ wcount, int w0)
{
    // w: the walker's place in this launch and in the workspace; w0: the launch's first slot in the batch
    const int w = blockIdx.x;
    if (wcount && w0 + w >= *wcount) return;
    const int tid = threadIdx.x, nz = d.nz;
    const double *row = dl + (size_t)w * ld_walker, *nu = nuis + (size_t)w * ld_nuis;
    double *Q = ws + (size_t)w * wl_ws_doubles(d);
    double *facr = Q + (size_t)d.nq * nz, *dch = facr + nz, *nchi = dch + nz;
    const double h = row[0], omm = row[1];
    const double *chis = row + 2, *Hs = chis + nz, *Dg = Hs + nz;
    const double *bias = nu, *dzl = nu + d.ngal + d.nzb + 3, *dzs = dzl + d.ngal;
    const double A = nu[d.ngal + d.nzb], alpha = nu[d.ngal + d.nzb + 1], z0 = nu[d.ngal + d.nzb + 2];

    for (int j = tid; j < nz; j += WL_THREADS) {
        double dc;   // :471-473
        if (j == 0) dc = (chis[1] + chis[0]) / 2;
        else if (j == nz - 1) dc = chis[nz - 1] - chis[nz - 2];
        else dc = (chis[j + 1] - chis[j - 1]) / 2;
        double f = dc / (chis[j] * chis[j]);
        if (!d.weyl) f = f / (h * h * h);
        dch[j] = dc;
        facr[j] = f;
    }
    for (int it = tid; it < d.nzb * nz; it += WL_THREADS) {
        const int b = it / nz, j = it - b * nz;
        nchi[it] = Hs[j] * wl_shifted(d.z, d.p_src + (size_t)b * nz, d.d2_src + (size_t)b * nz, nz, d.z[j] - dzs[b]);
    }
    for (int it = tid; it < d.ngal * nz; it += WL_THREADS) {
        const int b = it / nz, j = it - b * nz;
        Q[(size_t)d.nzb * nz + it] =
            Hs[j] * wl_shifted(d.z, d.p_gal + (size_t)b * nz, d.d2_gal + (size_t)b * nz, nz, d.z[j] - dzl[b]) * bias[b];
    }
    __syncthreads();
    // the lensing efficiency, the intrinsic-alignment term and the prefactor (:517-530)
    const double c5 = 1e5 / 2.99792458e8;
    for (int it = tid; it < d.nzb * nz; it += WL_THREADS) {
        const int b = it / nz, i = it - b * nz;
        const double *nc = nchi + (size_t)b * nz;
        const double ci = chis[i], zi = d.z[i];
        double s = 0.0;
        for (int j = i; j < nz; j++) s += (dch[j] * nc[j]) * (1.0 - ci / chis[j]);
        if (d.ia) {
            const double align = A * pow((1.0 + zi) / (1.0 + z0), alpha) * (double)0.0134f / Dg[i];
            s = s - align * nc[i] / (ci * (1.0 + zi) * 3.0 * (h * h) * (c5 * c5) / 2.0);
        }
        if (d.weyl) s = s * ci;
        else s = s * (3.0 / 2.0 * omm * (h * h) * (c5 * c5)) * ci * (1.0 + zi);
        Q[it] = s;
    }
}

// The Limber sums C[l][p] = sum_k P[l][k] (fac_k q_a(p)[k] q_b(p)[k]) on the f64
// MFMA, a 16 x 16 tile of (l, p) per wave at a time; a lane feeds 4 consecutive
// k of its row, so the k of one instruction are k0 + 4 (lane >> 4) + q in both
// operands.  Rows, columns and k beyond nl, ncol and nz are zeros formed in
// registers: nothing is read past the walker's row.  Then the used entries.
__global__ __launch_bounds__(WL_THREADS) void wl_kernel_corr(WlDev d, const double *__restrict__ dl,
                                                             long long ld_walker, const double *__restrict__ nuis,
                                                             long long ld_nuis, double *ws, double *__restrict__ xrows,
                                                             const int *__restrict__ wcount, int w0)
{
    const int w = blockIdx.x;
    if (wcount && w0 + w >= *wcount) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nz = d.nz, nlp = d.nlp;
    const double *P = dl + (size_t)w * ld_walker + 2 + 3 * (size_t)nz;
    const double *Q = ws + (size_t)w * wl_ws_doubles(d);
    const double *facr = Q + (size_t)d.nq * nz;
    double *C = ws + (size_t)w * wl_ws_doubles(d) + (size_t)(d.nq + 2 + d.nzb) * nz;
    const int nlt = nlp / 16, npt = (d.ncol + 15) / 16;
    for (int t = wave; t < nlt * npt; t += WL_THREADS / 64) {
        const int lt = t % nlt, pt = t / nlt;
        const int l = 16 * lt + (lane & 15), p = 16 * pt + (lane & 15);
        const bool lok = l < d.nl, pok = p < d.ncol;
        const double *pa = P + (size_t)(lok ? l : 0) * nz;
        const double *qa = Q + (size_t)(pok ? d.col_a[p] : 0) * nz, *qb = Q + (size_t)(pok ? d.col_b[p] : 0) * nz;
        wl_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < nz; k0 += 16) {
            const int kb = k0 + 4 * (lane >> 4);
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const bool kok = kb + q < nz;
                a[q] = (lok && kok) ? pa[kb + q] : 0.0;
                b[q] = (pok && kok) ? facr[kb + q] * (qa[kb + q] * qb[kb + q]) : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 4; q++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[q], acc, 0, 0, 0);
        }
        // lane layout of the result: column lane & 15, rows (lane >> 4) + 4 r
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int ll = 16 * lt + (lane >> 4) + 4 * r;
            if (pok && ll < d.nl) C[(size_t)p * nlp + ll] = acc[r];
        }
    }
    __syncthreads();   // C is in the walker's workspace for every wave
    // cl2corr at the used entries (:634-651), make_vector, minus the data vector; zeros to Np
    const double *m = nuis + (size_t)w * ld_nuis + d.ngal;
    double *x = xrows + (size_t)(w0 + w) * d.Np;
    for (int i = tid; i < d.Np; i += WL_THREADS) {
        double v = 0.0;
        if (i < d.n_used) {
            const int col = d.u_col[i];
            double s = 0.0;
            if (col >= 0) {
                const double *op = d.opT + (size_t)d.u_op[i] * d.nl * d.nth + d.u_th[i];
                const double *c = C + (size_t)col * nlp;
                for (int l = 0; l < d.nl; l++) s += op[(size_t)l * d.nth] * c[l];
                double fac2 = 1.0;
                if (d.u_m1[i] >= 0) fac2 = 1.0 + m[d.u_m1[i]];
                if (d.u_m2[i] >= 0) fac2 = fac2 * (1.0 + m[d.u_m2[i]]);
                s = s * fac2;
            }
            v = s - d.data[i];
        }
        x[i] = v;
    }
}

// a non-finite -lnL is logZero, for that walker alone
__global__ void wl_kernel_finish(double *__restrict__ out, int W, const int *__restrict__ wcount)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W || (wcount && w >= *wcount)) return;
    const double v = out[w];
    if (!(fabs(v) <= 1.79769313486231570e308)) out[w] = CMBL_LOGZERO;
}

// ------------------------------------------------------------ likelihood

struct WlLike : Like {
    WlData h;
    WlDev dev{};
    QuadForm qf;
    DevBuf b_z, b_ps, b_d2s, b_pg, b_d2g, b_ca, b_cb, b_op, b_uc, b_uo, b_ut, b_m1, b_m2, b_data;

    explicit WlLike(WlData &&data) : h(std::move(data)) {
        name = h.name;
        tag = "WL";
        n_nuis = h.n_params;
        nuisance_names = h.param_names;
        speed = 0;   // TDataLikelihood's default; wl_dataset_speed[TAG] is the caller's (WLLikelihood_Add :92)
        theory_len = 2 + 3 * h.nz + h.nl * h.nz;
        dev.nz = h.nz, dev.nl = h.nl, dev.nlp = (h.nl + 15) / 16 * 16;
        dev.nzb = h.nzb, dev.ngal = h.ngal, dev.nq = h.nzb + h.ngal;
        dev.ncol = (int)h.columns.size(), dev.n_used = h.n_used;
        dev.nth = h.ntheta - h.first_theta_bin_used + 1;
        dev.ia = h.ia_des1yr, dev.weyl = h.use_weyl;
        qf.init(h.invcov, h.n_used);
        dev.Np = qf.Np;
        std::vector<int> ca, cb, uc, uo, ut, m1, m2;
        for (const WlColumn &c : h.columns) {   // rows of Q: source bin b at b - 1, lens bin b at nzb + b - 1
            ca.push_back(c.type == WL_XIP ? c.f1 - 1 : h.nzb + c.f1 - 1);
            cb.push_back(c.type == WL_WTHETA ? h.nzb + c.f2 - 1 : c.f2 - 1);
        }
        for (int i = 0; i < h.n_used; i++) {
            const int *it = &h.used_items[(size_t)4 * i];
            const int tp = h.data_types[it[0] - 1];
            // xim is read off xip's C_l with J4, when xip is wanted and has the pair (:639-641)
            const int ctype = tp == WL_XIM ? WL_XIP : tp;
            int col = -1;
            for (int c = 0; c < dev.ncol && col < 0; c++)
                if (h.columns[c].type == ctype && h.columns[c].f1 == it[1] && h.columns[c].f2 == it[2]) col = c;
            uc.push_back(col);
            uo.push_back(tp == WL_XIM ? 2 : (tp == WL_GAMMAT ? 1 : 0));
            ut.push_back(it[3] - h.first_theta_bin_used);
            m1.push_back(tp == WL_XIP || tp == WL_XIM ? it[1] - 1 : -1);
            m2.push_back(tp == WL_WTHETA ? -1 : it[2] - 1);
        }
        dev.z = upload(b_z, h.z_p);
        dev.p_src = upload(b_ps, h.p_src), dev.d2_src = upload(b_d2s, h.d2_src);
        dev.p_gal = upload(b_pg, h.p_gal), dev.d2_gal = upload(b_d2g, h.d2_gal);
        dev.col_a = upload(b_ca, ca), dev.col_b = upload(b_cb, cb);
        dev.opT = upload(b_op, wl_operator(h));
        dev.u_col = upload(b_uc, uc), dev.u_op = upload(b_uo, uo), dev.u_th = upload(b_ut, ut);
        dev.u_m1 = upload(b_m1, m1), dev.u_m2 = upload(b_m2, m2);
        dev.data = upload(b_data, h.data_vector);
    }

    // the quadratic form's part for W walkers, then the per-walker part of one chunk
    size_t qf_bytes(int W) const { return (qf.workspace_size(W) + 255) & ~size_t(255); }
    size_t workspace_size(int W) const override {
        if (W <= 0) return 0;
        return qf_bytes(W) + wl_ws_doubles(dev) * 8 * (size_t)std::min(W, WL_MAXW);
    }

    void run(int W, const double *dl, long long ld_walker, const double *nuis, long long ld_nuis, double *out, void *ws,
             hipStream_t stream, const int *wcount) {
        if (W <= 0) return;
        nuis = nuisance_rows(nuis, nullptr);
        if (W > 1 && ld_nuis < n_nuis) fail(CMBL_ERR_ARG, "WL: ld_nuis %lld < %d", ld_nuis, n_nuis);   // one row has no stride
        if (ld_walker != 0 && ld_walker < theory_len)
            fail(CMBL_ERR_ARG, "WL: ld_walker %lld < the %d doubles of a walker's theory row", ld_walker, theory_len);
        if (!ws) {
            own_ws.grow(workspace_size(W));
            ws = own_ws.p;
        }
        double *scratch = reinterpret_cast<double *>(static_cast<char *>(ws) + qf_bytes(W));
        double *x = qf.x_rows(ws);
        // batches beyond the workspace's walkers run in chunks, one after another in stream order
        for (int w0 = 0; w0 < W; w0 += WL_MAXW) {
            const int Wc = std::min(WL_MAXW, W - w0);
            timed_launch("wl_kernel_q", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(wl_kernel_q, dim3(Wc), dim3(WL_THREADS), 0, stream, e0, e1, 0, dev,
                                      dl + (size_t)w0 * ld_walker, ld_walker, nuis + (size_t)w0 * ld_nuis, ld_nuis,
                                      scratch, wcount, w0);
            });
            HIP_CHECK(hipGetLastError());
            timed_launch("wl_kernel_corr", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(wl_kernel_corr, dim3(Wc), dim3(WL_THREADS), 0, stream, e0, e1, 0, dev,
                                      dl + (size_t)w0 * ld_walker, ld_walker, nuis + (size_t)w0 * ld_nuis, ld_nuis,
                                      scratch, x, wcount, w0);
            });
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipMemsetAsync(qf.counters(ws, W), 0, (size_t)qf.n_counters(W) * 4, stream));
        qf.launch(W, ws, nullptr, out, stream, "wl_quadform_ksplit", wcount);
        timed_launch("wl_kernel_finish", stream, [&](hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(wl_kernel_finish, dim3((W + 255) / 256), dim3(256), 0, stream, e0, e1, 0, out, W,
                                  wcount);
        });
        HIP_CHECK(hipGetLastError());
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

std::unique_ptr<Like> make_wl(const Ini &ini) { return std::unique_ptr<Like>(new WlLike(load_wl(ini))); }

bool wl_info(const Like *like, int *dims) {
    const WlLike *L = dynamic_cast<const WlLike *>(like);
    if (!L) return false;
    const int v[8] = {L->h.nz, L->h.nl, (int)L->h.ls_bessel.size(), (int)L->h.columns.size(), L->h.n_used,
                      L->h.first_theta_bin_used, L->h.nzb, L->h.ngal};
    if (dims) std::copy(v, v + 8, dims);
    return true;
}

bool wl_arrays(const Like *like, int *ls_cl, double *ls_bessel, int *used_items) {
    const WlLike *L = dynamic_cast<const WlLike *>(like);
    if (!L) return false;
    if (ls_cl) std::copy(L->h.ls_cl.begin(), L->h.ls_cl.end(), ls_cl);
    if (ls_bessel) std::copy(L->h.ls_bessel.begin(), L->h.ls_bessel.end(), ls_bessel);
    if (used_items) std::copy(L->h.used_items.begin(), L->h.used_items.end(), used_items);
    return true;
}

}  // namespace cmamd
