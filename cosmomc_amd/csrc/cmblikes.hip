// CMBlikes bandpower likelihoods (reference TCMBLikes, source/CMBlikes.f90)
// and the BICEP/Keck/Planck foreground model (TBK_planck,
// source/CMB_BK_Planck.f90), batched over W walkers on MI355X.
//
// Per walker (CMBLikes_LogLike, CMBlikes.f90:1165-1227):
//   map spectra  MapCl_ij(l) = Theory_{f_i f_j}(l) [+ aberration] [+ foregrounds] [/ cal^2]
//                                             (GetTheoryMapCls / AdaptTheoryForMaps :1022-1126)
//   binning      Cls(out, b) = sum_win dot(W(:,win,b), MapCl_in(win))  [+ linear correction]
//                                             (TBinWindows_bin :1230-1256, GetBinnedMapCls :981-995)
//   per bin      C = Cls (+ noise);  HL:  X_b = Transform(C, Chat_b, Cfid_b^1/2)   (:861-914)
//                                    gaussian: X_b = C - Chat_b
//   -lnL         = (bigX^T C^-1 bigX + (ln cal / sigma)^2) / 2         (:1220-1225)
//
// Where things are:
//   cmbldev.h     the structs the kernels take (CLDev, HLDev, ExactDev, work items) and constants
//   cmblfg.h      cmbl_bk_prologue, cmbl_smica_prologue: foreground SEDs and l profiles per walker
//   cmblwindow.h  cmbl_window_direct / cmbl_window_kernel / cmbl_window_group: every window
//                 column as a dot product with one map spectrum, a skinny f64 MFMA GEMM over l
//   cmblreduce.h  cmbl_reduce_kernel (binned C matrices / bigX rows) and cmbl_gauss_small_kernel
//                 (gaussian datasets with <= 64 bandpowers: chi^2 in one kernel)
//   cmblhl.h      cmbl_hl_rows_kernel<M>: the HL transform per (walker, bin), two symmetric
//                 eigendecompositions by one-sided (Hestenes) cyclic Jacobi
//   cmblexact.h   cmbl_exact_kernel: like_approx = exact (unbinned), ExactChiSq per (walker, l)
//   cmbldata.h    CLData: the dataset as read from its ini file (host only)
//   this file     device tables built from a CLData, the workspace layout, the launch driver;
//                 bigX^T C^-1 bigX / 2 is quadform_ksplit on the f64 MFMA (quadform.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>

#include "divrn.h"
#include "quadform.h"
#include "smallgauss.h"

namespace cmamd {

#include "cmbldev.h"
#include "cmblfg.h"
#include "cmblwindow.h"
#include "cmblreduce.h"
#include "cmblhl.h"
#include "cmblexact.h"
#include "cmbldata.h"

struct CMBLikes final : Like {
    const CLData d;
    QuadForm qf;
    // device tables
    CLDev dev{};                 // wcount, td0 and td_den stay null here: a call sets them on its own copy
    HLDev hl{};
    DevBuf d_pairs, d_items, d_wts, d_wdir, d_sumoff, d_sumcols, d_sumconst, d_corroff, d_corrcols, d_corrconst,
        d_etox, d_fidcorr, d_noise, d_chat, d_cluse, d_bkmaps, d_bpnu, d_bpR, d_bpdnu, d_hlchat, d_hlcf, d_hlu0, d_hlv0;
    int max_field = 0, n_part_rows = 0;
    bool items_even = true, small_gauss = false;
    bool use_group = false;      // BK foregrounds: grouped-pair window kernel
    int n_gitem = 0;
    DevBuf d_gitems, d_gw, d_bplnu, d_logl80;
    int small_ntask = 0;
    SmallDev sdev{};
    DevBuf d_invcov, d_stasks, d_smt, d_sct;
    // window columns (one per bin and window entry with an output; main then
    // correction), the map pairs they read, and per element its columns; kept
    // so the work items can be rebuilt on other segment boundaries (window_resegment)
    struct HCol { int pair, lo, hi; const double *W; double cst; bool fixed; };
    std::vector<HCol> wcols;
    std::vector<CLPair> pairs;
    std::vector<std::vector<int>> w_emain, w_ecorr;
    std::vector<WItem> h_items;                     // direct-path work items (host copy)
    std::vector<std::vector<int>> h_item_cols;      // their columns (indices into wcols)
    std::map<int, std::vector<int>> seg_starts;     // theory field -> segment starts (relative l); default 256

    CMBLikes(const Ini &ini, const std::string &tag_) : d(ini, tag_) {
        tag = tag_;
        name = d.name;
        nuisance_names = d.nuisance_names;
        n_nuis = d.n_nuis;
        derived_names = d.derived_names;
        n_derived = d.n_derived;
        std::copy(d.cl_lmax, d.cl_lmax + 16, cl_lmax);
        if (d.approx == 3) build_exact();
        else build_device();
    }

    // like_approx = exact: per-l table [nb][K] = N_l (ncl) | chol(Chat_l) (ncl) | ln det Chat_l | (2l+1) fksy
    ExactDev xdev{};
    DevBuf d_xtab;
    void build_exact() {
        const int nmaps = d.nmaps, ncl = d.ncl, nb = d.nb;
        xdev.n = nmaps;
        xdev.ncl = ncl;
        xdev.lmin = d.lmin;
        xdev.lmax = d.lmax;
        xdev.bmin = d.bin_min;
        xdev.nb = nb;
        xdev.K = 2 * ncl + 2;
        std::vector<double> tab((size_t)nb * xdev.K, 0.0);
        for (int b = 0; b < nb; b++) {
            double *t = &tab[(size_t)b * xdev.K];
            for (int e = 0; e < ncl; e++) t[e] = d.clnoise[(size_t)b * ncl + e];
            // Chat = R R^T (Matrix_Cholesky, as MatrixSym_LogDet :619-634 does for M)
            const double *M = &d.chatM[(size_t)b * nmaps * nmaps];
            std::vector<double> R((size_t)nmaps * nmaps, 0.0);
            double lndet = 0.0;
            for (int j = 0; j < nmaps; j++) {
                double dd = M[j * nmaps + j];
                for (int k = 0; k < j; k++) dd -= R[j * nmaps + k] * R[j * nmaps + k];
                if (!(dd > 0))
                    fail(CMBL_ERR_NUMERIC, "CMBlikes exact: cl_hat at l = %d is not positive definite", d.bin_min + b);
                dd = std::sqrt(dd);
                R[j * nmaps + j] = dd;
                lndet += std::log(dd);
                for (int i = j + 1; i < nmaps; i++) {
                    double v = M[i * nmaps + j];
                    for (int k = 0; k < j; k++) v -= R[i * nmaps + k] * R[j * nmaps + k];
                    R[i * nmaps + j] = v / dd;
                }
            }
            for (int i = 0, q = 0; i < nmaps; i++)
                for (int j = 0; j <= i; j++, q++) t[ncl + q] = R[i * nmaps + j];
            t[2 * ncl] = 2.0 * lndet;
            t[2 * ncl + 1] = (2.0 * (d.bin_min + b) + 1.0) * d.fksy;
        }
        // element (i, j), i >= j, of the lower triangle -> theory field
        for (int i = 1, q = 0; i <= nmaps; i++)
            for (int j = 1; j <= i; j++, q++) {
                xdev.field[q] = d.pair_field(i, j, xdev.cmb[q]);
                max_field = std::max(max_field, xdev.field[q]);
            }
        xdev.tab = upload(d_xtab, tab);
        xdev.aberration = d.aberration;
        xdev.cal_index = d.cal_index;
        xdev.log_cal_prior = d.log_cal_prior;
    }

    // Work items of the window stage, their partial rows, and the per-element
    // row lists and small-gaussian tasks that consume them (re-run by
    // window_resegment; the results depend on the segment boundaries only
    // through the summation split of each window's dot product).
    void build_items() {
        const int lmin = d.lmin, L = d.lmax - lmin + 1;
        const int nE = d.nb * d.ncl;
        max_field = 0;
        // work items: per pair, per l chunk, the overlapping columns in groups of WK_COLS
        std::vector<double> wdense, wdirect;
        std::vector<std::vector<int>> col_parts(wcols.size());
        int nrows = 0;
        const int SEG = WK_CHUNK * WK_NCH;
        // BK foregrounds without aberration: grouped-pair items (cmbl_window_group),
        // when no pair has more than 16 window columns
        use_group = d.bk && d.aberration == 0.0;
        if (use_group) {
            std::vector<int> per_pair(pairs.size(), 0);
            for (auto &cc : wcols)
                if (!cc.fixed && ++per_pair[cc.pair] > 16) use_group = false;
        }
        std::vector<GItem> gitems;
        std::vector<double> gw;
        if (use_group) {
            std::map<int, std::vector<int>> by_field;
            for (size_t p = 0; p < pairs.size(); p++) by_field[pairs[p].field].push_back((int)p);
            for (auto &fv : by_field)
                for (size_t g0 = 0; g0 < fv.second.size(); g0 += GP) {
                    const int npair = (int)std::min<size_t>(GP, fv.second.size() - g0);
                    for (int sg = 0; sg < (L + GSEG - 1) / GSEG; sg++) {
                        const int c0 = sg * GSEG, c1 = std::min(L - 1, c0 + GSEG - 1);
                        std::vector<std::vector<int>> sel(npair);
                        int lo = c1 + 1, hi = c0 - 1;
                        for (int g = 0; g < npair; g++)
                            for (size_t ci = 0; ci < wcols.size(); ci++)
                                if (!wcols[ci].fixed && wcols[ci].pair == fv.second[g0 + g] && wcols[ci].hi >= c0 &&
                                    wcols[ci].lo <= c1) {
                                    sel[g].push_back((int)ci);
                                    lo = std::min(lo, std::max(c0, wcols[ci].lo));
                                    hi = std::max(hi, std::min(c1, wcols[ci].hi));
                                }
                        if (hi < lo) continue;
                        GItem it{};
                        it.field = fv.first;
                        it.npair = npair;
                        it.l0 = (lo + lmin) & ~1;      // even: 16-byte loads (>= lmin - 1; profiles are 0 there)
                        it.nstep = (hi + lmin - it.l0 + 32) / 32;
                        it.woff = (long long)gw.size();
                        const int Lp = it.nstep * 32;
                        for (int g = 0; g < GP; g++) {
                            it.pair[g] = g < npair ? fv.second[g0 + g] : 0;
                            it.ncol[g] = g < npair ? (int)sel[g].size() : 0;
                            it.part[g] = nrows;
                            for (int cc = 0; cc < 16; cc++)
                                for (int l = 0; l < Lp; l++) {
                                    const int jl = it.l0 + l - lmin;
                                    gw.push_back(g < npair && cc < it.ncol[g] && jl >= lo && jl <= hi
                                                     ? wcols[sel[g][cc]].W[jl] : 0.0);
                                }
                            if (g < npair)
                                for (int ci : sel[g]) col_parts[ci].push_back(nrows++);
                        }
                        gitems.push_back(it);
                    }
                }
            for (auto &p : pairs) max_field = std::max(max_field, p.field);
        }
        n_gitem = (int)gitems.size();
        upload(d_gitems, gitems);
        upload(d_gw, gw);
        h_items.clear();
        h_item_cols.clear();
        for (size_t p = 0; p < (use_group ? 0 : pairs.size()); p++) {
            std::vector<int> segs;
            auto fs = seg_starts.find(pairs[p].field);
            if (fs != seg_starts.end()) segs = fs->second;
            else
                for (int c = 0; c < L; c += SEG) segs.push_back(c);
            for (size_t sg = 0; sg < segs.size(); sg++) {
                const int c0 = segs[sg], c1 = std::min(L - 1, sg + 1 < segs.size() ? segs[sg + 1] - 1 : L - 1);
                if (c1 < c0) continue;
                std::vector<int> sel;
                for (size_t ci = 0; ci < wcols.size(); ci++)
                    if (!wcols[ci].fixed && wcols[ci].pair == (int)p && wcols[ci].hi >= c0 && wcols[ci].lo <= c1)
                        sel.push_back((int)ci);
                for (size_t g0 = 0; g0 < sel.size(); g0 += WK_COLS) {
                    const size_t g1 = std::min(sel.size(), g0 + WK_COLS);
                    int lo = c1, hi = c0;
                    for (size_t g = g0; g < g1; g++) {
                        lo = std::min(lo, std::max(c0, wcols[sel[g]].lo));
                        hi = std::max(hi, std::min(c1, wcols[sel[g]].hi));
                    }
                    if ((lo + lmin) % 2 == 1 && lo > c0) lo--;     // even l0: 16-byte theory loads
                    WItem it{};
                    it.pair = (int)p;
                    it.l0 = lo + lmin;
                    it.l1 = hi + lmin;
                    it.ncol = (int)(g1 - g0);
                    it.part = nrows;
                    it.nch = (hi - lo + WK_CHUNK) / WK_CHUNK;
                    it.woff = (long long)wdense.size();
                    for (int l = lo; l < lo + it.nch * WK_CHUNK; l++)   // [nch][WK_CHUNK][WK_COLS], zero padded
                        for (int g = 0; g < WK_COLS; g++)
                            wdense.push_back(l <= hi && g0 + g < g1 ? wcols[sel[g0 + g]].W[l] : 0.0);
                    it.woff2 = (long long)wdirect.size();
                    const int ncb = (it.ncol + 15) / 16;
                    for (int ch = 0; ch < it.nch; ch++)         // [nch][ncb][16][WK_CHUNK], zero padded
                        for (int cb = 0; cb < ncb; cb++)
                            for (int g = 16 * cb; g < 16 * cb + 16; g++)
                                for (int k = 0; k < WK_CHUNK; k++) {
                                    const int l = lo + ch * WK_CHUNK + k;
                                    wdirect.push_back(l <= hi && g0 + g < g1 ? wcols[sel[g0 + g]].W[l] : 0.0);
                                }
                    for (size_t g = g0; g < g1; g++) col_parts[sel[g]].push_back(nrows++);
                    h_items.push_back(it);
                    h_item_cols.emplace_back(sel.begin() + g0, sel.begin() + g1);
                }
            }
        }
        n_part_rows = nrows;
        items_even = true;
        for (auto &it : h_items) items_even = items_even && (it.l0 % 2 == 0);
        for (auto &it : h_items) max_field = std::max(max_field, pairs[it.pair].field);
        // per element: the partial rows of its columns in window order, and the fixed-spectrum constants
        auto flatten = [&](const std::vector<std::vector<int>> &lists, std::vector<int> &off, std::vector<int> &rows,
                           std::vector<double> &cst) {
            off.assign(lists.size() + 1, 0);
            cst.assign(lists.size(), 0.0);
            for (size_t e = 0; e < lists.size(); e++) {
                off[e] = (int)rows.size();
                for (int ci : lists[e]) {
                    rows.insert(rows.end(), col_parts[ci].begin(), col_parts[ci].end());
                    cst[e] += wcols[ci].cst;
                }
            }
            off[lists.size()] = (int)rows.size();
        };
        std::vector<int> main_off, main_rows, corr_off, corr_rows;
        std::vector<double> main_cst, corr_cst;
        flatten(w_emain, main_off, main_rows, main_cst);
        flatten(w_ecorr, corr_off, corr_rows, corr_cst);
        {   // small-gaussian tasks: each element's rows in runs of <= 8 (main rows, then corr rows)
            std::vector<SmallTask> tasks;
            std::vector<int> rows_all(main_rows);
            rows_all.insert(rows_all.end(), corr_rows.begin(), corr_rows.end());
            std::vector<int> mt(nE + 1), ct(nE + 1);
            for (int e = 0; e < nE; e++) {
                mt[e] = (int)tasks.size();
                for (int q = main_off[e]; q < main_off[e + 1]; q += 8)
                    tasks.push_back({q, std::min(8, main_off[e + 1] - q)});
            }
            mt[nE] = (int)tasks.size();
            const int base = (int)main_rows.size();
            for (int e = 0; e < nE; e++) {
                ct[e] = (int)tasks.size();
                for (int q = corr_off[e]; q < corr_off[e + 1]; q += 8)
                    tasks.push_back({base + q, std::min(8, corr_off[e + 1] - q)});
            }
            ct[nE] = (int)tasks.size();
            small_ntask = (int)tasks.size();
            std::vector<int> trow(tasks.size() * 8, -1);
            for (size_t t = 0; t < tasks.size(); t++)
                for (int u = 0; u < tasks[t].count; u++) trow[8 * t + u] = rows_all[tasks[t].first + u];
            sdev.ntask = small_ntask;
            sdev.trow = upload(d_stasks, trow);
            sdev.e_main_t = upload(d_smt, mt);
            sdev.e_corr_t = upload(d_sct, ct);
        }
        small_gauss = d.approx == 2 && d.nX <= SMALL_NX && small_ntask <= SMALL_MAXTASK;
        dev.nitem = (int)h_items.size();
        dev.items = upload(d_items, h_items);
        dev.wdense = upload(d_wts, wdense);
        dev.wdirect = upload(d_wdir, wdirect);
        dev.e_main_off = upload(d_sumoff, main_off);
        dev.e_main_rows = upload(d_sumcols, main_rows);
        dev.e_main_const = upload(d_sumconst, main_cst);
        dev.e_corr_off = upload(d_corroff, corr_off);
        dev.e_corr_rows = upload(d_corrcols, corr_rows);
        dev.e_corr_const = upload(d_corrconst, corr_cst);
    }

    void build_device() {
        const int L = d.lmax - d.lmin + 1, nb = d.nb, ncl = d.ncl;
        // required map pairs (InitMapCls :997-1019)
        pairs.clear();
        auto pair_index = [&](int i, int j) { return (i - 1) * i / 2 + (j - 1); };   // i >= j, 1-based
        const int TT = 0, EE = 2, BB = 5;
        for (int i = 1; i <= d.nreq; i++)
            for (int j = 1; j <= i; j++) {
                CLPair p{};
                p.field = d.pair_field(i, j, p.cmb);
                p.fg = d.bk ? (p.field == EE ? 1 : p.field == BB ? 2 : 0)
                            : (d.smica && p.field == TT) ? 3 : 0;   // SMICA: CL%theory_i == 1 .and. CL%theory_j == 1
                p.mi = i - 1;
                p.mj = j - 1;
                pairs.push_back(p);
            }
        // window columns: one per (bin, window entry with an output); main then correction
        wcols.clear();
        const int nE = nb * ncl;
        w_emain.assign(nE, {});
        w_ecorr.assign(nE, {});
        auto add_windows = [&](const Windows &wn, std::vector<std::vector<int>> &lists) {
            const int norder = (int)wn.in_i.size();
            for (int b = 0; b < nb; b++)
                for (int k = 0; k < norder; k++) {
                    if (wn.out[k] <= 0) continue;
                    const double *Wk = &wn.W[((size_t)b * norder + k) * L];
                    HCol c{-1, L, -1, Wk, 0.0, false};
                    for (int l = 0; l < L; l++)
                        if (Wk[l] != 0.0) { c.lo = std::min(c.lo, l); c.hi = l; }
                    if (!wn.fix[k].empty()) {              // fix_cl: walker-independent dot
                        c.fixed = true;
                        for (int l = 0; l < L; l++) c.cst += Wk[l] * wn.fix[k][l];
                    } else {
                        if (wn.in_i[k] == 0 || wn.in_j[k] == 0)
                            fail(CMBL_ERR_FORMAT, "CMBlikes: bin window uses a spectrum of a map that is not required");
                        c.pair = pair_index(wn.in_i[k], wn.in_j[k]);
                    }
                    lists[(size_t)b * ncl + (wn.out[k] - 1)].push_back((int)wcols.size());
                    wcols.push_back(c);
                }
        };
        add_windows(d.bw, w_emain);
        if (d.cw.present) add_windows(d.cw, w_ecorr);
        build_items();
        std::vector<int> e_to_x(nE, -1);
        for (int b = 0; b < nb; b++)
            for (int u = 0; u < d.ncl_used; u++) e_to_x[b * ncl + d.cl_use[u]] = b * d.ncl_used + u;
        const std::vector<double> zeros(nE, 0.0);
        dev.pairs = upload(d_pairs, pairs);
        dev.e_to_x = upload(d_etox, e_to_x);
        dev.fidcorr = upload(d_fidcorr, d.cw.present ? d.fidcorr : zeros);
        dev.noise = upload(d_noise, d.have_noise ? d.clnoise : zeros);
        dev.chat = upload(d_chat, d.clhat);
        hl.cl_use = upload(d_cluse, d.cl_use);
        hl.chat = upload(d_hlchat, d.chatM);
        hl.cfhalf = upload(d_hlcf, d.cfh);
        if (d.approx == 1) {   // the HL eigensolves' starting bases (cmbl_hl_rows_kernel warm start; else null)
            const int n = d.nmaps;
            std::vector<double> u0((size_t)nb * n * n), v0((size_t)nb * n * n);
            for (int b = 0; b < nb; b++) {
                std::vector<double> cf(d.cfh.begin() + (size_t)b * n * n, d.cfh.begin() + (size_t)(b + 1) * n * n);
                std::vector<double> ev, U, cm = cf, R((size_t)n * n, 0.0), V;
                sym_eigen(cf, n, ev, U);                       // C_fid^1/2 and C_fid share eigenvectors
                bool ok = true;
                for (double e : ev) ok = ok && e > 0.0;
                if (ok) {
                    sym_power(cm, n, -1.0);                    // C_fid^-1/2
                    const double *ch = &d.chatM[(size_t)b * n * n];
                    std::vector<double> T((size_t)n * n, 0.0);
                    for (int i = 0; i < n; i++)
                        for (int j = 0; j < n; j++)
                            for (int k = 0; k < n; k++) T[i * n + j] += ch[i * n + k] * cm[k * n + j];
                    for (int i = 0; i < n; i++)
                        for (int j = 0; j < n; j++)
                            for (int k = 0; k < n; k++) R[i * n + j] += cm[i * n + k] * T[k * n + j];
                    sym_eigen(R, n, ev, V);
                } else {
                    U.assign((size_t)n * n, 0.0);
                    for (int i = 0; i < n; i++) U[i * n + i] = 1.0;
                    V = U;
                }
                std::copy(U.begin(), U.end(), u0.begin() + (size_t)b * n * n);
                std::copy(V.begin(), V.end(), v0.begin() + (size_t)b * n * n);
            }
            hl.u0 = upload(d_hlu0, u0);
            hl.v0 = upload(d_hlv0, v0);
        }
        dev.LP = (d.lmax + 2) & ~1;
        if (d.bk) {
            dev.bkmaps = upload(d_bkmaps, d.bkmaps);
            dev.bp_nu = upload(d_bpnu, d.bp_nu);
            dev.bp_R = upload(d_bpR, d.bp_R);
            dev.bp_dnu = upload(d_bpdnu, d.bp_dnu);
            std::vector<double> blnu(d.bp_nu.size()), ll80(dev.LP, 0.0);
            for (size_t k = 0; k < blnu.size(); k++) blnu[k] = std::log(d.bp_nu[k]);
            for (int l = 1; l < (int)ll80.size(); l++) ll80[l] = std::log(l / 80.0);
            dev.bp_lnu = upload(d_bplnu, blnu);
            dev.log_l80 = upload(d_logl80, ll80);
            dev.nsamp = (int)d.bp_nu.size();
        }
        qf.init(d.invcov, d.nX);
        upload(d_invcov, d.invcov);
        dev.lmin = d.lmin;
        dev.lmax = d.lmax;
        dev.aberration = d.aberration;
        dev.cal_index = d.cal_index;
        dev.log_cal_prior = d.log_cal_prior;
        dev.nE = nE;
        dev.ncl_used = d.ncl_used;
        dev.nX = d.nX;
        dev.Np = qf.Np;
        dev.approx = d.approx;
        dev.has_corr = d.cw.present ? 1 : 0;
        dev.bk = d.bk ? 1 : 0;
        dev.nreq = d.nreq;
        dev.smica_pivot = 2000.0;
        dev.fpivot_dust = d.fpivot_dust;
        dev.fpivot_sync = d.fpivot_sync;
        for (int k = 0; k < 2; k++) {
            dev.decorr_dust[k] = d.decorr_dust[k];
            dev.decorr_sync[k] = d.decorr_sync[k];
        }
        dev.lform_dust = d.lform_dust;
        dev.lform_sync = d.lform_sync;
        hl.n = d.nmaps;
        hl.m = std::max(2, (d.nmaps + 1) & ~1);
        hl.nb = nb;
        hl.ncl = ncl;
        hl.ncl_used = d.ncl_used;
        hl.nX = d.nX;
        hl.Np = qf.Np;
        hl.status = status_word();
    }

    // workspace: quadratic form | partial dots [rows][W] | C matrices [W][nE] (HL) |
    //            BK coef [W][3 nreq] + profiles [3][L][W] | addend [W]
    struct WsLayout { size_t part, cmat, coef, prof, add, td, total; };
    WsLayout layout(int W) const {
        auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
        WsLayout o{};
        o.part = al(qf.workspace_size(W));
        o.cmat = o.part + al((size_t)n_part_rows * W * 8);
        o.coef = o.cmat + al(d.approx == 1 ? (size_t)W * d.nb * d.ncl * 8 : 0);
        o.prof = o.coef + al(d.bk ? (size_t)W * 3 * d.nreq * 8 : 0);
        o.add = o.prof + al((d.bk || d.smica) ? (size_t)3 * dev.LP * W * 8 : 0);   // prof [W][3][LP]
        o.td = o.add + al((size_t)W * 8);
        o.total = o.td + al(d.bk ? (size_t)(dev.nsamp + 1) * 8 : 0);   // T_dust table: td0, then nsamp denominators
        return o;
    }
    size_t workspace_size(int W) const override { return d.approx == 3 ? 256 : layout(W).total; }

    void loglike_batch(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                       long long ld_nuis, double *out, void *ws, hipStream_t stream) override {
        run(W, dl, ld_field, ld_walker, nuis, ld_nuis, out, ws, stream, nullptr);
    }
    bool sparse_capable() const override { return d.approx != 3; }
    void loglike_batch_sparse(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                              long long ld_nuis, double *out, void *ws, hipStream_t stream,
                              const int *wcount) override {
        run(W, dl, ld_field, ld_walker, nuis, ld_nuis, out, ws, stream, wcount);
    }

    // The window stage is cmbl_window_direct's: no foregrounds or aberration, so the map
    // spectra are the theory rows (unbinned data are read only as like_approx = exact, and
    // use_group needs bk: neither wants a term of its own)
    bool direct_windows() const { return d.approx != 3 && !d.bk && !d.smica && d.aberration == 0.0; }

    // window stage: the direct path's work items, one column per (item, window column) writing its partial row
    bool window_stage(WinStage &st) const override {
        if (!direct_windows()) return false;
        st.kind = 0;
        st.cal_index = d.cal_index;
        st.cols.clear();
        for (size_t k = 0; k < h_items.size(); k++) {
            const WItem &it = h_items[k];
            const CLPair &pr = pairs[it.pair];
            for (size_t g = 0; g < h_item_cols[k].size(); g++) {
                const HCol &c = wcols[h_item_cols[k][g]];
                st.cols.push_back(WinCol{pr.field, it.l0, it.l1, c.W + (it.l0 - d.lmin), it.part + (int)g,
                                         (pr.cmb && d.cal_index >= 0) ? 1 : 0});
            }
        }
        return true;
    }
    double *window_out(void *ws, int W) const override {
        return reinterpret_cast<double *>(static_cast<char *>(ws) + layout(W).part);
    }
    QFDeferred after_window(int W, const double *nuis, long long ld_nuis, double *out, void *ws, hipStream_t stream,
                            bool defer, const SmallGaussLaunch *co = nullptr) override {
        if (co) fail(CMBL_ERR_ARG, "internal: %s carries no co-run", name.c_str());
        if (W <= 0) return QFDeferred{};
        const double *nu = nuisance_rows(nuis, ws);
        if (defer && !deferred_capable()) fail(CMBL_ERR_UNSUPPORTED, "%s: no deferred evaluation", name.c_str());
        return post_window(dev, W, nu, ld_nuis, out, ws, stream, defer);
    }
    // the small chi^2 as a co-run of another likelihood's deferred quadratic
    // form (the after_window stage of a fused small gaussian dataset)
    bool corun_small(SmallGaussLaunch &a, int W, const double *nuis, long long ld_nuis, double *out,
                     void *ws) override {
        if (!small_gauss || W <= 0 || !ws) return false;
        a = small_args(dev, W, nuisance_rows(nuis, ws), ld_nuis, out, ws);
        return true;
    }
    bool window_resegment(const std::map<int, std::vector<int>> &starts) override {
        if (!direct_windows()) return false;
        const int L = d.lmax - d.lmin + 1;
        seg_starts.clear();
        for (auto &kv : starts) {
            std::vector<int> v{0};
            for (int c : kv.second)
                if (c - d.lmin > v.back() && c - d.lmin < L) v.push_back(c - d.lmin);
            seg_starts[kv.first] = v;
        }
        build_items();
        return true;
    }
    std::map<int, std::vector<int>> window_segments() const override { return seg_starts; }
    void window_set_segments(const std::map<int, std::vector<int>> &segs) override {
        if (seg_starts == segs) return;
        seg_starts = segs;
        build_items();
    }

    // the quadratic-form datasets (HL and large gaussian) can leave the combine to the sampler
    bool deferred_capable() const override { return d.approx != 3 && !small_gauss; }
    QFDeferred loglike_batch_deferred(int W, const double *dl, long long ld_field, long long ld_walker,
                                      const double *nuis, long long ld_nuis, void *ws, hipStream_t stream) override {
        if (!deferred_capable()) fail(CMBL_ERR_UNSUPPORTED, "%s: no deferred evaluation", name.c_str());
        if (!ws) fail(CMBL_ERR_ARG, "deferred evaluation needs a caller workspace");
        return run(W, dl, ld_field, ld_walker, nuis, ld_nuis, nullptr, ws, stream, nullptr, true);
    }

    QFDeferred run(int W, const double *dl, long long ld_field, long long ld_walker, const double *nuis,
                   long long ld_nuis, double *out, void *ws, hipStream_t stream, const int *wcount,
                   bool defer = false) {
        if (W <= 0) return QFDeferred{};
        const double *nu = nuisance_rows(nuis, dl);
        const int lmax = d.lmax;
        if (ld_field < lmax + 1) fail(CMBL_ERR_ARG, "ld_field %lld < cl_lmax+1 = %d", ld_field, lmax + 1);
        if (W > 1 && ld_walker != 0 && ld_walker < (long long)(max_field + 1) * ld_field)
            fail(CMBL_ERR_ARG, "ld_walker must cover theory fields 0..%d", max_field);
        if (!ws) {
            own_ws.grow(workspace_size(W));
            ws = own_ws.p;
        }
        if (d.approx == 3) {
            timed_launch("cmbl_exact_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                const dim3 g((W + EXACT_WPB - 1) / EXACT_WPB), bl(256);
                switch (d.nmaps) {
#define CMBL_EXACT(N)                                                                                     \
    case N:                                                                                               \
        hipExtLaunchKernelGGL(cmbl_exact_kernel<N>, g, bl, 0, stream, e0, e1, 0, xdev, dl, ld_field, ld_walker, \
                              nu, ld_nuis, out, W);                                                       \
        break;
                    CMBL_EXACT(1) CMBL_EXACT(2) CMBL_EXACT(3) CMBL_EXACT(4)
#undef CMBL_EXACT
                    default: break;
                }
            });
            HIP_CHECK(hipGetLastError());
            return QFDeferred{};
        }
        const WsLayout o = layout(W);
        char *base = static_cast<char *>(ws);
        double *partial = reinterpret_cast<double *>(base + o.part);
        double *coef = reinterpret_cast<double *>(base + o.coef);
        double *prof = reinterpret_cast<double *>(base + o.prof);
        const int tiles = (W + 63) / 64;
        CLDev c = dev;   // this call's arguments: the tables, its live-walker count and its T_dust table
        c.wcount = wcount;
        if (d.bk) {
            // the T_dust table is per call (this workspace), so concurrent calls on
            // other streams -- the sampler's walker groups -- cannot overwrite it
            c.td0 = reinterpret_cast<double *>(base + o.td);
            c.td_den = c.td0 + 1;
            hipLaunchKernelGGL(cmbl_bk_tdtab, dim3((c.nsamp + 255) / 256), dim3(256), 0, stream, c, nu);
            HIP_CHECK(hipGetLastError());
            timed_launch("cmbl_bk_prologue", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(cmbl_bk_prologue, dim3(W), dim3(BKP_THREADS), 0, stream, e0, e1, 0, c, nu, ld_nuis,
                                      coef, prof, W);
            });
            HIP_CHECK(hipGetLastError());
        }
        if (d.smica) {
            timed_launch("cmbl_smica_prologue", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(cmbl_smica_prologue, dim3((c.LP + 255) / 256, W), dim3(256), 0, stream, e0, e1,
                                      0, c, nu, ld_nuis, prof, W);
            });
            HIP_CHECK(hipGetLastError());
        }
        // 16-byte theory loads need aligned rows and even chunk starts
        const bool gvec = theory_vec16(dl, ld_field, ld_walker);
        const bool vec_ok = gvec && items_even && (lmax + 1 < ld_field || (lmax % 2 == 1 && lmax + 1 <= ld_field));
        if (use_group) {
            const int txcd = tiles % 8 == 0 ? 1 : 0;
            const int nblk = txcd ? tiles * n_gitem : 8 * tiles * ((n_gitem + 7) / 8);
            timed_launch("cmbl_window_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                if (c.lform_dust != 0 || c.lform_sync != 0)
                    hipExtLaunchKernelGGL(cmbl_window_group<true>, dim3(nblk), dim3(256), 0, stream, e0, e1, 0, c,
                                          d_gitems.as<GItem>(), n_gitem, d_gw.as<double>(), dl, ld_field, ld_walker,
                                          nu, ld_nuis, (const double *)coef, (const double *)prof, c.LP, partial, W,
                                          tiles, (int)gvec, txcd);
                else
                    hipExtLaunchKernelGGL(cmbl_window_group<false>, dim3(nblk), dim3(256), 0, stream, e0, e1, 0, c,
                                          d_gitems.as<GItem>(), n_gitem, d_gw.as<double>(), dl, ld_field, ld_walker,
                                          nu, ld_nuis, (const double *)coef, (const double *)prof, c.LP, partial, W,
                                          tiles, (int)gvec, txcd);
            });
        } else if (direct_windows()) {
            const int nblk = 8 * tiles * ((c.nitem + 7) / 8);
            timed_launch("cmbl_window_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                hipExtLaunchKernelGGL(cmbl_window_direct, dim3(nblk), dim3(256), 0, stream, e0, e1, 0, c, dl,
                                      ld_field, ld_walker, nu, ld_nuis, partial, W, tiles, (int)vec_ok);
            });
        } else
        timed_launch("cmbl_window_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
#define CMBL_WINDOW(A, F)                                                                                        \
    hipExtLaunchKernelGGL(cmbl_window_kernel<A, F>, dim3(tiles, c.nitem), dim3(256), 0, stream, e0, e1, 0, c, dl, \
                          ld_field, ld_walker, nu, ld_nuis, (const double *)coef, (const double *)prof, partial, W,    \
                          (int)vec_ok)
            const bool ab = d.aberration != 0.0;
            if (d.bk || d.smica) {
                if (ab) CMBL_WINDOW(true, true);
                else CMBL_WINDOW(false, true);
            } else {
                if (ab) CMBL_WINDOW(true, false);
                else CMBL_WINDOW(false, false);
            }
#undef CMBL_WINDOW
        });
        HIP_CHECK(hipGetLastError());
        return post_window(c, W, nu, ld_nuis, out, ws, stream, defer);
    }

    void derived_batch(int W, const double *nuis, long long ld_nuis, double *out, long long ld_out,
                       hipStream_t stream) override {
        if (W <= 0 || n_derived <= 0) return;
        if (!out || ld_out < n_derived) fail(CMBL_ERR_ARG, "derived output needs %d columns", n_derived);
        if (!d.smica) return Like::derived_batch(W, nuis, ld_nuis, out, ld_out, stream);
        nuis = nuisance_rows(nuis, nullptr);   // SMICA has its five foreground parameters
        hipLaunchKernelGGL(cmbl_smica_derived, dim3((W + 63) / 64), dim3(64), 0, stream, dev,
                           pairs.empty() ? 0 : (int)(pairs[0].fg == 3), nuis, ld_nuis, out, ld_out, n_derived, W);
        HIP_CHECK(hipGetLastError());
    }

    SmallGaussLaunch small_args(const CLDev &c, int W, const double *nu, long long ld_nuis, double *out,
                                void *ws) const {
        SmallGaussLaunch a{};
        a.d = SmallGaussDev{c.nE,       c.nX,           c.has_corr,     c.cal_index,   c.log_cal_prior,
                            c.e_to_x,   c.e_main_const, c.e_corr_const, c.fidcorr,     c.chat,
                            sdev.ntask, sdev.trow,      sdev.e_main_t,  sdev.e_corr_t, c.wcount};
        a.partial = reinterpret_cast<const double *>(static_cast<const char *>(ws) + layout(W).part);
        a.nuis = nu;
        a.ld_nuis = ld_nuis;
        a.M = d_invcov.as<double>();
        a.out = out;
        a.W = W;
        return a;
    }

    // the kernels after the window stage: binned spectra, then chi^2 (small
    // gaussian) or the HL transform / gaussian residuals and the quadratic form;
    // c: the call's arguments (run's copy, or dev itself when every walker is live)
    QFDeferred post_window(const CLDev &c, int W, const double *nu, long long ld_nuis, double *out, void *ws,
                           hipStream_t stream, bool defer) {
        const WsLayout o = layout(W);
        char *base = static_cast<char *>(ws);
        void *qws = ws;
        double *partial = reinterpret_cast<double *>(base + o.part);
        double *cmat = reinterpret_cast<double *>(base + o.cmat);
        double *addend = reinterpret_cast<double *>(base + o.add);
        const bool use_add = d.log_cal_prior > 0 && d.cal_index >= 0;
        const int tiles = (W + 63) / 64;
        if (small_gauss) {
            const SmallGaussLaunch a = small_args(c, W, nu, ld_nuis, out, ws);
            timed_launch("cmbl_gauss_small_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                const int ng = (W + SMALL_WT - 1) / SMALL_WT;
                hipExtLaunchKernelGGL(cmbl_gauss_small_kernel<SMALL_WT>, dim3(small_gauss_blocks(ng)), dim3(256), 0,
                                      stream, e0, e1, 0, a, ng);
            });
            HIP_CHECK(hipGetLastError());
            return QFDeferred{};
        }
        timed_launch("cmbl_reduce_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(cmbl_reduce_kernel, dim3(tiles, (c.nE + 3) / 4), dim3(256), 0, stream, e0, e1, 0, c,
                                  (const double *)partial, nu, ld_nuis, qf.x_rows(qws), cmat, use_add ? addend : nullptr,
                                  qf.counters(qws, W), qf.n_counters(W), W);
        });
        HIP_CHECK(hipGetLastError());
        if (d.approx == 1) {
            HLDev h = hl;
            h.wcount = c.wcount;
            timed_launch("cmbl_hl_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
                const dim3 bl(64);
                switch (h.m) {
#define CMBL_HLR(MM)                                                                                              \
    case MM:                                                                                                      \
        hipExtLaunchKernelGGL(cmbl_hl_rows_kernel<MM>, dim3((W * h.nb + 64 / MM - 1) / (64 / MM)), bl, 0, stream,  \
                              e0, e1, 0, h, (const double *)cmat, qf.x_rows(qws), W);                            \
        break;
                    CMBL_HLR(2) CMBL_HLR(4) CMBL_HLR(6) CMBL_HLR(8) CMBL_HLR(10) CMBL_HLR(12) CMBL_HLR(14)
                    CMBL_HLR(16)
#undef CMBL_HLR
                    default: break;
                }
            });
            HIP_CHECK(hipGetLastError());
        }
        if (defer) return qf.launch_deferred(W, qws, use_add ? addend : nullptr, stream, "cmbl_quadform");
        qf.launch(W, qws, use_add ? addend : nullptr, out, stream, "cmbl_quadform", c.wcount);
        return QFDeferred{};
    }
};

std::unique_ptr<Like> make_cmblikes(const Ini &ini, const std::string &tag) {
    return std::unique_ptr<Like>(new CMBLikes(ini, tag));
}

}  // namespace cmamd

#ifdef CMAMD_STAMPS
extern "C" int cmamd_debug_hl_sweeps(unsigned int *host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(cmamd::g_hl_sweeps), sizeof(cmamd::g_hl_sweeps)) == hipSuccess ? 0 : -5;
}
extern "C" int cmamd_debug_hl_phase(unsigned long long *host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(cmamd::g_hl_phase), sizeof(cmamd::g_hl_phase)) == hipSuccess ? 0 : -5;
}
extern "C" int cmamd_debug_hl_tp(unsigned long long *host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(cmamd::g_hl_tp), sizeof(cmamd::g_hl_tp)) == hipSuccess ? 0 : -5;
}
#endif
