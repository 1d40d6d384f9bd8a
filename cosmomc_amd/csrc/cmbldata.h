// A CMBlikes dataset as its ini file describes it (CMBLikes_ReadIni with
// ReadClArr / ReadBinWindows / ReadCovmat, CMBlikes.f90:146-859, then
// Tsmica_planck_ReadIni or TBK_planck_ReadIni): host values only, nothing on
// the device.  cmblikes.hip builds its device tables from a CLData.
// (included by cmblikes.hip inside namespace cmamd, after cmbldev.h)
#pragma once

static int type_index(char ch) {   // TypeIndex: T E B P -> 1..4 (:134-144)
    const char *f = "TEBP";
    const char *p = std::strchr(f, ch);
    if (!p || !ch) fail(CMBL_ERR_FORMAT, "Invalid C_l part %c, must be one of: TEBP", ch);
    return (int)(p - f) + 1;
}

static std::string format_u(const std::string &fmt, int i) {   // FormatString(filename, i) for %u
    std::string s = fmt;
    size_t p = s.find("%u");
    if (p != std::string::npos) s.replace(p, 2, std::to_string(i));
    return s;
}

// File%LastTopComment (FileUtils.f90:1150-1168)
static std::string last_top_comment(const std::string &path) {
    std::ifstream f(path);
    if (!f) fail(CMBL_ERR_IO, "cannot read %s", path.c_str());
    std::string line, res;
    while (std::getline(f, line)) {
        size_t a = line.find_first_not_of(" \t\r");
        if (a == std::string::npos) continue;
        if (line[0] == '#') {
            std::string t = line.substr(1);
            size_t b = t.find_first_not_of(" \t");
            res = b == std::string::npos ? "" : t.substr(b);
            while (!res.empty() && (res.back() == ' ' || res.back() == '\r' || res.back() == '\t')) res.pop_back();
        } else {
            break;
        }
    }
    return res;
}

static bool ini_logical(const Ini &ini, const std::string &key, bool def) {
    std::string v = ini.str(key);
    if (v.empty()) return def;
    const char ch = (char)std::toupper(v[0] == '.' && v.size() > 1 ? v[1] : v[0]);
    if (ch == 'T' || ch == '1' || ch == 'Y') return true;
    if (ch == 'F' || ch == '0' || ch == 'N') return false;
    fail(CMBL_ERR_FORMAT, "%s: bad logical %s = %s", ini.filename().c_str(), key.c_str(), v.c_str());
    return def;
}

static int ini_int(const Ini &ini, const std::string &key, bool required, int def) {
    std::string v = required ? ini.str_required(key) : ini.str(key);
    if (v.empty()) return def;
    return std::stoi(v);
}

static double ini_double(const Ini &ini, const std::string &key, double def) {
    std::string v = ini.str(key);
    return v.empty() ? def : parse_fortran_double(v);
}

struct Windows {                   // TBinWindows (:27-34) for bins bin_min..bin_max
    std::vector<int> in_i, in_j;   // required-map indices (1-based, i >= j; 0 = not required)
    std::vector<int> out;          // used cl index (1-based, 0 = not used)
    std::vector<double> W;         // [bin][win][L]
    std::vector<std::vector<double>> fix;   // per window: fixed spectrum over L (empty = theory)
    bool present = false;
};

struct CLData {
    std::string name;
    bool has_map_names = false, bk = false, smica = false;
    std::vector<std::string> map_names, used_map_order;
    std::vector<int> map_fields, use_map, require_map, map_used_index, map_required_index, required_order;
    int approx = 0, nmaps = 0, nreq = 0, ncl = 0, ncl_used = 0;   // approx: 1 HL, 2 gaussian, 3 exact
    bool binned = true;
    double fksy = 1.0;                                              // fullsky_exact_fksy
    int lmin = 0, lmax = 0, nbins = 0, bin_min = 1, bin_max = 0, nb = 0;
    int cl_lmax[16] = {0};                                          // Like::cl_lmax
    double aberration = 0.0, log_cal_prior = -1.0;
    int cal_index = -1;
    Windows bw, cw;
    std::vector<double> clhat, clnoise, clfid, fidcorr;   // [bin][ncl]
    bool have_noise = false;                               // the noise is added to the theory's binned spectra
    std::vector<int> cl_use;                               // 0-based
    std::vector<double> invcov;                            // [nX][nX]
    int nX = 0;
    std::vector<double> chatM, cfh;                        // per bin [nmaps][nmaps]: Chat, C_fid^1/2 (HL)
    // nuisance and derived parameter names (Like's fields of the same names)
    std::string nuisance_names, derived_names;
    int n_nuis = 0, n_derived = 0;
    // BK: bandpass samples of all required maps, pivots and decorrelation options
    std::vector<BKMap> bkmaps;
    std::vector<double> bp_nu, bp_R, bp_dnu;
    double fpivot_dust = 0, fpivot_sync = 0, decorr_dust[2] = {0, 0}, decorr_sync[2] = {0, 0};
    int lform_dust = 0, lform_sync = 0;                    // 0 flat, 1 lin, 2 quad

    // The theory field (0..9: TT TE EE BT BE BB PT PE PB PP) of the pair of required
    // maps i >= j (1-based), and whether both are T/E/B so that aberration and
    // calibration apply (MapPair_to_Theory_i_j :284-299)
    int pair_field(int i, int j, int &cmb) const {
        int f1 = map_fields[required_order[i - 1] - 1], f2 = map_fields[required_order[j - 1] - 1];
        if (f2 > f1) std::swap(f1, f2);
        cmb = (f1 <= 3 && f2 <= 3);
        return f1 * (f1 - 1) / 2 + (f2 - 1);
    }

    std::string cl_name(const std::vector<std::string> &names, int i, int j) const {   // Cl_i_j_name (:328-343)
        return has_map_names ? names[i - 1] + "x" + names[j - 1] : names[i - 1] + names[j - 1];
    }
    int map_index(const std::string &s) const {
        for (size_t k = 0; k < map_names.size(); k++)
            if (map_names[k] == s) return (int)k + 1;
        return -1;
    }
    void pair_to_map_indices(const std::string &S, int &i1, int &i2) const {   // :195-213
        if (S.size() == 2) {
            if (has_map_names) fail(CMBL_ERR_FORMAT, "CMBlikes: CL names must use MAP1xMAP2 names");
            i1 = map_index(S.substr(0, 1));
            i2 = map_index(S.substr(1, 1));
        } else {
            size_t ix = S.find('x');
            if (ix == std::string::npos) fail(CMBL_ERR_FORMAT, "CMBLikes: invalid spectrum name %s", S.c_str());
            i1 = map_index(S.substr(0, ix));
            i2 = map_index(S.substr(ix + 1));
        }
        if (i1 == -1 || i2 == -1) fail(CMBL_ERR_FORMAT, "CMBLikes: unrecognised map name %s", S.c_str());
    }
    // UseString_to_Cl_i_j (:262-281) with PairStringToUsedMapIndices (:215-231)
    void use_string_to_cl_i_j(const std::string &S, const std::vector<int> &used_index, std::vector<int> &ii,
                              std::vector<int> &jj) const {
        ii.clear();
        jj.clear();
        for (auto &t : split_ws(S)) {
            int i1, i2;
            pair_to_map_indices(t, i1, i2);
            i1 = used_index[i1 - 1];
            i2 = used_index[i2 - 1];
            if (i2 > i1) std::swap(i1, i2);
            ii.push_back(i1);
            jj.push_back(i2);
        }
    }
    std::vector<int> use_string_to_cols(const std::string &S) const {   // :234-260
        std::vector<int> ii, jj, cols;
        use_string_to_cl_i_j(S, map_used_index, ii, jj);
        for (size_t k = 0; k < ii.size(); k++) {
            int ix = 0, c = 0;
            for (int a = 1; a <= nmaps; a++)
                for (int b = 1; b <= a; b++) {
                    ix++;
                    if (a == ii[k] && b == jj[k]) c = ix;
                }
            if (ii[k] == 0 || jj[k] == 0) c = 0;
            cols.push_back(c);
        }
        return cols;
    }
    int cols_from_order(const std::string &order, std::vector<int> &cols) const {   // GetColsFromOrder :345-369
        auto li = split_ws(order);
        auto index_of = [&](const std::string &s) {
            for (size_t k = 0; k < li.size(); k++)
                if (li[k] == s) return (int)k + 1;
            return -1;
        };
        cols.assign(ncl, 0);
        int ix = 0;
        for (int i = 1; i <= nmaps; i++)
            for (int j = 1; j <= i; j++) {
                ix++;
                int i1 = index_of(cl_name(used_map_order, i, j));
                if (i1 == -1 && i != j) i1 = index_of(cl_name(used_map_order, j, i));
                if (i1 != -1) {
                    if (cols[ix - 1] > 0) fail(CMBL_ERR_FORMAT, "GetColsFromOrder: duplicate CL type");
                    cols[ix - 1] = i1;
                }
            }
        return (int)li.size();
    }
    // ReadClArr (:146-193): Cl [bin_min..bin_max][ncl]
    bool read_cl_arr(const Ini &ini, const std::string &base, std::vector<double> &cl, bool optional) const {
        std::string fn = ini.relative_filename(base + "_file", !optional);
        if (fn.empty()) return false;
        std::string order = ini.str(base + "_order"), incols;
        if (order.empty()) {
            incols = last_top_comment(fn);
            if (incols.empty()) fail(CMBL_ERR_FORMAT, "No column order given for %s", fn.c_str());
        } else {
            incols = "L " + order;
        }
        std::vector<int> cols;
        const int norder = cols_from_order(incols, cols) - 1;
        cl.assign((size_t)nb * ncl, 0.0);
        auto rows = load_txt(fn);
        int ll = -1;
        for (auto &r : rows) {
            if ((int)r.size() < 1 + norder) fail(CMBL_ERR_FORMAT, "CMBLikes_ReadClArr: error reading line %s", fn.c_str());
            const int l = (int)r[0];
            ll = l;
            if (l >= bin_min && l <= bin_max)
                for (int ix = 0; ix < ncl; ix++)
                    if (cols[ix] != 0) cl[(size_t)(l - bin_min) * ncl + ix] = r[cols[ix] - 1];
        }
        if (ll < bin_max) fail(CMBL_ERR_FORMAT, "CMBLikes_ReadClArr: C_l file does not go up to maximum used: %d (%s)",
                               bin_max, fn.c_str());
        return true;
    }
    void read_bin_windows(const Ini &ini, const std::string &type, Windows &bwin) const {   // ReadBinWindows :371-464
        const int L = lmax - lmin + 1;
        std::string fname = ini.str_required(type + "_files");
        std::string order1 = ini.str_required(type + "_in_order");
        std::string order2 = ini.str(type + "_out_order", order1);
        if (order2.empty()) order2 = order1;
        use_string_to_cl_i_j(order1, map_required_index, bwin.in_i, bwin.in_j);
        bwin.out = use_string_to_cols(order2);
        const int norder = (int)bwin.in_i.size();
        if (norder != (int)bwin.out.size())
            fail(CMBL_ERR_FORMAT, "%s_in_order and %s_out_order must have same number of CL", type.c_str(), type.c_str());
        bwin.W.assign((size_t)nb * norder * L, 0.0);
        for (int b = bin_min; b <= bin_max; b++) {
            std::string S = ini.resolve_path(format_u(fname, b));
            auto rows = load_txt(S);
            for (auto &r : rows) {
                if ((int)r.size() < 1 + norder) fail(CMBL_ERR_FORMAT, "ReadBinWindows: error reading line %s", S.c_str());
                const int l = (int)r[0];
                if (l >= lmin && l <= lmax)
                    for (int k = 0; k < norder; k++) bwin.W[((size_t)(b - bin_min) * norder + k) * L + (l - lmin)] = r[1 + k];
            }
        }
        bwin.fix.assign(norder, {});
        std::string fixf = ini.relative_filename(type + "_fix_cl_file", false);
        if (!fixf.empty()) {
            std::string o1 = ini.str(type + "_fix_cl_file_order");
            if (o1.empty()) {
                o1 = last_top_comment(fixf);
                if (o1.empty()) fail(CMBL_ERR_FORMAT, "No column order given for %s", fixf.c_str());
                while (!o1.empty() && (o1[0] == ' ' || o1[0] == 'L')) o1 = o1.substr(1);
            }
            std::vector<int> fi, fj, ui, uj;
            use_string_to_cl_i_j(o1, map_required_index, fi, fj);
            use_string_to_cl_i_j(ini.str_required(type + "_fix_cl"), map_required_index, ui, uj);
            auto rows = load_txt(fixf);
            for (size_t u = 0; u < ui.size(); u++) {
                if (ui[u] == 0 || uj[u] == 0) continue;
                int idx = -1;
                for (size_t k = 0; k < fi.size(); k++)
                    if (fi[k] == ui[u] && fj[k] == uj[u]) { idx = (int)k; break; }
                if (idx < 0) fail(CMBL_ERR_FORMAT, "ReadBinWindows: fix_cl uses CL not in the fix_cl_file");
                std::vector<double> spec(L, 0.0);
                for (auto &r : rows) {
                    const int l = (int)r[0];
                    if (l >= lmin && l <= lmax && (int)r.size() > idx + 1) spec[l - lmin] = r[idx + 1];
                }
                for (int k = 0; k < norder; k++)
                    if (bwin.in_i[k] == ui[u] && bwin.in_j[k] == uj[u]) bwin.fix[k] = spec;
            }
        }
        bwin.present = true;
    }
    void read_covmat(const Ini &ini) {   // ReadCovmat (:752-859), binned
        std::string covmat_cl = ini.str_required("covmat_cl");
        std::string fn = ini.relative_filename("covmat_fiducial", true);
        const double scale = ini_double(ini, "covmat_scale", 1.0);
        auto cl_in = use_string_to_cols(covmat_cl);
        const int num_in = (int)cl_in.size();
        std::vector<int> cov_cl_used;
        for (int i = 0; i < num_in; i++)
            if (cl_in[i] != 0) {
                cl_use.push_back(cl_in[i] - 1);
                cov_cl_used.push_back(i);
            }
        ncl_used = (int)cl_use.size();
        if (ncl_used == 0) fail(CMBL_ERR_FORMAT, "CMBlikes: covmat_cl selects no used spectra");
        const int nin = num_in * nbins;
        std::vector<double> cov;
        for (auto &r : load_txt(fn)) cov.insert(cov.end(), r.begin(), r.end());
        if ((long long)cov.size() < (long long)nin * nin)
            fail(CMBL_ERR_FORMAT, "%s: covariance needs %d x %d entries", fn.c_str(), nin, nin);
        nX = nb * ncl_used;
        invcov.assign((size_t)nX * nX, 0.0);
        for (int bx = bin_min; bx <= bin_max; bx++)
            for (int by = bin_min; by <= bin_max; by++)
                for (int a = 0; a < ncl_used; a++)
                    for (int b = 0; b < ncl_used; b++)
                        invcov[(size_t)((bx - bin_min) * ncl_used + a) * nX + (by - bin_min) * ncl_used + b] =
                            scale * cov[(size_t)((bx - 1) * num_in + cov_cl_used[a]) * nin + (by - 1) * num_in +
                                        cov_cl_used[b]];
        spd_inverse(invcov, nX);
    }

    CLData(const Ini &ini, const std::string &tag) {
        bk = (tag == "BKPLANCK");
        smica = (tag == "SMICA");       // TSmica_planck (CMB.f90:94-95)
        name = ini.str("name");
        if (name.empty()) {
            std::string fn = ini.filename();
            size_t s = fn.find_last_of('/');
            fn = fn.substr(s == std::string::npos ? 0 : s + 1);
            size_t d = fn.find_last_of('.');
            name = d == std::string::npos ? fn : fn.substr(0, d);
        }
        // ---- CMBLikes_ReadIni (:466-749)
        std::string fmt = ini.str("dataset_format");
        if (fmt == "CMBLike") fail(CMBL_ERR_FORMAT, "CMBLikes dataset_format now CMBLike2");
        if (!fmt.empty() && fmt != "CMBLike2") fail(CMBL_ERR_FORMAT, "CMBLikes wrong dataset_format");
        std::string S = ini.str("map_names");
        has_map_names = !S.empty();
        if (has_map_names) {
            map_names = split_ws(S);
            auto mf = split_ws(ini.str_required("map_fields"));
            if (mf.size() != map_names.size()) fail(CMBL_ERR_FORMAT, "CMBLikes: number of map_fields does not match map_names");
            for (auto &f : mf) map_fields.push_back(type_index(f[0]));
        } else {
            map_names = {"T", "E", "B", "P"};
            map_fields = {1, 2, 3, 4};
        }
        bool use_field[5] = {false, false, false, false, false};
        S = ini.str("fields_use");
        if (!S.empty()) {
            for (auto &f : split_ws(S)) use_field[type_index(f[0])] = true;
        } else {
            if (!has_map_names) fail(CMBL_ERR_FORMAT, "CMBlikes: must have fields_use or map_names");
            for (int i = 1; i <= 4; i++) use_field[i] = true;
        }
        const int nm = (int)map_names.size();
        use_map.assign(nm, 0);
        S = ini.str("maps_use");
        if (!S.empty()) {
            for (auto &m : split_ws(S)) {
                const int j = map_index(m);
                if (j == -1) fail(CMBL_ERR_FORMAT, "CMBlikes: maps_use item not found - %s", m.c_str());
                use_map[j - 1] = 1;
            }
        } else {
            for (int i = 0; i < nm; i++) use_map[i] = use_field[map_fields[i]];
        }
        require_map = use_map;
        if (has_map_names) {
            S = ini.str("maps_required");
            if (ini.has("fields_required")) fail(CMBL_ERR_FORMAT, "CMBLikes: use maps_required not fields_required");
        } else {
            S = ini.str("fields_required");
        }
        for (auto &m : split_ws(S)) {
            const int j = map_index(m);
            if (j == -1) fail(CMBL_ERR_FORMAT, "CMBlikes: required item not found - %s", m.c_str());
            require_map[j - 1] = 1;
        }
        bool req_field[5] = {false, false, false, false, false};
        for (int i = 0; i < nm; i++)
            if (require_map[i]) req_field[map_fields[i]] = true;
        std::string la = ini.str_required("like_approx");
        if (la == "HL") approx = 1;
        else if (la == "gaussian") approx = 2;
        else if (la == "exact") approx = 3;
        else fail(CMBL_ERR_FORMAT, "CMBlikes: unknown like_approx %s", la.c_str());
        for (int i = 0; i < nm; i++) {
            nmaps += use_map[i];
            nreq += require_map[i];
        }
        if (nmaps < 1) fail(CMBL_ERR_FORMAT, "CMBlikes: no maps used");
        if (approx == 1 && nmaps > CL_MAXMAPS) fail(CMBL_ERR_UNSUPPORTED, "CMBlikes HL: at most %d maps", CL_MAXMAPS);
        if (approx == 3 && nmaps > EXACT_MAXMAPS)
            fail(CMBL_ERR_UNSUPPORTED, "CMBlikes exact: at most %d maps", EXACT_MAXMAPS);
        if (approx == 3 && bk) fail(CMBL_ERR_UNSUPPORTED, "BKPLANCK with like_approx = exact is not supported");
        if (approx == 3 && smica) fail(CMBL_ERR_UNSUPPORTED, "SMICA with like_approx = exact is not supported");
        if (nreq > CL_MAXREQ) fail(CMBL_ERR_UNSUPPORTED, "CMBlikes: at most %d required maps", CL_MAXREQ);
        map_required_index.assign(nm, 0);
        map_used_index.assign(nm, 0);
        int ix = 0;
        for (int i = 0; i < nm; i++)
            if (require_map[i]) {
                map_required_index[i] = ++ix;
                required_order.push_back(i + 1);
            }
        ix = 0;
        for (int i = 0; i < nm; i++)
            if (use_map[i]) {
                map_used_index[i] = ++ix;
                used_map_order.push_back(map_names[i]);
            }
        ncl = nmaps * (nmaps + 1) / 2;
        lmin = ini_int(ini, "cl_lmin", true, 0);
        lmax = ini_int(ini, "cl_lmax", true, 0);
        if (!ini.has("binned")) fail(CMBL_ERR_FORMAT, "CMBlikes: binned not given");   // Read_Logical('binned') :597
        binned = ini_logical(ini, "binned", false);
        aberration = ini_double(ini, "aberration_coeff", 0.0);
        if (binned) {
            if (approx == 3) fail(CMBL_ERR_FORMAT, "CMBLikes: exact like cannot be binned!");   // :1185
            nbins = ini_int(ini, "nbins", false, 0);
            bin_min = ini_int(ini, "use_min", false, 1);
            bin_max = ini_int(ini, "use_max", false, nbins);
            if (bin_min < 1 || bin_min > nbins || bin_max < bin_min || bin_max > nbins)
                fail(CMBL_ERR_FORMAT, "CMBlikes: use_min/use_max outside 1..nbins");
        } else {
            // unbinned (:601-605, :636-637): one "bin" per l; only the exact
            // likelihood (the reference marks unbinned HL / gaussian untested)
            if (approx != 3)
                fail(CMBL_ERR_UNSUPPORTED, "CMBlikes: unbinned HL / gaussian likelihoods are not supported "
                                           "(untested in the reference)");
            if (nmaps != nreq) fail(CMBL_ERR_FORMAT, "CMBlikes: Unbinned must have required==used");   // :1188
            nbins = lmax - lmin + 1;
            bin_min = ini_int(ini, "use_min", false, lmin);
            bin_max = ini_int(ini, "use_max", false, lmax);
            if (bin_min < lmin || bin_min > lmax || bin_max < bin_min || bin_max > lmax)
                fail(CMBL_ERR_FORMAT, "CMBlikes: use_min/use_max outside cl_lmin..cl_lmax");
            if (lmax - lmin < 2 && aberration != 0.0)
                fail(CMBL_ERR_FORMAT, "CMBlikes: aberration needs cl_lmax >= cl_lmin + 2");
        }
        nb = bin_max - bin_min + 1;
        if (binned) read_bin_windows(ini, "bin_window", bw);
        read_cl_arr(ini, "cl_hat", clhat, false);
        if (approx == 1) read_cl_arr(ini, "cl_fiducial", clfid, false);
        if (approx == 3) fksy = ini_double(ini, "fullsky_exact_fksy", 1.0);      // :645-648
        const bool includes_noise = ini_logical(ini, "cl_hat_includes_noise", false);
        if (approx != 2 || includes_noise) {
            read_cl_arr(ini, "cl_noise", clnoise, false);
            have_noise = true;
            if (!includes_noise) {
                for (size_t k = 0; k < clhat.size(); k++) clhat[k] = clhat[k] + clnoise[k];
            } else if (approx == 2) {
                for (size_t k = 0; k < clhat.size(); k++) clhat[k] = clhat[k] - clnoise[k];
                have_noise = false;
            }
        }
        for (int i = 1; i <= 4; i++)
            if (req_field[i]) cl_lmax[(i - 1) * 4 + (i - 1)] = lmax;
        if (req_field[1] && req_field[2]) cl_lmax[(2 - 1) * 4 + (1 - 1)] = lmax;
        if (ini.has("point_source_cl") || ini.has("beam_modes_file"))
            fail(CMBL_ERR_FORMAT, "dataset uses keywords no longer supported");
        bool fid_incl_noise = false;
        if (approx != 2) fid_incl_noise = ini_logical(ini, "cl_fiducial_includes_noise", false);
        // per-bin matrices (:711-724)
        chatM.resize((size_t)nb * nmaps * nmaps);
        cfh.resize((size_t)nb * nmaps * nmaps);
        auto to_matrix = [&](const double *X, double *M) {
            int q = 0;
            for (int i = 0; i < nmaps; i++)
                for (int j = 0; j <= i; j++, q++) M[i * nmaps + j] = M[j * nmaps + i] = X[q];
        };
        for (int b = 0; b < nb; b++) {
            to_matrix(&clhat[(size_t)b * ncl], &chatM[(size_t)b * nmaps * nmaps]);
            if (approx == 1) {
                std::vector<double> f(clfid.begin() + (size_t)b * ncl, clfid.begin() + (size_t)(b + 1) * ncl);
                if (!fid_incl_noise)
                    for (int k = 0; k < ncl; k++) f[k] = f[k] + clnoise[(size_t)b * ncl + k];
                std::vector<double> M((size_t)nmaps * nmaps);
                to_matrix(f.data(), M.data());
                sym_power(M, nmaps, 0.5);
                std::copy(M.begin(), M.end(), cfh.begin() + (size_t)b * nmaps * nmaps);
            }
        }
        if (approx != 3) read_covmat(ini);        // :726-728
        std::vector<double> fc;
        if (!binned && ini.has("linear_correction_fiducial_file"))
            fail(CMBL_ERR_UNSUPPORTED, "CMBlikes: linear corrections of an unbinned likelihood are not supported");
        if (read_cl_arr(ini, "linear_correction_fiducial", fc, true)) {
            fidcorr = fc;
            read_bin_windows(ini, "linear_correction_bin_window", cw);
        }
        std::string cp = ini.relative_filename("calibration_param", false);
        if (!cp.empty()) {
            nuisance_names = load_paramnames(cp, &n_nuis, &derived_names, &n_derived);
            cal_index = n_nuis - 1;
            log_cal_prior = ini_double(ini, "log_calibration_prior", -1.0);
        }
        // ---- Tsmica_planck_ReadIni (CMBlikes.f90:1281-1293): after the base ReadIni
        // (which may have set a calibration index from calibration_param), the
        // nuisance names are replaced by nuisance_params (loadParamNames ->
        // nuisance_params%init), and calibration_paramname, when given, sets the
        // calibration index to that name's position in them (ParamNames%Index:
        // -1, i.e. no calibration, for an unknown name)
        if (smica) {
            nuisance_names = load_paramnames(ini.relative_filename("nuisance_params", true), &n_nuis, &derived_names,
                                             &n_derived);
            if (n_nuis < 5) fail(CMBL_ERR_FORMAT, "SMICA: nuisance_params needs the foreground parameters A1 n1 n1run A2 n2");
            if (ini.has("calibration_paramname")) {
                const std::string cn = ini.str("calibration_paramname");
                const auto nm = split_ws(nuisance_names), dn = split_ws(derived_names);
                int ix = -1;
                for (size_t k = 0; k < nm.size() && ix < 0; k++)
                    if (nm[k] == cn) ix = (int)k;
                for (size_t k = 0; k < dn.size() && ix < 0; k++)
                    if (dn[k] == cn) fail(CMBL_ERR_FORMAT, "SMICA: calibration_paramname %s is a derived parameter", cn.c_str());
                cal_index = ix;   // -1: none
            }
        }
        // ---- TBK_planck_ReadIni (CMB_BK_Planck.f90:36-70).  As for SMICA, a
        // calibration_param read by the base ReadIni (:43) sets the calibration index
        // to its name count and loadParamNames (:46, nuisance_params%init) then replaces
        // the names: the index stays and points into the BK parameters
        if (bk) {
            nuisance_names = load_paramnames(ini.relative_filename("nuisance_params", true), &n_nuis);
            if (n_nuis < BK_NPARAM) fail(CMBL_ERR_FORMAT, "BKPLANCK: nuisance_params needs %d parameters", BK_NPARAM);
            fpivot_dust = ini_double(ini, "fpivot_dust", 353.0);
            fpivot_sync = ini_double(ini, "fpivot_sync", 23.0);
            decorr_dust[0] = ini_double(ini, "fpivot_dust_decorr(1)", 217.0);
            decorr_dust[1] = ini_double(ini, "fpivot_dust_decorr(2)", 353.0);
            decorr_sync[0] = ini_double(ini, "fpivot_sync_decorr(1)", 23.0);
            decorr_sync[1] = ini_double(ini, "fpivot_sync_decorr(2)", 33.0);
            auto lform = [&](const std::string &k) {
                std::string v = ini.str(k, "flat");
                return v == "lin" ? 1 : v == "quad" ? 2 : 0;
            };
            lform_dust = lform("lform_dust_decorr");
            lform_sync = lform("lform_sync_decorr");
            // the reference reads nmaps_required bandpasses named by used_map_order (:64-66),
            // which holds only the nmaps used maps: a required map beyond them has no defined
            // bandpass there, so the case is refused rather than given a meaning
            if (nreq != nmaps) fail(CMBL_ERR_UNSUPPORTED, "BKPLANCK: maps_required beyond maps_use not supported");
            const double G = ghz_kelvin();
            for (int i = 0; i < nreq; i++) {
                const std::string &mn = used_map_order[i];
                auto R = load_txt(ini.relative_filename("bandpass[" + mn + "]", true));
                const int n = (int)R.size();
                if (n < 2) fail(CMBL_ERR_FORMAT, "bandpass for %s too short", mn.c_str());
                BKMap m{};
                m.off = (int)bp_nu.size();
                m.n = n;
                std::vector<double> dnu(n);
                dnu[0] = R[1][0] - R[0][0];
                for (int k = 1; k < n - 1; k++) dnu[k] = (R[k + 1][0] - R[k - 1][0]) / 2;
                dnu[n - 1] = R[n - 1][0] - R[n - 2][0];
                double th_int = 0, s1 = 0, s2 = 0;
                for (int k = 0; k < n; k++) {
                    const double nu = R[k][0], r = R[k][1];
                    const double e = std::exp(G * nu / BK_TCMB);
                    th_int += dnu[k] * r * (nu * nu * nu * nu) * e / ((e - 1) * (e - 1));
                    s1 += dnu[k] * nu * r;
                    s2 += dnu[k] * r;
                    bp_nu.push_back(nu);
                    bp_R.push_back(r);
                    bp_dnu.push_back(dnu[k]);
                }
                auto th0 = [&](double nu0) {
                    const double e = std::exp(G * nu0 / BK_TCMB);
                    return (nu0 * nu0 * nu0 * nu0) * e / ((e - 1) * (e - 1));
                };
                m.th_dust = th_int / th0(fpivot_dust);
                m.th_sync = th_int / th0(fpivot_sync);
                m.nu_bar = s1 / s2;
                m.bc = mn.find("95") != std::string::npos ? 1 : mn.find("150") != std::string::npos ? 2
                       : mn.find("220") != std::string::npos ? 3 : 0;
                bkmaps.push_back(m);
            }
        }
    }
};
