// CMBlikes window stage: every window column as a dot product with one map spectrum.
// (included by cmblikes.hip inside namespace cmamd)
#pragma once

// Window contractions on the f64 MFMA.  One workgroup = 64 walkers x one work
// item (map pair, up to WK_NCH chunks of WK_CHUNK l, <= WK_COLS window columns):
//   partial[col][w] = sum_l Wt[l][col] MapCl_w(l)
// The walkers' map spectra MapCl_w(l) (GetTheoryMapCls + AdaptTheoryForMaps,
// CMBlikes.f90:1022-1126: aberration, foregrounds, calibration) are formed
// while staging each theory chunk into LDS from coalesced 16-byte row loads;
// the next chunk's loads are in flight during the current chunk's MFMAs.
// Each wave owns 16 walkers: v_mfma_f64_16x16x4f64 over (column block, 4 l).
// ABER / FG (the dataset's aberration / foreground switches) are template
// parameters so the lensing variant carries no foreground code.
template <bool ABER, bool FG>
__global__ __launch_bounds__(256) void cmbl_window_kernel(CLDev c, const double *__restrict__ dl, long long ld_field,
                                                         long long ld_walker, const double *__restrict__ nuis,
                                                         long long ld_nuis, const double *__restrict__ coef,
                                                         const double *__restrict__ prof, double *__restrict__ partial,
                                                         int W, int vec_ok)
{
    __shared__ __attribute__((aligned(16))) double wsh[WK_CHUNK * WK_COLS];   // weights [l][col]
    __shared__ __attribute__((aligned(16))) double tsh[64 * WK_TS];           // spectra [walker][l]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w0 = blockIdx.x * 64;
    const int Wc = live_walkers(c.wcount, W);
    if (w0 >= Wc) return;
    const WItem it = c.items[blockIdx.y];
    const CLPair pr = c.pairs[it.pair];
    const bool aber = ABER && c.aberration != 0.0 && pr.cmb;
    const bool fg = FG && pr.fg;
    // staging map: thread -> l pair q = tid % 32 of rows r_u = tid / 32 + 8 u (u < 8)
    constexpr int PER = 64 * (WK_CHUNK / 2) / 256;
    const int q = tid % (WK_CHUNK / 2), rbase = tid / (WK_CHUNK / 2);
    // per-walker constants of the thread's rows
    double calsq[PER];
    double dust[FG ? PER : 1], sync[FG ? PER : 1], dsync[FG ? PER : 1], ddf[FG ? PER : 1], dsf[FG ? PER : 1],
        nui[FG ? PER : 1], nuj[FG ? PER : 1], Ddust[FG ? PER : 1], Dsync[FG ? PER : 1];
    bool dd_l = false, ds_l = false;     // l-dependent decorrelation (lform lin / quad) in use
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int w = min(w0 + rbase + 8 * u, Wc - 1);
        const double *P = nuis + (long long)w * ld_nuis;
        const double cl = c.cal_index >= 0 ? P[c.cal_index] : 1.0;
        calsq[u] = cl * cl;
        if constexpr (FG) {
            dust[u] = sync[u] = dsync[u] = nui[u] = nuj[u] = 0.0;
            ddf[u] = dsf[u] = Ddust[u] = Dsync[u] = 1.0;
            if (fg && pr.fg != 3) {                           // :296-328
                const double *cw = coef + (long long)w * 3 * c.nreq;
                const int a = pr.mi, b = pr.mj;
                double d = cw[a] * cw[b], sy = cw[c.nreq + a] * cw[c.nreq + b];
                double ds = cw[a] * cw[c.nreq + b] + cw[c.nreq + a] * cw[b];
                if (pr.fg == 1) {
                    const double EEd = P[8], EEs = P[9];
                    d = d * EEd;
                    sy = sy * EEs;
                    ds = ds * sqrt(EEd * EEs);
                }
                dust[u] = d;
                sync[u] = sy;
                dsync[u] = ds;
                const double Delta_dust = P[10], Delta_sync = P[11];
                Ddust[u] = Delta_dust;
                Dsync[u] = Delta_sync;
                nui[u] = c.bkmaps[a].nu_bar * cw[2 * c.nreq + a];
                nuj[u] = c.bkmaps[b].nu_bar * cw[2 * c.nreq + b];
                // need_dust_decorr .and. i /= j (:288-289, :312); flat l-scaling is one factor per pair
                if (fabs(Delta_dust - 1) > 1e-5 && a != b) {
                    if (c.lform_dust == 0) ddf[u] = bk_decorr(Delta_dust, nui[u], nuj[u], c.decorr_dust, 0, 0);
                    else dd_l = true;
                } else {
                    Ddust[u] = 1.0;   // marks "no decorrelation" for this walker
                }
                if (fabs(Delta_sync - 1) > 1e-5 && a != b) {
                    if (c.lform_sync == 0) dsf[u] = bk_decorr(Delta_sync, nui[u], nuj[u], c.decorr_sync, 0, 0);
                    else ds_l = true;
                } else {
                    Dsync[u] = 1.0;
                }
            }
        }
    }
    double2 raw[PER];
    auto load_chunk = [&](int ch) {
        const int lq = it.l0 + ch * WK_CHUNK + 2 * q;
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int w = w0 + rbase + 8 * u;
            raw[u] = make_double2(0.0, 0.0);
            if (w < Wc && lq <= it.l1) {
                const double *Df = dl + (long long)w * ld_walker + (long long)pr.field * ld_field;
                if (vec_ok) {
                    raw[u] = *reinterpret_cast<const double2 *>(Df + lq);
                } else {
                    raw[u].x = Df[lq];
                    if (lq + 1 <= it.l1) raw[u].y = Df[lq + 1];
                }
            }
        }
    };
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const int li = lane & 15, lk = lane >> 4;
    const double *trow = tsh + (16 * wave + li) * WK_TS;
    load_chunk(0);
    for (int ch = 0; ch < it.nch; ch++) {
        {   // weights of this chunk (zero-padded to WK_COLS columns and WK_CHUNK l by the host)
            const double2 *src = reinterpret_cast<const double2 *>(c.wdense + it.woff) + ch * (WK_CHUNK * WK_COLS / 2);
            for (int i = tid; i < WK_CHUNK * WK_COLS / 2; i += 256) reinterpret_cast<double2 *>(wsh)[i] = src[i];
        }
        const int lq = it.l0 + ch * WK_CHUNK + 2 * q;
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int r = rbase + 8 * u, w = w0 + r;
            // a 16-byte load at lq == it.l1 also brought l1 + 1 (behind lmax: the caller's row padding);
            // its weight is 0, but 0 * NaN is NaN in the MFMA, so the slot holds 0
            double v2[2] = {raw[u].x, lq + 1 <= it.l1 ? raw[u].y : 0.0};
            if (w < Wc && lq <= it.l1) {
                const double *Df = dl + (long long)w * ld_walker + (long long)pr.field * ld_field;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int l = lq + h;
                    if (l > it.l1) break;
                    double v = v2[h];
                    if (aber) {                               // AddAberration :1062-1101
                        int la = l - 1, lb = l + 1;
                        if (l == c.lmin) { la = l; lb = l + 2; }
                        else if (l == c.lmax) { la = l - 2; lb = l; }
                        const double ea = la, eb = lb, el = l;
                        const double ca = Df[la] / (ea * (ea + 1)), cb = Df[lb] / (eb * (eb + 1));
                        const double deriv = 0.5 * (cb - ca);
                        v = v + c.aberration * (el * el * (el + 1) * deriv);
                    }
                    if constexpr (FG) {
                        if (fg && pr.fg == 3) {               // SMICA TT (CMBlikes.f90:1314-1317)
                            const double *pw = prof + (long long)w * 3 * c.LP + l;
                            v = v + pw[0];
                            v = v + pw[c.LP];
                        } else if (fg) {                      // :329-334
                            const double *pw = prof + (long long)w * 3 * c.LP + l;
                            const double Dd = (dd_l && Ddust[u] != 1.0)
                                                  ? bk_decorr(Ddust[u], nui[u], nuj[u], c.decorr_dust, l, c.lform_dust)
                                                  : ddf[u];
                            const double Ds = (ds_l && Dsync[u] != 1.0)
                                                  ? bk_decorr(Dsync[u], nui[u], nuj[u], c.decorr_sync, l, c.lform_sync)
                                                  : dsf[u];
                            v = v + dust[u] * pw[0] * Dd + sync[u] * pw[c.LP] * Ds + dsync[u] * pw[2 * c.LP];
                        }
                    }
                    if (c.cal_index >= 0 && pr.cmb) v = v / calsq[u];   // AdaptTheoryForMaps :1113-1124
                    v2[h] = v;
                }
            }
            tsh[r * WK_TS + 2 * q] = v2[0];
            tsh[r * WK_TS + 2 * q + 1] = v2[1];
        }
        if (ch + 1 < it.nch) load_chunk(ch + 1);          // in flight during this chunk's MFMAs
        __syncthreads();
        // A = Wt[col][k] (lane: col = lane&15, k = lane>>4); B = MapCl[k][walker] (walker = lane&15)
        const int clen = min(WK_CHUNK, it.l1 - (it.l0 + ch * WK_CHUNK) + 1);
        const int nk = (clen + 3) / 4;
        if (it.ncol > 16) {
            for (int s = 0; s < nk; s++) {
                const int k = 4 * s + lk;
                const double b = trow[k];
                const double a0 = wsh[k * WK_COLS + li];
                const double a1 = wsh[k * WK_COLS + 16 + li];
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc1, 0, 0, 0);
            }
        } else {                                            // one 16-column block suffices
            for (int s = 0; s < nk; s++) {
                const int k = 4 * s + lk;
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(wsh[k * WK_COLS + li], trow[k], acc0, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // D: walker = lane&15, col = (lane>>4) + 4 r
    const int w = w0 + 16 * wave + li;
    if (w < Wc) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int c0 = lk + 4 * r, c1 = 16 + lk + 4 * r;
            if (c0 < it.ncol) partial[(long long)(it.part + c0) * W + w] = acc0[r];
            if (c1 < it.ncol) partial[(long long)(it.part + c1) * W + w] = acc1[r];
        }
    }
}

// Window contraction without aberration or foregrounds (TBinWindows_bin
// :1230-1256 on GetTheoryMapCls :1022-1052).  The spectrum operand comes
// straight from global memory: lane (walker li, quarter kq) of a wave holds the
// 8 l {l0 + 32 st + 8 j + 2 kq + h : j < 4, h < 2} of its walker's spectrum in
// slot 2 j + h, and MFMA step s = 2 j + h contracts the four l {8 j + 2 kq + h};
// every load is a 16-byte vector, and the four kq lanes of a walker read 64
// contiguous bytes per load instruction (one half line, not four scattered
// quarters), and the next step's spectra are in flight during this step's MFMAs.  The weights
// (8 KB per 64 l) are shared by the block's four waves through a
// double-buffered LDS tile: read per wave from L2 they cost 24.2 vs 17.7 us per
// launch (lensing, W = 1024, MI355X).  The calibration (AdaptTheoryForMaps
// :1113-1124, D_l / cal^2 for T/E/B pairs) is linear and is applied to the
// sums.  Blocks are dealt to the 8 XCDs round-robin; the remap puts all walker
// tiles of an item on one XCD so its weights are fetched into one L2 (17.9 vs
// 18.7 us with the linear order; 17.5 vs 17.7 us against an XCD-balanced split).
__global__ __launch_bounds__(256) void cmbl_window_direct(CLDev c, const double *__restrict__ dl, long long ld_field,
                                                         long long ld_walker, const double *__restrict__ nuis,
                                                         long long ld_nuis, double *__restrict__ partial, int W,
                                                         int tiles, int vec_ok)
{
    constexpr int LPL = 8, STEP = 4 * LPL, NSUB = WK_CHUNK / STEP, WROW = STEP + 2;
    __shared__ __attribute__((aligned(16))) double wsh[2 * 2 * 16 * WROW];   // [buf][col block][col][l]
    // blocks are dealt to the XCDs round-robin: all walker tiles of an item on one XCD
    // (its weights in one L2); measured faster than an XCD-balanced split of the units
    const int b = blockIdx.x, xcd = b & 7, j = b >> 3;
    const int item = xcd + 8 * (j / tiles), tile = j % tiles;
    if (item >= c.nitem) return;
    const int Wc = live_walkers(c.wcount, W);
    if (tile * 64 >= Wc) return;
    const WItem it = c.items[item];
    const CLPair pr = c.pairs[it.pair];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int w = tile * 64 + wave * 16 + li;
    const int wl = min(w, Wc - 1);
    const double *Df = dl + (long long)wl * ld_walker + (long long)pr.field * ld_field;
    const int ncb = (it.ncol + 15) >> 4;
    const int nstep = it.nch * NSUB;
    double t[LPL], tn[LPL], tnn[LPL], a[LPL], a2[LPL];
    static_assert(LPL == 8, "slot 2 j + h holds l = 8 j + 2 kq + h");
    auto load_t = [&](int st, double *dst) {
        const int lb = it.l0 + st * STEP + 2 * kq;
        if (vec_ok && it.l0 + st * STEP + STEP - 1 <= it.l1) {
#pragma unroll
            for (int j = 0; j < LPL / 2; j++) {
                const double2 v = *reinterpret_cast<const double2 *>(Df + lb + 8 * j);
                dst[2 * j] = v.x;
                dst[2 * j + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < LPL / 2; j++)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int l = lb + 8 * j + h;
                    dst[2 * j + h] = (l <= it.l1) ? Df[l] : 0.0;
                }
        }
    };
    // weights [nch][ncb][16][WK_CHUNK]; thread tid moves column tid/16, l 2 (tid%16) .. +1
    auto wsrc = [&](int st, int cb) {
        const int ch = st / NSUB, sub = st % NSUB;
        return c.wdirect + it.woff2 + ((long long)ch * ncb + cb) * 16 * WK_CHUNK + sub * STEP;
    };
    const int wc = tid >> 4, wp = 2 * (tid & 15);
    double2 wr0, wr1;
    auto fetch_w = [&](int st) {
        wr0 = *reinterpret_cast<const double2 *>(wsrc(st, 0) + wc * WK_CHUNK + wp);
        if (ncb > 1) wr1 = *reinterpret_cast<const double2 *>(wsrc(st, 1) + wc * WK_CHUNK + wp);
    };
    auto store_w = [&](int buf) {
        *reinterpret_cast<double2 *>(wsh + ((buf * 2 + 0) * 16 + wc) * WROW + wp) = wr0;
        if (ncb > 1) *reinterpret_cast<double2 *>(wsh + ((buf * 2 + 1) * 16 + wc) * WROW + wp) = wr1;
    };
    auto read_w = [&](int buf, int cb, double *dst) {   // A operand: column li at the lane's LPL l
        const double *src = wsh + ((buf * 2 + cb) * 16 + li) * WROW + 2 * kq;
#pragma unroll
        for (int j = 0; j < LPL / 2; j++) {
            const double2 v = *reinterpret_cast<const double2 *>(src + 8 * j);
            dst[2 * j] = v.x;
            dst[2 * j + 1] = v.y;
        }
    };
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    // the spectra run two steps ahead (measured neutral: the read pattern itself
    // gives 4.2-4.5 TB/s here with the MFMAs removed, tools/membench2.hip 6.2)
    load_t(0, t);
    fetch_w(0);
    if (nstep > 1) load_t(1, tn);
    store_w(0);
    __syncthreads();
    for (int st = 0; st < nstep; st++) {
        const bool more = st + 1 < nstep;
        const int cur = st & 1;
        if (more) fetch_w(st + 1);                     // in flight across this step's MFMAs
        if (st + 2 < nstep) load_t(st + 2, tnn);
        read_w(cur, 0, a);
        if (ncb > 1) read_w(cur, 1, a2);
#pragma unroll
        for (int s = 0; s < LPL; s++) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], t[s], acc0, 0, 0, 0);
        if (ncb > 1) {
#pragma unroll
            for (int s = 0; s < LPL; s++) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[s], t[s], acc1, 0, 0, 0);
        }
        if (more) {
            store_w(cur ^ 1);      // buffer cur ^ 1 was last read before the previous barrier
            __syncthreads();
#pragma unroll
            for (int s = 0; s < LPL; s++) {
                t[s] = tn[s];
                tn[s] = tnn[s];
            }
        }
    }
    if (w < Wc) {
        double inv = 1.0;
        if (c.cal_index >= 0 && pr.cmb) {
            const double cl = nuis[(long long)w * ld_nuis + c.cal_index];
            inv = cl * cl;
        }
        // D: walker = lane&15, column = (lane>>4) + 4 r
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int c0 = kq + 4 * r, c1 = 16 + kq + 4 * r;
            if (c0 < it.ncol) partial[(long long)(it.part + c0) * W + w] = acc0[r] / inv;
            if (c1 < it.ncol) partial[(long long)(it.part + c1) * W + w] = acc1[r] / inv;
        }
    }
}

// BK foreground datasets (TBK_planck, CMB_BK_Planck.f90:229-340): every map pair
// p of a theory field reads the same four per-walker rows -- the theory D_l and
// the dust / sync / dust-sync l profiles of cmbl_bk_prologue -- and differs only
// in per-(pair, walker) SED coefficients:
//   MapCl_p(l) = D_l + (dust_p Pd(l) Dd_p(l) + sync_p Ps(l) Ds_p(l) + dsync_p Px(l))
// (the expression of cmbl_window_kernel's staging, :329-334 of the reference).
// A work item is (up to GP pairs of one field, <= GSEG l); the workgroup
// (64 walkers, 16 per wave) loads each lane's 4 consecutive l of the four rows
// once per 16-l step and forms every pair's MapCl in registers for
// v_mfma_f64_16x16x4f64 against that pair's <= 16 window columns, so a row
// element is read once per item instead of once per pair (78 B x B pairs for
// BK15).  l-dependent decorrelation (lform lin / quad with Delta /= 1) is
// evaluated per value, as in the staged kernel.

// LDEC: l-dependent decorrelation possible (lform_dust or lform_sync lin / quad);
// without it no pair's flags can be set, and the inner loop carries no
// decorrelation code (same arithmetic on the flags = 0 path)
template <bool LDEC>
__global__ __launch_bounds__(256, 2) void cmbl_window_group(CLDev c, const GItem *__restrict__ gitems, int ngitem,
                                                        const double *__restrict__ wts, const double *__restrict__ dl,
                                                        long long ld_field, long long ld_walker,
                                                        const double *__restrict__ nuis, long long ld_nuis,
                                                        const double *__restrict__ coef, const double *__restrict__ prof,
                                                        int LP, double *__restrict__ partial, int W, int tiles,
                                                        int vec_ok, int tile_xcd)
{
    constexpr int LPL = 4, STEP = 4 * LPL;
    // per-(pair, walker) SED coefficients: [GP][8][64] = dust, sync, dsync, ddf, dsf, nui, nuj, flags
    __shared__ double cf[GP][8][64];
    // the item's window weights of one step, double-buffered: [GP * 16 columns][STEP (+2 pad)]
    constexpr int WR = STEP + 2;
    __shared__ __attribute__((aligned(16))) double wsh[2][GP * 16 * WR];
    // blocks are dealt to the XCDs round-robin.  tile_xcd (tiles % 8 == 0): each XCD
    // owns tiles / 8 walker tiles and runs every item for them, so a walker's four
    // rows are fetched into one L2 (the items of one l segment re-read them once per
    // pair group); else all walker tiles of an item on one XCD (its weights in one L2)
    const int b = blockIdx.x, xcd = b & 7, j = b >> 3;
    int item, tile;
    if (tile_xcd) {
        const int tpx = tiles >> 3;
        tile = xcd + 8 * (j % tpx);
        item = j / tpx;
    } else {
        item = xcd + 8 * (j / tiles);
        tile = j % tiles;
    }
    if (item >= ngitem) return;
    const int Wc = live_walkers(c.wcount, W);
    if (tile * 64 >= Wc) return;
    const GItem &it = gitems[item];
    const int np = it.npair;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {   // staged kernel :226-258, one (walker, pair) per thread and pass
        const int ws = min(tile * 64 + lane, Wc - 1);
        const double *P = nuis + (long long)ws * ld_nuis;
        const double *cw = coef + (long long)ws * 3 * c.nreq;
        const double Delta_dust = P[10], Delta_sync = P[11];
        for (int g = wave; g < np; g += 4) {
            const CLPair pr = c.pairs[it.pair[g]];
            double d = 0.0, sy = 0.0, ds = 0.0, ddf = 1.0, dsf = 1.0, nui = 0.0, nuj = 0.0;
            int flags = 0;
            if (pr.fg) {
                const int a = pr.mi, bb = pr.mj;
                d = cw[a] * cw[bb];
                sy = cw[c.nreq + a] * cw[c.nreq + bb];
                ds = cw[a] * cw[c.nreq + bb] + cw[c.nreq + a] * cw[bb];
                if (pr.fg == 1) {
                    const double EEd = P[8], EEs = P[9];
                    d = d * EEd;
                    sy = sy * EEs;
                    ds = ds * sqrt(EEd * EEs);
                }
                nui = c.bkmaps[a].nu_bar * cw[2 * c.nreq + a];
                nuj = c.bkmaps[bb].nu_bar * cw[2 * c.nreq + bb];
                if (fabs(Delta_dust - 1) > 1e-5 && a != bb) {
                    if (c.lform_dust == 0) ddf = bk_decorr(Delta_dust, nui, nuj, c.decorr_dust, 0, 0);
                    else flags |= 1;
                }
                if (fabs(Delta_sync - 1) > 1e-5 && a != bb) {
                    if (c.lform_sync == 0) dsf = bk_decorr(Delta_sync, nui, nuj, c.decorr_sync, 0, 0);
                    else flags |= 2;
                }
            }
            cf[g][0][lane] = d;
            cf[g][1][lane] = sy;
            cf[g][2][lane] = ds;
            cf[g][3][lane] = ddf;
            cf[g][4][lane] = dsf;
            cf[g][5][lane] = nui;
            cf[g][6][lane] = nuj;
            cf[g][7][lane] = (double)flags;
        }
    }
    const int li = lane & 15, kq = lane >> 4;
    const int wr_ = wave * 16 + li;                // walker within the tile
    const int w = tile * 64 + wr_;
    const int wl = min(w, Wc - 1);
    const double *P = nuis + (long long)wl * ld_nuis;
    const double Delta_dust = P[10], Delta_sync = P[11];
    const double *Df = dl + (long long)wl * ld_walker + (long long)it.field * ld_field;
    const double *pw = prof + (long long)wl * 3 * LP;
    double t[4][LPL], tn[4][LPL];
    auto load = [&](int st, double (*dst)[LPL]) {
        const int lb = it.l0 + st * STEP + LPL * kq;
        if (vec_ok && lb + LPL - 1 <= c.lmax) {
#pragma unroll
            for (int s = 0; s < LPL / 2; s++) {
                const double2 v0 = reinterpret_cast<const double2 *>(Df + lb)[s];
                const double2 v1 = reinterpret_cast<const double2 *>(pw + lb)[s];
                const double2 v2 = reinterpret_cast<const double2 *>(pw + LP + lb)[s];
                const double2 v3 = reinterpret_cast<const double2 *>(pw + 2 * LP + lb)[s];
                dst[0][2 * s] = v0.x; dst[0][2 * s + 1] = v0.y;
                dst[1][2 * s] = v1.x; dst[1][2 * s + 1] = v1.y;
                dst[2][2 * s] = v2.x; dst[2][2 * s + 1] = v2.y;
                dst[3][2 * s] = v3.x; dst[3][2 * s + 1] = v3.y;
            }
            // an item of an odd first l starts at the even lmin - 1: zero weights and zero profiles
            // there, but the theory entry is the caller's, and 0 * NaN is NaN in the MFMA
            if (lb < c.lmin) dst[0][0] = 0.0;
        } else {
#pragma unroll
            for (int s = 0; s < LPL; s++) {
                const int l = lb + s;
                const bool ok = l <= c.lmax;
                dst[0][s] = ok && l >= c.lmin ? Df[l] : 0.0;
                dst[1][s] = ok ? pw[l] : 0.0;
                dst[2][s] = ok ? pw[LP + l] : 0.0;
                dst[3][s] = ok ? pw[2 * LP + l] : 0.0;
            }
        }
    };
    f64x4 acc[GP];
#pragma unroll
    for (int g = 0; g < GP; g++) acc[g] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int Lp = it.nstep * 32;
    const int nst = it.nstep * (32 / STEP);
    // weights of step st: GP*16 rows of STEP doubles; thread q moves rows q / (STEP/2) ...
    constexpr int NW2 = GP * 16 * STEP / 2, PERT = NW2 / 256;
    double2 wr[PERT];
    auto fetch_w = [&](int st) {
#pragma unroll
        for (int u = 0; u < PERT; u++) {
            const int q = tid + 256 * u, row = q / (STEP / 2), c2 = q % (STEP / 2);
            wr[u] = row < np * 16 ? reinterpret_cast<const double2 *>(wts + it.woff + (long long)row * Lp + st * STEP)[c2]
                                  : make_double2(0.0, 0.0);
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int u = 0; u < PERT; u++) {
            const int q = tid + 256 * u, row = q / (STEP / 2), c2 = q % (STEP / 2);
            *reinterpret_cast<double2 *>(&wsh[buf][row * WR + 2 * c2]) = wr[u];
        }
    };
    load(0, t);
    fetch_w(0);
    store_w(0);
    __syncthreads();
    for (int st = 0; st < nst; st++) {
        const bool more = st + 1 < nst;
        const int cur = st & 1;
        if (more) {                                    // in flight across this step's MFMAs
            load(st + 1, tn);
            fetch_w(st + 1);
        }
        const int lr = st * STEP + LPL * kq;
#pragma unroll
        for (int g = 0; g < GP; g++) {
            if (g >= np) break;
            const double *src = &wsh[cur][(g * 16 + li) * WR + LPL * kq];
            const double2 q0 = reinterpret_cast<const double2 *>(src)[0], q1 = reinterpret_cast<const double2 *>(src)[1];
            const double a[LPL] = {q0.x, q0.y, q1.x, q1.y};
            const double dg = cf[g][0][wr_], sg = cf[g][1][wr_], xg = cf[g][2][wr_];
            const int flags = (int)cf[g][7][wr_];
#pragma unroll
            for (int s = 0; s < LPL; s++) {
                double Dd = cf[g][3][wr_], Ds = cf[g][4][wr_];
                if (LDEC && flags) {
                    const int l = it.l0 + lr + s;
                    if (flags & 1) Dd = bk_decorr(Delta_dust, cf[g][5][wr_], cf[g][6][wr_], c.decorr_dust, l, c.lform_dust);
                    if (flags & 2) Ds = bk_decorr(Delta_sync, cf[g][5][wr_], cf[g][6][wr_], c.decorr_sync, l, c.lform_sync);
                }
                const double v = t[0][s] + (dg * t[1][s] * Dd + sg * t[2][s] * Ds + xg * t[3][s]);
                acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], v, acc[g], 0, 0, 0);
            }
        }
        if (more) {
            store_w(cur ^ 1);          // buffer cur ^ 1 was last read before the previous barrier
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int s = 0; s < LPL; s++) t[q][s] = tn[q][s];
        }
    }
    if (w < Wc) {
#pragma unroll
        for (int g = 0; g < GP; g++) {
            if (g >= np) break;
            double inv = 1.0;
            if (c.cal_index >= 0 && c.pairs[it.pair[g]].cmb) {
                const double cl = P[c.cal_index];
                inv = cl * cl;
            }
            // D: walker = lane & 15, column = (lane >> 4) + 4 r
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int col = kq + 4 * r;
                if (col < it.ncol[g]) partial[(long long)(it.part[g] + col) * W + w] = acc[g][r] / inv;
            }
        }
    }
}
