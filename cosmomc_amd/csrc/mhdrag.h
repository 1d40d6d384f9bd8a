// The fast-dragging kernels.  Included by sampler.hip after mhpropose.h and
// mhstage.h.
// (included inside namespace cmamd)
#pragma once

// ---------------------------------------------------------------- fast dragging
// TFastDraggingSampler_GetNewSample (MCMC.f90:338-452) in four launch stages,
// one thread per walker on the walker state in HBM (the drag scratch lives in
// separate rows, DragCfg::dd / di, so the Metropolis kernel's LDS image is
// unchanged).  Between stages the host evaluates the likelihoods:
//   set 1 at the trial-end rows T on the END slow point's theory,
//   set 2 at the trial-start rows T2 on the walker's current theory.
//   stage 0  TrialEnd = Cur + GetProposalSlow                        (:367-368)
//   stage 1  CurEndLike; abort on logZero (:370-374); first delta    (:386-394)
//   stage 2  interpolated Metropolis on (start, end) likes, sums; next delta,
//            or (last step) the drag accept + MoveDone                (:395-452)
// dst: 0 idle, 1 dragging, 2 aborted, 3 skipped (CurLike == logZero),
//      4 accepted (the walker's theory must become the end theory)
struct DragCfg {
    double *dd;      // [3 np + 4 + max_blk + n_like][ld]: CE, CS, T2, (cel, csl, ss, se), vec scratch,
                     //   per-likelihood terms at CE
    int *di;         // [1 + all_n][ld]: dst, RandIndices scratch
    int interp, istep;
    const double *like_terms2;            // [n_like][ld] at T2
    double *like_nuis2[MAXLIKE];          // [W][nn] DataParams at T2
};

// One walker's part of a drag stage (TFastDraggingSampler_GetNewSample,
// MCMC.f90:338-452) on views of its state: in HBM (drag_kernel) or in an LDS
// image (drag_staged_kernel).  STAGE 0 proposes the slow trial, 1 scores the
// end point, 2 runs interpolation step g.istep.
struct DragView {
    Col<double> T, CE, CS, T2, ET, lk1, lk2;
    double *cur, *mult, *cel, *csl, *ss, *se;
    int *nacc, *dst;
};

template <int STAGE>
__device__ __forceinline__ void drag_logic(const DevCfg &c, const DragCfg &g, const Tabs &t, Walker &k,
                                           const DragView &v, int w, double *hist_row, double *hist_terms)
{
    const size_t ld = c.ld;
    const int np = c.np;
    const Col<double> T = v.T, CE = v.CE, CS = v.CS, T2 = v.T2, ET = v.ET, lk1 = v.lk1, lk2 = v.lk2;
    double &cur = *v.cur;
    double &mult = *v.mult;
    int &nacc = *v.nacc;
    double &cel = *v.cel;
    double &csl = *v.csl;
    double &ss = *v.ss;
    double &se = *v.se;
    int &dst = *v.dst;
    auto keep_end_terms = [&]() {
        for (int l = 0; l < c.n_like; l++) ET[l] = lk1[l];
    };

    auto scatter = [&]() {            // DataParams of both trial points
        for (int l = 0; l < c.n_like; l++)
            for (int q = 0; q < c.like_nn[l]; q++) {
                c.like_nuis[l][(size_t)w * c.like_nn[l] + q] = T[t.ti[c.like_nidx[l] + q]];
                g.like_nuis2[l][(size_t)w * c.like_nn[l] + q] = T2[t.ti[c.like_nidx[l] + q]];
            }
    };
    auto next_delta = [&]() {         // GetProposalFastDelta (propose.f90:291-298) on both ends
        Col<double> keep = k.trial;
        for (int i = 0; i < np; i++) T2[i] = 0.0;
        k.trial = T2;
        proposal_fast(c, t, k);
        k.trial = keep;
        for (int i = 0; i < np; i++) {
            const double d = T2[i];
            T[i] = CE[i] + d;
            T2[i] = CS[i] + d;
        }
    };
    auto metropolis = [&](double like, double curl) {   // MCMC.f90:119-131
        if (like == LOGZERO) return false;
        bool a = curl > like;
        if (!a) a = (double)randexp1(k.r) > like - curl;
        return a;
    };

    if (STAGE == 0) {
        if (cur == LOGZERO) {
            dst = 3;
        } else {
            dst = 1;
            for (int i = 0; i < np; i++) {
                T[i] = k.P[i];
                CS[i] = k.P[i];
                T2[i] = k.P[i];
            }
            csl = cur;
            proposal_slow(c, t, k);
        }
        scatter();
    } else if (STAGE == 1) {
        if (dst == 1) {
            cel = target_like(c, t, T, lk1);
            if (cel == LOGZERO) {
                dst = 2;
                mult += 1.0;
            } else {
                for (int i = 0; i < np; i++) CE[i] = T[i];
                keep_end_terms();
                ss = csl;
                se = cel;
                next_delta();
            }
        }
        scatter();
    } else {
        if (dst == 1) {
            const double el = target_like(c, t, T, lk1);
            bool acc = el != LOGZERO;
            double sl = 0.0;
            if (acc) {
                sl = target_like(c, t, T2, lk2);
                acc = sl != LOGZERO;
                if (acc) {
                    const double frac = (double)g.istep / g.interp;
                    const double cint = csl * (1 - frac) + frac * cel;
                    const double ilike = sl * (1 - frac) + frac * el;
                    acc = metropolis(ilike, cint);
                }
            }
            if (acc) {
                for (int i = 0; i < np; i++) {
                    CE[i] = T[i];
                    CS[i] = T2[i];
                }
                cel = el;
                csl = sl;
                keep_end_terms();
            }
            ss = ss + csl;
            se = se + cel;
            if (g.istep < g.interp - 1) {
                next_delta();
            } else {
                const double cur_drag = ss / g.interp, drag = se / g.interp;
                if (metropolis(drag, cur_drag)) {        // MoveDone :166-190 + :437-445
                    if (mult > 0) nacc += 1;
                    mult = 1.0;
                    for (int i = 0; i < np; i++) k.P[i] = CE[i];
                    cur = cel;
                    for (int l = 0; l < c.n_like; l++) c.cur_terms[(size_t)l * ld + w] = ET[l];
                    dst = 4;
                } else {
                    mult += 1.0;
                    dst = 0;
                }
            }
        }
        if (g.istep < g.interp - 1) {
            scatter();
        } else {
            if (dst == 2 || dst == 3) dst = 0;
            if (hist_row)
            {
                for (int i = 0; i < c.n_used; i++) hist_row[(size_t)i * c.W + w] = k.P[t.params_used[i]];
                hist_row[(size_t)c.n_used * c.W + w] = cur;
            }
            if (hist_terms)
                for (int l = 0; l < c.n_like; l++) hist_terms[(size_t)l * c.W + w] = c.cur_terms[(size_t)l * ld + w];
        }
    }
}

template <int STAGE>
__global__ __launch_bounds__(64) void drag_kernel(DevCfg c, DragCfg g, double *hist_row, double *hist_terms)
{
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= c.W) return;
    const size_t ld = c.ld;
    const Rows &R = c.rows;
    const int np = c.np;
    auto drow = [&](double *b, int r) { return Col<double>{b + (size_t)r * ld + w, (int)ld}; };
    auto irow = [&](int *b, int r) { return Col<int>{b + (size_t)r * ld + w, (int)ld}; };
    const Tabs t = make_tabs(c, c.tab_i, c.tab_d);
    Walker k;
    k.r.u = drow(c.sd, R.U);
    k.r.c = c.sd[(size_t)R.C * ld + w];
    k.r.gset = c.sd[(size_t)R.G * ld + w];
    k.r.i97 = c.si[(size_t)R.I97 * ld + w];
    k.r.j97 = c.si[(size_t)R.J97 * ld + w];
    k.r.iset = c.si[(size_t)R.ISET * ld + w];
    k.R = drow(c.sd, R.R);
    k.P = drow(c.sd, R.P);
    k.trial = drow(c.sd, R.T);
    k.vec = drow(g.dd, 3 * np + 4);
    k.cyc = irow(c.si, R.CYC);
    k.cyclp = irow(c.si, R.CYCLP);
    k.blklp = irow(c.si, R.BLKLP);
    k.itmp = irow(g.di, 1);
    k.fast_ix = c.si[(size_t)R.FASTIX * ld + w];
    DragView v;
    v.T = k.trial;
    v.CE = drow(g.dd, 0);
    v.CS = drow(g.dd, np);
    v.T2 = drow(g.dd, 2 * np);
    v.ET = drow(g.dd, 3 * np + 4 + c.max_blk);   // terms at CE
    v.lk1 = Col<double>{const_cast<double *>(c.like_terms) + w, (int)ld};
    v.lk2 = Col<double>{const_cast<double *>(g.like_terms2) + w, (int)ld};
    v.cur = c.sd + (size_t)R.L * ld + w;
    v.mult = c.sd + (size_t)R.M * ld + w;
    v.nacc = c.si + (size_t)R.NACC * ld + w;
    v.cel = g.dd + (size_t)(3 * np + 0) * ld + w;
    v.csl = g.dd + (size_t)(3 * np + 1) * ld + w;
    v.ss = g.dd + (size_t)(3 * np + 2) * ld + w;
    v.se = g.dd + (size_t)(3 * np + 3) * ld + w;
    v.dst = g.di + w;
    drag_logic<STAGE>(c, g, t, k, v, w, hist_row, hist_terms);
    c.sd[(size_t)R.C * ld + w] = k.r.c;
    c.sd[(size_t)R.G * ld + w] = k.r.gset;
    c.si[(size_t)R.I97 * ld + w] = k.r.i97;
    c.si[(size_t)R.J97 * ld + w] = k.r.j97;
    c.si[(size_t)R.ISET * ld + w] = k.r.iset;
    c.si[(size_t)R.FASTIX * ld + w] = k.fast_ix;
}

// The same stage on an LDS image of MB walkers' state (mh_kernel's staging:
// the sampler rows, the drag rows, both likelihood-term sets and the tables by
// LDS-DMA, one wait), so the chain's dependent reads are LDS round trips
// instead of HBM ones; then the image is written back.  Used when the image
// fits (drag_lds_bytes).
__host__ __device__ inline int drag_rows(const DevCfg &c) { return 3 * c.np + 4 + c.max_blk + c.n_like; }

template <int STAGE>
__global__ __launch_bounds__(MH_THREADS) void drag_staged_kernel(DevCfg c, DragCfg g, double *hist_row,
                                                                 double *hist_terms)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const Rows &R = c.rows;
    const int lane = threadIdx.x % MB;
    const int wl64 = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = MH_THREADS / 64;
    const int wb = blockIdx.x * MB;
    const int w = wb + lane;
    const size_t W = c.ld;
    const int np = c.np;
    const int nlk = (c.n_like + 1) & ~1;            // LDS rows (even); nl, nr of them are moved
    const int nl = c.n_like;
    const int nr = drag_rows(c);
    const int ndd = (nr + 1) & ~1;
    const int nd_st = c.stage_R ? R.ND : R.ND - R.RR;
    const int ni_st = c.stage_cyc ? R.NI : R.CYC;
    const int ntd = c.stage_cov ? c.tl.n_dbl : c.tl.covinv;
    const bool skipR = !c.stage_R;
    double *sd = lds;                                        // [nd_st][MB]
    double *dd = sd + (size_t)nd_st * MB;                    // [ndd][MB] drag rows
    double *l1 = dd + (size_t)ndd * MB;                      // [nlk][MB] terms at T
    double *l2 = l1 + (size_t)nlk * MB;                      // [nlk][MB] terms at T2
    double *td = l2 + (size_t)nlk * MB;                      // [ntd rounded to 32]
    int *si = reinterpret_cast<int *>(td + ((ntd + 31) & ~31));   // [ni_st][MB]
    int *dst_l = si + (size_t)ni_st * MB;                    // [4][MB] dst (row 0)
    int *it = dst_l + 4 * MB;                                // [all_n][MB] RandIndices scratch
    int *ti = it + (size_t)c.all_n * MB;                     // [n_int rounded to 64]
#define SROW(r) ((skipR && (r) >= R.R) ? (r) - R.RR : (r))
    const int rEnd = R.R + R.RR;
    if (skipR) {
        dma_rows_f64(sd, 0, c.sd, 0, R.R, W, wb, wl64, wave, nwave);
        dma_rows_f64(sd, R.R, c.sd, rEnd, R.ND - rEnd, W, wb, wl64, wave, nwave);
    } else {
        dma_rows_f64(sd, 0, c.sd, 0, R.ND, W, wb, wl64, wave, nwave);
    }
    dma_rows_f64(dd, 0, g.dd, 0, nr, W, wb, wl64, wave, nwave);
    dma_rows_f64(l1, 0, c.like_terms, 0, nl, W, wb, wl64, wave, nwave);
    dma_rows_f64(l2, 0, g.like_terms2, 0, nl, W, wb, wl64, wave, nwave);
    dma_rows_i32(si, c.si, ni_st, W, wb, wl64, wave, nwave);
    dma_rows_i32(dst_l, g.di, 1, W, wb, wl64, wave, nwave);
    dma_words(td, c.tab_d, 2 * ntd, wl64, wave, nwave);
    dma_words(ti, c.tab_i, c.tl.n_int, wl64, wave, nwave);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x < MB && w < c.W) {
        const Tabs t = make_tabs(c, ti, td, c.stage_cov ? td : c.tab_d);
        auto lrow = [&](double *b, int r) { return Col<double>{b + (size_t)r * MB + lane, MB}; };
        Walker k;
        k.r.u = lrow(sd, R.U);
        k.r.c = sd[(size_t)R.C * MB + lane];
        k.r.gset = sd[(size_t)R.G * MB + lane];
        k.r.i97 = si[(size_t)R.I97 * MB + lane];
        k.r.j97 = si[(size_t)R.J97 * MB + lane];
        k.r.iset = si[(size_t)R.ISET * MB + lane];
        k.R = c.stage_R ? lrow(sd, R.R) : Col<double>{c.sd + (size_t)R.R * W + w, c.ld};
        k.P = lrow(sd, SROW(R.P));
        k.trial = lrow(sd, SROW(R.T));
        k.vec = lrow(dd, 3 * np + 4);
        k.cyc = c.stage_cyc ? Col<int>{si + (size_t)R.CYC * MB + lane, MB} : Col<int>{c.si + (size_t)R.CYC * W + w, c.ld};
        k.cyclp = Col<int>{si + (size_t)R.CYCLP * MB + lane, MB};
        k.blklp = Col<int>{si + (size_t)R.BLKLP * MB + lane, MB};
        k.itmp = Col<int>{it + lane, MB};
        k.fast_ix = si[(size_t)R.FASTIX * MB + lane];
        DragView v;
        v.T = k.trial;
        v.CE = lrow(dd, 0);
        v.CS = lrow(dd, np);
        v.T2 = lrow(dd, 2 * np);
        v.ET = lrow(dd, 3 * np + 4 + c.max_blk);
        v.lk1 = lrow(l1, 0);
        v.lk2 = lrow(l2, 0);
        v.cur = sd + (size_t)SROW(R.L) * MB + lane;
        v.mult = sd + (size_t)SROW(R.M) * MB + lane;
        v.nacc = si + (size_t)R.NACC * MB + lane;
        v.cel = dd + (size_t)(3 * np + 0) * MB + lane;
        v.csl = dd + (size_t)(3 * np + 1) * MB + lane;
        v.ss = dd + (size_t)(3 * np + 2) * MB + lane;
        v.se = dd + (size_t)(3 * np + 3) * MB + lane;
        v.dst = dst_l + lane;
        const int i97_0 = k.r.i97;
        drag_logic<STAGE>(c, g, t, k, v, w, hist_row, hist_terms);
        dst_l[MB + lane] = k.r.nd < 97 ? k.r.nd : 97;   // rows 1, 2: the ring entries the draws overwrote
        dst_l[2 * MB + lane] = i97_0;
        sd[(size_t)R.C * MB + lane] = k.r.c;
        sd[(size_t)R.G * MB + lane] = k.r.gset;
        si[(size_t)R.I97 * MB + lane] = k.r.i97;
        si[(size_t)R.J97 * MB + lane] = k.r.j97;
        si[(size_t)R.ISET * MB + lane] = k.r.iset;
        si[(size_t)R.FASTIX * MB + lane] = k.fast_ix;
    }
    __syncthreads();
    // of the RANMAR ring only the entries this stage's draws overwrote
    // (positions i97 - 1, i97 - 2, ... mod 97 of the first index), as mh_body:
    // the stages 63.4-63.8 against 63.8-67.4 us a drag step (round 6, DESIGN.md section 5's table)
    if (w < c.W) {
        const int nd = dst_l[MB + lane], i0 = dst_l[2 * MB + lane];
        for (int q = threadIdx.x / MB; q < nd; q += NV) {
            int p = i0 - 1 - q;
            if (p < 0) p += 97;
            c.sd[(size_t)(R.U + p) * W + w] = sd[(size_t)(R.U + p) * MB + lane];
        }
    }
    if (skipR) {
        stage_out(c.sd, sd, R.C, R.C, R.R, W, wb);
        stage_out(c.sd, sd, R.R, rEnd, R.ND, W, wb);
    } else {
        stage_out(c.sd, sd, R.C, R.C, R.ND, W, wb);
    }
    stage_out(g.dd, dd, 0, 0, nr, W, wb);
    stage_out(c.si, si, 0, 0, ni_st, W, wb);
    stage_out(g.di, dst_l, 0, 0, 1, W, wb);
#undef SROW
}

// accepted moves: the trial (end) slow point's theory becomes the walker's theory
// (flag[w] == value: drag_kernel dst 4, or the Metropolis accept flag row)
__global__ void drag_swap_theory(const int *flag, int value, int W, const double *src, long long src_ld,
                                 double *dstth, long long dst_ld, long long n)
{
    const int w = blockIdx.y;
    if (w >= W || flag[w] != value) return;
    const double *a = src + (long long)w * src_ld;
    double *d = dstth + (long long)w * dst_ld;
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {   // 16-byte moves
        const long long n2 = n / 2;
        for (long long i = t; i < n2; i += stride)
            reinterpret_cast<double2 *>(d)[i] = reinterpret_cast<const double2 *>(a)[i];
        if (t == 0 && (n & 1)) d[n - 1] = a[n - 1];
    } else {
        for (long long i = t; i < n; i += stride) d[i] = a[i];
    }
}
