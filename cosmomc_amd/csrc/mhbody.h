// The general Metropolis chain (any blocks, any likelihood set): accept the
// pending trial and propose the next one out of an LDS image of the walker
// state.  Included by sampler.hip after mhlean.h, which it dispatches to.
// (included inside namespace cmamd)
#pragma once

// One launch per Metropolis step boundary: accept/reject the pending trial
// (MetropolisAccept MCMC.f90:119-131 + MoveDone :166-190), then propose the
// next trial (GetProposal / GetProposalFast) and scatter its nuisance
// parameters for the likelihood kernels.  MB walkers per block.
// tw: the unified step launch's wait (mh_step_kernel), else null
template <bool ACCEPT, bool PROPOSE>
__device__ __forceinline__ void mh_body(const DevCfg &c, int fast_only, double *hist_row, double *hist_terms, int blk0,
                                        double *lds, int bx, const TailWait *tw = nullptr)
{
    if (c.lean.on) {   // a single one-parameter fast block (mhlean.h)
        mh_lean<ACCEPT, PROPOSE>(c, hist_row, hist_terms, blk0, lds, bx, tw);
        return;
    }
    const Rows &R = c.rows;
    const int lane = threadIdx.x % MB, grp = threadIdx.x / MB;    // walker in block, thread group
    const int wl64 = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = MH_THREADS / 64;
    const int wb = (blk0 + bx) * MB;
    const int w = wb + lane;
    const bool act = w < c.W;
    const size_t W = c.ld;
    const int nlk = (c.n_like + 1) & ~1;
    // LDS carve: state doubles | like terms | vec scratch | tables(d) | state ints | itmp | tables(i)
    const int nd_st = c.stage_R ? R.ND : R.ND - R.RR;           // staged double rows
    const int ni_st = c.stage_cyc ? R.NI : R.CYC;                // staged int rows
    const int ntd = c.stage_cov ? c.tl.n_dbl : c.tl.covinv;      // staged double-table words
    double *sd = lds;                                            // [nd_st][MB]
    double *lk = sd + (size_t)nd_st * MB;                        // [nlk][MB]
    double *vc = lk + (size_t)nlk * MB;                          // [max_blk][MB]
    double *tq = vc + (size_t)c.max_blk * MB;                    // [tq_rows][MB] test-Gaussian row sums / block
    double *dq = tq + (size_t)c.tq_rows * MB;                    // [def_cap][QF_GROUPS + 1][MB] deferred combines
    double *td = dq + (size_t)c.def_cap * (QF_GROUPS + 1) * MB;  // [ntd rounded to 32]
    int *si = reinterpret_cast<int *>(td + ((ntd + 31) & ~31));  // [ni_st][MB]
    int *it = si + (size_t)ni_st * MB;                           // [all_n][MB] when stage_cyc
    int *ti = it + (size_t)(c.stage_cyc ? c.all_n : 0) * MB;     // [n_int rounded to 64]
    int *oobw = ti + ((c.tl.n_int + 63) & ~63);                  // [MB] trial out of bounds (par_prior)
    double *zz = reinterpret_cast<double *>(oobw + MB);          // [np][MB] the trial's squared prior z (par_prior)
    int *ndw = reinterpret_cast<int *>(zz + (size_t)c.np * MB);  // [MB] ring entries the chain's draws wrote
    int *i0w = ndw + MB;                                         // [MB] the ring index before them
    if (threadIdx.x < MB) oobw[threadIdx.x] = 0;
    // the rotation list of this walker range: this launch appends to counter
    // rot_par; the other one (read by the previous step's rot_kernel) restarts
    if (PROPOSE && c.rot_defer && bx == 0 && threadIdx.x == 0)
        c.rot_cnt[2 * (blk0 * MB / 64) + (c.rot_par ^ 1)] = 0;
    const bool skipR = !c.stage_R;
    // staged double row index of global row r (rotation rows dropped when not staged)
#define SROW(r) ((skipR && (r) >= R.R) ? (r) - R.RR : (r))

    STAMP(0);
    // every wave issues the LDS-DMA of the state image; lanes 0..MB-1 of wave
    // 0 alone run the chain logic; every thread group writes the image back
    const int rEnd = R.R + R.RR;
    if (skipR) {
        dma_rows_f64(sd, 0, c.sd, 0, R.R, W, wb, wl64, wave, nwave);
        dma_rows_f64(sd, R.R, c.sd, rEnd, R.ND - rEnd, W, wb, wl64, wave, nwave);
    } else {
        dma_rows_f64(sd, 0, c.sd, 0, R.ND, W, wb, wl64, wave, nwave);
    }
    dma_rows_i32(si, c.si, ni_st, W, wb, wl64, wave, nwave);
    dma_words(td, c.tab_d, 2 * ntd, wl64, wave, nwave);
    dma_words(ti, c.tab_i, c.tl.n_int, wl64, wave, nwave);
    // fast-only proposals with R in HBM: the only fast block's next column
    // (R(:, lp + 1) when no rotation is due) fetched into the vec rows by the
    // thread groups (proposal_tail then skips its own read; a block that
    // rotates writes R only in rot_kernel).  When the host knows the loop
    // index (pre_lp) the loads go out here, beside the image; otherwise after
    // it, from the staged index
    const bool pre_col = PROPOSE && fast_only && !c.stage_R && c.pre_blk >= 0;
    constexpr int NRQ = (MAXBLK + NV - 1) / NV;
    double rq[NRQ];
    int col = -1, ncol = 0;
    const bool rq_early = pre_col && c.pre_lp >= 0;
    if (rq_early && act) {
        ncol = c.pre_n;
        if (c.pre_lp % ncol != 0) col = c.pre_off + c.pre_lp;
#pragma unroll
        for (int u = 0; u < NRQ; u++) {
            const int q = grp + u * NV;
            if (col >= 0 && q < ncol) rq[u] = c.sd[(size_t)(R.R + col + q * ncol) * W + w];
        }
    }
    if (tw) tail_wait(*tw, wb / 64);   // the trial's terms below come from this launch's producers
    dma_rows_f64(lk, 0, c.like_terms, 0, nlk, W, wb, wl64, wave, nwave);
    // per-likelihood terms of the current point, for the history (rejected walkers keep theirs)
    double ct[MAXLIKE];
    if (ACCEPT && hist_terms && grp == 0 && act) {
#pragma unroll
        for (int l = 0; l < MAXLIKE; l++)
            if (l < c.n_like) ct[l] = c.cur_terms[(size_t)l * W + w];
    }
    // deferred split-K combines: the 16 group sums of this walker tile's
    // partials, one group per wave, loaded beside the state image
    if (ACCEPT && c.n_def) {   // group g sums split-K group g of this block's walkers (columns wb % 64 + lane of the tile)
        const int tile = wb / QF_TILE, col = wb % QF_TILE + lane;
        for (int d = 0; d < MAXDEF; d++) {
            if (d >= c.n_def) break;
            const double *tp = c.def_part[d] + (size_t)tile * c.def_items[d] * QF_TILE;
            double *row = dq + (size_t)d * (QF_GROUPS + 1) * MB;
            if (grp < QF_GROUPS) row[(size_t)grp * MB + lane] = qf_group_sum(tp, c.def_items[d], grp, col);
            if (grp == NV - 1) row[(size_t)QF_GROUPS * MB + lane] = (c.def_add[d] && act) ? c.def_add[d][w] : 0.0;
        }
    }
    STAMP(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (ACCEPT && c.n_def && grp == 0 && act) {   // finish them in quadform.h's fixed order
        for (int d = 0; d < MAXDEF; d++) {
            if (d >= c.n_def) break;
            const double *row = dq + (size_t)d * (QF_GROUPS + 1) * MB;
            double v = qf_tree(row + lane, MB);
            if (c.def_add[d]) v = v + row[(size_t)QF_GROUPS * MB + lane];
            const int l = c.def_like[d];
            lk[(size_t)l * MB + lane] = v;
            const_cast<double *>(c.like_terms)[(size_t)l * W + w] = v;
        }
    }
    // the test-Gaussian rows of covinv . (trial - center) are spread over the
    // waves (each row summed by one thread, in order) instead of run serially
    // by the chain wave: first the differences (trial - center)_j, one row
    // each (tq rows n_used ..), then the rows' sums and their products with
    // the differences (tq rows 0 ..), every sum's loads in flight together
    const bool par_test = ACCEPT && c.test_like && c.n_used >= 4 && c.tq_rows >= 2 * c.n_used;
    const bool par_map = PROPOSE && c.max_blk >= 4 && c.tq_rows >= 2;
    // the trial's bounds check and squared Gaussian-prior z of every parameter,
    // spread over the thread groups (the chain thread then only sums them in order)
    const bool par_prior = ACCEPT;
    if (par_test || par_prior || pre_col) {
        if (pre_col && !rq_early && act) {
            const int b = c.pre_blk, off = ti[c.tl.blk_R_off + b];
            ncol = ti[c.tl.blk_n + b];
            const int lp = si[(size_t)(R.BLKLP + b) * MB + lane];
            if (lp % ncol != 0) col = off + lp;
#pragma unroll
            for (int u = 0; u < NRQ; u++) {
                const int q = grp + u * NV;
                if (col >= 0 && q < ncol) rq[u] = c.sd[(size_t)(R.R + col + q * ncol) * W + w];
            }
        }
        const Tabs t0 = make_tabs(c, ti, td, c.stage_cov ? td : c.tab_d);
        const Col<double> q{sd + (size_t)SROW(R.T) * MB + lane, MB};
        const int nu = c.n_used;
        double *dif = tq + (size_t)nu * MB + lane;
        if (act) {
            if (par_test)
                for (int i = grp; i < nu; i += NV) {
                    const int pi = t0.params_used[i];
                    dif[(size_t)i * MB] = q[pi] - t0.center[pi];
                }
            if (par_prior) {
                int oob = 0;
                for (int i = grp; i < c.np; i += NV) {
                    const double qv = q[i];
                    if (qv > t0.pmax[i] || qv < t0.pmin[i]) oob = 1;   // GetLogLikeBounds :97-109
                    double z2 = 0.0;
                    if (c.has_priors && t0.pstd[i] != 0.0) {           // GetLogPriors :111-124
                        const double z = (qv - t0.pmean[i]) / t0.pstd[i];
                        z2 = z * z;
                    }
                    zz[(size_t)i * MB + lane] = z2;
                }
                if (oob) atomicOr(&oobw[lane], 1);
            }
        }
        if (par_test) {
            __syncthreads();
            if (act)
                for (int i = grp; i < nu; i += NV) {   // test_row's sum, same order
                    const double *ci = t0.covinv + (size_t)i * nu;
                    double s = 0.0;
                    for (int j0 = 0; j0 < nu; j0 += RCH) {
                        double cv[RCH], dv[RCH];
#pragma unroll
                        for (int u = 0; u < RCH; u++) {
                            const int j = j0 + u < nu ? j0 + u : 0;
                            cv[u] = ci[j];
                            dv[u] = dif[(size_t)j * MB];
                        }
#pragma unroll
                        for (int u = 0; u < RCH; u++)
                            if (j0 + u < nu) s += cv[u] * dv[u];
                    }
                    tq[(size_t)i * MB + lane] = dif[(size_t)i * MB] * s;
                }
        }
#pragma unroll
        for (int u = 0; u < NRQ; u++) {
            const int qq = grp + u * NV;
            if (col >= 0 && qq < ncol) vc[(size_t)qq * MB + lane] = rq[u];
        }
        __syncthreads();
    }
    STAMP(2);
    if (grp == 0 && act) {

    const Tabs t = make_tabs(c, ti, td, c.stage_cov ? td : c.tab_d);
    Walker k;
    k.r.u = Col<double>{sd + (size_t)R.U * MB + lane, MB};
    k.r.c = sd[(size_t)R.C * MB + lane];
    k.r.gset = sd[(size_t)R.G * MB + lane];
    k.r.i97 = si[(size_t)R.I97 * MB + lane];
    k.r.j97 = si[(size_t)R.J97 * MB + lane];
    k.r.iset = si[(size_t)R.ISET * MB + lane];
    k.R = c.stage_R ? Col<double>{sd + (size_t)R.R * MB + lane, MB} : Col<double>{c.sd + (size_t)R.R * W + w, c.ld};
    k.P = Col<double>{sd + (size_t)SROW(R.P) * MB + lane, MB};
    k.trial = Col<double>{sd + (size_t)SROW(R.T) * MB + lane, MB};
    k.vec = Col<double>{vc + lane, MB};
    k.cyc = c.stage_cyc ? Col<int>{si + (size_t)R.CYC * MB + lane, MB} : Col<int>{c.si + (size_t)R.CYC * W + w, c.ld};
    k.cyclp = Col<int>{si + (size_t)R.CYCLP * MB + lane, MB};
    k.blklp = Col<int>{si + (size_t)R.BLKLP * MB + lane, MB};
    k.itmp = c.stage_cyc ? Col<int>{it + lane, MB} : Col<int>{c.itmp_g + w, c.ld};
    k.fast_ix = si[(size_t)R.FASTIX * MB + lane];
    const int i97_0 = k.r.i97;
    double &cur = sd[(size_t)SROW(R.L) * MB + lane];
    double &mult = sd[(size_t)SROW(R.M) * MB + lane];
    int &nacc = si[(size_t)R.NACC * MB + lane];

    bool moved = false;   // accepted: P = trial already
    if (ACCEPT) {
        if (c.mask_on) {   // unchanged likelihoods keep the current point's term (calclike.f90:377-384)
            for (int l = 0; l < c.n_like; l++) {
                const int f = c.like_flag[(size_t)l * W + w];
                double v;
                if (f == 0) v = c.cur_terms[(size_t)l * W + w];
                else if (c.like_out[l]) v = c.like_out[l][f - 1];        // sparse: compacted slot
                else v = lk[(size_t)l * MB + lane];
                lk[(size_t)l * MB + lane] = v;
            }
        }
        STAMP(8);
        const double like = target_like(c, t, k.trial, Col<double>{lk + lane, MB}, par_test ? tq + lane : nullptr,
                                        par_prior ? zz + lane : nullptr, par_prior ? oobw + lane : nullptr);
        STAMP(9);
        bool acc = false;
        if (like != LOGZERO) {
            acc = cur > like;
            if (!acc) acc = (double)randexp1(k.r) > like - cur;
        }
        STAMP(10);
        moved = acc;
        if (acc) {
            if (mult > 0) nacc += 1;
            mult = 1.0;
            for (int i0 = 0; !par_map && i0 < c.np; i0 += RCH) {   // P = trial (par_map: the groups, below)
                double v[RCH];
#pragma unroll
                for (int u = 0; u < RCH; u++) v[u] = k.trial[i0 + u < c.np ? i0 + u : 0];
#pragma unroll
                for (int u = 0; u < RCH; u++)
                    if (i0 + u < c.np) k.P[i0 + u] = v[u];
            }
            cur = like;
#pragma unroll
            for (int l = 0; l < MAXLIKE; l++)
                if (l < c.n_like) {
                    ct[l] = lk[(size_t)l * MB + lane];
                    c.cur_terms[(size_t)l * W + w] = ct[l];
                }
        } else {
            mult += 1.0;
        }
        STAMP(11);
        si[(size_t)R.ACCF * MB + lane] = acc ? 1 : 0;
        if (par_map) oobw[lane] = acc ? 1 : 0;   // (target_like has read the bounds verdict)
        if (hist_row) hist_row[(size_t)c.n_used * c.W + w] = cur;   // the parameters: every group, below
        if (hist_terms) {
#pragma unroll
            for (int l = 0; l < MAXLIKE; l++)
                if (l < c.n_like) hist_terms[(size_t)l * c.W + w] = ct[l];
        }
    }
    STAMP(3);
    if (PROPOSE) {
        for (int i0 = 0; !moved && !par_map && i0 < c.np; i0 += RCH) {   // Trial = CurParams (par_map: below)
            double v[RCH];
#pragma unroll
            for (int u = 0; u < RCH; u++) v[u] = k.P[i0 + u < c.np ? i0 + u : 0];
#pragma unroll
            for (int u = 0; u < RCH; u++)
                if (i0 + u < c.np) k.trial[i0 + u] = v[u];
        }
        STAMP(14);
        k.defer = par_map;
        k.defer_rot = c.rot_defer;
        k.col_pre = pre_col && k.blklp[c.pre_blk] % t.blk_n[c.pre_blk] != 0 &&
                    (!rq_early || k.blklp[c.pre_blk] == c.pre_lp);   // else proposal_tail reads the column itself
        if (fast_only) proposal_fast(c, t, k);
        else proposal(c, t, k);
        STAMP(15);
        si[(size_t)R.PROT * MB + lane] = k.pend_rot + 1;             // rot_kernel finishes this walker
        if (k.pend_rot >= 0) {
            const int slot = atomicAdd(c.rot_cnt + 2 * (blk0 * MB / 64) + c.rot_par, 1);
            c.rot_list[blk0 * MB + slot] = w;
            if (par_map) tq[lane] = -1.0;
        } else if (par_map) tq[lane] = (double)k.pend_b;             // the block, for the mapping waves
        else {
            for (int l = 0; l < c.n_like; l++)
                for (int q = 0; q < c.like_nn[l]; q++)
                    c.like_nuis[l][(size_t)w * c.like_nn[l] + q] = k.trial[t.ti[c.like_nidx[l] + q]];
            if (c.mask_on) write_like_flags(c, k.trial, k.P, w);
        }
    }
    STAMP(4);
    sd[(size_t)R.C * MB + lane] = k.r.c;
    sd[(size_t)R.G * MB + lane] = k.r.gset;
    si[(size_t)R.I97 * MB + lane] = k.r.i97;
    si[(size_t)R.J97 * MB + lane] = k.r.j97;
    si[(size_t)R.ISET * MB + lane] = k.r.iset;
    si[(size_t)R.FASTIX * MB + lane] = k.fast_ix;
    ndw[lane] = k.r.nd < 97 ? k.r.nd : 97;
    i0w[lane] = i97_0;
    }
    if (par_map) {   // UpdateParams' mapping product, rows spread over the waves (one thread per row, same order)
        __syncthreads();
        // first P = trial (accepted) or trial = P (rejected, or no accept in
        // this launch: oobw is 0), the chain having left both to the groups
        if (act) {
            double *Pr = sd + (size_t)SROW(R.P) * MB + lane, *Tr = sd + (size_t)SROW(R.T) * MB + lane;
            const bool mv = oobw[lane] != 0;
            for (int i = grp; i < c.np; i += NV) {
                if (mv) Pr[(size_t)i * MB] = Tr[(size_t)i * MB];
                else Tr[(size_t)i * MB] = Pr[(size_t)i * MB];
            }
        }
        __syncthreads();
        if (act && tq[lane] >= 0.0) {
            const Tabs t = make_tabs(c, ti, td, c.stage_cov ? td : c.tab_d);
            const int b = (int)tq[lane];
            const int n = t.blk_n[b], nc = t.blk_nchanged[b];
            const double *M = t.mapping + t.blk_map_off[b];
            const int *chg = t.changed + t.blk_changed_off[b];
            double *trial = sd + (size_t)SROW(R.T) * MB + lane;
            const double *vec = vc + lane;
            for (int j = grp; j < nc; j += NV) {
                double s = 0.0;
#pragma unroll 4
                for (int q = 0; q < n; q++) s += M[j * n + q] * vec[(size_t)q * MB];
                trial[(size_t)chg[j] * MB] += s;
            }
        }
        __syncthreads();
        STAMP(12);
        if (grp == 0 && act && si[(size_t)R.PROT * MB + lane] == 0) {
            const double *trial = sd + (size_t)SROW(R.T) * MB + lane;
            for (int l = 0; l < c.n_like; l++)
                for (int q = 0; q < c.like_nn[l]; q++)
                    c.like_nuis[l][(size_t)w * c.like_nn[l] + q] = trial[(size_t)ti[c.like_nidx[l] + q] * MB];
            if (c.mask_on)
                write_like_flags(c, Col<const double>{trial, MB}, Col<const double>{sd + (size_t)SROW(R.P) * MB + lane, MB},
                                 w);
        }
    }
    __syncthreads();
    STAMP(13);
    if (ACCEPT && hist_row && act) {   // the history row's parameters (P is final), rows spread over the groups
        const int *pu = ti + c.tl.params_used;
        for (int i = grp; i < c.n_used; i += NV)
            hist_row[(size_t)i * c.W + w] = sd[(size_t)(SROW(R.P) + pu[i]) * MB + lane];
    }
    if (PROPOSE && c.pub_on && threadIdx.x < MB && act)   // the fused pass / bins in this launch poll for these
        for (int k = 0; k < 2; k++) {
            const int pc = c.pub_pcal[k];
            const bool rp = si[(size_t)R.PROT * MB + lane] != 0;   // rot_kernel proposes it (bin co-run only)
            const double v = rp ? __longlong_as_double((long long)TP_PIPE_ROT)
                                : pc >= 0 ? sd[(size_t)(SROW(R.T) + pc) * MB + lane] : 1.0;
            __hip_atomic_store(c.calbuf + (size_t)k * W + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(c.calbuf_next + (size_t)k * W + w, __longlong_as_double((long long)TP_PIPE_UNSET),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // read by the next launch only
        }
    // write back the image (rows of walkers past W are padding of the ld-wide
    // rows: written back unchanged) -- of the RANMAR ring only the entries
    // this launch's draws overwrote (positions i97 - 1, i97 - 2, ... mod 97
    // of the first index)
    if (act) {
        const int nd = ndw[lane], i0 = i0w[lane];
        for (int t = grp; t < nd; t += NV) {
            int p = i0 - 1 - t;
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
    stage_out(c.si, si, 0, 0, ni_st, W, wb);
    STAMP(5);
#ifdef CMAMD_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(6);
#endif
#undef SROW
}
