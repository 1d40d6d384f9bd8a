// The per-walker view of the chain state, the blocked proposer (propose.f90)
// and the target density (calclike.f90).  Included by sampler.hip after mhrng.h.
// (included inside namespace cmamd)
#pragma once

// ------------------------------------------------------------ per-walker view

struct Tabs {   // shared tables (LDS copies)
    const int *ti;   // the whole int table (likelihood nuisance_indices at DevCfg::like_nidx offsets)
    const int *blk_n, *blk_nchanged, *blk_changed_off, *blk_map_off, *blk_R_off, *changed, *pfi, *params_used;
    const double *mapping, *pmin, *pmax, *pmean, *pstd, *lin_w, *lin_m, *lin_s, *covinv, *center;
};

// td_cov: where the test-Gaussian tables (covinv, center: the tail of the
// double table) live -- the LDS copy, or tab_d itself when not staged
__device__ Tabs make_tabs(const DevCfg &c, const int *ti, const double *td, const double *td_cov = nullptr)
{
    const TabLayout &l = c.tl;
    if (!td_cov) td_cov = td;
    return Tabs{ti, ti + l.blk_n, ti + l.blk_nchanged, ti + l.blk_changed_off, ti + l.blk_map_off, ti + l.blk_R_off,
                ti + l.changed, ti + l.pfi, ti + l.params_used, td + l.mapping, td + l.pmin, td + l.pmax,
                td + l.pmean, td + l.pstd, td + l.lin_w, td + l.lin_m, td + l.lin_s, td_cov + l.covinv,
                td_cov + l.center};
}

struct Walker {
    Rng r;
    Col<double> R, P, trial, vec;
    Col<int> cyc, cyclp, blklp, itmp;
    int fast_ix;
    int defer = 0;    // leave the mapping product to the caller (block index in pend_b, vec filled)
    int pend_b = -1;
    int defer_rot = 0;   // leave a new rotation of a wide block to rot_kernel (block index in pend_rot)
    int pend_rot = -1;
    double r1 = 0.0;     // a one-parameter block's rotation, just drawn (R may live in HBM: no read-back)
    int col_pre = 0;     // vec already holds the proposal's column of R (mh_body's pre_col)
};

__device__ int cyc_next(Walker &k, int which, int n, int base)
{   // CyclicIndexRandomizer%Next, propose.f90:75-86 (RandIndices RandUtils.f90:93-108)
    const int lp = k.cyclp[which] % n + 1;
    k.cyclp[which] = lp;
    if (lp == 1) {
        if (n == 1) {
            (void)ranmar(k.r);                      // ix = int(ranmar()*1)+1 = 1
            k.cyc[base] = 1;
        } else {
            for (int i = 0; i < n; i++) k.itmp[i] = i + 1;
            for (int i = 1; i <= n; i++) {
                const int ix = (int)(ranmar(k.r) * (n + 1 - i)) + 1;
                k.cyc[base + i - 1] = k.itmp[ix - 1];
                k.itmp[ix - 1] = k.itmp[n + 1 - i - 1];
            }
        }
    }
    return k.cyc[base + lp - 1];
}

// Rows of R may live in HBM (blocks too big for the LDS image): every pass over
// a row loads it RCH elements at a time, all in flight together, instead of one
// dependent round trip per element.  The sums keep the reference's q order.
static constexpr int RCH = 8;

__device__ void rot_matrix(Walker &k, int off, int n)
{   // RotMatrix propose.f90:88-102 -> RandRotationD RandUtils.f90:133-153
    // element (j,i) (row j) of this block's R at R[off + j*n + i]
    if (n > 1) {
        for (int j = 0; j < n; j++) {
            double norm;
            for (;;) {
                for (int i = 0; i < n; i++) k.vec[i] = gaussian1(k.r);
                for (int i = 0; i < j; i++) {   // vec = vec - sum(vec*R(i,:))*R(i,:)
                    const int base = off + i * n;
                    double s = 0.0;
                    for (int q0 = 0; q0 < n; q0 += RCH) {
                        double rv[RCH], vv[RCH];
#pragma unroll
                        for (int u = 0; u < RCH; u++) {
                            const int q = q0 + u;
                            rv[u] = q < n ? k.R[base + q] : 0.0;
                            vv[u] = q < n ? k.vec[q] : 0.0;
                        }
#pragma unroll
                        for (int u = 0; u < RCH; u++)
                            if (q0 + u < n) s += vv[u] * rv[u];
                    }
                    for (int q0 = 0; q0 < n; q0 += RCH) {
                        double rv[RCH];
#pragma unroll
                        for (int u = 0; u < RCH; u++) rv[u] = q0 + u < n ? k.R[base + q0 + u] : 0.0;
#pragma unroll
                        for (int u = 0; u < RCH; u++)
                            if (q0 + u < n) k.vec[q0 + u] = k.vec[q0 + u] - s * rv[u];
                    }
                }
                norm = 0.0;
                for (int q = 0; q < n; q++) norm += k.vec[q] * k.vec[q];
                if (norm > 1e-3) break;
            }
            const double sn = sqrt(norm), rsn = 1.0 / sn;
            for (int q = 0; q < n; q++) k.R[off + j * n + q] = div_rn(k.vec[q], sn, rsn);   // = vec(q) / sn
        }
    } else {
        for (int i = 0; i < n * n; i++) k.R[off + i] = 0.0;
        for (int i = 0; i < n; i++) {
            k.r1 = (ranmar(k.r) - 0.5) >= 0.0 ? 1.0 : -1.0;
            k.R[off + i * n + i] = k.r1;
        }
    }
}

// blocks this wide get their rotations from rot_kernel.  (Narrower ones stay
// in the chain: config5_bk15_plik's 7-wide foreground block deferred measured
// mh_kernel 34.2 -> 20.7 us plus rot_kernel 15.0 us a step, no gain.)
static constexpr int ROT_DEFER_MIN = 8;

__device__ void proposal_tail(const DevCfg &c, const Tabs &t, Walker &k, int b, int lp);
__device__ void proposal_r(const DevCfg &c, const Tabs &t, Walker &k, int b, int n, double r1);

__device__ __forceinline__ void block_proposal(const DevCfg &c, const Tabs &t, Walker &k, int bi /*1-based*/)
{   // GetBlockProposal :247-254 -> ProposeVec :105-120 -> Propose_r :122-139 -> UpdateParams :142-149
    const int b = bi - 1;
    const int n = t.blk_n[b];
    const int off = t.blk_R_off[b];
    int lp = k.blklp[b];
    if (lp % n == 0) {
        if (k.defer_rot && n >= ROT_DEFER_MIN) {   // rot_kernel draws it and finishes this proposal
            k.pend_rot = b;
            return;
        }
        rot_matrix(k, off, n);
        lp = 0;
        if (n == 1) {   // a fresh one-parameter rotation every step: its sign is in hand
            k.blklp[b] = 1;
            proposal_r(c, t, k, b, 1, k.r1);
            return;
        }
    }
    proposal_tail(c, t, k, b, lp);
}

// ProposeVec after the rotation check: loop index, step length, UpdateParams
__device__ void proposal_tail(const DevCfg &c, const Tabs &t, Walker &k, int b, int lp)
{
    const int n = t.blk_n[b];
    const int off = t.blk_R_off[b];
    lp++;
    k.blklp[b] = lp;
    // vec(q) = R(q, loopix) (the column of R is read once: R may live in HBM
    // when it is too big to stage), scaled by Propose_r's step below
    for (int q0 = 0; !k.col_pre && q0 < n; q0 += RCH) {
        double rv[RCH];
#pragma unroll
        for (int u = 0; u < RCH; u++) rv[u] = q0 + u < n ? k.R[off + (q0 + u) * n + (lp - 1)] : 0.0;
#pragma unroll
        for (int u = 0; u < RCH; u++)
            if (q0 + u < n) k.vec[q0 + u] = rv[u];
    }
    proposal_r(c, t, k, b, n, 0.0);
}

// Propose_r's step length and UpdateParams: vec *= r * wid (r1: the 1 x 1
// rotation itself, when n == 1 and it was just drawn), P(changed) += mapping . vec
__device__ void proposal_r(const DevCfg &c, const Tabs &t, Walker &k, int b, int n, double r1)
{
    double rf;
    if (ranmar(k.r) < 0.33) {
        rf = (double)randexp1(k.r);
    } else {
        const int m = n < 2 ? n : 2;
        rf = 0.0;
        for (int i = 0; i < m; i++) {
            const double g = gaussian1(k.r);
            rf += g * g;
        }
        rf = sqrt(rf / m);
    }
    const double scale = rf * c.propose_scale;
    const int nc = t.blk_nchanged[b];
    const double *M = t.mapping + t.blk_map_off[b];
    const int *chg = t.changed + t.blk_changed_off[b];
    if (r1 != 0.0) k.vec[0] = r1 * scale;
    else
        for (int q0 = 0; q0 < n; q0 += RCH) {   // RCH loads in flight
            double v[RCH];
#pragma unroll
            for (int u = 0; u < RCH; u++) v[u] = k.vec[q0 + u < n ? q0 + u : 0];
#pragma unroll
            for (int u = 0; u < RCH; u++)
                if (q0 + u < n) k.vec[q0 + u] = v[u] * scale;
        }
    if (k.defer) {
        k.pend_b = b;
        return;
    }
    for (int j = 0; j < nc; j++) {
        double s = 0.0;
        for (int q = 0; q < n; q++) s += M[j * n + q] * k.vec[q];
        k.trial[chg[j]] += s;
    }
}

__device__ __forceinline__ void proposal_fast(const DevCfg &c, const Tabs &t, Walker &k)
{   // :283-289
    const int q = cyc_next(k, 2, c.fast_n, c.all_n + c.slow_n);
    block_proposal(c, t, k, t.pfi[c.slow_n + q - 1]);
}

__device__ __forceinline__ void proposal_slow(const DevCfg &c, const Tabs &t, Walker &k)
{   // :275-281
    const int q = cyc_next(k, 1, c.slow_n, c.all_n);
    block_proposal(c, t, k, t.pfi[q - 1]);
}

__device__ __forceinline__ void proposal(const DevCfg &c, const Tabs &t, Walker &k)
{   // GetProposal :257-273
    if (k.fast_ix != 0) {
        proposal_fast(c, t, k);
        k.fast_ix--;
    } else if (cyc_next(k, 0, c.all_n, 0) > c.slow_n) {
        proposal_fast(c, t, k);
        k.fast_ix = c.oversample_fast - 1;
    } else {
        proposal_slow(c, t, k);
    }
}

// GetLogLike calclike.f90:136-151 with AddLikeTemp :82-94; likes[l] are the
// data-likelihood terms at q (LogLikeWithTheorySet :374-387)
// test_row(i): row i of covinv . (q - center) (TestLikelihoodFunction's inner sum)
template <class Q>
__device__ inline double test_row(const DevCfg &c, const Tabs &t, const Q &q, int i)
{
    const int n = c.n_used;
    double s = 0.0;
    for (int j = 0; j < n; j++) s += t.covinv[i * n + j] * (q[t.params_used[j]] - t.center[t.params_used[j]]);
    return s;
}

// trows (stride MB), when given, holds (q - center)_i x test_row(i) for every
// i, computed by the other waves of mh_kernel: the same products, summed here
// in the same order (built with -ffp-contract=off: no fused multiply-add)
// zrows / oobv (stride MB), when given, hold every parameter's squared prior z
// (0 where there is no prior) and the bounds verdict of q, formed by the other
// thread groups: the same terms, summed here in the same order
template <class Q, class L>
__device__ __forceinline__ double target_like(const DevCfg &c, const Tabs &t, const Q &q, const L &likes,
                              const double *trows = nullptr, const double *zrows = nullptr, const int *oobv = nullptr)
{
    // the parameter loops load RCH entries at a time (all in flight together;
    // the chain wave would otherwise wait out one LDS round trip per entry)
    bool oob = oobv ? *oobv != 0 : false;
    for (int i0 = 0; !oobv && i0 < c.np; i0 += RCH) {                // GetLogLikeBounds :97-109
        double qv[RCH], hi[RCH], lo[RCH];
#pragma unroll
        for (int u = 0; u < RCH; u++) {
            const int i = i0 + u < c.np ? i0 + u : 0;
            qv[u] = q[i];
            hi[u] = t.pmax[i];
            lo[u] = t.pmin[i];
        }
#pragma unroll
        for (int u = 0; u < RCH; u++)
            if (i0 + u < c.np && (qv[u] > hi[u] || qv[u] < lo[u])) oob = true;
    }
    if (oob) return LOGZERO;
    double main = 0.0;
    if (c.test_like) {                                               // TestLikelihoodFunction :180-199
        const int n = c.n_used;
        double d = 0.0;
        for (int i0 = 0; trows && i0 < n; i0 += RCH) {   // the products, formed by the thread groups
            double v[RCH];
#pragma unroll
            for (int u = 0; u < RCH; u++) v[u] = trows[(size_t)(i0 + u < n ? i0 + u : 0) * MB];
#pragma unroll
            for (int u = 0; u < RCH; u++)
                if (i0 + u < n) d += v[u];
        }
        for (int i = 0; !trows && i < n; i++)
            d += (q[t.params_used[i]] - t.center[t.params_used[i]]) * test_row(c, t, q, i);
        main = d / 2.0;
    }
    for (int l = 0; l < c.n_like; l++) {
        const double v = likes[l];
        if (v == LOGZERO) return LOGZERO;
        main += v;
    }
    double like = main / c.temperature;
    if (c.has_priors) {                                              // GetLogPriors :111-134
        double pri = 0.0;
        for (int i0 = 0; zrows && i0 < c.np; i0 += RCH) {
            double zv[RCH];
#pragma unroll
            for (int u = 0; u < RCH; u++) zv[u] = zrows[(size_t)(i0 + u < c.np ? i0 + u : 0) * MB];
#pragma unroll
            for (int u = 0; u < RCH; u++)
                if (i0 + u < c.np) pri += zv[u];
        }
        for (int i0 = 0; !zrows && i0 < c.np; i0 += RCH) {   // std already 0 where the varying/include_fixed gate (:119) is off
            double qv[RCH], mu[RCH], sd[RCH];
#pragma unroll
            for (int u = 0; u < RCH; u++) {
                const int i = i0 + u < c.np ? i0 + u : 0;
                qv[u] = q[i];
                mu[u] = t.pmean[i];
                sd[u] = t.pstd[i];
            }
#pragma unroll
            for (int u = 0; u < RCH; u++)
                if (i0 + u < c.np && sd[u] != 0.0) {
                    const double z = (qv[u] - mu[u]) / sd[u];
                    pri += z * z;
                }
        }
        for (int k = 0; k < c.n_lin; k++)    // linear combinations :125-131
            if (t.lin_s[k] != 0.0) {
                const double *wk = t.lin_w + (size_t)k * c.np;
                double s = 0.0;
                for (int i = 0; i < c.np; i++) s += wk[i] * q[i];
                const double z = (s - t.lin_m[k]) / t.lin_s[k];
                pri += z * z;
            }
        like = like + (pri / 2.0) / c.temperature;
    }
    return like;
}
