// Host side: the likelihoods' evaluation at a set of points.  Included once by
// sampler.hip inside namespace cmamd, after the kernels.
//
// An evaluation set names, per likelihood, the theory it reads, its DataParams
// rows, its row of terms and the workspace of its fused window stage.  There
// are three: the walkers' trial points (trial_set), a slow step's trial or
// drag end points on the trial theories (end_set), and a drag's start points
// on the walkers' theories (start_set: rows and workspaces of its own, so an
// interpolation step can evaluate both of its sets in one pair of launches).

struct EvalSet {
    TheoryView th[MAXLIKE];
    double *nuis[MAXLIKE];    // [W][n_nuis] DataParams
    double *terms[MAXLIKE];   // [W] -lnL
    void *ws[MAXLIKE];        // the fused likelihoods' workspaces
};

static EvalSet make_set(const cmbs *s, bool end_theory, bool start_rows) {
    EvalSet e{};
    double *terms = (start_rows ? s->like_terms2 : s->like_terms).as<double>();
    for (size_t i = 0; i < s->likes.size(); i++) {
        e.th[i] = end_theory ? s->end_theory[i] : s->likes[i].th;
        e.nuis[i] = start_rows ? s->nuis_bufs2[i].as<double>() : s->dc.like_nuis[i];
        e.terms[i] = terms + i * (size_t)s->dc.ld;
        e.ws[i] = (start_rows ? s->like_ws2 : s->like_ws)[i].p;
    }
    return e;
}
static EvalSet trial_set(const cmbs *s) { return make_set(s, false, false); }
static EvalSet end_set(const cmbs *s) { return make_set(s, true, false); }
static EvalSet start_set(const cmbs *s) { return make_set(s, false, true); }

// a deferrable likelihood's evaluation for the accepting mh_kernel that follows:
// the launches up to the quadratic form's partials, recorded in s->pending
static bool is_deferred(const cmbs *s, size_t i) {
    for (int q : s->defer_likes)
        if (q == (int)i) return true;
    return false;
}

static void record_deferred(cmbs *s, size_t i, const QFDeferred &d) {
    const int p = s->pending.n++;
    s->pending.like[p] = (int)i;
    s->pending.items[p] = d.n_items;
    s->pending.part[p] = d.partial;
    s->pending.add[p] = d.addend;
}

// likelihood i is one of the fused window pass's pair
static bool fused(const cmbs *s, size_t i) {
    return s->tpass && ((int)i == s->tp_like[0] || (int)i == s->tp_like[1]);
}

// the fused pair can run as one pass on this set: both read one theory view
static bool fusable(const cmbs *s, const EvalSet &e) {
    return s->tpass && e.th[s->tp_like[0]] == e.th[s->tp_like[1]];
}

// the pass's two outputs on a set: each fused likelihood's window rows in the
// set's workspace, calibrated by the set's DataParams.  With raw, the unified
// launch's form: the sums into raw[k], the kind-1 stage bin-major
// (steptail.h: its row stride is wpad(W))
static void fused_outs(const cmbs *s, const EvalSet &e, TPOut o[2], const DevBuf *raw = nullptr) {
    for (int k = 0; k < 2; k++) {
        const int i = s->tp_like[k];
        const WinStage &st = s->tp_stage[k];
        Like &L = *s->likes[i].like->like;
        o[k] = TPOut{st.kind, st.cal_index, raw && st.kind == 1 ? QuadForm::wpad(s->W) : st.ld, 0,
                     raw ? raw[k].as<double>() : L.window_out(e.ws[i], s->W), st.X, e.nuis[i],
                     (long long)std::max(1, L.n_nuis)};
    }
}

// the pass over a fusable set, whole walker set
static void launch_tpass(cmbs *s, hipStream_t stream, const EvalSet &e) {
    TPOut o[2];
    fused_outs(s, e, o);
    const TheoryView &t = e.th[s->tp_like[0]];
    s->tpass->launch(t.dl, t.ld_field, t.ld_walker, o, s->W, stream);
}

// The fused pass's two tails as one launch: when one fused likelihood is
// deferred and its quadratic form carries co-runs (plik_lite) and the other's
// whole after-window stage is a small chi^2 (Planck lensing), the chi^2's
// workgroups run in the quadratic form's launch (quadform_corun) and its term
// lands in its like_terms row as before.  The carrier and the carried index
// for this step, or -1, -1.
struct Corun {
    int carrier = -1, carried = -1;
    SmallGaussLaunch a{};
};

// likelihood i's whole after-window stage on a set as a small chi^2 that
// another launch can carry (false: it is no such stage)
static bool small_gauss_on(const cmbs *s, const EvalSet &e, int i, SmallGaussLaunch &g) {
    Like &L = *s->likes[i].like->like;
    return L.corun_small(g, s->W, e.nuis[i], L.n_nuis, e.terms[i], e.ws[i]);
}

static Corun plan_corun(cmbs *s, bool defer) {
    Corun c;
    if (!defer || !s->tpass || s->no_corun) return c;
    for (int k = 0; k < 2; k++) {
        const int h = s->tp_like[k], o = s->tp_like[1 - k];
        if (!is_deferred(s, h) || !s->likes[h].like->like->accepts_corun()) continue;
        if (small_gauss_on(s, trial_set(s), o, c.a)) {
            c.carrier = h;
            c.carried = o;
            return c;
        }
    }
    return c;
}

// the rest of a fused likelihood after the pass: deferred or into its like_terms row
static void eval_after_window(cmbs *s, size_t i, bool defer, hipStream_t stream, const Corun &co) {
    if ((int)i == co.carried) return;   // inside the carrier's launch
    Like &L = *s->likes[i].like->like;
    const bool d = defer && is_deferred(s, i);
    const QFDeferred q = L.after_window(s->W, s->dc.like_nuis[i], L.n_nuis,
                                        d ? nullptr : s->like_terms.as<double>() + i * (size_t)s->dc.ld,
                                        s->like_ws[i].p, stream, d, (int)i == co.carrier ? &co.a : nullptr);
    if (d) record_deferred(s, i, q);
}

static bool eval_deferred(cmbs *s, size_t i, hipStream_t stream) {
    if (!is_deferred(s, i)) return false;
    auto &l = s->likes[i];
    const QFDeferred d = l.like->like->loglike_batch_deferred(s->W, l.th.dl, l.th.ld_field, l.th.ld_walker,
                                                              s->dc.like_nuis[i], l.like->like->n_nuis,
                                                              s->like_ws[i].p, stream);
    record_deferred(s, i, d);
    return true;
}

// the likelihoods of a masked step: compaction of the sparse likelihoods'
// changed walkers, then every likelihood (sparse ones on the compacted slots)
static void eval_likes_masked(cmbs *s, hipStream_t stream, bool defer) {
    SparseSet ss{};
    const int ns = (int)s->sparse_likes.size();
    for (int b = 0; b < ns; b++) {
        const int li = s->sparse_likes[b];
        const int nn = s->likes[li].like->like->n_nuis;
        ss.like[b] = li;
        ss.nn[b] = nn;
        ss.nuisc[b] = s->like_nuisc[li].as<double>();
        ss.map[b] = reinterpret_cast<int *>(ss.nuisc[b] + (size_t)s->W * std::max(1, nn));
    }
    int *cnt = s->like_cnt.as<int>();
    hipLaunchKernelGGL(like_compact_kernel, dim3(ns), dim3(1024), 0, stream, s->dc, ss, cnt);
    HIP_CHECK(hipGetLastError());
    if (s->tpass) launch_tpass(s, stream, trial_set(s));   // the fused likelihoods are dense (setup_fusion)
    const Corun co = plan_corun(s, defer);
    for (size_t i = 0; i < s->likes.size(); i++) {
        auto &l = s->likes[i];
        const TheoryView &t = l.th;
        const int nn = l.like->like->n_nuis;
        int b = -1;
        for (int q = 0; q < ns; q++)
            if (ss.like[q] == (int)i) b = q;
        if (b < 0) {
            if (fused(s, i)) {
                eval_after_window(s, i, defer, stream, co);
                continue;
            }
            if (defer && eval_deferred(s, i, stream)) continue;
            l.like->like->loglike_batch(s->W, t.dl, t.ld_field, t.ld_walker, s->dc.like_nuis[i], nn,
                                        s->like_terms.as<double>() + i * (size_t)s->dc.ld, s->ws.p, stream);
            continue;
        }
        const double *dl = t.dl;
        if (t.ld_walker != 0) {
            double *dlc = s->like_dlc[i].as<double>();
            hipLaunchKernelGGL(gather_theory_kernel, dim3(s->W), dim3(256), 0, stream, t.dl, t.ld_walker,
                               theory_extent(*l.like->like, t.ld_field), (const int *)ss.map[b], (const int *)(cnt + b),
                               dlc);
            HIP_CHECK(hipGetLastError());
            dl = dlc;
        }
        l.like->like->loglike_batch_sparse(s->W, dl, t.ld_field, t.ld_walker, ss.nuisc[b], nn,
                                           s->like_outc[i].as<double>(), s->ws.p, stream, cnt + b);
    }
}

// likelihood terms of walkers [g0, g1) at their trial points
// defer: the accepting mh_kernel launched next finishes the deferrable
// likelihoods (all walkers, one group)
static void eval_likes(cmbs *s, hipStream_t stream, int g0, int g1, void *ws, bool defer = false) {
    const int Wg = g1 - g0;
    if (defer && (g0 != 0 || g1 != s->W)) fail(CMBL_ERR_ARG, "internal: deferred evaluation of a walker group");
    const bool fuse = s->tpass && g0 == 0 && g1 == s->W;
    if (fuse) launch_tpass(s, stream, trial_set(s));
    const Corun co = fuse ? plan_corun(s, defer) : Corun{};
    // the likelihoods run in order on the caller's stream: side by side on forked
    // streams the memory-bound likelihood kernels slow each other more than they
    // overlap (MI355X, W = 1024, plik_lite + lensing: 77.1 vs 71.9 us/step; the
    // binning kernel alone 12.5 -> 26.2 us next to the lensing windows).  Even
    // the fused pass's two tails (quadratic form and the lensing chi^2, 13.6 and
    // 7.1 us) lose: with the chi^2 on a side stream forked and joined by events
    // the step took 87.5 instead of 63.3 us (round 2).  They share one launch
    // instead (plan_corun): 15.4 us against 13.5 + 4.6 (round 3)
    for (size_t i = 0; i < s->likes.size(); i++) {
        auto &l = s->likes[i];
        const int nn = l.like->like->n_nuis;
        if (fuse && fused(s, i)) {
            eval_after_window(s, i, defer, stream, co);
            continue;
        }
        if (defer && eval_deferred(s, i, stream)) continue;
        l.like->like->loglike_batch(Wg, l.th.dl + (size_t)g0 * l.th.ld_walker, l.th.ld_field, l.th.ld_walker,
                                    s->dc.like_nuis[i] + (size_t)g0 * nn, nn,
                                    s->like_terms.as<double>() + i * (size_t)s->dc.ld + g0, ws, stream);
    }
}

// every walker's trial likelihoods in one group: masked or dense
static void eval_trial_likes(cmbs *s, hipStream_t stream, bool defer) {
    if (s->mask_on) eval_likes_masked(s, stream, defer);
    else eval_likes(s, stream, 0, s->W, s->ws.p, defer);
}

// DataParams of every likelihood at the trial rows.  (Only cmbs_set_start needs
// it: a proposing mh_kernel scatters the slices itself.)
static void gather_trial_nuis(cmbs *s, hipStream_t stream) {
    for (size_t i = 0; i < s->likes.size(); i++) {
        hipLaunchKernelGGL(gather_nuis, dim3((s->W + 255) / 256), dim3(256), 0, stream,
                           s->dc.sd + (size_t)s->dc.rows.T * s->dc.ld, s->W, s->dc.ld, s->dc.tab_i + s->dc.like_nidx[i],
                           s->likes[i].like->like->n_nuis, s->dc.like_nuis[i]);
        HIP_CHECK(hipGetLastError());
    }
}

// ---- a slow step's sets

// likelihood i on its own, whole walker set, into the set's terms row
static void eval_one(cmbs *s, const EvalSet &e, size_t i, hipStream_t stream) {
    Like &L = *s->likes[i].like->like;
    const TheoryView &t = e.th[i];
    L.loglike_batch(s->W, t.dl, t.ld_field, t.ld_walker, e.nuis[i], L.n_nuis, e.terms[i], s->ws.p, stream);
}

// the likelihood terms of a slow step's set: the fused pair as one pass when
// the set allows it
static void eval_likes_drag(cmbs *s, const EvalSet &e, hipStream_t stream) {
    const bool fuse = fusable(s, e);
    if (fuse) launch_tpass(s, stream, e);
    for (size_t i = 0; i < s->likes.size(); i++) {
        Like &L = *s->likes[i].like->like;
        if (fuse && fused(s, i)) L.after_window(s->W, e.nuis[i], L.n_nuis, e.terms[i], e.ws[i], stream, false);
        else eval_one(s, e, i, stream);
    }
}

// Both sets of a drag's interpolation step (end_set and, with both, start_set)
// as two launches instead of eight: the fused window pass over both theory
// sets (theory_window_pair, which also zeroes the tickets), then plik_lite's
// two in-launch-combined quadratic forms with both lensing chi^2s riding along
// (launch_qf_pair).  False when the sets cannot be fused (then eval_likes_drag
// runs each).
static bool eval_likes_drag_pair(cmbs *s, hipStream_t stream, bool both = true) {
    if (!s->tpass || s->no_drag_pair) return false;
    int kq = -1, kg = -1;
    for (int k = 0; k < 2; k++) (s->tp_stage[k].kind == 1 ? kq : kg) = k;
    if (kq < 0 || kg < 0) return false;
    const int qi = s->tp_like[kq], gi = s->tp_like[kg];
    const EvalSet a = end_set(s), b = start_set(s);
    if (!fusable(s, a)) return false;
    const TheoryView &ta = a.th[qi], &tb = b.th[qi];
    if (!s->tpass->vec_ok(ta.dl, ta.ld_field, ta.ld_walker) || !s->tpass->vec_ok(tb.dl, tb.ld_field, tb.ld_walker))
        return false;
    const int W = s->W;
    Like &Q = *s->likes[qi].like->like;
    QFSource qa, qb;
    if (!Q.qf_source(qa, W, a.ws[qi]) || !Q.qf_source(qb, W, b.ws[qi])) return false;
    SmallGaussLaunch ga{}, gb{};
    if (!small_gauss_on(s, a, gi, ga) || !small_gauss_on(s, b, gi, gb)) return false;
    TPOut oa[2], ob[2];
    fused_outs(s, a, oa);
    fused_outs(s, b, ob);
    s->tpass->launch_pair(ta.dl, ta.ld_field, ta.ld_walker, oa, qa.counters, both ? tb.dl : nullptr, tb.ld_field,
                          tb.ld_walker, ob, qb.counters, qa.n_counters, W, stream);
    launch_qf_pair(qa, a.terms[qi], both ? &qb : nullptr, b.terms[qi], W, &ga, both ? &gb : nullptr, stream,
                   "plik_quadform_pair");
    for (size_t i = 0; i < s->likes.size(); i++) {   // any other likelihood, one set after the other
        if (fused(s, i)) continue;
        eval_one(s, a, i, stream);
        if (both) eval_one(s, b, i, stream);
    }
    return true;
}
