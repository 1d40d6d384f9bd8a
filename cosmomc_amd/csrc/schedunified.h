// Host side: the unified fast-step schedule (mh_step_kernel, steptail.h; state:
// UnifiedSteps, sampler.h).  Included once by sampler.hip inside namespace
// cmamd, after launch_cfg.
//
// propose(1) + pass(1) | tails(1) + pass(2) + accept(1) + propose(2) | ... |
// tails(n) + accept(n): one launch per step.

// The launch's kernels and their profiler names, [binned-cache step][v]: v = 0
// propose + pass, 1 tails + pass + accept + propose, 2 tails + accept
using StepKernel = void (*)(DevCfg, int, double *, double *, StepTail, const int2 *, TailWait, int);
static const StepKernel step_kernels[2][3] = {
    {mh_step_kernel<false, true>, mh_step_kernel<true, true>, mh_step_kernel<true, false>},
    {mh_step_kernel<false, true>, mh_tail_kernel<true, true>, mh_tail_kernel<true, false>}};
static const char *const step_names[2][3] = {{"mh_step_first", "mh_step_kernel", "mh_step_last"},
                                             {"mh_step_first", "mh_tail_kernel", "mh_tail_last"}};

// Whether this run of fast steps can take the unified launches -- the fused
// pass's vectorised form over one walker group, no change mask, no rotations
// left to rot_kernel, and its two stages a deferred quadratic form (plik_lite:
// every row calibrated) and a small chi^2 another launch can carry (Planck
// lensing).  Sets up the raw-sum buffers once per W.
static bool unified_setup(cmbs *s, int fast_only) {
    // (the unified launch carries the fused pair alone: with a third likelihood the
    // run takes the unpipelined steps, whose eval_likes runs every likelihood; BASELINE
    // configs[2] with a lowl term would be such a run -- clik is absent, so none exists here)
    if (s->sched_mode == 0 || !fast_only || !s->tpass || s->n_groups != 1 || s->mask_on ||
        (s->dc.rot_defer && s->rot_fast_any) || s->likes.size() != 2 || !s->dlikes.empty())
        return false;
    const TheoryView &P = s->likes[s->tp_like[0]].th;
    if (!s->tpass->vec_ok(P.dl, P.ld_field, P.ld_walker)) return false;
    UnifiedSteps &u = s->unified;
    if (u.ready == s->W) return true;
    if (u.ready == -s->W) return false;
    u.qf = u.g = -1;
    SmallGaussLaunch g{};
    for (int k = 0; k < 2; k++) {
        const int i = s->tp_like[k];
        const WinStage &st = s->tp_stage[k];
        QFSource src;
        if (st.kind == 1 && is_deferred(s, (size_t)i) && s->likes[i].like->like->qf_source(src, s->W, s->like_ws[i].p)) {
            bool all_cal = st.cal_index >= 0;
            for (const WinCol &c : st.cols) all_cal = all_cal && c.cal;
            if (all_cal && st.ld == src.Np) u.qf = k;
        }
        if (st.kind == 0 && small_gauss_on(s, trial_set(s), i, g)) u.g = k;
    }
    if (u.qf < 0 || u.g < 0 || u.qf == u.g) {
        u.ready = -s->W;
        return false;
    }
    const size_t Wp = (size_t)QuadForm::wpad(s->W);
    int rows = 0;
    for (const WinCol &c : s->tp_stage[u.g].cols) rows = std::max(rows, c.row + 1);
    const size_t bytes[2] = {Wp * (size_t)s->tp_stage[u.qf].ld * 8, (size_t)rows * s->W * 8};
    for (int p = 0; p < 2; p++)
        for (int k = 0; k < 2; k++) u.S[p][k].alloc(bytes[k == u.qf ? 0 : 1]);   // zeroed: padding bins / walkers stay 0
    std::vector<unsigned char> rc((size_t)rows + 16, 0);
    for (const WinCol &c : s->tp_stage[u.g].cols) rc[c.row] = c.cal ? 1 : 0;
    u.rowcal.alloc(rc.size());
    u.rowcal.upload(rc.data(), rc.size());
    // the arrival counters (allocated zero; run_unified starts the epochs) and the LDS
    u.cnt_bytes = (Wp / QF_TILE * TW_PAD * 4 + 15) & ~(size_t)15;   // a multiple of 16 from the start
    u.cnt.alloc(u.cnt_bytes);
    s->pipe_status.init();
    u.lds = std::max({s->mh_lds, (size_t)QFS_LDS_DOUBLES * 8, (size_t)tp_vec_lds_bytes<2>(),
                      (size_t)small_gauss_lds_doubles<UNI_WT>(g.d.nX) * 8,
                      (size_t)small_gauss_lds_doubles<MB>(g.d.nX) * 8});
    for (auto &ks : step_kernels)
        for (StepKernel k : ks)
            HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)u.lds));
    for (auto &pl : u.plan) pl.key[0] = -1;
    u.ready = s->W;
    return true;
}

// Whether a launch's chi^2 runs folded into its Metropolis workgroups instead
// of as workgroups of its own: bit-identical while its 16-walker body's thread
// groups (256 / 16) cover the nX bandpowers.  Middle launches (with a pass)
// only: in the accept-only launch that ends a call the chi^2 would sit on the
// chain's critical path, 21.5 against 23.3 us
static bool fold_chi2(bool has_pass, int nX) { return has_pass && nX <= MH_THREADS / MB; }

// One step tail: the quadratic form and the chi^2 of the step whose raw sums
// are in half rd (rd < 0: none), and the pass storing the next step's raw sums
// into half wr (wr < 0: none).
static StepTail make_tail(cmbs *s, int rd, int wr) {
    const UnifiedSteps &u = s->unified;
    StepTail t;
    const int W = s->W;
    t.W = W;
    if (rd >= 0) {
        const int qi = s->tp_like[u.qf];
        Like &Q = *s->likes[qi].like->like;
        if (!Q.qf_source(t.q.src, W, s->like_ws[qi].p)) fail(CMBL_ERR_ARG, "internal: step tail quadratic form");
        t.q.S = u.S[rd][u.qf].as<double>();
        t.q.nuis = s->dc.like_nuis[qi];
        t.q.ld_nuis = std::max(1, Q.n_nuis);
        t.q.cal_index = s->tp_stage[u.qf].cal_index;
        t.q.W = W;
        t.q.Wp = QuadForm::wpad(W);
        t.nq = t.q.src.n_items * (QuadForm::wpad(W) / QF_TILE);
        if (!small_gauss_on(s, trial_set(s), s->tp_like[u.g], t.g)) fail(CMBL_ERR_ARG, "internal: step tail chi^2");
        t.g.partial = u.S[rd][u.g].as<double>();
        t.g.row_cal = u.rowcal.as<unsigned char>();
        t.g.stage_cal = s->tp_stage[u.g].cal_index;
        t.fold_g = fold_chi2(wr >= 0, t.g.d.nX) ? 1 : 0;
        t.ng = t.fold_g ? 0 : (W + UNI_WT - 1) / UNI_WT;
    }
    if (wr >= 0) {
        TPOut o[2];
        fused_outs(s, trial_set(s), o, u.S[wr]);
        t.tp = s->tpass->dev_args(o, W);
        const TheoryView &P = s->likes[s->tp_like[0]].th;
        t.dl = P.dl;
        t.ld_field = P.ld_field;
        t.ld_walker = P.ld_walker;
        t.np = s->tpass->n_blocks();
    }
    return t;
}

// One unified step launch: the tails of the step whose raw sums are in half
// rd (rd < 0: none), the pass into half wr (wr < 0: none), and the Metropolis
// workgroups accepting that step (when rd >= 0) and proposing the next
// (propose).
static void launch_unified(cmbs *s, hipStream_t stream, bool propose, int rd, int wr, const HistRow &row,
                           int fast_only) {
    UnifiedSteps &u = s->unified;
    const bool accept = rd >= 0;
    StepTail t = make_tail(s, rd, wr);
    DevCfg dc = launch_cfg(s, fast_only, false);
    dc.n_def = accept ? 1 : 0;
    if (accept) {   // plik's combine from this launch's partials (QFDeferred)
        dc.def_like[0] = s->tp_like[u.qf];
        dc.def_items[0] = t.q.src.n_items;
        dc.def_part[0] = t.q.src.partial;
        dc.def_add[0] = nullptr;
    }
    TailWait tw{};
    tw.cnt = u.cnt.as<unsigned int>();
    tw.epoch = u.epoch + (accept ? 1u : 0u);
    tw.epoch_g = u.epoch_g + ((accept && !t.fold_g) ? 1u : 0u);
    tw.nq_items = t.q.src.n_items;
    tw.ng = accept ? (s->W + UNI_WT - 1) / UNI_WT : 0;   // an unfolded launch's chi^2 workgroups (the target's
    tw.gwt = UNI_WT;                                      // per-tile count for the epoch_g launches)
    tw.status = s->pipe_status.dev;
    tw.nosignal = s->handoff_nosignal;
    tw.stamp_slot = propose ? 0 : 1;
    tw.ntiles = (int)(u.cnt_bytes / 4);
    const int nmh = (s->W + MB - 1) / MB;
    const int v = accept ? (propose ? 1 : 2) : 0;
    StepTailPlan &pl = u.plan[v];
    if (pl.key[0] != t.nq || pl.key[1] != t.ng || pl.key[2] != t.np) {
        const std::vector<int2> rows = tail_rows(t.nq, t.ng, t.np, nmh);
        pl.d_rows.alloc(rows.size() * sizeof(int2));
        pl.d_rows.upload(rows.data(), rows.size() * sizeof(int2));
        pl.nrows = (int)rows.size();
        pl.key[0] = t.nq;
        pl.key[1] = t.ng;
        pl.key[2] = t.np;
    }
    const dim3 grid((unsigned)pl.nrows * 8), b(MH_THREADS);
    const int2 *rows = pl.d_rows.as<int2>();
    const bool cached = u.binned_cache && accept && wr < 0 && rd == 0;   // the binned-cache steps (no pass)
    try {
        timed_launch(step_names[cached][v], stream, [&](hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(step_kernels[cached][v], grid, b, u.lds, stream, e0, e1, 0, dc, fast_only, row.p,
                                  row.t, t, rows, tw, nmh);
        });
        HIP_CHECK(hipGetLastError());
    } catch (...) {
        u.invalidate();
        s->pipe_status.post_nothrow(stream);
        throw;
    }
    if (accept) u.epoch++;
    if (accept && !t.fold_g) u.epoch_g++;
}

static void run_unified(cmbs *s, int n_steps, int fast_only, hipStream_t stream) {
    // the arrival counters start from 0 in every call (the first launch zeroes
    // them; the epochs are counted within it)
    s->unified.epoch = 0;
    s->unified.epoch_g = 0;
    launch_unified(s, stream, true, -1, 0, HistRow{}, fast_only);
    for (int k = 0; k < n_steps; k++) {
        const bool more = k + 1 < n_steps;
        // binned cache: the theory is fixed within the call, so every step's tails
        // read the raw sums the first launch's pass wrote (half 0), and no launch re-bins
        if (s->unified.binned_cache) launch_unified(s, stream, more, 0, -1, next_hist(s), fast_only);
        else launch_unified(s, stream, more, k % 2, more ? (k + 1) % 2 : -1, next_hist(s), fast_only);
    }
    s->pipe_status.post(stream);
}
