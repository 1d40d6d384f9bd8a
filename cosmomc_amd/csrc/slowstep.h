// Host side: the steps that move slow parameters (cmbs_step_theory,
// cmbs_step_drag, cmbs_refresh_theory) and their kernels.  Included once by
// sampler.hip inside namespace cmamd, after the fast steps.  The theory source
// (fill_trial_theory) fills the trial-theory buffers (cmbs::end_theory) at a
// set of parameter rows, the likelihoods run on end_set, and accepted walkers
// take the trial theory as their own.

void sampler_set_trial_theory(cmbs *s, int like_index, double *dl_end, long long ld_field, long long ld_walker) {
    if (like_index < 0 || like_index >= (int)s->likes.size()) fail(CMBL_ERR_ARG, "no likelihood %d", like_index);
    s->end_theory[like_index] = TheoryView{dl_end, ld_field, ld_walker};
}

void sampler_set_theory_calculator(cmbs *s, cmbt *calc) {
    s->calc = calc;
    if (calc && !s->calc_fail.p) s->calc_fail.alloc((size_t)s->dc.ld * 4);
}

void sampler_set_like_calculator(cmbs *s, int like_index, cmbt *calc) {
    if (like_index < 0 || like_index >= (int)s->likes.size()) fail(CMBL_ERR_ARG, "no likelihood %d", like_index);
    s->like_calc[like_index] = calc;
    if (calc && !s->calc_fail.p) s->calc_fail.alloc((size_t)s->dc.ld * 4);
    if (calc && !s->calc_fail2.p) s->calc_fail2.alloc((size_t)s->dc.ld * 4);
}

// The slow entries write through two kinds of view: the trial theories, which
// the calculator fills, and the walkers' theory rows, which take the accepted
// and the refreshed theories
static double *writable(const TheoryView &v) { return const_cast<double *>(v.dl); }

// Whether an earlier likelihood already covers likelihood i in a walk over the
// distinct theory buffers (fused likelihoods usually read one).  The
// calculator fills a trial-theory view once:
static bool trial_theory_seen(const cmbs *s, size_t i) {
    for (size_t j = 0; j < i; j++)
        if (s->end_theory[j] == s->end_theory[i]) return true;
    return false;
}
// and the accepted-theory copy, being idempotent, runs once per pair of trial
// and walker view (an earlier copy that moved at least as many doubles a row)
static bool same_theory_swap(const cmbs *s, size_t i) {
    const TheoryView &e = s->end_theory[i], &l = s->likes[i].th;
    for (size_t j = 0; j < i; j++) {
        const TheoryView &ej = s->end_theory[j], &lj = s->likes[j].th;
        if (ej == e && lj == l && std::min(ej.ld_walker, lj.ld_walker) >= std::min(e.ld_walker, l.ld_walker))
            return true;
    }
    return false;
}

// The calculator that fills likelihood i's trial-theory buffer: the override of
// the first likelihood reading that buffer which has one
// (cmbs_set_like_calculator), else the sampler's
static cmbt *trial_calculator(const cmbs *s, size_t i) {
    for (size_t j = 0; j < s->likes.size(); j++)
        if (s->like_calc[j] && s->end_theory[j] == s->end_theory[i]) return s->like_calc[j];
    return s->calc;
}
static bool any_like_calculator(const cmbs *s) {
    for (size_t j = 0; j < s->likes.size(); j++)
        if (s->like_calc[j]) return true;
    return false;
}

// flag[w] |= more[w]: a walker fails when any of its calculators flags it
__global__ void calc_fail_or(int *__restrict__ flag, const int *__restrict__ more, int W)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < W && more[w] != 0) flag[w] = 1;
}

// The theory source: the trial theories at parameter rows Prows [np][ld], from
// the theory function or, without one, from the calculator (one launch per
// distinct buffer).  True when the calculator made them: calc_fail then flags
// the walkers outside its box (apply_calc_fail after the likelihoods).  With
// per-likelihood calculators each launch overwrites its own flags, so every
// launch after the first writes calc_fail2, which is ORed into calc_fail.
static bool fill_trial_theory(cmbs *s, cmbs_theory_fn fn, void *user, const double *Prows, hipStream_t stream) {
    if (fn) {
        if (fn(user, s->W, Prows, (long long)s->dc.ld, stream) != 0) fail(CMBL_ERR_ARG, "theory function failed");
        return false;
    }
    const bool several = any_like_calculator(s);
    bool first = true;
    for (size_t i = 0; i < s->likes.size(); i++) {
        const TheoryView &e = s->end_theory[i];
        if (trial_theory_seen(s, i)) continue;
        int *flags = (several && !first) ? s->calc_fail2.as<int>() : s->calc_fail.as<int>();
        theorycalc_eval(several ? trial_calculator(s, i) : s->calc, s->W, Prows, (long long)s->dc.ld, s->np,
                        writable(e), e.ld_field, e.ld_walker, flags, stream);
        if (several && !first) {
            hipLaunchKernelGGL(calc_fail_or, dim3((s->W + 255) / 256), dim3(256), 0, stream, s->calc_fail.as<int>(),
                               (const int *)flags, s->W);
            HIP_CHECK(hipGetLastError());
        }
        first = false;
    }
    return true;
}

// A trial outside the calculator's box: every likelihood term becomes logZero,
// so target_like gives logZero as for a trial outside the sampler's bounds
// (the calculator's error flag, calclike.f90:308-313)
__global__ void calc_fail_terms(const int *__restrict__ flag, double *terms, int n_like, int W, size_t ld)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W || flag[w] == 0) return;
    for (int l = 0; l < n_like; l++) terms[(size_t)l * ld + w] = LOGZERO;
}

static void apply_calc_fail(cmbs *s, hipStream_t stream) {
    hipLaunchKernelGGL(calc_fail_terms, dim3((s->W + 255) / 256), dim3(256), 0, stream, s->calc_fail.as<int>(),
                       s->like_terms.as<double>(), s->n_rows(), s->W, (size_t)s->dc.ld);
    HIP_CHECK(hipGetLastError());
}

// What a slow entry needs, checked before its first launch so that a refusal
// leaves the sampler as it was: a chain state and, when it will ask for
// theories, a trial-theory buffer and a theory row per walker (an accepted
// walker keeps its trial theory there) for every likelihood, and a source.
static void check_slow_entry(const cmbs *s, const char *entry, cmbs_theory_fn fn, bool theory) {
    if (!s->started) fail(CMBL_ERR_ARG, "%s: no chain state (cmbs_set_start or cmbs_load_state first)", entry);
    if (!theory) return;
    for (size_t i = 0; i < s->likes.size(); i++) {
        if (!s->end_theory[i].dl)
            fail(CMBL_ERR_ARG, "%s: likelihood %zu has no trial-theory buffer (cmbs_set_trial_theory)", entry, i);
        if (s->likes[i].th.ld_walker == 0)
            fail(CMBL_ERR_ARG, "%s: likelihood %zu needs per-walker theory rows (ld_walker > 0)", entry, i);
    }
    if (!fn)
        for (size_t i = 0; i < std::max<size_t>(s->likes.size(), 1); i++)
            if (!(i < s->likes.size() ? trial_calculator(s, i) : s->calc))
                fail(CMBL_ERR_ARG, "%s needs a theory function or a theory calculator", entry);
    check_derived_calc(s, entry);
}

// The term rows of a slow step's end points Prows (the trial rows): the data
// likelihoods on the trial theories (`pair`: a drag's, by the paired launches
// when they apply), then the derived likelihoods from the calculator.  With the
// calculator as the theory source a point outside its box or a hard range gets
// logZero in every row; a callback step ignores the D_l failure flags, and a
// derived row is logZero outside the box by cmbg_eval's own rule.
static void eval_end_rows(cmbs *s, cmbs_theory_fn fn, void *user, const double *Prows, bool pair, hipStream_t stream) {
    const bool calc = fill_trial_theory(s, fn, user, Prows, stream);
    if (!s->likes.empty() && !(pair && eval_likes_drag_pair(s, stream, false))) eval_likes_drag(s, end_set(s), stream);
    // with no data likelihood no D_l launch has written the flags: the first
    // derived row's box flags, and the calculator's range test over them
    const bool own_flags = calc && s->likes.empty();
    eval_derived_rows(s, Prows, s->like_terms.as<double>(), own_flags ? s->calc_fail.as<int>() : nullptr, stream);
    if (!s->dlikes.empty()) s->drv_cur = false;
    if (own_flags) theorycalc_range_flags(s->calc, s->W, Prows, (long long)s->dc.ld, s->calc_fail.as<int>(), stream);
    if (calc) apply_calc_fail(s, stream);
}

// drag_staged_kernel's LDS image (0 when it would not fit a CU's 160 KB)
static size_t drag_lds_bytes(const cmbs *s) {
    const DevCfg &d = s->dc;
    const int nd_st = d.stage_R ? d.rows.ND : d.rows.ND - d.rows.RR;
    const int ni_st = d.stage_cyc ? d.rows.NI : d.rows.CYC;
    const int ntd = d.stage_cov ? d.tl.n_dbl : d.tl.covinv;
    const int nlk = (d.n_like + 1) & ~1, ndd = (drag_rows(d) + 1) & ~1;
    const size_t b = (size_t)(nd_st + ndd + 2 * nlk) * MB * 8 + (size_t)((ntd + 31) & ~31) * 8 +
                     (size_t)(ni_st + 4 + d.all_n) * MB * 4 + (size_t)((d.tl.n_int + 63) & ~63) * 4;
    return b <= 160 * 1024 ? b : 0;
}

template <int STAGE>
static void launch_drag(cmbs *s, const DragCfg &g, const HistRow &row, hipStream_t stream) {
    const size_t lds = drag_lds_bytes(s);
    timed_launch("drag_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
        if (lds && !s->drag_hbm)
            hipExtLaunchKernelGGL(drag_staged_kernel<STAGE>, dim3((s->W + MB - 1) / MB), dim3(MH_THREADS), lds, stream,
                                  e0, e1, 0, s->dc, g, row.p, row.t);
        else
            hipExtLaunchKernelGGL(drag_kernel<STAGE>, dim3((s->W + 63) / 64), dim3(64), 0, stream, e0, e1, 0, s->dc,
                                  g, row.p, row.t);
    });
    HIP_CHECK(hipGetLastError());
}

// the walkers with flag[w] == value take likelihood i's trial theory, n doubles
// a row, as their own (grid_x workgroups a walker)
static void swap_theory(cmbs *s, size_t i, const int *flag, int value, int grid_x, long long n, hipStream_t stream) {
    if (same_theory_swap(s, i)) return;
    const TheoryView &e = s->end_theory[i], &l = s->likes[i].th;
    hipLaunchKernelGGL(drag_swap_theory, dim3(grid_x, s->W), dim3(256), 0, stream, flag, value, s->W, e.dl,
                       e.ld_walker, writable(l), l.ld_walker, n);
    HIP_CHECK(hipGetLastError());
}

void sampler_step_drag(cmbs *s, int n_steps, double dragging_steps, cmbs_theory_fn fn, void *user,
                       hipStream_t stream) {
    rot_schedule_unknown(s);           // the drag proposals move the blocks' loop indices
    const bool drag = s->fast_n != 0 && s->slow_n != 0;   // else MCMC.f90:351-354: plain Metropolis
    const int nl = (int)s->likes.size(), nr = s->n_rows();
    check_slow_entry(s, "cmbs_step_drag", fn, n_steps > 0 && drag && nr > 0);
    check_theory_fresh(s);
    if (n_steps <= 0) return;
    if (!drag) {
        sampler_step(s, n_steps, 0, stream);
        return;
    }
    const size_t ld = s->dc.ld;
    if (!s->drag_dd.p) {
        s->drag_dd.alloc((size_t)(3 * s->np + 4 + s->dc.max_blk + std::max(1, nr)) * ld * 8);
        s->drag_di.alloc((size_t)(1 + s->all_n) * ld * 4);
        HIP_CHECK(hipMemset(s->drag_dd.p, 0, s->drag_dd.bytes));
        HIP_CHECK(hipMemset(s->drag_di.p, 0, s->drag_di.bytes));
        s->like_terms2.alloc((size_t)std::max(1, nr) * ld * 8);
        HIP_CHECK(hipMemset(s->like_terms2.p, 0, s->like_terms2.bytes));
        for (int i = 0; i < nl; i++)
            s->nuis_bufs2[i].alloc((size_t)std::max(s->likes[i].like->like->n_nuis, 1) * s->W * 8);
    }
    if (s->tpass)   // start_set's fused workspaces
        for (int i : s->tp_like) s->like_ws2[i].grow(s->likes[i].like->like->workspace_size(s->W));
    DragCfg g{};
    g.dd = s->drag_dd.as<double>();
    g.di = s->drag_di.as<int>();
    g.like_terms2 = s->like_terms2.as<double>();
    for (int i = 0; i < nl; i++) g.like_nuis2[i] = s->nuis_bufs2[i].as<double>();
    const int interp = std::max(2, (int)std::lround(dragging_steps * s->fast_n) + 1);   // MCMC.f90:386
    g.interp = interp;
    if (const size_t lds = drag_lds_bytes(s))
        for (const void *k : {(const void *)drag_staged_kernel<0>, (const void *)drag_staged_kernel<1>,
                              (const void *)drag_staged_kernel<2>})
            HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int step = 0; step < n_steps; step++) {
        s->num_drag++;
        if (s->num_drag % s->dc.oversample_fast != 0) {   // FastParameterSample (:357-361)
            derived_rows_current(s, stream);
            launch_mh(s, false, true, 1, HistRow{}, stream, 0, s->W, s->mask_on);
            eval_trial_likes(s, stream, false);
            launch_mh(s, true, false, 1, next_hist(s), stream, 0, s->W, s->mask_on);
            continue;
        }
        g.istep = 0;
        launch_drag<0>(s, g, HistRow{}, stream);
        if (nr > 0) {   // (a flagged end point aborts its drag in stage 1)
            eval_end_rows(s, fn, user, s->dc.sd + (size_t)s->dc.rows.T * ld, true, stream);
            // the slow point of a drag's start does not move: its derived terms are the walker's current ones
            if (nr > nl)
                HIP_CHECK(hipMemcpyAsync(s->like_terms2.as<double>() + (size_t)nl * ld,
                                         s->cur_terms.as<double>() + (size_t)nl * ld, (size_t)(nr - nl) * ld * 8,
                                         hipMemcpyDeviceToDevice, stream));
        }
        launch_drag<1>(s, g, HistRow{}, stream);
        for (int is = 1; is <= interp - 1; is++) {
            if (nl > 0 && !eval_likes_drag_pair(s, stream)) {
                eval_likes_drag(s, end_set(s), stream);
                eval_likes_drag(s, start_set(s), stream);
            }
            g.istep = is;
            const HistRow row = is == interp - 1 ? next_hist(s) : HistRow{};
            launch_drag<2>(s, g, row, stream);
        }
        s->theory_moved = s->theory_moved || nl > 0;
        for (int i = 0; i < nl; i++) {               // accepted drags (dst 4) keep the end theory
            const long long n = std::min(s->end_theory[i].ld_walker, s->likes[i].th.ld_walker);
            swap_theory(s, i, g.di, 4, 8, n > 0 ? n : 10 * s->likes[i].th.ld_field, stream);
        }
        // (every walker's dst is set again by the next drag's stage 0)
    }
}

// full TMetropolisSampler_GetNewSample steps (MCMC.f90:269-307) with the
// theory recomputed at every trial point: the theory source fills the
// trial-theory buffers, the likelihoods run on them, and accepted walkers
// take the trial theory as their own
static void swap_accepted_theory(cmbs *s, hipStream_t stream) {
    const int *flag = s->dc.si + (size_t)s->dc.rows.ACCF * s->dc.ld;
    s->theory_moved = true;
    for (size_t i = 0; i < s->likes.size(); i++)
        swap_theory(s, i, flag, 1, 16, std::min(s->end_theory[i].ld_walker, s->likes[i].th.ld_walker), stream);
}

void sampler_step_theory(cmbs *s, int n_steps, cmbs_theory_fn fn, void *user, hipStream_t stream) {
    check_slow_entry(s, "cmbs_step_theory", fn, n_steps > 0 && s->n_rows() > 0);
    check_theory_fresh(s);
    if (n_steps <= 0) return;
    if (s->n_rows() == 0) {
        sampler_step(s, n_steps, 0, stream);
        return;
    }
    // propose(1) | theories, likes | accept(1) + propose(2) | swap | theories, likes | ... | accept(n) | swap
    for (int k = 0; k <= n_steps; k++) {
        launch_mh(s, k > 0, k < n_steps, 0, k > 0 ? next_hist(s) : HistRow{}, stream, 0, s->W);
        if (k > 0) swap_accepted_theory(s, stream);
        if (k == n_steps) break;
        eval_end_rows(s, fn, user, s->dc.sd + (size_t)s->dc.rows.T * s->dc.ld, false, stream);
    }
}

// After a resume: the theory at every walker's current point (rows P) from the
// theory source, copied into each likelihood's walker theory rows
// (the reference recomputes theory at the restart point too,
// GeneralSetup.f90:123-131).  The restored CurLike and per-likelihood terms are
// kept as saved, not re-evaluated: the source must reproduce the theory the run
// had at those points (under a change mask, unchanged likelihoods keep their
// saved terms).
__global__ void copy_theory_rows(int W, const double *src, long long src_ld, double *dst, long long dst_ld, long long n)
{
    const int w = blockIdx.y;
    if (w >= W) return;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[(long long)w * dst_ld + i] = src[(long long)w * src_ld + i];
}

void sampler_refresh_theory(cmbs *s, cmbs_theory_fn fn, void *user, hipStream_t stream) {
    check_slow_entry(s, "cmbs_refresh_theory", fn, true);
    if (fill_trial_theory(s, fn, user, s->dc.sd + (size_t)s->dc.rows.P * s->dc.ld, stream)) {
        // the calculator: a point outside its box has no theory to resume with
        std::vector<int> bad(s->likes.empty() ? 0 : s->W);
        HIP_CHECK(hipMemcpyAsync(bad.data(), s->calc_fail.p, bad.size() * 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        const long n_bad = (long)std::count_if(bad.begin(), bad.end(), [](int b) { return b != 0; });
        if (n_bad > 0)
            fail(CMBL_ERR_NUMERIC, "cmbs_refresh_theory: %ld of %d walkers lie outside the theory calculator's box",
                 n_bad, s->W);
    }
    for (size_t i = 0; i < s->likes.size(); i++) {
        const TheoryView &e = s->end_theory[i], &l = s->likes[i].th;
        hipLaunchKernelGGL(copy_theory_rows, dim3(16, s->W), dim3(256), 0, stream, s->W, e.dl, e.ld_walker,
                           writable(l), l.ld_walker, std::min(e.ld_walker, l.ld_walker));
        HIP_CHECK(hipGetLastError());
    }
    s->theory_stale = false;
}
