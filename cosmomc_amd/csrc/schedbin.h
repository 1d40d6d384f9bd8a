// Host side: the bin co-run fast-step schedule (mh_bin_kernel; state: BinCorun,
// sampler.h).  Included once by sampler.hip inside namespace cmamd, after
// launch_mh.
//
// propose(1) + bins(1) | [rotations] | quadform(1) | accept(1) + propose(2) + bins(2) |
// ... | quadform(n) | accept(n)

// Whether this run of fast steps can take the bin co-run: one likelihood,
// plik_lite, deferred (its quadratic form's combine in the next mh launch),
// no fused pass, one walker group, no change mask.  Allocates the raw sums and
// sets up the calibration hand-off once per W.
static bool bin_setup(cmbs *s, int fast_only, PlikBinArgs &pb) {
    // (the unified launch needs the fused pass, so plik_lite alone comes here)
    if (s->sched_mode == 0 || !fast_only || s->tpass || s->n_groups != 1 || s->mask_on ||
        s->likes.size() != 1 || !s->dlikes.empty() || !is_deferred(s, 0))
        return false;
    const LikeSlot &L = s->likes[0];
    WinStage st;
    if (!L.like->like->bin_args(pb, L.th.dl, L.th.ld_field, L.th.ld_walker) || !L.like->like->window_stage(st) ||
        st.cal_index < 0)
        return false;
    BinCorun &bc = s->bin;
    bc.S.grow((size_t)QuadForm::wpad(s->W) * pb.Np * 8);   // allocated zero: the padding stays 0
    for (int f = 0; f < 3; f++)
        if (pb.fr.b1[f] - pb.fr.b0[f] > 2 * MH_THREADS) return false;   // mh_bin_kernel: two bins a thread
    bc.lds = std::max(s->mh_lds, (size_t)pb.lds_doubles * 8);
    if (bc.lds > 160 * 1024) return false;
    for (const void *k : {(const void *)mh_bin_kernel<true>, (const void *)mh_bin_kernel<false>})
        HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bc.lds));
    if (bc.ready == s->W) return true;
    s->pipe_status.init();
    // both halves unset: the first launch publishes into half 1, resets half 0
    const std::vector<unsigned long long> unset((size_t)4 * s->dc.ld, TP_PIPE_UNSET);
    bc.cal.alloc(unset.size() * 8);
    bc.cal.upload(unset.data(), unset.size() * 8);
    bc.epoch = 0;
    bc.ready = s->W;
    return true;
}

// A proposing Metropolis launch over every walker with plik's binning riding
// along (mh_bin_kernel), then the rotation launch when one is due
static void launch_mh_bin(cmbs *s, bool accept, int fast_only, const HistRow &row, hipStream_t stream,
                          const PlikBinArgs &pb) {
    BinCorun &bc = s->bin;
    if (s->pending.n && !accept) fail(CMBL_ERR_ARG, "internal: deferred likelihoods without an accepting step");
    DevCfg dc = launch_cfg(s, fast_only, false);
    const bool rot = rot_schedule(s, dc, true, fast_only, 0);
    Like &Q = *s->likes[0].like->like;
    WinStage st;
    Q.window_stage(st);
    dc.pub_on = s->handoff_nosignal ? 0 : 1;   // debug: never publish (the give-up test)
    dc.pub_pcal[0] = s->likes[0].nidx[st.cal_index];
    dc.pub_pcal[1] = -1;
    const unsigned e = bc.epoch + 1;   // this launch's half e % 2; it resets the other for the next
    dc.calbuf = bc.cal.as<double>() + (size_t)(e % 2) * 2 * dc.ld;
    dc.calbuf_next = bc.cal.as<double>() + (size_t)((e + 1) % 2) * 2 * dc.ld;
    dc.bin_on = 1;
    dc.bin_nused = pb.nused;
    dc.bin_Np = pb.Np;
    dc.bin_cal = st.cal_index;
    dc.bin_S = bc.S.as<double>();
    dc.bin_X = pb.X;
    dc.bin_delta = Q.window_out(s->like_ws[0].p, s->W);
    const int nmh = (s->W + MB - 1) / MB, nmh_pad = (nmh + 7) / 8 * 8;
    const dim3 gb(nmh_pad + s->W), b(MH_THREADS);
    try {
        timed_launch("mh_bin_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(accept ? mh_bin_kernel<true> : mh_bin_kernel<false>, gb, b, bc.lds, stream, e0, e1,
                                  0, dc, fast_only, row.p, row.t, nmh, nmh_pad, pb, s->pipe_status.dev);
        });
        HIP_CHECK(hipGetLastError());
    } catch (...) {
        bc.invalidate();
        s->pipe_status.post_nothrow(stream);
        throw;
    }
    bc.epoch = e;
    if (rot) launch_rot(dc, stream, 0, s->W);
}

// plik's deferred quadratic form over the Delta rows the bin co-run (and
// rot_kernel) formed; its combine runs in the next Metropolis launch
static void launch_bin_qf(cmbs *s, hipStream_t stream) {
    Like &Q = *s->likes[0].like->like;
    const QFDeferred d = Q.after_window(s->W, s->dc.like_nuis[0], std::max(1, Q.n_nuis), nullptr, s->like_ws[0].p,
                                        stream, true);
    record_deferred(s, 0, d);
}

static void run_bin_corun(cmbs *s, int n_steps, int fast_only, const PlikBinArgs &pb, hipStream_t stream) {
    for (int k = 0; k < n_steps; k++) {
        launch_mh_bin(s, k > 0, fast_only, k > 0 ? next_hist(s) : HistRow{}, stream, pb);
        launch_bin_qf(s, stream);
    }
    launch_mh(s, true, false, fast_only, next_hist(s), stream, 0, s->W, false);
    s->pipe_status.post(stream);
}
