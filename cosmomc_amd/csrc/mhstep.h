// The unified step launch's body: the roles of its rows of workgroups.
// Included by sampler.hip after qfs_body.h, smallgauss.h, theorypass_body.h,
// mhwait.h and mhbody.h.
// (included inside namespace cmamd)
#pragma once

// The unified step launch (sched_mode 3): one launch per fast step.  Rows of
// workgroups (tail_rows) run step k's tails -- plik_lite's quadratic form from
// raw sums and the lensing chi^2, which store write-through and arrive on
// their walker tile's counter -- the window pass storing step k + 1's raw sums,
// and the Metropolis workgroups (first when the chi^2 is folded into them, else
// last: steptail.hip), which wait for their tile's arrivals
// (tail_wait), accept step k (finishing plik's deferred combine from the
// partials of this launch) and propose step k + 1.  The pass waits on
// nothing; the Metropolis chain of a tile starts as soon as its tails are
// done instead of at a kernel boundary, and overlaps the pass.
// The hand-off between the rows is mhwait.h's.

// walkers per chi^2 workgroup of the chi^2 rows (4 / 8 / 16: 35.7-35.8 /
// 35.9-36.0 / 35.9-36.0 us per middle launch, round 5)
static constexpr int UNI_WT = 4;

template <bool ACCEPT, bool PROPOSE>
__device__ __forceinline__ void mh_step_body(DevCfg &c, int fast_only, double *hist_row, double *hist_terms,
                                             StepTail &t, const int2 *__restrict__ rows, TailWait &tw, int nmh)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int2 rr = rows[blockIdx.x >> 3];
    const int lb = rr.y * 8 + (blockIdx.x & 7);
    if (!ACCEPT && blockIdx.x == 0)   // a call's first launch (no tails): the arrival counters start from 0
        for (int i = threadIdx.x; i < tw.ntiles; i += MH_THREADS) tw.cnt[i] = 0u;
#ifdef CMAMD_STAMPS
    const bool stamp = ACCEPT && threadIdx.x == 0 && blockIdx.x < 2048;
    const int slot = PROPOSE ? 0 : 1;
    if (stamp) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_uni_stamps[slot][blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
        g_uni_stamps[slot][blockIdx.x][2] = xcc & 15;
        g_uni_stamps[slot][blockIdx.x][4] = 0;
        g_uni_stamps[slot][blockIdx.x][5] = 0;
    }
    struct End {
        bool on;
        int role, slot;
        __device__ ~End() {
            if (on) {
                g_uni_stamps[slot][blockIdx.x][3] = __builtin_amdgcn_s_memrealtime();
                g_uni_stamps[slot][blockIdx.x][4] = role + 1;
            }
        }
    } end_{stamp, rr.x, slot};
#endif
    if (rr.x == TAIL_QF) {
        if (lb >= t.nq) return;
        int item_ix, tile;
        qf_place(lb, t.q.src.n_items, t.q.src.xcd_map, item_ix, tile);
        // the quadratic form's waves above the pass's at issue (the Metropolis
        // waves' 3 stays highest): 35.98 / 36.26 -> 35.90 / 35.80 us per step in two
        // interleaved repetitions (round 6, DESIGN.md section 5's table)
        __builtin_amdgcn_s_setprio(2);
        qfs_body(lds, item_ix, tile, t.q);
        tail_arrive(tw, tile);
    } else if (rr.x == TAIL_GAUSS) {
        // contiguous walker groups per XCD (lb % 8 is the XCD): each partial row's
        // 128-byte lines are read by one XCD's L2 instead of four (35.1 -> 34.5 us)
        const int grows = (t.ng + 7) >> 3, q = (lb & 7) * grows + (lb >> 3);
        if (q >= t.ng) return;
        small_gauss_body<UNI_WT, true, true>(t.g, lds, q);
        tail_arrive(tw, q * UNI_WT / 64);
    } else if (rr.x == TAIL_PASS) {
        if (lb >= t.np) return;
        // the weights prefetched one step ahead: two, as the standalone kernels, measured
        // 0.3 us slower a launch with 288-l items and the same within noise with 352-l
        // items (32.6 / 32.0 / 31.8 against 32.1 / 32.4 / 31.9 us, round 6)
        tp_vec_body<2, true, false>(t.tp, t.dl, t.ld_field, t.ld_walker, t.W, reinterpret_cast<char *>(lds), lb);
    } else if (lb < nmh) {
        // the chain is latency on one lane: its waves, dispatched last (the youngest,
        // so the last in issue arbitration), take the SIMD first (34.6 -> 34.0 us)
        __builtin_amdgcn_s_setprio(3);
        if (ACCEPT && t.fold_g) {
            // the small chi^2 of this workgroup's 16 walkers (step k's raw partial
            // rows, whole 128-byte lines) while the quadratic form runs elsewhere:
            // nX <= 16, so its sums are those of the 4-walker rows (same bits); the
            // chain's loads of the term follow tail_wait's acquire
            small_gauss_body<MB, true, false>(t.g, lds, lb);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
#ifdef CMAMD_STAMPS
            if (threadIdx.x == 0 && blockIdx.x < 2048)
                g_uni_stamps[PROPOSE ? 0 : 1][blockIdx.x][5] = __builtin_amdgcn_s_memrealtime();
#endif
        }
        mh_body<ACCEPT, PROPOSE>(c, fast_only, hist_row, hist_terms, 0, lds, lb, ACCEPT ? &tw : nullptr);
    }
}
