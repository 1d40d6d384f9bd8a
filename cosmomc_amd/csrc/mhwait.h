// The in-launch hand-off of the unified step launch: the producers' arrival
// on their walker tile's counter and the Metropolis workgroups' wait for it.
// Included by sampler.hip after mhstage.h (mhlean.h and mhbody.h wait here).
// (included inside namespace cmamd)
#pragma once

// A Metropolis workgroup of the unified step launch waits here until its
// walker tile's quadratic-form and chi^2 workgroups have arrived (TailWait),
// then acquires their write-through outputs.  The producers are all earlier in
// the grid and wait on nothing, so the count arrives; the wait still gives up
// after TAIL_WAIT_SPINS polls and sets the status word, which the next step
// call reports as an error (sampler_check_pipe).  The bound counts polls, not
// wall-clock time: a poll does not advance while the wave is switched out (a
// shared GPU), so a waiter restored before its producers never gives up early.
// The per-tile arrival counters each on a line of their own (TW_PAD words
// apart), and the waiters poll them every TW_SLEEP x 64 cycles: the counters
// are agent-scope, so every poll and arrival goes past the XCD's L2, and 64
// waiters polling one line in a tight loop slow the quadratic form's own
// loads on the chip.
static constexpr int TW_SLEEP = 20;
static constexpr int TW_PAD = 64;
static constexpr long TAIL_WAIT_SPINS = (1l << 25) / TW_SLEEP;   // polls: ~1 s

// A give-up: the sampler's status word lives in pinned host memory (mapped),
// so the host reads it once the step call's event has completed, without a
// copy launch; every writer stores the same bit, so a plain system-scope store
// serves (no read-modify-write over the bus)
__device__ __forceinline__ void pipe_giveup(int *status)
{
    __hip_atomic_store(status, CMBL_STATUS_PIPE_WAIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ void tail_wait(const TailWait &tw, int tile)
{
    if (threadIdx.x == 0) {
        const int gpt = 64 / tw.gwt, g0 = tile * gpt;
        const int gq = max(0, min(gpt, tw.ng - g0));
        // every accepting launch adds its quadratic-form workgroups, and those whose
        // chi^2 ran as workgroups of its own (not folded) add the tile's chi^2 ones
        const unsigned target = tw.epoch * (unsigned)tw.nq_items + tw.epoch_g * (unsigned)gq;
        for (long it = 0;; it++) {
            const unsigned v = __hip_atomic_load(tw.cnt + tile * TW_PAD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v >= target) break;
            if (it == TAIL_WAIT_SPINS) {
                pipe_giveup(tw.status);
                break;
            }
            __builtin_amdgcn_s_sleep(TW_SLEEP);
        }
        // one acquire after the match (cdna_hip_programming.md Guideline 16 recipe): it drops this
        // CU's L1 lines; its own wait holds the barrier, then every wave loads
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef CMAMD_STAMPS
        if (blockIdx.x < 2048) g_uni_stamps[tw.stamp_slot][blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
#endif
    }
    __syncthreads();
}

// The hand-off is cdna_hip_programming.md's counter recipe in its
// write-through form (the note to its split-K combine, after Guideline 16):
// the producers' stores are sc1 (write-through past the XCD L2), so no
// release fence precedes the relaxed agent-scope fetch_add -- every wave
// drains its stores, the workgroup barriers, one lane adds; the consumer
// polls relaxed and takes one acquire fence after the match (tail_wait).
// A release fence here would be a whole-L2 write-back per producer
// workgroup (measured on the pass units: 35.8 -> 122 us a launch).
__device__ __forceinline__ void tail_arrive(const TailWait &tw, int tile)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's write-through stores are done
    __syncthreads();
    if (threadIdx.x == 0 && !tw.nosignal)
        __hip_atomic_fetch_add(tw.cnt + tile * TW_PAD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
