// Batched Metropolis sampler: W independent CosmoMC chains, one per walker
// (one GPU lane per walker for the sequential per-chain logic), with the
// likelihoods evaluated as batched kernels over all walkers in between.
//
// Per-walker semantics follow the reference exactly, including the random
// number call order, so that walker w with RANMAR seeds (ij_w, kl_w)
// reproduces a reference chain started with the same seeds:
//   RANMAR / Gaussian1 / randexp1 / RandIndices / RandRotationD  RandUtils.f90:93-374
//   BlockedProposer GetProposal{,Fast,Slow}, ProposeVec, Propose_r,
//   UpdateParams, CyclicIndexRandomizer%Next                      propose.f90:75-298
//   GetLogLike = bounds + like/T + priors/T                        calclike.f90:82-151
//   MetropolisAccept, MoveDone multiplicity                        MCMC.f90:119-190
//
// The chain logic is a long chain of dependent state reads (RNG index ->
// RNG table -> block cycle -> rotation -> mapping ...).  Served from HBM each
// would cost a memory round trip; instead mh_kernel stages the whole
// per-walker state (sampler.h Rows) and the shared tables into LDS with
// independent coalesced loads, runs the chain out of LDS and writes back.
//
// This file holds every kernel entry point of the chain, then the host side:
// set-up, the Metropolis launch and cmbs_step.  The device bodies are
// headers included inside namespace cmamd, in this order: mhrng.h (RANMAR),
// mhpropose.h (walker view, proposer, target), mhstage.h (LDS staging),
// mhwait.h (the unified launch's arrival and wait), mhlean.h and mhbody.h (the
// lean and the general chain), mhstep.h (the unified launch's roles), mhrot.h
// (deferred rotations), mhdrag.h (fast dragging).  Four host-side headers
// follow in the same way: likeeval.h (the likelihoods' evaluation at a set of
// points), schedbin.h and schedunified.h (the two pipelined fast-step
// schedules, each with its set-up, launches and run) and slowstep.h
// (cmbs_step_theory, cmbs_step_drag and cmbs_refresh_theory).  The history
// statistics are history.hip, the state image state.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <cstdlib>

#include "plikbin.h"
#include "qfs_body.h"
#include "quadform.h"
#include "sampler.h"
#include "smallgauss.h"
#include "theorycalc.h"
#ifdef CMAMD_STAMPS
namespace cmamd {
// mh_step_kernel (tools/uni_stamps.py), [0] the middle launches, [1] the last
// (accept-only) launch: start, the Metropolis wait's end, XCC id, end, role + 1
__device__ unsigned long long g_uni_stamps[2][2048][6];   // start, wait done, xcc, end, role + 1, folded chi^2 done
}
#endif
#include "theorypass_body.h"

namespace cmamd {

static constexpr double LOGZERO = CMBL_LOGZERO;
static constexpr int MAXP = 64;        // max parameters per chain
static constexpr int MAXBLK = 32;      // max block size
static constexpr int NB = 64;          // walker tile of the history / collector kernels (one wavefront)
// mh_kernel: MB walkers per block (lanes 0..MB-1 of wave 0 run their chain
// logic) and MH_THREADS threads, i.e. NV = MH_THREADS / MB groups of MB threads
// for the staging, the deferred combines and the multi-group products.  With
// 16-walker blocks a W = 1024 step spreads over 64 CUs instead of 16: each
// block stages a quarter of the state image (round 3: 64-walker blocks, 16
// waves, 12.9 us).
static constexpr int MB = 16;
static constexpr int MH_THREADS = 256;
static constexpr int NV = MH_THREADS / MB;
static_assert(NV >= QF_GROUPS && NV % QF_GROUPS == 0, "a group per split-K group sum");
static_assert(64 % MB == 0, "blocks tile the 64-walker rows of the split-K partials");

#include "mhrng.h"

__global__ void rng_init_kernel(DevCfg c, const int *ij, const int *kl)
{   // RMARIN, RandUtils.f90:286-348
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= c.W) return;
    const size_t W = c.ld;
    int i = (ij[w] / 177) % 177 + 2, j = ij[w] % 177 + 2, k = (kl[w] / 169) % 178 + 1, l = kl[w] % 169;
    for (int ii = 0; ii < 97; ii++) {
        double s = 0.0, t = 0.5;
        for (int jj = 0; jj < 24; jj++) {
            const int m = (((i * j) % 179) * k) % 179;
            i = j;
            j = k;
            k = m;
            l = (53 * l + 1) % 169;
            if ((l * m) % 64 >= 32) s += t;
            t *= 0.5;
        }
        c.sd[(c.rows.U + ii) * W + w] = s;
    }
    c.sd[c.rows.C * W + w] = 362436.0 / 16777216.0;
    c.sd[c.rows.G * W + w] = 0.0;
    c.si[c.rows.I97 * W + w] = 97;
    c.si[c.rows.J97 * W + w] = 33;
    c.si[c.rows.ISET * W + w] = 0;
}

#include "mhpropose.h"
#include "mhstage.h"
#include "mhwait.h"
#include "mhlean.h"

#include "mhbody.h"

template <bool ACCEPT, bool PROPOSE>
__global__ __launch_bounds__(MH_THREADS) void mh_kernel(DevCfg c, int fast_only, double *hist_row, double *hist_terms, int blk0)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    mh_body<ACCEPT, PROPOSE>(c, fast_only, hist_row, hist_terms, blk0, lds, blockIdx.x);
}

// A proposing mh_kernel with plik_lite's binning riding along (the bin
// co-run of sampler_step): workgroups [0, nmh) are mh_kernel's, the pad up to
// a multiple of 8 idle, the rest bin a walker each (its three fields in
// turn: one workgroup per walker keeps the whole grid resident beside the
// Metropolis workgroups' LDS size; plik_bin_products and the bin sums), wait
// for the walker's trial calibration (published by its Metropolis workgroup
// into DevCfg::calbuf straight after the proposal) and emit
// Delta = X - S / cal^2 into plik's rows -- or, for a walker whose proposal
// waits on a new rotation (TP_PIPE_ROT), the raw sums, from which rot_kernel
// forms its Delta after the launch.  The binning runs on the CUs the
// latency-bound Metropolis chain leaves idle (it takes 32 of 256 at
// W = 512); only its emit waits.
// The bins wait on workgroups with lower ids.  The HIP model does not promise
// that workgroups are dispatched in id order (cdna_hip_programming.md
// "Workgroups, grid, and XCD partitioning"); the hardware's dispatcher is
// observed to, so the Metropolis workgroups are resident before any waiting
// bin workgroup takes a slot and the wait ends.  The design does not rely on
// it for correctness: the wait is bounded by a count of polls
// (TAIL_WAIT_SPINS), and a give-up sets CMBL_STATUS_PIPE_WAIT in the
// sampler's status word, which the next step call or state readback turns
// into an error (sampler_check_pipe) instead of silently rejected trials.
template <bool ACCEPT>
__global__ __launch_bounds__(MH_THREADS) void mh_bin_kernel(DevCfg c, int fast_only, double *hist_row,
                                                            double *hist_terms, int nmh, int nmh_pad, PlikBinArgs pb,
                                                            int *status)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double cal_s;
    const int b = blockIdx.x;
    if (b < nmh_pad) {
        if (b < nmh) mh_body<ACCEPT, true>(c, fast_only, hist_row, hist_terms, 0, lds, b);
        return;
    }
    const int w = b - nmh_pad;
    for (int i = pb.nused + (int)threadIdx.x; i < pb.Np; i += MH_THREADS)   // the Delta row's padding columns
        c.bin_delta[(size_t)w * pb.Np + i] = 0.0;
    // the three fields in turn through one LDS image: this thread's bin sums
    // (plik_bin_emit's, at most two bins a field: bin_setup) before the wait,
    // so only the emit follows the calibration
    double acc[3][2] = {};
#pragma unroll
    for (int f = 0; f < 3; f++) {
        if (f > 0) __syncthreads();   // the previous field's sums have read the image
        if (!plik_bin_products(pb, lds, w, f)) continue;
        const double *P = lds - pb.fr.lo[f];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = pb.fr.b0[f] + (int)threadIdx.x + k * MH_THREADS;
            if (i < pb.fr.b1[f]) {
                const BinInfo bi = pb.bins[i];
                for (int l = bi.lmin; l <= bi.lmax; l++) acc[f][k] += P[l];
            }
        }
    }
    if (threadIdx.x == 0) {
        double cl;
        for (long it = 0;; it++) {   // bounded by polls (tail_wait): a safety net, reported loudly
            cl = __hip_atomic_load(c.calbuf + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned long long)__double_as_longlong(cl) != TP_PIPE_UNSET) break;
            if (it == (1l << 20)) {   // x s_sleep(24): ~0.7 s
                pipe_giveup(status);
                break;
            }
            __builtin_amdgcn_s_sleep(24);   // ~1500 cycles: 3 W pollers must not crowd the L2
        }
        cal_s = cl;
    }
    __syncthreads();
    const double cl = cal_s, c2 = cl * cl;
    const bool rot = (unsigned long long)__double_as_longlong(cl) == TP_PIPE_ROT;
    double *out = (rot ? const_cast<double *>(c.bin_S) : c.bin_delta) + (size_t)w * pb.Np;
#pragma unroll
    for (int f = 0; f < 3; f++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = pb.fr.b0[f] + (int)threadIdx.x + k * MH_THREADS;
            if (pb.fr.hi[f] >= pb.fr.lo[f] && i < pb.fr.b1[f]) out[i] = rot ? acc[f][k] : pb.X[i] - acc[f][k] / c2;
        }
}

#include "mhstep.h"

template <bool ACCEPT, bool PROPOSE>
__global__ __launch_bounds__(MH_THREADS, 3) void mh_step_kernel(DevCfg c, int fast_only, double *hist_row,
                                                                double *hist_terms, StepTail t,
                                                                const int2 *__restrict__ rows, TailWait tw, int nmh)
{
    mh_step_body<ACCEPT, PROPOSE>(c, fast_only, hist_row, hist_terms, t, rows, tw, nmh);
}

// The same launch without the pass, for the binned-theory cache
// (cmbs_set_binned_cache): its own symbol, so profiles of a run with both
// legs keep the headline launch's statistics apart
template <bool ACCEPT, bool PROPOSE>
__global__ __launch_bounds__(MH_THREADS, 3) void mh_tail_kernel(DevCfg c, int fast_only, double *hist_row,
                                                                double *hist_terms, StepTail t,
                                                                const int2 *__restrict__ rows, TailWait tw, int nmh)
{
    mh_step_body<ACCEPT, PROPOSE>(c, fast_only, hist_row, hist_terms, t, rows, tw, nmh);
}

#include "mhrot.h"
#include "mhdrag.h"

// Starting point: -lnL of P = trial (likelihood terms already evaluated)
__global__ void start_kernel(DevCfg c)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= c.W) return;
    const size_t W = c.ld;
    const Tabs t = make_tabs(c, c.tab_i, c.tab_d);
    Col<double> q{c.sd + (size_t)c.rows.T * W + w, c.ld};
    Col<const double> lk{c.like_terms + w, c.ld};
    c.sd[(size_t)c.rows.L * W + w] = target_like(c, t, q, lk);
    for (int l = 0; l < c.n_like; l++) c.cur_terms[(size_t)l * W + w] = lk[l];
    for (int i = 0; i < c.np; i++) c.sd[(size_t)(c.rows.P + i) * W + w] = q[i];
    c.sd[(size_t)c.rows.M * W + w] = 0.0;
    c.si[(size_t)c.rows.NACC * W + w] = 0;
}

// DataParams of every walker's trial point, P(nuisance_indices)
// (GeneralTypes.f90:642-646, calclike.f90:380): out[w][k] = trial[nidx[k]][w]
__global__ void gather_nuis(const double *trial, int W, int ld, const int *nidx, int n_nuis, double *out)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    for (int k = 0; k < n_nuis; k++) out[(size_t)w * n_nuis + k] = trial[(size_t)nidx[k] * ld + w];
}

// Change mask, sparse likelihoods: the walkers whose flag is set get compact
// slots in walker order (a deterministic block scan; one 1024-thread block per
// sparse likelihood); the flag becomes slot + 1, slot -> walker goes to map,
// the walker's DataParams row is copied to its slot, and cnt[b] is the count.
struct SparseSet {
    int like[MAXLIKE], nn[MAXLIKE];
    double *nuisc[MAXLIKE];
    int *map[MAXLIKE];
};

__global__ __launch_bounds__(1024) void like_compact_kernel(DevCfg c, SparseSet ss, int *__restrict__ cnt)
{
    __shared__ int wsum[16];
    const int b = blockIdx.x, l = ss.like[b], nn = ss.nn[b];
    int *flag = c.like_flag + (size_t)l * c.ld;
    const double *nuis = c.like_nuis[l];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int chunk = (c.W + 1023) / 1024, w0 = t * chunk, w1 = min(c.W, w0 + chunk);
    int n = 0;
    for (int w = w0; w < w1; w++) n += flag[w] != 0;
    int v = n;                                       // inclusive scan: wave, then the 16 wave totals
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int before = 0;
    for (int q = 0; q < wave; q++) before += wsum[q];
    int off = before + v - n;
    for (int w = w0; w < w1; w++)
        if (flag[w] != 0) {
            flag[w] = off + 1;
            ss.map[b][off] = w;
            for (int q = 0; q < nn; q++) ss.nuisc[b][(size_t)off * nn + q] = nuis[(size_t)w * nn + q];
            off++;
        }
    if (t == 1023) cnt[b] = before + v;
}

// theory rows of the compacted walkers (sparse likelihood with per-walker theory)
__global__ __launch_bounds__(256) void gather_theory_kernel(const double *__restrict__ dl, long long ld_walker,
                                                            long long ext, const int *__restrict__ map,
                                                            const int *__restrict__ cnt, double *__restrict__ dlc)
{
    const int w = blockIdx.x;
    if (w >= *cnt) return;
    const double *src = dl + (long long)map[w] * ld_walker;
    double *dst = dlc + (long long)w * ld_walker;
    for (long long i = threadIdx.x; i < ext; i += 256) dst[i] = src[i];
}

// ------------------------------------------------------------ host side

static size_t mh_lds_bytes(const cmbs *s) {
    const DevCfg &d = s->dc;
    const int nd_st = d.stage_R ? d.rows.ND : d.rows.ND - d.rows.RR;
    const int ni_st = d.stage_cyc ? d.rows.NI : d.rows.CYC;
    const int ntd = d.stage_cov ? d.tl.n_dbl : d.tl.covinv;
    return (size_t)(nd_st + MAXLIKE + d.max_blk + d.tq_rows + d.def_cap * (QF_GROUPS + 1)) * MB * 8 +
           (size_t)((ntd + 31) & ~31) * 8 +
           (size_t)(ni_st + (d.stage_cyc ? d.all_n : 0)) * MB * 4 + (size_t)((d.tl.n_int + 63) & ~63) * 4 +
           MB * 4 + (size_t)d.np * MB * 8 + 2 * MB * 4 + 64;
}

static void set_mh_lds(cmbs *s) {
    // The mh_kernel LDS image: everything staged when it fits the 160 KB of a
    // CU; otherwise, in this order, the rotation rows, the cyclic-index
    // permutations (+ RandIndices scratch), the test-Gaussian tables and the
    // multi-wave scratch rows stay in HBM and are read in place.
    DevCfg &d = s->dc;
    const size_t cap = 160 * 1024;
    // the rotation rows stay in HBM when they are many (128 or more) and
    // every rotation wider than one parameter is drawn by rot_kernel: the
    // chain then only reads one column
    // per proposal (fetched beside the image, pre_blk), and staging the n x n
    // rows in and out of LDS is most of the image (config4_fast21: 441 of
    // ~600 rows)
    bool all_deferred = d.rot_defer != 0 && s->R_total >= 128;
    for (int bn : s->blk_n) all_deferred = all_deferred && (bn == 1 || bn >= ROT_DEFER_MIN);
    d.stage_R = s->stage_R_force >= 0 ? s->stage_R_force : (all_deferred ? 0 : 1);
    d.stage_cyc = d.stage_cov = 1;
    d.tq_rows = d.test_like ? 2 * s->n_used : 2;   // two per test-Gaussian row, or the proposal's block and step
    d.def_cap = (int)s->defer_likes.size();
    if (mh_lds_bytes(s) > cap) {               // the deferred combines go first: the likelihoods combine in-launch
        d.def_cap = 0;
        s->defer_likes.clear();
    }
    if (mh_lds_bytes(s) > cap) d.stage_R = 0;
    if (mh_lds_bytes(s) > cap) d.stage_cyc = 0;
    if (mh_lds_bytes(s) > cap) d.stage_cov = 0;
    if (mh_lds_bytes(s) > cap) d.tq_rows = 0;
    s->mh_lds = mh_lds_bytes(s);
    if (s->mh_lds > cap) fail(CMBL_ERR_ARG, "sampler state too large for LDS (%zu bytes)", s->mh_lds);
    if (!d.stage_cyc && !s->itmp_g.p) {
        s->itmp_g.alloc((size_t)std::max(1, s->all_n) * d.ld * 4);
        d.itmp_g = s->itmp_g.as<int>();
    }
    for (const void *k : {(const void *)mh_kernel<true, true>, (const void *)mh_kernel<true, false>,
                          (const void *)mh_kernel<false, true>})
        HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->mh_lds));
}

static void upload_tables(cmbs *s) {
    HIP_CHECK(hipDeviceSynchronize());     // the old tables may be read by queued kernels
    // padded to whole 256-byte LDS-DMA pieces
    s->tab_i.alloc(((s->h_tab_i.size() + 63) / 64 + 1) * 256);
    s->tab_i.upload(s->h_tab_i.data(), s->h_tab_i.size() * 4);
    s->tab_d.alloc(((s->h_tab_d.size() + 31) / 32 + 1) * 256);
    s->tab_d.upload(s->h_tab_d.data(), s->h_tab_d.size() * 8);
    s->dc.tab_i = s->tab_i.as<int>();
    s->dc.tab_d = s->tab_d.as<double>();
}

void sampler_create(cmbs *s, const cmbs_config_t *cfg) {
    if (cfg->n_walkers <= 0 || cfg->num_params <= 0 || cfg->num_params > MAXP)
        fail(CMBL_ERR_ARG, "n_walkers > 0 and 0 < num_params <= %d required", MAXP);
    if (cfg->n_used <= 0 || cfg->n_used > cfg->num_params) fail(CMBL_ERR_ARG, "bad n_used");
    s->W = cfg->n_walkers;
    s->np = cfg->num_params;
    s->n_used = cfg->n_used;
    s->params_used.assign(cfg->params_used, cfg->params_used + cfg->n_used);
    for (int p : s->params_used)
        if (p < 1 || p > s->np) fail(CMBL_ERR_ARG, "params_used entry %d out of range", p);
    // BlockedProposer Init (propose.f90:151-208)
    std::vector<int> used_blocks;
    for (int b = 0; b < cfg->n_blocks; b++) {
        const int n = cfg->block_n[b];
        if (n > MAXBLK) fail(CMBL_ERR_ARG, "block of %d parameters exceeds %d", n, MAXBLK);
        if (n > 0) {
            s->all_n += n;
            if (b + 1 <= cfg->slow_block_max) s->slow_n += n;
            used_blocks.push_back(b);
        }
    }
    std::vector<int> boff(cfg->n_blocks + 1, 0);
    for (int b = 0; b < cfg->n_blocks; b++) boff[b + 1] = boff[b] + cfg->block_n[b];
    s->fast_n = s->all_n - s->slow_n;
    s->nblocks = (int)used_blocks.size();
    if (s->nblocks == 0) fail(CMBL_ERR_ARG, "no parameter blocks");
    s->indices.assign(s->all_n, 0);
    s->proposer_for_index.assign(s->all_n, 0);
    int ix = 1;
    for (int i = 0; i < s->nblocks; i++) {
        const int ub = used_blocks[i];
        s->blk_start.push_back(ix);
        s->blk_n.push_back(cfg->block_n[ub]);
        for (int k = 0; k < cfg->block_n[ub]; k++) {
            const int u = cfg->block_params[boff[ub] + k];
            if (u < 1 || u > s->n_used) fail(CMBL_ERR_ARG, "block parameter %d not a used index", u);
            s->indices[ix - 1 + k] = u;
            s->proposer_for_index[ix - 1 + k] = i + 1;
        }
        ix += cfg->block_n[ub];
    }
    for (int v : s->indices)
        if (v == 0) fail(CMBL_ERR_ARG, "DecomposeCovariance: not all used parameters blocked");
    for (int i = 0; i < s->nblocks; i++) {
        const int nc = s->all_n - s->blk_start[i] + 1;
        s->blk_nchanged.push_back(nc);
        s->blk_changed_off.push_back((int)s->changed.size());
        s->blk_map_off.push_back(s->map_total);
        s->blk_R_off.push_back(s->R_total);
        for (int k = 0; k < nc; k++) {
            const int u = s->indices[s->blk_start[i] - 1 + k];
            s->used_params_changed_all.push_back(u);
            s->changed.push_back(s->params_used[u - 1] - 1);
        }
        s->map_total += nc * s->blk_n[i];
        s->R_total += s->blk_n[i] * s->blk_n[i];
    }
    if (s->all_n > MAXP) fail(CMBL_ERR_ARG, "too many parameters");

    const int np = s->np, W = s->W, nb = s->nblocks;
    DevCfg &d = s->dc;
    d.W = W;
    d.np = np;
    d.n_used = s->n_used;
    d.nblocks = nb;
    d.slow_n = s->slow_n;
    d.fast_n = s->fast_n;
    d.all_n = s->all_n;
    d.oversample_fast = cfg->oversample_fast < 1 ? 1 : cfg->oversample_fast;
    d.propose_scale = cfg->propose_scale;
    d.temperature = cfg->temperature > 0 ? cfg->temperature : 1.0;
    d.R_total = s->R_total;
    d.max_blk = 1;
    for (int bn : s->blk_n) d.max_blk = std::max(d.max_blk, bn);
    d.rot_defer = d.max_blk >= ROT_DEFER_MIN ? 1 : 0;

    // ---- shared tables
    TabLayout &tl = d.tl;
    auto &vi = s->h_tab_i;
    auto &vd = s->h_tab_d;
    auto put_i = [&](int &off, const std::vector<int> &v) {
        off = (int)vi.size();
        vi.insert(vi.end(), v.begin(), v.end());
    };
    auto put_d = [&](int &off, const double *v, int n) {
        off = (int)vd.size();
        vd.insert(vd.end(), v, v + n);
    };
    put_i(tl.blk_n, s->blk_n);
    put_i(tl.blk_nchanged, s->blk_nchanged);
    put_i(tl.blk_changed_off, s->blk_changed_off);
    put_i(tl.blk_map_off, s->blk_map_off);
    put_i(tl.blk_R_off, s->blk_R_off);
    put_i(tl.changed, s->changed);
    put_i(tl.pfi, s->proposer_for_index);
    std::vector<int> pu0(s->n_used);
    for (int i = 0; i < s->n_used; i++) pu0[i] = s->params_used[i] - 1;
    put_i(tl.params_used, pu0);
    tl.n_int = (int)vi.size();
    std::vector<double> zeros(std::max(s->map_total, np), 0.0);
    put_d(tl.mapping, zeros.data(), s->map_total);
    put_d(tl.pmin, cfg->pmin, np);
    put_d(tl.pmax, cfg->pmax, np);
    std::vector<double> pm(np, 0.0), ps(np, 0.0);
    std::vector<char> varying(np, 0);
    for (int p : s->params_used) varying[p - 1] = 1;
    bool has_pri = false;
    if (cfg->prior_mean && cfg->prior_std) {
        for (int i = 0; i < np; i++) {
            // GetLogPriors gate, calclike.f90:119 (TBaseParameters_ReadPriors :175 reads no prior otherwise)
            if (!varying[i] && !cfg->include_fixed_parameter_priors) continue;
            pm[i] = cfg->prior_mean[i];
            ps[i] = cfg->prior_std[i];
            has_pri |= ps[i] != 0.0;
        }
    }
    put_d(tl.pmean, pm.data(), np);
    put_d(tl.pstd, ps.data(), np);
    const int nlin = cfg->n_lincomb > 0 ? cfg->n_lincomb : 0;
    if (nlin && (!cfg->lincomb_weights || !cfg->lincomb_mean || !cfg->lincomb_std))
        fail(CMBL_ERR_ARG, "n_lincomb > 0 needs lincomb_weights, lincomb_mean and lincomb_std");
    put_d(tl.lin_w, cfg->lincomb_weights, nlin * np);
    put_d(tl.lin_m, cfg->lincomb_mean, nlin);
    put_d(tl.lin_s, cfg->lincomb_std, nlin);
    for (int k = 0; k < nlin; k++) has_pri |= cfg->lincomb_std[k] != 0.0;
    d.n_lin = nlin;
    tl.covinv = tl.center = (int)vd.size();   // set by cmbs_set_test_gaussian
    tl.n_dbl = (int)vd.size();
    d.has_priors = has_pri;
    d.test_like = 0;
    upload_tables(s);

    // ---- per-walker state rows
    Rows &R = d.rows;
    R.RR = (s->R_total + 1) & ~1;
    R.P = R.R + R.RR;
    R.T = R.P + np;
    R.L = R.T + np;
    R.M = R.L + 1;
    R.ND = (R.M + 2) & ~1;
    R.ACCF = R.BLKLP + nb;
    R.PROT = R.ACCF + 1;
    R.CYC = (R.PROT + 1 + 3) & ~3;
    R.NI = (R.CYC + s->all_n + s->slow_n + s->fast_n + 3) & ~3;
    d.ld = (W + NB - 1) / NB * NB;
    s->sd.alloc((size_t)R.ND * d.ld * 8);
    s->si.alloc((size_t)R.NI * d.ld * 4);
    HIP_CHECK(hipMemset(s->sd.p, 0, (size_t)R.ND * d.ld * 8));
    HIP_CHECK(hipMemset(s->si.p, 0, (size_t)R.NI * d.ld * 4));
    d.sd = s->sd.as<double>();
    d.si = s->si.as<int>();
    // rotation lists: walker indices [ld] + two counters per 64-walker range
    s->rot.alloc((size_t)(d.ld + 2 * (d.ld / 64)) * 4);
    HIP_CHECK(hipMemset(s->rot.p, 0, (size_t)(d.ld + 2 * (d.ld / 64)) * 4));
    d.rot_list = s->rot.as<int>();
    d.rot_cnt = d.rot_list + d.ld;
    s->rot_par.assign(d.ld / 64, 0);
    s->rot_lp.assign(d.ld / 64, 0);                   // every loop index starts at 0
    {   // the fast blocks: any deferred?  a single one (its width)?
        std::vector<int> fb;
        for (int q = s->slow_n; q < s->all_n; q++) {
            const int b = s->proposer_for_index[q] - 1;
            if (std::find(fb.begin(), fb.end(), b) == fb.end()) fb.push_back(b);
        }
        s->rot_fast_any = false;
        for (int b : fb) s->rot_fast_any = s->rot_fast_any || s->blk_n[b] >= ROT_DEFER_MIN;
        s->rot_fast_n = (fb.size() == 1 && s->blk_n[fb[0]] >= ROT_DEFER_MIN) ? s->blk_n[fb[0]] : 0;
        d.pre_blk = (fb.size() == 1 && s->blk_n[fb[0]] >= 2) ? fb[0] : -1;
        d.pre_off = d.pre_blk >= 0 ? s->blk_R_off[d.pre_blk] : 0;
        d.pre_n = d.pre_blk >= 0 ? s->blk_n[d.pre_blk] : 0;
    }
    HIP_CHECK(hipFuncSetAttribute((const void *)rot_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(ROT_WAVES * sizeof(RotLds))));

    set_mh_lds(s);

    // seeds
    std::vector<int> ij(W), kl(W);
    for (int w = 0; w < W; w++) cmbs_walker_seed(cfg->seed_ij, cfg->seed_kl, cfg->first_walker + w, &ij[w], &kl[w]);
    DevBuf dij(W * 4), dkl(W * 4);
    dij.upload(ij.data(), W * 4);
    dkl.upload(kl.data(), W * 4);
    hipLaunchKernelGGL(rng_init_kernel, dim3((W + 255) / 256), dim3(256), 0, 0, d, dij.as<int>(), dkl.as<int>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
}

static void cholesky_lower(std::vector<double> &A, int n) {
    for (int j = 0; j < n; j++) {
        double dd = A[j * n + j];
        for (int k = 0; k < j; k++) dd -= A[j * n + k] * A[j * n + k];
        if (!(dd > 0.0)) fail(CMBL_ERR_NUMERIC, "Matrix_Cholesky: not positive definite %d", j + 1);
        dd = std::sqrt(dd);
        A[j * n + j] = dd;
        for (int i = j + 1; i < n; i++) {
            double x = A[i * n + j];
            for (int k = 0; k < j; k++) x -= A[i * n + k] * A[j * n + k];
            A[i * n + j] = x / dd;
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) A[i * n + j] = 0.0;
}

void sampler_set_covariance(cmbs *s, const double *cov) {
    // BlockedProposer_SetCovariance, propose.f90:210-244 (host, once per update)
    const int n = s->n_used, na = s->all_n;
    std::vector<double> sig(n), corr((size_t)n * n);
    for (int i = 0; i < n; i++) {
        if (!(cov[i * n + i] > 0)) fail(CMBL_ERR_NUMERIC, "proposal covariance has non-positive diagonal");
        sig[i] = std::sqrt(cov[i * n + i]);
        for (int j = 0; j < n; j++) corr[i * n + j] = cov[i * n + j] / sig[i];
    }
    for (int i = 0; i < n; i++)
        for (int k = 0; k < n; k++) corr[k * n + i] = corr[k * n + i] / sig[i];
    std::vector<double> L((size_t)na * na);
    for (int i = 0; i < na; i++)
        for (int j = 0; j < na; j++) L[i * na + j] = corr[(s->indices[i] - 1) * n + (s->indices[j] - 1)];
    cholesky_lower(L, na);
    int uoff = 0;
    for (int i = 0; i < s->nblocks; i++) {
        const int bn = s->blk_n[i], st = s->blk_start[i], nc = s->blk_nchanged[i];
        for (int j = 0; j < nc; j++)
            for (int k = 0; k < bn; k++)
                s->h_tab_d[s->dc.tl.mapping + s->blk_map_off[i] + j * bn + k] =
                    sig[s->used_params_changed_all[uoff + j] - 1] * L[(st - 1 + j) * na + (st - 1 + k)];
        uoff += nc;
    }
    upload_tables(s);
}

void sampler_set_test_gaussian(cmbs *s, const double *cov, const double *center) {
    const int n = s->n_used;
    std::vector<double> A(cov, cov + (size_t)n * n);
    // Matrix_Inverse (test_likelihood inverts its covariance, calclike.f90:187-195)
    for (int i = 0; i < n; i++)
        if (std::fabs(A[i * n + i]) < 1e-30) fail(CMBL_ERR_NUMERIC, "Matrix_Inverse: very small diagonal");
    cholesky_lower(A, n);
    for (int j = 0; j < n; j++) {
        A[j * n + j] = 1.0 / A[j * n + j];
        for (int i = j + 1; i < n; i++) {
            double x = 0.0;
            for (int k = j; k < i; k++) x += A[i * n + k] * A[k * n + j];
            A[i * n + j] = -x / A[i * n + i];
        }
    }
    std::vector<double> T((size_t)n * n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j <= i; j++) {
            double x = 0.0;
            for (int k = i; k < n; k++) x += A[k * n + i] * A[k * n + j];
            T[i * n + j] = T[j * n + i] = x;
        }
    auto &vd = s->h_tab_d;
    TabLayout &tl = s->dc.tl;
    vd.resize(tl.covinv);                   // replace any previous test_likelihood
    vd.insert(vd.end(), T.begin(), T.end());
    tl.center = (int)vd.size();
    vd.insert(vd.end(), center, center + s->np);
    tl.n_dbl = (int)vd.size();
    s->dc.test_like = 1;
    set_mh_lds(s);
    upload_tables(s);
}

static void set_change_mask(cmbs *s);

// the pipelined fast-step schedules' set-up no longer holds (likelihoods
// changed, or a hand-off gave up): each sets up afresh at its next run
static void invalidate_schedules(cmbs *s) {
    s->unified.invalidate();
    s->bin.invalidate();
}

// Segment starts (absolute l, even) about TP_MAXL apart over [lo, hi] at which
// none of the bins [b.first, b.second] is split.
static std::vector<int> bin_safe_cuts(const std::vector<std::pair<int, int>> &bins, int lo, int hi, int L) {
    auto valid = [&](int c) {
        if (c % 2 != 0) return false;
        for (auto &b : bins)
            if (b.first < c && c <= b.second) return false;
        return true;
    };
    std::vector<int> cuts;
    int pos = lo;
    while (pos + L <= hi) {
        int c = -1;
        for (int x = pos + L; x > pos && c < 0; x--)
            if (valid(x)) c = x;
        for (int x = pos + L + 1; x <= hi && c < 0; x++)
            if (valid(x)) c = x;
        if (c < 0) break;
        cuts.push_back(c);
        pos = c;
    }
    return cuts;
}

// Fused window pass: a plik_lite likelihood (window stage kind 1) and a
// CMBlikes likelihood (kind 0) evaluated densely on the same theory buffer.
// The CMBlikes windows are re-segmented at l where no plik bin is split, so
// every column of both lies in one work item of the pass.
static void setup_fusion(cmbs *s) {
    s->tpass.reset();
    s->tp_like[0] = s->tp_like[1] = -1;
    invalidate_schedules(s);
    const int nl = (int)s->likes.size();
    auto sparse = [&](int i) {
        for (int q : s->sparse_likes)
            if (q == i) return true;
        return false;
    };
    s->tp_why = 0;
    for (int i = 0; i < nl; i++)
        for (int j = 0; j < nl; j++) {
            if (i == j) continue;
            s->tp_why = std::max(s->tp_why, 1);
            if (sparse(i) || sparse(j)) continue;
            const LikeSlot &P = s->likes[i], &C = s->likes[j];
            s->tp_why = std::max(s->tp_why, 2);
            if (!(P.th == C.th)) continue;
            WinStage sp, sc;
            s->tp_why = std::max(s->tp_why, 3);
            if (!P.like->like->window_stage(sp) || sp.kind != 1) continue;
            s->tp_why = std::max(s->tp_why, 4);
            if (!C.like->like->window_stage(sc) || sc.kind != 0) continue;
            s->tp_why = std::max(s->tp_why, 5);
            std::map<int, std::vector<std::pair<int, int>>> bins;
            for (auto &c : sp.cols) bins[c.field].push_back({c.lo, c.hi});
            std::map<int, std::vector<int>> starts;
            for (auto &kv : bins) {
                int lo = 1 << 30, hi = -1;
                for (auto &c : sc.cols)
                    if (c.field == kv.first) {
                        lo = std::min(lo, c.lo);
                        hi = std::max(hi, c.hi);
                    }
                if (hi < lo) continue;
                starts[kv.first] = bin_safe_cuts(kv.second, lo & ~1, hi, TP_MAXL);
            }
            // the handle may be shared (standalone calls, other samplers): its
            // segmentation changes only if the fused pass is kept
            const auto saved = C.like->like->window_segments();
            if (!C.like->like->window_resegment(starts) || !C.like->like->window_stage(sc)) {
                C.like->like->window_set_segments(saved);
                continue;
            }
            s->tp_why = std::max(s->tp_why, 6);
            std::unique_ptr<TheoryPass> tp(new TheoryPass());
            if (!tp->build({sp, sc})) {
                C.like->like->window_set_segments(saved);
                continue;
            }
            s->tpass = std::move(tp);
            s->tp_like[0] = i;
            s->tp_like[1] = j;
            s->tp_stage[0] = sp;
            s->tp_stage[1] = sc;
            for (int k : s->tp_like) s->like_ws[k].release();
            size_t maxws = 0;   // the CMBlikes workspace follows its partial rows
            for (auto &l : s->likes) maxws = std::max(maxws, l.like->like->workspace_size(s->W));
            if (maxws > s->ws.bytes) s->ws.alloc(maxws);
            return;
        }
}

// One more term row (a likelihood was pushed): like_terms, cur_terms and the
// history's terms ring grow, the existing rows kept
static void add_term_row(cmbs *s) {
    const int rows = s->n_rows(), li = rows - 1;
    const size_t nlk = ((size_t)rows + 1) & ~size_t(1);
    DevBuf nt(nlk * (size_t)s->dc.ld * 8);
    HIP_CHECK(hipMemset(nt.p, 0, nt.bytes));
    if (li > 0) HIP_CHECK(hipMemcpy(nt.p, s->like_terms.p, (size_t)li * s->dc.ld * 8, hipMemcpyDeviceToDevice));
    std::swap(nt.p, s->like_terms.p);
    std::swap(nt.bytes, s->like_terms.bytes);
    s->dc.n_like = rows;
    s->dc.like_terms = s->like_terms.as<double>();
    {   // current-point terms: one more row, the existing ones kept
        DevBuf ct((size_t)rows * s->dc.ld * 8);
        HIP_CHECK(hipMemset(ct.p, 0, ct.bytes));
        if (li > 0) HIP_CHECK(hipMemcpy(ct.p, s->cur_terms.p, (size_t)li * s->dc.ld * 8, hipMemcpyDeviceToDevice));
        std::swap(ct.p, s->cur_terms.p);
        std::swap(ct.bytes, s->cur_terms.bytes);
        s->dc.cur_terms = s->cur_terms.as<double>();
    }
    if (s->hist_cap > 0) {   // the terms ring follows the number of likelihoods
        s->hist_terms.alloc((size_t)s->hist_cap * rows * s->W * 8);
        HIP_CHECK(hipMemset(s->hist_terms.p, 0, s->hist_terms.bytes));
    }
}

void sampler_add_likelihood(cmbs *s, cmbl_t *like, const int *nuisance_indices, const double *dl, long long ld_field,
                            long long ld_walker) {
    if (!like) fail(CMBL_ERR_ARG, "null likelihood");
    const int nn = like->like->n_nuis;
    if (nn > 0 && !nuisance_indices) fail(CMBL_ERR_ARG, "likelihood has %d nuisance parameters: indices needed", nn);
    std::vector<int> nidx(nn);
    for (int q = 0; q < nn; q++) {
        if (nuisance_indices[q] < 1 || nuisance_indices[q] > s->np)
            fail(CMBL_ERR_ARG, "nuisance index %d out of range 1..%d", nuisance_indices[q], s->np);
        nidx[q] = nuisance_indices[q] - 1;
    }
    if (!s->dlikes.empty())
        fail(CMBL_ERR_ARG, "data likelihoods are added before derived likelihoods (their term rows come first)");
    if ((int)s->likes.size() >= MAXLIKE) fail(CMBL_ERR_ARG, "at most %d likelihoods per sampler", MAXLIKE);
    const int li = (int)s->likes.size();
    s->likes.push_back({like, nidx, TheoryView{dl, ld_field, ld_walker}});
    // the index list joins the int table (LDS-staged with the proposer tables)
    s->dc.like_nidx[li] = (int)s->h_tab_i.size();
    s->h_tab_i.insert(s->h_tab_i.end(), nidx.begin(), nidx.end());
    s->dc.tl.n_int = (int)s->h_tab_i.size();
    set_mh_lds(s);
    upload_tables(s);
    add_term_row(s);
    s->nuis_bufs[li].alloc((size_t)std::max(nn, 1) * s->W * 8);
    s->dc.like_nuis[li] = s->nuis_bufs[li].as<double>();
    s->dc.like_nn[li] = nn;
    size_t maxws = 0;
    for (auto &l : s->likes) maxws = std::max(maxws, l.like->like->workspace_size(s->W));
    s->ws.alloc(maxws);
    set_change_mask(s);
    // likelihoods whose quadratic-form combine the accepting mh_kernel can take
    // over (dense evaluation only: the sparse ones write compacted slots)
    s->defer_likes.clear();
    for (int i = 0; i < (int)s->likes.size() && (int)s->defer_likes.size() < MAXDEF; i++) {
        bool sparse = false;
        for (int q : s->sparse_likes) sparse |= q == i;
        if (!sparse && s->likes[i].like->like->deferred_capable()) s->defer_likes.push_back(i);
    }
    for (int i = 0; i < MAXLIKE; i++) s->like_ws[i].release();
    set_mh_lds(s);
    setup_fusion(s);
    for (int i : s->defer_likes) s->like_ws[i].alloc(s->likes[i].like->like->workspace_size(s->W));
    for (int i : s->tp_like)
        if (i >= 0 && !s->like_ws[i].p) s->like_ws[i].alloc(s->likes[i].like->like->workspace_size(s->W));
    if (s->n_groups > 1) sampler_set_groups(s, s->n_groups);   // resize the group workspaces
}

// A derived likelihood: one more term row after the data likelihoods', with no
// DataParams and no dependent parameters.  The pipelined fast-step schedules
// carry the data likelihoods' rows alone, so with a derived likelihood the
// fast steps take the general schedule (the same bits).
void sampler_add_derived_likelihood(cmbs *s, cmbg *g) {
    if (!g) fail(CMBL_ERR_ARG, "null derived likelihood");
    if (s->n_rows() >= MAXLIKE) fail(CMBL_ERR_ARG, "at most %d likelihoods per sampler", MAXLIKE);
    const int r = s->n_rows();
    s->dlikes.push_back(g);
    add_term_row(s);
    s->dc.like_nidx[r] = 0;
    s->dc.like_nn[r] = 0;
    s->dc.like_nuis[r] = nullptr;
    set_change_mask(s);
    s->drv_cur = false;
    invalidate_schedules(s);
    s->drag_dd.release();   // the drag's scratch rows follow the number of term rows
}

// the derived likelihoods' term rows (of `terms` [n_like][ld]) at the
// parameter rows Prows [np][ld]
static void eval_derived_rows(cmbs *s, const double *Prows, double *terms, int *fail_flags, hipStream_t stream) {
    for (size_t k = 0; k < s->dlikes.size(); k++)
        theorygauss_eval(s->dlikes[k], s->W, Prows, (long long)s->dc.ld, s->np,
                         terms + (s->likes.size() + k) * (size_t)s->dc.ld, k == 0 ? fail_flags : nullptr, stream);
}

// A fast step's trial has the walker's slow point, so its derived terms are the
// current ones: the dense paths read every row from like_terms, whose derived
// rows hold a slow trial's terms after a slow step
static void derived_rows_current(cmbs *s, hipStream_t stream) {
    if (s->dlikes.empty() || s->drv_cur) return;
    const size_t off = s->likes.size() * (size_t)s->dc.ld;
    HIP_CHECK(hipMemcpyAsync(s->like_terms.as<double>() + off, s->cur_terms.as<double>() + off,
                             s->dlikes.size() * (size_t)s->dc.ld * 8, hipMemcpyDeviceToDevice, stream));
    s->drv_cur = true;
}

// derived likelihoods are evaluated by the sampler's calculator
static void check_derived_calc(const cmbs *s, const char *entry) {
    if (s->dlikes.empty()) return;
    if (!s->calc)
        fail(CMBL_ERR_ARG, "%s: derived likelihoods need the theory calculator (cmbs_set_theory_calculator)", entry);
    for (size_t k = 0; k < s->dlikes.size(); k++)
        if (s->dlikes[k]->calc != s->calc)
            fail(CMBL_ERR_ARG, "%s: derived likelihood %zu was created on another calculator than the sampler's", entry, k);
}

// Change mask set-up (recomputed as likelihoods are added).  dependent_params
// of a CMB likelihood are its nuisance parameters (GeneralTypes.f90:648) and
// every theory parameter (CosmologyTypes.f90:154); here the theory parameters
// are the ones no likelihood owns as a nuisance parameter.  A likelihood whose
// dependent set misses some varying parameter can be skipped for walkers that
// did not move it; those that support it are evaluated on compacted walker
// slots (sparse), the others densely with the same keep-the-current-term rule.
static void set_change_mask(cmbs *s) {
    const int nl = (int)s->likes.size(), W = s->W;
    const size_t ld = s->dc.ld;
    unsigned long long nuis_all = 0;
    for (auto &l : s->likes)
        for (int i : l.nidx) nuis_all |= 1ull << i;
    const unsigned long long all = (s->np >= 64) ? ~0ull : ((1ull << s->np) - 1);
    const unsigned long long theory = all & ~nuis_all;
    s->sparse_likes.clear();
    for (int li = 0; li < nl; li++) {
        unsigned long long dep = theory;
        for (int i : s->likes[li].nidx) dep |= 1ull << i;
        s->dc.like_dep[li] = dep;
        bool maskable = false;
        for (int u : s->params_used) maskable |= !((dep >> (u - 1)) & 1ull);
        s->dc.like_out[li] = nullptr;
        if (maskable && s->likes[li].like->like->sparse_capable()) s->sparse_likes.push_back(li);
    }
    for (int r = nl; r < s->n_rows(); r++) {   // derived likelihoods: a fast step's trial keeps their current term
        s->dc.like_dep[r] = 0;
        s->dc.like_out[r] = nullptr;
    }
    s->mask_on = !s->sparse_likes.empty();
    if (!s->mask_on) return;
    s->like_flag.alloc((size_t)s->n_rows() * ld * 4);
    s->dc.like_flag = s->like_flag.as<int>();
    s->like_cnt.alloc(256);
    for (int li : s->sparse_likes) {
        const int nn = std::max(1, s->likes[li].like->like->n_nuis);
        s->like_outc[li].alloc((size_t)W * 8);
        s->like_nuisc[li].alloc((size_t)W * nn * 8 + (size_t)ld * 4);   // + the slot -> walker map
        s->dc.like_out[li] = s->like_outc[li].as<double>();
        if (s->likes[li].th.ld_walker != 0) s->like_dlc[li].alloc((size_t)W * s->likes[li].th.ld_walker * 8);
    }
}

#include "likeeval.h"

// the history ring slots of the next recorded step (none when history is off)
struct HistRow {
    double *p = nullptr;   // [n_used + 1][W]: used parameters, CurLike
    double *t = nullptr;   // [n_like][W]: per-likelihood terms
};

static HistRow next_hist(cmbs *s) {
    HistRow r;
    if (s->hist_cap == 0) return r;
    const size_t slot = (size_t)(s->hist_count % s->hist_cap);
    r.p = s->hist.as<double>() + slot * (s->n_used + 1) * s->W;
    if (s->n_rows() > 0 && s->hist_terms.p) r.t = s->hist_terms.as<double>() + slot * s->n_rows() * s->W;
    s->hist_count++;
    return r;
}

// Whether a proposing launch over the walker range from g0 can leave a
// rotation pending, so rot_kernel is worth launching.  Fast-only steps
// propose only fast blocks: none of them deferred, never.  With a single fast
// block every walker proposes in it at every fast-only step, so all of its
// loop indices move together and the host knows them (rot_lp: proposals so
// far mod n, or -1 once anything else has touched them: full steps, dragging,
// a loaded state, a new walker split); a rotation is due when it is 0 mod n.
static bool rot_may_pend(cmbs *s, int fast_only, int g0) {
    if (!s->dc.rot_defer) return false;
    int &lp = s->rot_lp[g0 / 64];
    if (!fast_only) {
        lp = -1;
        return true;
    }
    if (!s->rot_fast_any) return false;
    if (s->rot_fast_n == 0 || lp < 0) return true;
    const bool due = lp % s->rot_fast_n == 0;
    lp = (lp + 1) % s->rot_fast_n;
    return due;
}

void rot_schedule_unknown(cmbs *s) { std::fill(s->rot_lp.begin(), s->rot_lp.end(), -1); }

void PipeStatus::init() {
    if (!host) {
        HIP_CHECK(hipHostMalloc((void **)&host, 64, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_CHECK(hipHostGetDevicePointer((void **)&dev, host, 0));
        HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    // no kernel of an earlier call still writes the word once ev has completed:
    // every call that launched a hand-off kernel recorded it afterwards (post,
    // also on the error paths), so waiting on this sampler's event suffices --
    // other samplers' and the caller's work on the device are not waited for.
    // A give-up that call left is raised here, not cleared unread
    check(true);
    *reinterpret_cast<volatile int *>(host) = 0;
}

void PipeStatus::post(hipStream_t stream) {
    HIP_CHECK(hipEventRecord(ev, stream));
    pending = true;
}

void PipeStatus::post_nothrow(hipStream_t stream) {
    if (ev && hipEventRecord(ev, stream) == hipSuccess) pending = true;
}

void PipeStatus::check(bool wait) {
    if (!pending) return;
    if (wait) HIP_CHECK(hipEventSynchronize(ev));
    const hipError_t q = hipEventQuery(ev);
    if (q == hipErrorNotReady) return;   // checked at a later call
    HIP_CHECK(q);
    pending = false;
    if (*reinterpret_cast<volatile int *>(host) & CMBL_STATUS_PIPE_WAIT) {
        *reinterpret_cast<volatile int *>(host) = 0;
        fail(CMBL_ERR_NUMERIC, "a pipelined step's in-launch hand-off gave up waiting (CMBL_STATUS_PIPE_WAIT): "
                               "the walkers' last steps are invalid");
    }
}

void sampler_check_pipe(cmbs *s, bool wait) {
    try {
        s->pipe_status.check(wait);
    } catch (...) {
        invalidate_schedules(s);
        throw;
    }
}

// The lean chain's LDS (mhlean.h's carve)
static size_t lean_lds_bytes(const cmbs *s) {
    const Rows &R = s->dc.rows;
    return (size_t)(R.R + R.ND - R.P + MAXDEF * (QF_GROUPS + 1) + s->np) * MB * 8 + (size_t)(8 + 3) * MB * 4;
}

// Whether a launch of fast-only steps takes the lean chain (mhlean.h): the
// only fast parameter is a one-parameter block, no test likelihood, no
// linear-combination priors, no change mask; and that block's constants.
static LeanCfg lean_cfg(const cmbs *s, int fast_only, bool masked) {
    LeanCfg L{};
    const DevCfg &d = s->dc;
    if (s->lean_off || !fast_only || masked || s->fast_n != 1 || d.test_like || d.n_lin || d.n_like > MAXLIKE)
        return L;
    const int b = s->proposer_for_index[s->slow_n] - 1;
    if (s->blk_n[b] != 1 || s->blk_nchanged[b] > LEAN_MAXC || lean_lds_bytes(s) > s->mh_lds) return L;
    for (int l = 0; l < (int)s->likes.size(); l++) {   // (a derived likelihood's row has none)
        const std::vector<int> &ni = s->likes[l].nidx;
        if ((int)ni.size() > LEAN_MAXQ) return LeanCfg{};
        L.nn[l] = (int)ni.size();
        for (size_t q = 0; q < ni.size(); q++) L.nuis[l][q] = ni[q];
    }
    L.nc = s->blk_nchanged[b];
    for (int j = 0; j < L.nc; j++) {
        L.chg[j] = s->changed[s->blk_changed_off[b] + j];
        L.map[j] = s->h_tab_d[d.tl.mapping + s->blk_map_off[b] + j];
    }
    L.r_row = d.rows.R + s->blk_R_off[b];
    L.cyc_row = d.rows.CYC + s->all_n + s->slow_n;
    L.blklp_row = d.rows.BLKLP + b;
    L.on = 1;
    return L;
}

// The DevCfg of one launch: the sampler's, with every per-launch field at its
// neutral value except the deferred combines the last evaluation left
// pending, which it takes over.  The launchers set what they use.
static DevCfg launch_cfg(cmbs *s, int fast_only, bool masked) {
    DevCfg dc = s->dc;
    dc.mask_on = masked ? 1 : 0;
    dc.lean = lean_cfg(s, fast_only, masked);
    dc.pre_lp = -1;
    dc.rot_par = 0;
    dc.pub_on = 0;
    dc.bin_on = 0;
    PendingDeferred &pd = s->pending;
    dc.n_def = pd.n;
    std::copy(pd.like, pd.like + pd.n, dc.def_like);
    std::copy(pd.items, pd.items + pd.n, dc.def_items);
    std::copy(pd.part, pd.part + pd.n, dc.def_part);
    std::copy(pd.add, pd.add + pd.n, dc.def_add);
    pd.n = 0;
    return dc;
}

// The rotation schedule's part of a launch over the walker range from g0:
// whether rot_kernel follows it (launch_rot), and then its rotation list
static bool rot_schedule(cmbs *s, DevCfg &dc, bool propose, int fast_only, int g0) {
    // the single deferred block's loop index before this launch's proposals (rot_may_pend)
    if (propose && fast_only && dc.rot_defer && s->rot_fast_n > 0 && dc.pre_blk >= 0 && s->rot_lp[g0 / 64] >= 0)
        dc.pre_lp = s->rot_lp[g0 / 64];
    const bool rot = propose && rot_may_pend(s, fast_only, g0);
    if (rot) {                       // alternate the two rotation-list counters of this walker range
        dc.rot_par = s->rot_par[g0 / 64];
        s->rot_par[g0 / 64] ^= 1;
    }
    return rot;
}

// the walkers of [g0, g1) whose proposal waits on a new rotation
static void launch_rot(const DevCfg &dc, hipStream_t stream, int g0, int g1) {
    timed_launch("rot_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
        hipExtLaunchKernelGGL(rot_kernel, dim3((g1 - g0 + ROT_WAVES - 1) / ROT_WAVES), dim3(64 * ROT_WAVES),
                              ROT_WAVES * sizeof(RotLds), stream, e0, e1, 0, dc, g0);
    });
    HIP_CHECK(hipGetLastError());
}

static void launch_mh(cmbs *s, bool accept, bool propose, int fast_only, const HistRow &row, hipStream_t stream,
                      int g0, int g1, bool masked = false) {
    const dim3 g((g1 - g0 + MB - 1) / MB), b(MH_THREADS);
    if (s->pending.n && !accept) fail(CMBL_ERR_ARG, "internal: deferred likelihoods without an accepting step");
    DevCfg dc = launch_cfg(s, fast_only, masked);
    const bool rot = rot_schedule(s, dc, propose, fast_only, g0);
    timed_launch("mh_kernel", stream, [&](hipEvent_t e0, hipEvent_t e1) {
        const auto k = !accept ? mh_kernel<false, true> : propose ? mh_kernel<true, true> : mh_kernel<true, false>;
        hipExtLaunchKernelGGL(k, g, b, s->mh_lds, stream, e0, e1, 0, dc, fast_only, row.p, row.t, g0 / MB);
    });
    HIP_CHECK(hipGetLastError());
    if (rot) launch_rot(dc, stream, g0, g1);
}

void sampler_set_start(cmbs *s, const double *P0, hipStream_t stream) {
    check_derived_calc(s, "cmbs_set_start");
    // host [W][np] -> device trial rows [np][W]
    std::vector<double> t((size_t)s->np * s->W);
    for (int w = 0; w < s->W; w++)
        for (int i = 0; i < s->np; i++) t[(size_t)i * s->W + w] = P0[(size_t)w * s->np + i];
    HIP_CHECK(hipMemcpy2DAsync(s->dc.sd + (size_t)s->dc.rows.T * s->dc.ld, (size_t)s->dc.ld * 8, t.data(),
                               (size_t)s->W * 8, (size_t)s->W * 8, s->np, hipMemcpyHostToDevice, stream));
    // t is pageable and local: the copy must be complete before anything below can throw and unwind it
    HIP_CHECK(hipStreamSynchronize(stream));
    gather_trial_nuis(s, stream);
    eval_likes(s, stream, 0, s->W, s->ws.p);
    eval_derived_rows(s, s->dc.sd + (size_t)s->dc.rows.T * s->dc.ld, s->like_terms.as<double>(), nullptr, stream);
    s->drv_cur = true;   // start_kernel makes these terms the current ones
    hipLaunchKernelGGL(start_kernel, dim3((s->W + 255) / 256), dim3(256), 0, stream, s->dc);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
    s->started = true;
}

static void check_theory_fresh(const cmbs *s) {
    if (s->theory_stale)
        fail(CMBL_ERR_ARG, "resumed from a state image whose walkers moved their slow parameters: recompute the "
                           "theory at the restored points with cmbs_refresh_theory before stepping");
}

#include "schedbin.h"
#include "schedunified.h"

// propose(1) | likes | accept(1)+propose(2) | likes | ... | likes | accept(n)
static void run_plain(cmbs *s, int n_steps, int fast_only, hipStream_t stream) {
    for (int k = 0; k <= n_steps; k++) {
        launch_mh(s, k > 0, k < n_steps, fast_only, k > 0 ? next_hist(s) : HistRow{}, stream, 0, s->W, s->mask_on);
        if (k < n_steps) eval_trial_likes(s, stream, true);
    }
}

// The same steps per walker group.  Groups are independent chains: fork from
// the caller's stream, issue the step chain of every group breadth-first so
// the queues interleave, join
static void run_groups(cmbs *s, int n_steps, int fast_only, hipStream_t stream) {
    const int G = s->n_groups;
    HIP_CHECK(hipEventRecord(s->events[MAXGROUPS], stream));
    for (int g = 0; g < G; g++) HIP_CHECK(hipStreamWaitEvent(s->streams[g], s->events[MAXGROUPS], 0));
    // A fused pair (the window pass over one theory buffer) is evaluated for the
    // whole walker set after the groups' Metropolis launches, all on the
    // caller's stream: a group's own loglike_batch splits the window sums
    // differently from the pass, and a walker's terms must not depend on the
    // number of groups.
    const bool whole = s->tpass != nullptr;
    for (int k = 0; k <= n_steps; k++) {
        const HistRow row = k > 0 ? next_hist(s) : HistRow{};
        for (int g = 0; g < G; g++) {
            const int g0 = s->grp0[g], g1 = s->grp0[g + 1];
            launch_mh(s, k > 0, k < n_steps, fast_only, row, whole ? stream : s->streams[g], g0, g1);
            if (k < n_steps && !whole) eval_likes(s, s->streams[g], g0, g1, s->ws_g[g].p);
        }
        if (k < n_steps && whole) eval_likes(s, stream, 0, s->W, s->ws.p);
    }
    for (int g = 0; g < G; g++) {
        HIP_CHECK(hipEventRecord(s->events[g], s->streams[g]));
        HIP_CHECK(hipStreamWaitEvent(stream, s->events[g], 0));
    }
}

void sampler_step(cmbs *s, int n_steps, int fast_only, hipStream_t stream) {
    if (!s->started) fail(CMBL_ERR_ARG, "cmbs_set_start must be called before cmbs_step");
    check_theory_fresh(s);
    if (fast_only && s->fast_n == 0) fail(CMBL_ERR_ARG, "no fast parameters");
    if (!fast_only && s->slow_n > 0 && s->n_rows() > 0)
        fail(CMBL_ERR_ARG, "slow proposals need the theory at the trial point: use cmbs_step_theory");
    check_derived_calc(s, "cmbs_step");
    if (n_steps <= 0) return;
    derived_rows_current(s, stream);
    sampler_check_pipe(s);
    const int G = s->n_groups;
    PlikBinArgs pb;
    if (G == 1 && unified_setup(s, fast_only)) run_unified(s, n_steps, fast_only, stream);
    else if (G == 1 && bin_setup(s, fast_only, pb)) run_bin_corun(s, n_steps, fast_only, pb, stream);
    else if (G == 1) run_plain(s, n_steps, fast_only, stream);
    else run_groups(s, n_steps, fast_only, stream);
}

#include "slowstep.h"

void sampler_set_groups(cmbs *s, int n_groups) {
    {   // the groups step together: a common known loop index carries over to the new split
        const int v = s->rot_lp.empty() ? -1 : s->rot_lp[0];
        const bool same = std::all_of(s->rot_lp.begin(), s->rot_lp.end(), [v](int x) { return x == v; });
        std::fill(s->rot_lp.begin(), s->rot_lp.end(), same ? v : -1);
    }
    const int nblk = (s->W + NB - 1) / NB;
    if (n_groups < 1 || n_groups > MAXGROUPS) fail(CMBL_ERR_ARG, "n_groups must be in 1..%d", MAXGROUPS);
    if (n_groups > nblk) n_groups = nblk;
    s->grp0.assign(n_groups + 1, 0);
    for (int g = 0; g <= n_groups; g++) s->grp0[g] = std::min(s->W, (int)((long long)nblk * g / n_groups) * NB);
    for (int g = 0; g < n_groups; g++) {
        if (!s->streams[g]) HIP_CHECK(hipStreamCreateWithFlags(&s->streams[g], hipStreamNonBlocking));
        size_t ws = 0;
        for (auto &l : s->likes) ws = std::max(ws, l.like->like->workspace_size(s->grp0[g + 1] - s->grp0[g]));
        s->ws_g[g].alloc(ws);
    }
    for (auto &e : s->events)
        if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s->n_groups = n_groups;
}

}  // namespace cmamd

#ifdef CMAMD_STAMPS
extern "C" int cmamd_debug_uni_stamps(unsigned long long *host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(cmamd::g_uni_stamps), sizeof(cmamd::g_uni_stamps)) == hipSuccess ? 0
                                                                                                               : -5;
}
extern "C" int cmamd_debug_stamps(unsigned long long *host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(cmamd::g_stamps), sizeof(cmamd::g_stamps)) == hipSuccess ? 0 : -5;
}
#endif

// number of work items of the sampler's fused window pass (0: none); for tests
// (without one: minus the last set-up check passed)
extern "C" int cmamd_debug_rot_serial(cmbs *s, int mode) {   // 1: rotations by the serial path; 2: parallel, no speculative lanes
    if (!s) return -1;
    s->dc.rot_serial = mode;
    return 0;
}
extern "C" int cmamd_debug_stage_R(cmbs *s, int on) {     // rotation rows staged in mh_kernel's LDS image
    if (!s) return -1;
    s->stage_R_force = on;   // -1: set_mh_lds decides
    cmamd::set_mh_lds(s);
    return 0;
}
extern "C" int cmamd_debug_tp_items(const cmbs *s, int *out, int cap) {   // (field, l0, l1, steps, columns, blocks) per item
    if (!s || !s->tpass) return -1;
    const int n = std::min(cap, s->tpass->n_items());
    for (int k = 0; k < n; k++) {
        const cmamd::TPItem &it = s->tpass->item(k);
        const int v[6] = {it.field, it.l0, it.l1, it.nst, it.ncol, it.nsb};
        for (int q = 0; q < 6; q++) out[6 * k + q] = v[q];
    }
    return s->tpass->n_items();
}
extern "C" int cmamd_debug_tail_rows(int nq, int ng, int np, int nm, int *out, int cap) {   // (role, row of the role) per row
    const std::vector<int2> rows = cmamd::tail_rows(nq, ng, np, nm);
    const int n = std::min(cap, (int)rows.size());
    for (int k = 0; k < n; k++) {
        out[2 * k] = rows[k].x;
        out[2 * k + 1] = rows[k].y;
    }
    return (int)rows.size();
}
extern "C" int cmamd_debug_pipeline(cmbs *s, int mode) {   // fast-step schedule (sampler_step): 0 unpipelined,
    if (!s || (mode != 0 && mode != 3)) return -1;   // 3 the unified launch (default), 0 unpipelined
    s->sched_mode = mode;
    return 0;
}
extern "C" int cmamd_debug_lean(cmbs *s, int on) {   // the lean chain where it applies (1, default) or mh_body (0)
    if (!s) return CMBL_ERR_ARG;
    s->lean_off = !on;
    return 0;
}
extern "C" int cmamd_debug_corun(cmbs *s, int on) {     // the lensing chi^2 inside plik's quadratic-form launch
    if (!s) return -1;
    s->no_corun = !on;
    return 0;
}
extern "C" int cmamd_debug_tail_nosignal(cmbs *s, int on) {   // in-launch producers never arrive / publish
    if (!s) return -1;
    s->handoff_nosignal = on;
    return 0;
}
extern "C" int cmamd_debug_drag_pair(cmbs *s, int on) {   // both drag evaluation sets in two launches
    if (!s) return -1;
    s->no_drag_pair = on == 0;
    return 0;
}
extern "C" int cmamd_debug_drag_hbm(cmbs *s, int on) {   // the drag stages on the HBM state (no LDS image)
    if (!s) return -1;
    s->drag_hbm = on != 0;
    return 0;
}
extern "C" int cmamd_debug_pipe_status(cmbs *s) {   // the give-up word (synchronises the device)
    if (!s || !s->pipe_status.host) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return *reinterpret_cast<volatile int *>(s->pipe_status.host);
}
extern "C" int cmamd_debug_tail(const cmbs *s) { return s ? s->unified.ready : 0; }   // W of the step tails' set-up
extern "C" int cmamd_debug_fused(const cmbs *s) { return !s ? 0 : s->tpass ? s->tpass->n_items() : -s->tp_why; }
