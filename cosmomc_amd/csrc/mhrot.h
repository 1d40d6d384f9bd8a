// rot_kernel: the rotations of wide blocks, deferred from the chain lane.
// Included by sampler.hip after mhpropose.h.
// (included inside namespace cmamd)
#pragma once

// ------------------------------------------------------- deferred rotations
// A new random rotation of a block of ROT_DEFER_MIN or more parameters
// (RotMatrix propose.f90:88-102 -> RandRotationD RandUtils.f90:133-153) is too
// big for the chain lane: mh_kernel stops that walker's proposal at the
// rotation (Rows::PROT), appends the walker to the step's rotation list, and
// rot_kernel, one wave per listed walker, finishes it.
//
// The Gaussians.  RANMAR's lagged-Fibonacci part is x_m = x_{m-97} - x_{m-33}
// mod 1 (RandUtils.f90:350-374), an integer recurrence mod 2^24 in units of
// 2^-24, and its carry c_m = c - (m+1) cd mod cm has a closed form, so the 64
// lanes make 64 uniforms per round (lanes 33..63 substitute x_{m-33} =
// x_{m-130} - x_{m-66}).  The lanes then take Gaussian1's polar pairs
// (uniforms 2p, 2p+1, RandUtils.f90:156-178) 32 at a time, and the accepted
// pairs are placed by a ballot prefix in stream order (v2 fac, then the saved
// deviate v1 fac).  Nothing is committed until the rotation is done; then the
// state advances by exactly the uniforms the consumed Gaussians used (ring,
// i97/j97, c, iset, gset): bit-identical to drawing them one at a time.
//
// Gram-Schmidt.  Lane j owns row j's vec in registers.  Row i is final once
// its projections on rows 0..i-1 are done, so the rows advance in lockstep:
// at iteration i lane i takes its norm (below 1e-3 row i is redrawn and the
// later rows restart on the shifted Gaussians) and publishes R(i,:) in LDS,
// then every lane j > i projects onto it.  Every sum runs over q in order, as
// the reference's sum() and rot_matrix do, so R is bit-identical.  A rotation
// whose Gaussians would overflow the LDS buffers (many redraws) is redone by
// the serial path (lane 0 draws, the lanes project with readlane sums), which
// is also the debug reference (DevCfg::rot_serial).

// sum of x over lanes 0..n-1 in lane order, formed identically on every lane
// from v_readlane broadcasts (no LDS round trip, no divergent lane-0 section)
__device__ __forceinline__ double lane_sum_ordered(double x, int n)
{
    const long long bits = __double_as_longlong(x);
    const int lo = (int)bits, hi = (int)(bits >> 32);
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < MAXBLK; q++)
        if (q < n) {
            const unsigned l = (unsigned)__builtin_amdgcn_readlane(lo, q);
            const long long h = __builtin_amdgcn_readlane(hi, q);
            s += __longlong_as_double((h << 32) | l);
        }
    return s;
}

__device__ __forceinline__ double readlane_f64(double x, int q)
{
    const long long bits = __double_as_longlong(x);
    const unsigned l = (unsigned)__builtin_amdgcn_readlane((int)bits, q);
    const long long h = __builtin_amdgcn_readlane((int)(bits >> 32), q);
    return __longlong_as_double((h << 32) | l);
}

// LDS written by some lanes of a wave and read by others (the wave's LDS
// operations complete in order; this keeps the compiler from moving them)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

static constexpr int ROT_WAVES = 4;                        // walkers per rot_kernel workgroup (a wave each)
static constexpr int ROT_GC = MAXBLK * (MAXBLK + 4);       // Gaussians a parallel rotation may use (>= n (n + ROT_SPEC))
static constexpr int ROT_GA = ROT_GC + 128;                // + one pair round's overshoot
static constexpr int ROT_UC = 1536;                        // uniforms (a multiple of 64)

struct RotLds {
    double g[ROT_GA];             // the Gaussian stream from the rotation's start (g[0] = gset if iset)
    double rm[MAXBLK * MAXBLK];   // R(i, q) at rm[i * MAXBLK + q]
    double u[98];                 // RANMAR u(1:97) as doubles (the state rows' form)
    double gs[MAXBLK];            // serial path: one attempt's Gaussians
    int x[ROT_UC];                // lagged-Fibonacci values x_m (units of 2^-24)
    int o[ROT_UC];                // uniforms x_m - c_m (units of 2^-24)
    int pi[ROT_GA / 2];           // pair index of the r-th accepted pair
    int ui[100];                  // u(1:97) in units of 2^-24
};

struct RotGen {
    int i97, j97, C0;             // RANMAR pointers and carry (units of 2^-24) at the start
    int off;                      // 1 when the start state holds a saved deviate (iset)
    int m = 0, p = 0, nr = 0;     // uniforms made, pairs taken, pairs accepted
    int cbase;                    // carry before this round's first call: C0 - m cd mod cm
    int ck;                       // this lane's (lane + 1) cd mod cm
};

__device__ __forceinline__ int mod97(int v) { return v >= 97 ? v - 97 : v; }   // v in [0, 194)

__device__ __forceinline__ int rot_x(const RotLds &L, const RotGen &G, int p)
{   // x_p; p in [-97, -1] is the start ring: u(i97 - 1 - p mod 97)
    return p >= 0 ? L.x[p] : L.ui[mod97(G.i97 - 1 - p)];
}

__device__ __forceinline__ int sub24(int a, int b) { const int d = a - b; return d < 0 ? d + (1 << 24) : d; }

static constexpr int RM_P = 16777213, RM_CD = 7654321;     // cm and cd in units of 2^-24

__device__ void rot_uniforms(RotLds &L, RotGen &G, int lane)
{   // 64 uniforms
    const int m = G.m + lane;
    const int b = lane < 33 ? rot_x(L, G, m - 33) : sub24(rot_x(L, G, m - 130), rot_x(L, G, m - 66));
    const int x = sub24(rot_x(L, G, m - 97), b);
    int cm = G.cbase - G.ck;                 // c after call m: C0 - (m + 1) cd mod cm
    if (cm < 0) cm += RM_P;
    L.x[m] = x;
    L.o[m] = sub24(x, cm);
    G.m += 64;
    G.cbase -= (64 * RM_CD) % RM_P;
    if (G.cbase < 0) G.cbase += RM_P;
    wave_sync();
}

__device__ void rot_pairs(RotLds &L, RotGen &G, int lane)
{   // up to 64 polar pairs of the uniforms made so far
    const int p = G.p + lane;
    bool acc = false;
    double v1 = 0.0, v2 = 0.0, rr = 0.0;
    if (2 * p < G.m) {
        v1 = 2.0 * ((double)L.o[2 * p] * (1.0 / 16777216.0)) - 1.0;
        v2 = 2.0 * ((double)L.o[2 * p + 1] * (1.0 / 16777216.0)) - 1.0;
        rr = v1 * v1 + v2 * v2;
        acc = rr < 1.0;
    }
    const unsigned long long mask = __ballot(acc);
    if (acc) {
        const int r = G.nr + __popcll(mask & ((1ull << lane) - 1ull));
        const double fac = sqrt(-2.0 * log(rr) / rr);
        L.g[G.off + 2 * r] = v2 * fac;
        L.g[G.off + 2 * r + 1] = v1 * fac;
        L.pi[r] = p;
    }
    G.nr += __popcll(mask);
    G.p = min(G.p + 64, G.m / 2);
    wave_sync();
}

// Gaussians g[0, need): the uniforms for about 1.3 pairs per missing
// accepted pair go first (their rounds are short), then the pairs 64 at a time
__device__ __forceinline__ bool rot_fill(RotLds &L, RotGen &G, int need, int lane)
{
    if (need > ROT_GC) return false;
    while (G.off + 2 * G.nr < need) {
        const int short_pairs = (need - G.off - 2 * G.nr + 1) / 2;
        int want = 2 * (G.p + short_pairs + short_pairs / 3 + 8);
        want = min(ROT_UC, (want + 63) & ~63);
        if (want <= G.m) {
            if (2 * G.p < G.m) want = G.m;        // pairs left to take
            else if (G.m + 64 <= ROT_UC) want = G.m + 64;
            else return false;                    // the uniform buffer is spent
        }
        while (G.m < want) rot_uniforms(L, G, lane);
        while (2 * G.p < G.m && G.off + 2 * G.nr < need) rot_pairs(L, G, lane);
    }
    return true;
}

// advance the RANMAR / Gaussian1 state past the first T Gaussians of the stream
__device__ void rot_commit(RotLds &L, const RotGen &G, int T, Rng &r, int lane)
{
    const int t = T - G.off;
    int K = 0;
    if (t > 0) {
        const int q = (t - 1) / 2;            // the pair that gave the last Gaussian
        K = 2 * (L.pi[q] + 1);
        r.iset = t & 1;
        r.gset = L.g[G.off + 2 * q + 1];
    } else {
        r.iset = 0;
    }
    for (int s = lane; s < 97; s += 64) {    // ring slot s (u(s+1)) last written by call m = i97-1-s mod 97 (+97k)
        const int r0 = mod97(G.i97 - 1 - s + 97);
        if (K - 1 >= r0) L.ui[s] = L.x[r0 + 97 * ((K - 1 - r0) / 97)];
        L.u[s] = (double)L.ui[s] * (1.0 / 16777216.0);
    }
    r.i97 = (G.i97 - 1 - K % 97 + 97) % 97 + 1;
    r.j97 = (G.j97 - 1 - K % 97 + 97) % 97 + 1;
    int cm = G.C0 - (int)((long long)K * RM_CD % RM_P);
    if (cm < 0) cm += RM_P;
    r.c = (double)cm * (1.0 / 16777216.0);
    wave_sync();
}

#ifdef CMAMD_STAMPS
__device__ unsigned long long g_rot_ticks[3];     // first listed walker: total, Gaussian draws, Gram-Schmidt
#define RTICK(v) (v) = __builtin_amdgcn_s_memtime()
#else
#define RTICK(v) ((void)0)
#endif

static constexpr int ROT_SPEC = 2;   // idle lanes n, n+1 carry the last row's next two attempts

// One lockstep Gram-Schmidt pass over rows start..n-1 (row j from the n
// Gaussians at g[gbase + (j - start) n]); NQ = n rounded up to 8.  The
// padding columns q in [n, NQ) hold +0.0 in vec and in R, so every product
// there is +0.0 and the sums (which start at +0.0) are bit-identical to sums
// over q < n, with no selects.  Lane i publishes its raw vec and the lanes
// divide one element each.  A redraw is most likely for the last row (its
// residual has one degree of freedom: P(norm <= 1e-3) = 2.5 %), so lanes n and
// n+1 project the Gaussians that follow as that row's second and third
// attempts and stand in when it fails.  Returns -1 and the last row's extra
// attempts in *extra, or the row to redraw and its failed attempts in *extra.
template <int NQ>
__device__ int rot_gs_pass(RotLds &L, int n, int start, int gbase, int lane, int spec, int *extra)
{
    const int top = n + spec;
    double v[NQ], pp[NQ];
    if (lane >= start && lane < top) {
        const double *gv = L.g + gbase + (lane - start) * n;   // within g: the fill covered (top - start) n
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const double x = gv[q];
            v[q] = q < n ? x : 0.0;
        }
    }
    for (int i = 0; i < n; i++) {
        if (i >= start) {
            const bool last = i == n - 1;
            double norm = 0.0;
            if (lane == i || (last && lane >= n && lane < top)) {
#pragma unroll
                for (int q = 0; q < NQ; q++) pp[q] = v[q] * v[q];
#pragma unroll
                for (int q = 0; q < NQ; q++) norm += pp[q];
            }
            int src = i, a = 0;
            double nv = readlane_f64(norm, i);
            if (!(nv > 1e-3)) {               // RandRotationD :143: draw row i again
                if (!last) {
                    *extra = 1;
                    return i;
                }
                for (a = 1; a <= spec; a++) {
                    nv = readlane_f64(norm, n - 1 + a);
                    if (nv > 1e-3) break;
                }
                if (a > spec) {
                    *extra = 1 + spec;
                    return i;
                }
                src = n - 1 + a;
            }
            *extra = a;
            double *ri = L.rm + i * MAXBLK;
            if (lane == src)
#pragma unroll
                for (int q = 0; q < NQ; q += 2) *reinterpret_cast<double2 *>(ri + q) = make_double2(v[q], v[q + 1]);
            wave_sync();
            if (lane < NQ) {                  // R(i, q) = vec(q) / sqrt(norm), lane q
                const double x = ri[lane];
                ri[lane] = lane < n ? x / sqrt(nv) : 0.0;
            }
            wave_sync();
        }
        if (i < n - 1 && lane > i && lane < top) {   // vec = vec - sum(vec*R(i,:))*R(i,:)
            const double *ri = L.rm + i * MAXBLK;
            double rv[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q += 2) {
                const double2 t = *reinterpret_cast<const double2 *>(ri + q);
                rv[q] = t.x;
                rv[q + 1] = t.y;
            }
#pragma unroll
            for (int q = 0; q < NQ; q++) pp[q] = v[q] * rv[q];
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < NQ; q++) s += pp[q];
#pragma unroll
            for (int q = 0; q < NQ; q++) pp[q] = s * rv[q];
#pragma unroll
            for (int q = 0; q < NQ; q++) v[q] = v[q] - pp[q];
        }
    }
    return -1;
}

// the parallel rotation into L.rm; false (state untouched) when the buffers overflow
__device__ bool rot_parallel(RotLds &L, Rng &r, int n, int lane, int spec, unsigned long long *tk)
{
    RotGen G;
    G.i97 = r.i97;
    G.j97 = r.j97;
    G.C0 = (int)(r.c * 16777216.0);
    G.off = r.iset ? 1 : 0;
    G.cbase = G.C0;
    G.ck = (lane + 1) * RM_CD % RM_P;                      // < 64 cd < 2^31
    if ((G.i97 - G.j97 + 97) % 97 != 64) return false;     // not RMARIN's pointer pair: serial path
    for (int s = lane; s < 97; s += 64) L.ui[s] = (int)(L.u[s] * 16777216.0);
    if (lane == 0 && G.off) L.g[0] = r.gset;
    wave_sync();
    int start = 0, gbase = 0;
    (void)tk;
    for (;;) {                                // one pass per redraw
#ifdef CMAMD_STAMPS
        unsigned long long t0, t1;
        RTICK(t0);
#endif
        if (!rot_fill(L, G, gbase + (n - start + spec) * n, lane)) return false;
#ifdef CMAMD_STAMPS
        RTICK(t1);
        tk[1] += t1 - t0;
#endif
        int extra = 0;
        const int fail = n <= 8    ? rot_gs_pass<8>(L, n, start, gbase, lane, spec, &extra)
                         : n <= 16 ? rot_gs_pass<16>(L, n, start, gbase, lane, spec, &extra)
                         : n <= 24 ? rot_gs_pass<24>(L, n, start, gbase, lane, spec, &extra)
                                   : rot_gs_pass<32>(L, n, start, gbase, lane, spec, &extra);
        static_assert(MAXBLK == 32, "rot_gs_pass widths");
#ifdef CMAMD_STAMPS
        RTICK(t0);
        tk[2] += t0 - t1;
#endif
        if (fail < 0) {
            rot_commit(L, G, gbase + (n - start + extra) * n, r, lane);
            return true;
        }
        gbase += (fail - start + extra) * n;
        start = fail;
    }
}

// the serial rotation into L.rm: lane 0 draws each attempt's Gaussians, lane q
// holds column q of R, every sum is formed in q order from readlane broadcasts
__device__ void rot_serial(RotLds &L, Rng &r, int n, int lane)
{
    double rcol[MAXBLK];
#pragma unroll
    for (int i = 0; i < MAXBLK; i++) rcol[i] = 0.0;
    for (int j = 0; j < n; j++) {
        double v, norm;
        for (;;) {
            if (lane == 0)
                for (int q = 0; q < n; q++) L.gs[q] = gaussian1(r);
            wave_sync();
            v = lane < n ? L.gs[lane] : 0.0;
#pragma unroll
            for (int i = 0; i < MAXBLK; i++) {
                if (i < j) {
                    const double s = lane_sum_ordered(v * rcol[i], n);
                    v = v - s * rcol[i];
                }
            }
            norm = lane_sum_ordered(v * v, n);
            wave_sync();
            if (norm > 1e-3) break;
        }
        const double rv = v / sqrt(norm);
#pragma unroll
        for (int i = 0; i < MAXBLK; i++)
            if (i == j) rcol[i] = rv;
        if (lane < n) L.rm[j * MAXBLK + lane] = rv;
    }
    // lane 0's RNG state is the walker's: broadcast it
    r.c = readlane_f64(r.c, 0);
    r.gset = readlane_f64(r.gset, 0);
    r.i97 = __builtin_amdgcn_readlane(r.i97, 0);
    r.j97 = __builtin_amdgcn_readlane(r.j97, 0);
    r.iset = __builtin_amdgcn_readlane(r.iset, 0);
    wave_sync();
}

// One wave: walker w's pending rotation, then the rest of its proposal.
__device__ void rot_walker(const DevCfg &c, int w, int lane, RotLds &L, bool stamp)
{
    const size_t ld = c.ld;
    const Rows &R = c.rows;
    const int b = c.si[(size_t)R.PROT * ld + w] - 1;
    const Tabs t = make_tabs(c, c.tab_i, c.tab_d, c.tab_d);
    const int n = t.blk_n[b], off = t.blk_R_off[b];
    for (int i = lane; i < 97; i += 64) L.u[i] = c.sd[(size_t)(R.U + i) * ld + w];
    Walker k;
    k.r.u = Col<double>{L.u, 1};
    k.r.c = c.sd[(size_t)R.C * ld + w];
    k.r.gset = c.sd[(size_t)R.G * ld + w];
    k.r.i97 = c.si[(size_t)R.I97 * ld + w];
    k.r.j97 = c.si[(size_t)R.J97 * ld + w];
    k.r.iset = c.si[(size_t)R.ISET * ld + w];
    wave_sync();
    unsigned long long tk[3] = {0, 0, 0};
#ifdef CMAMD_STAMPS
    RTICK(tk[0]);
#endif
    if (c.rot_serial == 1 || !rot_parallel(L, k.r, n, lane, c.rot_serial == 2 ? 0 : ROT_SPEC, tk))
        rot_serial(L, k.r, n, lane);
#ifdef CMAMD_STAMPS
    if (stamp && lane == 0) {
        g_rot_ticks[0] = __builtin_amdgcn_s_memtime() - tk[0];
        g_rot_ticks[1] = tk[1];
        g_rot_ticks[2] = tk[2];
    }
#else
    (void)stamp;
#endif
    // R(i, q) (rm, row stride MAXBLK) -> the state rows and a packed copy (row stride n) in g
    for (int e = lane; e < n * n; e += 64) {
        const double x = L.rm[(e / n) * MAXBLK + e % n];
        c.sd[(size_t)(R.R + off + e) * ld + w] = x;
        L.g[e] = x;
    }
    wave_sync();
    k.trial = Col<double>{c.sd + (size_t)R.T * ld + w, (int)ld};
    k.P = Col<double>{c.sd + (size_t)R.P * ld + w, (int)ld};
    if (lane == 0) {   // the rest of ProposeVec on column 1 of the packed copy of R, up to UpdateParams
        k.R = Col<double>{L.g - off, 1};
        k.vec = Col<double>{L.gs, 1};
        k.blklp = Col<int>{c.si + (size_t)R.BLKLP * ld + w, (int)ld};
        k.defer = 1;
        proposal_tail(c, t, k, b, 0);
    }
    wave_sync();
    {   // UpdateParams (propose.f90:142-149): one lane per changed parameter, each sum in q order
        const int nc = t.blk_nchanged[b];
        const double *M = t.mapping + t.blk_map_off[b];
        const int *chg = t.changed + t.blk_changed_off[b];
        for (int j = lane; j < nc; j += 64) {
            double s = 0.0;
            for (int q = 0; q < n; q++) s += M[j * n + q] * L.gs[q];
            k.trial[chg[j]] += s;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the trial row's stores, before lane 0 reads it
    __builtin_amdgcn_wave_barrier();
    double calr = 0.0;   // bin co-run: plik's trial calibration
    if (lane == 0) {
        for (int l = 0; l < c.n_like; l++)
            for (int q = 0; q < c.like_nn[l]; q++)
                c.like_nuis[l][(size_t)w * c.like_nn[l] + q] = k.trial[t.ti[c.like_nidx[l] + q]];
        if (c.bin_on) calr = k.trial[t.ti[c.like_nidx[0] + c.bin_cal]];
        if (c.mask_on) write_like_flags(c, k.trial, k.P, w);
        c.sd[(size_t)R.C * ld + w] = k.r.c;
        c.sd[(size_t)R.G * ld + w] = k.r.gset;
        c.si[(size_t)R.I97 * ld + w] = k.r.i97;
        c.si[(size_t)R.J97 * ld + w] = k.r.j97;
        c.si[(size_t)R.ISET * ld + w] = k.r.iset;
        c.si[(size_t)R.PROT * ld + w] = 0;
    }
    wave_sync();
    for (int i = lane; i < 97; i += 64) c.sd[(size_t)(R.U + i) * ld + w] = L.u[i];
    if (c.bin_on) {   // the walker's Delta rows from the bin co-run's raw sums (plik_bin_emit's operations)
        const double cl = __shfl(calr, 0), c2 = cl * cl;
        const size_t r = (size_t)w * c.bin_Np;
#pragma unroll 4
        for (int i = lane; i < c.bin_nused; i += 64) c.bin_delta[r + i] = c.bin_X[i] - c.bin_S[r + i] / c2;
    }
}

// One wave per listed walker (the launch's list counter is wave-uniform).
__global__ __launch_bounds__(64 * ROT_WAVES) void rot_kernel(DevCfg c, int g0)
{
    extern __shared__ __attribute__((aligned(16))) double rot_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = blockIdx.x * ROT_WAVES + wave;
    if (idx >= c.rot_cnt[2 * (g0 / 64) + c.rot_par]) return;
    rot_walker(c, c.rot_list[g0 + idx], lane, reinterpret_cast<RotLds *>(rot_lds)[wave], idx == 0);
}

#ifdef CMAMD_STAMPS
extern "C" int cmamd_debug_rot_ticks(unsigned long long *host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_rot_ticks), sizeof(g_rot_ticks)) == hipSuccess ? 0 : -5;
}
#endif
