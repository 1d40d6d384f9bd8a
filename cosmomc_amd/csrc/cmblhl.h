// CMBlikes HL transform (CMBLikes_Transform) per (walker, bin).
// (included by cmblikes.hip inside namespace cmamd)
#pragma once

// ------------------------------------------- HL, register-resident (M lanes / matrix)
// The two symmetric eigensolves and HL transform of CMBLikes_Transform
// (:861-914) by one-sided cyclic Jacobi (hl_ojacobi), with the matrices in
// registers: lane r of an M-lane group owns column r of the working matrix
// and of the eigenvector matrix, and a 64-lane block packs 64/M (walker, bin)
// problems.  The matrix products go through per-group LDS row buffers.
#ifdef CMAMD_STAMPS
__device__ unsigned int g_hl_sweeps[2][64];      // waves per sweep count, first / second eigensolve (tools/hl_stamps.py)
// s_memtime ticks per Jacobi round phase, summed over the rounds of lane 0 of
// every wave: [0] column write + barrier, [1] partner read, dot product and
// angle, [2] rotation + barrier, [3] rounds
__device__ unsigned long long g_hl_phase[4];
// s_memtime ticks per kernel phase, summed over lane 0 of every wave (tools/hl_stamps.py)
__device__ unsigned long long g_hl_tp[12];
#define HL_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define HL_STAMP(v) ((void)0)
#endif

// one problem's buffers; per-problem strides of 2 mod 32 LDS dwords put the
// groups' broadcast reads of one element on distinct bank pairs (at 16 mod 32,
// BK15's M = 12, groups 0, 2 and 4 shared a pair: 3-way conflicts)
template <int M>
struct HLGrpLds {
    static constexpr int SZ = 2 * M * (M + 1) + 2 * M;          // doubles before the pad
    double rows[2][M][M + 1];       // two row buffers (odd stride: fewer bank conflicts within a problem);
                                    // in the Jacobi, buffer 1 holds each row as of the round start
    double dg[M];                   // a diagonal / g(x) broadcast
    double isd[M];                  // 1 / sqrt of the first eigensolve's eigenvalues
    double pad[((1 - SZ) % 16 + 16) % 16 + 1];
};

template <int M>
struct HLRowsLds {
    static constexpr int G = 64 / M;   // problems per wave: M lanes each, packed (5 for M = 12)
    HLGrpLds<M> g[G];
};

template <int M>
__device__ inline int hl_partner(int rr, int r) {   // round-robin pairing of round rr (circle method)
    if (r == M - 1) return rr;
    if (r == rr) return M - 1;
    return ((2 * rr - r) % (M - 1) + (M - 1)) % (M - 1);
}

static constexpr int HL_MAX_SWEEPS = 40;   // as DSYEV's own iteration limit, a cap that fails loudly
// a sweep in which no pair of a problem was further from orthogonal than
// cos = 1e-6 is that problem's last (its own rotations leave every pair near
// cos 1e-12: -lnL within 2.4e-14 relative of the reference's DSYEV on the BK
// goldens, tools/hl_margin.py).  With the stop per problem a looser one buys
// little, since a wave runs until its slowest problem stops: BK15 at W = 1024
// HL 173.7 / 170.9 / 167.5 us at cos 1e-6 / 1e-5 / 1e-4, golden margins
// 2.4e-14 / 2.3e-12 / 2.1e-10, and cos 1e-4 fails the 9-map width test's
// rtol 1e-9 (round 5, profiles/r05_hl_stop.txt)
static constexpr double HL_SWEEP_COS2 = 1e-12;

// One-sided (Hestenes) cyclic Jacobi of the group's symmetric M x M matrix C:
// lane r owns column r of G = C V (initially C's column r, i.e. its row r; V,
// initially the identity, is not carried: see below).  A round pairs lanes (lo, hi) by the
// round-robin circle schedule; both lanes of a pair read the other's columns
// from LDS, form a_ll = g_l.g_l, a_hh = g_h.g_h, a_lh = g_l.g_h (the same sums
// in the same order, so both derive the same rotation) and rotate their own
// columns: g_l' = c g_l - s g_h, g_h' = s g_l + c g_h, with tan of the angle
// the smaller root of t^2 + 2 zeta t - 1 = 0, zeta = (a_hh - a_ll) / (2 a_lh).
// At convergence V holds orthonormal eigenvectors in its columns (returned in
// V, with lam eigenvalue r, signed).  One column exchange
// per round (two barriers) replaces the two-sided form's row exchange plus
// broadcast of every column's rotation (three barriers, about twice the LDS
// traffic); the column norms are carried across rounds, so a round forms one
// dot product, and the arithmetic is fused multiply-adds (the eigensolver is
// not the reference's DSYEV, so no operation order is there to follow).  Pairs
// with |a_lh| > 1e-15 sqrt(a_ll a_hh) are rotated; a sweep in which no pair of
// a problem had |a_lh| > 1e-6 sqrt(a_ll a_hh) (HL_SWEEP_COS2 = 1e-12 on the
// squares) ends that problem's solve (its own rotations, by the quadratic
// convergence of cyclic Jacobi, leave every pair near 1e-12: no separate check
// sweep).  The stop is per problem: a problem whose sweep met it rotates no
// more while the other problems of its wave go on, so its result depends on
// its own matrix only, not on which walkers share its wave.
// Returns true on lanes whose pair still needed rotating in sweep
// HL_MAX_SWEEPS (the caller fails that problem: NaN and a status bit).
// The matrices here are symmetric positive definite (C, and
// C^-1/2 Chat C^-1/2), so G = C V = U Sigma with U = V: eigenvalue r is the
// norm of column r and eigenvector r that column normalised, and V is formed
// at the end instead of being carried -- each round exchanges and rotates one
// column instead of two (the exchange is the round's cost: lane permutes
// through the LDS crossbar).
template <int M>
__device__ bool hl_ojacobi(double (&G)[M], double (&V)[M], HLRowsLds<M> &S, int grp, int r, int lane, int which,
                           double &lam)
{
    (void)which;
    (void)lane;
    const bool on = grp < HLRowsLds<M>::G;        // lanes past G*M idle
    // the input matrix (row r = column r), for the eigenvalues' signs after the solve
    if (on)
#pragma unroll
        for (int k = 0; k < M; k++) S.g[grp].rows[0][r][k] = G[k];
    __syncthreads();
    bool failed = false;
    bool done = !on;                              // this lane's problem has met the sweep stop
    const unsigned long long gmask = (M == 64 ? ~0ull : ((1ull << M) - 1)) << ((on ? grp : 0) * M);
#ifdef CMAMD_STAMPS
    unsigned long long ph0 = 0, ph1 = 0, ph2 = 0, nround = 0;
#endif
    for (int sweep = 0;; sweep++) {
        bool big = false;
        // the column's squared norm, recomputed every sweep and updated exactly
        // as Rutishauser's a_ll' = a_ll - t a_lh, a_hh' = a_hh + t a_lh in between
        double nrm = 0.0;
#pragma unroll
        for (int k = 0; k < M; k++) nrm = fma(G[k], G[k], nrm);
#pragma unroll 1
        for (int rr = 0; rr < M - 1; rr++) {
            const int p = on ? hl_partner<M>(rr, r) : r;
            HL_STAMP(t0);
            // the partner's column and norm by lane permutes (ds_bpermute: no LDS
            // banks, no barrier; the same values the row buffers carried)
            const int src = on ? grp * M + p : lane;
            HL_STAMP(t1);
#ifdef CMAMD_STAMPS
            unsigned long long t2 = 0;
#endif
            double Gp[M];
#pragma unroll
            for (int k = 0; k < M; k++) Gp[k] = __shfl(G[k], src);   // every permute in flight together
            const double np_ = __shfl(nrm, src);
            if (!done) {
                const bool low = r < p;
                const double all = low ? nrm : np_, ahh = low ? np_ : nrm;
                double alh = 0.0;
#pragma unroll
                for (int k = 0; k < M; k++) alh = fma(low ? G[k] : Gp[k], low ? Gp[k] : G[k], alh);
                if (alh != 0.0 && alh * alh > 1e-30 * (all * ahh)) {
                    // cos^2 > HL_SWEEP_COS2: columns this far from orthogonal need another
                    // sweep; below it this sweep's rotation leaves them near cos^2 squared
                    big = big || alh * alh > HL_SWEEP_COS2 * (all * ahh);
                    const double d = ahh - all, e = 2.0 * alh;
                    // the hardware square root (not correctly rounded): den only sets the
                    // angle, and c, s stay orthonormal to rounding whatever t is
                    const double den = fabs(d) + __builtin_amdgcn_sqrt(d * d + e * e);
                    const double q = __builtin_amdgcn_rcp(den);     // the hardware reciprocal: likewise
                    const double t = ((d >= 0) == (e >= 0) ? fabs(e) : -fabs(e)) * q;
                    const double c = rsqrt(t * t + 1.0), s = t * c;
#ifdef CMAMD_STAMPS
                    t2 = __builtin_amdgcn_s_memtime();
#endif
                    if (low) {
#pragma unroll
                        for (int k = 0; k < M; k++) G[k] = fma(-s, Gp[k], c * G[k]);
                        nrm = fma(-t, alh, all);
                    } else {
#pragma unroll
                        for (int k = 0; k < M; k++) G[k] = fma(s, Gp[k], c * G[k]);
                        nrm = fma(t, alh, ahh);
                    }
                }
            }
#ifdef CMAMD_STAMPS
            {
                const unsigned long long t3 = __builtin_amdgcn_s_memtime();
                const unsigned long long t2w = __shfl(t2, 0) ? __shfl(t2, 0) : t3;
                ph0 += t1 - t0;
                ph1 += t2w - t1;
                ph2 += t3 - t2w;
                nround++;
            }
#endif
        }
#ifdef CMAMD_STAMPS
        if (!__any(big) || sweep == HL_MAX_SWEEPS)
            if (lane == 0) atomicAdd(&g_hl_sweeps[which][sweep < 63 ? sweep : 63], 1u);
#endif
        // per problem: a sweep with no big pair is its last (wave-uniform exit once
        // every problem of the wave is done)
        const unsigned long long bal = __ballot(big);
        if (!(bal & gmask)) done = true;
        if (!bal) break;
        if (sweep == HL_MAX_SWEEPS) {
            failed = big;
            break;
        }
    }
#ifdef CMAMD_STAMPS
    if (lane == 0) {
        atomicAdd(&g_hl_phase[0], ph0);
        atomicAdd(&g_hl_phase[1], ph1);
        atomicAdd(&g_hl_phase[2], ph2);
        atomicAdd(&g_hl_phase[3], nround);
    }
#endif
    double n2 = 0.0;
#pragma unroll
    for (int k = 0; k < M; k++) n2 = fma(G[k], G[k], n2);
    const double sg = sqrt(n2), rsg = 1.0 / sg;
#pragma unroll
    for (int k = 0; k < M; k++) V[k] = n2 > 0.0 ? div_rn(G[k], sg, rsg) : (k == r ? 1.0 : 0.0);   // G[k] / sg
    // |g_r| is |lambda_r| and g_r / |g_r| is sign(lambda_r) u_r, so the norm alone
    // loses the sign of an eigenvalue of a matrix that is not positive definite
    // (a trial theory C can be): lambda_r = (A v)_i / v_i at the largest |v_i|,
    // so a negative eigenvalue stays negative and its sqrt / log give NaN, as the
    // reference's DSYEV eigenvalues do (CMBlikes.f90:877-894)
    int im = 0;
    double vm = V[0];
#pragma unroll
    for (int k = 1; k < M; k++)
        if (fabs(V[k]) > fabs(vm)) {
            im = k;
            vm = V[k];
        }
    double d = 0.0;
    if (on)
#pragma unroll
        for (int k = 0; k < M; k++) d = fma(S.g[grp].rows[0][im][k], V[k], d);
    __syncthreads();   // the callers reuse the row buffers
    lam = (d * vm < 0.0) ? -sg : sg;
    return failed;
}

template <int M>
__global__ __launch_bounds__(64, (M <= 12 ? 2 : 1)) void cmbl_hl_rows_kernel(HLDev h, const double *__restrict__ cmat,
                                                         double *__restrict__ xrows, int W)
{
    __shared__ HLRowsLds<M> S;
    constexpr int G = HLRowsLds<M>::G;
    const int lane = threadIdx.x, grp = lane / M, r = lane % M;
    const bool on = grp < G;                      // lanes past G*M idle
    const int prob = blockIdx.x * G + grp;
    const int nprob = live_walkers(h.wcount, W) * h.nb;
    if (blockIdx.x * G >= nprob) return;          // block-uniform: no live problem
    const bool live = on && prob < nprob;
    const int w = live ? prob / h.nb : 0, b = live ? prob % h.nb : 0;
    const int n = h.n;
    const bool row_ok = on && r < n;
    auto U_row = [&](int k, int j) { return S.g[grp].rows[0][k][j]; };
    // C row r from its lower-triangle elements (ElementsToMatrix :950-965), zero padded to M
    HL_STAMP(q0);
    double A[M], V[M];
    const double *cm = cmat + ((long long)w * h.nb + b) * h.ncl;
#pragma unroll
    for (int j = 0; j < M; j++) {
        double v = 0.0;
        if (live && row_ok && j < n) {
            const int a = r > j ? r : j, bb = r > j ? j : r;
            v = cm[a * (a + 1) / 2 + bb];
        }
        A[j] = v;
    }
    // Warm start: the solve runs on B0^T A B0, with B0 the eigenvectors of
    // the fiducial's matrix (host, per bin), which is nearly diagonal for
    // walkers near the fiducial, and maps its eigenvectors back (V <- B0 V).
    // Lane r holds row r of A (= column r); B0 rows go to row buffer 1.
    auto to_basis = [&](const double *B0) {
        if (on)
#pragma unroll
            for (int k = 0; k < M; k++) S.g[grp].rows[1][r][k] = (row_ok && k < n) ? B0[r * n + k] : (k == r ? 1.0 : 0.0);
        __syncthreads();
        double T[M];
#pragma unroll
        for (int j = 0; j < M; j++) {             // T = A B0, row r
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < M; k++) s += A[k] * S.g[grp].rows[1][k][j];
            T[j] = s;
        }
        if (on)
#pragma unroll
            for (int k = 0; k < M; k++) S.g[grp].rows[0][r][k] = T[k];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < M; j++) {             // B0^T T, row r
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < M; k++) s += S.g[grp].rows[1][k][r] * S.g[grp].rows[0][k][j];
            A[j] = s;
        }
        __syncthreads();
    };
    auto from_basis = [&]() {                     // V <- B0 V (column r), B0 still in row buffer 1
        double U[M];
#pragma unroll
        for (int i = 0; i < M; i++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < M; k++) s += S.g[grp].rows[1][i][k] * V[k];
            U[i] = s;
        }
#pragma unroll
        for (int i = 0; i < M; i++) V[i] = U[i];
        __syncthreads();
    };
    // (1) C = U diag U^T (lane r: eigenvector r, i.e. column r of U)
    double dgr;
#ifdef CMAMD_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    HL_STAMP(q1);
    if (h.u0) to_basis(h.u0 + (long long)b * n * n);
    HL_STAMP(q2);
    bool unconverged = hl_ojacobi<M>(A, V, S, grp, r, lane, 0, dgr);
    HL_STAMP(q3);
    if (h.u0) from_basis();
    if (on) {
        S.g[grp].dg[r] = dgr;
        S.g[grp].isd[r] = 1.0 / sqrt(dgr);
#pragma unroll
        for (int k = 0; k < M; k++) S.g[grp].rows[0][k][r] = V[k];     // U rows, from its columns
    }
    __syncthreads();
    // (2) T = Chat U ; R = U^T T scaled by 1/sqrt(diag) (:878-889)
    // row r of Chat (and below of Cfhalf) into registers first, every load in
    // flight together (a runtime-n loop waited on each load in turn); the sums
    // keep the k order
    double T[M], hr[M];
    const double *ch = h.chat + (long long)b * n * n;
#pragma unroll
    for (int k = 0; k < M; k++) hr[k] = (row_ok && k < n) ? ch[r * n + k] : 0.0;
#pragma unroll
    for (int j = 0; j < M; j++) {
        double s = 0.0;
        if (row_ok && j < n)
#pragma unroll
            for (int k = 0; k < M; k++)
                if (k < n) s += hr[k] * U_row(k, j);
        T[j] = s;
    }
    if (on)
#pragma unroll
        for (int k = 0; k < M; k++) S.g[grp].rows[1][r][k] = T[k];
    __syncthreads();
    double R[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        double s = 0.0;
        if (row_ok && j < n) {
#pragma unroll
            for (int k = 0; k < M; k++)
                if (k < n) s += U_row(k, r) * S.g[grp].rows[1][k][j];
            const int lo = r < j ? r : j, hi = r < j ? j : r;
            s = s * S.g[grp].isd[lo] * S.g[grp].isd[hi];   // the reference divides by each root (:886-889)
        }
        R[j] = s;
    }
    __syncthreads();
    HL_STAMP(q4);
    // (3) Rot = U R U^T (:891): T2 = R U^T (rows through LDS), A = U T2
    if (on)
#pragma unroll
        for (int k = 0; k < M; k++) S.g[grp].rows[1][r][k] = R[k];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < M; j++) {        // T2[r][j] = sum_k R[r][k] U[j][k]
        double s = 0.0;
        if (row_ok && j < n)
#pragma unroll
            for (int k = 0; k < M; k++)
                if (k < n) s += R[k] * U_row(j, k);
        T[j] = s;
    }
    __syncthreads();
    if (on)
#pragma unroll
        for (int k = 0; k < M; k++) S.g[grp].rows[1][r][k] = T[k];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < M; j++) {        // A[r][j] = sum_k U[r][k] T2[k][j]
        double s = 0.0;
        if (row_ok && j < n)
#pragma unroll
            for (int k = 0; k < M; k++)
                if (k < n) s += U_row(r, k) * S.g[grp].rows[1][k][j];
        A[j] = s;
    }
    __syncthreads();
    // (4) Rot = V diag V^T; g(x) = sign(x - 1) sqrt(2 max(0, x - ln x - 1))  (:892-894)
    double x;
    HL_STAMP(q5);
    if (h.v0) to_basis(h.v0 + (long long)b * n * n);
    HL_STAMP(q6);
    unconverged = hl_ojacobi<M>(A, V, S, grp, r, lane, 1, x) || unconverged;
    HL_STAMP(q7);
    if (h.v0) from_basis();
    __syncthreads();                               // the solve's last reads of the row buffers
    if (on) {
        // a NaN argument (x < 0 or NaN: a C that is not positive definite) stays NaN:
        // fmax(0, NaN) would make it 0 and the point's chi^2 finite
        const double arg = x - log(x) - 1;
        const double g = arg == arg ? sqrt(2 * fmax(0.0, arg)) : arg;
        S.g[grp].dg[r] = (x - 1 >= 0) ? g : -g;
#pragma unroll
        for (int k = 0; k < M; k++) S.g[grp].rows[0][k][r] = V[k];     // V rows, from its columns
    }
    __syncthreads();
    HL_STAMP(q8);
    // (5) U = Cfhalf V ; C = U diag(g) U^T (:907-912)
    const double *cf = h.cfhalf + (long long)b * n * n;
#pragma unroll
    for (int k = 0; k < M; k++) hr[k] = (row_ok && k < n) ? cf[r * n + k] : 0.0;
#pragma unroll
    for (int j = 0; j < M; j++) {
        double s = 0.0;
        if (row_ok && j < n)
#pragma unroll
            for (int k = 0; k < M; k++)
                if (k < n) s += hr[k] * U_row(k, j);
        T[j] = s;
    }
    __syncthreads();
    if (on)
#pragma unroll
        for (int k = 0; k < M; k++) S.g[grp].rows[1][r][k] = T[k];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < M; j++) {        // C[r][j] = sum_k (T[r][k] g_k) T[j][k]
        double s = 0.0;
        if (row_ok && j < n)
#pragma unroll
            for (int k = 0; k < M; k++)
                if (k < n) s += (T[k] * S.g[grp].dg[k]) * S.g[grp].rows[1][j][k];
        A[j] = s;
    }
    __syncthreads();
    if (on)
#pragma unroll
        for (int k = 0; k < M; k++) S.g[grp].rows[0][r][k] = A[k];
    __syncthreads();
    // an eigensolve that hit the sweep cap fails its (walker, bin): NaN bigX entries
    // (so -lnL is NaN) and a sticky status bit (cmbl_status); the reference stops the run
    const unsigned long long gmask = ((1ull << M) - 1) << (on ? grp * M : 0);
    const bool failed = on && (__ballot(unconverged) & gmask) != 0;
    if (live && failed && r == 0) atomicOr(h.status, CMBL_STATUS_HL_NOCONV);
    // vecp = lower-triangle elements (MatrixToElements :917-931); bigX entries of this bin
    if (live) {
        double *x = xrows + (long long)w * h.Np + (long long)b * h.ncl_used;
        for (int u = r; u < h.ncl_used; u += M) {
            const int k = h.cl_use[u];
            int i = 0;
            while ((i + 1) * (i + 2) / 2 <= k) i++;
            const int j = k - i * (i + 1) / 2;
            x[u] = failed ? __builtin_nan("") : S.g[grp].rows[0][i][j];
        }
    }
#ifdef CMAMD_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    HL_STAMP(q9);
    if (lane == 0) {
        const unsigned long long q[10] = {q0, q1, q2, q3, q4, q5, q6, q7, q8, q9};
        for (int i = 0; i < 9; i++) atomicAdd(&g_hl_tp[i], q[i + 1] - q[i]);
        atomicAdd(&g_hl_tp[11], 1ull);
    }
#endif
}
