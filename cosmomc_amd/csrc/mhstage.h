// Moving the walker state between HBM and a workgroup's LDS image (LDS-DMA in,
// 16-byte stores out), the instrumented build's phase stamps and the trial's
// change mask.  Included by sampler.hip after mhpropose.h.
// (included inside namespace cmamd)
#pragma once

// Phase timestamps (s_memtime) of the first 64 mh_kernel blocks, only in the
// instrumented build (make EXTRA=-DCMAMD_STAMPS; tools/mh_stamps.py).
#ifdef CMAMD_STAMPS
__device__ unsigned long long g_stamps[64][16];
#define STAMP(i)                                                                                \
    do {                                                                                        \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                            \
        if (ACCEPT && PROPOSE && lane == 0 && wave == 0 && blockIdx.x < 64) g_stamps[blockIdx.x][i] = t_;            \
    } while (0)
#else
#define STAMP(i) ((void)0)
#endif

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

// LDS-DMA (global_load_lds_dwordx4): rows [r0, r0+n) of a [rows][ld] double
// array, columns wb..wb+MB-1, into LDS rows [d0, d0+n) of [row][MB].  One wave
// instruction moves 1 KB (64 lanes x 16 bytes), i.e. 1024 / (8 MB) rows, and
// nothing passes through VGPRs, so every piece of the walker state is in
// flight at once.  Lanes past the last row are off.
__device__ inline void dma_rows_f64(double *dst, int d0, const double *src, int r0, int n, size_t ld, int wb,
                                    int lane, int wave = 0, int nw = 1)
{
    constexpr int LPR = MB / 2, RPI = 64 / LPR;   // lanes per row, rows per instruction
    for (int r = RPI * wave; r < n; r += RPI * nw) {
        const int rr = r + lane / LPR;
        if (rr < n) {
            const double *g = src + (size_t)(r0 + rr) * ld + wb + 2 * (lane % LPR);
            __builtin_amdgcn_global_load_lds((gbl_void_t *)g, (lds_void_t *)(dst + (size_t)(d0 + r) * MB), 16, 0, 0);
        }
    }
}

// same for int rows
__device__ inline void dma_rows_i32(int *dst, const int *src, int n, size_t ld, int wb, int lane, int wave = 0,
                                    int nw = 1)
{
    constexpr int LPR = MB / 4, RPI = 64 / LPR;
    for (int r = RPI * wave; r < n; r += RPI * nw) {
        const int rr = r + lane / LPR;
        if (rr < n) {
            const int *g = src + (size_t)rr * ld + wb + 4 * (lane % LPR);
            __builtin_amdgcn_global_load_lds((gbl_void_t *)g, (lds_void_t *)(dst + (size_t)r * MB), 16, 0, 0);
        }
    }
}

// flat copy of n 4-byte words (source allocation padded to a multiple of 64 words)
__device__ inline void dma_words(void *dst, const void *src, int n, int lane, int wave = 0, int nw = 1)
{
    for (int i = 64 * wave; i < n; i += 64 * nw) {
        const unsigned *g = reinterpret_cast<const unsigned *>(src) + i + lane;
        __builtin_amdgcn_global_load_lds((gbl_void_t *)g, (lds_void_t *)(reinterpret_cast<unsigned *>(dst) + i), 4,
                                         0, 0);
    }
}

// write-back of LDS rows [row][MB] (src rows src_r0 + (r - r0)) to HBM rows r
// in [r0, r1), columns wb .. wb+MB-1: 16 bytes per thread (MB = 16 doubles is 8
// threads a row, 16 ints 4 threads), all threads of the block, rows round-robin
template <class T>
__device__ inline void stage_out(T *dst, const T *src, int src_r0, int r0, int r1, size_t ld, int wb)
{
    constexpr int PER = 16 / sizeof(T), TPR = MB / PER, RPB = MH_THREADS / TPR;   // per thread, threads per row, rows per pass
    const int tr = threadIdx.x / TPR, col = (threadIdx.x % TPR) * PER;
    for (int r = r0 + tr; r < r1; r += RPB)
        *reinterpret_cast<uint4 *>(dst + (size_t)r * ld + wb + col) =
            *reinterpret_cast<const uint4 *>(src + (size_t)(src_r0 + r - r0) * MB + col);
}

// changeMask of the trial (TheoryLike_GetLogLikeMain, calclike.f90:302-306):
// likelihood l must be recomputed iff a parameter it depends on moved
// (LogLikeWithTheorySet :377); 1 = recompute, 0 = keep the current term
template <class QT, class QP>
__device__ inline void write_like_flags(const DevCfg &c, const QT &trial, const QP &P, int w)
{
    for (int l = 0; l < c.n_like; l++) {
        const unsigned long long m = c.like_dep[l];
        bool ch = false;
        for (int i = 0; i < c.np; i++)
            if (((m >> i) & 1ull) && trial[i] != P[i]) ch = true;
        c.like_flag[(size_t)l * c.ld + w] = ch ? 1 : 0;
    }
}
