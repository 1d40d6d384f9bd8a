// The history ring's statistics: per-chain means and covariances over a window
// of history rows and the per-GPU chain moments of the convergence test, and
// the ring's host-side copies.
#include <algorithm>

#include "sampler.h"

namespace cmamd {

// Per-chain mean and covariance over history rows first..last
// (SampleCollector.f90:235-246), two passes like the reference (mean, then
// the centred products).  A block owns 64 walkers (lane = walker, coalesced
// rows) and HS_PH row phases (wave p takes rows first+p, first+p+HS_PH, ...);
// the phase partials are combined in fixed order, so results are
// deterministic.  The covariance pass runs one block per (walker tile,
// parameter i) with the n products of row i in registers (NC = n rounded up).
static constexpr int HS_PH = 4;

template <int NC>
__global__ __launch_bounds__(64 * HS_PH) void hist_mean_kernel(const double *hist, int cap, int W, int n, int first,
                                                              int last, double *means)
{
    __shared__ double part[HS_PH][NC][64];
    const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int w = blockIdx.x * 64 + lane;
    double acc[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) acc[j] = 0.0;
    if (w < W)
        for (int tt = first + ph; tt <= last; tt += HS_PH) {
            const double *row = hist + (size_t)(tt % cap) * (n + 1) * W + w;
#pragma unroll
            for (int j = 0; j < NC; j++)
                if (j < n) acc[j] += row[(size_t)j * W];
        }
#pragma unroll
    for (int j = 0; j < NC; j++) part[ph][j][lane] = acc[j];
    __syncthreads();
    if (ph == 0 && w < W) {
        const double cnt = last - first + 1;
        for (int j = 0; j < n; j++) {
            double v = part[0][j][lane];
            for (int p = 1; p < HS_PH; p++) v += part[p][j][lane];
            means[(size_t)w * n + j] = v / cnt;
        }
    }
}

template <int NC>
__global__ __launch_bounds__(64 * HS_PH) void hist_cov_kernel(const double *hist, int cap, int W, int n, int first,
                                                             int last, const double *means, double *covs)
{
    __shared__ double part[HS_PH][NC][64];
    const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int w = blockIdx.x * 64 + lane, i = blockIdx.y;
    double acc[NC], m[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) {
        acc[j] = 0.0;
        m[j] = (w < W && j < n) ? means[(size_t)w * n + j] : 0.0;
    }
    double mi = 0.0;
#pragma unroll
    for (int j = 0; j < NC; j++)
        if (j == i) mi = m[j];
    if (w < W)
        for (int tt = first + ph; tt <= last; tt += HS_PH) {
            const double *row = hist + (size_t)(tt % cap) * (n + 1) * W + w;
            const double di = row[(size_t)i * W] - mi;
#pragma unroll
            for (int j = 0; j < NC; j++)
                if (j < n) acc[j] += (row[(size_t)j * W] - m[j]) * di;
        }
#pragma unroll
    for (int j = 0; j < NC; j++) part[ph][j][lane] = acc[j];
    __syncthreads();
    if (ph == 0 && w < W) {
        const double cnt = last - first + 1;
        for (int j = 0; j < n; j++) {
            double v = part[0][j][lane];
            for (int p = 1; p < HS_PH; p++) v += part[p][j][lane];
            covs[(size_t)w * n * n + (size_t)i * n + j] = v / cnt;
        }
    }
}

// Per-GPU partial sums of the chain moments for the convergence exchange
// (TMpiChainCollector_UpdateCovAndCheckConverge, SampleCollector.f90:233-286):
// every walker is one chain with count = last-first+1 samples.
//   gmean == nullptr : out = [S0 = sum count, sum count*m (n), sum count*cov (n*n),
//                             sum cov (n*n), number of chains]
//   gmean != nullptr : out = sum count*(m-gmean)(m-gmean)^T (n*n)
// One block; each thread owns a fixed strided set of walkers and the partials
// are combined in a fixed tree order, so the sums are deterministic.
__global__ __launch_bounds__(256) void chain_moments_kernel(const double *means, const double *covs, int W, int n,
                                                           double count, const int *wcount, const double *gmean,
                                                           double *out)
{   // wcount (may be null): each walker's own sample count (collector windows)
    __shared__ double red[256];
    const int nout = gmean ? n * n : 2 + n + 2 * n * n;
    for (int o = 0; o < nout; o++) {
        double acc = 0.0;
        for (int w = threadIdx.x; w < W; w += 256) {
            const double *m = means + (size_t)w * n;
            const double *C = covs + (size_t)w * n * n;
            const double cw = wcount ? (double)wcount[w] : count;
            double v;
            if (gmean) {
                const int i = o / n, j = o % n;
                v = cw * (m[i] - gmean[i]) * (m[j] - gmean[j]);
            } else if (o == 0) {
                v = cw;
            } else if (o <= n) {
                v = cw * m[o - 1];
            } else if (o <= n + n * n) {
                v = cw * C[o - 1 - n];
            } else if (o <= n + 2 * n * n) {
                v = C[o - 1 - n - n * n];
            } else {
                v = 1.0;
            }
            acc += v;
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[o] = red[0];
        __syncthreads();
    }
}

void chain_moments_launch(const double *means, const double *covs, int W, int n, double count, const int *wcount,
                          const double *gmean, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(chain_moments_kernel, dim3(1), dim3(256), 0, stream, means, covs, W, n, count, wcount, gmean,
                       out);
    HIP_CHECK(hipGetLastError());
}

void sampler_enable_history(cmbs *s, int capacity) {
    s->hist.alloc((size_t)capacity * (s->n_used + 1) * s->W * 8);   // per step: P(params_used) rows, CurLike row
    s->hist_cap = capacity;
    s->hist_count = 0;
    if (s->n_rows() > 0) {   // per step: each likelihood's -lnL at the current point
        s->hist_terms.alloc((size_t)capacity * s->n_rows() * s->W * 8);
        HIP_CHECK(hipMemset(s->hist_terms.p, 0, s->hist_terms.bytes));
    }
}

void sampler_history_stats(cmbs *s, int first, int last, double *means, double *covs, hipStream_t stream) {
    if (s->hist_cap == 0) fail(CMBL_ERR_ARG, "history not enabled");
    if (first < 0 || last < first || last >= s->hist_count || s->hist_count - first > s->hist_cap)
        fail(CMBL_ERR_ARG, "history rows [%d, %d] not available (count %d, capacity %d)", first, last,
             s->hist_count, s->hist_cap);
    const int n = s->n_used;
    const dim3 gm((s->W + 63) / 64), gc((s->W + 63) / 64, n), blk(64 * HS_PH);
    const double *h = s->hist.as<double>();
    auto run = [&](auto kmean, auto kcov) {
        hipLaunchKernelGGL(kmean, gm, blk, 0, stream, h, s->hist_cap, s->W, n, first, last, means);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(kcov, gc, blk, 0, stream, h, s->hist_cap, s->W, n, first, last, means, covs);
        HIP_CHECK(hipGetLastError());
    };
    if (n <= 8) run(hist_mean_kernel<8>, hist_cov_kernel<8>);
    else if (n <= 16) run(hist_mean_kernel<16>, hist_cov_kernel<16>);
    else if (n <= 32) run(hist_mean_kernel<32>, hist_cov_kernel<32>);
    else run(hist_mean_kernel<64>, hist_cov_kernel<64>);
}

void sampler_chain_moments(cmbs *s, int first, int last, const double *gmean, double *out, hipStream_t stream) {
    const int n = s->n_used;
    s->mom.grow((size_t)s->W * (n + n * n) * 8);
    double *means = s->mom.as<double>(), *covs = means + (size_t)s->W * n;
    sampler_history_stats(s, first, last, means, covs, stream);
    chain_moments_launch(means, covs, s->W, n, (double)(last - first + 1), nullptr, gmean, out, stream);
}

void sampler_history_host(cmbs *s, int first, int count, double *out) {
    if (s->hist_cap == 0) fail(CMBL_ERR_ARG, "history not enabled");
    const int oldest = std::max(0, s->hist_count - s->hist_cap);
    if (first < oldest || first + count > s->hist_count)
        fail(CMBL_ERR_ARG, "history rows [%d, %d) not kept (rows %d..%d)", first, first + count, oldest, s->hist_count - 1);
    HIP_CHECK(hipDeviceSynchronize());
    const size_t blk = (size_t)(s->n_used + 1) * s->W;
    for (int k = 0; k < count; k++) {
        const int slot = (first + k) % s->hist_cap;
        HIP_CHECK(hipMemcpy(out + (size_t)k * blk, s->hist.as<double>() + (size_t)slot * blk, blk * 8,
                            hipMemcpyDeviceToHost));
    }
}

void sampler_history_terms_host(cmbs *s, int first, int count, double *out) {
    if (s->hist_cap == 0) fail(CMBL_ERR_ARG, "history not enabled");
    const int oldest = std::max(0, s->hist_count - s->hist_cap);
    if (first < oldest || first + count > s->hist_count)
        fail(CMBL_ERR_ARG, "history rows [%d, %d) not kept (rows %d..%d)", first, first + count, oldest, s->hist_count - 1);
    const size_t blk = (size_t)s->n_rows() * s->W;
    if (blk == 0) return;
    HIP_CHECK(hipDeviceSynchronize());
    for (int k = 0; k < count; k++) {
        const int slot = (first + k) % s->hist_cap;
        HIP_CHECK(hipMemcpy(out + (size_t)k * blk, s->hist_terms.as<double>() + (size_t)slot * blk, blk * 8,
                            hipMemcpyDeviceToHost));
    }
}

// checkpoint resume of the history ring: rows [first, first + count) as
// written by sampler_history_host go back to their ring slots, and the ring
// continues at first + count (the samples the convergence test windows over,
// TMpiChainCollector_ReadState's Samples%LoadState, SampleCollector.f90:167)
void sampler_history_restore(cmbs *s, int first, int count, const double *in, const double *terms) {
    if (s->hist_cap == 0) fail(CMBL_ERR_ARG, "history not enabled");
    if (first < 0 || count < 0 || count > s->hist_cap)
        fail(CMBL_ERR_ARG, "history rows [%d, %d) do not fit the ring (capacity %d)", first, first + count,
             s->hist_cap);
    HIP_CHECK(hipDeviceSynchronize());
    const size_t blk = (size_t)(s->n_used + 1) * s->W;
    for (int k = 0; k < count; k++) {
        const int slot = (first + k) % s->hist_cap;
        HIP_CHECK(hipMemcpy(s->hist.as<double>() + (size_t)slot * blk, in + (size_t)k * blk, blk * 8,
                            hipMemcpyHostToDevice));
    }
    const size_t tblk = (size_t)s->n_rows() * s->W;
    if (terms && tblk)
        for (int k = 0; k < count; k++) {
            const int slot = (first + k) % s->hist_cap;
            HIP_CHECK(hipMemcpy(s->hist_terms.as<double>() + (size_t)slot * tblk, terms + (size_t)k * tblk,
                                tblk * 8, hipMemcpyHostToDevice));
        }
    s->hist_count = first + count;
}

}  // namespace cmamd
