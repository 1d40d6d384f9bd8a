// The chain state on the host: the current points, and the checkpoint image.
#include <cstring>
#include <vector>

#include "sampler.h"

namespace cmamd {

void sampler_get_state_host(cmbs *s, double *P, double *cur_like, double *mult, int *num_accept) {
    HIP_CHECK(hipDeviceSynchronize());
    const int W = s->W, np = s->np;
    const size_t ld = s->dc.ld;
    const Rows &R = s->dc.rows;
    if (P) {
        std::vector<double> t((size_t)np * ld);
        HIP_CHECK(hipMemcpy(t.data(), s->dc.sd + (size_t)R.P * ld, t.size() * 8, hipMemcpyDeviceToHost));
        for (int w = 0; w < W; w++)
            for (int i = 0; i < np; i++) P[(size_t)w * np + i] = t[(size_t)i * ld + w];
    }
    if (cur_like) HIP_CHECK(hipMemcpy(cur_like, s->dc.sd + (size_t)R.L * ld, (size_t)W * 8, hipMemcpyDeviceToHost));
    if (mult) HIP_CHECK(hipMemcpy(mult, s->dc.sd + (size_t)R.M * ld, (size_t)W * 8, hipMemcpyDeviceToHost));
    if (num_accept)
        HIP_CHECK(hipMemcpy(num_accept, s->dc.si + (size_t)R.NACC * ld, (size_t)W * 4, hipMemcpyDeviceToHost));
}

// Checkpoint image of every walker's chain state: the reference's .chk holds
// num_sample / MaxLike / num_accept (MCMC.f90:98-114, 199-218) and the
// proposal matrix (propose.f90:308-325) and restarts from the last chain row
// with a fresh RNG (GeneralSetup.f90:123-131); this image holds the complete
// device state instead -- point, CurLike, multiplicity, accept count, RANMAR
// table and Gaussian1 cache, cyclic-index and rotation state, each
// likelihood's term at the point -- so a resumed run continues each chain
// exactly.  Layout: StateHeader, double rows [ND][W], int rows [NI][W],
// current terms [n_like][W] (data then derived likelihoods).  The proposal covariance is the caller's part
// (cmbs_set_covariance before cmbs_load_state).
struct StateHeader {
    unsigned magic, version;
    int W, np, n_used, nblocks, all_n, slow_n, fast_n, R_total, ND, NI, n_like, theory_moved;
    int coll_cap, pad;      // sample-collector ring (0: not enabled) appended after the terms
    long long num_drag;
};
static constexpr unsigned STATE_MAGIC = 0x53424d43u;   // "CMBS"

size_t sampler_state_bytes(const cmbs *s) {
    const Rows &R = s->dc.rows;
    return sizeof(StateHeader) + (size_t)(R.ND + s->n_rows()) * s->W * 8 + (size_t)R.NI * s->W * 4 +
           sampler_collector_bytes(s);
}

static StateHeader state_header(const cmbs *s) {
    const Rows &R = s->dc.rows;
    return StateHeader{STATE_MAGIC, 2u, s->W, s->np, s->n_used, s->nblocks, s->all_n, s->slow_n, s->fast_n,
                       s->R_total, R.ND, R.NI, s->n_rows(), s->theory_moved ? 1 : 0,
                       s->coll.enabled ? s->coll.cap : 0, 0, s->num_drag};
}

void sampler_save_state(cmbs *s, void *buf, size_t bytes) {
    if (!s->started) fail(CMBL_ERR_ARG, "no chain state yet: cmbs_set_start first");
    if (bytes < sampler_state_bytes(s)) fail(CMBL_ERR_ARG, "state buffer too small (%zu < %zu bytes)", bytes,
                                            sampler_state_bytes(s));
    HIP_CHECK(hipDeviceSynchronize());
    const Rows &R = s->dc.rows;
    const size_t ld = s->dc.ld, W = s->W;
    char *p = static_cast<char *>(buf);
    const StateHeader h = state_header(s);
    std::memcpy(p, &h, sizeof h);
    p += sizeof h;
    HIP_CHECK(hipMemcpy2D(p, W * 8, s->dc.sd, ld * 8, W * 8, R.ND, hipMemcpyDeviceToHost));
    p += (size_t)R.ND * W * 8;
    HIP_CHECK(hipMemcpy2D(p, W * 4, s->dc.si, ld * 4, W * 4, R.NI, hipMemcpyDeviceToHost));
    p += (size_t)R.NI * W * 4;
    if (s->n_rows() > 0)
        HIP_CHECK(hipMemcpy2D(p, W * 8, s->dc.cur_terms, ld * 8, W * 8, s->n_rows(), hipMemcpyDeviceToHost));
    p += (size_t)s->n_rows() * W * 8;
    if (s->coll.enabled) sampler_collector_save(s, p);
}

void sampler_load_state(cmbs *s, const void *buf, size_t bytes) {
    rot_schedule_unknown(s);
    if (bytes < sizeof(StateHeader)) fail(CMBL_ERR_ARG, "state image too short");
    StateHeader h;
    std::memcpy(&h, buf, sizeof h);
    if (h.magic != STATE_MAGIC || h.version != 2u) fail(CMBL_ERR_FORMAT, "not a cmbs state image");
    const StateHeader m = state_header(s);
    if (h.W != m.W || h.np != m.np || h.n_used != m.n_used || h.nblocks != m.nblocks || h.all_n != m.all_n ||
        h.slow_n != m.slow_n || h.fast_n != m.fast_n || h.R_total != m.R_total || h.ND != m.ND || h.NI != m.NI ||
        h.n_like != m.n_like || h.coll_cap != m.coll_cap)
        fail(CMBL_ERR_ARG,
             "state image is for a different sampler (W %d np %d blocks %d likelihoods %d; this one W %d np %d "
             "blocks %d likelihoods %d)", h.W, h.np, h.nblocks, h.n_like, m.W, m.np, m.nblocks, m.n_like);
    if (bytes < sampler_state_bytes(s)) fail(CMBL_ERR_FORMAT, "state image truncated");
    const Rows &R = s->dc.rows;
    const size_t ld = s->dc.ld, W = s->W;
    const char *p = static_cast<const char *>(buf) + sizeof h;
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy2D(s->dc.sd, ld * 8, p, W * 8, W * 8, R.ND, hipMemcpyHostToDevice));
    p += (size_t)R.ND * W * 8;
    HIP_CHECK(hipMemcpy2D(s->dc.si, ld * 4, p, W * 4, W * 4, R.NI, hipMemcpyHostToDevice));
    p += (size_t)R.NI * W * 4;
    if (s->n_rows() > 0)
        HIP_CHECK(hipMemcpy2D(s->dc.cur_terms, ld * 8, p, W * 8, W * 8, s->n_rows(), hipMemcpyHostToDevice));
    p += (size_t)s->n_rows() * W * 8;
    s->drv_cur = false;   // the derived rows of like_terms are not part of the image
    if (s->coll.enabled) sampler_collector_load(s, p);
    s->num_drag = h.num_drag;
    s->theory_moved = h.theory_moved != 0;
    s->theory_stale = s->theory_moved && !s->likes.empty();
    s->started = true;
}

}  // namespace cmamd
