// C-ABI of the goodness-of-fit statistics over time (kernels_gof_dynamic.hpp; included by capi.hip after
// capi_gof.hpp, whose draws, batching and lane choice it shares).  The reference has no counterpart.
#pragma once

namespace {

// int64 entries per sample of the three records
struct GofDynSizes {
    size_t overlap, steps, geodesic;
    GofDynSizes(int T, int N, bool temporal, bool geo)
        : overlap(temporal ? (size_t)T * T : 0), steps(temporal ? (size_t)(T - 1) * 2 * N : 0),
          geodesic(geo ? (size_t)T * N : 0) {}
    size_t total() const { return overlap + steps + geodesic; }
};

int gof_dynamic_check(dlsm_chain *h, bool geo) {
    NEED(h, h->T <= 65535, "T=%d: the statistics over time hold at most 65535 time steps", h->T);
    if (geo && h->W > 64 * GOF_GEO_MAX_WORDS)
        FAIL(h, DLSM_E_LIMIT, "N=%d: the geodesic distances hold at most %d nodes", h->N, 2048 * GOF_GEO_MAX_WORDS);
    return DLSM_OK;
}

template <int NW>
void gof_geodesic_launch_nw(dlsm_chain *h, const uint32_t *rows, int nets, int directed, int64_t *dgeo) {
    const int N = h->N;
    const int nbx = std::max(1, std::min((N + 3) / 4, 8192 / nets));
    hipLaunchKernelGGL((k_gof_geodesic<NW>), dim3(nbx, nets), dim3(256), 0, h->stream, rows, N, h->W, directed,
                       dgeo);
}

// the records of n samples' networks: rows (and trows, directed) [n * T][N][W] on the device -> drec, the
// n samples' overlap [n][T][T], then steps [n][T-1][2N], then geodesic [n * T][N]; zeroed here
int gof_dynamic_launch(dlsm_chain *h, const uint32_t *rows, const uint32_t *trows, int n, bool temporal,
                       bool geo, int64_t *drec) {
    const int T = h->T, N = h->N, W = h->W;
    const GofDynSizes sz(T, N, temporal, geo);
    const int directed = h->model != DLSM_UNDIRECTED;           // trows: read by the steps alone
    HIPCHK(h, hipMemsetAsync(drec, 0, (size_t)n * sz.total() * sizeof(int64_t), h->stream));
    if (temporal) {
        // four quad-words per thread
        const unsigned gx = (unsigned)(((size_t)N * W / 4 + 1023) / 1024);
        hipLaunchKernelGGL(k_gof_overlap, dim3(gx, T, n), dim3(256), 0, h->stream, rows, T, N, W, directed, drec);
        HIPCHK(h, hipGetLastError());
        if (T > 1) {
            const int nets = n * (T - 1);
            const int nbx = std::max(1, std::min(N, 8192 / nets));
            hipLaunchKernelGGL(k_gof_step, dim3(nbx, nets), dim3(256), 0, h->stream, rows, trows, T, N, W,
                               gof_lanes_per_row(W), drec + (size_t)n * sz.overlap);
            HIPCHK(h, hipGetLastError());
        }
    }
    if (geo) {
        int64_t *dgeo = drec + (size_t)n * (sz.overlap + sz.steps);
        const int nw = (W + 63) / 64;
        if (nw <= 1) gof_geodesic_launch_nw<1>(h, rows, n * T, directed, dgeo);
        else if (nw <= 2) gof_geodesic_launch_nw<2>(h, rows, n * T, directed, dgeo);
        else if (nw <= 4) gof_geodesic_launch_nw<4>(h, rows, n * T, directed, dgeo);
        else if (nw <= 8) gof_geodesic_launch_nw<8>(h, rows, n * T, directed, dgeo);
        else gof_geodesic_launch_nw<GOF_GEO_MAX_WORDS>(h, rows, n * T, directed, dgeo);
        HIPCHK(h, hipGetLastError());
    }
    return DLSM_OK;
}

// device records of n samples -> the caller's arrays (at sample s0); the stream is synchronised here and the
// lower triangle of every overlap is filled from the upper one
int gof_dynamic_fetch(dlsm_chain *h, const int64_t *drec, int n, size_t s0, bool temporal, bool geo,
                      int64_t *overlap, int64_t *steps, int64_t *geodesic) {
    const int T = h->T;
    const GofDynSizes sz(T, h->N, temporal, geo);
    if (temporal) {
        HIPCHK(h, hipMemcpyAsync(overlap + s0 * sz.overlap, drec, (size_t)n * sz.overlap * sizeof(int64_t),
                                 hipMemcpyDeviceToHost, h->stream));
        if (sz.steps)
            HIPCHK(h, hipMemcpyAsync(steps + s0 * sz.steps, drec + (size_t)n * sz.overlap,
                                     (size_t)n * sz.steps * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    }
    if (geo)
        HIPCHK(h, hipMemcpyAsync(geodesic + s0 * sz.geodesic, drec + (size_t)n * (sz.overlap + sz.steps),
                                 (size_t)n * sz.geodesic * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (temporal)
        for (int s = 0; s < n; ++s) {
            int64_t *o = overlap + (s0 + s) * sz.overlap;
            for (int t = 0; t < T; ++t)
                for (int u = t + 1; u < T; ++u) o[(size_t)u * T + t] = o[(size_t)t * T + u];
        }
    return DLSM_OK;
}

}  // namespace

extern "C" {

int dlsm_gof_dynamic_simulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii,
                              int S, uint64_t seed, uint32_t first_index, int batch, int64_t *overlap,
                              int64_t *steps, int64_t *geodesic, uint32_t *bits) {
    NEED(h, h && Xs && intercepts, "null argument");
    const bool temporal = overlap != nullptr, geo = geodesic != nullptr;
    NEED(h, temporal || geo, "overlap and steps, or geodesic, or both must be given");
    NEED(h, temporal == (steps != nullptr) || h->T == 1, "overlap and steps go together");
    int rc = gof_simulate_check(h, radii, S, first_index, batch);
    if (rc || (rc = gof_dynamic_check(h, geo))) return rc;
    const GofDynSizes sz(h->T, h->N, temporal, geo);
    return gof_simulate_batches(h, Xs, intercepts, radii, S, seed, first_index, batch, sz.total(), bits,
                                [&](const uint32_t *rows, const uint32_t *trows, int n, size_t s0,
                                    int64_t *drec) -> int {
        if (int rc = gof_dynamic_launch(h, rows, trows, n, temporal, geo, drec)) return rc;
        return gof_dynamic_fetch(h, drec, n, s0, temporal, geo, overlap, steps, geodesic);
    });
}

int dlsm_gof_dynamic_observed(dlsm_chain *h, const uint32_t *bits, int64_t *overlap, int64_t *steps,
                              int64_t *geodesic) {
    NEED(h, h && bits, "null argument");
    const bool temporal = overlap != nullptr, geo = geodesic != nullptr;
    NEED(h, temporal || geo, "overlap and steps, or geodesic, or both must be given");
    NEED(h, temporal == (steps != nullptr) || h->T == 1, "overlap and steps go together");
    int rc = gof_dynamic_check(h, geo);
    if (rc) return rc;
    const int T = h->T, N = h->N, W = h->W;
    const size_t net_words = (size_t)N * W;
    if ((rc = check_packed_network(h, bits))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const bool directed = h->model != DLSM_UNDIRECTED;
    const bool need_t = directed && temporal && T > 1;          // only the shared partners read the columns
    const GofDynSizes sz(T, N, temporal, geo);
    DevArray<uint32_t> bBits, bT; DevArray<int64_t> bS;
    if (bBits.alloc(h, (size_t)T * net_words) || (need_t && bT.alloc(h, (size_t)T * net_words)) ||
        bS.alloc(h, sz.total())) return DLSM_E_HIP;
    HIPCHK(h, hipMemcpyAsync(bBits, bits, (size_t)T * net_words * sizeof(uint32_t), hipMemcpyHostToDevice,
                             h->stream));
    if (need_t) {
        hipLaunchKernelGGL(k_gof_transpose, dim3((unsigned)((net_words + 255) / 256), T), dim3(256), 0,
                           h->stream, bBits, N, W, bT);
        HIPCHK(h, hipGetLastError());
    }
    rc = gof_dynamic_launch(h, bBits, need_t ? bT.get() : nullptr, 1, temporal, geo,
                            bS);
    if (rc) return rc;
    return gof_dynamic_fetch(h, bS, 1, 0, temporal, geo, overlap, steps, geodesic);
}

}  // extern "C"
