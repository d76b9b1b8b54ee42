// C-ABI of the per-dyad convergence diagnostics (kernels_conv.hpp; included by capi.hip after capi_score.hpp:
// the tiles of capi_ic.hpp).  The reference has no counterpart.
#pragma once

namespace {

constexpr int CONV_G_MAX = 1 << 16;                       // workgroups of one time step

template <int D>
void conv_launch(dlsm_chain *h, bool directed, dim3 grid, const double *Xs, const double *ic, const double *radii,
                 const int2 *tiles, int n_tiles, int L, int M, int seg_len, int batch_len, const double *edges,
                 int n_rhat, int n_ess, conv_count_t *hist_rhat, conv_count_t *hist_ess, double *node_rhat,
                 double *node_ess, double *pointwise) {
    if (directed)
        hipLaunchKernelGGL((k_conv_accumulate<D, true>), grid, dim3(IC_NT), 0, h->stream, Xs, ic, radii, tiles,
                           n_tiles, L, M, seg_len, batch_len, h->T, h->N, edges, n_rhat, n_ess, hist_rhat, hist_ess,
                           node_rhat, node_ess, pointwise);
    else
        hipLaunchKernelGGL((k_conv_accumulate<D, false>), grid, dim3(IC_NT), 0, h->stream, Xs, ic, radii, tiles,
                           n_tiles, L, M, seg_len, batch_len, h->T, h->N, edges, n_rhat, n_ess, hist_rhat, hist_ess,
                           node_rhat, node_ess, pointwise);
}

// n edges, finite and ascending, into out [CONV_MAX_EDGES] padded with +inf
int conv_check_edges(dlsm_chain *h, const char *what, const double *edges, int n, double *out) {
    NEED(h, n >= 0 && n <= CONV_MAX_EDGES, "%s: %d edges, at most %d are held", what, n, CONV_MAX_EDGES);
    NEED(h, n == 0 || edges, "null argument");
    for (int e = 0; e < CONV_MAX_EDGES; ++e) out[e] = INFINITY;
    for (int e = 0; e < n; ++e) {
        if (!std::isfinite(edges[e])) FAIL(h, DLSM_E_DATA, "%s: edge %d is not finite", what, e);
        if (e && !(edges[e] > edges[e - 1])) FAIL(h, DLSM_E_DATA, "%s: the edges must ascend (edge %d)", what, e);
        out[e] = edges[e];
    }
    return DLSM_OK;
}

}  // namespace

extern "C" {

int dlsm_convergence_accumulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii,
                                int n_segments, int seg_len, int batch_len, const double *rhat_edges,
                                int n_rhat_edges, const double *ess_edges, int n_ess_edges, uint64_t *hist_rhat,
                                uint64_t *hist_ess, double *node_rhat_max, double *node_ess_min, double *pointwise) {
    NEED(h, h && Xs && intercepts && hist_rhat && hist_ess && node_rhat_max && node_ess_min, "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, n_segments >= 2 && n_segments % 2 == 0, "n_segments=%d: the halves of the chains, an even number >= 2",
         n_segments);
    NEED(h, seg_len >= 2, "seg_len=%d: a segment needs at least two samples", seg_len);
    NEED(h, batch_len >= 1 && batch_len <= seg_len / 2, "batch_len=%d: between 1 and seg_len / 2 = %d", batch_len,
         seg_len / 2);
    NEED(h, (long long)n_segments * seg_len <= 0x7FFFFFFFLL, "too many samples");
    const int T = h->T, N = h->N, D = h->D, S = n_segments * seg_len;
    double edges[2 * CONV_MAX_EDGES];
    if (int rc = conv_check_edges(h, "rhat_edges", rhat_edges, n_rhat_edges, edges)) return rc;
    if (int rc = conv_check_edges(h, "ess_edges", ess_edges, n_ess_edges, edges + CONV_MAX_EDGES)) return rc;
    if (directed)
        for (size_t k = 0; k < (size_t)S * N; ++k)
            if (!(radii[k] > 0.0)) FAIL(h, DLSM_E_DATA, "radii must be positive (sample %zu, node %zu)", k / N, k % N);
    HIPCHK(h, hipSetDevice(h->device));
    const int TI = D <= 4 ? IcPlan<1>::TI : IcPlan<8>::TI;
    const std::vector<int2> tiles = ic_tiles(N, TI, directed);
    const int n_tiles = (int)tiles.size();
    const int L = (n_tiles + CONV_G_MAX - 1) / CONV_G_MAX;
    const int G = L ? (n_tiles + L - 1) / L : 0;
    const size_t n_hr = (size_t)T * (n_rhat_edges + 1), n_he = (size_t)T * (n_ess_edges + 1);
    const size_t node_bytes = (size_t)T * N * sizeof(double), pw_bytes = (size_t)T * N * N * 2 * sizeof(double);
    // all S samples are resident: the accumulators of a dyad cannot be split across calls
    const size_t per_sample = ((size_t)T * N * D + 2 + (directed ? N : 0)) * sizeof(double);
    const size_t fixed = (size_t)n_tiles * sizeof(int2) + sizeof(edges) + (n_hr + n_he) * sizeof(conv_count_t) +
                         2 * node_bytes + (pointwise ? pw_bytes : 0) + ((size_t)64 << 20);
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    if (fixed + (size_t)S * per_sample > free_b) {
        const long long fit = free_b > fixed ? (long long)((free_b - fixed) / per_sample) : 0;
        FAIL(h, DLSM_E_LIMIT, "S=%d samples of T=%d N=%d D=%d need %.1f MB of device memory, %.1f MB are free: "
             "the largest S that fits is %lld", S, T, N, D, (fixed + (size_t)S * per_sample) / 1048576.0,
             free_b / 1048576.0, fit);
    }
    const std::vector<double> inf_row((size_t)T * N, INFINITY);
    DevBuf bX, bB, bR, bTiles, bE, bHR, bHE, bNR, bNE, bPW;
    HIPCHK(h, hipMalloc(&bX.p, (size_t)S * T * N * D * sizeof(double)));
    HIPCHK(h, hipMalloc(&bB.p, (size_t)S * 2 * sizeof(double)));
    if (directed) HIPCHK(h, hipMalloc(&bR.p, (size_t)S * N * sizeof(double)));
    HIPCHK(h, hipMalloc(&bTiles.p, std::max<size_t>(1, n_tiles) * sizeof(int2)));
    HIPCHK(h, hipMalloc(&bE.p, sizeof(edges)));
    HIPCHK(h, hipMalloc(&bHR.p, n_hr * sizeof(conv_count_t)));
    HIPCHK(h, hipMalloc(&bHE.p, n_he * sizeof(conv_count_t)));
    HIPCHK(h, hipMalloc(&bNR.p, node_bytes));
    HIPCHK(h, hipMalloc(&bNE.p, node_bytes));
    if (pointwise) {
        HIPCHK(h, hipMalloc(&bPW.p, pw_bytes));
        HIPCHK(h, hipMemsetAsync(bPW.p, 0, pw_bytes, h->stream));
    }
    HIPCHK(h, hipMemsetAsync(bHR.p, 0, n_hr * sizeof(conv_count_t), h->stream));
    HIPCHK(h, hipMemsetAsync(bHE.p, 0, n_he * sizeof(conv_count_t), h->stream));
    HIPCHK(h, hipMemsetAsync(bNR.p, 0, node_bytes, h->stream));
    HIPCHK(h, hipMemcpyAsync(bNE.p, inf_row.data(), node_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bX.p, Xs, (size_t)S * T * N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bB.p, intercepts, (size_t)S * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (directed)
        HIPCHK(h, hipMemcpyAsync(bR.p, radii, (size_t)S * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bTiles.p, tiles.data(), (size_t)n_tiles * sizeof(int2), hipMemcpyHostToDevice,
                             h->stream));
    HIPCHK(h, hipMemcpyAsync(bE.p, edges, sizeof(edges), hipMemcpyHostToDevice, h->stream));
    if (G) {                      // (N = 1 has no dyads: empty histograms, the nodes keep 0 and +inf)
        DISPATCH_D(h, D, conv_launch<DD>(h, directed, dim3((unsigned)G, (unsigned)T), bX.as<double>(),
                                         bB.as<double>(), directed ? bR.as<double>() : nullptr, bTiles.as<int2>(),
                                         n_tiles, L, n_segments, seg_len, batch_len, bE.as<double>(), n_rhat_edges,
                                         n_ess_edges, bHR.as<conv_count_t>(), bHE.as<conv_count_t>(),
                                         bNR.as<double>(), bNE.as<double>(),
                                         pointwise ? bPW.as<double>() : nullptr));
        HIPCHK(h, hipGetLastError());
    }
    static_assert(sizeof(conv_count_t) == sizeof(uint64_t), "the counts are 64-bit");
    HIPCHK(h, hipMemcpyAsync(hist_rhat, bHR.p, n_hr * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hist_ess, bHE.p, n_he * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(node_rhat_max, bNR.p, node_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(node_ess_min, bNE.p, node_bytes, hipMemcpyDeviceToHost, h->stream));
    if (pointwise) HIPCHK(h, hipMemcpyAsync(pointwise, bPW.p, pw_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
