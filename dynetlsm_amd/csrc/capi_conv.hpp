// C-ABI of the per-dyad convergence diagnostics (kernels_conv.hpp; included by capi.hip after capi_samples.hpp,
// whose input checks and resident samples it uses).  The reference has no counterpart.
#pragma once

namespace {

constexpr int CONV_G_MAX = 1 << 16;                       // workgroups of one time step

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
    if (int rc = check_radii_positive(h, radii, S)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    ResidentSamples in(h);
    const int n_tiles = in.n_tiles;
    const int L = (n_tiles + CONV_G_MAX - 1) / CONV_G_MAX;
    const int G = L ? (n_tiles + L - 1) / L : 0;
    const size_t n_hr = (size_t)T * (n_rhat_edges + 1), n_he = (size_t)T * (n_ess_edges + 1);
    const size_t node_bytes = (size_t)T * N * sizeof(double), pw_bytes = (size_t)T * N * N * 2 * sizeof(double);
    if (int rc = in.alloc(h, S, nullptr, nullptr, sizeof(edges) + (n_hr + n_he) * sizeof(conv_count_t) +
                          2 * node_bytes + (pointwise ? pw_bytes : 0), 0)) return rc;
    const std::vector<double> inf_row((size_t)T * N, INFINITY);
    DevBuf bE, bHR, bHE, bNR, bNE, bPW;
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
    if (int rc = in.upload(h, Xs, intercepts, radii, S)) return rc;
    HIPCHK(h, hipMemcpyAsync(bE.p, edges, sizeof(edges), hipMemcpyHostToDevice, h->stream));
    if (G) {                      // (N = 1 has no dyads: empty histograms, the nodes keep 0 and +inf)
        DISPATCH_D(h, D, LAUNCH_DIR(directed, k_conv_accumulate, dim3((unsigned)G, (unsigned)T), dim3(IC_NT), h->stream,
                                    in.X.as<double>(), in.B.as<double>(), in.R.as<double>(), in.tiles.as<int2>(),
                                    n_tiles, L, n_segments, seg_len, batch_len, T, N, bE.as<double>(), n_rhat_edges,
                                    n_ess_edges, bHR.as<conv_count_t>(), bHE.as<conv_count_t>(), bNR.as<double>(),
                                    bNE.as<double>(), bPW.as<double>()));
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
