// C-ABI of the per-dyad convergence diagnostics (kernels_conv.hpp) on capi_samples.hpp's pass driver; the error
// macros are capi.hip's.  The reference has no counterpart.
#pragma once
#include "capi_samples.hpp"
#include "kernels_conv.hpp"

extern "C" {

int dlsm_convergence_accumulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii,
                                int n_segments, int seg_len, int batch_len, const double *rhat_edges,
                                int n_rhat_edges, const double *ess_edges, int n_ess_edges, uint64_t *hist_rhat,
                                uint64_t *hist_ess, double *node_rhat_max, double *node_ess_min, double *pointwise) {
    NEED(h, n_segments >= 2 && n_segments % 2 == 0, "n_segments=%d: the halves of the chains, an even number >= 2",
         n_segments);
    NEED(h, seg_len >= 2, "seg_len=%d: a segment needs at least two samples", seg_len);
    NEED(h, batch_len >= 1 && batch_len <= seg_len / 2, "batch_len=%d: between 1 and seg_len / 2 = %d", batch_len,
         seg_len / 2);
    NEED(h, (long long)n_segments * seg_len <= 0x7FFFFFFFLL, "too many samples");
    const int S = n_segments * seg_len;
    if (int rc = pass_check_inputs(h, h && Xs && intercepts && hist_rhat && hist_ess && node_rhat_max && node_ess_min,
                                   nullptr, radii, S, 1)) return rc;
    const int T = h->T, N = h->N, D = h->D;
    double edges[2 * CONV_MAX_EDGES];
    if (int rc = check_hist_edges(h, "rhat_edges", rhat_edges, n_rhat_edges, edges)) return rc;
    if (int rc = check_hist_edges(h, "ess_edges", ess_edges, n_ess_edges, edges + CONV_MAX_EDGES)) return rc;
    TracePass p(h, S);
    const PassGrid g = pass_grid(p.n_tiles, PASS_G_MAX);
    const std::vector<double> inf_row((size_t)T * N, INFINITY);
    const int iE = p.buf<double>(2 * CONV_MAX_EDGES, 0, edges);
    const int iHR = p.out(hist_rhat, (size_t)T * (n_rhat_edges + 1), PASS_ZERO);
    const int iHE = p.out(hist_ess, (size_t)T * (n_ess_edges + 1), PASS_ZERO);
    const int iNR = p.out(node_rhat_max, inf_row.size(), PASS_ZERO);
    const int iNE = p.out(node_ess_min, inf_row.size(), 0, inf_row.data());
    const int iPW = p.out(pointwise, (size_t)T * N * N * 2, PASS_ZERO | PASS_OPTIONAL);
    if (int rc = p.begin(nullptr, nullptr, Xs, intercepts, radii)) return rc;
    if (g.G) {                    // (no tiles: empty histograms, the nodes keep 0 and +inf)
        DISPATCH_D(h, D, LAUNCH_DIR(p.directed, k_conv_accumulate, dim3((unsigned)g.G, (unsigned)T), dim3(IC_NT),
                                    h->stream, p.X(), p.B(), p.R(), p.tiles(), p.n_tiles, g.L, n_segments, seg_len,
                                    batch_len, T, N, p.at<double>(iE), n_rhat_edges, n_ess_edges,
                                    p.at<conv_count_t>(iHR), p.at<conv_count_t>(iHE), p.at<double>(iNR),
                                    p.at<double>(iNE), p.at<double>(iPW)));
        HIPCHK(h, hipGetLastError());
    }
    return p.finish();
}

}  // extern "C"
