// C-ABI of the tie dynamics (kernels_dynamics.hpp) on capi_samples.hpp's pass driver; the error macros are
// capi.hip's.  The reference has no counterpart.
#pragma once
#include "capi_samples.hpp"
#include "kernels_dynamics.hpp"

extern "C" {

int dlsm_dynamics_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                             const double *intercepts, const double *radii, int S, int min_count, int n_bins,
                             uint64_t *transitions, uint64_t *hist_up, uint64_t *node_changes,
                             uint64_t *node_turnover, double *pointwise) {
    if (int rc = pass_check_inputs(h, h && bits && Xs && intercepts && transitions && hist_up && node_changes &&
                                   node_turnover, bits, radii, S, 2)) return rc;
    NEED(h, h->T >= 2, "a step needs two time steps, the handle has T=%d", h->T);
    NEED(h, min_count >= 1 && min_count <= S, "min_count=%d is not in 1..S=%d", min_count, S);
    NEED(h, n_bins >= 1 && n_bins <= DYN_MAX_BINS, "n_bins=%d is not in 1..%d", n_bins, DYN_MAX_BINS);
    if (int rc = check_fixed_point_dyads(h)) return rc;
    const int T = h->T, N = h->N, D = h->D;
    TracePass p(h, S);
    const PassGrid g = pass_grid(p.n_tiles, PASS_G_MAX);
    const size_t U = (size_t)T - 1;
    const int iTr = p.out(transitions, U * 16, PASS_ZERO);
    const int iHist = p.out(hist_up, U * n_bins, PASS_ZERO);
    const int iCh = p.out(node_changes, U * N * 4, PASS_ZERO);
    const int iTo = p.out(node_turnover, U * N * 2, PASS_ZERO);
    const int iPW = p.out(pointwise, U * N * N * 4, PASS_ZERO | PASS_OPTIONAL);
    if (int rc = p.begin(bits, mask, Xs, intercepts, radii)) return rc;
    if (g.G) {                    // (no tiles: every table stays zero)
        DynArgs a;
        a.Xs = p.X(); a.ic = p.B(); a.radii = p.R(); a.bits = p.bits(); a.mask = p.mask(); a.tiles = p.tiles();
        a.n_tiles = p.n_tiles; a.L = g.L; a.S = S; a.T = T; a.N = N; a.W = h->W;
        a.min_count = min_count; a.n_bins = n_bins;
        a.transitions = p.at<conv_count_t>(iTr); a.hist_up = p.at<conv_count_t>(iHist);
        a.node_changes = p.at<conv_count_t>(iCh); a.node_turnover = p.at<conv_count_t>(iTo);
        a.pointwise = p.at<double>(iPW);
        const dim3 grid((unsigned)g.G, (unsigned)U);
        DISPATCH_D(h, D, LAUNCH_DIR(p.directed, k_dyn_accumulate, grid, dim3(IC_NT), h->stream, a));
        HIPCHK(h, hipGetLastError());
    }
    return p.finish();
}

}  // extern "C"
