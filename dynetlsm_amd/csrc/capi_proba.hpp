// C-ABI of the posterior edge probabilities (kernels_proba.hpp) on capi_samples.hpp's pass driver; the error macros
// are capi.hip's.  The reference has no counterpart.
#pragma once
#include "capi_samples.hpp"
#include "kernels_proba.hpp"

namespace {

// The order statistics that the interval at `level` of S samples needs: the position of the quantile q is
// (S - 1) q, as numpy's default method forms it; its floor and fraction give the two neighbours and the weight.
// The lower quantile counts its slots from the bottom, the upper one from the top.  K: the slots of a column,
// min(floor(alpha (S - 1)) + 2, S); the upper position is about S - 1 less the lower one, so its neighbours lie
// within K of the top - the max below keeps them inside the column whatever the rounding of the two products.
struct ProbaPlan { ProbaQuantile lower, upper; int K; };

ProbaPlan proba_plan(long long S, double level) {
    const double alpha = (1.0 - level) / 2.0, dS = (double)S;
    const auto position = [dS](double q) { return std::min(std::max((dS - 1.0) * q, 0.0), dS - 1.0); };
    ProbaPlan p;
    const double lo = position(alpha), hi = position(1.0 - alpha);
    const long long k0 = (long long)std::floor(lo), fh = (long long)std::floor(hi);
    p.K = (int)std::min(std::max(k0 + 2, S - fh), S);
    p.lower.prev = (int)k0;
    p.lower.next = (int)std::min(k0 + 1, S - 1);
    p.lower.g = lo - (double)k0;
    p.upper.prev = (int)(S - 1 - fh);
    p.upper.next = (int)std::max<long long>(S - 2 - fh, 0);
    p.upper.g = hi - (double)fh;
    return p;
}

// rows of a tile (wavefronts that hold dyads): the most whose two columns of K doubles per dyad fit the LDS; 0 if
// one row does not
int proba_tile_rows(long long K) {
    for (int rows = 4; rows >= 1; rows >>= 1)
        if ((size_t)(2 * K) * rows * IC_TJ * sizeof(double) <= PROBA_LDS_BUFFER_MAX) return rows;
    return 0;
}

}  // namespace

extern "C" {

int dlsm_proba_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                          const double *intercepts, const double *radii, int S, double level, int n_bins,
                          const double *width_edges, int n_edges, uint64_t *calib, uint64_t *brier,
                          uint64_t *node_sums, uint64_t *hist_width, double *pointwise) {
    if (int rc = pass_check_inputs(h, h && bits && Xs && intercepts && calib && brier && node_sums && hist_width, bits,
                                   radii, S, 2)) return rc;
    NEED(h, level > 0.0 && level < 1.0, "level=%g is not inside (0, 1)", level);
    NEED(h, n_bins >= 1 && n_bins <= PROBA_MAX_BINS, "n_bins=%d is not in 1..%d", n_bins, PROBA_MAX_BINS);
    const int T = h->T, N = h->N, D = h->D;
    double edges[PROBA_MAX_EDGES];
    static_assert(PROBA_MAX_EDGES == CONV_MAX_EDGES, "check_hist_edges pads to CONV_MAX_EDGES");
    if (int rc = check_hist_edges(h, "width_edges", width_edges, n_edges, edges)) return rc;
    if (int rc = check_fixed_point_dyads(h)) return rc;
    const ProbaPlan plan = proba_plan(S, level);
    const int K = plan.K;
    const int rows = proba_tile_rows(K);
    if (!rows) {
        long long fit = S - 1;                // the largest S below this one whose columns fit one row
        while (fit > 2 && !proba_tile_rows(proba_plan(fit, level).K)) --fit;
        FAIL(h, DLSM_E_LIMIT, "S=%d samples at level=%g need K=%d order statistics from either end: the two sorted "
             "columns of K values of 64 dyads need %zu bytes of LDS, %zu are at hand: the largest S that fits is %lld",
             S, level, K, (size_t)2 * K * IC_TJ * sizeof(double), PROBA_LDS_BUFFER_MAX, fit);
    }
    const size_t lds = (size_t)2 * K * rows * IC_TJ * sizeof(double);
    TracePass p(h, S, rows);
    const PassGrid g = pass_grid(p.n_tiles, PASS_G_MAX);
    const int iE = p.buf<double>(PROBA_MAX_EDGES, 0, edges);
    const int iCal = p.out(calib, (size_t)T * n_bins * 3, PASS_ZERO);
    const int iBr = p.out(brier, T, PASS_ZERO);
    const int iNode = p.out(node_sums, (size_t)T * N * 2, PASS_ZERO);
    const int iHist = p.out(hist_width, (size_t)T * (n_edges + 1), PASS_ZERO);
    const int iPW = p.out(pointwise, (size_t)T * N * N * 4, PASS_ZERO | PASS_OPTIONAL);
    if (int rc = p.begin(bits, mask, Xs, intercepts, radii)) return rc;
    if (g.G) {                    // (no tiles: every table stays zero)
        ProbaArgs a;
        a.Xs = p.X(); a.ic = p.B(); a.radii = p.R(); a.bits = p.bits(); a.mask = p.mask(); a.tiles = p.tiles();
        a.n_tiles = p.n_tiles; a.L = g.L; a.S = S; a.K = K; a.rows = rows; a.T = T; a.N = N; a.W = h->W;
        a.lower = plan.lower; a.upper = plan.upper;
        a.n_bins = n_bins; a.edges = p.at<double>(iE); a.n_edges = n_edges;
        a.calib = p.at<conv_count_t>(iCal); a.brier = p.at<conv_count_t>(iBr);
        a.node_sums = p.at<conv_count_t>(iNode); a.hist = p.at<conv_count_t>(iHist);
        a.pointwise = p.at<double>(iPW);
        const dim3 grid((unsigned)g.G, (unsigned)T);
        hipError_t launched = hipSuccess;
        DISPATCH_D(h, D, launched = p.directed
                       ? launch_lds(k_proba_accumulate<DD, true>, PROBA_LDS_BUFFER_MAX, grid, lds, h->stream, a)
                       : launch_lds(k_proba_accumulate<DD, false>, PROBA_LDS_BUFFER_MAX, grid, lds, h->stream, a));
        HIPCHK(h, launched);
    }
    return p.finish();
}

}  // extern "C"
