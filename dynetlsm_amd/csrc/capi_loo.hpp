// C-ABI of PSIS-LOO (kernels_loo.hpp; the totals are added up by kernels_ic.hpp's reduction) on capi_samples.hpp's
// pass driver; the error macros are capi.hip's.  The reference has no counterpart.
#pragma once
#include "capi_samples.hpp"
#include "kernels_ic.hpp"
#include "kernels_loo.hpp"
#include "psis_tail.hpp"

namespace {

// rows of a tile (wavefronts that hold dyads): the most whose sorted buffers of M + 1 doubles per dyad fit the
// LDS; 0 if one row does not
int loo_tile_rows(int M) {
    if (M < PSIS_MIN_TAIL) return 4;
    for (int rows = 4; rows >= 1; rows >>= 1)
        if ((size_t)(M + 1) * rows * IC_TJ * sizeof(double) <= LOO_LDS_BUFFER_MAX) return rows;
    return 0;
}

}  // namespace

extern "C" {

int dlsm_loo_accumulate(dlsm_chain *h, const uint32_t *bits, const double *Xs, const double *intercepts,
                        const double *radii, int S, const double *k_edges, int n_edges, double *totals,
                        uint64_t *hist_k, double *node_k_max, double *pointwise) {
    if (int rc = pass_check_inputs(h, h && bits && Xs && intercepts && totals && hist_k && node_k_max, bits, radii, S,
                                   1)) return rc;
    const int T = h->T, N = h->N, D = h->D;
    double edges[LOO_MAX_EDGES];
    static_assert(LOO_MAX_EDGES == CONV_MAX_EDGES, "check_hist_edges pads to CONV_MAX_EDGES");
    if (int rc = check_hist_edges(h, "k_edges", k_edges, n_edges, edges)) return rc;
    const int M = psis_tail_length(S);
    const int rows = loo_tile_rows(M);
    if (!rows) {
        long long lo = 1, hi = S;             // the largest S whose buffers fit one row: the tail length ascends
        while (lo < hi) {
            const long long mid = (lo + hi + 1) / 2;
            if (loo_tile_rows(psis_tail_length(mid))) lo = mid; else hi = mid - 1;
        }
        FAIL(h, DLSM_E_LIMIT, "S=%d samples have a tail of M=%d: the sorted buffers of M+1 values of 64 dyads need "
             "%zu bytes of LDS, %zu are at hand: the largest S that fits is %lld", S, M,
             (size_t)(M + 1) * IC_TJ * sizeof(double), LOO_LDS_BUFFER_MAX, lo);
    }
    const size_t lds = M >= PSIS_MIN_TAIL ? (size_t)(M + 1) * rows * IC_TJ * sizeof(double) : 0;
    TracePass p(h, S, rows);
    const PassGrid g = pass_grid(p.n_tiles, PASS_G_MAX);
    const size_t n_node = (size_t)T * N;
    const int iE = p.buf<double>(LOO_MAX_EDGES, 0, edges);
    const int iPT = p.buf<double>(std::max<size_t>(1, (size_t)T * g.G * LOO_NTOT));
    const int iTot = p.out(totals, (size_t)T * LOO_NTOT);
    const int iH = p.out(hist_k, (size_t)T * (n_edges + 1), PASS_ZERO);
    const int iNK = p.out(node_k_max, n_node, PASS_ZERO);      // keys on the device until k_loo_decode_nodes
    const int iPW = p.out(pointwise, (size_t)T * N * N * 2, PASS_ZERO | PASS_OPTIONAL);
    if (int rc = p.begin(bits, nullptr, Xs, intercepts, radii)) return rc;
    if (g.G) {                    // (no tiles: zero totals, empty histograms, the nodes keep -inf)
        LooArgs a;
        a.Xs = p.X(); a.ic = p.B(); a.radii = p.R(); a.bits = p.bits(); a.tiles = p.tiles();
        a.n_tiles = p.n_tiles; a.L = g.L; a.S = S; a.M = M; a.rows = rows; a.T = T; a.N = N; a.W = h->W;
        a.edges = p.at<double>(iE); a.n_edges = n_edges;
        a.part_tot = p.at<double>(iPT); a.hist = p.at<conv_count_t>(iH); a.node_key = p.at<conv_count_t>(iNK);
        a.pointwise = p.at<double>(iPW);
        const dim3 grid((unsigned)g.G, (unsigned)T);
        hipError_t launched = hipSuccess;
        DISPATCH_D(h, D, launched = p.directed
                       ? launch_lds(k_loo_accumulate<DD, true>, LOO_LDS_BUFFER_MAX, grid, lds, h->stream, a)
                       : launch_lds(k_loo_accumulate<DD, false>, LOO_LDS_BUFFER_MAX, grid, lds, h->stream, a));
        HIPCHK(h, launched);
    }
    hipLaunchKernelGGL(k_ic_reduce_totals, dim3((unsigned)T), dim3(IC_NT), 0, h->stream, p.at<double>(iPT), g.G,
                       p.at<double>(iTot));
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_loo_decode_nodes, dim3((unsigned)((n_node + IC_NT - 1) / IC_NT)), dim3(IC_NT), 0, h->stream,
                       p.at<conv_count_t>(iNK), n_node);
    HIPCHK(h, hipGetLastError());
    return p.finish();
}

}  // extern "C"
