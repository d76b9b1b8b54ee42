// C-ABI of the posterior edge probabilities (kernels_proba.hpp; included by capi.hip after capi_samples.hpp, whose
// input checks and resident samples it uses, and capi_conv.hpp, whose edge check it uses).  The reference has no
// counterpart.
#pragma once

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

template <int D, bool DIR>
hipError_t proba_launch(dim3 grid, size_t lds, hipStream_t stream, const ProbaArgs &args) {
    hipError_t e = hipFuncSetAttribute((const void *)k_proba_accumulate<D, DIR>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)PROBA_LDS_BUFFER_MAX);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_proba_accumulate<D, DIR>), grid, dim3(IC_NT), lds, stream, args);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int dlsm_proba_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                          const double *intercepts, const double *radii, int S, double level, int n_bins,
                          const double *width_edges, int n_edges, uint64_t *calib, uint64_t *brier,
                          uint64_t *node_sums, uint64_t *hist_width, double *pointwise) {
    NEED(h, h && bits && Xs && intercepts && calib && brier && node_sums && hist_width, "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, S >= 2, "needs at least two samples (the standard deviation has ddof = 1), got S=%d", S);
    NEED(h, level > 0.0 && level < 1.0, "level=%g is not inside (0, 1)", level);
    NEED(h, n_bins >= 1 && n_bins <= PROBA_MAX_BINS, "n_bins=%d is not in 1..%d", n_bins, PROBA_MAX_BINS);
    const int T = h->T, N = h->N, D = h->D;
    double edges[PROBA_MAX_EDGES];
    static_assert(PROBA_MAX_EDGES == CONV_MAX_EDGES, "conv_check_edges pads to CONV_MAX_EDGES");
    if (int rc = conv_check_edges(h, "width_edges", width_edges, n_edges, edges)) return rc;
    if (int rc = check_packed_network(h, bits)) return rc;
    if (int rc = check_radii_positive(h, radii, S)) return rc;
    // a sum of fix(x) <= 2^32 over the dyads of a time step stays below 2^63
    const double dyads = (double)N * (N - 1) / (directed ? 1.0 : 2.0);
    if (dyads >= 2147483648.0)
        FAIL(h, DLSM_E_LIMIT, "N=%d: %.0f dyads per time step, the fixed-point sums hold fewer than 2^31", N, dyads);
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
    HIPCHK(h, hipSetDevice(h->device));
    ResidentSamples in(h, rows);
    const int n_tiles = in.n_tiles;
    const int L = (n_tiles + CONV_G_MAX - 1) / CONV_G_MAX;
    const int G = L ? (n_tiles + L - 1) / L : 0;
    static_assert(sizeof(conv_count_t) == sizeof(uint64_t), "the counts are 64-bit");
    // one buffer of counters: calib, brier, node_sums, hist_width
    const size_t n_cal = (size_t)T * n_bins * 3, n_br = (size_t)T, n_node = (size_t)T * N * 2;
    const size_t n_hist = (size_t)T * (n_edges + 1), n_cnt = n_cal + n_br + n_node + n_hist;
    const size_t pw_bytes = (size_t)T * N * N * 4 * sizeof(double);
    if (int rc = in.alloc(h, S, bits, mask, sizeof(edges) + n_cnt * sizeof(conv_count_t) +
                          (pointwise ? pw_bytes : 0), 0)) return rc;
    DevBuf bE, bC, bPW;
    HIPCHK(h, hipMalloc(&bE.p, sizeof(edges)));
    HIPCHK(h, hipMalloc(&bC.p, n_cnt * sizeof(conv_count_t)));
    if (pointwise) {
        HIPCHK(h, hipMalloc(&bPW.p, pw_bytes));
        HIPCHK(h, hipMemsetAsync(bPW.p, 0, pw_bytes, h->stream));
    }
    HIPCHK(h, hipMemsetAsync(bC.p, 0, n_cnt * sizeof(conv_count_t), h->stream));
    if (int rc = in.upload(h, Xs, intercepts, radii, S)) return rc;
    HIPCHK(h, hipMemcpyAsync(bE.p, edges, sizeof(edges), hipMemcpyHostToDevice, h->stream));
    conv_count_t *cnt = bC.as<conv_count_t>();
    if (G) {                      // (N = 1 has no dyads: every table stays zero)
        ProbaArgs a;
        a.Xs = in.X.as<double>(); a.ic = in.B.as<double>(); a.radii = in.R.as<double>();
        a.bits = in.bits.as<uint32_t>(); a.mask = in.mask.as<uint32_t>(); a.tiles = in.tiles.as<int2>();
        a.n_tiles = n_tiles; a.L = L; a.S = S; a.K = K; a.rows = rows; a.T = T; a.N = N; a.W = h->W;
        a.lower = plan.lower; a.upper = plan.upper;
        a.n_bins = n_bins; a.edges = bE.as<double>(); a.n_edges = n_edges;
        a.calib = cnt; a.brier = cnt + n_cal; a.node_sums = a.brier + n_br; a.hist = a.node_sums + n_node;
        a.pointwise = bPW.as<double>();
        const dim3 grid((unsigned)G, (unsigned)T);
        hipError_t launched = hipSuccess;
        DISPATCH_D(h, D, launched = directed ? proba_launch<DD, true>(grid, lds, h->stream, a)
                                             : proba_launch<DD, false>(grid, lds, h->stream, a));
        HIPCHK(h, launched);
    }
    HIPCHK(h, hipMemcpyAsync(calib, cnt, n_cal * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(brier, cnt + n_cal, n_br * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(node_sums, cnt + n_cal + n_br, n_node * sizeof(uint64_t), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipMemcpyAsync(hist_width, cnt + n_cal + n_br + n_node, n_hist * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, h->stream));
    if (pointwise) HIPCHK(h, hipMemcpyAsync(pointwise, bPW.p, pw_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
