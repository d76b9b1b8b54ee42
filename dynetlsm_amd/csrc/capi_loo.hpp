// C-ABI of PSIS-LOO (kernels_loo.hpp; included by capi.hip after capi_samples.hpp, whose input checks and
// resident samples it uses, and capi_conv.hpp, whose edge check it uses).  The reference has no counterpart.
#pragma once

namespace {

// rows of a tile (wavefronts that hold dyads): the most whose sorted buffers of M + 1 doubles per dyad fit the
// LDS; 0 if one row does not
int loo_tile_rows(int M) {
    if (M < PSIS_MIN_TAIL) return 4;
    for (int rows = 4; rows >= 1; rows >>= 1)
        if ((size_t)(M + 1) * rows * IC_TJ * sizeof(double) <= LOO_LDS_BUFFER_MAX) return rows;
    return 0;
}

template <int D, bool DIR>
hipError_t loo_launch(dim3 grid, size_t lds, hipStream_t stream, const LooArgs &args) {
    hipError_t e = hipFuncSetAttribute((const void *)k_loo_accumulate<D, DIR>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)LOO_LDS_BUFFER_MAX);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_loo_accumulate<D, DIR>), grid, dim3(IC_NT), lds, stream, args);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int dlsm_loo_accumulate(dlsm_chain *h, const uint32_t *bits, const double *Xs, const double *intercepts,
                        const double *radii, int S, const double *k_edges, int n_edges, double *totals,
                        uint64_t *hist_k, double *node_k_max, double *pointwise) {
    NEED(h, h && bits && Xs && intercepts && totals && hist_k && node_k_max, "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, S >= 1, "needs at least one sample");
    const int T = h->T, N = h->N, D = h->D;
    double edges[LOO_MAX_EDGES];
    static_assert(LOO_MAX_EDGES == CONV_MAX_EDGES, "conv_check_edges pads to CONV_MAX_EDGES");
    if (int rc = conv_check_edges(h, "k_edges", k_edges, n_edges, edges)) return rc;
    if (int rc = check_packed_network(h, bits)) return rc;
    if (int rc = check_radii_positive(h, radii, S)) return rc;
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
    HIPCHK(h, hipSetDevice(h->device));
    ResidentSamples in(h, rows);
    const int n_tiles = in.n_tiles;
    const int L = (n_tiles + CONV_G_MAX - 1) / CONV_G_MAX;
    const int G = L ? (n_tiles + L - 1) / L : 0;
    const size_t n_hist = (size_t)T * (n_edges + 1);
    const size_t part_bytes = std::max<size_t>(1, (size_t)T * G * LOO_NTOT) * sizeof(double);
    const size_t tot_bytes = (size_t)T * LOO_NTOT * sizeof(double);
    const size_t node_bytes = (size_t)T * N * sizeof(double), pw_bytes = (size_t)T * N * N * 2 * sizeof(double);
    if (int rc = in.alloc(h, S, bits, nullptr, sizeof(edges) + part_bytes + tot_bytes + n_hist * sizeof(conv_count_t) +
                          node_bytes + (pointwise ? pw_bytes : 0), 0)) return rc;
    DevBuf bE, bPT, bTot, bH, bNK, bPW;
    HIPCHK(h, hipMalloc(&bE.p, sizeof(edges)));
    HIPCHK(h, hipMalloc(&bPT.p, part_bytes));
    HIPCHK(h, hipMalloc(&bTot.p, tot_bytes));
    HIPCHK(h, hipMalloc(&bH.p, n_hist * sizeof(conv_count_t)));
    HIPCHK(h, hipMalloc(&bNK.p, node_bytes));
    if (pointwise) {
        HIPCHK(h, hipMalloc(&bPW.p, pw_bytes));
        HIPCHK(h, hipMemsetAsync(bPW.p, 0, pw_bytes, h->stream));
    }
    HIPCHK(h, hipMemsetAsync(bH.p, 0, n_hist * sizeof(conv_count_t), h->stream));
    HIPCHK(h, hipMemsetAsync(bNK.p, 0, node_bytes, h->stream));
    if (int rc = in.upload(h, Xs, intercepts, radii, S)) return rc;
    HIPCHK(h, hipMemcpyAsync(bE.p, edges, sizeof(edges), hipMemcpyHostToDevice, h->stream));
    if (G) {                      // (N = 1 has no dyads: zero totals, empty histograms, the nodes keep -inf)
        LooArgs a;
        a.Xs = in.X.as<double>(); a.ic = in.B.as<double>(); a.radii = in.R.as<double>();
        a.bits = in.bits.as<uint32_t>(); a.tiles = in.tiles.as<int2>();
        a.n_tiles = n_tiles; a.L = L; a.S = S; a.M = M; a.rows = rows; a.T = T; a.N = N; a.W = h->W;
        a.edges = bE.as<double>(); a.n_edges = n_edges;
        a.part_tot = bPT.as<double>(); a.hist = bH.as<conv_count_t>(); a.node_key = bNK.as<conv_count_t>();
        a.pointwise = bPW.as<double>();
        const dim3 grid((unsigned)G, (unsigned)T);
        hipError_t launched = hipSuccess;
        DISPATCH_D(h, D, launched = directed ? loo_launch<DD, true>(grid, lds, h->stream, a)
                                             : loo_launch<DD, false>(grid, lds, h->stream, a));
        HIPCHK(h, launched);
    }
    hipLaunchKernelGGL(k_ic_reduce_totals, dim3((unsigned)T), dim3(IC_NT), 0, h->stream, bPT.as<double>(), G,
                       bTot.as<double>());
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_loo_decode_nodes, dim3((unsigned)(((size_t)T * N + IC_NT - 1) / IC_NT)), dim3(IC_NT), 0,
                       h->stream, bNK.as<conv_count_t>(), (size_t)T * N);
    HIPCHK(h, hipGetLastError());
    static_assert(sizeof(conv_count_t) == sizeof(uint64_t), "the counts are 64-bit");
    HIPCHK(h, hipMemcpyAsync(totals, bTot.p, tot_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hist_k, bH.p, n_hist * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(node_k_max, bNK.p, node_bytes, hipMemcpyDeviceToHost, h->stream));
    if (pointwise) HIPCHK(h, hipMemcpyAsync(pointwise, bPW.p, pw_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
