// C-ABI of the information criteria (kernels_ic.hpp; included by capi.hip after capi_gof.hpp).  The
// reference has no counterpart.
#pragma once

namespace {

constexpr size_t IC_PARTIAL_BYTES = (size_t)256 << 20;    // bound of the per-workgroup sample partials

// tiles of one time step: (row block of TI rows, column block of IC_TJ columns); undirected: those that
// hold a dyad i < j
std::vector<int2> ic_tiles(int N, int TI, bool directed) {
    std::vector<int2> tiles;
    const int nbi = (N + TI - 1) / TI, nbj = (N + IC_TJ - 1) / IC_TJ;
    for (int bi = 0; bi < nbi; ++bi)
        for (int bj = 0; bj < nbj; ++bj)
            if (directed || bi * TI < std::min(N, (bj + 1) * IC_TJ) - 1) tiles.push_back(make_int2(bi, bj));
    return tiles;
}

// what the passes over posterior samples ask of their inputs: the padding bits and the diagonal of the packed
// network are zero, the radii (directed; S * N) positive
int ic_check_inputs(dlsm_chain *h, const uint32_t *bits, const double *radii, int S) {
    const int T = h->T, N = h->N, W = h->W;
    for (size_t row = 0; row < (size_t)T * N; ++row) {
        const uint32_t *r = bits + row * W;
        const int i = (int)(row % N);
        if ((r[i >> 5] >> (i & 31)) & 1u)
            FAIL(h, DLSM_E_DATA, "network has a self-loop (t=%d, i=%d)", (int)(row / N), i);
        for (int w = N >> 5; w < W; ++w) {
            const int lo = 32 * w;
            const uint32_t pad = lo >= N ? 0xFFFFFFFFu : ~((1u << (N - lo)) - 1u);
            if (r[w] & pad) FAIL(h, DLSM_E_DATA, "padding bits beyond column N-1 must be zero");
        }
    }
    if (h->model != DLSM_UNDIRECTED)
        for (size_t k = 0; k < (size_t)S * N; ++k)
            if (!(radii[k] > 0.0)) FAIL(h, DLSM_E_DATA, "radii must be positive (sample %zu, node %zu)", k / N, k % N);
    return DLSM_OK;
}

template <int D>
void ic_launch(dlsm_chain *h, bool directed, dim3 grid, const double *Xs, const double *ic, const double *radii,
               const uint32_t *bits, const int2 *tiles, int n_tiles, int L, int S, double *part_tot,
               double *part_s, double *pointwise) {
    if (directed)
        hipLaunchKernelGGL((k_ic_accumulate<D, true>), grid, dim3(IC_NT), 0, h->stream, Xs, ic, radii, bits, tiles,
                           n_tiles, L, S, h->T, h->N, h->W, part_tot, part_s, pointwise);
    else
        hipLaunchKernelGGL((k_ic_accumulate<D, false>), grid, dim3(IC_NT), 0, h->stream, Xs, ic, radii, bits, tiles,
                           n_tiles, L, S, h->T, h->N, h->W, part_tot, part_s, pointwise);
}

}  // namespace

extern "C" {

int dlsm_ic_accumulate(dlsm_chain *h, const uint32_t *bits, const double *Xs, const double *intercepts,
                       const double *radii, int S, double *totals, double *sample_loglik, double *pointwise) {
    NEED(h, h && bits && Xs && intercepts && totals && sample_loglik, "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, S >= 1, "needs at least one sample");
    const int T = h->T, N = h->N, D = h->D, W = h->W;
    const size_t net_words = (size_t)N * W;
    if (int rc = ic_check_inputs(h, bits, radii, S)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const int TI = D <= 4 ? IcPlan<1>::TI : IcPlan<8>::TI;
    const std::vector<int2> tiles = ic_tiles(N, TI, directed);
    const int n_tiles = (int)tiles.size();
    // tiles per workgroup: as few as keep the sample partials [T][G][S] within IC_PARTIAL_BYTES
    const size_t one = (size_t)T * S * sizeof(double);
    const size_t g_max = std::max<size_t>(1, IC_PARTIAL_BYTES / one);
    const int L = (int)(((size_t)n_tiles + g_max - 1) / g_max);
    const int G = (n_tiles + L - 1) / L;
    // all S samples are resident: the accumulators of a dyad cannot be split across calls
    const size_t per_sample = ((size_t)T * N * D + 2 + (directed ? N : 0)) * sizeof(double) +
                              (size_t)T * G * sizeof(double);
    const size_t fixed = (size_t)T * net_words * sizeof(uint32_t) + (size_t)n_tiles * sizeof(int2) +
                         (size_t)T * G * IC_NTOT * sizeof(double) + (size_t)T * IC_NTOT * sizeof(double) +
                         (pointwise ? (size_t)T * N * N * 2 * sizeof(double) : 0) + ((size_t)64 << 20);
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    if (fixed + (size_t)S * per_sample > free_b) {
        const long long fit = free_b > fixed ? (long long)((free_b - fixed) / per_sample) : 0;
        FAIL(h, DLSM_E_LIMIT, "S=%d samples of T=%d N=%d D=%d need %.1f MB of device memory, %.1f MB are free: "
             "the largest S that fits is %lld", S, T, N, D, (fixed + (size_t)S * per_sample) / 1048576.0,
             free_b / 1048576.0, fit);
    }
    DevBuf bX, bB, bR, bBits, bTiles, bPT, bPS, bTot, bSL, bPW;
    HIPCHK(h, hipMalloc(&bX.p, (size_t)S * T * N * D * sizeof(double)));
    HIPCHK(h, hipMalloc(&bB.p, (size_t)S * 2 * sizeof(double)));
    if (directed) HIPCHK(h, hipMalloc(&bR.p, (size_t)S * N * sizeof(double)));
    HIPCHK(h, hipMalloc(&bBits.p, (size_t)T * net_words * sizeof(uint32_t)));
    HIPCHK(h, hipMalloc(&bTiles.p, (size_t)n_tiles * sizeof(int2)));
    HIPCHK(h, hipMalloc(&bPT.p, (size_t)T * G * IC_NTOT * sizeof(double)));
    HIPCHK(h, hipMalloc(&bPS.p, (size_t)T * G * S * sizeof(double)));
    HIPCHK(h, hipMalloc(&bTot.p, (size_t)T * IC_NTOT * sizeof(double)));
    HIPCHK(h, hipMalloc(&bSL.p, (size_t)S * T * sizeof(double)));
    if (pointwise) {
        HIPCHK(h, hipMalloc(&bPW.p, (size_t)T * N * N * 2 * sizeof(double)));
        HIPCHK(h, hipMemsetAsync(bPW.p, 0, (size_t)T * N * N * 2 * sizeof(double), h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(bX.p, Xs, (size_t)S * T * N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bB.p, intercepts, (size_t)S * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (directed)
        HIPCHK(h, hipMemcpyAsync(bR.p, radii, (size_t)S * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bBits.p, bits, (size_t)T * net_words * sizeof(uint32_t), hipMemcpyHostToDevice,
                             h->stream));
    HIPCHK(h, hipMemcpyAsync(bTiles.p, tiles.data(), (size_t)n_tiles * sizeof(int2), hipMemcpyHostToDevice,
                             h->stream));
    DISPATCH_D(h, D, ic_launch<DD>(h, directed, dim3((unsigned)G, (unsigned)T), bX.as<double>(), bB.as<double>(),
                                   directed ? bR.as<double>() : nullptr, bBits.as<uint32_t>(), bTiles.as<int2>(),
                                   n_tiles, L, S, bPT.as<double>(), bPS.as<double>(),
                                   pointwise ? bPW.as<double>() : nullptr));
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_ic_reduce_totals, dim3((unsigned)T), dim3(IC_NT), 0, h->stream, bPT.as<double>(), G,
                       bTot.as<double>());
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_ic_reduce_samples, dim3((unsigned)((S + 63) / 64), (unsigned)T), dim3(IC_NT), 0, h->stream,
                       bPS.as<double>(), G, S, T, bSL.as<double>());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(totals, bTot.p, (size_t)T * IC_NTOT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(sample_loglik, bSL.p, (size_t)S * T * sizeof(double), hipMemcpyDeviceToHost,
                             h->stream));
    if (pointwise)
        HIPCHK(h, hipMemcpyAsync(pointwise, bPW.p, (size_t)T * N * N * 2 * sizeof(double), hipMemcpyDeviceToHost,
                                 h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
