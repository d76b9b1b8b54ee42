// What the C-ABI's passes over posterior samples share (included by capi.hip before capi_gof.hpp): the checks of
// their inputs, and the device copies of the samples for the passes that keep all S of them resident
// (kernels_dyad_pass.hpp: capi_ic.hpp, capi_score.hpp, capi_conv.hpp).
#pragma once

namespace {

// the padding bits and the diagonal of the packed network bits [T][N][W] are zero
int check_packed_network(dlsm_chain *h, const uint32_t *bits) {
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
    return DLSM_OK;
}

// the radii [S][N] of a directed chain are positive (undirected chains have none)
int check_radii_positive(dlsm_chain *h, const double *radii, int S) {
    const size_t N = h->N;
    if (h->model != DLSM_UNDIRECTED)
        for (size_t k = 0; k < (size_t)S * N; ++k)
            if (!(radii[k] > 0.0)) FAIL(h, DLSM_E_DATA, "radii must be positive (sample %zu, node %zu)", k / N, k % N);
    return DLSM_OK;
}

// inside DISPATCH_D: kernel<DD, true> for a directed chain, kernel<DD, false> for an undirected one
#define LAUNCH_DIR(directed, kernel, grid, block, stream, ...)                                       \
    do {                                                                                             \
        if (directed) hipLaunchKernelGGL((kernel<DD, true>), grid, block, 0, stream, __VA_ARGS__);   \
        else hipLaunchKernelGGL((kernel<DD, false>), grid, block, 0, stream, __VA_ARGS__);           \
    } while (0)

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

// The inputs of a pass with all S samples resident (the accumulators of a dyad cannot be split across calls):
// the tile list, and the device copies of Xs [S][T][N][D], intercepts [S][2], radii [S][N] (directed), the
// packed network and its mask [T][N][W] (each unless NULL).  The constructor plans the tiles, on which the sizes
// of a caller's own buffers depend; alloc and upload are apart because a caller clears its outputs between them.
struct ResidentSamples {
    const bool directed;
    const std::vector<int2> host_tiles;
    const int n_tiles;
    const uint32_t *host_bits = nullptr, *host_mask = nullptr;      // what alloc was given: upload copies these
    DevBuf X, B, R, bits, mask, tiles;

    // tile_rows: the tile height of the pass; 0: IcPlan's (capi_loo.hpp has a height of its own)
    explicit ResidentSamples(dlsm_chain *h, int tile_rows = 0)
        : directed(h->model != DLSM_UNDIRECTED),
          host_tiles(ic_tiles(h->N, tile_rows ? tile_rows : h->D <= 4 ? IcPlan<1>::TI : IcPlan<8>::TI, directed)),
          n_tiles((int)host_tiles.size()) {}

    // DLSM_E_LIMIT unless the samples, the networks net and net_mask (each unless NULL), the tiles and the caller's
    // own `fixed` + S `per_sample` bytes fit into the free device memory; then the allocations
    int alloc(dlsm_chain *h, int S, const uint32_t *net, const uint32_t *net_mask, size_t fixed,
              size_t per_sample) {
        host_bits = net; host_mask = net_mask;
        const int T = h->T, N = h->N, D = h->D;
        const size_t net_bytes = (size_t)T * N * h->W * sizeof(uint32_t);
        per_sample += ((size_t)T * N * D + 2 + (directed ? N : 0)) * sizeof(double);
        fixed += ((host_bits ? 1 : 0) + (host_mask ? 1 : 0)) * net_bytes + (size_t)n_tiles * sizeof(int2) +
                 ((size_t)64 << 20);
        size_t free_b = 0, total_b = 0;
        HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
        if (fixed + (size_t)S * per_sample > free_b) {
            const long long fit = free_b > fixed ? (long long)((free_b - fixed) / per_sample) : 0;
            FAIL(h, DLSM_E_LIMIT, "S=%d samples of T=%d N=%d D=%d need %.1f MB of device memory, %.1f MB are free: "
                 "the largest S that fits is %lld", S, T, N, D, (fixed + (size_t)S * per_sample) / 1048576.0,
                 free_b / 1048576.0, fit);
        }
        HIPCHK(h, hipMalloc(&X.p, (size_t)S * T * N * D * sizeof(double)));
        HIPCHK(h, hipMalloc(&B.p, (size_t)S * 2 * sizeof(double)));
        if (directed) HIPCHK(h, hipMalloc(&R.p, (size_t)S * N * sizeof(double)));
        if (host_bits) HIPCHK(h, hipMalloc(&bits.p, net_bytes));
        if (host_mask) HIPCHK(h, hipMalloc(&mask.p, net_bytes));
        HIPCHK(h, hipMalloc(&tiles.p, std::max<size_t>(1, n_tiles) * sizeof(int2)));
        return DLSM_OK;
    }

    // the copies, on h->stream
    int upload(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii, int S) {
        const int T = h->T, N = h->N, D = h->D;
        const size_t net_bytes = (size_t)T * N * h->W * sizeof(uint32_t);
        HIPCHK(h, hipMemcpyAsync(X.p, Xs, (size_t)S * T * N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(B.p, intercepts, (size_t)S * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (directed)
            HIPCHK(h, hipMemcpyAsync(R.p, radii, (size_t)S * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (host_bits) HIPCHK(h, hipMemcpyAsync(bits.p, host_bits, net_bytes, hipMemcpyHostToDevice, h->stream));
        if (host_mask) HIPCHK(h, hipMemcpyAsync(mask.p, host_mask, net_bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(tiles.p, host_tiles.data(), (size_t)n_tiles * sizeof(int2), hipMemcpyHostToDevice,
                                 h->stream));
        return DLSM_OK;
    }
};

}  // namespace
