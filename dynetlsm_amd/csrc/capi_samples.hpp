// What the C-ABI's passes over posterior samples share: the checks of their inputs and, for the passes that keep all
// S samples resident (kernels_dyad_pass.hpp: capi_ic.hpp, capi_score.hpp, capi_conv.hpp, capi_loo.hpp,
// capi_proba.hpp, capi_dynamics.hpp), the driver that checks, allocates, fills and copies back what a pass declares.
// Includes pass_plan.hpp (the plan: plain C++) and the kernel headers whose constants it uses; the error macros are
// capi.hip's.
#pragma once
#include "kernels_conv.hpp"
#include "kernels_dyad_pass.hpp"
#include "pass_plan.hpp"

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

// a kernel of IC_NT threads that takes its arguments as one struct and `lds` bytes of dynamic LDS, lds_cap at most
template <typename Args>
hipError_t launch_lds(void (*kernel)(Args), size_t lds_cap, dim3 grid, size_t lds, hipStream_t stream,
                      const Args &args) {
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(IC_NT), lds, stream, args);
    return hipGetLastError();
}

static_assert(PASS_TJ == IC_TJ && sizeof(PassTile) == sizeof(int2), "pass_plan.hpp lists the tiles the kernels walk");
static_assert(sizeof(conv_count_t) == sizeof(uint64_t), "the counts of the C-ABI's tables are 64-bit");

// What the passes over resident samples check alike: `have_all` (the handle and every array the pass cannot do
// without), the radii of a directed chain, at least min_S (1 or 2) samples, the packed network (unless NULL) and
// the radii themselves; then the device is selected.
int pass_check_inputs(dlsm_chain *h, bool have_all, const uint32_t *net, const double *radii, int S, int min_S) {
    NEED(h, have_all, "null argument");
    NEED(h, h->model == DLSM_UNDIRECTED || radii, "directed models need the radii");
    if (min_S < 2) NEED(h, S >= 1, "needs at least one sample");
    else NEED(h, S >= 2, "needs at least two samples (the standard deviation has ddof = 1), got S=%d", S);
    if (net)
        if (int rc = check_packed_network(h, net)) return rc;
    if (int rc = check_radii_positive(h, radii, S)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return DLSM_OK;
}

// n edges of a histogram, finite and ascending, into out [CONV_MAX_EDGES] padded with +inf
int check_hist_edges(dlsm_chain *h, const char *what, const double *edges, int n, double *out) {
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

// a sum of fix(x) <= 2^32 over the dyads of a time step stays below 2^63
int check_fixed_point_dyads(dlsm_chain *h) {
    const double dyads = (double)h->N * (h->N - 1) / (h->model != DLSM_UNDIRECTED ? 1.0 : 2.0);
    if (dyads >= 2147483648.0)
        FAIL(h, DLSM_E_LIMIT, "N=%d: %.0f dyads per time step, the fixed-point sums hold fewer than 2^31", h->N, dyads);
    return DLSM_OK;
}

// A pass with all S samples resident (the accumulators of a dyad cannot be split across calls).  The constructor
// plans the tiles, on which the sizes of a pass's buffers depend; the pass then declares its buffers (buf, out),
// begin() adds the samples Xs [S][T][N][D], intercepts [S][2], radii [S][N] (directed), the packed network and its
// mask [T][N][W] (each unless NULL) and the tiles, checks the device memory, allocates every buffer on its own and
// starts them on h->stream - the pass's own ahead of the samples; after the launches finish() copies the outputs
// back and waits.
struct TracePass : PassBufs {
    dlsm_chain *const h;
    const int S;
    const bool directed;
    const std::vector<PassTile> host_tiles;
    const int n_tiles;
    int iX = -1, iB = -1, iR = -1, iBits = -1, iMask = -1, iTiles = -1;

    // tile_rows: the tile height of the pass; 0: IcPlan's
    TracePass(dlsm_chain *h_, int S_, int tile_rows = 0)
        : h(h_), S(S_), directed(h_->model != DLSM_UNDIRECTED),
          host_tiles(ic_tiles(h_->N, tile_rows ? tile_rows : h_->D <= 4 ? IcPlan<1>::TI : IcPlan<8>::TI, directed)),
          n_tiles((int)host_tiles.size()) {}
    ~TracePass() { for (PassBuf &b : list) if (b.dev) hipFree(b.dev); }

    template <typename T> int buf(size_t n, unsigned flags = 0, const void *fill = nullptr) {
        return add(sizeof(T), n, flags, fill);
    }
    template <typename T> int out(T *dest, size_t n, unsigned flags = 0, const void *fill = nullptr) {
        return output(sizeof(T), n, dest, flags, fill);
    }
    template <typename T> T *at(int id) const { return (T *)dev(id); }
    const double *X() const { return at<double>(iX); }
    const double *B() const { return at<double>(iB); }
    const double *R() const { return at<double>(iR); }
    const uint32_t *bits() const { return at<uint32_t>(iBits); }
    const uint32_t *mask() const { return at<uint32_t>(iMask); }
    const int2 *tiles() const { return at<int2>(iTiles); }

    // DLSM_E_LIMIT unless every declared buffer fits into the free device memory
    int begin(const uint32_t *net, const uint32_t *net_mask, const double *Xs, const double *intercepts,
              const double *radii) {
        const int T = h->T, N = h->N, D = h->D;
        const size_t n_net = (size_t)T * N * h->W;
        iX = buf<double>((size_t)T * N * D, PASS_PER_SAMPLE, Xs);
        iB = buf<double>(2, PASS_PER_SAMPLE, intercepts);
        if (directed) iR = buf<double>(N, PASS_PER_SAMPLE, radii);
        if (net) iBits = buf<uint32_t>(n_net, 0, net);
        if (net_mask) iMask = buf<uint32_t>(n_net, 0, net_mask);
        iTiles = buf<PassTile>(n_tiles, 0, host_tiles.data());
        size_t fixed = 0, per_sample = 0, free_b = 0, total_b = 0;
        bytes(fixed, per_sample);
        fixed += (size_t)64 << 20;            // slack
        HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
        if (fixed + (size_t)S * per_sample > free_b) {
            const long long fit = free_b > fixed ? (long long)((free_b - fixed) / per_sample) : 0;
            FAIL(h, DLSM_E_LIMIT, "S=%d samples of T=%d N=%d D=%d need %.1f MB of device memory, %.1f MB are free: "
                 "the largest S that fits is %lld", S, T, N, D, (fixed + (size_t)S * per_sample) / 1048576.0,
                 free_b / 1048576.0, fit);
        }
        for (PassBuf &b : list) HIPCHK(h, hipMalloc(&b.dev, b.total(S)));
        for (const PassBuf &b : list) {
            if (b.fill) HIPCHK(h, hipMemcpyAsync(b.dev, b.fill, b.total(S), hipMemcpyHostToDevice, h->stream));
            else if (b.flags & PASS_ZERO) HIPCHK(h, hipMemsetAsync(b.dev, 0, b.total(S), h->stream));
        }
        return DLSM_OK;
    }

    int finish() {
        for (const PassBuf *b : outputs())
            HIPCHK(h, hipMemcpyAsync(b->dest, b->dev, b->total(S), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return DLSM_OK;
    }
};

}  // namespace
