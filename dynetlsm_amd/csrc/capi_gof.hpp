// C-ABI of the posterior predictive goodness-of-fit check (kernels_gof.hpp; included by capi.hip after
// capi_samples.hpp).  The reference has no counterpart.
#pragma once

namespace {

constexpr size_t GOF_SCRATCH_BYTES = (size_t)256 << 20;   // device scratch of one batch (auto batching)

int gof_lanes_per_row(int W) {
    int L = 1;
    while (L < W / 4 && L < 64) L <<= 1;
    return L;
}

// statistics of `nets` networks: rows (and trows, directed) [nets][N][W] on the device -> dstats
// [nets][R], zeroed here
int gof_stats_launch(dlsm_chain *h, const uint32_t *rows, const uint32_t *trows, int nets, int64_t *dstats) {
    const int N = h->N, W = h->W;
    const size_t R = 2 + 3 * (size_t)N;
    HIPCHK(h, hipMemsetAsync(dstats, 0, (size_t)nets * R * sizeof(int64_t), h->stream));
    const int nbx = std::max(1, std::min(N, 8192 / nets));
    hipLaunchKernelGGL(k_gof_stats, dim3(nbx, nets), dim3(256), 0, h->stream, rows, trows, N, W,
                       gof_lanes_per_row(W), dstats);
    HIPCHK(h, hipGetLastError());
    return DLSM_OK;
}

// the checks of the arguments every *_simulate entry point takes (after its own null checks)
int gof_simulate_check(dlsm_chain *h, const double *radii, int S, uint32_t first_index, int batch) {
    NEED(h, h->model == DLSM_UNDIRECTED || radii, "directed models need the radii");
    NEED(h, S >= 1, "needs at least one sample");
    NEED(h, batch >= 0, "batch must be >= 0 (0: automatic)");
    NEED(h, (uint64_t)first_index + (uint64_t)S <= ((uint64_t)1 << 32), "first_index + S must be <= 2^32");
    return DLSM_OK;
}

// The batch loop of every *_simulate entry point.  The S samples go to the device `nb` at a time: `batch`,
// or as many as GOF_SCRATCH_BYTES hold of networks, positions and `record_entries` int64 of records per
// sample, and no more than the grid's y extent holds networks.  Per batch of n samples from sample s0:
// upload, draw the n * T networks (k_gof_draw: a function of seed, first_index + s and t alone), enqueue
// the copy of the rows to `bits` (if given), then `stats(rows, trows, n, s0, drec)` - rows and (directed,
// else NULL) transposed rows [n * T][N][W] and drec, nb * record_entries int64, all on the device - which
// launches the statistics, copies them to the caller and returns with the stream synchronised.
template <class Stats>
int gof_simulate_batches(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii, int S,
                         uint64_t seed, uint32_t first_index, int batch, size_t record_entries, uint32_t *bits,
                         Stats &&stats) {
    const bool directed = h->model != DLSM_UNDIRECTED;
    HIPCHK(h, hipSetDevice(h->device));
    const int T = h->T, N = h->N, D = h->D, W = h->W;
    const size_t net_words = (size_t)N * W, nmat = directed ? 2 : 1;
    const size_t per_sample = (size_t)T * (net_words * nmat * sizeof(uint32_t) + (size_t)N * D * sizeof(double)) +
                              record_entries * sizeof(int64_t);
    int nb = batch > 0 ? batch : (int)std::max<size_t>(1, GOF_SCRATCH_BYTES / per_sample);
    nb = std::min(nb, S);
    nb = std::min(nb, std::max(1, 65535 / T));          // networks of a batch: the grid's y extent
    DevArray<double> bX, bB, bR; DevArray<uint32_t> bBits;
    DevArray<int64_t> bS;
    if (bX.alloc(h, (size_t)nb * T * N * D) || bB.alloc(h, (size_t)nb * 2) ||
        (directed && bR.alloc(h, (size_t)nb * N)) || bBits.alloc(h, (size_t)nb * T * net_words * nmat) ||
        bS.alloc(h, (size_t)nb * record_entries)) return DLSM_E_HIP;
    const unsigned gx = (unsigned)((net_words + 255) / 256);
    for (int s0 = 0; s0 < S; s0 += nb) {
        const int n = std::min(nb, S - s0), nets = n * T;
        HIPCHK(h, hipMemcpyAsync(bX, Xs + (size_t)s0 * T * N * D, (size_t)nets * N * D * sizeof(double),
                                 hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(bB, intercepts + 2 * (size_t)s0, (size_t)n * 2 * sizeof(double),
                                 hipMemcpyHostToDevice, h->stream));
        if (directed)
            HIPCHK(h, hipMemcpyAsync(bR, radii + (size_t)s0 * N, (size_t)n * N * sizeof(double),
                                     hipMemcpyHostToDevice, h->stream));
        DISPATCH_D(h, D, hipLaunchKernelGGL((k_gof_draw<DD>), dim3(gx, nets, (unsigned)nmat), dim3(256), 0,
                                            h->stream, bX, bB,
                                            directed ? bR.get() : nullptr, T, N, W, (int)directed,
                                            seed, first_index + (uint32_t)s0, bBits));
        HIPCHK(h, hipGetLastError());
        const uint32_t *rows = bBits;
        if (bits)
            HIPCHK(h, hipMemcpyAsync(bits + (size_t)s0 * T * net_words, rows,
                                     (size_t)nets * net_words * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                     h->stream));
        if (int rc = stats(rows, directed ? rows + (size_t)nets * net_words : nullptr, n, (size_t)s0, bS.get()))
            return rc;
    }
    return DLSM_OK;
}

}  // namespace

extern "C" {

int dlsm_gof_simulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii, int S,
                      uint64_t seed, uint32_t first_index, int batch, int64_t *stats, uint32_t *bits) {
    NEED(h, h && Xs && intercepts && stats, "null argument");
    if (int rc = gof_simulate_check(h, radii, S, first_index, batch)) return rc;
    const size_t R = 2 + 3 * (size_t)h->N, TR = (size_t)h->T * R;
    return gof_simulate_batches(h, Xs, intercepts, radii, S, seed, first_index, batch, TR, bits,
                                [&](const uint32_t *rows, const uint32_t *trows, int n, size_t s0,
                                    int64_t *drec) -> int {
        if (int rc = gof_stats_launch(h, rows, trows, n * h->T, drec)) return rc;
        HIPCHK(h, hipMemcpyAsync(stats + s0 * TR, drec, (size_t)n * TR * sizeof(int64_t), hipMemcpyDeviceToHost,
                                 h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return DLSM_OK;
    });
}

int dlsm_gof_observed(dlsm_chain *h, const uint32_t *bits, int64_t *stats) {
    NEED(h, h && bits && stats, "null argument");
    const int T = h->T, N = h->N, W = h->W;
    const size_t R = 2 + 3 * (size_t)N, net_words = (size_t)N * W;
    if (int rc = check_packed_network(h, bits)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const bool directed = h->model != DLSM_UNDIRECTED;
    DevArray<uint32_t> bBits, bT; DevArray<int64_t> bS;
    if (bBits.alloc(h, (size_t)T * net_words) || (directed && bT.alloc(h, (size_t)T * net_words)) ||
        bS.alloc(h, (size_t)T * R)) return DLSM_E_HIP;
    HIPCHK(h, hipMemcpyAsync(bBits, bits, (size_t)T * net_words * sizeof(uint32_t), hipMemcpyHostToDevice,
                             h->stream));
    if (directed) {
        hipLaunchKernelGGL(k_gof_transpose, dim3((unsigned)((net_words + 255) / 256), T), dim3(256), 0,
                           h->stream, bBits, N, W, bT);
        HIPCHK(h, hipGetLastError());
    }
    int rc = gof_stats_launch(h, bBits, directed ? bT.get() : nullptr, T,
                              bS);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(stats, bS, (size_t)T * R * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
