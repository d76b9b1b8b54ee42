// C-ABI of the triad census of drawn and observed networks (kernels_gof_triads.hpp; included by capi.hip
// after capi_gof.hpp, whose checks, batch loop and lane choice it shares).  The reference has no counterpart.
#pragma once

namespace {

// records of `nets` networks: rows (and trows, directed; else NULL) [nets][N][W] on the device -> drec
// [nets][GOF_TRIAD_R], zeroed here
int gof_triads_launch(dlsm_chain *h, const uint32_t *rows, const uint32_t *trows, int nets, int64_t *drec) {
    const int N = h->N, W = h->W;
    HIPCHK(h, hipMemsetAsync(drec, 0, (size_t)nets * GOF_TRIAD_R * sizeof(int64_t), h->stream));
    const dim3 grid(std::max(1, std::min(N, 8192 / nets)), nets);
    if (trows)
        hipLaunchKernelGGL(k_gof_triads<true>, grid, dim3(256), 0, h->stream, rows, trows, N, W,
                           gof_lanes_per_row(W), drec);
    else
        hipLaunchKernelGGL(k_gof_triads<false>, grid, dim3(256), 0, h->stream, rows, trows, N, W,
                           gof_lanes_per_row(W), drec);
    HIPCHK(h, hipGetLastError());
    return DLSM_OK;
}

}  // namespace

extern "C" {

int dlsm_gof_triads_simulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii,
                             int S, uint64_t seed, uint32_t first_index, int batch, int64_t *triads,
                             uint32_t *bits) {
    NEED(h, h && Xs && intercepts && triads, "null argument");
    if (int rc = gof_simulate_check(h, radii, S, first_index, batch)) return rc;
    const size_t TR = (size_t)h->T * GOF_TRIAD_R;
    return gof_simulate_batches(h, Xs, intercepts, radii, S, seed, first_index, batch, TR, bits,
                                [&](const uint32_t *rows, const uint32_t *trows, int n, size_t s0,
                                    int64_t *drec) -> int {
        if (int rc = gof_triads_launch(h, rows, trows, n * h->T, drec)) return rc;
        HIPCHK(h, hipMemcpyAsync(triads + s0 * TR, drec, (size_t)n * TR * sizeof(int64_t), hipMemcpyDeviceToHost,
                                 h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return DLSM_OK;
    });
}

int dlsm_gof_triads_observed(dlsm_chain *h, const uint32_t *bits, int64_t *triads) {
    NEED(h, h && bits && triads, "null argument");
    const int T = h->T, N = h->N, W = h->W;
    const size_t net_words = (size_t)N * W;
    if (int rc = check_packed_network(h, bits)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const bool directed = h->model != DLSM_UNDIRECTED;
    DevArray<uint32_t> bBits, bT; DevArray<int64_t> bS;
    if (bBits.alloc(h, (size_t)T * net_words) || (directed && bT.alloc(h, (size_t)T * net_words)) ||
        bS.alloc(h, (size_t)T * GOF_TRIAD_R)) return DLSM_E_HIP;
    HIPCHK(h, hipMemcpyAsync(bBits, bits, (size_t)T * net_words * sizeof(uint32_t), hipMemcpyHostToDevice,
                             h->stream));
    if (directed) {
        hipLaunchKernelGGL(k_gof_transpose, dim3((unsigned)((net_words + 255) / 256), T), dim3(256), 0,
                           h->stream, bBits, N, W, bT);
        HIPCHK(h, hipGetLastError());
    }
    if (int rc = gof_triads_launch(h, bBits, directed ? bT.get() : nullptr, T, bS)) return rc;
    HIPCHK(h, hipMemcpyAsync(triads, bS, (size_t)T * GOF_TRIAD_R * sizeof(int64_t), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
