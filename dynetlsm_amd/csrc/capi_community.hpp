// C-ABI of the community structure of stored labellings (kernels_community.hpp); the error macros, DevArray and
// check_packed_network (capi_samples.hpp) are capi.hip's.  The reference has modularity(Y, z) alone
// (network_statistics.py:31-61), for one labelling on the host.
#pragma once
#include "capi_samples.hpp"
#include "kernels_community.hpp"

namespace {

// The excluded dyads as the kernel walks them - `mask` (or nothing) without diagonal and padding bits, on an
// undirected handle with both orientations of every listed dyad - and the in-degrees [T][N] of bits & ~mask.
// An undirected network must be symmetric.
int comm_prepare(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, std::vector<uint32_t> &eff,
                 std::vector<uint32_t> &indeg) {
    const int T = h->T, N = h->N, W = h->W;
    const bool sym = h->model == DLSM_UNDIRECTED;
    const size_t rows = (size_t)T * N;
    indeg.assign(rows, 0u);
    if (mask) {
        eff.assign(mask, mask + rows * W);
        for (size_t r = 0; r < rows; ++r) {
            uint32_t *m = eff.data() + r * W;
            const int i = (int)(r % N);
            m[i >> 5] &= ~(1u << (i & 31));
            for (int w = N >> 5; w < W; ++w) {
                const int lo = 32 * w;
                m[w] &= lo >= N ? 0u : (1u << (N - lo)) - 1u;
            }
        }
        if (sym)
            for (size_t r = 0; r < rows; ++r) {
                const size_t t0 = r / N * N;
                const int i = (int)(r % N);
                for (int w = 0; w < W; ++w)
                    for (uint32_t x = mask[r * W + w]; x; x &= x - 1) {
                        const int j = 32 * w + __builtin_ctz(x);
                        if (j < N && j != i) eff[(t0 + j) * W + (i >> 5)] |= 1u << (i & 31);
                    }
            }
    }
    for (size_t r = 0; r < rows; ++r) {
        const size_t t0 = r / N * N;
        const int i = (int)(r % N);
        for (int w = 0; w < W; ++w) {
            const uint32_t y = bits[r * W + w];
            for (uint32_t x = y; sym && x; x &= x - 1) {
                const int j = 32 * w + __builtin_ctz(x);
                if (!((bits[(t0 + j) * W + (i >> 5)] >> (i & 31)) & 1u))
                    FAIL(h, DLSM_E_DATA, "the network of an undirected handle must be symmetric (t=%d, i=%d, j=%d)",
                         (int)(r / N), i, j);
            }
            for (uint32_t x = mask ? y & ~eff[r * W + w] : y; x; x &= x - 1)
                ++indeg[t0 + 32 * w + __builtin_ctz(x)];
        }
    }
    return DLSM_OK;
}

}  // namespace

extern "C" {

int dlsm_community_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const int64_t *zs, int S,
                              int K, int batch, int64_t *clusters, int64_t *node_within, int64_t *node_switch,
                              int64_t *moved, int64_t *blocks) {
    NEED(h, h && bits && zs && clusters && node_within, "null argument");
    NEED(h, h->T == 1 || (node_switch && moved), "null argument");
    NEED(h, S >= 1, "needs at least one sample");
    NEED(h, K >= 1 && K <= 256, "n_components must be in 1..256 (labels are kept as bytes)");
    NEED(h, batch >= 0, "batch=%d is negative", batch);
    const int T = h->T, N = h->N, W = h->W, U = T - 1;
    const size_t per = (size_t)T * N;
    for (size_t q = 0; q < (size_t)S * per; ++q)
        if (zs[q] < 0 || zs[q] >= K) FAIL(h, DLSM_E_DATA, "label out of range at %zu", q);
    if (int rc = check_packed_network(h, bits)) return rc;
    std::vector<uint32_t> eff, indeg;
    if (int rc = comm_prepare(h, bits, mask, eff, indeg)) return rc;
    // the shape of the walk: the lanes of a row, the rows and the LDS of a workgroup
    int lpr = 4;
    while (lpr < 64 && lpr < W) lpr *= 2;
    const int min_chunks = (N + CM_ROWS_MAX - 1) / CM_ROWS_MAX;
    if (comm_lds_bytes(W, K, std::min(N, CM_ROWS_MAX)) > (size_t)64 * 1024)
        FAIL(h, DLSM_E_LIMIT, "N=%d: the labels of a time step do not fit a workgroup's LDS", N);
    HIPCHK(h, hipSetDevice(h->device));
    // samples per staging batch: 64 MB of int64 labels, and of the block tables when they are asked for
    size_t chunk = batch ? (size_t)batch : std::max<size_t>(1, ((size_t)64 << 20) / (per * sizeof(int64_t)));
    const size_t n_cl = (size_t)T * K * CM_SLOTS, n_bl = (size_t)T * K * K * 2;
    if (!batch && blocks) chunk = std::max<size_t>(1, std::min(chunk, ((size_t)64 << 20) / (n_bl * sizeof(int64_t))));
    chunk = std::min<size_t>(chunk, S);
    const size_t n_net = per * W;
    DevArray<int64_t> stage; DevArray<uint8_t> z8;
    DevArray<uint32_t> d_bits, d_mask, d_indeg; DevArray<cm_count_t> d_cl, d_nw, d_sw, d_mv, d_bl;
    if (stage.alloc(h, chunk * per) || z8.alloc(h, chunk * per) || d_bits.alloc(h, n_net) ||
        (mask && d_mask.alloc(h, n_net)) || d_indeg.alloc(h, per) || d_cl.alloc(h, chunk * n_cl) ||
        d_nw.alloc(h, per)) return DLSM_E_HIP;
    if (U) {
        if (d_sw.alloc(h, (size_t)U * N) || d_mv.alloc(h, chunk * U)) return DLSM_E_HIP;
        HIPCHK(h, hipMemsetAsync(d_sw, 0, (size_t)U * N * sizeof(cm_count_t), h->stream));
    }
    if (blocks) { if (int rc = d_bl.alloc(h, chunk * n_bl)) return rc; }
    HIPCHK(h, hipMemcpyAsync(d_bits, bits, n_net * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (mask) HIPCHK(h, hipMemcpyAsync(d_mask, eff.data(), n_net * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_indeg, indeg.data(), per * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(d_nw, 0, per * sizeof(cm_count_t), h->stream));
    CommArgs a;
    a.z8 = z8; a.bits = d_bits; a.mask = d_mask;
    a.indeg = d_indeg; a.T = T; a.N = N; a.W = W; a.K = K; a.lpr = lpr;
    a.clusters = d_cl; a.node_within = d_nw; a.blocks = d_bl;
    for (size_t s0 = 0; s0 < (size_t)S; s0 += chunk) {
        const int ns = (int)std::min(chunk, (size_t)S - s0);
        const size_t n_lab = (size_t)ns * per;
        HIPCHK(h, hipMemcpyAsync(stage, zs + s0 * per, n_lab * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemsetAsync(d_cl, 0, (size_t)ns * n_cl * sizeof(cm_count_t), h->stream));
        if (U) HIPCHK(h, hipMemsetAsync(d_mv, 0, (size_t)ns * U * sizeof(cm_count_t), h->stream));
        if (blocks) HIPCHK(h, hipMemsetAsync(d_bl, 0, (size_t)ns * n_bl * sizeof(cm_count_t), h->stream));
        // (some 8 workgroups per CU: sample groups first - a group re-stages N bytes per sample, a row chunk
        // flushes a cluster table per sample)
        const int target = 8 * std::max(h->n_cu, 1);
        const int groups = std::max(1, std::min(ns, (target + T - 1) / T));
        const int chunks = std::max(min_chunks, std::min((N + 63) / 64, (target + T * groups - 1) / (T * groups)));
        a.ns = ns; a.rows = (N + chunks - 1) / chunks;
        const dim3 grid((unsigned)((N + a.rows - 1) / a.rows), (unsigned)T, (unsigned)groups);
        const size_t lds = comm_lds_bytes(W, K, a.rows);
        {
            ProfScope ps(h, DLSM_K_LABELS);
            const unsigned nb = (unsigned)std::min<size_t>(4096, (n_lab + 255) / 256);
            hipLaunchKernelGGL(k_comm_pack_labels, dim3(nb), dim3(256), 0, h->stream, stage, n_lab,
                               z8);
            if (blocks) hipLaunchKernelGGL(k_comm_rows<true>, grid, dim3(CM_NT), lds, h->stream, a);
            else hipLaunchKernelGGL(k_comm_rows<false>, grid, dim3(CM_NT), lds, h->stream, a);
            if (U)
                hipLaunchKernelGGL(k_comm_switch, dim3((unsigned)((N + 255) / 256), (unsigned)U), dim3(256), 0,
                                   h->stream, z8, ns, T, N, d_sw,
                                   d_mv);
        }
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(clusters + s0 * n_cl, d_cl, (size_t)ns * n_cl * sizeof(int64_t),
                                 hipMemcpyDeviceToHost, h->stream));
        if (U) HIPCHK(h, hipMemcpyAsync(moved + s0 * U, d_mv, (size_t)ns * U * sizeof(int64_t),
                                        hipMemcpyDeviceToHost, h->stream));
        if (blocks) HIPCHK(h, hipMemcpyAsync(blocks + s0 * n_bl, d_bl, (size_t)ns * n_bl * sizeof(int64_t),
                                             hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));         // the staging buffers are reused
    }
    HIPCHK(h, hipMemcpyAsync(node_within, d_nw, per * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (U) HIPCHK(h, hipMemcpyAsync(node_switch, d_sw, (size_t)U * N * sizeof(int64_t), hipMemcpyDeviceToHost,
                                    h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
