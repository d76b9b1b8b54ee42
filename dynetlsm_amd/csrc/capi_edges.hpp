// C-ABI of the edge-list upload (kernels_edges.hpp; included by capi.hip).  Stands for the float64 upload of
// lsm.py:341 and, on case-control chains, for the host loops of case_control_likelihood.py:45-68: a sparse
// network reaches the chain as its list of ties, never as T x N x N values.
#pragma once
#include "kernels_edges.hpp"

namespace {

// the pairs of time step t into the two zeroed [N][W] arrays (enqueued; nothing for an empty step)
void enqueue_scatter(dlsm_chain *h, const int32_t *d_src, const int32_t *d_dst, const int64_t *offsets, int t,
                     uint32_t *rows, uint32_t *cols, int *dflag) {
    const long n = (long)(offsets[t + 1] - offsets[t]);
    if (n <= 0) return;
    const long nblk = std::min<long>((n + EDGES_THREADS - 1) / EDGES_THREADS, EDGES_MAX_BLOCKS);
    hipLaunchKernelGGL(k_edges_scatter, dim3((unsigned)nblk), dim3(EDGES_THREADS), 0, h->stream, d_src + offsets[t],
                       d_dst + offsets[t], n, h->N, h->W, rows, cols, dflag);
}

int edges_flag_error(dlsm_chain *h, int flag) {
    FAIL(h, DLSM_E_DATA, "edge list violates the layout (code %d: %d a node index outside 0..%d, %d src == dst)",
         flag, EDGE_BAD_INDEX, h->N - 1, EDGE_SELF_LOOP);
}

// undirected / directed chains: ybits (and ytbits) and the column-major copy, as dlsm_upload_network leaves them
int edges_to_packed(dlsm_chain *h, const int32_t *d_src, const int32_t *d_dst, const int64_t *offsets, int *dflag) {
    const size_t slice = (size_t)h->N * h->W, words = (size_t)h->T * slice;
    const bool directed = h->model == DLSM_DIRECTED;
    if (!h->ybits) { int rc = h->ybits.alloc(h, words); if (rc) return rc; }
    if (directed && !h->ytbits) { int rc = h->ytbits.alloc(h, words); if (rc) return rc; }
    HIPCHK(h, hipMemsetAsync(h->ybits, 0, words * sizeof(uint32_t), h->stream));
    if (directed) HIPCHK(h, hipMemsetAsync(h->ytbits, 0, words * sizeof(uint32_t), h->stream));
    for (int t = 0; t < h->T; ++t)
        enqueue_scatter(h, d_src, d_dst, offsets, t, h->ybits + t * slice,
                        (directed ? h->ytbits : h->ybits) + t * slice, dflag);
    HIPCHK(h, hipGetLastError());
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (flag) return edges_flag_error(h, flag);
    { int rc = build_colmajor(h); if (rc) return rc; }
    h->have_network = true;
    h->have_hops = false;
    return DLSM_OK;
}

// case-control chains: degree, in_edges, out_edges and their widths, as build_edge_lists + dlsm_upload_edges leave
// them.  The chain keeps no packed network, so the two bit arrays are temporaries of one time step (2 N W words),
// filled twice: once for the degrees - the tables' widths are their maxima -, once for the emit.
int edges_to_tables(dlsm_chain *h, const int32_t *d_src, const int32_t *d_dst, const int64_t *offsets, int *dflag) {
    const size_t slice = (size_t)h->N * h->W, TN = (size_t)h->T * h->N;
    DevArray<uint32_t> bits;            // [2][N][W]: rows, then columns
    DevArray<int> dmax;
    if (bits.alloc(h, 2 * slice) || dmax.alloc(h, 2)) return DLSM_E_HIP;
    { int rc = h->degree.alloc(h, TN * 2); if (rc) return rc; }
    uint32_t *rows = bits, *cols = bits + slice;
    const dim3 row_grid((unsigned)((h->N + ROWS_WAVES - 1) / ROWS_WAVES));
    HIPCHK(h, hipMemsetAsync(dmax, 0, 2 * sizeof(int), h->stream));
    for (int t = 0; t < h->T; ++t) {
        HIPCHK(h, hipMemsetAsync(bits, 0, 2 * slice * sizeof(uint32_t), h->stream));
        enqueue_scatter(h, d_src, d_dst, offsets, t, rows, cols, dflag);
        hipLaunchKernelGGL(k_rows_degree, row_grid, dim3(64 * ROWS_WAVES), 0, h->stream, rows, cols, h->N, h->W,
                           h->degree + (size_t)t * h->N * 2, dmax);
    }
    HIPCHK(h, hipGetLastError());
    int flag = 0, width[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(width, dmax, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (flag) return edges_flag_error(h, flag);
    const int Din = width[0], Dout = width[1];
    { int rc = h->in_edges.alloc(h, TN * Din); if (rc) return rc; }
    { int rc = h->out_edges.alloc(h, TN * Dout); if (rc) return rc; }
    HIPCHK(h, hipMemsetAsync(h->in_edges, 0, TN * Din * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(h->out_edges, 0, TN * Dout * sizeof(int32_t), h->stream));
    for (int t = 0; t < h->T; ++t) {
        if (offsets[t + 1] == offsets[t]) continue;     // (no ties: the step's rows stay padding)
        HIPCHK(h, hipMemsetAsync(bits, 0, 2 * slice * sizeof(uint32_t), h->stream));
        enqueue_scatter(h, d_src, d_dst, offsets, t, rows, cols, dflag);
        hipLaunchKernelGGL(k_rows_emit, dim3(row_grid.x, 2), dim3(64 * ROWS_WAVES), 0, h->stream, rows, cols, h->N,
                           h->W, h->in_edges + (size_t)t * h->N * Din, Din, h->out_edges + (size_t)t * h->N * Dout,
                           Dout);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));         // (the temporaries go when this returns)
    h->Din = Din; h->Dout = Dout;
    h->have_edges = true;
    h->cc_terms_valid = false;
    return DLSM_OK;
}

}  // namespace

extern "C" {

int dlsm_upload_network_edges(dlsm_chain *h, const int64_t *offsets, const int32_t *src, const int32_t *dst) {
    NEED(h, h && offsets, "null argument");
    drop_graph(h);
    // a failed call leaves the chain without a network or edges, never new contents behind old strides
    // (dlsm_upload_edges): whatever the chain held is gone from here on
    h->have_network = false; h->have_hops = false; h->have_edges = false;
    NEED(h, offsets[0] == 0, "offsets[0] = %lld, must be 0", (long long)offsets[0]);
    for (int t = 0; t < h->T; ++t)
        NEED(h, offsets[t + 1] >= offsets[t], "offsets decrease at time step %d (%lld after %lld)", t,
             (long long)offsets[t + 1], (long long)offsets[t]);
    const size_t n = (size_t)offsets[h->T];
    NEED(h, n == 0 || (src && dst), "null edge arrays");
    HIPCHK(h, hipSetDevice(h->device));
    DevArray<int32_t> d_src, d_dst;
    DevArray<int> dflag;
    if (d_src.alloc(h, n) || d_dst.alloc(h, n) || dflag.alloc(h, 1)) return DLSM_E_HIP;
    HIPCHK(h, hipMemsetAsync(dflag, 0, sizeof(int), h->stream));
    if (n) {
        HIPCHK(h, hipMemcpyAsync(d_src, src, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_dst, dst, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    }
    const int rc = h->model == DLSM_DIRECTED_CASE_CONTROL ? edges_to_tables(h, d_src, d_dst, offsets, dflag)
                                                          : edges_to_packed(h, d_src, d_dst, offsets, dflag);
    // (the staged lists are freed on return: nothing may still read them)
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) FAIL(h, DLSM_E_HIP, "hipStreamSynchronize failed");
    return rc;
}

int dlsm_edge_table_widths(dlsm_chain *h, int *Din, int *Dout) {
    NEED(h, h && Din && Dout, "null argument");
    NEED(h, h->model == DLSM_DIRECTED_CASE_CONTROL, "not a case-control chain");
    NEED(h, h->have_edges, "edge lists not uploaded");
    *Din = h->Din; *Dout = h->Dout;
    return DLSM_OK;
}

int dlsm_get_edges(dlsm_chain *h, int64_t *in_edges, int64_t *out_edges, int64_t *degree) {
    NEED(h, h && in_edges && out_edges && degree, "null argument");
    NEED(h, h->model == DLSM_DIRECTED_CASE_CONTROL, "not a case-control chain");
    NEED(h, h->have_edges, "edge lists not uploaded");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t TN = (size_t)h->T * h->N;
    const struct { int64_t *to; const int32_t *from; size_t n; } parts[] = {
        {in_edges, h->in_edges, TN * h->Din}, {out_edges, h->out_edges, TN * h->Dout}, {degree, h->degree, TN * 2}};
    std::vector<int32_t> tmp;
    for (const auto &p : parts) {
        if (!p.n) continue;
        tmp.resize(p.n);
        int rc = d2h(h, tmp.data(), p.from, p.n); if (rc) return rc;
        for (size_t k = 0; k < p.n; ++k) p.to[k] = tmp[k];
    }
    return DLSM_OK;
}

}  // extern "C"
