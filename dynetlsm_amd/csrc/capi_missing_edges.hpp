// C-ABI of the missing dyads given as lists (kernels_missing_edges.hpp; included by capi.hip behind capi_edges.hpp,
// whose scatter it shares).  Stands for the nan mask of lsm.py:345-359 as the imputation step of lsm.py:525-545
// reads it: what dlsm_set_missing builds from canonical (t, i, j) rows with a host sort, built on the device from
// pairs in any order and orientation.
#pragma once
#include "kernels_missing_edges.hpp"

namespace {

int miss_edges_flag_error(dlsm_chain *h, int flag) {
    FAIL(h, DLSM_E_DATA, "missing list violates the layout (code %d: %d a node index outside 0..%d, %d src == dst, "
         "%d a listed dyad is an observed tie)", flag, EDGE_BAD_INDEX, h->N - 1, EDGE_SELF_LOOP, MISS_TIE_LISTED);
}

// The tables of dlsm_set_missing for the set of listed dyads.  Two passes over the time steps, each scattering the
// step's list into the temporaries again (edges_to_tables): the counts, then - the T * nz * N counts summed on the
// host, which has to learn the sizes for the allocations anyway - the emit.
int miss_edges_build(dlsm_chain *h, const int64_t *offsets, const int32_t *src, const int32_t *dst, int allow_ties) {
    NEED(h, h->model != DLSM_DIRECTED_CASE_CONTROL, "case-control chains hold edge lists: no dyads to impute");
    NEED(h, offsets[0] == 0, "offsets[0] = %lld, must be 0", (long long)offsets[0]);
    for (int t = 0; t < h->T; ++t)
        NEED(h, offsets[t + 1] >= offsets[t], "offsets decrease at time step %d (%lld after %lld)", t,
             (long long)offsets[t + 1], (long long)offsets[t]);
    const size_t n_listed = (size_t)offsets[h->T];
    NEED(h, n_listed == 0 || (src && dst), "null pair arrays");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    miss_free(h);
    h->miss_on = false;
    if (n_listed == 0) return DLSM_OK;
    NEED(h, h->have_network, "network not uploaded");
    if (h->N >= MISS_N_MAX) FAIL(h, DLSM_E_LIMIT, "N=%d: the draws' counters hold node indices below 2^24", h->N);

    const bool directed = h->model == DLSM_DIRECTED;
    const int nz = directed ? 2 : 1, N = h->N, W = h->W;
    const size_t slice = (size_t)N * W, rows_all = (size_t)h->T * nz * N;
    DevArray<int32_t> d_src, d_dst, d_cnt, d_own;
    DevArray<uint32_t> bits;            // [nz][N][W]: forward, then (directed) transposed
    DevArray<int> dflag;
    if (d_src.alloc(h, n_listed) || d_dst.alloc(h, n_listed) || d_cnt.alloc(h, rows_all) ||
        d_own.alloc(h, rows_all) || bits.alloc(h, nz * slice) || dflag.alloc(h, 1)) return DLSM_E_HIP;
    uint32_t *fwd = bits, *bwd = bits + (nz - 1) * slice;
    HIPCHK(h, hipMemsetAsync(dflag, 0, sizeof(int), h->stream));
    HIPCHK(h, hipMemsetAsync(d_cnt, 0, rows_all * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d_own, 0, rows_all * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemcpyAsync(d_src, src, n_listed * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_dst, dst, n_listed * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    const unsigned row_blocks = (unsigned)((N + ROWS_WAVES - 1) / ROWS_WAVES);
    for (int t = 0; t < h->T; ++t) {
        if (offsets[t + 1] == offsets[t]) continue;
        HIPCHK(h, hipMemsetAsync(bits, 0, nz * slice * sizeof(uint32_t), h->stream));
        enqueue_scatter(h, d_src, d_dst, offsets, t, fwd, bwd, dflag);
        hipLaunchKernelGGL(k_miss_rows_count, dim3(row_blocks, nz), dim3(64 * ROWS_WAVES), 0, h->stream, fwd, bwd,
                           allow_ties ? (const uint32_t *)nullptr : h->ybits + t * slice, N, W, directed ? 0 : 1,
                           d_cnt + (size_t)t * nz * N, d_own + (size_t)t * nz * N, dflag);
    }
    HIPCHK(h, hipGetLastError());
    int flag = 0;
    std::vector<int32_t> cnt(rows_all), own(rows_all);
    HIPCHK(h, hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(cnt.data(), d_cnt, rows_all * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(own.data(), d_own, rows_all * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (flag) return miss_edges_flag_error(h, flag);

    // exclusive sums over the (2 t + matrix, row) sequence: entry offsets, slot bases, the non-empty rows as jobs
    std::vector<int32_t> jobs, slot0;
    std::vector<int> job_lo(h->T + 1, 0);
    int64_t entries = 0, n = 0;
    for (int t = 0; t < h->T; ++t) {
        for (int z = 0; z < nz; ++z)
            for (int i = 0; i < N; ++i) {
                const size_t k = ((size_t)t * nz + z) * N + i;
                if (!cnt[k]) continue;
                if (entries + cnt[k] >= ((int64_t)1 << 31) || n + own[k] >= ((int64_t)1 << 30))
                    FAIL(h, DLSM_E_LIMIT, "the lists hold fewer than 2^30 missing dyads");
                jobs.insert(jobs.end(), {2 * t + z, i, (int32_t)entries, (int32_t)(entries + cnt[k])});
                slot0.push_back((int32_t)n);
                entries += cnt[k]; n += own[k];
            }
        job_lo[t + 1] = (int)slot0.size();
    }
    // (every listed pair set a bit, and the flag is clear: n >= 1 here)
    const size_t njobs = slot0.size();
    DevArray<int32_t> d_slot0;
    if (h->miss_jobs.alloc(h, jobs.size()) || h->miss_cols.alloc(h, (size_t)entries) ||
        h->miss_slot.alloc(h, (size_t)entries) || h->miss_psum.alloc(h, (size_t)n) ||
        h->miss_ones.alloc(h, (size_t)n) || h->miss_nacc.alloc(h, 1) || d_slot0.alloc(h, njobs)) return DLSM_E_HIP;
    HIPCHK(h, hipMemcpyAsync(h->miss_jobs, jobs.data(), jobs.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                             h->stream));
    HIPCHK(h, hipMemcpyAsync(d_slot0, slot0.data(), njobs * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    for (int t = 0; t < h->T; ++t) {
        const int nj = job_lo[t + 1] - job_lo[t];
        if (!nj) continue;
        HIPCHK(h, hipMemsetAsync(bits, 0, nz * slice * sizeof(uint32_t), h->stream));
        enqueue_scatter(h, d_src, d_dst, offsets, t, fwd, bwd, dflag);
        hipLaunchKernelGGL(k_miss_rows_emit, dim3((unsigned)((nj + ROWS_WAVES - 1) / ROWS_WAVES)),
                           dim3(64 * ROWS_WAVES), 0, h->stream, fwd, bwd, W, directed ? 0 : 1,
                           (const MissJob *)h->miss_jobs.get() + job_lo[t], d_slot0 + job_lo[t], nj,
                           h->miss_cols.get(), h->miss_slot.get());
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));         // (the temporaries and the host vectors go on return)
    h->miss_n = n; h->miss_njobs = (int)njobs;
    return dlsm_reset_missing_sums(h);
}

}  // namespace

extern "C" {

int dlsm_set_missing_edges(dlsm_chain *h, const int64_t *offsets, const int32_t *src, const int32_t *dst,
                           int allow_ties) {
    NEED(h, h && offsets, "null argument");
    drop_graph(h);
    const int rc = miss_edges_build(h, offsets, src, dst, allow_ties);
    // old tables never sit behind a new list, and a failed call leaves none at all (the network stays)
    if (rc) {
        hipStreamSynchronize(h->stream);
        miss_free(h);
        h->miss_on = false;
    }
    return rc;
}

int dlsm_missing_count(dlsm_chain *h, int64_t *n) {
    NEED(h, h && n, "null argument");
    *n = h->miss_n;
    return DLSM_OK;
}

int dlsm_get_missing_index(dlsm_chain *h, int32_t *tij) {
    NEED(h, h && tij, "null argument");
    NEED(h, h->miss_n > 0, "no missing dyads set (dlsm_set_missing)");
    HIPCHK(h, hipSetDevice(h->device));
    DevArray<int32_t> d_tij;
    { int rc = d_tij.alloc(h, (size_t)h->miss_n * 3); if (rc) return rc; }
    hipLaunchKernelGGL(k_miss_index, dim3((unsigned)((h->miss_njobs + ROWS_WAVES - 1) / ROWS_WAVES)),
                       dim3(64 * ROWS_WAVES), 0, h->stream, (const MissJob *)h->miss_jobs.get(), h->miss_njobs,
                       h->miss_cols.get(), h->miss_slot.get(), (long)h->miss_n, d_tij.get());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(tij, d_tij, (size_t)h->miss_n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
