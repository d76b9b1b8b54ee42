// C-ABI of the missing-dyad imputation step (kernels_missing.hpp; included by capi.hip ahead of the LSM loop's
// drivers, which enqueue the step as an iteration's last launch).  Stands for lsm.py:525-545 and
// hdp_lpcm.py:1025-1049 of the reference.
#pragma once

namespace {

void miss_free(dlsm_chain *h) {
    h->miss_jobs.reset(); h->miss_cols.reset(); h->miss_slot.reset();
    h->miss_psum.reset(); h->miss_ones.reset(); h->miss_nacc.reset();
    h->miss_n = 0; h->miss_njobs = 0;
}

int miss_check_ready(dlsm_chain *h) {
    NEED(h, h->miss_n > 0, "no missing dyads set (dlsm_set_missing)");
    NEED(h, h->have_network, "network not uploaded");
    NEED(h, h->have_X, "latent positions not set");
    NEED(h, h->model == DLSM_UNDIRECTED || h->have_radii, "radii not set");
    NEED(h, !h->squared, "missing dyads are drawn from the Euclidean-distance predictor only");
    return DLSM_OK;
}

// the step on queue `q`; accumulate: 0 never, 1 always, 2 when the iteration is beyond `after`
template <int DD>
int enqueue_impute(dlsm_chain *h, hipStream_t q, IterRef ir, int accumulate, uint32_t after) {
    MissArgs a;
    a.jobs = (const MissJob *)h->miss_jobs.get(); a.cols = h->miss_cols; a.slot = h->miss_slot;
    a.ybits = h->ybits; a.ytbits = h->ytbits;
    a.ycm32 = h->model == DLSM_UNDIRECTED ? (uint32_t *)h->ycm.get() : nullptr;
    a.psum = h->miss_psum; a.ones = h->miss_ones; a.nacc = h->miss_nacc;
    a.accumulate = accumulate; a.acc_after = after;
    hipLaunchKernelGGL((k_impute_missing<DD>), dim3((unsigned)h->miss_njobs), dim3(64), 0, q, h->view(), a, ir);
    HIPCHK(h, hipGetLastError());
    return DLSM_OK;
}

// ... as the last launch of an iteration of dlsm_lsm_run, when the sampling is switched on
template <int DD>
int enqueue_impute_in_loop(dlsm_chain *h, hipStream_t q, IterRef ir) {
    if (!h->miss_on) return DLSM_OK;
    return enqueue_impute<DD>(h, q, ir, h->miss_after < 0 ? 1 : 2, (uint32_t)std::max<int64_t>(h->miss_after, 0));
}

}  // namespace

extern "C" {

int dlsm_set_missing(dlsm_chain *h, const int32_t *tij, int64_t n) {
    NEED(h, h != nullptr, "null handle");
    drop_graph(h);
    NEED(h, h->model != DLSM_DIRECTED_CASE_CONTROL, "case-control chains hold edge lists: no dyads to impute");
    NEED(h, n >= 0 && (n == 0 || tij), "bad argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n == 0) { miss_free(h); h->miss_on = false; return DLSM_OK; }
    NEED(h, h->have_network, "network not uploaded");
    if (h->N >= MISS_N_MAX) FAIL(h, DLSM_E_LIMIT, "N=%d: the draws' counters hold node indices below 2^24", h->N);
    if (n >= ((int64_t)1 << 30)) FAIL(h, DLSM_E_LIMIT, "%lld missing dyads: the lists hold fewer than 2^30", (long long)n);
    const bool directed = h->model == DLSM_DIRECTED;
    struct Entry { int32_t tz, row, col, slot; };
    std::vector<Entry> es;
    es.reserve((size_t)2 * n);
    for (int64_t k = 0; k < n; ++k) {
        const int32_t t = tij[3 * k], i = tij[3 * k + 1], j = tij[3 * k + 2];
        if (t < 0 || t >= h->T || i < 0 || i >= h->N || j < 0 || j >= h->N)
            FAIL(h, DLSM_E_DATA, "missing[%lld] = (%d, %d, %d) outside T=%d, N=%d", (long long)k, t, i, j, h->T, h->N);
        if (directed ? i == j : i >= j)
            FAIL(h, DLSM_E_DATA, "missing[%lld] = (%d, %d, %d): %s", (long long)k, t, i, j,
                 directed ? "the diagonal is not a dyad" : "undirected dyads are listed with i < j");
        es.push_back(Entry{2 * t, i, j, (int32_t)k});
        es.push_back(Entry{2 * t + (directed ? 1 : 0), j, i, -1});
    }
    std::sort(es.begin(), es.end(), [](const Entry &a, const Entry &b) {
        if (a.tz != b.tz) return a.tz < b.tz;
        if (a.row != b.row) return a.row < b.row;
        return a.col < b.col;
    });
    std::vector<int32_t> jobs, cols(es.size()), slot(es.size());
    for (size_t e = 0; e < es.size(); ++e) {
        if (e && es[e].tz == es[e - 1].tz && es[e].row == es[e - 1].row && es[e].col == es[e - 1].col)
            FAIL(h, DLSM_E_DATA, "missing dyad (%d, %d, %d) is listed twice", es[e].tz >> 1,
                 (es[e].tz & 1) ? es[e].col : es[e].row, (es[e].tz & 1) ? es[e].row : es[e].col);
        cols[e] = es[e].col; slot[e] = es[e].slot;
        if (!e || es[e].tz != es[e - 1].tz || es[e].row != es[e - 1].row) {
            if (!jobs.empty()) jobs[jobs.size() - 1] = (int32_t)e;
            jobs.insert(jobs.end(), {es[e].tz, es[e].row, (int32_t)e, 0});
        }
    }
    jobs[jobs.size() - 1] = (int32_t)es.size();
    miss_free(h);
    if (h->miss_jobs.alloc(h, jobs.size()) || h->miss_cols.alloc(h, cols.size()) ||
        h->miss_slot.alloc(h, slot.size()) || h->miss_psum.alloc(h, (size_t)n) || h->miss_ones.alloc(h, (size_t)n) ||
        h->miss_nacc.alloc(h, 1)) return DLSM_E_HIP;
    HIPCHK(h, hipMemcpy(h->miss_jobs, jobs.data(), jobs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->miss_cols, cols.data(), cols.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->miss_slot, slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    h->miss_n = n; h->miss_njobs = (int)(jobs.size() / 4);
    return dlsm_reset_missing_sums(h);
}

int dlsm_reset_missing_sums(dlsm_chain *h) {
    NEED(h, h != nullptr, "null handle");
    NEED(h, h->miss_n > 0, "no missing dyads set (dlsm_set_missing)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->miss_psum, 0, (size_t)h->miss_n * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->miss_ones, 0, (size_t)h->miss_n * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(h->miss_nacc, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

int dlsm_impute_missing(dlsm_chain *h, uint32_t iter, int accumulate) {
    NEED(h, h != nullptr, "null handle");
    { int rc_ = miss_check_ready(h); if (rc_) return rc_; }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = DLSM_OK;
    DISPATCH_D(h, h->D, rc = enqueue_impute<DD>(h, h->stream, IterRef{iter, nullptr}, accumulate ? 1 : 0, 0u));
    return rc;
}

int dlsm_missing_sampling(dlsm_chain *h, int on, int accumulate_after) {
    NEED(h, h != nullptr, "null handle");
    drop_graph(h);
    if (on) { int rc_ = miss_check_ready(h); if (rc_) return rc_; }
    h->miss_on = on != 0;
    h->miss_after = accumulate_after;
    return DLSM_OK;
}

int dlsm_get_missing(dlsm_chain *h, double *p_sum, uint32_t *ones, int64_t *n_accumulated) {
    NEED(h, h != nullptr, "null handle");
    NEED(h, h->miss_n > 0, "no missing dyads set (dlsm_set_missing)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    { int rc_ = check_pipe_err(h); if (rc_) return rc_; }
    if (p_sum) HIPCHK(h, hipMemcpy(p_sum, h->miss_psum, (size_t)h->miss_n * sizeof(double), hipMemcpyDeviceToHost));
    if (ones) HIPCHK(h, hipMemcpy(ones, h->miss_ones, (size_t)h->miss_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n_accumulated) {
        unsigned long long k = 0;
        HIPCHK(h, hipMemcpy(&k, h->miss_nacc, sizeof(k), hipMemcpyDeviceToHost));
        *n_accumulated = (int64_t)k;
    }
    return DLSM_OK;
}

}  // extern "C"
