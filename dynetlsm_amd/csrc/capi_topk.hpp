// C-ABI of the link prediction (kernels_topk.hpp) on capi_samples.hpp's pass driver; the error macros and ProfScope
// are capi.hip's.  The reference has no counterpart.
#pragma once
#include "capi_samples.hpp"
#include "kernels_topk.hpp"

namespace {

constexpr size_t TOPK_HIST_BYTES = (size_t)128 << 20;     // bound of the histograms: time steps go in groups

}  // namespace

extern "C" {

int dlsm_topk_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                         const double *intercepts, const double *radii, int S, int among, int largest, int64_t k,
                         int64_t max_candidates, int32_t *cand_index, double *cand_value, int32_t *n_cand,
                         int64_t *diag) {
    if (int rc = pass_check_inputs(h, h && bits && Xs && intercepts && cand_index && cand_value && n_cand && diag,
                                   bits, radii, S, 2)) return rc;
    NEED(h, among >= 0 && among < TOPK_AMONG_COUNT, "among=%d is not in 0..%d", among, TOPK_AMONG_COUNT - 1);
    NEED(h, largest == 0 || largest == 1, "largest=%d is not 0 or 1", largest);
    NEED(h, k >= 1, "k=%lld: at least one dyad must be asked for", (long long)k);
    NEED(h, max_candidates >= k, "max_candidates=%lld is below k=%lld", (long long)max_candidates, (long long)k);
    NEED(h, among != TOPK_MISSING || mask, "among = missing needs the mask");
    const int T = h->T, N = h->N, D = h->D;
    TracePass p(h, S);
    // the counts of a time step and the slots of its candidates are held in 32 bits
    const double dyads = (double)N * (N - 1) / (p.directed ? 1.0 : 2.0);
    if (dyads >= 2147483648.0)
        FAIL(h, DLSM_E_LIMIT, "N=%d: %.0f dyads per time step, the selection holds fewer than 2^31", N, dyads);
    // slots of a time step on the device: no more than it has dyads
    const size_t cap = (size_t)std::min<int64_t>(max_candidates, (int64_t)dyads);
    const PassGrid g = pass_grid(p.n_tiles, PASS_G_MAX);
    const size_t slot_bytes = (size_t)SCORE_HSTRIDE * sizeof(score_count_t);
    const int TG = std::min<int>(T, std::max<int>(1, (int)(TOPK_HIST_BYTES / slot_bytes)));
    const size_t row = (size_t)TOPK_META + p.n_tiles;
    const int iHist = p.buf<score_count_t>((size_t)TG * SCORE_HSTRIDE);
    const int iMeta = p.buf<uint32_t>((size_t)T * row);
    const int iList = p.buf<int2>(std::max<size_t>(1, (size_t)T * p.n_tiles));
    const int iIdx = p.buf<int4>((size_t)T * cap);
    const int iVal = p.buf<double2>((size_t)T * cap);
    static_assert(sizeof(unsigned int) == sizeof(int32_t), "n_cand is counted in 32 bits");
    const int iN = p.out(n_cand, T, PASS_ZERO);
    if (int rc = p.begin(bits, mask, Xs, intercepts, radii)) return rc;
    score_count_t *hist = p.at<score_count_t>(iHist);
    uint32_t *meta = p.at<uint32_t>(iMeta);
    for (int t0 = 0; t0 < T; t0 += TG) {
        const int nt = std::min(TG, T - t0);
        if (g.G) {                // (no tiles: the histograms stay empty)
            ProfScope ps(h, DLSM_K_TOPK_COUNT);
            HIPCHK(h, hipMemsetAsync(hist, 0, (size_t)nt * slot_bytes, h->stream));
            DISPATCH_D(h, D, LAUNCH_DIR(p.directed, k_topk_count, dim3((unsigned)g.G, (unsigned)nt), dim3(IC_NT),
                                        h->stream, p.X(), p.B(), p.R(), p.bits(), p.mask(), p.tiles(), p.n_tiles, g.L,
                                        S, T, N, h->W, t0, among, largest, hist, meta));
            HIPCHK(h, hipGetLastError());
        } else {
            HIPCHK(h, hipMemsetAsync(hist, 0, (size_t)nt * slot_bytes, h->stream));
        }
        ProfScope ps(h, DLSM_K_TOPK_SCAN);
        hipLaunchKernelGGL(k_topk_threshold, dim3((unsigned)nt), dim3(SCORE_SCAN_NT), 0, h->stream, hist,
                           (unsigned long long)k, largest, t0, row, meta);
        HIPCHK(h, hipGetLastError());
    }
    // the host's step: the thresholds and the tiles' keys in one copy, the one wait before the second launch
    std::vector<uint32_t> host_meta((size_t)T * row);
    HIPCHK(h, hipMemcpyAsync(host_meta.data(), meta, host_meta.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<int2> list;
    std::vector<size_t> emitted((size_t)T);
    const bool top = largest != 0;
    for (int t = 0; t < T; ++t) {
        const uint32_t *m = host_meta.data() + (size_t)t * row;
        const uint32_t kappa = m[3];
        size_t revisit = 0;
        for (int q = 0; q < p.n_tiles; ++q) {
            if (m[0] && topk_reaches(m[TOPK_META + q], kappa, top)) {
                list.push_back(make_int2(t, q));
                ++revisit;
            }
        }
        emitted[(size_t)t] = (size_t)m[1] + m[2];
        int64_t *d = diag + 5 * (size_t)t;
        d[0] = m[0]; d[1] = m[1]; d[2] = m[2]; d[3] = m[0] ? (int64_t)kappa : -1; d[4] = (int64_t)revisit;
    }
    for (int t = 0; t < T; ++t)
        if (emitted[(size_t)t] > (size_t)max_candidates)
            FAIL(h, DLSM_E_LIMIT, "time step %d: %zu dyads lie beyond or at the key of the k-th (k=%lld), "
                 "max_candidates=%lld holds fewer: too many dyads share that key", t, emitted[(size_t)t], (long long)k,
                 (long long)max_candidates);
    if (!list.empty()) {
        HIPCHK(h, hipMemcpyAsync(p.at<int2>(iList), list.data(), list.size() * sizeof(int2), hipMemcpyHostToDevice,
                                 h->stream));
        ProfScope ps(h, DLSM_K_TOPK_EMIT);
        DISPATCH_D(h, D, LAUNCH_DIR(p.directed, k_topk_emit, dim3((unsigned)list.size()), dim3(IC_NT), h->stream,
                                    p.X(), p.B(), p.R(), p.bits(), p.mask(), p.tiles(), p.at<int2>(iList), p.n_tiles,
                                    S, T, N, h->W, among, largest, meta, (uint32_t)cap, p.at<unsigned int>(iN),
                                    p.at<int4>(iIdx), p.at<double2>(iVal)));
        HIPCHK(h, hipGetLastError());
    }
    // the slots that were taken: exactly the count of each time step (kernels_topk.hpp), at most `cap`
    for (int t = 0; t < T; ++t) {
        const size_t n = emitted[(size_t)t];
        if (!n) continue;
        HIPCHK(h, hipMemcpyAsync(cand_index + 4 * (size_t)t * max_candidates, p.at<int4>(iIdx) + (size_t)t * cap,
                                 n * sizeof(int4), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(cand_value + 2 * (size_t)t * max_candidates, p.at<double2>(iVal) + (size_t)t * cap,
                                 n * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    }
    if (int rc = p.finish()) return rc;
    for (int t = 0; t < T; ++t)
        if ((size_t)(uint32_t)n_cand[t] != emitted[(size_t)t])
            FAIL(h, DLSM_E_HIP, "time step %d: %u dyads took a slot, %zu were counted: the two launches disagree", t,
                 (uint32_t)n_cand[t], emitted[(size_t)t]);
    return DLSM_OK;
}

}  // extern "C"
