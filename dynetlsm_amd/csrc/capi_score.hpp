// C-ABI of the in-sample scores (kernels_score.hpp) on capi_samples.hpp's pass driver; the error macros and ProfScope
// are capi.hip's.  The reference has no counterpart.
#pragma once
#include "capi_samples.hpp"
#include "kernels_score.hpp"

namespace {

constexpr size_t SCORE_HIST_BYTES = (size_t)256 << 20;    // bound of the histograms: time steps go in groups
constexpr int SCORE_G_MAX = 1 << 16;                      // workgroups of one time step

}  // namespace

extern "C" {

int dlsm_score_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                          const double *intercepts, const double *radii, int S, uint64_t *counts,
                          double *logloss_sum) {
    if (int rc = pass_check_inputs(h, h && bits && Xs && intercepts && counts && logloss_sum, bits, radii, S, 1))
        return rc;
    const int T = h->T, N = h->N, D = h->D;
    TracePass p(h, S);
    // u2 <= 2 n_pos n_neg <= dyads^2 / 2 is held in 64 bits
    const double dyads = (double)T * N * (N - 1) / (p.directed ? 1.0 : 2.0);
    if (dyads >= 4294967296.0)
        FAIL(h, DLSM_E_LIMIT, "T=%d N=%d: %.0f dyads, the rank statistic holds fewer than 2^32 per call", T, N, dyads);
    const PassGrid g = pass_grid(p.n_tiles, SCORE_G_MAX);
    // time steps per group: their histograms and the pooled one within SCORE_HIST_BYTES
    const size_t slot_bytes = SCORE_SLOT * sizeof(score_count_t);
    const int TG = std::min<int>(T, std::max<int>(1, (int)(SCORE_HIST_BYTES / slot_bytes) - 1));
    static_assert(sizeof(score_count_t) == sizeof(uint64_t), "the counts are 64-bit");
    const int iHist = p.buf<score_count_t>((size_t)(TG + 1) * SCORE_SLOT);
    const int iPL = p.buf<double>(std::max<size_t>(1, (size_t)T * g.G));
    const int iCnt = p.out(counts, (size_t)(T + 1) * 4);
    const int iLL = p.out(logloss_sum, T);
    if (int rc = p.begin(bits, mask, Xs, intercepts, radii)) return rc;
    score_count_t *hist = p.at<score_count_t>(iHist), *pooled = hist + (size_t)TG * SCORE_SLOT;
    score_count_t *cnt = p.at<score_count_t>(iCnt);
    {
        ProfScope ps(h, DLSM_K_SCORE_CLEAR);
        HIPCHK(h, hipMemsetAsync(pooled, 0, slot_bytes, h->stream));
    }
    for (int t0 = 0; t0 < T; t0 += TG) {
        const int nt = std::min(TG, T - t0);
        {
            ProfScope ps(h, DLSM_K_SCORE_CLEAR);
            HIPCHK(h, hipMemsetAsync(hist, 0, (size_t)nt * slot_bytes, h->stream));
        }
        if (g.G) {                // (no tiles: the histograms stay empty)
            ProfScope ps(h, DLSM_K_SCORE_ACCUMULATE);
            DISPATCH_D(h, D, LAUNCH_DIR(p.directed, k_score_accumulate, dim3((unsigned)g.G, (unsigned)nt), dim3(IC_NT),
                                        h->stream, p.X(), p.B(), p.R(), p.bits(), p.mask(), p.tiles(), p.n_tiles, g.L,
                                        S, T, N, h->W, t0, hist, p.at<double>(iPL)));
            HIPCHK(h, hipGetLastError());
        }
        ProfScope ps(h, DLSM_K_SCORE_SCAN);
        hipLaunchKernelGGL(k_score_scan, dim3((unsigned)nt), dim3(SCORE_SCAN_NT), 0, h->stream, hist, pooled,
                           cnt + 4 * (size_t)t0);
        HIPCHK(h, hipGetLastError());
    }
    {
        ProfScope ps(h, DLSM_K_SCORE_SCAN);
        hipLaunchKernelGGL(k_score_scan, dim3(1), dim3(SCORE_SCAN_NT), 0, h->stream, pooled,
                           (score_count_t *)nullptr, cnt + 4 * (size_t)T);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(k_score_reduce_logloss, dim3((unsigned)T), dim3(IC_NT), 0, h->stream, p.at<double>(iPL),
                           g.G, p.at<double>(iLL));
        HIPCHK(h, hipGetLastError());
    }
    return p.finish();
}

}  // extern "C"
