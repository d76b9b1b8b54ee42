// C-ABI of the in-sample scores (kernels_score.hpp; included by capi.hip after capi_samples.hpp, whose input
// checks and resident samples it uses).  The reference has no counterpart.
#pragma once

namespace {

constexpr size_t SCORE_HIST_BYTES = (size_t)256 << 20;    // bound of the histograms: time steps go in groups
constexpr int SCORE_G_MAX = 1 << 16;                      // workgroups of one time step

}  // namespace

extern "C" {

int dlsm_score_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                          const double *intercepts, const double *radii, int S, uint64_t *counts,
                          double *logloss_sum) {
    NEED(h, h && bits && Xs && intercepts && counts && logloss_sum, "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, S >= 1, "needs at least one sample");
    const int T = h->T, N = h->N, D = h->D;
    if (int rc = check_packed_network(h, bits)) return rc;
    if (int rc = check_radii_positive(h, radii, S)) return rc;
    // u2 <= 2 n_pos n_neg <= dyads^2 / 2 is held in 64 bits
    const double dyads = (double)T * N * (N - 1) / (directed ? 1.0 : 2.0);
    if (dyads >= 4294967296.0)
        FAIL(h, DLSM_E_LIMIT, "T=%d N=%d: %.0f dyads, the rank statistic holds fewer than 2^32 per call", T, N, dyads);
    HIPCHK(h, hipSetDevice(h->device));
    ResidentSamples in(h);
    const int n_tiles = in.n_tiles;
    const int L = (n_tiles + SCORE_G_MAX - 1) / SCORE_G_MAX;
    const int G = L ? (n_tiles + L - 1) / L : 0;
    // time steps per group: their histograms and the pooled one within SCORE_HIST_BYTES
    const size_t slot_bytes = SCORE_SLOT * sizeof(score_count_t);
    const int TG = std::min<int>(T, std::max<int>(1, (int)(SCORE_HIST_BYTES / slot_bytes) - 1));
    if (int rc = in.alloc(h, S, bits, mask, (size_t)(TG + 1) * slot_bytes + (size_t)T * (G + 1) * sizeof(double) +
                          (size_t)(T + 1) * 4 * sizeof(score_count_t), 0)) return rc;
    DevBuf bHist, bPL, bCnt, bLL;
    HIPCHK(h, hipMalloc(&bHist.p, (size_t)(TG + 1) * slot_bytes));
    HIPCHK(h, hipMalloc(&bPL.p, std::max<size_t>(1, (size_t)T * G) * sizeof(double)));
    HIPCHK(h, hipMalloc(&bCnt.p, (size_t)(T + 1) * 4 * sizeof(score_count_t)));
    HIPCHK(h, hipMalloc(&bLL.p, (size_t)T * sizeof(double)));
    if (int rc = in.upload(h, Xs, intercepts, radii, S)) return rc;
    score_count_t *hist = bHist.as<score_count_t>(), *pooled = hist + (size_t)TG * SCORE_SLOT;
    score_count_t *cnt = bCnt.as<score_count_t>();
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
        if (G) {                  // (N = 1 has no dyads: the histograms stay empty)
            ProfScope ps(h, DLSM_K_SCORE_ACCUMULATE);
            DISPATCH_D(h, D, LAUNCH_DIR(directed, k_score_accumulate, dim3((unsigned)G, (unsigned)nt), dim3(IC_NT),
                                        h->stream, in.X.as<double>(), in.B.as<double>(), in.R.as<double>(),
                                        in.bits.as<uint32_t>(), in.mask.as<uint32_t>(), in.tiles.as<int2>(), n_tiles,
                                        L, S, T, N, h->W, t0, hist, bPL.as<double>()));
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
        hipLaunchKernelGGL(k_score_reduce_logloss, dim3((unsigned)T), dim3(IC_NT), 0, h->stream, bPL.as<double>(), G,
                           bLL.as<double>());
        HIPCHK(h, hipGetLastError());
    }
    static_assert(sizeof(score_count_t) == sizeof(uint64_t), "the counts are 64-bit");
    HIPCHK(h, hipMemcpyAsync(counts, bCnt.p, (size_t)(T + 1) * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(logloss_sum, bLL.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
