// C-ABI of the in-sample scores (kernels_score.hpp; included by capi.hip after capi_ic.hpp, whose tiles and
// input checks it shares).  The reference has no counterpart.
#pragma once

namespace {

constexpr size_t SCORE_HIST_BYTES = (size_t)256 << 20;    // bound of the histograms: time steps go in groups
constexpr int SCORE_G_MAX = 1 << 16;                      // workgroups of one time step

template <int D>
void score_launch(dlsm_chain *h, bool directed, dim3 grid, const double *Xs, const double *ic, const double *radii,
                  const uint32_t *bits, const uint32_t *mask, const int2 *tiles, int n_tiles, int L, int S, int t0,
                  score_count_t *hist, double *part_ll) {
    if (directed)
        hipLaunchKernelGGL((k_score_accumulate<D, true>), grid, dim3(IC_NT), 0, h->stream, Xs, ic, radii, bits, mask,
                           tiles, n_tiles, L, S, h->T, h->N, h->W, t0, hist, part_ll);
    else
        hipLaunchKernelGGL((k_score_accumulate<D, false>), grid, dim3(IC_NT), 0, h->stream, Xs, ic, radii, bits, mask,
                           tiles, n_tiles, L, S, h->T, h->N, h->W, t0, hist, part_ll);
}

}  // namespace

extern "C" {

int dlsm_score_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                          const double *intercepts, const double *radii, int S, uint64_t *counts,
                          double *logloss_sum) {
    NEED(h, h && bits && Xs && intercepts && counts && logloss_sum, "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, S >= 1, "needs at least one sample");
    const int T = h->T, N = h->N, D = h->D, W = h->W;
    const size_t net_words = (size_t)N * W;
    if (int rc = ic_check_inputs(h, bits, radii, S)) return rc;
    // u2 <= 2 n_pos n_neg <= dyads^2 / 2 is held in 64 bits
    const double dyads = (double)T * N * (N - 1) / (directed ? 1.0 : 2.0);
    if (dyads >= 4294967296.0)
        FAIL(h, DLSM_E_LIMIT, "T=%d N=%d: %.0f dyads, the rank statistic holds fewer than 2^32 per call", T, N, dyads);
    HIPCHK(h, hipSetDevice(h->device));
    const int TI = D <= 4 ? IcPlan<1>::TI : IcPlan<8>::TI;
    const std::vector<int2> tiles = ic_tiles(N, TI, directed);
    const int n_tiles = (int)tiles.size();
    const int L = (n_tiles + SCORE_G_MAX - 1) / SCORE_G_MAX;
    const int G = L ? (n_tiles + L - 1) / L : 0;
    // time steps per group: their histograms and the pooled one within SCORE_HIST_BYTES
    const size_t slot_bytes = SCORE_SLOT * sizeof(score_count_t);
    const int TG = std::min<int>(T, std::max<int>(1, (int)(SCORE_HIST_BYTES / slot_bytes) - 1));
    // all S samples are resident, as in dlsm_ic_accumulate
    const size_t per_sample = ((size_t)T * N * D + 2 + (directed ? N : 0)) * sizeof(double);
    const size_t fixed = (size_t)T * net_words * sizeof(uint32_t) * (mask ? 2 : 1) + (size_t)n_tiles * sizeof(int2) +
                         (size_t)(TG + 1) * slot_bytes + (size_t)T * (G + 1) * sizeof(double) +
                         (size_t)(T + 1) * 4 * sizeof(score_count_t) + ((size_t)64 << 20);
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    if (fixed + (size_t)S * per_sample > free_b) {
        const long long fit = free_b > fixed ? (long long)((free_b - fixed) / per_sample) : 0;
        FAIL(h, DLSM_E_LIMIT, "S=%d samples of T=%d N=%d D=%d need %.1f MB of device memory, %.1f MB are free: "
             "the largest S that fits is %lld", S, T, N, D, (fixed + (size_t)S * per_sample) / 1048576.0,
             free_b / 1048576.0, fit);
    }
    DevBuf bX, bB, bR, bBits, bMask, bTiles, bHist, bPL, bCnt, bLL;
    HIPCHK(h, hipMalloc(&bX.p, (size_t)S * T * N * D * sizeof(double)));
    HIPCHK(h, hipMalloc(&bB.p, (size_t)S * 2 * sizeof(double)));
    if (directed) HIPCHK(h, hipMalloc(&bR.p, (size_t)S * N * sizeof(double)));
    HIPCHK(h, hipMalloc(&bBits.p, (size_t)T * net_words * sizeof(uint32_t)));
    if (mask) HIPCHK(h, hipMalloc(&bMask.p, (size_t)T * net_words * sizeof(uint32_t)));
    HIPCHK(h, hipMalloc(&bTiles.p, std::max<size_t>(1, n_tiles) * sizeof(int2)));
    HIPCHK(h, hipMalloc(&bHist.p, (size_t)(TG + 1) * slot_bytes));
    HIPCHK(h, hipMalloc(&bPL.p, std::max<size_t>(1, (size_t)T * G) * sizeof(double)));
    HIPCHK(h, hipMalloc(&bCnt.p, (size_t)(T + 1) * 4 * sizeof(score_count_t)));
    HIPCHK(h, hipMalloc(&bLL.p, (size_t)T * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(bX.p, Xs, (size_t)S * T * N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bB.p, intercepts, (size_t)S * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (directed)
        HIPCHK(h, hipMemcpyAsync(bR.p, radii, (size_t)S * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bBits.p, bits, (size_t)T * net_words * sizeof(uint32_t), hipMemcpyHostToDevice,
                             h->stream));
    if (mask)
        HIPCHK(h, hipMemcpyAsync(bMask.p, mask, (size_t)T * net_words * sizeof(uint32_t), hipMemcpyHostToDevice,
                                 h->stream));
    HIPCHK(h, hipMemcpyAsync(bTiles.p, tiles.data(), (size_t)n_tiles * sizeof(int2), hipMemcpyHostToDevice,
                             h->stream));
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
            DISPATCH_D(h, D, score_launch<DD>(h, directed, dim3((unsigned)G, (unsigned)nt), bX.as<double>(),
                                              bB.as<double>(), directed ? bR.as<double>() : nullptr,
                                              bBits.as<uint32_t>(), mask ? bMask.as<uint32_t>() : nullptr,
                                              bTiles.as<int2>(), n_tiles, L, S, t0, hist, bPL.as<double>()));
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
