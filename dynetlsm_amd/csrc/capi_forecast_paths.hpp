// C-ABI of the multi-step posterior predictive forecasts (kernels_forecast_paths.hpp; included by capi.hip
// after capi_score.hpp).  The reference has only the one-step undirected form (hdp_lpcm.py:555-626).
#pragma once

namespace {

constexpr size_t FP_SCRATCH_BYTES = (size_t)256 << 20;    // device scratch of one batch (auto batching)

}  // namespace

extern "C" {

int dlsm_forecast_paths(dlsm_chain *h, const double *X0, const double *intercepts, const double *radii,
                        const int32_t *z0, const double *trans, const double *mu, const double *sigma,
                        const double *lmbda, int K, double sigma_sq, int H, int S, uint64_t seed,
                        uint32_t first_index, int batch, double *probas, double *paths, int32_t *labels) {
    NEED(h, h && X0 && intercepts && probas, "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    const bool mixture = z0 != nullptr;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, S >= 1, "needs at least one sample");
    NEED(h, H >= 1 && H <= 65535, "the horizon must be in 1..65535, got %d", H);
    NEED(h, batch >= 0, "batch must be >= 0 (0: automatic)");
    NEED(h, (uint64_t)first_index + (uint64_t)S <= ((uint64_t)1 << 32), "first_index + S must be <= 2^32");
    const int N = h->N, D = h->D;
    if (mixture) {
        NEED(h, K >= 1, "the mixture needs K >= 1 components, got %d", K);
        NEED(h, trans && mu && sigma && lmbda, "the mixture needs trans, mu, sigma and lmbda");
        for (size_t k = 0; k < (size_t)S * N; ++k)
            if (z0[k] < 0 || z0[k] >= K)
                FAIL(h, DLSM_E_DATA, "z0 = %d outside [0, %d) (sample %zu, node %zu)", (int)z0[k], K, k / N, k % N);
        for (size_t k = 0; k < (size_t)S * K; ++k)
            if (!(sigma[k] >= 0.0)) FAIL(h, DLSM_E_DATA, "sigma must be >= 0 (sample %zu, component %zu)", k / K, k % K);
        for (size_t r = 0; r < (size_t)S * K; ++r) {
            double tot = 0.0;
            for (int k = 0; k < K; ++k) {
                const double w = trans[r * K + k];
                if (!(w >= 0.0)) FAIL(h, DLSM_E_DATA, "transition weights must be >= 0 (sample %zu, row %zu)", r / K, r % K);
                tot += w;
            }
            if (!(tot > 0.0) || !std::isfinite(tot))
                FAIL(h, DLSM_E_DATA, "a transition row must have a positive, finite sum (sample %zu, row %zu)", r / K, r % K);
        }
    } else {
        NEED(h, K == 0 && !trans && !mu && !sigma && !lmbda, "the random walk (z0 == NULL) takes K = 0 and no mixture arrays");
        NEED(h, sigma_sq >= 0.0 && std::isfinite(sigma_sq), "sigma_sq must be >= 0");
        NEED(h, !labels, "the random walk has no labels");
    }
    if (int rc = check_radii_positive(h, radii, S)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    // samples per batch: the draws of a batch ([H][nb][N][D] and the labels) within FP_SCRATCH_BYTES
    const size_t per_sample = (size_t)H * N * (D * sizeof(double) + (mixture ? sizeof(int32_t) : 0)) +
                              (size_t)N * (D + 1) * sizeof(double) + (size_t)N * sizeof(int32_t) +
                              (mixture ? ((size_t)K * K + (size_t)K * D + K + 1) * sizeof(double) : 0);
    int nb = batch > 0 ? batch : (int)std::max<size_t>(1, FP_SCRATCH_BYTES / per_sample);
    nb = std::min(nb, S);
    nb = std::min(nb, 65535);                              // the draw grid's y extent
    const size_t ND = (size_t)N * D;
    DevArray<double> bX, bB, bR, bW, bM, bSg, bL, bP, bSum; DevArray<int32_t> bZ, bLab;
    if (bX.alloc(h, (size_t)nb * ND) || bB.alloc(h, (size_t)nb * 2) ||
        (directed && bR.alloc(h, (size_t)nb * N))) return DLSM_E_HIP;
    if (mixture) {
        if (bZ.alloc(h, (size_t)nb * N) || bW.alloc(h, (size_t)nb * K * K) || bM.alloc(h, (size_t)nb * K * D) ||
            bSg.alloc(h, (size_t)nb * K) || bL.alloc(h, (size_t)nb) ||
            bLab.alloc(h, (size_t)H * nb * N)) return DLSM_E_HIP;
    }
    if (bP.alloc(h, (size_t)H * nb * ND) || bSum.alloc(h, (size_t)H * N * N)) return DLSM_E_HIP;
    // the draws come back horizon-major; the caller's arrays are sample-major
    std::vector<double> hostP;
    std::vector<int32_t> hostL;
    if (paths) hostP.resize((size_t)H * nb * ND);
    if (labels) hostL.resize((size_t)H * nb * N);
    const int nt = (N + FC_TILE - 1) / FC_TILE;
    for (int s0 = 0; s0 < S; s0 += nb) {
        const int n = std::min(nb, S - s0);
        HIPCHK(h, hipMemcpyAsync(bX, X0 + (size_t)s0 * ND, (size_t)n * ND * sizeof(double), hipMemcpyHostToDevice,
                                 h->stream));
        HIPCHK(h, hipMemcpyAsync(bB, intercepts + 2 * (size_t)s0, (size_t)n * 2 * sizeof(double),
                                 hipMemcpyHostToDevice, h->stream));
        if (directed)
            HIPCHK(h, hipMemcpyAsync(bR, radii + (size_t)s0 * N, (size_t)n * N * sizeof(double),
                                     hipMemcpyHostToDevice, h->stream));
        if (mixture) {
            HIPCHK(h, hipMemcpyAsync(bZ, z0 + (size_t)s0 * N, (size_t)n * N * sizeof(int32_t),
                                     hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(bW, trans + (size_t)s0 * K * K, (size_t)n * K * K * sizeof(double),
                                     hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(bM, mu + (size_t)s0 * K * D, (size_t)n * K * D * sizeof(double),
                                     hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(bSg, sigma + (size_t)s0 * K, (size_t)n * K * sizeof(double),
                                     hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(bL, lmbda + s0, (size_t)n * sizeof(double), hipMemcpyHostToDevice,
                                     h->stream));
        }
        {
            ProfScope ps(h, DLSM_K_LOGLIK);
            DISPATCH_D(h, D, hipLaunchKernelGGL((k_forecast_paths_draw<DD>), dim3((unsigned)((N + 255) / 256), (unsigned)n),
                                                dim3(256), 0, h->stream, bX,
                                                mixture ? bZ.get() : nullptr, bW,
                                                bM, bSg, bL, K, sigma_sq, H,
                                                N, seed, first_index + (uint32_t)s0, bP,
                                                bLab));
            HIPCHK(h, hipGetLastError());
            DISPATCH_D(h, D, LAUNCH_DIR(directed, k_forecast_paths_mean, dim3(nt, nt, (unsigned)H), dim3(256),
                                        h->stream, bP, bB, bR, n, N,
                                        (int)(s0 == 0), (int)(s0 + n == S), S, bSum));
            HIPCHK(h, hipGetLastError());
        }
        if (paths)
            HIPCHK(h, hipMemcpyAsync(hostP.data(), bP, (size_t)H * n * ND * sizeof(double), hipMemcpyDeviceToHost,
                                     h->stream));
        if (labels)
            HIPCHK(h, hipMemcpyAsync(hostL.data(), bLab, (size_t)H * n * N * sizeof(int32_t),
                                     hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int hh = 0; hh < H; ++hh)
            for (int s = 0; s < n; ++s) {
                if (paths)
                    memcpy(paths + ((size_t)(s0 + s) * H + hh) * ND, hostP.data() + ((size_t)hh * n + s) * ND,
                           ND * sizeof(double));
                if (labels)
                    memcpy(labels + ((size_t)(s0 + s) * H + hh) * N, hostL.data() + ((size_t)hh * n + s) * N,
                           (size_t)N * sizeof(int32_t));
            }
    }
    HIPCHK(h, hipMemcpyAsync(probas, bSum, (size_t)H * N * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
