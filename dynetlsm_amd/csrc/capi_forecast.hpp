// C-ABI of the one-step-ahead forecasts (included by capi.hip after capi_init.hpp).
#pragma once

extern "C" {

int dlsm_forecast_mean_probas(dlsm_chain *h, const double *Xs, const double *intercepts, int S,
                              int zero_diag, double *out) {
    NEED(h, h && Xs && intercepts && out, "null argument");
    NEED(h, S >= 1, "needs at least one sample");
    HIPCHK(h, hipSetDevice(h->device));
    const int N = h->N, D = h->D;
    DevArray<double> bX, bB, bO;
    if (bX.alloc(h, (size_t)S * N * D) || bB.alloc(h, (size_t)S) || bO.alloc(h, (size_t)N * N)) return DLSM_E_HIP;
    HIPCHK(h, hipMemcpyAsync(bX, Xs, (size_t)S * N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bB, intercepts, (size_t)S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const int nt = (N + FC_TILE - 1) / FC_TILE;
    {
        ProfScope ps(h, DLSM_K_LOGLIK);
        DISPATCH_D(h, D, hipLaunchKernelGGL((k_forecast_mean<DD>), dim3(nt, nt), dim3(256), 0, h->stream,
                                            bX, bB, S, N, zero_diag,
                                            bO));
    }
    HIPCHK(h, hipGetLastError());
    return d2h(h, out, bO, (size_t)N * N);
}

int dlsm_forecast_marginal(dlsm_chain *h, const double *x, const double *W, const double *intercepts,
                           int S, double *out) {
    NEED(h, h && x && W && intercepts && out, "null argument");
    NEED(h, S >= 1, "needs at least one sample");
    HIPCHK(h, hipSetDevice(h->device));
    const int N = h->N, D = h->D;
    DevArray<double> bX, bW, bB, bO;
    if (bX.alloc(h, (size_t)N * D) || bW.alloc(h, (size_t)S * N) || bB.alloc(h, (size_t)S) ||
        bO.alloc(h, (size_t)N * N)) return DLSM_E_HIP;
    HIPCHK(h, hipMemcpyAsync(bX, x, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bW, W, (size_t)S * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(bB, intercepts, (size_t)S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const int nt = (N + FC_TILE - 1) / FC_TILE;
    {
        ProfScope ps(h, DLSM_K_LOGLIK);
        DISPATCH_D(h, D, hipLaunchKernelGGL((k_forecast_marginal<DD>), dim3(nt, nt), dim3(256), 0,
                                            h->stream, bX, bW,
                                            bB, S, N, bO));
    }
    HIPCHK(h, hipGetLastError());
    return d2h(h, out, bO, (size_t)N * N);
}

}  // extern "C"
