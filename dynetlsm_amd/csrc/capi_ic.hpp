// C-ABI of the information criteria (kernels_ic.hpp; included by capi.hip after capi_samples.hpp, whose input
// checks and resident samples it uses).  The reference has no counterpart.
#pragma once

namespace {

constexpr size_t IC_PARTIAL_BYTES = (size_t)256 << 20;    // bound of the per-workgroup sample partials

}  // namespace

extern "C" {

int dlsm_ic_accumulate(dlsm_chain *h, const uint32_t *bits, const double *Xs, const double *intercepts,
                       const double *radii, int S, double *totals, double *sample_loglik, double *pointwise) {
    NEED(h, h && bits && Xs && intercepts && totals && sample_loglik, "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, S >= 1, "needs at least one sample");
    const int T = h->T, N = h->N, D = h->D;
    if (int rc = check_packed_network(h, bits)) return rc;
    if (int rc = check_radii_positive(h, radii, S)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    ResidentSamples in(h);
    const int n_tiles = in.n_tiles;
    // tiles per workgroup: as few as keep the sample partials [T][G][S] within IC_PARTIAL_BYTES
    const size_t one = (size_t)T * S * sizeof(double);
    const size_t g_max = std::max<size_t>(1, IC_PARTIAL_BYTES / one);
    const int L = (int)(((size_t)n_tiles + g_max - 1) / g_max);
    const int G = (n_tiles + L - 1) / L;
    const size_t pw_bytes = (size_t)T * N * N * 2 * sizeof(double);
    if (int rc = in.alloc(h, S, bits, nullptr,
                          (size_t)T * G * IC_NTOT * sizeof(double) + (size_t)T * IC_NTOT * sizeof(double) +
                          (pointwise ? pw_bytes : 0), (size_t)T * G * sizeof(double))) return rc;
    DevBuf bPT, bPS, bTot, bSL, bPW;
    HIPCHK(h, hipMalloc(&bPT.p, (size_t)T * G * IC_NTOT * sizeof(double)));
    HIPCHK(h, hipMalloc(&bPS.p, (size_t)T * G * S * sizeof(double)));
    HIPCHK(h, hipMalloc(&bTot.p, (size_t)T * IC_NTOT * sizeof(double)));
    HIPCHK(h, hipMalloc(&bSL.p, (size_t)S * T * sizeof(double)));
    if (pointwise) {
        HIPCHK(h, hipMalloc(&bPW.p, pw_bytes));
        HIPCHK(h, hipMemsetAsync(bPW.p, 0, pw_bytes, h->stream));
    }
    if (int rc = in.upload(h, Xs, intercepts, radii, S)) return rc;
    DISPATCH_D(h, D, LAUNCH_DIR(directed, k_ic_accumulate, dim3((unsigned)G, (unsigned)T), dim3(IC_NT), h->stream,
                                in.X.as<double>(), in.B.as<double>(), in.R.as<double>(), in.bits.as<uint32_t>(),
                                in.tiles.as<int2>(), n_tiles, L, S, T, N, h->W, bPT.as<double>(), bPS.as<double>(),
                                bPW.as<double>()));
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_ic_reduce_totals, dim3((unsigned)T), dim3(IC_NT), 0, h->stream, bPT.as<double>(), G,
                       bTot.as<double>());
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_ic_reduce_samples, dim3((unsigned)((S + 63) / 64), (unsigned)T), dim3(IC_NT), 0, h->stream,
                       bPS.as<double>(), G, S, T, bSL.as<double>());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(totals, bTot.p, (size_t)T * IC_NTOT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(sample_loglik, bSL.p, (size_t)S * T * sizeof(double), hipMemcpyDeviceToHost,
                             h->stream));
    if (pointwise)
        HIPCHK(h, hipMemcpyAsync(pointwise, bPW.p, pw_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
