// C-ABI of the tie dynamics (kernels_dynamics.hpp; included by capi.hip after capi_samples.hpp, whose input checks
// and resident samples it uses).  The reference has no counterpart.
#pragma once

extern "C" {

int dlsm_dynamics_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                             const double *intercepts, const double *radii, int S, int min_count, int n_bins,
                             uint64_t *transitions, uint64_t *hist_up, uint64_t *node_changes,
                             uint64_t *node_turnover, double *pointwise) {
    NEED(h, h && bits && Xs && intercepts && transitions && hist_up && node_changes && node_turnover,
         "null argument");
    const bool directed = h->model != DLSM_UNDIRECTED;
    NEED(h, !directed || radii, "directed models need the radii");
    NEED(h, S >= 2, "needs at least two samples (the standard deviation has ddof = 1), got S=%d", S);
    NEED(h, h->T >= 2, "a step needs two time steps, the handle has T=%d", h->T);
    NEED(h, min_count >= 1 && min_count <= S, "min_count=%d is not in 1..S=%d", min_count, S);
    NEED(h, n_bins >= 1 && n_bins <= DYN_MAX_BINS, "n_bins=%d is not in 1..%d", n_bins, DYN_MAX_BINS);
    const int T = h->T, N = h->N, D = h->D;
    if (int rc = check_packed_network(h, bits)) return rc;
    if (int rc = check_radii_positive(h, radii, S)) return rc;
    // a sum of fix(x) <= 2^32 over the dyads of a step stays below 2^63
    const double dyads = (double)N * (N - 1) / (directed ? 1.0 : 2.0);
    if (dyads >= 2147483648.0)
        FAIL(h, DLSM_E_LIMIT, "N=%d: %.0f dyads per time step, the fixed-point sums hold fewer than 2^31", N, dyads);
    HIPCHK(h, hipSetDevice(h->device));
    ResidentSamples in(h);
    const int n_tiles = in.n_tiles;
    const int L = (n_tiles + CONV_G_MAX - 1) / CONV_G_MAX;
    const int G = L ? (n_tiles + L - 1) / L : 0;
    static_assert(sizeof(conv_count_t) == sizeof(uint64_t), "the counts are 64-bit");
    // one buffer of counters: transitions, hist_up, node_changes, node_turnover
    const size_t U = (size_t)T - 1;
    const size_t n_tr = U * 16, n_hist = U * n_bins, n_ch = U * N * 4, n_to = U * N * 2;
    const size_t n_cnt = n_tr + n_hist + n_ch + n_to;
    const size_t pw_bytes = U * N * N * 4 * sizeof(double);
    if (int rc = in.alloc(h, S, bits, mask, n_cnt * sizeof(conv_count_t) + (pointwise ? pw_bytes : 0), 0)) return rc;
    DevBuf bC, bPW;
    HIPCHK(h, hipMalloc(&bC.p, n_cnt * sizeof(conv_count_t)));
    if (pointwise) {
        HIPCHK(h, hipMalloc(&bPW.p, pw_bytes));
        HIPCHK(h, hipMemsetAsync(bPW.p, 0, pw_bytes, h->stream));
    }
    HIPCHK(h, hipMemsetAsync(bC.p, 0, n_cnt * sizeof(conv_count_t), h->stream));
    if (int rc = in.upload(h, Xs, intercepts, radii, S)) return rc;
    conv_count_t *cnt = bC.as<conv_count_t>();
    if (G) {                      // (N = 1 has no dyads: every table stays zero)
        DynArgs a;
        a.Xs = in.X.as<double>(); a.ic = in.B.as<double>(); a.radii = in.R.as<double>();
        a.bits = in.bits.as<uint32_t>(); a.mask = in.mask.as<uint32_t>(); a.tiles = in.tiles.as<int2>();
        a.n_tiles = n_tiles; a.L = L; a.S = S; a.T = T; a.N = N; a.W = h->W;
        a.min_count = min_count; a.n_bins = n_bins;
        a.transitions = cnt; a.hist_up = cnt + n_tr; a.node_changes = a.hist_up + n_hist;
        a.node_turnover = a.node_changes + n_ch;
        a.pointwise = bPW.as<double>();
        const dim3 grid((unsigned)G, (unsigned)U);
        DISPATCH_D(h, D, LAUNCH_DIR(directed, k_dyn_accumulate, grid, dim3(IC_NT), h->stream, a));
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(transitions, cnt, n_tr * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hist_up, cnt + n_tr, n_hist * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(node_changes, cnt + n_tr + n_hist, n_ch * sizeof(uint64_t), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipMemcpyAsync(node_turnover, cnt + n_tr + n_hist + n_ch, n_to * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, h->stream));
    if (pointwise) HIPCHK(h, hipMemcpyAsync(pointwise, bPW.p, pw_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DLSM_OK;
}

}  // extern "C"
