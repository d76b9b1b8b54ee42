// C-ABI of the information criteria (kernels_ic.hpp) on capi_samples.hpp's pass driver; the error macros are
// capi.hip's.  The reference has no counterpart.
#pragma once
#include "capi_samples.hpp"
#include "kernels_ic.hpp"

namespace {

constexpr size_t IC_PARTIAL_BYTES = (size_t)256 << 20;    // bound of the per-workgroup sample partials

}  // namespace

extern "C" {

int dlsm_ic_accumulate(dlsm_chain *h, const uint32_t *bits, const double *Xs, const double *intercepts,
                       const double *radii, int S, double *totals, double *sample_loglik, double *pointwise) {
    if (int rc = pass_check_inputs(h, h && bits && Xs && intercepts && totals && sample_loglik, bits, radii, S, 1))
        return rc;
    const int T = h->T, N = h->N, D = h->D;
    TracePass p(h, S);
    // tiles per workgroup: as few as keep the sample partials [T][G][S] within IC_PARTIAL_BYTES
    const PassGrid g = pass_grid(p.n_tiles, std::max<size_t>(1, IC_PARTIAL_BYTES / ((size_t)T * S * sizeof(double))));
    const int part_tot = p.buf<double>((size_t)T * g.G * IC_NTOT);
    const int part_s = p.buf<double>((size_t)T * g.G, PASS_PER_SAMPLE);
    const int tot = p.out(totals, (size_t)T * IC_NTOT);
    const int sl = p.out(sample_loglik, T, PASS_PER_SAMPLE);
    const int pw = p.out(pointwise, (size_t)T * N * N * 2, PASS_ZERO | PASS_OPTIONAL);
    if (int rc = p.begin(bits, nullptr, Xs, intercepts, radii)) return rc;
    DISPATCH_D(h, D, LAUNCH_DIR(p.directed, k_ic_accumulate, dim3((unsigned)g.G, (unsigned)T), dim3(IC_NT), h->stream,
                                p.X(), p.B(), p.R(), p.bits(), p.tiles(), p.n_tiles, g.L, S, T, N, h->W,
                                p.at<double>(part_tot), p.at<double>(part_s), p.at<double>(pw)));
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_ic_reduce_totals, dim3((unsigned)T), dim3(IC_NT), 0, h->stream, p.at<double>(part_tot), g.G,
                       p.at<double>(tot));
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_ic_reduce_samples, dim3((unsigned)((S + 63) / 64), (unsigned)T), dim3(IC_NT), 0, h->stream,
                       p.at<double>(part_s), g.G, S, T, p.at<double>(sl));
    HIPCHK(h, hipGetLastError());
    return p.finish();
}

}  // extern "C"
