// C-ABI of the per-node link prediction (kernels_partners.hpp) on capi_samples.hpp's pass driver; the error macros
// and ProfScope are capi.hip's.  The reference has no counterpart.
#pragma once
#include "capi_samples.hpp"
#include "kernels_partners.hpp"

extern "C" {

int dlsm_partners_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                             const double *intercepts, const double *radii, int S, int among, int largest, int k,
                             const int32_t *row_blocks, int n_row_blocks, int32_t *partner, double *value,
                             int32_t *y, int32_t *eligible) {
    if (int rc = pass_check_inputs(h, h && bits && Xs && intercepts && partner && value && y && eligible, bits,
                                   radii, S, 2)) return rc;
    NEED(h, among >= 0 && among < TOPK_AMONG_COUNT, "among=%d is not in 0..%d", among, TOPK_AMONG_COUNT - 1);
    NEED(h, largest == 0 || largest == 1, "largest=%d is not 0 or 1", largest);
    NEED(h, k >= 1 && k <= PARTNERS_K_MAX, "k=%d is not in 1..%d, the entries of a node's list", k, PARTNERS_K_MAX);
    NEED(h, among != TOPK_MISSING || mask, "among = missing needs the mask");
    const int T = h->T, N = h->N, D = h->D;
    const int TI = D <= 4 ? IcPlan<1>::TI : IcPlan<8>::TI;
    const int n_all = (N + TI - 1) / TI;
    std::vector<int32_t> blocks;
    if (row_blocks) {
        NEED(h, n_row_blocks >= 0 && n_row_blocks <= n_all, "n_row_blocks=%d is not in 0..%d", n_row_blocks, n_all);
        for (int q = 0; q < n_row_blocks; ++q) {
            NEED(h, row_blocks[q] >= 0 && row_blocks[q] < n_all, "row_blocks[%d]=%d is not a block of %d rows in "
                 "0..%d", q, (int)row_blocks[q], TI, n_all - 1);
            NEED(h, !q || row_blocks[q] > row_blocks[q - 1], "row_blocks must ascend strictly (entry %d)", q);
        }
        blocks.assign(row_blocks, row_blocks + n_row_blocks);
    } else {
        for (int q = 0; q < n_all; ++q) blocks.push_back(q);
    }
    const size_t n_blocks = blocks.size(), rows = (size_t)T * N;
    if (n_blocks * (size_t)T >= 2147483648.0)
        FAIL(h, DLSM_E_LIMIT, "T=%d time steps of %zu row blocks: the grid holds fewer than 2^31 workgroups", T,
             n_blocks);
    TracePass p(h, S);
    const int iBlocks = p.buf<int32_t>(std::max<size_t>(1, n_blocks), 0, n_blocks ? blocks.data() : nullptr);
    const int iPartner = p.out(partner, rows * k), iValue = p.out(value, rows * k * 2), iY = p.out(y, rows * k);
    const int iEligible = p.out(eligible, rows);
    if (int rc = p.begin(bits, mask, Xs, intercepts, radii)) return rc;
    // the padding: partner = y = eligible = -1 and a NaN, every byte set; the kernel writes the entries there are
    HIPCHK(h, hipMemsetAsync(p.dev(iPartner), 0xFF, rows * k * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(p.dev(iValue), 0xFF, rows * k * sizeof(double2), h->stream));
    HIPCHK(h, hipMemsetAsync(p.dev(iY), 0xFF, rows * k * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(p.dev(iEligible), 0xFF, rows * sizeof(int32_t), h->stream));
    if (n_blocks) {
        ProfScope ps(h, DLSM_K_PARTNERS);
        DISPATCH_D(h, D, LAUNCH_DIR(p.directed, k_partners_select, dim3((unsigned)(n_blocks * T)), dim3(IC_NT),
                                    h->stream, p.X(), p.B(), p.R(), p.bits(), p.mask(), p.at<int32_t>(iBlocks),
                                    (int)n_blocks, S, T, N, h->W, among, largest, k, p.at<int32_t>(iPartner),
                                    p.at<double2>(iValue), p.at<int32_t>(iY), p.at<int32_t>(iEligible)));
        HIPCHK(h, hipGetLastError());
    }
    return p.finish();
}

}  // extern "C"
