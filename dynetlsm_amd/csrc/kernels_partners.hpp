// Per-node link prediction (no reference counterpart): for every node i and time step t the k eligible partners j
// that come first by the posterior-mean edge probability pbar(t, i, j) of kernels_topk.hpp - descending, or
// ascending with largest = 0 -, ties by j ascending, k <= 64, with the standard deviation of p_s and the bit of the
// network.  No (T, N, N) array is formed and nothing is sorted on the host.
//
// The selection of kernels_topk.hpp (one histogram of rank keys per time step, a threshold, a second pass) does not
// transfer: a row-wise selection would need a histogram per (t, node).  A row's list is short instead, so it is kept
// sorted while the row's columns stream by:
//
//   k_partners_select   one workgroup owns one row block (IcPlan<D>::TI rows) of one time step and walks all its
//                       column tiles j0 = 0, 64, ...  Per tile the sample loop is topk_tile_samples<D, DIR, true>,
//                       so pbar and sd of a dyad have the bits they have in k_topk_emit: the same instructions on
//                       the same inputs in the same order.  Then each wavefront merges the 64 candidates (one per
//                       lane) of each of its DPT rows into that row's running list, which lives one entry per lane
//                       in the registers of the wavefront: pbar, sd and j | y << 31.  Empty slots hold a value that
//                       no probability reaches (-1, or 2 with largest = 0) and j = -1.
//
// The merge of one row: a ballot of "eligible and strictly ahead of the list's k-th entry" selects the lanes to insert
// (entries behind the k-th are never written out, so a candidate that does not beat it cannot matter).  They are taken
// from the lowest lane up: the candidate is broadcast, its position is the number of entries that rank before it -
// those it is not strictly ahead of -, and the entries behind it move one lane up.  Columns arrive in ascending j and
// an equal value never displaces an earlier one, so ties come out in j order without a comparison on j.  A row whose
// probabilities rise with j inserts every candidate (64 per tile), a typical one a few per tile once the list is full.
//
// Undirected chains: every row needs both triangles, so all j != i are visited and the cost is about N^2 dyad
// evaluations per sample and time step, against N^2 / 2 for k_topk_count.  eta is symmetric to the bit there (the
// squares of x_i - x_j and x_j - x_i agree), so a dyad has the same pbar and sd in both of its rows.  The network bit
// and the mask bits are read as kernels_topk.hpp reads them: the bit of (min(i, j), max(i, j)), either orientation of
// the mask excluding the dyad.
//
// Not done: splitting a row's columns over several workgroups, for a grid T ceil(N / TI) too small to fill the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_dyad_pass.hpp"
#include "kernels_topk.hpp"

namespace dlsm {

constexpr int PARTNERS_K_MAX = 64;                  // entries of a row's list: one per lane
constexpr uint32_t PARTNERS_EMPTY = 0xFFFFFFFFu;    // j | y << 31 of an empty slot

// The tile's dyads of this thread (rows i0 + 4 k + wv, column j) at time step t, as topk_tile_bits, but the dyad
// exists when i != j for both models; an undirected chain reads the bits of (min(i, j), max(i, j)).  A sibling, not
// a flag: kernels_topk.hpp and the code of its kernels stay as they are.
template <int D, bool DIR>
__device__ __forceinline__ void partners_tile_bits(const uint32_t *bits, const uint32_t *mask, int among, int t,
                                                   int N, int W, int i0, int j, int wv, uint32_t &elig,
                                                   uint32_t &ybits) {
    elig = 0; ybits = 0;
#pragma unroll
    for (int k = 0; k < IcPlan<D>::DPT; ++k) {
        const int i = i0 + 4 * k + wv;
        if (!(i < N && j < N && i != j)) continue;
        const int a = DIR ? i : min(i, j), b = DIR ? j : max(i, j);
        const size_t at = ((size_t)t * N + a) * W + (b >> 5);
        const uint32_t y = (bits[at] >> (b & 31)) & 1u;
        uint32_t mb = 0;
        if (mask) {
            mb = mask[at] >> (b & 31);
            if (!DIR) mb |= mask[((size_t)t * N + b) * W + (a >> 5)] >> (a & 31);
            mb &= 1u;
        }
        bool ok;
        switch (among) {
            case TOPK_NON_TIES: ok = !mb && !y; break;
            case TOPK_TIES: ok = !mb && y; break;
            case TOPK_OBSERVED: ok = !mb; break;
            case TOPK_MISSING: ok = mb; break;
            default: ok = true;
        }
        elig |= (uint32_t)ok << k;
        ybits |= y << k;
    }
}

// a ranks strictly before b
__device__ __forceinline__ bool partners_ahead(double a, double b, bool top) { return top ? a > b : a < b; }

// One row's candidates of a tile - lane: column, `ok`: eligible, (p, sd, jy) - into its list (lp, ls, lj), one entry
// per lane, sorted; kk entries count.  Called by whole wavefronts.
__device__ __forceinline__ void partners_merge(bool top, int kk, int lane, bool ok, double p, double sd, uint32_t jy,
                                               double &lp, double &ls, uint32_t &lj) {
    // (read by every lane: a shuffle under `ok &&` would run with the other lanes switched off, and a lane that is
    // switched off hands out 0, not its entry)
    const double kth = __shfl(lp, kk - 1);
    unsigned long long todo = __ballot(ok && partners_ahead(p, kth, top));
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const double cp = __shfl(p, src), cs = __shfl(sd, src);
        const uint32_t cj = __shfl(jy, src);
        const int pos = __popcll(__ballot(!partners_ahead(cp, lp, top)));
        if (pos >= kk) continue;            // an earlier insertion moved the k-th entry ahead of this one
        const double up_p = __shfl_up(lp, 1), up_s = __shfl_up(ls, 1);
        const uint32_t up_j = __shfl_up(lj, 1);
        if (lane > pos) { lp = up_p; ls = up_s; lj = up_j; }
        else if (lane == pos) { lp = cp; ls = cs; lj = cj; }
    }
}

// Xs [S][T][N][D], ic [S][2], radii [S][N] (DIR); bits [T][N][W]; mask NULL or [T][N][W]; row_blocks [n_blocks]
// ascending in 0 .. ceil(N / TI) - 1.  Workgroup blockIdx.x takes row block row_blocks[blockIdx.x % n_blocks] of
// time step blockIdx.x / n_blocks.  partner, y [T][N][kk], value [T][N][kk] = (pbar, sd), eligible [T][N]: the rows
// of the listed blocks get eligible and their min(kk, eligible) entries, the rest is the caller's padding.
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) void k_partners_select(
    const double *__restrict__ Xs, const double *__restrict__ ic, const double *__restrict__ radii,
    const uint32_t *__restrict__ bits, const uint32_t *__restrict__ mask, const int32_t *__restrict__ row_blocks,
    int n_blocks, int S, int T, int N, int W, int among, int largest, int kk, int32_t *__restrict__ partner,
    double2 *__restrict__ value, int32_t *__restrict__ y, int32_t *__restrict__ eligible) {
    typedef IcStage<D, DIR> St;
    constexpr int DPT = IcPlan<D>::DPT, TI = IcPlan<D>::TI;
    __shared__ double stage[2 * St::N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = blockIdx.x / n_blocks, i0 = row_blocks[blockIdx.x % n_blocks] * TI;
    const bool top = largest != 0;
    double lp[DPT], ls[DPT];
    uint32_t lj[DPT];
    int count[DPT];
#pragma unroll
    for (int k = 0; k < DPT; ++k) { lp[k] = top ? -1.0 : 2.0; ls[k] = 0.0; lj[k] = PARTNERS_EMPTY; count[k] = 0; }
    for (int j0 = 0; j0 < N; j0 += IC_TJ) {
        const int j = j0 + lane;
        uint32_t elig, ybits;
        partners_tile_bits<D, DIR>(bits, mask, among, t, N, W, i0, j, wv, elig, ybits);
        double psum[DPT], mean[DPT], m2[DPT];
        topk_tile_samples<D, DIR, true>(stage, Xs, ic, radii, S, T, t, N, i0, j0, tid, psum, mean, m2);
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
            const bool ok = (elig >> k) & 1u;
            const unsigned long long any = __ballot(ok);
            if (!any) continue;
            count[k] += __popcll(any);
            partners_merge(top, kk, lane, ok, topk_pbar(psum[k], S), sqrt(m2[k] / (double)(S - 1)),
                           (uint32_t)j | ((ybits >> k) & 1u) << 31, lp[k], ls[k], lj[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
        const int i = i0 + 4 * k + wv;
        if (i >= N) continue;
        const size_t row = (size_t)t * N + i;
        if (lane < kk && lj[k] != PARTNERS_EMPTY) {
            const size_t at = row * kk + lane;
            partner[at] = (int32_t)(lj[k] & 0x7FFFFFFFu);
            y[at] = (int32_t)(lj[k] >> 31);
            value[at] = make_double2(lp[k], ls[k]);
        }
        if (lane == 0) eligible[row] = count[k];
    }
}

}  // namespace dlsm
