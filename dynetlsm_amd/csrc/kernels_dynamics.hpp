// Tie dynamics (no reference counterpart): the posterior change of every edge probability between consecutive
// time steps.  A step u = t -> t + 1 (u = t = 0 .. T - 2) of a dyad, over the S posterior samples, with
// p_{s,t} = expit(eta_{s,t}):
//
//     delta_mean, delta_sd (ddof 1)  of  d_s = p_{s,t+1} - p_{s,t}
//     up, down                       the samples with eta_{s,t+1} > eta_{s,t}, and with <  (a tie counts as neither)
//     pbar_t, pbar_{t+1}, persist    mean_s p_{s,t}, mean_s p_{s,t+1}, mean_s p_{s,t} p_{s,t+1}
//
// - the joint posterior of two time steps, which no marginal summary of one time step gives.  Over the scored steps
// (the dyad is unmasked at t and at t + 1) the class of the observed pair c = 2 y_t + y_{t+1} collects the expected
// transition counts, up is counted into a histogram, and every node counts its dyads that moved in one direction
// in at least min_count samples and sums |delta_mean|.
//
// Per-dyad state, in registers: Welford's mean and M2 of d (a constant trace gives M2 = 0 exactly), the three sums
// of probabilities and the two counters.  A thread adds its samples in order: the values of a dyad do not depend on
// the launch.
//
// Work: the tiles, the LDS staging and eta are those of a pass over posterior samples (kernels_dyad_pass.hpp):
// IcPlan<D>::TI x 64 dyads, lane = column, wavefront + 4 k = row.  Per sample the blocks of both time steps are
// staged (two time steps x two buffers x IcStage::N doubles, 23.1 KB at D = 8 directed), one barrier per sample.
// A thread holds DYN_DPT = 4 dyads at a time - 12 registers of state each, next to two columns and two chains of
// sqrt, exp and division per dyad: with IcPlan's 8 at D <= 4 the kernel needs more than 256 vector registers and
// parks some in accumulation registers -, so at D <= 4 a tile is walked in two passes over the samples, rows
// 0 .. 15 and 16 .. 31.  The kernel asks for two wavefronts per SIMD (256 vector registers); every instantiation
// fits without a spill.
// Both etas of a step are dyad_eta on a stage buffer: the same instructions on the same kind of input, so
// eta_{s,t+1} == eta_{s,t} holds exactly when the two time steps' inputs are equal.  An interior time step's eta is
// computed twice, as t + 1 of one step and as t of the next.
//
// Everything that is accumulated across dyads is an integer added with 64-bit atomics - counts, and probabilities
// in fixed point, proba_fix (kernels_proba.hpp) -, so the same call returns the same bits whatever the order.  The
// transition table and the histogram are staged per workgroup in LDS and flushed once; a node's sums are reduced
// over the wavefront (rows) and through LDS (columns) before the global atomic, as kernels_proba.hpp does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_conv.hpp"
#include "kernels_dyad_pass.hpp"
#include "kernels_proba.hpp"
#include "kernels_score.hpp"

namespace dlsm {

constexpr int DYN_MAX_BINS = PROBA_MAX_BINS;        // bins of the histogram of up
constexpr int DYN_DPT = 4;                          // dyads of a thread in registers at a time

struct DynArgs {
    const double *Xs, *ic, *radii;          // [S][T][N][D], [S][2], [S][N] (DIR)
    const uint32_t *bits, *mask;            // [T][N][W]; mask NULL or a set bit: the dyad is not scored at that t
    const int2 *tiles;                      // [n_tiles] = (row block, column block)
    int n_tiles, L, S, T, N, W;
    int min_count, n_bins;
    conv_count_t *transitions;              // [T-1][4][4]: class c: steps, sums of fix(pbar_t, pbar_{t+1}, persist)
    conv_count_t *hist_up;                  // [T-1][n_bins]: steps per bin min(up n_bins / S, n_bins - 1)
    conv_count_t *node_changes;             // [T-1][N][4]: up >= min_count: slot 0 of i, 1 of j; down: 2 of i, 3 of j
    conv_count_t *node_turnover;            // [T-1][N][2]: fix(|delta_mean|) into slot 0 of i and slot 1 of j
    double *pointwise;                      // NULL or [T-1][N][N][4] = (delta_mean, delta_sd, prob_up, prob_down)
};                                          // every output zero on entry

// *p += v unless v is 0, which changes nothing
__device__ __forceinline__ void dyn_add(conv_count_t *p, conv_count_t v) {
    if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// workgroup g = blockIdx.x takes tiles g L .. g L + L - 1 of step blockIdx.y
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) __attribute__((amdgpu_waves_per_eu(2))) void k_dyn_accumulate(
    const DynArgs a) {
    typedef IcStage<D, DIR> St;
    constexpr int DPT = DYN_DPT, PASSES = IcPlan<D>::DPT / DYN_DPT, TI = IcPlan<D>::TI, PT = St::PER_THREAD;
    static_assert(PASSES * DYN_DPT == IcPlan<D>::DPT, "a tile is a whole number of passes");
    __shared__ double stage[2][2][St::N];                     // [time step of the pair][buffer]
    __shared__ conv_count_t colred[2][4][IC_TJ];
    __shared__ conv_count_t ltrans[16];
    __shared__ unsigned int lhist[DYN_MAX_BINS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = blockIdx.y, g = blockIdx.x;
    const int S = a.S, N = a.N;
    if (tid < 16) ltrans[tid] = 0ull;
    if (tid < DYN_MAX_BINS) lhist[tid] = 0u;
    __syncthreads();
    const double dS = (double)S;
    const int q0 = g * a.L, q1 = min(a.n_tiles, q0 + a.L);
    for (int q = q0; q < q1; ++q) {
        const int i0 = a.tiles[q].x * TI, j0 = a.tiles[q].y * IC_TJ;
        const int j = j0 + lane;
        // the tile's dyads of this thread: which steps are scored, and the network's bits at t and at t + 1
        uint32_t valid0, valid1, y0, y1;
        dyad_tile_bits<D, DIR>(a.bits, a.mask, t, N, a.W, i0, j, wv, valid0, y0);
        dyad_tile_bits<D, DIR>(a.bits, a.mask, t + 1, N, a.W, i0, j, wv, valid1, y1);
        conv_count_t col_flags = 0ull, col_turn = 0ull;        // this thread's column over the tile's rows
#pragma unroll 1
        for (int h = 0; h < PASSES; ++h) {                    // rows 4 (h DPT + k) + wv of the tile
            const uint32_t scored = (valid0 & valid1) >> (h * DPT);
            const uint32_t yb0 = y0 >> (h * DPT), yb1 = y1 >> (h * DPT);
            double mean[DPT], m2[DPT], sp0[DPT], sp1[DPT], spp[DPT];
            int up[DPT], down[DPT];
#pragma unroll
            for (int k = 0; k < DPT; ++k) { mean[k] = m2[k] = sp0[k] = sp1[k] = spp[k] = 0.0; up[k] = down[k] = 0; }
            dyad_stage_first<D, DIR>(stage[0][0], a.Xs, a.ic, a.radii, t, N, i0, j0, tid);
            dyad_stage_first<D, DIR>(stage[1][0], a.Xs, a.ic, a.radii, t + 1, N, i0, j0, tid);
            __syncthreads();
            for (int s = 0; s < S; ++s) {
                const int cur = s & 1;
                const double *sb0 = stage[0][cur], *sb1 = stage[1][cur];
                double pre0[PT], pre1[PT];    // the next sample's blocks, in flight under this sample's arithmetic
                if (s + 1 < S) {
                    dyad_stage_prefetch<D, DIR>(pre0, a.Xs, a.ic, a.radii, s + 1, a.T, t, N, i0, j0, tid);
                    dyad_stage_prefetch<D, DIR>(pre1, a.Xs, a.ic, a.radii, s + 1, a.T, t + 1, N, i0, j0, tid);
                }
                const DyadColumn<D> c0 = dyad_column<D, DIR>(sb0, lane), c1 = dyad_column<D, DIR>(sb1, lane);
                const double inv = 1.0 / (double)(s + 1);
#pragma unroll
                for (int k = 0; k < DPT; ++k) {
                    const double eta0 = dyad_eta<D, DIR>(sb0, 4 * (h * DPT + k) + wv, c0);
                    const double eta1 = dyad_eta<D, DIR>(sb1, 4 * (h * DPT + k) + wv, c1);
                    const double p0 = proba_expit(eta0), p1 = proba_expit(eta1);
                    const double d = p1 - p0;
                    const double dl = d - mean[k];
                    mean[k] = fma(dl, inv, mean[k]);
                    m2[k] = fma(dl, d - mean[k], m2[k]);
                    sp0[k] += p0;
                    sp1[k] += p1;
                    spp[k] = fma(p0, p1, spp[k]);
                    up[k] += eta1 > eta0;
                    down[k] += eta1 < eta0;
                }
                if (s + 1 < S) {
                    dyad_stage_commit<D, DIR>(stage[0][cur ^ 1], pre0, tid);
                    dyad_stage_commit<D, DIR>(stage[1][cur ^ 1], pre1, tid);
                }
                __syncthreads();
            }
            // the tile's dyads: the pointwise quadruple, and - if the step is scored - the integer tables.  A node's
            // counts travel packed: up >= min_count in the low word, down >= min_count in the high one.
#pragma unroll
            for (int k = 0; k < DPT; ++k) {
                const int i = i0 + 4 * (h * DPT + k) + wv;
                const bool exists = i < N && j < N && (DIR ? i != j : i < j);
                if (exists && a.pointwise) {
                    double2 *out = (double2 *)(a.pointwise + (((size_t)t * N + i) * N + j) * 4);
                    out[0] = make_double2(mean[k], sqrt(m2[k] / (double)(S - 1)));
                    out[1] = make_double2((double)up[k] / dS, (double)down[k] / dS);
                }
                conv_count_t flags = 0ull, turn = 0ull;           // 0 changes nothing: no atomic for it
                if ((scored >> k) & 1u) {
                    const int c = (int)(2u * ((yb0 >> k) & 1u) + ((yb1 >> k) & 1u));
                    atomicAdd(&ltrans[c * 4], 1ull);
                    atomicAdd(&ltrans[c * 4 + 1], proba_fix(sp0[k] / dS));
                    atomicAdd(&ltrans[c * 4 + 2], proba_fix(sp1[k] / dS));
                    atomicAdd(&ltrans[c * 4 + 3], proba_fix(spp[k] / dS));
                    const long long b = (long long)up[k] * a.n_bins / S;
                    atomicAdd(&lhist[min((int)b, a.n_bins - 1)], 1u);
                    flags = (up[k] >= a.min_count ? 1ull : 0ull) | (down[k] >= a.min_count ? 1ull << 32 : 0ull);
                    turn = proba_fix(fabs(mean[k]));
                }
                // the row's node ...
                const conv_count_t row_flags = score_wave_sum(flags), row_turn = score_wave_sum(turn);
                if (lane == 0 && i < N) {
                    conv_count_t *nc = a.node_changes + ((size_t)t * N + i) * 4;
                    dyn_add(nc, row_flags & 0xFFFFFFFFull);
                    dyn_add(nc + 2, row_flags >> 32);
                    dyn_add(a.node_turnover + ((size_t)t * N + i) * 2, row_turn);
                }
                col_flags += flags;
                col_turn += turn;
            }
        }                     // (the sample loop's last barrier: the next pass may write the first stage buffers)
        // ... then the columns' nodes through LDS
        colred[0][wv][lane] = col_flags;
        colred[1][wv][lane] = col_turn;
        __syncthreads();          // also: every thread is done with the last sample's stage buffers
        if (wv == 0 && j < N) {
            const conv_count_t (*cr)[4][IC_TJ] = colred;
            const conv_count_t cf = (cr[0][0][lane] + cr[0][1][lane]) + (cr[0][2][lane] + cr[0][3][lane]);
            const conv_count_t ct = (cr[1][0][lane] + cr[1][1][lane]) + (cr[1][2][lane] + cr[1][3][lane]);
            conv_count_t *nc = a.node_changes + ((size_t)t * N + j) * 4;
            dyn_add(nc + 1, cf & 0xFFFFFFFFull);
            dyn_add(nc + 3, cf >> 32);
            dyn_add(a.node_turnover + ((size_t)t * N + j) * 2 + 1, ct);
        }
        __syncthreads();          // colred and the first stage buffers are free for the next tile
    }
    // the workgroup's tables (the last barrier of the tile loop ordered the LDS atomics before these reads)
    if (tid < 16) dyn_add(a.transitions + (size_t)t * 16 + tid, ltrans[tid]);
    if (tid < a.n_bins) dyn_add(a.hist_up + (size_t)t * a.n_bins + tid, (conv_count_t)lhist[tid]);
}

}  // namespace dlsm
