// Posterior edge probabilities (no reference counterpart): of p_s = expit(eta_s) of every dyad over S posterior
// samples, in one pass, the mean, the standard deviation (ddof 1) and the equal-tailed credible interval - the
// quantiles at alpha = (1 - level) / 2 and at 1 - alpha as numpy's default defines them: linear interpolation of
// the order statistics at position q (S - 1).  Over the scored dyads (observed and not masked) the posterior mean
// pbar is counted into a reliability table, a Brier sum, the nodes' expected degrees and a histogram of the
// interval's width.
//
// Per-dyad state.  One dyad per thread.  Welford's mean and M2 of p_s in registers; two sorted columns of K
// doubles in LDS, laid out [slot][thread] as kernels_loo.hpp lays out its buffer: the K smallest eta, and the K
// largest stored negated, so that both columns ascend and one insertion routine serves them.  expit is weakly
// monotone: the order statistics of p are expit of those of eta, and only the two or four that the quantiles
// need are ever turned into a probability; the interpolation is done on p.  The first K samples fill a column by
// insertion; after that a sample is inserted only when it beats the column's last slot (a divergent branch, taken
// with probability about K / s, as in kernels_loo.hpp).  A value equal to the last slot stays out: the column
// holds the same multiset either way, so ties count with their multiplicity.  The columns are independent; with
// 2 K > S they hold overlapping samples.  The host derives the slots and weights (ProbaQuantile) and K.
//
// Work: the tiles, the LDS staging and eta are those of a pass over posterior samples (kernels_dyad_pass.hpp),
// with PSIS-LOO's tile height: `rows` = 4, 2 or 1 rows of 64 columns, wavefront = row, so that 2 * rows * 64
// columns of K * 8 bytes fit PROBA_LDS_BUFFER_MAX (the host picks the form; the wavefronts beyond `rows` only help
// staging).
//
// Everything that is accumulated across dyads is an integer added with 64-bit atomics - counts, and probabilities
// in fixed point, proba_fix(x) = llrint(x 2^32) -, so the same call returns the same bits whatever the order.  The
// reliability table and the width histogram are staged per workgroup in LDS (as kernels_conv.hpp stages its
// histograms) and flushed once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_conv.hpp"
#include "kernels_dyad_pass.hpp"
#include "kernels_loo.hpp"
#include "kernels_score.hpp"

namespace dlsm {

constexpr int PROBA_MAX_EDGES = CONV_MAX_EDGES;
constexpr int PROBA_MAX_BINS = 64;          // bins of the reliability table
constexpr size_t PROBA_LDS_BUFFER_MAX = LOO_LDS_BUFFER_MAX;   // both columns; the rest is staging and tables

// A quantile of S ascending values v_(0..S-1) at position fl + g: lerp(v_(prev), v_(next), g), with prev and next
// counted as slots of the column that holds them (from the bottom for the lower quantile, from the top for the
// upper one)
struct ProbaQuantile { int prev, next; double g; };

struct ProbaArgs {
    const double *Xs, *ic, *radii;          // [S][T][N][D], [S][2], [S][N] (DIR)
    const uint32_t *bits, *mask;            // [T][N][W]; mask NULL or a set bit: the dyad is not scored
    const int2 *tiles;                      // [n_tiles] = (row block of `rows` rows, column block)
    int n_tiles, L, S, K, rows, T, N, W;
    ProbaQuantile lower, upper;
    int n_bins;
    const double *edges;                    // [PROBA_MAX_EDGES], padded with +inf
    int n_edges;
    conv_count_t *calib;                    // [T][n_bins][3] = scored dyads, those with y = 1, sum fix(pbar)
    conv_count_t *brier;                    // [T] sum fix((y - pbar)^2)
    conv_count_t *node_sums;                // [T][N][2]: fix(pbar) of dyad (i, j) into slot 0 of i and slot 1 of j
    conv_count_t *hist;                     // [T][n_edges + 1] of upper - lower
    double *pointwise;                      // NULL or [T][N][N][4] = (mean, sd, lower, upper)
};                                          // every output zero on entry

__device__ __forceinline__ conv_count_t proba_fix(double x) {       // x in [0, 1]
    return (conv_count_t)__double2ll_rn(x * 4294967296.0);
}

// expit(eta) = w (eta >= 0) or e w, with e = exp(-|eta|) <= 1, w = 1 / (1 + e): no overflow, no cancellation
__device__ __forceinline__ double proba_expit(double eta) {
    const double e = exp(-fabs(eta));
    const double w = 1.0 / (1.0 + e);
    return eta >= 0.0 ? w : e * w;
}

// numpy's linear interpolation: a + (b - a) t, from b's side for t >= 1/2
__device__ __forceinline__ double proba_lerp(double a, double b, double t) {
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// Sample s (counted from 0) into the ascending column col (slot m at col[m * stride]) of the K smallest values so
// far; top: the column's last slot once it is full (s >= K - 1)
__device__ __forceinline__ void proba_insert(double *col, int stride, int K, int s, double v, double &top) {
    int p = s;
    if (s >= K) {                           // uniform: the column is full
        if (!(v < top)) return;
        p = K - 1;
    }
    while (p > 0) {
        const double below = col[(size_t)(p - 1) * stride];
        if (!(below > v)) break;
        col[(size_t)p * stride] = below;
        --p;
    }
    col[(size_t)p * stride] = v;
    if (s >= K - 1) top = col[(size_t)(K - 1) * stride];
}

// workgroup g = blockIdx.x takes tiles g L .. g L + L - 1 of time step blockIdx.y; dynamic LDS: 2 K rows 64 doubles
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) void k_proba_accumulate(const ProbaArgs a) {
    typedef IcStage<D, DIR> St;
    constexpr int PT = St::PER_THREAD;
    extern __shared__ __attribute__((aligned(16))) double proba_buf[];
    __shared__ double stage[2][St::N];
    __shared__ conv_count_t colred[4][IC_TJ];
    __shared__ conv_count_t lcal[PROBA_MAX_BINS * 3];
    __shared__ unsigned int lhist[CONV_NBINS];
    __shared__ double ledges[PROBA_MAX_EDGES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = blockIdx.y, g = blockIdx.x;
    const int S = a.S, K = a.K, N = a.N, rows = a.rows;
    const int stride = rows * IC_TJ;
    const bool active = wv < rows;                            // wavefront-uniform
    double *col_lo = proba_buf + (active ? wv * IC_TJ + lane : 0);
    double *col_hi = col_lo + (size_t)K * stride;
    const double inf = __builtin_inf();
    if (tid < PROBA_MAX_BINS * 3) lcal[tid] = 0ull;
    if (tid < CONV_NBINS) lhist[tid] = 0u;
    if (tid < PROBA_MAX_EDGES) ledges[tid] = a.edges[tid];
    __syncthreads();
    conv_count_t brier = 0ull;                                // this thread's dyads so far
    const int q0 = g * a.L, q1 = min(a.n_tiles, q0 + a.L);
    for (int q = q0; q < q1; ++q) {
        const int i0 = a.tiles[q].x * rows, j0 = a.tiles[q].y * IC_TJ;
        const int i = i0 + wv, j = j0 + lane;
        const bool exists = active && i < N && j < N && (DIR ? i != j : i < j);
        bool scored = exists;
        double y = 0.0;
        if (exists) {
            const size_t at = ((size_t)t * N + i) * a.W + (j >> 5);
            y = (double)((a.bits[at] >> (j & 31)) & 1u);
            if (a.mask) {
                uint32_t mb = a.mask[at] >> (j & 31);
                if (!DIR) mb |= a.mask[((size_t)t * N + j) * a.W + (i >> 5)] >> (i & 31);
                scored = !(mb & 1u);
            }
        }
        double mean = 0.0, m2 = 0.0;        // Welford over p_s
        double top_lo = inf, top_hi = inf;  // the columns' last slots once they are full
        dyad_stage_first<D, DIR>(stage[0], a.Xs, a.ic, a.radii, t, N, i0, j0, tid);
        __syncthreads();
        for (int s = 0; s < S; ++s) {
            const int cur = s & 1;
            const double *sb = stage[cur];
            double pre[PT];           // the next sample's block, in flight under this sample's arithmetic
            if (s + 1 < S) dyad_stage_prefetch<D, DIR>(pre, a.Xs, a.ic, a.radii, s + 1, a.T, t, N, i0, j0, tid);
            if (active) {
                const DyadColumn<D> dc = dyad_column<D, DIR>(sb, lane);
                const double eta = dyad_eta<D, DIR>(sb, wv, dc);
                const double p = proba_expit(eta);
                const double dl = p - mean;
                mean += dl / (double)(s + 1);
                m2 = fma(dl, p - mean, m2);
                proba_insert(col_lo, stride, K, s, eta, top_lo);
                proba_insert(col_hi, stride, K, s, -eta, top_hi);
            }
            if (s + 1 < S) dyad_stage_commit<D, DIR>(stage[cur ^ 1], pre, tid);
            __syncthreads();
        }
        // the tile's dyads: the interval, the pointwise quadruple, and - if scored - the integer tables
        conv_count_t fix = 0ull;            // fix(pbar) of a scored dyad, else 0: adds nothing to a node
        if (exists) {
            const double lower = proba_lerp(proba_expit(col_lo[(size_t)a.lower.prev * stride]),
                                            proba_expit(col_lo[(size_t)a.lower.next * stride]), a.lower.g);
            const double upper = proba_lerp(proba_expit(-col_hi[(size_t)a.upper.prev * stride]),
                                            proba_expit(-col_hi[(size_t)a.upper.next * stride]), a.upper.g);
            if (a.pointwise) {
                double2 *out = (double2 *)(a.pointwise + (((size_t)t * N + i) * N + j) * 4);
                out[0] = make_double2(mean, sqrt(m2 / (double)(S - 1)));
                out[1] = make_double2(lower, upper);
            }
            if (scored) {
                fix = proba_fix(mean);
                // (the clamps hold for every pbar in [0, 1]; they are there for a NaN, positions that are not finite)
                const int bin = min(max((int)(mean * (double)a.n_bins), 0), a.n_bins - 1);
                atomicAdd(&lcal[bin * 3], 1ull);
                if (y != 0.0) atomicAdd(&lcal[bin * 3 + 1], 1ull);
                atomicAdd(&lcal[bin * 3 + 2], fix);
                const double r = y - mean;
                brier += proba_fix(r * r);
                atomicAdd(&lhist[conv_bin(ledges, a.n_edges, upper - lower)], 1u);
            }
        }
        // the row's node, then the columns' nodes through LDS (0 changes nothing: no atomic for it)
        const conv_count_t row_fix = score_wave_sum(fix);
        if (lane == 0 && i < N && row_fix)
            __hip_atomic_fetch_add(a.node_sums + ((size_t)t * N + i) * 2, row_fix, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        colred[wv][lane] = fix;
        __syncthreads();          // also: every thread is done with the last sample's stage buffer
        if (wv == 0) {
            const conv_count_t cf = (colred[0][lane] + colred[1][lane]) + (colred[2][lane] + colred[3][lane]);
            if (j < N && cf)
                __hip_atomic_fetch_add(a.node_sums + ((size_t)t * N + j) * 2 + 1, cf, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();          // colred and stage[0] are free for the next tile
    }
    // the workgroup's tables (the last barrier of the tile loop ordered the LDS atomics before these reads)
    brier = score_wave_sum(brier);
    if (lane == 0 && brier)
        __hip_atomic_fetch_add(a.brier + t, brier, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < a.n_bins * 3 && lcal[tid])
        __hip_atomic_fetch_add(a.calib + (size_t)t * a.n_bins * 3 + tid, lcal[tid], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    if (tid <= a.n_edges && lhist[tid])
        __hip_atomic_fetch_add(a.hist + (size_t)t * (a.n_edges + 1) + tid, (conv_count_t)lhist[tid],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace dlsm
