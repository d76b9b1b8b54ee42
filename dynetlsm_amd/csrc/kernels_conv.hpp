// Convergence of every dyad (no reference counterpart): split R-hat and a batch-means effective sample size of
// the linear predictor eta_s of dyad (t, i, j) over S = M h samples, M segments (the two halves of every chain)
// of h samples each, segment after segment.  eta (conv_eta, kernels_dyad_pass.hpp) is invariant to rotation,
// reflection, translation and label switching, so chains pool without alignment.  Per dyad, in eight float64
// registers and without storing the series:
//
//     segment m:   Welford's mean_m, M2_m;  at its end  sw += M2_m / (h - 1)  and (mm, mM2), Welford's mean and
//                  M2 of the segment means, take mean_m
//     batch q:     the samples [q b, (q + 1) b) of a segment, q < a = h / b (the tail of a segment enters no
//                  batch): the running sum bs; at its end (bm, bM2), Welford's mean and M2 of all batch means,
//                  take bs / b
//     W = sw / M,  B = h mM2 / (M - 1),  var+ = (h - 1) / h W + B / h,  v_bm = b bM2 / (M a - 1)
//     rhat = sqrt(var+ / W)     (W == 0: 1 if B == 0, else +inf)
//     ess  = S var+ / v_bm      (v_bm == 0: S if var+ == 0, else +inf; not capped)
//
// Segment and batch boundaries depend on s alone: they are uniform branches.  Finite inputs give no NaN (every
// M2 is a sum of products of two differences of one sign).
//
// Outputs.  Both quantities are >= 0 or +inf, so a float64's bit pattern orders as an unsigned 64-bit integer.
//   hist_rhat [T][n_r + 1], hist_ess [T][n_e + 1]: the bin of a value is the number of edges <= it; counted in
//     LDS over the workgroup's tiles, then one 64-bit integer atomic add per bin that is not empty
//   node_rhat [T][N] (max), node_ess [T][N] (min) over the dyads that contain the node, as row or as column:
//     rows are reduced across the lanes, columns across a thread's rows and the four wavefronts, then one 64-bit
//     integer atomic max / min per node and tile; the caller initialises them to 0 / +inf
//   pointwise NULL or [T][N][N][2] = (rhat, ess)
// Only integer atomics: the same bits on every call.
//
// Tiling, LDS staging of the samples and the tile list are the shared ones of a pass over posterior samples
// (kernels_dyad_pass.hpp), eta its conv_eta; the network itself is not read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_dyad_pass.hpp"

namespace dlsm {

constexpr int CONV_MAX_EDGES = 16;
constexpr int CONV_NBINS = CONV_MAX_EDGES + 1;

typedef unsigned long long conv_count_t;

// number of edges <= v (searchsorted right) of edges [CONV_MAX_EDGES], ascending, the entries from n on +inf;
// v = +inf: n
__device__ __forceinline__ int conv_bin(const double *edges, int n, double v) {
    int bin = 0;
#pragma unroll
    for (int e = 0; e < CONV_MAX_EDGES; ++e) bin += edges[e] <= v ? 1 : 0;
    return min(bin, n);
}

// max / min over the wavefront, in every lane (all 64 lanes active; no NaN)
__device__ __forceinline__ double conv_wave_max(double v) {
    v = fmax(v, dpp_move<0xB1>(v));
    v = fmax(v, dpp_move<0x4E>(v));
    v = fmax(v, dpp_move<0x141>(v));
    v = fmax(v, dpp_move<0x140>(v));
    return fmax(fmax(lane_value(v, 0), lane_value(v, 16)), fmax(lane_value(v, 32), lane_value(v, 48)));
}
__device__ __forceinline__ double conv_wave_min(double v) {
    v = fmin(v, dpp_move<0xB1>(v));
    v = fmin(v, dpp_move<0x4E>(v));
    v = fmin(v, dpp_move<0x141>(v));
    v = fmin(v, dpp_move<0x140>(v));
    return fmin(fmin(lane_value(v, 0), lane_value(v, 16)), fmin(lane_value(v, 32), lane_value(v, 48)));
}

// Xs [S][T][N][D], ic [S][2], radii [S][N] (DIR), S = M h; tiles [n_tiles] = (row block, column block);
// workgroup g = blockIdx.x takes tiles g L .. g L + L - 1 of time step blockIdx.y.
// edges [2][CONV_MAX_EDGES]: those of rhat, those of ess, each padded with +inf.
// hist_rhat [T][n_rhat + 1], hist_ess [T][n_ess + 1] zero on entry; node_rhat [T][N] 0 on entry,
// node_ess [T][N] +inf on entry; pointwise NULL or [T][N][N][2].
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) void k_conv_accumulate(
    const double *__restrict__ Xs, const double *__restrict__ ic, const double *__restrict__ radii,
    const int2 *__restrict__ tiles, int n_tiles, int L, int M, int h, int b, int T, int N,
    const double *__restrict__ edges, int n_rhat, int n_ess, conv_count_t *__restrict__ hist_rhat,
    conv_count_t *__restrict__ hist_ess, double *__restrict__ node_rhat, double *__restrict__ node_ess,
    double *__restrict__ pointwise) {
    typedef IcStage<D, DIR> St;
    constexpr int DPT = IcPlan<D>::DPT, TI = IcPlan<D>::TI, PT = St::PER_THREAD;
    __shared__ double stage[2][St::N];
    __shared__ double colred[2][4][IC_TJ];
    __shared__ unsigned int lhist[2][CONV_NBINS];
    __shared__ double ledges[2][CONV_MAX_EDGES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = blockIdx.y, g = blockIdx.x;
    const int S = M * h, ab = (h / b) * b;                    // ab: the samples of a segment that are in a batch
    const double inf = __builtin_inf();
    if (tid < 2 * CONV_NBINS) (&lhist[0][0])[tid] = 0u;
    if (tid < 2 * CONV_MAX_EDGES) (&ledges[0][0])[tid] = edges[tid];
    __syncthreads();
    const int q0 = g * L, q1 = min(n_tiles, q0 + L);
    for (int q = q0; q < q1; ++q) {
        const int i0 = tiles[q].x * TI, j0 = tiles[q].y * IC_TJ;
        const int j = j0 + lane;
        uint32_t valid = 0;
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
            const int i = i0 + 4 * k + wv;
            if (i < N && j < N && (DIR ? i != j : i < j)) valid |= 1u << k;
        }
        double mean[DPT], m2[DPT], sw[DPT], mm[DPT], mm2[DPT], bs[DPT], bm[DPT], bm2[DPT];
#pragma unroll
        for (int k = 0; k < DPT; ++k)
            mean[k] = m2[k] = sw[k] = mm[k] = mm2[k] = bs[k] = bm[k] = bm2[k] = 0.0;
        dyad_stage_first<D, DIR>(stage[0], Xs, ic, radii, t, N, i0, j0, tid);
        __syncthreads();
        int pos = 0, bpos = 0, seg = 0, nb = 0;               // s % h, (s % h) % b, s / h, batches so far
        for (int s = 0; s < S; ++s) {
            const int cur = s & 1;
            const double *sb = stage[cur];
            double pre[PT];           // the next sample's block, in flight under this sample's arithmetic
            if (s + 1 < S) dyad_stage_prefetch<D, DIR>(pre, Xs, ic, radii, s + 1, T, t, N, i0, j0, tid);
            const DyadColumn<D> col = dyad_column<D, DIR>(sb, lane);
            const double inv_n = 1.0 / (double)(pos + 1);
            const bool batch_first = bpos == 0;
#pragma unroll
            for (int k = 0; k < DPT; ++k) {
                const int row = 4 * k + wv;
                const double eta = conv_eta<D, DIR>(sb + St::XI + row * D, col.xj, col.b0, col.b1, col.rj,
                                                    DIR ? sb[St::RI + row] : 1.0);
                const double delta = eta - mean[k];
                mean[k] = fma(delta, inv_n, mean[k]);
                m2[k] = fma(delta, eta - mean[k], m2[k]);
                bs[k] = batch_first ? eta : bs[k] + eta;
            }
            if (pos < ab && bpos == b - 1) {                  // a batch ends
                ++nb;
                const double inv_b = 1.0 / (double)nb, db = (double)b;
#pragma unroll
                for (int k = 0; k < DPT; ++k) {
                    const double v = bs[k] / db;
                    const double delta = v - bm[k];
                    bm[k] = fma(delta, inv_b, bm[k]);
                    bm2[k] = fma(delta, v - bm[k], bm2[k]);
                }
            }
            bpos = bpos == b - 1 ? 0 : bpos + 1;
            if (pos == h - 1) {                               // a segment ends
                ++seg;
                const double inv_m = 1.0 / (double)seg, dh1 = (double)(h - 1);
#pragma unroll
                for (int k = 0; k < DPT; ++k) {
                    sw[k] += m2[k] / dh1;
                    const double delta = mean[k] - mm[k];
                    mm[k] = fma(delta, inv_m, mm[k]);
                    mm2[k] = fma(delta, mean[k] - mm[k], mm2[k]);
                    mean[k] = 0.0; m2[k] = 0.0;
                }
                pos = 0; bpos = 0;
            } else {
                ++pos;
            }
            if (s + 1 < S) dyad_stage_commit<D, DIR>(stage[cur ^ 1], pre, tid);
            __syncthreads();
        }
        // the tile's dyads: rhat and ess; a dyad that does not exist holds the identities 0 and +inf
        const double dM = (double)M, dh = (double)h, dS = (double)S;
        const double c1 = (double)(h - 1) / dh, dM1 = (double)(M - 1), dnb1 = (double)(nb - 1), db = (double)b;
        double col_r = 0.0, col_e = inf;
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
            const bool ok = (valid >> k) & 1u;
            const double W = sw[k] / dM, B = dh * mm2[k] / dM1;
            const double varp = c1 * W + B / dh;
            const double vbm = db * bm2[k] / dnb1;
            double rhat = W == 0.0 ? (B == 0.0 ? 1.0 : inf) : sqrt(varp / W);
            double ess = vbm == 0.0 ? (varp == 0.0 ? dS : inf) : dS * varp / vbm;
            const int i = i0 + 4 * k + wv;
            if (ok) {
                atomicAdd(&lhist[0][conv_bin(ledges[0], n_rhat, rhat)], 1u);
                atomicAdd(&lhist[1][conv_bin(ledges[1], n_ess, ess)], 1u);
                if (pointwise)
                    *(double2 *)(pointwise + (((size_t)t * N + i) * N + j) * 2) = make_double2(rhat, ess);
            } else {
                rhat = 0.0; ess = inf;
            }
            col_r = fmax(col_r, rhat); col_e = fmin(col_e, ess);
            // the row's node (the identities change nothing: no atomic for them)
            const double row_r = conv_wave_max(rhat), row_e = conv_wave_min(ess);
            if (lane == 0 && i < N) {
                if (row_r != 0.0)
                    __hip_atomic_fetch_max((conv_count_t *)node_rhat + (size_t)t * N + i,
                                           (conv_count_t)__double_as_longlong(row_r), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                if (row_e != inf)
                    __hip_atomic_fetch_min((conv_count_t *)node_ess + (size_t)t * N + i,
                                           (conv_count_t)__double_as_longlong(row_e), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        // the columns' nodes: the four wavefronts through LDS
        colred[0][wv][lane] = col_r; colred[1][wv][lane] = col_e;
        __syncthreads();          // also: every thread is done with the last sample's stage buffer
        if (wv == 0) {
            const double r = fmax(fmax(colred[0][0][lane], colred[0][1][lane]),
                                  fmax(colred[0][2][lane], colred[0][3][lane]));
            const double e = fmin(fmin(colred[1][0][lane], colred[1][1][lane]),
                                  fmin(colred[1][2][lane], colred[1][3][lane]));
            if (j < N) {
                if (r != 0.0)
                    __hip_atomic_fetch_max((conv_count_t *)node_rhat + (size_t)t * N + j,
                                           (conv_count_t)__double_as_longlong(r), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                if (e != inf)
                    __hip_atomic_fetch_min((conv_count_t *)node_ess + (size_t)t * N + j,
                                           (conv_count_t)__double_as_longlong(e), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();          // colred and stage[0] are free for the next tile
    }
    // the workgroup's counts (the last barrier of the tile loop ordered the LDS atomics before these reads)
    if (tid <= n_rhat && lhist[0][tid])
        __hip_atomic_fetch_add(hist_rhat + (size_t)t * (n_rhat + 1) + tid, (conv_count_t)lhist[0][tid],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid >= 64 && tid - 64 <= n_ess && lhist[1][tid - 64])
        __hip_atomic_fetch_add(hist_ess + (size_t)t * (n_ess + 1) + (tid - 64),
                               (conv_count_t)lhist[1][tid - 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace dlsm
