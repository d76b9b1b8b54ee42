// PSIS-LOO (no reference counterpart): Pareto-smoothed importance-sampling leave-one-out of every dyad over S
// posterior samples, in one pass.  With l_s the pointwise log-likelihood of kernels_ic.hpp, M =
// psis_tail_length(S) and c = min_s l_s, the log ratios are lr_s = c - l_s; the M largest are replaced by the
// quantiles of the generalised Pareto distribution fitted to them (psis_tail.hpp), and
//
//     elpd_loo = logsumexp_s(lw_s + l_s) - logsumexp_s(lw_s),   lppd = logsumexp_s(l_s) - log S,   k.
//
// Per-dyad state.  One dyad per thread.  The M + 1 smallest l so far are kept sorted (ascending) in LDS, laid out
// [slot][thread]: the threads of a wavefront touch one slot at consecutive addresses, free of bank conflicts.  From
// sample M + 1 on every sample adds exactly one term to a streaming log-sum-exp of -l over the samples outside the
// buffer - the larger of l and the buffer's largest value - and only if l is the smaller one it is inserted (a
// divergent branch, taken with probability about (M + 1) / s).  Off the tail lw_s + l_s = c, so the numerator needs
// the non-tail samples' count only, and no raw tail sum is ever subtracted.  lppd is k_ic_accumulate's
// streaming log-sum-exp.  After the last sample a thread fits and smooths its own column.  For M < 5 (S < 25)
// there is no buffer: k = +inf and elpd_loo = log S - logsumexp_s(-l_s), as for every dyad that is not fitted.
//
// Work: the tiles, the LDS staging and eta are those of a pass over posterior samples (kernels_dyad_pass.hpp),
// with a tile height of its own: `rows` = 4, 2 or 1 rows of 64 columns, wavefront = row, so that rows * 64 buffers
// of (M + 1) * 8 bytes fit the LDS (the host picks the form; the wavefronts beyond `rows` only help staging).
//
// Sums leave the kernel as per-workgroup partials added in a fixed order (kernels_ic.hpp, whose k_ic_reduce_totals
// adds them up); the histogram of k and the nodes' largest k use integer atomics as kernels_conv.hpp does.  k can
// be negative, so the nodes' maxima are taken over an order-preserving 64-bit key (loo_key), which
// k_loo_decode_nodes undoes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_conv.hpp"
#include "kernels_dyad_pass.hpp"
#include "kernels_ic.hpp"
#include "psis_tail.hpp"

namespace dlsm {

constexpr int LOO_NTOT = 5;                 // sum elpd_loo, sum elpd_loo^2, sum lppd, dyads, unfitted dyads
static_assert(LOO_NTOT == IC_NTOT, "k_ic_reduce_totals adds the partials up");
constexpr int LOO_MAX_EDGES = CONV_MAX_EDGES;
constexpr size_t LOO_LDS_BUFFER_MAX = (size_t)144 << 10;      // of the 160 KB: the rest is staging and reductions

// unsigned keys that order as the doubles do (no NaN); 0 is below every double's key
__device__ __forceinline__ conv_count_t loo_key(double v) {
    const conv_count_t b = (conv_count_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double loo_unkey(conv_count_t key) {
    if (key == 0) return -__builtin_inf();
    return __longlong_as_double((long long)((key >> 63) ? key & 0x7FFFFFFFFFFFFFFFull : ~key));
}

struct LooColumn {                          // a thread's sorted buffer: slot i at col[i * stride]
    const double *col;
    int stride;
    __device__ __forceinline__ double operator()(int i) const { return col[(size_t)i * stride]; }
};

struct LooArgs {
    const double *Xs, *ic, *radii;          // [S][T][N][D], [S][2], [S][N] (DIR)
    const uint32_t *bits;                   // [T][N][W]
    const int2 *tiles;                      // [n_tiles] = (row block of `rows` rows, column block)
    int n_tiles, L, S, M, rows, T, N, W;
    const double *edges;                    // [LOO_MAX_EDGES], padded with +inf
    int n_edges;
    double *part_tot;                       // [T][G][LOO_NTOT]
    conv_count_t *hist;                     // [T][n_edges + 1], zero on entry
    conv_count_t *node_key;                 // [T][N] keys of the largest k, zero on entry
    double *pointwise;                      // NULL or [T][N][N][2] = (elpd_loo, k)
};

// workgroup g = blockIdx.x takes tiles g L .. g L + L - 1 of time step blockIdx.y; dynamic LDS: (M + 1) rows 64
// doubles (M >= 5), else none
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) void k_loo_accumulate(const LooArgs a) {
    typedef IcStage<D, DIR> St;
    constexpr int PT = St::PER_THREAD;
    extern __shared__ __attribute__((aligned(16))) double loo_buf[];
    __shared__ double stage[2][St::N];
    __shared__ double redt[LOO_NTOT][4];
    __shared__ double colred[4][IC_TJ];
    __shared__ unsigned int lhist[CONV_NBINS];
    __shared__ double ledges[LOO_MAX_EDGES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = blockIdx.y, g = blockIdx.x;
    const int S = a.S, M = a.M, N = a.N, rows = a.rows;
    const int K = M >= PSIS_MIN_TAIL ? M + 1 : 0;             // slots of a buffer
    const int stride = rows * IC_TJ;
    const bool active = wv < rows;                            // wavefront-uniform
    double *col = loo_buf + (active ? wv * IC_TJ + lane : 0);
    const double inf = __builtin_inf();
    if (tid < CONV_NBINS) lhist[tid] = 0u;
    if (tid < LOO_MAX_EDGES) ledges[tid] = a.edges[tid];
    __syncthreads();
    double tot[LOO_NTOT] = {0.0, 0.0, 0.0, 0.0, 0.0};         // thread 0: the workgroup's tiles so far
    const int q0 = g * a.L, q1 = min(a.n_tiles, q0 + a.L);
    for (int q = q0; q < q1; ++q) {
        const int i0 = a.tiles[q].x * rows, j0 = a.tiles[q].y * IC_TJ;
        const int i = i0 + wv, j = j0 + lane;
        const bool valid = active && i < N && j < N && (DIR ? i != j : i < j);
        const double y = valid ? (double)((a.bits[((size_t)t * N + i) * a.W + (j >> 5)] >> (j & 31)) & 1u) : 0.0;
        double lm = -inf, lr = 0.0;         // log-sum-exp of l (lppd)
        double nm = -inf, nr = 0.0;         // log-sum-exp of -l over the samples outside the buffer
        double top = -inf;                  // the buffer's largest value once it is full
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
                const double l = y * eta - (fmax(eta, 0.0) + log1p(exp(-fabs(eta))));
                psis_lse_add(lm, lr, l);
                int p = -1;                                   // the slot l is inserted below, or -1
                if (s >= K) {                                 // uniform: the buffer is full (K = 0: there is none)
                    psis_lse_add(nm, nr, -fmax(l, top));
                    if (l < top) p = K - 1;
                } else {
                    p = s;
                }
                if (p >= 0) {
                    while (p > 0) {
                        const double below = col[(size_t)(p - 1) * stride];
                        if (!(below > l)) break;
                        col[(size_t)p * stride] = below;
                        --p;
                    }
                    col[(size_t)p * stride] = l;
                    if (s >= K - 1) top = col[(size_t)(K - 1) * stride];
                }
            }
            if (s + 1 < S) dyad_stage_commit<D, DIR>(stage[cur ^ 1], pre, tid);
            __syncthreads();
        }
        // the tile's dyads: fit, smooth, and the sums; a dyad that does not exist holds k = -inf
        double sums[LOO_NTOT] = {0.0, 0.0, 0.0, 0.0, 0.0};
        double kv = -inf;
        if (active) {
            const LooColumn tail = {col, stride};
            const double dS = (double)S;
            const double lppd = lm + log(lr / dS);
            PsisFit fit;
            fit.fitted = false; fit.k = inf; fit.sigma = 0.0; fit.ecut = 0.0;
            if (K) fit = psis_fit(tail, M);
            double elpd;
            if (fit.fitted) {
                const double c = tail(0);
                psis_lse_add(nm, nr, -tail(M));               // the cutoff sample is off the tail
                double am = 0.0, ar = (double)(S - M);        // of lw_s + l_s - c: S - M samples off the tail
                double bm = c + nm, br = nr;                  // of lw_s: c - l_s off the tail
                for (int m = 1; m <= M; ++m) {
                    const double lw = psis_smoothed(fit, m, M);
                    psis_lse_add(bm, br, lw);
                    psis_lse_add(am, ar, lw + (tail(M - m) - c));
                }
                elpd = c + ((am + log(ar)) - (bm + log(br)));
            } else {
                for (int m = 0; m < K; ++m) psis_lse_add(nm, nr, -tail(m));
                elpd = log(dS) - (nm + log(nr));
            }
            if (valid) {
                kv = fit.k;
                sums[0] = elpd; sums[1] = elpd * elpd; sums[2] = lppd; sums[3] = 1.0;
                sums[4] = fit.fitted ? 0.0 : 1.0;
                atomicAdd(&lhist[conv_bin(ledges, a.n_edges, kv)], 1u);
                if (a.pointwise)
                    *(double2 *)(a.pointwise + (((size_t)t * N + i) * N + j) * 2) = make_double2(elpd, kv);
            }
        }
#pragma unroll
        for (int c = 0; c < LOO_NTOT; ++c) {
            const double v = wave_sum_all(sums[c]);
            if (lane == 0) redt[c][wv] = v;
        }
        // the row's node, then the columns' nodes through LDS (-inf changes nothing: no atomic for it)
        const double row_k = conv_wave_max(kv);
        if (lane == 0 && row_k != -inf)
            __hip_atomic_fetch_max(a.node_key + (size_t)t * N + i, loo_key(row_k), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        colred[wv][lane] = kv;
        __syncthreads();          // also: every thread is done with the last sample's stage buffer
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < LOO_NTOT; ++c) tot[c] += (redt[c][0] + redt[c][1]) + (redt[c][2] + redt[c][3]);
        }
        if (wv == 0) {
            const double ck = fmax(fmax(colred[0][lane], colred[1][lane]), fmax(colred[2][lane], colred[3][lane]));
            if (ck != -inf)
                __hip_atomic_fetch_max(a.node_key + (size_t)t * N + j, loo_key(ck), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();          // redt, colred and stage[0] are free for the next tile
    }
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < LOO_NTOT; ++c) a.part_tot[((size_t)t * gridDim.x + g) * LOO_NTOT + c] = tot[c];
    }
    // the workgroup's counts (the last barrier of the tile loop ordered the LDS atomics before these reads)
    if (tid <= a.n_edges && lhist[tid])
        __hip_atomic_fetch_add(a.hist + (size_t)t * (a.n_edges + 1) + tid, (conv_count_t)lhist[tid],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// node_k[q] = the double of key[q] (in place: both are 64 bits); a node without a dyad: -inf
__global__ __launch_bounds__(IC_NT) void k_loo_decode_nodes(conv_count_t *key, size_t n) {
    const size_t q = (size_t)blockIdx.x * IC_NT + threadIdx.x;
    if (q < n) ((double *)key)[q] = loo_unkey(key[q]);
}

}  // namespace dlsm
