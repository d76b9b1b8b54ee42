// Information criteria (no reference counterpart): the pointwise log-likelihood of every dyad over S
// posterior samples, reduced in one pass to what WAIC and DIC need.  For dyad (t, i, j) and sample s
//
//     l_s = y eta_s - log(1 + exp(eta_s)),      eta as k_gof_draw (kernels_gof.hpp)
//
// the kernel keeps four accumulators per dyad in registers - the running maximum m and the rescaled
// sum r = sum_s exp(l_s - m) of a streaming log-sum-exp, and Welford's mean and M2 - and never stores
// l_s.  At the end lppd = m + log(r / S), var = M2 / (S - 1) (0 for S = 1), elpd = lppd - var.
//
// Work: the tiles, the LDS staging of the samples and eta are the shared ones of a pass over posterior samples
// (kernels_dyad_pass.hpp); the library's exp / log1p give the outputs at a few ulp of numpy.
//
// Sums leave the kernel as per-workgroup partials, added in a fixed order (DPP butterflies, the four
// wavefronts in index order, a workgroup's tiles in index order) and summed over the workgroups in index
// order by the two small kernels below: no floating-point atomics, the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_dyad_pass.hpp"

namespace dlsm {

constexpr int IC_NTOT = 5;                  // sum lppd, sum var, sum mean, sum elpd^2, dyads

// Xs [S][T][N][D], ic [S][2], radii [S][N] (DIR); bits [T][N][W]; tiles [n_tiles] = (row block, column
// block); workgroup g = blockIdx.x takes tiles g L .. g L + L - 1 of time step blockIdx.y.
// part_tot [T][G][IC_NTOT], part_s [T][G][S] (G = gridDim.x); pointwise NULL or [T][N][N][2].
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) void k_ic_accumulate(
    const double *__restrict__ Xs, const double *__restrict__ ic, const double *__restrict__ radii,
    const uint32_t *__restrict__ bits, const int2 *__restrict__ tiles, int n_tiles, int L, int S, int T, int N,
    int W, double *__restrict__ part_tot, double *part_s, double *__restrict__ pointwise) {
    typedef IcStage<D, DIR> St;
    constexpr int DPT = IcPlan<D>::DPT, TI = IcPlan<D>::TI, PT = St::PER_THREAD;
    __shared__ double stage[2][St::N];
    __shared__ double red[2][4];
    __shared__ double redt[IC_NTOT][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = blockIdx.y, g = blockIdx.x;
    double *ps = part_s + ((size_t)t * gridDim.x + g) * S;
    double tot[IC_NTOT] = {0.0, 0.0, 0.0, 0.0, 0.0};          // thread 0: the workgroup's tiles so far
    const int q0 = g * L, q1 = min(n_tiles, q0 + L);
    for (int q = q0; q < q1; ++q) {
        const int i0 = tiles[q].x * TI, j0 = tiles[q].y * IC_TJ;
        const int j = j0 + lane;
        uint32_t valid, ybits;        // the tile's dyads of this thread: which exist, and the network's bits
        dyad_tile_bits<D, DIR>(bits, nullptr, t, N, W, i0, j, wv, valid, ybits);
        // m = -inf makes the first sample an ordinary update: r = 0 * e^-inf + 1, mean = l, M2 = 0
        double m[DPT], r[DPT], mean[DPT], m2[DPT];
#pragma unroll
        for (int k = 0; k < DPT; ++k) { m[k] = -__builtin_inf(); r[k] = 0.0; mean[k] = 0.0; m2[k] = 0.0; }
        dyad_stage_first<D, DIR>(stage[0], Xs, ic, radii, t, N, i0, j0, tid);
        __syncthreads();
        for (int s = 0; s < S; ++s) {
            const int cur = s & 1;
            const double *sb = stage[cur];
            double pre[PT];           // the next sample's block, in flight under this sample's arithmetic
            if (s + 1 < S) dyad_stage_prefetch<D, DIR>(pre, Xs, ic, radii, s + 1, T, t, N, i0, j0, tid);
            const DyadColumn<D> col = dyad_column<D, DIR>(sb, lane);
            const double inv_n = 1.0 / (double)(s + 1);
            double lsum = 0.0;
#pragma unroll
            for (int k = 0; k < DPT; ++k) {
                const double eta = dyad_eta<D, DIR>(sb, 4 * k + wv, col);
                // y eta - log(1 + e^eta) = y eta - max(eta, 0) - log1p(e^-|eta|): finite for any finite eta
                const double y = (double)((ybits >> k) & 1u);
                const double l = y * eta - (fmax(eta, 0.0) + log1p(exp(-fabs(eta))));
                const double dl = l - m[k];
                const double e = exp(-fabs(dl));
                r[k] = dl > 0.0 ? fma(r[k], e, 1.0) : r[k] + e;
                m[k] = fmax(m[k], l);
                const double delta = l - mean[k];
                mean[k] = fma(delta, inv_n, mean[k]);
                m2[k] = fma(delta, l - mean[k], m2[k]);
                lsum += ((valid >> k) & 1u) ? l : 0.0;
            }
            lsum = wave_sum_all(lsum);
            if (lane == 0) red[cur][wv] = lsum;
            if (s + 1 < S) dyad_stage_commit<D, DIR>(stage[cur ^ 1], pre, tid);
            __syncthreads();
            if (tid == 0) {
                const double v = (red[cur][0] + red[cur][1]) + (red[cur][2] + red[cur][3]);
                ps[s] = (q == q0 ? 0.0 : ps[s]) + v;
            }
        }
        // the tile's dyads: lppd, var, and the sums
        const double dS = (double)S, inv_S1 = S > 1 ? 1.0 / (double)(S - 1) : 0.0;
        double sums[IC_NTOT] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
            if ((valid >> k) & 1u) {
                const double lppd = m[k] + log(r[k] / dS);
                const double var = m2[k] * inv_S1;
                const double elpd = lppd - var;
                sums[0] += lppd; sums[1] += var; sums[2] += mean[k]; sums[3] = fma(elpd, elpd, sums[3]);
                sums[4] += 1.0;
                if (pointwise) {
                    const int i = i0 + 4 * k + wv;
                    *(double2 *)(pointwise + (((size_t)t * N + i) * N + j) * 2) = make_double2(lppd, var);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < IC_NTOT; ++c) {
            const double v = wave_sum_all(sums[c]);
            if (lane == 0) redt[c][wv] = v;
        }
        __syncthreads();          // also: every thread is done with the last sample's stage buffer
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < IC_NTOT; ++c) tot[c] += (redt[c][0] + redt[c][1]) + (redt[c][2] + redt[c][3]);
        }
        __syncthreads();          // redt and stage[0] are free for the next tile
    }
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < IC_NTOT; ++c) part_tot[((size_t)t * gridDim.x + g) * IC_NTOT + c] = tot[c];
    }
}

// totals[t][c] = sum_g part_tot[t][g][c]: thread q adds g = q, q + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(IC_NT) void k_ic_reduce_totals(const double *__restrict__ part_tot, int G,
                                                            double *__restrict__ totals) {
    __shared__ double buf[IC_NT];
    const int tid = threadIdx.x, t = blockIdx.x;
    for (int c = 0; c < IC_NTOT; ++c) {
        double v = 0.0;
        for (int g = tid; g < G; g += IC_NT) v += part_tot[((size_t)t * G + g) * IC_NTOT + c];
        buf[tid] = v;
        __syncthreads();
        for (int o = IC_NT / 2; o > 0; o >>= 1) {
            if (tid < o) buf[tid] += buf[tid + o];
            __syncthreads();
        }
        if (tid == 0) totals[t * IC_NTOT + c] = buf[0];
        __syncthreads();
    }
}

// sample_loglik[s][t] = sum_g part_s[t][g][s]: lane = sample, wavefront w adds g = w, w + 4, ... in
// order, then the four wavefronts in index order
__global__ __launch_bounds__(IC_NT) void k_ic_reduce_samples(const double *__restrict__ part_s, int G, int S,
                                                             int T, double *__restrict__ sample_loglik) {
    __shared__ double buf[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = blockIdx.y, s = blockIdx.x * 64 + lane;
    double v = 0.0;
    if (s < S)
        for (int g = wv; g < G; g += 4) v += part_s[((size_t)t * G + g) * S + s];
    buf[wv][lane] = v;
    __syncthreads();
    if (wv == 0 && s < S)
        sample_loglik[(size_t)s * T + t] = (buf[0][lane] + buf[1][lane]) + (buf[2][lane] + buf[3][lane]);
}

}  // namespace dlsm
