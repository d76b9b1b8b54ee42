// Multi-step posterior predictive forecasts (the reference has only the one-step undirected form,
// hdp_lpcm.py:555-626): one trajectory of H future time steps per posterior sample, drawn from the model's
// own dynamics, and the mean edge probability of every future step over the trajectories.
//
// Draw (k_forecast_paths_draw): one thread per (sample, node) walks h = 1..H.
//   random walk   x_h = x_{h-1} + sqrt(sigma_sq) eps
//   mixture       z_h ~ Categorical(w[z_{h-1}, :]),  x_h = lmbda mu[z_h] + (1 - lmbda) x_{h-1} + sqrt(sigma[z_h]) eps
// (sigma is a variance, as in the likelihood and mixture_density.)  The randoms of (node i, step h, sample
// index q) are Philox4x32-10 keyed by the seed at counter
//     (i, h | draw << 16, q, STREAM_FORECAST)
// draw 0: its first u53 is the label uniform; draw 1 + d / 2: the two uniforms of box_muller for coordinates
// d, d + 1.  q = first_index + s, so nothing depends on the grid, the batching or how the samples are split
// across calls.  The label is the smallest k with u * c_{K-1} <= c_k, c the running sum of the raw transition
// row in index order (plain double adds), capped at K - 1.
// The draws are written horizon-major, [H][S][N][D]: step h of all samples is one contiguous [S][N][D] block,
// the layout k_forecast_mean reads, so the mean pass of step h streams it without a stride.
//
// Mean (k_forecast_paths_mean): the 64 x 64 tile, 4 x 4 per thread of k_forecast_mean with the horizon in
// blockIdx.z; undirected: tiles on or above the diagonal, mirrored; directed: all tiles, the sample's
// reciprocal radii staged next to the positions and two intercepts per sample.  The sums stay un-normalised
// across sample batches; the last batch divides by S.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_forecast.hpp"

namespace dlsm {

constexpr uint32_t STREAM_FORECAST = 9;

// Samples per LDS refill of the mean pass.  One sample stages 2 * 64 * D positions, (directed) 2 * 64
// reciprocal radii and two intercepts: 1024 D + 1040 bytes.  The chunk shrinks with D so that a workgroup
// stays below 40 KB (D = 8 directed: 4 * 9232 = 36 928 bytes; 16 samples would be 147 712 of the CU's
// 163 840 and leave one workgroup per CU): the LDS admits four workgroups per CU.  The registers decide below
// that: 80 to 166 per lane over the sixteen instantiations, three or more wavefronts per SIMD.
template <int D> struct FpPlan { static constexpr int CHUNK = D <= 1 ? 16 : D <= 3 ? 8 : 4; };

template <int D, bool DIR>
constexpr int fp_lds_bytes() {
    return FpPlan<D>::CHUNK * (2 * FC_TILE * D + (DIR ? 2 * FC_TILE : 0) + 2) * (int)sizeof(double);
}
static_assert(fp_lds_bytes<8, true>() <= 40 * 1024 && fp_lds_bytes<1, true>() <= 40 * 1024 &&
              fp_lds_bytes<3, true>() <= 40 * 1024, "the mean pass's LDS plan: a quarter of a CU at most");

// X0 [nb][N][D]; mixture (z0 != NULL): z0 [nb][N], trans [nb][K][K], mu [nb][K][D], sigma [nb][K], lmbda [nb];
// random walk (z0 == NULL): sigma_sq.  paths [H][nb][N][D]; labels [H][nb][N] or NULL.  Grid (ceil(N / 256), nb).
template <int D>
__global__ __launch_bounds__(256) void k_forecast_paths_draw(
    const double *__restrict__ X0, const int32_t *__restrict__ z0, const double *__restrict__ trans,
    const double *__restrict__ mu, const double *__restrict__ sigma, const double *__restrict__ lmbda, int K,
    double sigma_sq, int H, int N, uint64_t seed, uint32_t first, double *__restrict__ paths,
    int32_t *__restrict__ labels) {
    const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, nb = gridDim.y;
    if (i >= N) return;
    const bool mixture = z0 != nullptr;
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = X0[((size_t)s * N + i) * D + d];
    int z = mixture ? z0[(size_t)s * N + i] : 0;
    const double lm = mixture ? lmbda[s] : 0.0;
    const double *W = mixture ? trans + (size_t)s * K * K : nullptr;
    const double *M = mixture ? mu + (size_t)s * K * D : nullptr;
    const double *Sg = mixture ? sigma + (size_t)s * K : nullptr;
    double sd = mixture ? 0.0 : sqrt(sigma_sq);
    for (int h = 1; h <= H; ++h) {
        const uint32_t c1 = (uint32_t)h;
        if (mixture) {
            const U4 q = philox4x32_10(seed, (uint32_t)i, c1, first + (uint32_t)s, STREAM_FORECAST);
            const double u = u53(q.x, q.y);
            const double *row = W + (size_t)z * K;
            double tot = 0.0;
            for (int k = 0; k < K; ++k) tot += row[k];
            const double thr = u * tot;
            double c = 0.0;
            int zn = K - 1;
            for (int k = 0; k < K; ++k) {
                c += row[k];
                if (thr <= c) { zn = k; break; }
            }
            z = zn;
            sd = sqrt(Sg[z]);
            labels[((size_t)(h - 1) * nb + s) * N + i] = z;
        }
        double *out = paths + (((size_t)(h - 1) * nb + s) * N + i) * D;
#pragma unroll
        for (int d = 0; d < D; d += 2) {
            const U4 q = philox4x32_10(seed, (uint32_t)i, c1 | ((uint32_t)(1 + d / 2) << 16), first + (uint32_t)s,
                                       STREAM_FORECAST);
            double e0, e1;
            box_muller(u53(q.x, q.y), u53(q.z, q.w), e0, e1);
            if (mixture) {
                x[d] = lm * M[(size_t)z * D + d] + (1.0 - lm) * x[d] + sd * e0;
                if (d + 1 < D) x[d + 1] = lm * M[(size_t)z * D + d + 1] + (1.0 - lm) * x[d + 1] + sd * e1;
            } else {
                x[d] = x[d] + sd * e0;
                if (d + 1 < D) x[d + 1] = x[d + 1] + sd * e1;
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d) out[d] = x[d];
    }
}

// sum[h][i][j] (+)= sum_s expit(eta_s(h, i, j)) over the ns samples of this batch; Xh [H][ns][N][D] (the draw
// kernel's layout), ic [ns][2], radii [ns][N] (DIR).  first != 0: the sums start here; last != 0: the sums are
// divided by S_total.  The diagonal is 0.  Grid (nt, nt, H).
template <int D, bool DIR>
__global__ __launch_bounds__(256) void k_forecast_paths_mean(const double *__restrict__ Xh,
                                                             const double *__restrict__ ic,
                                                             const double *__restrict__ radii, int ns, int N,
                                                             int first, int last, int S_total,
                                                             double *__restrict__ sum) {
    constexpr int CH = FpPlan<D>::CHUNK;
    const int ti0 = blockIdx.y, tj0 = blockIdx.x;
    if (!DIR && tj0 < ti0) return;
    __shared__ double sXi[CH][FC_TILE * D];
    __shared__ double sXj[CH][FC_TILE * D];
    __shared__ double sRi[DIR ? CH : 1][FC_TILE];      // reciprocal radii
    __shared__ double sRj[DIR ? CH : 1][FC_TILE];
    __shared__ double sB[CH][2];
    const int i0 = ti0 * FC_TILE, j0 = tj0 * FC_TILE;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const double *X = Xh + (size_t)blockIdx.z * ns * N * D;
    double *out = sum + (size_t)blockIdx.z * N * N;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
    for (int s0 = 0; s0 < ns; s0 += CH) {
        const int nc = min(CH, ns - s0);
        for (int q = tid; q < nc * FC_TILE * D; q += 256) {
            const int s = q / (FC_TILE * D), r = q % (FC_TILE * D);
            const int gi = min(i0 * D + r, N * D - 1), gj = min(j0 * D + r, N * D - 1);
            sXi[s][r] = X[(size_t)(s0 + s) * N * D + gi];
            sXj[s][r] = X[(size_t)(s0 + s) * N * D + gj];
        }
        if (DIR) {
            for (int q = tid; q < nc * FC_TILE; q += 256) {
                const int s = q / FC_TILE, r = q % FC_TILE;
                sRi[s][r] = 1.0 / radii[(size_t)(s0 + s) * N + min(i0 + r, N - 1)];
                sRj[s][r] = 1.0 / radii[(size_t)(s0 + s) * N + min(j0 + r, N - 1)];
            }
        }
        if (tid < 2 * nc) sB[tid >> 1][tid & 1] = ic[2 * (size_t)s0 + tid];
        __syncthreads();
        for (int s = 0; s < nc; ++s) {
            const double b0 = sB[s][0], b1 = sB[s][1];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = dist_fast<D>(&sXi[s][(4 * ti + a) * D], &sXj[s][(4 * tj + c) * D], 0);
                    // arc i -> j: intercept_in with the receiver's radius, intercept_out with the sender's
                    const double eta = DIR ? b0 * (1.0 - d * sRj[s][4 * tj + c]) + b1 * (1.0 - d * sRi[s][4 * ti + a])
                                           : b0 - d;
                    acc[a][c] += 1.0 / (1.0 + fast_exp(-eta));
                }
        }
        __syncthreads();
    }
    // a diagonal tile of the undirected form holds both (i, j) and (j, i): every thread writes its own entry;
    // a tile above the diagonal is mirrored
    const bool mirror = !DIR && tj0 != ti0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + 4 * ti + a, j = j0 + 4 * tj + c;
            if (i < N && j < N) {
                double v = acc[a][c];
                if (!first) v += out[(size_t)i * N + j];
                if (last) v = v / (double)S_total;
                if (i == j) v = 0.0;
                out[(size_t)i * N + j] = v;
                if (mirror) out[(size_t)j * N + i] = v;
            }
        }
}

}  // namespace dlsm
