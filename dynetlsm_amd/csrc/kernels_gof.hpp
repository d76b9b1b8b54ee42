// Posterior predictive goodness of fit (no reference counterpart; the check of latentnet's / ergm's
// gof()): networks drawn from the model at posterior samples, and the structural statistics of a
// bit-packed network - edges, mutual pairs, degree and edgewise-shared-partner histograms.
//
// Draw: one bit per (sample, t, i, j) in the chain's row layout ([N][W] uint32 words per network, bit
// j % 32 of word j / 32 of row i = Y[i, j]); directed networks also get the transposed rows (bit i of
// row j = Y[i, j]), drawn from the same counters rather than transposed.  The uniform of dyad (i, j)
// is Philox4x32-10 at counter (min(i, j), max(i, j), sample index, t << 8 | STREAM_GOF): an undirected
// dyad takes the first u53 of its unordered pair (both rows see the same bit); the arc i -> j takes the
// first when i < j and the second otherwise.  Nothing depends on the grid or the batching.
//
// Statistics: one record of R = 2 + 3N int64 per network - edges, mutual, deg_out[N], deg_in[N],
// esp[N] (layout in include/dynetlsm_hip.h).  Histogram bins below GOF_HB accumulate in LDS integer
// atomics and go to the record with one global add per non-empty bin; integer sums do not depend on
// the order of arrival, so records are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"

namespace dlsm {

constexpr uint32_t STREAM_GOF = 7;
constexpr int GOF_HB = 2048;          // histogram bins held in LDS (higher bins: global atomics)
constexpr int GOF_CHUNK = 256;        // row words scanned per step of the statistics kernel (one per thread)

// the uniform of arc i -> j (undirected: of the pair)
__device__ __forceinline__ double gof_uniform(uint64_t seed, uint32_t sample, int t, int i, int j,
                                           int directed) {
    const uint32_t lo = (uint32_t)min(i, j), hi = (uint32_t)max(i, j);
    const U4 q = philox4x32_10(seed, lo, hi, sample, ((uint32_t)t << 8) | STREAM_GOF);
    return (directed && i > j) ? u53(q.z, q.w) : u53(q.x, q.y);
}

// Xs [nb][T][N][D], ic [nb][2], radii [nb][N] (directed) or NULL; bits [z][nb * T][N][W]: z = 0 the
// rows, z = 1 (directed) the transposed rows.  One thread per word; padding words are written as 0.
template <int D>
__global__ __launch_bounds__(256) void k_gof_draw(const double *__restrict__ Xs, const double *__restrict__ ic,
                                                  const double *__restrict__ radii, int T, int N, int W,
                                                  int directed, uint64_t seed, uint32_t first,
                                                  uint32_t *__restrict__ bits) {
    const int net = blockIdx.y, z = blockIdx.z;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)N * W) return;
    const int r = (int)(idx / W), w = (int)(idx % W);
    const int s = net / T, t = net % T;
    const double *X = Xs + (size_t)net * N * D;
    const double *rad = directed ? radii + (size_t)s * N : nullptr;
    const double b0 = ic[2 * s], b1 = ic[2 * s + 1];
    double xr[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xr[d] = X[(size_t)r * D + d];
    uint32_t word = 0;
    const int c0 = 32 * w, c1 = min(N, c0 + 32);
    for (int c = c0; c < c1; ++c) {
        if (c == r) continue;
        // row r of the rows holds arc r -> c; row r of the transposed rows holds arc c -> r
        const int i = z ? c : r, j = z ? r : c;
        double s2 = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double df = xr[d] - X[(size_t)c * D + d];
            s2 += df * df;
        }
        const double dist = sqrt(s2);
        const double eta = directed ? b0 * (1.0 - dist / rad[j]) + b1 * (1.0 - dist / rad[i]) : b0 - dist;
        const double p = 1.0 / (1.0 + exp(-eta));
        const double u = gof_uniform(seed, first + (uint32_t)s, t, i, j, directed);
        word |= (uint32_t)(u < p) << (c - c0);
    }
    bits[((size_t)z * gridDim.y + net) * N * W + idx] = word;
}

// bits j > i of word w of row i
__device__ __forceinline__ uint32_t gof_upper_mask(int i, int w) {
    const int b = i - 32 * w;
    if (b < 0) return 0xFFFFFFFFu;
    if (b >= 31) return 0u;
    return 0xFFFFFFFFu << (b + 1);
}

// One workgroup walks rows blockIdx.x, + gridDim.x, ... of network blockIdx.y.  rows / trows [net][N][W]
// (trows: the transposed rows, directed only, else NULL); stats [net][R] zeroed by the caller.
// Shared partners: undirected, pairs i < j with an edge, popcount(row_i & row_j); directed, arcs
// i -> j, popcount(row_i & trow_j).  The neighbours of a row are compacted into LDS one chunk of
// words at a time, then `L` lanes (a power of two) per neighbour sum the popcounts over the words.
__global__ __launch_bounds__(256) void k_gof_stats(const uint32_t *__restrict__ rows,
                                                   const uint32_t *__restrict__ trows, int N, int W, int L,
                                                   int64_t *__restrict__ stats) {
    __shared__ uint32_t h_out[GOF_HB], h_in[GOF_HB], h_esp[GOF_HB];
    __shared__ int32_t nbr[GOF_CHUNK * 32];
    __shared__ int32_t wsum[4];
    __shared__ int32_t row_deg, row_din, row_cnt;
    __shared__ unsigned long long s_edges, s_mutual;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int net = blockIdx.y;
    const int directed = trows != nullptr;
    const int HB = min(N, GOF_HB);
    const uint32_t *R0 = rows + (size_t)net * N * W;
    const uint32_t *R1 = directed ? trows + (size_t)net * N * W : R0;
    int64_t *rec = stats + (size_t)net * (2 + 3 * (size_t)N);
    for (int b = tid; b < HB; b += 256) { h_out[b] = 0; h_in[b] = 0; h_esp[b] = 0; }
    if (tid == 0) { s_edges = 0; s_mutual = 0; }
    const int Wq = W / 4, G = 256 / L, g = tid / L, gl = tid % L;
    for (int i = blockIdx.x; i < N; i += gridDim.x) {
        const uint32_t *ri = R0 + (size_t)i * W;
        const uint32_t *ti = R1 + (size_t)i * W;
        int deg = 0, din = 0, mut = 0;
        if (tid == 0) { row_deg = 0; row_din = 0; row_cnt = 0; }
        for (int w0 = 0; w0 < W; w0 += GOF_CHUNK) {
            const int w = w0 + tid;
            uint32_t cand = 0;
            if (w < W) {
                const uint32_t v = ri[w];
                deg += __popc(v);
                if (directed) {
                    const uint32_t vt = ti[w];
                    din += __popc(vt);
                    mut += __popc(v & vt & gof_upper_mask(i, w));
                    cand = v;
                } else {
                    cand = v & gof_upper_mask(i, w);
                }
            }
            // exclusive scan of the candidate counts over the workgroup
            const int c = __popc(cand);
            int incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            __syncthreads();                    // the previous chunk's list has been consumed
            if (lane == 63) wsum[wid] = incl;
            __syncthreads();
            int base = 0, M = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                base += q < wid ? wsum[q] : 0;
                M += wsum[q];
            }
            int pos = base + incl - c;
            while (cand) {
                const int b = __ffs(cand) - 1;
                cand &= cand - 1;
                nbr[pos++] = 32 * w + b;
            }
            __syncthreads();
            // shared partners of the listed neighbours; every lane runs the same trips (shuffles)
            const uint4 *a4 = reinterpret_cast<const uint4 *>(ri);
            for (int e0 = 0; e0 < M; e0 += G) {
                const int e = e0 + g;
                int k = 0;
                if (e < M) {
                    const uint4 *b4 = reinterpret_cast<const uint4 *>(R1 + (size_t)nbr[e] * W);
                    for (int q = gl; q < Wq; q += L) {
                        const uint4 x = a4[q], y = b4[q];
                        k += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
                    }
                }
                for (int o = L >> 1; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
                if (e < M && gl == 0) {
                    if (k < HB) atomicAdd(&h_esp[k], 1u);
                    else atomicAdd((unsigned long long *)&rec[2 + 2 * (size_t)N + k], 1ull);
                }
            }
            if (tid == 0) row_cnt += M;
        }
        // the row's degrees and mutual pairs
        atomicAdd(&row_deg, deg);
        if (directed) { atomicAdd(&row_din, din); atomicAdd((unsigned long long *)&s_mutual, (unsigned long long)mut); }
        __syncthreads();
        if (tid == 0) {
            if (row_deg < HB) atomicAdd(&h_out[row_deg], 1u);
            else atomicAdd((unsigned long long *)&rec[2 + row_deg], 1ull);
            if (directed) {
                if (row_din < HB) atomicAdd(&h_in[row_din], 1u);
                else atomicAdd((unsigned long long *)&rec[2 + (size_t)N + row_din], 1ull);
            }
            s_edges += (unsigned long long)row_cnt;       // undirected: pairs i < j; directed: arcs
        }
        __syncthreads();
    }
    for (int b = tid; b < HB; b += 256) {
        if (h_out[b]) atomicAdd((unsigned long long *)&rec[2 + b], (unsigned long long)h_out[b]);
        if (h_in[b]) atomicAdd((unsigned long long *)&rec[2 + (size_t)N + b], (unsigned long long)h_in[b]);
        if (h_esp[b]) atomicAdd((unsigned long long *)&rec[2 + 2 * (size_t)N + b], (unsigned long long)h_esp[b]);
    }
    if (tid == 0) {
        if (s_edges) atomicAdd((unsigned long long *)&rec[0], s_edges);
        if (s_mutual) atomicAdd((unsigned long long *)&rec[1], s_mutual);
    }
}

// trows[net][j] word w, bit b = bit j of row 32 w + b of rows[net] (the observed network's columns)
__global__ __launch_bounds__(256) void k_gof_transpose(const uint32_t *__restrict__ rows, int N, int W,
                                                      uint32_t *__restrict__ trows) {
    const int net = blockIdx.y;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)N * W) return;
    const int j = (int)(idx / W), w = (int)(idx % W);
    const uint32_t *R = rows + (size_t)net * N * W;
    uint32_t word = 0;
    const int i0 = 32 * w, i1 = min(N, i0 + 32);
    for (int i = i0; i < i1; ++i) word |= ((R[(size_t)i * W + (j >> 5)] >> (j & 31)) & 1u) << (i - i0);
    trows[(size_t)net * N * W + idx] = word;
}

}  // namespace dlsm
