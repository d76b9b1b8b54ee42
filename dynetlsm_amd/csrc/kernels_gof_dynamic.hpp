// Goodness of fit over time (no reference counterpart; the statistics of ergm's / latentnet's gof() that
// look beyond one time step and beyond two hops): over the bit-packed networks kernels_gof.hpp draws -
// rows [net][N][W] uint32, net = sample * T + t, directed chains with their transposed rows - the
//   overlap  [sample][T][T]     dyads present at both t and u (diagonal: the edges of t)
//   steps    [sample][T-1][2N]  per step t -> t+1: persist_degree[N], nodes by their ties present at both
//                               steps (directed: out-arcs); formed_sp[N], dyads absent at t and present at
//                               t+1 by their shared partners at t (the partner definition of k_gof_stats)
//   geodesic [net][N]           pairs by shortest-path length (bin 0: no path); undirected pairs i < j,
//                               directed ordered pairs along the arcs
// all int64 and zeroed by the caller.  Every sum is an integer sum: records are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gof.hpp"

namespace dlsm {

constexpr int GOF_GEO_MAX_WORDS = 16;     // row words per lane of the BFS: W <= 64 * 16 (N <= 32768)

__device__ __forceinline__ int gof_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Workgroup (blockIdx.x, t = blockIdx.y, sample blockIdx.z) sums popcount(A_t & A_u) over its share of
// the N * W / 4 quad-words for every u >= t: per wavefront by shuffles, per workgroup through LDS, then
// one 64-bit atomic per (workgroup, u) into overlap[t][u]; the host mirrors the upper triangle.
// Undirected rows keep j > i.
__global__ __launch_bounds__(256) void k_gof_overlap(const uint32_t *__restrict__ rows, int T, int N, int W,
                                                     int directed, int64_t *__restrict__ overlap) {
    __shared__ int32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int t = blockIdx.y, s = blockIdx.z;
    const int64_t nq = (int64_t)N * W / 4, stride = (int64_t)gridDim.x * 256;
    const uint4 *At = reinterpret_cast<const uint4 *>(rows + ((size_t)s * T + t) * N * W);
    int64_t *rec = overlap + (size_t)s * T * T;
    for (int u = t; u < T; ++u) {
        const uint4 *Au = reinterpret_cast<const uint4 *>(rows + ((size_t)s * T + u) * N * W);
        int64_t acc = 0;
        for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < nq; q += stride) {
            const uint4 a = At[q], b = Au[q];
            uint4 m = make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w);
            if (!directed) {
                const int i = (int)(4 * q / W), w = (int)(4 * q % W);
                m.x &= gof_upper_mask(i, w);
                m.y &= gof_upper_mask(i, w + 1);
                m.z &= gof_upper_mask(i, w + 2);
                m.w &= gof_upper_mask(i, w + 3);
            }
            acc += __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
        }
        // the launch gives a thread at most four trips of 128 bits (capi_gof_dynamic.hpp): int sums hold
        const int ws = gof_wave_sum((int)acc);
        __syncthreads();                        // the previous u's sums have been read
        if (lane == 0) wsum[wid] = ws;
        __syncthreads();
        if (tid == 0) {
            const unsigned long long tot = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
            if (tot) atomicAdd((unsigned long long *)&rec[(size_t)t * T + u], tot);
        }
    }
}

// The step t -> t+1 of one sample: A = the network at t, B at t+1; blockIdx.y = sample * (T-1) + t.  One
// workgroup walks rows blockIdx.x, + gridDim.x, ... as k_gof_stats does: the row's candidates B_i & ~A_i
// (undirected: j > i) are compacted into LDS one chunk of words at a time, then `L` lanes (a power of
// two) per candidate sum popcount(A_i & A_j) (directed: row_i(A) & trow_j(A)) over the row words.
// persist_degree takes popcount(A_i & B_i) of the whole row.  steps [sample][T-1][2N] zeroed by the caller.
__global__ __launch_bounds__(256) void k_gof_step(const uint32_t *__restrict__ rows,
                                                  const uint32_t *__restrict__ trows, int T, int N, int W, int L,
                                                  int64_t *__restrict__ steps) {
    __shared__ uint32_t h_pd[GOF_HB], h_sp[GOF_HB];
    __shared__ int32_t nbr[GOF_CHUNK * 32];
    __shared__ int32_t wsum[4];
    __shared__ int32_t row_pd;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int s = blockIdx.y / (T - 1), t = blockIdx.y % (T - 1);
    const int directed = trows != nullptr;
    const int HB = min(N, GOF_HB);
    const size_t net = (size_t)s * T + t;
    const uint32_t *A0 = rows + net * N * W;
    const uint32_t *A1 = directed ? trows + net * N * W : A0;
    const uint32_t *B0 = A0 + (size_t)N * W;
    int64_t *rec = steps + (size_t)blockIdx.y * 2 * N;
    for (int b = tid; b < HB; b += 256) { h_pd[b] = 0; h_sp[b] = 0; }
    const int Wq = W / 4, G = 256 / L, g = tid / L, gl = tid % L;
    for (int i = blockIdx.x; i < N; i += gridDim.x) {
        const uint32_t *ai = A0 + (size_t)i * W;
        const uint32_t *bi = B0 + (size_t)i * W;
        int pd = 0;
        if (tid == 0) row_pd = 0;
        for (int w0 = 0; w0 < W; w0 += GOF_CHUNK) {
            const int w = w0 + tid;
            uint32_t cand = 0;
            if (w < W) {
                const uint32_t va = ai[w], vb = bi[w];
                pd += __popc(va & vb);
                cand = vb & ~va;
                if (!directed) cand &= gof_upper_mask(i, w);
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
            // shared partners at t of the listed dyads; every lane runs the same trips (shuffles)
            const uint4 *a4 = reinterpret_cast<const uint4 *>(ai);
            for (int e0 = 0; e0 < M; e0 += G) {
                const int e = e0 + g;
                int k = 0;
                if (e < M) {
                    const uint4 *b4 = reinterpret_cast<const uint4 *>(A1 + (size_t)nbr[e] * W);
                    for (int q = gl; q < Wq; q += L) {
                        const uint4 x = a4[q], y = b4[q];
                        k += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
                    }
                }
                for (int o = L >> 1; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
                if (e < M && gl == 0) {
                    if (k < HB) atomicAdd(&h_sp[k], 1u);
                    else atomicAdd((unsigned long long *)&rec[(size_t)N + k], 1ull);
                }
            }
        }
        atomicAdd(&row_pd, pd);
        __syncthreads();
        if (tid == 0) {
            if (row_pd < HB) atomicAdd(&h_pd[row_pd], 1u);
            else atomicAdd((unsigned long long *)&rec[row_pd], 1ull);
        }
        __syncthreads();
    }
    for (int b = tid; b < HB; b += 256) {
        if (h_pd[b]) atomicAdd((unsigned long long *)&rec[b], (unsigned long long)h_pd[b]);
        if (h_sp[b]) atomicAdd((unsigned long long *)&rec[(size_t)N + b], (unsigned long long)h_sp[b]);
    }
}

// Level-synchronous, bit-parallel breadth-first search, one source per wavefront: the sources of network
// blockIdx.y are 4 blockIdx.x + wavefront, + 4 gridDim.x, ...  `visited` and `frontier` are bit sets of W
// words held in registers, NW words per lane (word 64 k + lane in slot k: at N <= 2048 one word per lane).
// A level ORs the rows of the frontier's nodes - found by a ballot over the lanes' frontier words, then
// bit by bit, both uniform over the wavefront - into `next`, drops the visited bits, and adds the
// popcount to bin `level`; undirected sources count the targets j > i only.  The search ends with the
// first empty frontier, after N - 1 levels at the latest; the wavefronts of a workgroup share no barrier
// inside it.  Bin 0 takes the source's targets that were never reached.  Bins below GOF_HB accumulate in
// LDS, one global add per non-empty bin and workgroup; the bins above go straight to the record.
template <int NW>
__global__ __launch_bounds__(256) void k_gof_geodesic(const uint32_t *__restrict__ rows, int N, int W,
                                                      int directed, int64_t *__restrict__ geodesic) {
    __shared__ uint32_t h[GOF_HB];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int HB = min(N, GOF_HB);
    const uint32_t *R = rows + (size_t)blockIdx.y * N * W;
    int64_t *rec = geodesic + (size_t)blockIdx.y * N;
    for (int b = tid; b < HB; b += 256) h[b] = 0;
    __syncthreads();
    for (int src = 4 * blockIdx.x + wid; src < N; src += 4 * gridDim.x) {
        uint32_t visited[NW], frontier[NW], count[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int w = 64 * k + lane;
            frontier[k] = (src >> 5) == w ? 1u << (src & 31) : 0u;
            visited[k] = frontier[k];
            count[k] = directed ? 0xFFFFFFFFu : gof_upper_mask(src, w);
        }
        int reached = 0;
        for (int level = 1; level < N; ++level) {
            uint32_t next[NW];
#pragma unroll
            for (int k = 0; k < NW; ++k) next[k] = 0;
#pragma unroll
            for (int kf = 0; kf < NW; ++kf) {
                unsigned long long live = __ballot(frontier[kf] != 0);
                while (live) {
                    const int l = __ffsll(live) - 1;
                    live &= live - 1;
                    // the word and its bits are uniform over the wavefront: a scalar loop, two rows a trip
                    uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)frontier[kf], l);
                    const int v0 = 32 * (64 * kf + l);
                    while (f) {
                        const int b1 = __ffs(f) - 1;
                        f &= f - 1;
                        const int b2 = f ? __ffs(f) - 1 : b1;
                        f &= f - 1;
                        const uint32_t *r1 = R + (size_t)(v0 + b1) * W, *r2 = R + (size_t)(v0 + b2) * W;
#pragma unroll
                        for (int k = 0; k < NW; ++k)
                            if (64 * k + lane < W) next[k] |= r1[64 * k + lane] | r2[64 * k + lane];
                    }
                }
            }
            int c = 0, any = 0;
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                next[k] &= ~visited[k];
                visited[k] |= next[k];
                frontier[k] = next[k];
                any |= next[k] != 0;
                c += __popc(next[k] & count[k]);
            }
            if (!__any(any)) break;
            c = gof_wave_sum(c);
            reached += c;
            if (lane == 0 && c) {
                if (level < HB) atomicAdd(&h[level], (uint32_t)c);
                else atomicAdd((unsigned long long *)&rec[level], (unsigned long long)c);
            }
        }
        const int targets = directed ? N - 1 : N - 1 - src;
        if (lane == 0 && targets > reached) atomicAdd(&h[0], (uint32_t)(targets - reached));
    }
    __syncthreads();
    for (int b = tid; b < HB; b += 256)
        if (h[b]) atomicAdd((unsigned long long *)&rec[b], (unsigned long long)h[b]);
}

}  // namespace dlsm
