// Triad census of bit-packed networks (no reference counterpart; sna's triad.census, ergm's triadcensus
// term): the triadic family of the posterior predictive goodness-of-fit check.  The networks are those of
// kernels_gof.hpp - rows and, directed, transposed rows, drawn by k_gof_draw or uploaded.
//
// Every connected pair i < j (at least one arc between them) has the dyad code c = Y[i,j] + 2 Y[j,i] in
// {1, 2, 3}; every third node k has the states a = Y[i,k] + 2 Y[k,i] and b = Y[j,k] + 2 Y[k,j].  A
// network's record of R = GOF_TRIAD_R int64 holds, summed over the connected pairs, the number of k in
// each state: [(c - 1) * 16 + a * 4 + b], and at [48 + c - 1] the number of pairs of code c (layout in
// include/dynetlsm_hip.h).  A triad with m non-null dyads is visited m times; null pairs are never
// visited, so the work is (connected pairs) x W like the shared partners'.  The host maps (c, a, b) to
// the 16 MAN classes (dynetlsm_amd/gof.py).  Integer sums do not depend on the order of arrival, so
// records are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gof.hpp"

namespace dlsm {

constexpr int GOF_TRIAD_R = 51;       // int64 entries of one record: 3 x 16 state counts, 3 pair counts
// A thread's sixteen uint32 counters go to the workgroup's int64 block once they may hold this many bits
// (and at the end of a pass).  Exactness needs a wavefront's 64 counters of one state to sum below 2^32:
// a thread sees a step of at most W / 4 * 128 <= 2^25 bits per partner (N < 2^31) and a counter never
// exceeds max(limit, step), so 64 of them stay at or below 2^31 for any limit up to 2^25.  The limit is
// far lower so that one dense row of a few thousand nodes already takes the path: a flush is sixteen
// wavefront sums, against at least 128 partners' words between two.
constexpr uint32_t GOF_TRIAD_FLUSH_BITS = 1u << 14;

// bits k < N of word w of a row
__device__ __forceinline__ uint32_t gof_node_mask(int N, int w) {
    const int left = N - 32 * w;
    if (left >= 32) return 0xFFFFFFFFu;
    if (left <= 0) return 0u;
    return (1u << left) - 1u;
}

// bit k of word w, if k lies in it
__device__ __forceinline__ uint32_t gof_bit_in_word(int k, int w) {
    return (k >> 5) == w ? 1u << (k & 31) : 0u;
}

// One workgroup walks rows blockIdx.x, + gridDim.x, ... of network blockIdx.y, once per dyad code c (the
// outer loop: the sixteen counters of a thread then belong to one c and live across pairs, chunks and
// rows).  rows / trows [net][N][W] (undirected: DIRECTED = false and trows is not read: only c = 3 and
// the states 0 and 3 occur); records [net][GOF_TRIAD_R] zeroed by the caller.  As in k_gof_stats the
// partners j > i of code c are compacted into LDS one chunk of row words at a time and L lanes (a power
// of two) per partner walk the words, a uint4 of each of the four rows at a time.
// The masks of state 0 are complements: they would count the padding bits, and i and j themselves (j in
// i's mask and i in j's); `ok` clears those.  The other states need nothing: the diagonal and the padding
// bits of a packed network are zero.
template <bool DIRECTED>
__global__ __launch_bounds__(256) void k_gof_triads(const uint32_t *__restrict__ rows,
                                                    const uint32_t *__restrict__ trows, int N, int W, int L,
                                                    int64_t *__restrict__ records) {
    __shared__ int32_t nbr[GOF_CHUNK * 32];
    __shared__ int32_t wsum[4];
    __shared__ unsigned long long s_rec[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int net = blockIdx.y;
    const uint32_t *R0 = rows + (size_t)net * N * W;
    const uint32_t *R1 = DIRECTED ? trows + (size_t)net * N * W : R0;
    int64_t *rec = records + (size_t)net * GOF_TRIAD_R;
    const int Wq = W / 4, G = 256 / L, g = tid / L, gl = tid % L;
    const uint32_t step = (uint32_t)((Wq + L - 1) / L) * 128u;      // bits a thread looks at per partner
    if (tid < 16) s_rec[tid] = 0;
    __syncthreads();

    uint32_t cnt[16];
    uint32_t pending = 0;               // upper bound of every cnt[]; the same in all threads
#pragma unroll
    for (int s = 0; s < 16; ++s) cnt[s] = 0;
    // the wavefront's sums of the counters -> s_rec; every lane runs it (shuffles)
    auto flush = [&]() {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if (!DIRECTED && (s & 3) != 0 && (s & 3) != 3) continue;
            if (!DIRECTED && (s >> 2) != 0 && (s >> 2) != 3) continue;
            uint32_t v = cnt[s];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0 && v) atomicAdd(&s_rec[s], (unsigned long long)v);
            cnt[s] = 0;
        }
        pending = 0;
    };

#pragma unroll 1
    for (int c = DIRECTED ? 1 : 3; c <= 3; ++c) {
        unsigned long long pairs = 0;                   // thread 0's
#pragma unroll 1
        for (int i = blockIdx.x; i < N; i += gridDim.x) {
            const uint32_t *ri = R0 + (size_t)i * W;
            const uint32_t *ti = R1 + (size_t)i * W;
            const uint4 *oi4 = reinterpret_cast<const uint4 *>(ri);
            const uint4 *ii4 = reinterpret_cast<const uint4 *>(ti);
#pragma unroll 1
            for (int w0 = 0; w0 < W; w0 += GOF_CHUNK) {
                const int w = w0 + tid;
                uint32_t cand = 0;
                if (w < W) {
                    const uint32_t o = ri[w], in = DIRECTED ? ti[w] : o;
                    cand = (c == 1 ? o & ~in : c == 2 ? in & ~o : o & in) & gof_upper_mask(i, w);
                }
                // exclusive scan of the candidate counts over the workgroup
                const int nc = __popc(cand);
                int incl = nc;
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
                int pos = base + incl - nc;
                while (cand) {
                    const int b = __ffs(cand) - 1;
                    cand &= cand - 1;
                    nbr[pos++] = 32 * w + b;
                }
                __syncthreads();
                pairs += (unsigned long long)M;
#pragma unroll 1
                for (int e0 = 0; e0 < M; e0 += G) {
                    if (pending + step > GOF_TRIAD_FLUSH_BITS) flush();
                    pending += step;
                    const int e = e0 + g;
                    if (e < M) {                        // (the trips are counted by e0: `flush` sees every lane)
                        const int j = nbr[e];
                        const uint4 *oj4 = reinterpret_cast<const uint4 *>(R0 + (size_t)j * W);
                        const uint4 *ij4 = reinterpret_cast<const uint4 *>(R1 + (size_t)j * W);
#pragma unroll 1
                        for (int q = gl; q < Wq; q += L) {
                            const uint4 oi = oi4[q], oj = oj4[q];
                            const uint4 ii = DIRECTED ? ii4[q] : oi, ij = DIRECTED ? ij4[q] : oj;
                            const uint32_t xoi[4] = {oi.x, oi.y, oi.z, oi.w}, xii[4] = {ii.x, ii.y, ii.z, ii.w};
                            const uint32_t xoj[4] = {oj.x, oj.y, oj.z, oj.w}, xij[4] = {ij.x, ij.y, ij.z, ij.w};
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int wd = 4 * q + u;
                                const uint32_t ok = gof_node_mask(N, wd) &
                                                    ~(gof_bit_in_word(i, wd) | gof_bit_in_word(j, wd));
                                uint32_t mi[4], mj[4];
                                mi[0] = ~(xoi[u] | xii[u]) & ok; mi[1] = xoi[u] & ~xii[u];
                                mi[2] = xii[u] & ~xoi[u];        mi[3] = xoi[u] & xii[u];
                                mj[0] = ~(xoj[u] | xij[u]) & ok; mj[1] = xoj[u] & ~xij[u];
                                mj[2] = xij[u] & ~xoj[u];        mj[3] = xoj[u] & xij[u];
#pragma unroll
                                for (int a = 0; a < 4; ++a) {
                                    if (!DIRECTED && a != 0 && a != 3) continue;
#pragma unroll
                                    for (int b = 0; b < 4; ++b) {
                                        if (!DIRECTED && b != 0 && b != 3) continue;
                                        cnt[4 * a + b] += __popc(mi[a] & mj[b]);
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        // the pass's counters -> the record
        flush();
        __syncthreads();
        if (tid < 16 && s_rec[tid]) {
            atomicAdd((unsigned long long *)&rec[(c - 1) * 16 + tid], s_rec[tid]);
            s_rec[tid] = 0;
        }
        if (tid == 0 && pairs) atomicAdd((unsigned long long *)&rec[48 + c - 1], pairs);
        __syncthreads();
    }
}

}  // namespace dlsm
