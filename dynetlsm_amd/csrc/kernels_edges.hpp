// Edge lists -> the packed network or the case-control tables (dlsm_upload_network_edges, capi_edges.hpp).
//
//   k_edges_scatter   an (i, j) list of one time step -> bit j of row i and bit i of row j of two [N][W] word arrays
//   k_rows_degree     popcount of every row of both arrays -> degree[t, i, 1] (out) / [t, i, 0] (in), and their maxima
//   k_rows_emit       the column indices of a row's set bits, ascending -> the zero-padded edge tables
//
// The words have the layout of k_pack_bits (kernels_loglik.hpp): bit j % 32 of word j / 32 of row i = Y[t, i, j],
// W a multiple of 4 words per row.  Nothing is sorted anywhere: ascending neighbours follow from the bit order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dlsm {

constexpr int EDGE_BAD_INDEX = 1;       // flag bits of k_edges_scatter
constexpr int EDGE_SELF_LOOP = 2;
constexpr int EDGES_THREADS = 256;
constexpr int EDGES_MAX_BLOCKS = 1024;  // the scatter's grid is capped: four workgroups per CU, then grid-stride
constexpr int ROWS_WAVES = 4;           // rows (wavefronts) per workgroup of k_rows_degree / k_rows_emit

// Grid-stride over the n pairs (src[e], dst[e]) of one time step, whole wavefronts at a time.  Every pair ORs bit
// j into row i of `rows` and bit i into row j of `cols` (the undirected model passes the same array twice; a
// duplicate sets a set bit again, so no pair is ever looked for).  A pair with an index outside 0..N-1 or with
// i == j writes nothing and raises its bit in flag[0].
// Lists usually arrive grouped by source with targets near each other, so neighbouring lanes hit the same word of
// `rows`: a run of adjacent lanes with the same word ORs its masks along the run (a segmented scan over six
// shuffle steps) and the run's last lane alone issues the atomic (measured against one atomic per pair: DESIGN.md
// 4.25).  The transposed array takes one atomic per pair: its words differ from lane to lane in such a list.
__global__ __launch_bounds__(EDGES_THREADS) void k_edges_scatter(const int32_t *__restrict__ src,
                                                                 const int32_t *__restrict__ dst, long n, int N,
                                                                 int W, uint32_t *__restrict__ rows,
                                                                 uint32_t *__restrict__ cols,
                                                                 int *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * EDGES_THREADS;
    for (long e0 = (long)blockIdx.x * EDGES_THREADS + (threadIdx.x & ~63); e0 < n; e0 += stride) {
        const long e = e0 + lane;
        int i = 0, j = 0, bad = 0;
        bool ok = e < n;
        if (ok) {
            i = src[e]; j = dst[e];
            if ((unsigned)i >= (unsigned)N || (unsigned)j >= (unsigned)N) bad = EDGE_BAD_INDEX;
            else if (i == j) bad = EDGE_SELF_LOOP;
            if (bad) { atomicOr(flag, bad); ok = false; }
        }
        // (from here on i, j < N: every word index below lies inside its [N][W] array)
        if (ok) atomicOr(cols + (long long)j * W + (i >> 5), 1u << (i & 31));
        const long long word = ok ? (long long)i * W + (j >> 5) : -1 - lane;    // (idle lanes: keys nobody shares)
        unsigned mask = ok ? 1u << (j & 31) : 0u;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned m_up = __shfl_up(mask, d);
            const long long w_up = __shfl_up(word, d);
            if (lane >= d && w_up == word) mask |= m_up;
        }
        const long long w_next = __shfl_down(word, 1);
        if (lane < 63 && w_next == word) ok = false;            // not the last lane of its run: that one writes
        if (ok) atomicOr(rows + word, mask);
    }
}

// One wavefront per row i of one time step: the set bits of its words in `rows` are its out-degree, those in
// `cols` its in-degree.  deg_t: degree + t * N * 2.  dmax[0] / dmax[1]: the largest in- / out-degree seen, one
// atomicMax per workgroup and direction.
__global__ __launch_bounds__(64 * ROWS_WAVES) void k_rows_degree(const uint32_t *__restrict__ rows,
                                                                 const uint32_t *__restrict__ cols, int N, int W,
                                                                 int32_t *__restrict__ deg_t,
                                                                 int *__restrict__ dmax) {
    __shared__ int s_max[2][ROWS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * ROWS_WAVES + wave;
    int out = 0, in = 0;
    if (i < N) {
        const uint32_t *r = rows + (size_t)i * W, *c = cols + (size_t)i * W;
        for (int w = lane; w < W; w += 64) { out += __popc(r[w]); in += __popc(c[w]); }
    }
    for (int d = 32; d > 0; d >>= 1) { out += __shfl_xor(out, d); in += __shfl_xor(in, d); }
    if (lane == 0) {
        if (i < N) { deg_t[(size_t)i * 2] = in; deg_t[(size_t)i * 2 + 1] = out; }
        s_max[0][wave] = in; s_max[1][wave] = out;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        int m = 0;
        for (int k = 0; k < ROWS_WAVES; ++k) m = max(m, s_max[threadIdx.x][k]);
        if (m > 0) atomicMax(dmax + threadIdx.x, m);
    }
}

// One wavefront per row and direction (blockIdx.y = 0: `cols` -> in_t of width Din, 1: `rows` -> out_t of width
// Dout; both tables of this time step, zeroed beforehand - the padding).  Per trip a lane takes one word; the
// wave-exclusive prefix sum of the popcounts is where the lane's columns go, behind those of the trips before.
__global__ __launch_bounds__(64 * ROWS_WAVES) void k_rows_emit(const uint32_t *__restrict__ rows,
                                                               const uint32_t *__restrict__ cols, int N, int W,
                                                               int32_t *__restrict__ in_t, int Din,
                                                               int32_t *__restrict__ out_t, int Dout) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * ROWS_WAVES + wave;
    if (i >= N) return;
    const bool outward = blockIdx.y != 0;
    const uint32_t *r = (outward ? rows : cols) + (size_t)i * W;
    const int width = outward ? Dout : Din;
    int32_t *table = (outward ? out_t : in_t) + (size_t)i * width;
    int base = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int w = w0 + lane;
        uint32_t v = w < W ? r[w] : 0u;
        const int cnt = __popc(v);
        int incl = cnt;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        int pos = base + incl - cnt;
        while (v) {
            const int b = __ffs(v) - 1;
            v &= v - 1;
            if (pos < width) table[pos] = 32 * w + b;       // (the widths are these rows' largest popcounts: always)
            ++pos;
        }
        base += __shfl(incl, 63);
    }
}

}  // namespace dlsm
