// Data augmentation for missing dyads (the reference's step at lsm.py:525-545 / hdp_lpcm.py:1025-1049, whose
// write-back is lost in a fancy-index copy): every missing dyad is drawn from its conditional given the chain's
// current positions, intercept(s) and radii, and the draw is written into EVERY copy of the packed network, so
// that the next sweep and likelihood pass condition on it.
//
// Counter layout (a test can regenerate every draw; tests/missing_ref.py does):
//   Philox4x32-10 keyed by the chain's seed at counter
//     c0 = min(i, j) | (t & 0xFF) << 24
//     c1 = max(i, j) | (t >> 8)   << 24          (N < 2^24, T <= 65535)
//     c2 = iteration
//     c3 = chain << 8 | STREAM_MISSING (= 8)
//   an undirected dyad takes the first u53 of its pair's counter (words x, y); the arc i -> j takes the first
//   when i < j and the second (words z, w) otherwise - the convention of gof_uniform.  bit = u < p,
//   p = 1 / (1 + exp(-eta)), eta the predictor of kernels_gof.hpp: b - d undirected, b_in (1 - d / r_j) +
//   b_out (1 - d / r_i) directed.  A draw is a function of (seed, chain, iteration, t, pair) alone.
//
// Ownership: the list is stored as per-(matrix, t, row) segments in BOTH orientations, columns ascending, and
// one wavefront owns one segment - the words of that row of `ybits` (undirected: and the same words of the
// column-block-major copy `ycm`; directed: segments of matrix 1 are rows of `ytbits`).  The wavefront of row j
// recomputes the draw that the wavefront of row i computes (the same instructions on the same operands: |x_i -
// x_j| does not depend on the order of its arguments), so symmetry / the transpose hold without a hand-off.  64
// entries at a time: the lanes OR their bit into the set / touched masks of their word in LDS (integer ORs: any
// order gives the same word), the first lane of each word's run does a plain read-modify-write of the word.  No
// global atomics; only listed bits change, so the diagonal and the padding stay zero.
// Accumulators (one double sum of p, one uint32 count of ones per listed dyad) are written by the wavefront
// that owns the listed orientation: row i of the undirected pair i < j, matrix 0 of the arc i -> j.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain.hpp"
#include "device_common.hpp"

namespace dlsm {

constexpr uint32_t STREAM_MISSING = 8;
constexpr int MISS_N_MAX = 1 << 24;             // node indices share a counter word with a byte of t

// one (matrix, t, row) segment: entries [begin, end) of the column / slot lists
struct MissJob { int32_t tz, row, begin, end; };            // tz = 2 t + matrix

struct MissArgs {
    const MissJob *jobs;
    const int32_t *cols;        // per entry: the column
    const int32_t *slot;        // per entry: the dyad's index in the caller's list (owning orientation), else -1
    uint32_t *ybits, *ytbits;   // the chain's packed network (ytbits: directed)
    uint32_t *ycm32;            // the column-block-major copy as 32-bit halves (undirected), else NULL
    double *psum; uint32_t *ones; unsigned long long *nacc;
    int accumulate;             // 0 never, 1 always, 2 when iteration > acc_after
    uint32_t acc_after;
};

__device__ __forceinline__ double missing_uniform(uint64_t seed, uint32_t chain, uint32_t iter, int t, int i,
                                                  int j, int directed) {
    const uint32_t lo = (uint32_t)min(i, j), hi = (uint32_t)max(i, j);
    const U4 q = philox4x32_10(seed, lo | (((uint32_t)t & 0xFFu) << 24), hi | (((uint32_t)t >> 8) << 24), iter,
                               stream_word(chain, STREAM_MISSING));
    return (directed && i > j) ? u53(q.z, q.w) : u53(q.x, q.y);
}

// One wavefront per segment (grid = segments, 64 threads).
template <int D>
__global__ __launch_bounds__(64) void k_impute_missing(ChainView v, MissArgs a, IterRef iter) {
    __shared__ uint32_t s_set[64], s_all[64];
    const int lane = threadIdx.x;
    const MissJob job = a.jobs[blockIdx.x];
    const uint32_t it = iter.get();
    const int t = job.tz >> 1, z = job.tz & 1, r = job.row;
    const int N = v.N, W = v.W;
    const int directed = v.model != DLSM_UNDIRECTED;
    const bool acc = a.accumulate == 1 || (a.accumulate == 2 && it > a.acc_after);
    if (acc && blockIdx.x == 0 && lane == 0) *a.nacc += 1ull;
    const double *X = v.X + (size_t)t * N * D;
    double xr[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xr[d] = X[(size_t)r * D + d];
    const double b0 = v.intercept[0], b1 = directed ? v.intercept[1] : 0.0;
    const double rad_r = directed ? v.radii[r] : 1.0;
    uint32_t *row = (z ? a.ytbits : a.ybits) + ((size_t)t * N + r) * W;
    uint32_t *cm = a.ycm32 ? a.ycm32 + ((size_t)t * (W / 2) * v.Ncm + r) * 2 : nullptr;
    for (int e0 = job.begin; e0 < job.end; e0 += 64) {
        const int e = e0 + lane;
        const bool on = e < job.end;
        int c = 0, y = 0;
        double p = 0.0;
        if (on) {
            c = a.cols[e];
            double s2 = 0.0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const double df = xr[d] - X[(size_t)c * D + d];
                s2 += df * df;
            }
            const double dist = sqrt(s2);
            // matrix 0: row r holds the arc r -> c; matrix 1 (the transposed rows): the arc c -> r
            const int i = z ? c : r, j = z ? r : c;
            double eta = b0 - dist;
            if (directed) {
                const double rad_c = v.radii[c];
                const double rad_i = z ? rad_c : rad_r, rad_j = z ? rad_r : rad_c;
                eta = b0 * (1.0 - dist / rad_j) + b1 * (1.0 - dist / rad_i);
            }
            p = 1.0 / (1.0 + exp(-eta));
            y = missing_uniform(v.seed, v.chain, it, t, i, j, directed) < p;
        }
        // the runs of entries that share a word (columns ascend): ordinal of the run = its LDS slot
        const int w = on ? c >> 5 : -1;
        const int wprev = __shfl_up(w, 1, 64);
        const bool head = on && (lane == 0 || wprev != w);
        const unsigned long long heads = __ballot(head);
        const int ord = __popcll(heads & ((2ull << lane) - 1ull)) - 1;
        s_set[lane] = 0u;
        s_all[lane] = 0u;
        __syncthreads();
        if (on) {
            atomicOr(&s_all[ord], 1u << (c & 31));
            if (y) atomicOr(&s_set[ord], 1u << (c & 31));
        }
        __syncthreads();
        if (head) {
            const uint32_t nw = (row[w] & ~s_all[ord]) | s_set[ord];
            row[w] = nw;
            if (cm) cm[(size_t)(w >> 1) * v.Ncm * 2 + (w & 1)] = nw;
        }
        if (acc && on) {
            const int s = a.slot[e];
            if (s >= 0) {
                a.psum[s] += p;
                a.ones[s] += (uint32_t)y;
            }
        }
        // a word whose run straddles two trips is read again by another lane: the store has landed
        __syncthreads();
    }
}

}  // namespace dlsm
