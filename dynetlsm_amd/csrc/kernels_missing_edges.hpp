// Lists of missing dyads -> the job tables of the imputation step (dlsm_set_missing_edges, capi_missing_edges.hpp).
//
//   k_miss_rows_count   per row of a time step's two bit arrays: its bits, its owning bits, overlap with the network
//   k_miss_rows_emit    per non-empty row: its columns, ascending, and each entry's slot -> miss_cols / miss_slot
//   k_miss_index        the (t, i, j) row of every slot, read back from jobs / cols / slot (either builder's)
//
// The lists reach the bit arrays through k_edges_scatter (kernels_edges.hpp): pairs in any order and orientation,
// duplicates and mirrored pairs collapse into one bit, so the tables are a function of the SET of listed dyads.  The
// forward array holds bit j of row i for a pair (i, j), the transposed one bit i of row j; the undirected model
// passes one array twice.  A dyad's slot is its rank in row-major (t, i, j) order - i < j undirected -: the slot
// base of a row (an exclusive sum over the rows before it) plus its rank among the row's owning bits, which are the
// columns beyond the row (undirected) or all bits of the forward array (directed).  Nothing is sorted anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_edges.hpp"
#include "kernels_missing.hpp"

namespace dlsm {

constexpr int MISS_TIE_LISTED = 4;      // flag bit beside EDGE_BAD_INDEX / EDGE_SELF_LOOP: a listed dyad is a tie

// the bits of word w of row `row` of matrix z that own their dyad
__device__ __forceinline__ uint32_t miss_own_mask(int undirected, int z, int row, int w) {
    if (!undirected) return z ? 0u : ~0u;
    if (32 * w > row) return ~0u;
    if (32 * w + 31 <= row) return 0u;
    return ~((2u << (row & 31)) - 1u);          // (row & 31 < 31 here)
}

// One wavefront per row i and matrix (blockIdx.y = 0: `fwd`, 1: `bwd`, directed only).  cnt_t / own_t: [nz][N] of
// this time step.  ynet: the same time step's rows of the packed network, or NULL for no tie check (matrix 0 only:
// the transposed rows say the same).
__global__ __launch_bounds__(64 * ROWS_WAVES) void k_miss_rows_count(const uint32_t *__restrict__ fwd,
                                                                     const uint32_t *__restrict__ bwd,
                                                                     const uint32_t *__restrict__ ynet, int N, int W,
                                                                     int undirected, int32_t *__restrict__ cnt_t,
                                                                     int32_t *__restrict__ own_t,
                                                                     int *__restrict__ flag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * ROWS_WAVES + wave, z = blockIdx.y;
    if (i >= N) return;
    const uint32_t *r = (z ? bwd : fwd) + (size_t)i * W;
    const uint32_t *y = (ynet && !z) ? ynet + (size_t)i * W : nullptr;
    int cnt = 0, own = 0;
    uint32_t both = 0u;
    for (int w = lane; w < W; w += 64) {
        const uint32_t v = r[w];
        cnt += __popc(v);
        own += __popc(v & miss_own_mask(undirected, z, i, w));
        if (y) both |= v & y[w];
    }
    for (int d = 32; d > 0; d >>= 1) { cnt += __shfl_xor(cnt, d); own += __shfl_xor(own, d); }
    if (__ballot(both != 0u) && lane == 0) atomicOr(flag, MISS_TIE_LISTED);
    if (lane == 0) { cnt_t[(size_t)z * N + i] = cnt; own_t[(size_t)z * N + i] = own; }
}

// One wavefront per job of this time step (jobs[0 .. nj), slot0[k] the slot base of job k).  Per trip a lane takes
// one word; the wave-exclusive prefix sums of the words' popcounts are where the lane's entries and slots go, behind
// those of the trips before (k_rows_emit).  An entry that does not own its dyad gets slot -1.
__global__ __launch_bounds__(64 * ROWS_WAVES) void k_miss_rows_emit(const uint32_t *__restrict__ fwd,
                                                                    const uint32_t *__restrict__ bwd, int W,
                                                                    int undirected, const MissJob *__restrict__ jobs,
                                                                    const int32_t *__restrict__ slot0, int nj,
                                                                    int32_t *__restrict__ cols,
                                                                    int32_t *__restrict__ slot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * ROWS_WAVES + wave;
    if (k >= nj) return;
    const MissJob job = jobs[k];
    const int z = job.tz & 1, row = job.row;
    const uint32_t *r = (z ? bwd : fwd) + (size_t)row * W;
    int base = job.begin, sbase = slot0[k];
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int w = w0 + lane;
        uint32_t v = w < W ? r[w] : 0u;
        const uint32_t om = w < W ? miss_own_mask(undirected, z, row, w) : 0u;
        const int cnt = __popc(v), ocnt = __popc(v & om);
        int incl = cnt, oincl = ocnt;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d), oup = __shfl_up(oincl, d);
            if (lane >= d) { incl += up; oincl += oup; }
        }
        int pos = base + incl - cnt, spos = sbase + oincl - ocnt;
        while (v) {
            const int b = __ffs(v) - 1;
            const bool owns = (om >> b) & 1u;
            v &= v - 1;
            if (pos < job.end) {                // (the segment is this row's popcount: always)
                cols[pos] = 32 * w + b;
                slot[pos] = owns ? spos : -1;
            }
            ++pos;
            spos += owns;
        }
        base += __shfl(incl, 63);
        sbase += __shfl(oincl, 63);
    }
}

// One wavefront per job of the finished tables: the entry that owns slot s writes row s of tij[n][3].  Every slot
// has exactly one owning entry, so every row is written once.
__global__ __launch_bounds__(64 * ROWS_WAVES) void k_miss_index(const MissJob *__restrict__ jobs, int nj,
                                                                const int32_t *__restrict__ cols,
                                                                const int32_t *__restrict__ slot, long n,
                                                                int32_t *__restrict__ tij) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * ROWS_WAVES + wave;
    if (k >= nj) return;
    const MissJob job = jobs[k];
    for (int e = job.begin + lane; e < job.end; e += 64) {
        const int s = slot[e];
        if (s < 0 || s >= n) continue;
        // matrix 0: row r holds the dyad (r, c); matrix 1 (the transposed rows): (c, r)
        const int c = cols[e];
        tij[3 * (size_t)s] = job.tz >> 1;
        tij[3 * (size_t)s + 1] = (job.tz & 1) ? c : job.row;
        tij[3 * (size_t)s + 2] = (job.tz & 1) ? job.row : c;
    }
}

}  // namespace dlsm
