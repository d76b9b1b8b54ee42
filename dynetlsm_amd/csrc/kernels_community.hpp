// Community structure of stored labellings against the packed network (capi_community.hpp; the definition of the
// tables: include/dynetlsm_hip.h, dlsm_community_accumulate).  The reference has modularity(Y, z) for one labelling
// on the host (network_statistics.py:31-61: a dense S^T B S per time step); everything else here has no counterpart.
//
// Per tie, not per cluster: a labelling (s, t) stages its N byte labels in LDS, a row's set bits are walked and
// the label of every neighbour is gathered from LDS.  The cost follows the ties and does not depend on K; the
// other form - K membership masks per labelling, AND + popcount against the row words - costs N W K_used words
// and K W words of LDS.
//
// Everything added across workgroups is an integer added with a vector atomic: the tables do not depend on the
// order, the grid or the staging batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dlsm {

constexpr int CM_NT = 256;            // threads of a workgroup
constexpr int CM_SLOTS = 5;           // per cluster: size, within, out-volume, in-volume, excluded within
constexpr int CM_ROWS_MAX = 4096;     // rows of one workgroup (their node_within sums sit in LDS)

typedef unsigned long long cm_count_t;

// int64 labels [n] (validated on the host) -> bytes
__global__ __launch_bounds__(256) void k_comm_pack_labels(const int64_t *__restrict__ zs, size_t n,
                                                          uint8_t *__restrict__ z8) {
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256)
        z8[q] = (uint8_t)zs[q];
}

struct CommArgs {
    const uint8_t *z8;          // [ns][T][N] labels of the staged samples
    const uint32_t *bits;       // [T][N][W] the network
    const uint32_t *mask;       // [T][N][W] excluded dyads (symmetric for undirected handles, no diagonal, no
                                // padding bit), or NULL
    const uint32_t *indeg;      // [T][N] in-degrees of bits & ~mask
    int ns, T, N, W, K;
    int rows;                   // rows of a workgroup (<= CM_ROWS_MAX)
    int lpr;                    // lanes that share a row: a power of two in 4..64
    cm_count_t *clusters;       // [ns][T][K][CM_SLOTS]
    cm_count_t *node_within;    // [T][N]
    cm_count_t *blocks;         // [ns][T][K][K][2] or NULL
};

// LDS of k_comm_rows in bytes: the labels of every bit position of a row, the cluster table, the rows' sums
inline size_t comm_lds_bytes(int W, int K, int rows) {
    return (size_t)W * 32 + ((size_t)K * CM_SLOTS + rows) * sizeof(uint32_t);
}

// the set bits of `word` (columns base ..): how many carry label `a`; BLOCKS: each adds 1 to blk[2 * label]
// (runs of one label are added at once)
template <bool BLOCKS>
__device__ __forceinline__ uint32_t comm_walk(uint32_t word, int base, const uint8_t *zl, int a, cm_count_t *blk,
                                              int &cur, uint32_t &run) {
    uint32_t same = 0;
    while (word) {
        const int j = base + __builtin_ctz(word);
        word &= word - 1;
        const int b = zl[j];
        same += b == a;
        if (BLOCKS) {
            if (b != cur) {
                if (run) atomicAdd(blk + 2 * cur, (cm_count_t)run);
                cur = b; run = 0;
            }
            ++run;
        }
    }
    return same;
}

// grid (row chunks, T, sample groups): workgroup (c, t, g) owns rows c rows .. and walks them for the staged
// samples g, g + gridDim.z, ...
template <bool BLOCKS>
__global__ __launch_bounds__(CM_NT) void k_comm_rows(CommArgs p) {
    extern __shared__ uint32_t cm_lds[];
    uint8_t *zl = (uint8_t *)cm_lds;                        // [32 W]: beyond N never read (no such bit is set)
    uint32_t *cl = cm_lds + p.W * 8;                        // [K][CM_SLOTS]
    uint32_t *nw = cl + p.K * CM_SLOTS;                     // [rows]
    const int tid = threadIdx.x, t = blockIdx.y, N = p.N, W = p.W, K = p.K;
    const int r0 = blockIdx.x * p.rows, r1 = min(N, r0 + p.rows);
    const int lpr = p.lpr, sub = tid & (lpr - 1), slot = tid / lpr, per_pass = CM_NT / lpr;
    for (int q = tid; q < r1 - r0; q += CM_NT) nw[q] = 0u;
    for (int s = blockIdx.z; s < p.ns; s += gridDim.z) {
        __syncthreads();                                    // the last sample's table is flushed, its labels read
        const size_t lab = (size_t)s * p.T + t;
        const uint8_t *z = p.z8 + lab * N;
        for (int q = tid; q < N; q += CM_NT) zl[q] = z[q];
        for (int q = tid; q < K * CM_SLOTS; q += CM_NT) cl[q] = 0u;
        __syncthreads();
        for (int i = r0 + slot; i < r1; i += per_pass) {    // the lpr lanes of a row leave together
            const int a = zl[i];
            const uint32_t *row = p.bits + ((size_t)t * N + i) * W;
            const uint32_t *mrow = p.mask ? p.mask + ((size_t)t * N + i) * W : nullptr;
            cm_count_t *blk = BLOCKS ? p.blocks + (lab * K + a) * K * 2 : nullptr;     // [b][ties, excluded]
            cm_count_t *blk_ex = BLOCKS ? blk + 1 : nullptr;
            uint32_t within = 0, vol = 0, excl = 0;
            for (int w = sub; w < W; w += lpr) {
                const uint32_t m = mrow ? mrow[w] : 0u;
                const uint32_t y = row[w] & ~m;
                int cur = 0; uint32_t run = 0;
                vol += __popc(y);
                within += comm_walk<BLOCKS>(y, 32 * w, zl, a, blk, cur, run);
                if (BLOCKS && run) atomicAdd(blk + 2 * cur, (cm_count_t)run);
                cur = 0; run = 0;
                excl += comm_walk<BLOCKS>(m, 32 * w, zl, a, blk_ex, cur, run);
                if (BLOCKS && run) atomicAdd(blk_ex + 2 * cur, (cm_count_t)run);
            }
            for (int o = lpr >> 1; o; o >>= 1) {
                within += __shfl_xor(within, o);
                vol += __shfl_xor(vol, o);
                excl += __shfl_xor(excl, o);
            }
            if (sub == 0) {
                uint32_t *c = cl + a * CM_SLOTS;
                atomicAdd(c + 0, 1u);
                if (within) atomicAdd(c + 1, within);
                if (vol) atomicAdd(c + 2, vol);
                const uint32_t in = p.indeg[(size_t)t * N + i];
                if (in) atomicAdd(c + 3, in);
                if (excl) atomicAdd(c + 4, excl);
                nw[i - r0] += within;                       // this lane alone holds the row
            }
        }
        __syncthreads();
        cm_count_t *out = p.clusters + lab * K * CM_SLOTS;
        for (int q = tid; q < K * CM_SLOTS; q += CM_NT)
            if (cl[q]) atomicAdd(out + q, (cm_count_t)cl[q]);
    }
    __syncthreads();
    for (int q = tid; q < r1 - r0; q += CM_NT)
        if (nw[q]) atomicAdd(p.node_within + (size_t)t * N + r0 + q, (cm_count_t)nw[q]);
}

// node_switch[u][i] += #{staged s : z[s][u+1][i] != z[s][u][i]}, moved[s][u] += #{i : ...}.  grid (ceil(N / 256),
// T - 1): thread (i, u) owns its entry of node_switch, a wavefront adds its count to moved.
__global__ __launch_bounds__(256) void k_comm_switch(const uint8_t *__restrict__ z8, int ns, int T, int N,
                                                     cm_count_t *__restrict__ node_switch,
                                                     cm_count_t *__restrict__ moved) {
    const int i = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    const bool live = i < N;
    uint32_t mine = 0;
    for (int s = 0; s < ns; ++s) {
        const uint8_t *z = z8 + ((size_t)s * T + u) * N;
        const bool d = live && z[i] != z[(size_t)N + i];
        mine += d;
        const unsigned long long b = __ballot(d);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(moved + (size_t)s * (T - 1) + u, (cm_count_t)__popcll(b));
    }
    if (live && mine) atomicAdd(node_switch + (size_t)u * N + i, (cm_count_t)mine);
}

}  // namespace dlsm
