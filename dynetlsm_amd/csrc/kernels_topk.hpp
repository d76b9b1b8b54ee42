// Link prediction (no reference counterpart): per time step the k eligible dyads that come first by the
// posterior-mean edge probability
//
//     pbar(t, i, j) = (1 / S) sum_s expit(eta_s),      eta as dyad_eta (kernels_dyad_pass.hpp), s = 0 .. S - 1 in order
//
// (descending, or ascending with largest = 0), exactly and without storing or sorting the T N^2 values: selection by
// the rank key of kernels_score.hpp, which is monotone in pbar.
//
//   1. k_topk_count    the sample loop over every tile: each eligible dyad's score_key(pbar) is counted into
//                      hist[t][key - SCORE_KEY_LO] (one class, the 64-bit counters and the wave-aggregated add of
//                      kernels_score.hpp), and the tile's extreme key - the largest, or with largest = 0 the smallest;
//                      topk_none() for a tile without an eligible dyad - goes to meta[t][TOPK_META + q].
//   2. k_topk_threshold  one workgroup per time step walks the histogram from the top (largest = 0: from the bottom)
//                      to the key kappa_t with count(beyond kappa_t) < k <= count(beyond or at kappa_t) and writes
//                      meta[t][0..3] = eligible_t, n_beyond_t, n_at_t, kappa_t.  Fewer than k eligible dyads: kappa_t
//                      is the last key that is not empty.  None: kappa_t is the key that nothing reaches.
//      The host reads meta once, refuses a step whose n_beyond + n_at is beyond the caller's room, and lists the
//      (t, tile) whose extreme key reaches kappa_t.
//   3. k_topk_emit     the same sample loop over the listed tiles only, with Welford's mean and M2 of p_s next to
//                      the sum (as k_proba_accumulate forms them); every eligible dyad whose key reaches kappa_t takes
//                      a slot by a returning atomicAdd on n_cand[t] and writes (i, j, y) and (pbar, sd).
//
// The k first dyads by (pbar, i, j) are among the emitted ones, because the key never decreases with pbar; the host
// sorts the emitted dyads by the doubles and cuts, so the order of the atomics shows in no output.
//
// Both launches form pbar in topk_tile_samples: the same instructions on the same inputs in the same order, with
// expit and the sum kept from being fused with anything around them, so a dyad has the same bits and the same key
// in both.  That is why the room cannot be overrun: the counts of step 2 are exact integers of the very keys that
// step 3 compares with kappa_t, so exactly n_beyond_t + n_at_t dyads take a slot, and the host has checked that number
// against the room before the launch.  The kernel bounds the slot all the same, and the host compares n_cand with
// the count afterwards.
//
// Tiling, LDS staging of the samples, the bit-packed network reads and eta are the shared ones of a pass over
// posterior samples (kernels_dyad_pass.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_dyad_pass.hpp"
#include "kernels_score.hpp"

namespace dlsm {

// which dyads are eligible (`among`): observed = its mask bit is clear (undirected: that of (j, i) as well)
enum : int {
    TOPK_NON_TIES = 0,      // observed and y = 0
    TOPK_TIES = 1,          // observed and y = 1
    TOPK_OBSERVED = 2,      // observed
    TOPK_MISSING = 3,       // masked
    TOPK_ALL = 4,           // every dyad of the model
    TOPK_AMONG_COUNT = 5
};

constexpr int TOPK_META = 4;        // words of a time step's row of meta ahead of its tiles' keys

// the extreme key of a tile without an eligible dyad, and the threshold of a time step without one: no key
// reaches the latter, and the former reaches no threshold
__host__ __device__ __forceinline__ uint32_t topk_none(bool largest) { return largest ? 0u : 0xFFFFFFFFu; }
__host__ __device__ __forceinline__ uint32_t topk_unreachable(bool largest) { return largest ? 0xFFFFFFFFu : 0u; }
__host__ __device__ __forceinline__ bool topk_reaches(uint32_t key, uint32_t kappa, bool largest) {
    return largest ? key >= kappa : key <= kappa;
}

// The tile's dyads of this thread (rows i0 + 4 k + wv, column j) at time step t, as dyad_tile_bits: bit k of elig -
// the dyad exists and is eligible under `among` -, bit k of ybits - its bit of the network, eligible or not.
template <int D, bool DIR>
__device__ __forceinline__ void topk_tile_bits(const uint32_t *bits, const uint32_t *mask, int among, int t, int N,
                                               int W, int i0, int j, int wv, uint32_t &elig, uint32_t &ybits) {
    elig = 0; ybits = 0;
#pragma unroll
    for (int k = 0; k < IcPlan<D>::DPT; ++k) {
        const int i = i0 + 4 * k + wv;
        if (!(i < N && j < N && (DIR ? i != j : i < j))) continue;
        const size_t at = ((size_t)t * N + i) * W + (j >> 5);
        const uint32_t y = (bits[at] >> (j & 31)) & 1u;
        uint32_t mb = 0;
        if (mask) {
            mb = mask[at] >> (j & 31);
            if (!DIR) mb |= mask[((size_t)t * N + j) * W + (i >> 5)] >> (i & 31);
            mb &= 1u;
        }
        bool ok;
        switch (among) {
            case TOPK_NON_TIES: ok = !mb && !y; break;
            case TOPK_TIES: ok = !mb && y; break;
            case TOPK_OBSERVED: ok = !mb; break;
            case TOPK_MISSING: ok = mb; break;
            default: ok = true;
        }
        elig |= (uint32_t)ok << k;
        ybits |= y << k;
    }
}

// psum + expit(eta), and p = expit(eta) = w (eta >= 0) or e w, with e = exp(-|eta|) <= 1, w = 1 / (1 + e) (as
// k_score_accumulate).  Every operation is rounded on its own, whatever the caller does with p.
__device__ __forceinline__ double topk_add_expit(double psum, double eta, double &p) {
#pragma clang fp contract(off)
    const double e = exp(-fabs(eta));
    const double w = 1.0 / (1.0 + e);
    p = eta >= 0.0 ? w : e * w;
    return psum + p;
}

__device__ __forceinline__ double topk_pbar(double psum, int S) { return psum / (double)S; }

// The sample loop of one tile (rows i0.., columns j0.. of time step t) on the stage buffers stage [2][IcStage::N]:
// psum [DPT] of this thread's dyads over the S samples and, with WELFORD, the running mean and M2 [DPT] of p_s.
// Ends on the barrier after the last sample: stage is free for the next tile.
template <int D, bool DIR, bool WELFORD>
__device__ __forceinline__ void topk_tile_samples(double *stage, const double *__restrict__ Xs,
                                                  const double *__restrict__ ic, const double *__restrict__ radii,
                                                  int S, int T, int t, int N, int i0, int j0, int tid, double *psum,
                                                  double *mean, double *m2) {
    typedef IcStage<D, DIR> St;
    constexpr int DPT = IcPlan<D>::DPT, PT = St::PER_THREAD;
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < DPT; ++k) { psum[k] = 0.0; mean[k] = 0.0; m2[k] = 0.0; }
    dyad_stage_first<D, DIR>(stage, Xs, ic, radii, t, N, i0, j0, tid);
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        const int cur = s & 1;
        const double *sb = stage + cur * St::N;
        double pre[PT];               // the next sample's block, in flight under this sample's arithmetic
        if (s + 1 < S) dyad_stage_prefetch<D, DIR>(pre, Xs, ic, radii, s + 1, T, t, N, i0, j0, tid);
        const DyadColumn<D> col = dyad_column<D, DIR>(sb, lane);
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
            const double eta = dyad_eta<D, DIR>(sb, 4 * k + wv, col);
            double p;
            psum[k] = topk_add_expit(psum[k], eta, p);
            if (WELFORD) {
                const double dl = p - mean[k];
                mean[k] += dl / (double)(s + 1);
                m2[k] = fma(dl, p - mean[k], m2[k]);
            }
        }
        if (s + 1 < S) dyad_stage_commit<D, DIR>(stage + (cur ^ 1) * St::N, pre, tid);
        __syncthreads();
    }
}

// Xs [S][T][N][D], ic [S][2], radii [S][N] (DIR); bits [T][N][W]; mask NULL or [T][N][W]; tiles [n_tiles] = (row
// block, column block); workgroup g = blockIdx.x takes tiles g L .. g L + L - 1 of time step t0 + blockIdx.y.
// hist [gridDim.y][SCORE_HSTRIDE], zero on entry; meta [T][TOPK_META + n_tiles].
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) void k_topk_count(
    const double *__restrict__ Xs, const double *__restrict__ ic, const double *__restrict__ radii,
    const uint32_t *__restrict__ bits, const uint32_t *__restrict__ mask, const int2 *__restrict__ tiles,
    int n_tiles, int L, int S, int T, int N, int W, int t0, int among, int largest,
    score_count_t *__restrict__ hist, uint32_t *__restrict__ meta) {
    typedef IcStage<D, DIR> St;
    constexpr int DPT = IcPlan<D>::DPT, TI = IcPlan<D>::TI;
    __shared__ double stage[2 * St::N];
    __shared__ uint32_t kred[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = t0 + blockIdx.y, g = blockIdx.x;
    score_count_t *hist_t = hist + (size_t)blockIdx.y * SCORE_HSTRIDE;
    uint32_t *tile_key = meta + (size_t)t * (TOPK_META + n_tiles) + TOPK_META;
    const bool top = largest != 0;
    const int q0 = g * L, q1 = min(n_tiles, q0 + L);
    for (int q = q0; q < q1; ++q) {
        const int i0 = tiles[q].x * TI, j0 = tiles[q].y * IC_TJ;
        uint32_t elig, ybits;
        topk_tile_bits<D, DIR>(bits, mask, among, t, N, W, i0, j0 + lane, wv, elig, ybits);
        double psum[DPT], mean[DPT], m2[DPT];
        topk_tile_samples<D, DIR, false>(stage, Xs, ic, radii, S, T, t, N, i0, j0, tid, psum, mean, m2);
        uint32_t ext = topk_none(top);
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
            if ((elig >> k) & 1u) {
                const uint32_t key = score_key(topk_pbar(psum[k], S));
                score_hist_add(hist_t, key - SCORE_KEY_LO, lane);
                ext = top ? max(ext, key) : min(ext, key);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = __shfl_xor(ext, o);
            ext = top ? max(ext, other) : min(ext, other);
        }
        if (lane == 0) kred[wv] = ext;
        __syncthreads();
        if (tid == 0)
            tile_key[q] = top ? max(max(kred[0], kred[1]), max(kred[2], kred[3]))
                              : min(min(kred[0], kred[1]), min(kred[2], kred[3]));
        __syncthreads();          // kred is free for the next tile
    }
}

// the counts at the positions p .. p + V - 1 of the scan order (p a multiple of V): position p is bin p from the
// bottom, or with `top` bin SCORE_HSTRIDE - 1 - p
__device__ __forceinline__ void topk_scan_load(const score_count_t *__restrict__ h, uint32_t p, bool top,
                                               score_count_t (&c)[SCORE_SCAN_V]) {
    constexpr int V = SCORE_SCAN_V;
    const ulonglong2 *src = (const ulonglong2 *)(h + (top ? SCORE_HSTRIDE - V - p : p));
    score_count_t a[V];
#pragma unroll
    for (int v = 0; v < V; v += 2) {
        const ulonglong2 x = src[v / 2];
        a[v] = x.x; a[v + 1] = x.y;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) c[v] = top ? a[V - 1 - v] : a[v];
}

// meta [t0 + blockIdx.x][0..3] = eligible, n_beyond, n_at, kappa of hist [gridDim.x][SCORE_HSTRIDE] (row: the
// words of one time step in meta).  One workgroup per histogram.  Wavefront w owns the positions w SEG ..
// (w + 1) SEG - 1 of the scan order and adds them up, skipping empty stretches as k_score_scan does; the wavefront
// in whose segment the running count reaches min(k, eligible) then walks it again, a wavefront scan per step, to
// the bin.  Every count is below 2^31 (the caller bounds the dyads of a time step).
__global__ __launch_bounds__(SCORE_SCAN_NT) void k_topk_threshold(const score_count_t *__restrict__ hist,
                                                                  unsigned long long k, int largest, int t0,
                                                                  size_t row, uint32_t *__restrict__ meta) {
    constexpr int V = SCORE_SCAN_V;
    __shared__ score_count_t seg[SCORE_SCAN_NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool top = largest != 0;
    const score_count_t *h = hist + (size_t)blockIdx.x * SCORE_HSTRIDE;
    uint32_t *out = meta + (size_t)(t0 + blockIdx.x) * row;
    const uint32_t lo = wv * SCORE_SCAN_SEG, hi = lo + SCORE_SCAN_SEG;
    score_count_t sum = 0;
    for (uint32_t p0 = lo; p0 < hi; p0 += 64 * V) {
        score_count_t c[V];
        topk_scan_load(h, p0 + lane * V, top, c);
        score_count_t mine = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) mine += c[v];
        if (__ballot(mine != 0) == 0) continue;              // an empty stretch: most of the histogram
        sum += mine;
    }
    sum = score_wave_sum(sum);
    if (lane == 0) seg[wv] = sum;
    __syncthreads();
    score_count_t eligible = 0;
    for (int w = 0; w < SCORE_SCAN_NW; ++w) eligible += seg[w];
    if (eligible == 0) {
        if (tid == 0) { out[0] = 0u; out[1] = 0u; out[2] = 0u; out[3] = topk_unreachable(top); }
        return;
    }
    const score_count_t need = min((score_count_t)k, eligible);      // >= 1
    score_count_t beyond = 0;         // the counts of the segments before the one that reaches `need`
    int ws = 0;
    while (ws < SCORE_SCAN_NW - 1 && beyond + seg[ws] < need) beyond += seg[ws++];   // they add up to eligible >= need
    if (wv != ws) return;
    for (uint32_t p0 = lo; p0 < hi; p0 += 64 * V) {
        score_count_t c[V];
        topk_scan_load(h, p0 + lane * V, top, c);
        score_count_t mine = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) mine += c[v];
        if (__ballot(mine != 0) == 0) continue;
        score_count_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const score_count_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        const unsigned long long hit = __ballot(beyond + incl >= need);
        if (hit == 0) { beyond += __shfl(incl, 63); continue; }
        if (lane == __ffsll(hit) - 1) {
            score_count_t b = beyond + (incl - mine);         // < need: the lane before did not reach it
            bool done = false;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (!done && b + c[v] >= need) {
                    const uint32_t p = p0 + lane * V + v;
                    out[0] = (uint32_t)eligible; out[1] = (uint32_t)b; out[2] = (uint32_t)c[v];
                    out[3] = SCORE_KEY_LO + (top ? SCORE_HSTRIDE - 1 - p : p);
                    done = true;
                }
                b += c[v];
            }
        }
        return;
    }
}

// Workgroup blockIdx.x takes the tile list[blockIdx.x] = (t, q); meta as k_topk_count and k_topk_threshold left it.
// n_cand [T], zero on entry; cand_index [T][cap] = (i, j, y, 0), cand_value [T][cap] = (pbar, sd).
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) void k_topk_emit(
    const double *__restrict__ Xs, const double *__restrict__ ic, const double *__restrict__ radii,
    const uint32_t *__restrict__ bits, const uint32_t *__restrict__ mask, const int2 *__restrict__ tiles,
    const int2 *__restrict__ list, int n_tiles, int S, int T, int N, int W, int among, int largest,
    const uint32_t *__restrict__ meta, uint32_t cap, unsigned int *__restrict__ n_cand,
    int4 *__restrict__ cand_index, double2 *__restrict__ cand_value) {
    typedef IcStage<D, DIR> St;
    constexpr int DPT = IcPlan<D>::DPT, TI = IcPlan<D>::TI;
    __shared__ double stage[2 * St::N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = list[blockIdx.x].x, q = list[blockIdx.x].y;
    const bool top = largest != 0;
    const uint32_t kappa = meta[(size_t)t * (TOPK_META + n_tiles) + 3];
    const int i0 = tiles[q].x * TI, j0 = tiles[q].y * IC_TJ;
    const int j = j0 + lane;
    uint32_t elig, ybits;
    topk_tile_bits<D, DIR>(bits, mask, among, t, N, W, i0, j, wv, elig, ybits);
    double psum[DPT], mean[DPT], m2[DPT];
    topk_tile_samples<D, DIR, true>(stage, Xs, ic, radii, S, T, t, N, i0, j0, tid, psum, mean, m2);
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
        if (!((elig >> k) & 1u)) continue;
        const double pbar = topk_pbar(psum[k], S);
        if (!topk_reaches(score_key(pbar), kappa, top)) continue;
        const unsigned int slot = atomicAdd(n_cand + t, 1u);
        if (slot < cap) {
            const size_t at = (size_t)t * cap + slot;
            cand_index[at] = make_int4(i0 + 4 * k + wv, j, (int)((ybits >> k) & 1u), 0);
            cand_value[at] = make_double2(pbar, sqrt(m2[k] / (double)(S - 1)));
        }
    }
}

}  // namespace dlsm
