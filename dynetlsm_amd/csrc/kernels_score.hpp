// In-sample scores (no reference counterpart): the AUC and the log-loss of the posterior-mean edge probability
//
//     pbar(t, i, j) = (1 / S) sum_s expit(eta_s),      eta as dyad_eta (kernels_dyad_pass.hpp)
//
// over all scored dyads, without storing or sorting them.  A dyad's rank key is the top 24 bits of (float)pbar,
// clamped from below: key = max(bits(f) >> 8, SCORE_KEY_LO) - 2^15 bins per octave of pbar, every pbar <= 2^-63
// in the lowest one.  k_score_accumulate counts the dyads of a time step into hist[class][key - SCORE_KEY_LO]
// (class = y) with 64-bit integer atomics; k_score_scan turns a histogram into n_pos, n_neg,
//
//     u2 = sum_b pos_b (2 cumneg_b + neg_b)     (twice the Mann-Whitney statistic of the keys, ties counted half)
//     ties = sum_b pos_b neg_b                  (only pairs inside one bin can be ordered differently by pbar)
//
// All four are exact integers, whatever the order of the atomics.  The log-loss term of a dyad,
// -log P(y | pbar) = -log mean_s P(y | eta_s), is the streaming log-sum-exp of kernels_ic.hpp in a cheaper
// form: P(y | eta) = exp(a) w with a = min(eta', 0) <= 0, w = 1 / (1 + exp(-|eta|)) in [1/2, 1] and
// eta' = eta (y = 1) or -eta (y = 0), so the running maximum is kept over a and the sum over w exp(a - max):
// finite for any finite eta, one exp for the probability and one for the rescaling.  The terms leave the kernel
// as per-workgroup partials added in a fixed order (kernels_ic.hpp), so the sums are the same bits on every call.
//
// Tiling, LDS staging of the samples, the bit-packed network reads and eta are the shared ones of a pass over
// posterior samples (kernels_dyad_pass.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "kernels_dyad_pass.hpp"

namespace dlsm {

constexpr uint32_t SCORE_KEY_LO = 0x200000u;                 // bits(2^-63f) >> 8
constexpr uint32_t SCORE_KEY_HI = 0x3F8000u;                 // bits(1.0f) >> 8
constexpr uint32_t SCORE_NBINS = SCORE_KEY_HI - SCORE_KEY_LO + 1;       // 2 064 385
constexpr int SCORE_SCAN_NT = 1024, SCORE_SCAN_NW = SCORE_SCAN_NT / 64;
constexpr int SCORE_SCAN_V = 4;                              // consecutive bins of a lane per step of the scan
// bins of one class as stored: padded so that each wavefront of the scan owns a whole number of its steps
// (the bins beyond SCORE_NBINS are never counted into and stay zero)
constexpr uint32_t SCORE_SCAN_SEG =
    (SCORE_NBINS + SCORE_SCAN_NW * 64 * SCORE_SCAN_V - 1) / (SCORE_SCAN_NW * 64 * SCORE_SCAN_V) * (64 * SCORE_SCAN_V);
constexpr uint32_t SCORE_HSTRIDE = SCORE_SCAN_SEG * SCORE_SCAN_NW;
constexpr size_t SCORE_SLOT = 2 * (size_t)SCORE_HSTRIDE;     // counters of one histogram: [class][bin]

typedef unsigned long long score_count_t;

// The key of pbar.  The upper clamp holds for every pbar in [0, 1]; it is there for a NaN (positions that are
// not finite), whose bits would index beyond the histogram.
__device__ __forceinline__ uint32_t score_key(double pbar) {
    const uint32_t u = __float_as_uint((float)pbar);         // round to nearest even
    return min(max(u >> 8, SCORE_KEY_LO), SCORE_KEY_HI);
}

// hist[c] += 1 from every active lane.  Coincident or saturated positions put whole wavefronts into one bin:
// when the active lanes all hold the same c, the first of them adds their number.
__device__ __forceinline__ void score_hist_add(score_count_t *__restrict__ hist, uint32_t c, int lane) {
    const unsigned long long active = __ballot(1);
    const uint32_t c0 = __builtin_amdgcn_readfirstlane(c);
    if (__ballot(c != c0) == 0) {
        if (lane == __ffsll(active) - 1)
            __hip_atomic_fetch_add(hist + c0, (score_count_t)__popcll(active), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    } else {
        __hip_atomic_fetch_add(hist + c, (score_count_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Xs [S][T][N][D], ic [S][2], radii [S][N] (DIR); bits [T][N][W]; mask NULL or [T][N][W], a set bit: the dyad
// is not scored (undirected: either of (i, j), (j, i)); tiles [n_tiles] = (row block, column block); workgroup
// g = blockIdx.x takes tiles g L .. g L + L - 1 of time step t0 + blockIdx.y.
// hist [gridDim.y][2][SCORE_HSTRIDE], zero on entry; part_ll [T][G] (G = gridDim.x).
template <int D, bool DIR>
__global__ __launch_bounds__(IC_NT) void k_score_accumulate(
    const double *__restrict__ Xs, const double *__restrict__ ic, const double *__restrict__ radii,
    const uint32_t *__restrict__ bits, const uint32_t *__restrict__ mask, const int2 *__restrict__ tiles,
    int n_tiles, int L, int S, int T, int N, int W, int t0, score_count_t *__restrict__ hist,
    double *__restrict__ part_ll) {
    typedef IcStage<D, DIR> St;
    constexpr int DPT = IcPlan<D>::DPT, TI = IcPlan<D>::TI, PT = St::PER_THREAD;
    __shared__ double stage[2][St::N];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = t0 + blockIdx.y, g = blockIdx.x;
    score_count_t *hist_t = hist + (size_t)blockIdx.y * SCORE_SLOT;
    double tot = 0.0;                                         // thread 0: the workgroup's tiles so far
    const int q0 = g * L, q1 = min(n_tiles, q0 + L);
    for (int q = q0; q < q1; ++q) {
        const int i0 = tiles[q].x * TI, j0 = tiles[q].y * IC_TJ;
        const int j = j0 + lane;
        uint32_t valid, ybits;        // the tile's dyads of this thread: which are scored, and the network's bits
        dyad_tile_bits<D, DIR>(bits, mask, t, N, W, i0, j, wv, valid, ybits);
        // m = -inf makes the first sample an ordinary update: r = 0 * e^-inf + w
        double psum[DPT], m[DPT], r[DPT];
#pragma unroll
        for (int k = 0; k < DPT; ++k) { psum[k] = 0.0; m[k] = -__builtin_inf(); r[k] = 0.0; }
        dyad_stage_first<D, DIR>(stage[0], Xs, ic, radii, t, N, i0, j0, tid);
        __syncthreads();
        for (int s = 0; s < S; ++s) {
            const int cur = s & 1;
            const double *sb = stage[cur];
            double pre[PT];           // the next sample's block, in flight under this sample's arithmetic
            if (s + 1 < S) dyad_stage_prefetch<D, DIR>(pre, Xs, ic, radii, s + 1, T, t, N, i0, j0, tid);
            const DyadColumn<D> col = dyad_column<D, DIR>(sb, lane);
#pragma unroll
            for (int k = 0; k < DPT; ++k) {
                const double eta = dyad_eta<D, DIR>(sb, 4 * k + wv, col);
                // expit(eta) = w (eta >= 0) or e w, with e = exp(-|eta|) <= 1: no overflow, no cancellation
                const double e = exp(-fabs(eta));
                const double w = 1.0 / (1.0 + e);
                psum[k] += eta >= 0.0 ? w : e * w;
                // P(y | eta) = exp(a) w
                const double a = fmin(((ybits >> k) & 1u) ? eta : -eta, 0.0);
                const double da = a - m[k];
                const double ex = exp(-fabs(da));
                r[k] = da > 0.0 ? fma(r[k], ex, w) : fma(w, ex, r[k]);
                m[k] = fmax(m[k], a);
            }
            if (s + 1 < S) dyad_stage_commit<D, DIR>(stage[cur ^ 1], pre, tid);
            __syncthreads();
        }
        // the tile's dyads: the key into the histogram, the log-loss term into the sum
        const double dS = (double)S;
        double ll = 0.0;
#pragma unroll
        for (int k = 0; k < DPT; ++k) {
            if ((valid >> k) & 1u) {
                const uint32_t bin = score_key(psum[k] / dS) - SCORE_KEY_LO;
                score_hist_add(hist_t, ((ybits >> k) & 1u) * SCORE_HSTRIDE + bin, lane);
                ll -= m[k] + log(r[k] / dS);
            }
        }
        ll = wave_sum_all(ll);
        if (lane == 0) red[wv] = ll;
        __syncthreads();
        if (tid == 0) tot += (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();          // red is free for the next tile
    }
    if (tid == 0) part_ll[(size_t)t * gridDim.x + g] = tot;
}

// logloss[t] = sum_g part_ll[t][g]: thread q adds g = q, q + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(IC_NT) void k_score_reduce_logloss(const double *__restrict__ part_ll, int G,
                                                                double *__restrict__ logloss) {
    __shared__ double buf[IC_NT];
    const int tid = threadIdx.x, t = blockIdx.x;
    double v = 0.0;
    for (int g = tid; g < G; g += IC_NT) v += part_ll[(size_t)t * G + g];
    buf[tid] = v;
    __syncthreads();
    for (int o = IC_NT / 2; o > 0; o >>= 1) {
        if (tid < o) buf[tid] += buf[tid + o];
        __syncthreads();
    }
    if (tid == 0) logloss[t] = buf[0];
}

__device__ __forceinline__ score_count_t score_wave_sum(score_count_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// counts [gridDim.x][4] = n_pos, n_neg, u2, ties of hist [gridDim.x][2][SCORE_HSTRIDE]; pooled != NULL: every
// histogram is also added into pooled [2][SCORE_HSTRIDE].  One workgroup per histogram, one pass over the bins:
// wavefront w owns the bins w SEG .. (w + 1) SEG - 1 and scans them with cumneg counted from its own first bin
// (a lane takes SCORE_SCAN_V consecutive bins per step, the wavefront an exclusive scan of the lanes' sums);
// the negatives of the wavefronts below enter at the end, u2 = sum_w u2_w + 2 n_pos_w sum_{w' < w} n_neg_w'.
// Every intermediate is at most 2 n_pos n_neg, which the caller keeps below 2^64.
__global__ __launch_bounds__(SCORE_SCAN_NT) void k_score_scan(const score_count_t *__restrict__ hist,
                                                              score_count_t *__restrict__ pooled,
                                                              score_count_t *__restrict__ counts) {
    constexpr int V = SCORE_SCAN_V;
    __shared__ score_count_t part[4][SCORE_SCAN_NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const score_count_t *neg_h = hist + (size_t)blockIdx.x * SCORE_SLOT, *pos_h = neg_h + SCORE_HSTRIDE;
    score_count_t carry = 0, n_pos = 0, u2 = 0, ties = 0;     // carry: the wavefront's negatives so far
    const uint32_t lo = wv * SCORE_SCAN_SEG, hi = lo + SCORE_SCAN_SEG;
    for (uint32_t b0 = lo; b0 < hi; b0 += 64 * V) {
        const uint32_t b = b0 + lane * V;
        score_count_t neg[V], pos[V];
        {
            const ulonglong2 *pn = (const ulonglong2 *)(neg_h + b), *pp = (const ulonglong2 *)(pos_h + b);
#pragma unroll
            for (int v = 0; v < V; v += 2) {
                const ulonglong2 a = pn[v / 2], c = pp[v / 2];
                neg[v] = a.x; neg[v + 1] = a.y; pos[v] = c.x; pos[v + 1] = c.y;
            }
        }
        score_count_t any = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) any |= neg[v] | pos[v];
        if (__ballot(any != 0) == 0) continue;               // an empty stretch: most of the histogram
        if (pooled) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (neg[v])
                    __hip_atomic_fetch_add(pooled + b + v, neg[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (pos[v])
                    __hip_atomic_fetch_add(pooled + SCORE_HSTRIDE + b + v, pos[v], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        score_count_t mine = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) mine += neg[v];
        score_count_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const score_count_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        score_count_t below = carry + (incl - mine);          // negatives in the bins below this lane's
#pragma unroll
        for (int v = 0; v < V; ++v) {
            u2 += pos[v] * (2 * below + neg[v]);
            ties += pos[v] * neg[v];
            n_pos += pos[v];
            below += neg[v];
        }
        carry += __shfl(incl, 63);
    }
    n_pos = score_wave_sum(n_pos); u2 = score_wave_sum(u2); ties = score_wave_sum(ties);
    if (lane == 0) { part[0][wv] = n_pos; part[1][wv] = carry; part[2][wv] = u2; part[3][wv] = ties; }
    __syncthreads();
    if (tid == 0) {
        score_count_t P = 0, Nn = 0, U = 0, Ti = 0;
        for (int w = 0; w < SCORE_SCAN_NW; ++w) {
            U += part[2][w] + 2 * part[0][w] * Nn;
            P += part[0][w]; Nn += part[1][w]; Ti += part[3][w];
        }
        score_count_t *out = counts + 4 * (size_t)blockIdx.x;
        out[0] = P; out[1] = Nn; out[2] = U; out[3] = Ti;
    }
}

}  // namespace dlsm
