// Building blocks of a pass over posterior samples that keeps its accumulators per dyad in registers:
// k_ic_accumulate (kernels_ic.hpp), k_score_accumulate (kernels_score.hpp), k_conv_accumulate (kernels_conv.hpp).
//
// Work: a workgroup of IC_NT = 256 threads owns tiles of IcPlan<D>::TI x 64 dyads of one time step (rows x
// columns; undirected: only tiles that hold a dyad i < j; the host's list: ic_tiles, capi_samples.hpp).
// Lane = column, wavefront + 4 k = row: IcPlan<D>::DPT dyads per thread.  Per sample the tile's two position
// blocks (directed: two radii blocks as well) and the intercepts are staged in LDS, double buffered: sample s + 1
// is loaded into registers before the arithmetic of sample s and stored to the other buffer after it, one barrier
// per sample.  A kernel's loops over its tiles and the samples read
//
//     for q:  i0, j0 of tiles[q];  dyad_tile_bits (with a network);  its accumulators = identities
//             dyad_stage_first(stage[0], ...);  barrier
//             for s:  if (s + 1 < S) dyad_stage_prefetch(pre, ..., s + 1, ...)
//                     col = dyad_column(stage[s & 1], lane)
//                     for k:  eta = dyad_eta(stage[s & 1], 4 k + wv, col)  or  conv_eta(...);  its arithmetic
//                     if (s + 1 < S) dyad_stage_commit(stage[(s & 1) ^ 1], pre);  barrier
//             its results of the tile;  a barrier before stage[0] is written again
//
// The loops, the accumulators and the barriers are the kernel's own: what happens between the arithmetic and the
// barrier differs (a wave sum and a workgroup partial per sample; segment and batch boundaries; nothing).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"

namespace dlsm {

constexpr int IC_TJ = 64;                   // columns of a tile: one per lane
constexpr int IC_NT = 256;                  // threads of a workgroup
// dyads per thread: 4 accumulators each (8 registers) next to D coordinates of the column
template <int D> struct IcPlan { static constexpr int DPT = D <= 4 ? 8 : 4, TI = 4 * DPT; };

// doubles staged per sample: rows' positions, columns' positions, rows' radii, columns' radii, intercepts
template <int D, bool DIR> struct IcStage {
    static constexpr int TI = IcPlan<D>::TI;
    static constexpr int XI = 0, XJ = TI * D, RI = XJ + IC_TJ * D, RJ = RI + (DIR ? TI : 0),
                         B = RJ + (DIR ? IC_TJ : 0), N = B + 2;
    static constexpr int PER_THREAD = (N + IC_NT - 1) / IC_NT;
};

// element e of the staging block of one sample (X [N][D] of its time step, ic [2], rad [N]) for the tile
// of rows i0.., columns j0..; rows and columns beyond N read as position 0 and radius 1 (their dyads are
// masked out), e >= IcStage::N as 0
template <int D, bool DIR>
__device__ __forceinline__ double ic_stage_load(const double *__restrict__ X, const double *__restrict__ ic,
                                                const double *__restrict__ rad, int N, int i0, int j0, int e) {
    typedef IcStage<D, DIR> St;
    if (e < St::XJ) return (i0 * D + e < N * D) ? X[(size_t)i0 * D + e] : 0.0;
    if (e < St::RI) { e -= St::XJ; return (j0 * D + e < N * D) ? X[(size_t)j0 * D + e] : 0.0; }
    if (DIR && e < St::RJ) { e -= St::RI; return (i0 + e < N) ? rad[i0 + e] : 1.0; }
    if (DIR && e < St::B) { e -= St::RJ; return (j0 + e < N) ? rad[j0 + e] : 1.0; }
    if (e < St::N) return ic[e - St::B];
    return 0.0;
}

// The tile's dyads of this thread (rows i0 + 4 k + wv, column j) at time step t: bit k of valid - the dyad exists
// and, with mask [T][N][W] != NULL, its bit there is clear (undirected: that of (j, i) as well) -, bit k of ybits
// - its bit of the network bits [T][N][W].  (k_conv_accumulate reads no network and forms valid itself.)
template <int D, bool DIR>
__device__ __forceinline__ void dyad_tile_bits(const uint32_t *bits, const uint32_t *mask, int t, int N, int W,
                                               int i0, int j, int wv, uint32_t &valid, uint32_t &ybits) {
    valid = 0; ybits = 0;
#pragma unroll
    for (int k = 0; k < IcPlan<D>::DPT; ++k) {
        const int i = i0 + 4 * k + wv;
        bool ok = i < N && j < N && (DIR ? i != j : i < j);
        if (ok && mask) {
            uint32_t mb = mask[((size_t)t * N + i) * W + (j >> 5)] >> (j & 31);
            if (!DIR) mb |= mask[((size_t)t * N + j) * W + (i >> 5)] >> (i & 31);
            ok = !(mb & 1u);
        }
        if (ok) {
            valid |= 1u << k;
            ybits |= ((bits[((size_t)t * N + i) * W + (j >> 5)] >> (j & 31)) & 1u) << k;
        }
    }
}

// sample 0 of time step t (Xs [S][T][N][D], ic [S][2], radii [S][N]) into the stage buffer stage0
template <int D, bool DIR>
__device__ __forceinline__ void dyad_stage_first(double *stage0, const double *Xs,
                                                 const double *ic, const double *radii,
                                                 int t, int N, int i0, int j0, int tid) {
    typedef IcStage<D, DIR> St;
    const double *X0 = Xs + (size_t)t * N * D;
#pragma unroll
    for (int p = 0; p < St::PER_THREAD; ++p) {
        const int e = tid + p * IC_NT;
        if (e < St::N) stage0[e] = ic_stage_load<D, DIR>(X0, ic, radii, N, i0, j0, e);
    }
}

// this thread's elements of sample sn's block into pre [IcStage::PER_THREAD]: in flight under the arithmetic of the
// sample before
template <int D, bool DIR>
__device__ __forceinline__ void dyad_stage_prefetch(double *pre, const double *Xs,
                                                    const double *ic, const double *radii,
                                                    int sn, int T, int t, int N, int i0, int j0, int tid) {
    const double *Xn = Xs + ((size_t)sn * T + t) * N * D;
    const double *icn = ic + 2 * (size_t)sn;
    const double *rn = DIR ? radii + (size_t)sn * N : nullptr;
#pragma unroll
    for (int p = 0; p < IcStage<D, DIR>::PER_THREAD; ++p)
        pre[p] = ic_stage_load<D, DIR>(Xn, icn, rn, N, i0, j0, tid + p * IC_NT);
}

// pre into the stage buffer that the next sample is read from (the caller's barrier follows)
template <int D, bool DIR>
__device__ __forceinline__ void dyad_stage_commit(double *stage_next, const double *pre, int tid) {
    typedef IcStage<D, DIR> St;
#pragma unroll
    for (int p = 0; p < St::PER_THREAD; ++p) {
        const int e = tid + p * IC_NT;
        if (e < St::N) stage_next[e] = pre[p];
    }
}

// what a lane's dyads of one sample share: its column's position and radius (undirected: 1), the intercepts
template <int D> struct DyadColumn { double xj[D], b0, b1, rj; };

template <int D, bool DIR>
__device__ __forceinline__ DyadColumn<D> dyad_column(const double *sb, int lane) {
    typedef IcStage<D, DIR> St;
    DyadColumn<D> c;
#pragma unroll
    for (int d = 0; d < D; ++d) c.xj[d] = sb[St::XJ + lane * D + d];
    c.b0 = sb[St::B]; c.b1 = sb[St::B + 1];
    c.rj = DIR ? sb[St::RJ + lane] : 1.0;
    return c;
}

// eta of the dyad (row of the tile, the lane's column) from the stage buffer sb, as k_gof_draw (kernels_gof.hpp);
// the compiler contracts the sum of squares into fused multiply-adds.  The arithmetic is its correctly rounded
// sqrt and division: the outputs are compared with numpy at a few ulp, which the engine's lean sqrt (35 ulp on a
// distance, device_common.hpp) does not give.
template <int D, bool DIR>
__device__ __forceinline__ double dyad_eta(const double *sb, int row, const DyadColumn<D> &c) {
    typedef IcStage<D, DIR> St;
    double s2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double df = sb[St::XI + row * D + d] - c.xj[d];
        s2 += df * df;
    }
    const double dist = sqrt(s2);
    return DIR ? c.b0 * (1.0 - dist / c.rj) + c.b1 * (1.0 - dist / sb[St::RI + row]) : c.b0 - dist;
}

// The same eta, every operation rounded on its own (no fused multiply-add): bit for bit what float64 numpy
// gives for the definition.  Not to be merged with dyad_eta: where a segment's variance is small against the
// predictor, k_conv_accumulate's rhat amplifies a last-bit difference in eta by |eta| / |eta_s - eta_s'|;
// measured at h = 2, a fused sum of squares moved an rhat of 33 by 250 ulp.
template <int D, bool DIR>
__device__ __forceinline__ double conv_eta(const double *xi, const double (&xj)[D], double b0, double b1, double rj,
                                           double ri) {
#pragma clang fp contract(off)
    double s2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double df = xi[d] - xj[d];
        s2 = s2 + df * df;
    }
    const double dist = sqrt(s2);
    if (DIR) {
        const double in = b0 * (1.0 - dist / rj), out = b1 * (1.0 - dist / ri);
        return in + out;
    }
    return b0 - dist;
}

}  // namespace dlsm
