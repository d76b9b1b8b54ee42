// The parts of the pipelined sweep's LDS evaluators (kernels_pipe_lds.hpp) as trip lists: plain C++ shared by the
// host (capi.hip fills PipeLds::plan with pipe_plan_entry), the device (PipePlan::trip) and a GPU-free test of the
// partition (tests/test_pipe_plan_cpu.py compiles this header with g++).
#pragma once
#include <stdint.h>
#include <stddef.h>
#ifdef __HIPCC__
#define DLSM_PLAN_HD __host__ __device__
#else
#define DLSM_PLAN_HD
#endif

namespace dlsm {

constexpr int PL_EXPTAB_DOUBLES = 2048;     // = EXPTAB11_N (device_common.hpp): the evaluators' exp table in front of the rows

constexpr int PL_WIN = 4;           // window trips a part can hold (P = 1: all four)

// trips (and LDS rows) the longest part can hold
DLSM_PLAN_HD inline int pipe_lds_trip_cap(int ntrip, int parts) { return (ntrip + parts - 1) / parts + PL_WIN; }
// bytes of dynamic LDS the evaluators need: exp table, the longest part's rows, its window trips' proposals
DLSM_PLAN_HD inline size_t pipe_lds_eval_bytes(int N, int D, int parts) {
    const int ntrip = (N + 63) / 64;
    return ((size_t)PL_EXPTAB_DOUBLES + (size_t)(pipe_lds_trip_cap(ntrip, parts) + PL_WIN) * 64 * D) * sizeof(double);
}

// The trips of a node of batch `be` (its workgroup's first node k0) as P parts.  Window trips: [glo, glo + nwin)
// = the previous batch's two (be > 0), trip 2 be of the own batch, and trip 2 be + 1 when the workgroup's nodes
// reach into it (k0 >= 64); window trip i goes to part i mod P and is the part's trip i / P.  The other ntrip -
// nwin trips, in ascending order, are cut into runs r_0 .. r_{P-1} with r_j + 2 w_j as equal as integers allow.
// (w, r, s) depend on (nwin, p) only: the host computes the 4 P triples once (pipe_plan_entry) and the launch
// carries them as kernel arguments (PipeBuf::plan) - the evaluators' row requests wait for nothing but a decode.
struct PipePlan {
    int glo, nwin;      // the window's trips
    int w, r, s;        // this part: window trips, other trips, rank of its first other trip
    DLSM_PLAN_HD inline int trips() const { return w + r; }
    DLSM_PLAN_HD inline int trip(int u, int p, int P) const {      // the part's u-th trip
        if (u < w) return glo + p + P * u;
        const int rho = s + (u - w);
        return rho < glo ? rho : rho + nwin;
    }
};
// w | r << 3 | s << 16 of part p when the window holds nwin trips (1 .. 4) of ntrip
inline uint32_t pipe_plan_entry(int ntrip, int P, int nwin, int p) {
    auto wof = [&](int j) { return j < nwin ? (nwin - j + P - 1) / P : 0; };
    const int R = ntrip - nwin, S = R + 2 * nwin;
    const int q = S / P, rem = S % P;
    const bool balanced = R >= 0 && q >= 2 * wof(0);             // (tiny N: plain runs of the other trips)
    const int Rp = R > 0 ? R : 0;
    int s = 0, w = 0, r = 0;
    for (int j = 0; j <= p; ++j) {
        const int wj = wof(j);
        const int rj = balanced ? q + (j < rem ? 1 : 0) - 2 * wj : Rp / P + (j < Rp % P ? 1 : 0);
        if (j < p) s += rj; else { w = wj; r = rj; }
    }
    return (uint32_t)w | ((uint32_t)r << 3) | ((uint32_t)s << 16);
}
// the window of a workgroup whose first node is k0 of batch be, and its part p's (w, r, s) from a plan entry
DLSM_PLAN_HD inline PipePlan pipe_plan_from_entry(uint32_t e, int ntrip, int be, int k0) {
    PipePlan pl;
    pl.glo = be > 0 ? 2 * be - 2 : 0;
    const int ghi0 = 2 * be + (k0 >= 64 ? 1 : 0);
    const int ghi = ghi0 < ntrip - 1 ? ghi0 : ntrip - 1;
    pl.nwin = ghi - pl.glo + 1;                                  // 1 .. 4 (trip 2 be exists: the batch has nodes)
    pl.w = (int)(e & 7u); pl.r = (int)((e >> 3) & 0x1fffu); pl.s = (int)(e >> 16);
    return pl;
}

// ---- the deal: which (active slice, part, node) a wavefront of an evaluator workgroup takes -----------------------
// Evaluator workgroup e of a launch holds q = 2^qs consecutive nodes of one active slice and part, one per wavefront
// (its first q wavefronts; all sixteen stage the part's rows): e = (p nsl + si) (PL_B / q) + node group.  q = 16
// fills the workgroup; q = 8 spreads a launch that has few items over twice the workgroups, so that a SIMD issues
// two items instead of four.
constexpr int PL_B = 128;           // = PP_B: nodes per batch, node slots per (slice, part)
constexpr int PL_WAVES = 16;        // = PP_WAVES: wavefronts per evaluator workgroup

// the evaluator workgroups of a launch on n_cu compute units beside its T resolvers, and the parts of a node: as
// many as fill those workgroups' wavefronts (at most 8: PipeLds::plan) - for the undirected model in ONE round of
// items, a part less when rounding up would leave items for a second round
inline int pipe_eval_workgroups(int n_cu, int T) { return n_cu / 2 > n_cu - T ? n_cu / 2 : n_cu - T; }
inline int pipe_parts(int ne_wg, int T, bool one_round) {
    int parts = (int)((double)ne_wg * PL_WAVES / ((double)T * PL_B) + 0.5);
    parts = parts < 1 ? 1 : parts > 8 ? 8 : parts;
    if (one_round && parts > 1 && (long)parts * T * PL_B > (long)ne_wg * PL_WAVES) --parts;
    return parts;
}
inline int pipe_parts_undirected(int ne_wg, int T) { return pipe_parts(ne_wg, T, true); }

// launch l resolves batch l of the even slices and batch l - 1 of the odd ones (kernels_spec_pipe.hpp)
DLSM_PLAN_HD inline bool pipe_launch_resolves(int T, int nbat, int l) {
    return (l >= 0 && l < nbat) || (T > 1 && l >= 1 && l - 1 < nbat);
}
// ... and evaluates batch l + 1 of the even slices and batch l of the odd ones: its active slices
DLSM_PLAN_HD inline int pipe_launch_slices(int T, int nbat, int l) {
    const int nE = (T + 1) / 2, nO = T / 2;
    return (l + 1 >= 0 && l + 1 < nbat ? nE : 0) + (l >= 0 && l < nbat ? nO : 0);
}
// log2 of the nodes per evaluator workgroup of launch l: 3 (q = 8) when the launch's items, eight to a workgroup,
// still fit its ne_wg evaluator workgroups and no resolver of the launch has a batch to resolve - a launch that
// carries resolvers is as long as they are, and halving its evaluators' trips buys nothing; 4 (q = 16) otherwise
DLSM_PLAN_HD inline int pipe_launch_qshift(int T, int nbat, int parts, int ne_wg, int l, bool spread) {
    if (!spread || pipe_launch_resolves(T, nbat, l)) return 4;
    const long wgs8 = (long)parts * pipe_launch_slices(T, nbat, l) * (PL_B / 8);
    return wgs8 > 0 && wgs8 <= (long)ne_wg ? 3 : 4;
}
// evaluator workgroup e: its node group's first node k0, its live wavefronts, and r = p nsl + si
struct PipeDeal { int k0, nlive, r; };
DLSM_PLAN_HD inline PipeDeal pipe_deal(int e, int qs) {
    PipeDeal d;
    d.k0 = (e & ((PL_B >> qs) - 1)) << qs;
    d.nlive = 1 << qs;
    d.r = e >> (7 - qs);
    return d;
}
static_assert(PL_B == 1 << 7, "pipe_deal: node groups by shifts");
// r / nsl as a multiplication (r < 2^16 / nsl): the magic number the host computes, and the quotient
inline uint32_t pipe_deal_magic(int nsl) { return (65536u + (uint32_t)nsl - 1u) / (uint32_t)nsl; }
DLSM_PLAN_HD inline int pipe_deal_part(int r, uint32_t nsl_magic) { return (int)(((uint32_t)r * nsl_magic) >> 16); }

}  // namespace dlsm
