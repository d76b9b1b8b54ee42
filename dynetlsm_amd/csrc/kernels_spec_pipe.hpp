// Pipelined speculative sweep (algo 4): the speculative-batch scan of
// kernels_spec_sweep.hpp with the evaluation of batch b + 1 moved off the
// critical path.
//
// In the two-kernel form eval(b + 1) reads the positions resolve(b) has just
// written, so the launches alternate strictly.  Two facts remove that edge:
//   * a node moves at most once per parity, so "the position of node i before its
//     own step" is its position at the start of the parity: a snapshot taken by the
//     propose kernel is valid for every node that is not resolved yet, however far
//     the resolver has got;
//   * the effect of batch b's acceptances on node k of batch b + 1 is the same
//     H[k][m] correction that already couples the nodes inside a batch.
// So eval(b + 1) uses X for nodes of batches < b (final), the snapshot for all
// others, and emits the cross block Hx[k][m], m in batch b, next to its own diagonal
// block; resolve(b + 1) adds the Hx rows of the nodes batch b accepted.  eval(b + 1)
// then depends on resolve(b - 1) only, and ONE launch carries both roles:
//
//     launch b:  workgroups [0, nsl)   resolve batch b of their slice
//                workgroups [nsl, ..)  evaluate batch b + 1 (one item per wavefront)
//
// No workgroup of a launch reads what another one of the same launch writes; the
// kernel boundary is the only synchronisation.  Algebraically this is still the
// sequential Gauss-Seidel scan (differences are rounding only).
//
// Both parities run in the same launches.  Slices of different parity interact only
// through the prior term of node (t, j), which looks at X[t +- 1][j]; if the odd
// slices run ONE BATCH BEHIND the even ones, an even node of batch l still sees the
// odd slices' node j untouched, and an odd node of batch l - 1 sees the even slices'
// node j final - exactly the even-then-odd order of the reference.  Launch l
// therefore resolves batch l of the even slices and batch l - 1 of the odd ones and
// evaluates batches l + 1 / l; the prior delta is computed by the resolver.
//
// The accept test runs in the multiplicative domain, u_k < exp(r_k) * prod_m H[k][m]:
// the evaluators hand over products of (1 + E e^{-d}) factors as they accumulate
// them, so a wavefront spends one division where the additive form needs a
// float64 log per node part and per H entry (each executed by all 64 lanes); the
// resolver pays one exp per node instead.  (A node whose log-ratio is beyond +-700 - exp would
// saturate - is resolved in the log domain, with the logs of its H factors.)
#pragma once
#include "kernels_spec_sweep.hpp"
#include "kernel_stamps.hpp"

namespace dlsm {

// A wavefront's issue priority falls as its item advances (s_setprio 3 for the first quarter of the
// prefetched trips .. 0 for the last).  The arbiter serves a SIMD's ready wavefronts oldest first: its four
// items ran nearly one after the other (first trip done after 0.7 / 1.4 / 3.0 / 4.5 us, exit after 3.8 / 5.3 /
// 7.1 / 8.6: profiles/r04_h_entry_ablation.md), and the youngest ran its tail alone, with nobody to fill the
// slots its dependent float64 instructions leave.  With the priority tied to progress the four advance
// together and end together: k_pipe_step 10.53 -> 10.08 us per launch, C2 4300 -> 4470 it/s (boundaries at
// the quarters or one trip later: the same; two levels instead of four: half the gain); with priority 3 from
// the item's FIRST instruction (pipe_item_prologue: a wavefront that enters late gets its loads out at once)
// 9.90 us, 4570 it/s.  (The table's fill + barrier moved behind the item's operand requests, so that the two
// round trips overlap: 10.65 us - the barrier then holds all sixteen wavefronts until the last one's operands
// have arrived; dropped.)
#define DLSM_TRIP_PRIO_STEP(U_)                                                                \
        if ((U_) == 0) __builtin_amdgcn_s_setprio(3);                                          \
        else if ((U_) == (PP_NPRE * 1) / 4) __builtin_amdgcn_s_setprio(2);                     \
        else if ((U_) == (PP_NPRE * 2) / 4) __builtin_amdgcn_s_setprio(1);                     \
        else if ((U_) == (PP_NPRE * 3) / 4) __builtin_amdgcn_s_setprio(0);
constexpr int PP_THREADS = 1024;
constexpr int PP_WAVES = PP_THREADS / 64;
constexpr int PP_B = 128;               // nodes per batch (two 64-lane halves)
constexpr int PP_MAXPARTS = 8;          // (PipeLds::plan holds 8 parts)
// per (slice, batch slot) of PipeBuf::acc: [0] count, [1 .. PP_B] the accepted nodes ascending (the [m][k]
// resolver's gather list), [PP_ACC_MASK ..] the same set as two 64-bit masks (the row resolver's)
constexpr int PP_ACC = PP_B + 8;
constexpr int PP_ACC_MASK = PP_B + 4;

// What an evaluator of kernels_pipe_lds.hpp reads of the launch's arguments, in ONE piece at the head of PipeBuf's
// tail: its first 128 bytes are requested together by the wavefront's first instructions (the compiler fetches a
// kernel argument where it is first used - a dozen scalar loads, each with a wait of its own, in a prologue that
// the four wavefronts of a SIMD issue one after the other).
struct PipeLds {
    const double *X; const uint32_t *ybits; double *prop; double *full0; double *H; int32_t *acc; double *consts;
    double *xprod;
    int T, N, W, squared, parts, nbat, lds_cap, flags;      // (flags: PP_F_*, per launch)
    // per launch: the batch evaluated / its nodes / the active slices (even and odd slices); evaluator workgroup e
    // (blockIdx.x - T) holds q = 16 or 8 consecutive nodes (e mod 128 / q) of active slice si and part p,
    // e / (128 / q) = p nsl + si (pipe_plan.hpp, pipe_deal) with
    // the quotient as a multiplication: r / nsl = r nsl_magic >> 16 (nsl_magic = ceil(2^16 / nsl), r < 2^16 / nsl)
    int beE, beO, nbE, nbO, nslE, nslO, xstride; uint32_t nsl_magic;
    uint32_t plan[4][8];        // the parts' trip lists (pipe_plan_entry), by (window trips - 1, part)
};
static_assert(sizeof(PipeLds) == 256, "PipeLds: two 64-byte halves of scalars and the plan table");
// The launch's switches, one word for both roles (PipeLds::flags for the evaluators, PipeBuf::flags for the resolvers):
//   PP_F_XSERVE  the evaluators multiply the resolvers' cross products (pipe_xserve_*)
//   PP_F_WT      what the launch hands to a later one - H rows, item records, accepted positions, the samplers'
//                bookkeeping, the acceptance masks - is stored write-through (sc1): the readers are on other XCDs
//                and read from memory either way, and the end-of-kernel release finds nothing dirty to write back
//                (2 MB per launch as plain stores)
//   PP_F_SPREAD  8 nodes per evaluator workgroup instead of 16 (pipe_plan.hpp, pipe_launch_qshift)
constexpr int PP_F_XSERVE = 1, PP_F_WT = 2, PP_F_SPREAD = 4;
// a hand-off store of the sweep: write-through when the launch says so
__device__ __forceinline__ void pipe_store(bool wt, double *p, double v) {
    if (wt) coh_store<true>(p, v); else coh_store<false>(p, v);
}
__device__ __forceinline__ void pipe_store2(bool wt, void *base, uint32_t off, double2 v) {
    if (wt) coh_store2<true>(base, off, v); else coh_store2<false>(base, off, v);
}
__device__ __forceinline__ void pipe_store_i32(bool wt, int32_t *p, int32_t v) {
    if (wt) coh_store_i32(p, v); else *p = v;
}

// One batch is resolved (and the next one evaluated) per launch.  Batch b is evaluated while batch b - 1 is still
// unresolved - its WINDOW: the previous batch, if any - and everything produced per batch lives in slot b & 1.
//
// The H factors of a (slot, slice) - exp(H[k][m]): what node m's acceptance does to the ratio of a later node k -
// are PP_H_SLICE doubles of PipeBuf::H, filed in one of two forms:
//   rows   (the exact-likelihood models; written by pipe_h_entry and pipe_lds_trips, read by row_resolve and
//          pipe_xserve_request): [2][T][PP_B][window PP_B | own PP_B], one row of PP_H_ROW factors per later node
//          k - those of its window's nodes, then those of the earlier nodes of its own batch
//   dense case-control (written by pipe_cc_writeout, read by pipe_resolve_ccdense): blocks indexed [m][k], the
//          diagonal ones (m and k > m in the batch) as [2][T][PP_B][PP_B] at H, the cross ones (m in the window)
//          as [2][T][PP_B][PP_B] behind them, at H + pipe_h_cc_cross(T)
constexpr int PP_H_ROW = 2 * PP_B;
constexpr int PP_H_SLICE = PP_B * PP_H_ROW;
__host__ __device__ constexpr size_t pipe_h_doubles(int T) { return (size_t)2 * T * PP_H_SLICE; }
// dense case-control form: the cross blocks start behind the [2][T] diagonal blocks
__host__ __device__ constexpr size_t pipe_h_cc_cross(int T) { return (size_t)2 * T * PP_B * PP_B; }
static_assert(2 * PP_B * PP_B == PP_H_SLICE, "a diagonal and a cross block fill the (slot, slice)'s share of H");
struct PipeBuf {
    double *prop;    // [T][N][2D + 2] : x1[D], u, (unused), x0[D] (snapshot)
    double *full0;   // [2][T][PP_B][parts][2] : (sum of linear terms, ratio of products)
    double *H;       // pipe_h_doubles(T) : the H factors, by rows or as dense case-control blocks (above)
    LsmDeviceState *lsm_draw;   // not NULL: the proposal pass also draws the intercept proposal
                     // (the fourth pointer: the fields behind it keep their 16-byte alignment in the kernel's argument
                     // block.  8 bytes earlier the compiler groups their scalar loads differently, and the directed
                     // evaluator, at the SGPR limit, came out 60 instructions longer: profiles/pipe_one_batch_refactor.md)
    int32_t *acc;    // [T][2][PP_ACC] : count, accepted nodes of the batch in that slot, their masks
    double *consts;  // [2] : E = exp(sum of intercepts), flush interval
    const int32_t *nctrl;   // case-control: valid controls per (t, i, direction)
    int parts, per, nbat;
    PipeLds lds;     // kernels_pipe_lds.hpp: the evaluators' arguments (filled by the host per launch)
    // the cross products by the evaluators (kernels_pipe_lds.hpp, pipe_xserve): slot [t][k] holds PP_XP_EMPTY
    // until the wavefront that serves row k of slice t has stored prod_{m accepted} Hx[k][m]; the row's owner in
    // the resolver workgroup polls it past its L1 and empties it again
    double *xprod; int32_t *err; int flags, budget;     // (flags: PP_F_*, per launch)
    int lds_eval;    // undirected model: the evaluators of kernels_pipe_lds.hpp (rows staged in LDS, interleaved
                     // parts, H factors inside the trips); 0: pipe_eval_item
};
// (the argument loads of the evaluators keep their grouping only while the fields behind lsm_draw stay where they are)
static_assert(offsetof(PipeBuf, acc) % 16 == 0 && offsetof(PipeBuf, lds) % 16 == 8, "PipeBuf: see lsm_draw");
constexpr unsigned long long PP_XP_EMPTY = 0x7FF8C0DE5EED0002ull;     // a NaN payload no arithmetic produces
constexpr int PP_ERR_XSERVE = 1 << 29;          // sticky error word: a resolver ran out of its poll budget
// the window of batch b starts with the batch before it, if any
__host__ __device__ __forceinline__ int pipe_window_start(int b) { return b > 0 ? b - 1 : 0; }

// The proposal pass of a sweep, as pieces: it runs as its own launch (k_pipe_propose) or, inside
// the device-resident loops, as extra workgroups of the previous iteration's last launch
// (kernels_tail_propose.hpp) - everything it reads is final by then.
__device__ __forceinline__ void pipe_propose_consts(const ChainView &c, double *consts,
                                                    const double *intercept) {
    const double E = c.model == DLSM_UNDIRECTED ? exp(intercept[0]) : exp(intercept[0] + intercept[1]);
    consts[0] = E;
    consts[1] = (double)flush_interval(E);
}

// The undirected loop's intercept proposal and the log-uniform of its accept test
// (sample_coefficients.py:76-86; Philox stream INTERCEPT, counters (0, 0 | 1, iter)) - what the
// centring pass draws (k_post_apply), from the same counters and the same intercept and step size,
// which are settled when the previous iteration ends: drawn with the sweep's proposals, the
// likelihood pass can run before the centring pass (kernels_tail_propose.hpp).
__device__ __forceinline__ void pipe_propose_intercept(const ChainView &c, LsmDeviceState *lsm,
                                                       const double *intercept, uint32_t iter) {
    double u0, u1, z0, z1;
    philox_uniform2(c.seed, 0, 0, iter, stream_word(c.chain, STREAM_INTERCEPT), u0, u1);
    box_muller(u0, u1, z0, z1);
    const double b0 = intercept[0];
    lsm->cand[0] = b0;
    lsm->cand[1] = b0 + lsm->i_step[0] * z0;
    philox_uniform2(c.seed, 0, 1, iter, stream_word(c.chain, STREAM_INTERCEPT), u0, u1);
    lsm->logu = log(u0);
}

// the proposal of node (t, j) from its position x0
template <int D>
__device__ __forceinline__ void pipe_propose_row_from(const ChainView &c, const ProposeBuf &pb, uint32_t iter,
                                                      int t, int j, const double (&x0)[D]) {
    const int N = c.N;
    double x1[D], logu;
    make_proposal<D>(c, iter, t, j, x0, c.step[(size_t)t * N + j], x1, logu);
    double *pr = pb.prop + ((size_t)t * N + j) * (2 * D + 2);
#pragma unroll
    for (int d = 0; d < D; ++d) pr[d] = x1[d];
    {   // the uniform itself (same draw as make_proposal's log u)
        double u0, u1;
        philox_uniform2(c.seed, (uint32_t)j, (uint32_t)t, iter,
                        stream_word(c.chain, STREAM_SWEEP_UNIFORM), u0, u1);
        pr[D] = u0;
    }
    pr[D + 1] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) pr[D + 2 + d] = x0[d];     // the snapshot, in the row's order
}

// workgroup `fb` of ceil(N / 256) T, 256 threads
template <int D>
__device__ __forceinline__ void pipe_propose_rows(const ChainView &c, const ProposeBuf &pb, uint32_t iter,
                                                  int fb, int tid) {
    const int N = c.N, nbx = (N + 255) / 256;
    const int t = fb / nbx;
    const int j = (fb - t * nbx) * 256 + tid;
    if (j >= N) return;
    // valid for the whole sweep: X[t, j] and its step size change only at step (t, j)
    double x0[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x0[d] = c.X[((size_t)t * N + j) * D + d];
    pipe_propose_row_from<D>(c, pb, iter, t, j, x0);
}

template <int D>
__global__ __launch_bounds__(256) void k_pipe_propose(ChainView c, PipeBuf pb, IterRef ir) {
    const int fb = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    if (fb == 0 && threadIdx.x == 0) {
        pipe_propose_consts(c, pb.consts, c.intercept);
        if (pb.lsm_draw) pipe_propose_intercept(c, pb.lsm_draw, c.intercept, ir.get());
    }
    const ProposeBuf nb{pb.prop, pb.consts, pb.lsm_draw};
    pipe_propose_rows<D>(c, nb, ir.get(), fb, (int)threadIdx.x);
}

// (phase stamps of every evaluator wavefront - PIPE_ITEM_T - and every resolver workgroup - PIPE_RES_T - of the last
// sweep: kernel_stamps.hpp; profiles/pipe_timing.py reads them)

// ---- the item's wavefront reductions -------------------------------------------------------
// An evaluator launch is bound by float64 VALU issue (profiles/pipe_timing.py: the four
// wavefronts of a SIMD run one after the other, the SIMD is busy from the first operand's
// arrival to the launch's end), so what is not a neighbour term is overhead to be counted in
// instructions.  Only lane 0 stores the record: the sum and the two products are reduced
// towards it, the two products share one tree from the second step on (even lanes carry P0, odd lanes
// P1: quad_perm xor 2 and the row rotations keep the parity), and the rows are combined
// through the LDS crossbar (ds_bpermute: no VALU cycles) instead of v_readlane.
__device__ __forceinline__ double lane_get(double v, int byte_addr) {      // 4 * source lane
    return __hiloint2double(__builtin_amdgcn_ds_bpermute(byte_addr, __double2hiint(v)),
                            __builtin_amdgcn_ds_bpermute(byte_addr, __double2loint(v)));
}
// lane 0: sum = sum over the wavefront of s, ratio = prod a / prod b
__device__ __forceinline__ void pipe_reduce(double s, double a, double b, int lane, double &sum,
                                            double &ratio) {
    const int x16 = (lane ^ 16) << 2, x32 = (lane ^ 32) << 2;
    s += dpp_move<0xB1>(s);         // quad_perm [1, 0, 3, 2]
    a *= dpp_move<0xB1>(a);
    b *= dpp_move<0xB1>(b);
    double q = (lane & 1) ? b : a;
    s += dpp_move<0x4E>(s);         // quad_perm [2, 3, 0, 1]
    q *= dpp_move<0x4E>(q);
    s += dpp_move<0x124>(s);        // row_ror:4
    q *= dpp_move<0x124>(q);
    s += dpp_move<0x128>(s);        // row_ror:8
    q *= dpp_move<0x128>(q);
    s += lane_get(s, x16);
    q *= lane_get(q, x16);
    s += lane_get(s, x32);
    q *= lane_get(q, x32);
    sum = s;
    // lane 0: prod a / prod b (products of factors >= 1 that the caller keeps inside the double
    // range: the reciprocal's Newton form, within 2 ulp of the division at a fifth of it)
    ratio = q * fast_rcp(dpp_move<0xB1>(q));
}

#include "kernels_pipe_item.hpp"
#include "kernels_pipe_ccdense.hpp"

// ---- the resolver for H blocks stored BY ROWS (every launch of the exact-likelihood models) ----------------------
// The evaluators file the factors of later node kk as ONE row [window (PP_B) | own batch (PP_B)]: a wavefront's
// 64 entries - consecutive entries of one row in the flat list of pipe_h_decode - are 512 contiguous bytes
// instead of 64 stores a kilobyte apart (the [m][k] blocks: 2.15 MB written and 7.9 MB fetched per launch, each
// 128-byte line assembled from 16 wavefronts on eight XCDs).
constexpr int PR_LD = PP_B + 1;          // LDS row stride of the diagonal block (doubles)

// the product (or, for a node resolved in the log domain, the sum) over the 8 adjacent lanes
// that share a node: quad_perm xor 1, xor 2, then the half-row mirror
__device__ __forceinline__ double group8_prod(double v) {
    v *= dpp_move<0xB1>(v);
    v *= dpp_move<0x4E>(v);
    v *= dpp_move<0x141>(v);
    return v;
}
__device__ __forceinline__ double group8_sum(double v) {
    v += dpp_move<0xB1>(v);
    v += dpp_move<0x4E>(v);
    v += dpp_move<0x141>(v);
    return v;
}

template <int D>
__device__ __forceinline__ void row_resolve(const ChainView &c, const PipeBuf &pb, int b, int t,
                                                double *sD, double *sPart,
                                                unsigned long long (*sMask)[2],
                                                double *sCross,
                                                unsigned long long *sSatMask, double *sTab, bool served,
                                                Stamps<PIPE_RES_T> rst) {
    constexpr int PW = 2 * D + 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    DLSM_STAMP(rst, 0, (double)tid)
    const int N = c.N;
    const int j0 = b * PP_B;
    const int nb = min(PP_B, N - j0);
    const int bb = b & 1;
    const int half = wave & 1, part = wave >> 1;
    const int k = 64 * half + lane;
    const bool owner = wave < 2;
    const bool valid = k < nb;
    const double *H = pb.H + ((size_t)bb * c.T + t) * PP_H_SLICE;
    // ---- every load of the batch, at once ------------------------------------------------------
    // cross factors: node kx = tid / 8; trip u: window nodes 16 u + 2 jx, + 1 - the 8 lanes of a
    // node read one 128-byte line per trip
    const int kx = tid >> 3, jx = tid & 7;
    double cr[16];
    const uint32_t cr_off = (uint32_t)((kx * (2 * PP_B) + 2 * jx) * sizeof(double));
    // (served: the launch's evaluators multiply the accepted factors of every row and hand over one number per
    // node - the 128 KB of the cross block were 1.8 us of this workgroup's 4.1 us until its blocks were in LDS)
    if (b > 0 && !served) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double2 v = coh_load2<false>(H, cr_off, (uint32_t)(16 * u * sizeof(double)));
            cr[2 * u] = v.x; cr[2 * u + 1] = v.y;
        }
    }
    // diagonal block: 16 bytes per thread and trip, a wavefront per row (rows >= nb and columns
    // >= the row's node were never written: never read either)
    // (trip u: row 16 u + wave, columns 2 lane, 2 lane + 1)
    // (d = 3, 4: the block in two halves - the owners' positions, proposals and prior operands are 8 d
    // registers more, and all of it at once spilled 3 - 35 registers: the second half is requested once
    // the first has left for LDS, one round trip later, on instantiations no benchmark configuration runs)
    constexpr int BLK_H = D <= 2 ? 8 : 4;
    double2 blk[BLK_H];
    const uint32_t blk_off = (uint32_t)((wave * (2 * PP_B) + PP_B + 2 * lane) * sizeof(double));
#pragma unroll
    for (int u = 0; u < BLK_H; ++u)
        blk[u] = coh_load2<false>(H, blk_off, (uint32_t)(u * PP_WAVES * (2 * PP_B) * sizeof(double)));
    // the owners' inputs (requested now, used once the blocks above have left their registers)
    double2 tv[4];
    double x1[D], x0[D], uk = 1.0, st = 0.0;
    int32_t na = 0, ns = 0, un = 0;
    NodePriorPre<D> npre;
    const int kc = min(k, nb - 1);
    const int p1 = pb.parts;
    const double2 *frec = (const double2 *)pb.full0 + ((size_t)bb * c.T + t) * PP_B * pb.parts;
#pragma unroll
    for (int d = 0; d < D; ++d) { x1[d] = 0.0; x0[d] = 0.0; }
#pragma unroll
    for (int u = 0; u < 4; ++u) tv[u] = make_double2(0.0, 1.0);
    auto owner_loads = [&]() {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            tv[u] = coh_load2<false>(frec, (uint32_t)((kc * p1 + min(u, p1 - 1)) * sizeof(double2)));
        const double *pr = pb.prop + ((size_t)t * N + j0 + kc) * PW;
#pragma unroll
        for (int d = 0; d < D; ++d) { x1[d] = pr[d]; x0[d] = pr[D + 2 + d]; }
        uk = pr[D];
        const size_t tjc = (size_t)t * N + j0 + kc;
        st = c.step[tjc]; na = c.nacc[tjc]; ns = c.nsteps[tjc]; un = c.until[tjc];
        npre.request1(c, t, j0 + kc);        // the prior terms' operands, with everything else
    };
    if (owner) owner_loads();
    // the owners' exponential table (tab_exp), requested with everything else: it is read behind the barrier
    // below (round 6: its own fill + barrier in front of this function kept every request of the batch
    // a memory round trip late - the resolver is the launch's critical path once the evaluators are shorter)
    double tabv = 0.0;
    if (tid < EXPTAB_N) tabv = c_exp2_tab[tid];
#pragma unroll
    for (int u = 0; u < BLK_H; ++u) {
        double *dst = sD + (u * PP_WAVES + wave) * PR_LD + 2 * lane;
        dst[0] = blk[u].x; dst[1] = blk[u].y;
    }
    if (BLK_H < 8) {
        __builtin_amdgcn_sched_barrier(0);              // (not hoisted among the loads above)
#pragma unroll
        for (int u = 0; u < 8 - BLK_H; ++u)
            blk[u] = coh_load2<false>(H, blk_off, (uint32_t)((BLK_H + u) * PP_WAVES * (2 * PP_B) * sizeof(double)));
#pragma unroll
        for (int u = 0; u < 8 - BLK_H; ++u) {
            double *dst = sD + ((BLK_H + u) * PP_WAVES + wave) * PR_LD + 2 * lane;
            dst[0] = blk[u].x; dst[1] = blk[u].y;
        }
    }
    if (owner) npre.request2(c);               // (the labels are in: the components' means and variances)
    // the window's accepted nodes among this thread's 16 factors: cr[2 u + i] belongs to node
    // 16 u + 2 jx + i -> bit 2 u + i of mp.  Multiplicative domain; a node that turns out to be
    // resolved in the log domain (below) redoes its part from memory.
    unsigned int mp = 0u;
    if (b > 0) {
        // the previous batch's acceptances (the launch before left them)
        const unsigned long long *pmg = (const unsigned long long *)(pb.acc + ((size_t)t * 2 + ((b - 1) & 1)) * PP_ACC +
                                                                     PP_ACC_MASK);
        const unsigned long long pm0 = pmg[0], pm1 = pmg[1];
        const unsigned long long mlo = pm0 >> (2 * jx), mhi = pm1 >> (2 * jx);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            mp |= ((unsigned int)((u < 4 ? mlo : mhi) >> (16 * (u & 3))) & 3u) << (2 * u);
        if (!served) {
            double prod = 1.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) prod *= (mp >> i) & 1u ? cr[i] : 1.0;
            const double v = group8_prod(prod);
            if (jx == 0) sCross[kx] = v;
        }
    }
    // multiplicative domain: r = exp(log-ratio of node k), lu = its uniform draw.  A node whose
    // log-ratio is beyond +-700 (exp would saturate) is resolved in the log domain instead
    // (as in pipe_resolve_ccdense)
    double r = 0.0, lu = 0.0, lr = 0.0;
    bool sat = false;
    if (owner) {
        double tot = tv[0].x, pr_ = tv[0].y;
#pragma unroll
        for (int u = 1; u < 4; ++u)
            if (u < p1) { tot += tv[u].x; pr_ *= tv[u].y; }
        for (int u = 4; u < p1; ++u) {                 // more than four parts (short slices, many CUs)
            const double2 w = coh_load2<false>(frec, (uint32_t)((kc * p1 + u) * sizeof(double2)));
            tot += w.x; pr_ *= w.y;
        }
        // prior terms of the step's logp closure, the neighbouring slices as they are now (the
        // odd slices wait for the even ones: header)
        const double prior = npre.value(x1) - npre.value(x0);
        const double ek = tot + prior;
        sat = !(fabs(ek) <= 700.0);
        // (r = exp(ek) pr_ behind the barrier: the table is in LDS by then)
        r = sat ? 1.0 : pr_;
        lr = ek;
        lu = uk;
        if (sat) { lr = ek + log(pr_); lu = log(lu); }
        const unsigned long long sm = __ballot(sat);
        if (lane == 0) sSatMask[half] = sm;
    }
    if (tid < EXPTAB_N) sTab[tid] = tabv;
    __syncthreads();                                   // sD, sCross, sSatMask, sTab visible
    // (the table exponential: the compiler's exp() keeps a dozen float64 constants alive through
    // the whole batch loop, in registers the blocks above need - it spilled them)
    if (owner && !sat) r *= tab_exp(lr, sTab);
    DLSM_STAMP(rst, 1, (double)tid)
    const unsigned long long sat0 = sSatMask[0], sat1 = sSatMask[1];
    const bool anysat = (sat0 | sat1) != 0ull;         // workgroup-uniform; practically never
    const bool satk = (((half ? sat1 : sat0) >> lane) & 1ull) != 0ull;
    if (anysat && b > 0) {
        // slow path: the log-domain nodes' cross terms as sums of logs
        const bool satx = ((((kx >> 6) ? sat1 : sat0) >> (kx & 63)) & 1ull) != 0ull;
        if (__ballot(satx) != 0ull) {
            double lsum = 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double2 v = coh_load2<false>(H, cr_off, (uint32_t)(16 * u * sizeof(double)));
                if (satx && ((mp >> (2 * u)) & 1u)) lsum += log(v.x);
                if (satx && ((mp >> (2 * u + 1)) & 1u)) lsum += log(v.y);
            }
            const double vs = group8_sum(lsum);
            if (satx && jx == 0) sCross[kx] = vs;
        }
        __syncthreads();
    }
    if (owner) {
        if (b > 0) {
            double vk;
            if (served && !sat) {
                // the product announces itself: the slot is PP_XP_EMPTY until the serving wavefront has stored it
                vk = 1.0;
                if (valid) {
                    const unsigned long long *slotp = (const unsigned long long *)&pb.xprod[(size_t)t * PP_B + k];
                    unsigned long long got = PP_XP_EMPTY;
                    for (int n = 0; n < pb.budget; ++n) {
                        got = __hip_atomic_load(slotp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (__ballot(got == PP_XP_EMPTY) == 0ull) break;
                        __builtin_amdgcn_s_sleep(1);
                    }
                    if (got == PP_XP_EMPTY)
                        __hip_atomic_fetch_or(pb.err, PP_ERR_XSERVE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    vk = __longlong_as_double((long long)got);
                    // taken: empty again for the next launch (the kernel boundary publishes the plain store)
                    pb.xprod[(size_t)t * PP_B + k] = __longlong_as_double((long long)PP_XP_EMPTY);
                }
            } else {
                if (served && valid)    // (a node resolved in the log domain: its slot is emptied, its sum is sCross's)
                    pb.xprod[(size_t)t * PP_B + k] = __longlong_as_double((long long)PP_XP_EMPTY);
                vk = sCross[k];
            }
            if (sat) lr += vk; else r *= vk;
        }
        const unsigned long long g = __ballot(valid && !(sat ? lu >= lr : lu >= r));
        if (lane == 0) sMask[0][half] = g;
    }
    __syncthreads();
    DLSM_STAMP(rst, 2, (double)tid)
    int cur = 0;
    for (int pass = 0; pass < 2 * PP_B + 2; ++pass) {
        const unsigned long long gm = sMask[cur][part >> 2];
        unsigned int bits = (unsigned int)(gm >> (16 * (part & 3))) & 0xFFFFu;
        const int mbase = 16 * part;
        double sum = 1.0, lsum = 0.0;
        if (half == 1 || part < 4) {                   // rows >= 64 never touch half 0
            const double *rowk = sD + k * PR_LD;
            while (bits) {
                int f[4];
                double h[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    f[u] = bits ? mbase + __builtin_ctz(bits) : 1 << 20;
                    bits &= bits - 1u;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) h[u] = rowk[f[u] < (1 << 20) ? f[u] : 0];
                if (!anysat) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) sum *= k > f[u] ? h[u] : 1.0;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (k > f[u]) { if (satk) lsum += log(h[u]); else sum *= h[u]; }
                }
            }
        }
        sPart[wave * 64 + lane] = satk ? lsum : sum;
        __syncthreads();
        if (owner) {
            double q = sat ? lr : r;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const double v = sPart[(2 * p + half) * 64 + lane];
                if (sat) q += v; else q *= v;
            }
            const unsigned long long g = __ballot(valid && !(lu >= q));
            if (lane == 0) sMask[cur ^ 1][half] = g;
        }
        __syncthreads();
        const bool same = sMask[cur ^ 1][0] == sMask[cur][0] &&
                          sMask[cur ^ 1][1] == sMask[cur][1];
        cur ^= 1;
        if (same) break;
    }
    DLSM_STAMP(rst, 3, (double)cur)
    if (owner) {
        const unsigned long long m0 = sMask[cur][0], m1 = sMask[cur][1];
        const unsigned long long mine = half == 0 ? m0 : m1;
        const int accepted = (int)((mine >> lane) & 1ull);
        // (all of it for later launches: write-through under PP_F_WT, like the evaluators' rows and records)
        const bool wt = (pb.flags & PP_F_WT) != 0;
        if (valid) {
            const size_t tj = (size_t)t * N + j0 + k;
            if (accepted) {
#pragma unroll
                for (int d = 0; d < D; ++d) pipe_store(wt, &c.X[tj * D + d], x1[d]);
            }
            metropolis_bookkeeping(st, na, ns, un, c.tune, c.tune_interval, accepted);
            pipe_store(wt, &c.step[tj], st);
            pipe_store_i32(wt, &c.nacc[tj], na); pipe_store_i32(wt, &c.nsteps[tj], ns); pipe_store_i32(wt, &c.until[tj], un);
        }
        // the next batch's window: this batch's acceptances, as a mask
        if (tid == 0) {
            unsigned long long *pmw = (unsigned long long *)(pb.acc + ((size_t)t * 2 + (b & 1)) * PP_ACC + PP_ACC_MASK);
            if (wt) {
                __hip_atomic_store(pmw, m0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(pmw + 1, m1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                pmw[0] = m0; pmw[1] = m1;
            }
        }
    }
    DLSM_STAMP(rst, 4, (double)cur)
    if (tid == 0) rst.flush();
}

}  // namespace dlsm
#include "kernels_pipe_lds.hpp"
namespace dlsm {

// Launch l: even slices resolve batch l and evaluate batch l + 1; odd slices run one launch behind (batches
// outside [0, nbat) do nothing).
// Workgroups [0, T) are the resolvers, the rest evaluate one item per wavefront and round.
// MODEL = PIPE_UNDIRECTED_LONG: the undirected model with parts longer than the prefetch
constexpr int PIPE_UNDIRECTED_LONG = 3;

template <int D, int MODEL_, int G = 1>
__global__ __launch_bounds__(PP_THREADS) void k_pipe_step(ChainView c, PipeBuf pb, int l) {
    // (the benchmark's roofline, profiles/ and six rounds of stored profiler output name this kernel k_pipe_step<2,0,1>)
    static_assert(G == 1, "one batch per launch: the third parameter only keeps the kernel's symbol");
    constexpr int MODEL = MODEL_ == PIPE_UNDIRECTED_LONG ? DLSM_UNDIRECTED : MODEL_;
    constexpr bool TP = MODEL_ != DLSM_UNDIRECTED;
    extern __shared__ __attribute__((aligned(16))) double pp_sH[];      // 128 x PR_LD
    __shared__ double sPart[PP_WAVES * 64];
    __shared__ unsigned long long sMask[2][2];
    const int T = c.T;
    const int bx = (int)blockIdx.x;
    const bool grid3 = MODEL_ == DLSM_UNDIRECTED && pb.lds_eval && (int)gridDim.x > T;    // kernels_pipe_lds.hpp's evaluators
    if (grid3) {
        if (bx >= T) {
            Stamps<PIPE_ITEM_T> first;                  // (read by the item's record, never flushed itself)
            DLSM_STAMP(first, 0, (double)threadIdx.x)               // the wavefront's first instruction
            pipe_eval_lds<D>(c, pb, l, pp_sH, first);
            return;
        }
    }
    if (bx < T) {
        const int t = bx;
        const int b = l - (t & 1);
        if (MODEL == DLSM_DIRECTED_CASE_CONTROL) {
            __shared__ int sPrev[PP_B];
            __shared__ unsigned char sSat[PP_B];
            if (b < 0 || b >= pb.nbat) return;
            pipe_resolve_ccdense<D>(c, pb, b, t, pp_sH, sPart, sMask, sPrev, sSat, Stamps<PIPE_RES_T>(l + 1, t));
            return;
        }
        // exact likelihoods: the H factors by rows and their resolver
        __shared__ double sCross[PP_B];
        __shared__ unsigned long long sSatMask[2];
        __shared__ double sTab[EXPTAB_N];
        const bool served = (pb.flags & PP_F_XSERVE) != 0 && grid3;                 // (both sides decide by the same rule)
        if (l == -1 && threadIdx.x < PP_B)                            // the sweep's first launch: every slot empty
            pb.xprod[(size_t)t * PP_B + threadIdx.x] = __longlong_as_double((long long)PP_XP_EMPTY);
        if (b < 0 || b >= pb.nbat) return;
        row_resolve<D>(c, pb, b, t, pp_sH, sPart, sMask, sCross, sSatMask, sTab, served, Stamps<PIPE_RES_T>(l + 1, t));
        return;
    }
    // (the undirected model's evaluators are kernels_pipe_lds.hpp's above; when their rows do not fit the LDS or
    // the items need a second round the host launches the PIPE_UNDIRECTED_LONG instantiation, whose evaluators are
    // pipe_eval_item's software-pipelined trips below)
    if (MODEL_ == DLSM_UNDIRECTED) return;
    Stamps<PIPE_ITEM_T> first;                  // (read by the item's record, never flushed itself)
    DLSM_STAMP(first, 0, (double)threadIdx.x)                       // the wavefront's first instruction
    const int lane = threadIdx.x & 63;
    const int nE = (T + 1) / 2, nO = T / 2;
    const int beE = l + 1, beO = l;                  // the batch evaluated (even / odd slices)
    const int nbE = (beE >= 0 && beE < pb.nbat) ? min(PP_B, c.N - beE * PP_B) : 0;
    const int nbO = (beO >= 0 && beO < pb.nbat) ? min(PP_B, c.N - beO * PP_B) : 0;
    if (MODEL == DLSM_DIRECTED_CASE_CONTROL) {
        // four nodes per workgroup round, CC_PARTS wavefronts each (pb.parts == CC_PARTS)
        static_assert(PP_B == 128 && CC_PARTS * 64 == 2 * PP_B, "a group's wavefronts cover its LDS column");
        const int wave = threadIdx.x >> 6, sub = wave & (CC_PARTS - 1), grp = wave / CC_PARTS;
        constexpr int GROUPS = PP_WAVES / CC_PARTS;
        double *col = pp_sH + grp * (2 * PP_B);
        const int nodesE = nE * nbE, nodes = nodesE + nO * nbO;
        for (int base = ((int)blockIdx.x - T) * GROUPS; base < nodes;
             base += ((int)gridDim.x - T) * GROUPS) {
            const int q = base + grp;
            const bool valid = q < nodes;
            const bool odd = q >= nodesE;
            const int qq = odd ? q - nodesE : q;
            const int nb = max(odd ? nbO : nbE, 1);
            const int k = qq % nb;
            const int t = 2 * (qq / nb) + (odd ? 1 : 0);
            const int be = odd ? beO : beE;
            col[64 * sub + lane] = 0.0;
            __syncthreads();
            if (valid) pipe_cc_accumulate<D>(c, pb, be, t, k, sub, lane, col);
            __syncthreads();
            if (valid) pipe_cc_writeout<D>(c, pb, be, t, k, sub, lane, col);
            __syncthreads();
        }
        return;
    }
    // items ordered (part, active slice, k) with PP_B k-slots per slice, so that an item id
    // decodes with a shift, a mask and one small quotient (no integer divisions)
    const int nslE = nbE > 0 ? nE : 0, nslO = nbO > 0 ? nO : 0, nsl = nslE + nslO;
    const int nitems = (pb.parts * nsl) << 7;
    const float inv_nsl = 1.0f / (float)max(nsl, 1);
    // the evaluators' table of 2^(j / 2048) (tab_exp11) in the dynamic LDS the resolvers use for H
    // (a barrier-free fill - every wavefront copying the table itself with global_load_lds_dwordx4 -
    // measured no better: 3614 against 3638 it/s; nor did the barrier behind the item's loads: 3615)
    if (MODEL == DLSM_UNDIRECTED) {
        exp_table11_fill<PP_THREADS>(pp_sH, threadIdx.x);
        __syncthreads();
    }
    const int nwaves = ((int)gridDim.x - T) * PP_WAVES;
    const int gw = __builtin_amdgcn_readfirstlane(
        ((int)blockIdx.x - T) * PP_WAVES + (int)(threadIdx.x >> 6));
    for (int q = gw; q < nitems; q += nwaves) {
        const int k = q & (PP_B - 1);
        const int r = q >> 7;
        const int p = (int)(((float)r + 0.5f) * inv_nsl);        // r / nsl (r < 2^20)
        const int si = r - p * nsl;
        const bool odd = si >= nslE;
        const int be = odd ? beO : beE;
        const int nb = be < pb.nbat ? min(PP_B, c.N - be * PP_B) : 0;
        if (k >= nb) continue;
        const int t = odd ? 2 * (si - nslE) + 1 : 2 * si;
        PipeItemPre<D> pre;
        pipe_item_prologue<D, MODEL>(c, pb, be, t, k, p, lane, pre);
        pipe_eval_item<D, MODEL, TP>(c, pb, be, nb, t, k, p, lane, pp_sH, pre, Stamps<PIPE_ITEM_T>(l + 1, gw));
        // (slot 4, "H operands here", gives way to the wavefront's first stamp in the kernel: both evaluators
        // on one time axis)
        Stamps<PIPE_ITEM_T> item(l + 1, q);
        item.set(4, first.get(0));
        if (lane == 0) item.flush(1u << 4);
    }
}

// The sweep's LAST launch only resolves (the last batch of the odd slices; of the even ones when
// T = 1): a handful of workgroups busy for 9 us and the chip idle - while the centring sums, the next
// launch, need nothing but the positions that are final already.  Here they ride in that launch as
// workgroups T ..: every row except the nodes i >= jl of the slices that are still being resolved
// (and the difference terms that touch them: post_row_own_left / post_row_diff_left), which the
// resolver workgroups sum themselves once they have settled them (records nwg .. nwg + T - 1).
// The resolver workgroups run exactly what k_pipe_step runs for them before that.
struct PipePostRide { const double *xref; IterRef ir; double *rec; int nwg, jl, par; };
// workgroup `bx` of T + nwg (the LDS of k_pipe_step's resolvers is the caller's)
template <int D>
__device__ __forceinline__ void pipe_last_ride_wg(const ChainView &c, const PipeBuf &pb, int l,
                                                  const PipePostRide &pr, int bx, double *pp_sH,
                                                  double *sPart, unsigned long long (*sMask)[2]) {
    const int T = c.T;
    if (bx < T) {
        // The rows this launch is still moving (nodes i >= jl of this slice) and the difference terms
        // that touch them are summed HERE, by the workgroup that has just settled them, into record
        // nwg + t: nobody else may read those rows while the launch runs, and the centring pass may
        // not read any position at all once its workgroups have begun to rewrite them in place.
        constexpr int W = PostRec<D>::W;
        __shared__ double sRedL[W][PP_WAVES];
        const int t = bx, tid = threadIdx.x;
        const int b = l - (t & 1);
        const bool mine = b >= 0 && b < pb.nbat;
        if (mine) {
            __shared__ double sCross[PP_B];
            __shared__ unsigned long long sSatMask[2];
            __shared__ double sTab[EXPTAB_N];
            row_resolve<D>(c, pb, b, t, pp_sH, sPart, sMask, sCross, sSatMask, sTab, false, Stamps<PIPE_RES_T>(l + 1, t));
        }
        __syncthreads();                    // the accepted positions of this workgroup are in memory
        double acc[W];
#pragma unroll
        for (int q = 0; q < W; ++q) acc[q] = 0.0;
        if (mine && (t & 1) == pr.par) {
            const int nl = c.N - pr.jl;
            for (int q = tid; q < 2 * nl; q += PP_THREADS) {
                const bool nxt = q >= nl;                   // the difference term of the slice behind
                const int i = pr.jl + (nxt ? q - nl : q), tt = nxt ? t + 1 : t;
                if (tt >= T) continue;
                post_row_terms<D>(c, pr.xref, (long)tt * c.N + i, !nxt, tt >= 1, acc);
            }
        }
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const double v = wave_sum_all(acc[q]);
            if ((tid & 63) == 0) sRedL[q][tid >> 6] = v;
        }
        __syncthreads();
        if (tid < W) {
            double v = 0.0;
#pragma unroll
            for (int w = 0; w < PP_WAVES; ++w) v += sRedL[tid][w];
            pr.rec[(size_t)(pr.nwg + t) * W + tid] = v;
        }
        return;
    }
    post_reduce_wg<D, PP_THREADS>(c, pr.xref, -1, pr.ir, pr.rec, bx - T, pr.nwg, pr.jl, pr.par);
}

template <int D>
__global__ __launch_bounds__(PP_THREADS) void k_pipe_last_ride(ChainView c, PipeBuf pb, int l, PipePostRide pr) {
    extern __shared__ __attribute__((aligned(16))) double pp_sH[];      // 128 x 128
    __shared__ double sPart[PP_WAVES * 64];
    __shared__ unsigned long long sMask[2][2];
    pipe_last_ride_wg<D>(c, pb, l, pr, (int)blockIdx.x, pp_sH, sPart, sMask);
}

}  // namespace dlsm
