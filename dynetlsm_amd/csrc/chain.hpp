// Host-side chain handle and the POD view of it that kernels receive by value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/dynetlsm_hip.h"
#include "device_mem.hpp"

namespace dlsm {

// Everything a kernel needs to know about one chain (device pointers + scalars).
struct ChainView {
    int T, N, D, model, squared;
    int W;                      // uint32 words per bit row (multiple of 4)
    const uint32_t *ybits;      // [T][N][W]  bit i of row j = Y[t, j, i]
    const uint32_t *ytbits;     // [T][N][W]  bit i of row j = Y[t, i, j] (directed)
    // undirected: the same words column-block-major, [T][W / 2][Ncm] of 8 bytes - word (i, cb)
    // = bits 64 cb .. 64 cb + 63 of row i - so that the rows of one 64-column block are contiguous
    // (the log-likelihood pass reads a tile's row words as whole lines); Ncm = N rounded up to its 128-row tiles
    const unsigned long long *ycm; int Ncm;
    // case-control (int32 on device)
    const int32_t *in_edges;  int Din;
    const int32_t *out_edges; int Dout;
    const int32_t *degree;      // [T][N][2]
    const int32_t *ctrl_in;     // [T][N][C], -1 padded
    const int32_t *ctrl_out;  int C;
    double *X;                  // [T][N][D]
    const double *intercept;    // device [2]
    const double *radii;        // device [N]
    int prior_kind;
    double tau_sq, sigma_sq;
    const double *mu; const double *sigma;
    const double *lmbda_p;      // device scalar: the blending coefficient (set_prior_mixture / the HDP loop)
    const int32_t *z; int K;
    double *step; int32_t *nacc; int32_t *nsteps; int32_t *until;
    int tune, tune_interval;
    uint64_t seed; uint32_t chain;
};

// What the proposal pass of the pipelined sweeps writes (kernels_spec_pipe.hpp): the iteration's
// last launch can carry the next sweep's pass (kernels_tail_propose.hpp)
struct LsmDeviceState;
struct ProposeBuf {
    double *prop, *consts;
    LsmDeviceState *lsm_draw;   // not NULL: the pass also draws the undirected loop's intercept proposal
};

// intercept sampler + LSM bookkeeping that lives on the device
struct LsmDeviceState {
    double intercept_prior[2];
    double intercept_var;
    double i_step[2];
    int32_t i_nacc[2], i_nsteps[2], i_until[2];
    int32_t i_tune, i_tune_interval;
    double cand[4];             // candidate intercepts of the current MH step
    double prior_x;             // latent-position prior terms of logp (lsm.py:604-613)
    double logu;                // log-uniform of the intercept accept test
    uint32_t iter;              // iteration counter of the captured-graph path
    uint32_t pad_;
    // directed loop: radii sampler (Dirichlet proposal), current log-likelihood, proposal
    // density ratio of the radii step
    double r_step;
    int32_t r_nacc, r_nsteps, r_until, r_tune, r_tune_interval, r_pad_;
    double ll_cur, dir_q;
    double r_logu;              // log-uniform of the radii step's accept test (its own word: the proposal
                                // is closed while the intercept steps still use `logu`)
    // case-control loop: BOTH intercept steps around one four-candidate pass (kernels_dirloop.hpp):
    // (b_in', b_out), (b_in, b_out), (b_in', b_out'), (b_in, b_out') and the second step's log-uniform
    double cand8[8];
    double logu2;
};

// Device-resident HDP-LPCM loop (hdp_lpcm.py:823-1069): hyper-parameters the loop resamples,
// the fixed hyper-priors, the blending coefficient and the carried log-likelihood.  The
// intercept sampler lives in LsmDeviceState.
struct HdpDeviceState {
    double gamma, alpha_init, alpha, kappa, mvp, b;     // resampled (hdp_lpcm.py:957-1023)
    double a, a0, b0, c0, d0;
    int32_t has_a0, has_c0;
    double lambda_prior, lambda_var;
    double gamma_shape, gamma_rate, alpha0_shape, alpha0_rate, ak_shape, ak_rate;
    double lmbda;               // current blending coefficient (ChainView::lmbda_p points here)
    double ll;                  // network log-likelihood after the intercept step
    // totals of the auxiliary variables of the current iteration (k_hdp_globals)
    double mbar_total, mbar_positive, m00_total, m_rest_total, override_total;
};

// What one sweep carries over to the next on the same handle: the proposal buffers of the pipelined sweep
// enqueued last (valid for a pipelined sweep only), the iteration whose proposals an earlier launch has
// already drawn into them, and the iteration whose head (the proposal pass and the first, evaluate-only
// launch) is enqueued already - on the HDP-LPCM loop's second queue (capi_hdp.hpp)
struct SweepCarry {
    ProposeBuf next_prop{}; bool next_prop_ok = false;
    long prop_drawn_for = -1, head_done_for = -1;
    void reset() { next_prop_ok = false; prop_drawn_for = -1; head_done_for = -1; }
    // were iteration `it`'s proposals (it < 0: counted on the device - never) drawn into these buffers
    bool drawn(long it, const ProposeBuf &nb) const {
        return it >= 0 && prop_drawn_for == it && next_prop_ok && next_prop.prop == nb.prop &&
               next_prop.consts == nb.consts && next_prop.lsm_draw == nb.lsm_draw;
    }
    // a pipelined sweep has taken the buffers `nb` (and whatever was drawn ahead into them)
    void taken(const ProposeBuf &nb) { next_prop = nb; next_prop_ok = true; prop_drawn_for = -1; }
};

struct ProfileSlot {
    double ms = 0.0;
    int launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

}  // namespace dlsm

struct dlsm_chain {
    template <typename T> using Dev = dlsm::DevArray<T>;
    int device = 0;
    int T = 0, N = 0, D = 0, model = 0, squared = 0;
    uint64_t seed = 0; uint32_t chain = 0;
    hipStream_t stream = nullptr;
    dlsm::HostArray<char> stage;            // pinned host staging for the small copies of the C-ABI
    // HDP-LPCM loop, undirected: the intercept's likelihood pass on a queue of its own beside the label
    // update and the conjugate draws, handed over through device flags (kernels_hdploop.hpp, HdpFork)
    hipStream_t fork_stream = nullptr; hipEvent_t fork_ev = nullptr;
    Dev<int32_t> fork_flags; int32_t fork_ticket = 0; bool fork_armed = false;
    dlsm::HostArray<int32_t> fork_err;      // sticky error word (mapped host memory: get() here, dev() in kernels)
    bool fork_wait_value = false;           // the queues' waits are hipStreamWaitValue32 (else the gate kernel)
    // network
    int W = 0;
    Dev<uint32_t> ybits, ytbits;
    Dev<unsigned long long> ycm;            // undirected: column-block-major copy of ybits
    bool have_network = false;
    int Din = 0, Dout = 0, C = 0;
    Dev<int32_t> in_edges, out_edges, degree;
    Dev<int32_t> ctrl_in, ctrl_out;
    bool have_edges = false, have_controls = false;
    // state
    Dev<double> X, intercept, radii, radii_alt;
    bool have_X = false, have_radii = false;
    Dev<double> step; Dev<int32_t> nacc, nsteps, until;
    int tune = -1, tune_interval = 100;
    bool have_samplers = false;
    int prior_kind = 0; double tau_sq = 2.0, sigma_sq = 0.1;
    Dev<double> mu, sigma; double lmbda = 0.0; Dev<int32_t> z;
    Dev<dlsm::HdpDeviceState> hdp;          // always allocated (holds lmbda)
    // device-resident HDP-LPCM loop: auxiliary buffers (workspace.hpp, hdp_loop_layout) and traces
    Dev<double> hdp_buf; int hdp_K = 0;
    bool hdp_configured = false;
    dlsm_hdp_config hdp_cfg{};
    Dev<double> htr_mu, htr_sigma, htr_beta, htr_w, htr_lambda, htr_hyper;
    Dev<uint8_t> htr_z;
    int htr_n = 0, htr_K = 0;
    int K = 0; bool have_prior = false;
    // scratch
    Dev<double> partials;
    Dev<double> xr;                // packed (x, r, r') records (case-control)
    Dev<double> dsmall;            // 128 doubles of device scratch ([64, 128): a d x d rotation, d <= 8)
    dlsm::HostArray<double> hsmall;         // 64 doubles of pinned host scratch
    Dev<double> xref;              // T*N*D (procrustes reference staging)
    Dev<int32_t> lab_n, lab_nk; Dev<double> lab_w;         // lab_n, lab_w: the T*K*K they were sized for
    // sweep v2 scratch (workspace.hpp: spec_layout; pipe_layout / ccpipe_layout)
    Dev<double> spec;
    Dev<double> pipe;                                   // pipelined sweeps (algo 4, algo 5) buffers
    int pipe_head_q = 0;                                // nodes per evaluator workgroup of its last head launch (0: none yet)
    dlsm::SweepCarry carry;
    int n_cu = 256;
    Dev<int32_t> nctrl;                                 // valid controls per (t, i, dir)
    bool nctrl_valid = false;
    // case-control model: a node's counts, control weights and its four index lists as one row (cc_rows.hpp)
    Dev<int32_t> cc_terms; bool cc_terms_valid = false; int cc_tw = 0;
    // the likelihood pass's walking order (cc_rows.hpp, k_cc_order): entries, then a count per slice
    Dev<int32_t> cc_order; int32_t *cc_order_cnt = nullptr; int cc_emax = 0;
    Dev<int32_t> cc_pos;                                     // where a node's row lies (cc_rows.hpp: k_cc_pos)
    Dev<unsigned long long> stamps;                     // in-kernel timestamps (profiling): [start, end] pairs
    size_t stamps_used = 0;                             // in pairs
    std::vector<std::pair<size_t, size_t>> stamp_launches;   // (first pair, pairs) per launch
    // initialisation pipeline: hop matrices [T][N][N] and the per-slice maximum
    Dev<uint16_t> hops; Dev<int> hops_max; bool have_hops = false;
    // post-loop processing: labels of the kept samples (bytes, [T][N][Spad]) and the
    // co-occurrence probabilities [T][N][N]
    Dev<uint8_t> post_zt; Dev<double> post_cooc; int post_S = 0, post_Spad = 0;
    // LSM device-resident chain
    Dev<dlsm::LsmDeviceState> lsm;
    dlsm_lsm_config lsm_cfg{};
    bool lsm_configured = false;
    Dev<double> trace_X, trace_ic, trace_logp;
    Dev<double> trace_radii;
    int trace_n = 0;
    // dlsm_lsm_run's last radii step is still where it left it (radii_alt, dsmall[16], the sampler's words):
    // dlsm_lsm_get_radii_step; cleared by whatever writes one of them
    bool radii_step_fresh = false;
    // one captured Gibbs iteration (hipGraph), replayed by dlsm_lsm_run
    hipGraph_t graph = nullptr; hipGraphExec_t graph_exec = nullptr;
    int graph_ref = -2, graph_algo = -1; bool graph_failed = false;
    // missing-dyad imputation (kernels_missing.hpp): per-(matrix, t, row) segments of the list in both
    // orientations, the accumulators per listed dyad, and whether dlsm_lsm_run ends its iterations with the step
    int64_t miss_n = 0; int miss_njobs = 0;
    Dev<int32_t> miss_jobs, miss_cols, miss_slot;
    Dev<double> miss_psum; Dev<uint32_t> miss_ones; Dev<unsigned long long> miss_nacc;
    bool miss_on = false; int64_t miss_after = 0;
    // measurement
    bool profiling = false;
    dlsm::ProfileSlot prof[DLSM_K_COUNT];
    hipEvent_t timer0 = nullptr, timer1 = nullptr;
    std::string err;

    dlsm::ChainView view() const {
        dlsm::ChainView v;
        v.T = T; v.N = N; v.D = D; v.model = model; v.squared = squared; v.W = W;
        v.ybits = ybits; v.ytbits = ytbits;
        v.ycm = ycm; v.Ncm = (N + 127) / 128 * 128;
        v.in_edges = in_edges; v.Din = Din; v.out_edges = out_edges; v.Dout = Dout;
        v.degree = degree; v.ctrl_in = ctrl_in; v.ctrl_out = ctrl_out; v.C = C;
        v.X = X; v.intercept = intercept; v.radii = radii;
        v.prior_kind = prior_kind; v.tau_sq = tau_sq; v.sigma_sq = sigma_sq;
        v.mu = mu; v.sigma = sigma; v.lmbda_p = hdp ? &hdp->lmbda : nullptr; v.z = z; v.K = K;
        v.step = step; v.nacc = nacc; v.nsteps = nsteps; v.until = until;
        v.tune = tune; v.tune_interval = tune_interval;
        v.seed = seed; v.chain = chain;
        return v;
    }
};
