/*
 * dynetlsm_hip.h -- C-ABI of the MI355X (gfx950) engine for DynetLSM's
 * Metropolis-within-Gibbs hot path.
 *
 * The reference (joshloyal/dynetlsm v0.1.0) has no FFI: its seams are Python
 * function calls.  Each entry point below names the reference
 * call it replaces (file:line relative to the reference tree).  A chain handle
 * owns ALL device state (bit-packed network, latent positions, Metropolis
 * state, Philox key); one handle per chain per device.  A handle is not
 * thread-safe; different handles may be used from different host threads.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (DLSM_E_*);
 *     dlsm_last_error() gives the message.  No exceptions, no callbacks.
 *   - host arrays are C-contiguous little-endian float64 / int64 / int32 as
 *     stated; the callee never keeps a host pointer past return.
 *   - calls are synchronous at return (results are in the host buffers) except
 *     the *_async / run calls, which only enqueue on the handle's stream and
 *     are completed by dlsm_synchronize().
 *   - counter RNG: Philox4x32-10 keyed by `seed`, counter (index, t|draw<<16,
 *     iteration, chain<<8|stream); the CPU oracle uses the same draws.
 */
#ifndef DYNETLSM_HIP_H
#define DYNETLSM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLSM_ABI_VERSION 1

enum {
    DLSM_OK = 0,
    DLSM_E_ARG = -1,      /* bad argument / wrong state */
    DLSM_E_HIP = -2,      /* HIP runtime error */
    DLSM_E_NODEV = -3,    /* no usable gfx950 device */
    DLSM_E_DATA = -4,     /* network entries not in {0,1} etc. */
    DLSM_E_LIMIT = -5     /* size beyond what the kernels support */
};

enum { DLSM_UNDIRECTED = 0, DLSM_DIRECTED = 1, DLSM_DIRECTED_CASE_CONTROL = 2 };
enum { DLSM_PRIOR_RANDOM_WALK = 0, DLSM_PRIOR_MIXTURE = 1 };

typedef struct dlsm_chain dlsm_chain;

int dlsm_abi_version(void);
int dlsm_device_count(int *count);
/* message of the last failing call on this handle (or of dlsm_create if NULL) */
const char *dlsm_last_error(const dlsm_chain *h);

/* ---- lifecycle ------------------------------------------------------- */
/* replaces the per-fit allocations of lsm.py:371-383,451-470 /
 * hdp_lpcm.py:691-747: one chain of a T x N x N network, D latent features */
int dlsm_create(int device, int T, int N, int D, int model, uint64_t seed,
                uint32_t chain_id, dlsm_chain **out);
void dlsm_destroy(dlsm_chain *h);
int dlsm_synchronize(dlsm_chain *h);

/* ---- network --------------------------------------------------------- */
/* Y: T*N*N float64 row-major exactly as fit(Y) receives it (lsm.py:341).
 * Packed on device to 1 bit/dyad (+ the transpose for directed models).
 * Entries other than 0.0 / 1.0 -> DLSM_E_DATA (the estimators impute -1 coded
 * dyads before the upload, as imputer.py / lsm.py:345-359 do). */
int dlsm_upload_network(dlsm_chain *h, const double *Y);
/* the network as the chain holds it (1 bit per dyad; [T][N][W] uint32 words,
 * W = dlsm_network_packed_words / (T N), followed by the transposed copy for the directed
 * model), so that one chain's upload can be broadcast to the chains on the other GPUs
 * (RCCL) without a host round trip of the float64 tensor: at T=10, N=2000 5 MB instead of
 * 320 MB.  `buf` may be a device or a host pointer (hipMemcpyDefault).  The reference has
 * no counterpart (examples/homogeneous_simulation.py:178-184 refits seeds serially). */
int dlsm_network_packed_words(dlsm_chain *h, int64_t *n_words);
int dlsm_get_network_packed(dlsm_chain *h, uint32_t *buf, int64_t n_words);
int dlsm_set_network_packed(dlsm_chain *h, const uint32_t *buf, int64_t n_words);
/* case-control: zero padded edge lists and degrees exactly as
 * DirectedCaseControlSampler.init builds them (case_control_likelihood.py:45-68):
 * in_edges T*N*Din, out_edges T*N*Dout, degree T*N*2 (col 0 in, col 1 out). */
int dlsm_upload_edges(dlsm_chain *h, const int64_t *in_edges, int Din,
                      const int64_t *out_edges, int Dout, const int64_t *degree);
/* The network as lists of ties: the pairs (src[e], dst[e]) of time step t are e in
 * offsets[t] .. offsets[t+1] - 1 (offsets: T+1 values, offsets[0] = 0, non-decreasing; any order
 * inside a step, duplicates allowed).  Replaces the float64 upload of lsm.py:341 and, on
 * case-control chains, the host loops of case_control_likelihood.py:45-68; nothing of size N*N
 * crosses the bus.  Leaves what the dense calls leave for the same network:
 *   DLSM_UNDIRECTED             the packed words of dlsm_upload_network, both orientations of every pair
 *   DLSM_DIRECTED               the packed words and their transpose
 *   DLSM_DIRECTED_CASE_CONTROL  degree, in_edges, out_edges of dlsm_upload_edges (zero padded,
 *                               neighbours ascending, widths = the largest in- / out-degree)
 * A node index outside 0..N-1 or src == dst -> DLSM_E_DATA, bad offsets -> DLSM_E_ARG; after a
 * failed call the chain has no network / edge lists. */
int dlsm_upload_network_edges(dlsm_chain *h, const int64_t *offsets, const int32_t *src,
                              const int32_t *dst);
/* the case-control tables as the chain holds them: the widths, then in_edges T*N*Din,
 * out_edges T*N*Dout, degree T*N*2 as int64 (in_edges_ / out_edges_ / degrees_ of
 * case_control_likelihood.py:45-68) */
int dlsm_edge_table_widths(dlsm_chain *h, int *Din, int *Dout);
int dlsm_get_edges(dlsm_chain *h, int64_t *in_edges, int64_t *out_edges, int64_t *degree);
/* control_nodes_in_/out_: T*N*C int64, -1 padded (case_control_likelihood.py:79-82) */
int dlsm_set_controls(dlsm_chain *h, const int64_t *ctrl_in,
                      const int64_t *ctrl_out, int C);
int dlsm_get_controls(dlsm_chain *h, int64_t *ctrl_in, int64_t *ctrl_out);
/* DirectedCaseControlSampler.sample (case_control_likelihood.py:75-112) on
 * device: for every (t, i) draw min(n_control, #zeros) distinct non-neighbours
 * != i, separately for the out and the in direction, Philox stream CONTROLS. */
int dlsm_resample_controls(dlsm_chain *h, uint32_t iter, int n_control);

/* ---- chain state (so host and device paths can be swapped mid-chain) --- */
int dlsm_set_positions(dlsm_chain *h, const double *X);        /* T*N*D */
int dlsm_get_positions(dlsm_chain *h, double *X);
int dlsm_set_intercepts(dlsm_chain *h, const double *b, int n); /* 1 or 2 */
int dlsm_get_intercepts(dlsm_chain *h, double *b, int n);
int dlsm_set_radii(dlsm_chain *h, const double *radii);         /* N */
int dlsm_get_radii(dlsm_chain *h, double *radii);
int dlsm_set_squared(dlsm_chain *h, int squared);
/* T x N grid of random-walk Metropolis samplers (metropolis.py:85-94);
 * tune < 0 means tune=None */
int dlsm_set_samplers(dlsm_chain *h, const double *step_size,
                      const int32_t *n_accepted, const int32_t *n_steps,
                      const int32_t *steps_until_tune, int tune, int tune_interval);
int dlsm_get_samplers(dlsm_chain *h, double *step_size, int32_t *n_accepted,
                      int32_t *n_steps, int32_t *steps_until_tune);
/* prior of sample_latent_positions (sample_latent_positions.py:132-140) */
int dlsm_set_prior_random_walk(dlsm_chain *h, double tau_sq, double sigma_sq);
/* prior of sample_latent_positions_mixture (:187-199): mu K*D, sigma K
 * (variances), z T*N int64; z = NULL keeps the labels already on the device (those of
 * the last dlsm_sample_labels / dlsm_set_prior_mixture with the same K) */
int dlsm_set_prior_mixture(dlsm_chain *h, const double *mu, const double *sigma,
                           double lmbda, const int64_t *z, int K);

/* ---- kernels --------------------------------------------------------- */
/* a4/a5/a6: dynamic_network_loglikelihood_undirected (network_likelihoods.py:26-33),
 * directed_network_loglikelihood_fast (directed_likelihoods_fast.pyx:185-205),
 * approx_directed_network_loglikelihood (:208-270) at the handle's current X
 * for m candidate intercepts (m*1 undirected, m*2 directed: [b_in, b_out]).
 * intercepts == NULL evaluates the handle's current intercept (m = 1). */
int dlsm_loglik_full(dlsm_chain *h, int m, const double *intercepts, double *out);
/* directed models: out[0] at the handle's radii, out[1] at radii_alt, both at
 * the current intercepts (sample_radii, sample_coefficients.py:91-121) */
int dlsm_loglik_full_radii(dlsm_chain *h, const double *radii_alt, double *out);
/* a1/a2/a3: partial_loglikelihood (static_network_fast.pyx:17-44),
 * directed_partial_loglikelihood (directed_likelihoods_fast.pyx:46-80),
 * approx_directed_partial_loglikelihood (:83-182) of node j at time t with
 * X[t, j] replaced by x (x == NULL: current position).  with_prior != 0 adds
 * the prior terms of the sweep's logp closure. */
int dlsm_loglik_partial(dlsm_chain *h, int t, int j, const double *x,
                        int with_prior, double *out);
/* the same for every (t, j) at the current state: out T*N */
int dlsm_loglik_partial_all(dlsm_chain *h, int with_prior, double *out);
/* a8-a10: one sweep of sample_latent_positions / _mixture: T*N random-walk MH
 * steps, even-t slices concurrently then odd-t slices, Gauss-Seidel inside a
 * slice; updates X and the sampler grid on device.  algo 0 = auto,
 * 1 = one workgroup per slice, 2 = speculative batches over the whole chip,
 * 3 = speculative batches with one launch pair per two 128-node sub-batches,
 * 4 = pipelined speculative batches: one fused launch resolves batch b and
 *     evaluates batch b + 1, both parities in the same launches,
 * 5 = (case-control model) the pipelined form with sparse correction lists and batches
 *     of 512 nodes.
 * (6 = two batches per launch and 7 = one persistent launch per sweep existed in rounds 2-4,
 *  measured slower than 4 and were removed in round 5: DLSM_E_ARG.) */
int dlsm_sweep_positions(dlsm_chain *h, uint32_t iter, int algo);
/* the algorithm `algo` resolves to for this handle (what 0 = auto picks): 1, 2, 4 or 5; a
 * non-zero `algo` is returned as it is after the same checks as dlsm_sweep_positions */
int dlsm_resolve_sweep_algo(dlsm_chain *h, int algo);
/* nodes per evaluator workgroup of the last pipelined sweep's (algo 4) head launch: 16, or 8 when the
 * launch was spread over twice the workgroups (DLSM_PIPE_HEAD_SPREAD); 0 before the first such sweep */
int dlsm_pipe_head_nodes(dlsm_chain *h, int *nodes);
/* lsm.py:501 / hdp_lpcm.py:852 */
int dlsm_center(dlsm_chain *h);
/* longitudinal_procrustes_rotation (procrustes.py:28-35): X <- X R with
 * R = argmin ||X R - X_ref||_F ; X_ref T*N*D ; R_out (D*D, may be NULL) */
int dlsm_procrustes(dlsm_chain *h, const double *X_ref, double *R_out);
/* a11: compute_gaussian_likelihood(X[:, node], mu, sigma, lmbda, normalize)
 * (gaussian_likelihood_fast.pyx:30-54) with the mixture prior's parameters */
int dlsm_gaussian_likelihood(dlsm_chain *h, int node, int normalize, double *out);
/* a12: sample_labels_block (sample_labels.py:134-190); w T*K*K (w[0,0,:] the
 * initial distribution).  Writes z (T*N), n (T*K*K), nk (T*K) and keeps the new
 * z on device as the mixture prior's labels. */
int dlsm_sample_labels(dlsm_chain *h, uint32_t iter, const double *w, int64_t *z,
                       double *n, int64_t *nk);

/* the O(T N) sums of the HDP-LPCM conjugate updates over the nodes that
 * carry a label, at the handle's positions and labels (the z of the last
 * dlsm_sample_labels / dlsm_set_prior_mixture), K = the mixture prior's components:
 *   stage 0 (hdp_lpcm.py:901-921)  out T*K*D : sum_i V_ti, V_0 = X_0, V_t = X_t - (1-lmbda) X_{t-1}
 *   stage 1 (:924-938)             out T*K   : sum_i squared residuals about the NEW mu
 *   stage 2 (:941-954)             out T*K*2 : the two sums of the lambda update per (t, k)
 *   stage 3 (:1213-1262)           out T*K   : the node terms of DynamicNetworkHDPLPCM.logp
 *                                              (label transitions w, Gaussian and inverse-gamma
 *                                              terms; a, b the variance prior's parameters)
 * mu K*D, sigma K, w T*K*K are the values the update holds at that point (they are not
 * stored in the handle).  Fixed summation order: bitwise reproducible. */
int dlsm_hdp_label_sums(dlsm_chain *h, int stage, const double *mu, const double *sigma,
                        double lmbda, const double *w, double a, double b, double *out);

/* ---- device-resident LSM chain (lsm.py:474-572, fully observed network) -- */
typedef struct {
    double intercept_prior[2];
    double intercept_variance_prior;
    /* intercept samplers (metropolis.py:85-94); [0] = b or b_in, [1] = b_out */
    double i_step_size[2];
    int32_t i_n_accepted[2], i_n_steps[2], i_steps_until_tune[2];
    int32_t i_tune, i_tune_interval;           /* i_tune < 0 == None */
    int32_t n_iter_procrustes;                 /* lsm.py:362-368 */
    int32_t sweep_algo;                        /* as dlsm_sweep_positions */
    /* directed models: the radii sampler (scaled-Dirichlet proposal, metropolis.py:57-82;
     * r_tune < 0 == None, as DynamicNetworkLSM sets it) */
    double r_step_size;
    int32_t r_n_accepted, r_n_steps, r_steps_until_tune, r_tune, r_tune_interval, r_pad;
} dlsm_lsm_config;
int dlsm_lsm_configure(dlsm_chain *h, const dlsm_lsm_config *cfg);
int dlsm_lsm_get_config(dlsm_chain *h, dlsm_lsm_config *cfg);
/* device trace buffers Xs_[n_total,T,N,D], intercepts_[n_total,2],
 * logps_[n_total]; row 0 is filled from the current state, logp0 given */
int dlsm_trace_alloc(dlsm_chain *h, int n_total, double logp0);
/* enqueue iterations it = first .. first+count-1: sweep, Procrustes to row
 * `procrustes_ref` of the trace if it > n_iter_procrustes, centring, then
 *   undirected: intercept RW-MH fused with the log-posterior trace;
 *   directed / case-control: intercept_in, intercept_out (sample_coefficients.py:12-75)
 *   and radii (:91-121) MH steps, each around one fused two-candidate pass, with Philox
 *   draws (the caller resamples controls between calls at its own cadence).
 * Asynchronous. */
int dlsm_lsm_run(dlsm_chain *h, int first, int count, int procrustes_ref);
int dlsm_trace_read(dlsm_chain *h, int first, int count, double *Xs,
                    double *intercepts, double *logps);
/* rows first .. first+count-1 of the radii trace (count*N), directed models */
int dlsm_trace_read_radii(dlsm_chain *h, int first, int count, double *radii);
/* A read-only view of the radii step of the last iteration dlsm_lsm_run ran, accepted or not
 * (directed and case-control handles): proposal[N] = the scaled-Dirichlet proposal, after the repair
 * of an exact zero if there was one; terms[4] = the proposal density ratio
 * log Dir(radii | step x) - log Dir(x | step radii), the log-uniform of the accept test, the network
 * log-likelihood at the proposal, and the one at the radii the step started from (both at the
 * intercepts the two intercept steps left).  The step was accepted if and only if
 * terms[1] < (terms[2] - terms[3]) + terms[0]; a NaN on the right-hand side rejects.  Waits for the
 * handle's stream and copies; no kernel runs.  An undirected or unconfigured handle, no
 * dlsm_lsm_run (of at least one iteration) yet, or a dlsm_loglik_full, dlsm_loglik_full_radii,
 * dlsm_loglik_partial, dlsm_lsm_configure, dlsm_hdp_configure or dlsm_hdp_run call since, which
 * reuse the step's buffers -> DLSM_E_ARG. */
int dlsm_lsm_get_radii_step(dlsm_chain *h, double *proposal, double *terms);

/* ---- device-resident HDP-LPCM chain (hdp_lpcm.py:823-1069) --------------------------
 * the whole Gibbs iteration of DynamicNetworkHDPLPCM._fit on the device -
 * sweep with the AR-mixture prior, centring, intercept MH, label block update
 * (sample_labels.py:134-190), table counts and override variables
 * (sample_auxillary.py:6-50), beta / w0 / w Dirichlet draws (hdp_lpcm.py:887-898), cluster
 * means, variances and the blending coefficient (:901-954), the variance hyper-parameters
 * (:957-972), the concentration parameters (sample_concentration.py:6-21,
 * hdp_lpcm.py:977-1023) and the log-posterior trace (:1188-1280) - with Philox draws (stream
 * HDP = 6, counter (index, kind | attempt << 8, iteration)): no host round trip inside an
 * iteration.  The mixture's state (mu, sigma, lmbda, z) is what dlsm_set_prior_mixture
 * left on the device.  Directed and case-control models: the intercept step is the two steps of
 * sample_coefficients.py:12-75 followed by the radii step (:91-121), as in dlsm_lsm_run's
 * directed loop (the caller resamples the controls between calls at its own cadence); the radii
 * trace is read with dlsm_trace_read_radii. */
typedef struct {
    /* resampled by the loop */
    double gamma, alpha_init, alpha, kappa, mean_variance_prior, b;
    /* fixed hyper-priors (hdp_lpcm.py:760-793); has_a0 / has_c0 = 0 switch the updates of
     * mean_variance_prior / b off (mean_variance_prior_std / sigma_prior_std = None) */
    double a, a0, b0, c0, d0;
    int32_t has_a0, has_c0;
    double lambda_prior, lambda_variance_prior;
    double gamma_prior_shape, gamma_prior_rate, alpha_init_shape, alpha_init_rate,
           alpha_kappa_shape, alpha_kappa_rate;
    double intercept_prior, intercept_variance_prior;
    /* the intercept's random-walk sampler (metropolis.py:85-94); i_tune < 0 == None */
    double i_step_size;
    int32_t i_n_accepted, i_n_steps, i_steps_until_tune, i_tune, i_tune_interval;
    int32_t sweep_algo;                        /* as dlsm_sweep_positions */
    /* directed models (hdp_lpcm.py:731-747, sample_coefficients.py:12-121): the fields above
     * describe intercept_in, these intercept_out and the radii sampler (scaled-Dirichlet
     * proposal, metropolis.py:57-82; r_tune < 0 == None) */
    double intercept_prior_out, i_step_size_out;
    int32_t i_n_accepted_out, i_n_steps_out, i_steps_until_tune_out, r_tune;
    double r_step_size;
    int32_t r_n_accepted, r_n_steps, r_steps_until_tune, r_tune_interval;
} dlsm_hdp_config;
/* beta K, weights T*K*K (weights[0,0,:] the initial distribution), K = the mixture prior's */
int dlsm_hdp_configure(dlsm_chain *h, const dlsm_hdp_config *cfg, const double *beta,
                       const double *weights);
/* the current hyper-parameters and sampler state */
int dlsm_hdp_get_config(dlsm_chain *h, dlsm_hdp_config *cfg);
/* device trace of n_total samples: Xs_, intercepts_, logps_ (shared with the LSM loop's
 * buffers), mus_, sigmas_, zs_, betas_, weights_, lambdas_ and the six resampled
 * hyper-parameters; row 0 = the current state, logp0 given */
int dlsm_hdp_trace_alloc(dlsm_chain *h, int n_total, double logp0);
/* enqueue iterations first .. first+count-1.  Asynchronous.
 * Undirected model: the intercept step's likelihood pass (sample_coefficients.py:76-86 inside
 * hdp_lpcm.py:855-874) - and behind it the head of the next iteration's sweep, which reads positions,
 * step sizes and the settled intercept only - runs on a second queue of the handle beside the label
 * update and the conjugate draws (hdp_lpcm.py:876-1023), which do not read its result; the queues hand over through words in
 * device memory and are joined before the call's log-posterior pass, so the call still orders like one
 * stream.  Chosen while the handle is the process's only live chain (environment: DLSM_HDP_QUEUES=1
 * never, =2 always); the trace is bit for bit the one-queue trace.  Processes that SHARE a device
 * should set DLSM_HDP_QUEUES=1 (multichain.launch_ranks does): queues of two processes taking turns on
 * one GPU lose more than the second queue hides. */
int dlsm_hdp_run(dlsm_chain *h, int first, int count);
/* queues the last dlsm_hdp_run call of this handle used: 1 or 2 */
int dlsm_hdp_queues(dlsm_chain *h, int *queues);
/* rows first .. first+count-1; any pointer may be NULL.  zs count*T*N int64, hypers count*6
 * [gamma, alpha_init, alpha, kappa, mean_variance_prior, b]; intercepts count*2 (undirected
 * model: the second column carries the network log-likelihood of the stored state) */
int dlsm_hdp_trace_read(dlsm_chain *h, int first, int count, double *Xs, double *intercepts,
                        double *logps, double *mus, double *sigmas, int64_t *zs, double *betas,
                        double *weights, double *lambdas, double *hypers);
/* the mirror of dlsm_hdp_trace_read (intercepts: count*1 for the undirected model, count*2 for
 * the directed ones): rows first ..
 * first+count-1 of the device-resident trace from host arrays; any pointer may be NULL.  Lets a
 * caller continue or post-process on the device a trace it holds on the host (the reference
 * keeps Xs_, zs_, ... as attributes of the fitted estimator, hdp_lpcm.py:691-747). */
int dlsm_hdp_trace_write(dlsm_chain *h, int first, int count, const double *Xs,
                         const double *intercepts, const double *logps, const double *mus,
                         const double *sigmas, const int64_t *zs, const double *betas,
                         const double *weights, const double *lambdas);
/* auxiliary variables of the last iteration (tests): m T*K*K tables, m_bar K, w_over (T-1)*K
 * override counts, n T*K*K and nk T*K label counts */
int dlsm_hdp_get_aux(dlsm_chain *h, int64_t *m, double *m_bar, int64_t *w_over, int64_t *n,
                     int64_t *nk);

/* ---- starting values (generalized_mds + conditional MLEs) -- */
/* shortest_path_dissimilarity (latent_space.py:36-44) of every time slice, from
 * the bit-packed network (symmetrised for directed models, as
 * csgraph.shortest_path(directed=False, unweighted=True) does): hop counts
 * [T][N][N] kept on the device as uint16, unconnected pairs = largest finite
 * hop count of the slice + 1. */
int dlsm_init_shortest_paths(dlsm_chain *h);
/* slice t of the above as float64 N*N */
int dlsm_init_get_dissimilarity(dlsm_chain *h, int t, double *out);
/* MDS(dissimilarity='precomputed').fit_transform(D[t]) (latent_space.py:66-68):
 * sklearn's metric SMACOF (_smacof_single, scikit-learn >= 1.7 convergence rule
 * (old_stress - stress) / (sum dis^2 / 2) < eps) run from n_init starting
 * configurations X0 (n_init*N*D, the caller draws them: RandomState.uniform)
 * concurrently.  Per run: final configuration, raw stress and n_iter; the caller
 * keeps the run of least stress as sklearn.manifold.smacof does. */
int dlsm_init_smacof(dlsm_chain *h, int t, int n_init, const double *X0, int max_iter,
                     double eps, double *X_out, double *stress_out, int32_t *n_iter_out);
/* one step t >= 1 of generalized_mds (latent_space.py:71-89): top-D eigenpairs of
 * alpha H(-D_t^2/2)H + beta X_prev X_prev^T (alpha = 1/(1+lmbda), beta =
 * lmbda/(1+lmbda)) by Lanczos with full reorthogonalisation (at most max_lanczos
 * vectors, stop at relative residual tol), X = V sqrt(evals), then the Procrustes
 * rotation onto X_prev (procrustes.py:20-25).  X_prev, X_out: N*D. */
int dlsm_init_gmds_step(dlsm_chain *h, int t, const double *X_prev, double lmbda,
                        int max_lanczos, double tol, double *X_out, double *evals_out,
                        int32_t *n_lanczos_out, double *resid_out);
/* objective and gradient of the conditional MLEs at the handle's positions:
 * undirected (scale_intercept_mle, lsm.py:32-70): p0 = log scale, p1 = intercept,
 *   out = [loglik, scale_grad, undirected_intercept_grad];
 * directed (directed_intercept_mle, lsm.py:73-97): p0 = b_in, p1 = b_out,
 *   out = [loglik, directed_intercept_grad in, out]
 *   (directed_likelihoods_fast.pyx:20-43). */
int dlsm_init_mle_sums(dlsm_chain *h, double p0, double p1, double *out);
/* the Lloyd iterations of longitudinal_kmeans (latent_space.py:98-137: sklearn.cluster.KMeans on
 * the N x F matrix of time-stacked trajectories, F = T d), scikit-learn's _kmeans_single_lloyd:
 * X N*F (centred by the caller, as KMeans.fit does), centers_init K*F (k-means++ seeding, drawn by
 * the caller from its RandomState), tol the absolute tolerance (KMeans' tol x mean feature
 * variance).  centers_out K*F, labels_out N, n_iter_out.  empty_out != 0: a cluster lost all its
 * members at iteration n_iter_out (scikit-learn then relocates it to the farthest sample): the
 * outputs are not set and the caller finishes with the library. */
int dlsm_init_kmeans_lloyd(dlsm_chain *h, const double *X, int N, int F, int K,
                           const double *centers_init, int max_iter, double tol, double *centers_out,
                           int32_t *labels_out, int32_t *n_iter_out, int32_t *empty_out);
/* free the hop matrices */
int dlsm_init_release(dlsm_chain *h);

/* ---- post-loop processing of the stored labels -------- */
/* _calculate_posterior_cooccurrences (hdp_lpcm.py:1180-1186, label_utils.py:40-62): zs is
 * the kept part of zs_ (zs_[n_burn:], S*T*N int64, labels < K); cooc_out (T*N*N, may be
 * NULL) = fraction of the S samples in which nodes i and j share a label at time t.  The
 * labels and the matrices stay on the device for dlsm_post_expected_vi_sums. */
int dlsm_post_cooccurrence(dlsm_chain *h, const int64_t *zs, int S, int K, double *cooc_out);
/* the sample-dependent sum of posterior_expected_vi (model_selection/posterior_vi.py:23-43):
 * out[t*S + s] = sum_i log2( sum_j cooc[t,i,j] [z_stj == z_sti] ) for every kept sample */
int dlsm_post_expected_vi_sums(dlsm_chain *h, double *out);
int dlsm_post_release(dlsm_chain *h);
/* The same processing straight from the device-resident trace of dlsm_hdp_run (rows
 * first .. first + count - 1 = the kept samples), so that fit() does not move the trace to the host
 * and back (hdp_lpcm.py:1085-1162):
 *   label_counts: nk count*T*K int32, nodes per label, time and sample - what approx_bic.py:26-51
 *     (models' sizes), posterior_vi.py:31-36 (the n_k log2 n_k term) and label_utils.py:73-81
 *     (posterior group counts) are computed from;
 *   cooccurrence: as dlsm_post_cooccurrence; cooc_out (T*N*N) and row_sums (T*N: sum_j C_t[i][j],
 *     posterior_vi.py:43) may be NULL; the matrices stay on the device for the VI sums and
 *     dlsm_post_get_cooccurrence;
 *   align: hdp_lpcm.py:1141-1146 - every row (positions and cluster means) rotated onto row
 *     `ref_row` by the orthogonal Procrustes rotation over all T N positions (procrustes.py:20-35,
 *     scipy.linalg.orthogonal_procrustes), in place on the device;
 *   mean: X_mean_ (T*N*D) = mean of the rows (hdp_lpcm.py:1149). */
int dlsm_post_trace_label_counts(dlsm_chain *h, int first, int count, int32_t *nk);
int dlsm_post_trace_cooccurrence(dlsm_chain *h, int first, int count, double *cooc_out,
                                 double *row_sums);
int dlsm_post_get_cooccurrence(dlsm_chain *h, double *cooc_out);
int dlsm_post_trace_align(dlsm_chain *h, int first, int count, int ref_row);
int dlsm_post_trace_mean(dlsm_chain *h, int first, int count, double *X_mean);
/* latent_marginal_loglikelihood (model_selection/approx_bic.py:54-76): forward algorithm over
 * the label chain of every node, at trace row `row` (row < 0: the handle's current positions);
 * init_w K, trans_w T*K*K (trans_w[0] unused), mu K*D, sigma K (variances), K <= 64 */
int dlsm_post_latent_marginal_loglik(dlsm_chain *h, int row, const double *init_w,
                                     const double *trans_w, const double *mu, const double *sigma,
                                     double lmbda, int K, double *out);

/* ---- one-step-ahead forecasts (undirected models) ------ */
/* the accumulation of forecast_probas / forecast_probas_pp_ (hdp_lpcm.py:555-626):
 * out[i,j] = (1/S) sum_s expit(intercepts[s] - |Xs[s,i] - Xs[s,j]|), Xs S*N*D the sampled
 * one-step-ahead positions (drawn by the caller: the draws keep the reference's MT19937
 * order), out N*N; zero_diag != 0 zeroes the diagonal as forecast_probas does. */
int dlsm_forecast_mean_probas(dlsm_chain *h, const double *Xs, const double *intercepts, int S,
                              int zero_diag, double *out);
/* marginal_forecast (forecast.pyx:79-128): out[i,j] = sum_s W[s,i] W[s,j]
 * expit(intercepts[s] - |x_i - x_j|) / sum_s W[s,i] W[s,j] for i != j, 0 on the diagonal;
 * x N*D the plug-in positions, W S*N the per-sample mixture densities of x_i (O(S N K), computed
 * by the caller: mixture_normal_pdf, forecast.pyx:39-54). */
int dlsm_forecast_marginal(dlsm_chain *h, const double *x, const double *W, const double *intercepts,
                           int S, double *out);

/* ---- posterior predictive goodness of fit ------------------------------ */
/* No reference counterpart (the check of latentnet's / ergm's gof()).  A record of R = 2 + 3N int64
 * per (sample, t): [0] edges (num_edges of network_statistics.py:13-14: undirected pairs, or
 * directed arcs), [1] mutual (pairs i < j with both arcs; 0 undirected), [2 + k] nodes of out-degree
 * k (undirected: the degree), [2 + N + k] nodes of in-degree k (0 undirected), [2 + 2N + k] edges
 * with k shared partners (undirected: pairs i < j with an edge, common neighbours; directed: arcs
 * i -> j, nodes m with i -> m -> j), k = 0..N-1.  Packed networks are [T][N][W] uint32, bit j % 32 of
 * word j / 32 of row i = Y[t, i, j], W = dlsm_network_packed_words / (T N) of an undirected handle
 * of the same N (a multiple of 4), padding bits zero. */
/* posterior predictive draws and their statistics: Xs S*T*N*D, intercepts S*2 (undirected models
 * read [s][0]; directed [s] = (intercept_in, intercept_out)), radii S*N (directed and case-control
 * handles; NULL otherwise); sample s uses RNG index first_index + s (Philox4x32-10 keyed by `seed`,
 * counter (min(i,j), max(i,j), index, t<<8|7): results do not depend on how the samples are split
 * across calls or batches); batch = samples per device batch (0: automatic, bounded scratch);
 * stats S*T*R int64; bits NULL or S*T*N*W uint32 (the drawn networks' rows).  Directed draws
 * (the exact model of metrics.py:57-60) for directed and case-control handles. */
int dlsm_gof_simulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii,
                      int S, uint64_t seed, uint32_t first_index, int batch, int64_t *stats,
                      uint32_t *bits);
/* the same statistics (no reference counterpart; edges as network_statistics.py:13-14) of a packed
 * network `bits` T*N*W uint32 supplied by the caller; stats T*R int64.  A set diagonal or padding
 * bit -> DLSM_E_DATA. */
int dlsm_gof_observed(dlsm_chain *h, const uint32_t *bits, int64_t *stats);
/* goodness of fit over time (no reference counterpart): the statistics of the same draws that look
 * across time steps and beyond two hops.  "Dyad": an unordered pair i < j of an undirected handle, an
 * arc i -> j of a directed or case-control handle (as `edges` above); all records int64.
 *   overlap  S*T*T: [t][u] dyads present at both t and u (symmetric; the diagonal is edges[t])
 *   steps    S*(T-1)*2N, per step t -> t+1: [k] nodes with k ties present at both t and t+1 (directed:
 *            out-arcs); [N + k] dyads absent at t and present at t+1 with k shared partners at t (the
 *            partner definition of the record above), k = 0..N-1
 *   geodesic S*T*N: [k] pairs at shortest-path length k = 1..N-1 (undirected: pairs i < j; directed:
 *            ordered pairs, paths along the arcs), [0] pairs without a path; N <= 32768, else DLSM_E_LIMIT
 * overlap and steps go together (steps may be NULL when T = 1); that pair or geodesic may be NULL and
 * is then not computed, both NULL -> DLSM_E_ARG.  Every other argument, check, the batching and the RNG
 * indexing are those of dlsm_gof_simulate: the same seed and first_index draw the same networks. */
int dlsm_gof_dynamic_simulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii,
                              int S, uint64_t seed, uint32_t first_index, int batch, int64_t *overlap,
                              int64_t *steps, int64_t *geodesic, uint32_t *bits);
/* the same records (S = 1) of a packed network `bits` T*N*W uint32 supplied by the caller, validated as
 * dlsm_gof_observed validates it. */
int dlsm_gof_dynamic_observed(dlsm_chain *h, const uint32_t *bits, int64_t *overlap, int64_t *steps,
                              int64_t *geodesic);
/* triad census of the same draws (no reference counterpart; the statistic of sna's triad.census and ergm's
 * triadcensus term).  A record of 51 int64 per (sample, t), summed over the connected pairs i < j - those
 * with at least one arc between them - of dyad code c = Y[i,j] + 2 Y[j,i] in {1, 2, 3}:
 *   [(c - 1) * 16 + a * 4 + b]  third nodes k (not i, not j) with a = Y[i,k] + 2 Y[k,i] and
 *                               b = Y[j,k] + 2 Y[k,j], a, b = 0..3
 *   [48 + c - 1]                connected pairs of code c
 * Undirected handles: only c = 3 and a, b in {0, 3} occur.  A triad with m non-null dyads is counted m
 * times; the host maps (c, a, b) to the 16 MAN classes and gets class 003 by subtraction from C(N, 3)
 * (dynetlsm_amd/gof.py).  triads S*T*51; every other argument, check, the batching and the RNG indexing are
 * those of dlsm_gof_simulate: the same seed and first_index draw the same networks. */
int dlsm_gof_triads_simulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii,
                             int S, uint64_t seed, uint32_t first_index, int batch, int64_t *triads,
                             uint32_t *bits);
/* the same records of a packed network `bits` T*N*W uint32 supplied by the caller, validated as
 * dlsm_gof_observed validates it; triads T*51 int64. */
int dlsm_gof_triads_observed(dlsm_chain *h, const uint32_t *bits, int64_t *triads);

/* ---- information criteria (WAIC, DIC) ----------------------------------- */
/* No reference counterpart.  The pointwise log-likelihood l_s = y eta_s - log(1 + exp(eta_s)) of every
 * dyad of the packed network `bits` (T*N*W uint32 as dlsm_gof_observed takes it; undirected handles: t,
 * i < j; directed and case-control handles: t, i != j, the exact model of metrics.py:57-60) at the S
 * samples Xs S*T*N*D, intercepts S*2, radii S*N (directed) or NULL, reduced over s in one pass:
 * lppd = log mean_s exp(l_s) (streaming log-sum-exp), var = the sample variance of l_s (Welford; 0 for
 * S = 1), mean = mean_s l_s.
 *   totals        T*5: per time step sum lppd, sum var, sum mean, sum (lppd - var)^2, number of dyads
 *   sample_loglik S*T: sum over the dyads of l_s - the network log-likelihood of sample s at time t
 *   pointwise     NULL or T*N*N*2: (lppd, var) of dyad (t, i, j); undirected: i < j filled, the rest 0
 * Every sum is taken in a fixed order (no floating-point atomics): the same call returns the same bits.
 * All S samples are held on the device at once; if they do not fit -> DLSM_E_LIMIT, and the message
 * names the largest S that does.  A set diagonal or padding bit, a radius <= 0 -> DLSM_E_DATA. */
int dlsm_ic_accumulate(dlsm_chain *h, const uint32_t *bits, const double *Xs, const double *intercepts,
                       const double *radii, int S, double *totals, double *sample_loglik,
                       double *pointwise);

/* ---- in-sample scores (AUC, log-loss of the posterior mean) ------------- */
/* No reference counterpart (metrics.py:10-24 sorts the probabilities of one sample on the host).  For every
 * dyad of the packed network `bits` (as dlsm_ic_accumulate takes it: the same dyads, the same linear predictor
 * eta, the same samples Xs S*T*N*D, intercepts S*2, radii S*N or NULL) whose bit in `mask` (NULL, or T*N*W
 * uint32 packed like the network; undirected handles: either of (i, j), (j, i)) is not set, the posterior-mean
 * probability pbar = mean_s expit(eta_s) in float64 and its rank key
 *   key = max(bits((float)pbar) >> 8, 0x200000)        (2^15 bins per octave; pbar <= 2^-63 share one bin)
 * are formed in one pass, and the keys are counted per class into histograms of 0x3F8000 - 0x200000 + 1 bins
 * in device memory (time steps in groups, within a fixed budget).  Nothing of size T*N*N is stored or sorted.
 *   counts      (T+1)*4 uint64: per time step, row T pooled over time, n_pos, n_neg (scored dyads with
 *               y = 1 / 0), u2 = sum_b pos_b (2 cumneg_b + neg_b) (twice the Mann-Whitney statistic of the
 *               keys, ties counted half: auc = u2 / (2 n_pos n_neg)) and ties = sum_b pos_b neg_b (the AUC of
 *               the keys is within ties / (2 n_pos n_neg) of the exact AUC of pbar)
 *   logloss_sum T: sum over the scored dyads of -[y log pbar + (1 - y) log(1 - pbar)], finite for any finite eta
 * The counts are exact integers (the same on every call, whatever the order of the atomics); the log-loss sums
 * are taken in a fixed order.  T*N*(N-1) (undirected: half) >= 2^32 dyads, or samples that do not fit the
 * device -> DLSM_E_LIMIT; a set diagonal or padding bit of `bits`, a radius <= 0 -> DLSM_E_DATA. */
int dlsm_score_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                          const double *intercepts, const double *radii, int S, uint64_t *counts,
                          double *logloss_sum);

/* ---- convergence of every dyad (split R-hat, batch-means ESS) ------------ */
/* No reference counterpart.  The linear predictor eta_s of every dyad (as dlsm_ic_accumulate forms it: the same
 * dyads, the same samples Xs S*T*N*D, intercepts S*2, radii S*N or NULL) is invariant to rotation, reflection,
 * translation and label switching, so its series can be pooled over chains.  The S = n_segments * seg_len samples
 * are the halves of the chains (n_segments = 2 * chains), segment after segment, each of seg_len samples in
 * iteration order.  Per dyad, in one pass and without storing the series (Welford's recurrences):
 *   W = mean over the segments of their variance (ddof 1), B = seg_len * variance of the segment means (ddof 1),
 *   var+ = (seg_len - 1) / seg_len * W + B / seg_len
 *   rhat = sqrt(var+ / W)                    (W == 0: 1 if B == 0, else +inf)
 *   v_bm = batch_len * variance (ddof 1) of the means of all batches: the samples [q batch_len, (q + 1) batch_len)
 *          of a segment, q < seg_len / batch_len (the tail of a segment enters no batch)
 *   ess  = S * var+ / v_bm                   (v_bm == 0: S if var+ == 0, else +inf; not capped at S)
 * Outputs (bin of a value: the number of edges <= it, so +inf falls into the last one):
 *   hist_rhat      T*(n_rhat_edges+1) uint64: dyads of time step t per bin of rhat_edges
 *   hist_ess       T*(n_ess_edges+1) uint64: the same for ess over ess_edges
 *   node_rhat_max  T*N: the largest rhat over the dyads that contain the node (directed: as sender or receiver);
 *                  0 for a node without a dyad (N = 1)
 *   node_ess_min   T*N: the smallest ess over the same dyads; +inf for a node without a dyad
 *   pointwise      NULL or T*N*N*2: (rhat, ess) of dyad (t, i, j); undirected: i < j filled, the rest 0
 * Only integer atomics are used: the same call returns the same bits.  n_segments odd or < 2, seg_len < 2,
 * batch_len outside 1..seg_len/2, more than 16 edges -> DLSM_E_ARG; edges that are not finite and ascending, a
 * radius <= 0 -> DLSM_E_DATA.  All S samples are held on the device at once; if they do not fit ->
 * DLSM_E_LIMIT, and the message names the largest S that does. */
int dlsm_convergence_accumulate(dlsm_chain *h, const double *Xs, const double *intercepts, const double *radii,
                                int n_segments, int seg_len, int batch_len, const double *rhat_edges,
                                int n_rhat_edges, const double *ess_edges, int n_ess_edges, uint64_t *hist_rhat,
                                uint64_t *hist_ess, double *node_rhat_max, double *node_ess_min,
                                double *pointwise);

/* ---- PSIS-LOO (Pareto-smoothed importance-sampling leave-one-out) -------- */
/* No reference counterpart.  For every dyad of the packed network `bits` (as dlsm_ic_accumulate takes it: the
 * same dyads, the same pointwise log-likelihood l_s, the same samples Xs S*T*N*D, intercepts S*2, radii S*N or
 * NULL), in one pass over the samples, PSIS as the R package loo does it with r_eff = 1:
 *   M = min(floor(S/5), ceil(3 sqrt(S))); lr_s = min_s l_s - l_s; the tail is the M largest lr, lr_cut the
 *   next one below.  With M >= 5, a tail that is not constant (lr_(M) - lr_(1) >= DBL_EPSILON/100) and a finite
 *   fit, the generalised Pareto fit of Zhang & Stephens 2009 to exp(lr) - exp(lr_cut) gives (k, sigma), k takes
 *   the adjustment (M k + 5)/(M + 10), and the tail's lr are replaced in their order by
 *   lw_(m) = min(0, log(exp(lr_cut) + sigma expm1(-k log1p(-p_m))/k)), p_m = (m - 0.5)/M.  Otherwise the dyad is
 *   unfitted: k = +inf and lw = lr (csrc/psis_tail.hpp).
 *   elpd_loo = logsumexp_s(lw_s + l_s) - logsumexp_s(lw_s),  lppd = logsumexp_s(l_s) - log S
 * Outputs (bin of a value: the number of edges <= it, so +inf falls into the last one):
 *   totals      T*5: per time step sum elpd_loo, sum elpd_loo^2, sum lppd, number of dyads, unfitted dyads
 *   hist_k      T*(n_edges+1) uint64: dyads of time step t per bin of k over k_edges
 *   node_k_max  T*N: the largest k over the dyads that contain the node (directed: as sender or receiver);
 *               -inf for a node without a dyad (N = 1)
 *   pointwise   NULL or T*N*N*2: (elpd_loo, k) of dyad (t, i, j); undirected: i < j filled, the rest 0
 * Every sum is taken in a fixed order and only integer atomics are used: the same call returns the same bits.
 * More than 16 edges -> DLSM_E_ARG; edges that are not finite and ascending, a set diagonal or padding bit, a
 * radius <= 0 -> DLSM_E_DATA.  All S samples are held on the device at once, and every dyad keeps its M + 1
 * smallest l_s in the LDS; if either does not fit -> DLSM_E_LIMIT, and the message names the largest S that
 * does. */
int dlsm_loo_accumulate(dlsm_chain *h, const uint32_t *bits, const double *Xs, const double *intercepts,
                        const double *radii, int S, const double *k_edges, int n_edges, double *totals,
                        uint64_t *hist_k, double *node_k_max, double *pointwise);

/* ---- posterior edge probabilities (credible intervals, calibration) ------ */
/* No reference counterpart.  For every dyad of the handle (undirected: t, i < j; directed and case-control: t,
 * i != j; the same linear predictor eta, the same samples Xs S*T*N*D, intercepts S*2, radii S*N or NULL as
 * dlsm_score_accumulate takes them), of p_s = expit(eta_s) over the S samples, in one pass:
 *   mean = pbar, sd (ddof 1), and the equal-tailed interval at `level`: lower and upper are the quantiles at
 *   alpha = (1 - level)/2 and at 1 - alpha as numpy's default defines them - linear interpolation of the order
 *   statistics at position (S - 1) q.  Every dyad keeps its K = min(floor(alpha (S - 1)) + 2, S) smallest and its
 *   K largest eta_s sorted in the LDS; expit is monotone, so the interpolation is on p.
 * The dyads whose bit in `mask` (NULL, or T*N*W uint32 packed like the network `bits`; undirected handles: either of
 * (i, j), (j, i)) is not set are scored against y = their bit of `bits`.  With fix(x) = llrint(x 2^32), over the
 * scored dyads of time step t:
 *   calib       T*n_bins*3 uint64: per bin b = min(floor(pbar n_bins), n_bins - 1) the dyads, those with y = 1, and
 *               sum fix(pbar)
 *   brier       T uint64: sum fix((y - pbar)^2)
 *   node_sums   T*N*2 uint64: fix(pbar) of dyad (i, j) is added to slot 0 of node i and to slot 1 of node j (directed:
 *               expected out- and in-degree; undirected: the dyads are i < j, and the two slots add up to the degree)
 *   hist_width  T*(n_edges+1) uint64: dyads per bin of upper - lower over width_edges (bin of a value: the number of
 *               edges <= it)
 *   pointwise   NULL or T*N*N*4: (mean, sd, lower, upper) of every dyad (t, i, j), scored or not; undirected: i < j
 *               filled, the rest 0
 * Everything accumulated across dyads is an integer added with 64-bit atomics: the same call returns the same bits,
 * whatever the order, with and without `pointwise`.  The fixed point costs at most half a unit of 2^-32 per dyad.
 * S < 2, level outside (0, 1), n_bins outside 1..64, more than 16 edges -> DLSM_E_ARG; edges that are not finite and
 * ascending, a set diagonal or padding bit of `bits`, a radius <= 0 -> DLSM_E_DATA.  2^31 or more dyads per time step
 * (the sums stay below 2^63), samples that do not fit the device, or two columns of K values that do not fit the LDS
 * (K <= 144) -> DLSM_E_LIMIT; for the samples and the columns the message names the largest S that fits at this
 * level. */
int dlsm_proba_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                          const double *intercepts, const double *radii, int S, double level, int n_bins,
                          const double *width_edges, int n_edges, uint64_t *calib, uint64_t *brier,
                          uint64_t *node_sums, uint64_t *hist_width, double *pointwise);

/* ---- tie dynamics (posterior change of the edge probabilities between steps) ---- */
/* No reference counterpart.  A step u = t -> t + 1 (u = 0 .. T - 2) of a dyad of the handle (undirected: i < j;
 * directed and case-control: i != j; the same linear predictor eta, the same samples Xs S*T*N*D, intercepts S*2,
 * radii S*N or NULL as dlsm_proba_accumulate takes them), with p_{s,t} = expit(eta_{s,t}), over the S samples in one
 * pass - the joint posterior of two consecutive time steps:
 *   delta_mean, delta_sd (ddof 1) of d_s = p_{s,t+1} - p_{s,t}
 *   up = the samples with eta_{s,t+1} > eta_{s,t}, down = those with < (a tie counts as neither);
 *   prob_up = up / S, prob_down = down / S
 *   persist = mean_s p_{s,t} p_{s,t+1}, and the marginals pbar_t, pbar_{t+1}
 * Both etas of a step come from the same instructions: they are equal exactly when the two time steps' inputs are.
 * A step of a dyad is scored when its bit in `mask` (NULL, or T*N*W uint32 packed like the network `bits`; undirected
 * handles: either of (i, j), (j, i)) is set neither at t nor at t + 1.  With fix(x) = llrint(x 2^32), over the scored
 * steps u:
 *   transitions    (T-1)*4*4 uint64: per observed class c = 2 y_t + y_{t+1} the dyads, sum fix(pbar_t),
 *                  sum fix(pbar_{t+1}) and sum fix(persist)
 *   hist_up        (T-1)*n_bins uint64: dyads per bin b = min(up * n_bins / S, n_bins - 1), in integer arithmetic
 *   node_changes   (T-1)*N*4 uint64: dyad (i, j) with up >= min_count adds 1 to slot 0 of node i and to slot 1 of
 *                  node j, with down >= min_count to slot 2 of i and slot 3 of j
 *   node_turnover  (T-1)*N*2 uint64: fix(|delta_mean|) is added to slot 0 of node i and to slot 1 of node j (the
 *                  convention of node_sums of dlsm_proba_accumulate)
 *   pointwise      NULL or (T-1)*N*N*4: (delta_mean, delta_sd, prob_up, prob_down) of every dyad (u, i, j), scored or
 *                  not; undirected: i < j filled, the rest 0
 * Everything accumulated across dyads is an integer added with 64-bit atomics: the same call returns the same bits,
 * whatever the order, with and without `pointwise`.  The fixed point costs at most half a unit of 2^-32 per dyad.
 * S < 2, a handle with T < 2, min_count outside 1..S, n_bins outside 1..64, radii NULL on a directed handle ->
 * DLSM_E_ARG; a set diagonal or padding bit of `bits`, a radius <= 0 -> DLSM_E_DATA.  2^31 or more dyads per time
 * step (the sums stay below 2^63), or samples that do not fit the device -> DLSM_E_LIMIT; for the samples the message
 * names the largest S that fits. */
int dlsm_dynamics_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                             const double *intercepts, const double *radii, int S, int min_count, int n_bins,
                             uint64_t *transitions, uint64_t *hist_up, uint64_t *node_changes,
                             uint64_t *node_turnover, double *pointwise);

/* ---- link prediction (top-k dyads by posterior edge probability) --------- */
/* No reference counterpart (probas_ of one selected sample and a dense argsort on the host).  For every time step t,
 * over the eligible dyads of the handle (undirected: i < j; directed and case-control: i != j), with
 *   pbar(t, i, j) = (1/S) sum_s expit(eta_s)      (eta and the samples Xs S*T*N*D, intercepts S*2, radii S*N or NULL as
 *                                                  dlsm_score_accumulate takes them; s = 0 .. S-1 in order)
 * the dyads that can be among the k first in the total order (pbar descending, i ascending, j ascending; largest = 0:
 * pbar ascending, i, j) are returned, each with its pbar, the standard deviation (ddof 1, Welford) of p_s =
 * expit(eta_s) and its bit y of the packed network `bits` (T*N*W uint32).  Eligible (`among`), with "observed" = the
 * dyad's bit of `mask` (NULL, or T*N*W uint32 packed like the network; undirected handles: either of (i, j), (j, i))
 * is not set:
 *   0 observed and y = 0 (predicted links)    1 observed and y = 1 (implausible ties)    2 observed
 *   3 masked (needs `mask`)                   4 every dyad
 * Selection is by the rank key of dlsm_score_accumulate, key = max(bits((float)pbar) >> 8, 0x200000), which never
 * decreases with pbar: a first pass over the samples counts the keys of the eligible dyads per time step into a
 * histogram in device memory (time steps in groups, within a fixed budget) and keeps the extreme key of every tile of
 * 32 x 64 dyads (n_features > 4: 16 x 64); a scan finds the key kappa_t with
 *   n_beyond_t = count(keys beyond kappa_t) < k <= n_beyond_t + n_at_t,   n_at_t = count(keys equal to kappa_t)
 * (fewer than k eligible dyads: kappa_t is the last key that is not empty, and all of them are returned); a second
 * pass over the tiles whose extreme key reaches kappa_t writes the n_beyond_t + n_at_t dyads whose key does.  The
 * caller sorts them by (pbar, i, j) and keeps k: they are written in no particular order.  Nothing of size T*N*N is
 * stored or sorted.
 *   cand_index  T*max_candidates*4 int32: (i, j, y, 0) of the dyads of time step t in its first n_cand[t] rows
 *   cand_value  T*max_candidates*2: (pbar, sd) of the same rows
 *   n_cand      T int32: = n_beyond_t + n_at_t
 *   diag        T*5 int64: eligible_t, n_beyond_t, n_at_t, kappa_t (-1: no eligible dyad) and the tiles of the time step
 *               that the second pass visited
 * The counts are exact integers and both passes form pbar with the same instructions: the same call returns the same
 * set of rows.  S < 2, among outside 0..4, largest not 0 or 1, k < 1, max_candidates < k, among = 3 without a mask ->
 * DLSM_E_ARG; a set diagonal or padding bit of `bits`, a radius <= 0 -> DLSM_E_DATA.  n_beyond_t + n_at_t >
 * max_candidates for some t (more dyads share the key of the k-th than there is room for; the message names t, the
 * count and max_candidates), 2^31 or more dyads per time step, or samples that do not fit the device -> DLSM_E_LIMIT. */
int dlsm_topk_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                         const double *intercepts, const double *radii, int S, int among, int largest, int64_t k,
                         int64_t max_candidates, int32_t *cand_index, double *cand_value, int32_t *n_cand,
                         int64_t *diag);

/* ---- per-node link prediction (each node's top-k partners) ---------------- */
/* No reference counterpart.  For every time step t and every node i of the listed row blocks, over the eligible
 * partners j != i (`among`, `mask`, pbar, sd, y and the samples as dlsm_topk_accumulate; 2 <= S), the k first in the
 * order (pbar(t, i, j) descending, j ascending; largest = 0: pbar ascending, j ascending), 1 <= k <= 64.  Directed and
 * case-control handles rank the receivers j of sender i by p(i -> j); the senders of a receiver are ranked by the same
 * call on the transposed network and mask with the two intercept columns swapped.  Undirected handles visit both
 * triangles (about N*N dyad evaluations per sample and time step); the bit of the network and of the mask of {i, j} are
 * those of (min(i, j), max(i, j)), either orientation of the mask excluding the dyad, and a dyad has the same pbar and
 * sd in both of its rows.  pbar and sd have the bits that dlsm_topk_accumulate returns for the dyad.  A row's list is
 * kept sorted in the registers of one wavefront while its columns stream by: nothing of size T*N*N is stored or sorted.
 *   row_blocks  NULL: every row; else n_row_blocks strictly ascending blocks of 32 rows (n_features > 4: 16 rows) in
 *               0 .. ceil(N / rows of a block) - 1: only their rows are computed
 *   partner     T*N*k int32: the partners of node i at t in rank order, then -1
 *   value       T*N*k*2: (pbar, sd) of the same entries, then NaN
 *   y           T*N*k int32: their bits of the network, then -1
 *   eligible    T*N int32: the eligible partners of the row; -1 for the rows of blocks that are not listed (all padding)
 * S < 2, among outside 0..4, largest not 0 or 1, k outside 1..64, among = 3 without a mask, row_blocks not ascending or
 * out of range -> DLSM_E_ARG; a set diagonal or padding bit of `bits`, a radius <= 0 -> DLSM_E_DATA; samples that do
 * not fit the device -> DLSM_E_LIMIT. */
int dlsm_partners_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const double *Xs,
                             const double *intercepts, const double *radii, int S, int among, int largest, int k,
                             const int32_t *row_blocks, int n_row_blocks, int32_t *partner, double *value,
                             int32_t *y, int32_t *eligible);

/* ---- community structure of stored labellings ---------------------------- */
/* The reference has modularity(Y, z) for one labelling on the host (network_statistics.py:31-61); the rest has no
 * counterpart.  zs S*T*N int64 labels in [0, K), 1 <= K <= 256 (packed to bytes on the device, staged in batches of
 * `batch` samples, 0: automatic; no table depends on it); bits T*N*W uint32 the packed network (undirected handles:
 * symmetric), mask NULL or the excluded dyads packed alike - its diagonal and padding bits are ignored, and on an
 * undirected handle a dyad is excluded when either of (i, j), (j, i) is set.  A tie is a set bit (i, j) of `bits` whose
 * dyad is not excluded; every count is of ordered pairs (an undirected tie counts twice).  With a = z[s][t][i]:
 *   clusters     S*T*K*5 int64, per labelling (s, t) and cluster a: the nodes with label a; the ties (i, j) with
 *                z_i = z_j = a; the out-volume, ties (i, j) with z_i = a; the in-volume, ties (i, j) with z_j = a
 *                (undirected: the out-volume again); the excluded ordered dyads i != j with z_i = z_j = a
 *   node_within  T*N int64: over the S samples, the ties (i, j) of node i with z_j = z_i
 *   node_switch  (T-1)*N int64: the samples with z[s][t+1][i] != z[s][t][i]
 *   moved        S*(T-1) int64: the nodes i with z[s][t+1][i] != z[s][t][i]
 *                (T = 1: both are empty and may be NULL)
 *   blocks       NULL or S*T*K*K*2 int64: per labelling and ordered pair of clusters (a, b) the ties (i, j) with
 *                z_i = a, z_j = b, and the excluded ordered dyads i != j with z_i = a, z_j = b
 * Everything added across workgroups is an integer added with an atomic: the same call returns the same tables,
 * whatever the order and the batch.  S < 1, K outside 1..256, batch < 0 -> DLSM_E_ARG; a label outside [0, K), a set
 * diagonal or padding bit of `bits`, an undirected network that is not symmetric -> DLSM_E_DATA, all before any
 * device work; N beyond what a workgroup's LDS holds of labels (some 40 000) -> DLSM_E_LIMIT. */
int dlsm_community_accumulate(dlsm_chain *h, const uint32_t *bits, const uint32_t *mask, const int64_t *zs, int S,
                              int K, int batch, int64_t *clusters, int64_t *node_within, int64_t *node_switch,
                              int64_t *moved, int64_t *blocks);

/* ---- multi-step posterior predictive forecasts --------------------------- */
/* The reference has only the one-step undirected form (hdp_lpcm.py:555-626, drawn on the host).  One
 * trajectory of H future time steps per sample s, started at the sample's last time step X0 S*N*D:
 *   random walk (z0 == NULL, K = 0):  x_h = x_{h-1} + sqrt(sigma_sq) eps
 *   mixture (z0 S*N int32 labels of the last step, trans S*K*K raw transition rows - the device divides by
 *   the row sum -, mu S*K*D, sigma S*K variances, lmbda S):
 *       z_h ~ Categorical(trans[s][z_{h-1}][:]),  x_h = lmbda mu[z_h] + (1 - lmbda) x_{h-1} + sqrt(sigma[z_h]) eps
 * and probas H*N*N: probas[h][i][j] = (1/S) sum_s expit(eta_s(h, i, j)), eta = b - |x_i - x_j| for undirected
 * handles (intercepts S*2, [s][0] read) and the directed model of metrics.py:57-60 with the sample's
 * intercepts and radii S*N, held fixed over the horizon, for directed and case-control handles; diagonal 0.
 * Sample s uses RNG index first_index + s: Philox4x32-10 keyed by `seed` at counter (node, h | draw << 16,
 * index, 9), h = 1..H; draw 0 gives the label uniform (the label is the smallest k with u * c_{K-1} <= c_k,
 * c the running sum of the row), draw 1 + d/2 the Box-Muller pair of coordinates d, d + 1.  Results do not
 * depend on how the samples are split across calls or batches (batch = samples per device batch, 0:
 * automatic, bounded scratch; probas is the mean over the S samples of the call).
 *   paths   NULL or S*H*N*D: the drawn positions
 *   labels  NULL or S*H*N int32: the drawn labels (mixture only)
 * H outside 1..65535, K < 1 for the mixture, first_index + S > 2^32 -> DLSM_E_ARG; a label outside [0, K), a
 * radius <= 0, a sigma < 0, a negative weight or a row sum that is not positive -> DLSM_E_DATA. */
int dlsm_forecast_paths(dlsm_chain *h, const double *X0, const double *intercepts, const double *radii,
                        const int32_t *z0, const double *trans, const double *mu, const double *sigma,
                        const double *lmbda, int K, double sigma_sq, int H, int S, uint64_t seed,
                        uint32_t first_index, int batch, double *probas, double *paths, int32_t *labels);

/* ---- missing dyads: the data-augmentation step --------------------------- */
/* lsm.py:525-545 / hdp_lpcm.py:1025-1049 draw y_ij ~ Bernoulli(p_ij) for the -1 coded dyads every
 * iteration (their write-back into the network is lost in a fancy-index copy; hdp_lpcm.py:1155-1156
 * averages the draws into missings_).  Here the draw lands in every copy of the packed network, so the
 * next sweep and likelihood pass condition on it: the chain targets the posterior given the observed
 * dyads alone.  The uniform of a dyad is Philox4x32-10 keyed by the chain's seed at counter
 * (min(i,j) | (t & 255) << 24, max(i,j) | (t >> 8) << 24, iteration, chain << 8 | 8): an undirected
 * dyad takes the first 53-bit uniform, the arc i -> j the first when i < j and the second otherwise;
 * bit = u < p, p = expit(b - d) or the directed model of metrics.py:57-60.  A draw depends on (seed,
 * chain, iteration, t, pair) alone. */
/* the missing dyads (lsm.py:345-359's nan mask as a list): n triples (t, i, j), i < j for the undirected
 * model, i != j for the directed one; n = 0 clears the list and switches the sampling off.  Needs the
 * network uploaded (the estimators impute the -1 entries once for it, imputer.py).  An entry out of
 * range, off its triangle or listed twice -> DLSM_E_DATA; a case-control chain (it holds edge lists)
 * -> DLSM_E_ARG; N >= 2^24 or n >= 2^30 -> DLSM_E_LIMIT.  Zeroes the accumulators. */
int dlsm_set_missing(dlsm_chain *h, const int32_t *tij, int64_t n);
/* the same list (lsm.py:345-359's nan mask, read by the step of lsm.py:525-545) as pairs: those of time step t
 * are src / dst[offsets[t] .. offsets[t+1]), int32 node ids in any order, duplicates allowed.  The undirected
 * model reads a pair in either orientation as the dyad {i, j}, the directed one as the arc i -> j.  Leaves
 * exactly the tables dlsm_set_missing leaves for the distinct dyads in row-major (t, i, j) order, i < j
 * undirected - the order of the accumulators and of dlsm_get_missing_index -, built on the device with nothing
 * sorted.  allow_ties == 0: a listed dyad that is a tie of the uploaded network is an error (a held-out tie
 * must have left the edge list); != 0: no such check (the network already holds imputed values).  A node id
 * outside 0..N-1, src == dst or such a tie -> DLSM_E_DATA; a case-control chain, no network or bad offsets ->
 * DLSM_E_ARG; N >= 2^24 or 2^30 dyads -> DLSM_E_LIMIT.  offsets all 0 clears the list and switches the
 * sampling off; a failed call leaves the network and no list at all. */
int dlsm_set_missing_edges(dlsm_chain *h, const int64_t *offsets, const int32_t *src, const int32_t *dst,
                           int allow_ties);
/* the number of dyads either call left (0: none set) */
int dlsm_missing_count(dlsm_chain *h, int64_t *n);
/* the list in the accumulators' order (lsm.py:345-359, :525-545: what the reference indexes its draws with):
 * tij [n][3] rows (t, i, j), after dlsm_set_missing the caller's own rows.  Waits for the handle's stream. */
int dlsm_get_missing_index(dlsm_chain *h, int32_t *tij);
/* one step (lsm.py:525-545, hdp_lpcm.py:1039-1049) at the handle's current positions, intercepts and
 * radii with the draws of iteration `iter`; accumulate != 0 adds p and the drawn bit of every dyad to
 * the accumulators.  Enqueued on the handle's stream. */
int dlsm_impute_missing(dlsm_chain *h, uint32_t iter, int accumulate);
/* on != 0: dlsm_lsm_run ends every iteration `it` with the step, after the trace row of `it` is written
 * and from exactly the state that row stores (lsm.py:525-545 sits at the same place of the loop), and
 * accumulates when it > accumulate_after (hdp_lpcm.py:1046: the burn-in; < 0: always).  While it is on
 * dlsm_hdp_run returns DLSM_E_ARG: that loop has no imputation step. */
int dlsm_missing_sampling(dlsm_chain *h, int on, int accumulate_after);
/* the accumulators in the order of the list given to dlsm_set_missing: p_sum n (sum of p_ij), ones n
 * (drawn ones: hdp_lpcm.py:1046-1049's missings_ before its division), n_accumulated the steps that
 * accumulated; any pointer may be NULL.  Waits for the handle's stream. */
int dlsm_get_missing(dlsm_chain *h, double *p_sum, uint32_t *ones, int64_t *n_accumulated);
/* zero the accumulators and the step count (hdp_lpcm.py:699-706 allocates missings_ as zeros) */
int dlsm_reset_missing_sums(dlsm_chain *h);

/* ---- host-stream auxiliary draws ----------------------- */
/* sample_tables (sample_auxillary.py:6-28): m T*K*K int64 = tables per (restaurant, dish)
 * given the transition counts n T*K*K (n[0,0,:] = initial counts) and beta K.  The
 * Bernoulli draws come from the CALLER's numpy RandomState, in the reference's order:
 * numpy_bitgen is the address of its bitgen_t (RandomState._bit_generator.ctypes.bit_generator).
 * Runs on the host; needs no chain.  -1: a probability outside [0, 1] (numpy raises there). */
int dlsm_host_sample_tables(void *numpy_bitgen, int T, int K, const double *n, const double *beta,
                            double alpha_init, double alpha, double kappa, int64_t *m);

/* ---- measurement ------------------------------------------------------ */
enum {
    DLSM_K_LOGLIK = 0, DLSM_K_SWEEP = 1, DLSM_K_CENTER = 2, DLSM_K_LABELS = 3,
    DLSM_K_FINALIZE = 4,
    DLSM_K_SWEEP_EVAL = 5,     /* k_spec_eval launches of the speculative sweep */
    DLSM_K_SWEEP_RESOLVE = 6,  /* k_spec_resolve launches */
    DLSM_K_INIT = 7,           /* every kernel of the dlsm_init_* calls */
    DLSM_K_HDP_TAIL = 8,       /* dlsm_hdp_run: everything after the label update */
    DLSM_K_SCORE_ACCUMULATE = 9,   /* dlsm_score_accumulate: k_score_accumulate (sample loop + histogram) */
    DLSM_K_SCORE_CLEAR = 10,       /* ... the histograms' hipMemsetAsync */
    DLSM_K_SCORE_SCAN = 11,        /* ... k_score_scan (pooling included) and the log-loss reduction */
    DLSM_K_TOPK_COUNT = 12,        /* dlsm_topk_accumulate: k_topk_count and the histograms' hipMemsetAsync */
    DLSM_K_TOPK_SCAN = 13,         /* ... k_topk_threshold */
    DLSM_K_TOPK_EMIT = 14,         /* ... k_topk_emit */
    DLSM_K_PARTNERS = 15,          /* dlsm_partners_accumulate: k_partners_select */
    DLSM_K_COUNT = 16
};
/* when enabled every launch of the kernel classes above is bracketed by HIP
 * events on the handle's stream; read returns accumulated ms and launches */
int dlsm_profile_enable(dlsm_chain *h, int on);
int dlsm_profile_read(dlsm_chain *h, int kernel, double *total_ms, int *launches);
/* while profiling, the sweep's dominant kernel (k_spec_eval) also stamps the 100 MHz
 * wall clock in-kernel (min start / max end over its workgroups): mean duration in us
 * without the dispatch latency that brackets of HIP events include */
int dlsm_profile_read_eval_stamps(dlsm_chain *h, double *mean_us, int *launches);
/* wall-clock of a region on the handle's stream, by HIP events */
int dlsm_timer_start(dlsm_chain *h);
int dlsm_timer_stop(dlsm_chain *h, double *ms);

#ifdef __cplusplus
}
#endif
#endif
