"""Host restatement of the post-loop processing of the stored trace (numpy; integers for the counts,
np.longdouble for everything that is rounded), written from the definitions in oracle/post_oracle.py
and independently of dynetlsm_amd/csrc/kernels_post.hpp: label counts and co-occurrence counts, the
sample-dependent sum of the expected-VI criterion, the scaled forward algorithm of the latent marginal
likelihood and the posterior mean of the positions; and the synthetic traces the shape tests run on.

TEST INFRASTRUCTURE ONLY."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble


def synthetic_trace(T, N, D, K, S, seed, flip=0.3, n_labels=None):
    """A stored trace of S samples with well-conditioned values: ``Y`` (T, N, N) symmetric 0/1, ``Xs``
    (S, T, N, D), ``zs`` (S, T, N) int64, ``mus`` (S, K, D), ``sigmas`` (S, K) in [0.5, 2] (variances),
    ``betas`` (S, K) and ``weights`` (S, T, K, K) with Dirichlet rows, ``lambdas`` (S, 1), ``intercepts``
    (S, 1), ``logps`` (S,).

    The labels of a sample are one partition shared by the trace with a fraction ``flip`` of the nodes
    redrawn, so that the co-occurrence counts take many values; ``n_labels`` (S,) folds the labels of sample
    s into 0 .. n_labels[s] - 1 (samples that use different numbers of components).  The positions are
    drawn from the mixture they are scored under: X_0 ~ N(mu_z, sigma_z), X_t ~ N(lambda mu_z +
    (1 - lambda) X_{t-1}, sigma_z), which keeps every normaliser of the forward algorithm far from
    underflow."""
    rng = np.random.RandomState(seed)
    Y = (rng.rand(T, N, N) < 0.2).astype(np.float64)
    Y = np.triu(Y, 1)
    Y = Y + Y.transpose(0, 2, 1)
    base = rng.randint(0, K, size=(T, N))
    redraw = rng.rand(S, T, N) < flip
    zs = np.where(redraw, rng.randint(0, K, size=(S, T, N)), base[None]).astype(np.int64)
    if n_labels is not None:
        zs = zs % np.asarray(n_labels, dtype=np.int64)[:, None, None]
    mus = rng.randn(S, K, D) * 2.0
    sigmas = rng.uniform(0.5, 2.0, size=(S, K))
    betas = rng.dirichlet(np.ones(K), size=S)
    weights = rng.dirichlet(np.ones(K), size=(S, T, K))
    lambdas = rng.uniform(0.5, 0.95, size=(S, 1))
    intercepts = rng.randn(S, 1) * 0.1 + 0.5
    logps = rng.randn(S) * 10
    Xs = np.empty((S, T, N, D))
    sid = np.arange(S)[:, None]
    for t in range(T):
        m = mus[sid, zs[:, t]]                                    # (S, N, D)
        sd = np.sqrt(sigmas[sid, zs[:, t]])[:, :, None]
        if t > 0:
            lm = lambdas[:, :, None]
            m = lm * m + (1 - lm) * Xs[:, t - 1]
        Xs[:, t] = m + sd * rng.randn(S, N, D)
    return SimpleNamespace(Y=Y, Xs=Xs, zs=zs, mus=mus, sigmas=sigmas, betas=betas, weights=weights,
                           lambdas=lambdas, intercepts=intercepts, logps=logps, T=T, N=N, D=D, K=K, S=S)


def label_counts(zs, K):
    """(S, T, K): nodes carrying label k at time t of sample s"""
    return np.stack([[np.bincount(z_t, minlength=K) for z_t in z] for z in zs])


def cooccurrence_counts(zs, K):
    """(T, N, N) int64: the number of samples in which nodes i and j share a label at time t, by one-hot
    products per label (0/1 products summed in float64 are exact far beyond any sample count)"""
    S, T, N = zs.shape
    out = np.zeros((T, N, N), dtype=np.int64)
    for t in range(T):
        acc = np.zeros((N, N))
        for k in range(K):
            ind = (zs[:, t] == k).astype(np.float64)              # (S, N)
            acc += ind.T.dot(ind)
        out[t] = np.rint(acc).astype(np.int64)
        assert (out[t] == acc).all()
    return out


def cooccurrence_probas(counts, S):
    """count / n_samples: one division (label_utils.py:62), in float64 as the trace keeps them"""
    return counts.astype(np.float64) / float(S)


def vi_sums(zs, cooc, samples=None):
    """(T, len(samples)) np.longdouble: sum_i log2( sum_j C_t[i][j] [z_stj == z_sti] ) of the samples
    ``samples`` (all of them by default) of ``zs`` (S, T, N); ``cooc`` (T, N, N) probabilities"""
    S, T, N = zs.shape
    samples = np.arange(S) if samples is None else np.asarray(samples)
    C = np.asarray(cooc, dtype=LD)
    out = np.zeros((T, samples.shape[0]), dtype=LD)
    for q, s in enumerate(samples):
        for t in range(T):
            z = zs[s, t]
            same = z[:, None] == z[None, :]
            out[t, q] = np.log2(np.where(same, C[t], LD(0)).sum(axis=1)).sum()
    return out


def forward_loglik(X, init_w, trans_w, mu, sigma, lmbda):
    """approx_bic.py:54-76 in np.longdouble throughout: the scaled forward algorithm over the label chain of
    every node, sum over nodes and times of the log normalisers.  X (T, N, D), init_w (K,), trans_w
    (T, K, K) (row j: from label j), mu (K, D), sigma (K,) variances."""
    X = np.asarray(X, dtype=LD)
    init_w, trans_w = np.asarray(init_w, dtype=LD), np.asarray(trans_w, dtype=LD)
    mu, sigma = np.asarray(mu, dtype=LD), np.asarray(sigma, dtype=LD)
    lmbda = LD(np.ravel(lmbda)[0])
    T, N, D = X.shape
    two_pi = LD(8) * np.arctan(LD(1))
    lognorm = -LD(D) / LD(2) * np.log(two_pi * sigma)             # (K,)
    ll = LD(0)
    f = None
    for t in range(T):
        mean = mu[None] if t == 0 else lmbda * mu[None] + (LD(1) - lmbda) * X[t - 1][:, None, :]
        ss = ((X[t][:, None, :] - mean) ** 2).sum(axis=2)         # (N, K)
        g = np.exp(lognorm[None] - ss / (LD(2) * sigma[None]))
        if t == 0:
            f = init_w[None] * g
        else:
            f = g * (f[:, :, None] * trans_w[t][None]).sum(axis=1)
        c = f.sum(axis=1)
        ll += np.log(c).sum()
        f = f / c[:, None]
    return ll


def trace_mean(Xs):
    """(mean, sum_s |x_s|) per element of the samples Xs (S, ...), in np.longdouble"""
    X = np.asarray(Xs, dtype=LD)
    return X.sum(axis=0) / LD(X.shape[0]), np.abs(X).sum(axis=0)


# ---- the shapes of tests/test_gpu_post_shapes.py (the smallest that cross each boundary of the kernels) and
# the traces they run on; tests/test_post_ref_cpu.py checks this file against the oracle at the same inputs
LABEL_CASES = [(1, 5, 1, 4, 0, 4), (3, 256, 33, 6, 1, 5), (2, 257, 64, 9, 3, 6),
               (1, 513, 64, 4, 1, 3)]                             # (T, N, K, stored, first, count)
COOC_CASES = [(3, 64, 2, 1, 3), (2, 65, 3, 7, 65), (2, 129, 64, 5, 67), (1, 257, 7, 0, 130)]  # (T, N, K, first, count)
FORWARD_CASES = [(1, 5, 1, 1), (5, 9, 2, 2), (4, 66, 3, 33), (3, 257, 5, 63), (6, 131, 8, 64)]    # (T, N, D, K)
MEAN_SHAPE, MEAN_FIRST, MEAN_COUNTS = (2, 65, 3), 2, (1, 63, 64, 65, 130, 200)
LONG_CASE = dict(T=1, N=5, D=1, K=2, stored=70003, first=3, count=70000)
LONG_VI_SAMPLES = (0, 63, 64, 65535, 65536, 69999)
STAGED_CASE = dict(T=1, N=64, K=3, S=131072 + 70)
STAGED_VI_SAMPLES = (0, 131071, 131072, 131072 + 69)
SELECT_CASE = dict(T=2, N=130, D=2, K=9, n_burn=10, kept=80)


def label_trace(T, N, K, stored, first, count):
    return synthetic_trace(T, N, 1, K, stored, seed=1000 + N + K)


def cooc_trace(T, N, K, first, count):
    """first + count + 2 stored samples; the rows outside first .. first + count - 1 carry labels drawn
    uniformly (another distribution than the kept ones: they must not matter); the last kept sample is made
    a copy of the first kept one"""
    stored = first + count + 2
    tr = synthetic_trace(T, N, 2, K, stored, seed=2000 + N + K)
    rng = np.random.RandomState(N * 7 + K)
    outside = np.r_[0:first, first + count:stored]
    tr.zs[outside] = rng.randint(0, K, size=(outside.shape[0], T, N))
    tr.zs[first + count - 1] = tr.zs[first]
    tr.first, tr.count = first, count
    return tr


def forward_case(T, N, D, K):
    """a three-sample trace and the parameters of its row 2: (trace, row, init_w, trans_w, mu, sigma, lmbda)"""
    tr = synthetic_trace(T, N, D, K, 3, seed=3000 + N + K)
    row = 2
    return tr, row, tr.weights[row, 0, 0], tr.weights[row], tr.mus[row], tr.sigmas[row], tr.lambdas[row]


def without_component(k, init_w, trans_w, mu, sigma):
    """((K parameters in which component k has no mass), (the K - 1 parameters without it)): zero initial
    weight and zero incoming transition column, the rest renormalised"""
    keep = np.delete(np.arange(sigma.shape[0]), k)
    iw = init_w.copy()
    iw[k] = 0.0
    iw /= iw.sum()
    tw = trans_w.copy()
    tw[:, :, k] = 0.0
    tw /= tw.sum(axis=2, keepdims=True)
    return (iw, tw, mu, sigma), (iw[keep], tw[:, keep][:, :, keep], mu[keep], sigma[keep])


def select_trace():
    """samples that use 3 .. 9 components (the model sizes of the BIC table), distinct partitions"""
    c = SELECT_CASE
    S = c['n_burn'] + c['kept']
    n_labels = 3 + np.arange(S) % 7
    return synthetic_trace(c['T'], c['N'], c['D'], c['K'], S, seed=4000, n_labels=n_labels)


def assembled_vi(zs_kept, counts):
    """posterior_vi.py:23-52 of every kept sample, assembled in np.longdouble from this file's parts:
    the time average of (1/N) [ sum_k n_k log2 n_k - 2 vi_sum + sum_i log2 sum_j C_ij ]"""
    S, T, N = zs_kept.shape
    K = int(zs_kept.max()) + 1
    C = cooccurrence_probas(counts, S)
    nk = label_counts(zs_kept, K).astype(LD)                      # (S, T, K)
    t1 = np.where(nk > 0, nk * np.log2(np.maximum(nk, 1)), LD(0)).sum(axis=2)
    t3 = np.log2(C.astype(LD).sum(axis=2)).sum(axis=1)            # (T,)
    return ((t1 - 2 * vi_sums(zs_kept, C).T + t3[None]) / LD(N)).mean(axis=1)
