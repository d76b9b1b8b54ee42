"""Host restatement of the in-sample scores (numpy): the posterior-mean edge probability pbar of every
dyad in float64, its rank key, the histograms and the four integers per time step and pooled (Python-int
arithmetic), the log-loss sums in float64 and np.longdouble, and the exact AUC of pbar by scikit-learn.
Written independently of dynetlsm_amd/scores.py and csrc/kernels_score.hpp; dense (S, T, N, N) arrays,
for the small shapes of the tests."""
import numpy as np

KEY_LO = 0x200000                      # bits(2^-63 as float32) >> 8
KEY_HI = 0x3F8000                      # bits(1.0 as float32) >> 8
N_BINS = KEY_HI - KEY_LO + 1


def dyad_mask(N, directed):
    return ~np.eye(N, dtype=bool) if directed else np.triu(np.ones((N, N), dtype=bool), 1)


def scored_dyads(T, N, directed, mask=None):
    """(T, N, N) boolean: the dyads of the model whose mask entry is not set (undirected: neither of
    (i, j), (j, i))"""
    sc = np.broadcast_to(dyad_mask(N, directed), (T, N, N)).copy()
    if mask is not None:
        m = np.asarray(mask) != 0
        if not directed:
            m = m | m.transpose(0, 2, 1)
        sc &= ~m
    return sc


def linear_predictor(Xs, ic, radii, directed, dtype=np.float64):
    """eta (S, T, N, N) in ``dtype``: Xs (S, T, N, D), ic (S, 2), radii (S, N) or None"""
    Xs = np.asarray(Xs, dtype=dtype)
    ic = np.asarray(ic, dtype=dtype)
    S, T, N, D = Xs.shape
    s2 = np.zeros((S, T, N, N), dtype=dtype)
    for d in range(D):
        df = Xs[:, :, :, None, d] - Xs[:, :, None, :, d]
        s2 += df * df
    dist = np.sqrt(s2)
    if directed:
        r = np.asarray(radii, dtype=dtype)
        b_in, b_out = ic[:, 0, None, None, None], ic[:, 1, None, None, None]
        return b_in * (1 - dist / r[:, None, None, :]) + b_out * (1 - dist / r[:, None, :, None])
    return ic[:, 0, None, None, None] - dist


def posterior_mean_proba(eta):
    """pbar (T, N, N) = mean over the samples of expit(eta), without overflow"""
    e = np.exp(-np.abs(eta))
    p = np.where(eta >= 0, 1 / (1 + e), e / (1 + e))
    return p.sum(axis=0) / eta.shape[0]


def key(p):
    """the rank key of float64 probabilities: the top 24 bits of the float32 (round to nearest even),
    clamped from below"""
    u = np.asarray(p, dtype=np.float64).astype(np.float32).view(np.uint32) >> 8
    return np.maximum(u, KEY_LO).astype(np.int64)


def keys_are_stable(p, margin=1e-12):
    """every key is the same a relative ``margin`` below and above the probability"""
    p = np.asarray(p, dtype=np.float64)
    return bool(np.all(key(p * (1 - margin)) == key(p * (1 + margin))))


def rank_counts(k, y):
    """(n_pos, n_neg, u2, ties) as Python ints from keys ``k`` and 0 / 1 labels ``y`` (flat arrays)"""
    k = np.asarray(k, dtype=np.int64) - KEY_LO
    y = np.asarray(y) != 0
    pos = np.bincount(k[y], minlength=N_BINS)
    neg = np.bincount(k[~y], minlength=N_BINS)
    n_pos, n_neg, u2, ties, cum = 0, 0, 0, 0, 0
    for b in np.nonzero(pos + neg)[0]:
        pb, nb = int(pos[b]), int(neg[b])
        u2 += pb * (2 * cum + nb)
        ties += pb * nb
        cum += nb
        n_pos += pb
        n_neg += nb
    return n_pos, n_neg, u2, ties


def logloss_sums(Y, eta, scored, dtype=np.float64):
    """(T,) sums over the scored dyads of -[y log pbar + (1 - y) log(1 - pbar)] in ``dtype``, as
    -log mean_s exp(l_s) with l_s = y eta_s - log(1 + exp(eta_s)): finite for any finite eta"""
    eta = np.asarray(eta, dtype=dtype)
    y = np.asarray(np.asarray(Y) != 0, dtype=dtype)[None]
    l = y * eta - np.logaddexp(dtype(0), eta)
    lp = np.logaddexp.reduce(l, axis=0) - np.log(dtype(eta.shape[0]))
    return -np.where(scored, lp, dtype(0)).sum(axis=(1, 2))


def exact_auc(p, y):
    """the AUC of the probabilities themselves (NaN when a class is empty)"""
    from sklearn.metrics import roc_auc_score
    y = np.asarray(y) != 0
    if y.all() or not y.any():
        return float('nan')
    return float(roc_auc_score(y, p))


def reference(Y, Xs, ic, radii, directed, mask=None):
    """Everything the tests compare: dict with 'counts' ((T + 1) rows of 4 Python ints, row T pooled),
    'logloss' / 'logloss_ld' ((T,) sums in float64 / longdouble), 'pbar' (T, N, N), 'scored' (T, N, N),
    'auc_exact_t' (T,) and 'auc_exact' (pooled) of pbar by scikit-learn"""
    Y = np.asarray(Y)
    T, N = Y.shape[:2]
    scored = scored_dyads(T, N, directed, mask)
    eta = linear_predictor(Xs, ic, radii, directed)
    pbar = posterior_mean_proba(eta)
    k = key(pbar)
    counts = [rank_counts(k[t][scored[t]], Y[t][scored[t]]) for t in range(T)]
    counts.append(rank_counts(k[scored], Y[scored]))
    return {'counts': counts, 'pbar': pbar, 'scored': scored,
            'logloss': logloss_sums(Y, eta, scored),
            'logloss_ld': logloss_sums(Y, linear_predictor(Xs, ic, radii, directed, np.longdouble), scored,
                                       np.longdouble),
            'auc_exact_t': np.array([exact_auc(pbar[t][scored[t]], Y[t][scored[t]]) for t in range(T)]),
            'auc_exact': exact_auc(pbar[scored], Y[scored])}


def auc_of_counts(row):
    """(auc, auc_bound) of one row of counts in exact arithmetic"""
    n_pos, n_neg, u2, ties = row
    den = 2 * n_pos * n_neg
    return (u2 / den, ties / den) if den else (float('nan'), float('nan'))
