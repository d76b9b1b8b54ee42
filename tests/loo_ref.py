"""Host restatement of PSIS-LOO (numpy; any float dtype, float64 and np.longdouble in the tests), written from
the definition in include/dynetlsm_hip.h, independently of dynetlsm_amd/loo.py and csrc/psis_tail.hpp.

For one dyad with pointwise log-likelihoods l_1..l_S (ic_ref.loglik_rows), r_eff = 1:

    M = min(floor(S/5), ceil(3 sqrt(S))),  lr_s = c - l_s,  c = min_s l_s
    tail: the M largest lr, ascending lr_(1..M);  lr_cut: the next one below
    fitted iff M >= 5, lr_(M) - lr_(1) >= DBL_EPSILON/100, every quantity of the fit finite, xstar > 0
    fit:  x_m = exp(lr_(m)) - exp(lr_cut),  G = 30 + floor(sqrt(M)),  xstar = x_q, q = floor(M/4 + 0.5)
          theta_j = 1/x_M + (1 - sqrt(G/(j - 0.5)))/(3 xstar),  k_j = mean_m log1p(-theta_j x_m)
          L_j = M (log(-theta_j/k_j) - k_j - 1),  w_j = 1/sum_i exp(L_i - L_j),  theta = sum_j w_j theta_j
          k = mean_m log1p(-theta x_m),  sigma = -k/theta,  k <- (M k + 5)/(M + 10)
    smoothing:  lw_(m) = min(0, log(exp(lr_cut) + sigma expm1(-k log1p(-p_m))/k)),  p_m = (m - 0.5)/M
                (k == 0: -sigma log1p(-p_m) for the quotient); off the tail and for unfitted dyads lw = lr
    elpd_loo = logsumexp_s(lw_s + l_s) - logsumexp_s(lw_s),  lppd = logsumexp_s(l_s) - log S,  k (unfitted: +inf)

Vectorised over the dyads; the passes over a network walk the rows in chunks on a few threads."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ic_ref  # noqa: E402

WORKERS = ic_ref.WORKERS
MIN_SPREAD = np.finfo(np.float64).eps / 100


def tail_length(S):
    return int(min(S // 5, int(np.ceil(3 * np.sqrt(S)))))


def k_threshold(S):
    return min(1 - 1 / np.log10(S), 0.7)


def _exp(v):
    """exp in v's dtype, for the two exponentials of x.  Whether a tail is fitted can hinge on their last bit (xstar
    = x_q > 0, where a tail value lies within an ulp of the cutoff), and numpy's float64 exp, a SIMD routine, is
    not the correctly rounded one for 4.6 % of the arguments in (-2, 0) (measured against long double; glibc's exp:
    0.08 %).  So the float64 evaluation takes exp through long double and rounds once more - correctly rounded but
    for double rounding; where long double is no wider than float64 this is numpy's exp."""
    v = np.asarray(v)
    if v.dtype == np.float64 and np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant:
        return np.exp(v.astype(np.longdouble)).astype(np.float64)
    return np.exp(v)


def fit_tails(tails):
    """tails (n, M + 1): the M + 1 smallest l of n dyads, ascending, in the dtype to compute in.  Returns
    (k (n,) adjusted, +inf where unfitted; sigma (n,); fitted (n,) bool; lw (n, M): the smoothed lw_(1..M),
    ascending in lr - garbage where unfitted)"""
    tails = np.asarray(tails)
    dtype = tails.dtype.type
    n, M = tails.shape[0], tails.shape[1] - 1
    k = np.full(n, np.inf, dtype=dtype)
    sigma = np.zeros(n, dtype=dtype)
    fitted = np.zeros(n, dtype=bool)
    lw = np.zeros((n, M), dtype=dtype)
    if M < 5 or n == 0:
        return k, sigma, fitted, lw
    G = 30 + int(np.floor(np.sqrt(M)))
    q = int(np.floor(M / 4 + 0.5))
    j = np.arange(1, G + 1).astype(dtype)
    p = (np.arange(1, M + 1).astype(dtype) - dtype(0.5)) / dtype(M)
    step = max(1, int(2e6 // (G * M)))
    with np.errstate(all='ignore'):
        for a in range(0, n, step):
            t = tails[a:a + step]
            c = t[:, 0]
            lr = c[:, None] - t[:, M - 1::-1]                  # (n, M) ascending: lr_(m) = c - l(M - m)
            assert lr.shape[1] == M
            lr_cut = c - t[:, M]
            ecut = _exp(lr_cut)
            x = _exp(lr) - ecut[:, None]
            xstar = x[:, q - 1]
            theta_j = 1 / x[:, -1, None] + (1 - np.sqrt(dtype(G) / (j - dtype(0.5))))[None] / (3 * xstar[:, None])
            k_j = np.log1p(-theta_j[:, :, None] * x[:, None, :]).mean(axis=2)
            L_j = M * (np.log(-theta_j / k_j) - k_j - 1)
            w_j = 1 / np.exp(L_j[:, None, :] - L_j[:, :, None]).sum(axis=2)
            theta = (w_j * theta_j).sum(axis=1)
            kk = np.log1p(-theta[:, None] * x).mean(axis=1)
            sg = -kk / theta
            ok = (lr[:, -1] - lr[:, 0] >= MIN_SPREAD) & (xstar > 0)
            for arr in (theta_j, k_j, L_j, w_j):
                ok &= np.isfinite(arr).all(axis=1)
            ok &= np.isfinite(theta) & np.isfinite(kk) & np.isfinite(sg)
            kk = (M * kk + 5) / (M + 10)
            lp = np.log1p(-p)[None]
            quot = np.where(kk[:, None] == 0, -sg[:, None] * lp, sg[:, None] * np.expm1(-kk[:, None] * lp) / kk[:, None])
            lw[a:a + step] = np.minimum(0, np.log(ecut[:, None] + quot))
            k[a:a + step] = np.where(ok, kk, np.inf)
            sigma[a:a + step] = sg
            fitted[a:a + step] = ok
    return k, sigma, fitted, lw


def psis_dyads(l):
    """l (S, n) in the dtype to compute in.  Returns (elpd_loo, lppd, k, fitted), each (n,)"""
    l = np.asarray(l)
    dtype = l.dtype.type
    S = l.shape[0]
    M = tail_length(S)
    ls = np.sort(l, axis=0)
    lw = ls[0][None] - ls                                      # lr, in ascending order of l
    k, _, fitted, lw_tail = fit_tails(ls[:M + 1].T if M >= 5 else ls[:1].T)
    if M >= 5:
        # slot i of the sorted l is lr_(M - i)
        lw[:M] = np.where(fitted[None], lw_tail[:, ::-1].T, lw[:M])
    elpd = np.logaddexp.reduce(lw + ls, axis=0) - np.logaddexp.reduce(lw, axis=0)
    lppd = np.logaddexp.reduce(l, axis=0) - np.log(dtype(S))
    return elpd, lppd, k, fitted


def _rows(args):
    Y, Xs, ic, radii, directed, i0, i1, dtype, perturb_seed = args
    N = Y.shape[1]
    j0 = 0 if directed else i0
    if perturb_seed is None:
        l = ic_ref.loglik_rows(Y, Xs, ic, radii, directed, i0, i1, dtype, j0)
    else:                                                      # every l_s moved by 4 ulp, random signs
        l = ic_ref.loglik_rows(Y, Xs, ic, radii, directed, i0, i1, np.float64, j0)
        sign = np.random.RandomState(perturb_seed + i0).randint(0, 2, l.shape) * 2.0 - 1.0
        l = (l + sign * 4.0 * np.spacing(np.abs(l))).astype(dtype)
    S, T = l.shape[:2]
    elpd, lppd, k, fitted = psis_dyads(l.reshape(S, -1))
    shape = l.shape[1:]
    return i0, i1, j0, elpd.reshape(shape), lppd.reshape(shape), k.reshape(shape), fitted.reshape(shape)


def accumulate(Y, Xs, ic, radii, directed, k_edges=(), dtype=np.float64, perturb_seed=None, rows=None):
    """What Chain.loo_accumulate returns, in ``dtype``: totals (T, 5), hist_k (T, len(k_edges) + 1) int64,
    node_k_max (T, N), pointwise (T, N, N, 2) - and fitted (T, N, N) bool.  ``perturb_seed``: the l_s are those
    of float64, each moved by +-4 ulp."""
    Y = np.asarray(Y)
    S, T, N, D = np.shape(Xs)
    M = tail_length(S)
    G = 30 + int(np.sqrt(max(M, 1)))
    if rows is None:
        rows = max(1, min(N, int(4e6 // max(1, max(S, G * M if M >= 5 else 0) * T * N))))
    jobs = [(Y, Xs, ic, radii, directed, i0, min(N, i0 + rows), dtype, perturb_seed) for i0 in range(0, N, rows)]
    if len(jobs) > 1 and WORKERS > 1:
        with ThreadPoolExecutor(WORKERS) as ex:
            parts = list(ex.map(_rows, jobs))
    else:
        parts = [_rows(job) for job in jobs]
    mask = ic_ref.dyad_mask(N, directed)
    pw = np.zeros((T, N, N, 2), dtype=dtype)
    lppd_all = np.zeros((T, N, N), dtype=dtype)
    fitted_all = np.zeros((T, N, N), dtype=bool)
    for i0, i1, j0, elpd, lppd, k, fitted in parts:
        pw[:, i0:i1, j0:, 0] = elpd
        pw[:, i0:i1, j0:, 1] = k
        lppd_all[:, i0:i1, j0:] = lppd
        fitted_all[:, i0:i1, j0:] = fitted
    pw[:, ~mask] = 0
    fitted_all[:, ~mask] = False
    elpd_d, k_d = pw[..., 0][:, mask], pw[..., 1][:, mask]     # (T, n)
    totals = np.zeros((T, 5), dtype=dtype)
    totals[:, 0] = elpd_d.sum(axis=1)
    totals[:, 1] = (elpd_d * elpd_d).sum(axis=1)
    totals[:, 2] = lppd_all[:, mask].sum(axis=1)
    totals[:, 3] = mask.sum()
    totals[:, 4] = mask.sum() - fitted_all[:, mask].sum(axis=1)
    edges = np.asarray(k_edges, dtype=np.float64).ravel()
    hist = np.zeros((T, edges.size + 1), dtype=np.int64)
    for t in range(T):
        hist[t] = np.bincount(np.searchsorted(edges, k_d[t].astype(np.float64), side='right'),
                              minlength=edges.size + 1)
    kfull = np.where(mask[None], pw[..., 1], dtype(-np.inf))
    if N > 1:
        node = np.maximum(kfull.max(axis=2), kfull.max(axis=1))
    else:
        node = np.full((T, N), -np.inf, dtype=dtype)
    return totals, hist, node, pw, fitted_all


def result(pw, lppd_t, directed):
    """LooResult's quantities by brute force from the pointwise array (T, N, N, 2) and lppd per time step"""
    pw = np.asarray(pw, dtype=np.float64)
    mask = ic_ref.dyad_mask(pw.shape[1], directed)
    e = pw[..., 0][:, mask]
    n = e.size
    out = {'n_dyads': n, 'elpd_loo': e.sum(), 'elpd_loo_t': e.sum(axis=1), 'lppd': np.sum(lppd_t)}
    out['p_loo'] = out['lppd'] - out['elpd_loo']
    out['looic'] = -2 * out['elpd_loo']
    out['se_elpd_loo'] = np.sqrt(n * np.var(e.ravel(), ddof=1)) if n > 1 else 0.0
    out['n_unfitted'] = int(np.isinf(pw[..., 1][:, mask]).sum())
    out['max_k'] = pw[..., 1][:, mask].max()
    return out
