"""Host restatement of the information criteria (numpy; any float dtype, float64 and np.longdouble in
the tests): the pointwise log-likelihood l_s of every dyad, its reduction over the samples and the
WAIC / DIC formulas, written independently of dynetlsm_amd/ic.py.

The reduction walks the rows in chunks (a few threads: numpy releases the GIL), so that full-size
networks never hold S x N x N values at once."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

WORKERS = max(1, min(16, os.cpu_count() or 1))


def dyad_mask(N, directed):
    return ~np.eye(N, dtype=bool) if directed else np.triu(np.ones((N, N), dtype=bool), 1)


def loglik_rows(Y, Xs, ic, radii, directed, i0, i1, dtype=np.float64, j0=0):
    """l_s of the dyads (rows i0..i1-1, columns j0..N-1): (S, T, i1 - i0, N - j0) in ``dtype``; Y (T, N, N),
    Xs (S, T, N, D), ic (S, 2), radii (S, N) or None.  The mask of the dyads is not applied."""
    Xs = np.asarray(Xs, dtype=dtype)
    ic = np.asarray(ic, dtype=dtype)
    S, T, N, D = Xs.shape
    s2 = np.zeros((S, T, i1 - i0, N - j0), dtype=dtype)
    for d in range(D):
        df = Xs[:, :, i0:i1, None, d] - Xs[:, :, None, j0:, d]
        s2 += df * df
    dist = np.sqrt(s2)
    if directed:
        r = np.asarray(radii, dtype=dtype)
        b_in, b_out = ic[:, 0, None, None, None], ic[:, 1, None, None, None]
        eta = b_in * (1 - dist / r[:, None, None, j0:]) + b_out * (1 - dist / r[:, None, i0:i1, None])
    else:
        eta = ic[:, 0, None, None, None] - dist
    y = np.asarray(Y[:, i0:i1, j0:] != 0, dtype=dtype)[None]
    return y * eta - np.logaddexp(dtype(0), eta)


def _reduce_rows(args):
    Y, Xs, ic, radii, directed, i0, i1, dtype = args
    S = np.shape(Xs)[0]
    N = Y.shape[1]
    j0 = 0 if directed else i0                  # undirected: the dyads i < j of these rows
    l = loglik_rows(Y, Xs, ic, radii, directed, i0, i1, dtype, j0)
    mask = dyad_mask(N, directed)[i0:i1, j0:]
    lppd = np.logaddexp.reduce(l, axis=0) - np.log(dtype(S))
    var = np.var(l, axis=0, ddof=1) if S > 1 else np.zeros(l.shape[1:], dtype=dtype)
    mean = np.mean(l, axis=0)
    sl = np.where(mask, l, dtype(0)).sum(axis=(2, 3))                     # (S, T)
    z = dtype(0)
    return i0, i1, j0, np.where(mask, lppd, z), np.where(mask, var, z), np.where(mask, mean, z), sl


def accumulate(Y, Xs, ic, radii, directed, dtype=np.float64, want_pointwise=True, rows=None):
    """What Chain.ic_accumulate returns, in ``dtype``: totals (T, 5), sample_loglik (S, T) and
    pointwise (T, N, N, 2) (None unless ``want_pointwise``)"""
    Y = np.asarray(Y)
    S, T, N, D = np.shape(Xs)
    if rows is None:
        rows = max(1, min(N, int(4e6 // max(1, S * T * N))))
    jobs = [(Y, Xs, ic, radii, directed, i0, min(N, i0 + rows), dtype) for i0 in range(0, N, rows)]
    if len(jobs) > 1 and WORKERS > 1:
        with ThreadPoolExecutor(WORKERS) as ex:
            parts = list(ex.map(_reduce_rows, jobs))
    else:
        parts = [_reduce_rows(j) for j in jobs]
    totals = np.zeros((T, 5), dtype=dtype)
    sample_loglik = np.zeros((S, T), dtype=dtype)
    pw = np.zeros((T, N, N, 2), dtype=dtype) if want_pointwise else None
    for i0, i1, j0, lppd, var, mean, sl in parts:
        elpd = lppd - var
        totals[:, 0] += lppd.sum(axis=(1, 2))
        totals[:, 1] += var.sum(axis=(1, 2))
        totals[:, 2] += mean.sum(axis=(1, 2))
        totals[:, 3] += (elpd * elpd).sum(axis=(1, 2))
        sample_loglik += sl
        if want_pointwise:
            pw[:, i0:i1, j0:, 0] = lppd
            pw[:, i0:i1, j0:, 1] = var
    totals[:, 4] = dyad_mask(N, directed).sum()
    return totals, sample_loglik, pw


def sample_loglik(Y, Xs, ic, radii, directed, dtype=np.float64):
    return accumulate(Y, Xs, ic, radii, directed, dtype, want_pointwise=False)[1]


def criteria(pointwise, sample_ll, loglik_hat, directed):
    """WAIC and DIC by brute force from the pointwise arrays (T, N, N, 2), sample_loglik (S, T) and the
    log-likelihood (T,) at the point estimate: a dict of totals and per-time-step arrays ('*_t')"""
    pointwise = np.asarray(pointwise, dtype=np.float64)
    T, N = pointwise.shape[:2]
    mask = dyad_mask(N, directed)
    lppd_ij = pointwise[..., 0][:, mask]                   # (T, n)
    var_ij = pointwise[..., 1][:, mask]
    elpd_ij = lppd_ij - var_ij
    n = elpd_ij.size
    out = {'n_dyads': n, 'lppd': lppd_ij.sum(), 'p_waic': var_ij.sum(), 'elpd_waic': elpd_ij.sum(),
           'lppd_t': lppd_ij.sum(axis=1), 'p_waic_t': var_ij.sum(axis=1), 'elpd_waic_t': elpd_ij.sum(axis=1)}
    out['waic'] = -2 * out['elpd_waic']
    out['waic_t'] = -2 * out['elpd_waic_t']
    out['se_elpd'] = np.sqrt(n * np.var(elpd_ij.ravel(), ddof=1)) if n > 1 else 0.0
    out['se_elpd_t'] = np.array([np.sqrt(e.size * np.var(e, ddof=1)) if e.size > 1 else 0.0 for e in elpd_ij])
    dev = -2 * np.asarray(sample_ll, dtype=np.float64)
    out['d_bar_t'] = dev.mean(axis=0)
    out['d_bar'] = dev.sum(axis=1).mean()
    out['d_hat_t'] = -2 * np.asarray(loglik_hat, dtype=np.float64)
    out['d_hat'] = out['d_hat_t'].sum()
    out['p_d'] = out['d_bar'] - out['d_hat']
    out['dic'] = out['d_bar'] + out['p_d']
    out['p_v'] = np.var(dev.sum(axis=1), ddof=1) / 2 if dev.shape[0] > 1 else 0.0
    out['dic_v'] = out['d_bar'] + out['p_v']
    return out


def compare(pw_a, pw_b, directed):
    """(elpd_a - elpd_b, sqrt(n Var(elpd_a,ij - elpd_b,ij))) by brute force"""
    mask = dyad_mask(pw_a.shape[1], directed)
    d = ((pw_a[..., 0] - pw_a[..., 1]) - (pw_b[..., 0] - pw_b[..., 1]))[:, mask].ravel()
    return d.sum(), np.sqrt(d.size * np.var(d, ddof=1))


def tolerance(ref64, refld, factor=16.0, ulps=4.0):
    """The device's allowance on one output array: ``factor`` times eps, the reference's own rounding error
    on this input (max |float64 - longdouble| over the array), plus ``ulps`` ulp of each value"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    eps = float(np.max(np.abs(ref64.astype(np.longdouble) - refld))) if ref64.size else 0.0
    return factor * eps + ulps * np.spacing(np.abs(ref64)), eps
