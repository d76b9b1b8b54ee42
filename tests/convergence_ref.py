"""Host restatement of the per-dyad convergence diagnostics (numpy; any float dtype, float64 and
np.longdouble in the tests), written independently of dynetlsm_amd/convergence.py: the linear predictor
eta_s of every dyad, and over its series the split R-hat and the batch-means effective sample size by the
recurrences the kernel follows (Welford's, one sample at a time; not two-pass).

The S = n_segments * seg_len samples are the halves of the chains, segment after segment."""
import numpy as np


def dyad_mask(N, directed):
    return ~np.eye(N, dtype=bool) if directed else np.triu(np.ones((N, N), dtype=bool), 1)


def eta_series(Xs, ic, radii, directed, dtype=np.float64):
    """eta_s of every ordered pair: (S, T, N, N) in ``dtype``; Xs (S, T, N, D), ic (S, 2), radii (S, N) or None"""
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


def series_rhat_ess(eta, n_segments, seg_len, batch_len, dtype=np.float64):
    """(rhat, ess) of the series eta (S, ...) along axis 0, elementwise over the other axes, in ``dtype``"""
    eta = np.asarray(eta, dtype=dtype)
    M, h, b = int(n_segments), int(seg_len), int(batch_len)
    S = M * h
    assert eta.shape[0] == S and M >= 2 and M % 2 == 0 and h >= 2 and 1 <= b <= h // 2
    a = h // b
    shape = eta.shape[1:]
    z = lambda: np.zeros(shape, dtype=dtype)                 # noqa: E731
    mean, m2, sw, mm, mm2, bs, bm, bm2 = z(), z(), z(), z(), z(), z(), z(), z()
    seg = nb = 0
    for s in range(S):
        p = s % h
        x = eta[s]
        delta = x - mean
        mean = mean + delta / dtype(p + 1)
        m2 = m2 + delta * (x - mean)
        bs = x.copy() if p % b == 0 else bs + x
        if p < a * b and p % b == b - 1:                     # a batch ends
            nb += 1
            v = bs / dtype(b)
            delta = v - bm
            bm = bm + delta / dtype(nb)
            bm2 = bm2 + delta * (v - bm)
        if p == h - 1:                                       # a segment ends
            seg += 1
            sw = sw + m2 / dtype(h - 1)
            delta = mean - mm
            mm = mm + delta / dtype(seg)
            mm2 = mm2 + delta * (mean - mm)
            mean, m2 = z(), z()
    assert seg == M and nb == M * a
    W = sw / dtype(M)
    B = dtype(h) * mm2 / dtype(M - 1)
    varp = dtype(h - 1) / dtype(h) * W + B / dtype(h)
    vbm = dtype(b) * bm2 / dtype(nb - 1)
    inf = dtype(np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        rhat = np.where(W == 0, np.where(B == 0, dtype(1), inf), np.sqrt(varp / np.where(W == 0, dtype(1), W)))
        ess = np.where(vbm == 0, np.where(varp == 0, dtype(S), inf),
                       dtype(S) * varp / np.where(vbm == 0, dtype(1), vbm))
    return rhat.astype(dtype), ess.astype(dtype)


def bins(values, edges):
    """the bin of a value: the number of edges <= it"""
    return np.searchsorted(np.asarray(edges, dtype=np.float64), np.asarray(values, dtype=np.float64), side='right')


def accumulate(Xs, ic, radii, directed, n_segments, seg_len, batch_len, rhat_edges, ess_edges, dtype=np.float64):
    """What Chain.convergence_accumulate returns with want_pointwise, the real arrays in ``dtype``:
    hist_rhat (T, len(rhat_edges) + 1), hist_ess (T, len(ess_edges) + 1) int64, node_rhat_max (T, N),
    node_ess_min (T, N), pointwise (T, N, N, 2)"""
    S, T, N, D = np.shape(Xs)
    mask = dyad_mask(N, directed)
    rhat, ess = series_rhat_ess(eta_series(Xs, ic, radii, directed, dtype), n_segments, seg_len, batch_len, dtype)
    assert not np.isnan(rhat[:, mask]).any() and not np.isnan(ess[:, mask]).any()
    hist_rhat = np.zeros((T, len(rhat_edges) + 1), dtype=np.int64)
    hist_ess = np.zeros((T, len(ess_edges) + 1), dtype=np.int64)
    for t in range(T):
        hist_rhat[t] = np.bincount(bins(rhat[t][mask], rhat_edges), minlength=len(rhat_edges) + 1)
        hist_ess[t] = np.bincount(bins(ess[t][mask], ess_edges), minlength=len(ess_edges) + 1)
    R = np.where(mask, rhat, dtype(0))
    E = np.where(mask, ess, dtype(np.inf))
    node_rhat = np.maximum(R.max(axis=2), R.max(axis=1))
    node_ess = np.minimum(E.min(axis=2), E.min(axis=1))
    pw = np.zeros((T, N, N, 2), dtype=dtype)
    pw[..., 0] = R
    pw[..., 1] = np.where(mask, ess, dtype(0))
    return hist_rhat, hist_ess, node_rhat, node_ess, pw


def tolerance(ref64, refld, factor=16.0, ulps=4.0):
    """The device's allowance on one output array, by the rule of tests/ic_ref.py: ``factor`` times eps, the
    reference's own rounding error on this input (max |float64 - longdouble| over the finite values of the
    array), plus ``ulps`` ulp of each value.  An infinite value has the allowance 0: it must be met exactly."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    fin = np.isfinite(ref64)
    assert np.array_equal(fin, np.isfinite(refld)), 'float64 and longdouble disagree on what is infinite'
    d = np.abs(ref64.astype(np.longdouble)[fin] - np.asarray(refld)[fin])
    eps = float(d.max()) if d.size else 0.0
    tol = np.zeros(ref64.shape)
    tol[fin] = factor * eps + ulps * np.spacing(np.abs(ref64[fin]))
    return tol, eps


def error(got, ref64):
    """|got - ref64| where the reference is finite; where it is infinite 0 if ``got`` is the same infinity,
    else +inf"""
    got = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64)
    fin = np.isfinite(ref64)
    err = np.where(got == ref64, 0.0, np.inf)
    err[fin] = np.abs(got[fin] - ref64[fin])
    err[np.isnan(got)] = np.inf
    return err
