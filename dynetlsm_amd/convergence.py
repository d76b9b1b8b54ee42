"""Convergence of every dyad of a fitted dynamic latent space model: split R-hat and effective sample
size of the trace, on the device.

The reference has no counterpart.  ``diagnostics.py`` and ``multichain.split_rhat`` look at a handful
of scalar traces; the latent positions, where such a model mixes badly (hubs, isolates, nodes that
switch cluster), cannot be compared across chains - or within one without Procrustes.  The linear
predictor eta of a dyad can: ``b - |x_i - x_j|`` undirected, the directed model of ``metrics.py``
(probas_) for directed and case-control fits, is invariant to rotation, reflection, translation and
label switching, and it is what the likelihood sees.  Chains started from different seeds are pooled
with no alignment.

Every chain's n kept samples are cut into two halves of h = n // 2 (an odd last sample is dropped, as
``multichain.split_rhat`` does): M = 2 C segments, S = M h samples.  Per dyad, over its series eta_s:

* ``rhat``: with W the mean of the segments' variances and B = h Var(segment means) (both ddof 1),
  ``var+ = (h - 1) / h W + B / h`` and ``rhat = sqrt(var+ / W)`` (Gelman et al., BDA3 11.4) - for
  chains of even length ``multichain.split_rhat`` of the same series.  W == 0: 1 if B == 0, else inf.
* ``ess``: a BATCH-MEANS effective sample size (Flegal & Jones 2010), not the autocorrelation sum of
  ``diagnostics.effective_n`` - no lag window fits in registers for 8 dyads per thread.  With
  b = floor(sqrt(h)) and a = h // b batches per segment over its samples [q b, (q + 1) b) (the tail of
  a segment enters no batch), ``v_bm = b Var(all M a batch means)`` (ddof 1) and
  ``ess = S var+ / v_bm``.  It is not capped: negatively correlated draws give ess > S.
  v_bm == 0: S if var+ == 0, else inf.  With ``n_samples`` thinning it is the ESS of the THINNED
  series.

The device streams the samples through a tile and keeps eight running moments per dyad in registers
(``Chain.convergence_accumulate``: csrc/kernels_conv.hpp); nothing of size T N N is stored unless
``pointwise`` asks for it.  It returns histograms of both quantities per time step and, per node, the
largest rhat and the smallest ess over the dyads the node is part of.
"""
import numpy as np

from ._trace import model_chain, sample_rows, trace_samples

__all__ = ['convergence_diagnostics', 'ConvergenceResult', 'split_segments', 'series_rhat', 'series_ess']


def split_segments(chains):
    """(C, n) scalar traces -> (2 C, n // 2): the two halves of every chain, chain after chain (an odd
    last sample is dropped)"""
    c = np.asarray(chains, dtype=np.float64)
    if c.ndim == 1:
        c = c[None]
    h = c.shape[1] // 2
    return np.stack([c[:, :h], c[:, h:2 * h]], axis=1).reshape(2 * c.shape[0], h)


def _var_plus(q):
    h = q.shape[1]
    W = q.var(axis=1, ddof=1).mean()
    B = h * q.mean(axis=1).var(ddof=1)
    return W, B, (h - 1.0) / h * W + B / h


def series_rhat(segments):
    """split R-hat of the segments (M, h) of a scalar series, as the device computes it per dyad"""
    q = np.asarray(segments, dtype=np.float64)
    W, B, varp = _var_plus(q)
    if W == 0.0:
        return 1.0 if B == 0.0 else float('inf')
    return float(np.sqrt(varp / W))


def series_ess(segments, batch_len=None):
    """batch-means effective sample size of the segments (M, h) of a scalar series, as the device
    computes it per dyad; ``batch_len`` defaults to floor(sqrt(h))"""
    q = np.asarray(segments, dtype=np.float64)
    M, h = q.shape
    b = int(np.floor(np.sqrt(h))) if batch_len is None else int(batch_len)
    a = h // b
    means = q[:, :a * b].reshape(M * a, b).mean(axis=1)
    v_bm = b * means.var(ddof=1)
    varp = _var_plus(q)[2]
    if v_bm == 0.0:
        return float(M * h) if varp == 0.0 else float('inf')
    return float(M * h * varp / v_bm)


class ConvergenceResult(object):
    """Result of ``convergence_diagnostics``.

    n_chains, n_segments, seg_len, batch_len : C, M = 2 C, h, b of the module's text
    n_samples        : S = M h samples the device saw
    sample_ids       : trace rows of each chain they came from
    rhat_edges, ess_edges : the histograms' edges; the bin of a value is the number of edges <= it
    rhat_hist_t, ess_hist_t : (T, edges + 1) dyad counts per time step; rhat_hist, ess_hist: pooled
    node_rhat_, node_ess_ : (T, N) largest rhat / smallest ess over the dyads that contain the node
                       (directed: as sender or as receiver)
    max_rhat, min_ess, max_rhat_t, min_ess_t : over all dyads, in total and per time step
    pointwise_rhat, pointwise_ess : (T, N, N) when asked for (undirected: i < j filled, the rest 0),
                       else None
    scalars          : {'intercepts[0]': (rhat, ess), 'logps': ..., 'lambdas': ...} of the scalar
                       traces over the same rows, by the same two definitions on the host
    """

    def __init__(self, n_chains, seg_len, batch_len, sample_ids, rhat_edges, ess_edges, hist_rhat, hist_ess,
                 node_rhat, node_ess, is_directed, pointwise=None, scalars=None):
        self.n_chains = int(n_chains)
        self.n_segments = 2 * self.n_chains
        self.seg_len, self.batch_len = int(seg_len), int(batch_len)
        self.n_samples = self.n_segments * self.seg_len
        self.sample_ids = sample_ids
        self.is_directed = bool(is_directed)
        self.rhat_edges = np.asarray(rhat_edges, dtype=np.float64)
        self.ess_edges = np.asarray(ess_edges, dtype=np.float64)
        self.rhat_hist_t = np.asarray(hist_rhat).astype(np.int64)
        self.ess_hist_t = np.asarray(hist_ess).astype(np.int64)
        self.rhat_hist, self.ess_hist = self.rhat_hist_t.sum(axis=0), self.ess_hist_t.sum(axis=0)
        self.node_rhat_ = np.asarray(node_rhat, dtype=np.float64)
        self.node_ess_ = np.asarray(node_ess, dtype=np.float64)
        self.n_nodes = int(self.node_rhat_.shape[1])
        self.n_dyads_t = self.rhat_hist_t.sum(axis=1)
        self.n_dyads = int(self.n_dyads_t.sum())
        self.max_rhat_t, self.min_ess_t = self.node_rhat_.max(axis=1), self.node_ess_.min(axis=1)
        self.max_rhat, self.min_ess = float(self.max_rhat_t.max()), float(self.min_ess_t.min())
        if pointwise is None:
            self.pointwise_rhat = self.pointwise_ess = None
        else:
            self.pointwise_rhat, self.pointwise_ess = pointwise[..., 0], pointwise[..., 1]
        self.scalars = dict(scalars or {})

    def worst_nodes(self, k=10):
        """the k worst (t, node, rhat, ess): largest rhat first, the smaller ess among equals"""
        T, N = self.node_rhat_.shape
        r, e = self.node_rhat_.ravel(), self.node_ess_.ravel()
        order = np.lexsort((e, -r))[:max(0, int(k))]
        return [(int(o // N), int(o % N), float(r[o]), float(e[o])) for o in order]

    def summary(self):
        """Text table: the dyads per bin in total and per time step, the extremes and the scalar traces"""
        T = self.rhat_hist_t.shape[0]
        head = '%-16s %12s' % ('', 'total') + ''.join(' %12s' % ('t=%d' % t) for t in range(T))
        lines = ['convergence of eta: %d chain(s), %d segments of %d samples (batches of %d), %d dyads (%s)'
                 % (self.n_chains, self.n_segments, self.seg_len, self.batch_len, self.n_dyads,
                    'directed' if self.is_directed else 'undirected'), head]

        def labels(name, edges):
            if not len(edges):
                return ['%s all' % name]
            return (['%s < %g' % (name, edges[0])]
                    + ['%s %g - %g' % (name, lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]
                    + ['%s >= %g' % (name, edges[-1])])

        for name, edges, pooled, per_t in (('rhat', self.rhat_edges, self.rhat_hist, self.rhat_hist_t),
                                           ('ess', self.ess_edges, self.ess_hist, self.ess_hist_t)):
            for k, label in enumerate(labels(name, edges)):
                lines.append('%-16s %12d' % (label, pooled[k]) + ''.join(' %12d' % v for v in per_t[:, k]))
        lines.append('%-16s %12.6g' % ('max rhat', self.max_rhat) + ''.join(' %12.6g' % v for v in self.max_rhat_t))
        lines.append('%-16s %12.6g' % ('min ess', self.min_ess) + ''.join(' %12.6g' % v for v in self.min_ess_t))
        for name in sorted(self.scalars):
            lines.append('%-16s rhat %10.6g  ess %10.6g' % ((name,) + tuple(self.scalars[name])))
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _check_edges(name, edges):
    e = np.asarray(edges, dtype=np.float64).ravel()
    if e.size > 16:
        raise ValueError('%s: at most 16 edges, got %d' % (name, e.size))
    if not np.isfinite(e).all() or (e.size > 1 and not (np.diff(e) > 0).all()):
        raise ValueError('%s must be finite and ascending, got %r' % (name, tuple(edges)))
    return e


def _scalar_traces(model):
    """name -> (n_rows,) for every column of the model's scalar traces"""
    out = {}
    for name in ('intercepts', 'logps', 'lambdas'):
        tr = getattr(model, name + '_', None)
        if tr is None:
            continue
        tr = np.asarray(tr, dtype=np.float64)
        if tr.ndim == 1:
            out[name] = tr
        else:
            tr = tr.reshape(tr.shape[0], -1)
            for j in range(tr.shape[1]):
                out['%s[%d]' % (name, j)] = tr[:, j]
    return out


def convergence_diagnostics(models, n_samples=None, pointwise=False, rhat_edges=(1.01, 1.05, 1.1, 1.2, 1.5, 2.0),
                            ess_edges=(10, 50, 100, 200, 400, 1000)):
    """Split R-hat and batch-means ESS of the linear predictor of every dyad (see the module's text).

    ``models``: one fitted ``DynamicNetworkLSM`` (undirected, directed or case-control),
    ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM``, or a sequence of them - chains of the same
    model on the same network (for instance fits with different ``random_state``), which are pooled.
    They must agree in class, shape, directedness, ``Y_fit_`` and number of kept rows.  The samples of
    each chain are all kept rows of its trace (after the burn-in), or ``n_samples`` of them evenly spaced
    (``information_criteria`` picks them the same way); at least 4 are needed.  ``pointwise=True`` also
    returns both quantities per dyad (two (T, N, N) arrays).  The edges (at most 16 each, ascending) cut
    the histograms: the bin of a value is the number of edges <= it.

    Returns a ``ConvergenceResult``.
    """
    if isinstance(models, (list, tuple)):
        models = list(models)
        if not models:
            raise ValueError('no model given')
    else:
        models = [models]
    re_ = _check_edges('rhat_edges', rhat_edges)
    ee = _check_edges('ess_edges', ess_edges)
    ids = [sample_rows(m, n_samples) for m in models]
    first = models[0]
    for m, i in zip(models[1:], ids[1:]):
        if type(m) is not type(first):
            raise ValueError('the chains are of different classes: %s and %s' % (type(first).__name__, type(m).__name__))
        if bool(m.is_directed) != bool(first.is_directed):
            raise ValueError('a directed and an undirected chain cannot be pooled')
        if np.shape(m.Xs_)[1:] != np.shape(first.Xs_)[1:]:
            raise ValueError('the chains differ in shape: %s and %s' % (np.shape(first.Xs_)[1:], np.shape(m.Xs_)[1:]))
        if len(i) != len(ids[0]):
            raise ValueError('the chains differ in their number of kept rows: %d and %d' % (len(ids[0]), len(i)))
        if np.shape(m.Y_fit_) != np.shape(first.Y_fit_) or not np.array_equal(m.Y_fit_, first.Y_fit_):
            raise ValueError('the chains were fit to different networks')
    n = len(ids[0])
    if n < 4:
        raise ValueError('%d kept rows: split R-hat needs at least 4 per chain' % n)
    h = n // 2
    b = int(np.floor(np.sqrt(h)))
    C_ = len(models)
    directed = bool(first.is_directed)

    # the two halves of every chain's rows, chain after chain
    parts = [trace_samples(m, i[:2 * h]) for m, i in zip(models, ids)]
    Xs, ic = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in (0, 1))
    radii = np.concatenate([p[2] for p in parts]) if directed else None
    S, T, N, D = Xs.shape
    scalars = {}
    traces = [_scalar_traces(m) for m in models]
    for name in traces[0]:
        if all(name in tr for tr in traces):
            q = split_segments(np.stack([tr[name][i] for tr, i in zip(traces, ids)]))
            scalars[name] = (series_rhat(q), series_ess(q, b))

    with model_chain(first, T, N, D, directed) as chain:
        out = chain.convergence_accumulate(Xs, ic, radii, n_segments=2 * C_, seg_len=h, batch_len=b,
                                           rhat_edges=re_, ess_edges=ee, want_pointwise=pointwise)
    return ConvergenceResult(C_, h, b, ids if len(ids) > 1 else ids[0], re_, ee, out[0], out[1], out[2], out[3],
                             directed, out[4] if pointwise else None, scalars)
