"""PSIS-LOO of a fitted dynamic latent space model: Pareto-smoothed importance-sampling leave-one-out.

The reference has no counterpart.  From the pointwise log-likelihood ``l_s(t, i, j)`` of the observed
dyads over the posterior samples (the same samples, the same observed network and the same likelihood as
``information_criteria``), every dyad's leave-one-out predictive density is estimated by importance
sampling with the ratios ``1 / p(y_ij | theta_s)``, whose largest ``M = min(S/5, 3 sqrt(S))`` values are
replaced by quantiles of a generalised Pareto distribution fitted to them (Vehtari, Gelman & Gabry 2017;
Vehtari, Simpson, Gelman, Yao & Gabry; the fit of Zhang & Stephens 2009 as the R package ``loo`` does
it).  The relative efficiency ``r_eff`` of the samples is taken as 1: autocorrelation of the trace does
not enter ``k_threshold`` or the tail length.

Besides ``elpd_loo`` the fit returns the Pareto shape ``k`` of every dyad.  Where ``k`` exceeds
``k_threshold = min(1 - 1/log10(S), 0.7)`` the estimate of that dyad cannot be trusted - and WAIC, which
has no such diagnostic, is unreliable there too -; these are the dyads the model fits badly (hubs,
isolates, nodes that switch cluster).  Dyads whose tail cannot be fitted (fewer than 25 samples, a
constant tail) keep their raw ratios and carry ``k = inf``.

The device does the whole pass (``Chain.loo_accumulate``: csrc/kernels_loo.hpp, csrc/psis_tail.hpp);
the host turns the sums into the result.  Higher ``elpd_loo`` (lower ``looic``) is better.
"""
import numpy as np

from ._trace import model_chain, observed_network, sample_rows, trace_samples
from .engine import pack_network
from .ic import _se

__all__ = ['loo', 'compare_loo', 'LooResult']


def k_threshold(n_samples):
    """min(1 - 1/log10(S), 0.7): the largest Pareto shape at which S samples give a reliable estimate"""
    with np.errstate(divide='ignore'):
        return float(min(1.0 - 1.0 / np.log10(float(n_samples)), 0.7)) if n_samples > 1 else -np.inf


def k_edges(n_samples):
    """the histogram's edges: 0.5, 0.7, 1.0 and the threshold, de-duplicated and ascending"""
    edges = {0.5, 0.7, 1.0}
    thr = k_threshold(n_samples)
    if np.isfinite(thr):
        edges.add(thr)
    return np.array(sorted(edges), dtype=np.float64)


class LooResult(object):
    """Result of ``loo``.

    Totals are floats; every ``*_t`` attribute is the (T,) array of the time steps, which sum to the
    total (``se_elpd_loo_t`` is the standard error within a time step).

    sample_ids       : trace rows the estimate was computed from
    n_samples        : their number S
    n_dyads          : dyads of the network (undirected: t, i < j; directed: t, i != j)
    n_unfitted       : dyads whose tail was not fitted (k = inf)
    elpd_loo, p_loo = lppd - elpd_loo, looic = -2 elpd_loo, se_elpd_loo = sqrt(n Var_dyads), lppd
    k_threshold      : min(1 - 1/log10(S), 0.7)
    k_edges          : edges of the histogram of k: 0.5, 0.7, 1.0 and k_threshold
    k_hist_t, k_hist : (T, len(k_edges) + 1) and (len(k_edges) + 1,) dyads per bin; the bin of a k is the
                       number of edges <= it
    n_bad_t, n_bad   : dyads with k > k_threshold (unfitted ones included)
    node_k_          : (T, N) largest k over the dyads of each node
    max_k            : largest k of all dyads
    pointwise_elpd_loo, pointwise_k : (T, N, N) when asked for (undirected: i < j filled, the rest 0),
                       else None
    """

    def __init__(self, sample_ids, n_samples, totals, k_edges, k_hist, node_k, is_directed, n_nodes,
                 pointwise=None):
        totals = np.asarray(totals, dtype=np.float64)
        self.sample_ids = sample_ids
        self.n_samples = int(n_samples)
        self.is_directed = bool(is_directed)
        self.n_nodes = int(n_nodes)
        self.n_dyads_t = np.rint(totals[:, 3]).astype(np.int64)
        self.n_dyads = int(self.n_dyads_t.sum())
        self.n_unfitted_t = np.rint(totals[:, 4]).astype(np.int64)
        self.n_unfitted = int(self.n_unfitted_t.sum())
        self.elpd_loo_t, self.lppd_t = totals[:, 0].copy(), totals[:, 2].copy()
        self.p_loo_t = self.lppd_t - self.elpd_loo_t
        self.looic_t = -2.0 * self.elpd_loo_t
        self.se_elpd_loo_t = _se(self.elpd_loo_t, totals[:, 1], self.n_dyads_t)
        self.elpd_loo, self.lppd = float(self.elpd_loo_t.sum()), float(self.lppd_t.sum())
        self.p_loo = self.lppd - self.elpd_loo
        self.looic = -2.0 * self.elpd_loo
        self.se_elpd_loo = float(_se(self.elpd_loo, totals[:, 1].sum(), self.n_dyads))
        self.k_threshold = k_threshold(self.n_samples)
        self.k_edges = np.asarray(k_edges, dtype=np.float64)
        self.k_hist_t = np.asarray(k_hist).astype(np.int64)
        self.k_hist = self.k_hist_t.sum(axis=0)
        # k > threshold: the bins above the threshold's edge (a k equal to the edge counts as above it)
        above = int(np.searchsorted(self.k_edges, self.k_threshold, side='right'))
        self.n_bad_t = self.k_hist_t[:, above:].sum(axis=1)
        self.n_bad = int(self.n_bad_t.sum())
        self.node_k_ = np.asarray(node_k, dtype=np.float64)
        self.max_k = float(self.node_k_.max()) if self.node_k_.size else -np.inf
        if pointwise is None:
            self.pointwise_elpd_loo = self.pointwise_k = None
        else:
            self.pointwise_elpd_loo, self.pointwise_k = pointwise[..., 0], pointwise[..., 1]

    def dyad_mask(self):
        """(N, N) boolean: the dyads of one time step"""
        N = self.n_nodes
        return ~np.eye(N, dtype=bool) if self.is_directed else np.triu(np.ones((N, N), dtype=bool), 1)

    def summary(self):
        """Text table: the estimate in total and per time step, and the histogram of k"""
        T = self.elpd_loo_t.shape[0]
        head = '%-12s %14s' % ('', 'total') + ''.join(' %14s' % ('t=%d' % t) for t in range(T))
        lines = ['PSIS-LOO: %d samples, %d dyads (%s), r_eff = 1'
                 % (self.n_samples, self.n_dyads, 'directed' if self.is_directed else 'undirected'), head]

        def row(label, total, per_t, fmt='%14.6g'):
            lines.append('%-12s ' % label + fmt % total + ''.join(' ' + fmt % v for v in per_t))

        row('elpd_loo', self.elpd_loo, self.elpd_loo_t)
        row('se_elpd_loo', self.se_elpd_loo, self.se_elpd_loo_t)
        row('p_loo', self.p_loo, self.p_loo_t)
        row('looic', self.looic, self.looic_t)
        row('lppd', self.lppd, self.lppd_t)
        lines.append('Pareto k (threshold %.3g):' % self.k_threshold)
        lo = ['-inf'] + ['%.3g' % e for e in self.k_edges]
        hi = ['%.3g' % e for e in self.k_edges] + ['inf']
        for b in range(self.k_hist.shape[0]):
            row('[%s, %s)' % (lo[b], hi[b]), self.k_hist[b], self.k_hist_t[:, b], '%14d')
        row('n_bad', self.n_bad, self.n_bad_t, '%14d')
        row('n_unfitted', self.n_unfitted, self.n_unfitted_t, '%14d')
        lines.append('%-12s %14.6g' % ('max_k', self.max_k))
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def loo(model, n_samples=None, pointwise=False):
    """PSIS-LOO of a fitted ``DynamicNetworkLSM`` (undirected, directed or case-control),
    ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM``: ``elpd_loo`` for comparing fits of the same
    network as ``information_criteria`` does, and the Pareto shape ``k`` of every dyad, which says where
    the estimate (and WAIC) cannot be trusted.

    The samples, the observed network (``Y_fit_``) and the likelihood are those of
    ``information_criteria``; ``r_eff`` is taken as 1.  ``pointwise=True`` also returns the per-dyad
    ``elpd_loo`` and ``k`` (two (T, N, N) arrays), which ``compare_loo`` needs.

    Returns a ``LooResult``.
    """
    ids = sample_rows(model, n_samples)
    directed = bool(model.is_directed)
    Xs, ic, radii = trace_samples(model, ids)
    S, T, N, D = Xs.shape
    edges = k_edges(S)
    bits = pack_network(observed_network(model))
    with model_chain(model, T, N, D, directed) as chain:
        out = chain.loo_accumulate(bits, Xs, ic, radii, k_edges=edges, want_pointwise=pointwise)
    return LooResult(ids, S, out[0], edges, out[1], out[2], directed, N, out[3] if pointwise else None)


def compare_loo(a, b):
    """Difference of two fits of the same network in expected log predictive density.

    ``a`` and ``b`` are ``LooResult``s with ``pointwise=True``.  Returns ``(elpd_diff, se_diff)``:
    ``elpd_diff = elpd_loo(a) - elpd_loo(b)`` (positive: ``a`` predicts better) and its standard error
    ``sqrt(n Var_dyads(elpd_a,ij - elpd_b,ij))`` from the paired pointwise values."""
    for r in (a, b):
        if not isinstance(r, LooResult):
            raise ValueError('compare_loo takes two LooResult objects')
        if r.pointwise_elpd_loo is None:
            raise ValueError('both results need the pointwise arrays: loo(model, pointwise=True)')
    if a.pointwise_elpd_loo.shape != b.pointwise_elpd_loo.shape:
        raise ValueError('the results are of different networks: shapes %s and %s'
                         % (a.pointwise_elpd_loo.shape, b.pointwise_elpd_loo.shape))
    if a.is_directed != b.is_directed:
        raise ValueError('a directed and an undirected result do not share their dyads')
    mask = a.dyad_mask()
    d = (a.pointwise_elpd_loo - b.pointwise_elpd_loo)[:, mask]
    n = d.size
    diff = float(d.sum())
    se = float(np.sqrt(n * np.var(d, ddof=1))) if n > 1 else 0.0
    return diff, se
