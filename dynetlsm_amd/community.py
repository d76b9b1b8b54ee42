"""Community structure of the posterior of a clustered dynamic latent space model (``DynamicNetworkHDPLPCM``,
``DynamicNetworkLPCM``): how strong the communities are and how sure the posterior is of it, how dense each
community is and how densely it is tied to the others, how embedded each node is in its own community, and who
changes community between t and t + 1.

The reference has ``modularity(Y, z)`` (network_statistics.py:31-61): one labelling, a dense ``S^T B S`` per time
step on the host.  Here the device counts, for every stored labelling (s, t) against the bit-packed network
(``Chain.community_accumulate``: csrc/kernels_community.hpp; every count is of ordered pairs, an undirected tie
counts twice; a tie is a set bit whose dyad is not excluded),

    clusters      per cluster a: its nodes n_a, the ties inside it W_a, its out-volume and in-volume (the ties that
                  leave and that reach its nodes; equal for undirected models) and the excluded ordered dyads in it
    node_within   per node, over the samples, its ties into its own cluster
    node_switch   per node and step t -> t + 1, the samples in which its label changed; ``moved``: per sample
    blocks        for the selected labelling ``z_`` alone: ties and excluded ordered dyads from cluster a to b

and ``CommunityResult`` divides on the host.  Every quantity is invariant to the names of the labels within a
sample, or is defined against ``z_``: label switching across samples does no harm.

Modularity, as the reference defines it, per time step with W = sum_a W_a:

    undirected    2m = sum_a vol_a,          Q = [W - sum_a vol_a^2 / (2m)] / (2m)
    directed      m = sum_a vol_out_a,       Q = [W - sum_a ((vol_out_a + vol_in_a) / 2)^2 / (2m)] / (2m)

(the directed form is the reference's: the symmetrised network with its own 2m), and the mean over the time steps.
A time step without a tie has no modularity: NaN in ``modularity_t_samples``, and ``modularity_samples`` is the
``nanmean`` over the steps (NaN when no step has a tie).
"""
import warnings

import numpy as np

from ._trace import model_chain, observed_network, sample_rows
from .engine import pack_network
from .probabilities import _ints
from .scores import _excluded_dyads

__all__ = ['community_structure', 'CommunityResult', 'modularity_from_clusters']

SIZE, WITHIN, VOL_OUT, VOL_IN, EXCLUDED = range(5)


def _div(num, den):
    """num / den elementwise, NaN where den is 0"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _nanmean(a, axis=None):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)        # an all-NaN slice gives NaN, which is the answer
        return np.nanmean(a, axis=axis)


def modularity_from_clusters(clusters, is_directed):
    """(..., K, 5) cluster tables -> (...) modularities (NaN where the network has no tie)"""
    c = np.asarray(clusters, dtype=np.float64)
    within, vol_out, vol_in = c[..., WITHIN].sum(-1), c[..., VOL_OUT], c[..., VOL_IN]
    two_m = (2.0 if is_directed else 1.0) * vol_out.sum(-1)
    degree = 0.5 * (vol_out + vol_in) if is_directed else vol_out
    null = _div((degree * degree).sum(-1), two_m)
    return _div(within - null, two_m)


class CommunityResult(object):
    """Result of ``community_structure``.  S samples, T time steps, N nodes, K label slots of the trace, G groups
    of the selected labelling ``z_``.  Counts are of ordered pairs (an undirected tie or dyad counts twice).

    sample_ids, n_samples : trace rows the result was computed from, and their number S
    modularity_t_samples (S, T), modularity_samples (S,) : modularity per step (NaN: no tie) and its nanmean
    modularity, modularity_sd : mean and standard deviation (ddof 1; NaN for S = 1) of ``modularity_samples``
    modularity_interval(level=0.9) : its central posterior interval
    n_clusters_samples (S, T) : labels in use
    density_within_samples, density_between_samples (S, T) : ties over observed dyads inside clusters and across
                       them (NaN: no such dyad); ``density_ratio_samples`` their ratio; ``density_within``,
                       ``density_between``, ``density_ratio``: the means over samples and steps
    embeddedness (T, N) : posterior mean of the share of a node's ties (directed: out-ties) that stay inside its
                       own cluster; NaN where the node has no tie
    switch_proba (T - 1, N) : P(z_{t+1,i} != z_{t,i}); n_moved_samples (S, T - 1): nodes that changed cluster
    groups (G,), z (T, N) : the labels of ``z_`` in use, and ``z_`` renumbered 0..G-1 in their order
    block_ties, block_dyads (T, G, G) : ties and observed dyads from group a to group b; block_density: their
                       ratio (NaN: no dyad); flows (T - 1, G, G): nodes in group a at t and in b at t + 1
    modularity_selected, modularity_selected_t (T,) : the modularity of ``z_``
    counts           : the integer tables as Python ints: ``clusters`` (S, T, K, 5), ``node_within`` (T, N),
                       ``node_switch`` (T - 1, N), ``moved`` (S, T - 1), ``selected_clusters`` (T, G, 5),
                       ``selected_blocks`` (T, G, G, 2)
    """

    def __init__(self, sample_ids, clusters, node_within, node_switch, moved, degree, n_excluded_t, is_directed,
                 selected_z=None, selected_clusters=None, selected_blocks=None):
        self.sample_ids = sample_ids
        self.is_directed = bool(is_directed)
        cl = np.asarray(clusters, dtype=np.int64)
        S, T, K, _ = cl.shape
        degree = np.asarray(degree, dtype=np.int64).reshape(T, -1)
        N = degree.shape[1]
        self.n_samples, self.n_time_steps, self.n_nodes, self.n_components = S, T, N, K
        nw = np.asarray(node_within, dtype=np.int64).reshape(T, N)
        sw = np.asarray(node_switch, dtype=np.int64).reshape(T - 1, N)
        mv = np.asarray(moved, dtype=np.int64).reshape(S, T - 1)
        self.counts = {'clusters': _ints(cl), 'node_within': _ints(nw), 'node_switch': _ints(sw), 'moved': _ints(mv)}
        self.modularity_t_samples = modularity_from_clusters(cl, self.is_directed)
        self.modularity_samples = _nanmean(self.modularity_t_samples, axis=1)
        self.modularity = float(_nanmean(self.modularity_samples))
        ok = self.modularity_samples[~np.isnan(self.modularity_samples)]
        self.modularity_sd = float(np.std(ok, ddof=1)) if ok.size > 1 else float('nan')
        size = cl[..., SIZE]
        self.n_clusters_samples = (size > 0).sum(-1)
        within, ties = cl[..., WITHIN].sum(-1), cl[..., VOL_OUT].sum(-1)
        dyads_within = (size * (size - 1) - cl[..., EXCLUDED]).sum(-1)
        dyads = N * (N - 1) - np.asarray(n_excluded_t, dtype=np.int64).reshape(1, T)
        self.density_within_samples = _div(within, dyads_within)
        self.density_between_samples = _div(ties - within, dyads - dyads_within)
        self.density_ratio_samples = _div(self.density_within_samples, self.density_between_samples)
        self.density_within = float(_nanmean(self.density_within_samples))
        self.density_between = float(_nanmean(self.density_between_samples))
        self.density_ratio = float(_nanmean(self.density_ratio_samples))
        self.embeddedness = _div(nw, S * degree)
        self.switch_proba = sw / float(S)
        self.n_moved_samples = mv
        self.groups = self.z = self.block_ties = self.block_dyads = self.block_density = self.flows = None
        self.modularity_selected_t, self.modularity_selected = None, float('nan')
        if selected_z is not None:
            self._selected(selected_z, selected_clusters, selected_blocks)

    def _selected(self, z, clusters, blocks):
        T, N = self.n_time_steps, self.n_nodes
        self.groups, inv = np.unique(np.asarray(z).ravel(), return_inverse=True)
        self.z = inv.reshape(T, N).astype(np.int64)
        G = len(self.groups)
        cl = np.asarray(clusters, dtype=np.int64).reshape(T, G, 5)
        bl = np.asarray(blocks, dtype=np.int64).reshape(T, G, G, 2)
        self.counts['selected_clusters'], self.counts['selected_blocks'] = _ints(cl), _ints(bl)
        n = cl[..., SIZE]
        self.block_ties = bl[..., 0].copy()
        self.block_dyads = n[:, :, None] * n[:, None, :] - np.eye(G, dtype=np.int64) * n[:, :, None] - bl[..., 1]
        self.block_density = _div(self.block_ties, self.block_dyads)
        self.flows = np.zeros((T - 1, G, G), dtype=np.int64)
        for t in range(T - 1):
            self.flows[t] = np.bincount(self.z[t] * G + self.z[t + 1], minlength=G * G).reshape(G, G)
        self.modularity_selected_t = modularity_from_clusters(cl, self.is_directed)
        self.modularity_selected = float(_nanmean(self.modularity_selected_t))

    def modularity_interval(self, level=0.9):
        """central ``level`` posterior interval of ``modularity_samples`` (samples without any tie left out)"""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError('level must lie in (0, 1), got %r' % (level,))
        ok = self.modularity_samples[~np.isnan(self.modularity_samples)]
        if not ok.size:
            return float('nan'), float('nan')
        lo, hi = np.quantile(ok, [(1 - level) / 2, (1 + level) / 2])
        return float(lo), float(hi)

    def most_mobile(self, k=10):
        """The ``k`` nodes that change cluster most: rows (node, expected number of changes over the T - 1 steps),
        largest first (ties: the lower node first)"""
        expected = self.switch_proba.sum(axis=0)
        order = np.argsort(-expected, kind='stable')[:max(int(k), 0)]
        return [(int(i), float(expected[i])) for i in order]

    def summary(self):
        """Text table: modularity, clusters in use, densities and moved nodes, pooled and per time step"""
        T = self.n_time_steps
        head = '%-22s %14s' % ('', 'pooled') + ''.join(' %14s' % ('t=%d' % t) for t in range(T))
        lo, hi = self.modularity_interval(0.9)
        lines = ['community structure: %d samples, %d nodes (%s); modularity %.6g (sd %.3g, 90%% interval %.6g .. %.6g)'
                 % (self.n_samples, self.n_nodes, 'directed' if self.is_directed else 'undirected', self.modularity,
                    self.modularity_sd, lo, hi), head]

        def row(label, total, per_t, fmt='%14.6g'):
            lines.append('%-22s ' % label + fmt % total + ''.join(' ' + fmt % v for v in per_t))

        row('modularity', self.modularity, _nanmean(self.modularity_t_samples, axis=0))
        if self.modularity_selected_t is not None:
            row('modularity of z_', self.modularity_selected, self.modularity_selected_t)
        row('clusters in use', self.n_clusters_samples.mean(), self.n_clusters_samples.mean(axis=0))
        row('density within', self.density_within, _nanmean(self.density_within_samples, axis=0))
        row('density between', self.density_between, _nanmean(self.density_between_samples, axis=0))
        row('within / between', self.density_ratio, _nanmean(self.density_ratio_samples, axis=0))
        row('embeddedness', _nanmean(self.embeddedness), _nanmean(self.embeddedness, axis=1))
        if T > 1:
            moved = self.n_moved_samples.mean(axis=0)
            lines.append('%-22s ' % 'nodes moved' + '%14.6g' % moved.sum() + ' %14s' % ''
                         + ''.join(' %14.6g' % v for v in moved))
            lines.append('most mobile nodes: ' + ', '.join('%d (%.3g)' % r for r in self.most_mobile(5)))
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _labels(model):
    if not hasattr(model, 'Y_fit_') or not hasattr(model, 'intercepts_'):
        raise ValueError('Model not fit.')
    try:
        zs = model.zs_
    except AttributeError:
        zs = None
    if zs is None:
        raise ValueError('the model has no labels (zs_): community_structure needs a DynamicNetworkHDPLPCM or a '
                         'DynamicNetworkLPCM, got %s' % type(model).__name__)
    return zs


def community_structure(model, n_samples=None, batch=0):
    """Community structure of the posterior of a fitted ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM``,
    undirected or directed: the modularity of every stored labelling (the reference's definition, with its time
    average) and its posterior mean, standard deviation and interval, the clusters in use, the tie density inside
    and across clusters, every node's embeddedness in its own cluster and its probability of changing cluster
    between consecutive time steps, and - for the selected labelling ``z_`` - block ties, dyads and densities, the
    flows of nodes between groups and its modularity.  The counting runs on the device in one pass over the labels.

    The samples are the kept rows of the trace (after the burn-in), or ``n_samples`` of them evenly spaced, as
    ``in_sample_scores`` picks them.  The observed network is ``Y_fit_``; the dyads that were missing in the data
    (``missing_index_`` of a ``sample_missing=True`` fit, ``nan_mask_``) are neither ties nor dyads.  ``batch``:
    samples staged on the device at a time (0: automatic); the result does not depend on it.

    A time step without a tie has no modularity (NaN), and a sample's modularity is the ``nanmean`` over its steps.

    Returns a ``CommunityResult``.
    """
    zs_all = _labels(model)
    ids = sample_rows(model, n_samples)
    if int(batch) != batch or int(batch) < 0:
        raise ValueError('batch must be a non-negative integer, got %r' % (batch,))
    directed = bool(model.is_directed)
    zs = np.ascontiguousarray(np.asarray(zs_all)[ids], dtype=np.int64)
    S, T, N = zs.shape
    Y = observed_network(model)
    bits = pack_network(Y)
    excluded = _excluded_dyads(model, Y.shape, directed)
    mask = None
    n_excluded_t = np.zeros(T, dtype=np.int64)
    if excluded is not None:
        mask = pack_network(excluded)
        if not directed:
            excluded = excluded | excluded.transpose(0, 2, 1)
        excluded[:, np.arange(N), np.arange(N)] = False
        n_excluded_t = excluded.sum(axis=(1, 2))
        Y &= ~excluded
    degree = Y.sum(axis=2)
    groups, z_sel = np.unique(np.asarray(model.z_).ravel(), return_inverse=True)
    z_sel = z_sel.reshape(1, T, N).astype(np.int64)
    K = int(model.n_components)
    D =int(np.shape(model.X_)[-1])
    with model_chain(model, T, N, D, directed) as chain:
        clusters, node_within, node_switch, moved, _ = chain.community_accumulate(bits, zs, K, mask=mask,
                                                                                  batch=int(batch))
        sel_clusters, _, _, _, sel_blocks = chain.community_accumulate(bits, z_sel, len(groups), mask=mask,
                                                                       want_blocks=True)
    return CommunityResult(ids, clusters, node_within, node_switch, moved, degree, n_excluded_t, directed,
                           selected_z=z_sel[0], selected_clusters=sel_clusters[0], selected_blocks=sel_blocks[0])
