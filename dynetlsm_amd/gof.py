"""Posterior predictive goodness of fit of a fitted dynamic latent space model.

The reference has no counterpart; the check is the one latentnet's and ergm's ``gof()`` make.
Networks are drawn from the model at posterior samples of the trace and their structural statistics
- edges, density, reciprocity, the degree distribution and the edgewise shared partners (ESP) - are
compared with those of the observed network.  The draws and the statistics run on the device
(``Chain.gof_simulate``, ``Chain.gof_observed``: csrc/kernels_gof.hpp); the host derives the
triangle counts, transitivity and the Monte Carlo p-values from the integer records.
"""
import numpy as np

from .engine import Chain, pack_network
from .lsm import check_random_state

__all__ = ['posterior_predictive_check', 'GofResult', 'derive_statistics', 'mc_p_values',
           'network_statistics_from_records']


def network_statistics_from_records(stats, N, is_directed):
    """Split int64 records (..., 2 + 3N) into named arrays: 'edges', 'mutual', 'degree' or
    'out_degree' / 'in_degree' (histograms over k = 0..N-1) and 'esp' (edges with k shared partners)"""
    stats = np.asarray(stats)
    out = {'edges': stats[..., 0], 'esp': stats[..., 2 + 2 * N:2 + 3 * N]}
    if is_directed:
        out['mutual'] = stats[..., 1]
        out['out_degree'] = stats[..., 2:2 + N]
        out['in_degree'] = stats[..., 2 + N:2 + 2 * N]
    else:
        out['degree'] = stats[..., 2:2 + N]
    return out


def _n_possible(N, is_directed):
    """dyads of one time step as network_statistics.py:17-28 counts them"""
    return N * (N - 1) if is_directed else N * (N - 1) / 2.0


def derive_statistics(stats, N, is_directed):
    """The named statistics of records (..., 2 + 3N): those of ``network_statistics_from_records``
    plus 'density' (edges over the possible dyads) and, undirected, 'triangles' (sum_k k esp[k] / 3:
    every triangle gives three edges one shared partner each) and 'transitivity' (3 triangles over the
    connected triples sum_i deg_i (deg_i - 1) / 2; 0 without triples)"""
    out = network_statistics_from_records(stats, N, is_directed)
    out['density'] = out['edges'] / _n_possible(N, is_directed)
    if not is_directed:
        k = np.arange(N)
        closed = out['esp'] @ k
        triples = out['degree'] @ (k * (k - 1) // 2)
        out['triangles'] = closed // 3
        with np.errstate(invalid='ignore', divide='ignore'):
            out['transitivity'] = np.where(triples > 0, closed / np.maximum(triples, 1), 0.0)
    return out


def mc_p_values(simulated, observed):
    """Two-sided Monte Carlo p-value per entry: min(1, 2 min(P(sim >= obs), P(sim <= obs))) over the
    first axis of ``simulated``"""
    sim = np.asarray(simulated, dtype=np.float64)
    obs = np.asarray(observed, dtype=np.float64)
    ge = np.mean(sim >= obs, axis=0)
    le = np.mean(sim <= obs, axis=0)
    return np.minimum(1.0, 2.0 * np.minimum(ge, le))


class GofResult(object):
    """Result of ``posterior_predictive_check``.

    sample_ids : trace rows the networks were drawn at
    observed   : name -> array (T,) or (T, N) of the observed network
    simulated  : name -> array (S, T) or (S, T, N) of the drawn networks
    p_values   : name -> two-sided Monte Carlo p-value per time step (and bin)
    """
    HIST = ('degree', 'out_degree', 'in_degree', 'esp')

    def __init__(self, sample_ids, observed, simulated, is_directed, n_nodes):
        self.sample_ids = sample_ids
        self.observed = observed
        self.simulated = simulated
        self.is_directed = is_directed
        self.n_nodes = n_nodes
        self.p_values = {name: mc_p_values(simulated[name], observed[name]) for name in observed}

    def pooled(self):
        """(observed, simulated) with the time steps pooled: counts summed over t, density and
        transitivity as ratios of the pooled counts"""
        def pool(d, axis):
            out = {}
            for name in ('edges', 'mutual', 'triangles') + self.HIST:
                if name in d:
                    out[name] = d[name].sum(axis=axis)
            T = d['edges'].shape[axis]
            out['density'] = out['edges'] / (T * _n_possible(self.n_nodes, self.is_directed))
            if 'transitivity' in d:
                k = np.arange(self.n_nodes)
                closed = out['esp'] @ k
                triples = out['degree'] @ (k * (k - 1) // 2)
                out['transitivity'] = np.where(triples > 0, closed / np.maximum(triples, 1), 0.0)
            return out
        return pool(self.observed, 0), pool(self.simulated, 1)

    def summary(self):
        """Text table: per statistic (histograms per bin, time steps pooled) the observed value, the
        simulated 2.5 / 50 / 97.5 % quantiles and the two-sided Monte Carlo p-value"""
        obs, sim = self.pooled()
        lines = ['%-16s %12s %12s %12s %12s %8s' % ('statistic', 'observed', 'sim 2.5%', 'sim 50%',
                                                     'sim 97.5%', 'p')]

        def row(label, o, s):
            q = np.percentile(s, [2.5, 50, 97.5])
            p = mc_p_values(s, o)
            lines.append('%-16s %12.6g %12.6g %12.6g %12.6g %8.3f' % (label, o, q[0], q[1], q[2], p))

        for name in ('edges', 'density', 'mutual', 'triangles', 'transitivity'):
            if name in obs:
                row(name, obs[name], sim[name])
        for name in self.HIST:
            if name not in obs:
                continue
            hi = np.percentile(sim[name], 97.5, axis=0)
            nz = np.nonzero((obs[name] > 0) | (hi > 0))[0]
            for k in range(int(nz[-1]) + 1 if nz.size else 0):
                row('%s[%d]' % (name, k), obs[name][k], sim[name][:, k])
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _kept_start(model, n_rows):
    from .hdp_lpcm import DynamicNetworkHDPLPCM
    n_burn = model.n_burn_
    if isinstance(model, DynamicNetworkHDPLPCM):      # its n_burn_ counts iterations: rows are thinned
        n_burn = -(-n_burn // (model.thin or 1))
    return min(int(n_burn), n_rows - 1)


def _observed_network(model):
    Y = np.asarray(model.Y_fit_) != 0         # a new boolean array
    idx = np.arange(Y.shape[1])
    Y[:, idx, idx] = False
    return Y


def posterior_predictive_check(model, n_samples=100, random_state=None):
    """Posterior predictive goodness-of-fit check of a fitted ``DynamicNetworkLSM`` (undirected,
    directed or case-control), ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM``.

    One network per time step is drawn at each of ``n_samples`` trace rows, evenly spaced over the
    kept rows (after the burn-in), from the exact likelihood of the model: ``expit(b - |x_i - x_j|)``
    undirected, the directed model of ``metrics.py`` (probas_) for directed and case-control fits.
    The observed network is ``Y_fit_``, the network the chain was fit to: if the data had missing
    dyads, these are their imputed values.  Both the observed and the simulated statistics cover all
    dyads.  ``random_state`` (default: the model's ``random_state``) seeds the draws, so the same
    call returns the same result.

    Returns a ``GofResult``.
    """
    if not hasattr(model, 'Y_fit_') or not hasattr(model, 'intercepts_'):
        raise ValueError('Model not fit.')
    n_samples_i = int(n_samples)
    if n_samples_i != n_samples or n_samples_i < 1:
        raise ValueError('n_samples must be a positive integer, got %r' % (n_samples,))
    n_rows = np.shape(model.intercepts_)[0]
    start = _kept_start(model, n_rows)
    if n_samples_i > n_rows - start:
        raise ValueError('n_samples=%d exceeds the %d kept samples of the trace'
                         % (n_samples_i, n_rows - start))
    directed = bool(model.is_directed)
    rng = check_random_state(model.random_state if random_state is None else random_state)
    seed = int(rng.randint(0, 2 ** 31 - 1)) | (int(rng.randint(0, 2 ** 31 - 1)) << 31)

    ids = np.round(np.linspace(start, n_rows - 1, n_samples_i)).astype(np.int64)
    Xs = np.ascontiguousarray(model.Xs_[ids], dtype=np.float64)
    S, T, N, D = Xs.shape
    ic = np.asarray(model.intercepts_, dtype=np.float64)[ids].reshape(S, -1)
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    radii = np.asarray(model.radiis_, dtype=np.float64)[ids] if directed else None

    chain = model.__dict__.get('chain_')
    own = chain is None or getattr(chain, '_h', None) is None
    if own:
        chain = Chain(T, N, D, 'directed' if directed else 'undirected', device=getattr(model, 'device', 0))
    try:
        obs_rec = chain.gof_observed(pack_network(_observed_network(model)))
        sim_rec = chain.gof_simulate(Xs, ic[:, :2], radii, seed=seed)
    finally:
        if own:
            chain.close()
    observed = derive_statistics(obs_rec, N, directed)
    simulated = derive_statistics(sim_rec, N, directed)
    return GofResult(ids, observed, simulated, directed, N)
