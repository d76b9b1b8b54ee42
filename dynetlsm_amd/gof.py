"""Posterior predictive goodness of fit of a fitted dynamic latent space model.

The reference has no counterpart; the check is the one latentnet's and ergm's ``gof()`` make.
Networks are drawn from the model at posterior samples of the trace and their structural statistics
- edges, density, reciprocity, the degree distribution and the edgewise shared partners (ESP) - are
compared with those of the observed network.  The draws and the statistics run on the device
(``Chain.gof_simulate``, ``Chain.gof_observed``: csrc/kernels_gof.hpp); the host derives the
triangle counts, transitivity and the Monte Carlo p-values from the integer records.

Two further families look at what makes the model dynamic and at structure beyond two hops
(``Chain.gof_dynamic_simulate``, ``Chain.gof_dynamic_observed``: csrc/kernels_gof_dynamic.hpp):
``statistics='temporal'`` - the overlap of every pair of time steps, ties persisted, formed and
dissolved, the persistence-degree histogram and the shared partners of newly formed ties - and
``statistics='geodesic'`` - the distribution of shortest-path lengths.  The draws at t and t + 1
are independent given the positions, so all persistence of ties comes from persistence of positions.
"""
import numpy as np

from ._trace import model_chain, observed_network, sample_rows, trace_samples
from .engine import pack_network
from .lsm import check_random_state

__all__ = ['posterior_predictive_check', 'GofResult', 'derive_statistics', 'mc_p_values',
           'network_statistics_from_records', 'derive_dynamic_statistics', 'FAMILIES']

FAMILIES = ('structural', 'temporal', 'geodesic')


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


def _ratio(num, den):
    """num / den, 0 where den is 0"""
    num = np.asarray(num, dtype=np.float64)
    den = np.asarray(den, dtype=np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def derive_dynamic_statistics(overlap, steps, geodesic, edges, N, is_directed):
    """The named statistics of the records over time (layouts: include/dynetlsm_hip.h,
    dlsm_gof_dynamic_simulate); a leading sample axis is carried through.

    From ``overlap`` (..., T, T) and ``steps`` (..., T - 1, 2N) (both None: left out), with ``edges``
    (..., T) (None: the diagonal of ``overlap``): 'overlap'; 'persisted', 'formed', 'dissolved'
    (..., T - 1), the dyads of step t -> t+1 present at both, at t+1 only, at t only; 'persistence',
    persisted / edges_t (0 without edges); 'stability' (..., T - 1), for lag l = 1..T-1 the sum over t of
    overlap[t, t+l] over the sum of edges_t over the t that have a partner; 'persist_degree' and
    'formed_sp' (..., T - 1, N).  From ``geodesic`` (..., T, N) (None: left out): 'geodesic';
    'unreachable', its bin 0; 'mean_geodesic', the mean length over the connected pairs (0 without any);
    'diameter', the largest length that occurs.  A dyad is an unordered pair (undirected) or an arc."""
    out = {}
    if overlap is not None:
        overlap = np.asarray(overlap)
        T = overlap.shape[-1]
        idx = np.arange(T)
        e = overlap[..., idx, idx] if edges is None else np.asarray(edges)
        out['overlap'] = overlap
        pers = overlap[..., idx[:-1], idx[1:]]
        out['persisted'] = pers
        out['formed'] = e[..., 1:] - pers
        out['dissolved'] = e[..., :-1] - pers
        out['persistence'] = _ratio(pers, e[..., :-1])
        lag_sum = np.stack([overlap[..., idx[:T - l], idx[l:]].sum(-1) for l in range(1, T)], axis=-1) \
            if T > 1 else np.zeros(overlap.shape[:-2] + (0,), dtype=np.int64)
        lag_den = np.stack([e[..., :T - l].sum(-1) for l in range(1, T)], axis=-1) \
            if T > 1 else np.zeros(overlap.shape[:-2] + (0,), dtype=np.int64)
        out['stability'] = _ratio(lag_sum, lag_den)
        steps = np.asarray(steps)
        out['persist_degree'] = steps[..., :N]
        out['formed_sp'] = steps[..., N:2 * N]
    if geodesic is not None:
        geodesic = np.asarray(geodesic)
        k = np.arange(N)
        out['geodesic'] = geodesic
        out['unreachable'] = geodesic[..., 0]
        out['mean_geodesic'] = _ratio(geodesic @ k, geodesic[..., 1:].sum(-1))
        out['diameter'] = np.where(geodesic[..., 1:] > 0, k[1:], 0).max(axis=-1) if N > 1 \
            else np.zeros(geodesic.shape[:-1], dtype=np.int64)
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

    With the temporal and geodesic families (``derive_dynamic_statistics``) the names and shapes are
    'overlap' (T, T); 'persisted', 'formed', 'dissolved', 'persistence' (T - 1,) per step; 'stability'
    (T - 1,) per lag; 'persist_degree', 'formed_sp' (T - 1, N); 'geodesic' (T, N); 'unreachable',
    'mean_geodesic', 'diameter' (T,) - simulated with a leading S.
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
            if 'edges' in d:
                T = d['edges'].shape[axis]
                out['density'] = out['edges'] / (T * _n_possible(self.n_nodes, self.is_directed))
            if 'transitivity' in d:
                k = np.arange(self.n_nodes)
                closed = out['esp'] @ k
                triples = out['degree'] @ (k * (k - 1) // 2)
                out['transitivity'] = np.where(triples > 0, closed / np.maximum(triples, 1), 0.0)
            if 'overlap' in d:
                # over the steps t -> t+1: counts summed, persistence as the ratio of the pooled counts
                for name in ('persisted', 'formed', 'dissolved'):
                    out[name] = d[name].sum(axis=axis)
                out['persistence'] = _ratio(out['persisted'], out['persisted'] + out['dissolved'])
                out['stability'] = d['stability']
            if 'geodesic' in d:
                out['geodesic'] = d['geodesic'].sum(axis=axis)
                out['unreachable'] = d['unreachable'].sum(axis=axis)
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
        if 'persistence' in obs:
            for name in ('persistence', 'formed', 'dissolved'):
                row(name, obs[name], sim[name])
            for lag in range(1, min(obs['stability'].shape[-1], 5) + 1):
                row('stability[%d]' % lag, obs['stability'][lag - 1], sim['stability'][:, lag - 1])
        if 'geodesic' in obs:
            nz = np.nonzero((obs['geodesic'][1:] > 0) | (sim['geodesic'][:, 1:] > 0).any(axis=0))[0]
            for k in range(1, int(nz[-1]) + 2 if nz.size else 1):
                row('geodesic[%d]' % k, obs['geodesic'][k], sim['geodesic'][:, k])
            row('unreachable', obs['unreachable'], sim['unreachable'])
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _families(statistics):
    """'structural' | 'temporal' | 'geodesic' | 'all' | a tuple of the first three -> the tuple, in
    the order of FAMILIES"""
    if isinstance(statistics, str):
        names = FAMILIES if statistics == 'all' else (statistics,)
    else:
        try:
            names = tuple(statistics)
        except TypeError:
            names = (statistics,)
    bad = [n for n in names if n not in FAMILIES]
    if bad or not names:
        raise ValueError("statistics must be 'structural', 'temporal', 'geodesic', 'all' or a tuple of the "
                         "first three, got %r" % (statistics,))
    return tuple(f for f in FAMILIES if f in names)


def posterior_predictive_check(model, n_samples=100, random_state=None, statistics='structural'):
    """Posterior predictive goodness-of-fit check of a fitted ``DynamicNetworkLSM`` (undirected,
    directed or case-control), ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM``.

    One network per time step is drawn at each of ``n_samples`` trace rows, evenly spaced over the
    kept rows (after the burn-in), from the exact likelihood of the model: ``expit(b - |x_i - x_j|)``
    undirected, the directed model of ``metrics.py`` (probas_) for directed and case-control fits.
    The observed network is ``Y_fit_``, the network the chain was fit to: if the data had missing
    dyads, these are their imputed values.  Both the observed and the simulated statistics cover all
    dyads.  ``random_state`` (default: the model's ``random_state``) seeds the draws, so the same
    call returns the same result.

    ``statistics`` chooses the families: 'structural' (the default: the statistics above, one time step
    at a time), 'temporal' (tie persistence from one step to the next; needs T >= 2), 'geodesic' (the
    shortest-path lengths: about N^2 W row-word reads per network, the slowest family), 'all', or a tuple
    of the first three.  The seed does not depend on it: every family of one ``random_state`` describes
    the same drawn networks.

    Returns a ``GofResult``.
    """
    families = _families(statistics)
    if not hasattr(model, 'Y_fit_') or not hasattr(model, 'intercepts_'):
        raise ValueError('Model not fit.')
    if 'temporal' in families and np.shape(model.Y_fit_)[0] < 2:
        raise ValueError("statistics='temporal' needs at least two time steps, the model has T = %d"
                         % np.shape(model.Y_fit_)[0])
    int(n_samples)            # (None is a TypeError: here the number of samples is required)
    ids = sample_rows(model, n_samples)
    directed = bool(model.is_directed)
    rng = check_random_state(model.random_state if random_state is None else random_state)
    seed = int(rng.randint(0, 2 ** 31 - 1)) | (int(rng.randint(0, 2 ** 31 - 1)) << 31)
    Xs, ic, radii = trace_samples(model, ids)
    _, T, N, D = Xs.shape
    temporal, geodesic = 'temporal' in families, 'geodesic' in families
    observed, simulated = {}, {}
    with model_chain(model, T, N, D, directed) as chain:
        bits = pack_network(observed_network(model))
        if 'structural' in families:
            observed = derive_statistics(chain.gof_observed(bits), N, directed)
            simulated = derive_statistics(chain.gof_simulate(Xs, ic, radii, seed=seed), N, directed)
        if temporal or geodesic:
            obs_rec = chain.gof_dynamic_observed(bits, temporal=temporal, geodesic=geodesic)
            sim_rec = chain.gof_dynamic_simulate(Xs, ic, radii, seed=seed, temporal=temporal,
                                                 geodesic=geodesic)
    if temporal or geodesic:
        observed.update(derive_dynamic_statistics(*obs_rec, None, N, directed))
        simulated.update(derive_dynamic_statistics(*sim_rec, None, N, directed))
    return GofResult(ids, observed, simulated, directed, N)
