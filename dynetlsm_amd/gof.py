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

A fourth family, ``statistics='triadic'``, is the triad census (``Chain.gof_triads_simulate``,
``Chain.gof_triads_observed``: csrc/kernels_gof_triads.hpp): the 16 Holland-Leinhardt MAN classes of a
directed network - sna's ``triad.census``, ergm's ``triadcensus`` term - or the four of an undirected one,
with the dyad census, the transitive triples and the two-paths.  The device counts, per connected pair, the
third nodes in each of their 16 states; the host maps those states to the classes by a table it derives
from one representative per class.
"""
import itertools

import numpy as np

from ._trace import model_chain, observed_network, sample_rows, trace_samples
from .engine import pack_network
from .lsm import check_random_state

__all__ = ['posterior_predictive_check', 'GofResult', 'derive_statistics', 'mc_p_values',
           'network_statistics_from_records', 'derive_dynamic_statistics', 'FAMILIES',
           'derive_triad_statistics', 'TRIAD_NAMES', 'UNDIRECTED_TRIAD_NAMES']

FAMILIES = ('structural', 'temporal', 'geodesic')       # what 'all' means
TRIADIC = 'triadic'                                     # asked for by name


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


# One representative per MAN class, in the standard order (the convention of sna and networkx), as arcs on
# the nodes A, B, C.  Everything else about the classes is derived from these below.
_TRIAD_REPRESENTATIVES = (
    ('003', ''), ('012', 'AB'), ('102', 'AB BA'), ('021D', 'BA BC'), ('021U', 'AB CB'), ('021C', 'AB BC'),
    ('111D', 'AB BA CB'), ('111U', 'AB BA BC'), ('030T', 'AB CB AC'), ('030C', 'BA CB AC'),
    ('201', 'AB BA BC CB'), ('120D', 'BA BC AC CA'), ('120U', 'AB CB AC CA'), ('120C', 'AB BC AC CA'),
    ('210', 'AB BC CB AC CA'), ('300', 'AB BA BC CB AC CA'))
TRIAD_NAMES = tuple(name for name, _ in _TRIAD_REPRESENTATIVES)
UNDIRECTED_TRIAD_NAMES = ('empty', 'edge', 'path', 'triangle')
_UNDIRECTED_CLASSES = tuple(TRIAD_NAMES.index(n) for n in ('003', '102', '201', '300'))


def _derive_triad_tables():
    """From the representatives: ``table`` (4, 4, 4), the class of the labelled triad on (i, j, k) with the
    dyad codes c of (i, j), a of (i, k) and b of (j, k) - code = arc from the first to the second node + 2 x
    the arc back -, and per class the non-null dyads, the transitive triples (ordered x -> y -> z with
    x -> z) and the two-paths (ordered x -> y -> z, x != z)"""
    nodes = (0, 1, 2)
    perms = list(itertools.permutations(nodes))

    def canonical(arcs):
        return min(tuple(sorted((p[x], p[y]) for x, y in arcs)) for p in perms)

    reps = [frozenset(('ABC'.index(a[0]), 'ABC'.index(a[1])) for a in arcs.split())
            for _, arcs in _TRIAD_REPRESENTATIVES]
    class_of = {canonical(arcs): k for k, arcs in enumerate(reps)}
    assert len(class_of) == len(reps)
    table = np.zeros((4, 4, 4), dtype=np.int64)
    for c, a, b in itertools.product(range(4), repeat=3):
        arcs = set()
        for code, (x, y) in ((c, (0, 1)), (a, (0, 2)), (b, (1, 2))):
            if code & 1:
                arcs.add((x, y))
            if code & 2:
                arcs.add((y, x))
        table[c, a, b] = class_of[canonical(arcs)]
    dyads = np.array([sum(1 for x, y in ((0, 1), (0, 2), (1, 2)) if (x, y) in r or (y, x) in r) for r in reps])
    paths = np.array([sum(1 for x, y, z in perms if (x, y) in r and (y, z) in r) for r in reps])
    trans = np.array([sum(1 for x, y, z in perms if (x, y) in r and (y, z) in r and (x, z) in r) for r in reps])
    return table, dyads, trans, paths


TRIAD_TABLE, TRIAD_DYADS, TRIAD_TRANSITIVE, TRIAD_TWO_PATHS = _derive_triad_tables()


def derive_triad_statistics(records, N, is_directed):
    """The named statistics of triad records (..., 51) (layout: include/dynetlsm_hip.h,
    dlsm_gof_triads_simulate): 'triad_census' (..., 16) in the order of ``TRIAD_NAMES``, or (..., 4)
    undirected - ``UNDIRECTED_TRIAD_NAMES``, the classes 003, 102, 201 and 300 -; 'dyad_census' (..., 3),
    mutual, asymmetric and null pairs; 'transitive_triples', the ordered (i, j, k) with i -> j, j -> k and
    i -> k; 'two_paths', i -> j -> k with i != k; 'triad_transitivity', their ratio (0 without two-paths;
    undirected, the structural family's 'transitivity').

    The records count every triad once per non-null dyad of it, so each class's sum of states is divided
    by that number; class 003, which no connected pair sees, is C(N, 3) minus the rest."""
    records = np.asarray(records, dtype=np.int64)
    states = records[..., :48].reshape(records.shape[:-1] + (3, 16))
    visits = np.zeros(records.shape[:-1] + (16,), dtype=np.int64)
    for c in (1, 2, 3):
        for k in range(1, 16):
            visits[..., k] += states[..., c - 1, TRIAD_TABLE[c].ravel() == k].sum(-1)
    census = visits // np.maximum(TRIAD_DYADS, 1)
    census[..., 0] = N * (N - 1) * (N - 2) // 6 - census[..., 1:].sum(-1)
    mutual, asym = records[..., 50], records[..., 48] + records[..., 49]
    dyad = np.stack([mutual, asym, N * (N - 1) // 2 - mutual - asym], axis=-1)
    trans, paths = census @ TRIAD_TRANSITIVE, census @ TRIAD_TWO_PATHS
    return {'triad_census': census if is_directed else census[..., list(_UNDIRECTED_CLASSES)],
            'dyad_census': dyad, 'transitive_triples': trans, 'two_paths': paths,
            'triad_transitivity': _ratio(trans, paths)}


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

    With the triadic family (``derive_triad_statistics``): 'triad_census' (T, 16) or, undirected, (T, 4);
    'dyad_census' (T, 3); 'transitive_triples', 'two_paths', 'triad_transitivity' (T,).
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
            if 'triad_census' in d:
                # counts summed, the ratio from the pooled counts
                for name in ('triad_census', 'dyad_census', 'transitive_triples', 'two_paths'):
                    out[name] = d[name].sum(axis=axis)
                out['triad_transitivity'] = _ratio(out['transitive_triples'], out['two_paths'])
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
        if 'triad_census' in obs:
            for k, name in enumerate(TRIAD_NAMES if self.is_directed else UNDIRECTED_TRIAD_NAMES):
                row('triad[%s]' % name, obs['triad_census'][k], sim['triad_census'][:, k])
            row('triad_transitivity', obs['triad_transitivity'], sim['triad_transitivity'])
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _families(statistics):
    """'structural' | 'temporal' | 'geodesic' | 'triadic' | 'all' (the first three) | a tuple of the first
    four -> the tuple, in the order of FAMILIES with 'triadic' last"""
    known = FAMILIES + (TRIADIC,)
    if isinstance(statistics, str):
        names = FAMILIES if statistics == 'all' else (statistics,)
    else:
        try:
            names = tuple(statistics)
        except TypeError:
            names = (statistics,)
    bad = [n for n in names if n not in known]
    if bad or not names:
        raise ValueError("statistics must be 'structural', 'temporal', 'geodesic', 'triadic', 'all' (the first "
                         "three) or a tuple of the first four, got %r" % (statistics,))
    return tuple(f for f in known if f in names)


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
    shortest-path lengths: about N^2 W row-word reads per network, the slowest family), 'triadic' (the
    triad census - 16 MAN classes directed, four undirected -, the dyad census, transitive triples and
    two-paths), 'all' (the first three), or a tuple of the first four.  The seed does not depend on it:
    every family of one ``random_state`` describes the same drawn networks.

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
        if TRIADIC in families:
            obs_tri = chain.gof_triads_observed(bits)
            sim_tri = chain.gof_triads_simulate(Xs, ic, radii, seed=seed)
    if temporal or geodesic:
        observed.update(derive_dynamic_statistics(*obs_rec, None, N, directed))
        simulated.update(derive_dynamic_statistics(*sim_rec, None, N, directed))
    if TRIADIC in families:
        observed.update(derive_triad_statistics(obs_tri, N, directed))
        simulated.update(derive_triad_statistics(sim_tri, N, directed))
    return GofResult(ids, observed, simulated, directed, N)
