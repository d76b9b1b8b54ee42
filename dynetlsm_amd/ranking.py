"""Link prediction from a fitted dynamic latent space model: per time step the k dyads that come first by the
posterior-mean edge probability

    pbar(t, i, j) = mean over the kept samples of expit(eta_s)     (the probability of ``edge_probabilities`` and
                                                                    ``in_sample_scores``)

among the dyads one asks about - the ties the model expects that are not in the data (``among='non_ties'``), the
observed ties it finds least plausible (``'ties'``, ranked from the smallest probability), all observed dyads, the
dyads that were missing in the data (``'missing'``: the ranking of the held-out dyads of a ``sample_missing=True``
fit) or every dyad.  The selection runs on the device (``Chain.topk_accumulate``: csrc/kernels_topk.hpp on the shared
pass of csrc/kernels_dyad_pass.hpp) and never holds more than the winners and the dyads that share the rank key of the
last one: no (T, N, N) array is formed and nothing of that size is sorted, so it serves the large N at which
``edge_probabilities(model, pointwise=True)`` does not fit.  Ties in the probability are broken by (i, j), so the
result is the same on every call.  The reference has no counterpart (``probas_`` of the one selected sample and a
dense ``argsort``).

``top_partners`` asks the per-node question - for every node its k most likely partners, its least plausible ties, or
the ranking of its held-out dyads - which the lists per time step cannot answer: at large N they lie in the few
densest neighbourhoods.  A row-wise selection has no use for the histogram per time step; each row's short list is
kept sorted on the device while the row's columns stream by (``Chain.partners_accumulate``:
csrc/kernels_partners.hpp), again without a (T, N, N) array.
"""
import collections

import numpy as np

from ._trace import model_chain, observed_network, sample_rows, trace_samples
from .engine import Chain, check_node_ids, pack_network
from .scores import _excluded_dyads

__all__ = ['top_dyads', 'TopDyadsResult', 'top_partners', 'TopPartnersResult', 'DyadList']

AMONG = Chain.TOPK_AMONG

DyadList = collections.namedtuple('DyadList', 't i j proba sd y')
DyadList.__doc__ = """Ranked dyads: time step, sender (undirected: the smaller node), receiver, posterior-mean edge
probability, its posterior standard deviation, and the bit of the network the model was fit to"""


def _ranked(proba, largest, *keys):
    """the order by (probability descending - ascending unless ``largest`` -, then ``keys`` ascending); the lists
    that ``Chain.topk_accumulate`` returns are in that order already and are not sorted again"""
    cols = (-proba if largest else proba,) + keys
    if proba.size > 1:
        ahead = np.zeros(proba.size - 1, dtype=bool)          # row r + 1 is strictly after row r
        equal = np.ones(proba.size - 1, dtype=bool)           # ... or the two agree on the keys so far
        for c in cols:
            d = np.diff(c)
            ahead |= equal & (d > 0)
            equal &= d == 0
        if not (ahead | equal).all():
            return np.lexsort(tuple(reversed(cols)))
    return np.arange(proba.size)


class TopDyadsResult(object):
    """Result of ``top_dyads``.

    t, i, j, proba, sd, y : flat arrays, grouped by time step and ranked within it: probability descending
                       (``largest=False``: ascending), then i, then j; at most ``k`` entries per time step
    eligible_t       : (T,) the dyads of each time step that the ranking chose from
    k, among, largest, is_directed, n_nodes, n_samples, sample_ids : what was asked and on which trace rows
    diagnostics      : what the device reported (``Chain.topk_accumulate``), or None
    """

    def __init__(self, sample_ids, n_samples, k, among, largest, is_directed, n_nodes, steps, eligible_t,
                 diagnostics=None):
        self.sample_ids = None if sample_ids is None else np.asarray(sample_ids)
        self.n_samples, self.k, self.among, self.largest = int(n_samples), int(k), among, bool(largest)
        self.is_directed, self.n_nodes = bool(is_directed), int(n_nodes)
        self.eligible_t = np.asarray(eligible_t, dtype=np.int64)
        self.diagnostics = diagnostics
        cols = [[] for _ in range(6)]
        for t, (i, j, y, proba, sd) in enumerate(steps):
            i, j, y = (np.asarray(a, dtype=np.int64) for a in (i, j, y))
            proba, sd = np.asarray(proba, dtype=np.float64), np.asarray(sd, dtype=np.float64)
            order = _ranked(proba, self.largest, i, j)[:self.k]
            for col, a in zip(cols, (np.full(order.size, t, dtype=np.int64), i[order], j[order], proba[order],
                                     sd[order], y[order])):
                col.append(a)
        self.n_time_steps = len(steps)
        self.t, self.i, self.j, self.proba, self.sd, self.y = (
            np.concatenate(c) if c else np.zeros(0, dtype=d)
            for c, d in zip(cols, (np.int64, np.int64, np.int64, np.float64, np.float64, np.int64)))

    def _take(self, sel):
        return DyadList(self.t[sel], self.i[sel], self.j[sel], self.proba[sel], self.sd[sel], self.y[sel])

    def at(self, t):
        """the ranked dyads of time step ``t``"""
        if not 0 <= int(t) < self.n_time_steps:
            raise ValueError('t=%r is not a time step in 0..%d' % (t, self.n_time_steps - 1))
        return self._take(self.t == int(t))

    def pooled(self, k=None):
        """the ``k`` (default: this result's k) first dyads over all time steps, by (probability, t, i, j): a subset
        of the lists per time step, since a dyad among the k first of all is among the k first of its time step"""
        k = self.k if k is None else int(k)
        if not 1 <= k <= self.k:
            raise ValueError('k=%r is not in 1..%d, the length of the lists per time step' % (k, self.k))
        return self._take(_ranked(self.proba, self.largest, self.t, self.i, self.j)[:k])

    def for_node(self, i):
        """the returned dyads that node ``i`` is part of (directed: as sender or as receiver), in this result's order"""
        if not 0 <= int(i) < self.n_nodes:
            raise ValueError('i=%r is not a node in 0..%d' % (i, self.n_nodes - 1))
        return self._take((self.i == int(i)) | (self.j == int(i)))

    def precision_at_k(self, Y_true):
        """the share of the returned dyads that are ties in ``Y_true`` (T, N, N), the full network: for an
        ``among='missing'`` ranking the held-out dyads are looked up in it, as ``metrics.heldout_scores`` scores
        them.  NaN if nothing was returned."""
        Y_true = np.asarray(Y_true)
        if Y_true.shape != (self.n_time_steps, self.n_nodes, self.n_nodes):
            raise ValueError('Y_true has shape %s, expected %s'
                             % (Y_true.shape, (self.n_time_steps, self.n_nodes, self.n_nodes)))
        if not self.t.size:
            return float('nan')
        return float(np.mean(Y_true[self.t, self.i, self.j] == 1))

    def summary(self, n=10):
        """Text table: what was ranked and the first ``n`` dyads over all time steps"""
        lines = ['top dyads: %s, %s %d per time step of %d samples (%s); eligible per time step: %s'
                 % (self.among, 'largest' if self.largest else 'smallest', self.k, self.n_samples,
                    'directed' if self.is_directed else 'undirected', ' '.join(str(int(e)) for e in self.eligible_t))]
        if self.t.size:
            first = self.pooled(min(self.k, max(1, int(n))))
            lines.append('%4s %6s %6s %10s %10s %2s' % ('t', 'i', 'j', 'proba', 'sd', 'y'))
            for row in zip(*first):
                lines.append('%4d %6d %6d %10.6f %10.6f %2d' % row)
        else:
            lines.append('(no eligible dyad)')
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def top_dyads(model, k=100, among='non_ties', largest=None, n_samples=None):
    """The ``k`` dyads of every time step that come first by the posterior-mean edge probability of a fitted
    ``DynamicNetworkLSM`` (undirected, directed or case-control), ``DynamicNetworkHDPLPCM`` or
    ``DynamicNetworkLPCM``, selected on the device without a (T, N, N) array.

    ``among`` - the dyads to choose from, against the network the model was fit to (``Y_fit_``):
    ``'non_ties'`` observed dyads without a tie: the links the model predicts; ``'ties'`` observed ties: ranked from
    the smallest probability, the ties the model finds least plausible; ``'observed'`` both; ``'missing'`` the dyads
    that were missing in the data (``missing_index_`` of a ``sample_missing=True`` fit, ``nan_mask_``): the ranking of
    the held-out dyads; ``'all'`` every dyad.  ``largest`` - rank from the largest probability; the default is True,
    and False for ``among='ties'``.  Equal probabilities are ranked by (i, j).  Fewer than ``k`` eligible dyads at a
    time step: all of them are returned.

    The samples are the kept rows of the trace (after the burn-in), or ``n_samples`` of them evenly spaced, as
    ``edge_probabilities`` picks them; at least two (each dyad comes with the posterior standard deviation of its
    probability).

    Returns a ``TopDyadsResult``.
    """
    if among not in AMONG:
        raise ValueError('among must be one of %s, got %r' % (', '.join(map(repr, AMONG)), among))
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError('k must be a positive integer, got %r' % (k,))
    if largest is None:
        largest = among != 'ties'
    ids = sample_rows(model, n_samples)
    if len(ids) < 2:
        raise ValueError('the standard deviation needs at least two samples, got %d' % len(ids))
    directed = bool(model.is_directed)
    Xs, ic, radii = trace_samples(model, ids)
    S, T, N, D = Xs.shape
    Y = observed_network(model)
    excluded = _excluded_dyads(model, Y.shape, directed)
    if among == 'missing' and excluded is None:
        raise ValueError("among='missing' needs a model with missing dyads (missing_index_ of a sample_missing=True "
                         "fit, or nan_mask_)")
    if not (np.all(np.isfinite(Xs)) and np.all(np.isfinite(ic)) and (radii is None or np.all(np.isfinite(radii)))):
        raise ValueError('the trace samples are not finite')
    bits = pack_network(Y)
    mask = pack_network(excluded) if excluded is not None else None
    with model_chain(model, T, N, D, directed) as chain:
        steps, diag = chain.topk_accumulate(bits, Xs, ic, radii, int(k), among=among, largest=bool(largest),
                                            mask=mask)
    return TopDyadsResult(ids, S, int(k), among, bool(largest), directed, N, steps, diag['eligible'], diag)


class TopPartnersResult(object):
    """Result of ``top_partners``.

    partner          : (T, N, k) int64, the partners of node i at time step t in rank order - probability descending
                       (``largest=False``: ascending), then j -, padded with -1: rows with fewer than k eligible
                       partners, and rows that were not asked for
    proba, sd        : (T, N, k) the posterior-mean edge probability of the dyad and its posterior standard deviation,
                       padded with NaN.  ``direction='out'``: of i -> partner; ``'in'``: of partner -> i
    y                : (T, N, k) int64, the dyad's bit of the network the model was fit to, padded with -1
    eligible         : (T, N) the partners that node i's ranking chose from, -1 for a node that was not asked for
    nodes            : the asked nodes, ascending (all of them unless ``nodes`` was given)
    k, among, largest, direction, is_directed, n_nodes, n_samples, sample_ids : what was asked and on which trace rows
    """

    def __init__(self, sample_ids, n_samples, k, among, largest, direction, is_directed, partner, proba, sd, y,
                 eligible):
        self.sample_ids = None if sample_ids is None else np.asarray(sample_ids)
        self.n_samples, self.k, self.among, self.largest = int(n_samples), int(k), among, bool(largest)
        self.direction, self.is_directed = direction, bool(is_directed)
        self.partner, self.y = np.asarray(partner, dtype=np.int64), np.asarray(y, dtype=np.int64)
        self.proba, self.sd = np.asarray(proba, dtype=np.float64), np.asarray(sd, dtype=np.float64)
        self.eligible = np.asarray(eligible, dtype=np.int64)
        self.n_time_steps, self.n_nodes = self.partner.shape[:2]
        for a in (self.proba, self.sd, self.y):
            if a.shape != self.partner.shape:
                raise ValueError('partner, proba, sd and y must have one shape, got %s and %s'
                                 % (self.partner.shape, a.shape))
        if self.partner.ndim != 3 or self.partner.shape[2] != self.k or self.eligible.shape != self.partner.shape[:2]:
            raise ValueError('partner must be (T, N, k=%d) and eligible (T, N), got %s and %s'
                             % (self.k, self.partner.shape, self.eligible.shape))
        self.nodes = np.nonzero((self.eligible >= 0).any(axis=0))[0]

    def _take(self, sel):
        """the entries ``sel`` (T, N, k) boolean, by (t, i, rank): the dyad is (i, partner) with i the asked node"""
        t, i, r = np.nonzero(sel & (self.partner >= 0))
        return DyadList(t, i, self.partner[t, i, r], self.proba[t, i, r], self.sd[t, i, r], self.y[t, i, r])

    def _select(self, t=None, i=None):
        sel = np.zeros(self.partner.shape, dtype=bool)
        sel[slice(None) if t is None else int(t), slice(None) if i is None else int(i)] = True
        return sel

    def _check_t(self, t):
        if not 0 <= int(t) < self.n_time_steps:
            raise ValueError('t=%r is not a time step in 0..%d' % (t, self.n_time_steps - 1))

    def for_node(self, i, t=None):
        """the ranked partners of node ``i`` as a ``DyadList`` whose i is that node, at time step ``t`` or at every
        time step in turn"""
        if not 0 <= int(i) < self.n_nodes:
            raise ValueError('i=%r is not a node in 0..%d' % (i, self.n_nodes - 1))
        if t is not None:
            self._check_t(t)
        return self._take(self._select(t, i))

    def at(self, t):
        """the lists of every node at time step ``t``, node by node"""
        self._check_t(t)
        return self._take(self._select(t))

    def as_dyads(self):
        """all entries without the padding, by (t, i, rank)"""
        return self._take(self._select())

    def _truth(self, Y_true):
        Y_true = np.asarray(Y_true)
        shape = (self.n_time_steps, self.n_nodes, self.n_nodes)
        if Y_true.shape != shape:
            raise ValueError('Y_true has shape %s, expected %s' % (Y_true.shape, shape))
        d = self.as_dyads()
        hit = (Y_true[d.t, d.j, d.i] if self.direction == 'in' else Y_true[d.t, d.i, d.j]) == 1
        return d, hit

    def precision_at_k(self, Y_true):
        """the share of the returned entries that are ties in ``Y_true`` (T, N, N), the full network
        (``direction='in'``: the tie partner -> i).  NaN if nothing was returned."""
        d, hit = self._truth(Y_true)
        return float(np.mean(hit)) if hit.size else float('nan')

    def hit_rate(self, Y_true):
        """(T,) per time step the share of the asked nodes with at least one returned partner that is a tie in
        ``Y_true`` (T, N, N)"""
        d, hit = self._truth(Y_true)
        found = np.zeros((self.n_time_steps, self.n_nodes), dtype=bool)
        found[d.t[hit], d.i[hit]] = True
        asked = self.eligible >= 0
        with np.errstate(invalid='ignore', divide='ignore'):
            return (found & asked).sum(axis=1) / asked.sum(axis=1).astype(np.float64)

    def summary(self, n=5):
        """Text table: what was ranked and the lists of the first ``n`` asked nodes at the first time step"""
        asked = self.eligible >= 0
        lines = ['top partners (%s): %s, %s %d per node of %d samples (%s); %d of %d nodes, %d time steps; '
                 'eligible partners per node: %s'
                 % (self.direction, self.among, 'largest' if self.largest else 'smallest', self.k, self.n_samples,
                    'directed' if self.is_directed else 'undirected', self.nodes.size, self.n_nodes,
                    self.n_time_steps,
                    'min %d, median %d, max %d' % (self.eligible[asked].min(), np.median(self.eligible[asked]),
                                                   self.eligible[asked].max()) if asked.any() else '-')]
        if (self.partner >= 0).any():
            lines.append('%4s %6s %6s %10s %10s %2s' % ('t', 'i', 'j', 'proba', 'sd', 'y'))
            for i in self.nodes[:max(1, int(n))]:
                for row in zip(*self.for_node(i, 0)):
                    lines.append('%4d %6d %6d %10.6f %10.6f %2d' % row)
        else:
            lines.append('(no eligible partner)')
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def top_partners(model, k=10, among='non_ties', largest=None, n_samples=None, nodes=None, direction='out'):
    """For every node (or the nodes ``nodes``) and time step the ``k`` <= 64 partners that come first by the
    posterior-mean edge probability of a fitted ``DynamicNetworkLSM`` (undirected, directed or case-control),
    ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM``: the per-node question that the lists of ``top_dyads``, which
    lie in the densest neighbourhoods, cannot answer.  Selected on the device without a (T, N, N) array.

    ``among``, ``largest``, ``n_samples`` as ``top_dyads``: the partners are chosen among the node's dyads of that
    class.  ``direction`` (directed models): ``'out'`` ranks the receivers j of sender i by p(i -> j), ``'in'`` the
    senders j of receiver i by p(j -> i); undirected models take ``'out'`` only.  Equal probabilities are ranked by
    j.  A node with fewer than ``k`` eligible partners gets all of them.

    Returns a ``TopPartnersResult``.
    """
    if among not in AMONG:
        raise ValueError('among must be one of %s, got %r' % (', '.join(map(repr, AMONG)), among))
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError('k must be a positive integer, got %r' % (k,))
    if int(k) > Chain.PARTNERS_K_MAX:
        raise ValueError('k must be at most %d, the entries of a node\'s list on the device, got %r'
                         % (Chain.PARTNERS_K_MAX, k))
    if direction not in ('out', 'in'):
        raise ValueError("direction must be 'out' or 'in', got %r" % (direction,))
    if largest is None:
        largest = among != 'ties'
    ids = sample_rows(model, n_samples)
    if len(ids) < 2:
        raise ValueError('the standard deviation needs at least two samples, got %d' % len(ids))
    directed = bool(model.is_directed)
    if direction == 'in' and not directed:
        raise ValueError("direction='in' needs a directed model: an undirected one has one probability per dyad")
    Xs, ic, radii = trace_samples(model, ids)
    S, T, N, D = Xs.shape
    if nodes is not None:
        nodes = check_node_ids(nodes, N, 'nodes')
    Y = observed_network(model)
    excluded = _excluded_dyads(model, Y.shape, directed)
    if among == 'missing' and excluded is None:
        raise ValueError("among='missing' needs a model with missing dyads (missing_index_ of a sample_missing=True "
                         "fit, or nan_mask_)")
    if not (np.all(np.isfinite(Xs)) and np.all(np.isfinite(ic)) and (radii is None or np.all(np.isfinite(radii)))):
        raise ValueError('the trace samples are not finite')
    if direction == 'in':
        # eta with the two intercepts swapped is that of the reversed dyad: rank the rows of the transposed problem
        Y = Y.transpose(0, 2, 1)
        excluded = None if excluded is None else excluded.transpose(0, 2, 1)
        ic = np.ascontiguousarray(ic[:, ::-1])
    bits = pack_network(Y)
    mask = pack_network(excluded) if excluded is not None else None
    with model_chain(model, T, N, D, directed) as chain:
        partner, proba, sd, y, eligible = chain.partners_accumulate(
            bits, Xs, ic, radii, int(k), among=among, largest=bool(largest), mask=mask, rows=nodes)
    return TopPartnersResult(ids, S, int(k), among, bool(largest), direction, directed, partner, proba, sd, y,
                             eligible)
