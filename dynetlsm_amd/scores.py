"""In-sample scores of a fitted dynamic latent space model: the AUC and the mean log-loss of the
posterior-mean edge probability over the observed dyads, per time step and pooled.

The reference has ``auc_`` (metrics.py:10-24): the probabilities of the one selected sample as dense
(T, N, N) arrays on the host, sorted by scikit-learn.  Here the device forms, for every dyad,

    pbar = (1 / S) sum_s expit(eta_s)

over S posterior samples (eta: ``b - |x_i - x_j|`` undirected, the directed model of ``metrics.py``
(probas_) for directed and case-control fits), counts a 24-bit rank key of pbar into histograms and
returns exact integers (``Chain.score_accumulate``: csrc/kernels_score.hpp, on the shared pass of
csrc/kernels_dyad_pass.hpp):

    n_pos, n_neg   scored dyads with y = 1 / y = 0
    u2             sum_b pos_b (2 cumneg_b + neg_b): twice the Mann-Whitney statistic of the keys
    ties           sum_b pos_b neg_b

``auc = u2 / (2 n_pos n_neg)``.  Only pairs inside one bin (2^15 bins per octave of pbar) can be ordered
differently by pbar itself, so the exact AUC of pbar lies within ``auc_bound = ties / (2 n_pos n_neg)`` of
``auc``.  ``log_loss`` is the mean of ``-[y log pbar + (1 - y) log(1 - pbar)]``.
"""
import math

import numpy as np

from ._trace import model_chain, observed_network, point_estimate, sample_rows, trace_samples
from .engine import pack_network

__all__ = ['in_sample_scores', 'scores_from_counts', 'ScoreResult']


def _ratio(num, den):
    """num / den of two exact integers, correctly rounded (NaN for den = 0)"""
    return int(num) / int(den) if den else float('nan')


def scores_from_counts(counts, logloss_sum, sample_ids=None, is_directed=False):
    """The ``ScoreResult`` of what ``Chain.score_accumulate`` returns: ``counts`` (T + 1, 4) integers
    (n_pos, n_neg, u2, ties per time step, row T pooled) and ``logloss_sum`` (T,)."""
    # (Python ints throughout: u2 can exceed 2^63, which a mixed numpy conversion would turn into floats)
    rows = [[int(v) for v in row] for row in (counts.tolist() if isinstance(counts, np.ndarray) else counts)]
    lls = [float(v) for v in np.asarray(logloss_sum, dtype=np.float64).ravel()]
    if any(len(row) != 4 for row in rows) or len(rows) != len(lls) + 1:
        raise ValueError('counts must be (T + 1, 4) and logloss_sum (T,)')
    return ScoreResult(sample_ids, rows, lls, is_directed)


class ScoreResult(object):
    """Result of ``in_sample_scores``.

    Pooled over time: ``auc``, ``auc_bound`` (the exact AUC of the posterior-mean probabilities is
    within ``auc_bound`` of ``auc``), ``log_loss``, ``n_pos``, ``n_neg``, ``n``; per time step the
    (T,) arrays ``auc_t``, ``auc_bound_t``, ``log_loss_t``, ``n_pos_t``, ``n_neg_t``, ``n_t``.  The AUC
    and its bound are NaN where a class is empty, the log-loss where no dyad is scored.

    sample_ids : trace rows the scores were computed from (None: the point estimate)
    counts     : (T + 1, 4) Python ints n_pos, n_neg, u2, ties; row T pooled
    """

    def __init__(self, sample_ids, counts, logloss_sum, is_directed=False):
        self.sample_ids = sample_ids
        self.is_directed = bool(is_directed)
        self.counts = counts
        T = len(logloss_sum)

        def derive(row, ll):
            n_pos, n_neg, u2, ties = row
            den = 2 * n_pos * n_neg
            return _ratio(u2, den), _ratio(ties, den), (ll / (n_pos + n_neg) if n_pos + n_neg else float('nan'))

        per_t = [derive(counts[t], logloss_sum[t]) for t in range(T)]
        self.auc_t = np.array([v[0] for v in per_t], dtype=np.float64)
        self.auc_bound_t = np.array([v[1] for v in per_t], dtype=np.float64)
        self.log_loss_t = np.array([v[2] for v in per_t], dtype=np.float64)
        self.n_pos_t = np.array([counts[t][0] for t in range(T)], dtype=np.int64)
        self.n_neg_t = np.array([counts[t][1] for t in range(T)], dtype=np.int64)
        self.n_t = self.n_pos_t + self.n_neg_t
        self.logloss_sum_t = np.array(logloss_sum, dtype=np.float64)
        self.n_pos, self.n_neg = counts[T][0], counts[T][1]
        self.n = self.n_pos + self.n_neg
        self.auc, self.auc_bound, self.log_loss = derive(counts[T], math.fsum(logloss_sum))

    def summary(self):
        """Text table: the scores pooled and per time step"""
        T = self.auc_t.shape[0]
        head = '%-10s %14s' % ('', 'pooled') + ''.join(' %14s' % ('t=%d' % t) for t in range(T))
        what = ('the point estimate' if self.sample_ids is None
                else 'posterior mean of %d samples' % len(self.sample_ids))
        lines = ['in-sample scores: %s, %d dyads (%s)'
                 % (what, self.n, 'directed' if self.is_directed else 'undirected'), head]

        def row(label, total, per_t, fmt):
            lines.append('%-10s ' % label + fmt % total + ''.join(' ' + fmt % v for v in per_t))

        row('auc', self.auc, self.auc_t, '%14.6f')
        row('auc_bound', self.auc_bound, self.auc_bound_t, '%14.3g')
        row('log_loss', self.log_loss, self.log_loss_t, '%14.6g')
        row('n_pos', self.n_pos, self.n_pos_t, '%14d')
        row('n_neg', self.n_neg, self.n_neg_t, '%14d')
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _excluded_dyads(model, shape, directed):
    """(T, N, N) boolean of the dyads that were not observed - ``missing_index_`` of a
    ``sample_missing=True`` fit and ``nan_mask_`` where the estimator sets it - or None"""
    M = None
    index = getattr(model, 'missing_index_', None)
    if index is not None and len(index):
        index = np.asarray(index)
        M = np.zeros(shape, dtype=bool)
        M[index[:, 0], index[:, 1], index[:, 2]] = True
    nan_mask = getattr(model, 'nan_mask_', None)
    if nan_mask is not None and np.any(nan_mask):
        # one entry per dyad in the row-major order of metrics.network_auc
        N = shape[1]
        dyads = ~np.eye(N, dtype=bool) if directed else np.triu(np.ones((N, N), dtype=bool), 1)
        t, i, j = np.nonzero(np.broadcast_to(dyads, shape))
        sel = np.asarray(nan_mask, dtype=bool)
        M = np.zeros(shape, dtype=bool) if M is None else M
        M[t[sel], i[sel], j[sel]] = True
    return M


def in_sample_scores(model, n_samples=None, estimate='posterior_mean'):
    """AUC and mean log-loss of a fitted ``DynamicNetworkLSM`` (undirected, directed or case-control),
    ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM`` on the network it was fit to, per time step and
    pooled, computed on the device without a (T, N, N) array or a sort.

    ``estimate='posterior_mean'`` scores the posterior-mean edge probability over the kept rows of the
    trace (after the burn-in), or ``n_samples`` of them evenly spaced, as ``information_criteria`` picks
    them; ``estimate='map'`` scores the point estimate (``X_``, ``intercept_``, ``radii_``): the device
    counterpart of ``auc_``.  The probability is the exact one of the model, also for case-control fits.
    The observed network is ``Y_fit_``; the dyads that were missing in the data (``missing_index_`` of a
    ``sample_missing=True`` fit, ``nan_mask_``) are not scored.

    Returns a ``ScoreResult``.
    """
    if estimate not in ('posterior_mean', 'map'):
        raise ValueError("estimate must be 'posterior_mean' or 'map', got %r" % (estimate,))
    ids = sample_rows(model, n_samples)
    directed = bool(model.is_directed)
    if estimate == 'map':
        ids = None
        Xs, ic, radii = point_estimate(model)
    else:
        Xs, ic, radii = trace_samples(model, ids)
    _, T, N, D = Xs.shape
    Y = observed_network(model)
    bits = pack_network(Y)
    excluded = _excluded_dyads(model, Y.shape, directed)
    mask = pack_network(excluded) if excluded is not None else None
    with model_chain(model, T, N, D, directed) as chain:
        counts, logloss_sum = chain.score_accumulate(bits, Xs, ic, radii, mask=mask)
    return scores_from_counts(counts, logloss_sum, ids, directed)
