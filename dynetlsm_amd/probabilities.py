"""Posterior edge probabilities of a fitted dynamic latent space model: how sure the model is of every tie,
and whether its probabilities are calibrated.

The reference has ``probas_``: one number per dyad from the one selected sample.  Here the device forms, for
every dyad, over S posterior samples (the same samples and the same linear predictor eta as
``in_sample_scores``) of ``p_s = expit(eta_s)``

    mean, sd (ddof 1), and the equal-tailed credible interval at ``level``: the quantiles at
    alpha = (1 - level) / 2 and at 1 - alpha, numpy's default definition (linear interpolation at q (S - 1))

and, over the scored dyads - observed in the data and not masked, as ``in_sample_scores`` scores them -, counts
the posterior mean into integer tables (``Chain.proba_accumulate``: csrc/kernels_proba.hpp on the shared pass of
csrc/kernels_dyad_pass.hpp; probabilities are summed in units of 2^-32, at most half a unit off per dyad):

    calib       per time step and bin of the mean: dyads, ties among them, sum of the mean
    brier       sum (y - mean)^2
    node_sums   the mean of dyad (i, j) added to node i and to node j: expected degrees, no simulated networks
    hist_width  dyads per bin of upper - lower

``EdgeProbabilityResult`` turns them into a reliability table, the Brier score, the expected calibration error
``ECE = sum_b (n_b / n) |ties_b / n_b - mean predicted_b|`` and the nodes' expected degrees next to the observed
ones.

The pointwise arrays cover every dyad of the model: a dyad that was missing in the data gets its posterior
predictive probability.  They take 32 T N^2 bytes (four float64 (T, N, N) arrays); ``pointwise=False`` is the
form for large N.
"""
import numpy as np

from ._trace import model_chain, observed_network, sample_rows, trace_samples
from .engine import pack_network
from .scores import _excluded_dyads, _ratio

__all__ = ['edge_probabilities', 'EdgeProbabilityResult']

FIX = 1 << 32                                  # units of a probability in the integer tables
DEFAULT_WIDTH_EDGES = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)


def _ints(a):
    """nested lists of Python ints (a uint64 sum can exceed what a mixed numpy conversion keeps exact)"""
    return np.asarray(a).astype(object).tolist() if not isinstance(a, list) else a


class EdgeProbabilityResult(object):
    """Result of ``edge_probabilities``.

    sample_ids, n_samples, level : trace rows the result was computed from, their number S, the interval's level
    mean, sd, lower, upper : (T, N, N) float64 of every dyad (undirected: symmetric; diagonal 0), or None
                       (``pointwise=False``)
    calibration      : dict of (T + 1, n_bins) arrays, row T pooled over time: ``n`` scored dyads whose mean falls
                       into bin b = min(floor(mean n_bins), n_bins - 1), ``ties`` of them with y = 1,
                       ``mean_predicted`` and ``observed_frequency`` (NaN for an empty bin); ``bin_edges``
                       (n_bins + 1,)
    n_t, n, n_ties_t, n_ties : scored dyads and the ties among them, (T,) and pooled
    brier_t, brier   : mean of (y - mean)^2 over the scored dyads, (T,) and pooled (NaN where none is scored)
    ece_t, ece       : sum_b (n_b / n) |ties_b / n_b - mean predicted_b|, (T,) and pooled (NaN where none is scored)
    expected_degree, observed_degree : (T, N) undirected: the sum of the mean, and of y, over the scored dyads of
                       each node; directed: None, and ``expected_out_degree`` / ``expected_in_degree`` /
                       ``observed_out_degree`` / ``observed_in_degree`` (None for undirected models)
    width_edges, width_hist, width_hist_t : edges, and dyads per bin of upper - lower pooled (n_edges + 1,) and per
                       time step (T, n_edges + 1); the bin of a width is the number of edges <= it
    counts           : the integer tables as Python ints: ``calib`` (T, n_bins, 3), ``brier`` (T,), ``node_sums``
                       (T, N, 2), in units of 2^-32 where they hold probabilities
    """

    def __init__(self, sample_ids, n_samples, level, calib, brier, node_sums, width_edges, hist_width,
                 observed_degrees, is_directed, n_nodes, pointwise=None):
        self.sample_ids = sample_ids
        self.n_samples = int(n_samples)
        self.level = float(level)
        self.is_directed = bool(is_directed)
        self.n_nodes = int(n_nodes)
        calib, brier, node_sums = _ints(calib), _ints(brier), _ints(node_sums)
        self.counts = {'calib': calib, 'brier': brier, 'node_sums': node_sums}
        T = len(brier)
        n_bins = len(calib[0]) if T else 0
        self.n_bins = n_bins
        pooled = [[sum(calib[t][b][c] for t in range(T)) for c in range(3)] for b in range(n_bins)]
        tables = calib + [pooled]                                  # pooled row last
        briers = brier + [sum(brier)]

        def derive(rows, brier_fix):
            n = sum(r[0] for r in rows)
            ties = sum(r[1] for r in rows)
            pred = [_ratio(r[2], r[0] * FIX) for r in rows]
            freq = [_ratio(r[1], r[0]) for r in rows]
            ece = (sum(r[0] / n * abs(f - p) for r, f, p in zip(rows, freq, pred) if r[0]) if n else float('nan'))
            return n, ties, pred, freq, _ratio(brier_fix, n * FIX), ece

        per = [derive(rows, bf) for rows, bf in zip(tables, briers)]
        self.calibration = {
            'n': np.array([[r[0] for r in rows] for rows in tables], dtype=np.int64).reshape(T + 1, n_bins),
            'ties': np.array([[r[1] for r in rows] for rows in tables], dtype=np.int64).reshape(T + 1, n_bins),
            'mean_predicted': np.array([v[2] for v in per], dtype=np.float64).reshape(T + 1, n_bins),
            'observed_frequency': np.array([v[3] for v in per], dtype=np.float64).reshape(T + 1, n_bins),
            'bin_edges': np.arange(n_bins + 1, dtype=np.float64) / max(n_bins, 1),
        }
        self.n_t = np.array([v[0] for v in per[:T]], dtype=np.int64)
        self.n_ties_t = np.array([v[1] for v in per[:T]], dtype=np.int64)
        self.brier_t = np.array([v[4] for v in per[:T]], dtype=np.float64)
        self.ece_t = np.array([v[5] for v in per[:T]], dtype=np.float64)
        self.n, self.n_ties, self.brier, self.ece = per[T][0], per[T][1], per[T][4], per[T][5]
        node = np.array([[[s / FIX for s in pair] for pair in row] for row in node_sums],
                        dtype=np.float64).reshape(T, self.n_nodes, 2)
        obs = [np.asarray(d, dtype=np.int64) for d in observed_degrees]
        self.expected_degree = self.observed_degree = None
        self.expected_out_degree = self.expected_in_degree = None
        self.observed_out_degree = self.observed_in_degree = None
        if self.is_directed:
            self.expected_out_degree, self.expected_in_degree = node[..., 0].copy(), node[..., 1].copy()
            self.observed_out_degree, self.observed_in_degree = obs
        else:
            self.expected_degree = np.array([[(pair[0] + pair[1]) / FIX for pair in row] for row in node_sums],
                                            dtype=np.float64).reshape(T, self.n_nodes)
            self.observed_degree = obs[0] + obs[1]
        self.width_edges = np.asarray(width_edges, dtype=np.float64)
        self.width_hist_t = np.asarray(hist_width).astype(np.int64)
        self.width_hist = self.width_hist_t.sum(axis=0)
        if pointwise is None:
            self.mean = self.sd = self.lower = self.upper = None
        else:
            pw = np.asarray(pointwise, dtype=np.float64)
            if not self.is_directed:                               # i < j is filled, the rest 0
                pw = pw + pw.transpose(0, 2, 1, 3)
            self.mean, self.sd, self.lower, self.upper = (np.ascontiguousarray(pw[..., c]) for c in range(4))

    def summary(self):
        """Text table: the scores pooled and per time step, the reliability table and the interval widths"""
        T = self.n_t.shape[0]
        head = '%-14s %14s' % ('', 'pooled') + ''.join(' %14s' % ('t=%d' % t) for t in range(T))
        lines = ['edge probabilities: posterior mean of %d samples, %g%% intervals, %d scored dyads (%s)'
                 % (self.n_samples, 100 * self.level, self.n, 'directed' if self.is_directed else 'undirected'),
                 head]

        def row(label, total, per_t, fmt):
            lines.append('%-14s ' % label + fmt % total + ''.join(' ' + fmt % v for v in per_t))

        row('brier', self.brier, self.brier_t, '%14.6g')
        row('ece', self.ece, self.ece_t, '%14.6g')
        row('n', self.n, self.n_t, '%14d')
        row('ties', self.n_ties, self.n_ties_t, '%14d')
        if self.is_directed:
            gaps = (('out-degree gap', self.expected_out_degree - self.observed_out_degree),
                    ('in-degree gap', self.expected_in_degree - self.observed_in_degree))
        else:
            gaps = (('degree gap', self.expected_degree - self.observed_degree),)
        for label, gap in gaps:                                    # largest |expected - observed| over the nodes
            per_t = np.abs(gap).max(axis=1) if gap.shape[1] else np.zeros(T)
            row(label, per_t.max() if T else 0.0, per_t, '%14.6g')
        cal = self.calibration
        lines.append('reliability (pooled):')
        lines.append('%-14s %14s %14s %14s %14s' % ('mean in', 'n', 'ties', 'predicted', 'observed'))
        for b in range(self.n_bins):
            lines.append('%-14s %14d %14d %14.6g %14.6g'
                         % ('[%.3g, %.3g%s' % (cal['bin_edges'][b], cal['bin_edges'][b + 1],
                                               ']' if b == self.n_bins - 1 else ')'),
                            cal['n'][T, b], cal['ties'][T, b], cal['mean_predicted'][T, b],
                            cal['observed_frequency'][T, b]))
        lines.append('interval width (upper - lower):')
        lo = ['0'] + ['%.3g' % e for e in self.width_edges]
        hi = ['%.3g' % e for e in self.width_edges] + ['1']
        for b in range(self.width_hist.shape[0]):
            row('[%s, %s)' % (lo[b], hi[b]), self.width_hist[b], self.width_hist_t[:, b], '%14d')
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _observed_degrees(Y, excluded, directed):
    """(T, N) sums of y over the scored dyads (i, j) by i and by j (undirected: the dyads are i < j, and a dyad is
    excluded by either orientation)"""
    T, N = Y.shape[:2]
    scored = np.broadcast_to(~np.eye(N, dtype=bool) if directed else np.triu(np.ones((N, N), dtype=bool), 1),
                             Y.shape)
    if excluded is not None:
        scored = scored & ~(excluded if directed else excluded | excluded.transpose(0, 2, 1))
    ties = Y & scored
    return ties.sum(axis=2, dtype=np.int64), ties.sum(axis=1, dtype=np.int64)


def edge_probabilities(model, n_samples=None, level=0.9, pointwise=True, n_bins=20,
                       width_edges=DEFAULT_WIDTH_EDGES):
    """Posterior mean, standard deviation and equal-tailed credible interval of the edge probability of every
    dyad of a fitted ``DynamicNetworkLSM`` (undirected, directed or case-control), ``DynamicNetworkHDPLPCM`` or
    ``DynamicNetworkLPCM``, and the calibration of the posterior mean on the network it was fit to: a reliability
    table over ``n_bins`` (1..64) equal bins, the Brier score, the expected calibration error, every node's
    expected degree next to its observed one, and a histogram of the intervals' widths over ``width_edges`` (at
    most 16, ascending) - per time step and pooled, computed on the device in one pass over the trace.

    The samples are the kept rows of the trace (after the burn-in), or ``n_samples`` of them evenly spaced, as
    ``loo`` picks them; at least two.  ``level`` in (0, 1): the interval runs from the quantile at
    (1 - level) / 2 to the one at 1 - (1 - level) / 2 (numpy's default definition).  The observed network is
    ``Y_fit_``; the dyads that were missing in the data (``missing_index_`` of a ``sample_missing=True`` fit,
    ``nan_mask_``) enter none of the scores, but the pointwise arrays hold them: their posterior predictive
    probability.

    ``pointwise=True`` returns ``mean``, ``sd``, ``lower`` and ``upper`` as (T, N, N) float64 arrays (undirected:
    symmetric; diagonal 0): 32 T N^2 bytes.  For large N pass ``pointwise=False``: the scores need none of them.

    Returns an ``EdgeProbabilityResult``.
    """
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError('level must lie in (0, 1), got %r' % (level,))
    if int(n_bins) != n_bins or not 1 <= int(n_bins) <= 64:
        raise ValueError('n_bins must be an integer between 1 and 64, got %r' % (n_bins,))
    edges = np.ascontiguousarray(np.ravel(width_edges), dtype=np.float64)
    if edges.size > 16:
        raise ValueError('at most 16 width_edges, got %d' % edges.size)
    if not np.all(np.isfinite(edges)) or np.any(np.diff(edges) <= 0):
        raise ValueError('width_edges must be finite and ascending')
    ids = sample_rows(model, n_samples)
    if len(ids) < 2:
        raise ValueError('the interval and the standard deviation need at least two samples, got %d' % len(ids))
    directed = bool(model.is_directed)
    Xs, ic, radii = trace_samples(model, ids)
    S, T, N, D = Xs.shape
    Y = observed_network(model)
    bits = pack_network(Y)
    excluded = _excluded_dyads(model, Y.shape, directed)
    mask = pack_network(excluded) if excluded is not None else None
    with model_chain(model, T, N, D, directed) as chain:
        calib, brier, node_sums, hist_width, pw = chain.proba_accumulate(
            bits, Xs, ic, radii, level, mask=mask, n_bins=int(n_bins), width_edges=edges, pointwise=pointwise)
    return EdgeProbabilityResult(ids, S, level, calib, brier, node_sums, edges, hist_width,
                                 _observed_degrees(Y, excluded, directed), directed, N, pw)
