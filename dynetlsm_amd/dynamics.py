"""Tie dynamics of a fitted dynamic latent space model: which relations strengthened or weakened between two
consecutive time steps, with what posterior certainty, and whether the model reproduces the persistence of ties.

Every other pass over the trace treats one time step at a time; this one reads the joint posterior of two.  With
``p_{s,t} = expit(eta_{s,t})`` (the same samples and the same linear predictor eta as ``edge_probabilities``), the
device forms for every dyad and every step u = t -> t + 1 (u = 0 .. T - 2), over S posterior samples

    delta_mean, delta_sd (ddof 1) of d_s = p_{s,t+1} - p_{s,t}
    up, down     the samples in which eta rose, and fell (a tie counts as neither); prob_up = up / S
    persist      mean_s p_{s,t} p_{s,t+1} - the expected persistence of a tie is not the product of the two means

and, over the scored steps - the dyad is observed and not masked at t and at t + 1 -, counts them into integer
tables (``Chain.dynamics_accumulate``: csrc/kernels_dynamics.hpp on the shared pass of csrc/kernels_dyad_pass.hpp;
probabilities are summed in units of 2^-32, at most half a unit off per dyad):

    transitions    per step and observed class 2 y_t + y_{t+1}: dyads, sum pbar_t, sum pbar_{t+1}, sum persist
    hist_up        dyads per bin of up
    node_changes   per node, its dyads that rose (fell) in at least ``min_count`` = ceil(level S) samples
    node_turnover  per node, the sum of |delta_mean| over its dyads

``TieDynamicsResult`` turns them into observed and expected counts of persisted, formed and dissolved ties, the
persistence and formation rates next to the model's, and the nodes whose neighbourhood changed.  ``gof.py``'s
simulated ``'temporal'`` family asks the same question with Monte Carlo noise and nothing per dyad.

The pointwise arrays cover every dyad of the model.  They take 32 (T - 1) N^2 bytes; ``pointwise=False`` is the
form for large N.
"""
import math

import numpy as np

from ._trace import model_chain, observed_network, sample_rows, trace_samples
from .engine import pack_network
from .probabilities import FIX, _ints
from .scores import _excluded_dyads, _ratio

__all__ = ['tie_dynamics', 'TieDynamicsResult']


def _min_count(level, S):
    """samples that make a direction certain at ``level``: ceil(level S), above S / 2 so that no dyad has both"""
    return min(max(int(math.ceil(level * S - 1e-12)), S // 2 + 1), S)


class TieDynamicsResult(object):
    """Result of ``tie_dynamics``.  A step u is t = u -> t + 1; U = T - 1 steps.

    sample_ids, n_samples, level, min_count : trace rows the result was computed from, their number S, the level,
                       and the samples ceil(level S) in which a dyad must move one way to count as changed
    n_t, n           : scored steps of a dyad (unmasked at t and t + 1), (U,) and pooled
    observed_persisted_t, observed_formed_t, observed_dissolved_t : (U,) dyads with (y_t, y_{t+1}) = (1, 1), (0, 1),
                       (1, 0); ``observed_persisted`` etc. pooled
    expected_persisted_t, expected_formed_t, expected_dissolved_t : (U,) sum persist, sum pbar_{t+1} - sum persist,
                       sum pbar_t - sum persist over the scored steps; ``expected_persisted`` etc. pooled
    persistence_observed_t, persistence_expected_t : (U,) n11 / (n10 + n11), and the mean of pbar_{t+1} over the
                       dyads with y_t = 1; ``formation_observed_t`` / ``formation_expected_t``: n01 / (n00 + n01) and
                       the same mean over y_t = 0; pooled without ``_t``; NaN where the denominator is 0
    strengthened, weakened, turnover : (U, N) undirected: per node its dyads with up >= min_count, with down >=
                       min_count, and the sum of |delta_mean|; directed: None, and ``strengthened_out`` /
                       ``strengthened_in`` etc. (None for undirected models)
    n_strengthened_t, n_weakened_t : (U,) dyads with up >= min_count, with down >= min_count
    prob_up_hist     : (U, n_bins) dyads per bin min(up * n_bins // S, n_bins - 1)
    delta_mean, delta_sd, prob_up, prob_down : (U, N, N) float64 of every dyad (undirected: symmetric; diagonal 0),
                       or None (``pointwise=False``)
    counts           : the integer tables as Python ints: ``transitions`` (U, 4, 4), ``hist_up`` (U, n_bins),
                       ``node_changes`` (U, N, 4), ``node_turnover`` (U, N, 2), in units of 2^-32 where they hold
                       probabilities
    """

    def __init__(self, sample_ids, n_samples, level, min_count, transitions, hist_up, node_changes, node_turnover,
                 is_directed, n_nodes, pointwise=None):
        self.sample_ids = sample_ids
        self.n_samples = int(n_samples)
        self.level = float(level)
        self.min_count = int(min_count)
        self.is_directed = bool(is_directed)
        self.n_nodes = N = int(n_nodes)
        tr, hist = _ints(transitions), _ints(hist_up)
        changes, turn = _ints(node_changes), _ints(node_turnover)
        self.counts = {'transitions': tr, 'hist_up': hist, 'node_changes': changes, 'node_turnover': turn}
        U = len(tr)
        self.n_steps = U
        self.n_bins = len(hist[0]) if U else 0
        pooled = [[sum(tr[u][c][v] for u in range(U)) for v in range(4)] for c in range(4)]

        def derive(tab):
            n00, n01, n10, n11 = (tab[c][0] for c in range(4))
            s0, s1, sp = (sum(tab[c][v] for c in range(4)) for v in (1, 2, 3))
            return {'n': n00 + n01 + n10 + n11,
                    'observed_persisted': n11, 'observed_formed': n01, 'observed_dissolved': n10,
                    'expected_persisted': sp / FIX, 'expected_formed': (s1 - sp) / FIX,
                    'expected_dissolved': (s0 - sp) / FIX,
                    'persistence_observed': _ratio(n11, n10 + n11),
                    'persistence_expected': _ratio(tab[2][2] + tab[3][2], (n10 + n11) * FIX),
                    'formation_observed': _ratio(n01, n00 + n01),
                    'formation_expected': _ratio(tab[0][2] + tab[1][2], (n00 + n01) * FIX)}

        per = [derive(tab) for tab in tr]
        for key, value in derive(pooled).items():
            is_count = key == 'n' or key.startswith('observed_')
            setattr(self, key, value)
            setattr(self, key + '_t', np.array([p[key] for p in per], dtype=np.int64 if is_count else np.float64))
        node = np.array(changes, dtype=np.int64).reshape(U, N, 4)
        fix_turn = [[[s / FIX for s in pair] for pair in row] for row in turn]
        tout = np.array(fix_turn, dtype=np.float64).reshape(U, N, 2)
        self.strengthened = self.weakened = self.turnover = None
        self.strengthened_out = self.strengthened_in = self.weakened_out = self.weakened_in = None
        self.turnover_out = self.turnover_in = None
        if self.is_directed:
            self.strengthened_out, self.strengthened_in = node[..., 0].copy(), node[..., 1].copy()
            self.weakened_out, self.weakened_in = node[..., 2].copy(), node[..., 3].copy()
            self.turnover_out, self.turnover_in = tout[..., 0].copy(), tout[..., 1].copy()
        else:
            self.strengthened = node[..., 0] + node[..., 1]
            self.weakened = node[..., 2] + node[..., 3]
            self.turnover = np.array([[(pair[0] + pair[1]) / FIX for pair in row] for row in turn],
                                     dtype=np.float64).reshape(U, N)
        self.n_strengthened_t = node[..., 0].sum(axis=1)
        self.n_weakened_t = node[..., 2].sum(axis=1)
        self.n_strengthened, self.n_weakened = int(self.n_strengthened_t.sum()), int(self.n_weakened_t.sum())
        self.prob_up_hist = np.array(hist, dtype=np.int64).reshape(U, self.n_bins)
        if pointwise is None:
            self.delta_mean = self.delta_sd = self.prob_up = self.prob_down = None
        else:
            pw = np.asarray(pointwise, dtype=np.float64)
            if not self.is_directed:                               # i < j is filled, the rest 0
                pw = pw + pw.transpose(0, 2, 1, 3)
            self.delta_mean, self.delta_sd, self.prob_up, self.prob_down = (
                np.ascontiguousarray(pw[..., c]) for c in range(4))

    def top_changes(self, k=10, step=None):
        """The ``k`` dyads with the largest |delta_mean| among those that moved one way in at least ``min_count``
        samples, of step ``step`` or of all steps: rows (step, i, j, delta_mean, prob_up), largest first
        (undirected: i < j).  Needs the pointwise arrays."""
        if self.delta_mean is None:
            raise ValueError('top_changes needs the pointwise arrays: call tie_dynamics(..., pointwise=True)')
        S = self.n_samples
        sure = ((np.rint(self.prob_up * S) >= self.min_count) | (np.rint(self.prob_down * S) >= self.min_count))
        if not self.is_directed:
            sure &= np.triu(np.ones((self.n_nodes, self.n_nodes), dtype=bool), 1)
        if step is not None:
            if not 0 <= int(step) < self.n_steps:
                raise ValueError('step must lie in 0..%d, got %r' % (self.n_steps - 1, step))
            only = np.zeros(self.n_steps, dtype=bool)
            only[int(step)] = True
            sure &= only[:, None, None]
        at = np.argwhere(sure)
        size = np.abs(self.delta_mean[sure])
        order = np.argsort(-size, kind='stable')[:max(int(k), 0)]
        return [(int(u), int(i), int(j), float(self.delta_mean[u, i, j]), float(self.prob_up[u, i, j]))
                for u, i, j in at[order]]

    def summary(self):
        """Text table: observed against expected transitions and rates, and the changed dyads, pooled and per step"""
        U = self.n_steps
        head = '%-22s %14s' % ('', 'pooled') + ''.join(' %14s' % ('t=%d->%d' % (u, u + 1)) for u in range(U))
        lines = ['tie dynamics: %d samples, a change counts at %g%% (%d samples), %d scored steps of a dyad (%s)'
                 % (self.n_samples, 100 * self.level, self.min_count, self.n,
                    'directed' if self.is_directed else 'undirected'), head]

        def row(label, total, per_t, fmt):
            lines.append('%-22s ' % label + fmt % total + ''.join(' ' + fmt % v for v in per_t))

        for what in ('persisted', 'formed', 'dissolved'):
            row(what + ' observed', getattr(self, 'observed_' + what), getattr(self, 'observed_%s_t' % what), '%14d')
            row(what + ' expected', getattr(self, 'expected_' + what), getattr(self, 'expected_%s_t' % what),
                '%14.6g')
        for what in ('persistence', 'formation'):
            row(what + ' observed', getattr(self, what + '_observed'), getattr(self, what + '_observed_t'), '%14.6g')
            row(what + ' expected', getattr(self, what + '_expected'), getattr(self, what + '_expected_t'), '%14.6g')
        row('strengthened dyads', self.n_strengthened, self.n_strengthened_t, '%14d')
        row('weakened dyads', self.n_weakened, self.n_weakened_t, '%14d')
        if self.is_directed:
            moved = (('max changed out-ties', self.strengthened_out + self.weakened_out),
                     ('max changed in-ties', self.strengthened_in + self.weakened_in),
                     ('max out-turnover', self.turnover_out), ('max in-turnover', self.turnover_in))
        else:
            moved = (('max changed ties', self.strengthened + self.weakened), ('max turnover', self.turnover))
        for label, a in moved:                                     # the node that changed most
            per_t = a.max(axis=1) if a.shape[1] else np.zeros(U, dtype=a.dtype)
            row(label, per_t.max() if U else 0, per_t, '%14d' if a.dtype.kind == 'i' else '%14.6g')
        lines.append('P(eta rose) over the samples, dyads per bin:')
        for b in range(self.n_bins):
            row('[%.3g, %.3g%s' % (b / self.n_bins, (b + 1) / self.n_bins, ']' if b == self.n_bins - 1 else ')'),
                self.prob_up_hist[:, b].sum(), self.prob_up_hist[:, b], '%14d')
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def tie_dynamics(model, n_samples=None, level=0.9, pointwise=True, n_bins=20):
    """Posterior change of the edge probability of every dyad between consecutive time steps of a fitted
    ``DynamicNetworkLSM`` (undirected, directed or case-control), ``DynamicNetworkHDPLPCM`` or
    ``DynamicNetworkLPCM`` with T >= 2: the mean and standard deviation of p_{t+1} - p_t, the posterior probability
    that the tie strengthened or weakened, and - against the network the model was fit to - observed and expected
    numbers of persisted, formed and dissolved ties, persistence and formation rates, the nodes whose ties changed
    and a histogram of the probability of strengthening over ``n_bins`` (1..64) equal bins, per step and pooled,
    computed on the device in one pass over the trace.

    The samples are the kept rows of the trace (after the burn-in), or ``n_samples`` of them evenly spaced, as
    ``edge_probabilities`` picks them; at least two.  ``level`` in (0.5, 1): a dyad counts as strengthened
    (weakened) when its linear predictor rose (fell) in at least ceil(level S) of the S samples.  The observed
    network is ``Y_fit_``; a dyad that was missing in the data at t or at t + 1 enters no table at that step, but the
    pointwise arrays hold it.

    ``pointwise=True`` returns ``delta_mean``, ``delta_sd``, ``prob_up`` and ``prob_down`` as (T - 1, N, N) float64
    arrays (undirected: symmetric; diagonal 0): 32 (T - 1) N^2 bytes.  For large N pass ``pointwise=False``.

    Returns a ``TieDynamicsResult``.
    """
    level = float(level)
    if not 0.5 < level < 1.0:
        raise ValueError('level must lie in (0.5, 1), got %r' % (level,))
    if int(n_bins) != n_bins or not 1 <= int(n_bins) <= 64:
        raise ValueError('n_bins must be an integer between 1 and 64, got %r' % (n_bins,))
    ids = sample_rows(model, n_samples)
    if len(ids) < 2:
        raise ValueError('the standard deviation of the change needs at least two samples, got %d' % len(ids))
    if np.shape(model.Y_fit_)[0] < 2:
        raise ValueError('a step needs two time steps, the model has T=%d' % np.shape(model.Y_fit_)[0])
    directed = bool(model.is_directed)
    Xs, ic, radii = trace_samples(model, ids)
    S, T, N, D = Xs.shape
    Y = observed_network(model)
    bits = pack_network(Y)
    excluded = _excluded_dyads(model, Y.shape, directed)
    mask = pack_network(excluded) if excluded is not None else None
    min_count = _min_count(level, S)
    with model_chain(model, T, N, D, directed) as chain:
        transitions, hist_up, node_changes, node_turnover, pw = chain.dynamics_accumulate(
            bits, Xs, ic, radii, min_count, mask=mask, n_bins=int(n_bins), pointwise=pointwise)
    return TieDynamicsResult(ids, S, level, min_count, transitions, hist_up, node_changes, node_turnover, directed,
                             N, pw)
