"""Information criteria of a fitted dynamic latent space model: WAIC and DIC.

The reference has no counterpart.  Both criteria come from the pointwise log-likelihood of the
observed dyads over the posterior samples of the trace,

    l_s(t, i, j) = y eta_s - log(1 + exp(eta_s)),

with eta the linear predictor of the model (``b - |x_i - x_j|`` undirected, the directed model of
``metrics.py`` (probas_) for directed and case-control fits).  The device reduces it over the samples
in one pass without storing it (``Chain.ic_accumulate``: csrc/kernels_ic.hpp, on the shared pass of
csrc/kernels_dyad_pass.hpp); the host turns the sums into the criteria:

* WAIC (Watanabe 2010; Vehtari, Gelman & Gabry 2017): ``lppd = sum log mean_s exp(l_s)``,
  ``p_waic = sum var_s(l_s)``, ``elpd_waic = lppd - p_waic``, ``waic = -2 elpd_waic`` and the standard
  error ``se_elpd = sqrt(n Var_dyads(elpd_ij))``.
* DIC (Spiegelhalter et al. 2002): with the deviance ``D_s = -2 sum_dyads l_s``, ``d_bar = mean_s D_s``,
  ``d_hat`` the deviance at the estimator's point estimate (``X_``, ``intercept_``, ``radii_``),
  ``p_d = d_bar - d_hat``, ``dic = d_bar + p_d``; and Gelman's variant ``p_v = var_s(D_s) / 2``,
  ``dic_v = d_bar + p_v``.

Lower ``waic`` / ``dic`` (higher ``elpd_waic``) is better.
"""
import numpy as np

from ._trace import model_chain, observed_network, point_estimate, sample_rows, trace_samples
from .engine import pack_network

__all__ = ['information_criteria', 'compare_information_criteria', 'ICResult']


class ICResult(object):
    """Result of ``information_criteria``.

    Totals are floats; every ``*_t`` attribute is the (T,) array of the time steps, which sum to the
    total (``se_elpd_t`` is the standard error within a time step).

    sample_ids       : trace rows the criteria were computed from
    n_samples        : their number S
    n_dyads          : dyads of the network (undirected: t, i < j; directed: t, i != j)
    lppd, p_waic, elpd_waic, waic, se_elpd
    sample_loglik    : (S, T) network log-likelihood of each sample
    d_bar, d_hat, p_d, dic, p_v, dic_v
    pointwise_lppd, pointwise_p_waic : (T, N, N) when asked for (undirected: i < j filled, the rest
                       0), else None
    """

    def __init__(self, sample_ids, totals, sample_loglik, loglik_hat, is_directed, n_nodes, pointwise=None):
        totals = np.asarray(totals, dtype=np.float64)
        sample_loglik = np.asarray(sample_loglik, dtype=np.float64)
        loglik_hat = np.asarray(loglik_hat, dtype=np.float64)
        self.sample_ids = sample_ids
        self.n_samples = int(sample_loglik.shape[0])
        self.is_directed = bool(is_directed)
        self.n_nodes = int(n_nodes)
        self.sample_loglik = sample_loglik
        self.n_dyads_t = np.rint(totals[:, 4]).astype(np.int64)
        self.n_dyads = int(self.n_dyads_t.sum())
        self.lppd_t, self.p_waic_t = totals[:, 0].copy(), totals[:, 1].copy()
        self.mean_loglik_t = totals[:, 2].copy()
        self.elpd_waic_t = self.lppd_t - self.p_waic_t
        self.waic_t = -2.0 * self.elpd_waic_t
        self.se_elpd_t = _se(self.elpd_waic_t, totals[:, 3], self.n_dyads_t)
        self.lppd, self.p_waic = float(self.lppd_t.sum()), float(self.p_waic_t.sum())
        self.elpd_waic = self.lppd - self.p_waic
        self.waic = -2.0 * self.elpd_waic
        self.se_elpd = float(_se(self.elpd_waic, totals[:, 3].sum(), self.n_dyads))
        # DIC from the samples' deviances
        dev = -2.0 * sample_loglik                               # (S, T)
        self.d_bar_t = dev.mean(axis=0)
        self.d_hat_t = -2.0 * loglik_hat
        self.p_d_t = self.d_bar_t - self.d_hat_t
        self.dic_t = self.d_bar_t + self.p_d_t
        self.d_bar, self.d_hat = float(self.d_bar_t.sum()), float(self.d_hat_t.sum())
        self.p_d = self.d_bar - self.d_hat
        self.dic = self.d_bar + self.p_d
        self.p_v = float(np.var(dev.sum(axis=1), ddof=1) / 2.0) if self.n_samples > 1 else 0.0
        self.dic_v = self.d_bar + self.p_v
        if pointwise is None:
            self.pointwise_lppd = self.pointwise_p_waic = None
        else:
            self.pointwise_lppd, self.pointwise_p_waic = pointwise[..., 0], pointwise[..., 1]

    def dyad_mask(self):
        """(N, N) boolean: the dyads of one time step"""
        N = self.n_nodes
        return ~np.eye(N, dtype=bool) if self.is_directed else np.triu(np.ones((N, N), dtype=bool), 1)

    def summary(self):
        """Text table: the criteria in total and per time step"""
        T = self.lppd_t.shape[0]
        head = '%-10s %14s' % ('', 'total') + ''.join(' %14s' % ('t=%d' % t) for t in range(T))
        lines = ['information criteria: %d samples, %d dyads (%s)'
                 % (self.n_samples, self.n_dyads, 'directed' if self.is_directed else 'undirected'), head]

        def row(label, total, per_t):
            lines.append('%-10s %14.6g' % (label, total) + ''.join(' %14.6g' % v for v in per_t))

        row('lppd', self.lppd, self.lppd_t)
        row('p_waic', self.p_waic, self.p_waic_t)
        row('elpd_waic', self.elpd_waic, self.elpd_waic_t)
        row('se_elpd', self.se_elpd, self.se_elpd_t)
        row('waic', self.waic, self.waic_t)
        row('d_bar', self.d_bar, self.d_bar_t)
        row('d_hat', self.d_hat, self.d_hat_t)
        row('p_d', self.p_d, self.p_d_t)
        row('dic', self.dic, self.dic_t)
        lines.append('%-10s %14.6g' % ('p_v', self.p_v))
        lines.append('%-10s %14.6g' % ('dic_v', self.dic_v))
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _se(sum_elpd, sum_elpd_sq, n):
    """sqrt(n Var(elpd_ij)) from the sum and the sum of squares over n dyads (0 for n < 2)"""
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        var = (sum_elpd_sq - sum_elpd * sum_elpd / n) / (n - 1.0)
        return np.where(n > 1, np.sqrt(n * np.maximum(var, 0.0)), 0.0)


def information_criteria(model, n_samples=None, pointwise=False):
    """WAIC and DIC of a fitted ``DynamicNetworkLSM`` (undirected, directed or case-control),
    ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM``, for comparing fits of the same network
    (``n_features``, directed against undirected, LSM against the clustered models).

    The samples are all kept rows of the trace (after the burn-in), or ``n_samples`` of them evenly
    spaced as ``posterior_predictive_check`` picks them.  The likelihood is the exact one of the
    model, also for case-control fits.  The observed network is ``Y_fit_``, the network the chain was
    fit to, over all its dyads: if the data had missing dyads, these are their imputed values.
    ``pointwise=True`` also returns the per-dyad ``lppd`` and ``p_waic`` (two (T, N, N) arrays), which
    ``compare_information_criteria`` needs.

    Returns an ``ICResult``.
    """
    ids = sample_rows(model, n_samples)
    directed = bool(model.is_directed)
    Xs, ic, radii = trace_samples(model, ids)
    _, T, N, D = Xs.shape
    X_hat, ic_hat, radii_hat = point_estimate(model)      # for DIC's d_hat
    bits = pack_network(observed_network(model))
    with model_chain(model, T, N, D, directed) as chain:
        out = chain.ic_accumulate(bits, Xs, ic, radii, want_pointwise=pointwise)
        _, loglik_hat = chain.ic_accumulate(bits, X_hat, ic_hat, radii_hat)
    return ICResult(ids, out[0], out[1], loglik_hat[0], directed, N, out[2] if pointwise else None)


def compare_information_criteria(a, b):
    """Difference of two fits of the same network in expected log predictive density.

    ``a`` and ``b`` are ``ICResult``s with ``pointwise=True``.  Returns ``(elpd_diff, se_diff)``:
    ``elpd_diff = elpd_waic(a) - elpd_waic(b)`` (positive: ``a`` predicts better) and its standard
    error ``sqrt(n Var_dyads(elpd_a,ij - elpd_b,ij))`` from the paired pointwise values."""
    for r in (a, b):
        if not isinstance(r, ICResult):
            raise ValueError('compare_information_criteria takes two ICResult objects')
        if r.pointwise_lppd is None or r.pointwise_p_waic is None:
            raise ValueError('both results need the pointwise arrays: information_criteria(model, pointwise=True)')
    if a.pointwise_lppd.shape != b.pointwise_lppd.shape:
        raise ValueError('the results are of different networks: shapes %s and %s'
                         % (a.pointwise_lppd.shape, b.pointwise_lppd.shape))
    if a.is_directed != b.is_directed:
        raise ValueError('a directed and an undirected result do not share their dyads')
    mask = a.dyad_mask()
    d = ((a.pointwise_lppd - a.pointwise_p_waic) - (b.pointwise_lppd - b.pointwise_p_waic))[:, mask]
    n = d.size
    diff = float(d.sum())
    se = float(np.sqrt(n * np.var(d, ddof=1))) if n > 1 else 0.0
    return diff, se
