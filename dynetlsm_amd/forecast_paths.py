"""Multi-step posterior predictive forecasts of a fitted dynamic latent space model, and their scores
against the networks observed later.

The reference forecasts one step ahead, for the undirected HDP-LPCM / LPCM only, with the labels and
positions drawn on the host (``hdp_lpcm.py:555-626``; here ``forecast.py``, kept as it is).  ``forecast``
covers all three estimators, undirected and directed (case-control fits included: they use the exact
directed model), at any horizon H >= 1.  One trajectory per posterior sample starts at that sample's last
time step and follows the model's own dynamics:

    DynamicNetworkLSM       x_h = x_{h-1} + sqrt(sigma_sq) eps       (sigma_sq: the estimator's hyperparameter)
    HDP-LPCM / LPCM         z_h ~ Categorical(w_s[z_{h-1}, :])
                            x_h = lmbda_s mu_s[z_h] + (1 - lmbda_s) x_{h-1} + sqrt(sigma_s[z_h]) eps

with ``w_s`` the sample's own transition matrix (HDP-LPCM: ``weights_[s, -1]``, the last one, reused at every
future step; LPCM: ``trans_weights_[s]``), all K components and the raw rows (the device divides by the row
sum).  ``sigma`` is a variance, as in the likelihood and in ``forecast.mixture_density``: the forecast follows
the model.  (The reference's one-step ``forecast_probas`` multiplies ``randn`` by ``sigma`` itself; that
method and its fixtures stay as they are.)  The edge probabilities are

    P[h, i, j] = (1 / S) sum_s expit(eta_s(h, i, j))

``eta = b - |x_i - x_j|`` undirected, the directed model of ``metrics.py`` (probas_) with the sample's
intercepts and radii, held fixed over the horizon, for directed fits; the diagonal is 0.  The draws and the
accumulation run on the device (``Chain.forecast_paths``: csrc/kernels_forecast_paths.hpp) with Philox
counters, so every draw can be replayed on the host.
"""
import numpy as np

from ._trace import model_chain, point_estimate, sample_rows, trace_samples
from .engine import Chain, pack_network
from .lsm import check_random_state
from .scores import scores_from_counts

__all__ = ['forecast', 'ForecastResult']


class ForecastResult(object):
    """Result of ``forecast``.

    probas     : (H, N, N) posterior predictive edge probabilities of the H future time steps
    sample_ids : trace rows the trajectories started from (None: the point estimate)
    paths      : (S, H, N, D) drawn positions, ``keep_paths=True`` only (else None)
    labels     : (S, H, N) drawn labels of the clustered models, ``keep_paths=True`` only (else None)
    intercepts, radii : (S, 2) and (S, N) (directed) of the trajectories, ``keep_paths=True`` only
    """

    def __init__(self, probas, sample_ids, is_directed, paths=None, labels=None, intercepts=None, radii=None,
                 device=0):
        self.probas = probas
        self.sample_ids = sample_ids
        self.is_directed = bool(is_directed)
        self.paths, self.labels = paths, labels
        self.intercepts, self.radii = intercepts, radii
        self.device = device
        self.horizon, self.n_nodes = int(probas.shape[0]), int(probas.shape[1])

    def score(self, Y_future):
        """AUC and log-loss of the forecast against the networks observed later.

        ``Y_future`` (H', N, N), H' <= H, entries 1 / 0 and -1 for a dyad that was not observed (not
        scored).  Step h of ``Y_future`` is scored with the mean probability of the kept trajectories at
        step h (``Chain.score_accumulate`` on a chain of T = H').  Returns a ``ScoreResult``: per horizon
        step (``auc_t``, ``log_loss_t``, ...) and pooled.  Needs ``keep_paths=True``."""
        if self.paths is None:
            raise ValueError('score needs the trajectories: call forecast(..., keep_paths=True)')
        Y = np.asarray(Y_future)
        N = self.n_nodes
        if Y.ndim != 3 or Y.shape[1:] != (N, N) or not 1 <= Y.shape[0] <= self.horizon:
            raise ValueError('Y_future has shape %s, expected (H\', %d, %d) with 1 <= H\' <= %d'
                             % (Y.shape, N, N, self.horizon))
        Hs = Y.shape[0]
        missing = Y == -1
        if not self.is_directed:
            missing = missing | missing.swapaxes(1, 2)
        edges = (Y != 0) & ~missing
        idx = np.arange(N)
        edges[:, idx, idx] = False
        mask = pack_network(missing) if missing.any() else None
        Xs = np.ascontiguousarray(self.paths[:, :Hs])
        with Chain(Hs, N, Xs.shape[3], 'directed' if self.is_directed else 'undirected', device=self.device) as c:
            counts, logloss_sum = c.score_accumulate(pack_network(edges), Xs, self.intercepts, self.radii, mask=mask)
        return scores_from_counts(counts, logloss_sum, self.sample_ids, self.is_directed)

    def summary(self):
        """Text table: per future step the mean and the largest edge probability and the expected edges"""
        what = ('the point estimate' if self.sample_ids is None
                else '%d posterior samples' % len(self.sample_ids))
        lines = ['forecast: horizon %d from %s, %d nodes (%s)'
                 % (self.horizon, what, self.n_nodes, 'directed' if self.is_directed else 'undirected'),
                 '%-6s %14s %14s %16s' % ('step', 'mean proba', 'max proba', 'expected edges')]
        n_dyads = self.n_nodes * (self.n_nodes - 1)
        for h in range(self.horizon):
            P = self.probas[h]
            total = P.sum() / (1.0 if self.is_directed else 2.0)
            lines.append('%-6s %14.6f %14.6f %16.2f' % ('h=%d' % (h + 1), P.sum() / max(n_dyads, 1), P.max(), total))
        return '\n'.join(lines)

    def __repr__(self):
        return self.summary()


def _kind(model):
    """'lsm', 'hdp' or 'lpcm' by the attributes of the fit"""
    if hasattr(model, 'trans_weights_') and not hasattr(model, 'weights_') and hasattr(model, 'zs_'):
        return 'lpcm'
    if hasattr(model, 'weights_') and hasattr(model, 'zs_'):
        return 'hdp'
    return 'lsm'


def _inputs(model, ids, estimate, n_samples):
    """the arguments of ``Chain.forecast_paths`` as a dict"""
    directed = bool(model.is_directed)
    kind = _kind(model)
    if estimate == 'map':
        S = n_samples

        def tile(a):
            a = np.asarray(a)
            return np.ascontiguousarray(np.broadcast_to(a[None], (S,) + a.shape))

        X, ic, radii = point_estimate(model)
        kw = dict(X0=tile(X[0, -1]), intercepts=tile(ic[0]), radii=tile(radii[0]) if directed else None)
        if kind != 'lsm':
            w = model.trans_weights_[-1] if kind == 'hdp' else model.trans_weight_
            kw.update(z0=tile(np.asarray(model.z_)[-1]), trans=tile(w), mu=tile(model.mu_), sigma=tile(model.sigma_),
                      lmbda=np.full(S, float(np.ravel(model.lambda_)[0])))
    else:
        X0, ic, radii = trace_samples(model, ids, step=-1)
        kw = dict(X0=X0, intercepts=ic, radii=radii)
        if kind != 'lsm':
            w = model.weights_[ids, -1] if kind == 'hdp' else model.trans_weights_[ids]
            kw.update(z0=model.zs_[ids, -1], trans=w, mu=model.mus_[ids], sigma=model.sigmas_[ids],
                      lmbda=np.asarray(model.lambdas_, dtype=np.float64)[ids].reshape(len(ids), -1)[:, 0])
    if kind == 'lsm':
        kw['sigma_sq'] = float(model.sigma_sq)
    return kw


def forecast(model, horizon=1, n_samples=None, estimate='posterior', random_state=None, keep_paths=False):
    """Posterior predictive forecast of the next ``horizon`` networks of a fitted ``DynamicNetworkLSM``
    (undirected, directed or case-control), ``DynamicNetworkHDPLPCM`` or ``DynamicNetworkLPCM``.

    ``estimate='posterior'`` starts one trajectory at each kept row of the trace (after the burn-in), or at
    ``n_samples`` of them evenly spaced, as ``information_criteria`` picks them.  ``estimate='map'`` runs
    ``n_samples`` trajectories (required) from the selected point estimate (``X_``, ``z_``, ...); their RNG
    indices differ, so the trajectories do.  ``random_state`` (default: the model's) seeds the draws: the same
    call returns the same result.  ``keep_paths=True`` also returns the drawn positions (and labels), which
    ``ForecastResult.score`` needs.

    The positions follow the model's law with ``sigma`` as a variance; the reference's one-step
    ``forecast_probas`` scales its normal draws by ``sigma`` itself and is kept as it is.

    Returns a ``ForecastResult``.
    """
    try:
        H = int(horizon)
    except (TypeError, ValueError):
        H = 0
    if H != horizon or H < 1:
        raise ValueError('horizon must be an integer >= 1, got %r' % (horizon,))
    if estimate not in ('posterior', 'map'):
        raise ValueError("estimate must be 'posterior' or 'map', got %r" % (estimate,))
    if not hasattr(model, 'Y_fit_') or not hasattr(model, 'intercepts_') or not hasattr(model, 'X_'):
        raise ValueError('Model not fit.')
    if estimate == 'map':
        if n_samples is None:
            raise ValueError("estimate='map' needs n_samples, the number of trajectories")
        S = int(n_samples)
        if S != n_samples or S < 1:
            raise ValueError('n_samples must be a positive integer, got %r' % (n_samples,))
        ids = None
    else:
        ids = sample_rows(model, n_samples)
        S = len(ids)
    directed = bool(model.is_directed)
    rng = check_random_state(model.random_state if random_state is None else random_state)
    seed = int(rng.randint(0, 2 ** 31 - 1)) | (int(rng.randint(0, 2 ** 31 - 1)) << 31)
    kw = _inputs(model, ids, estimate, S)
    mixture = 'z0' in kw
    _, N, D = kw['X0'].shape

    with model_chain(model, 1, N, D, directed) as chain:
        probas, paths, labels = chain.forecast_paths(horizon=H, seed=seed, want_paths=keep_paths,
                                                     want_labels=keep_paths and mixture, **kw)
    return ForecastResult(probas, ids, directed, paths, labels,
                          kw['intercepts'] if keep_paths else None, kw['radii'] if keep_paths else None,
                          device=getattr(model, 'device', 0))
