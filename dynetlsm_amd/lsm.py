"""DynamicNetworkLSM with the reference's constructor, ``fit(Y)`` and fitted
attributes (lsm.py:100-625), running the Gibbs loop on one MI355X.

Host code is orchestration only.  For the undirected model the whole loop
(lsm.py:474-572) is device resident: sweep, Procrustes, centring, intercept MH
fused with the log-posterior trace, samples stored in a device trace that is
read back once.  Directed models (exact and case-control) drive the same
kernels from the host because the radii step draws a Dirichlet proposal with
the numpy stream (metropolis.py:57-82).

Differences from the reference that a user can see:
  * random numbers: the latent-position sweep uses the engine's Philox streams
    (keyed by a seed drawn from ``random_state``) and the even/odd-t scan order,
    so chains are equal in distribution, not sample for sample;
  * missing edges (-1 coded dyads) are imputed once before the chain, as the reference
    effectively does (see ``imputer``); with ``sample_missing=True`` the device loop then draws
    them again from their conditional at the end of every iteration (data augmentation: the
    chain targets the posterior given the observed dyads); NaN entries are rejected;
  * ``fit(Y, init=...)`` accepts starting values and skips the init pipeline.
"""
import time

import numpy as np

from .engine import Chain, check_n_features
from . import _fit
from . import initialization as init_mod
from ._fit import (Estimator, _ScalarMetropolis, _missing_attributes,
                   check_random_state)      # (other modules import check_random_state from here)
from .metrics import missing_index
from .sparse import SparseNetwork

__all__ = ['DynamicNetworkLSM']


def latent_prior_terms(X, tau_sq, sigma_sq):
    """lsm.py:604-613"""
    diff = X[1:] - X[:-1]
    return -(0.5 * np.sum(X[0] * X[0]) / tau_sq + 0.5 * np.sum(diff * diff) / sigma_sq)


class DynamicNetworkLSM(Estimator):
    """Latent space model for dynamic networks (Sewell & Chen) on MI355X.

    Constructor parameters are the reference's (lsm.py:234-268) plus
    ``device`` (GPU index), ``chain_id`` (Philox stream of this chain) and
    ``sweep_algo`` (0 auto; 1 .. 5 as ``dlsm_sweep_positions`` in include/dynetlsm_hip.h).
    ``sample_missing=True`` re-draws the -1 coded dyads on the device every iteration and leaves
    ``missing_index_`` (n, 3), ``missing_probas_`` (post-burn-in mean of p_ij) and ``missings_``
    (post-burn-in mean of the draws); ``Y_fit_`` stays the initial imputation."""

    def __init__(self, n_features=2, is_directed=False, n_iter=5000, tune=2500,
                 tune_interval=100, burn=2500, intercept_prior='auto',
                 intercept_variance_prior=2.0, tau_sq=2.0, sigma_sq=0.1, step_size_X=0.1,
                 step_size_intercept=0.1, step_size_radii=175000, n_control=None,
                 n_resample_control=100, copy=True, random_state=None, device=0,
                 chain_id=0, sweep_algo=0, directed_loop='device', sample_missing=False):
        self.directed_loop = directed_loop
        self.sample_missing = sample_missing
        self.n_iter = n_iter
        self.is_directed = is_directed
        self.n_features = n_features
        self.tau_sq = tau_sq
        self.sigma_sq = sigma_sq
        self.step_size_X = step_size_X
        self.intercept_prior = intercept_prior
        self.intercept_variance_prior = intercept_variance_prior
        self.step_size_intercept = step_size_intercept
        self.step_size_radii = step_size_radii
        self.tune = tune
        self.tune_interval = tune_interval
        self.burn = burn
        self.n_control = n_control
        self.n_resample_control = n_resample_control
        self.copy = copy
        self.random_state = random_state
        self.device = device
        self.chain_id = chain_id
        self.sweep_algo = sweep_algo

    @property
    def n_burn_(self):
        return (self.burn or 0) + (self.tune or 0)

    # -- fit ------------------------------------------------------------------
    def fit(self, Y, init=None):
        """Sample the posterior given the dynamic network ``Y`` (T, N, N),
        float64 binary adjacency matrices, or a ``SparseNetwork`` of its ties (no dense
        tensor is formed; ``Y_fit_`` is then the container - with the container's missing dyads, if
        it lists any, filled once as ties or non-ties).  ``init`` may give starting values
        ``dict(X=..., intercept=..., radii=...)``; otherwise they come from the
        GMDS / conditional-MLE pipeline as in the reference (lsm.py:386-407)."""
        Y = _fit.check_network(Y, self.copy)
        _fit.check_options(self)
        Y, sparse, held = _fit.sparse_network(self, Y)
        miss_lists, miss_index = held if held is not None else (None, None)
        if not sparse and np.any(Y == -1):          # lsm.py:345-359
            if self.sample_missing:
                miss_index = missing_index(Y, self.is_directed)
            Y = _fit.impute(Y)
        rng = check_random_state(self.random_state)
        self.Y_fit_ = Y
        n_total = _fit.extend_n_iter(self)
        seed = _fit.chain_seed(rng)     # before the starting values consume the stream

        # ---- starting values ------------------------------------------------
        if init is not None:
            X, intercept, radii = _fit.init_values(self, init)
        else:
            X, intercept, radii = self._init_pipeline(Y, rng)
        X = X - np.mean(X, axis=(0, 1))
        if isinstance(self.tau_sq, str) and self.tau_sq == 'auto':
            self.tau_sq = np.mean(X[0] * X[0])
        ip = _fit.resolve_intercept_prior(self, intercept)

        # ---- the chain ------------------------------------------------------
        chain = _fit.open_chain(self, Y, X, intercept, radii, seed)
        chain.set_prior_random_walk(self.tau_sq, self.sigma_sq)
        logp0 = self._log_prior(X, intercept, ip) + chain.loglik_full()
        self._impute = miss_index is not None and miss_index.shape[0] > 0
        if self._impute:             # lsm.py:525-545, with the draw written back
            if miss_lists is not None:      # (the same tables, from the container's lists)
                chain.set_missing_edges(miss_lists, allow_ties=True)
            else:
                chain.set_missing(miss_index)
            chain.missing_sampling(True, accumulate_after=self.n_burn_)

        t_loop = time.perf_counter()
        if not self.is_directed or self.directed_loop == 'device':
            self._fit_device(chain, n_total, logp0, ip)
        else:
            self._fit_directed(chain, rng, X, intercept, radii, n_total, logp0, ip)
        chain.get_samplers(self.latent_samplers)
        self.loop_seconds_ = time.perf_counter() - t_loop     # Gibbs loop only
        if self._impute:
            _missing_attributes(self, chain, miss_index)
            chain.missing_sampling(False)
        self._set_map(n_total)
        return self

    def _init_pipeline(self, Y, rng):
        """lsm.py:386-407: GMDS positions, then the conditional MLE of the other parameters"""
        T, N, _ = Y.shape
        with Chain(T, N, check_n_features(self.n_features),
                   'directed' if self.is_directed else 'undirected', device=self.device) as c0:
            if isinstance(Y, SparseNetwork):
                c0.upload_network_edges(Y)
            else:
                c0.upload_network(Y)
            X = init_mod.generalized_mds(c0, is_directed=self.is_directed, random_state=rng)
            if self.is_directed:
                radii = init_mod.initialize_radii(Y)
                b_in, b_out = init_mod.directed_intercept_mle(c0, X, radii)
                return X, np.array([b_in, b_out]), radii
            scale, b = init_mod.scale_intercept_mle(c0, X)
            return X * np.exp(scale), np.array([b]), None

    def _log_prior(self, X, intercept, ip):
        """lsm.py:604-623"""
        lp = latent_prior_terms(X, self.tau_sq, self.sigma_sq)
        diff = intercept - ip
        return lp - np.sum(0.5 * (diff * diff) / self.intercept_variance_prior)

    def _fit_device(self, chain, n_total, logp0, ip):
        """lsm.py:474-572 with the iterations enqueued on the device (``dlsm_lsm_run``): sweep,
        Procrustes / centring, the intercept step fused with the log-posterior trace - for the directed
        models two intercept steps and the radii step with Philox draws - and the samples stored in a
        device trace that is read back once.  The host only keeps the cadence of the control
        resampling and picks the Procrustes reference (lsm.py:496)."""
        n_iter_procrustes = self.n_burn_
        # lsm.py:465-467: the undirected intercept sampler ignores tune_interval
        chain.lsm_configure(ip, self.intercept_variance_prior,
                            step_size_intercept=self.step_size_intercept, tune=self.tune,
                            tune_interval=self.tune_interval if self.is_directed else 100,
                            n_iter_procrustes=n_iter_procrustes, sweep_algo=self.sweep_algo,
                            step_size_radii=self.step_size_radii, radii_tune=None)
        chain.trace_alloc(n_total, logp0=float(logp0))
        ccs = self.case_control_sampler_
        first = min(n_iter_procrustes, n_total - 1)
        if first > 0:
            _fit.run_ranges(ccs, 1, first, chain.lsm_run)
        if n_total - 1 > first:
            _, _, lps = chain.trace_read(0, n_iter_procrustes + 1, positions=False)
            prev_map = int(np.argmax(lps))          # lsm.py:496
            _fit.run_ranges(ccs, first + 1, n_total - 1,
                            lambda it, count: chain.lsm_run(it, count, procrustes_ref=prev_map))
        self.Xs_, self.intercepts_, self.logps_ = chain.trace_read(0, n_total)
        if self.is_directed:
            self.radiis_ = chain.trace_read_radii(0, n_total)
        _fit.samplers_from_lsm_config(self, chain.lsm_get_config())

    def _fit_directed(self, chain, rng, X, intercept, radii, n_total, logp0, ip):
        """the directed models' loop driven from the host, coefficient draws on the numpy stream"""
        T, N, D = X.shape
        n_iter_procrustes = self.n_burn_
        self.Xs_ = np.zeros((n_total, T, N, D))
        self.intercepts_ = np.zeros((n_total, 2))
        self.radiis_ = np.zeros((n_total, N))
        self.logps_ = np.zeros(n_total)
        self.Xs_[0], self.intercepts_[0], self.radiis_[0], self.logps_[0] = (
            X, intercept, radii, logp0)
        isamp = [_ScalarMetropolis(self.step_size_intercept, self.tune, self.tune_interval)
                 for _ in range(2)]
        rsamp = _ScalarMetropolis(self.step_size_radii, None, dirichlet=True)
        self.intercept_samplers, self.radii_sampler = isamp, rsamp
        for it in range(1, n_total):
            if self.case_control_sampler_ is not None:
                self.case_control_sampler_.resample(it)
            chain.sweep_positions(it, self.sweep_algo)
            if it > n_iter_procrustes:
                prev_map = int(np.argmax(self.logps_[:n_iter_procrustes + 1]))
                chain.procrustes(self.Xs_[prev_map])
            chain.center()
            intercept, radii, ll = _fit.coefficient_steps(
                chain, rng, intercept, radii, ip, self.intercept_variance_prior, isamp, rsamp,
                group_proposal_terms=True)
            Xc = chain.get_positions()
            self.Xs_[it], self.intercepts_[it], self.radiis_[it] = Xc, intercept, radii
            self.logps_[it] = ll + self._log_prior(Xc, intercept, ip)
            if self._impute:
                chain.impute_missing(it, it > self.n_burn_)

    def _set_map(self, n_total):
        """MAP bookkeeping of lsm.py:554-566, replayed over the trace."""
        best = 0
        logp = self.logps_[0]
        for it in range(1, n_total):
            if self.tune and it == (self.tune + (self.burn or 0)):
                best, logp = it, self.logps_[it]
            elif self.logps_[it] > logp:
                best, logp = it, self.logps_[it]
        self.logp_ = logp
        self.X_ = self.Xs_[best]
        self.intercept_ = self.intercepts_[best]
        if self.is_directed:
            self.radii_ = self.radiis_[best]
        self.map_index_ = best

    def logp(self, Y, X, intercept, radii=None, dist=None):
        """lsm.py:576-625 for arbitrary arguments (one GPU pass)."""
        model = ('undirected' if not self.is_directed else 'directed')
        T, N, D = X.shape
        with Chain(T, N, D, model, device=self.device) as c:
            c.upload_network(np.ascontiguousarray(Y, dtype=np.float64))
            c.set_positions(X)
            if self.is_directed:
                c.set_radii(radii)
            ic = np.atleast_1d(np.asarray(intercept, dtype=np.float64))
            ll = c.loglik_full([ic])[0]
        ip = np.atleast_1d(np.asarray(self.intercept_prior, dtype=np.float64))
        return ll + self._log_prior(X, ic, ip)
