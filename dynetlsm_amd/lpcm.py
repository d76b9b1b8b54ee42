"""DynamicNetworkLPCM (the finite-mixture latent position cluster model with a
time-homogeneous label chain) with the reference's constructor, ``fit(Y)`` and per-sample
traces (lpcm.py:135-760), Gibbs loop on one MI355X.

Every device piece is shared with DynamicNetworkHDPLPCM: latent-position sweep with the
AR-mixture prior, centring, intercept (and radii) MH over fused log-likelihood passes, the
label block update (``sample_labels_block_lpcm`` is ``sample_labels_block`` with w[t] = the
transition matrix for every t >= 1 and w[0, 0] = the initial distribution), the label-wise
sums of the conjugate updates and the post-loop co-occurrence / expected-VI kernels.  The
host keeps the O(K^2) Dirichlet draws and the cluster draws in the reference's MT19937
order (``hdp_updates.lpcm_gibbs_updates``).
"""
import time

import numpy as np

from .engine import check_n_features
from . import _fit
from . import forecast as fc
from . import hdp_updates as hu
from . import posterior as post
from ._fit import Estimator, _ScalarMetropolis, _missing_attributes, check_random_state

__all__ = ['DynamicNetworkLPCM']


class DynamicNetworkLPCM(Estimator):
    """Constructor parameters are the reference's (lpcm.py:135-187) plus ``device``,
    ``chain_id`` and ``sweep_algo``."""

    def __init__(self, n_features=2, n_components=5, is_directed=False, selection_type='map',
                 n_iter=5000, tune=2500, tune_interval=100, burn=2500, thin=None,
                 intercept_prior='auto', intercept_variance_prior=2, mean_variance_prior='auto',
                 a=2.0, b='auto', lambda_prior=0.9, lambda_variance_prior=0.01,
                 dirichlet_prior='uniform', sigma_prior_std=4.0, mean_variance_prior_std=4.0,
                 step_size_X='auto', step_size_intercept=0.1, step_size_radii=175000,
                 n_control=None, n_resample_control=100, copy=True, random_state=None,
                 device=0, chain_id=0, sweep_algo=0, sample_missing=False):
        self.n_iter = n_iter
        self.sample_missing = sample_missing
        self.is_directed = is_directed
        self.selection_type = selection_type
        self.n_features = n_features
        self.n_components = n_components
        self.dirichlet_prior = dirichlet_prior
        self.step_size_X = step_size_X
        self.intercept_prior = intercept_prior
        self.intercept_variance_prior = intercept_variance_prior
        self.step_size_intercept = step_size_intercept
        self.mean_variance_prior = mean_variance_prior
        self.a = a
        self.b = b
        self.lambda_prior = lambda_prior
        self.lambda_variance_prior = lambda_variance_prior
        self.mean_variance_prior_std = mean_variance_prior_std
        self.sigma_prior_std = sigma_prior_std
        self.step_size_radii = step_size_radii
        self.tune = tune
        self.tune_interval = tune_interval
        self.burn = burn
        self.thin = thin
        self.n_control = n_control
        self.n_resample_control = n_resample_control
        self.copy = copy
        self.random_state = random_state
        self.device = device
        self.chain_id = chain_id
        self.sweep_algo = sweep_algo

    @property
    def n_burn_(self):
        n_burn = (self.burn or 0) + (self.tune or 0)
        return int(np.ceil(n_burn / self.thin)) if self.thin else n_burn      # lpcm.py:189-197

    # -- one-step-ahead forecasts (lpcm.py:228-318; undirected models) ----------------
    @property
    def forecast_probas_map_(self):
        return fc.lpcm_forecast_probas_map(self, self._forecast_ready())

    @property
    def forecast_probas_plugin_(self):
        return fc.lpcm_forecast_probas_plugin(self, self._forecast_ready())

    @property
    def forecast_probas_marginalized_(self):
        return fc.lpcm_forecast_probas_marginalized(self, self._forecast_ready())

    def forecast_probas(self, n_samples=5000):
        return fc.lpcm_forecast_probas(self, self._forecast_ready(), n_samples=n_samples)

    @staticmethod
    def _stack(init_w, trans_w, T):
        w = np.empty((T,) + trans_w.shape)
        w[:] = trans_w[None]
        w[0, 0] = init_w
        return w

    # ------------------------------------------------------------------- fit
    def fit(self, Y, init=None):
        self._prepare(Y, init)
        t_loop = time.perf_counter()
        self._run(1, self._n_total - 1)
        self.loop_seconds_ = time.perf_counter() - t_loop
        return self._finish()

    def _prepare(self, Y, init=None):
        """Everything of ``fit`` before the Gibbs loop (lpcm.py:45-132, :340-560): checks, starting
        values - LSM warm start, longitudinal k-means, empirical initial distribution, uniform
        transition matrix -, hyper-priors, the chain handle and the trace arrays."""
        Y_raw = _fit.check_network(Y, self.copy)
        _fit.check_options(self)
        T, N, _ = Y_raw.shape
        K, D = self.n_components, check_n_features(self.n_features)
        rng = check_random_state(self.random_state)
        Y_raw, sparse, _ = _fit.sparse_network(self, Y_raw, missing_lists=False)
        Y, self._miss, self._miss_index = ((Y_raw, None, None) if sparse else
                                           _fit.prepare_missing(self, Y_raw))
        n_total = _fit.extend_n_iter(self)
        Y, X, intercept, radii, mu, sigma, z = _fit.warm_start(self, Y, rng, init, Y_raw=Y_raw)
        self.Y_fit_ = Y
        self.dirichlet_prior_ = 1. if self.dirichlet_prior == 'uniform' else 1. / K
        self.hyper_, ip = _fit.mixture_hyper(self, N, D, intercept)

        chain = _fit.open_chain(self, Y, X, intercept, radii, _fit.chain_seed(rng))
        n_ic = 2 if self.is_directed else 1
        self.intercept_samplers = [_ScalarMetropolis(self.step_size_intercept, self.tune)
                                   for _ in range(n_ic)]
        self.radii_sampler = _ScalarMetropolis(self.step_size_radii, self.tune, dirichlet=True)

        self.Xs_ = np.zeros((n_total, T, N, D))
        self.intercepts_ = np.zeros((n_total, n_ic))
        self.mus_ = np.zeros((n_total, K, D))
        self.sigmas_ = np.zeros((n_total, K))
        self.zs_ = np.zeros((n_total, T, N), dtype=np.int64)
        self.init_weights_ = np.zeros((n_total, K))
        self.trans_weights_ = np.zeros((n_total, K, K))
        self.lambdas_ = np.zeros((n_total, 1))
        self.radiis_ = np.zeros((n_total, N)) if self.is_directed else None
        self.logps_ = np.zeros(n_total)

        lmbda = np.array([self.lambda_prior], dtype=np.float64)
        chain.set_prior_mixture(mu, sigma, lmbda, z)
        self._n_total, self._rng, self._ip = n_total, rng, ip
        self._sums = hu.DeviceLabelSums(chain)
        self._st = dict(X=X, intercept=intercept, mu=mu, sigma=sigma, z=z,
                        init_w=np.bincount(z[0], minlength=K) / float(N),
                        trans_w=np.full((K, K), 1. / K), lmbda=lmbda, radii=radii)
        self._store(0, chain.loglik_full())
        if self._miss_index is not None:
            chain.set_missing(self._miss_index)
        return self

    def _store(self, it, ll):
        st = self._st
        self.Xs_[it], self.intercepts_[it] = st['X'], st['intercept']
        self.mus_[it], self.sigmas_[it], self.zs_[it] = st['mu'], st['sigma'], st['z']
        self.init_weights_[it], self.trans_weights_[it] = st['init_w'], st['trans_w']
        self.lambdas_[it] = st['lmbda']
        if self.is_directed:
            self.radiis_[it] = st['radii']
        self.logps_[it] = np.ravel(ll + hu.lpcm_log_posterior_terms(
            self._sums, st['intercept'], self._ip, self.intercept_variance_prior, st['mu'],
            st['sigma'], st['init_w'], st['trans_w'], st['lmbda'], self.hyper_,
            self.dirichlet_prior_, radii=st['radii']))[0]

    def _run(self, first, count):
        """Gibbs iterations first .. first + count - 1 (lpcm.py:562-700): the kernels of the engine
        around numpy draws on the caller's MT19937 stream"""
        chain, rng, st, T = self.chain_, self._rng, self._st, self.chain_.T
        X, intercept, mu, sigma, radii = st['X'], st['intercept'], st['mu'], st['sigma'], st['radii']
        init_w, trans_w, lmbda = st['init_w'], st['trans_w'], st['lmbda']
        for it in range(first, first + count):
            if self.case_control_sampler_ is not None:
                self.case_control_sampler_.resample(it)
            chain.set_prior_mixture(mu, sigma, lmbda, None)      # z: the device keeps its own
            chain.sweep_positions(it, self.sweep_algo)
            chain.center()
            intercept, radii, ll = _fit.coefficient_steps(
                chain, rng, intercept, radii, self._ip, self.intercept_variance_prior,
                self.intercept_samplers, self.radii_sampler)
            z, n, nk = chain.sample_labels(it, self._stack(init_w, trans_w, T))
            X = chain.get_positions()
            mu, sigma = mu.copy(), sigma.copy()
            init_w, trans_w = init_w.copy(), trans_w.copy()
            lmbda = hu.lpcm_gibbs_updates(self._sums, n, nk, mu, sigma, init_w, trans_w, lmbda,
                                          self.hyper_, rng, self.dirichlet_prior_)
            if self._miss_index is not None:         # lpcm.py:676-689, with the draw written back
                chain.impute_missing(it, it > self.n_burn_)
            if self._miss is not None:               # lpcm.py:676-689
                y_ij = _fit.draw_missing(rng, X, intercept[0], self._miss)
                if it > self.n_burn_:
                    self.missings_ += y_ij
            st.update(X=X, intercept=intercept, mu=mu, sigma=sigma, z=z, init_w=init_w,
                      trans_w=trans_w, lmbda=lmbda, radii=radii)
            self._store(it, ll)

    def _finish(self):
        """Everything of ``fit`` after the Gibbs loop (lpcm.py:703-760)."""
        chain = self.chain_
        if self._miss is not None:
            self.missings_ /= max(1, self._n_total - self.n_burn_)
        if self._miss_index is not None:
            _missing_attributes(self, chain, self._miss_index)
        chain.get_samplers(self.latent_samplers)
        self.mean_variance_prior_, self.b_ = self.hyper_.mean_variance_prior, self.hyper_.b

        _fit.thin_traces(self, ('Xs_', 'intercepts_', 'mus_', 'sigmas_', 'zs_', 'init_weights_',
                                'trans_weights_', 'lambdas_', 'logps_'))
        n_burn = min(self.n_burn_, self.logps_.shape[0] - 1)
        self.cooccurrence_probas_ = post.posterior_cooccurrences(self, chain, n_burn)
        if self.selection_type == 'map':
            # lpcm.py:724 takes the argmax over logps_[n_burn:] and uses it as an index into
            # the full trace (without adding n_burn); kept as it is
            best = int(np.argmax(self.logps_[n_burn:]))
        else:
            best, self.expected_vis_ = post.minimize_posterior_expected_vi(
                self, chain, n_burn, cooc=self.cooccurrence_probas_)
        chain.post_release()
        self.selected_id_ = best
        self.logp_ = self.logps_[best]
        self.X_, self.intercept_ = self.Xs_[best].copy(), self.intercepts_[best]
        self.lambda_ = self.lambdas_[best]
        if self.is_directed:
            self.radii_ = self.radiis_[best]
        self.z_ = self.zs_[best]
        self.init_weight_, self.trans_weight_ = self.init_weights_[best], self.trans_weights_[best]
        self.mu_, self.sigma_ = self.mus_[best].copy(), self.sigmas_[best]
        post.procrustes_align_samples(self)          # lpcm.py:742-749
        self.X_mean_ = self.Xs_[n_burn:].mean(axis=0)
        self.lambda_mean_ = self.lambdas_[n_burn:].mean(axis=0)
        self.intercepts_mean_ = self.intercepts_[n_burn:].mean(axis=0)
        if self.is_directed:
            self.radii_mean_ = self.radiis_[n_burn:].mean(axis=0)
        return self
