"""What ``DynamicNetworkLSM``, ``DynamicNetworkLPCM`` and ``DynamicNetworkHDPLPCM`` share: the checks
and bookkeeping of ``fit`` before the Gibbs loop, the chain set-up, the warm start and hyper-priors of
the two mixture models, the host-driven coefficient step, and what copies the device loops' state
back.  Plain functions of the estimator (``est``); the only class-level sharing is ``Estimator``.
"""
import numpy as np
from scipy.special import gammaln, xlogy

from .engine import Chain, SamplerGrid, check_n_features
from . import hdp_updates as hu
from . import initialization as init_mod
from .imputer import SimpleNetworkImputer, fill_missing_lists
from .metrics import FittedQuantities, missing_index
from .sparse import SparseNetwork


def check_random_state(seed):
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError('%r cannot be used to seed a numpy.random.RandomState' % seed)


class _ScalarMetropolis(object):
    """Host mirror of metropolis.py:85-136 for the scalar / Dirichlet blocks
    the directed models update from the host."""

    def __init__(self, step_size, tune, tune_interval=100, dirichlet=False):
        self.step_size, self.tune, self.tune_interval = step_size, tune, tune_interval
        self.steps_until_tune = tune_interval
        self.n_accepted = 0
        self.n_steps = 0
        self.dirichlet = dirichlet

    def book(self, accepted):
        self.n_accepted += accepted
        self.n_steps += 1
        if self.tune is not None:
            if self.n_steps < self.tune and self.steps_until_tune == 0:
                r = self.n_accepted / self.tune_interval
                s = self.step_size
                if self.dirichlet:      # metropolis.py:23-37
                    s *= (10.0 if r < 0.001 else 2 if r < 0.05 else 1.1 if r < 0.25 else
                          0.1 if r > 0.95 else 0.5 if r > 0.75 else 0.9 if r > 0.4 else 1)
                else:                   # metropolis.py:5-20
                    s *= (0.1 if r < 0.001 else 0.5 if r < 0.05 else 0.9 if r < 0.25 else
                          10.0 if r > 0.95 else 2.0 if r > 0.75 else 1.1 if r > 0.4 else 1)
                self.step_size = s
                self.n_accepted = 0
                self.steps_until_tune = self.tune_interval
            else:
                self.steps_until_tune -= 1


def _dirichlet_logpdf(x, alpha):
    """scipy.stats.dirichlet.logpdf(x, alpha) without its input checks (the proposal
    density ratio of metropolis.py:70-76)"""
    return gammaln(np.sum(alpha)) - np.sum(gammaln(alpha)) + np.sum(xlogy(alpha - 1.0, x))


class Estimator(FittedQuantities):
    """what the three estimators inherit beyond the fitted quantities"""

    def _forecast_ready(self):
        """the chain of a fitted undirected model, for the one-step-ahead forecasts of ``forecast.py``"""
        if not hasattr(self, 'X_'):
            raise ValueError('Model not fit.')
        if self.is_directed:
            raise ValueError('forecasts are implemented for undirected models '
                             '(as the reference formulas are)')
        return self.chain_

    def forecast(self, horizon=1, **kw):
        """posterior predictive forecast of the next ``horizon`` networks, drawn on the device; undirected and
        directed fits (``forecast_paths.forecast``)"""
        from .forecast_paths import forecast
        return forecast(self, horizon=horizon, **kw)


# ---- before the loop ---------------------------------------------------------------------------
def check_network(Y, copy=True):
    """``Y`` as a C-ordered float64 (T, N, N) array, copied as ``numpy.array(copy=copy)`` does;
    ``copy=None`` keeps a float64 array as it is, whatever its order (for a caller that never reads it).
    A ``SparseNetwork`` passes through as it is (tested first: ``numpy.asarray`` of it would densify)."""
    if isinstance(Y, SparseNetwork):
        return Y
    Y = (np.asarray(Y, dtype=np.float64) if copy is None
         else np.array(Y, dtype=np.float64, copy=copy, order='C'))
    if Y.ndim != 3 or Y.shape[1] != Y.shape[2]:
        raise ValueError('Y must have shape (n_time_steps, n_nodes, n_nodes)')
    if np.any(np.isnan(Y)):
        raise ValueError('NaN entries are not supported: code missing dyads as -1')
    return Y


def check_options(est):
    if est.sample_missing and est.n_control is not None:
        raise ValueError('sample_missing=True is not supported with n_control: the case-control '
                         'chain holds edge lists and control samples, not the dyads to re-draw')
    if est.n_control is not None and not est.is_directed:
        raise ValueError('The case-control likelihood currently only '
                         'supported for directed networks.')


def sparse_network(est, Y, missing_lists=True):
    """``Y`` if it is no ``SparseNetwork``; else the container as the estimator sees it - symmetrised
    for an undirected model - and without missing dyads: neither ``impute`` nor ``prepare_missing`` is
    for it.  Returns ``(Y, is_sparse, held)``.

    A container that lists missing dyads is validated on a temporary chain of the estimator's model
    (a dyad listed both as a tie and as missing is an error there), which also returns the canonical
    index - the distinct dyads, row-major, i < j undirected.  They get their first fill
    (``imputer.fill_missing_lists``) and the returned container is the filled one; ``held`` is
    ``(Y with its lists, index)`` for ``Chain.set_missing_edges`` / ``_missing_attributes`` when
    ``sample_missing`` is set, else None.  ``missing_lists=False``: the estimator takes no such
    container.  The refusals answer before any chain is opened."""
    if not isinstance(Y, SparseNetwork):
        return Y, False, None
    if Y.has_missing and not missing_lists:
        raise ValueError('%s does not take a SparseNetwork that lists missing dyads: its warm start '
                         're-imputes them from dense edge probabilities (fit the dense array)'
                         % type(est).__name__)
    if Y.has_missing and est.n_control is not None:
        raise ValueError('n_control is not supported with a SparseNetwork that lists missing dyads: the '
                         'case-control chain holds edge tables and control samples, not the dyads to fill')
    if est.sample_missing and not Y.has_missing:
        raise ValueError('sample_missing=True is not supported with a SparseNetwork that lists no '
                         'missing dyads')
    est.nan_mask_ = None
    symmetric = not est.is_directed
    if not Y.has_missing:
        return Y.as_seen(symmetric), True, None
    T, N, _ = Y.shape
    with Chain(T, N, check_n_features(est.n_features), model_name(est), device=est.device) as tmp:
        tmp.upload_network_edges(Y)
        tmp.set_missing_edges(Y, allow_ties=False)
        index = tmp.get_missing_index()
    n_observed = Y.degrees(symmetric)[:, :, 1].sum(axis=1)
    ties = fill_missing_lists(index, n_observed, N) == 1
    filled = Y.with_ties(index[ties]).without_missing().as_seen(symmetric)
    return filled, True, ((Y, index) if est.sample_missing else None)


def impute(Y):
    """the one-off imputation of the -1 coded dyads before the chain (lsm.py:345-359)"""
    return SimpleNetworkImputer(strategy='random', missing_value=-1).fit_transform(Y)


def prepare_missing(est, Y):
    """Missing-dyad bookkeeping of the mixture models (lpcm.py:352-366, hdp_lpcm.py:669-706): sets
    ``nan_mask_`` (and zeroes ``missings_`` where the host will average draws into it) and returns the
    network imputed once, ``miss`` and ``miss_index``.  ``miss``: the (t, i, j) index arrays, row-major
    with i < j, of the dyads an undirected model draws on the host every iteration; ``miss_index``:
    the (n, 3) rows that ``sample_missing=True`` has the device draw instead (no host draws then)."""
    est.nan_mask_, miss, miss_index = None, None, None
    if not np.any(Y == -1):
        return Y, miss, miss_index
    if est.sample_missing:
        miss_index = missing_index(Y, est.is_directed)
    if not est.is_directed:
        iu = np.nonzero(np.triu(np.ones(Y.shape, dtype=bool), 1))
        est.nan_mask_ = Y[iu] == -1
        if miss_index is None:
            miss = np.nonzero(np.triu(Y == -1, 1))
            est.missings_ = np.zeros(miss[0].shape[0])
    else:
        off = np.nonzero(~np.eye(Y.shape[1], dtype=bool)[None].repeat(Y.shape[0], 0))
        est.nan_mask_ = Y[off] == -1
    return impute(Y), miss, miss_index


def extend_n_iter(est):
    """``n_iter`` counts the burn-in and tuning iterations too; the reference mutates it as well
    (lsm.py:362-368).  Returns the total."""
    est.n_iter += (est.burn or 0) + (est.tune or 0)
    return est.n_iter


def model_name(est):
    return ('undirected' if not est.is_directed else
            'case_control' if est.n_control is not None else 'directed')


def chain_seed(rng):
    """the 62-bit seed of the chain's Philox streams, from two draws of the caller's stream"""
    return int(rng.randint(0, 2 ** 31 - 1)) | (int(rng.randint(0, 2 ** 31 - 1)) << 31)


def init_values(est, init):
    """``X``, ``intercept`` and ``radii`` (None unless directed) of ``fit(Y, init=...)``"""
    X = np.array(init['X'], dtype=np.float64)
    intercept = np.atleast_1d(np.asarray(init['intercept'], dtype=np.float64)).copy()
    radii = np.array(init['radii'], dtype=np.float64) if est.is_directed else None
    return X, intercept, radii


def resolve_intercept_prior(est, intercept):
    """``intercept_prior='auto'`` is the starting value; returns the prior mean as an array"""
    if isinstance(est.intercept_prior, str) and est.intercept_prior == 'auto':
        est.intercept_prior = intercept.copy()
    return np.atleast_1d(np.asarray(est.intercept_prior, dtype=np.float64))


def open_chain(est, Y, X, intercept, radii, seed, network_from=None):
    """The chain handle with the network (or the case-control sampler's edge lists), the starting
    values and the latent-position samplers: sets ``chain_``, ``case_control_sampler_`` and
    ``latent_samplers``.  ``network_from``: callable(chain) that loads the network some other way than
    the float64 upload."""
    T, N, _ = Y.shape
    model = model_name(est)
    chain = Chain(T, N, check_n_features(est.n_features), model, seed=seed, chain_id=est.chain_id,
                  device=est.device)
    est.chain_ = chain
    est.case_control_sampler_ = None
    if model == 'case_control':
        from .case_control import DirectedCaseControlSampler
        est.case_control_sampler_ = DirectedCaseControlSampler(
            n_control=est.n_control, n_resample=est.n_resample_control, chain=chain).init(Y)
    elif network_from is not None:
        network_from(chain)
    elif isinstance(Y, SparseNetwork):
        chain.upload_network_edges(Y)
    else:
        chain.upload_network(Y)
    chain.set_positions(X)
    chain.set_intercepts(intercept)
    if est.is_directed:
        chain.set_radii(radii)
    est.latent_samplers = SamplerGrid(T, N, est.step_size_X, tune=est.tune,
                                      tune_interval=est.tune_interval)
    chain.set_samplers(est.latent_samplers)
    return chain


def warm_start(est, Y, rng, init, Y_raw=None, kmeans_on_device=False):
    """Starting values of the mixture models (lpcm.py:45-132, hdp_lpcm.py:48-141): positions,
    intercepts and radii from ``init`` or a short LSM fit, then cluster means, scales and labels from
    ``init`` or longitudinal k-means.  Returns ``(Y, X, intercept, radii, mu, sigma, z)``.

    ``Y_raw`` (LPCM): the warm start is fitted on the network with its -1 coded dyads, and they are
    imputed again by thresholding its edge probabilities (lpcm.py:77-81) - the returned ``Y``.
    ``kmeans_on_device`` (HDP-LPCM): the Lloyd iterations run on a temporary chain, not on the host."""
    from .lsm import DynamicNetworkLSM
    N, D = Y.shape[1], check_n_features(est.n_features)
    if init is not None and 'X' in init:
        X, intercept, radii = init_values(est, init)
    else:
        kw = (dict(sigma_sq=0.001, tau_sq='auto', step_size_X=0.0075,
                   n_control=est.n_control, n_resample_control=est.n_resample_control)
              if est.is_directed else dict(sigma_sq=0.1, tau_sq=2.0, step_size_X=0.1))
        emb = DynamicNetworkLSM(n_iter=500, n_features=D, tune=250, burn=250,
                                is_directed=est.is_directed, random_state=rng,
                                device=est.device, chain_id=est.chain_id,
                                sweep_algo=est.sweep_algo, **kw).fit(Y if Y_raw is None else Y_raw)
        X, intercept = emb.X_.copy(), np.array(emb.intercept_, dtype=np.float64)
        radii = emb.radii_.copy() if est.is_directed else None
        if Y_raw is not None and not isinstance(Y_raw, SparseNetwork) and np.any(Y_raw == -1):
            Y = Y_raw.copy()
            Y[Y_raw == -1] = emb.probas_[Y_raw == -1] > 0.5
        emb.chain_.close()
    if init is not None and 'mu' in init:
        mu = np.array(init['mu'], dtype=np.float64)
        sigma = np.array(init['sigma'], dtype=np.float64)
        z = np.array(init['z'], dtype=np.int64)
    elif kmeans_on_device:      # any handle will do
        with Chain(1, N, D, 'undirected', device=est.device) as tmp:
            mu, sigma, z = init_mod.longitudinal_kmeans(X, n_clusters=est.n_components,
                                                        random_state=rng, chain=tmp)
    else:
        mu, sigma, z = init_mod.longitudinal_kmeans(X, n_clusters=est.n_components, random_state=rng)
    return Y, X, intercept, radii, mu, sigma, z.astype(np.int64)


def mixture_hyper(est, N, D, intercept, **hdp_only):
    """The hyper-priors of the mixture models (lpcm.py, hdp_lpcm.py:760-793) as an ``HDPHyper``, and
    the intercept prior mean; resolves ``step_size_X``, ``intercept_prior``, ``mean_variance_prior``
    and ``b`` from ``'auto'``.  ``hdp_only``: the HDP's concentration parameters and their priors."""
    if isinstance(est.step_size_X, str) and est.step_size_X == 'auto':
        est.step_size_X = 0.01 if est.is_directed else 0.1
    ip = resolve_intercept_prior(est, intercept)
    if isinstance(est.mean_variance_prior, str) and est.mean_variance_prior == 'auto':
        mvp = (2 * (1. / N) ** (2. / D) if est.is_directed else (N ** (2. / D)) / 50.)
    else:
        mvp = est.mean_variance_prior
    hp = hu.HDPHyper(est.n_components, mean_variance_prior=mvp, a=est.a,
                     lambda_prior=est.lambda_prior,
                     lambda_variance_prior=est.lambda_variance_prior, **hdp_only)
    if est.mean_variance_prior_std is not None:
        hp.a0 = (est.mean_variance_prior_std ** 2 + 2) * 2
        hp.b0 = (hp.a0 - 2) * mvp * 2
    hp.b = (est.a + 2) * mvp if (isinstance(est.b, str) and est.b == 'auto') else est.b
    if est.sigma_prior_std is not None:
        hp.d0 = (est.sigma_prior_std ** 2 / hp.b) * 2
        hp.c0 = hp.b * hp.d0
    return hp, ip


# ---- inside the loop ---------------------------------------------------------------------------
def coefficient_steps(chain, rng, intercept, radii, ip, var, isamp, rsamp, group_proposal_terms=False):
    """The host-driven coefficient step (sample_coefficients.py:12-121, metropolis.py:40-82) at the
    chain's positions: one scalar random-walk Metropolis step per sampler of ``isamp`` on the
    intercepts, each over a fused pass, then - iff ``radii`` is not None - the Dirichlet Metropolis
    step on the radii.  Draws from ``rng`` in the reference's order: one normal and one uniform
    draw per intercept, then the Dirichlet proposal and one uniform draw.  Returns ``(intercept,
    radii, ll)``, ``ll`` the log-likelihood at the returned state; the chain holds that state too.

    ``group_proposal_terms``: add the difference of the two proposal densities to the radii step's
    ratio as one term, as metropolis.py:70-74 does, instead of one density after the other."""
    for k, samp in enumerate(isamp):
        prop = intercept.copy()
        prop[k] = intercept[k] + samp.step_size * rng.randn(1)[0]
        if k == 0:
            ll_prop, ll_cur = chain.loglik_full([prop, intercept])
        else:       # same positions, and `intercept` is the state the last step left:
            ll_prop, ll_cur = chain.loglik_full([prop])[0], ll      # its value is known
        ratio = ((ll_prop - (prop[k] - ip[k]) ** 2 / (2 * var)) -
                 (ll_cur - (intercept[k] - ip[k]) ** 2 / (2 * var)))
        accepted = int(not (np.log(rng.rand()) >= ratio))
        ll = ll_cur
        if accepted:
            intercept, ll = prop, ll_prop
        samp.book(accepted)
    chain.set_intercepts(intercept)
    if radii is not None:
        x = rng.dirichlet(rsamp.step_size * radii)
        if np.any(x == 0.):     # occasionally draws are zero due to precision (metropolis.py:63-67)
            x += 1e-5
            x /= np.sum(x)
        ll_cur, ll_prop = chain.loglik_full_radii(x)
        back = _dirichlet_logpdf(radii, rsamp.step_size * x)
        forth = _dirichlet_logpdf(x, rsamp.step_size * radii)
        ratio = ((ll_prop - ll_cur) + (back - forth) if group_proposal_terms
                 else ll_prop - ll_cur + back - forth)
        # a NaN ratio (a proposal that is not finite: every gamma variate underflowed) rejects; the
        # reference's `log(u) >= ratio` would accept it and keep NaN radii for good
        accepted = int(np.log(rng.rand()) < ratio)
        ll = ll_cur
        if accepted:
            radii, ll = x, ll_prop
            chain.set_radii(radii)
        rsamp.book(accepted)
    return intercept, radii, ll


def draw_missing(rng, X, intercept0, miss):
    """one Bernoulli draw of every missing dyad of an undirected model from its conditional
    (lpcm.py:676-689, hdp_lpcm.py:1039-1049); ``miss`` as ``prepare_missing`` returns it"""
    dm = X[miss[0], miss[1]] - X[miss[0], miss[2]]
    eta = intercept0 - np.sqrt(np.sum(dm * dm, axis=1))
    return rng.binomial(1, 1. / (1. + np.exp(-eta)))


def run_ranges(ccs, first, last, run):
    """``run(it, count)`` over the iterations first .. last of a device loop: one call, or with a
    case-control sampler ``ccs`` one call per maximal range between two resamplings of the controls,
    whose cadence the host keeps (case_control_likelihood.py:27-33)"""
    if ccs is None:
        run(first, last - first + 1)
        return
    it = first
    while it <= last:
        ccs.resample(it)
        nxt = it + 1                  # next iteration that resamples
        # n_resample=None: never resample (case_control_likelihood.py:28)
        while nxt <= last and (ccs.n_resample is None or ccs.n_iter % ccs.n_resample != 0):
            ccs.n_iter += 1
            nxt += 1
        run(it, nxt - it)
        it = nxt


# ---- after the loop ----------------------------------------------------------------------------
def _sampler_state(sm, step_size, n_accepted, n_steps, steps_until_tune=None):
    sm.step_size, sm.n_accepted, sm.n_steps = step_size, n_accepted, n_steps
    if steps_until_tune is not None:
        sm.steps_until_tune = steps_until_tune
    return sm


def samplers_from_lsm_config(est, cfg):
    """``intercept_samplers`` (and ``radii_sampler``) of an LSM fit from the device loop's state"""
    # lsm.py:465-467: the undirected intercept sampler ignores tune_interval
    n_ic, interval = (2, est.tune_interval) if est.is_directed else (1, 100)
    est.intercept_samplers = [
        _sampler_state(_ScalarMetropolis(cfg.i_step_size[k], est.tune, interval), cfg.i_step_size[k],
                       cfg.i_n_accepted[k], cfg.i_n_steps[k], cfg.i_steps_until_tune[k])
        for k in range(n_ic)]
    if est.is_directed:
        est.radii_sampler = _sampler_state(_ScalarMetropolis(cfg.r_step_size, None, dirichlet=True),
                                           cfg.r_step_size, cfg.r_n_accepted, cfg.r_n_steps)


def samplers_from_hdp_config(est, cfg):
    """the hyper-parameters the HDP-LPCM's device loop resampled -> ``hyper_``, and its samplers' state
    -> ``intercept_samplers`` (and ``radii_sampler``)"""
    hp = est.hyper_
    hp.gamma, hp.alpha_init, hp.alpha, hp.kappa = cfg.gamma, cfg.alpha_init, cfg.alpha, cfg.kappa
    hp.mean_variance_prior, hp.b = cfg.mean_variance_prior, cfg.b
    _sampler_state(est.intercept_samplers[0], cfg.i_step_size, cfg.i_n_accepted, cfg.i_n_steps,
                   cfg.i_steps_until_tune)
    if est.is_directed:
        _sampler_state(est.intercept_samplers[1], cfg.i_step_size_out, cfg.i_n_accepted_out,
                       cfg.i_n_steps_out, cfg.i_steps_until_tune_out)
        _sampler_state(est.radii_sampler, cfg.r_step_size, cfg.r_n_accepted, cfg.r_n_steps,
                       cfg.r_steps_until_tune)


def _missing_attributes(est, chain, index):
    """``missing_index_``, ``missing_probas_`` and ``missings_`` of a ``sample_missing=True`` fit from
    the chain's accumulators (NaN when no iteration beyond the burn-in accumulated)"""
    p_sum, ones, k = chain.get_missing()
    est.missing_index_ = index
    est.n_missing_accumulated_ = k
    with np.errstate(invalid='ignore', divide='ignore'):
        est.missing_probas_ = p_sum / k if k else np.full(p_sum.shape, np.nan)
        est.missings_ = ones / float(k) if k else np.full(p_sum.shape, np.nan)



def thin_traces(est, names):
    """keep every ``thin``-th stored sample (lpcm.py:703-716, hdp_lpcm.py:1072-1083)"""
    if est.thin is None:
        return
    for name in names + (('radiis_',) if est.is_directed else ()):
        setattr(est, name, getattr(est, name)[::est.thin])
