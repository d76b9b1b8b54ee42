"""The host logic the three estimators share (``dynetlsm_amd/_fit.py``), without a device: the
coefficient step against a fake chain and a second, equally seeded numpy stream; the cadence of the
control resampling around ranged device runs; the input checks of ``fit``; the missing-dyad
bookkeeping; the 'auto' hyper-priors."""
import numpy as np
import pytest

from dynetlsm_amd import (DynamicNetworkHDPLPCM, DynamicNetworkLPCM, DynamicNetworkLSM, _fit,
                          metrics)


# ---- coefficient_steps ------------------------------------------------------------------------
def _ll(ic, radii):
    """a fixed smooth function of the intercepts and the radii"""
    ll = -40.0 - 3.0 * np.sum((np.asarray(ic) - 0.4) ** 2)
    return ll if radii is None else ll - 60.0 * np.sum((radii - 1.0 / radii.shape[0]) ** 2)


class FakeChain:
    """``loglik_full`` evaluates the intercepts it is given at the radii last set; ``loglik_full_radii``
    (current, proposed) at the intercepts last set"""

    def __init__(self, ic, radii):
        self.ic, self.radii, self.calls = np.array(ic), radii, []

    def loglik_full(self, ics):
        self.calls.append(('loglik_full', [np.array(i) for i in ics]))
        return [_ll(i, self.radii) for i in ics]

    def loglik_full_radii(self, x):
        self.calls.append(('loglik_full_radii', np.array(x)))
        return _ll(self.ic, self.radii), _ll(self.ic, x)

    def set_intercepts(self, ic):
        self.calls.append(('set_intercepts', np.array(ic)))
        self.ic = np.array(ic)

    def set_radii(self, r):
        self.calls.append(('set_radii', np.array(r)))
        self.radii = np.array(r)


class Sampler:
    def __init__(self, step_size):
        self.step_size, self.booked = step_size, []

    def book(self, accepted):
        self.booked.append(accepted)


def _same_stream(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


IP, VAR = np.array([0.1, -0.2]), 2.0


def _replay_intercepts(rng, chain_calls, ic, radii, steps):
    """the documented draw order - randn(1), rand() per intercept - on ``rng``: checks the proposals the
    chain saw and returns (intercept, ll, flags)"""
    flags, ll = [], None
    for k, step in enumerate(steps):
        prop = ic.copy()
        prop[k] = ic[k] + step * rng.randn(1)[0]
        name, seen = chain_calls[k]
        assert name == 'loglik_full'
        # the first step is a fused two-candidate pass; the later ones evaluate the proposal alone
        assert len(seen) == (2 if k == 0 else 1)
        assert np.array_equal(seen[0], prop)
        if k == 0:
            assert np.array_equal(seen[1], ic)
            ll = _ll(ic, radii)
        ll_prop = _ll(prop, radii)
        ratio = ((ll_prop - (prop[k] - IP[k]) ** 2 / (2 * VAR)) - (ll - (ic[k] - IP[k]) ** 2 / (2 * VAR)))
        accepted = int(np.log(rng.rand()) < ratio)
        flags.append(accepted)
        if accepted:
            ic, ll = prop, ll_prop      # the next step's current value is this step's result
    return ic, ll, flags


def test_coefficient_steps_directed_draw_order_and_bookkeeping():
    outcomes = set()
    for seed in range(24):
        ic0 = np.array([0.7, -0.5])
        radii0 = np.random.RandomState(100 + seed).dirichlet(np.full(6, 5.0))
        chain = FakeChain(ic0, radii0.copy())
        isamp, rsamp = [Sampler(0.8), Sampler(0.5)], Sampler(40.0)
        rng, twin = np.random.RandomState(seed), np.random.RandomState(seed)
        ic, radii, ll = _fit.coefficient_steps(chain, rng, ic0.copy(), radii0.copy(), IP, VAR, isamp, rsamp)

        want_ic, want_ll, flags = _replay_intercepts(twin, chain.calls, ic0, radii0, [0.8, 0.5])
        assert [s.booked for s in isamp] == [[flags[0]], [flags[1]]]
        assert np.array_equal(ic, want_ic)
        # set_intercepts once, after the intercept steps and before the radii pass
        assert [c[0] for c in chain.calls].count('set_intercepts') == 1
        assert chain.calls[2][0] == 'set_intercepts' and np.array_equal(chain.calls[2][1], want_ic)
        x = twin.dirichlet(40.0 * radii0)
        assert chain.calls[3][0] == 'loglik_full_radii' and np.array_equal(chain.calls[3][1], x)
        ll_prop = _ll(want_ic, x)
        ratio = (ll_prop - want_ll + _fit._dirichlet_logpdf(radii0, 40.0 * x)
                 - _fit._dirichlet_logpdf(x, 40.0 * radii0))
        accepted = int(np.log(twin.rand()) < ratio)
        assert rsamp.booked == [accepted]
        assert len(chain.calls) == 4 + accepted
        if accepted:
            assert chain.calls[4][0] == 'set_radii' and np.array_equal(chain.calls[4][1], x)
        assert np.array_equal(radii, x if accepted else radii0)
        assert ll == (ll_prop if accepted else want_ll)
        assert _same_stream(rng, twin)
        outcomes.add((flags[0], flags[1], accepted))
    assert {o[0] for o in outcomes} == {0, 1} and {o[1] for o in outcomes} == {0, 1}
    assert {o[2] for o in outcomes} == {0, 1}       # set_radii iff accepted was seen both ways


def test_coefficient_steps_groups_the_proposal_terms_on_request():
    """the two ways of summing the radii step's ratio decide alike away from a tie"""
    out = []
    for grouped in (False, True):
        chain = FakeChain([0.7, -0.5], np.full(4, 0.25))
        out.append(_fit.coefficient_steps(chain, np.random.RandomState(3), np.array([0.7, -0.5]),
                                          np.full(4, 0.25), IP, VAR, [Sampler(0.8), Sampler(0.5)],
                                          Sampler(40.0), group_proposal_terms=grouped))
    assert all(np.array_equal(a, b) for a, b in zip(*out))


def test_coefficient_steps_undirected():
    for seed in range(8):
        ic0 = np.array([0.9])
        chain, samp = FakeChain(ic0, None), Sampler(0.6)
        rng, twin = np.random.RandomState(seed), np.random.RandomState(seed)
        ic, radii, ll = _fit.coefficient_steps(chain, rng, ic0.copy(), None, IP, VAR, [samp], None)
        want_ic, want_ll, flags = _replay_intercepts(twin, chain.calls, ic0, None, [0.6])
        assert radii is None and np.array_equal(ic, want_ic) and ll == want_ll
        assert samp.booked == flags
        assert [c[0] for c in chain.calls] == ['loglik_full', 'set_intercepts']
        assert _same_stream(rng, twin)


class _ZeroDirichlet:
    """a numpy stream whose Dirichlet draw underflowed in one coordinate"""

    def __init__(self, seed, x):
        self.rs, self.x, self.alphas = np.random.RandomState(seed), x, []
        self.randn, self.rand = self.rs.randn, self.rs.rand

    def dirichlet(self, alpha):
        self.alphas.append(np.array(alpha))
        return self.x.copy()


def test_coefficient_steps_renormalises_a_zero_in_the_radii_proposal():
    radii0 = np.array([0.1, 0.2, 0.3, 0.4])
    x = np.array([0.0, 0.5, 0.3, 0.2])
    chain = FakeChain([0.7, -0.5], radii0.copy())
    rng = _ZeroDirichlet(0, x)
    _fit.coefficient_steps(chain, rng, np.array([0.7, -0.5]), radii0.copy(), IP, VAR,
                           [Sampler(0.8), Sampler(0.5)], Sampler(40.0))
    assert len(rng.alphas) == 1 and np.array_equal(rng.alphas[0], 40.0 * radii0)
    seen = [c[1] for c in chain.calls if c[0] == 'loglik_full_radii'][0]
    want = x + 1e-5
    want /= np.sum(want)
    assert np.array_equal(seen, want) and seen.min() > 0


def test_coefficient_steps_rejects_a_radii_proposal_that_is_not_finite():
    """every gamma variate of the Dirichlet draw underflowed: 0 / 0 in every coordinate.  The ratio is
    NaN, and the step is a rejection - radii kept, nothing set on the chain, booked as rejected -
    whichever way the ratio is summed"""
    radii0 = np.array([0.1, 0.2, 0.3, 0.4])
    for grouped in (False, True):
        chain = FakeChain([0.7, -0.5], radii0.copy())
        rng, rsamp = _ZeroDirichlet(0, np.full(4, np.nan)), Sampler(1e-3)
        with np.errstate(invalid='ignore'):
            ic, radii, ll = _fit.coefficient_steps(chain, rng, np.array([0.7, -0.5]), radii0.copy(), IP, VAR,
                                                   [Sampler(0.8), Sampler(0.5)], rsamp,
                                                   group_proposal_terms=grouped)
        assert len(rng.alphas) == 1
        seen = [c[1] for c in chain.calls if c[0] == 'loglik_full_radii'][0]
        assert np.all(np.isnan(seen))                   # (no zero to repair: NaN == 0 is false)
        assert rsamp.booked == [0]
        assert 'set_radii' not in [c[0] for c in chain.calls]
        assert np.array_equal(radii, radii0) and np.array_equal(chain.radii, radii0)
        assert np.isfinite(ll) and ll == _ll(ic, radii0)


# ---- run_ranges --------------------------------------------------------------------------------
class CountingSampler:
    """the cadence of DirectedCaseControlSampler.resample, counting instead of drawing"""

    def __init__(self, n_resample):
        self.n_resample, self.n_iter, self.sampled_at, self.resample_calls = n_resample, 1, [], []

    def resample(self, it):
        self.resample_calls.append(it)
        if self.n_resample is not None and self.n_iter % self.n_resample == 0:
            self.sampled_at.append(it)
        self.n_iter += 1


@pytest.mark.parametrize('n_resample', [1, 3, None])
@pytest.mark.parametrize('first,last', [(1, 11), (5, 5), (4, 10)])
def test_run_ranges_keeps_the_resampling_cadence(n_resample, first, last):
    ccs, ranges = CountingSampler(n_resample), []
    ccs.n_iter = first                  # what the iterations before `first` left
    _fit.run_ranges(ccs, first, last, lambda it, count: ranges.append((it, count, ccs.n_iter)))
    # the ranges tile first .. last
    assert ranges[0][0] == first and sum(c for _, c, _ in ranges) == last - first + 1
    assert all(a[0] + a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert all(c >= 1 for _, c, _ in ranges)
    assert ccs.n_iter == first + (last - first + 1)
    # one resample call per range, at its first iteration
    assert ccs.resample_calls == [r[0] for r in ranges]
    # against the per-iteration loop: controls are drawn at the same iterations, every range but the
    # first begins with a draw, and no range holds a second one
    ref = CountingSampler(n_resample)
    ref.n_iter = first
    for it in range(first, last + 1):
        ref.resample(it)
    assert ccs.sampled_at == ref.sampled_at
    assert [r[0] for r in ranges[1:]] == [it for it in ref.sampled_at if it > first]
    if n_resample is not None:          # a range ends exactly where n_iter % n_resample == 0
        assert all(n_iter % n_resample == 0 for _, _, n_iter in ranges[:-1])
    else:
        assert len(ranges) == 1


def test_run_ranges_without_a_sampler_is_one_call():
    ranges = []
    _fit.run_ranges(None, 3, 9, lambda it, count: ranges.append((it, count)))
    assert ranges == [(3, 7)]


# ---- the checks of fit -------------------------------------------------------------------------
def test_check_network_rejects_what_fit_rejected():
    Y = np.zeros((2, 5, 5))
    out = _fit.check_network(Y.astype(np.int64), True)
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (2, 5, 5)
    assert _fit.check_network(Y, True) is not Y
    Yn = Y.copy()
    Yn[0, 1, 2] = np.nan
    with pytest.raises(ValueError, match='NaN entries are not supported: code missing dyads as -1'):
        _fit.check_network(Yn, True)
    for bad in (np.zeros((2, 5, 4)), np.zeros((5, 5))):
        with pytest.raises(ValueError, match=r'Y must have shape \(n_time_steps, n_nodes, n_nodes\)'):
            _fit.check_network(bad, True)
    # a loader that never reads the array: a float64 array is kept as it is, whatever its order
    F = np.asfortranarray(Y)
    assert _fit.check_network(F, None) is F


@pytest.mark.parametrize('cls', [DynamicNetworkLSM, DynamicNetworkLPCM, DynamicNetworkHDPLPCM])
def test_check_options_rejects_what_fit_rejected(cls):
    with pytest.raises(ValueError, match='The case-control likelihood currently only supported for '
                                         'directed networks.'):
        _fit.check_options(cls(n_control=3))
    with pytest.raises(ValueError, match='sample_missing=True is not supported with n_control'):
        _fit.check_options(cls(n_control=3, is_directed=True, sample_missing=True))
    _fit.check_options(cls(n_control=3, is_directed=True))
    _fit.check_options(cls(sample_missing=True))


def test_hdp_sample_missing_needs_the_host_loop():
    """(the one option check that is the HDP-LPCM's own; it fires before anything touches a device)"""
    m = DynamicNetworkHDPLPCM(sample_missing=True, hdp_loop='device')
    with pytest.raises(ValueError, match="sample_missing=True runs on the host-driven loop"):
        m._prepare(np.zeros((2, 5, 5)))


# ---- prepare_missing ---------------------------------------------------------------------------
def _network(directed):
    rng = np.random.RandomState(5)
    Y = (rng.rand(2, 6, 6) < 0.4).astype(np.float64)
    for t in range(2):
        np.fill_diagonal(Y[t], 0)
    holes = [(0, 1, 2), (0, 0, 5), (1, 3, 4)]
    if directed:
        holes[1], holes[2] = (0, 5, 0), (1, 4, 3)
    else:
        Y = np.triu(Y, 1)
        Y = Y + Y.transpose(0, 2, 1)
    for t, i, j in holes:
        Y[t, i, j] = -1
        if not directed:
            Y[t, j, i] = -1
    return Y, holes


@pytest.mark.parametrize('cls', [DynamicNetworkLPCM, DynamicNetworkHDPLPCM])
@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('sample_missing', [False, True])
def test_prepare_missing(cls, directed, sample_missing):
    Y, holes = _network(directed)
    est = cls(is_directed=directed, sample_missing=sample_missing)
    Yi, miss, miss_index = _fit.prepare_missing(est, Y)
    assert set(np.unique(Yi)) <= {0.0, 1.0} and np.array_equal(Yi, _fit.impute(Y))
    if not directed:                    # (the reference's imputer symmetrises a directed slice)
        assert np.array_equal(Yi[Y != -1], Y[Y != -1])
    # nan_mask_ runs over the upper triangle of every slice (undirected) or over all off-diagonal
    # entries (directed), row-major, as the reference's does
    cells = [(t, i, j) for t in range(2) for i in range(6) for j in range(6)
             if (i != j if directed else i < j)]
    assert est.nan_mask_.shape == (len(cells),) == ((60,) if directed else (30,))
    assert [c for c, m in zip(cells, est.nan_mask_) if m] == sorted(holes)
    if sample_missing:
        assert miss is None and not hasattr(est, 'missings_')
        assert np.array_equal(miss_index, metrics.missing_index(Y, directed))
        assert miss_index.tolist() == [list(h) for h in sorted(holes)]
    elif directed:                      # the reference averages draws for undirected models only
        assert miss is None and miss_index is None and not hasattr(est, 'missings_')
    else:
        assert miss_index is None
        assert list(zip(*(m.tolist() for m in miss))) == sorted(holes)
        assert np.array_equal(est.missings_, np.zeros(3))


def test_prepare_missing_without_missing_dyads():
    Y = np.zeros((2, 6, 6))
    est = DynamicNetworkLPCM(sample_missing=True)
    Yi, miss, miss_index = _fit.prepare_missing(est, Y)
    assert Yi is Y and miss is None and miss_index is None and est.nan_mask_ is None


# ---- mixture_hyper -----------------------------------------------------------------------------
@pytest.mark.parametrize('directed,N,D', [(False, 100, 2), (True, 50, 2), (False, 30, 3)])
def test_mixture_hyper_auto_values(directed, N, D):
    est = DynamicNetworkHDPLPCM(is_directed=directed, n_components=7, a=2.0,
                                mean_variance_prior_std=4.0, sigma_prior_std=4.0)
    intercept = np.array([0.3, -0.1]) if directed else np.array([0.3])
    hp, ip = _fit.mixture_hyper(est, N, D, intercept, gamma=2.5, kappa=3.0)
    # E(tau_sq): 2 (1 / n_nodes)^(2 / n_features) for directed networks, n_nodes^(2 / n_features) / 50 else
    mvp = 2 * (1. / N) ** (2. / D) if directed else (N ** (2. / D)) / 50.
    assert hp.mean_variance_prior == mvp
    if (directed, N, D) == (False, 100, 2):
        assert mvp == 2.0               # "for n_nodes = 100, tau_sq = 2.0 is good, so use this scale"
    # tau_sq ~ Inv-Gamma(a0 / 2, b0 / 2)
    assert hp.a0 == (4.0 ** 2 + 2) * 2 == 36.0
    assert hp.b0 == (36.0 - 2) * mvp * 2
    # b 'auto', and b ~ Gamma(c0 / 2, 2 / d0) with E(b) = c0 / d0 = b
    assert hp.b == (2.0 + 2) * mvp
    assert hp.d0 == (4.0 ** 2 / hp.b) * 2
    assert hp.c0 == hp.b * hp.d0 and np.isclose(hp.c0 / hp.d0, hp.b)
    assert est.step_size_X == (0.01 if directed else 0.1)
    assert np.array_equal(est.intercept_prior, intercept) and est.intercept_prior is not intercept
    assert np.array_equal(ip, intercept)
    assert (hp.n_components, hp.a, hp.gamma, hp.kappa, hp.alpha) == (7, 2.0, 2.5, 3.0, 1.0)
    assert (hp.lambda_prior, hp.lambda_variance_prior) == (0.9, 0.01)


def test_mixture_hyper_given_values_and_switched_off_priors():
    est = DynamicNetworkLPCM(mean_variance_prior=1.5, b=0.7, step_size_X=0.05, intercept_prior=0.2,
                             mean_variance_prior_std=None, sigma_prior_std=None)
    hp, ip = _fit.mixture_hyper(est, 40, 2, np.array([0.9]))
    assert (hp.mean_variance_prior, hp.b, est.step_size_X) == (1.5, 0.7, 0.05)
    assert np.array_equal(ip, [0.2]) and est.intercept_prior == 0.2
    # no hyper-prior on tau_sq and b: HDPHyper's defaults stay
    assert (hp.a0, hp.b0, hp.c0, hp.d0) == (None, None, None, None)
