"""Multi-step posterior predictive forecasts on the device (csrc/kernels_forecast_paths.hpp,
dynetlsm_amd/forecast_paths.py) against the numpy replica tests/forecast_paths_ref.py.  Needs an MI355X: -m gpu.

Labels are compared exactly: the running sums of a transition row are the same sequence of double adds on both
sides.  Positions are held to PATH_ATOL = 1e-9, the bound tests/test_gpu_parity.py holds positions made of
device Box-Muller draws to against the oracle (``get_positions`` after a sweep, atol=1e-9); a wrong counter
moves a coordinate by a fraction of a standard deviation.  The largest deviation of every case is printed.
The probabilities are compared with the numpy mean of expit(eta) over the device's own paths at rtol=1e-12,
atol=1e-15, the bound of test_kernels_match_oracle."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import forecast_paths_ref as fpr  # noqa: E402
import score_cases  # noqa: E402
import score_ref  # noqa: E402

pytestmark = pytest.mark.gpu

PATH_ATOL = 1e-9
NS, DS, SS, HS, KS = (30, 65, 130), (1, 2, 3, 8), (1, 17, 33), (1, 3), (1, 4, 20)


def _grid():
    """every (N, D) pair, undirected and directed; S, H and the dynamics (random walk, K = 1, 4, 20) cycle so
    that every D meets every S (the LDS chunk is 16, 8 or 4 samples by D) and every value of the table occurs"""
    cases = []
    for a, N in enumerate(NS):
        for b, D in enumerate(DS):
            for directed in (False, True):
                S = SS[(a + b + directed) % 3]
                H = HS[(a + b) % 2]
                K = (0,) + KS
                cases.append((N, D, S, H, K[(2 * a + b + 2 * directed) % 4], directed))
    return cases


CASES = _grid()
IDS = ['N%d-D%d-S%d-H%d-%s-%s' % (N, D, S, H, 'K%d' % K if K else 'rw', 'dir' if directed else 'und')
       for N, D, S, H, K, directed in CASES]


def test_the_grid_covers_the_table():
    for col, values in zip(range(5), (NS, DS, SS, HS, (0,) + KS)):
        assert {c[col] for c in CASES} == set(values)
    for D in DS:
        assert {c[2] for c in CASES if c[1] == D} == set(SS)
        assert {c[5] for c in CASES if c[1] == D} == {False, True}


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


@pytest.fixture(scope='module')
def philox():
    from oracle import oracle as orc
    return orc.philox4x32


def _inputs(rng, S, N, D, K, directed):
    """arguments of Chain.forecast_paths: positions of unit scale, asymmetric radii and two intercepts for the
    directed model, raw transition rows (not normalised, some zero weights)"""
    kw = dict(X0=rng.randn(S, N, D) * (1.5 / np.sqrt(D)),
              intercepts=np.stack([rng.uniform(-0.5, 1.5, S), rng.uniform(-0.5, 1.5, S) if directed else np.zeros(S)],
                                  axis=1),
              radii=rng.uniform(0.5, 2.0, (S, N)) if directed else None)
    if K:
        w = rng.gamma(0.5, 1.0, (S, K, K)) + 1e-3
        if K > 1:
            w[:, :, 1] *= rng.rand(S, K) < 0.5
        kw.update(z0=rng.randint(0, K, (S, N)), trans=w, mu=rng.randn(S, K, D), sigma=rng.uniform(0.01, 0.3, (S, K)),
                  lmbda=rng.uniform(0.1, 0.9, S))
    else:
        kw['sigma_sq'] = 0.07
    return kw


def _replica(philox, kw, H, seed, first):
    return fpr.paths(philox, seed, first, kw['X0'], H, **{k: v for k, v in kw.items()
                                                           if k not in ('X0', 'intercepts', 'radii')})


def _chain(da, N, D, directed):
    return da.Chain(1, N, D, 'directed' if directed else 'undirected')


@pytest.mark.parametrize('N,D,S,H,K,directed', CASES, ids=IDS)
def test_paths_labels_and_probabilities_against_the_replica(da, philox, N, D, S, H, K, directed):
    rng = np.random.RandomState(N * 64 + D * 4 + K + directed)
    kw = _inputs(rng, S, N, D, K, directed)
    seed, first = 0x5EED0000ABCD + N, 5
    with _chain(da, N, D, directed) as c:
        probas, paths, labels = c.forecast_paths(horizon=H, seed=seed, first_index=first, want_paths=True,
                                                 want_labels=bool(K), **kw)
    want_paths, want_labels = _replica(philox, kw, H, seed, first)
    assert paths.shape == (S, H, N, D) and probas.shape == (H, N, N)
    if K:
        assert labels.shape == (S, H, N) and labels.dtype == np.int32
        np.testing.assert_array_equal(labels, want_labels)
        assert labels.min() >= 0 and labels.max() < K
    else:
        assert labels is None
    dev = np.abs(paths - want_paths).max()
    print('largest path deviation %.3e' % dev)
    assert dev <= PATH_ATOL
    ref = fpr.mean_probas(paths, kw['intercepts'], kw['radii'])
    print('largest probability deviation %.3e relative' % (np.abs(probas - ref) / np.maximum(ref, 1e-300)).max())
    np.testing.assert_allclose(probas, ref, rtol=1e-12, atol=1e-15)
    idx = np.arange(N)
    assert (probas[:, idx, idx] == 0).all()
    assert ((probas >= 0) & (probas <= 1)).all()
    if directed:
        assert not np.array_equal(probas, probas.swapaxes(1, 2))
    else:
        np.testing.assert_array_equal(probas, probas.swapaxes(1, 2))


@pytest.mark.parametrize('K,directed', [(0, False), (4, True), (20, False)])
def test_results_do_not_depend_on_the_batch_or_the_split(da, K, directed):
    rng = np.random.RandomState(17 + K)
    S, N, D, H = 33, 65, 3, 3
    kw = _inputs(rng, S, N, D, K, directed)

    def part(a, b):
        return {k: (v[a:b] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}

    with _chain(da, N, D, directed) as c:
        def run(args, seed=11, **more):
            return c.forecast_paths(horizon=H, seed=seed, want_paths=True, want_labels=bool(K), **args, **more)
        auto = run(kw)
        for batch in (1, 5):
            got = run(kw, batch=batch)
            np.testing.assert_array_equal(got[1], auto[1])
            if K:
                np.testing.assert_array_equal(got[2], auto[2])
            np.testing.assert_allclose(got[0], auto[0], rtol=1e-13, atol=0)
        a = run(part(0, 13), first_index=0)
        b = run(part(13, S), first_index=13, batch=7)
        other = run(kw, seed=12)
    np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), auto[1])
    if K:
        np.testing.assert_array_equal(np.concatenate([a[2], b[2]]), auto[2])
    np.testing.assert_allclose((13 * a[0] + (S - 13) * b[0]) / S, auto[0], rtol=1e-13, atol=0)
    assert np.abs(other[1] - auto[1]).min() > 0


@pytest.mark.parametrize('D', [1, 2, 8])
def test_a_random_walk_without_variance_stays_where_it_started(da, D):
    """sigma_sq = 0: every horizon is the mean probability at the samples' last positions"""
    rng = np.random.RandomState(D)
    S, N, H = 17, 65, 3
    kw = _inputs(rng, S, N, D, 0, False)
    kw['sigma_sq'] = 0.0
    with _chain(da, N, D, False) as c:
        probas, paths, _ = c.forecast_paths(horizon=H, seed=3, want_paths=True, **kw)
        want = c.forecast_mean_probas(kw['X0'], kw['intercepts'][:, 0], zero_diag=True)
    for h in range(H):
        np.testing.assert_array_equal(paths[:, h], kw['X0'])
        np.testing.assert_allclose(probas[h], want, rtol=1e-13, atol=0)


def test_one_hot_transitions_without_variance_have_a_closed_form(da):
    """labels never move and x_h = lmbda mu_g + (1 - lmbda) x_{h-1}, iterated"""
    rng = np.random.RandomState(4)
    S, N, D, H, K = 17, 30, 2, 3, 4
    kw = _inputs(rng, S, N, D, K, True)
    kw['trans'] = np.broadcast_to(np.eye(K) * 2.5, (S, K, K)).copy()
    kw['sigma'] = np.zeros((S, K))
    with _chain(da, N, D, True) as c:
        probas, paths, labels = c.forecast_paths(horizon=H, seed=3, want_paths=True, want_labels=True, **kw)
    x = kw['X0']
    lm = kw['lmbda'][:, None, None]
    m = np.take_along_axis(kw['mu'], kw['z0'][:, :, None].repeat(D, axis=2), axis=1)      # (S, N, D)
    for h in range(H):
        np.testing.assert_array_equal(labels[:, h], kw['z0'])
        x = lm * m + (1 - lm) * x
        np.testing.assert_allclose(paths[:, h], x, rtol=0, atol=1e-14)
    np.testing.assert_allclose(probas, fpr.mean_probas(paths, kw['intercepts'], kw['radii']), rtol=1e-12, atol=1e-15)


def test_one_component(da, philox):
    rng = np.random.RandomState(6)
    S, N, D, H = 17, 65, 2, 3
    kw = _inputs(rng, S, N, D, 1, False)
    with _chain(da, N, D, False) as c:
        _, paths, labels = c.forecast_paths(horizon=H, seed=8, want_paths=True, want_labels=True, **kw)
    assert (labels == 0).all()
    x = kw['X0']
    for h in range(1, H + 1):
        eps = np.stack([fpr.normals(philox, 8, s, h, N, D) for s in range(S)])
        lm = kw['lmbda'][:, None, None]
        x = lm * kw['mu'][:, :1] + (1 - lm) * x + np.sqrt(kw['sigma'][:, 0])[:, None, None] * eps
        assert np.abs(paths[:, h - 1] - x).max() <= PATH_ATOL


def test_bad_arguments_are_rejected(da):
    rng = np.random.RandomState(0)
    S, N, D, K = 3, 9, 2, 4
    kw = _inputs(rng, S, N, D, K, True)
    with _chain(da, N, D, True) as c:
        def code(**change):
            with pytest.raises(da.EngineError) as e:
                c.forecast_paths(**dict(kw, **change))
            return e.value.code
        assert code(horizon=65536) == -1
        assert code(first_index=2 ** 32 - 2) == -1
        assert code(batch=-1) == -1
        assert code(z0=np.full((S, N), K)) == -4
        assert code(radii=kw['radii'] * 0) == -4
        assert code(sigma=-kw['sigma']) == -4
        w = kw['trans'].copy()
        w[1, 2] = 0
        assert code(trans=w) == -4
        with pytest.raises(ValueError):
            c.forecast_paths(**dict(kw, radii=None))
        with pytest.raises(ValueError):
            c.forecast_paths(**dict(kw, mu=None))
        with pytest.raises(ValueError):
            c.forecast_paths(kw['X0'], kw['intercepts'], kw['radii'], sigma_sq=0.1, want_labels=True)
        with pytest.raises(da.EngineError) as e:
            c.forecast_paths(kw['X0'], kw['intercepts'], kw['radii'], sigma_sq=-0.1)
        assert e.value.code == -1
        # still usable afterwards
        probas, _, _ = c.forecast_paths(**kw)
        assert np.isfinite(probas).all()


class Fit(object):
    """the fitted attributes forecast() reads, around a synthetic LSM trace"""

    def __init__(self, rng, n, T, N, D, directed):
        self.is_directed, self.n_burn_, self.random_state, self.sigma_sq = directed, 2, 7, 0.05
        self.Y_fit_ = np.zeros((T, N, N))
        self.Xs_ = rng.randn(n, T, N, D)
        self.intercepts_ = rng.uniform(0.2, 1.2, (n, 2 if directed else 1))
        self.radiis_ = rng.uniform(0.5, 2.0, (n, N)) if directed else None
        self.X_, self.intercept_ = self.Xs_[-1], self.intercepts_[-1]
        self.radii_ = self.radiis_[-1] if directed else None


def test_the_same_random_state_gives_the_same_forecast(da):
    fit = Fit(np.random.RandomState(1), 12, 3, 30, 2, False)
    a = da.forecast(fit, horizon=2, keep_paths=True)
    b = da.forecast(fit, horizon=2, keep_paths=True)
    c = da.forecast(fit, horizon=2, keep_paths=True, random_state=8)
    assert a.sample_ids.tolist() == list(range(2, 12)) and a.paths.shape == (10, 2, 30, 2) and a.labels is None
    np.testing.assert_array_equal(a.paths, b.paths)
    np.testing.assert_array_equal(a.probas, b.probas)
    assert np.abs(a.paths - c.paths).min() > 0
    few = da.forecast(fit, horizon=1, n_samples=4)
    assert few.sample_ids.tolist() == [2, 5, 8, 11] and few.paths is None and few.probas.shape == (1, 30, 30)
    # the point estimate, tiled: the RNG index makes the trajectories differ
    point = da.forecast(fit, horizon=2, n_samples=6, estimate='map', keep_paths=True)
    assert point.sample_ids is None and point.paths.shape == (6, 2, 30, 2)
    assert np.abs(point.paths[0] - point.paths[1]).min() > 0
    step = point.paths[:, 0] - fit.X_[-1]
    assert abs(step.std() - np.sqrt(fit.sigma_sq)) < 0.2 * np.sqrt(fit.sigma_sq)
    assert 'horizon 2' in point.summary()


@pytest.mark.parametrize('directed', [False, True])
def test_score_against_a_direct_call_and_the_host_reference(da, directed):
    from test_gpu_scores import _check
    rng = np.random.RandomState(20 + directed)
    N, D, H, Hs = 33, 2, 3, 2
    fit = Fit(rng, 9, 2, N, D, directed)
    res = da.forecast(fit, horizon=H, keep_paths=True)
    S = len(res.sample_ids)
    Y = (rng.rand(Hs, N, N) < 0.3).astype(np.float64)
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.swapaxes(1, 2)
    idx = np.arange(N)
    Y[:, idx, idx] = 0
    hidden = rng.rand(Hs, N, N) < 0.1
    if not directed:
        hidden = np.triu(hidden, 1)
        hidden = hidden | hidden.swapaxes(1, 2)
    hidden[:, idx, idx] = False
    Yf = Y.copy()
    Yf[hidden] = -1
    got = res.score(Yf)
    Xs = np.ascontiguousarray(res.paths[:, :Hs])
    with da.Chain(Hs, N, D, 'directed' if directed else 'undirected') as c:
        counts, ll = c.score_accumulate(da.engine.pack_network(Y * ~hidden), Xs, res.intercepts, res.radii,
                                        mask=da.engine.pack_network(hidden))
    direct = da.scores.scores_from_counts(counts, ll, res.sample_ids, directed)
    assert got.counts == direct.counts and got.logloss_sum_t.tolist() == direct.logloss_sum_t.tolist()
    assert got.auc == direct.auc and got.log_loss == direct.log_loss and got.auc_t.shape == (Hs,)
    ref = score_ref.reference(Y * ~hidden, Xs, res.intercepts, res.radii, directed, hidden)
    assert score_cases.stable(ref)
    _check((counts, ll), ref, 'forecast score dir=%d' % directed)
    n_dyads = N * (N - 1) if directed else N * (N - 1) // 2
    assert got.n == Hs * n_dyads - int(hidden.sum()) // (1 if directed else 2) and S == 7
    # the whole horizon, nothing hidden
    full = res.score(np.concatenate([Y, Y[:1]]))
    assert full.n == H * n_dyads and full.auc_t.shape == (H,)


@pytest.mark.parametrize('kind', ['lsm', 'lsm-directed', 'lsm-case-control', 'hdp', 'lpcm'])
def test_end_to_end_on_a_short_fit(da, kind):
    from test_gpu_gof import _splitting
    T, N = 3, 18
    directed = kind in ('lsm-directed', 'lsm-case-control')
    Y = _splitting(N, T, directed, seed=3)
    if kind == 'hdp':
        m = da.DynamicNetworkHDPLPCM(n_iter=30, burn=10, tune=10, n_components=4, random_state=1).fit(Y)
    elif kind == 'lpcm':
        m = da.DynamicNetworkLPCM(n_iter=30, burn=10, tune=10, n_components=3, random_state=1).fit(Y)
    elif directed:
        m = da.DynamicNetworkLSM(n_iter=40, burn=10, tune=10, is_directed=True, random_state=5, tau_sq='auto',
                                 n_control=6 if kind == 'lsm-case-control' else None, sigma_sq=0.001,
                                 step_size_X=0.0075).fit(Y)
    else:
        m = da.DynamicNetworkLSM(n_iter=40, burn=10, tune=10, random_state=5).fit(Y)
    res = m.forecast(horizon=2)
    assert res.probas.shape == (2, N, N) and np.isfinite(res.probas).all()
    assert ((res.probas >= 0) & (res.probas <= 1)).all() and res.probas.max() > 0
    assert (res.probas[:, np.arange(N), np.arange(N)] == 0).all()
    assert res.is_directed == directed and len(res.sample_ids) == m.Xs_.shape[0] - res.sample_ids[0]
    if not directed:
        np.testing.assert_array_equal(res.probas, res.probas.swapaxes(1, 2))
    kept = m.forecast(horizon=2, n_samples=5, keep_paths=True)
    assert kept.paths.shape == (5, 2, N, 2) and (kept.labels is not None) == (kind in ('hdp', 'lpcm'))
    ref = fpr.mean_probas(kept.paths, kept.intercepts, kept.radii)
    np.testing.assert_allclose(kept.probas, ref, rtol=1e-12, atol=1e-15)
    point = m.forecast(horizon=1, n_samples=8, estimate='map')
    assert point.probas.shape == (1, N, N) and np.isfinite(point.probas).all()
    score = kept.score(Y[-2:])
    assert score.n == 2 * N * (N - 1) // (1 if directed else 2) and 0 <= score.auc <= 1
