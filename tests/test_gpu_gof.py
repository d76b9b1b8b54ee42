"""Posterior predictive goodness of fit on the device (csrc/kernels_gof.hpp, dynetlsm_amd/gof.py):
every drawn bit regenerated on the host from the Philox counters and numpy probabilities, the integer
statistics records against numpy, invariance to how the samples are split, the law of the draws and
the check end to end on fitted models.  Needs an MI355X: -m gpu."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gof_stats  # noqa: E402
from conftest import load_golden  # noqa: E402
from dynetlsm_amd.gof import mc_p_values  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _params(rng, S, T, N, D, directed):
    Xs = rng.randn(S, T, N, D) * (1.5 / np.sqrt(D))
    ic = np.stack([rng.uniform(-0.5, 1.5, S), rng.uniform(-0.5, 1.5, S)], axis=1)
    radii = rng.uniform(0.5, 2.0, (S, N)) if directed else None
    return Xs, ic, radii


def _c_philox_agrees(seed, counters):
    """the numpy Philox of the oracle module against orc_philox4x32 of liboracle.so on a few counters"""
    from oracle import oracle as orc
    L = orc.lib()
    for c in counters:
        out = (C.c_uint32 * 4)()
        L.orc_philox4x32(seed, *[int(v) for v in c], C.byref(out))
        want = [int(np.asarray(v).ravel()[0]) for v in orc.philox4x32(seed, *c)]
        assert list(out) == want, (c, list(out), want)


CASES = [(1, 2, 1, False), (3, 2, 2, True), (3, 7, 5, False), (1, 7, 8, True), (3, 33, 2, False),
         (3, 33, 1, True), (1, 64, 8, False), (3, 64, 5, True), (3, 65, 2, False), (1, 65, 8, True),
         (3, 200, 5, False), (3, 200, 2, True), (1, 2000, 2, False), (1, 2000, 8, True)]


@pytest.mark.parametrize('T,N,D,directed', CASES)
def test_draws_and_statistics_are_exact(da, T, N, D, directed):
    from oracle import oracle as orc
    rng = np.random.RandomState(N * 16 + D + 8 * directed)
    S, seed, first = 2, 0x1234ABCD5678 + N, 7
    Xs, ic, radii = _params(rng, S, T, N, D, directed)
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        stats, bits = c.gof_simulate(Xs, ic, radii, seed=seed, first_index=first, want_bits=True)
    assert stats.shape == (S, T, 2 + 3 * N) and bits.shape == (S, T, N, gof_stats.row_words(N))
    _c_philox_agrees(seed, [(0, 1, first, 7), (N - 2, N - 1, first + 1, ((T - 1) << 8) | 7)])
    Y = gof_stats.unpack(bits, N)
    n_close = 0
    for s in range(S):
        P = gof_stats.probabilities(Xs[s], ic[s], radii[s] if directed else None, directed)
        U = gof_stats.uniforms(orc.philox4x32, seed, first + s, T, N, directed)
        want = U < P
        sure = np.abs(U - P) >= 1e-12
        n_close += int((~sure).sum())
        assert np.array_equal(Y[s][sure], want[sure]), (s, int((Y[s] != want)[sure].sum()))
        np.testing.assert_array_equal(stats[s], gof_stats.records(Y[s], directed))
    assert n_close <= 2
    idx = np.arange(N)
    assert not Y[..., idx, idx].any()
    if not directed:
        assert np.array_equal(Y, Y.swapaxes(-1, -2))
    # padding bits of the rows are zero
    assert not gof_stats.unpack(bits, 32 * bits.shape[-1])[..., N:].any()


@pytest.mark.parametrize('directed', [False, True])
def test_observed_statistics_on_the_monks(da, directed):
    Y = load_golden('monks.npz')['Y_directed' if directed else 'Y_undirected']
    T, N = Y.shape[:2]
    with da.Chain(T, N, 2, 'directed' if directed else 'undirected') as c:
        got = c.gof_observed(da.engine.pack_network(Y))
    np.testing.assert_array_equal(got, gof_stats.records(Y, directed))


def test_observed_statistics_at_full_size(da):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    Y = synthetic_lsm_network(T=10, N=2000, density=0.03, seed=3)['Y']
    with da.Chain(10, 2000, 2, 'undirected') as c:
        got = c.gof_observed(da.engine.pack_network(Y))
    np.testing.assert_array_equal(got, gof_stats.records(Y, False))
    Yd = synthetic_lsm_network(T=2, N=2000, density=0.03, seed=4, directed=True)['Y']
    with da.Chain(2, 2000, 2, 'case_control') as c:
        got = c.gof_observed(da.engine.pack_network(Yd))
    np.testing.assert_array_equal(got, gof_stats.records(Yd, True))


def test_bad_arguments_are_rejected(da):
    rng = np.random.RandomState(0)
    Xs, ic, radii = _params(rng, 2, 2, 9, 2, True)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.gof_simulate(Xs, ic, None)
        with pytest.raises(da.EngineError) as e:
            c.gof_simulate(Xs, ic, radii, first_index=2 ** 32 - 1)
        assert e.value.code == -1
        with pytest.raises(da.EngineError) as e:
            c.gof_simulate(Xs, ic, radii, batch=-1)
        assert e.value.code == -1
        Y = np.zeros((2, 9, 9)); Y[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.gof_observed(da.engine.pack_network(Y))
        assert e.value.code == -4


@pytest.mark.parametrize('directed', [False, True])
def test_results_do_not_depend_on_the_split(da, directed):
    rng = np.random.RandomState(5)
    T, N, D = 3, 65, 2
    Xs, ic, radii = _params(rng, 64, T, N, D, directed)
    r = (lambda a, b: None) if radii is None else (lambda a, b: radii[a:b])
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        whole, bw = c.gof_simulate(Xs, ic, radii, seed=11, want_bits=True)
        a, ba = c.gof_simulate(Xs[:32], ic[:32], r(0, 32), seed=11, first_index=0, want_bits=True)
        b, bb = c.gof_simulate(Xs[32:], ic[32:], r(32, 64), seed=11, first_index=32, want_bits=True)
        small = c.gof_simulate(Xs, ic, radii, seed=11, batch=5)
        other = c.gof_simulate(Xs, ic, radii, seed=12)
    np.testing.assert_array_equal(whole, np.concatenate([a, b]))
    np.testing.assert_array_equal(bw, np.concatenate([ba, bb]))
    np.testing.assert_array_equal(whole, small)
    assert not np.array_equal(whole, other)


def test_draws_follow_the_model(da):
    rng = np.random.RandomState(9)
    S, N, D = 2000, 200, 2
    X, ic, radii = _params(rng, 1, 1, N, D, True)
    for directed in (False, True):
        with da.Chain(1, N, D, 'directed' if directed else 'undirected') as c:
            st = c.gof_simulate(np.broadcast_to(X, (S, 1, N, D)), np.repeat(ic, S, axis=0),
                                np.repeat(radii, S, axis=0) if directed else None, seed=21)[:, 0]
        P = gof_stats.probabilities(X[0], ic[0], radii[0], directed)[0]
        if directed:
            pe = P[~np.eye(N, dtype=bool)]
            q = (P * P.T)[np.triu_indices(N, 1)]
            mean_m, se_m = q.sum(), np.sqrt((q * (1 - q)).sum() / S)
            assert abs(st[:, 1].mean() - mean_m) < 5 * se_m, (st[:, 1].mean(), mean_m, se_m)
        else:
            pe = P[np.triu_indices(N, 1)]
            assert (st[:, 1] == 0).all()
        mean_e, se_e = pe.sum(), np.sqrt((pe * (1 - pe)).sum() / S)
        assert abs(st[:, 0].mean() - mean_e) < 5 * se_e, (st[:, 0].mean(), mean_e, se_e)


def _pooled_p(res, name):
    obs, sim = res.pooled()
    return mc_p_values(sim[name], obs[name]), obs[name], sim[name]


def test_check_of_a_well_specified_fit(da):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    Y = synthetic_lsm_network(T=3, N=100, density=0.1, seed=1)['Y']
    m = da.DynamicNetworkLSM(n_iter=300, burn=150, tune=150, random_state=2).fit(Y)
    res = da.posterior_predictive_check(m, n_samples=100)
    assert len(res.sample_ids) == 100 and res.sample_ids.min() >= m.n_burn_
    assert res.sample_ids.max() == m.Xs_.shape[0] - 1 and len(np.unique(res.sample_ids)) == 100
    assert res.observed['degree'].shape == (3, 100) and res.simulated['esp'].shape == (100, 3, 100)
    for name in ('edges', 'density', 'triangles', 'transitivity'):
        assert res.simulated[name].shape == (100, 3) and np.isfinite(res.simulated[name]).all()
    p, _, _ = _pooled_p(res, 'edges')
    assert p > 0.05, p
    pd, obs, sim = _pooled_p(res, 'degree')
    lo, hi = np.percentile(sim, [2.5, 97.5], axis=0)
    seen = obs > 0
    assert ((obs >= lo) & (obs <= hi))[seen].mean() >= 0.7
    again = da.posterior_predictive_check(m, n_samples=100)
    np.testing.assert_array_equal(again.simulated['esp'], res.simulated['esp'])
    assert 'edges' in res.summary()


def test_check_sees_planted_hubs(da):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N = 2, 100
    Y = synthetic_lsm_network(T=T, N=N, density=0.05, seed=4)['Y']
    rng = np.random.RandomState(4)
    hubs = np.arange(5)
    for t in range(T):
        for h in hubs:
            nb = rng.rand(N) < 0.9
            nb[h] = False
            Y[t, h, nb] = Y[t, nb, h] = 1.0
    m = da.DynamicNetworkLSM(n_iter=300, burn=150, tune=150, random_state=3).fit(Y)
    res = da.posterior_predictive_check(m, n_samples=100)
    obs, sim = res.pooled()
    k0 = int(0.8 * N)
    tail_obs = obs['degree'][k0:].sum()
    tail_sim = sim['degree'][:, k0:].sum(axis=1)
    assert tail_obs >= T * len(hubs) - 2
    assert mc_p_values(tail_sim, tail_obs) < 0.05, (tail_obs, np.percentile(tail_sim, [50, 97.5]))
    assert (res.p_values['degree'][:, k0:][:, obs['degree'][k0:] > 0] < 0.1).any()


def _splitting(n_nodes, T, directed, seed=0):
    rng = np.random.RandomState(seed)
    Y = np.zeros((T, n_nodes, n_nodes))
    X = rng.randn(T, n_nodes, 2)
    for t in range(T):
        d = np.sqrt(((X[t][:, None] - X[t][None]) ** 2).sum(-1))
        A = (rng.rand(n_nodes, n_nodes) < 1 / (1 + np.exp(-(1.0 - d)))).astype(float)
        np.fill_diagonal(A, 0)
        if not directed:
            A = np.triu(A, 1); A = A + A.T
        Y[t] = A
    return Y


def _check_shapes(res, S, T, N, directed):
    for name in (('out_degree', 'in_degree', 'esp') if directed else ('degree', 'esp')):
        assert res.observed[name].shape == (T, N) and res.simulated[name].shape == (S, T, N)
    names = ('edges', 'density') + (('mutual',) if directed else ('triangles', 'transitivity'))
    for name in names:
        assert res.observed[name].shape == (T,) and res.simulated[name].shape == (S, T)
    for name, p in res.p_values.items():
        assert np.isfinite(p).all() and ((p >= 0) & (p <= 1)).all(), name
    assert ('mutual' in res.simulated) == directed and ('degree' in res.simulated) != directed
    if directed:
        assert (res.simulated['out_degree'].sum(-1) == N).all()
        assert (res.simulated['in_degree'].sum(-1) == N).all()
    else:
        assert (res.simulated['degree'].sum(-1) == N).all()
    assert (res.simulated['esp'].sum(-1) == res.simulated['edges']).all()


def test_check_runs_on_every_model(da):
    Yd = _splitting(30, 2, True, seed=1)
    Yu = _splitting(30, 2, False, seed=2)
    hdp = da.DynamicNetworkHDPLPCM(n_iter=30, burn=10, tune=10, n_components=4, random_state=1).fit(Yu)
    res = da.posterior_predictive_check(hdp, n_samples=10)
    _check_shapes(res, 10, 2, 30, False)
    hdp.release_device_trace()                        # the check then makes a chain of its own
    res2 = da.posterior_predictive_check(hdp, n_samples=10)
    np.testing.assert_array_equal(res2.simulated['esp'], res.simulated['esp'])
    hdpd = da.DynamicNetworkHDPLPCM(n_iter=30, burn=10, tune=10, n_components=4, is_directed=True,
                                    random_state=1).fit(Yd)
    _check_shapes(da.posterior_predictive_check(hdpd, n_samples=10), 10, 2, 30, True)
    lpcm = da.DynamicNetworkLPCM(n_iter=30, burn=10, tune=10, n_components=3, random_state=1).fit(Yu)
    _check_shapes(da.posterior_predictive_check(lpcm, n_samples=10), 10, 2, 30, False)
    for n_control in (None, 10):
        lsm = da.DynamicNetworkLSM(n_iter=40, burn=10, tune=10, is_directed=True, n_control=n_control,
                                   random_state=5, tau_sq='auto', sigma_sq=0.001,
                                   step_size_X=0.0075).fit(Yd)
        res = da.posterior_predictive_check(lsm, n_samples=20, random_state=3)
        _check_shapes(res, 20, 2, 30, True)
