"""Goodness of fit over time on the device (csrc/kernels_gof_dynamic.hpp, dynetlsm_amd/gof.py): the
overlap, step and geodesic records of drawn and of observed networks against the numpy replica
(tests/gof_dynamic_ref.py) - every comparison is integer equality -, the drawn bits against those of
gof_simulate, invariance to batching and splitting, the law of the persistence and the check end to end
on fitted models.  Needs an MI355X: -m gpu."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gof_dynamic_ref as ref  # noqa: E402
import gof_stats  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_gof import _params  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, FIRST, S = 0x5EED0F7135, 3, 2


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _mode(directed):
    return 'directed' if directed else 'undirected'


def _sparse_params(rng, S, T, N, D, directed, degree=2.0):
    """positions as the dense level's; the intercepts (directed: with one scale of the radii) that give an
    expected mean degree (directed: out-degree) of `degree`, by bisection on the exact probabilities"""
    Xs, ic, radii = _params(rng, S, T, N, D, directed)
    ic = np.array(ic)
    for s in range(S):
        def expected_degree(v):
            if directed:
                P = gof_stats.probabilities(Xs[s], (6.0, 6.0), radii[s] * v, True)
            else:
                P = gof_stats.probabilities(Xs[s], (v, 0.0), None, False)
            return P.sum() / (T * N)
        lo, hi = (1e-3, 10.0) if directed else (-40.0, 10.0)
        with np.errstate(over='ignore'):            # exp(-eta) of a dyad that is never drawn
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if expected_degree(mid) < degree else (lo, mid)
        if directed:
            ic[s] = (6.0, 6.0)
            radii[s] = radii[s] * hi
        else:
            ic[s] = (hi, 0.0)
    return Xs, ic, radii


CASES = [(1, 2, 1, False), (3, 2, 2, True), (3, 7, 5, False), (3, 33, 2, False), (3, 33, 1, True),
         (2, 64, 2, True), (3, 65, 2, False), (2, 129, 2, True), (2, 200, 2, False), (2, 200, 2, True)]


def case_params(T, N, D, directed, level):
    rng = np.random.RandomState(N * 16 + D + 8 * directed + 1000 * (level == 'sparse'))
    make = _sparse_params if level == 'sparse' else _params
    return make(rng, S, T, N, D, directed)


def host_draws(Xs, ic, radii, T, N, directed):
    """the networks the device draws at (SEED, FIRST): a pure function of the Philox counters"""
    from oracle import oracle as orc
    Y = np.zeros((S, T, N, N), dtype=bool)
    for s in range(S):
        with np.errstate(over='ignore'):            # exp(-eta) of a dyad that is never drawn
            P = gof_stats.probabilities(Xs[s], ic[s], radii[s] if directed else None, directed)
        Y[s] = gof_stats.uniforms(orc.philox4x32, SEED, FIRST + s, T, N, directed) < P
    return Y


def _assert_records(got, Y, directed, temporal=True, geodesic=True):
    ov, st, geo = got
    want = ref.records(Y, directed)
    if temporal:
        np.testing.assert_array_equal(ov, want[0])
        np.testing.assert_array_equal(st, want[1])
    else:
        assert ov is None and st is None
    if geodesic:
        np.testing.assert_array_equal(geo, want[2])
    else:
        assert geo is None
    return want


@pytest.mark.parametrize('level', ['dense', 'sparse'])
@pytest.mark.parametrize('T,N,D,directed', CASES)
def test_records_of_drawn_networks_are_exact(da, T, N, D, directed, level):
    Xs, ic, radii = case_params(T, N, D, directed, level)
    temporal = (T, N) != (1, 2)                 # the one-step case asks for the geodesic family alone
    with da.Chain(T, N, D, _mode(directed)) as c:
        ov, st, geo, bits = c.gof_dynamic_simulate(Xs, ic, radii, seed=SEED, first_index=FIRST,
                                                   temporal=temporal, want_bits=True)
    assert bits.shape == (S, T, N, gof_stats.row_words(N)) and geo.shape == (S, T, N)
    if temporal:
        assert ov.shape == (S, T, T) and st.shape == (S, T - 1, 2 * N)
    Y = gof_stats.unpack(bits, N)
    longest, unreachable = 0, 0
    for s in range(S):
        want = _assert_records((ov[s], st[s], geo[s]) if temporal else (None, None, geo[s]), Y[s], directed,
                               temporal=temporal)
        unreachable += int(want[2][:, 0].sum())
        longest = max(longest, int(np.nonzero(want[2].sum(0))[0].max()) if want[2].sum() else 0)
    if level == 'sparse' and N >= 33:
        # otherwise the search is not exercised beyond its first levels
        assert unreachable >= 1 and longest >= 4, (unreachable, longest)
        # ... and the host draws of the same counters said so before any device was asked
        host = ref.geodesic(host_draws(Xs, ic, radii, T, N, directed).reshape(S * T, N, N), directed)
        assert host[:, 0].sum() >= 1 and np.nonzero(host.sum(0))[0].max() >= 4


@pytest.mark.parametrize('T,N,D,directed', [(3, 65, 2, False), (2, 129, 2, True)])
def test_draws_are_those_of_gof_simulate(da, T, N, D, directed):
    Xs, ic, radii = case_params(T, N, D, directed, 'dense')
    with da.Chain(T, N, D, _mode(directed)) as c:
        stats, bits0 = c.gof_simulate(Xs, ic, radii, seed=SEED, first_index=FIRST, want_bits=True)
        ov, st, geo, bits = c.gof_dynamic_simulate(Xs, ic, radii, seed=SEED, first_index=FIRST, want_bits=True)
    np.testing.assert_array_equal(bits, bits0)
    idx = np.arange(T)
    np.testing.assert_array_equal(ov[:, idx, idx], stats[..., 0])
    np.testing.assert_array_equal(geo[..., 1], stats[..., 0])


@pytest.mark.parametrize('directed', [False, True])
def test_observed_records_on_the_monks(da, directed):
    Y = load_golden('monks.npz')['Y_directed' if directed else 'Y_undirected']
    T, N = Y.shape[:2]
    with da.Chain(T, N, 2, _mode(directed)) as c:
        got = c.gof_dynamic_observed(da.engine.pack_network(Y))
    _assert_records(got, Y, directed)


def test_observed_records_of_an_empty_and_a_complete_network(da):
    for directed in (False, True):
        N = 65
        Y = np.zeros((2, N, N))
        Y[1] = 1 - np.eye(N)
        with da.Chain(2, N, 2, _mode(directed)) as c:
            ov, st, geo = c.gof_dynamic_observed(da.engine.pack_network(Y))
        pairs = N * (N - 1) if directed else N * (N - 1) // 2
        np.testing.assert_array_equal(ov, [[0, 0], [0, pairs]])
        np.testing.assert_array_equal(geo[0], [pairs] + [0] * (N - 1))
        np.testing.assert_array_equal(geo[1], [0, pairs] + [0] * (N - 2))
        # no tie persists; every dyad forms with no partner at the empty step
        np.testing.assert_array_equal(st[0, :N], [N] + [0] * (N - 1))
        np.testing.assert_array_equal(st[0, N:], [pairs] + [0] * (N - 1))
        _assert_records((ov, st, geo), Y, directed)


def test_observed_records_of_a_directed_cycle(da):
    N = 130
    Y = np.zeros((2, N, N))
    Y[0, np.arange(N), (np.arange(N) + 1) % N] = 1
    Y[1, np.arange(N), (np.arange(N) - 1) % N] = 1           # the same cycle the other way round
    with da.Chain(2, N, 2, 'directed') as c:
        ov, st, geo = c.gof_dynamic_observed(da.engine.pack_network(Y))
    np.testing.assert_array_equal(geo, np.tile([0] + [N] * (N - 1), (2, 1)))
    np.testing.assert_array_equal(ov, [[N, 0], [0, N]])
    _assert_records((ov, st, geo), Y, True)


def test_observed_records_of_a_long_path(da):
    """distances up to 2099: the bins above the LDS histogram go to the record by global atomics"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    N = 2100
    Y = np.zeros((2, N, N), dtype=bool)
    i = np.arange(N - 1)
    Y[:, i, i + 1] = True
    Y[1, N - 2, N - 1] = False                  # the last edge moves: node N-1 hangs on node 1
    Y[1, 1, N - 1] = True
    Y = Y | Y.swapaxes(1, 2)
    with da.Chain(2, N, 2, 'undirected') as c:
        ov, st, geo = c.gof_dynamic_observed(da.engine.pack_network(Y))
    up = np.triu_indices(N, 1)
    for t in range(2):
        d = shortest_path(csr_matrix(Y[t].astype(np.float64)), directed=False, unweighted=True)
        np.testing.assert_array_equal(geo[t], np.bincount(d[up].astype(np.int64), minlength=N)[:N])
    np.testing.assert_array_equal(geo[0], [0] + [N - k for k in range(1, N)])
    # after the move the longest paths end in node N-2 and start in node 0 or node N-1: length N-2
    assert geo[0, N - 1] == 1 and geo[1, N - 1] == 0 and geo[1, N - 2] == 2
    np.testing.assert_array_equal(ov, [[N - 1, N - 2], [N - 2, N - 1]])
    np.testing.assert_array_equal(st, ref.steps(Y, False))
    assert st[0, N:].sum() == 1 and st[0, N] == 1           # the moved edge closes no triangle


def test_observed_records_at_full_size(da):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    Y = synthetic_lsm_network(T=10, N=2000, density=0.03, seed=3)['Y']
    with da.Chain(10, 2000, 2, 'undirected') as c:
        got = c.gof_dynamic_observed(da.engine.pack_network(Y))
    _assert_records(got, Y, False)


@pytest.mark.parametrize('directed', [False, True])
def test_results_do_not_depend_on_batch_or_split(da, directed):
    T, N, D = 3, 65, 2
    rng = np.random.RandomState(5)
    Xs, ic, radii = _sparse_params(rng, 4, T, N, D, directed, degree=3.0)
    r = (lambda a, b: None) if radii is None else (lambda a, b: radii[a:b])
    with da.Chain(T, N, D, _mode(directed)) as c:
        whole = c.gof_dynamic_simulate(Xs, ic, radii, seed=11, want_bits=True)
        one = c.gof_dynamic_simulate(Xs, ic, radii, seed=11, batch=1, want_bits=True)
        a = c.gof_dynamic_simulate(Xs[:2], ic[:2], r(0, 2), seed=11, first_index=0, want_bits=True)
        b = c.gof_dynamic_simulate(Xs[2:], ic[2:], r(2, 4), seed=11, first_index=2, want_bits=True)
        other = c.gof_dynamic_simulate(Xs, ic, radii, seed=12)
    for k in range(4):
        np.testing.assert_array_equal(whole[k], one[k])
        np.testing.assert_array_equal(whole[k], np.concatenate([a[k], b[k]]))
    assert not np.array_equal(whole[0], other[0])


def test_persistence_follows_the_model(da):
    rng = np.random.RandomState(9)
    n_draws, T, N, D = 200, 3, 33, 2
    for directed in (False, True):
        X, ic, radii = _params(rng, 1, T, N, D, directed)
        with da.Chain(T, N, D, _mode(directed)) as c:
            ov, _, _ = c.gof_dynamic_simulate(np.broadcast_to(X, (n_draws, T, N, D)), np.repeat(ic, n_draws, axis=0),
                                              np.repeat(radii, n_draws, axis=0) if directed else None, seed=21,
                                              geodesic=False)
        P = gof_stats.probabilities(X[0], ic[0], radii[0] if directed else None, directed)
        dy = ~np.eye(N, dtype=bool) if directed else np.triu(np.ones((N, N), dtype=bool), 1)
        for t in range(T - 1):
            q = (P[t] * P[t + 1])[dy]
            mean, se = q.sum(), np.sqrt((q * (1 - q)).sum() / n_draws)
            got = ov[:, t, t + 1].mean()
            assert abs(got - mean) < 5 * se, (directed, t, got, mean, se)


def test_bad_arguments_are_rejected(da):
    rng = np.random.RandomState(0)
    Xs, ic, radii = _params(rng, 2, 2, 9, 2, True)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.gof_dynamic_simulate(Xs, ic, None)
        with pytest.raises(ValueError):
            c.gof_dynamic_simulate(Xs, ic, radii, temporal=False, geodesic=False)
        # both outputs NULL at the C boundary
        with pytest.raises(da.EngineError) as e:
            c._ck(c._L.dlsm_gof_dynamic_simulate(c._h, da.engine._p(Xs), da.engine._p(ic), da.engine._p(radii), 2,
                                                 0, 0, 0, None, None, None, None))
        assert e.value.code == -1
        bits = da.engine.pack_network(np.zeros((2, 9, 9)))
        with pytest.raises(da.EngineError) as e:
            c._ck(c._L.dlsm_gof_dynamic_observed(c._h, bits.ctypes.data_as(da._lib.c_u32_p), None, None, None))
        assert e.value.code == -1
        with pytest.raises(da.EngineError) as e:
            c.gof_dynamic_simulate(Xs, ic, radii, batch=-1)
        assert e.value.code == -1
        with pytest.raises(da.EngineError) as e:
            c.gof_dynamic_simulate(Xs, ic, radii, first_index=2 ** 32 - 1)
        assert e.value.code == -1
        Y = np.zeros((2, 9, 9)); Y[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.gof_dynamic_observed(da.engine.pack_network(Y))
        assert e.value.code == -4


@pytest.mark.parametrize('directed', [False, True])
def test_check_end_to_end_on_the_monks(da, directed):
    Y = load_golden('monks.npz')['Y_directed' if directed else 'Y_undirected']
    T, N = Y.shape[:2]
    S_ = 20
    m = da.DynamicNetworkLSM(n_iter=300, burn=100, tune=100, is_directed=directed, random_state=4).fit(Y)
    res = da.posterior_predictive_check(m, S_, statistics='all', random_state=6)
    base = da.posterior_predictive_check(m, S_, random_state=6)
    assert set(base.simulated) < set(res.simulated)
    for name in base.simulated:
        np.testing.assert_array_equal(res.simulated[name], base.simulated[name])
        np.testing.assert_array_equal(res.observed[name], base.observed[name])
        np.testing.assert_array_equal(res.p_values[name], base.p_values[name])
    shapes = {'overlap': (T, T), 'persisted': (T - 1,), 'formed': (T - 1,), 'dissolved': (T - 1,),
              'persistence': (T - 1,), 'stability': (T - 1,), 'persist_degree': (T - 1, N),
              'formed_sp': (T - 1, N), 'geodesic': (T, N), 'unreachable': (T,), 'mean_geodesic': (T,),
              'diameter': (T,)}
    for name, shp in shapes.items():
        assert res.observed[name].shape == shp and res.simulated[name].shape == (S_,) + shp, name
    for name, p in res.p_values.items():
        assert np.isfinite(p).all() and ((p >= 0) & (p <= 1)).all(), name
    # all families describe the same drawn networks
    idx = np.arange(T)
    np.testing.assert_array_equal(res.simulated['overlap'][:, idx, idx], res.simulated['edges'])
    np.testing.assert_array_equal(res.simulated['geodesic'][..., 1], res.simulated['edges'])
    np.testing.assert_array_equal(res.observed['geodesic'][..., 1], res.observed['edges'])
    one = da.posterior_predictive_check(m, S_, statistics=('temporal',), random_state=6)
    np.testing.assert_array_equal(one.simulated['formed_sp'], res.simulated['formed_sp'])
    assert 'edges' not in one.simulated and 'geodesic' not in one.simulated
    labels = [line.split()[0] for line in res.summary().splitlines()]
    assert 'persistence' in labels and 'geodesic[1]' in labels and 'unreachable' in labels
    assert base.summary() == '\n'.join(res.summary().splitlines()[:len(base.summary().splitlines())])
