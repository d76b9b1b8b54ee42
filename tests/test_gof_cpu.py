"""Posterior predictive goodness of fit (dynetlsm_amd/gof.py): the host arithmetic, without a device -
the numpy statistics helper against loops, the reference's edge and density definitions, the Monte
Carlo p-values and the summary, the bit order of the packed network and the argument checks."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gof_stats  # noqa: E402
from dynetlsm_amd import gof  # noqa: E402
from dynetlsm_amd.engine import pack_network, packed_row_words  # noqa: E402


def _random_network(rng, T, N, p, directed):
    Y = rng.rand(T, N, N) < p
    idx = np.arange(N)
    Y[:, idx, idx] = False
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y | Y.transpose(0, 2, 1)
    return Y


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('N,p', [(2, 0.9), (5, 0.5), (11, 0.3), (17, 0.6)])
def test_helper_matches_loops(directed, N, p):
    rng = np.random.RandomState(N)
    Y = _random_network(rng, 3, N, p, directed)
    np.testing.assert_array_equal(gof_stats.records(Y, directed), gof_stats.records_loops(Y, directed))


def _num_edges(Y, is_directed):           # network_statistics.py:13-14
    return np.sum(Y) if is_directed else 0.5 * np.sum(Y)


def _density(Y, is_directed):             # network_statistics.py:17-28 (dynamic Y)
    n = Y.shape[1]
    n_possible = n * (n - 1) * Y.shape[0]
    if not is_directed:
        n_possible *= 0.5
    return _num_edges(Y, is_directed) / n_possible


@pytest.mark.parametrize('directed', [False, True])
def test_edges_and_density_follow_the_reference_definitions(directed):
    rng = np.random.RandomState(3)
    Y = _random_network(rng, 4, 13, 0.35, directed).astype(np.float64)
    st = gof.derive_statistics(gof_stats.records(Y, directed), 13, directed)
    for t in range(4):
        assert st['edges'][t] == _num_edges(Y[t], directed)
        assert st['density'][t] == pytest.approx(_density(Y[t:t + 1], directed), rel=1e-15)
    assert st['density'].mean() == pytest.approx(_density(Y, directed), rel=1e-14)
    assert ('mutual' in st) == directed and ('transitivity' in st) == (not directed)


def test_triangles_and_transitivity_from_esp_and_degrees():
    # a triangle 0-1-2 with a pendant edge 2-3 and an isolated node 4
    A = np.zeros((1, 5, 5))
    for i, j in ((0, 1), (1, 2), (0, 2), (2, 3)):
        A[0, i, j] = A[0, j, i] = 1
    st = gof.derive_statistics(gof_stats.records(A, False), 5, False)
    assert st['edges'][0] == 4 and st['triangles'][0] == 1
    np.testing.assert_array_equal(st['degree'][0], [1, 1, 2, 1, 0])      # degrees 2, 2, 3, 1, 0
    np.testing.assert_array_equal(st['esp'][0], [1, 3, 0, 0, 0])
    # 3 closed of 1 + 1 + 3 connected triples
    assert st['transitivity'][0] == pytest.approx(3.0 / 5.0)
    empty = gof.derive_statistics(gof_stats.records(np.zeros((2, 4, 4)), False), 4, False)
    np.testing.assert_array_equal(empty['transitivity'], [0.0, 0.0])


def test_directed_records_on_a_hand_made_network():
    # 0 -> 1, 1 -> 0, 1 -> 2, 0 -> 2: one mutual pair; arcs 0 -> 2 (0 -> 1 -> 2) and 1 -> 2
    # (1 -> 0 -> 2) have one transitive partner, 0 -> 1 and 1 -> 0 none
    A = np.zeros((1, 3, 3))
    for i, j in ((0, 1), (1, 0), (1, 2), (0, 2)):
        A[0, i, j] = 1
    st = gof.derive_statistics(gof_stats.records(A, True), 3, True)
    assert st['edges'][0] == 4 and st['mutual'][0] == 1
    np.testing.assert_array_equal(st['out_degree'][0], [1, 0, 2])     # out-degrees 2, 2, 0
    np.testing.assert_array_equal(st['in_degree'][0], [0, 2, 1])      # in-degrees 1, 1, 2
    np.testing.assert_array_equal(st['esp'][0], [2, 2, 0])
    assert st['density'][0] == pytest.approx(4 / 6)


def test_p_values_on_hand_made_arrays():
    sim = np.array([[0, 5], [1, 5], [2, 5], [3, 6]], dtype=np.int64)
    obs = np.array([0, 5])
    # bin 0: P(sim >= 0) = 1, P(sim <= 0) = 1/4 -> 1/2; bin 1: P(>= 5) = 1, P(<= 5) = 3/4 -> 1
    np.testing.assert_allclose(gof.mc_p_values(sim, obs), [0.5, 1.0])
    np.testing.assert_allclose(gof.mc_p_values(sim, [9, 4]), [0.0, 0.0])
    # P(sim >= 2) = 8/10, P(sim <= 2) = 3/10
    np.testing.assert_allclose(gof.mc_p_values(np.arange(10.0)[:, None], [2.0]), [0.6])


def test_result_pooling_and_summary_on_hand_made_records():
    N, T, S = 4, 2, 5
    rng = np.random.RandomState(1)
    obs_Y = _random_network(rng, T, N, 0.5, False)
    sims = np.stack([gof_stats.records(_random_network(rng, T, N, 0.5, False), False) for _ in range(S)])
    res = gof.GofResult(np.arange(S), gof.derive_statistics(gof_stats.records(obs_Y, False), N, False),
                        gof.derive_statistics(sims, N, False), False, N)
    assert res.simulated['esp'].shape == (S, T, N) and res.observed['degree'].shape == (T, N)
    assert res.p_values['edges'].shape == (T,) and res.p_values['degree'].shape == (T, N)
    obs, sim = res.pooled()
    assert obs['edges'] == res.observed['edges'].sum()
    np.testing.assert_array_equal(sim['degree'], res.simulated['degree'].sum(axis=1))
    assert obs['density'] == pytest.approx(_density(obs_Y.astype(float), False))
    text = res.summary()
    lines = text.splitlines()
    assert lines[0].split()[:2] == ['statistic', 'observed']
    row = [l for l in lines if l.split()[0] == 'edges'][0].split()
    q = np.percentile(sim['edges'], [2.5, 50, 97.5])
    assert float(row[1]) == obs['edges']
    np.testing.assert_allclose([float(v) for v in row[2:5]], q, rtol=1e-5)
    assert float(row[5]) == pytest.approx(gof.mc_p_values(sim['edges'], obs['edges']), abs=1e-3)
    assert any(l.startswith('degree[0]') for l in lines) and any(l.startswith('esp[0]') for l in lines)
    assert 'transitivity' in text and 'mutual' not in text


@pytest.mark.parametrize('N', [2, 7, 31, 32, 33, 64, 65, 130])
def test_packed_network_bit_order(N):
    rng = np.random.RandomState(N)
    Y = rng.rand(2, N, N) < 0.5
    B = pack_network(Y)
    W = packed_row_words(N)
    assert B.dtype == np.uint32 and B.shape == (2, N, W) and W % 4 == 0 and 32 * W >= N
    for t, i, j in zip(rng.randint(0, 2, 50), rng.randint(0, N, 50), rng.randint(0, N, 50)):
        assert bool((int(B[t, i, j // 32]) >> (j % 32)) & 1) == Y[t, i, j]
    # padding bits are zero
    for w in range(W):
        lo = 32 * w
        if lo + 32 > N:
            keep = 0 if lo >= N else (1 << (N - lo)) - 1
            assert not (B[..., w] & np.uint32(~keep & 0xFFFFFFFF)).any()
    np.testing.assert_array_equal(gof_stats.unpack(B, N), Y)


class _Unfit(object):
    random_state = 0


class _Fitted(object):
    """the attributes posterior_predictive_check reads before any device call"""
    is_directed = False
    random_state = 0
    n_burn_ = 6

    def __init__(self):
        self.Y_fit_ = np.zeros((2, 5, 5))
        self.Xs_ = np.zeros((10, 2, 5, 2))
        self.intercepts_ = np.zeros((10, 1))


def test_value_errors_before_any_device_call():
    import dynetlsm_amd as da
    with pytest.raises(ValueError, match='not fit'):
        da.posterior_predictive_check(_Unfit())
    with pytest.raises(ValueError, match='not fit'):
        da.posterior_predictive_check(da.DynamicNetworkLSM())
    with pytest.raises(ValueError, match='not fit'):
        da.posterior_predictive_check(da.DynamicNetworkHDPLPCM())
    with pytest.raises(ValueError, match='n_samples'):
        da.posterior_predictive_check(_Fitted(), n_samples=0)
    with pytest.raises(ValueError, match='n_samples'):
        da.posterior_predictive_check(_Fitted(), n_samples=2.5)
    # rows 6..9 are kept: four samples at most
    with pytest.raises(ValueError, match='exceeds the 4 kept'):
        da.posterior_predictive_check(_Fitted(), n_samples=5)
