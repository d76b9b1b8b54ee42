"""``SparseNetwork`` on the host (dynetlsm_amd/sparse.py): round trips against the dense tensor, the checks that
answer before any device call, and the radii of the init pipeline from degree counts.  No GPU needed."""
import pickle

import numpy as np
import pytest

import dynetlsm_amd as da
from dynetlsm_amd import initialization as init_mod
from dynetlsm_amd.sparse import SparseNetwork


def _dense(rng, T, N, directed, density=0.2):
    Y = (rng.rand(T, N, N) < density).astype(np.float64)
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.swapaxes(1, 2)
    idx = np.arange(N)
    Y[:, idx, idx] = 0.0
    return Y


def _triples(Y):
    return np.stack(np.nonzero(Y), axis=1)


def test_round_trips():
    rng = np.random.RandomState(0)
    for directed in (True, False):
        Y = _dense(rng, 3, 17, directed)
        net = SparseNetwork.from_dense(Y)
        np.testing.assert_array_equal(net.to_dense(), Y)
        assert net.to_dense().dtype == np.float64
        assert net.shape == (3, 17, 17) and net.n_time_steps == 3 and net.n_nodes == 17
        np.testing.assert_array_equal(net.n_edges, Y.sum(axis=(1, 2)).astype(np.int64))
        offsets, src, dst = net.by_time()
        assert offsets.dtype == np.int64 and src.dtype == np.int32 and dst.dtype == np.int32
        assert offsets.shape == (4,) and offsets[0] == 0 and offsets[-1] == src.shape[0] == dst.shape[0]
        # degrees: column 0 the in-degree (column sums), column 1 the out-degree (row sums)
        deg = net.degrees()
        assert deg.dtype == np.int64 and deg.shape == (3, 17, 2)
        np.testing.assert_array_equal(deg[:, :, 0], Y.sum(axis=1))
        np.testing.assert_array_equal(deg[:, :, 1], Y.sum(axis=2))
        assert net.n_ties() == int(Y.sum())
    # the diagonal of a dense tensor is ignored; an upper triangle symmetrises on request
    Yd = _dense(rng, 2, 9, False)
    Yloop = Yd.copy(); Yloop[:, 3, 3] = 1.0
    np.testing.assert_array_equal(SparseNetwork.from_dense(Yloop).to_dense(), Yd)
    upper = SparseNetwork.from_dense(np.triu(Yd, 1))
    np.testing.assert_array_equal(upper.to_dense(symmetric=True), Yd)
    # ... and that is what numpy sees of the container an undirected estimator stored
    np.testing.assert_array_equal(np.asarray(upper.as_seen(symmetric=True)), Yd)
    np.testing.assert_array_equal(np.asarray(upper), np.triu(Yd, 1))
    np.testing.assert_array_equal(upper.as_seen(True).degrees()[:, :, 0], Yd.sum(axis=1))
    assert upper.as_seen(True).n_ties() == int(Yd.sum())

    # from_scipy == from_dense
    import scipy.sparse as sp
    Y = _dense(rng, 3, 12, True)
    for fmt in (sp.csr_matrix, sp.coo_matrix, sp.csc_matrix):
        np.testing.assert_array_equal(SparseNetwork.from_scipy([fmt(Y[t]) for t in range(3)]).to_dense(), Y)

    # from_triples: shuffled and duplicated rows, an empty time step
    Y[1] = 0.0
    tij = _triples(Y)
    tij = np.concatenate([tij, tij[::3]])[rng.permutation(tij.shape[0] + tij[::3].shape[0])]
    net = SparseNetwork.from_triples(tij, 3, 12)
    np.testing.assert_array_equal(net.to_dense(), Y)
    assert net.n_edges[1] == 0 and net.n_edges.sum() == tij.shape[0]
    np.testing.assert_array_equal(net.degrees()[:, :, 1], Y.sum(axis=2))        # duplicates count once
    assert net.n_ties() == int(Y.sum())
    np.testing.assert_array_equal(SparseNetwork([np.zeros((0, 2), dtype=int)] * 2, 5).to_dense(), np.zeros((2, 5, 5)))

    # np.shape reads .shape: no densification
    class NoDense(SparseNetwork):
        def __array__(self, *a, **k):
            raise AssertionError('densified')
    nd = NoDense([np.array([[0, 1]])], 4)
    assert np.shape(nd) == (1, 4, 4)

    # pickle
    back = pickle.loads(pickle.dumps(net))
    assert back.shape == net.shape and back.symmetric == net.symmetric
    for a, b in zip(back.by_time(), net.by_time()):
        np.testing.assert_array_equal(a, b)
    assert pickle.loads(pickle.dumps(net.as_seen(True))).symmetric


def test_value_errors_before_any_device_call():
    e = np.array([[0, 1], [2, 3]])
    with pytest.raises(ValueError, match='outside 0..3'):
        SparseNetwork([np.array([[0, 4]])], 4)                      # out of range
    with pytest.raises(ValueError, match='outside 0..3'):
        SparseNetwork([np.array([[-1, 2]])], 4)                     # negative
    with pytest.raises(ValueError, match='self loop'):
        SparseNetwork([e, np.array([[2, 2]])], 4)
    with pytest.raises(ValueError, match='integer'):
        SparseNetwork([e.astype(np.float64)], 4)
    with pytest.raises(ValueError, match='integer'):
        SparseNetwork([e.astype(bool)], 4)
    with pytest.raises(ValueError, match=r'shape \(n_t, 2\)'):
        SparseNetwork([np.array([[0, 1, 2]])], 4)
    with pytest.raises(ValueError, match='time step'):
        SparseNetwork.from_triples(np.array([[2, 0, 1]]), 2, 4)
    with pytest.raises(ValueError, match='integer'):
        SparseNetwork.from_triples(np.array([[0., 0., 1.]]), 2, 4)
    Y = np.zeros((2, 4, 4)); Y[0, 1, 2] = -1
    with pytest.raises(ValueError, match='-1'):
        SparseNetwork.from_dense(Y)
    with pytest.raises(ValueError, match='n_time_steps, n_nodes, n_nodes'):
        SparseNetwork.from_dense(np.zeros((4, 4)))

    # the estimators: no chain is opened before these answer (this box may have no GPU at all)
    net = SparseNetwork([e, e], 4)
    kw = dict(n_iter=3, tune=None, burn=None, sample_missing=True)
    for est in (da.DynamicNetworkLSM(**kw), da.DynamicNetworkLSM(is_directed=True, **kw),
                da.DynamicNetworkLPCM(**kw), da.DynamicNetworkHDPLPCM(hdp_loop='host', **kw)):
        with pytest.raises(ValueError, match='sample_missing=True is not supported with a SparseNetwork'):
            est.fit(net)
    from dynetlsm_amd.multichain import fit_chains
    with pytest.raises(ValueError, match='does not support a SparseNetwork yet'):
        fit_chains(da.DynamicNetworkLSM(n_iter=3, tune=None, burn=None), net, n_chains=2)


def test_check_network_passes_the_container_through():
    from dynetlsm_amd import _fit

    class NoDense(SparseNetwork):
        def __array__(self, *a, **k):
            raise AssertionError('densified')
    net = NoDense([np.array([[0, 1]])], 4)
    for copy in (True, False, None):
        assert _fit.check_network(net, copy) is net


def test_initialize_radii_from_degrees_is_bitwise_the_dense_path():
    rng = np.random.RandomState(3)
    Y = _dense(rng, 4, 23, True, density=0.15)
    got = init_mod.initialize_radii(SparseNetwork.from_dense(Y))
    want = init_mod.initialize_radii(Y)
    assert not np.any(want == 0.)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    # a node without ties in either direction: the regularised branch
    Y[:, 5, :] = 0.0; Y[:, :, 5] = 0.0
    net = SparseNetwork.from_dense(Y)
    # (shuffled and duplicated lists give the same counts)
    tij = _triples(Y)
    tij = np.concatenate([tij, tij[:40]])[rng.permutation(tij.shape[0] + 40)]
    want = init_mod.initialize_radii(Y)
    assert Y.sum(axis=(0, 1))[5] == 0 and Y.sum(axis=(0, 2))[5] == 0 and 0 < want[5] < 1e-4
    for n in (net, SparseNetwork.from_triples(tij, 4, 23)):
        assert init_mod.initialize_radii(n).tobytes() == want.tobytes()


def test_synthetic_network_key():
    from dynetlsm_amd.synthetic import synthetic_directed_from_model
    net = synthetic_directed_from_model(T=2, N=60, mean_degree=5.0, seed=1, use_torch=False)
    sp_net = net['network']
    assert isinstance(sp_net, SparseNetwork) and sp_net.shape == (2, 60, 60)
    np.testing.assert_array_equal(sp_net.degrees(), net['degree'])
