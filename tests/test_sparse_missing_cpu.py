"""Missing dyads of a ``SparseNetwork`` on the host: the container's missing lists, the split and the scores without
any N x N array, the first fill from the lists, and the estimators' refusals.  No GPU needed."""
import tracemalloc

import numpy as np
import pytest

import dynetlsm_amd as da
from dynetlsm_amd import metrics
from dynetlsm_amd.imputer import SimpleNetworkImputer, fill_missing_lists, impute_missing_arcs
from dynetlsm_amd.model_selection import train_test_split
from dynetlsm_amd.sparse import SparseNetwork


def _dense(rng, T, N, directed, density=0.2):
    Y = (rng.rand(T, N, N) < density).astype(np.float64)
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.swapaxes(1, 2)
    idx = np.arange(N)
    Y[:, idx, idx] = 0.0
    return Y


def _with_holes(rng, T, N, directed, skip=None):
    """a network and its copy with 10 % of every slice coded -1 (none in time step ``skip``)"""
    Y = _dense(rng, T, N, directed)
    Ym, index = train_test_split(Y, 0.1, random_state=rng, is_directed=directed)
    if skip is not None:
        Ym[skip] = Y[skip]
        index = index[index[:, 0] != skip]
    return Y, Ym, index


@pytest.mark.parametrize('directed', [False, True])
def test_container_round_trip(directed):
    import scipy.sparse as sp
    rng = np.random.RandomState(1)
    T, N = 3, 19
    Y, Ym, index = _with_holes(rng, T, N, directed, skip=1)
    net = SparseNetwork.from_dense(Ym, missing_value=-1)
    assert net.has_missing and not SparseNetwork.from_dense(Y).has_missing
    np.testing.assert_array_equal(net.to_dense(symmetric=not directed), Ym)
    np.testing.assert_array_equal(net.to_dense(), Ym)        # (both orientations are listed)
    np.testing.assert_array_equal(np.asarray(net.as_seen(not directed)), Ym)
    np.testing.assert_array_equal(net.n_missing, (Ym == -1).sum(axis=(1, 2)))
    assert net.n_missing[1] == 0
    mo, ms, md = net.missing_by_time()
    assert mo.dtype == np.int64 and ms.dtype == np.int32 and md.dtype == np.int32 and mo[-1] == ms.shape[0]
    # the canonical rows alone say the same to an undirected reader
    tri = SparseNetwork.from_triples(np.stack(np.nonzero(Ym == 1), axis=1), T, N,
                                     missing=index[rng.permutation(index.shape[0])])
    np.testing.assert_array_equal(tri.to_dense(symmetric=not directed), Ym)
    full = SparseNetwork.from_triples(np.stack(np.nonzero(Ym == 1), axis=1), T, N,
                                      missing=np.stack(np.nonzero(Ym == -1), axis=1))
    for a, b in zip(full.missing_by_time(), net.missing_by_time()):
        np.testing.assert_array_equal(a, b)
    # scipy: the stored -1 entries
    for fmt in (sp.csr_matrix, sp.coo_matrix):
        got = SparseNetwork.from_scipy([fmt(Ym[t]) for t in range(T)], missing_value=-1)
        np.testing.assert_array_equal(got.to_dense(), Ym)
        for a, b in zip(got.missing_by_time(), net.missing_by_time()):
            np.testing.assert_array_equal(np.sort(a), np.sort(b))
    with pytest.raises(ValueError, match='-1'):
        SparseNetwork.from_scipy([sp.csr_matrix(Ym[t]) for t in range(T)])
    with pytest.raises(ValueError, match='-1'):
        SparseNetwork.from_dense(Ym)
    # a coded diagonal entry is no dyad
    Yd = Ym.copy(); Yd[0, 4, 4] = -1
    np.testing.assert_array_equal(SparseNetwork.from_dense(Yd, missing_value=-1).to_dense(), Ym)

    # ties only: degrees, n_ties, n_edges
    seen = net.as_seen(not directed)
    ties = (Ym == 1)
    np.testing.assert_array_equal(seen.degrees()[:, :, 1], ties.sum(axis=2))
    np.testing.assert_array_equal(seen.degrees()[:, :, 0], ties.sum(axis=1))
    assert seen.n_ties() == int(ties.sum())
    np.testing.assert_array_equal(net.n_edges, ties.sum(axis=(1, 2)))
    assert seen.has_missing and seen.symmetric == (not directed)

    # without_missing / with_ties
    bare = net.without_missing()
    assert not bare.has_missing and bare.n_missing.sum() == 0
    np.testing.assert_array_equal(bare.to_dense(), np.where(Ym == -1, 0.0, Ym))
    assert net.has_missing                                        # (the original is untouched)
    some = index[::2]
    want = np.where(Ym == -1, 0.0, Ym)
    want[some[:, 0], some[:, 1], some[:, 2]] = 1.0
    if not directed:
        want[some[:, 0], some[:, 2], some[:, 1]] = 1.0
    np.testing.assert_array_equal(net.with_ties(some).without_missing().to_dense(symmetric=not directed), want)
    assert net.with_ties(some).has_missing
    np.testing.assert_array_equal(net.with_ties(np.zeros((0, 3), dtype=np.int64)).to_dense(), Ym)

    # lookup by keys
    rows = np.stack(np.nonzero(np.ones((T, N, N))), axis=1)
    np.testing.assert_array_equal(net.lookup(rows, symmetric=not directed), Ym.ravel())


def test_bad_missing_lists_raise_as_bad_edges_do():
    e = [np.array([[0, 1], [2, 3]])]
    with pytest.raises(ValueError, match='outside 0..3'):
        SparseNetwork(e, 4, missing=[np.array([[0, 4]])])
    with pytest.raises(ValueError, match='outside 0..3'):
        SparseNetwork(e, 4, missing=[np.array([[-1, 2]])])
    with pytest.raises(ValueError, match='self loop'):
        SparseNetwork(e, 4, missing=[np.array([[2, 2]])])
    with pytest.raises(ValueError, match='integer'):
        SparseNetwork(e, 4, missing=[np.array([[0., 1.]])])
    with pytest.raises(ValueError, match='integer'):
        SparseNetwork(e, 4, missing=[np.array([[True, False]])])
    with pytest.raises(ValueError, match=r'shape \(n_t, 2\)'):
        SparseNetwork(e, 4, missing=[np.array([[0, 1, 2]])])
    with pytest.raises(ValueError, match='per time step'):
        SparseNetwork(e, 4, missing=[np.array([[0, 1]])] * 2)
    with pytest.raises(ValueError, match='time step'):
        SparseNetwork.from_triples(np.array([[0, 0, 1]]), 2, 4, missing=np.array([[2, 0, 1]]))
    with pytest.raises(ValueError, match='integer'):
        SparseNetwork.from_triples(np.array([[0, 0, 1]]), 2, 4, missing=np.array([[0., 0., 1.]]))
    # an empty list is no missing dyad
    assert not SparseNetwork(e, 4, missing=[np.zeros((0, 2), dtype=int)]).has_missing


class _StandIn(object):
    """what ``heldout_scores`` reads of a fitted model"""

    def __init__(self, index, probas, is_directed):
        self.missing_index_, self.missing_probas_, self.is_directed = index, probas, is_directed


@pytest.mark.parametrize('directed', [False, True])
def test_split(directed):
    rng = np.random.RandomState(7)
    T, N = 2, 50
    Y = _dense(rng, T, N, directed)
    # lists as a user has them: shuffled, with duplicates; undirected: one orientation of some pairs, both of others
    tij = np.stack(np.nonzero(Y if directed else np.triu(Y, 1)), axis=1)
    if not directed:
        tij = np.concatenate([tij, tij[::2][:, [0, 2, 1]]])
    tij = np.concatenate([tij, tij[::5]])
    net = SparseNetwork.from_triples(tij[rng.permutation(tij.shape[0])], T, N)
    net_train, index = train_test_split(net, 0.1, random_state=3, is_directed=directed)
    _, dense_index = train_test_split(Y, 0.1, random_state=3, is_directed=directed)
    assert index.dtype == np.int64 and index.shape[1] == 3
    # the dense function's count, per time step
    np.testing.assert_array_equal(np.bincount(index[:, 0], minlength=T), np.bincount(dense_index[:, 0], minlength=T))
    # distinct and row-major, on the model's triangle
    key = (index[:, 0] * N + index[:, 1]) * N + index[:, 2]
    assert (np.diff(key) > 0).all()
    assert (index[:, 1] != index[:, 2]).all() and (directed or (index[:, 1] < index[:, 2]).all())
    # the training network: the original with -1 exactly at the index
    want = Y.copy()
    want[index[:, 0], index[:, 1], index[:, 2]] = -1.0
    if not directed:
        want[index[:, 0], index[:, 2], index[:, 1]] = -1.0
    np.testing.assert_array_equal(net_train.to_dense(symmetric=not directed), want)
    assert 0 < Y[index[:, 0], index[:, 1], index[:, 2]].sum() < index.shape[0]     # ties and non-ties were held out
    for t in range(T):      # no orientation of a held-out tie stays in the lists
        o, s, d = net_train.by_time()
        assert not (want[t, s[o[t]:o[t + 1]], d[o[t]:o[t + 1]]] == -1).any()
    # the truth comes back through the scores' lookup
    truth = Y[index[:, 0], index[:, 1], index[:, 2]]
    np.testing.assert_array_equal(net.lookup(index, symmetric=not directed), truth)
    p = np.where(truth == 1, 0.9, 0.2)
    got = metrics.heldout_scores(_StandIn(index, p, directed), net)
    assert got == metrics.heldout_scores(_StandIn(index, p, directed), Y)
    assert got['n'] == index.shape[0] and got['auc'] == 1.0
    with pytest.raises(ValueError, match='0 / 1'):
        metrics.heldout_scores(_StandIn(index, p, directed), net_train)     # (the held-out dyads are missing there)
    # the same seed, the same split; another seed, another
    again, index2 = train_test_split(net, 0.1, random_state=3, is_directed=directed)
    np.testing.assert_array_equal(index2, index)
    for a, b in zip(again.by_time() + again.missing_by_time(), net_train.by_time() + net_train.missing_by_time()):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(train_test_split(net, 0.1, random_state=4, is_directed=directed)[1], index)
    with pytest.raises(ValueError, match='already lists missing'):
        train_test_split(net_train, 0.1, random_state=3, is_directed=directed)
    # more than half held out: the complement is drawn
    _, big = train_test_split(net, 0.8, random_state=3, is_directed=directed)
    n_dyads = N * (N - 1) // (1 if directed else 2)
    assert big.shape[0] == T * int(round(0.8 * n_dyads))
    assert np.unique((big[:, 0] * N + big[:, 1]) * N + big[:, 2]).shape[0] == big.shape[0]


def test_unrank_is_the_row_major_enumeration():
    from dynetlsm_amd.model_selection import _unrank
    for N in (2, 3, 7, 64):
        i, j = _unrank(np.arange(N * (N - 1) // 2, dtype=np.int64), N, False)
        np.testing.assert_array_equal(np.stack([i, j]), np.stack(np.triu_indices(N, 1)))
        i, j = _unrank(np.arange(N * (N - 1), dtype=np.int64), N, True)
        np.testing.assert_array_equal(np.stack([i, j]), np.stack(np.nonzero(~np.eye(N, dtype=bool))))
    # ranks beyond float precision: the last pairs of a network of 2^31 - 1 nodes
    N = 2 ** 31 - 1
    last = N * (N - 1) // 2 - 1
    i, j = _unrank(np.array([0, N - 2, N - 1, last - 2, last - 1, last], dtype=np.int64), N, False)
    np.testing.assert_array_equal(i, [0, 0, 1, N - 3, N - 3, N - 2])
    np.testing.assert_array_equal(j, [1, N - 1, 2, N - 2, N - 1, N - 1])


@pytest.mark.parametrize('directed', [False, True])
def test_split_memory_stays_far_below_the_dense_slice(directed):
    N, T = 20000, 2
    rng = np.random.RandomState(2)
    src = np.repeat(np.arange(N), 10)
    edges = [np.stack([src, (src + 1 + rng.randint(0, N - 1, src.shape[0])) % N], axis=1) for _ in range(T)]
    net = SparseNetwork(edges, N)
    tracemalloc.start()
    net_train, index = train_test_split(net, 1e-4, random_state=0, is_directed=directed)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    print('peak %.1f MB' % (peak / 1e6))
    assert peak < N * N / 8
    n_dyads = N * (N - 1) // (1 if directed else 2)
    assert index.shape == (T * int(round(1e-4 * n_dyads)), 3)
    np.testing.assert_array_equal(net_train.n_missing, np.bincount(index[:, 0]))
    assert (net_train.lookup(index, symmetric=not directed) == -1).all()


def test_first_fill_undirected_is_the_dense_imputer():
    rng = np.random.RandomState(5)
    T, N = 4, 40
    Y, Ym, index = _with_holes(rng, T, N, False, skip=2)
    want = SimpleNetworkImputer(strategy='random', missing_value=-1).fit_transform(Ym)
    net = SparseNetwork.from_dense(Ym, missing_value=-1)
    np.testing.assert_array_equal(index, metrics.missing_index(Ym, False))      # the canonical order
    n_observed = net.degrees(symmetric=True)[:, :, 1].sum(axis=1)
    ties = fill_missing_lists(index, n_observed, N)
    assert ties.shape == (index.shape[0],) and 0 < ties.sum() < ties.shape[0]
    got = net.with_ties(index[ties == 1]).without_missing().to_dense(symmetric=True)
    np.testing.assert_array_equal(got, want)


def test_first_fill_directed_draws_the_listed_arcs_only():
    rng = np.random.RandomState(6)
    T, N = 4, 40
    Y, Ym, index = _with_holes(rng, T, N, True, skip=0)
    want = impute_missing_arcs(Ym)
    assert np.isin(want, (0.0, 1.0)).all()
    np.testing.assert_array_equal(want[Ym != -1], Ym[Ym != -1])                 # observed arcs stay
    net = SparseNetwork.from_dense(Ym, missing_value=-1)
    n_observed = net.degrees(symmetric=False)[:, :, 1].sum(axis=1)
    np.testing.assert_array_equal(n_observed, (Ym == 1).sum(axis=(1, 2)))
    ties = fill_missing_lists(index, n_observed, N)
    got = net.with_ties(index[ties == 1]).without_missing().to_dense()
    np.testing.assert_array_equal(got, want)
    assert 0 < ties.sum() < ties.shape[0]
    # the stream: one RandomState(123), p per step, in step order
    r = np.random.RandomState(123)
    for t in range(T):
        m = int((index[:, 0] == t).sum())
        p = n_observed[t] / (N * (N - 1)) if m else 0.0
        np.testing.assert_array_equal(ties[index[:, 0] == t], r.choice([0, 1], p=[1 - p, p], size=m))


def test_refusals_answer_before_any_chain():
    e = np.array([[0, 1], [2, 3]])
    miss = np.array([[1, 2]])
    net = SparseNetwork([e, e], 4, missing=[miss, miss])
    kw = dict(n_iter=3, tune=None, burn=None)
    for sample in (False, True):
        with pytest.raises(ValueError, match='DynamicNetworkLPCM does not take a SparseNetwork that lists missing'):
            da.DynamicNetworkLPCM(sample_missing=sample, **kw).fit(net)
    with pytest.raises(ValueError, match='n_control is not supported with a SparseNetwork that lists missing'):
        da.DynamicNetworkLSM(is_directed=True, n_control=2, **kw).fit(net)
    with pytest.raises(ValueError, match='n_control is not supported with a SparseNetwork that lists missing'):
        da.DynamicNetworkHDPLPCM(is_directed=True, n_control=2, hdp_loop='host', **kw).fit(net)
    bare = net.without_missing()
    for est in (da.DynamicNetworkLSM(sample_missing=True, **kw),
                da.DynamicNetworkLSM(is_directed=True, sample_missing=True, **kw),
                da.DynamicNetworkHDPLPCM(hdp_loop='host', sample_missing=True, **kw)):
        with pytest.raises(ValueError, match='sample_missing=True is not supported with a SparseNetwork that lists '
                                             'no missing dyads'):
            est.fit(bare)
    with pytest.raises(ValueError, match="hdp_loop='device'"):
        da.DynamicNetworkHDPLPCM(hdp_loop='device', sample_missing=True, **kw).fit(net)
