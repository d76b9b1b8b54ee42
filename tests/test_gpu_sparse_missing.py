"""Missing dyads from lists on the device (csrc/kernels_missing_edges.hpp, capi_missing_edges.hpp): the job tables
of ``set_missing_edges`` against those of the host builder ``set_missing`` on the same chain state - the canonical
index, every copy of the packed network after two imputation steps, the accumulators, all bitwise -, the error
paths, and the estimators fitted from a ``SparseNetwork`` with missing lists against the same fits from the dense
tensor.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _network(rng, T, N, directed, density=0.15):
    Y = (rng.rand(T, N, N) < density).astype(np.float64)
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.swapaxes(1, 2)
    Y[:, np.arange(N), np.arange(N)] = 0.0
    return Y


def _state(rng, T, N, directed, D=2):
    X = rng.randn(T, N, D)
    ic = rng.uniform(-0.5, 1.5, 2 if directed else 1)
    radii = None
    if directed:        # eta = b (1 - d / r) with r ~ 1 / N: keep the probabilities off 0 and 1
        radii = rng.uniform(0.5, 2.0, N)
        radii = radii / radii.sum()
        ic, X = ic * 0.05, X * (1.0 / N)
    return X, ic, radii


def _packed(c):
    n = c.network_packed_words()
    buf = np.zeros(n, dtype=np.uint32)
    c.get_network_packed(buf.ctypes.data, n)
    return buf


def _canonical(index, N, directed):
    """distinct rows, row-major, i < j undirected"""
    index = np.asarray(index, dtype=np.int64).reshape(-1, 3)
    if not directed:
        index = np.stack([index[:, 0], index[:, 1:].min(axis=1), index[:, 1:].max(axis=1)], axis=1)
    key = np.unique((index[:, 0] * N + index[:, 1]) * N + index[:, 2])
    return np.stack([key // (N * N), key // N % N, key % N], axis=1)


def _messy(da, rng, index, T, N, directed):
    """the canonical rows as a user lists them: shuffled, every fourth twice, and (undirected) a third of the
    pairs in the other orientation and another third in both"""
    rows = [index, index[::4]]
    if not directed:
        kind = rng.randint(0, 3, index.shape[0])
        rows = [index[kind == 0], index[kind >= 1][:, [0, 2, 1]], index[kind == 2], index[::4]]
    rows = np.concatenate(rows)
    rows = rows[rng.permutation(rows.shape[0])]
    return da.SparseNetwork.from_triples(np.zeros((0, 3), dtype=np.int64), T, N, missing=rows)


def _open(da, model, T, N, seed, X, ic, radii):
    c = da.Chain(T, N, X.shape[2], model, seed=seed, chain_id=2)
    c.set_positions(X)
    c.set_intercepts(ic)
    if radii is not None:
        c.set_radii(radii)
    return c


def _check_against_host_builder(da, rng, Y, index, directed, allow_ties=True, lists=None):
    """chain A: dense upload + the host builder on the canonical rows; chain B: edge-list upload + the device
    builder on the messy lists.  The index, the network after two accumulating steps and the accumulators agree."""
    T, N, _ = Y.shape
    model = 'directed' if directed else 'undirected'
    X, ic, radii = _state(rng, T, N, directed)
    lists = _messy(da, rng, index, T, N, directed) if lists is None else lists
    assert lists.n_missing.sum() > index.shape[0] or index.shape[0] < 4
    with _open(da, model, T, N, 77, X, ic, radii) as a, _open(da, model, T, N, 77, X, ic, radii) as b:
        a.upload_network(Y)
        a.set_missing(index)
        b.upload_network_edges(da.SparseNetwork.from_dense(Y))
        np.testing.assert_array_equal(_packed(b), _packed(a))
        b.set_missing_edges(lists, allow_ties=allow_ties)
        assert b.n_missing == a.n_missing == index.shape[0]
        got = b.get_missing_index()
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, index)
        np.testing.assert_array_equal(a.get_missing_index(), index)     # (read back from the host builder's tables)
        for c in (a, b):
            c.impute_missing(5, accumulate=True)
            c.impute_missing(6, accumulate=True)
        wa, wb = _packed(a), _packed(b)
        np.testing.assert_array_equal(wb, wa)
        (pa, oa, ka), (pb, ob, kb) = a.get_missing(), b.get_missing()
        assert ka == kb == 2
        assert pa.tobytes() == pb.tobytes() and oa.tobytes() == ob.tobytes()
        assert pa.min() > 0 and pa.max() < 2
        return wa, oa


def _random_index(rng, T, N, directed):
    from dynetlsm_amd.model_selection import train_test_split
    return train_test_split(np.zeros((T, N, N)), 0.1, random_state=rng, is_directed=directed)[1]


# ---- 1. the tables against the host builder's -----------------------------------------------------------------
@pytest.mark.parametrize('directed', [False, True])
def test_random_tenth(da, directed):
    rng = np.random.RandomState(3 + directed)
    T, N = 3, 40
    Y = _network(rng, T, N, directed)
    index = _random_index(rng, T, N, directed)
    words, ones = _check_against_host_builder(da, rng, Y, index, directed)
    assert 0 < ones.sum() < 2 * ones.shape[0]


def _edge_rows(T, N, directed):
    """N = 70: every dyad of node r at t = 0 (more than one 64-entry trip), nothing at t = 1, and at t = 2 the
    columns 31 / 32 / 63 / 64 / N - 1 on rows 0 and N - 1 and around the word boundaries"""
    r = N // 2
    rows = [(0, r, j) for j in range(N) if j != r]
    if directed:
        rows += [(0, j, r) for j in range(N) if j != r]
    for c in (31, 32, 63, 64, N - 1):
        rows += [(2, 0, c), (2, c - 1, c)]
        rows += [(2, N - 1, c)] if c != N - 1 else []
        if directed:
            rows += [(2, c, 0), (2, c, c - 1)]
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize('kind', ['edges', 'last_step'])
@pytest.mark.parametrize('directed', [False, True])
def test_layout_edges(da, directed, kind):
    rng = np.random.RandomState(13 + directed)
    T, N = 3, 70
    Y = _network(rng, T, N, directed)
    rows = _edge_rows(T, N, directed)
    if kind == 'last_step':
        rows = rows[rows[:, 0] == 2]
    index = _canonical(rows, N, directed)
    if kind == 'edges':
        per_row = np.bincount(index[index[:, 0] == 0, 1], minlength=N)
        assert per_row.max() == (N - 1 if directed else N - 1 - N // 2) and not (index[:, 0] == 1).any()
        assert {0, N - 1} <= set(index[:, 1]) | set(index[:, 2])
    else:
        assert (index[:, 0] == T - 1).all()
    _check_against_host_builder(da, rng, Y, index, directed)


def test_directed_arc_listed_beside_its_observed_reverse(da):
    """the arc i -> j is missing, j -> i is an observed tie: no conflict for the directed model (allow_ties=False)"""
    rng = np.random.RandomState(21)
    T, N = 3, 40
    Y = _network(rng, T, N, True)
    index = _random_index(rng, T, N, True)
    Y[index[:, 0], index[:, 1], index[:, 2]] = 0.0
    Y[index[:, 0], index[:, 2], index[:, 1]] = 1.0
    Y[:, np.arange(N), np.arange(N)] = 0.0
    index = index[Y[index[:, 0], index[:, 1], index[:, 2]] == 0]        # (a pair held out in both directions)
    assert index.shape[0] > 100
    _check_against_host_builder(da, rng, Y, index, True, allow_ties=False)


@pytest.mark.parametrize('directed', [False, True])
def test_beyond_one_trip_of_words_and_one_pass_of_the_scatter(da, directed):
    """N = 2100: 68 words per row; 300 000 distinct pairs and more listed - past one pass of the scatter's
    1024 x 256 grid - on 150 rows, every one of which reaches the last word in use"""
    rng = np.random.RandomState(23)
    T, N = 1, 2100
    Y = _network(rng, T, N, directed, density=0.02)
    if directed:
        i, j = np.nonzero(~np.eye(N, dtype=bool)[N - 150:])
        i = i + N - 150
    else:
        i, j = np.nonzero(np.triu(np.ones((N, N), dtype=bool), 1)[:150])
    index = np.stack([np.zeros(i.shape[0], dtype=np.int64), i, j], axis=1)
    assert index.shape[0] > 300000 and (index[:, 2] == N - 1).sum() >= 149
    _check_against_host_builder(da, rng, Y, index, directed)


@pytest.mark.parametrize('directed', [False, True])
def test_empty_list_after_a_list_clears_the_tables(da, directed):
    rng = np.random.RandomState(25)
    T, N = 3, 40
    model = 'directed' if directed else 'undirected'
    Y = _network(rng, T, N, directed)
    index = _random_index(rng, T, N, directed)
    X, ic, radii = _state(rng, T, N, directed)
    empty = da.SparseNetwork.from_triples(np.zeros((0, 3), dtype=np.int64), T, N)
    with _open(da, model, T, N, 5, X, ic, radii) as a, _open(da, model, T, N, 5, X, ic, radii) as b:
        a.upload_network(Y)
        b.upload_network(Y)
        a.set_missing(index)
        b.set_missing_edges(_messy(da, rng, index, T, N, directed), allow_ties=True)
        assert b.n_missing == index.shape[0]
        a.set_missing(np.zeros((0, 3), dtype=np.int64))
        b.set_missing_edges(empty)
        assert b.n_missing == 0 and b.get_missing_index().shape == (0, 3)
        codes = []
        for c in (a, b):
            with pytest.raises(da.EngineError, match='no missing dyads set') as e:
                c.impute_missing(1)
            codes.append(e.value.code)
        assert codes[0] == codes[1]
        np.testing.assert_array_equal(_packed(b), _packed(a))


# ---- 2. errors ------------------------------------------------------------------------------------------------
def _raw_set(c, offsets, src, dst, allow_ties=0):
    from dynetlsm_amd._lib import c_i64_p, c_i32_p
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    src = np.ascontiguousarray(src, dtype=np.int32); dst = np.ascontiguousarray(dst, dtype=np.int32)
    rc = c._L.dlsm_set_missing_edges(c._h, offsets.ctypes.data_as(c_i64_p), src.ctypes.data_as(c_i32_p),
                                     dst.ctypes.data_as(c_i32_p), allow_ties)
    msg = c._L.dlsm_last_error(c._h)
    return rc, (msg.decode() if msg else '')


@pytest.mark.parametrize('directed', [False, True])
def test_bad_lists_leave_the_network_and_no_tables(da, directed):
    rng = np.random.RandomState(27)
    T, N = 2, 40
    model = 'directed' if directed else 'undirected'
    Y = _network(rng, T, N, directed)
    X, ic, radii = _state(rng, T, N, directed)
    index = _random_index(rng, T, N, directed)
    index = index[Y[index[:, 0], index[:, 1], index[:, 2]] == 0]
    good = _messy(da, rng, index, T, N, directed)
    offsets, src, dst = good.missing_by_time()
    t1, i1, j1 = np.argwhere(Y == 1)[-1]                   # an observed tie of the last time step
    assert t1 == T - 1
    tie = (offsets, np.append(src, i1), np.append(dst, j1))
    mirrored = (offsets, np.append(src, j1), np.append(dst, i1))
    grow = offsets.copy(); grow[-1] += 1
    bad = src.copy(); bad[3] = N
    neg = dst.copy(); neg[0] = -1
    loop = dst.copy(); loop[5] = src[5]
    cases = [('tie listed', (grow, tie[1], tie[2]), 'code 4'), ('index out of range', (offsets, bad, dst), 'code 1'),
             ('negative index', (offsets, src, neg), 'code 1'), ('self loop', (offsets, src, loop), 'code 2')]
    if not directed:
        cases.append(('tie listed in the other orientation', (grow, mirrored[1], mirrored[2]), 'code 4'))
    with _open(da, model, T, N, 9, X, ic, radii) as c:
        c.upload_network_edges(da.SparseNetwork.from_dense(Y))
        words = _packed(c)
        for what, args, word in cases:
            c.set_missing_edges(good)                       # tables that must not survive the failure
            assert c.n_missing == index.shape[0]
            rc, msg = _raw_set(c, *args)
            assert rc == -4 and word in msg and 'a listed dyad is an observed tie' in msg, (what, rc, msg)
            assert c.get_missing_index().shape == (0, 3), what
            with pytest.raises(da.EngineError, match='no missing dyads set'):
                c.impute_missing(1)
            with pytest.raises(da.EngineError, match='no missing dyads set'):
                c.missing_sampling(True)
            np.testing.assert_array_equal(_packed(c), words, err_msg=what)      # the network is as it was
        # with allow_ties the listed tie is just a dyad to draw
        rc, msg = _raw_set(c, grow, tie[1], tie[2], allow_ties=1)
        assert rc == 0, msg
        assert c.get_missing_index().shape[0] == index.shape[0] + 1
        if directed:        # the reverse of an observed arc is no conflict unless it is a tie itself
            rc, msg = _raw_set(c, grow, mirrored[1], mirrored[2])
            assert (rc == 0) == (Y[t1, j1, i1] == 0), msg


def test_wrong_state_is_an_argument_error(da):
    T, N = 2, 12
    lists = da.SparseNetwork.from_triples(np.zeros((0, 3), dtype=np.int64), T, N, missing=np.array([[0, 1, 2]]))
    with da.Chain(T, N, 2, 'case_control') as c:
        with pytest.raises(da.EngineError, match='case-control') as e:
            c.set_missing_edges(lists)
        assert e.value.code == -1
    with da.Chain(T, N, 2, 'undirected') as c:
        with pytest.raises(da.EngineError, match='network not uploaded') as e:
            c.set_missing_edges(lists)
        assert e.value.code == -1 and c.n_missing == 0
        with pytest.raises(ValueError, match='shape'):
            c.set_missing_edges(da.SparseNetwork([np.zeros((0, 2), dtype=int)] * T, N + 1))


# ---- 3. the estimators ----------------------------------------------------------------------------------------
def _train(directed, seed=51):
    from dynetlsm_amd.model_selection import train_test_split
    rng = np.random.RandomState(seed)
    Y = _network(rng, 3, 40, directed)
    Y_train, index = train_test_split(Y, 0.1, random_state=rng, is_directed=directed)
    return Y, Y_train, index


def _same(dense, sparse, names):
    for name in names:
        a, b = np.asarray(getattr(dense, name)), np.asarray(getattr(sparse, name))
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize('sample', [True, False])
def test_undirected_lsm_from_lists_is_the_dense_fit(da, sample):
    Y, Y_train, index = _train(False)
    kw = dict(n_iter=60, tune=20, burn=20, random_state=7, sample_missing=sample)
    dense = da.DynamicNetworkLSM(**kw).fit(Y_train)
    sparse = da.DynamicNetworkLSM(**kw).fit(da.SparseNetwork.from_dense(Y_train, missing_value=-1))
    assert isinstance(sparse.Y_fit_, da.SparseNetwork) and not sparse.Y_fit_.has_missing
    assert sparse.nan_mask_ is None
    np.testing.assert_array_equal(np.asarray(sparse.Y_fit_), dense.Y_fit_)
    assert not (dense.Y_fit_ == -1).any()
    _same(dense, sparse, ['Xs_', 'intercepts_', 'logps_', 'X_'])
    if sample:
        np.testing.assert_array_equal(sparse.missing_index_, index)
        _same(dense, sparse, ['missing_index_', 'missing_probas_', 'missings_'])
        assert np.isfinite(sparse.missing_probas_).all() and sparse.n_missing_accumulated_ > 0
    else:
        assert not hasattr(sparse, 'missing_probas_')


def test_directed_lsm_from_lists_is_the_dense_fit_on_the_arc_wise_fill(da, monkeypatch):
    from dynetlsm_amd import _fit
    from dynetlsm_amd.imputer import impute_missing_arcs
    Y, Y_train, index = _train(True)
    kw = dict(n_iter=60, tune=20, burn=20, random_state=7, sample_missing=True, is_directed=True)
    sparse = da.DynamicNetworkLSM(**kw).fit(da.SparseNetwork.from_dense(Y_train, missing_value=-1))
    monkeypatch.setattr(_fit, 'impute', lambda Y: impute_missing_arcs(Y))
    dense = da.DynamicNetworkLSM(**kw).fit(Y_train)
    np.testing.assert_array_equal(np.asarray(sparse.Y_fit_), dense.Y_fit_)
    np.testing.assert_array_equal(sparse.missing_index_, index)
    _same(dense, sparse, ['Xs_', 'intercepts_', 'logps_', 'X_', 'radiis_', 'missing_index_', 'missing_probas_',
                          'missings_'])


def test_hdp_lpcm_host_loop_from_lists_is_the_dense_fit(da):
    Y, Y_train, index = _train(False, seed=53)
    kw = dict(hdp_loop='host', n_components=5, n_iter=20, tune=10, burn=10, sample_missing=True, random_state=9)
    dense = da.DynamicNetworkHDPLPCM(**kw).fit(Y_train)
    sparse = da.DynamicNetworkHDPLPCM(**kw).fit(da.SparseNetwork.from_dense(Y_train, missing_value=-1))
    np.testing.assert_array_equal(sparse.missing_index_, index)
    for name in ('logps_', 'z_', 'X_', 'missing_probas_'):
        np.testing.assert_array_equal(getattr(sparse, name), getattr(dense, name), err_msg=name)


def test_edge_list_workflow_end_to_end(da):
    from dynetlsm_amd.metrics import heldout_scores
    from dynetlsm_amd.model_selection import train_test_split
    from dynetlsm_amd.ranking import top_dyads
    rng = np.random.RandomState(55)
    T, N = 3, 60
    net = da.SparseNetwork.from_dense(np.triu(_network(rng, T, N, False), 1))
    net_train, index = train_test_split(net, 0.1, random_state=2)
    fit = da.DynamicNetworkLSM(n_iter=60, tune=20, burn=20, random_state=7, sample_missing=True).fit(net_train)
    np.testing.assert_array_equal(fit.missing_index_, index)
    scores = heldout_scores(fit, net)
    assert scores['n'] == index.shape[0]
    assert np.isfinite(scores['auc']) and np.isfinite(scores['log_loss'])
    top = top_dyads(fit, k=10, among='missing')
    assert top is not None
