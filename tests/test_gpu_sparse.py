"""Edge-list upload on the device (csrc/kernels_edges.hpp, capi_edges.hpp): the packed words and the case-control
tables against what the dense calls leave for the same network, the error paths of the raw binding, the estimators
fitted from a ``SparseNetwork`` against the same fits from the dense tensor, and a fit at a size whose dense tensor
must never be formed.  Needs an MI355X: -m gpu."""
import ctypes as C
import tracemalloc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(31, 1), (32, 3), (33, 1), (64, 3), (65, 1), (129, 3), (257, 1)]


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _network(rng, T, N, directed, density=0.3, isolate=False):
    """random ties with the layout's edges in it: a time step without ties (T > 1), a full row - degree N - 1 - at
    the last time step only (the largest degree is attained at t != 0 when T > 1), column N - 1 set on the last
    row but one; ``isolate``: node 3 has no ties in either direction at any time (the full row has N - 2 then)"""
    Y = (rng.rand(T, N, N) < density).astype(np.float64)
    Y[T - 1, 2, :] = 1.0
    if isolate:
        Y[:, 3, :] = 0.0; Y[:, :, 3] = 0.0
    Y[:, N - 2, N - 1] = 1.0
    if T > 1:
        Y[1] = 0.0
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.swapaxes(1, 2)
    idx = np.arange(N)
    Y[:, idx, idx] = 0.0
    return Y


def _packed(c):
    n = c.network_packed_words()
    buf = np.zeros(n, dtype=np.uint32)
    c.get_network_packed(buf.ctypes.data, n)
    return buf


def _triples(Y):
    return np.stack(np.nonzero(Y), axis=1)


def _variants(da, rng, Y, directed):
    """(name, SparseNetwork) forms of the same network"""
    T, N, _ = Y.shape
    S = da.SparseNetwork
    tij = _triples(Y)
    out = [('as listed', S.from_dense(Y)),
           ('shuffled', S.from_triples(tij[rng.permutation(tij.shape[0])], T, N)),
           ('every edge twice', S.from_triples(np.repeat(tij, 2, axis=0), T, N)),
           ('twice, shuffled', S.from_triples(np.concatenate([tij, tij])[rng.permutation(2 * tij.shape[0])], T, N))]
    if not directed:
        out += [('upper triangle', S.from_dense(np.triu(Y, 1))), ('lower triangle', S.from_dense(np.tril(Y, -1)))]
    return out


# ---- 1. packed words ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['undirected', 'directed'])
def test_packed_words_equal_the_dense_upload(da, model):
    rng = np.random.RandomState(11)
    directed = model == 'directed'
    for N, T in SIZES:
        Y = _network(rng, T, N, directed)
        with da.Chain(T, N, 2, model) as ref, da.Chain(T, N, 2, model) as c:
            ref.upload_network(Y)
            want = _packed(ref)
            assert want.any()
            for name, net in _variants(da, rng, Y, directed):
                c.upload_network_edges(net)
                np.testing.assert_array_equal(_packed(c), want, err_msg='%s N=%d T=%d %s' % (model, N, T, name))
            # a wholly empty network, over the words the chain held: nothing of the last upload stays
            ref.upload_network(np.zeros((T, N, N)))
            c.upload_network_edges(da.SparseNetwork([np.zeros((0, 2), dtype=np.int64)] * T, N))
            got = _packed(c)
            assert not got.any()
            np.testing.assert_array_equal(got, _packed(ref))


@pytest.mark.parametrize('model', ['undirected', 'directed'])
def test_packed_words_when_a_wavefront_shares_its_words(da, model):
    """64 consecutive edges of one row inside one word pair (columns 32 .. 95), first in the list: every lane of
    the first wavefront targets the same one or two words; and the same with all 64 lanes on one bit (duplicates)"""
    N, T = 129, 1
    run = np.stack([np.full(64, 5), np.arange(32, 96)], axis=1)
    rest = np.array([[7, 0], [128, 127], [0, 128], [6, 33]])
    for edges in (np.concatenate([run, rest]), np.concatenate([np.repeat(run[:1], 64, axis=0), rest]),
                  np.concatenate([rest[:1], run, rest[1:]])):
        net = da.SparseNetwork([edges], N)
        Y = net.to_dense(symmetric=model == 'undirected')
        with da.Chain(T, N, 2, model) as ref, da.Chain(T, N, 2, model) as c:
            ref.upload_network(Y)
            c.upload_network_edges(net)
            np.testing.assert_array_equal(_packed(c), _packed(ref))


@pytest.mark.parametrize('model', ['undirected', 'directed'])
def test_packed_words_beyond_one_trip_and_one_grid_pass(da, model):
    """N = 2100: 68 words per row, and 1.3 million pairs - several passes of the scatter's capped grid"""
    rng = np.random.RandomState(5)
    N, directed = 2100, model == 'directed'
    Y = _network(rng, 1, N, directed)
    tij = _triples(Y)
    assert tij.shape[0] > 4 * 1024 * 256
    with da.Chain(1, N, 2, model) as ref, da.Chain(1, N, 2, model) as c:
        ref.upload_network(Y)
        want = _packed(ref)
        for net in (da.SparseNetwork.from_dense(Y),
                    da.SparseNetwork.from_triples(tij[rng.permutation(tij.shape[0])], 1, N)):
            c.upload_network_edges(net)
            np.testing.assert_array_equal(_packed(c), want)


# ---- 2. case-control tables -----------------------------------------------------------------------------------
def _check_tables(da, Y, nets, n_control=7, seed=12345):
    from dynetlsm_amd.case_control import build_edge_lists
    T, N, _ = Y.shape
    deg, ie, oe = build_edge_lists(Y)
    with da.Chain(T, N, 2, 'case_control', seed=seed) as ref, da.Chain(T, N, 2, 'case_control', seed=seed) as c:
        ref.upload_edges(ie, oe, deg)
        ref.resample_controls(0, n_control)
        want_ci, want_co = ref.get_controls()
        for net in nets:
            c.upload_network_edges(net)
            assert c.edge_table_widths() == (ie.shape[2], oe.shape[2])
            got_ie, got_oe, got_deg = c.get_edge_tables()
            assert got_ie.dtype == got_oe.dtype == got_deg.dtype == np.int64
            np.testing.assert_array_equal(got_deg, deg)
            np.testing.assert_array_equal(got_ie, ie)
            np.testing.assert_array_equal(got_oe, oe)
            c.resample_controls(0, n_control)
            ci, co = c.get_controls()
            np.testing.assert_array_equal(ci, want_ci)
            np.testing.assert_array_equal(co, want_co)
    return deg


def test_case_control_tables_equal_the_host_build(da):
    rng = np.random.RandomState(21)
    for N, T in SIZES:
        Y = _network(rng, T, N, True, isolate=True)
        deg = _check_tables(da, Y, [net for _, net in _variants(da, rng, Y, True)])
        assert (deg[:, 3] == 0).all()                                   # a node with in- and out-degree 0
        if T > 1:                                                       # the largest degree at a t other than 0
            assert deg[:, :, 1].max() == N - 2 and deg[0, :, 1].max() < N - 2 and deg[T - 1, 2, 1] == N - 2
    # no ties at all: tables of width 0
    with da.Chain(2, 31, 2, 'case_control') as c:
        c.upload_network_edges(da.SparseNetwork([np.zeros((0, 2), dtype=np.int64)] * 2, 31))
        assert c.edge_table_widths() == (0, 0)
        ie, oe, dg = c.get_edge_tables()
        assert ie.shape == (2, 31, 0) and oe.shape == (2, 31, 0) and not dg.any()


def test_case_control_tables_with_a_hub_beyond_one_trip(da):
    """N = 2100: a row and a column of degree 2098 > 2048 - the emit's second trip of 64 words"""
    rng = np.random.RandomState(22)
    N = 2100
    Y = _network(rng, 1, N, True, density=0.01)
    Y[0, 7, :] = 1.0; Y[0, :, 9] = 1.0
    Y[0, 3, :] = 0.0; Y[0, :, 3] = 0.0
    Y[0, np.arange(N), np.arange(N)] = 0.0
    tij = _triples(Y)
    deg = _check_tables(da, Y, [da.SparseNetwork.from_dense(Y),
                                da.SparseNetwork.from_triples(tij[rng.permutation(tij.shape[0])], 1, N)])
    assert deg[0, 7, 1] == N - 2 > 2048 and deg[0, 9, 0] == N - 2


# ---- 3. error paths through the raw binding -------------------------------------------------------------------
def _raw_upload(c, offsets, src, dst):
    from dynetlsm_amd._lib import c_i64_p, c_i32_p
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    src = np.ascontiguousarray(src, dtype=np.int32); dst = np.ascontiguousarray(dst, dtype=np.int32)
    rc = c._L.dlsm_upload_network_edges(c._h, offsets.ctypes.data_as(c_i64_p), src.ctypes.data_as(c_i32_p),
                                        dst.ctypes.data_as(c_i32_p))
    msg = c._L.dlsm_last_error(c._h)
    return rc, (msg.decode() if msg else '')


@pytest.mark.parametrize('model', ['undirected', 'directed', 'case_control'])
def test_bad_edge_lists_leave_the_chain_without_a_network(da, model):
    rng = np.random.RandomState(31)
    T, N = 2, 33
    Y = _network(rng, T, N, model != 'undirected')
    net = da.SparseNetwork.from_dense(Y)
    offsets, src, dst = net.by_time()
    X = rng.randn(T, N, 2) * 0.1
    with da.Chain(T, N, 2, model, seed=3) as c:
        c.set_positions(X)
        c.set_intercepts([0.3] if model == 'undirected' else [0.3, 0.2])
        if model != 'undirected':
            c.set_radii(np.full(N, 1.0 / N))

        def load():
            c.upload_network_edges(net)
            if model == 'case_control':
                c.resample_controls(0, 5)
            return c.loglik_full()

        ll = load()
        assert np.isfinite(ll)
        bad_dst = dst.copy(); bad_dst[5] = N
        neg_src = src.copy(); neg_src[-1] = -1
        loop = dst.copy(); loop[7] = src[7]
        down = offsets.copy(); down[1] = offsets[2] + 1
        first = offsets.copy(); first[0] = 1
        for what, args, code, word in (('dst out of range', (offsets, src, bad_dst), -4, 'code 1'),
                                       ('negative src', (offsets, neg_src, dst), -4, 'code 1'),
                                       ('src == dst', (offsets, src, loop), -4, 'code 2'),
                                       ('decreasing offsets', (down, src, dst), -1, 'offsets decrease'),
                                       ('offsets[0] != 0', (first, src, dst), -1, 'offsets[0]')):
            rc, msg = _raw_upload(c, *args)
            assert rc == code and word in msg, (what, rc, msg)
            # the chain reads no stale contents: it has no network / no edge lists now
            with pytest.raises(da.EngineError, match='network not uploaded|edge lists'):
                c.loglik_full()
            if model != 'case_control':
                with pytest.raises(da.EngineError, match='network not uploaded'):
                    _packed(c)
            else:
                with pytest.raises(da.EngineError, match='edge lists not uploaded'):
                    c.get_edge_tables()
            assert load() == ll, what          # a valid upload afterwards works


# ---- 4. estimator equivalence ---------------------------------------------------------------------------------
_FITS = {}


def _plain_network(rng, T, N, directed, density=0.15):
    """random ties only (a full row leaves a case-control chain no controls to draw for it)"""
    Y = (rng.rand(T, N, N) < density).astype(np.float64)
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y + Y.swapaxes(1, 2)
    Y[:, np.arange(N), np.arange(N)] = 0.0
    return Y


def _lsm_pair(da, kind):
    """the same LSM fit from the dense tensor and from its SparseNetwork, without ``init=`` (the init pipeline
    uploads through the edge lists too)"""
    if kind not in _FITS:
        rng = np.random.RandomState(41)
        directed = kind != 'undirected'
        Y = _plain_network(rng, 3, 40, directed)
        kw = dict(n_iter=60, tune=20, burn=20, is_directed=directed, random_state=7)
        if kind == 'case_control':
            kw.update(n_control=10, n_resample_control=25)
        dense = da.DynamicNetworkLSM(**kw).fit(Y)
        sparse = da.DynamicNetworkLSM(**kw).fit(da.SparseNetwork.from_dense(Y))
        _FITS[kind] = (Y, dense, sparse)
    return _FITS[kind]


@pytest.mark.parametrize('kind', ['undirected', 'directed', 'case_control'])
def test_lsm_fit_from_edge_lists_is_the_dense_fit(da, kind):
    Y, dense, sparse = _lsm_pair(da, kind)
    assert isinstance(sparse.Y_fit_, da.SparseNetwork) and np.shape(sparse.Y_fit_) == Y.shape
    np.testing.assert_array_equal(np.asarray(sparse.Y_fit_), Y)
    names = ['Xs_', 'intercepts_', 'logps_', 'X_'] + (['radiis_'] if kind != 'undirected' else [])
    for name in names:
        a, b = getattr(dense, name), getattr(sparse, name)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert np.all(np.isfinite(sparse.logps_))
    if kind == 'case_control':
        from dynetlsm_amd.case_control import build_edge_lists
        deg, ie, oe = build_edge_lists(Y)
        ccs = sparse.case_control_sampler_
        np.testing.assert_array_equal(ccs.degrees_, deg)        # read back from the chain on first access
        np.testing.assert_array_equal(ccs.in_edges_, ie)
        np.testing.assert_array_equal(ccs.out_edges_, oe)


@pytest.mark.parametrize('which', ['hdp', 'lpcm'])
def test_mixture_fit_from_edge_lists_is_the_dense_fit(da, which):
    rng = np.random.RandomState(43)
    Y = _plain_network(rng, 3, 40, False)
    if which == 'hdp':
        make = lambda: da.DynamicNetworkHDPLPCM(n_iter=20, tune=10, burn=10, n_components=5, random_state=9)
    else:
        make = lambda: da.DynamicNetworkLPCM(n_iter=20, tune=10, burn=10, n_components=3, random_state=9)
    dense = make().fit(Y)
    sparse = make().fit(da.SparseNetwork.from_dense(np.triu(Y, 1)))     # one orientation per tie is enough
    assert isinstance(sparse.Y_fit_, da.SparseNetwork)
    np.testing.assert_array_equal(np.asarray(sparse.Y_fit_), Y)
    for name in ('logps_', 'z_', 'X_'):
        np.testing.assert_array_equal(getattr(sparse, name), getattr(dense, name), err_msg=name)
    assert sparse.auc_ == dense.auc_


@pytest.mark.parametrize('kind', ['undirected', 'directed'])
def test_trace_passes_read_the_container(da, kind):
    _, dense, sparse = _lsm_pair(da, kind)
    a, b = da.in_sample_scores(dense), da.in_sample_scores(sparse)
    np.testing.assert_array_equal(np.asarray(a.counts, dtype=np.float64), np.asarray(b.counts, dtype=np.float64))
    assert a.auc == b.auc and a.log_loss == b.log_loss
    np.testing.assert_array_equal(a.auc_t, b.auc_t)
    a, b = da.information_criteria(dense), da.information_criteria(sparse)
    assert a.waic == b.waic and a.dic == b.dic and a.lppd == b.lppd
    np.testing.assert_array_equal(a.sample_loglik, b.sample_loglik)


# ---- 5. no dense tensor ---------------------------------------------------------------------------------------
def test_fit_at_a_size_whose_dense_tensor_is_never_formed(da):
    """N = 20 000, T = 2, ten out-neighbours per node: peak traced host memory stays below one byte per dyad
    (800 MB, an eighth of the float64 tensor); the container, the tables' read-back and the trace are tens of MB"""
    rng = np.random.RandomState(51)
    T, N, k = 2, 20000, 10
    edges = []
    for t in range(T):
        dst = rng.randint(0, N - 1, size=(N, k))
        src = np.repeat(np.arange(N), k).reshape(N, k)
        dst = dst + (dst >= src)                # uniform over the other nodes (duplicates allowed)
        edges.append(np.stack([src.ravel(), dst.ravel()], axis=1))
    net = da.SparseNetwork(edges, N)
    out_deg = net.degrees()[:, :, 1]
    assert 9 * N * T < out_deg.sum() <= 10 * N * T
    init = dict(X=rng.randn(T, N, 2) * 0.01, intercept=np.array([0.3, 0.7]), radii=np.full(N, 1.0 / N))
    model = da.DynamicNetworkLSM(is_directed=True, n_control=50, n_iter=4, tune=2, burn=2, random_state=1)
    tracemalloc.start()
    try:
        model.fit(net, init=init)
        degrees = model.case_control_sampler_.degrees_
        _, peak = tracemalloc.get_traced_memory()
    finally:
        tracemalloc.stop()
    print('peak traced host memory: %.1f MB (bound %.1f MB)' % (peak / 1e6, T * N * N / 1e6))
    assert peak < T * N * N
    assert model.logps_.shape == (8,) and np.all(np.isfinite(model.logps_))
    np.testing.assert_array_equal(degrees[:, :, 1], out_deg)
    assert model.Y_fit_.shape == (T, N, N)
