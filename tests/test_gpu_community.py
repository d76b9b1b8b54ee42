"""Community structure on the device (csrc/kernels_community.hpp, dynetlsm_amd/community.py) against the numpy
restatement tests/community_ref.py.  Needs an MI355X: -m gpu.

Every table is an integer count: the device must return the oracle's tables exactly.  The shapes sit where the walk
can go wrong: padding bits in the last word (N = 33) and whole words of padding (N = 70: three words rounded up to
four), more rows than a workgroup walks in one trip and a row longer than the lanes that share it at its width
(N = 300), one cluster, labels past 63 and label 255, a node and a time step without a tie, one and two time steps,
excluded dyads (some 10 %, tied ones and ones inside clusters among them), and the staging batch's boundary."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import community_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TABLES = ('clusters', 'node_within', 'node_switch', 'moved', 'blocks')


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _model(directed):
    return 'directed' if directed else 'undirected'


@functools.lru_cache(maxsize=None)
def _inputs(N, T, K, S, directed, masked, labels='all'):
    """a random network with node 1 isolated and (T >= 3) no tie at step 1; labels: 'all' of [0, K), or 'sparse':
    0, K - 1 and one label in between, the rest empty"""
    rng = np.random.RandomState(7 * N + 64 * T + K + 1000 * directed + 13 * S)
    Y = (rng.rand(T, N, N) < 0.15).astype(np.int64)
    if not directed:
        Y = np.triu(Y, 1) + np.triu(Y, 1).transpose(0, 2, 1)
    Y[:, np.arange(N), np.arange(N)] = 0
    Y[:, 1, :] = 0
    Y[:, :, 1] = 0
    if T >= 3:
        Y[1] = 0
    if labels == 'sparse':
        zs = np.array([0, K // 3, K - 1])[rng.randint(0, 3, size=(S, T, N))]
    else:
        zs = rng.randint(0, K, size=(S, T, N))
    zs[0, 0, N - 1] = K - 1                                          # the last label and the last node are in use
    excluded = None
    if masked:
        excluded = rng.rand(T, N, N) < 0.1
        if not directed:
            excluded = np.triu(excluded, 1)                          # as the estimators list them: i < j
    return Y, zs.astype(np.int64), excluded


def _compare(got, want, label):
    for name, g, w in zip(TABLES, got, want):
        if w is None:
            assert g is None, (label, name)
            continue
        assert g.dtype == np.int64 and g.shape == w.shape, (label, name, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg='%s %s' % (label, name))


def _run(da, inputs, K, directed, label, batch=0):
    Y, zs, excluded = inputs
    S, T, N = zs.shape
    bits = da.engine.pack_network(Y)
    pm = da.engine.pack_network(excluded) if excluded is not None else None
    want = community_ref.tables(Y, zs, K, directed, excluded, want_blocks=True)
    with da.Chain(T, N, 2, _model(directed)) as c:
        full = c.community_accumulate(bits, zs, K, mask=pm, batch=batch, want_blocks=True)
        lean = c.community_accumulate(bits, zs, K, mask=pm, batch=batch)
    _compare(full, want, label)
    _compare(lean, want[:4] + (None,), label + ' (no blocks)')
    clusters, blocks = full[0], full[4]
    # identities of the tables: every node in one cluster, the blocks' rows and diagonals are the clusters' columns
    assert (clusters[..., 0].sum(-1) == N).all(), label
    np.testing.assert_array_equal(blocks[..., 0].sum(-1), clusters[..., 2], err_msg=label)
    np.testing.assert_array_equal(blocks[..., 0].sum(-2), clusters[..., 3], err_msg=label)
    np.testing.assert_array_equal(np.diagonal(blocks[..., 0], axis1=2, axis2=3), clusters[..., 1], err_msg=label)
    np.testing.assert_array_equal(np.diagonal(blocks[..., 1], axis1=2, axis2=3), clusters[..., 4], err_msg=label)
    return full, want


SHAPES = [
    # N, T, K, S, labels
    (33, 2, 5, 3, 'all'),           # one word and one bit; W = 4: three words of padding
    (70, 3, 7, 4, 'all'),           # 3 words rounded up to 4, six padding bits in the third; a step without a tie
    (300, 3, 6, 3, 'all'),          # W = 12 on 16 lanes: 16 rows a trip, 300 rows; T = 3
    (40, 1, 1, 2, 'all'),           # one cluster, one time step: node_switch and moved are empty
    (70, 2, 70, 3, 'all'),          # labels spread past 63, blocks at K = 70
    (50, 2, 256, 3, 'sparse'),      # label 255 in use, 253 labels empty
    (2100, 2, 4, 2, 'all'),         # W = 68: a second word for four of the 64 lanes that share a row
]


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('N,T,K,S,labels', SHAPES)
def test_every_table_is_the_oracles(da, N, T, K, S, labels, directed, masked):
    inputs = _inputs(N, T, K, S, directed, masked, labels)
    Y, zs, excluded = inputs
    label = 'N=%d T=%d K=%d dir=%d masked=%d' % (N, T, K, directed, masked)
    full, want = _run(da, inputs, K, directed, label)
    clusters, node_within, node_switch, moved, blocks = full
    assert node_switch.shape == (T - 1, N) and moved.shape == (S, T - 1)
    A, E = community_ref.effective(Y, excluded, directed)
    # the inputs are what the case is about
    assert not A[:, 1].any() and not A[:, :, 1].any() and (node_within[:, 1] == 0).all()
    assert clusters[0, 0, K - 1, 0] >= 1 and zs.max() == K - 1
    if T >= 3:
        assert not A[1].any() and not clusters[:, 1, :, 1:4].any() and clusters[:, 1, :, 0].any()
    if K > 1 and T > 1:
        assert moved.any() and node_switch.any()
    if labels == 'sparse':
        assert (clusters[..., 0] == 0).all(axis=(0, 1)).sum() == K - 3
    if masked:
        Yb = np.asarray(Y) != 0
        assert (Yb & E).any() and clusters[..., 4].any()            # tied dyads among the excluded, some inside clusters
        assert abs(E.mean() - 0.1) < 0.04                            # some 10 % of the ordered dyads
        assert clusters[..., 2].sum() == S * A.sum() < S * Yb.sum()
    else:
        assert not clusters[..., 4].any() and not blocks[..., 1].any()


def test_results_do_not_depend_on_the_staging_batch(da):
    for directed in (False, True):
        inputs = _inputs(70, 3, 7, 5, directed, True)
        ref = None
        for batch in (0, 2, 1, 5, 8):
            got, _ = _run(da, inputs, 7, directed, 'batch=%d dir=%d' % (batch, directed), batch=batch)
            if ref is None:
                ref = got
            for x, y in zip(got, ref):
                assert x.tobytes() == y.tobytes()


def test_an_undirected_mask_excludes_a_dyad_by_either_orientation(da):
    Y, zs, excluded = _inputs(70, 3, 7, 4, False, True)
    both = excluded | excluded.transpose(0, 2, 1)
    diag = both.copy()
    diag[:, np.arange(70), np.arange(70)] = True                     # the mask's diagonal is ignored
    bits = da.engine.pack_network(Y)
    with da.Chain(3, 70, 2, 'undirected') as c:
        outs = [c.community_accumulate(bits, zs, 7, mask=da.engine.pack_network(m), want_blocks=True)
                for m in (excluded, both, np.tril(both, -1), diag)]
        pad = da.engine.pack_network(both)
        pad[:, :, 2] |= np.uint32(0xFFFFFFC0)                        # N = 70: the bits beyond column 69 are ignored
        pad[:, :, 3] = np.uint32(0xFFFFFFFF)
        outs.append(c.community_accumulate(bits, zs, 7, mask=pad, want_blocks=True))
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert x.tobytes() == y.tobytes()


def _raw(c, bits, zs, S, K, batch=0, null_zs=False):
    """the library's own answer, past the checks of Chain.community_accumulate"""
    from dynetlsm_amd import _lib
    i64 = _lib.c_i64_p
    U = c.T - 1
    zs = np.ascontiguousarray(zs, dtype=np.int64)
    Kc = max(min(K, 256), 1)
    keep = [np.full((max(S, 1), c.T, Kc, 5), -1, dtype=np.int64), np.full((c.T, c.N), -1, dtype=np.int64),
            np.full((max(U, 1), c.N), -1, dtype=np.int64), np.full((max(S, 1), max(U, 1)), -1, dtype=np.int64)]
    rc = c._L.dlsm_community_accumulate(
        c._h, bits.ctypes.data_as(_lib.c_u32_p), None, None if null_zs else zs.ctypes.data_as(i64), S, K, batch,
        keep[0].ctypes.data_as(i64), keep[1].ctypes.data_as(i64), keep[2].ctypes.data_as(i64),
        keep[3].ctypes.data_as(i64), None)
    return rc, keep


def test_bad_arguments_are_rejected_before_any_device_work(da):
    Y, zs, _ = _inputs(33, 2, 5, 3, True, False)
    bits = da.engine.pack_network(Y)
    with da.Chain(2, 33, 2, 'directed') as c:
        for bad, K in ((zs[None], 5), (zs[:, :1], 5), (zs[:0], 5), (zs, 0), (zs, 257)):
            with pytest.raises(ValueError):
                c.community_accumulate(bits, bad, K)
        with pytest.raises(ValueError):
            c.community_accumulate(bits[:1], zs, 5)
        with pytest.raises(ValueError, match='batch'):
            c.community_accumulate(bits, zs, 5, batch=-1)
        rc, _ = _raw(c, bits, zs, 3, 5)
        assert rc == 0
        at_k = zs.copy()
        at_k[2, 1, 32] = 5                                           # a label equal to K, in the last entry
        neg = zs.copy()
        neg[0, 0, 0] = -1
        for args, code in (((at_k, 3, 5), -4), ((neg, 3, 5), -4), ((zs, 3, 257), -1), ((zs, 3, 0), -1),
                           ((zs, 0, 5), -1), ((zs, 3, 5, -1), -1)):
            rc, keep = _raw(c, bits, *args)
            assert rc == code, (args[1:], rc)
            assert all((k == -1).all() for k in keep)               # nothing was written
        rc, keep = _raw(c, bits, zs, 3, 5, null_zs=True)
        assert rc == -1 and all((k == -1).all() for k in keep)
        with pytest.raises(da.EngineError) as e:
            c.community_accumulate(bits, at_k, 5)
        assert e.value.code == -4 and 'label out of range' in str(e.value)
        loop = Y.copy()
        loop[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.community_accumulate(da.engine.pack_network(loop), zs, 5)
        assert e.value.code == -4
        pad = bits.copy()
        pad[0, 3, 1] |= np.uint32(1 << 1)                            # N = 33: a bit beyond column 32
        with pytest.raises(da.EngineError) as e:
            c.community_accumulate(pad, zs, 5)
        assert e.value.code == -4
    with da.Chain(2, 33, 2, 'undirected') as c:                      # a directed network on an undirected handle
        assert (Y != Y.transpose(0, 2, 1)).any()
        with pytest.raises(da.EngineError, match='symmetric') as e:
            c.community_accumulate(bits, zs, 5)
        assert e.value.code == -4


def _network_with_groups(N, T, seed):
    """three groups of nodes, dense inside and sparse across; a fifth of the nodes changes group at every step"""
    rng = np.random.RandomState(seed)
    g = rng.randint(0, 3, size=N)
    Y = np.zeros((T, N, N))
    for t in range(T):
        if t:
            movers = rng.rand(N) < 0.2
            g = np.where(movers, rng.randint(0, 3, size=N), g)
        p = np.where(g[:, None] == g[None, :], 0.6, 0.05)
        A = np.triu(rng.rand(N, N) < p, 1)
        Y[t] = A + A.T
    return Y


def _check_result(model, res, held=None):
    ids = res.sample_ids
    directed = bool(model.is_directed)
    Y = np.asarray(model.Y_fit_)
    T, N = Y.shape[:2]
    zs = np.asarray(model.zs_)[ids]
    S, K = len(ids), int(model.n_components)
    want = community_ref.tables(Y, zs, K, directed, held)
    for name, w in zip(TABLES[:4], want[:4]):
        assert res.counts[name] == w.tolist(), name
    # the modularity of every row used: the issue's formula in integers, and the reference's dense form
    per_t = np.array([[community_ref.decomposed_modularity(want[0][s, t], directed) for t in range(T)]
                      for s in range(S)])
    assert res.modularity_t_samples.shape == (S, T) and res.modularity_samples.shape == (S,)
    np.testing.assert_allclose(res.modularity_t_samples, per_t, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.modularity_samples, np.nanmean(per_t, axis=1), rtol=0, atol=1e-12)
    for s in (0, S // 2, S - 1):
        assert abs(res.modularity_samples[s] - community_ref.dense_modularity(Y, zs[s], directed, held)[1]) <= 1e-12
    assert abs(res.modularity - res.modularity_samples.mean()) <= 1e-15
    lo, hi = res.modularity_interval()
    assert res.modularity_samples.min() <= lo <= hi <= res.modularity_samples.max()
    # the selected labelling
    z = np.asarray(model.z_)
    dense_t, dense = community_ref.dense_modularity(Y, z, directed, held)
    assert abs(res.modularity_selected - dense) <= 1e-12
    np.testing.assert_allclose(res.modularity_selected_t, dense_t, rtol=0, atol=1e-12)
    G = len(res.groups)
    np.testing.assert_array_equal(res.groups[res.z], z)
    sel = community_ref.tables(Y, res.z[None], G, directed, held, want_blocks=True)
    assert res.counts['selected_blocks'] == sel[4][0].tolist()
    assert res.block_ties.shape == res.block_dyads.shape == (T, G, G) and res.flows.shape == (T - 1, G, G)
    n = np.stack([np.bincount(res.z[t], minlength=G) for t in range(T)])
    excl = np.array(res.counts['selected_blocks'], dtype=np.int64)[..., 1]
    np.testing.assert_array_equal(res.block_dyads + excl,
                                  n[:, :, None] * n[:, None, :] - np.eye(G, dtype=np.int64) * n[:, :, None])
    assert (excl.sum() > 0) == (held is not None)
    A, _ = community_ref.effective(Y, held, directed)
    assert res.block_ties.sum() == A.sum() and (res.flows.sum(axis=(1, 2)) == N).all()
    np.testing.assert_array_equal(res.flows.sum(axis=2), n[:-1])
    # per node
    np.testing.assert_allclose(res.switch_proba, (zs[:, 1:] != zs[:, :-1]).mean(axis=0), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(res.n_moved_samples, (zs[:, 1:] != zs[:, :-1]).sum(axis=2))
    share = np.full((T, N), np.nan)
    deg = A.sum(axis=2)
    np.divide(want[1], S * deg, out=share, where=deg > 0)
    np.testing.assert_allclose(res.embeddedness, share, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(res.n_clusters_samples, [[len(np.unique(zs[s, t])) for t in range(T)]
                                                           for s in range(S)])
    ties_in, dyads_in = want[0][..., 1].sum(-1), (want[0][..., 0] * (want[0][..., 0] - 1) - want[0][..., 4]).sum(-1)
    np.testing.assert_allclose(res.density_within_samples, ties_in / dyads_in, rtol=0, atol=1e-15)
    assert len(res.most_mobile(3)) == 3 and 'modularity' in res.summary()
    return want


def test_end_to_end_on_a_short_hdp_lpcm_fit(da):
    T, N = 3, 40
    Y = _network_with_groups(N, T, seed=3)
    hdp = da.DynamicNetworkHDPLPCM(n_iter=200, burn=50, tune=50, n_components=6, random_state=1).fit(Y)
    res = da.community_structure(hdp)
    assert res.n_samples == len(da._trace.sample_rows(hdp, None)) and res.n_components == 6
    _check_result(hdp, res)
    few = da.community_structure(hdp, n_samples=7, batch=3)
    assert few.n_samples == 7 and few.sample_ids[-1] == res.sample_ids[-1]
    assert few.counts['selected_blocks'] == res.counts['selected_blocks']
    keep = np.isin(res.sample_ids, few.sample_ids)
    assert few.counts['clusters'] == np.array(res.counts['clusters'], dtype=np.int64)[keep].tolist()
    hdp.release_device_trace()                                       # the call then makes a chain of its own
    again = da.community_structure(hdp)
    assert again.counts == res.counts
    print(res.summary())


def test_end_to_end_on_a_short_lpcm_fit_with_held_out_dyads(da):
    from dynetlsm_amd.model_selection import train_test_split
    T, N = 3, 40
    Y = _network_with_groups(N, T, seed=5)
    Yt, index = train_test_split(Y, 0.1, random_state=1, is_directed=False)
    lp = da.DynamicNetworkLPCM(n_iter=200, burn=50, tune=50, n_components=3, random_state=2,
                               sample_missing=True).fit(Yt)
    held = np.zeros(Y.shape, dtype=bool)
    held[index[:, 0], index[:, 1], index[:, 2]] = True
    res = da.community_structure(lp)
    _check_result(lp, res, held)
    lp.chain_.close()
    print(res.summary())
