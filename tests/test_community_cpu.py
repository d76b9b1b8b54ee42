"""Community structure without a GPU: the decomposed modularity of tests/community_ref.py and of the package against
the reference's dense form and against the reference's own recorded outputs, the arithmetic of CommunityResult on a
hand-made example, the facade's argument checks (before the library is loaded), and the C-ABI declaration with its
binding."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import community_ref  # noqa: E402
from standin_estimator import StandInEstimator  # noqa: E402

sys.path.insert(0, ROOT)
from dynetlsm_amd.community import CommunityResult, modularity_from_clusters  # noqa: E402  (loads no library)


def _random_case(directed, seed, T=4, N=17, K=6, S=3, p=0.25, with_excluded=True):
    """labels in [0, K) with label 2 never used, no tie at the last step, some 10 % of the dyads excluded"""
    rng = np.random.RandomState(seed + 100 * directed)
    Y = (rng.rand(T, N, N) < p).astype(np.int64)
    if not directed:
        Y = np.triu(Y, 1) + np.triu(Y, 1).transpose(0, 2, 1)
    Y[:, np.arange(N), np.arange(N)] = 0
    Y[T - 1] = 0
    zs = rng.randint(0, K, size=(S, T, N))
    zs[zs == 2] = 3
    excluded = None
    if with_excluded:
        excluded = rng.rand(T, N, N) < 0.1
        if not directed:
            excluded = np.triu(excluded, 1)                        # as the estimators list them: i < j
    return Y, zs, excluded


@pytest.mark.parametrize('with_excluded', [False, True])
@pytest.mark.parametrize('directed', [False, True])
def test_decomposed_modularity_is_the_dense_form(directed, with_excluded):
    K = 6
    for seed in range(4):
        Y, zs, excluded = _random_case(directed, seed, with_excluded=with_excluded)
        S, T, N = zs.shape
        clusters, _, _, _, _ = community_ref.tables(Y, zs, K, directed, excluded)
        assert (clusters[..., 2, :] == 0).all() and (clusters[..., 0].sum(-1) == N).all()     # the empty label
        if with_excluded:
            A, E = community_ref.effective(Y, excluded, directed)
            assert ((np.asarray(Y) != 0) & E).any() and clusters[..., 4].sum() > 0  # tied ones, some inside clusters
        got = modularity_from_clusters(clusters, directed)
        assert got.shape == (S, T)
        for s in range(S):
            dense_t, dense = community_ref.dense_modularity(Y, zs[s], directed, excluded)
            assert np.isnan(dense_t[T - 1]) and not np.isnan(dense_t[:T - 1]).any()
            for t in range(T):
                mine = community_ref.decomposed_modularity(clusters[s, t], directed)
                if t == T - 1:
                    assert np.isnan(mine) and np.isnan(got[s, t])
                    continue
                assert abs(mine - dense_t[t]) <= 1e-12, (s, t, mine, dense_t[t])
                assert abs(got[s, t] - dense_t[t]) <= 1e-12, (s, t, got[s, t], dense_t[t])
            assert abs(np.nanmean(got[s]) - dense) <= 1e-12


@pytest.mark.parametrize('tag,directed', [('u', False), ('d', True)])
def test_decomposed_modularity_is_the_references_own(tag, directed):
    """tests/golden/community_modularity.npz: modularity() and static_modularity() of the reference itself"""
    from conftest import load_golden
    g = load_golden('community_modularity.npz')
    Y, z = g[tag + '_Y'], g[tag + '_z']
    K = int(z.max()) + 1
    assert not (z[0] == 1).any()                                   # a label without a node
    clusters, _, _, _, _ = community_ref.tables(Y, z[None], K, directed)
    got = modularity_from_clusters(clusters[0], directed)
    np.testing.assert_allclose(got, g[tag + '_modularity_t'], rtol=0, atol=1e-12)
    assert abs(got.mean() - float(g[tag + '_modularity'])) <= 1e-12
    dense_t, dense = community_ref.dense_modularity(Y, z, directed)
    np.testing.assert_allclose(dense_t, g[tag + '_modularity_t'], rtol=0, atol=1e-12)
    for t in range(len(z)):
        assert abs(community_ref.decomposed_modularity(clusters[0, t], directed) - g[tag + '_modularity_t'][t]) <= 1e-12


def _two_cliques():
    """nodes 0-2 and 3-5 are cliques, 2 - 3 is the one tie between them, at both time steps; sample 0 moves node 2
    to the other clique's cluster at the last step, sample 1 moves nobody; ``z_`` is sample 0"""
    N = 6
    A = np.zeros((N, N), dtype=np.int64)
    for grp in ((0, 1, 2), (3, 4, 5)):
        for i in grp:
            for j in grp:
                A[i, j] = i != j
    A[2, 3] = A[3, 2] = 1
    Y = np.stack([A, A])
    home, moved = [0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 1]
    zs = np.array([[home, moved], [home, home]])
    return Y, zs


def test_result_on_two_cliques_and_a_node_that_moves():
    Y, zs = _two_cliques()
    K = 4                                                          # two label slots stay empty
    # the selected labelling carries other names (5 and 9): it is relabelled to its groups in use
    z_sel = np.where(zs[0] == 0, 5, 9)
    clusters, node_within, node_switch, moved, _ = community_ref.tables(Y, zs, K, False)
    _, inv = np.unique(z_sel.ravel(), return_inverse=True)
    sel_cl, _, _, _, sel_bl = community_ref.tables(Y, inv.reshape(1, 2, 6), 2, False, want_blocks=True)
    res = CommunityResult(np.array([7, 9]), clusters, node_within, node_switch, moved, Y.sum(axis=2), np.zeros(2), False,
                          selected_z=z_sel, selected_clusters=sel_cl[0], selected_blocks=sel_bl[0])
    assert (res.n_samples, res.n_time_steps, res.n_nodes, res.n_components) == (2, 2, 6, 4)
    # 14 ordered ties.  {0,1,2},{3,4,5}: W = 12, volumes 7 and 7: Q = (12 - 98/14) / 14 = 5/14.
    # {0,1},{2,3,4,5}: W = 2 + 8, volumes 4 and 10: Q = (10 - 116/14) / 14 = 6/49.
    q_home, q_moved = 5 / 14, 6 / 49
    np.testing.assert_allclose(res.modularity_t_samples, [[q_home, q_moved], [q_home, q_home]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(res.modularity_samples, [(q_home + q_moved) / 2, q_home], rtol=0, atol=1e-15)
    assert res.modularity == pytest.approx((3 * q_home + q_moved) / 4, abs=1e-15)
    assert res.modularity_sd == pytest.approx(abs(q_home - q_moved) / 2 / np.sqrt(2), abs=1e-15)
    lo, hi = res.modularity_interval(0.9)
    assert res.modularity_samples.min() <= lo < hi <= res.modularity_samples.max()
    assert res.modularity_selected == pytest.approx((q_home + q_moved) / 2, abs=1e-15)
    np.testing.assert_allclose(res.modularity_selected_t, [q_home, q_moved], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(res.n_clusters_samples, [[2, 2], [2, 2]])
    # densities, ordered: 12 of 12 dyads inside and 2 of 18 across; after the move 10 of 2 + 12 inside, 4 of 16 across
    np.testing.assert_allclose(res.density_within_samples, [[1.0, 10 / 14], [1.0, 1.0]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(res.density_between_samples, [[2 / 18, 4 / 16], [2 / 18, 2 / 18]], rtol=0, atol=1e-15)
    assert res.density_ratio == pytest.approx((3 * 9 + (10 / 14) / (4 / 16)) / 4, abs=1e-12)
    # the selected labelling
    np.testing.assert_array_equal(res.groups, [5, 9])
    np.testing.assert_array_equal(res.z, zs[0])
    np.testing.assert_array_equal(res.block_ties, [[[6, 1], [1, 6]], [[2, 2], [2, 8]]])
    np.testing.assert_array_equal(res.block_dyads, [[[6, 9], [9, 6]], [[2, 8], [8, 12]]])
    np.testing.assert_allclose(res.block_density, [[[1, 1 / 9], [1 / 9, 1]], [[1, 1 / 4], [1 / 4, 8 / 12]]], atol=1e-15)
    np.testing.assert_array_equal(res.flows, [[[2, 1], [0, 3]]])
    # nodes: node 2 moves in one of two samples; its ties 0, 1, 3: two stay inside at home, one after the move
    np.testing.assert_array_equal(res.switch_proba, [[0, 0, 0.5, 0, 0, 0]])
    np.testing.assert_array_equal(res.n_moved_samples, [[1], [0]])
    np.testing.assert_allclose(res.embeddedness, [[1, 1, 2 / 3, 2 / 3, 1, 1], [0.75, 0.75, 0.5, 5 / 6, 1, 1]],
                               rtol=0, atol=1e-15)
    assert res.most_mobile(2) == [(2, 0.5), (0, 0.0)] and len(res.most_mobile()) == 6
    assert res.counts['moved'] == [[1], [0]] and type(res.counts['clusters'][0][0][0][0]) is int
    assert res.counts['selected_blocks'][1][1][1] == [8, 0]
    text = res.summary()
    for word in ('modularity', 'density within', 'embeddedness', 'nodes moved', 'most mobile'):
        assert word in text, word
    assert repr(res) == text
    with pytest.raises(ValueError, match='level'):
        res.modularity_interval(1.0)


def test_result_without_ties_a_single_step_and_an_isolated_node():
    """T = 1: no step to move in; a node without a tie has no embeddedness; a network without a tie no modularity"""
    Y = np.zeros((1, 4, 4), dtype=np.int64)
    Y[0, 0, 1] = Y[0, 1, 0] = 1
    zs = np.array([[[0, 0, 1, 1]]])
    clusters, node_within, node_switch, moved, _ = community_ref.tables(Y, zs, 2, False)
    assert node_switch.shape == (0, 4) and moved.shape == (1, 0)
    res = CommunityResult(np.array([0]), clusters, node_within, node_switch, moved, Y.sum(axis=2), [0], False)
    assert res.modularity == 0.0 and np.isnan(res.modularity_sd)   # one tie inside one cluster: (2 - 4/2) / 2
    np.testing.assert_array_equal(np.isnan(res.embeddedness), [[False, False, True, True]])
    assert res.switch_proba.shape == (0, 4) and res.most_mobile(3) == [(0, 0.0), (1, 0.0), (2, 0.0)]
    assert res.block_ties is None and np.isnan(res.modularity_selected) and 'modularity' in res.summary()
    empty = CommunityResult(np.array([0]), np.zeros((1, 1, 2, 5), dtype=np.int64), np.zeros((1, 4)), np.zeros((0, 4)),
                            np.zeros((1, 0)), np.zeros((1, 4)), [0], True)
    assert np.isnan(empty.modularity) and np.isnan(empty.modularity_samples).all()
    assert empty.modularity_interval() != empty.modularity_interval()                  # (nan, nan)
    assert 'nan' in empty.summary()


def _fitted(with_labels, n_iter=20, burn=8, T=3, N=5):
    est = StandInEstimator(n_iter=n_iter, burn=burn).fit(np.zeros((T, N, N)))
    est.is_directed = False
    est.Y_fit_ = np.zeros((T, N, N))
    est.n_components = 3
    if with_labels:
        est.zs_ = np.zeros((n_iter, T, N), dtype=np.int64)
    return est


def test_facade_argument_checks_come_before_any_device_call():
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib
    loaded = _lib._LIB
    with pytest.raises(ValueError, match='Model not fit.'):
        da.community_structure(StandInEstimator())
    with pytest.raises(ValueError, match='has no labels'):
        da.community_structure(_fitted(False))
    for bad in (0, -3, 2.5, 13):                                   # 12 rows are kept
        with pytest.raises(ValueError, match='n_samples'):
            da.community_structure(_fitted(True), n_samples=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match='batch'):
            da.community_structure(_fitted(True), batch=bad)
    assert _lib._LIB is loaded                                     # none of this loaded the library


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    import dynetlsm_amd as da
    from dynetlsm_amd import _lib
    from dynetlsm_amd.build import build, dependencies
    src = open(os.path.join(ROOT, 'include', 'dynetlsm_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dlsm_community_accumulate\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'include/dynetlsm_hip.h does not declare dlsm_community_accumulate'
    args = [a.strip() for a in m.group(1).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['h', 'bits', 'mask', 'zs', 'S', 'K', 'batch', 'clusters',
                                                         'node_within', 'node_switch', 'moved', 'blocks']
    res, argtypes = _lib.SIGNATURES['dlsm_community_accumulate']
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert argtypes[3] is _lib.c_i64_p and argtypes[6] is ctypes.c_int and argtypes[11] is _lib.c_i64_p
    lib = ctypes.CDLL(build())
    assert hasattr(lib, 'dlsm_community_accumulate')
    assert callable(da.community_structure) and callable(da.Chain.community_accumulate)
    for name in ('community', 'community_structure', 'CommunityResult'):
        assert name in da.__all__ and hasattr(da, name)
    assert 'dlsm_community_accumulate(' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert {'kernels_community.hpp', 'capi_community.hpp'} <= {os.path.basename(d) for d in dependencies()}


def test_the_kernels_hold_their_tables_in_lds_without_scratch_memory():
    sys.path.insert(0, os.path.join(ROOT, 'profiles'))
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    names = ['k_comm_rows<false>', 'k_comm_rows<true>', 'k_comm_switch', 'k_comm_pack_labels']
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
    assert sorted(k for k in md if k.startswith('k_comm_')) == sorted(names)
