"""Goodness of fit over time without a device: the numpy replica of the records (tests/gof_dynamic_ref.py)
against plain loops, scipy and hand-counted networks, the identities between the records, the derived
statistics and summary rows of dynetlsm_amd/gof.py, the argument checks that need no device, and the
register hygiene of the new kernels in the built code object."""
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import gof_dynamic_ref as ref  # noqa: E402
from dynetlsm_amd import gof  # noqa: E402


def _random_network(rng, T, N, directed, density):
    Y = rng.rand(T, N, N) < density
    idx = np.arange(N)
    Y[:, idx, idx] = False
    if not directed:
        Y = np.triu(Y, 1)
        Y = Y | Y.swapaxes(1, 2)
    return Y


def _sym(A):
    A = np.asarray(A, dtype=bool)
    return A | A.T


def _path(N):
    A = np.zeros((N, N), dtype=bool)
    A[np.arange(N - 1), np.arange(1, N)] = True
    return _sym(A)


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('N', [2, 5, 11, 17])
def test_replica_agrees_with_plain_loops(N, directed):
    rng = np.random.RandomState(N + 100 * directed)
    for density in (0.15, 0.5):
        Y = _random_network(rng, 3, N, directed, density)
        for got, want in zip(ref.records(Y, directed), ref.records_loops(Y, directed)):
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('directed', [False, True])
def test_replica_geodesics_agree_with_scipy(directed):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    rng = np.random.RandomState(7 + directed)
    N = 60
    Y = _random_network(rng, 2, N, directed, 0.03)
    for t in range(2):
        d = shortest_path(csr_matrix(Y[t].astype(float)), directed=True, unweighted=True)
        d = np.where(np.isfinite(d), d, 0).astype(np.int64)
        np.testing.assert_array_equal(ref.distances(Y[t]), d)
    geo = ref.geodesic(Y, directed)
    assert geo[:, 0].min() > 0 and (geo[:, 4:].sum(1) > 0).all()       # the case has long paths and none


def test_geodesics_of_a_path_graph():
    N = 9
    geo = ref.geodesic(_path(N)[None], False)[0]
    np.testing.assert_array_equal(geo, [0] + [N - k for k in range(1, N)])          # N - k pairs at length k


def test_geodesics_of_two_components_and_an_isolated_node():
    # a triangle 0-1-2, a path 3-4-5-6 and node 7 alone
    A = np.zeros((8, 8), dtype=bool)
    for i, j in ((0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (5, 6)):
        A[i, j] = True
    geo = ref.geodesic(_sym(A)[None], False)[0]
    # 28 pairs: 3 + 3 at length 1, (3,5) (4,6) at 2, (3,6) at 3, the other 19 have no path
    np.testing.assert_array_equal(geo, [19, 6, 2, 1, 0, 0, 0, 0])
    got = gof.derive_dynamic_statistics(None, None, geo[None], None, 8, False)
    assert got['unreachable'][0] == 19 and got['diameter'][0] == 3
    assert got['mean_geodesic'][0] == pytest.approx((6 * 1 + 2 * 2 + 1 * 3) / 9.0)


def test_geodesics_of_a_directed_cycle():
    N = 7
    A = np.zeros((N, N), dtype=bool)
    A[np.arange(N), (np.arange(N) + 1) % N] = True
    np.testing.assert_array_equal(ref.distances(A), (np.arange(N)[None, :] - np.arange(N)[:, None]) % N)
    np.testing.assert_array_equal(ref.geodesic(A[None], True)[0], [0] + [N] * (N - 1))


@pytest.mark.parametrize('directed', [False, True])
def test_geodesics_of_a_complete_graph(directed):
    N = 6
    A = ~np.eye(N, dtype=bool)
    pairs = N * (N - 1) if directed else N * (N - 1) // 2
    np.testing.assert_array_equal(ref.geodesic(A[None], directed)[0], [0, pairs, 0, 0, 0, 0])


def test_three_steps_counted_by_hand():
    # t = 0: path 0-1-2-3 and the edge 1-4;  t = 1: 0-1, 1-2 stay, 2-3 and 1-4 go, 0-2 (one shared
    # partner at t = 0: node 1) and 2-4 (one: node 1) and 3-4 (none) form;  t = 2: the network of t = 1
    # without 0-1 and with 0-4 (partners at t = 1: node 2)
    N = 5
    Y = np.zeros((3, N, N), dtype=bool)
    for t, es in enumerate([((0, 1), (1, 2), (2, 3), (1, 4)),
                            ((0, 1), (1, 2), (0, 2), (2, 4), (3, 4)),
                            ((1, 2), (0, 2), (2, 4), (3, 4), (0, 4))]):
        for i, j in es:
            Y[t, i, j] = Y[t, j, i] = True
    ov, st, geo = ref.records(Y, False)
    np.testing.assert_array_equal(ov, [[4, 2, 1], [2, 5, 4], [1, 4, 5]])
    # step 0 -> 1: ties kept per node: 0: {1}, 1: {0, 2}, 2: {1}, 3: none, 4: none
    np.testing.assert_array_equal(st[0, :N], [2, 2, 1, 0, 0])
    np.testing.assert_array_equal(st[0, N:], [1, 2, 0, 0, 0])
    # step 1 -> 2: kept 1-2, 0-2, 2-4, 3-4: node 0: 1, 1: 1, 2: 3, 3: 1, 4: 2; formed 0-4, partner 2
    np.testing.assert_array_equal(st[1, :N], [0, 3, 1, 1, 0])
    np.testing.assert_array_equal(st[1, N:], [0, 1, 0, 0, 0])
    d = gof.derive_dynamic_statistics(ov, st, geo, None, N, False)
    np.testing.assert_array_equal(d['persisted'], [2, 4])
    np.testing.assert_array_equal(d['formed'], [3, 1])
    np.testing.assert_array_equal(d['dissolved'], [2, 1])
    np.testing.assert_allclose(d['persistence'], [2 / 4.0, 4 / 5.0])
    np.testing.assert_allclose(d['stability'], [(2 + 4) / 9.0, 1 / 4.0])
    np.testing.assert_array_equal(d['persist_degree'], st[:, :N])
    np.testing.assert_array_equal(d['formed_sp'], st[:, N:])
    # t = 0 is a tree: 0-1-2-3 with 4 on 1: lengths 1: 4, 2: 0-2 1-3 0-4 2-4, 3: 0-3 3-4
    np.testing.assert_array_equal(geo[0], [0, 4, 4, 2, 0])
    np.testing.assert_array_equal(d['diameter'], [3, 3, 3])           # t = 2: 1-2-4-3


@pytest.mark.parametrize('directed', [False, True])
def test_identities_between_the_records(directed):
    rng = np.random.RandomState(3 + directed)
    T, N = 4, 23
    Y = _random_network(rng, T, N, directed, 0.12)
    ov, st, geo = ref.records(Y, directed)
    edges = np.array([(Y[t].sum() if directed else np.triu(Y[t], 1).sum()) for t in range(T)])
    np.testing.assert_array_equal(np.diag(ov), edges)
    np.testing.assert_array_equal(ov, ov.T)
    for t in range(T - 1):
        assert st[t, N:].sum() == edges[t + 1] - ov[t, t + 1]
        assert st[t, :N].sum() == N
    np.testing.assert_array_equal(geo[:, 1], edges)
    assert (geo.sum(1) == (N * (N - 1) if directed else N * (N - 1) // 2)).all()


def _small_result(directed=False, S=6, T=3, N=12):
    rng = np.random.RandomState(11)
    Yo = _random_network(rng, T, N, directed, 0.2)
    obs = gof.derive_dynamic_statistics(*ref.records(Yo, directed), None, N, directed)
    recs = [ref.records(_random_network(rng, T, N, directed, 0.2), directed) for _ in range(S)]
    sim = gof.derive_dynamic_statistics(*[np.stack([r[k] for r in recs]) for k in range(3)], None, N, directed)
    return gof.GofResult(np.arange(S), obs, sim, directed, N), S, T, N


def test_derived_statistics_pooled_and_summary_rows():
    res, S, T, N = _small_result()
    shapes = {'overlap': (T, T), 'persisted': (T - 1,), 'formed': (T - 1,), 'dissolved': (T - 1,),
              'persistence': (T - 1,), 'stability': (T - 1,), 'persist_degree': (T - 1, N),
              'formed_sp': (T - 1, N), 'geodesic': (T, N), 'unreachable': (T,), 'mean_geodesic': (T,),
              'diameter': (T,)}
    assert set(res.observed) == set(shapes) == set(res.p_values)
    for name, shp in shapes.items():
        assert res.observed[name].shape == shp, name
        assert res.simulated[name].shape == (S,) + shp, name
        p = res.p_values[name]
        assert p.shape == shp and ((p >= 0) & (p <= 1)).all(), name
    sim = res.simulated
    idx = np.arange(T)
    edges = sim['overlap'][:, idx, idx]
    np.testing.assert_array_equal(sim['persisted'] + sim['formed'], edges[:, 1:])
    np.testing.assert_array_equal(sim['persisted'] + sim['dissolved'], edges[:, :-1])
    np.testing.assert_allclose(sim['stability'][:, 0], sim['persisted'].sum(1) / edges[:, :-1].sum(1))
    np.testing.assert_allclose(sim['stability'][:, 1], sim['overlap'][:, 0, 2] / edges[:, 0])
    obs_p, sim_p = res.pooled()
    assert obs_p['formed'] == res.observed['formed'].sum() and sim_p['dissolved'].shape == (S,)
    assert obs_p['persistence'] == pytest.approx(res.observed['persisted'].sum() / float(np.diag(res.observed['overlap'])[:-1].sum()))
    np.testing.assert_array_equal(obs_p['geodesic'], res.observed['geodesic'].sum(0))
    assert 'density' not in obs_p and 'edges' not in obs_p
    text = res.summary()
    labels = [line.split()[0] for line in text.splitlines()[1:]]
    last = int(np.nonzero((obs_p['geodesic'][1:] > 0) | (sim_p['geodesic'][:, 1:] > 0).any(0))[0][-1]) + 1
    assert labels == (['persistence', 'formed', 'dissolved', 'stability[1]', 'stability[2]'] +
                      ['geodesic[%d]' % k for k in range(1, last + 1)] + ['unreachable'])
    # no edges at all: ratios are 0, not nan
    z = gof.derive_dynamic_statistics(np.zeros((2, 2), int), np.zeros((1, 8), int), np.zeros((2, 4), int), None, 4,
                                      False)
    assert z['persistence'][0] == 0 and z['stability'][0] == 0 and z['mean_geodesic'][0] == 0 and z['diameter'][0] == 0


def test_structural_summary_has_no_new_rows():
    import gof_stats
    rng = np.random.RandomState(2)
    N = 9
    rec = lambda: gof_stats.records(_random_network(rng, 2, N, False, 0.3), False)  # noqa: E731
    res = gof.GofResult(np.arange(3), gof.derive_statistics(rec(), N, False),
                        gof.derive_statistics(np.stack([rec() for _ in range(3)]), N, False), False, N)
    assert set(res.pooled()[0]) == {'edges', 'triangles', 'degree', 'esp', 'density', 'transitivity'}
    text = res.summary()
    for word in ('persistence', 'stability', 'geodesic', 'unreachable', 'formed'):
        assert word not in text


def _fitted(T, N=6):
    """what posterior_predictive_check reads of a fitted model, and no device"""
    return types.SimpleNamespace(Y_fit_=np.zeros((T, N, N)), intercepts_=np.zeros((10, 1)),
                                 Xs_=np.zeros((10, T, N, 2)), n_burn_=2, is_directed=False, random_state=1,
                                 chain_=None)


def test_statistics_argument_is_checked_before_any_device_call():
    import torch
    for bad in ('geodesics', ('temporal', 'paths'), (), 3):
        with pytest.raises(ValueError, match='statistics must be'):
            gof.posterior_predictive_check(_fitted(3), 5, statistics=bad)
    with pytest.raises(ValueError, match='at least two time steps'):
        gof.posterior_predictive_check(_fitted(1), 5, statistics='temporal')
    with pytest.raises(ValueError, match='at least two time steps'):
        gof.posterior_predictive_check(_fitted(1), 5, statistics='all')
    assert gof._families('all') == ('structural', 'temporal', 'geodesic') == gof.FAMILIES
    assert gof._families(('geodesic', 'structural')) == ('structural', 'geodesic')
    if not torch.cuda.is_available():
        # a valid request gets as far as the device and says so
        from dynetlsm_amd import EngineError
        with pytest.raises(EngineError):
            gof.posterior_predictive_check(_fitted(1), 5, statistics='geodesic')


def test_exports_and_binding():
    import inspect
    from dynetlsm_amd import Chain, _lib, posterior_predictive_check
    assert 'derive_dynamic_statistics' in gof.__all__
    assert inspect.signature(posterior_predictive_check).parameters['statistics'].default == 'structural'
    for name in ('gof_dynamic_simulate', 'gof_dynamic_observed'):
        assert callable(getattr(Chain, name))
        assert 'dlsm_' + name in _lib.SIGNATURES
    p = inspect.signature(Chain.gof_dynamic_simulate).parameters
    assert p['temporal'].default is True and p['geodesic'].default is True and p['want_bits'].default is False


def test_new_kernels_use_no_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    lib = build()
    md, funcs = ic.kernel_metadata(lib), ic.disassemble(lib)
    names = ['k_gof_overlap', 'k_gof_step'] + ['k_gof_geodesic<%d>' % nw for nw in (1, 2, 4, 8, 16)]
    for name in names:
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
    for mangled, lines in funcs.items():
        if 'k_gof_overlap' in mangled or 'k_gof_step' in mangled or 'k_gof_geodesic' in mangled:
            assert not [line for line in lines if 'scratch_' in line], mangled
    # k_gof_stats is what it was: the kernels share nothing but inlined helpers
    assert md['k_gof_stats']['scratch_bytes'] == 0
