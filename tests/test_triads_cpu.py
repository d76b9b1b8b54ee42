"""The triad census without a device: the class tables dynetlsm_amd/gof.py derives from its sixteen
representatives, ``derive_triad_statistics`` of the numpy replica's records (tests/triad_ref.py) against the
brute-force census and networkx, its agreement with the structural family, the family argument, the summary
rows, the exports and the binding.  Every comparison of counts is integer equality."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gof_stats  # noqa: E402
import triad_ref as ref  # noqa: E402
from dynetlsm_amd import gof  # noqa: E402

UNDIRECTED = [ref.NAMES.index(n) for n in ('003', '102', '201', '300')]


def test_names_and_class_table():
    assert gof.TRIAD_NAMES == ref.NAMES
    assert gof.UNDIRECTED_TRIAD_NAMES == ('empty', 'edge', 'path', 'triangle')
    assert gof.TRIAD_TABLE.shape == (4, 4, 4)
    np.testing.assert_array_equal(np.bincount(gof.TRIAD_TABLE.ravel(), minlength=16),
                                  [1, 6, 3, 3, 3, 6, 6, 6, 6, 2, 3, 3, 3, 6, 6, 1])
    # the same table from the definitions: code bits (i,j) (j,i) (i,k) (k,i) (j,k) (k,j)
    for c in range(4):
        for a in range(4):
            for b in range(4):
                assert gof.TRIAD_TABLE[c, a, b] == ref.CLASS_OF_CODE[c | a << 2 | b << 4], (c, a, b)


def test_class_weights():
    by_name = lambda w: {n: int(v) for n, v in zip(gof.TRIAD_NAMES, w) if v}  # noqa: E731
    assert by_name(gof.TRIAD_TRANSITIVE) == {'030T': 1, '120D': 2, '120U': 2, '120C': 1, '210': 3, '300': 6}
    np.testing.assert_array_equal(gof.TRIAD_TWO_PATHS, [0, 0, 0, 0, 0, 1, 1, 1, 1, 3, 2, 2, 2, 3, 4, 6])
    np.testing.assert_array_equal(gof.TRIAD_DYADS, [int(n[0]) + int(n[1]) for n in ref.NAMES])


def test_brute_force_census_of_hand_counted_networks():
    # 0 -> 1 -> 2, 0 -> 2 and an isolate: one 030T, three triads with the isolate hold one arc each
    Y = np.zeros((1, 4, 4))
    Y[0, 0, 1] = Y[0, 1, 2] = Y[0, 0, 2] = 1
    want = np.zeros(16, dtype=np.int64)
    want[ref.NAMES.index('030T')] = 1
    want[ref.NAMES.index('012')] = 3
    np.testing.assert_array_equal(ref.census(Y)[0], want)
    # 0 <-> 1 <- 2 is 111D, 0 <-> 1 -> 2 is 111U
    D = np.zeros((3, 3)); D[0, 1] = D[1, 0] = D[2, 1] = 1
    U = np.zeros((3, 3)); U[0, 1] = U[1, 0] = U[1, 2] = 1
    assert ref.classify(D) == '111D' and ref.classify(U) == '111U'


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('N', [2, 3, 4, 9, 20, 37])
def test_derived_census_equals_brute_force(N, directed):
    rng = np.random.RandomState(N + 100 * directed)
    for density in (0.05, 0.3, 0.8):
        Y = ref.random_network(rng, 3, N, directed, density)
        got = gof.derive_triad_statistics(ref.records(Y), N, directed)
        want = ref.census(Y)
        np.testing.assert_array_equal(got['triad_census'], want if directed else want[:, UNDIRECTED])
        assert got['triad_census'].shape == (3, 16 if directed else 4)
        assert (got['triad_census'].sum(-1) == N * (N - 1) * (N - 2) // 6).all()
        A = Y.astype(np.int64)
        up = np.triu(np.ones((N, N), dtype=bool), 1)
        mutual = (A * A.swapaxes(1, 2))[:, up].sum(-1)
        asym = (A != A.swapaxes(1, 2))[:, up].sum(-1)
        np.testing.assert_array_equal(got['dyad_census'], np.stack([mutual, asym, up.sum() - mutual - asym], -1))
        # i -> j -> k with i != k, and those closed by i -> k
        P = A @ A
        idx = np.arange(N)
        P[:, idx, idx] = 0
        np.testing.assert_array_equal(got['two_paths'], P.sum((1, 2)))
        np.testing.assert_array_equal(got['transitive_triples'], (P * A).sum((1, 2)))
        with np.errstate(invalid='ignore'):
            want_ratio = np.where(P.sum((1, 2)) > 0, (P * A).sum((1, 2)) / np.maximum(P.sum((1, 2)), 1), 0.0)
        np.testing.assert_array_equal(got['triad_transitivity'], want_ratio)


@pytest.mark.parametrize('directed', [False, True])
def test_derived_census_equals_networkx(directed):
    nx = pytest.importorskip('networkx')
    rng = np.random.RandomState(5 + directed)
    for N, density in ((3, 0.5), (12, 0.2), (25, 0.6)):
        Y = ref.random_network(rng, 2, N, directed, density)
        got = gof.derive_triad_statistics(ref.records(Y), N, True)['triad_census']
        for t in range(2):
            want = nx.triadic_census(nx.from_numpy_array(Y[t].astype(int), create_using=nx.DiGraph))
            assert {n: int(v) for n, v in zip(gof.TRIAD_NAMES, got[t])} == want


def test_undirected_agrees_with_the_structural_family():
    rng = np.random.RandomState(8)
    N = 31
    for density in (0.0, 0.1, 0.5):
        Y = ref.random_network(rng, 3, N, False, density)
        tri = gof.derive_triad_statistics(ref.records(Y), N, False)
        struct = gof.derive_statistics(gof_stats.records(Y, False), N, False)
        np.testing.assert_array_equal(tri['triad_census'][:, 3], struct['triangles'])
        np.testing.assert_array_equal(tri['triad_transitivity'], struct['transitivity'])
        np.testing.assert_array_equal(tri['dyad_census'][:, 0], struct['edges'])
        assert (tri['dyad_census'][:, 1] == 0).all()


def test_families():
    assert gof._families('triadic') == ('triadic',)
    assert gof._families(('triadic', 'structural')) == ('structural', 'triadic')
    assert gof._families(('geodesic', 'triadic', 'temporal')) == ('temporal', 'geodesic', 'triadic')
    assert gof._families('all') == ('structural', 'temporal', 'geodesic') == gof.FAMILIES
    for bad in ('triads', ('triadic', 'all'), ()):
        with pytest.raises(ValueError, match="statistics must be .*'triadic'"):
            gof._families(bad)


def _result(directed, with_triads, S=5, T=2, N=10):
    rng = np.random.RandomState(3)

    def stats(Y, lead):
        out = gof.derive_statistics(np.reshape([gof_stats.records(y, directed) for y in Y], lead + (T, -1)), N,
                                    directed)
        if with_triads:
            out.update(gof.derive_triad_statistics(np.reshape([ref.records(y) for y in Y], lead + (T, ref.R)), N,
                                                   directed))
        return out
    obs = stats([ref.random_network(rng, T, N, directed, 0.3)], ())
    sim = stats([ref.random_network(rng, T, N, directed, 0.3) for _ in range(S)], (S,))
    return gof.GofResult(np.arange(S), obs, sim, directed, N)


@pytest.mark.parametrize('directed', [False, True])
def test_summary_rows_and_pooled_counts(directed):
    plain, res = _result(directed, False), _result(directed, True)
    base = plain.summary().splitlines()
    lines = res.summary().splitlines()
    assert lines[:len(base)] == base                     # the new rows go after the existing ones
    assert 'triad' not in plain.summary() and 'triad_census' not in plain.pooled()[0]
    names = gof.TRIAD_NAMES if directed else gof.UNDIRECTED_TRIAD_NAMES
    assert [line.split()[0] for line in lines[len(base):]] == ['triad[%s]' % n for n in names] + ['triad_transitivity']
    obs_p, sim_p = res.pooled()
    np.testing.assert_array_equal(obs_p['triad_census'], res.observed['triad_census'].sum(0))
    np.testing.assert_array_equal(sim_p['dyad_census'], res.simulated['dyad_census'].sum(1))
    assert sim_p['triad_census'].shape == (5, len(names))
    assert obs_p['triad_transitivity'] == res.observed['transitive_triples'].sum() / res.observed['two_paths'].sum()
    for name in ('triad_census', 'dyad_census', 'transitive_triples', 'two_paths', 'triad_transitivity'):
        p = res.p_values[name]
        assert p.shape == res.observed[name].shape and ((p >= 0) & (p <= 1)).all()


def test_exports_and_binding():
    import inspect
    from dynetlsm_amd import Chain, _lib
    for name in ('derive_triad_statistics', 'TRIAD_NAMES', 'UNDIRECTED_TRIAD_NAMES'):
        assert name in gof.__all__
    for name in ('gof_triads_simulate', 'gof_triads_observed'):
        assert callable(getattr(Chain, name))
        assert 'dlsm_' + name in _lib.SIGNATURES
    assert _lib.SIGNATURES['dlsm_gof_triads_simulate'] == _lib.SIGNATURES['dlsm_gof_simulate']
    assert _lib.SIGNATURES['dlsm_gof_triads_observed'] == _lib.SIGNATURES['dlsm_gof_observed']
    p = inspect.signature(Chain.gof_triads_simulate).parameters
    assert list(p)[1:] == ['Xs', 'intercepts', 'radii', 'seed', 'first_index', 'batch', 'want_bits']
    assert p['want_bits'].default is False and p['batch'].default == 0 and p['radii'].default is None
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'dynetlsm_hip.h')).read()
    assert 'int dlsm_gof_triads_simulate(' in header and 'int dlsm_gof_triads_observed(' in header
