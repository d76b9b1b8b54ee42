"""The triad census on the device (csrc/kernels_gof_triads.hpp, dynetlsm_amd/gof.py): the (c, a, b) records
of drawn and of observed networks against the numpy replica and the derived census against the brute force
(tests/triad_ref.py), constructed networks with a census known in closed form - two of them with more than
2^32 visits -, the drawn bits against those of gof_simulate, invariance to batching and splitting, the
argument checks, the check end to end and the kernel's register hygiene.  Every comparison of counts is
integer equality.  Needs an MI355X: -m gpu."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

import gof_stats  # noqa: E402
import triad_ref as ref  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_gof import _params  # noqa: E402
from test_gpu_gof_dynamic import CASES as DYNAMIC_CASES, FIRST, S, SEED, _mode, _sparse_params, case_params, \
    host_draws  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = DYNAMIC_CASES + [(1, 3, 2, True)]
UNDIRECTED = [ref.NAMES.index(n) for n in ('003', '102', '201', '300')]
K = {n: k for k, n in enumerate(ref.NAMES)}


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _census(da, records, N, directed):
    return da.gof.derive_triad_statistics(records, N, directed)['triad_census']


def _brute(Y, directed):
    want = ref.census(Y)
    return want if directed else want[:, UNDIRECTED]


def choose3(n):
    return n * (n - 1) * (n - 2) // 6


@pytest.mark.parametrize('level', ['dense', 'sparse'])
@pytest.mark.parametrize('T,N,D,directed', CASES)
def test_records_of_drawn_networks_are_exact(da, T, N, D, directed, level):
    Xs, ic, radii = case_params(T, N, D, directed, level)
    with da.Chain(T, N, D, _mode(directed)) as c:
        got, bits = c.gof_triads_simulate(Xs, ic, radii, seed=SEED, first_index=FIRST, want_bits=True)
    assert got.shape == (S, T, ref.R) and got.dtype == np.int64
    assert bits.shape == (S, T, N, gof_stats.row_words(N))
    Y = host_draws(Xs, ic, radii, T, N, directed)            # drawn on the host from the same counters
    np.testing.assert_array_equal(gof_stats.unpack(bits, N), Y)
    for s in range(S):
        np.testing.assert_array_equal(got[s], ref.records(Y[s]))
        np.testing.assert_array_equal(_census(da, got[s], N, directed), _brute(Y[s], directed))
    if N == 2:
        assert not got[..., :48].any()                       # no third node
    if not directed:
        used = [32 + 4 * a + b for a in (0, 3) for b in (0, 3)] + [50]
        assert not np.delete(got, used, axis=-1).any()


@pytest.mark.parametrize('level', ['dense', 'sparse'])
@pytest.mark.parametrize('T,N,D,directed', CASES)
def test_records_of_observed_networks_are_exact(da, T, N, D, directed, level):
    rng = np.random.RandomState(7 * N + T + 2 * directed + 500 * (level == 'sparse'))
    Y = ref.random_network(rng, T, N, directed, 0.5 if level == 'dense' else min(0.5, 2.0 / N))
    with da.Chain(T, N, D, _mode(directed)) as c:
        got = c.gof_triads_observed(da.engine.pack_network(Y))
    assert got.shape == (T, ref.R) and got.dtype == np.int64
    np.testing.assert_array_equal(got, ref.records(Y))
    np.testing.assert_array_equal(_census(da, got, N, directed), _brute(Y, directed))


def _constructed(N):
    """six directed networks and their census in closed form"""
    i = np.arange(N)
    Y = np.zeros((6, N, N), dtype=bool)
    want = np.zeros((6, 16), dtype=np.int64)
    want[0, K['003']] = choose3(N)                           # empty
    Y[1, [0, 1, 2], [1, 2, 0]] = True                        # the cycle 0 -> 1 -> 2 -> 0 and isolates
    want[1, K['030C']] = 1
    want[1, K['012']] = 3 * (N - 3)                          # one arc of the cycle and an isolate
    want[1, K['003']] = choose3(N) - 1 - 3 * (N - 3)
    Y[2, 0, 1:] = True                                       # out-star: the hub and two leaves, 021D
    want[2, K['021D']] = (N - 1) * (N - 2) // 2
    want[2, K['003']] = choose3(N - 1)
    Y[3, 1:, 0] = True                                       # in-star: 021U
    want[3, K['021U']] = (N - 1) * (N - 2) // 2
    want[3, K['003']] = choose3(N - 1)
    Y[4] = i[:, None] < i[None, :]                           # transitive tournament
    want[4, K['030T']] = choose3(N)
    Y[5] = i[:, None] != i[None, :]                          # complete mutual
    want[5, K['300']] = choose3(N)
    return Y, want


@pytest.mark.parametrize('N', [3, 40, 131])
def test_constructed_networks(da, N):
    Y, want = _constructed(N)
    with da.Chain(6, N, 2, 'directed') as c:
        got = c.gof_triads_observed(da.engine.pack_network(Y))
    d = da.gof.derive_triad_statistics(got, N, True)
    np.testing.assert_array_equal(d['triad_census'], want)
    pairs = N * (N - 1) // 2
    np.testing.assert_array_equal(d['dyad_census'], [[0, 0, pairs], [0, 3, pairs - 3], [0, N - 1, pairs - N + 1],
                                                     [0, N - 1, pairs - N + 1], [0, pairs, 0], [pairs, 0, 0]])
    np.testing.assert_array_equal(d['transitive_triples'], [0, 0, 0, 0, choose3(N), 6 * choose3(N)])
    np.testing.assert_array_equal(d['two_paths'], [0, 3, 0, 0, choose3(N), 6 * choose3(N)])
    # the symmetric ones on an undirected chain
    with da.Chain(2, N, 2, 'undirected') as c:
        und = c.gof_triads_observed(da.engine.pack_network(Y[[0, 5]]))
    np.testing.assert_array_equal(_census(da, und, N, False), [[choose3(N), 0, 0, 0], [0, 0, 0, choose3(N)]])


def test_more_than_2_32_visits(da):
    """every triad of a tournament and of a complete network is seen from its three pairs: 3 C(2100, 3) =
    4.6e9 visits, all in one state"""
    N = 2100
    Y, want = _constructed(N)
    assert 3 * choose3(N) > 2 ** 32
    with da.Chain(1, N, 2, 'directed') as c:
        tournament = c.gof_triads_observed(da.engine.pack_network(Y[4:5]))
        complete = c.gof_triads_observed(da.engine.pack_network(Y[5:6]))
    with da.Chain(1, N, 2, 'undirected') as c:
        und = c.gof_triads_observed(da.engine.pack_network(Y[5:6]))
    pairs = N * (N - 1) // 2
    # pairs i < j of a tournament have code 1; a third node k lies below both (a = b = 2), between them
    # (a = 1, b = 2) or above both (a = b = 1): C(N, 3) each
    rec = np.zeros((1, ref.R), dtype=np.int64)
    rec[0, [4 * 2 + 2, 4 * 1 + 2, 4 * 1 + 1]] = choose3(N)
    rec[0, 48] = pairs
    np.testing.assert_array_equal(tournament, rec)
    rec = np.zeros((1, ref.R), dtype=np.int64)
    rec[0, 32 + 15], rec[0, 50] = 3 * choose3(N), pairs
    np.testing.assert_array_equal(complete, rec)
    np.testing.assert_array_equal(und, rec)
    np.testing.assert_array_equal(_census(da, tournament, N, True), want[4:5])
    np.testing.assert_array_equal(_census(da, complete, N, True), want[5:6])
    np.testing.assert_array_equal(_census(da, und, N, False), [[0, 0, 0, choose3(N)]])


@pytest.mark.parametrize('T,N,D,directed', [(3, 65, 2, False), (2, 129, 2, True)])
def test_draws_are_those_of_gof_simulate(da, T, N, D, directed):
    Xs, ic, radii = case_params(T, N, D, directed, 'dense')
    with da.Chain(T, N, D, _mode(directed)) as c:
        stats, bits0 = c.gof_simulate(Xs, ic, radii, seed=SEED, first_index=FIRST, want_bits=True)
        tri, bits = c.gof_triads_simulate(Xs, ic, radii, seed=SEED, first_index=FIRST, want_bits=True)
    np.testing.assert_array_equal(bits, bits0)
    d = da.gof.derive_triad_statistics(tri, N, directed)
    st = da.gof.derive_statistics(stats, N, directed)
    if directed:
        np.testing.assert_array_equal(d['dyad_census'][..., 0], st['mutual'])
        np.testing.assert_array_equal(d['dyad_census'][..., 1] + 2 * d['dyad_census'][..., 0], st['edges'])
    else:
        np.testing.assert_array_equal(d['triad_census'][..., 3], st['triangles'])
        np.testing.assert_array_equal(d['triad_transitivity'], st['transitivity'])
        np.testing.assert_array_equal(d['dyad_census'][..., 0], st['edges'])


@pytest.mark.parametrize('directed', [False, True])
def test_results_do_not_depend_on_batch_or_split(da, directed):
    T, N, D = 3, 65, 2
    rng = np.random.RandomState(5)
    Xs, ic, radii = _sparse_params(rng, 4, T, N, D, directed, degree=3.0)
    r = (lambda a, b: None) if radii is None else (lambda a, b: radii[a:b])
    with da.Chain(T, N, D, _mode(directed)) as c:
        whole = c.gof_triads_simulate(Xs, ic, radii, seed=11, want_bits=True)
        one = c.gof_triads_simulate(Xs, ic, radii, seed=11, batch=1, want_bits=True)
        a = c.gof_triads_simulate(Xs[:2], ic[:2], r(0, 2), seed=11, first_index=0, want_bits=True)
        b = c.gof_triads_simulate(Xs[2:], ic[2:], r(2, 4), seed=11, first_index=2, want_bits=True)
        other = c.gof_triads_simulate(Xs, ic, radii, seed=12)
    for k in range(2):
        np.testing.assert_array_equal(whole[k], one[k])
        np.testing.assert_array_equal(whole[k], np.concatenate([a[k], b[k]]))
    assert not np.array_equal(whole[0], other)


def test_bad_arguments_are_rejected(da):
    rng = np.random.RandomState(0)
    Xs, ic, radii = _params(rng, 2, 2, 9, 2, True)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.gof_triads_simulate(Xs, ic, None)
        # null radii at the C boundary
        with pytest.raises(da.EngineError) as e:
            c._ck(c._L.dlsm_gof_triads_simulate(c._h, da.engine._p(Xs), da.engine._p(ic), None, 2, 0, 0, 0,
                                                da.engine._p(np.zeros((2, 2, ref.R), dtype=np.int64)), None))
        assert e.value.code == -1
        with pytest.raises(da.EngineError) as e:
            c.gof_triads_simulate(Xs, ic, radii, first_index=2 ** 32 - 1)
        assert e.value.code == -1
        with pytest.raises(da.EngineError) as e:
            c.gof_triads_simulate(Xs, ic, radii, batch=-1)
        assert e.value.code == -1
        Y = np.zeros((2, 9, 9)); Y[1, 4, 4] = 1
        with pytest.raises(da.EngineError) as e:
            c.gof_triads_observed(da.engine.pack_network(Y))
        assert e.value.code == -4
        with pytest.raises(ValueError):
            c.gof_triads_observed(np.zeros((2, 9, 3), dtype=np.uint32))


@pytest.mark.parametrize('directed', [False, True])
def test_check_end_to_end_on_the_monks(da, directed):
    Y = load_golden('monks.npz')['Y_directed' if directed else 'Y_undirected']
    T, N = Y.shape[:2]
    S_ = 20
    m = da.DynamicNetworkLSM(n_iter=300, burn=100, tune=100, is_directed=directed, random_state=4).fit(Y)
    res = da.posterior_predictive_check(m, S_, statistics=('structural', 'triadic'), random_state=6)
    base = da.posterior_predictive_check(m, S_, random_state=6)
    assert set(base.simulated) < set(res.simulated)
    for name in base.simulated:
        np.testing.assert_array_equal(res.simulated[name], base.simulated[name])
        np.testing.assert_array_equal(res.observed[name], base.observed[name])
        np.testing.assert_array_equal(res.p_values[name], base.p_values[name])
    shapes = {'triad_census': (T, 16 if directed else 4), 'dyad_census': (T, 3), 'transitive_triples': (T,),
              'two_paths': (T,), 'triad_transitivity': (T,)}
    assert set(res.simulated) - set(base.simulated) == set(shapes)
    for name, shp in shapes.items():
        assert res.observed[name].shape == shp and res.simulated[name].shape == (S_,) + shp, name
    for name, p in res.p_values.items():
        assert np.isfinite(p).all() and ((p >= 0) & (p <= 1)).all(), name
    # the observed census is that of the data, and both families describe the same drawn networks
    np.testing.assert_array_equal(res.observed['triad_census'], _brute(Y, directed))
    if directed:
        np.testing.assert_array_equal(res.simulated['dyad_census'][..., 0], res.simulated['mutual'])
    else:
        np.testing.assert_array_equal(res.simulated['triad_census'][..., 3], res.simulated['triangles'])
        np.testing.assert_array_equal(res.simulated['triad_transitivity'], res.simulated['transitivity'])
    one = da.posterior_predictive_check(m, S_, statistics='triadic', random_state=6)
    assert set(one.simulated) == set(shapes)
    np.testing.assert_array_equal(one.simulated['triad_census'], res.simulated['triad_census'])
    labels = [line.split()[0] for line in res.summary().splitlines()]
    assert 'triad[%s]' % ('030T' if directed else 'triangle') in labels and labels[-1] == 'triad_transitivity'
    assert base.summary() == '\n'.join(res.summary().splitlines()[:len(base.summary().splitlines())])


def test_kernel_uses_no_scratch_memory():
    import instr_counts as ic
    if not os.path.exists(ic.OBJDUMP):
        pytest.skip('llvm-objdump not at hand')
    from dynetlsm_amd.build import build
    md = ic.kernel_metadata(build())
    for name in ('k_gof_triads<true>', 'k_gof_triads<false>'):
        assert name in md, 'kernel %s is not in the library' % name
        assert md[name]['scratch_bytes'] == 0 and md[name]['vgpr_spill'] == 0, (name, md[name])
