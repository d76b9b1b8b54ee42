"""The edge-list reference of the goodness-of-fit records (tests/gof_rows_ref.py) without a device: every
function against the plain loops at N <= 33 and against the dense references (tests/gof_stats.py,
tests/gof_dynamic_ref.py) at N = 65, 130 and 300, the component shortcut of the geodesic histogram against
the search from every node, and - by the reference alone, at full size - the conditions that make each case
of tests/test_gpu_gof_shapes.py worth its time on the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gof_dynamic_ref as dref  # noqa: E402
import gof_rows_ref as rr  # noqa: E402
import gof_stats  # noqa: E402
from dynetlsm_amd.engine import pack_network, packed_row_words  # noqa: E402

HB = rr.GOF_HB


def _random_case(N, directed, density, seed):
    rng = np.random.RandomState(seed)
    Y = rng.rand(2, N, N) < density
    Y[:, np.arange(N), np.arange(N)] = False
    if not directed:
        Y = np.triu(Y, 1)
    return dict(N=N, T=2, directed=directed, edges=rr.edges_of_dense(Y, directed))


def _family(kind, N, directed):
    """the networks of the device tests, scaled down to N nodes"""
    if kind == 'sparse':
        return _random_case(N, directed, 0.05, N)
    if kind == 'dense':
        return _random_case(N, directed, 0.5, N + 1)
    if kind == 'row':
        return rr.net_full_row(N, directed)
    if kind == 'clique':
        return rr.net_clique(N, 2 * N // 3, directed)
    if kind == 'hubs':              # the hubs are twins: the same neighbours but for a few
        return rr.net_hubs(N, directed, hubs=(1, N // 2, N - 1), n_common=N // 3, n_pair=2, n_late=N // 12,
                           must_have=(N - 2,))
    if kind == 'components':
        return rr.net_geodesic(N, directed, n_cycle=N // 3)
    raise KeyError(kind)


KINDS = ['sparse', 'dense', 'row', 'clique', 'hubs', 'components']


def _check_against(case, stats_ref, dynamic_ref):
    T, N, directed, edges = case['T'], case['N'], case['directed'], case['edges']
    Y = rr.dense(T, N, edges, directed)
    assert not Y[:, np.arange(N), np.arange(N)].any()
    assert directed or np.array_equal(Y, Y.swapaxes(1, 2))
    bits = rr.pack_edges(T, N, edges, directed)
    np.testing.assert_array_equal(bits, pack_network(Y))
    np.testing.assert_array_equal(rr.pack_edges(T, N, edges, directed, transposed=True),
                                  pack_network(Y.swapaxes(1, 2)))
    for t in range(T):
        np.testing.assert_array_equal(rr.edges_of_dense(Y, directed)[t],
                                      np.stack(rr.dyads(N, edges[t], directed), 1))
    want_stats = stats_ref(Y, directed)
    want_ov, want_st, want_geo = dynamic_ref(Y, directed)
    np.testing.assert_array_equal(rr.stats_records(T, N, edges, directed), want_stats)
    np.testing.assert_array_equal(rr.overlap(T, N, edges, directed), want_ov)
    np.testing.assert_array_equal(rr.steps(T, N, edges, directed), want_st)
    for t in range(T):
        np.testing.assert_array_equal(rr.geodesic_bfs(N, edges[t], directed, chunk=50), want_geo[t])
        if 'sources' in case:
            np.testing.assert_array_equal(rr.geodesic_components(N, edges[t], directed, case['sources'][t]),
                                          want_geo[t])
    return Y, want_stats, (want_ov, want_st, want_geo)


def test_the_geodesic_refusal_starts_past_32768_nodes():
    assert rr.row_words(32768) == 64 * 16 < rr.row_words(32800)


# the constructed families need room for their parts: at N = 33 only
@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('N,kind', [(2, 'sparse'), (2, 'dense'), (7, 'sparse'), (7, 'dense')] +
                         [(33, kind) for kind in KINDS])
def test_against_plain_loops(N, kind, directed):
    Y, stats, dyn = _check_against(_family(kind, N, directed), gof_stats.records_loops, dref.records_loops)
    # the batched dense statistics of the drawn cases, over leading axes
    Yb = np.stack([Y, Y[::-1]])
    np.testing.assert_array_equal(rr.batch_stats(Yb, directed), np.stack([stats, stats[::-1]]))
    ov, st, geo = rr.batch_dynamic(Yb, directed)
    back = dref.records_loops(Y[::-1], directed)
    for got, a, b in zip((ov, st, geo), dyn, back):
        np.testing.assert_array_equal(got, np.stack([a, b]))


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N', [65, 130, 300])
def test_against_dense_references(N, kind, directed):
    _check_against(_family(kind, N, directed), gof_stats.records, dref.records)


@pytest.mark.parametrize('directed', [False, True])
def test_components_against_every_source(directed):
    c = rr.net_geodesic(600, directed, n_cycle=220, seed=9)
    assert not np.array_equal(np.sort(c['edges'][1], axis=None), c['edges'][1].ravel())     # relabelled
    for t in range(2):
        want = rr.geodesic_bfs(600, c['edges'][t], directed, chunk=256)
        np.testing.assert_array_equal(rr.geodesic_components(600, c['edges'][t], directed, c['sources'][t]), want)
    # t = 1: the cycle's distances reach 110 (directed: 219), and 220 * 380 pairs have no path
    assert want[0] == 220 * 380 * (2 if directed else 1)
    assert np.flatnonzero(want).max() == (219 if directed else 110)
    with pytest.raises(AssertionError):
        rr.geodesic_components(600, c['edges'][1], directed, c['sources'][0])


def test_draws_over_the_sample_index():
    from oracle import oracle as orc
    for directed in (False, True):
        S, T, N, D = 5, 2, 9, 2
        Xs, ic, radii = rr.draw_params(3, S, T, N, D, directed)
        U = rr.batch_uniforms(orc.philox4x32, 77, 4, S, T, N, directed)
        P = rr.batch_probabilities(Xs, ic, radii, directed)
        for s in range(S):
            np.testing.assert_array_equal(U[s], gof_stats.uniforms(orc.philox4x32, 77, 4 + s, T, N, directed))
            np.testing.assert_array_equal(P[s], gof_stats.probabilities(Xs[s], ic[s], radii[s] if directed else None,
                                                                        directed))


# ---- the cases of tests/test_gpu_gof_shapes.py at full size ---------------------------------------------------
def _two_increments_and_two_bins(hist):
    """some bin >= GOF_HB takes two increments, and two such bins take any"""
    tail = np.asarray(hist)[HB:]
    return tail.max() >= 2 and (tail > 0).sum() >= 2


def _candidates(case, what):
    """per step, the dyads (i, j) whose j the kernel lists in row i: k_gof_stats the row's edges, k_gof_step
    the ones that form (undirected: j > i)"""
    N, directed, edges = case['N'], case['directed'], case['edges']
    if what == 'stats':
        return [rr.dyads(N, e, directed) for e in edges]
    ka, kb = [rr.dyads(N, e, directed) for e in edges]
    formed = ~np.isin(kb[0] * N + kb[1], ka[0] * N + ka[1])
    return [(kb[0][formed], kb[1][formed])]


def _longest_list(case, what):
    """the most candidates any row has within one chunk of columns"""
    N = case['N']
    n_chunks = -(-N // rr.COLS_PER_CHUNK)
    return max(int(np.bincount(i * n_chunks + j // rr.COLS_PER_CHUNK).max()) for i, j in _candidates(case, what))


def _row_in_every_chunk(case, what):
    N = case['N']
    n_chunks = -(-rr.row_words(N) // rr.GOF_CHUNK)
    for i, j in _candidates(case, what):
        seen = np.zeros((N, n_chunks), dtype=bool)
        seen[i, j // rr.COLS_PER_CHUNK] = True
        if seen.all(1).any():
            return True
    return False


def _level_in_every_slot(case, t):
    """some level of a search from the case's (or a hub's) first source has nodes in every used slot"""
    N = case['N']
    used, nw = rr.geodesic_slots(N)
    src = case['sources'][t][0] if 'sources' in case else int(case['hubs'][0])
    lev = rr.bfs_levels(N, case['edges'][t], case['directed'], src)
    slots = np.zeros((lev.max() + 1, used), dtype=bool)
    slots[lev[lev > 0], np.flatnonzero(lev > 0) // rr.COLS_PER_SLOT] = True
    return slots[1:].all(1).any()


# name -> (W, L, NW, chunks): the switches of the table in test_gpu_gof_shapes.py's docstring
SHAPES = {'row300': (12, 4, 1, 1), 'row700': (24, 8, 1, 1), 'clique2100': (68, 32, 2, 1),
          'hubs4200': (132, 64, 4, 1), 'hubs8200': (260, 64, 8, 2), 'geo8200': (260, 64, 8, 2),
          'geo16400': (516, 64, 16, 3)}


@pytest.mark.parametrize('name', sorted(rr.OBSERVED))
def test_shapes_of_the_observed_cases(name):
    N = rr.OBSERVED[name][1]['N']
    W, L, NW, chunks = SHAPES[name]
    assert (rr.row_words(N), packed_row_words(N)) == (W, W) and rr.lanes_per_row(W) == L
    assert rr.geodesic_slots(N)[1] == NW and -(-W // rr.GOF_CHUNK) == chunks
    if name == 'row300':
        assert W // 4 < L                           # lanes without a quad-word
    if chunks > 1:
        assert (W // 4) % L != 0                    # lane 0 of a neighbour makes a second trip
    if NW >= 4:
        used = rr.geodesic_slots(N)[0]
        assert used < NW and W % 64 != 0            # an empty slot, a part-filled one


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('name', ['row300', 'row700', 'clique2100', 'hubs4200', 'hubs8200'])
def test_conditions_of_the_constructed_cases(name, directed):
    case = rr.observed_case(name, directed)
    T, N, edges = case['T'], case['N'], case['edges']
    G = 256 // SHAPES[name][1]
    assert _longest_list(case, 'stats') > G and _longest_list(case, 'step') > G
    if name.startswith('row'):
        deg = np.bincount(rr.dyads(N, edges[1], True)[0] if directed else np.concatenate(rr.dyads(N, edges[1], False)))
        assert deg[case['hub']] == N - 1 and np.sort(deg)[-2] < N // 2
        return
    if name == 'clique2100':                        # two million edges: the dense references are quicker here
        Y = rr.dense(T, N, edges, directed)
        stats, st = gof_stats.records(Y, directed), dref.steps(Y, directed)
    else:
        stats, st = rr.stats_records(T, N, edges, directed), rr.steps(T, N, edges, directed)
    family = {'deg_out': stats[:, 2:2 + N], 'deg_in': stats[:, 2 + N:2 + 2 * N], 'esp': stats[:, 2 + 2 * N:],
              'persist_degree': st[:, :N], 'formed_sp': st[:, N:]}
    for fam in case['claims']:
        assert _two_increments_and_two_bins(family[fam].sum(0)), fam
    if name == 'clique2100':
        assert stats[1, 2 + 2 * N + HB:].sum() > 2e6 * (2 if directed else 1) and st[0, N:].sum() > 2e5
        if directed:
            assert not np.array_equal(stats[:, 2:2 + N], stats[:, 2 + N:2 + 2 * N])
    if name.startswith('hubs'):
        # the hub dyads are absent at t = 0, form with >= 2100 shared partners, and the hubs keep >= 2048 ties
        assert st[0, N + 2100:].sum() == 3 * (2 if directed else 1) and st[0, HB:N].sum() == 3
        assert stats[1, 2 + 2 * N + 2100:].sum() >= 3 and stats[1, 2 + 2102:2 + N].sum() == 3
        assert _level_in_every_slot(case, 0) and _level_in_every_slot(case, 1)
    if name == 'hubs8200':
        assert _row_in_every_chunk(case, 'stats') and _row_in_every_chunk(case, 'step')
        i, j = rr.dyads(N, edges[1], directed)
        assert ((i == case['hubs'][0]) & (j >= rr.COLS_PER_CHUNK)).sum() > 4


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('name', ['geo8200', 'geo16400'])
def test_conditions_of_the_geodesic_cases(name, directed):
    case = rr.observed_case(name, directed)
    N, edges, n_cycle = case['N'], case['edges'], case['n_cycle']
    geo = [rr.geodesic_components(N, edges[t], directed, case['sources'][t]) for t in range(2)]
    pairs = N * (N - 1) // (1 if directed else 2)
    assert geo[0][0] == 0 and geo[0].sum() == pairs and geo[1].sum() == pairs
    assert geo[1][0] == n_cycle * (N - n_cycle) * (2 if directed else 1)
    far = n_cycle - 1 if directed else n_cycle // 2
    assert far >= HB and np.flatnonzero(geo[1]).max() == far
    assert _two_increments_and_two_bins(geo[1])
    # t = 0: short distances, so wide frontiers, one of them in every used slot at once; the cycle's frontiers
    # of two nodes (directed: one) wander through the slots
    assert np.flatnonzero(geo[0]).max() < 256 and _level_in_every_slot(case, 0)
    lev = rr.bfs_levels(N, edges[1], directed, case['sources'][1][0])
    assert len(np.unique(np.flatnonzero(lev >= 1) // rr.COLS_PER_SLOT)) == rr.geodesic_slots(N)[0]
    # the bins above GOF_HB hold the cycle alone: n_cycle ordered pairs per distance
    np.testing.assert_array_equal(geo[1][HB:far], np.full(far - HB, n_cycle))


@pytest.mark.parametrize('name,directed', [(n, d) for n in sorted(rr.DRAWN) for d in rr.DRAWN[n][4]])
def test_conditions_of_the_drawn_cases(name, directed):
    T, N, D, S, _, _ = rr.DRAWN[name]
    Xs, ic, radii, Y, sure = rr.drawn_case(name, directed)
    assert Y.shape == (S, T, N, N) and (~sure).sum() <= 2
    assert 0.05 < Y.mean() < 0.95
    if name == 'one_workgroup':
        assert 8192 < S * T <= 65535                # one workgroup per network, one batch
    if name == 'two_batches':
        assert S * T > 65535 and 65535 // T == 21845 and S - 21845 < 21845
    if name == 'wide_draw':
        assert rr.row_words(N) > 64
        assert not np.array_equal(Y.sum(-1), Y.sum(-2))        # in-degrees tell the transposed plane apart
