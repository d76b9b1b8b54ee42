"""The goodness-of-fit kernels (csrc/kernels_gof.hpp, csrc/kernels_gof_dynamic.hpp) through
``Chain.gof_observed``, ``gof_dynamic_observed``, ``gof_simulate`` and ``gof_dynamic_simulate`` at the smallest
shapes that cross each of their structural switches.  Every record is an integer record and every comparison
is equality with a host reference: the edge-list reference tests/gof_rows_ref.py, which
tests/test_gof_rows_ref_cpu.py pins to the plain loops and to the dense references and which also builds the
networks, and the dense references themselves where they are affordable.  That file also shows, by the
reference alone, that each case does reach what it is listed for here.  Needs an MI355X: -m gpu.

W = 4 ceil(ceil(N / 32) / 4) row words, L = gof_lanes_per_row(W) lanes per listed neighbour, NW register
slots of the search.

  switch                                                     crossed by
  ---------------------------------------------------------  --------------------------------------------------
  bins >= GOF_HB = 2048 go to the record by global atomics   deg_out, deg_in, esp: clique2100 (two million edges
                                                             into a few bins), hubs4200, hubs8200; persist_degree,
                                                             formed_sp: hubs4200, hubs8200 (three increments
                                                             each, two of them into one bin); geodesic levels:
                                                             geo8200, geo16400 (undirected and directed, 4400
                                                             sources into every bin from 2048 to 2200 or 4399)
  a row scanned in more than one chunk of 256 words          hubs8200 (hub rows with neighbours, and formed
                                                             dyads, on both sides of column 8192), geo8200;
                                                             three chunks: geo16400
  L = 4, Wq = 3 < L; L = 8; L = 32; L = 64                   row300; row700; clique2100; hubs4200 and larger
  Wq not a multiple of L: a second trip of lane 0            hubs8200, geo8200 (Wq = 65), geo16400 (Wq = 129)
  a list longer than 256 / L: several trips of the e0 loop   row300 ... hubs8200, in k_gof_stats and k_gof_step;
                                                             more than four in the second chunk: hubs8200
  k_gof_geodesic<NW>, NW = 4, 8, 16: a part-filled slot, an  hubs4200 (4); geo8200 (8); geo16400 (16)
  empty one, the frontier in slots k >= 1
  a directed search with NW >= 2                             clique2100 (2), hubs4200, geo8200, geo16400
  the geodesic refusal above 32768 nodes                     test_geodesic_is_refused_past_32768_nodes
  one workgroup per network (S T > 8192)                     one_workgroup (k_gof_stats, k_gof_step, k_gof_geodesic)
  a batch cut at the grid's y extent (S T > 65535)           two_batches
  k_gof_transpose and k_gof_draw (both planes) at W > 64     directed clique2100 ... geo16400; wide_draw
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gof_dynamic_ref as dref  # noqa: E402
import gof_rows_ref as rr  # noqa: E402
import gof_stats  # noqa: E402

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize('directed', [False, True], ids=['undirected', 'directed'])


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _mode(directed):
    return 'directed' if directed else 'undirected'


def _observed(da, case, geodesic=True):
    """the device's records of a case's network: stats, overlap, steps, geodesic"""
    T, N, directed = case['T'], case['N'], case['directed']
    bits = rr.pack_edges(T, N, case['edges'], directed)
    with da.Chain(T, N, 2, _mode(directed)) as c:
        stats = c.gof_observed(bits)
        ov, st, geo = c.gof_dynamic_observed(bits, geodesic=geodesic)
    return stats, ov, st, geo


def _assert_edge_list_records(case, stats, ov, st):
    T, N, directed, edges = case['T'], case['N'], case['directed'], case['edges']
    np.testing.assert_array_equal(stats, rr.stats_records(T, N, edges, directed))
    np.testing.assert_array_equal(ov, rr.overlap(T, N, edges, directed))
    np.testing.assert_array_equal(st, rr.steps(T, N, edges, directed))


def _assert_dense_records(case, stats, ov, st, geo):
    T, N, directed = case['T'], case['N'], case['directed']
    Y = rr.dense(T, N, case['edges'], directed)
    np.testing.assert_array_equal(stats, gof_stats.records(Y, directed))
    np.testing.assert_array_equal(ov, dref.overlap(Y, directed))
    np.testing.assert_array_equal(st, dref.steps(Y, directed))
    np.testing.assert_array_equal(geo, dref.geodesic(Y, directed))


# ---- observed records on constructed networks -----------------------------------------------------------------
@BOTH
@pytest.mark.parametrize('name', ['row300', 'row700'])
def test_a_full_row_at_four_and_eight_lanes(da, name, directed):
    case = rr.observed_case(name, directed)
    stats, ov, st, geo = _observed(da, case)
    _assert_edge_list_records(case, stats, ov, st)
    _assert_dense_records(case, stats, ov, st, geo)


@BOTH
def test_a_clique_past_the_lds_bins(da, directed):
    case = rr.observed_case('clique2100', directed)
    stats, ov, st, geo = _observed(da, case)
    _assert_dense_records(case, stats, ov, st, geo)
    np.testing.assert_array_equal(ov, rr.overlap(2, case['N'], case['edges'], directed))


@BOTH
def test_hubs_at_sixty_four_lanes(da, directed):
    case = rr.observed_case('hubs4200', directed)
    N, edges = case['N'], case['edges']
    stats, ov, st, geo = _observed(da, case)
    _assert_edge_list_records(case, stats, ov, st)
    # the host's search from every node takes seconds per network: the directed variant is held to it at
    # t = 1 alone (the step with the hub dyads), the undirected one at both steps
    for t in ((1,) if directed else (0, 1)):
        np.testing.assert_array_equal(geo[t], rr.geodesic_bfs(N, edges[t], directed))
    np.testing.assert_array_equal(geo[:, 1], stats[:, 0])
    np.testing.assert_array_equal(geo.sum(1), np.full(2, N * (N - 1) // (1 if directed else 2)))


@BOTH
def test_hubs_across_two_chunks(da, directed):
    case = rr.observed_case('hubs8200', directed)
    stats, ov, st, _ = _observed(da, case, geodesic=False)
    _assert_edge_list_records(case, stats, ov, st)


@BOTH
@pytest.mark.parametrize('name', ['geo8200', 'geo16400'])
def test_long_and_wide_searches(da, name, directed):
    case = rr.observed_case(name, directed)
    N, edges = case['N'], case['edges']
    stats, ov, st, geo = _observed(da, case)
    for t in range(2):
        np.testing.assert_array_equal(geo[t], rr.geodesic_components(N, edges[t], directed, case['sources'][t]))
    _assert_edge_list_records(case, stats, ov, st)


@BOTH
def test_geodesic_is_refused_past_32768_nodes(da, directed):
    case = rr.net_sparse(32800, 1, directed)
    N = case['N']
    bits = rr.pack_edges(1, N, case['edges'], directed)
    with da.Chain(1, N, 2, _mode(directed)) as c:
        with pytest.raises(da.EngineError) as e:
            c.gof_dynamic_observed(bits, geodesic=True)
        assert e.value.code == -5                   # DLSM_E_LIMIT
        ov, st, geo = c.gof_dynamic_observed(bits, geodesic=False)
    assert geo is None and st.shape == (0, 2 * N)
    np.testing.assert_array_equal(ov, rr.overlap(1, N, case['edges'], directed))
    assert ov[0, 0] == len(rr.dyads(N, case['edges'][0], directed)[0]) > N


# ---- drawn networks across the launch caps --------------------------------------------------------------------
def _simulate(c, Xs, ic, radii, first):
    stats, bits = c.gof_simulate(Xs, ic, radii, seed=rr.DRAW_SEED, first_index=first, want_bits=True)
    ov, st, geo, bits2 = c.gof_dynamic_simulate(Xs, ic, radii, seed=rr.DRAW_SEED, first_index=first, want_bits=True)
    np.testing.assert_array_equal(bits2, bits)
    return stats, ov, st, geo, bits


def _assert_drawn(got, N, Y_host, sure, directed):
    """the drawn bits are the host's wherever u is not within 1e-12 of p, at most two draws are that close,
    and every record is the host's of the drawn networks"""
    stats, ov, st, geo, bits = got
    Y = gof_stats.unpack(bits, N)
    assert (~sure).sum() <= 2
    assert np.array_equal(Y[sure], Y_host[sure]), int((Y != Y_host)[sure].sum())
    assert not gof_stats.unpack(bits, 32 * bits.shape[-1])[..., N:].any()
    np.testing.assert_array_equal(stats, rr.batch_stats(Y, directed))
    want = rr.batch_dynamic(Y, directed)
    for a, b in zip((ov, st, geo), want):
        np.testing.assert_array_equal(a, b)


@BOTH
def test_one_workgroup_per_network(da, directed):
    T, N, D, S, _, _ = rr.DRAWN['one_workgroup']
    Xs, ic, radii, Y_host, sure = rr.drawn_case('one_workgroup', directed)
    with da.Chain(T, N, D, _mode(directed)) as c:
        got = _simulate(c, Xs, ic, radii, rr.DRAW_FIRST)
    _assert_drawn(got, N, Y_host, sure, directed)


def test_two_batches_at_the_grid_cap(da):
    T, N, D, S, _, _ = rr.DRAWN['two_batches']
    Xs, ic, _, Y_host, sure = rr.drawn_case('two_batches', False)
    with da.Chain(T, N, D, 'undirected') as c:
        got = _simulate(c, Xs, ic, None, rr.DRAW_FIRST)
        # the second batch starts at sample 65535 // T = 21845
        singles = {s: _simulate(c, Xs[s:s + 1], ic[s:s + 1], None, rr.DRAW_FIRST + s) for s in (21844, 21845, 21999)}
    _assert_drawn(got, N, Y_host, sure, False)
    for s, one in singles.items():
        for a, b in zip(got, one):
            np.testing.assert_array_equal(a[s], b[0])


def test_one_wide_directed_draw(da):
    T, N, D, S, _, _ = rr.DRAWN['wide_draw']
    Xs, ic, radii, Y_host, sure = rr.drawn_case('wide_draw', True)
    with da.Chain(T, N, D, 'directed') as c:
        stats, bits = c.gof_simulate(Xs, ic, radii, seed=rr.DRAW_SEED, first_index=rr.DRAW_FIRST, want_bits=True)
    Y = gof_stats.unpack(bits, N)
    assert (~sure).sum() <= 2
    assert np.array_equal(Y[sure], Y_host[sure]), int((Y != Y_host)[sure].sum())
    # the in-degrees are counted in the transposed plane, which the device draws on its own
    np.testing.assert_array_equal(stats[0, 0, 2 + N:2 + 2 * N], np.bincount(Y[0, 0].sum(0), minlength=N)[:N])
    np.testing.assert_array_equal(stats[0], gof_stats.records(Y[0], True))
