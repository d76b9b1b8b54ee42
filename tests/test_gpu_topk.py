"""Link prediction on the device (csrc/kernels_topk.hpp, dynetlsm_amd/ranking.py) against the host restatement
tests/topk_ref.py.  Needs an MI355X: -m gpu.

Tolerance of proba and sd: the project's rule of proba_ref.tolerance, 16 eps + 4 ulp of the value, with eps the
reference's own error on that input: the larger of max |float64 - longdouble| and the largest change when every p_s is
moved by +-4 ulp with random signs.  Nothing enters it from the code under test.

The returned set of dyads is compared exactly.  Every case first asserts on its own inputs (topk_ref.cut_is_decided)
that the cut is decided at that tolerance: the reference's k-th and (k + 1)-th value differ by more than twice the
tolerance, or they lie in a group of bit-equal values whose neighbours on both sides are that far away.  A case that
fails the condition fails with 'pick another seed'; no dyad is left out of any comparison.  Inside the list the
device's own values must be sorted, ties by (i, j), and the reference's values along it must not rise (largest=False:
fall) by more than twice the tolerance."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import score_ref  # noqa: E402
import topk_ref  # noqa: E402
from test_gpu_ic import _case  # noqa: E402
from test_gpu_proba import _mask  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 7, 64, 300)
# the counters of one histogram as the device stores them (kernels_score.hpp: the bins padded to 16 segments of
# whole steps of 64 lanes x 4 bins) and the time steps whose histograms fit the 128 MB of a group (capi_topk.hpp)
HIST_COUNTERS = -(-score_ref.N_BINS // (16 * 64 * 4)) * (64 * 4) * 16
GROUP_STEPS = (128 << 20) // (HIST_COUNTERS * 8)


@pytest.fixture(scope='module')
def da():
    import dynetlsm_amd
    return dynetlsm_amd


def _model(directed):
    return 'directed' if directed else 'undirected'


@functools.lru_cache(maxsize=None)
def _inputs(N, T, D, S, directed, masked=False, seed=0):
    rng = np.random.RandomState(1000 * seed + 16 * N + D + 8 * directed + S)
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
    return Y, Xs, ic, radii, (_mask(rng, T, N) if masked else None)


def _check(got, ref, k, largest, label):
    """(steps, diag) of Chain.topk_accumulate against the reference"""
    steps, diag = got
    tol_p, tol_sd = topk_ref.tolerances(ref)
    T = ref['eligible'].shape[0]
    assert len(steps) == T
    np.testing.assert_array_equal(diag['eligible'], ref['eligible_t'], err_msg=label)
    worst = 0.0
    for t in range(T):
        assert topk_ref.cut_is_decided(ref, t, k, tol_p), '%s t=%d k=%d: pick another seed' % (label, t, k)
        ri, rj = ref['rank'][t]
        n = min(k, ri.size)
        i, j, y, proba, sd = steps[t]
        assert i.size == n, (label, t, i.size, n)
        assert sorted(zip(i.tolist(), j.tolist())) == sorted(zip(ri[:n].tolist(), rj[:n].tolist())), (label, t)
        if not n:
            continue
        want_p, want_sd = ref['pw'][t, i, j, 0], ref['pw'][t, i, j, 1]
        err_p, err_sd = np.abs(proba - want_p), np.abs(sd - want_sd)
        worst = max(worst, float((err_p / tol_p[t, i, j]).max()), float((err_sd / tol_sd[t, i, j]).max()))
        assert (err_p <= tol_p[t, i, j]).all(), (label, t, 'proba', float((err_p / tol_p[t, i, j]).max()))
        assert (err_sd <= tol_sd[t, i, j]).all(), (label, t, 'sd', float((err_sd / tol_sd[t, i, j]).max()))
        np.testing.assert_array_equal(y, ref['Y'][t, i, j].astype(np.int64), err_msg=label)
        # sorted by its own values, ties by (i, j)
        np.testing.assert_array_equal(np.lexsort((j, i, -proba if largest else proba)), np.arange(n), err_msg=label)
        # the reference's values along the list
        step = np.diff(want_p) * (1.0 if largest else -1.0)
        assert (step <= 2.0 * np.maximum(tol_p[t, i, j][1:], tol_p[t, i, j][:-1])).all(), (label, t, 'order')
        # the counts: k-th key's dyads and those beyond it hold the list
        assert diag['n_beyond'][t] < min(k, ri.size) <= diag['n_beyond'][t] + diag['n_at'][t], (label, t)
    return worst


def _run(da, chain, inputs, directed, k, among, largest, label, base=None, max_candidates=None):
    Y, Xs, ic, radii, mask = inputs
    bits = da.engine.pack_network(Y)
    pm = da.engine.pack_network(mask) if mask is not None else None
    ref = topk_ref.reference(Y, Xs, ic, radii, directed, among, largest, mask, base=base)
    got = chain.topk_accumulate(bits, Xs, ic, radii, k, among=among, largest=largest, mask=pm,
                                max_candidates=max_candidates)
    worst = _check(got, ref, k, largest, label)
    return got, ref, worst


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('N,T,D,S,directed', [(70, 2, 2, 20, False), (37, 3, 3, 25, True), (40, 2, 5, 12, True)])
def test_parity_on_two_column_tiles_and_ragged_edges(da, N, T, D, S, directed, masked):
    """every among, both orders, k inside one wavefront's dyads, one tile and several tiles"""
    inputs = _inputs(N, T, D, S, directed, masked)
    base = topk_ref.values(inputs[1], inputs[2], inputs[3], directed)
    worst = 0.0
    with da.Chain(T, N, D, _model(directed)) as c:
        for among in topk_ref.AMONG:
            for largest in (True, False):
                for k in KS:
                    label = 'N=%d dir=%d masked=%d %s largest=%d k=%d' % (N, directed, masked, among, largest, k)
                    if among == 'missing' and not masked:
                        with pytest.raises(ValueError, match='mask'):
                            c.topk_accumulate(da.engine.pack_network(inputs[0]), inputs[1], inputs[2], inputs[3], k,
                                              among=among, largest=largest)
                        continue
                    worst = max(worst, _run(da, c, inputs, directed, k, among, largest, label, base)[2])
    print('N=%d dir=%d masked=%d: max err/tol %.3f' % (N, directed, masked, worst))


@pytest.mark.parametrize('directed', [False, True])
@pytest.mark.parametrize('D', range(1, 9))
def test_every_instantiation(da, D, directed):
    inputs = _inputs(20, 1, D, 12, directed, True)
    with da.Chain(1, 20, D, _model(directed)) as c:
        for among, largest in (('non_ties', True), ('ties', False), ('missing', True)):
            _run(da, c, inputs, directed, 5, among, largest, 'D=%d dir=%d %s' % (D, directed, among))


@pytest.mark.parametrize('directed', [False, True])
def test_k_beyond_the_eligible_dyads_returns_all_of_them_ranked(da, directed):
    inputs = _inputs(12, 2, 2, 9, directed, True)
    with da.Chain(2, 12, 2, _model(directed)) as c:
        for among in topk_ref.AMONG:
            for largest in (True, False):
                (steps, diag), ref, _ = _run(da, c, inputs, directed, 1000, among, largest,
                                             'k=1000 dir=%d %s' % (directed, among))
                assert [s[0].size for s in steps] == ref['eligible_t'].tolist()
                np.testing.assert_array_equal(diag['n_beyond'] + diag['n_at'], ref['eligible_t'])


@pytest.mark.parametrize('directed', [False, True])
def test_a_time_step_without_an_eligible_dyad_returns_nothing(da, directed):
    Y, Xs, ic, radii, mask = _inputs(37, 3, 3, 25, directed, True)
    mask = mask.copy()
    mask[1] = True
    inputs = (Y, Xs, ic, radii, mask)
    plain = _inputs(37, 3, 3, 25, directed, True)
    with da.Chain(3, 37, 3, _model(directed)) as c:
        for among in ('non_ties', 'ties', 'observed'):
            (steps, diag), _, _ = _run(da, c, inputs, directed, 7, among, True, 'empty step %s' % among)
            (other, _), _, _ = _run(da, c, plain, directed, 7, among, True, 'plain %s' % among)
            assert steps[1][0].size == 0 and diag['eligible'][1] == 0 and diag['key'][1] == -1
            assert diag['tiles_revisited'][1] == 0 and diag['n_beyond'][1] == 0 and diag['n_at'][1] == 0
            for t in (0, 2):                                    # the other time steps do not notice
                for a, b in zip(steps[t], other[t]):
                    assert a.tobytes() == b.tobytes()
        (steps, diag), ref, _ = _run(da, c, inputs, directed, 7, 'missing', True, 'all missing')
        assert steps[1][0].size == 7 and diag['eligible'][1] == ref['exists'][1].sum()


def _coincident(directed, nodes=(3, 40, 69)):
    """N = 70: the nodes share positions and radii in every sample - they span the row blocks 0, 1 and 2 and both
    column tiles -, so whole groups of dyads have bit-equal pbar"""
    Y, Xs, ic, radii, _ = _inputs(70, 2, 2, 10, directed)
    Xs = Xs.copy()
    Xs[:, :, nodes[1:], :] = Xs[:, :, nodes[:1], :]
    if directed:
        radii = radii.copy()
        radii[:, nodes[1:]] = radii[:, nodes[:1]]
    return Y, Xs, ic, radii, None


@pytest.mark.parametrize('directed', [False, True])
def test_exact_ties_are_cut_by_i_then_j(da, directed):
    inputs = _coincident(directed)
    base = topk_ref.values(inputs[1], inputs[2], inputs[3], directed)
    full = topk_ref.reference(inputs[0], inputs[1], inputs[2], inputs[3], directed, 'all', True, base=base)
    with da.Chain(2, 70, 2, _model(directed)) as c:
        cuts = 0
        for largest in (True, False):
            ref = full if largest else topk_ref.reference(inputs[0], inputs[1], inputs[2], inputs[3], directed, 'all',
                                                          False, base=base)
            # every k that cuts through a group of bit-equal values of time step 0
            i, j = ref['rank'][0]
            v = ref['pw'][0, i, j, 0]
            ks = [k for k in range(1, v.size) if v[k - 1] == v[k]]
            assert len(ks) >= 6, 'the groups of coincident nodes are missing'
            for k in ks[:3] + ks[len(ks) // 2:len(ks) // 2 + 2] + ks[-2:]:
                (steps, _), _, _ = _run(da, c, inputs, directed, k, 'all', largest,
                                        'ties dir=%d largest=%d k=%d' % (directed, largest, k), base)
                # the reference's stable sort keeps (i, j) order inside a group: the device returns that very prefix
                np.testing.assert_array_equal(steps[0][0], i[:k])
                np.testing.assert_array_equal(steps[0][1], j[:k])
                cuts += 1
        assert cuts >= 12


@pytest.mark.parametrize('directed', [False, True])
def test_all_dyads_equal_and_the_room_for_candidates(da, directed):
    """every node at one position: one pbar, one key.  With room for all of them the first k in (i, j) order are
    returned; with room for k only, the call is refused with DLSM_E_LIMIT and the chain goes on working"""
    N, T, k = 40, 2, 5
    Y, Xs, ic, radii, _ = _inputs(N, T, 2, 8, directed)
    Xs = np.broadcast_to(Xs[:, :, :1, :], Xs.shape).copy()
    inputs = (Y, Xs, ic, radii, None)
    dyads = N * (N - 1) // (1 if directed else 2)
    bits = da.engine.pack_network(Y)
    with da.Chain(T, N, 2, _model(directed)) as c:
        (steps, diag), ref, _ = _run(da, c, inputs, directed, k, 'all', True, 'equal dir=%d' % directed,
                                     max_candidates=dyads)
        assert len(np.unique(ref['pw'][..., 0][ref['exists']])) == 1
        i, j = np.nonzero(ref['exists'][0])
        for t in range(T):
            np.testing.assert_array_equal(steps[t][0], i[:k])
            np.testing.assert_array_equal(steps[t][1], j[:k])
        assert (diag['n_beyond'] == 0).all() and (diag['n_at'] == dyads).all()
        with pytest.raises(da.EngineError) as e:
            c.topk_accumulate(bits, Xs, ic, radii, k, among='all', max_candidates=k)
        assert e.value.code == -5
        msg = str(e.value)
        assert 'time step 0' in msg and str(dyads) in msg and 'max_candidates=%d' % k in msg, msg
        again, _, _ = _run(da, c, inputs, directed, k, 'all', True, 'equal again dir=%d' % directed)
        for t in range(T):
            for a, b in zip(again[0][t], steps[t]):
                assert a.tobytes() == b.tobytes()
        with pytest.raises(ValueError, match='max_candidates'):
            c.topk_accumulate(bits, Xs, ic, radii, k, among='all', max_candidates=k - 1)


def test_clamped_keys_are_still_ordered_by_the_doubles(da):
    """intercept 40 and distances up to 22: every pbar rounds to 1.0f, the last key; intercept -200: every pbar is
    below 2^-63, the first key.  All eligible dyads share one bin; the list is ordered by the doubles"""
    N, T, S = 40, 2, 6
    Y, Xs, ic, _, _ = _inputs(N, T, 2, S, False)
    dist = np.sqrt(((Xs[:, :, :, None] - Xs[:, :, None]) ** 2).sum(-1))
    Xs = Xs * (22.0 / dist.max())
    dyads = N * (N - 1) // 2
    with da.Chain(T, N, 2, 'undirected') as c:
        hi = (Y, Xs, np.stack([np.full(S, 40.0), np.zeros(S)], axis=1), None, None)
        (steps, diag), ref, _ = _run(da, c, hi, False, 7, 'all', False, 'intercept 40')
        p = ref['pw'][..., 0][ref['exists']]
        assert (p.astype(np.float32) == 1.0).all() and len(np.unique(p)) > dyads // 2
        assert (diag['key'] == score_ref.KEY_HI).all() and (diag['n_at'] == dyads).all()
        assert (diag['n_beyond'] == 0).all() and all(len(np.unique(s[3])) == 7 for s in steps)
        lo = (Y, Xs, np.stack([np.full(S, -200.0), np.zeros(S)], axis=1), None, None)
        (steps, diag), ref, _ = _run(da, c, lo, False, 7, 'all', True, 'intercept -200')
        p = ref['pw'][..., 0][ref['exists']]
        assert (p < 2.0 ** -63).all() and (p > 0).all()
        assert (diag['key'] == score_ref.KEY_LO).all() and (diag['n_at'] == dyads).all()
        assert all(len(np.unique(s[3])) == 7 for s in steps)


def test_one_time_step_more_than_a_group_of_histograms(da):
    assert GROUP_STEPS == 8
    T, N = GROUP_STEPS + 1, 12
    for directed in (False, True):
        inputs = _inputs(N, T, 2, 5, directed, True)
        with da.Chain(T, N, 2, _model(directed)) as c:
            for among, largest in (('non_ties', True), ('all', False)):
                (steps, diag), ref, _ = _run(da, c, inputs, directed, 4, among, largest,
                                             'T=%d dir=%d %s' % (T, directed, among))
                assert steps[T - 1][0].size == 4 and diag['eligible'][T - 1] == ref['eligible_t'][T - 1]


@pytest.mark.parametrize('directed', [False, True])
def test_only_the_tiles_that_reach_the_threshold_are_revisited(da, directed):
    """N = 200: ten nodes of row block 0 and column tile 0 tight together, the rest far apart"""
    N, T, D, S, k = 200, 2, 2, 6, 20
    rng = np.random.RandomState(11 + directed)
    Y, Xs, ic, radii = _case(rng, S, T, N, D, directed)
    Xs = Xs * 8.0
    close = np.array([0, 2, 5, 7, 11, 13, 17, 19, 23, 29])
    Xs[:, :, close, :] = 0.05 * rng.randn(S, T, close.size, D)
    inputs = (Y, Xs, ic, radii, None)
    with da.Chain(T, N, D, _model(directed)) as c:
        (steps, diag), ref, _ = _run(da, c, inputs, directed, k, 'all', True, 'tiles dir=%d' % directed)
    assert score_ref.keys_are_stable(ref['pw'][..., 0][ref['exists']]), 'pick another seed'
    reach, n_tiles = topk_ref.tiles_reaching(ref, D, directed, k, True)
    assert diag['n_tiles'] == n_tiles
    np.testing.assert_array_equal(diag['tiles_revisited'], reach)
    assert 0 < reach.sum() < T * n_tiles and (reach <= 2).all()
    for t in range(T):
        assert np.isin(steps[t][0], close).all() and np.isin(steps[t][1], close).all()


def test_two_calls_on_one_chain_return_the_same_bits(da):
    for directed in (False, True):
        Y, Xs, ic, radii, mask = _inputs(130, 2, 5, 12, directed, True)
        bits, pm = da.engine.pack_network(Y), da.engine.pack_network(mask)
        with da.Chain(2, 130, 5, _model(directed)) as c:
            a = c.topk_accumulate(bits, Xs, ic, radii, 300, mask=pm)
            b = c.topk_accumulate(bits, Xs, ic, radii, 300, mask=pm)
        with da.Chain(2, 130, 5, _model(directed)) as c:
            f = c.topk_accumulate(bits, Xs, ic, radii, 300, mask=pm)
        for other in (b, f):
            for x, y in zip(other[0], a[0]):
                for u, v in zip(x, y):
                    assert u.tobytes() == v.tobytes()
            for key in a[1]:
                np.testing.assert_array_equal(other[1][key], a[1][key])


def test_bad_arguments_are_rejected(da):
    import ctypes
    from dynetlsm_amd import _lib
    rng = np.random.RandomState(0)
    Y, Xs, ic, radii = _case(rng, 4, 2, 9, 2, True)
    bits = da.engine.pack_network(Y)
    with da.Chain(2, 9, 2, 'directed') as c:
        with pytest.raises(ValueError):
            c.topk_accumulate(bits, Xs, ic, None, 3)
        with pytest.raises(ValueError):
            c.topk_accumulate(bits[:1], Xs, ic, radii, 3)
        with pytest.raises(ValueError, match='two samples'):
            c.topk_accumulate(bits, Xs[:1], ic[:1], radii[:1], 3)
        for k in (0, -2, 1.5):
            with pytest.raises(ValueError, match='k must'):
                c.topk_accumulate(bits, Xs, ic, radii, k)
        with pytest.raises(ValueError, match='among'):
            c.topk_accumulate(bits, Xs, ic, radii, 3, among='edges')
        with pytest.raises(da.EngineError) as e:
            c.topk_accumulate(bits, Xs, ic, radii * 0, 3)
        assert e.value.code == -4
        # the library's own checks
        dp = ctypes.POINTER(ctypes.c_double)
        keep = [np.ascontiguousarray(Xs), np.ascontiguousarray(ic), np.ascontiguousarray(radii),
                np.zeros((2, 80, 4), dtype=np.int32), np.zeros((2, 80, 2)), np.zeros(2, dtype=np.int32),
                np.zeros((2, 5), dtype=np.int64)]

        def raw(S=4, among=0, largest=1, k=3, room=80, mask=None, radii=keep[2]):
            return c._L.dlsm_topk_accumulate(
                c._h, bits.ctypes.data_as(_lib.c_u32_p), mask, keep[0].ctypes.data_as(dp), keep[1].ctypes.data_as(dp),
                radii.ctypes.data_as(dp) if radii is not None else None, S, among, largest, k, room,
                keep[3].ctypes.data_as(_lib.c_i32_p), keep[4].ctypes.data_as(dp), keep[5].ctypes.data_as(_lib.c_i32_p),
                keep[6].ctypes.data_as(_lib.c_i64_p))

        assert raw() == 0 and keep[5].tolist() == keep[6][:, 1:3].sum(axis=1).tolist()
        assert raw(S=1) == -1 and raw(among=5) == -1 and raw(among=-1) == -1 and raw(largest=2) == -1
        assert raw(k=0) == -1 and raw(k=5, room=4) == -1 and raw(among=3) == -1 and raw(radii=None) == -1
        assert raw(among=3, mask=bits.ctypes.data_as(_lib.c_u32_p)) == 0


def _trace_inputs(model, ids):
    directed = bool(model.is_directed)
    ic = np.asarray(model.intercepts_)[ids].reshape(len(ids), -1)
    if ic.shape[1] == 1:
        ic = np.concatenate([ic, np.zeros_like(ic)], axis=1)
    radii = np.asarray(model.radiis_)[ids] if directed else None
    Y = np.asarray(model.Y_fit_).copy()
    idx = np.arange(Y.shape[1])
    Y[:, idx, idx] = 0
    return Y, np.asarray(model.Xs_)[ids], ic, radii


@pytest.mark.parametrize('directed', [False, True])
def test_facade_on_a_short_lsm_fit(da, directed):
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N, k = 3, 30, 15
    Ynet = synthetic_lsm_network(T=T, N=N, density=0.2, seed=2, directed=directed)['Y']
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, is_directed=directed, random_state=4).fit(Ynet)
    res = da.top_dyads(m, k=k)
    assert res.among == 'non_ties' and res.largest and res.n_samples == m.Xs_.shape[0] - m.n_burn_
    Y, Xs, ic, radii = _trace_inputs(m, res.sample_ids)
    ref = topk_ref.reference(Y, Xs, ic, radii, directed, 'non_ties', True)
    _check(([res.at(t)[1:3] + (res.at(t).y, res.at(t).proba, res.at(t).sd) for t in range(T)], res.diagnostics), ref,
           k, True, 'facade dir=%d' % directed)
    # the same rows through the chain
    with da.Chain(T, N, Xs.shape[3], _model(directed)) as c:
        steps, diag = c.topk_accumulate(da.engine.pack_network(Y), Xs, ic, radii, k)
    for name, col in (('i', 0), ('j', 1), ('y', 2), ('proba', 3), ('sd', 4)):
        assert getattr(res, name).tobytes() == np.concatenate([s[col] for s in steps]).tobytes(), name
    np.testing.assert_array_equal(res.t, np.repeat(np.arange(T), k))
    np.testing.assert_array_equal(res.eligible_t, diag['eligible'])
    assert (res.y == 0).all()
    # pooled: the merge of the lists per time step
    order = np.lexsort((res.j, res.i, res.t, -res.proba))[:k]
    pooled = res.pooled()
    for got, want in zip(pooled, (res.t, res.i, res.j, res.proba, res.sd, res.y)):
        np.testing.assert_array_equal(got, want[order])
    # implausible ties: the default order is ascending
    ties = da.top_dyads(m, k=5, among='ties', n_samples=30)
    assert not ties.largest and ties.n_samples == 30 and (ties.y == 1).all() and ties.t.size == 5 * T
    Yt, Xt, it, rt = _trace_inputs(m, ties.sample_ids)
    _check(([ties.at(t)[1:3] + (ties.at(t).y, ties.at(t).proba, ties.at(t).sd) for t in range(T)], ties.diagnostics),
           topk_ref.reference(Yt, Xt, it, rt, directed, 'ties', False), 5, False, 'facade ties dir=%d' % directed)
    # precision against brute force (here: against the network the model was fit to, so no returned non-tie hits)
    assert res.precision_at_k(Ynet) == 0.0 and ties.precision_at_k(Ynet) == 1.0
    other = synthetic_lsm_network(T=T, N=N, density=0.3, seed=9, directed=directed)['Y']
    assert res.precision_at_k(other) == np.mean([other[t, i, j] == 1 for t, i, j in zip(res.t, res.i, res.j)])
    assert 'top dyads' in res.summary()
    with pytest.raises(ValueError, match='missing'):
        da.top_dyads(m, among='missing')


def test_facade_ranks_the_held_out_dyads_of_a_sample_missing_fit(da):
    from dynetlsm_amd.model_selection import train_test_split
    from dynetlsm_amd.synthetic import synthetic_lsm_network
    T, N = 3, 30
    Y = synthetic_lsm_network(T=T, N=N, density=0.2, seed=3)['Y']
    Yt, index = train_test_split(Y, 0.1, random_state=1, is_directed=False)
    m = da.DynamicNetworkLSM(n_iter=200, burn=100, tune=100, random_state=4, sample_missing=True).fit(Yt)
    k = 10
    res = da.top_dyads(m, k=k, among='missing', n_samples=40)
    held = np.zeros(Y.shape, dtype=bool)
    held[index[:, 0], index[:, 1], index[:, 2]] = True
    held |= held.transpose(0, 2, 1)
    assert held[res.t, res.i, res.j].all() and (res.i < res.j).all()
    np.testing.assert_array_equal(res.eligible_t, np.triu(held, 1).sum(axis=(1, 2)))
    Yf, Xs, ic, radii = _trace_inputs(m, res.sample_ids)
    ref = topk_ref.reference(Yf, Xs, ic, radii, False, 'missing', True, held)
    _check(([res.at(t)[1:3] + (res.at(t).y, res.at(t).proba, res.at(t).sd) for t in range(T)], res.diagnostics), ref,
           k, True, 'held out')
    # scored against the full network, as metrics.heldout_scores scores the held-out dyads
    assert res.precision_at_k(Y) == np.mean([Y[t, i, j] == 1 for t, i, j in zip(res.t, res.i, res.j)])
    observed = da.top_dyads(m, k=k, among='observed', n_samples=40)
    assert not held[observed.t, observed.i, observed.j].any()
